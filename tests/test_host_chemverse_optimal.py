"""ChemVerse's cost oracle without a GPU: route search, optimal conditions and the yield threshold against the reference's
recorded values, the host restatement against its recorded searches (tests/chemverse_opt_util.py states the comparison),
the pricing code on recorded rows, the fixtures' own conditions, refusals."""
import math

import numpy as np
import pytest

import chemverse_opt_util as ou
from xenoverse_amd import _lib
from xenoverse_amd.chemverse import (chain_costs, compute_optimal_costs, find_reaction_chains, one_pot_costs,
                                     optimal_conditions, yield_threshold)
from xenoverse_amd.chemverse import optimal_host as H
from xenoverse_amd.chemverse import tables as T

QUICK_S = 3.0      # candidates whose reference run took less are searched again here


@pytest.mark.parametrize("tag", ou.TAGS)
def test_routes_and_conditions_equal_the_reference(tag):
    fx = ou.fixture(tag)
    tab, doc = fx["tab"], fx["doc"]
    rids = tab["rxn_ids"]
    above = [tab["chem_ids"][c] for c in range(tab["C"]) if tab["layer"][c] > 1]
    assert sorted(doc["routes"]) == sorted(above) and above
    for cid, rec in doc["routes"].items():
        for key, steps in (("request", max(6, tab["num_layers"] * 2)), ("one_pot", 6)):
            got = [[rids[r] for r in ch] for ch in find_reaction_chains(tab, cid, 5, steps)]
            assert got == rec[key], "%s %s %s" % (tag, cid, key)
    temps, durs = optimal_conditions(tab)
    assert len(doc["conditions"]) == tab["R"]
    for r, rid in enumerate(rids):
        assert [temps[r], durs[r]] == doc["conditions"][rid], "%s %s" % (tag, rid)


def test_tables_carry_the_oracles_columns():
    fx = ou.fixture("b")
    tab, chems = fx["tab"], fx["world"]["chemicals"]
    for i, cid in enumerate(tab["chem_ids"]):
        c = chems[cid]
        assert tab["layer"][i] == c["layer"] and tab["base_toxicity"][i] == c["base_toxicity"]
        assert tab["medicinal_value"][i] == c["medicinal_expected"] * c["medicinal_efficacy"]
        assert (math.isnan(tab["price_per_gram"][i]) if c["price_per_gram"] is None else tab["price_per_gram"][i] == c["price_per_gram"])
    assert tab["num_layers"] == fx["world"]["metadata"]["num_layers"]
    assert tab["cost_params"] == dict(T.DEFAULT_COST_PARAMS, **fx["world"]["cost_params"])
    e = tab["equip_names"].index("autoclave")
    spec = fx["world"]["equipment"]["autoclave"]
    assert (tab["base_cost_per_hour"][e], tab["cost_multiplier"][e]) == (spec["base_cost_per_hour"], spec["cost_multiplier"])


@pytest.mark.parametrize("m", [0.5, 1.0, 0.25, 0.1234567, 1e-6])
def test_yield_threshold_is_the_rounded_comparison(m):
    thr = yield_threshold(m)
    assert round(thr, 6) >= m and not round(math.nextafter(thr, -math.inf), 6) >= m
    rs = np.random.RandomState(int(m * 1e7) % 2 ** 31)
    y = thr
    ys = []
    for k in rs.randint(-64, 65, size=1000):
        y = thr
        for _ in range(abs(int(k))):
            y = math.nextafter(y, math.inf if k > 0 else -math.inf)
        ys.append(y)
    assert all((round(y, 6) >= m) == (y >= thr) for y in ys)


@pytest.fixture(scope="module")
def quick_chains():
    """the host's search of every recorded route the reference ran in under QUICK_S seconds, once"""
    picked = [(t, w, c) for t, w, c in ou.all_cases("chains") if c["seconds"] < QUICK_S]
    tabs = [ou.fixture(t)["tab"] for t in ou.TAGS]
    results, solved = chain_costs(tabs, [dict(c, world=w) for _, w, c in picked], backend="host", details=True)
    return picked, results, solved


def test_host_chain_costs_equal_the_reference(quick_chains):
    picked, results, solved = quick_chains
    assert any(c["found"] for _, _, c in picked) and any(not c["found"] for _, _, c in picked)
    checked = 0
    for (tag, _, case), r, s in zip(picked, results, solved):
        ou.compare_chain(ou.fixture(tag)["tab"], case, r, s, ou.Worst(), exact=True, label=tag + " ")
        checked += case["stable"] and case["order_free"]
    assert checked >= 3


@pytest.mark.parametrize("tag", ["b", "c"])
def test_host_one_pot_candidate_equals_the_reference(tag):
    """one recorded (charge, temperature) candidate per world — the first that passed — searched on the host"""
    fx = ou.fixture(tag)
    tab, case = fx["tab"], fx["doc"]["one_pots"][0]
    k = next(i for i, c in enumerate(case["candidates"]) if c["found"])
    cand = case["candidates"][k]
    plans = H.one_pot_plans(tab, case["target"], case["max_time_seconds"])
    assert len(plans) == len(case["candidates"]) and [p["steps"][0]["T"] for p in plans] == [c["T"] for c in case["candidates"]]
    s = H.solve_plans_host([tab], [0], [plans[k]], [case["min_yield_g"]])[0]
    assert (s["found"], s["bits"], s["best_scale"]) == (True, cand["bits"], cand["best_scale"])
    ids = tab["chem_ids"]
    entries = plans[k]["steps"][0]["entries"]
    assert sorted(set(ids[c] for c, _ in entries)) == sorted(cand["charge_order"])      # the same charge, in index order here
    got = {}
    for j, (c, _) in enumerate(entries):
        got[ids[c]] = got.get(ids[c], 0) + float(s["rows"]["charged"][0, j])
    assert got == cand["amounts"]
    if case["order_free"]:
        pool = {ids[c]: float(g) for c, g in enumerate(s["rows"]["final_pool"]) if g > 1e-9}
        assert pool == cand["final_pool"]


def test_host_one_pot_without_a_passing_candidate_is_none():
    """world a / C012: every (charge, temperature) candidate fails its 12 passes and the pass at scale_hi"""
    fx = ou.fixture("a")
    case = fx["doc"]["one_pots"][0]
    assert case["result"] is None and case["candidates"] and not any(c["found"] for c in case["candidates"])
    results, parts = one_pot_costs([fx["tab"]], [case], backend="host", details=True)
    assert results == [None]
    ou.compare_one_pot(fx["tab"], case, results[0], parts[0], ou.Worst(), exact=True, label="a ")


def test_direct_purchase_wins_the_recorded_request():
    """world c at (0.25, 1.6, 0.5): the layer-1 C011 qualifies beside two compounds above layer 1, and buying it is the
    reference's answer.  The searches are left out here (the fixture script runs them on the host, the device test on the
    GPU): with no candidate found the purchase stands, and a cheaper route still replaces it."""
    fx = ou.fixture("c")
    tab = fx["tab"]
    case = next(c for c in fx["doc"]["requests"] if c["result"]["found"] and c["result"]["num_steps"] == 0)
    planned = H.request_plans(tab, case["request"])
    layers = [int(tab["layer"][c]) for c in planned["qualifying"]]
    assert 1 in layers and max(layers) > 1 and planned["chains"] and planned["one_pot"]
    none = dict(found=False, best_scale=0.0, bits=0, rows=None)
    got = H.request_result(tab, planned, [none] * len(planned["chains"]), [[none] * len(ps) for _, ps in planned["one_pot"]])
    assert got == case["result"]
    assert got["route_detail"] == {"note": "Direct purchase"} and "in 0 step(s), 0s." in got["message"]
    # a route that costs less than the purchase takes its place, one that costs the same does not (strict <)
    route = next(c for c in fx["doc"]["chains"] if c["found"] and c["result"] is not None)
    plan, rows = _rows_of(tab, route)
    target = H.chem_index(tab, route["target"])
    buy = planned["qualifying"][layers.index(1)]
    solved = dict(found=True, best_scale=route["best_scale"], rows=rows)
    cost, m = route["result"]["total_cost"], case["request"]["min_yield_g"]
    assert m == 0.5      # price * 0.5 is exact, so the purchase below costs exactly what it is meant to
    for order, first in (([buy, target], "purchase"), ([target, buy], "route")):
        mixed = dict(planned, qualifying=order, chains=[(target, plan)], one_pot=[])
        for purchase, winner in ((cost * 2.0, "route"), (cost * 0.5, "purchase"), (cost, first)):
            priced = dict(tab, price_per_gram=tab["price_per_gram"].copy())
            priced["price_per_gram"][buy] = purchase / m
            r = H.request_result(priced, mixed, [solved], [])
            assert r["found"] and (r["num_steps"] == 0) == (winner == "purchase"), (order, purchase)
            assert r["optimal_cost"] == (round(purchase, 4) if winner == "purchase" else cost)


def _rows_of(tab, case):
    """a recorded chain case's pass at best_scale as rows"""
    plan = H.chain_plan(tab, case["chain"], case["target"])
    n, k, C = len(plan["steps"]), max(len(s["entries"]) for s in plan["steps"]), tab["C"]
    rows = dict(charged=np.zeros((n, k)), consumed=np.zeros((n, C)), produced=np.zeros((n, C)), byproduct=np.zeros((n, C)),
                failure=np.zeros(n, np.uint8), final_pool=np.zeros(C))
    for s, (step, rec) in enumerate(zip(plan["steps"], case["steps"])):
        for j, (c, _) in enumerate(step["entries"]):
            rows["charged"][s, j] = rec["amounts"][tab["chem_ids"][c]]
        for key in ("consumed", "produced", "byproduct"):
            for cid, g in rec[key].items():
                rows[key][s, H.chem_index(tab, cid)] = g
    return plan, rows


def test_pricing_recorded_rows_gives_the_recorded_dict():
    """finish_chain on the reference's own per-step rows (hash seed 0's, whatever the simulation's sums depended on): costs,
    every rounding, the rounded yield"""
    n = 0
    for tag, _, case in ou.all_cases("chains"):
        if not (case["found"] and case["result"] is not None):
            continue
        tab = ou.fixture(tag)["tab"]
        plan, rows = _rows_of(tab, case)
        for step in plan["steps"]:      # a chemical charged twice in a step would need its two parts, which are not recorded
            assert len(set(c for c, _ in step["entries"])) == len(step["entries"])
        assert H.finish_chain(tab, plan, case["best_scale"], rows) == case["result"], "%s %s" % (tag, case["chain"])
        n += 1
    assert n >= 3


def test_time_allowance_and_strict_winner():
    fx = ou.fixture("b")
    tab = fx["tab"]
    case = next(c for c in fx["doc"]["chains"] if c["found"] and c["result"] is not None)
    plan, rows = _rows_of(tab, case)
    solved = dict(found=True, best_scale=case["best_scale"], rows=rows)
    total = case["result"]["total_time"]
    assert H.chain_result(tab, plan, solved, total) == case["result"]
    assert H.chain_result(tab, plan, solved, total / 1.04) == case["result"]      # over the budget, inside the 5 % allowance
    assert H.chain_result(tab, plan, solved, total / 1.06) is None
    assert H.chain_result(tab, plan, dict(found=False, best_scale=0.0, rows=None), total) is None
    # the winner: the first of equal costs stays (strict <), a cheaper later one replaces it
    target = H.chem_index(tab, case["target"])
    planned = dict(request=dict(H.REQUEST_DEFAULTS, min_yield_g=case["min_yield_g"]), qualifying=[target],
                   chains=[(target, plan), (target, dict(plan, steps=plan["steps"][:1]))], one_pot=[])
    cheap = dict(rows, charged=rows["charged"][:1] * 0.5, consumed=rows["consumed"][:1], produced=rows["produced"][:1],
                 byproduct=rows["byproduct"][:1], failure=rows["failure"][:1])
    same = H.request_result(tab, planned, [solved, dict(solved, found=False, rows=None)], [])
    assert same["found"] and same["optimal_cost"] == case["result"]["total_cost"] and same["num_steps"] == len(plan["steps"])
    other = H.request_result(tab, planned, [solved, dict(found=True, best_scale=case["best_scale"] * 0.5, rows=cheap)], [])
    assert other["num_steps"] == 1 and other["optimal_cost"] < case["result"]["total_cost"]
    assert set(other) == {"success", "found", "optimal_cost", "target", "medicinal_value", "base_toxicity", "num_steps",
                          "total_time_seconds", "route_detail", "message"}
    twice = dict(planned, chains=[(target, plan), (target, plan)])
    tie = H.request_result(tab, twice, [solved, dict(solved, best_scale=case["best_scale"] + 0.5)], [])      # same rows and cost
    assert tie["route_detail"] == case["result"]


def test_request_without_a_qualifying_compound():
    fx = ou.fixture("a")
    case = fx["doc"]["requests"][0]
    assert case["result"]["success"] is False
    assert compute_optimal_costs([fx["world"]], [case["request"]], backend="host") == [case["result"]]


def test_fixture_conditions():
    cases = [c for g in ("chains", "one_pots", "requests") for _, _, c in ou.all_cases(g)]
    assert sum(not c["stable"] for c in cases) * 8 <= len(cases)
    chains = [c for _, _, c in ou.all_cases("chains")]
    assert any(c["stable"] and c["found"] for c in chains) and any(c["stable"] and not c["found"] for c in chains)
    counts = ou.fixture("a")["doc"]["branches"]      # counted over the three fixtures together
    for b in ("chain_found", "chain_none", "chain_probe_run", "catalyst_layer1", "pool_floor", "one_pot_found", "one_pot_none",
              "request_found", "request_nothing_qualifies", "request_purchase"):
        assert counts[b] > 0, b


def test_refusals():
    fx = ou.fixture("c")
    tab = fx["tab"]
    long_route = list(range(T.CHAIN_MAX + 1))
    with pytest.raises(_lib.XenoError, match="CHAIN_MAX") as ei:
        chain_costs([tab], [dict(target="C005", chain=long_route, min_yield_g=0.5)], backend="host")
    assert ei.value.code == _lib.XV_ERR_UNSUPPORTED
    with pytest.raises(ValueError, match="not a reaction"):
        chain_costs([tab], [dict(target="C005", chain=["R999"], min_yield_g=0.5)], backend="host")
    with pytest.raises(ValueError, match="not a chemical"):
        chain_costs([tab], [dict(target="C999", chain=["R001"], min_yield_g=0.5)], backend="host")
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite"):
            chain_costs([tab], [dict(target="C005", chain=["R001"], min_yield_g=bad)], backend="host")
        with pytest.raises(ValueError, match="finite"):
            one_pot_costs([tab], [dict(target="C005", min_yield_g=0.5, max_time_seconds=bad)], backend="host")
        with pytest.raises(ValueError, match="finite"):
            compute_optimal_costs([tab], [dict(max_toxicity=bad)], backend="host")
    for bad in ((100.0, 0.0), (100.0, -5.0), (6000.0, 60.0)):      # a duration that is not positive, an absurd temperature
        with pytest.raises(ValueError, match="duration_s must be positive"):
            chain_costs([tab], [dict(target="C005", chain=["R001"], min_yield_g=0.5, conditions={0: bad})], backend="host")
    with pytest.raises(_lib.XenoError, match="STEPS_MAX"):
        chain_costs([tab], [dict(target="C005", chain=["R001"], min_yield_g=0.5, conditions={0: (100.0, 1e6)})], backend="host")
    with pytest.raises(ValueError, match="backend"):
        chain_costs([tab], [dict(target="C005", chain=["R001"], min_yield_g=0.5)], backend="numpy")
