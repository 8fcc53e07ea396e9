"""ChemVerse's cost oracle on the device against the reference's recorded searches (goldens only; tests/chemverse_opt_util.py
states the comparison and its bounds), batch independence, handle reuse, a failing first stage, the error word and the
route-length limit."""
import numpy as np
import pytest

import chemverse_opt_util as ou
from xenoverse_amd import _lib
from xenoverse_amd.chemverse import tables as T

pytestmark = pytest.mark.gpu


def worlds():
    return [ou.fixture(t)["world"] for t in ou.TAGS]


@pytest.fixture(scope="module")
def handle():
    from xenoverse_amd.chemverse import ChemVerseOptimal
    h = ChemVerseOptimal(worlds(), 256)
    yield h
    h.close()


def chain_candidates():
    return [dict(c, world=w) for _, w, c in ou.all_cases("chains")]


@pytest.fixture(scope="module")
def whole(handle):
    """every recorded route — the worlds interleaved in one handle, the longest lane 30 passes over one 720-step and two
    60-step stages — in one call; left unchanged"""
    from xenoverse_amd.chemverse import chain_costs
    res = chain_costs(None, chain_candidates(), handle=handle, details=True)
    assert handle.check_errors() == 0
    return res


def same_solved(a, b):
    if (a["found"], a["bits"], a["best_scale"], a["yield"]) != (b["found"], b["bits"], b["best_scale"], b["yield"]):
        return False
    if a["found"]:
        return all(np.array_equal(a["rows"][k], b["rows"][k]) for k in ("charged", "consumed", "produced", "byproduct", "failure"))
    return True


def test_chain_costs_against_the_reference(whole):
    results, solved = whole
    worst = ou.Worst()
    cases = ou.all_cases("chains")
    assert max(len(c["chain"]) for _, _, c in cases) >= 7
    for (tag, _, case), r, s in zip(cases, results, solved):
        ou.compare_chain(ou.fixture(tag)["tab"], case, r, s, worst, exact=False, label=tag + " ")
    print("chain candidates: largest deviation-to-bound ratio %.3g at %s" % (worst.ratio, worst.where))


def test_one_pot_costs_against_the_reference(handle):
    from xenoverse_amd.chemverse import one_pot_costs
    cases = ou.all_cases("one_pots")
    results, parts = one_pot_costs(None, [dict(c, world=w) for _, w, c in cases], handle=handle, details=True)
    assert handle.check_errors() == 0
    worst = ou.Worst()
    assert any(c["stable"] and c["result"] is None and c["candidates"] for _, _, c in cases)      # every candidate fails
    assert any(c["stable"] and c["result"] is not None for _, _, c in cases)
    for (tag, _, case), r, part in zip(cases, results, parts):
        ou.compare_one_pot(ou.fixture(tag)["tab"], case, r, part, worst, exact=False, label=tag + " ")
    print("one-pot candidates: largest deviation-to-bound ratio %.3g at %s" % (worst.ratio, worst.where))


def test_whole_requests_against_the_reference(handle):
    from xenoverse_amd.chemverse import compute_optimal_costs
    cases = ou.all_cases("requests")
    got = compute_optimal_costs(None, [dict(c["request"], world=w) for _, w, c in cases], handle=handle)
    assert handle.check_errors() == 0
    worst = ou.Worst()
    outcomes = set()
    for (tag, _, case), g in zip(cases, got):
        ref = case["result"]
        assert set(g) == set(ref), tag
        assert (g["success"], g["found"]) == (ref["success"], ref["found"]), tag
        outcomes.add((ref["success"], ref["found"]))
        if not ref["found"]:
            assert g == ref
            continue
        if not case["stable"]:
            continue
        assert (g["target"], g["num_steps"]) == (ref["target"], ref["num_steps"]), tag
        assert g["route_detail"].get("strategy") == ref["route_detail"].get("strategy"), tag
        assert g["route_detail"].get("m1_scale_g") == ref["route_detail"].get("m1_scale_g"), tag
        if ref["num_steps"] == 0:      # a direct purchase: nothing of it is simulated
            assert g == ref, tag
            outcomes.add("purchase")
        worst.see(g["optimal_cost"], ref["optimal_cost"], case["spread"].get("/result/optimal_cost", 0.0), True, tag + " optimal_cost")
    assert (True, True) in outcomes and (False, False) in outcomes and "purchase" in outcomes
    print("whole requests: largest deviation-to-bound ratio %.3g at %s" % (worst.ratio, worst.where))


def test_batch_independence(handle, whole):
    """device against device, bit-equal: a candidate alone, among 65 candidates of its world, in the whole mixed batch"""
    from xenoverse_amd.chemverse import chain_costs
    cands = chain_candidates()
    k = next(i for i, c in enumerate(cands) if c["world"] == 1 and len(c["chain"]) == 3 and c["seconds"] < 3.0)
    alone = chain_costs(None, [cands[k]], handle=handle, details=True)
    others = [c for c in cands if c["world"] == 1 and c["seconds"] < 3.0]
    crowd = [dict(others[i % len(others)], min_yield_g=0.25 + 0.02 * i) for i in range(32)] + [cands[k]] + \
            [dict(others[i % len(others)], min_yield_g=0.3 + 0.03 * i) for i in range(32)]
    assert len(crowd) == 65
    among = chain_costs(None, crowd, handle=handle, details=True)
    assert handle.check_errors() == 0
    assert alone[0][0] == among[0][32] == whole[0][k] and alone[0][0] is not None
    assert same_solved(alone[1][0], among[1][32]) and same_solved(alone[1][0], whole[1][k])


def test_handle_reuse(handle):
    from xenoverse_amd.chemverse import ChemVerseOptimal, chain_costs, one_pot_costs
    cands = [c for c in chain_candidates() if c["seconds"] < 3.0]
    pots = [dict(c, world=w) for _, w, c in ou.all_cases("one_pots")][:1]
    first = chain_costs(None, cands[:2], handle=handle, details=True)
    second = one_pot_costs(None, pots, handle=handle, details=True)
    third = chain_costs(None, cands[2:], handle=handle, details=True)
    for call, args, got in ((chain_costs, cands[:2], first), (one_pot_costs, pots, second), (chain_costs, cands[2:], third)):
        fresh = ChemVerseOptimal(worlds(), 64)
        try:
            want = call(None, args, handle=fresh, details=True)
        finally:
            fresh.close()
        assert got[0] == want[0]
        flat = lambda d: d if call is chain_costs else [s for _, ss in d for s in ss]      # noqa: E731
        assert all(same_solved(a, b) for a, b in zip(flat(got[1]), flat(want[1])))


def test_failing_first_stage_leaves_neighbours_alone(handle, whole):
    """a route whose first stage is set above the autoclave's max_temp_C fails its equipment check: None, neighbours as before"""
    from xenoverse_amd.chemverse import chain_costs
    cands = chain_candidates()
    near = [i for i, c in enumerate(cands) if c["world"] == 1 and c["seconds"] < 3.0][:2]
    tab = ou.fixture("b")["tab"]
    e = tab["equip_names"].index("autoclave")
    hot = tab["equip_specs"][e]["max_temp_C"] + 10.0
    bad = dict(cands[near[0]], conditions={0: (hot, 60.0)})
    results, solved = chain_costs(None, [cands[near[0]], bad, cands[near[1]]], handle=handle, details=True)
    assert handle.check_errors() == 0
    assert results[1] is None and not solved[1]["found"] and solved[1]["bits"] == 0
    for j, i in ((0, near[0]), (2, near[1])):
        assert results[j] == whole[0][i] and same_solved(solved[j], whole[1][i])


def test_route_longer_than_the_limit_is_refused(handle, whole):
    from xenoverse_amd.chemverse import chain_costs
    cands = chain_candidates()
    with pytest.raises(_lib.XenoError, match="CHAIN_MAX") as ei:
        chain_costs(None, [dict(world=2, target="C005", chain=list(range(T.CHAIN_MAX + 1)), min_yield_g=0.5)], handle=handle)
    assert ei.value.code == _lib.XV_ERR_UNSUPPORTED
    # the C entry refuses the width too, naming its limit, and the handle stays usable
    import ctypes
    import torch
    b = handle.batch
    z = torch.zeros(64, dtype=torch.float64, device=b.device)      # never read: the width is refused before any launch
    out = _lib.ChemOptOut()
    rc = b.lib.xv_chem_optimal(b._h, 1, T.CHAIN_MAX + 1, 1, 1, *([_lib.ptr(z)] * 13), 5.0, ctypes.byref(out), None)
    assert rc == _lib.XV_ERR_UNSUPPORTED and b"XV_CHEM_CHAIN_MAX = %d" % T.CHAIN_MAX in b.lib.xv_last_error()
    k = next(i for i, c in enumerate(cands) if c["seconds"] < 3.0 and c["found"])
    again = chain_costs(None, [cands[k]], handle=handle, details=True)
    assert handle.check_errors() == 0
    assert again[0][0] == whole[0][k] and same_solved(again[1][0], whole[1][k])
