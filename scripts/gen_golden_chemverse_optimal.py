"""Record the reference's cost oracle (xenoverse/chemverse/environment/api.py compute_optimal_cost :1777-2266) on the committed
worlds tests/golden/chemverse_world_{a,b,c}.json -> tests/golden/chemverse_opt_{a,b,c}.npz.  Runs only where the reference
tree is; the tests read the fixtures alone.

What a fixture holds (one JSON document, `cases_json`; floats are written with repr and read back bit for bit):
  routes        for every chemical above layer 1 the routes of _find_reaction_chains at (5 routes, max(6, 2 layers) steps),
                the whole request's search, and at (5, 6), the one-pot search's
  conditions    _optimal_temp_for_reaction of every reaction
  chains        single routes through _compute_chain_cost: every decision (the 30 bisection passes and the pass at scale_hi),
                best_scale, the unrounded yield, the result dict, and of the pass at best_scale every step's charge and the
                simulator's consumed / produced / byproduct dicts, unrounded
  one_pots      (world, target) requests through _compute_one_pot_cost: the result dict and, per (charge, temperature)
                candidate in the reference's order, the decisions, best_scale, the charge in the reference's own order and
                the final pool of the pass at best_scale
  requests      whole compute_optimal_cost calls and their result dicts
and per case `seconds` (one reference run, this machine), `stable`, `order_free` and, per float, `spread`:
  * eight further runs with the simulator's exp / log moved by a random integer in [-2, 2] ulp (the method of
    scripts/gen_golden_chemverse.py) and four further string-hash seeds
  * stable: decisions and discrete outcomes the same in every run; order_free: bit-identical under every hash seed; spread:
    the largest deviation of a float under the perturbed runs.
The script stops unless at least 7 of every 8 recorded cases are stable, a stable found and a stable None candidate exist
and every listed branch has a candidate; then it runs the host restatement (xenoverse_amd/chemverse/optimal_host.py) on
everything recorded, whole requests included, and stops on any difference where order_free holds.

usage: python scripts/gen_golden_chemverse_optimal.py      (spawns its workers with fixed PYTHONHASHSEEDs; some minutes)
"""
import concurrent.futures as cf
import io
import json
import os
import subprocess
import sys
import tempfile
import time
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import _refimport  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
TAGS = ("a", "b", "c")
HASH_SEEDS = (0, 1, 2, 3, 4)
N_PERTURBED = 8
SEED = 20262
MAX_TIME = 28800.0
CHAINS = {      # tag -> (target, route, min_yield_g).  The routes without their first reaction are hand-made: the search never
    # gives one, a caller of chain_costs can — their first reactant above layer 1 is charged at the 0.01 g floor
    "a": [("C012", ["R004"], 0.5)],
    "b": [("C004", ["R003", "R002", "R001"], 0.5), ("C004", ["R010", "R002", "R001"], 0.5), ("C004", ["R002", "R001"], 0.002)],
    "c": [("C005", ["R003", "R002", "R001"], 0.5), ("C005", ["R003", "R005", "R004", "R007", "R002", "R011", "R027"], 0.5),
          ("C005", ["R002", "R001"], 0.5)],
}
EXTRA_CHAINS = 1      # per world: the shortest further route with a layer-1 catalyst
ONE_POTS = {"a": [("C012", 0.5)], "b": [("C004", 0.5)], "c": [("C005", 0.5)]}      # a / C012: every candidate fails, None
REQUESTS = {"a": [dict(min_medicinal_value=1.0, max_toxicity=4.0, min_yield_g=0.5)],
            "b": [dict(min_medicinal_value=3.0, max_toxicity=4.0, min_yield_g=0.5)],
            "c": [dict(min_medicinal_value=2.5, max_toxicity=4.0, min_yield_g=0.5),
                  # C005, the layer-1 C011 and C024 qualify: the direct purchase competes with routes and one-pots
                  dict(min_medicinal_value=0.25, max_toxicity=1.6, min_yield_g=0.5)]}
BRANCHES = ("chain_found", "chain_none", "chain_probe_run", "catalyst_layer1", "pool_floor", "one_pot_found", "one_pot_none",
            "request_found", "request_nothing_qualifies", "request_purchase")
GAPS = ("chain_time_rule",)      # reported with what was found, not required


def world_path(tag):
    return os.path.join(GOLD, "chemverse_world_%s.json" % tag)


def extra_chains(tag, world, env):
    """further routes of the world's own search: with a layer-1 catalyst, and with a reactant or catalyst above layer 1 that
    the route has not made when it is charged (the 0.01 floor) — the shortest of each, where the world has one"""
    picks, seen = [], set(tuple(r) for _, r, _ in CHAINS[tag])
    for want in ("catalyst", "floor"):
        best = None
        for cid, chem in world.chemicals.items():
            if chem.layer <= 1:
                continue
            for chain in env._find_reaction_chains(cid, 5, max(6, world.num_layers * 2)):
                ids = tuple(r.id for r in chain)
                if ids in seen:
                    continue
                made = set()
                cat = any(world.chemicals[c].layer == 1 for r in chain for c in r.catalysts)
                floor = False
                for r in chain:
                    for c in [x for x, _ in r.reactants] + list(r.catalysts):
                        if world.chemicals[c].layer > 1 and c not in made:
                            floor = True
                    made.update(p for p, _ in r.products)
                    made.update(p for p, _ in r.byproducts)
                if (cat if want == "catalyst" else floor) and (best is None or len(ids) < len(best[1])):
                    best = (cid, list(ids), 0.5)
        if best is not None:
            seen.add(tuple(best[1]))
            picks.append(best)
    return picks[:EXTRA_CHAINS]


def worker(out_path, perturb_seed):
    """one run of the reference over every case -> JSON.  perturb_seed >= 0: exp / log moved by up to 2 ulp"""
    _refimport.setup()
    from gen_golden_chemverse import PerturbedNumpy
    from xenoverse.chemverse.environment import api, simulator as sim
    if perturb_seed >= 0:
        sim.np = PerturbedNumpy(np.random.RandomState(SEED + perturb_seed))
    real_sim = api.simulate_chain_reaction
    calls = []

    def traced(world, amounts, T, P, dur, **kw):
        res = real_sim(world, amounts, T, P, dur, **kw)
        calls.append(dict(amounts=dict(amounts), T=T, dur=dur, equipment=kw.get("equipment"), res=res))
        return res

    api.simulate_chain_reaction = traced
    out = {}
    for tag in TAGS:
        env = api.ChemistryEnvironment(world_path(tag))
        world = env._world
        doc = dict(routes={}, conditions={}, chains=[], one_pots=[], requests=[])
        for cid, chem in world.chemicals.items():
            if chem.layer > 1:
                doc["routes"][cid] = {"request": [[r.id for r in ch] for ch in
                                                  env._find_reaction_chains(cid, 5, max(6, world.num_layers * 2))],
                                      "one_pot": [[r.id for r in ch] for ch in env._find_reaction_chains(cid, 5, 6)]}
        for rid, rxn in world.reactions.items():
            doc["conditions"][rid] = list(env._optimal_temp_for_reaction(rxn))

        for target, route, m in CHAINS[tag] + extra_chains(tag, world, env):
            chain = [world.reactions[r] for r in route]
            passes = []
            real_chain = env._simulate_chain

            def chain_traced(ch, tid, scale, passes=passes):
                first = len(calls)
                res = real_chain(ch, tid, scale)
                passes.append(dict(scale=scale, result=res, calls=calls[first:]))
                return res

            env._simulate_chain = chain_traced
            t0 = time.time()
            result = env._compute_chain_cost(chain, target, m, MAX_TIME)
            seconds = time.time() - t0
            del env._simulate_chain
            bits = 0
            for i, p in enumerate(passes[:30]):
                if p["result"]["target_yield_g"] >= m:
                    bits |= 1 << i
            probe = bits == 0
            if probe and passes[30]["result"]["target_yield_g"] >= m:
                bits |= 1 << 31
            found = bits != 0
            last = passes[-1]
            case = dict(target=target, chain=route, min_yield_g=m, max_time_seconds=MAX_TIME, seconds=seconds, bits=bits,
                        found=found, probe_run=probe, result=result, best_scale=last["scale"] if found else 0.0)
            if found:      # the pass at best_scale: every step's charge and totals, and the virtual pool's unrounded yield
                vpool, steps = {}, []
                for c in last["calls"]:
                    r = c["res"]
                    steps.append(dict(amounts=c["amounts"], T=c["T"], dur=c["dur"], consumed=r.get("consumed_g", {}),
                                      produced=r.get("produced_g", {}), byproduct=r.get("byproduct_g", {}),
                                      failure=bool(r.get("equipment_failure", False))))
                    for k, g in r.get("consumed_g", {}).items():
                        vpool[k] = max(0.0, vpool.get(k, 0.0) - g)
                    for key in ("produced_g", "byproduct_g"):
                        for k, g in r.get(key, {}).items():
                            if g >= 0.001:
                                vpool[k] = vpool.get(k, 0.0) + g
                case.update(steps=steps, yield_unrounded=vpool.get(target, 0.0))
            doc["chains"].append(case)

        for target, m in ONE_POTS.get(tag, []):
            first = len(calls)
            t0 = time.time()
            result = env._compute_one_pot_cost(target, m, MAX_TIME)
            seconds = time.time() - t0
            mine, cands, i = calls[first:], [], 0
            while i < len(mine):      # per candidate: 12 passes, the pass at scale_hi if none passed, the pass at best_scale
                bits, best, lo, hi = 0, None, 0.5, 200.0
                for it in range(12):
                    mid = (lo + hi) / 2.0
                    if mine[i + it]["res"]["final_pool_g"].get(target, 0.0) >= m:
                        bits |= 1 << it
                        best, hi = mid, mid
                    else:
                        lo = mid
                i += 12
                if best is None:
                    if mine[i]["res"]["final_pool_g"].get(target, 0.0) >= m:
                        bits |= 1 << 31
                        best = hi
                    i += 1
                cand = dict(T=mine[i - 1]["T"], bits=bits, found=best is not None, best_scale=best or 0.0)
                if best is not None:
                    cand.update(charge_order=list(mine[i]["amounts"]), amounts=mine[i]["amounts"],
                                final_pool=mine[i]["res"]["final_pool_g"])
                    i += 1
                cands.append(cand)
            doc["one_pots"].append(dict(target=target, min_yield_g=m, max_time_seconds=MAX_TIME, seconds=seconds,
                                        result=result, candidates=cands))

        for req in REQUESTS[tag]:
            t0 = time.time()
            result = env.compute_optimal_cost(**req)
            doc["requests"].append(dict(request=req, seconds=time.time() - t0, result=result))
        out[tag] = doc
    with open(out_path, "w") as f:
        json.dump(out, f)


def floats_of(x, path=""):
    """every float of a nested case, by path"""
    if isinstance(x, bool) or x is None or isinstance(x, (str, int)):
        return
    if isinstance(x, float):
        yield path, x
    elif isinstance(x, dict):
        for k, v in x.items():
            if k != "seconds":
                yield from floats_of(v, path + "/" + str(k))
    elif isinstance(x, list):
        for i, v in enumerate(x):
            yield from floats_of(v, path + "/" + str(i))


def discrete_of(x):
    """a case without its floats and timings: what must not move"""
    if isinstance(x, float):
        return None
    if isinstance(x, dict):
        return {k: discrete_of(v) for k, v in sorted(x.items()) if k not in ("seconds", "charge_order")}
    if isinstance(x, list):
        return [discrete_of(v) for v in x]
    return x


def merge(base, perturbed, seeded):
    for tag in TAGS:
        for group in ("chains", "one_pots", "requests"):
            for i, case in enumerate(base[tag][group]):
                others = [r[tag][group][i] for r in perturbed + seeded]
                mine, fixed = dict(floats_of(case)), discrete_of(case)      # before the case gains its marks
                case["stable"] = all(discrete_of(o) == fixed for o in others)
                case["order_free"] = all(discrete_of(o) == fixed and dict(floats_of(o)) == mine
                                         for o in (r[tag][group][i] for r in seeded))
                spread = {}
                for o in (r[tag][group][i] for r in perturbed):
                    theirs = dict(floats_of(o))
                    for k, v in mine.items():
                        if k in theirs:
                            spread[k] = max(spread.get(k, 0.0), abs(theirs[k] - v))
                case["spread"] = spread
    return base


def self_check(doc):
    """the host restatement on everything recorded"""
    from xenoverse_amd.chemverse import build_tables, optimal_host as H
    from xenoverse_amd.chemverse.optimal import chain_costs, compute_optimal_costs, one_pot_costs
    bad = []
    for tag in TAGS:
        tab = build_tables(json.load(open(world_path(tag))))
        ids, rids = tab["chem_ids"], tab["rxn_ids"]
        d = doc[tag]
        for cid, rec in d["routes"].items():
            for key, steps in (("request", max(6, tab["num_layers"] * 2)), ("one_pot", 6)):
                got = [[rids[r] for r in ch] for ch in H.find_reaction_chains(tab, cid, 5, steps)]
                if got != rec[key]:
                    bad.append("%s routes %s %s" % (tag, cid, key))
        temps, durs = H.optimal_conditions(tab)
        for r, rid in enumerate(rids):
            if [temps[r], durs[r]] != d["conditions"][rid]:
                bad.append("%s conditions %s" % (tag, rid))
        res, solved = chain_costs([tab], d["chains"], backend="host", details=True)
        for case, r, s in zip(d["chains"], res, solved):
            if not case["order_free"]:
                continue
            if (s["bits"], s["found"], s["best_scale"]) != (case["bits"], case["found"], case["best_scale"]) or r != case["result"]:
                bad.append("%s chain %s %s" % (tag, case["target"], case["chain"]))
            elif case["found"] and s["rows"]["yield"] != case["yield_unrounded"]:
                bad.append("%s chain %s %s: unrounded yield" % (tag, case["target"], case["chain"]))
        res, parts = one_pot_costs([tab], d["one_pots"], backend="host", details=True)
        for case, r, (plans, solved) in zip(d["one_pots"], res, parts):
            if not case["order_free"]:
                continue
            if r != case["result"] or len(solved) != len(case["candidates"]):
                bad.append("%s one-pot %s" % (tag, case["target"]))
                continue
            for cand, p, s in zip(case["candidates"], plans, solved):
                if (s["bits"], s["found"], s["best_scale"], p["steps"][0]["T"]) != (cand["bits"], cand["found"],
                                                                                    cand["best_scale"], cand["T"]):
                    bad.append("%s one-pot %s at %s" % (tag, case["target"], cand["T"]))
        res = compute_optimal_costs([tab], [c["request"] for c in d["requests"]], backend="host")
        for case, r in zip(d["requests"], res):
            if case["order_free"] and r != case["result"]:
                bad.append("%s request %s" % (tag, case["request"]))
    return bad


def count_branches(doc):
    n = dict((b, 0) for b in BRANCHES + GAPS)
    for tag in TAGS:
        world = json.load(open(world_path(tag)))
        layer = {c: v["layer"] for c, v in world["chemicals"].items()}
        for case in doc[tag]["chains"]:
            n["chain_found" if case["found"] else "chain_none"] += case["stable"]
            n["chain_probe_run"] += case["probe_run"]
            made = set()
            for rid in case["chain"]:
                rxn = world["reactions"][rid]
                n["catalyst_layer1"] += any(layer[c] == 1 for c in rxn["catalysts"])
                n["pool_floor"] += any(layer[c] > 1 and c not in made for c in [x for x, _ in rxn["reactants"]] + rxn["catalysts"])
                made.update(p for p, _ in rxn["products"] + rxn["byproducts"])
            n["chain_time_rule"] += case["found"] and case["result"] is None
        for case in doc[tag]["one_pots"]:
            n["one_pot_found" if case["result"] is not None else "one_pot_none"] += 1
        for case in doc[tag]["requests"]:
            r = case["result"]
            n["request_found"] += bool(r["found"])
            n["request_nothing_qualifies"] += not r["success"]
            n["request_purchase"] += bool(r["found"]) and r["num_steps"] == 0
    return n


def write_npz(path, arrays):
    """a deterministic .npz: fixed timestamps, sorted names"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.save(buf, arrays[k], allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(2026, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def count_routes(n_seeds=100):
    """--count-routes: the longest route _find_reaction_chains gives at (5 routes, max(6, 2 layers) steps) over the 40
    evaluation worlds and the samplers' presets — what XV_CHEM_CHAIN_MAX is set from; a graph search only"""
    _refimport.setup()
    from xenoverse.chemverse.world_gen.models import World
    from xenoverse.chemverse.world_gen.sampler import WorldSampler
    from xenoverse.chemverse.world_gen.sampler_v2 import BackwardDesignSampler
    from xenoverse_amd.chemverse import build_tables, optimal_host as H

    def longest(world):
        tab = build_tables(world.to_dict())
        steps = max(6, tab["num_layers"] * 2)
        routes = [ch for c in range(tab["C"]) if tab["layer"][c] > 1 for ch in H.find_reaction_chains(tab, c, 5, steps)]
        return max([len(ch) for ch in routes] or [0]), tab["num_layers"]

    d = os.path.join(_refimport.REF_ROOT, "xenoverse", "chemverse", "worlds")
    files = sorted(f for f in os.listdir(d) if f.startswith("eval_world_") and f.endswith(".json"))
    rows = [longest(World.load(os.path.join(d, f))) for f in files]
    print("evaluation worlds: %d, longest route %d, most layers %d" % (len(rows), max(r[0] for r in rows), max(r[1] for r in rows)))
    for name, cls in (("WorldSampler", WorldSampler), ("BackwardDesignSampler", BackwardDesignSampler)):
        for level in ("easy", "medium", "hard"):
            rows = [longest(cls(seed, complexity_level=level).sample_world("w%d" % seed)) for seed in range(n_seeds)]
            print("%s %s, %d seeds: longest route %d, most layers %d" % (name, level, n_seeds, max(r[0] for r in rows),
                                                                        max(r[1] for r in rows)))


def main():
    if len(sys.argv) >= 4 and sys.argv[1] == "--worker":
        return worker(sys.argv[2], int(sys.argv[3]))
    if len(sys.argv) >= 2 and sys.argv[1] == "--count-routes":
        return count_routes(int(sys.argv[2]) if len(sys.argv) > 2 else 100)
    with tempfile.TemporaryDirectory() as tmp:
        jobs = [("seed%d" % hs, hs, -1) for hs in HASH_SEEDS] + [("ulp%d" % k, 0, k) for k in range(N_PERTURBED)]

        def run(job):
            name, hs, k = job
            out = os.path.join(tmp, name + ".json")
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--worker", out, str(k)],
                                  env=dict(os.environ, PYTHONHASHSEED=str(hs)))
            return json.load(open(out))

        with cf.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
            runs = list(ex.map(run, jobs))
    base, seeded, perturbed = runs[0], runs[1:len(HASH_SEEDS)], runs[len(HASH_SEEDS):]
    doc = merge(base, perturbed, seeded)
    cases = [c for tag in TAGS for g in ("chains", "one_pots", "requests") for c in doc[tag][g]]
    unstable = sum(not c["stable"] for c in cases)
    print("cases %d, unstable %d, not order_free %d" % (len(cases), unstable, sum(not c["order_free"] for c in cases)))
    if unstable * 8 > len(cases):
        sys.exit("more than one case in eight is unstable")
    counts = count_branches(doc)
    print("branches:", counts)
    missing = [b for b in BRANCHES if counts[b] == 0]
    if missing:
        sys.exit("no candidate for the branches %s" % missing)
    bad = self_check(doc)
    if bad:
        sys.exit("the host restatement differs from the reference on:\n  " + "\n  ".join(bad))
    print("host restatement equals the reference on every recorded case that is order_free")
    for tag in TAGS:
        doc[tag]["branches"] = counts
        path = os.path.join(GOLD, "chemverse_opt_%s.npz" % tag)
        write_npz(path, {"cases_json": np.frombuffer(json.dumps(doc[tag]).encode(), np.uint8)})
        print(path, os.path.getsize(path), "bytes")
        for g in ("chains", "one_pots", "requests"):
            for c in doc[tag][g]:
                print("  %s %s: %.1f s, stable %s, order_free %s" % (g, c.get("chain") or c.get("target") or c.get("request"),
                                                                   c["seconds"], c["stable"], c["order_free"]))


if __name__ == "__main__":
    main()
