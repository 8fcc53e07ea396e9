"""ChemVerse's cost oracle on the device (csrc/chemverse_optimal.hip, xenoverse_amd.chemverse.compute_optimal_costs): batches of
1, 64 and 1,024 compute_optimal_cost requests on the committed fixture worlds b and c (min_medicinal_value 3.0 / 2.5,
max_toxicity 4.0), alternating, min_yield_g spread evenly over [0.25, 2.0] — every candidate of every request, routes and
one-pot charges, through one set of launches.

Reported per batch size: the candidates (lanes), the launches issued, the whole call's wall-clock time (route search and
planning on the host, uploads, launches, pricing: what a caller sees) and per request, the time inside xv_chem_optimal's
launches and the longest single launch (events between the launches).  Beside them, unless --gpu-only: the host restatement
(optimal_host.py) for ONE request of world b on one core of the same box.

usage: python scripts/bench_chemverse_optimal.py [--quick] [--gpu-only] [--out profiles/chemverse_optimal.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = (1, 64, 1024)
CONSTRAINTS = (dict(min_medicinal_value=3.0, max_toxicity=4.0), dict(min_medicinal_value=2.5, max_toxicity=4.0))


def requests_of(n):
    yields = np.linspace(0.25, 2.0, n) if n > 1 else np.array([0.5])
    return [dict(CONSTRAINTS[i % 2], world=i % 2, min_yield_g=float(round(y, 4))) for i, y in enumerate(yields)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="1 and 64 requests only")
    ap.add_argument("--gpu-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chemverse_optimal.json"))
    args = ap.parse_args()
    import torch
    from xenoverse_amd.build import source_hash
    from xenoverse_amd.chemverse import ChemVerseOptimal, compute_optimal_costs
    from xenoverse_amd.chemverse import optimal_host as H
    from xenoverse_amd.chemverse import build_tables
    worlds = [json.load(open(os.path.join(ROOT, "tests", "golden", "chemverse_world_%s.json" % t))) for t in "bc"]
    tabs = [build_tables(w) for w in worlds]
    res = {"device": torch.cuda.get_device_name(0), "kernel_source_hash": source_hash(["chemverse.hip", "chemverse_optimal.hip"]),
           "worlds": ["b", "c"], "batches": []}
    for n in SIZES[:2] if args.quick else SIZES:
        reqs = requests_of(n)
        lanes = sum(len(pl["chains"]) + sum(len(ps) for _, ps in pl["one_pot"])
                    for pl in (H.request_plans(tabs[r["world"]], r) for r in reqs))
        handle = ChemVerseOptimal(tabs, lanes)
        try:
            compute_optimal_costs(None, reqs[:1], handle=handle)      # warm-up: module load, first allocations
            handle.time_launches = True
            t0 = time.perf_counter()
            out = compute_optimal_costs(None, reqs, handle=handle)
            wall = time.perf_counter() - t0
            ms = handle.last_launch_ms
        finally:
            handle.close()
        row = dict(requests=n, lanes=lanes, found=sum(bool(o["found"]) for o in out), launches=len(ms), wall_s=wall,
                   wall_s_per_request=wall / n, launches_ms=float(sum(ms)), longest_launch_ms=float(max(ms)),
                   requests_per_s=n / wall)
        print(json.dumps(row), flush=True)
        res["batches"].append(row)
    if not args.gpu_only:
        t0 = time.perf_counter()
        ref = H.compute_optimal_cost_host(tabs[0], **{k: v for k, v in requests_of(1)[0].items() if k != "world"})
        res["host_one_request_s"] = time.perf_counter() - t0
        res["host_one_request_cost"] = ref["optimal_cost"]
        print(json.dumps({"host_one_request_s": res["host_one_request_s"], "optimal_cost": ref["optimal_cost"]}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
