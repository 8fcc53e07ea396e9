"""Device LinDS task sampler and zero-order-hold builder (csrc/linds_sampler.hip) against the host path.

Per shape (16, 8, 8) and (32, 8, 8): seconds for 1,024 accepted tasks from `sample_tasks_device` (max_draws = 2^20; every
repetition a fresh seed, all samples kept), the candidates and start attempts spent, and `linds.task_sampler.sample_batch`
on this box's CPU for 32 tasks, extrapolated to 1,024 and labelled as such (one core; the host sampler gives up after
20,000 draws and shrinks the start states, the device does not).  Then `build_tables_device` against `build_tables` for the
1,024 sampled (16, 8, 8) tasks.

usage: python scripts/bench_linds_sampler.py [--quick] [--out profiles/linds_sampler_bench.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="128 tasks, 1 repetition, 4 host tasks")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from xenoverse_amd.engine import Engine
    from xenoverse_amd.linds import build_tables, build_tables_device, sample_tasks_device, task_dicts_from_device
    from xenoverse_amd.linds.task_sampler import sample_batch
    n_tasks, reps, n_host = (128, 1, 4) if args.quick else (1024, 3, 32)
    eng = Engine("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "n_tasks": n_tasks, "max_draws": 1 << 20, "shapes": []}
    keep = None
    for shape in ((16, 8, 8), (32, 8, 8)):
        sample_tasks_device(4, *shape, seed=99, engine=eng, max_draws=4096)      # warm-up: module load, allocator
        row = {"shape": shape, "samples": []}
        for r in range(reps):
            out = sample_tasks_device(n_tasks, *shape, seed=1000 + r, engine=eng, dense=(shape == (16, 8, 8) and r == 0))
            st = out["stats"]
            row["samples"].append({"seconds": st["seconds"], "candidates": st["candidates"], "status": st["status"],
                                   "attempts_of_accepted": st["attempts_total"], "attempts_log2_hist": st["attempts_log2"],
                                   "batch": st["batch"]})
            print(json.dumps({"shape": shape, **row["samples"][-1]}), flush=True)
            if "A" in out:
                keep = out
        t0 = time.perf_counter()
        sample_batch(n_host, seed=7, state_dim=shape[0], action_dim=shape[1], observation_dim=shape[2])
        host = time.perf_counter() - t0
        row["host_sample_batch"] = {"tasks": n_host, "seconds": host, "seconds_for_n_tasks_extrapolated": host * n_tasks / n_host,
                                    "note": "one CPU core, extrapolated from %d tasks; 20,000-draw cap with the shrinking fallback" % n_host}
        row["speedup_vs_host_extrapolated"] = row["host_sample_batch"]["seconds_for_n_tasks_extrapolated"] / \
            min(s["seconds"] for s in row["samples"])
        print(json.dumps({"shape": shape, "host": row["host_sample_batch"]}), flush=True)
        res["shapes"].append(row)
    tasks = task_dicts_from_device(keep)
    build_tables_device(tasks[:8], eng)      # warm-up
    dev_s, host_s = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        build_tables_device(tasks, eng)
        dev_s.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        build_tables(tasks)
        host_s.append(time.perf_counter() - t0)
    res["build_tables"] = {"tasks": len(tasks), "shape": (16, 8, 8), "build_tables_device_s": dev_s, "build_tables_s": host_s,
                           "note": "both include the host-side packing of the other table fields"}
    print(json.dumps(res["build_tables"]), flush=True)
    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
