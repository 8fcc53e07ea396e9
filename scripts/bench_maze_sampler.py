"""Device MazeWorld task sampler and resampler (csrc/maze_sampler.hip) against the host MazeTaskSampler.

Per argument set (n fixed at 15; the default n_range (9, 25)): seconds for 16,384 accepted tasks from
`sample_tasks_device` (every repetition a fresh seed, all samples kept; the time includes the host-side numpy.tan column
and the status read-back), the candidates spent and the status histogram, one `resample_tasks_device` over the batch, and
the host `MazeTaskSampler` on this box's CPU for 64 tasks of the same arguments in the same process, extrapolated to
16,384 and labelled as such (one core).

usage: python scripts/bench_maze_sampler.py [--quick] [--out profiles/maze_sampler_bench.json]
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
    ap.add_argument("--quick", action="store_true", help="1,024 tasks, 1 repetition, 8 host tasks")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from xenoverse_amd.engine import Engine
    from xenoverse_amd.mazeworld import MazeTaskSampler, resample_tasks_device, sample_tasks_device
    n_tasks, reps, n_host = (1024, 1, 8) if args.quick else (16384, 3, 64)
    eng = Engine("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "n_tasks": n_tasks, "cases": []}
    for name, kwargs in (("n15", dict(n_range=(15, 16))), ("default_n_range", dict())):
        sample_tasks_device(64, seed=99, engine=eng, **kwargs)      # warm-up: module load, allocator
        row = {"case": name, "sampler_kwargs": {k: list(v) for k, v in kwargs.items()}, "samples": []}
        out = None
        for r in range(reps):
            out = sample_tasks_device(n_tasks, seed=1000 + r, engine=eng, **kwargs)
            st = out["stats"]
            row["samples"].append({"seconds": st["seconds"], "candidates": st["candidates"], "status": st["status"],
                                   "batch": st["batch"], "passes_mean": float(out["info"]["passes"].mean()),
                                   "idle_mean": float(out["info"]["idle"].mean())})
            print(json.dumps({"case": name, **row["samples"][-1]}), flush=True)
        row["resample_seconds"] = []
        for r in range(reps):
            eng.sync()
            t0 = time.perf_counter()
            resample_tasks_device(out, seed=5, episode=r, engine=eng)
            row["resample_seconds"].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        for k in range(n_host):
            MazeTaskSampler(seed=7 + k, **kwargs)
        host = time.perf_counter() - t0
        row["host_MazeTaskSampler"] = {"tasks": n_host, "seconds": host,
                                       "seconds_for_n_tasks_extrapolated": host * n_tasks / n_host,
                                       "note": "one CPU core, extrapolated from %d tasks" % n_host}
        row["speedup_vs_host_extrapolated"] = row["host_MazeTaskSampler"]["seconds_for_n_tasks_extrapolated"] / \
            min(s["seconds"] for s in row["samples"])
        print(json.dumps({"case": name, "resample_seconds": row["resample_seconds"], "host": row["host_MazeTaskSampler"],
                          "speedup_vs_host_extrapolated": row["speedup_vs_host_extrapolated"]}), flush=True)
        res["cases"].append(row)
    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
