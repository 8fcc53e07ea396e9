"""Tasks per second of the on-device AnyHVAC task sampler, beside the host path it replaces.  No pass mark.

(i)  `sample_tasks_device(n)` at the default configuration and at a small-room configuration (rooms of 5-8 x 5-8 cells of
     1-2 m): accepted tasks per second, candidates tried, the status histogram.  The first call of each shape is a warm-up
     and is not timed; each figure is the median of `--repeats` calls, all samples are kept.
(ii) the host path for the same configurations: `HVACTaskSampler` (numpy's stream) + `tables.build_tables`, the way
     `HVACVecEnv.set_task(list of dicts)` makes its rows.  It takes seconds per task, so `--host-tasks` tasks are timed and
     the rate is EXTRAPOLATED from them: the entry says so (`extrapolated_from_tasks`).

Clock: time.perf_counter around calls that end in a stream synchronise (device) or return (host).

usage: python scripts/bench_anyhvac_sampler.py [--tasks 64] [--small-tasks 1024] [--host-tasks 3] [--repeats 3]
                                               [--out profiles/anyhvac_sampler_bench.json]
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from xenoverse_amd.anyhvac import HVACTaskSampler, build_tables, sample_tasks_device, table_dims  # noqa: E402
from xenoverse_amd.engine import Engine  # noqa: E402

SMALL = dict(ROOM_W_GRID_SIZE_LOW=5, ROOM_W_GRID_SIZE_HIGH=9, ROOM_L_GRID_SIZE_LOW=5, ROOM_L_GRID_SIZE_HIGH=9,
             CELL_SIZE_LOW=1.0, CELL_SIZE_HIGH=2.0)


def device_rate(engine, n, config, repeats, generate_task=False):
    sample_tasks_device(min(n, 8), seed=0, config=config, engine=engine, generate_task=generate_task)      # warm-up
    samples, stats = [], None
    for r in range(repeats):
        engine.sync()
        t0 = time.perf_counter()
        t = sample_tasks_device(n, seed=1 + r, config=config, engine=engine, generate_task=generate_task)
        engine.sync()
        samples.append(time.perf_counter() - t0)
        stats = t["stats"]
    s = statistics.median(samples)
    return dict(tasks=n, dims=list(table_dims(config)), generate_task=generate_task, seconds=s, tasks_per_s=n / s,
                samples_s=samples, last_stats={k: stats[k] for k in ("candidates", "accepted", "status", "batch")})


def host_rate(n, config, generate_task=False):
    np.random.seed(0)
    random.seed(0)
    t0 = time.perf_counter()
    tasks = []
    while len(tasks) < n:
        try:
            tasks.append(HVACTaskSampler(config=config))
        except ValueError:      # the reference's one-cooler unification raises: drawn again, as a caller would
            pass
    t1 = time.perf_counter()
    build_tables(tasks, generate_task=generate_task)
    t2 = time.perf_counter()
    return dict(extrapolated_from_tasks=n, generate_task=generate_task, sampler_s_per_task=(t1 - t0) / n,
                build_tables_s_per_task=(t2 - t1) / n, tasks_per_s=n / (t2 - t0),
                note="HVACTaskSampler + build_tables on the host: a handful of tasks timed, the rate extrapolated from them")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tasks", type=int, default=64)
    ap.add_argument("--small-tasks", type=int, default=1024)
    ap.add_argument("--host-tasks", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "anyhvac_sampler_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_anyhvac_sampler.py measures on the GPU; none found")
    engine = Engine("cuda:0")
    out = dict(device=torch.cuda.get_device_name(0), clock="time.perf_counter around calls ending in a stream synchronise",
               default=dict(device=device_rate(engine, a.tasks, None, a.repeats),
                            device_generate_task=device_rate(engine, a.tasks, None, a.repeats, generate_task=True),
                            host=host_rate(a.host_tasks, None)),
               small=dict(config=SMALL, device=device_rate(engine, a.small_tasks, SMALL, a.repeats),
                          host=host_rate(max(a.host_tasks, 8), SMALL)))
    engine.close()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: {q: (v[q]["tasks_per_s"] if isinstance(v[q], dict) and "tasks_per_s" in v[q] else None)
                          for q in v} for k, v in out.items() if isinstance(v, dict)}))


if __name__ == "__main__":
    main()
