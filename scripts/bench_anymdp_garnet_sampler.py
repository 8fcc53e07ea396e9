"""Garnet and bandit AnyMDP tasks per second, made and set: the on-device samplers beside the host loop they replace.
No pass mark.

(i)   Garnet, device: `sample_garnet_tasks_device(n)` at the defaults (128 states, 5 actions, b = 2) followed by
      `set_task(tables)` on an env batch with one env per task: the tables are made on the GPU and borrowed as they are.
      `sample` is the sampler alone, with the bytes it stores per second beside the 8 TB/s peak (a description only: the
      kernel has an fp64 log / sincos per stored entry in front of every store).
(ii)  Garnet, host: the loop over `GarnetTaskSampler(seed=i)` on numpy's stream followed by `set_task(list)`, over
      `--host-tasks` tasks, reported per task: what a user paid before.
(iii) Bandit: `sample_bandit_tasks_device(n, 5)` followed by `set_task(tables)`, with the status histogram, beside the loop
      over `AnyMDPTaskSampler(state_space=1, seed=i)` and `set_task(list)` over `--host-bandits` tasks.

The first device call of each size is a warm-up and is not timed; a device figure is the median of `--repeats` calls; all
samples are kept.  Clock: time.perf_counter around calls behind a device synchronise.

usage: python scripts/bench_anymdp_garnet_sampler.py [--tasks 1024 4096] [--bandits 65536] [--repeats 5] [--host-tasks 64]
                                                     [--host-bandits 1024] [--out profiles/anymdp_garnet_sampler.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from xenoverse_amd.anymdp import (AnyMDPTaskSampler, AnyMDPVecEnv, GarnetTaskSampler, row_lines,  # noqa: E402
                                  sample_bandit_tasks_device, sample_garnet_tasks_device)
from xenoverse_amd.engine import Engine  # noqa: E402

PEAK_BYTES_PER_S = 8.0e12
S, A, B = 128, 5, 2


def _median(fn, repeats):
    samples = []
    for r in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(r)
        torch.cuda.synchronize()
        samples.append(time.perf_counter() - t0)
    return statistics.median(samples), samples


def _entry(n, seconds, samples):
    return dict(tasks=n, seconds=seconds, tasks_per_s=n / seconds, samples_s=samples)


def _device(n, engine, repeats, sample, bytes_per_task):
    env = AnyMDPVecEnv(n, engine=engine)
    try:
        env.set_task(sample(0))      # warm-up
        s, samples = _median(lambda r: env.set_task(sample(1 + r)), repeats)
        k, k_samples = _median(lambda r: sample(1 + r), repeats)
    finally:
        env.close()
    out = _entry(n, s, samples)
    out["sample"] = _entry(n, k, k_samples)
    rate = n * bytes_per_task / k
    out["sample"].update(bytes_stored=n * bytes_per_task, bytes_per_s=rate, share_of_peak=rate / PEAK_BYTES_PER_S)
    return out


def _host(n, engine, make):
    env = AnyMDPVecEnv(n, engine=engine)
    try:
        s, samples = _median(lambda r: env.set_task(make(1000 * r)), 1)
        k, k_samples = _median(lambda r: make(1000 * r), 1)
    finally:
        env.close()
    out = _entry(n, s, samples)
    out["sample"] = _entry(n, k, k_samples)
    out["seconds_per_task"] = s / n
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tasks", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--bandits", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-tasks", type=int, default=64)
    ap.add_argument("--host-bandits", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "anymdp_garnet_sampler.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_anymdp_garnet_sampler.py measures on the GPU; none found")
    engine = Engine("cuda:0")
    out = dict(device=torch.cuda.get_device_name(0), clock="time.perf_counter around calls behind a device synchronise",
               peak_bytes_per_s=PEAK_BYTES_PER_S, sizes=dict(garnet=dict(state_space=S, action_space=A, b=B), bandit=dict(action_space=5)),
               garnet={}, bandit={})
    row_bytes = S * A * row_lines(S) * 128 + (S + 2 * 4 + 2) * 4 + 8 + 4 * 8      # the records + the task's small vectors
    for n in a.tasks:
        r = out["garnet"][str(n)] = dict(device=_device(
            n, engine, a.repeats, lambda seed: sample_garnet_tasks_device(n, S, A, b=B, seed=seed, engine=engine), row_bytes))
        print("garnet", n, json.dumps(dict(tasks_per_s=r["device"]["tasks_per_s"], sample=r["device"]["sample"]["tasks_per_s"],
                                           share_of_peak=r["device"]["sample"]["share_of_peak"])), flush=True)
    h = out["garnet"]["host"] = _host(a.host_tasks, engine,
                                      lambda seed: [GarnetTaskSampler(S, A, b=B, seed=seed + i) for i in range(a.host_tasks)])
    print("garnet host", json.dumps(dict(seconds_per_task=h["seconds_per_task"])), flush=True)
    for n in a.tasks:
        out["garnet"][str(n)]["speedup"] = out["garnet"][str(n)]["device"]["tasks_per_s"] / h["tasks_per_s"]

    n = a.bandits
    stats = {}

    def bandits(seed):
        t = sample_bandit_tasks_device(n, 5, seed=seed, engine=engine)
        stats.update(t["stats"])
        return t

    bandit_bytes = 2 * 5 * row_lines(2) * 128 + (2 + 2 * 4 + 2) * 4 + 8 + 4 * 8 + 4
    d = out["bandit"]["device"] = _device(n, engine, a.repeats, bandits, bandit_bytes)
    d["stats"] = dict(candidates=stats["candidates"], status=stats["status"], batch=stats["batch"])
    hb = out["bandit"]["host"] = _host(a.host_bandits, engine,
                                       lambda seed: [AnyMDPTaskSampler(1, 5, seed=seed + i) for i in range(a.host_bandits)])
    out["bandit"]["speedup"] = d["tasks_per_s"] / hb["tasks_per_s"]
    print("bandit", n, json.dumps(dict(tasks_per_s=d["tasks_per_s"], host_tasks_per_s=hb["tasks_per_s"], status=d["stats"]["status"])),
          flush=True)
    engine.close()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
