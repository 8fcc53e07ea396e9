"""Accepted MetaLMV3 tasks per second of the on-device task sampler, beside the two paths that were there before it.
No pass mark.

(i)   `sample_tasks_device(n)` at the default size (32, 16, 32) and at the limits (256, 64, 128): generation and the
      acceptance protocol in one launch per batch; the result is the device tables `set_task` borrows.  Beside it
      `launch`: one `sample_candidates` launch of the same number of candidates alone, to show what of (i) is the kernel.
(ii)  `sample_and_check_tasks(n, backend="device")`: every candidate built on the host (MT19937, a RandomLMHost each),
      stacked and uploaded, four launches, filtered on the host.  Its result is a list of host objects, which `set_task`
      stacks and uploads again: `with_set_task` adds that, as a generator that goes on to `stream()` pays it.
(iii) `sample_and_check_tasks(n, backend="host")`: the numpy restatement, one candidate at a time.  `--host-tasks` tasks are
      timed and the rate is EXTRAPOLATED from them: the entry says so.

The first call of each shape and path is a warm-up and is not timed; each figure is the median of `--repeats` calls, all
samples are kept.  Clock: time.perf_counter around calls that end in a stream synchronise (device) or return (host).

usage: python scripts/bench_metalm_sampler.py [--tasks 4096] [--limit-tasks 256] [--host-tasks 32] [--repeats 3]
                                              [--out profiles/metalm_sampler.json]
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

from xenoverse_amd.engine import Engine  # noqa: E402
from xenoverse_amd.metalang import (MetaLMV3VecEnv, sample_and_check_tasks, sample_candidates,  # noqa: E402
                                    sample_tasks_device)


def _median(fn, repeats):
    samples = []
    for r in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(r)
        torch.cuda.synchronize()
        samples.append(time.perf_counter() - t0)
    return statistics.median(samples), samples


def device_sampler_rate(engine, n, shape, repeats):
    sample_tasks_device(min(n, 64), *shape, seed=0, engine=engine)      # warm-up
    last = {}

    def run(r):
        last["t"] = sample_tasks_device(n, *shape, seed=1 + r, engine=engine)
    s, samples = _median(run, repeats)
    stats = last["t"]["stats"]
    n_cand = stats["batch"]
    k, k_samples = _median(lambda r: sample_candidates(engine, 1 + r, 0, n_cand, *shape), repeats)
    return dict(tasks=n, seconds=s, tasks_per_s=n / s, samples_s=samples,
                last_stats={q: stats[q] for q in ("candidates", "accepted", "status", "batch")},
                launch=dict(candidates=n_cand, seconds=k, candidates_per_s=n_cand / k, samples_s=k_samples))


def parent_device_rate(n, shape, repeats):
    sample_and_check_tasks(min(n, 64), *shape, seed=0, backend="device")      # warm-up
    last = {}

    def run(r):
        last["tasks"], last["seeds"] = sample_and_check_tasks(n, *shape, seed=1000 * (1 + r), backend="device")
    s, samples = _median(run, repeats)
    env = MetaLMV3VecEnv(n)
    try:
        u, u_samples = _median(lambda r: env.set_task(last["tasks"]), repeats)
    finally:
        env.close()
    return dict(tasks=n, seconds=s, tasks_per_s=n / s, samples_s=samples,
                candidates=int(last["seeds"][-1]) - 1000 * repeats + 1,
                set_task=dict(seconds=u, samples_s=u_samples),
                with_set_task=dict(seconds=s + u, tasks_per_s=n / (s + u)))


def host_rate(n, shape):
    t0 = time.perf_counter()
    _, seeds = sample_and_check_tasks(n, *shape, seed=1, backend="host")
    s = time.perf_counter() - t0
    return dict(extrapolated_from_tasks=n, candidates=int(seeds[-1]), seconds_per_task=s / n, tasks_per_s=n / s,
                note="sample_and_check_tasks(backend='host'): a few tasks timed, the rate extrapolated from them")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tasks", type=int, default=4096)
    ap.add_argument("--limit-tasks", type=int, default=256)
    ap.add_argument("--host-tasks", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metalm_sampler.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_metalm_sampler.py measures on the GPU; none found")
    engine = Engine("cuda:0")
    out = dict(device=torch.cuda.get_device_name(0), clock="time.perf_counter around calls ending in a stream synchronise",
               max_len=1024)
    for name, shape, n, n_host in (("default", (32, 16, 32), a.tasks, a.host_tasks),
                                   ("limits", (256, 64, 128), a.limit_tasks, max(2, a.host_tasks // 8))):
        out[name] = dict(shape=list(shape), device_sampler=device_sampler_rate(engine, n, shape, a.repeats),
                         parent_device_backend=parent_device_rate(n, shape, a.repeats), host_backend=host_rate(n_host, shape))
        print(name, json.dumps({k: v.get("tasks_per_s") for k, v in out[name].items() if isinstance(v, dict)}), flush=True)
    engine.close()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({name: {k: v.get("tasks_per_s") for k, v in out[name].items() if isinstance(v, dict)}
                      for name in ("default", "limits")}))


if __name__ == "__main__":
    main()
