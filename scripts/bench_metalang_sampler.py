"""MetaLangV2 / MetaLangV1 tasks per second, made and set: the on-device samplers beside the host loop they replace.
No pass mark.

(i)  device: `sample_tasks_v2_device(n)` / `sample_tasks_v1_device(n)` followed by `set_task(tables)` on a handle with one
     group / sequence per task: the tables are made on the GPU and borrowed as they are.  `sample` is the sampler alone.
(ii) host: the loop over `TaskSamplerV2(seed=i)` / `TaskSamplerV1(seed=i)` on numpy's stream followed by `set_task(list)`,
     which stacks the tasks and uploads them: what a user paid before.  `sample` is the loop alone.  Above `--host-cap-v2` /
     `--host-cap-v1` tasks the host path is timed at the cap and the rate carried over: the entry says `extrapolated_from_tasks`
     (65,536 default-size V2 tasks are 12 GB on the host, and again as much stacked).

Sizes: V2's defaults (n_emb 16, n_hidden 64, n_vocab 256, n_gram 3: 24,000 fp64 normals a task) and V1's (n_vocab 64,
n_patterns 10, n_gram 64).  The first device call of each size is a warm-up and is not timed; a device figure is the median
of `--repeats` calls, a host figure of `--host-repeats`; all samples are kept.  Clock: time.perf_counter around calls
behind a device synchronise.

usage: python scripts/bench_metalang_sampler.py [--tasks 4096 65536] [--repeats 5] [--host-repeats 1]
                                                [--host-cap-v2 4096] [--host-cap-v1 65536] [--out profiles/metalang_sampler.json]
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
from xenoverse_amd.metalang import (MetaLangV1Batch, MetaLangV2Batch, TaskSamplerV1, TaskSamplerV2,  # noqa: E402
                                    sample_tasks_v1_device, sample_tasks_v2_device)


def _median(fn, repeats):
    samples = []
    for r in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(r)
        torch.cuda.synchronize()
        samples.append(time.perf_counter() - t0)
    return statistics.median(samples), samples


def _entry(n, seconds, samples, sample_seconds, sample_samples):
    return dict(tasks=n, seconds=seconds, tasks_per_s=n / seconds, samples_s=samples,
                sample=dict(seconds=sample_seconds, tasks_per_s=n / sample_seconds, samples_s=sample_samples))


def measure(version, n, engine, repeats, host_repeats, host_cap):
    if version == "v2":
        def handle(k):
            return MetaLangV2Batch(k, 1)

        def device(k, seed):
            return sample_tasks_v2_device(k, seed=seed, engine=engine)

        def host(k, seed):
            return [TaskSamplerV2(seed=seed + i) for i in range(k)]
    else:
        def handle(k):
            return MetaLangV1Batch(k)

        def device(k, seed):
            return sample_tasks_v1_device(k, seed=seed, engine=engine)

        def host(k, seed):
            return [TaskSamplerV1(seed=seed + i) for i in range(k)]
    out = {}
    gen = handle(n)
    try:
        gen.set_task(device(n, 0))      # warm-up
        s, samples = _median(lambda r: gen.set_task(device(n, 1 + r)), repeats)
        k, k_samples = _median(lambda r: device(n, 1 + r), repeats)
        out["device"] = _entry(n, s, samples, k, k_samples)
    finally:
        gen.close()
    n_host = min(n, host_cap)
    gen = handle(n_host)
    try:
        s, samples = _median(lambda r: gen.set_task(host(n_host, 1000 * r)), host_repeats)
        k, k_samples = _median(lambda r: host(n_host, 1000 * r), host_repeats)
        out["host"] = _entry(n_host, s, samples, k, k_samples)
        if n_host != n:
            out["host"]["extrapolated_from_tasks"] = n_host
    finally:
        gen.close()
    out["speedup"] = out["device"]["tasks_per_s"] / out["host"]["tasks_per_s"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tasks", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=1)
    ap.add_argument("--host-cap-v2", type=int, default=4096)
    ap.add_argument("--host-cap-v1", type=int, default=65536)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metalang_sampler.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_metalang_sampler.py measures on the GPU; none found")
    engine = Engine("cuda:0")
    out = dict(device=torch.cuda.get_device_name(0), clock="time.perf_counter around calls behind a device synchronise",
               sizes=dict(v2=dict(n_emb=16, n_hidden=64, n_vocab=256, n_gram=3), v1=dict(n_vocab=64, n_patterns=10, n_gram=64)))
    for version, cap in (("v2", a.host_cap_v2), ("v1", a.host_cap_v1)):
        out[version] = {}
        for n in a.tasks:
            r = out[version][str(n)] = measure(version, n, engine, a.repeats, a.host_repeats, cap)
            print(version, n, json.dumps({k: r[k]["tasks_per_s"] for k in ("device", "host")}), flush=True)
    engine.close()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
