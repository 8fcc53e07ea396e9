"""MetaLangV2 on the device (csrc/metalang.hip, xenoverse_amd.metalang.MetaLangV2Batch), L = 4096 tokens per sequence.

Reports tokens/s (median of 3 timed calls after one warm-up, wall clock including the synchronise) of
  - generate, free-running  (a) 4,096 groups x B = 1 at the sampler's defaults (V 256, H 64, E 16, n 3), one task per group
                            (b) 16,384 groups x B = 1 at the generator CLI's defaults (V 64, H 16, E 16, n from 3-6)
                            (c) 1,024 groups x B = 16 of (b)'s size
                            and (a) at 256 ... 8,192 groups: where the device fills
  - log_prob                teacher forcing on (a)'s output
and, measured on the same box before the process touches the GPU, the host restatement (MetaLangV2Host, numpy) on 16
processes, one task per process and vectorised over B — the reference's style of use — at the sizes of (a), (b), (c).
Kernel statistics: a separate `rocprofv3 --kernel-trace --stats` run of `--quick --gpu-only`.

usage: python scripts/bench_metalang.py [--quick] [--gpu-only] [--out profiles/metalang_v2_bench.json]
"""
import argparse
import json
import multiprocessing as mp
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
L = 4096
PROCS = 16
DEFAULTS = dict(n_vocab=256, n_hidden=64, n_emb=16, n_gram=3)
CLI = dict(n_vocab=64, n_hidden=16, n_emb=16, n_gram=[3, 4, 5, 6])
CASES = {"a": (4096, 1, DEFAULTS), "b": (16384, 1, CLI), "c": (1024, 16, CLI)}
SWEEP = (256, 512, 1024, 2048, 4096, 8192)


def _host_job(args):
    idx, case, seconds = args
    from xenoverse_amd.metalang import MetaLangV2Host, TaskSamplerV2
    _, B, kw = CASES[case]
    host = MetaLangV2Host(TaskSamplerV2(seed=idx, **kw))
    rs = np.random.RandomState(idx)
    window = np.zeros((B, host.n), np.int64)
    tokens, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:      # forward()'s step, 64 at a time
        for _ in range(64):
            p = host.probabilities(window)
            nxt = (p.cumsum(1) > rs.random_sample(B)[:, None]).argmax(1)
            window[:, :-1] = window[:, 1:]
            window[:, -1] = nxt
        tokens += 64 * B
    return tokens / (time.perf_counter() - t0)


def cpu_lines(seconds):
    ctx = mp.get_context("fork")          # nothing in this process has touched the GPU yet
    res = {"cpu_seconds_each": seconds, "cpu_processes": PROCS, "os_cpu_count": os.cpu_count(),
           "host_note": "MetaLangV2Host.probabilities + cumsum / argmax per step, one task per process, vectorised over B"}
    for case in sorted(CASES):
        with ctx.Pool(PROCS) as pool:
            rates = pool.map(_host_job, [(i, case, seconds) for i in range(PROCS)], chunksize=1)
        res["host_16proc_%s_tokens_per_s" % case] = float(sum(rates))
        print("host, 16 processes, (%s): %.3e tokens/s" % (case, sum(rates)), flush=True)
    return res


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), ts


def gpu_lines(quick):
    import torch
    from xenoverse_amd.metalang import MetaLangV2Batch, TaskSamplerV2
    reps = 1 if quick else 3
    res = {"L": L, "device": torch.cuda.get_device_name(0)}
    errors = 0
    for case in sorted(CASES):
        G, B, kw = CASES[case]
        groups = SWEEP if case == "a" and not quick else (G,)
        tasks = [TaskSamplerV2(seed=10000 + k, **kw) for k in range(max(groups))]
        for g in groups:
            gen = MetaLangV2Batch(g, B, seed=1)
            gen.set_task(tasks[:g])
            med, ts = timed(lambda: gen.generate(L), reps)
            name = "generate_%s" % case if g == G else "generate_a_sweep_%d_groups" % g
            res[name + "_tokens_per_s"] = g * B * L / med
            res[name + "_seconds"] = ts
            if g == G:
                res[name + "_config"] = dict(groups=g, seqs_per_group=B, n_vocab=kw["n_vocab"], n_hidden=kw["n_hidden"],
                                             n_emb=kw["n_emb"], n_gram=kw["n_gram"])
                res[name + "_us_per_step_of_the_whole_batch"] = med / L * 1e6
            print("%s: %.3e tokens/s (%.1f ms per call)" % (name, g * B * L / med, med * 1e3), flush=True)
            if case == "a" and g == G:
                tokens = gen.generate(L)
                med, ts = timed(lambda: gen.log_prob(tokens), reps)
                res["log_prob_a_tokens_per_s"] = g * B * L / med
                res["log_prob_a_seconds"] = ts
                print("log_prob_a: %.3e tokens/s (%.1f ms per call)" % (g * B * L / med, med * 1e3), flush=True)
            errors |= gen.check_errors()
            gen.close()
    res["device_errors"] = int(errors)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--gpu-only", action="store_true")
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=6.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {}
    if not args.gpu_only:
        res.update(cpu_lines(args.cpu_seconds))
    if not args.cpu_only:
        res.update(gpu_lines(args.quick))
    for case in sorted(CASES):
        d, h = res.get("generate_%s_tokens_per_s" % case), res.get("host_16proc_%s_tokens_per_s" % case)
        if d and h:
            res["device_vs_host_16proc_%s" % case] = d / h
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
