"""MetaLangV1 on the device (csrc/metalang_v1.hip, xenoverse_amd.metalang.MetaLangV1Batch): 65,536 sequences of L = 4096 under
65,536 distinct tasks (TaskSamplerV1's defaults: 10 patterns of about 64 tokens, n_vocab 64, error_ratio 0.1), free-running
draws, one launch per call.  Reported: sequences/s, tokens/s and the achieved store bandwidth — 8 bytes per position for
features and labels, 9 with kinds — against the 8 TB/s HBM peak of an MI355X; and, measured on the same box before the process
touches the GPU, the host restatement (MetaLangV1Host over a RandomState, the reference's own way of drawing) on 16
processes.  Median of 5 calls after a warm-up; every call's seconds are kept.

usage: python scripts/bench_metalang_v1.py [--quick] [--gpu-only] [--out profiles/metalang_v1_bench.json]
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
N_SEQ = 65536
PROCS = 16
HBM_PEAK = 8.0e12


def _host_job(args):
    idx, seconds = args
    from xenoverse_amd.metalang import MetaLangV1Host, TaskSamplerV1
    host = MetaLangV1Host(TaskSamplerV1(seed=idx))
    rs = np.random.RandomState(idx)
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        host.run(L, batch=8, rng=rs)
        n += 8
    return n / (time.perf_counter() - t0)


def cpu_lines(seconds):
    ctx = mp.get_context("fork")          # nothing in this process has touched the GPU yet
    with ctx.Pool(PROCS) as pool:
        rates = pool.map(_host_job, [(i, seconds) for i in range(PROCS)], chunksize=1)
    print("host, %d processes: %.3e sequences/s" % (PROCS, sum(rates)), flush=True)
    return {"cpu_seconds_each": seconds, "cpu_processes": PROCS, "os_cpu_count": os.cpu_count(),
            "host_note": "MetaLangV1Host.run(L, batch=8) over a RandomState, one task per process",
            "host_16proc_sequences_per_s": float(sum(rates)), "host_16proc_tokens_per_s": float(sum(rates)) * L}


def gpu_lines(quick):
    import torch
    from xenoverse_amd.metalang import MetaLangV1Batch, TaskSamplerV1
    n_seq, reps = (4096, 2) if quick else (N_SEQ, 5)
    tasks = [TaskSamplerV1(seed=20000 + k) for k in range(n_seq)]
    gen = MetaLangV1Batch(n_seq, seed=1)
    gen.set_task(tasks)
    res = {"L": L, "n_seq": n_seq, "n_task": n_seq, "device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK}
    for name, with_kinds, bytes_per_pos in (("generate", False, 8), ("generate_with_kinds", True, 9)):
        out = gen.generate(L, return_kinds=with_kinds)      # warm-up: the allocator holds the outputs' blocks from here on
        del out
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = gen.generate(L, return_kinds=with_kinds)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
            del out
        med = statistics.median(ts)
        bw = n_seq * L * bytes_per_pos / med
        res.update({name + "_seconds": ts, name + "_sequences_per_s": n_seq / med, name + "_tokens_per_s": n_seq * L / med,
                    name + "_store_bytes_per_s": bw, name + "_share_of_hbm_peak": bw / HBM_PEAK})
        print("%s: %.3e sequences/s, %.2f ms per call, %.2f TB/s stored (%.1f %% of 8 TB/s)" % (
            name, n_seq / med, med * 1e3, bw / 1e12, 100 * bw / HBM_PEAK), flush=True)
    res["device_errors"] = int(gen.check_errors())
    gen.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--gpu-only", action="store_true")
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=5.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {}
    if not args.gpu_only:
        res.update(cpu_lines(args.cpu_seconds))
    if not args.cpu_only:
        res.update(gpu_lines(args.quick))
    d, h = res.get("generate_sequences_per_s"), res.get("host_16proc_sequences_per_s")
    if d and h:
        res["device_vs_host_16proc"] = d / h
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
