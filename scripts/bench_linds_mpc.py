"""Device MPC teacher of LinDS (csrc/linds_mpc.hip) at BASELINE config 3: 65,536 envs = 1,024 tasks x 64, ns = 32, na = 8,
no = 8 (16 distinct sampled tasks tiled to 1,024 task indices, as scripts/bench_families.py), K = 20 and K = 50.

Reports per K: ms per teacher step (one xv_linds_mpc_action over every env; median of 5, device events and wall clock),
teacher env-steps/s, mean / max ADMM iterations, the FLOPs the tiles computed (shapes x iterations: a tile of 16 envs runs
until its slowest env has converged) over kernel time against the 157-TF fp32 matrix peak, the table set-up time, the fused
roll-out per step, and a CPU baseline: the host LTISystemMPC.solve (exact optimum) per env-step over 16 processes.
Kernel statistics come from a separate `rocprofv3 --kernel-trace --stats` run of `--quick`.

usage: python scripts/bench_linds_mpc.py [--quick] [--out profiles/linds_mpc_bench.json]
"""
import argparse
import concurrent.futures as cf
import json
import multiprocessing as mp
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_TF = 157.3


def tasks_config3(n_task, distinct=16):
    from xenoverse_amd.linds import LinearDSSampler
    ts = []
    for k in range(distinct):
        t = LinearDSSampler(32, 8, 8, seed=k)
        t["max_steps"] = 500
        ts.append(t)
    return [ts[k % distinct] for k in range(n_task)]


_MPC = {}


def _cpu_job(args):
    """one env-step of the host teacher: solve() only; the LTISystemMPC of a task is built once per worker process"""
    key, task, K, x, ref = args
    from xenoverse_amd.linds.teacher import LTISystemMPC
    if (key, K) not in _MPC:
        _MPC[(key, K)] = LTISystemMPC(task, K=K)
    t = time.perf_counter()
    _MPC[(key, K)].solve(x, ref)
    return time.perf_counter() - t


def cpu_baseline(tasks, K, n_solve=64, procs=16):
    keys = ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS")
    for k in keys:
        os.environ[k] = "1"
    jobs = []
    for i in range(n_solve):
        t = tasks[i % len(tasks)]
        jobs.append((i % len(tasks), t, K, np.asarray(t["initial_states"][0]), np.tile(t["command"] * t["target_valid"], (K, 1))
                     if t["target_type"] == "static_target" else np.stack([t["command"](j) * t["target_valid"] for j in range(K)])))
    with cf.ProcessPoolExecutor(max_workers=procs, mp_context=mp.get_context("spawn")) as ex:
        list(ex.map(_cpu_job, jobs))                  # builds the workers' LTISystemMPC objects
        per = list(ex.map(_cpu_job, jobs))            # the same solves again, timed around solve() alone
    # `procs` processes each solving back to back (they ran concurrently, so contention is in the per-solve times)
    return {"solves": n_solve, "processes": procs, "s_per_solve_one_core": statistics.median(per),
            "env_steps_per_s": procs / statistics.mean(per), "timed": "solve() only, MPC built beforehand"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="K = 20 only, 2 repetitions, no CPU baseline (the profiler run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from xenoverse_amd.linds import LinDSVecEnv
    n_task, per = 1024, 64
    n = n_task * per
    tasks = tasks_config3(n_task)
    env = LinDSVecEnv(n, autoreset_mode="same_step", seed=1)
    env.set_task(tasks)
    env.reset(seed=1)
    a = torch.zeros((n, 8), device=env.device)
    for _ in range(7):
        env.step(a)
    res = {"workload": "linds config 3: 65,536 envs = 1,024 tasks x 64, ns=32 na=8 no=8 (pads 32/8/16)", "results": []}
    reps = 2 if args.quick else 5
    for K in ((20,) if args.quick else (20, 50)):
        t0 = time.perf_counter()
        _, info = env._mpc(K, 0.99)
        torch.cuda.synchronize()
        setup = time.perf_counter() - t0
        env.mpc_action(K=K)     # warm-up
        torch.cuda.synchronize()
        dev_ms, wall_ms = [], []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            e0.record()
            act, st = env.mpc_action(K=K, return_info=True)
            e1.record()
            torch.cuda.synchronize()
            wall_ms.append((time.perf_counter() - w0) * 1e3)
            dev_ms.append(e0.elapsed_time(e1))
        iters = st["iters"].cpu().numpy()
        status = st["status"].cpu().numpy()
        npad, nin = info["n_pad"], info["n_in"]
        tile_iters = iters.reshape(-1, 16).max(1)            # env order is tile-aligned here (64 envs per task)
        flops = 16 * (2.0 * npad * nin * len(tile_iters) + 2.0 * npad * npad * tile_iters.sum())
        ms = statistics.median(dev_ms)
        T = 8
        env.rollout_teacher(T, K=K)
        torch.cuda.synchronize()
        r0 = time.perf_counter()
        env.rollout_teacher(T, K=K)
        torch.cuda.synchronize()
        roll_ms = (time.perf_counter() - r0) * 1e3 / T
        row = {"K": K, "n_pad": npad, "n_in": nin, "ms_per_teacher_step_device": ms,
               "ms_per_teacher_step_wall": statistics.median(wall_ms), "teacher_env_steps_per_s": n / (ms * 1e-3),
               "iters_mean": float(iters.mean()), "iters_max": int(iters.max()), "tile_iters_mean": float(tile_iters.mean()),
               "converged": float(status.mean()), "flops": flops, "tflops": flops / (ms * 1e-3) / 1e12,
               "frac_of_fp32_matrix_peak": flops / (ms * 1e-3) / 1e12 / PEAK_TF, "table_setup_s": setup,
               "rollout_teacher_T8_ms_per_step_wall": roll_ms, "samples_ms_device": dev_ms}
        if not args.quick:
            row["cpu_baseline"] = cpu_baseline(tasks[:16], K)
            row["speedup_vs_cpu"] = row["teacher_env_steps_per_s"] / row["cpu_baseline"]["env_steps_per_s"]
        res["results"].append(row)
        print(json.dumps(row))
        env._drop_mpc()
    env.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
