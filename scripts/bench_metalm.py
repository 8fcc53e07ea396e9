"""MetaLMV3 on the device (csrc/metalm.hip, xenoverse_amd.metalang.MetaLMV3VecEnv).

One ENV-STEP is what the reference's loop does per step: action = policy(T = 1), then step(action) — on the device two
launches (policy: one pass per env; step: the label, greedy and rnd passes and the next query of every env, and the reward).
Reports env-steps/s and tokens/s over all five passes (every pass counts its stop step), free-running draws, median of 3
timed env-steps after one warm-up, wall clock including the synchronise, of
  (a) 65,536 envs at the sampler's defaults (V 32, E 16, H 32), one task per env, max_len 256
  (b) the same over 64 shared tasks
  (c) 16,384 envs at (V 128, E 32, H 64) over 64 tasks, max_len 512
and (b) at 1,024 ... 32,768 envs: where the device fills.  Passes cut at max_len are counted (`cut_flag`).
The host line, measured on the same box before the process touches the GPU: RandomLMHost (numpy) doing the same env-step on
16 processes, one task per process, at the sizes of (a) and (c).
Kernel statistics: a separate `rocprofv3 --kernel-trace --stats` run of `--quick --gpu-only`.

usage: python scripts/bench_metalm.py [--quick] [--gpu-only] [--out profiles/metalm_v3_bench.json]
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
PROCS = 16
CASES = {  # name: (envs, tasks (None: one per env), (V, E, H), max_len)
    "a": (65536, None, (32, 16, 32), 256),
    "b": (65536, 64, (32, 16, 32), 256),
    "c": (16384, 64, (128, 32, 64), 512),
}
SWEEP = (1024, 2048, 4096, 8192, 16384, 32768)


def _host_job(args):
    idx, case, seconds = args
    from xenoverse_amd.metalang import TaskSamplerV3
    V, E, H = CASES[case][2]
    lm = TaskSamplerV3(V, E, H, seed=idx)["lm"]
    lm.generate_query()
    steps = tokens = 0
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        ans, _ = lm.generate_answer_softmax(T=1.0)
        lm.label_answer(ans)
        g, _ = lm.generate_answer_greedy()
        lo, _ = lm.generate_answer_low()
        q = lm.generate_query()
        steps += 1
        tokens += 2 * (len(ans) + 1) + len(g) + len(lo) + len(q) + 3
    dt = time.perf_counter() - t0
    return steps / dt, tokens / dt


def cpu_lines(seconds):
    ctx = mp.get_context("fork")          # nothing in this process has touched the GPU yet
    res = {"cpu_seconds_each": seconds, "cpu_processes": PROCS, "os_cpu_count": os.cpu_count(),
           "host_note": "RandomLMHost: policy, label, greedy, rnd, query per env-step; one task per process"}
    for case in ("a", "c"):
        with ctx.Pool(PROCS) as pool:
            rates = pool.map(_host_job, [(i, case, seconds) for i in range(PROCS)], chunksize=1)
        res["host_16proc_%s_env_steps_per_s" % case] = float(sum(r[0] for r in rates))
        res["host_16proc_%s_tokens_per_s" % case] = float(sum(r[1] for r in rates))
        print("host, 16 processes, (%s): %.3e env-steps/s, %.3e tokens/s" % (
            case, res["host_16proc_%s_env_steps_per_s" % case], res["host_16proc_%s_tokens_per_s" % case]), flush=True)
    return res


def env_step(env):
    """-> tokens of the five passes"""
    answer, answer_len = env.policy(1.0)
    obs, r, term, trunc, info = env.step(answer, answer_len)
    return 2 * (answer_len + 1).sum() + (info["greedy_len"] + 1).sum() + (info["low_len"] + 1).sum() + (obs[1] + 1).sum()


def gpu_lines(quick):
    import torch
    from xenoverse_amd.metalang import MetaLMV3VecEnv, TaskSamplerV3
    reps = 1 if quick else 3
    res = {"device": torch.cuda.get_device_name(0)}
    for case in sorted(CASES):
        if quick and case == "a":      # 65,536 task tables take a minute to make on the host
            continue
        n_env, n_task, (V, E, H), max_len = CASES[case]
        sizes = (n_env,) if quick or case != "b" else SWEEP + (n_env,)
        tasks = [TaskSamplerV3(V, E, H, seed=20000 + k) for k in range(n_task or n_env)]
        for n in sizes:
            env = MetaLMV3VecEnv(n, max_len=max_len, seed=1)
            env.set_task(tasks, (np.arange(n) % len(tasks)).astype(np.int32))
            env.reset()
            env_step(env)
            torch.cuda.synchronize()
            ts, toks = [], []
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                k = env_step(env)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
                toks.append(int(k))
            med = statistics.median(ts)
            name = "step_%s" % case if n == n_env else "step_b_sweep_%d_envs" % n
            res[name + "_env_steps_per_s"] = n / med
            res[name + "_tokens_per_s"] = statistics.median(toks) / med
            res[name + "_seconds"] = ts
            res[name + "_cut_flag"] = int(env.check_errors())
            if n == n_env:
                res[name + "_config"] = dict(envs=n, tasks=len(tasks), n_vocab=V, n_emb=E, n_hidden=H, max_len=max_len,
                                             tokens_per_env_step=statistics.median(toks) / n)
            print("%s: %.3e env-steps/s, %.3e tokens/s (%.1f ms per env-step of the batch)" % (
                name, n / med, statistics.median(toks) / med, med * 1e3), flush=True)
            env.close()
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
    for case, host in (("a", "a"), ("b", "a"), ("c", "c")):
        d, h = res.get("step_%s_env_steps_per_s" % case), res.get("host_16proc_%s_env_steps_per_s" % host)
        if d and h:
            res["device_vs_host_16proc_%s" % case] = d / h
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
