"""Device model-based learners of AnyMDP (csrc/anymdp_mbrl.hip, AnyMDPVecEnv.rollout_learner) at BASELINE config 2:
65,536 envs, S = 64, A = 8, one synthetic task per env (the tasks bench.py generates, xv_anymdp_synth_tasks), T = 256 per
call, c = 0.05 (the reference's train()).

Reports env-steps/s (median of 3 timed calls after one warm-up, wall clock including the call's synchronisation) and the
mean fraction of envs whose episode ends per step, of
  - rollout_learner          [MBRL policy -> step -> learn (+ estimator for the envs that ended)], free-running draws
  - rollout_learner greedy   the same with argmax actions
  - burst                    one step at which EVERY env ends (each env's step counter set to its task's max_steps - 1, so
                             the step truncates whatever does not terminate): the estimator runs for all 65,536 envs.
                             Its time is the call's minus that of a one-step call in which few envs end; its bytes are
                             what the estimator must move per ended env: est_r twice (mean, then squared deviations) and
                             vis_cnt once = 768 KiB at 64x8 if the second est_r pass came from cache, 1 MiB if this
                             kernel's three est_r passes (mean, deviations, sweep) all come from HBM
and two CPU lines measured before the GPU is touched:
  - host restatement         xenoverse_amd.anymdp.mbrl.MBRLHost (numpy, vectorised over 256 agents) per process, 16
                             processes: agent work only (policy + learn on synthetic transitions, 2 % of agents ending
                             per step)
  - per-object loop          one env object (oracle/py_ref_style.py) and one single-agent MBRLHost per env, one step()
                             + policy() + learn() call each per env-step, 16 processes x 8 envs.  MBRLHost's sweep is
                             numpy-vectorised over each (s, a) row (S A numpy calls), so this loop is FASTER than the
                             reference's own agent without numba, whose sweep interprets S A S iterations: the time of
                             one such interpreted sweep (update_value_matrix restated in plain Python, 64 x 8) is
                             reported beside it, and the device's speed-up over the reference is larger than
                             learner_vs_per_object_loop says
Kernel statistics: a separate `rocprofv3 --kernel-trace --stats` run of `--quick --gpu-only`; bytes per ended env of the
estimator kernel: a separate `rocprofv3 --pmc FETCH_SIZE WRITE_SIZE` run of `--burst-only`.

usage: python scripts/bench_anymdp_mbrl.py [--quick] [--gpu-only] [--burst-only] [--out profiles/anymdp_mbrl_bench.json]
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))
N_ENV, S, A, T = 65536, 64, 8, 256
PROCS = 16
C = 0.05
KIB = 1024


def _host_job(seconds):
    from xenoverse_amd.anymdp.mbrl import MBRLHost
    n = 256
    rng = np.random.RandomState(os.getpid() & 0xFFFF)
    h = MBRLHost(n, S, A, c=C)
    obs = rng.randint(0, S, n)
    steps, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        a = h.policy(obs, rng.random_sample((n, A)))
        ns = rng.randint(0, S, n)
        h.learn(obs, a, ns, rng.standard_normal(n), rng.random_sample(n) < 0.01, rng.random_sample(n) < 0.01)
        obs = ns
        steps += n
    return steps / (time.perf_counter() - t0)


def _ref_style_job(args):
    idx, seconds = args
    import oracle
    from oracle.py_ref_style import RefStyleAnyMDPEnv, task_dict_from_tables
    from xenoverse_amd.anymdp.mbrl import MBRLHost
    n_obj = 8
    tab = oracle.anymdp_synth(seed=7, task_index_base=idx * n_obj, n_task=n_obj, S=S, A=A, s0_max=4)
    envs, agents, obs = [], [], []
    for k in range(n_obj):
        e = RefStyleAnyMDPEnv()
        e.set_task(task_dict_from_tables(tab, k))
        e.max_steps = float(tab["max_steps"][k])
        obs.append(e.reset()[0])
        envs.append(e)
        agents.append(MBRLHost(1, S, A, c=C))
    np.random.seed(idx)
    steps, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for k, (e, ag) in enumerate(zip(envs, agents)):
            a = int(ag.policy([obs[k]], np.random.random_sample((1, A)))[0])
            ns, r, te, tr, _ = e.step(a)
            ag.learn([obs[k]], [a], [ns], [r], [te], [tr])
            obs[k] = e.reset()[0] if (te or tr) else ns
            steps += 1
    return steps / (time.perf_counter() - t0)


def _interpreted_sweep_seconds(reps=3):
    """one update_value_matrix(t, r, gamma, vm, max_iteration=1) sweep at 64 x 8, restated in plain Python loops the way
    the reference runs it without numba (solver.py:70-78)"""
    rng = np.random.RandomState(1)
    t = rng.random_sample((S, A, S)).tolist()
    r = rng.randn(S, A, S).tolist()
    vm0 = rng.randn(S, A).tolist()
    best = None
    for _ in range(reps):
        vm = [row[:] for row in vm0]
        t0 = time.perf_counter()
        for s in range(S):
            for a in range(A):
                exp_q = 0.0
                ts, rs = t[s][a], r[s][a]
                for sn in range(S):
                    exp_q += ts[sn] * (0.99 * max(vm[sn]) + rs[sn])
                vm[s][a] += 1.0 * (exp_q - vm[s][a])
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best


def cpu_lines(seconds):
    ctx = mp.get_context("fork")          # nothing in this process has touched the GPU yet
    with ctx.Pool(PROCS) as pool:
        host = pool.map(_host_job, [seconds] * PROCS, chunksize=1)
    with ctx.Pool(PROCS) as pool:
        ref = pool.map(_ref_style_job, [(i, seconds) for i in range(PROCS)], chunksize=1)
    return {"host_restatement_16proc_env_steps_per_s": float(sum(host)),
            "host_restatement_note": "MBRLHost, 256 agents per process, policy + learn on synthetic transitions, 2% ending "
                                     "per step (no env)",
            "per_object_loop_16proc_env_steps_per_s": float(sum(ref)),
            "per_object_loop_note": "RefStyleAnyMDPEnv + one single-agent MBRLHost per env, 8 envs per process; its sweep "
                                    "is numpy-vectorised per (s, a) row, so it is faster than the reference's own agent",
            "interpreted_sweep_64x8_s": _interpreted_sweep_seconds(),
            "interpreted_sweep_note": "one update_value_matrix sweep (max_iteration=1) in plain Python, as the reference "
                                      "runs it without numba: the cost of every episode end of its agent",
            "cpu_seconds_each": seconds, "cpu_processes": PROCS, "os_cpu_count": os.cpu_count()}


def timed(fn, reps, prep=None):
    import torch
    if prep:
        prep()
    fn()
    torch.cuda.synchronize()
    ts, outs = [], []
    for _ in range(reps):
        if prep:
            prep()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs.append(fn())
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), ts, outs


def gpu_lines(quick, burst_only):
    import torch
    from bench_anymdp_qlearn import make_tables
    from xenoverse_amd import _lib
    from xenoverse_amd.anymdp import AnyMDPMBRLLearner, AnyMDPVecEnv
    reps = 1 if quick else 3
    env = AnyMDPVecEnv(N_ENV, seed=1, autoreset_mode="same_step")
    tab = make_tables(env, torch, _lib, N_ENV, seed=2)
    env.set_task(tab, env_task_index=np.arange(N_ENV, dtype=np.int32))
    env.reset()
    ml = AnyMDPMBRLLearner(env, c=C)
    per_env = 8 * (2 * S * A * S + 3 * S * A)
    res = {"n_env": N_ENV, "n_task": N_ENV, "S": S, "A": A, "T": T, "c": C, "agent_state_bytes": N_ENV * per_env}
    if not burst_only:
        rows = [("rollout_learner", lambda: env.rollout_learner(ml, T)),
                ("rollout_learner_greedy", lambda: env.rollout_learner(ml, T, greedy=True))]
        for name, fn in rows:
            med, ts, outs = timed(fn, reps)
            ended = float(np.mean([(o["terminated"] | o["truncated"]).float().mean().item() for o in outs]))
            res[name + "_env_steps_per_s"] = N_ENV * T / med
            res[name + "_us_per_step"] = med / T * 1e6
            res[name + "_ended_fraction_per_step"] = ended
            res[name + "_samples_s"] = ts
            print(name, "%.3e env-steps/s, %.2f us per vector step, %.4f of envs end per step" % (
                N_ENV * T / med, med / T * 1e6, ended), flush=True)
    # a burst: every env's step counter at max_steps - 1, so the next step ends every episode
    max_steps = tab["max_steps"].to(torch.int32)

    def arm():
        env.set_state(steps=max_steps - 1)
    one = lambda: env.rollout_learner(ml, 1)       # noqa: E731
    med1, ts1, outs1 = timed(one, max(reps, 3))
    medb, tsb, outsb = timed(one, max(reps, 3), prep=arm)
    ended1 = float(np.mean([(o["terminated"] | o["truncated"]).sum().item() for o in outs1]))
    endedb = float(np.mean([(o["terminated"] | o["truncated"]).sum().item() for o in outsb]))
    est_s = (medb - med1) * (endedb / max(endedb - ended1, 1.0))
    peak = 8.0e12
    for tag, b in (("768KiB", 768 * KIB), ("1MiB", 1024 * KIB)):
        res["burst_bytes_" + tag] = endedb * b
        res["burst_fraction_of_8TBps_" + tag] = endedb * b / est_s / peak
    res.update({"one_step_call_s": med1, "one_step_ended_envs": ended1, "burst_call_s": medb, "burst_ended_envs": endedb,
                "burst_estimator_s": est_s, "burst_call_samples_s": tsb, "one_step_call_samples_s": ts1,
                "burst_target_s": 13e-3})
    print("burst: %d envs ended, call %.3f ms against %.3f ms for a step with %d ending: estimator %.3f ms, %.2f / %.2f of "
          "8 TB/s on 768 KiB / 1 MiB per env" % (endedb, medb * 1e3, med1 * 1e3, ended1, est_s * 1e3,
                                                 res["burst_fraction_of_8TBps_768KiB"],
                                                 res["burst_fraction_of_8TBps_1MiB"]), flush=True)
    res["device_errors"] = int(env.check_errors())
    ml.close()
    env.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--gpu-only", action="store_true")
    ap.add_argument("--burst-only", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=10.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {}
    if not (args.gpu_only or args.burst_only):
        res.update(cpu_lines(args.cpu_seconds))
        print(json.dumps(res), flush=True)
    res.update(gpu_lines(args.quick, args.burst_only))
    if "per_object_loop_16proc_env_steps_per_s" in res and "rollout_learner_env_steps_per_s" in res:
        res["learner_vs_per_object_loop"] = (res["rollout_learner_env_steps_per_s"] /
                                             res["per_object_loop_16proc_env_steps_per_s"])
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
