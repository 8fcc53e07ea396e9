"""Device Q-learners of AnyMDP (csrc/anymdp_qlearn.hip, AnyMDPVecEnv.rollout_learner) at BASELINE config 2: 65,536 envs,
S = 64, A = 8, one synthetic task per env (the tasks bench.py generates, xv_anymdp_synth_tasks), T = 256 per call.

Reports env-steps/s (median of 3 timed calls after one warm-up, wall clock including the call's synchronisation) of
  - rollout_learner       [Q-learner policy -> step -> learner] per env-step, free-running draws
  - rollout_learner greedy  the same with argmax actions (no policy draw, no softmax)
  - rollout_teacher       the optimal teacher's fused rollout on the same tasks (greedy table solved on the device)
  - rollout               the fused open-loop step rollout alone (given actions): what the env step costs
and two CPU lines measured on the same box before the GPU is touched:
  - host restatement      xenoverse_amd.anymdp.qlearner.QLearnerHost (numpy, vectorised over 4,096 agents) per process,
                          16 processes: agent work only (policy + learn on synthetic transitions, no env)
  - reference style       one env object (oracle/py_ref_style.py) and one single-agent QLearnerHost per env, one step()
                          + policy() + learn() call each per env-step, 16 processes x 8 envs: the reference's train() loop
Kernel statistics: a separate `rocprofv3 --kernel-trace --stats` run of `--quick --gpu-only`; bytes per env-step of the
learner kernel: a separate `rocprofv3 --pmc FETCH_SIZE` / `WRITE_SIZE` run of the same.

usage: python scripts/bench_anymdp_qlearn.py [--quick] [--gpu-only] [--out profiles/anymdp_qlearn_bench.json]
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
N_ENV, S, A, T = 65536, 64, 8, 256
PROCS = 16


def _host_job(seconds):
    from xenoverse_amd.anymdp.qlearner import QLearnerHost
    n = 4096
    rng = np.random.RandomState(os.getpid() & 0xFFFF)
    ql = QLearnerHost(n, S, A)
    obs = rng.randint(0, S, n)
    steps, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        a = ql.policy(obs, rng.random_sample(n))
        ns = rng.randint(0, S, n)
        ql.learn(obs, a, ns, rng.standard_normal(n), rng.random_sample(n) < 0.05)
        obs = ns
        steps += n
    return steps / (time.perf_counter() - t0)


def _ref_style_job(args):
    idx, seconds = args
    import oracle
    from oracle.py_ref_style import RefStyleAnyMDPEnv, task_dict_from_tables
    from xenoverse_amd.anymdp.qlearner import QLearnerHost
    n_obj = 8
    tab = oracle.anymdp_synth(seed=7, task_index_base=idx * n_obj, n_task=n_obj, S=S, A=A, s0_max=4)
    envs, agents, obs = [], [], []
    for k in range(n_obj):
        e = RefStyleAnyMDPEnv()
        e.set_task(task_dict_from_tables(tab, k))
        e.max_steps = float(tab["max_steps"][k])
        obs.append(e.reset()[0])
        envs.append(e)
        agents.append(QLearnerHost(1, S, A))
    np.random.seed(idx)
    steps, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for k, (e, ag) in enumerate(zip(envs, agents)):
            a = int(ag.policy([obs[k]], [np.random.random_sample()])[0])
            ns, r, te, tr, _ = e.step(a)
            ag.learn([obs[k]], [a], [ns], [r], [te])
            obs[k] = e.reset()[0] if (te or tr) else ns
            steps += 1
    return steps / (time.perf_counter() - t0)


def cpu_lines(seconds):
    ctx = mp.get_context("fork")          # nothing in this process has touched the GPU yet
    with ctx.Pool(PROCS) as pool:
        host = pool.map(_host_job, [seconds] * PROCS, chunksize=1)
    with ctx.Pool(PROCS) as pool:
        ref = pool.map(_ref_style_job, [(i, seconds) for i in range(PROCS)], chunksize=1)
    return {"host_restatement_16proc_env_steps_per_s": float(sum(host)),
            "host_restatement_note": "QLearnerHost, 4,096 agents per process, policy + learn on synthetic transitions (no env)",
            "ref_style_16proc_env_steps_per_s": float(sum(ref)),
            "ref_style_note": "per-object loop: RefStyleAnyMDPEnv + one single-agent QLearnerHost per env, 8 envs per process",
            "cpu_seconds_each": seconds, "cpu_processes": PROCS, "os_cpu_count": os.cpu_count()}


def make_tables(env, torch, _lib, n_task, seed):
    from xenoverse_amd.anymdp import row_lines
    eng, d = env.engine, env.device
    t = dict(S=S, A=A, s0_max=4,
             rows=torch.empty((n_task, S, A, row_lines(S), 16), dtype=torch.float64, device=d),
             state_map=torch.empty((n_task, S), dtype=torch.int32, device=d),
             term_mask=torch.empty((n_task, (S + 63) // 64), dtype=torch.int64, device=d),
             s0_cdf=torch.empty((n_task, 4), dtype=torch.float64, device=d),
             s0_ids=torch.empty((n_task, 4), dtype=torch.int32, device=d),
             max_steps=torch.empty(n_task, dtype=torch.int32, device=d))
    _lib.check(eng.lib.xv_anymdp_synth_tasks(eng.handle, seed, 0, n_task, S, A, 4,
                                             *[_lib.ptr(t[k]) for k in ("rows", "state_map", "term_mask", "s0_cdf",
                                                                        "s0_ids", "max_steps")]))
    eng.sync()
    return t


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
    from xenoverse_amd import _lib
    from xenoverse_amd.anymdp import AnyMDPQLearner, AnyMDPVecEnv
    reps = 1 if quick else 3
    env = AnyMDPVecEnv(N_ENV, seed=1, autoreset_mode="same_step")
    env.set_task(make_tables(env, torch, _lib, N_ENV, seed=2), env_task_index=np.arange(N_ENV, dtype=np.int32))
    env.reset()
    ql = AnyMDPQLearner(env)
    res = {"n_env": N_ENV, "n_task": N_ENV, "S": S, "A": A, "T": T, "search": env.effective_search,
           "agent_state_bytes": N_ENV * (S * A * 12 + S * 4 + 4)}
    rows = [("rollout_learner", lambda: env.rollout_learner(ql, T)),
            ("rollout_learner_greedy", lambda: env.rollout_learner(ql, T, greedy=True)),
            ("rollout_teacher", lambda: env.rollout_teacher(T))]
    acts = torch.randint(0, A, (T, N_ENV), dtype=torch.int32, device=env.device)
    rows.append(("rollout_open_loop", lambda: env.rollout(acts)))
    for name, fn in rows:
        med, ts = timed(fn, reps)
        res[name + "_env_steps_per_s"] = N_ENV * T / med
        res[name + "_us_per_step"] = med / T * 1e6
        res[name + "_samples_s"] = ts
        print(name, "%.3e env-steps/s, %.2f us per vector step" % (N_ENV * T / med, med / T * 1e6), flush=True)
    res["device_errors"] = int(env.check_errors())
    ql.close()
    env.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--gpu-only", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=10.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {}
    if not args.gpu_only:
        res.update(cpu_lines(args.cpu_seconds))
        print(json.dumps(res), flush=True)
    res.update(gpu_lines(args.quick))
    if "ref_style_16proc_env_steps_per_s" in res:
        res["learner_vs_ref_style"] = res["rollout_learner_env_steps_per_s"] / res["ref_style_16proc_env_steps_per_s"]
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
