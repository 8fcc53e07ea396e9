"""What the on-device PID teacher of AnyHVAC costs, and what the batched gain search takes.  No pass mark.

(i)  rollout_teacher(T) against rollout(actions) of the same T and batch, in the same process, alternating: the same step
     kernel with and without the controller in front of every step.  The actions replayed are the teacher's own, from
     the same starting state, so both sides do the same thermal work.
(ii) HVACSolverGridSearchPID.search: 10 x 10 x 10 gain triples, 64 steps, on the `rot` room (6 coolers, 6 sensors) — one
     batch of 1,000 envs; the time includes building the private env and its tables.

(iii) with --action-mode discrete | diff: rollout(actions) of shape (i) under that action mode (the difference mode with
     integer bins and the action cost on) against the box-mode rollout of the same room, batch and T, alternating.

(iv) the host path of one call: 200 consecutive step() calls at 64 envs of `rot` with iter_per_step = 1 (the kernel is
     short, so the host side of the call is what the clock sees), in box mode and in the difference mode with integer bins.

Clock: a host clock around calls that end in a device synchronise.  Every timed shape is run once before it is timed;
each figure is the median of `--repeats` alternated samples, all samples are kept in the output.

usage: python scripts/bench_anyhvac_pid.py [--envs 1024] [--T 16] [--repeats 5] [--action-mode box]
                                           [--out profiles/anyhvac_pid_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from xenoverse_amd.anyhvac import HVACEnv, HVACSolverGridSearchPID, HVACVecEnv  # noqa: E402


def load_room(name):
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "pid_anyhvac_%s.npz" % name), allow_pickle=False))
    task = {k[5:]: (v if v.ndim else v[()]) for k, v in g.items() if k.startswith("task_")}
    return task, g["init_grid"]


def timed(fn, env):
    env.engine.sync()
    t0 = time.perf_counter()
    fn()
    env.engine.sync()
    return time.perf_counter() - t0


def controller_cost(room, n, T, repeats, iter_per_step, sec_per_iter):
    task, grid = load_room(room)
    env = HVACVecEnv(n, iter_per_step=iter_per_step, sec_per_iter=sec_per_iter, autoreset_mode="disabled")
    env.set_task([task], generate_task=True)
    env.set_pid("gt")
    grids = np.repeat(grid[None], n, axis=0)

    def start():
        env.reset_injected(grids)      # (also resets the controllers)
    start()
    actions = env.rollout_teacher(T)[4]["action"].clone()
    start()
    env.rollout(actions)      # warm-up of the second shape
    teacher, replay = [], []
    for _ in range(repeats):
        start()
        teacher.append(timed(lambda: env.rollout_teacher(T), env))
        start()
        replay.append(timed(lambda: env.rollout(actions), env))
    errors = env.check_errors()
    env.close()
    a, b = statistics.median(teacher), statistics.median(replay)
    return dict(room=room, coolers=len(task["cooler_loc"]), sensors=len(task["sensor_loc"]), envs=n, T=T,
                iter_per_step=iter_per_step, sec_per_iter=sec_per_iter, rollout_teacher_s=a, rollout_s=b,
                teacher_ms_per_step=a / T * 1e3, rollout_ms_per_step=b / T * 1e3, teacher_over_rollout=a / b,
                teacher_env_steps_per_s=n * T / a, samples_teacher_s=teacher, samples_rollout_s=replay, device_errors=errors)


def action_mode_cost(room, n, T, repeats, iter_per_step, sec_per_iter, mode):
    task, grid = load_room(room)
    grids = np.repeat(grid[None], n, axis=0)
    C = len(task["cooler_loc"])
    rng = np.random.RandomState(0)
    opts = dict(action_mode=mode)
    if mode == "diff":
        opts.update(discretize_rl_action_space=True, add_action_cost=True)
        mapped_actions = torch.from_numpy(rng.randint(0, 13, (T, n, C)).astype(np.int32)).cuda()
    else:
        mapped_actions = torch.from_numpy(rng.uniform(0, 1, (T, n, C)).astype(np.float32)).cuda()
    box_actions = torch.from_numpy(rng.uniform(0, 1, (T, n, C)).astype(np.float32)).cuda()
    envs = []
    for o in ({}, opts):
        env = HVACVecEnv(n, iter_per_step=iter_per_step, sec_per_iter=sec_per_iter, autoreset_mode="disabled", **o)
        env.set_task([task], generate_task=True)
        envs.append(env)
    box, mapped = envs
    samples = {"box": [], mode: []}
    for i in range(repeats + 1):      # (the first round warms both shapes up)
        for key, env, acts in (("box", box, box_actions), (mode, mapped, mapped_actions)):
            env.reset_injected(grids)
            t = timed(lambda: env.rollout(acts), env)
            if i:
                samples[key].append(t)
    errors = box.check_errors() | mapped.check_errors()
    box.close()
    mapped.close()
    a, b = statistics.median(samples["box"]), statistics.median(samples[mode])
    return dict(room=room, coolers=C, sensors=len(task["sensor_loc"]), envs=n, T=T, iter_per_step=iter_per_step,
                sec_per_iter=sec_per_iter, action_mode=mode, box_rollout_s=a, mapped_rollout_s=b, mapped_over_box=b / a,
                samples_box_s=samples["box"], samples_mapped_s=samples[mode], device_errors=errors)


def host_path(repeats, n=64, calls=200):
    task, grid = load_room("gt_rot")
    grids = np.repeat(grid[None], n, axis=0)
    C = len(task["cooler_loc"])
    rng = np.random.RandomState(0)
    out = dict(room="gt_rot", envs=n, calls=calls, iter_per_step=1, sec_per_iter=0.15)
    for mode, opts, acts in (("box", {}, torch.from_numpy(rng.uniform(0, 1, (n, C)).astype(np.float32)).cuda()),
                             ("diff", dict(action_mode="diff", discretize_rl_action_space=True),
                              torch.from_numpy(rng.randint(0, 13, (n, C)).astype(np.int32)).cuda())):
        env = HVACVecEnv(n, iter_per_step=1, sec_per_iter=0.15, autoreset_mode="disabled", **opts)
        env.set_task([task], generate_task=True)

        def block():
            for _ in range(calls):
                env.step(acts)
        samples = []
        for i in range(repeats + 1):      # (the first round warms the shape up)
            env.reset_injected(grids)
            t = timed(block, env)
            if i:
                samples.append(t)
        out["device_errors_" + mode] = env.check_errors()
        env.close()
        out[mode + "_us_per_step"] = statistics.median(samples) / calls * 1e6
        out["samples_%s_s" % mode] = samples
    return out


def search_time(repeats, max_steps=64, points=10):
    task, grid = load_room("gt_rot")
    env = HVACEnv()
    env.set_task(task, generate_task=True)
    solver = HVACSolverGridSearchPID(env, (1e-3, 5e-2, points), (1e-2, 1e-1, points), (1e-3, 2e-2, points))
    solver.search(max_steps, init_grid=grid, apply_best=False)      # warm-up
    samples = []
    for _ in range(repeats):
        samples.append(timed(lambda: solver.search(max_steps, init_grid=grid, apply_best=False), env.vec))
    best = {k: float(v) for k, v in solver.best_params.items()}
    iter_per_step, sec_per_iter = env.vec.iter_per_step, env.vec.sec_per_iter
    env.close()
    s = statistics.median(samples)
    n = points ** 3
    return dict(room="gt_rot", candidates=n, max_steps=max_steps, iter_per_step=iter_per_step, sec_per_iter=sec_per_iter, search_s=s,
                candidate_steps_per_s=n * max_steps / s, samples_s=samples, best_params=best)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--T", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--action-mode", default="box", choices=("box", "discrete", "diff"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "anyhvac_pid_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_anyhvac_pid.py measures on the GPU; none found")
    out = dict(device=torch.cuda.get_device_name(0), clock="time.perf_counter around calls ending in a stream synchronise",
               controller_cost=[controller_cost("gt_rot", a.envs, a.T, a.repeats, 200, 0.15),
                                controller_cost("gt_wide", max(a.envs // 4, 1), max(a.T // 4, 1), a.repeats, 200, 0.15)],
               search=search_time(a.repeats), host_path=host_path(a.repeats))
    if a.action_mode != "box":
        out["action_mode_cost"] = [action_mode_cost("gt_rot", a.envs, a.T, a.repeats, 200, 0.15, a.action_mode),
                                   action_mode_cost("gt_wide", max(a.envs // 4, 1), max(a.T // 4, 1), a.repeats, 200, 0.15,
                                                    a.action_mode)]
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("controller_cost", "search", "host_path", "action_mode_cost") if k in out}))


if __name__ == "__main__":
    main()
