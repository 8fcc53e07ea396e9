"""MazeWorld teacher data collection: the Python loop (`mazeworld.teacher_rollout`, unchanged: the baseline) against the
fused `MazeWorldVecEnv.rollout_teacher`, with frames (`frames=1`) and without (`frames=None`), both teachers, episodes
resampled on the device or not.

Workloads: 15x15 mazes at 64x64 frames, max_steps 200, Discrete16 — 16,384 envs (the `bench_families` batch) and 1,024 envs.
  shared   256 (16) host-sampled tasks x 64 envs, episodes not resampled: the bench_families tasks
  own      one device-sampled task per env (`sample_tasks_device`), episodes not resampled / resampled (start + commands)
Timing: T = 128 steps after 32 untimed ones (the batch is past the reset transient), median of 5 repetitions, each timed
by device events on the engine's stream AND by a host clock around the call that ends in a device synchronise; both are
reported per step.  Every repetition continues the trajectory of the one before (agents keep their memories).

usage: python scripts/bench_maze_rollout.py [--quick] [--out profiles/maze_rollout.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="256 envs, T = 16, 2 repetitions (a rehearsal of every row)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is nothing to time without one"
    from xenoverse_amd import build as xb
    from xenoverse_amd.mazeworld import (MazeTaskSampler, MazeWorldVecEnv, OracleAgent, SmartSLAMAgent, make_texture_library,
                                         sample_tasks_device, teacher_rollout)
    T, warm, reps = (16, 4, 2) if args.quick else (128, 32, 5)
    sizes = (256,) if args.quick else (16384, 1024)
    tex = make_texture_library(8, 4, 4, seed=0)
    res = {"device": torch.cuda.get_device_name(0), "T": T, "untimed_steps": warm, "repetitions": reps,
           "frames": "64x64", "max_steps": 200, "kernel_sources": xb.source_hash(["maze_rollout.hip", "maze.hip",
                                                                                  "maze_agent.hip", "maze_sampler.hip"]),
           "rows": []}
    shared_tasks, own_tables = {}, {}      # (set_task takes device tables as they are; resampling works on private copies)

    def make(n, tasks_kind, resample):
        env = MazeWorldVecEnv(n, resolution=(64, 64), textures=tex, autoreset_mode="same_step", max_steps=200,
                              action_space_type="Discrete16", seed=1)
        if tasks_kind == "shared":
            n_task = n // 64
            if n_task not in shared_tasks:
                shared_tasks[n_task] = [MazeTaskSampler(n_range=(15, 16), seed=k, n_wall_textures=8, n_ground_textures=4,
                                                        n_ceiling_textures=4) for k in range(n_task)]
            env.set_task(shared_tasks[n_task])
        else:
            if n not in own_tables:
                own_tables[n] = sample_tasks_device(n, seed=7, engine=env.engine, n_range=(15, 16), n_wall_textures=8,
                                                    n_ground_textures=4, n_ceiling_textures=4)
            env.set_task(own_tables[n])
        if resample:
            env.set_episode_resample(seed=3)
        env.reset()
        return env

    def timed(fn):
        ev, wall = [], []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3 / T)
            ev.append(a.elapsed_time(b) / T)
        return {"event_ms_per_step": statistics.median(ev), "wall_ms_per_step": statistics.median(wall),
                "event_ms_per_step_all": ev, "wall_ms_per_step_all": wall}

    for n in sizes:
        for tasks_kind, resample in (("shared", False), ("own", False), ("own", True)):
            for kind, cls in (("SmartSLAMAgent", SmartSLAMAgent), ("OracleAgent", OracleAgent)):
                for path in ("teacher_rollout loop, frames stacked", "teacher_rollout loop", "rollout_teacher frames=1",
                             "rollout_teacher frames=None"):
                    env = make(n, tasks_kind, resample)
                    agent = cls(maze_env=env)
                    if path.startswith("teacher_rollout"):
                        stacked = path.endswith("stacked")
                        teacher_rollout(env, agent, warm, frames=stacked)
                        row = timed(lambda: teacher_rollout(env, agent, T, frames=stacked))
                    else:
                        fr = 1 if path.endswith("=1") else None
                        env.rollout_teacher(agent, warm, frames=fr)
                        keep = {}      # the second call on writes into the tensors of the first: no allocation is timed twice
                        row = timed(lambda: keep.update(env.rollout_teacher(agent, T, frames=fr, out=keep or None)))
                        del keep
                    row = dict({"envs": n, "tasks": tasks_kind, "episodes_resampled": resample, "agent": kind, "path": path},
                               **row)
                    row["env_steps_per_s_event"] = n / (row["event_ms_per_step"] * 1e-3)
                    assert env.check_errors() == 0
                    print(json.dumps({k: v for k, v in row.items() if not k.endswith("_all")}), flush=True)
                    res["rows"].append(row)
                    agent.close(); env.close()
                    del env, agent
                    torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
