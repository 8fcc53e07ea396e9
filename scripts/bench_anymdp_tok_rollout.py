"""Per-step time of the fused POMDP / multi-token rollout against the other ways of making the same steps, T = 256.

Configuration: the token configuration of the benchmark's families (scripts/bench_families.py: bench_anymdp_tok) — 65,536
envs over 1,024 shared synthetic tasks (BASELINE config 2b), S = 64, A = 8, n_obs = 64, d_obs = 2, d_act = 2, SAME_STEP.

Lines (us per vector step of 65,536 envs; median of --reps timed windows after a warm-up, each window by HIP events AND by
the host clock around launches that end in a synchronise):
  rollout, per-lane            xv_anymdp_rollout_tokens under search = fence (the per-lane kernel)
  rollout, cooperative         the same under search = bucket (bucket lines of transitions and observations)
  step_tokens_many, one stream / overlapped     T token steps issued from C, per-lane and cooperative kernels
  python step() loop           T calls of AnyMDPVecEnv.step (copy=False)

--tree DIR imports xenoverse_amd from DIR (a built checkout of another commit, e.g. the parent) and times only the lines that
commit has; --yardstick-tree DIR runs that as a child process of the same GPU visit and stores its lines under "yardstick".

usage: python scripts/bench_anymdp_tok_rollout.py [--out profiles/anymdp_tok_rollout.json] [--yardstick-tree DIR]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--tasks", type=int, default=1024)
    ap.add_argument("--tree", default=None)
    ap.add_argument("--yardstick-tree", default=None)
    ap.add_argument("--out", default=None)
    return ap.parse_args()


args = parse()
sys.path.insert(0, os.path.abspath(args.tree) if args.tree else ROOT)

import torch  # noqa: E402
from xenoverse_amd import _lib  # noqa: E402
from xenoverse_amd.anymdp import AnyMDPVecEnv, row_lines  # noqa: E402


def make_env(n, n_task, S=64, A=8, n_obs=64, d_obs=2, d_act=2):
    env = AnyMDPVecEnv(n, seed=1, autoreset_mode="same_step", copy=False)
    d = env.device
    tab = dict(S=S, A=A, s0_max=4, rows=torch.empty((n_task, S, A, row_lines(S), 16), dtype=torch.float64, device=d),
               state_map=torch.empty((n_task, S), dtype=torch.int32, device=d),
               term_mask=torch.empty((n_task, 1), dtype=torch.int64, device=d),
               s0_cdf=torch.empty((n_task, 4), dtype=torch.float64, device=d),
               s0_ids=torch.empty((n_task, 4), dtype=torch.int32, device=d),
               max_steps=torch.empty(n_task, dtype=torch.int32, device=d))
    _lib.check(env.lib.xv_anymdp_synth_tasks(env.engine.handle, 7, 0, n_task, S, A, 4, *[_lib.ptr(tab[k]) for k in
               ("rows", "state_map", "term_mask", "s0_cdf", "s0_ids", "max_steps")]))
    g = torch.Generator(device=d)
    g.manual_seed(5)
    w = torch.rand((n_task, d_obs, S, n_obs), dtype=torch.float64, device=d, generator=g) + 0.05
    obs_cdf = torch.cumsum(w, -1)
    obs_cdf = (obs_cdf / obs_cdf[..., -1:]).contiguous()
    obs_cdf[..., -1] = 1.0
    env.set_task(dict(tab, obs_cdf=obs_cdf, n_obs=n_obs, d_obs=d_obs, d_act=d_act, task_type="MTPOMDP"))
    env.reset()
    return env


def window(fn, steps):
    """one timed window of `steps` vector steps -> (us per step by HIP events, by the host clock)"""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    return e0.elapsed_time(e1) * 1e3 / steps, (t1 - t0) * 1e6 / steps


def measure(fn, steps, reps):
    import gc
    gc.collect()
    gc.disable()
    try:
        for _ in range(2):
            fn()
        w = [window(fn, steps) for _ in range(reps)]
    finally:
        gc.enable()
    ev, host = [x[0] for x in w], [x[1] for x in w]
    return {"us_per_step_events": statistics.median(ev), "us_per_step_host": statistics.median(host),
            "events_min_max": [min(ev), max(ev)], "windows": reps, "steps_per_window": steps}


def main():
    T, n = args.T, args.envs
    env = make_env(n, args.tasks)
    A, d_act = env.A, env._tok[1]
    g = torch.Generator(device=env.device)
    g.manual_seed(11)
    acts = torch.randint(0, A, (T, n, d_act), device=env.device, dtype=torch.int32, generator=g)
    lines = {}
    has_rollout = hasattr(env.lib, "xv_anymdp_rollout_tokens")
    P = 8
    ring = env.step_tokens_many(P, acts[:P])
    for search, kernel in (("fence", "per-lane"), ("bucket", "cooperative")):
        env.set_search("bucket", n_bucket=16) if search == "bucket" else env.set_search(search)
        assert env.token_kernel == kernel
        if has_rollout:
            out = env.rollout(acts)
            lines["rollout, %s" % kernel] = measure(lambda: env.rollout(acts, out=out), T, args.reps)
        lines["step_tokens_many, one stream, %s" % kernel] = measure(
            lambda: env.step_tokens_many(T, acts[:P], out=ring), T, args.reps)
    env.set_step_many_overlap(True)
    row = measure(lambda: env.step_tokens_many(T, acts[:P], out=ring), T, args.reps)
    row["taken"] = env.step_many_overlap_state == 1
    lines["step_tokens_many, overlapped, cooperative"] = row
    env.set_step_many_overlap(False)

    def loop():
        for ts in range(T):
            env.step(acts[ts])
    lines["python step() loop, cooperative"] = measure(loop, T, max(3, args.reps // 2))
    flags = env.check_errors()
    env.close()
    res = {"workload": "%d envs over %d shared synthetic tasks (config 2b), S=64 A=8 n_obs=64 d_obs=2 d_act=2, SAME_STEP, T=%d" % (
               n, args.tasks, T),
           "unit": "us per vector step", "tree": args.tree or ".", "lines": lines, "device_error_flags": flags,
           "device": torch.cuda.get_device_name(0)}
    if args.yardstick_tree:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", args.yardstick_tree, "--T", str(T), "--reps",
                            str(args.reps), "--envs", str(n), "--tasks", str(args.tasks)], capture_output=True, text=True, timeout=400)
        if r.returncode != 0:
            raise RuntimeError("yardstick run failed:\n%s\n%s" % (r.stdout[-2000:], r.stderr[-2000:]))
        res["yardstick"] = json.loads(r.stdout.strip().splitlines()[-1])["lines"]
    text = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(text)


if __name__ == "__main__":
    main()
