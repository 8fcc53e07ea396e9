"""MetaLMV3 training streams: MetaLMV3VecEnv.stream (one launch, csrc/metalm.hip metalm_stream_kernel) against the same
streams assembled by the loop of policy() / step() calls with the splicing on the host — the path there is without it.

QAR streams of L = 2048 tokens, drawn temperatures, free-running draws, at the configurations (b) and (c) of
scripts/bench_metalm.py: 65,536 envs at the sampler's defaults (V 32, E 16, H 32) over 64 shared tasks, max_len 256, and
16,384 envs at (V 128, E 32, H 64) over 64 tasks, max_len 512.  Reported: stream tokens/s (envs x L over the wall clock,
the synchronise and, for the loop, the host splicing included), median of 3 after a warm-up, both paths from this process.
The loop runs rounds until the slowest env of the batch has its L tokens, pulls every round's ragged rows to the host and
splices them there with numpy.

usage: python scripts/bench_metalm_stream.py [--quick] [--out profiles/metalm_stream_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
L = 2048
CASES = {  # name: (envs, tasks, (V, E, H), max_len)
    "b": (65536, 64, (32, 16, 32), 256),
    "c": (16384, 64, (128, 32, 64), 512),
}
S, Q, A, R1 = 0, 1, 2, 3


def _put(dst, cur, tokens, length):
    """tokens[e, :length[e]] to dst[e, cur[e]:...] (cut at the row's end); cur advances"""
    n_env, width = tokens.shape
    cols = np.arange(width)[None, :]
    at = cur[:, None] + cols
    keep = (cols < length[:, None]) & (at < dst.shape[1])
    rows = np.broadcast_to(np.arange(n_env)[:, None], keep.shape)
    dst[rows[keep], at[keep]] = tokens[keep]
    cur += length


def _mark(dst, cur, token):
    ok = cur < dst.shape[1]
    dst[np.nonzero(ok)[0], cur[ok]] = token[ok] if np.ndim(token) else token
    cur += 1


def loop_stream(env, choices, rng):
    """generate_data_v3_single_task_qar for every env by policy() / step() and numpy splicing -> data, label, rounds"""
    n_env = env.num_envs
    data = np.zeros((n_env, L), np.int32)
    label = np.zeros((n_env, L), np.int32)
    dc = np.zeros(n_env, np.int64)
    lc = np.zeros(n_env, np.int64)
    obs, obs_len = (x.cpu().numpy() for x in env.reset())
    rounds = 0
    while (dc < L).any():
        T = choices[rng.randint(0, len(choices), n_env)]
        answer, answer_len = env.policy(T)
        nxt, r, _, _, info = env.step(answer, answer_len)
        a, n, lab, r = answer.cpu().numpy(), answer_len.cpu().numpy(), info["label"].cpu().numpy(), r.cpu().numpy()
        rt = (R1 + (r >= 0).astype(np.int32) + (r >= 0.5) + (r >= 1.0) + (r >= 2.0)).astype(np.int32)
        _mark(data, dc, Q); _put(data, dc, obs, obs_len); _mark(data, dc, S); _mark(data, dc, A)
        _put(data, dc, a, n); _mark(data, dc, S); _mark(data, dc, rt)
        _put(label, lc, obs, obs_len); _mark(label, lc, S); _mark(label, lc, A); _put(label, lc, lab, n + 1)
        _mark(label, lc, S); _mark(label, lc, rt); _mark(label, lc, Q)
        obs, obs_len = nxt[0].cpu().numpy(), nxt[1].cpu().numpy()
        rounds += 1
    return data, label, rounds


def fused_stream(env):
    env.reset()
    data, label, info = env.stream("QAR", L)
    return data.cpu().numpy(), label.cpu().numpy(), int(info["rounds"].max())


def _time(fn, reps):
    import torch
    fn()      # warm-up
    torch.cuda.synchronize()
    ts, last = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        last = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return ts, last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="an eighth of the envs, one repetition")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from xenoverse_amd.metalang import MetaLMV3VecEnv, TaskSamplerV3
    from xenoverse_amd.metalang.stream_host import default_T_choices
    res = {"device": torch.cuda.get_device_name(0), "datatype": "QAR", "L": L}
    reps = 1 if args.quick else 3
    for case in sorted(CASES):
        n_env, n_task, (V, E, H), max_len = CASES[case]
        if args.quick:
            n_env //= 8
        tasks = [TaskSamplerV3(V, E, H, seed=20000 + k) for k in range(n_task)]
        env = MetaLMV3VecEnv(n_env, max_len=max_len, seed=1)
        env.set_task(tasks, (np.arange(n_env) % n_task).astype(np.int32))
        rng = np.random.RandomState(1)
        t_fused, (d, lab, rounds_fused) = _time(lambda: fused_stream(env), reps)
        flags = int(env.check_errors())
        t_loop, (d2, lab2, rounds_loop) = _time(lambda: loop_stream(env, default_T_choices(), rng), reps)
        env.close()
        assert (d[:, 0] == Q).all() and (d2[:, 0] == Q).all() and d.shape == d2.shape == (n_env, L)
        mf, ml = statistics.median(t_fused), statistics.median(t_loop)
        res["stream_%s" % case] = dict(
            config=dict(envs=n_env, tasks=n_task, n_vocab=V, n_emb=E, n_hidden=H, max_len=max_len),
            fused_seconds=t_fused, loop_seconds=t_loop, fused_tokens_per_s=n_env * L / mf, loop_tokens_per_s=n_env * L / ml,
            fused_over_loop=ml / mf, longest_env_rounds_fused=rounds_fused, loop_rounds=rounds_loop, cut_flag=flags)
        print("(%s) %d envs: one launch %.3e tokens/s (%.1f ms), policy/step loop + host splice %.3e tokens/s (%.1f ms): %.2fx" % (
            case, n_env, n_env * L / mf, mf * 1e3, n_env * L / ml, ml * 1e3, ml / mf), flush=True)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
