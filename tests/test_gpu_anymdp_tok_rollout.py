"""Fused rollouts of the POMDP / multi-token POMDP tasks (AnyMDPVecEnv.rollout / rollout_teacher on a token env;
xv_anymdp_rollout_tokens, xv_anymdp_rollout_tokens_teacher): a rollout is T token steps under SAME_STEP bit for bit — against
a stepped twin and against the CPU oracle —, splitting T changes nothing, and the teacher acts as the reference's
AnyMDPSolverOpt does (tests/golden/teacher_anymdptok_ref.npz).  N = 200 envs: no multiple of 64 or 256."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import oracle
from xenoverse_amd import _lib
from xenoverse_amd.anymdp import AnyMDPVecEnv, build_obs_tables, build_tables, to_blocked
from util import GOLD, anymdp_env, anymdp_tasks16, close_f32, golden_files, load_anymdp_tok_golden

pytestmark = pytest.mark.gpu
FILES = golden_files("anymdptok_")
N, SEED, BASE = 200, 77, 1000
SHORT = (7, 13)      # max_steps of the tasks in turn: truncation restarts fall inside every rollout
XV_DEVERR_ACTION_RANGE = 1
KEYS = ("obs", "reward", "reward_gt", "terminated", "truncated", "final_obs")

# name -> (tasks, search): tasks "pomdp" / "mtpomdp" (the reference-sampled fixtures) or synthetic (n_obs, d_obs, d_act, S, A)
CASES = {
    "pomdp-fence": ("pomdp", "fence"),
    "mtpomdp-fence": ("mtpomdp", "fence"),
    "mtpomdp-bucket": ("mtpomdp", "bucket"),
    "syn15x1x1-bucket": ((15, 1, 1, 64, 8), "bucket"),
    "syn64x3x2-binary": ((64, 3, 2, 64, 8), "binary"),
    "syn22x2x3-bucket": ((22, 2, 3, 64, 8), "bucket"),
    "syn300x2x2-bucket": ((300, 2, 2, 64, 8), "bucket"),      # n_obs > 256: no observation lines, the per-lane kernel
    "syn40x2x2-S300-bucket": ((40, 2, 2, 300, 4), "bucket"),  # S > 256: the six-cut transition lines with 16-bit ids
}


def _np(t):
    return t.detach().cpu().numpy()


def golden_tasks(kind, da1=False):
    """the fixtures' tasks with short episodes; kind "pomdp": the one POMDP task twice (max_steps 7 and 13), "mtpomdp": the
    two multi-token tasks.  da1: one action token per step (`da` is a field of the task dict only; the tensors do not
    depend on it)"""
    paths = [p for p in FILES if ("mtpomdp" in p) == (kind == "mtpomdp")]
    if kind == "pomdp":
        paths = paths * 2
    tasks = []
    for p, ms in zip(paths, SHORT):
        t = dict(load_anymdp_tok_golden(p)[1], max_steps=float(ms))
        if da1 and "da" in t:
            t["da"] = 1
        tasks.append(t)
    return tasks, [os.path.basename(p)[:-4] for p in paths]


@functools.lru_cache(maxsize=None)
def tables(tasks_key, da1=False):
    """-> (what set_task takes, oracle tables, obs_cdf, d_obs, d_act, A, task_type)"""
    if isinstance(tasks_key, str):
        tasks, _ = golden_tasks(tasks_key, da1)
        tab = build_tables(tasks)
        obs_cdf, n_obs, d_obs, d_act = build_obs_tables(tasks, tab["S"])
        return tasks, tab, obs_cdf, d_obs, d_act, int(tab["A"]), tasks[0]["task_type"]
    n_obs, d_obs, d_act, S, A = tasks_key
    n_task = 3 if S > 256 else 6
    tab = oracle.anymdp_synth(seed=17, task_index_base=0, n_task=n_task, S=S, A=A, s0_max=3)
    tab["max_steps"] = np.array([SHORT[k % 2] for k in range(n_task)], np.int32)
    rng = np.random.RandomState(n_obs)
    w = rng.random_sample((n_task, d_obs, S, n_obs)) * (rng.random_sample((n_task, d_obs, S, n_obs)) < 0.5) + 1e-3
    obs_cdf = np.cumsum(w, -1)
    obs_cdf = np.ascontiguousarray(obs_cdf / obs_cdf[..., -1:])
    task_type = "MTPOMDP" if (d_obs > 1 or d_act > 1) else "POMDP"
    dev = dict(S=S, A=A, s0_max=tab["s0_max"], obs_cdf=obs_cdf, n_obs=n_obs, d_obs=d_obs, d_act=d_act, task_type=task_type)
    blocked = dict(tab, rows=to_blocked(tab["cdf"], tab["rs"]))
    for k in ("rows", "state_map", "term_mask", "s0_cdf", "s0_ids", "max_steps"):
        v = np.ascontiguousarray(blocked[k])
        dev[k] = v.view(np.int64) if v.dtype == np.uint64 else v
    return dev, tab, obs_cdf, d_obs, d_act, A, task_type


def env_task_of(tab):
    return (np.arange(N) % len(tab["max_steps"])).astype(np.int32)


def make_env(tasks_key, search, da1=False, seed=SEED):
    what, tab, _, d_obs, d_act, A, _ = tables(tasks_key, da1)
    env = AnyMDPVecEnv(N, autoreset_mode="same_step", seed=seed, env_id_base=BASE)
    env.set_task(what, env_task_index=env_task_of(tab))
    env.set_search("bucket", n_bucket=16) if search == "bucket" else env.set_search(search)
    if search == "bucket":
        lines = tab["S"] <= 512 and tables(tasks_key, da1)[2].shape[-1] <= 256
        assert env.token_kernel == ("cooperative" if lines else "per-lane")
    else:
        assert env.token_kernel == "per-lane"
    return env


def actions_for(case, T):
    _, _, _, _, d_act, A, _ = tables(CASES[case][0])
    return np.random.RandomState(len(case) + T).randint(0, A, (T, N, d_act)).astype(np.int32)


def rolled(out, d_obs):
    r = {k: _np(out[k]).copy() for k in KEYS}
    r["obs"], r["final_obs"] = r["obs"].reshape(-1, N, d_obs), r["final_obs"].reshape(-1, N, d_obs)
    return r


def state_of(env):
    s, st, nr = env.get_state()
    return dict(state=_np(s).copy(), steps=_np(st).copy(), need_reset=_np(nr).copy(), tick=int(env.engine.tick))


def step_rows(env, acts, d_obs, before=None):
    """len(acts) step() calls -> the rollout's arrays; before(ts): called ahead of step ts"""
    rows = []
    for ts in range(len(acts)):
        if before is not None:
            before(ts)
        a = acts[ts]
        o, r, te, tr, info = env.step(a if a.shape[-1] > 1 else a[:, 0])
        rows.append(dict(obs=_np(o).reshape(N, d_obs), reward=_np(r), reward_gt=_np(info["reward_gt"]),
                         terminated=_np(te).astype(np.uint8), truncated=_np(tr).astype(np.uint8),
                         final_obs=_np(info["final_obs"]).reshape(N, d_obs)))
    return {k: np.stack([row[k] for row in rows]) for k in KEYS}


@functools.lru_cache(maxsize=None)
def stepped(case):
    """the twin of `case` stepped 49 times with actions_for(case, 49): the first 48 steps' arrays, the state after them,
    and the 49th step's arrays"""
    key, search = CASES[case]
    d_obs = tables(key)[3]
    acts = actions_for(case, 49)
    env = make_env(key, search)
    tick0 = int(env.engine.tick)
    o0, _ = env.reset()
    rows = step_rows(env, acts[:48], d_obs)
    st = state_of(env)
    last = step_rows(env, acts[48:], d_obs)
    assert env.check_errors() == 0
    env.close()
    return dict(rows=rows, state=st, last=last, tick0=tick0, obs0=_np(o0).reshape(N, d_obs).copy())


def same(a, b, keys=KEYS):
    for k in keys:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("case", list(CASES))
def test_rollout_equals_stepping(case):
    key, search = CASES[case]
    _, _, _, d_obs, d_act, _, task_type = tables(key)
    ref = stepped(case)
    acts = actions_for(case, 49)[:48]
    env = make_env(key, search)
    env.reset()
    out = env.rollout(acts if d_act > 1 else acts[:, :, 0])
    shape = (48, N) if task_type == "POMDP" else (48, N, d_obs)
    assert tuple(out["obs"].shape) == shape and tuple(out["final_obs"].shape) == shape
    same(rolled(out, d_obs), ref["rows"])
    st = state_of(env)
    for k in ref["state"]:
        assert np.array_equal(st[k], ref["state"][k]), k
    assert st["tick"] == ref["tick0"] + 1 + 48      # the reset's tick and one per step
    done = (ref["rows"]["terminated"] | ref["rows"]["truncated"]).astype(bool)
    assert done.sum() > 50 and ref["rows"]["truncated"].any()
    assert (ref["rows"]["final_obs"][~done] == -1).all() and (ref["rows"]["final_obs"][done] >= 0).all()
    assert env.check_errors() == 0
    env.close()


@pytest.mark.parametrize("case", list(CASES))
def test_rollout_vs_oracle(case):
    key, search = CASES[case]
    _, tab, obs_cdf, d_obs, d_act, _, _ = tables(key)
    acts = actions_for(case, 49)[:48]
    env = make_env(key, search)
    ora = oracle.AnyMDPTokOracle(tab, env_task_of(tab), obs_cdf, d_act)
    tick = int(env.engine.tick)
    o0, _ = env.reset()
    assert np.array_equal(_np(o0).reshape(N, d_obs), ora.tok_reset(SEED, BASE, tick))
    tick0 = int(env.engine.tick)
    got = rolled(env.rollout(acts), d_obs)
    ended = 0
    for ts in range(48):
        o = ora.tok_step(SEED, BASE, tick0 + ts, acts[ts], 2)
        assert np.array_equal(got["obs"][ts], o[0]) and np.array_equal(got["final_obs"][ts], o[5]), ts
        assert close_f32(got["reward"][ts], o[1], 1e-5, 4e-6), ts
        assert np.array_equal(got["reward_gt"][ts], o[2]), ts
        assert np.array_equal(got["terminated"][ts], o[3]) and np.array_equal(got["truncated"][ts], o[4]), ts
        ended += int((o[3] | o[4]).sum())
    st = state_of(env)
    assert np.array_equal(st["state"], ora.state) and np.array_equal(st["steps"], ora.steps)
    assert ended > 50
    env.close()


@pytest.mark.parametrize("case", ["pomdp-fence", "mtpomdp-bucket", "syn64x3x2-binary", "syn22x2x3-bucket"])
def test_splitting_and_continuing(case):
    key, search = CASES[case]
    d_obs = tables(key)[3]
    ref = stepped(case)
    acts = actions_for(case, 49)
    # rollout(40) == rollout(17) then rollout(23)
    whole, parts = make_env(key, search), make_env(key, search)
    whole.reset(); parts.reset()
    a = rolled(whole.rollout(acts[:40]), d_obs)
    b1, b2 = rolled(parts.rollout(acts[:17]), d_obs), rolled(parts.rollout(acts[17:40]), d_obs)
    same(a, {k: np.concatenate([b1[k], b2[k]]) for k in KEYS})
    sa, sb = state_of(whole), state_of(parts)
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    same(a, {k: v[:40] for k, v in ref["rows"].items()})
    # T = 1 equals one step(): steps 40 .. 47 one at a time, then step() itself continues where the rollouts ended
    for ts in range(40, 48):
        one = rolled(whole.rollout(acts[ts:ts + 1]), d_obs)
        same(one, {k: v[ts:ts + 1] for k, v in ref["rows"].items()})
    st = state_of(whole)
    for k in st:
        assert np.array_equal(st[k], ref["state"][k]), k
    # the env's current observation is the last step's (a restarted env's: its restart's)
    assert np.array_equal(_np(whole._tobs), ref["rows"]["obs"][47])
    same(step_rows(whole, acts[48:], d_obs), ref["last"])
    assert whole.check_errors() == 0 and parts.check_errors() == 0
    whole.close(); parts.close()


def fixture_greedy(names):
    ref = np.load(os.path.join(GOLD, "teacher_anymdptok_ref.npz"))
    return np.stack([ref["greedy_" + n] for n in names]).astype(np.uint8)


@pytest.mark.parametrize("search", ["fence", "bucket"])
@pytest.mark.parametrize("kind", ["pomdp", "mtpomdp"])
def test_teacher_greedy(kind, search):
    """epsilon = 0: the action of every step is the reference's argmax_a Q[inner state before the step]; every other output
    equals a twin's that is stepped with those actions; greedy=None (solved on the device) gives the same rollout"""
    _, names = golden_tasks(kind, da1=True)
    what, tab, _, d_obs, d_act, A, _ = tables(kind, True)
    assert d_act == 1
    greedy = fixture_greedy(names)
    env_task = env_task_of(tab)
    T = 48
    env = make_env(kind, search, da1=True)
    env.reset()
    out = env.rollout_teacher(T, greedy=greedy)
    assert tuple(out["action"].shape) == (T, N) and out["action"].dtype == torch.int32
    acts = _np(out["action"]).copy()
    got = rolled(out, d_obs)
    twin = make_env(kind, search, da1=True)
    twin.reset()
    before = []
    rows = step_rows(twin, acts[:, :, None], d_obs, before=lambda ts: before.append(_np(twin.inner_state).copy()))
    before = np.stack(before)
    assert np.array_equal(acts, greedy[env_task[None, :], before].astype(np.int32))
    same(got, rows)
    sa, sb = state_of(env), state_of(twin)
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    assert ((rows["terminated"] | rows["truncated"]) != 0).sum() > 50
    solved = make_env(kind, search, da1=True)
    solved.reset()
    out2 = solved.rollout_teacher(T)
    assert np.array_equal(_np(out2["action"]), acts)
    same(rolled(out2, d_obs), got)
    for e in (env, twin, solved):
        assert e.check_errors() == 0
        e.close()


@pytest.mark.parametrize("search", ["fence", "bucket"])
def test_teacher_epsilon(search):
    """N = 200, T = 400.  epsilon = 1: every action in [0, A), each action's count within 5 binomial standard deviations of
    N T / A.  epsilon = 0.25: the share of steps whose action differs from greedy within 5 standard deviations of
    0.25 (A - 1) / A (the inner state ahead of every step is read between one-step rollouts: splitting changes nothing)"""
    _, names = golden_tasks("pomdp")
    _, tab, _, d_obs, _, A, _ = tables("pomdp")
    greedy = fixture_greedy(names)
    env_task = env_task_of(tab)
    T = 400
    env = make_env("pomdp", search)
    env.reset()
    acts = _np(env.rollout_teacher(T, greedy=greedy, epsilon=1.0)["action"])
    assert acts.min() >= 0 and acts.max() < A
    cnt = np.bincount(acts.reshape(-1), minlength=A)
    sd = np.sqrt(N * T * (1.0 / A) * (1.0 - 1.0 / A))
    print("epsilon = 1: counts", cnt, "expected", N * T / A, "sd", sd)
    assert (np.abs(cnt - N * T / A) <= 5.0 * sd).all()
    differs = 0
    for ts in range(T):
        s = _np(env.inner_state)
        a = _np(env.rollout_teacher(1, greedy=greedy, epsilon=0.25)["action"])[0]
        differs += int((a != greedy[env_task, s]).sum())
    p = 0.25 * (A - 1) / A
    share, sd = differs / float(N * T), np.sqrt(p * (1.0 - p) / (N * T))
    print("epsilon = 0.25: share", share, "expected", p, "sd", sd)
    assert abs(share - p) <= 5.0 * sd
    assert env.check_errors() == 0
    env.close()


@pytest.mark.parametrize("name", ["anymdptok_mtpomdp_16x4_seed0", "anymdptok_mtpomdp_16x4_seed6", "anymdptok_pomdp_16x4_seed5"])
def test_teacher_beats_random(name):
    """Mean reward_gt over 200 envs x 2,000 steps, the task as the fixture has it (its own max_steps; one action token per
    step): teacher > uniformly random actions (epsilon = 1).  The same comparison on the CPU with oracle.AnyMDPTokOracle
    (scripts/check_anymdp_tok_teacher_sanity.py: greedy[state] against uniform actions, 200 envs x 2,000 steps, standard
    errors from the per-env means) shows the gap at far more than 5 standard errors on all three tasks — mtpomdp seed0:
    0.4366 vs -0.1150 (437 s.e.), mtpomdp seed6: 0.2731 vs 0.0151 (229 s.e.), pomdp seed5: 0.7961 vs 0.1547 (611 s.e.) —
    so no task is left out."""
    path = [p for p in FILES if name in p][0]
    task = dict(load_anymdp_tok_golden(path)[1])
    if "da" in task:
        task["da"] = 1
    greedy = fixture_greedy([name])
    means = []
    for eps in (0.0, 1.0):
        env = AnyMDPVecEnv(N, autoreset_mode="same_step", seed=SEED, env_id_base=BASE)
        env.set_task(task)
        env.reset()
        out = env.rollout_teacher(2000, greedy=greedy, epsilon=eps)
        means.append(float(out["reward_gt"].double().mean()))
        assert env.check_errors() == 0
        env.close()
    print(name, "teacher", means[0], "random", means[1])
    assert means[0] > means[1]


def test_refusals_happen_before_any_launch():
    mt = make_env("mtpomdp", "fence")
    mt.reset()
    tick = int(mt.engine.tick)
    _, _, _, d_obs, d_act, A, _ = tables("mtpomdp")
    assert d_act == 2
    with pytest.raises(ValueError, match="one action token per step"):
        mt.rollout_teacher(8)
    good = np.zeros((4, N, d_act), np.int32)
    for bad in (good[:, :, 0], good[:, :N - 1], np.zeros((4, N, d_act + 1), np.int32), good[0], good[:0], good.reshape(-1)):
        with pytest.raises(ValueError):
            mt.rollout(bad)
    # the C entry points
    T = 4
    dev = mt.device
    g = torch.zeros((len(SHORT), mt.S), dtype=torch.uint8, device=dev)
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)      # noqa: E731
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)    # noqa: E731
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8, device=dev)       # noqa: E731
    outs = [i32(T, N, d_obs), f32(T, N), f32(T, N), u8(T, N), u8(T, N), i32(T, N, d_obs)]
    ptrs = [_lib.ptr(x) for x in outs]
    acts = i32(T, N, d_act)
    lib = mt.lib
    assert lib.xv_anymdp_rollout_tokens_teacher(mt._h, T, _lib.ptr(g), 0.0, _lib.ptr(i32(T, N)), *ptrs) == _lib.XV_ERR_UNSUPPORTED
    assert b"one action token per step" in lib.xv_last_error()
    assert lib.xv_anymdp_rollout_tokens(mt._h, 0, _lib.ptr(acts), *ptrs) == _lib.XV_ERR_INVALID
    assert lib.xv_anymdp_rollout_tokens(mt._h, T, None, *ptrs) == _lib.XV_ERR_INVALID
    assert lib.xv_anymdp_rollout_tokens(mt._h, T, _lib.ptr(acts), None, *ptrs[1:]) == _lib.XV_ERR_INVALID
    assert int(mt.engine.tick) == tick and mt.check_errors() == 0
    mt.close()

    one = make_env("pomdp", "fence")
    one.reset()
    tick = int(one.engine.tick)
    with pytest.raises(ValueError):
        one.rollout_teacher(0)
    g1 = torch.zeros((len(SHORT), one.S), dtype=torch.uint8, device=dev)
    outs1 = [i32(T, N, 1), f32(T, N), f32(T, N), u8(T, N), u8(T, N), i32(T, N, 1)]
    p1 = [_lib.ptr(x) for x in outs1]
    a1 = i32(T, N)
    for eps in (-0.01, 1.5, float("nan")):
        assert lib.xv_anymdp_rollout_tokens_teacher(one._h, T, _lib.ptr(g1), eps, _lib.ptr(a1), *p1) == _lib.XV_ERR_INVALID
    assert lib.xv_anymdp_rollout_tokens_teacher(one._h, 0, _lib.ptr(g1), 0.0, _lib.ptr(a1), *p1) == _lib.XV_ERR_INVALID
    assert lib.xv_anymdp_rollout_tokens_teacher(one._h, T, None, 0.0, _lib.ptr(a1), *p1) == _lib.XV_ERR_INVALID
    assert lib.xv_anymdp_rollout_tokens_teacher(one._h, T, _lib.ptr(g1), 0.0, None, *p1) == _lib.XV_ERR_INVALID
    assert int(one.engine.tick) == tick and one.check_errors() == 0
    one.close()

    mdp = anymdp_env(anymdp_tasks16(), N, seed=3)
    mdp.reset()
    tick = int(mdp.engine.tick)
    assert lib.xv_anymdp_rollout_tokens(mdp._h, T, _lib.ptr(a1), *p1) == _lib.XV_ERR_INVALID
    assert lib.xv_anymdp_rollout_tokens_teacher(mdp._h, T, _lib.ptr(g1), 0.0, _lib.ptr(a1), *p1) == _lib.XV_ERR_INVALID
    assert int(mdp.engine.tick) == tick
    out = mdp.rollout(np.zeros((T, N), np.int32))      # MDP envs: nothing changes
    assert tuple(out["obs"].shape) == (T, N) and int(mdp.engine.tick) == tick + T
    mdp.close()


@pytest.mark.parametrize("search", ["fence", "bucket"])
def test_action_out_of_range_is_flagged_and_clamped(search):
    _, _, _, d_obs, d_act, A, _ = tables("mtpomdp")
    acts = actions_for("mtpomdp-" + search, 8)
    bad = acts.copy()
    bad[2, 5, 1], bad[6, N - 1, 0] = A, -3
    clamped = np.clip(bad, 0, A - 1)
    res = []
    for a in (bad, clamped):
        env = make_env("mtpomdp", search)
        env.reset()
        res.append(rolled(env.rollout(a), d_obs))
        flags = env.check_errors()
        assert bool(flags & XV_DEVERR_ACTION_RANGE) == (a is bad)
        env.close()
    same(res[0], res[1])
