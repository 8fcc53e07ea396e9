"""The overlapped AnyMDP step (HAND kernels) makes its draws, the clamped action, the partial line index and the whole outcome of a
restart in front of the wait for the env records, and its tail behind the table line is selects, not branches — GPU tests.

Each case steps one small env twice from the same seed: with plain launches on one stream (graph off, overlap off — the path
tests/test_gpu_anymdp.py pins to the oracle) and overlapped, in calls of 64-96 steps on rings of 4 and 8 slots.  Every ring after
every call, the final get_state(), the tick and the device error word are compared bit for bit, and every overlapped call must
have taken the overlapped path (step_many_overlap_state == 1): a case that did not take it fails.

What the cases cover that tests/test_gpu_chains.py does not: autoreset_mode "disabled" (envs stepped from terminal states), restarts
at nearly every step (max_steps 1 and 2), out-of-range actions in all three modes, waves without a valid lane and ragged last
workgroups, and the layouts reached through the HAND kernels (two-block fence entries, the six-cut bucket packing, bucket lines
that cannot answer any draw)."""
import numpy as np
import pytest
import torch

import oracle
from util import close_f32
from xenoverse_amd.anymdp import AnyMDPVecEnv, to_blocked

pytestmark = pytest.mark.gpu

ACTION_RANGE, STEP_TERMINAL = 1, 2      # XV_DEVERR_* (xeno.h)
PLAN = (64, 96, 72)                     # whole cycles of both ring sizes: every step of every call is overlapped
RINGS = (4, 8)


def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def _dev_tables(tab, dev="cuda:0"):
    out = dict(S=tab["S"], A=tab["A"], s0_max=tab["s0_max"])
    tab = dict(tab, rows=to_blocked(tab["cdf"], tab["rs"]))
    for k in ("rows", "state_map", "term_mask", "s0_cdf", "s0_ids", "max_steps"):
        v = np.ascontiguousarray(tab[k])
        if v.dtype == np.uint64:
            v = v.view(np.int64)
        out[k] = torch.from_numpy(v).to(dev)
    return out


def _env_task(n, n_task):
    t = (np.arange(n) * n_task // n).astype(np.int32)
    np.random.RandomState(n).shuffle(t)      # the lanes of a wave mix tasks
    return t


def _run(tab, n, acts, search, mode, overlapped, seed=91):
    """-> [the ring after every call ..., (state, steps, need_reset, tick, error word)], (the tick of the reset, of the first step)"""
    env = AnyMDPVecEnv(n, seed=seed, autoreset_mode=mode, bucket_lines="off")
    env.set_task(_dev_tables(tab), env_task_index=_env_task(n, len(tab["max_steps"])))
    if search == "bucket":
        env.set_search("bucket", n_bucket=16)
    else:
        env.set_search(search)
    env.set_step_many_graph(overlapped)
    env.set_step_many_overlap(overlapped)
    t_reset = int(env.engine.tick)
    env.reset()
    t0 = int(env.engine.tick)
    a = torch.as_tensor(acts, device=env.device)
    rec, ring = [], None
    for n_steps in PLAN:
        ring = env.step_many(n_steps, a, out=ring)
        torch.cuda.synchronize()
        rec.append({k: _np(v).copy() for k, v in ring.items()})
        if overlapped:
            assert env.step_many_overlap_state == 1, (n_steps, env.step_many_overlap_state)
    s, st, nr = env.get_state()
    rec.append({"state": _np(s), "steps": _np(st), "need_reset": _np(nr), "tick": np.asarray(env.engine.tick),
                "err": np.asarray(env.check_errors())})
    env.close()
    return rec, (t_reset, t0)


def _both(tab, n, search, mode, acts_of=None):
    """both paths on both ring sizes, compared; -> [(plain record, actions, ticks)] per ring size"""
    out = []
    for P in RINGS:
        acts = np.random.RandomState(100 + P).randint(0, tab["A"], (P, n)).astype(np.int32)
        if acts_of is not None:
            acts = acts_of(acts)
        ref, ticks = _run(tab, n, acts, search, mode, False)
        got, ticks_got = _run(tab, n, acts, search, mode, True)
        assert len(ref) == len(got) and ticks == ticks_got
        for c, (x, y) in enumerate(zip(ref, got)):
            for k in x:
                assert np.array_equal(x[k], y[k]), (P, c, k)
        out.append((ref, acts, ticks))
    return out


def _synth(S=64, A=8, n_task=8, seed=12):
    return oracle.anymdp_synth(seed=seed, task_index_base=0, n_task=n_task, S=S, A=A, s0_max=4)


@pytest.mark.parametrize("max_steps", [1, 2])
@pytest.mark.parametrize("mode", ["same_step", "next_step"])
def test_restarts_at_nearly_every_step(mode, max_steps):
    """max_steps 1 and 2: the restart outcome made in front of the wait is applied at (nearly) every step — and only there"""
    tab = _synth()
    tab["max_steps"][:] = max_steps
    for ref, _, _ in _both(tab, 2000, "bucket", mode):
        assert int(ref[-1]["err"]) == 0
        for r in ref[:-1]:
            done = (r["terminated"] | r["truncated"]).astype(bool)
            # (a ring of four holds at least one done step of next_step's cycle of three at max_steps = 2: norm, norm, reset only)
            assert done.mean() > (0.2 if mode == "next_step" else 0.45)
            if mode == "same_step":
                assert np.array_equal(r["final_obs"] >= 0, done)


def test_disabled_mode_steps_from_terminal_states():
    """no auto-reset: envs that reach a terminal state stay there and raise XV_DEVERR_STEP_TERMINAL at every later step, on both
    paths alike; truncated envs go on stepping"""
    tab = _synth()
    for ref, _, _ in _both(tab, 2000, "bucket", "disabled"):
        assert int(ref[-1]["err"]) == STEP_TERMINAL
        assert ref[-2]["terminated"].any()


@pytest.mark.parametrize("mode", ["disabled", "next_step", "same_step"])
def test_out_of_range_actions(mode):
    """-1, A and A + 5 at a few envs (one of a wave's first lanes, its last lane, a ragged workgroup's last env): clamped, flagged,
    the same outputs on both paths"""
    tab = _synth()
    n, A = 2000, tab["A"]

    def bad(acts):
        acts[:, 3] = -1
        acts[1::2, 63] = A
        acts[:, 1999] = A + 5
        acts[0, 700] = -1
        return acts

    for ref, _, _ in _both(tab, n, "bucket", mode, bad):
        assert int(ref[-1]["err"]) == ACTION_RANGE | (STEP_TERMINAL if mode == "disabled" else 0)


def test_next_step_ignores_the_action_of_an_env_that_needs_a_reset():
    """max_steps = 1 under next_step: every env steps at even ticks and only returns its reset observation at odd ones, where the
    action is ignored (anymdp_env.py's auto-reset wrapper never hands it to the env) — out-of-range actions in the odd ring slots
    raise nothing; in an even slot they do"""
    tab = _synth()
    tab["max_steps"][:] = 1
    A = tab["A"]

    def odd(acts):
        acts[1::2, 5] = A
        acts[1::2, 64] = -1
        acts[3, 1999] = A + 5
        return acts

    def even(acts):
        acts[2, 5] = A
        return odd(acts)

    for ref, _, _ in _both(tab, 2000, "bucket", "next_step", odd):
        assert int(ref[-1]["err"]) == 0
    for ref, _, _ in _both(tab, 2000, "bucket", "next_step", even):
        assert int(ref[-1]["err"]) == ACTION_RANGE


@pytest.mark.parametrize("n_env", [1, 63, 65, 257, 2000])
def test_ragged_env_counts(n_env):
    """waves without a valid lane (n_env = 1, 63, 65, 257: one to three of a workgroup's four waves are empty) and ragged last
    workgroups"""
    tab = _synth()
    for ref, _, _ in _both(tab, n_env, "bucket", "same_step"):
        assert int(ref[-1]["err"]) == 0


def _uniform_rows(S=128):
    """every row uniform over all S = 128 next states: each of the 16 buckets holds eight live states, one more than a line's seven
    groups can name — no line answers its draw and the fence fall-back runs at every step, inside the overlapped kernel"""
    tab = _synth(S=S, A=4, n_task=4, seed=17)
    tab["cdf"][...] = np.arange(1, S + 1, dtype=np.float64) / S
    return tab


@pytest.mark.parametrize("layout", ["fence_S128", "bucket_S257", "bucket_uniform_S128"])
def test_layouts_reached_through_the_hand_kernels(layout):
    """fence search with two blocks per fence entry (S = 128), bucket search in the six-cut packing (S = 257), bucket lines that
    always fall back (uniform rows over 128 states, 16 buckets); the last one is also checked against the C oracle"""
    n = 600
    if layout == "fence_S128":
        tab, search = _synth(S=128, A=5, n_task=4, seed=5), "fence"
    elif layout == "bucket_S257":
        tab, search = _synth(S=257, A=3, n_task=3, seed=6), "bucket"
    else:
        tab, search = _uniform_rows(), "bucket"
    res = _both(tab, n, search, "same_step")
    for ref, _, _ in res:
        assert int(ref[-1]["err"]) == 0
    if layout != "bucket_uniform_S128":
        return
    # the plain path equals the overlapped one (above); the oracle replays it: the last P steps of every call are in the ring
    for (ref, acts, (t_reset, t0)), P in zip(res, RINGS):
        ora = oracle.AnyMDPOracle(tab, _env_task(n, len(tab["max_steps"])))
        ora.reset(91, 0, t_reset)
        k = 0
        for c, n_steps in enumerate(PLAN):
            for _ in range(n_steps):
                o_obs, o_r, o_rgt, o_term, o_trunc, o_fobs = ora.step(91, 0, t0 + k, acts[k % P], 2)
                if n_steps - (k - sum(PLAN[:c])) <= P:
                    r, j = ref[c], k % P
                    assert np.array_equal(r["obs"][j], o_obs) and np.array_equal(r["final_obs"][j], o_fobs)
                    assert np.array_equal(r["terminated"][j].astype(np.uint8), o_term)
                    assert np.array_equal(r["truncated"][j].astype(np.uint8), o_trunc)
                    assert np.array_equal(r["reward_gt"][j], o_rgt)
                    assert close_f32(r["reward"][j], o_r, rel=1e-5, abs_=2e-6)
                k += 1
        assert np.array_equal(ref[-1]["state"], ora.state) and np.array_equal(ref[-1]["steps"], ora.steps)
