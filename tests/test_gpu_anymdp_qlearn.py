"""The device Q-learner (csrc/anymdp_qlearn.hip: AnyMDPQLearner, AnyMDPVecEnv.rollout_learner) against the reference's own
training loop (tests/golden/qlearn_anymdp_*.npz), against the host restatement (xenoverse_amd/anymdp/qlearner.py) and
against itself."""
import ctypes as C

import numpy as np
import pytest
import torch

from util import close_f32, golden_files, load_anymdp_golden, load_anymdp_tok_golden
from xenoverse_amd import _lib
from xenoverse_amd.anymdp import AnyMDPQLearner, AnyMDPVecEnv, QLearnerHost

pytestmark = pytest.mark.gpu
FILES = golden_files("qlearn_anymdp_")
MARGIN = 1e-4


def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def _fixture_task(g):
    return dict(ns=int(g["ns"]), na=int(g["na"]), max_steps=float(g["max_steps"]), state_mapping=g["state_mapping"],
                task_type="MDP", s_0=g["s_0"], s_0_prob=g["s_0_prob"], s_e=g["s_e"], transition=g["transition"],
                reward=g["reward"], reward_noise=g["reward_noise"])


def _tasks16():
    return [load_anymdp_golden(p)[1] for p in golden_files("anymdp_16x4")[:4]]


def _env(tasks, n, seed, mode="same_step"):
    env = AnyMDPVecEnv(n, seed=seed, autoreset_mode=mode)
    env.set_task(tasks)
    return env


@pytest.mark.parametrize("path", FILES, ids=lambda p: p.rsplit("/", 1)[-1])
def test_device_replays_reference_training_loop(path):
    """all draws injected: actions equal the reference's at least up to the first step whose recorded margin is below 1e-4
    (the fp32 reward is what limits this; the replay goes on past such steps for as long as the actions agree, and a
    disagreement is allowed only at one of them); Q within 1e-4 and the counts exact at every snapshot up to there"""
    g = dict(np.load(path))
    T = len(g["action"])
    low = np.nonzero(g["margin"] < MARGIN)[0]
    t_first_low = int(low[0]) if len(low) else T
    snap = {int(k): j for j, k in enumerate(g["snap_at"])}
    is_test = g["is_test"].astype(bool)
    cuts = sorted({0, T} | set(snap) | {t for t in range(1, T) if is_test[t] != is_test[t - 1]})
    env = _env(_fixture_task(g), 1, seed=0)
    o0 = env.reset_injected([float(g["init_u"])])
    assert int(_np(o0)[0]) == int(g["init_obs"])
    ql = AnyMDPQLearner(env, gamma=float(g["gamma"]), alpha=float(g["alpha"]), max_steps=int(g["learner_max_steps"]))
    ql.set_state(g["init_q"][None], g["init_sa"][None].astype(np.int32), g["init_s"][None].astype(np.int32))
    compared, n_snap = 0, 0
    for t0, t1 in zip(cuts[:-1], cuts[1:]):
        sl = slice(t0, t1)
        draws = dict(u_policy=g["u_policy"][sl, None], u=g["u"][sl, None], z=g["z"][sl, None].astype(np.float32),
                     u_reset=g["u_reset"][sl, None])
        out = {k: _np(v)[:, 0] for k, v in env.rollout_learner(ql, t1 - t0, greedy=bool(is_test[t0]), draws=draws).items()}
        bad = np.nonzero(out["action"] != g["action"][sl])[0]
        n_ok = int(bad[0]) if len(bad) else t1 - t0
        if len(bad):      # only where the reference's own choice was within 1e-4 of a cut (or of a tie)
            assert g["margin"][t0 + n_ok] < MARGIN, (t0 + n_ok, g["margin"][t0 + n_ok])
        ok = slice(t0, t0 + n_ok)
        assert np.array_equal(out["terminated"][:n_ok], g["terminated"][ok])
        assert np.array_equal(out["truncated"][:n_ok], g["truncated"][ok])
        done = (g["terminated"][ok] | g["truncated"][ok]).astype(bool)
        assert np.array_equal(np.where(done, out["final_obs"][:n_ok], out["obs"][:n_ok]), g["next_obs"][ok])
        assert close_f32(out["reward"][:n_ok], g["r"][ok])
        compared += n_ok
        if len(bad):
            break
        if t1 in snap:
            q, sa, sv = (_np(x)[0] for x in ql.get_state())
            j = snap[t1]
            assert np.abs(q - g["snap_q"][j]).max() <= 1e-4, (t1, np.abs(q - g["snap_q"][j]).max())
            assert np.array_equal(sa, g["snap_sa"][j]) and np.array_equal(sv, g["snap_s"][j]), t1
            n_snap += 1
    print("%s: %d of %d steps compared (first margin < 1e-4 at %d), %d snapshots" % (
        path.rsplit("/", 1)[-1], compared, T, t_first_low, n_snap))
    assert compared >= t_first_low
    assert env.check_errors() == 0
    ql.close()
    env.close()


@pytest.mark.parametrize("cfg", ["16x4", "64x8"])
def test_device_equals_host_restatement(cfg):
    """4,096 envs, T = 512, injected draws; the host is fed the device's own obs, fp32 rewards and flags: actions equal,
    Q and the counts bit-equal"""
    tasks = _tasks16() if cfg == "16x4" else [load_anymdp_golden(golden_files("anymdp_64x8")[0])[1]]
    n, T = 4096, 512
    env = _env(tasks, n, seed=5)
    env.reset()
    obs = _np(env.state).astype(np.int64)
    ql = AnyMDPQLearner(env)
    rng = np.random.RandomState(11)
    draws = dict(u_policy=rng.random_sample((T, n)), u=rng.random_sample((T, n)),
                 z=rng.standard_normal((T, n)).astype(np.float32), u_reset=rng.random_sample((T, n)))
    out = {k: _np(v) for k, v in env.rollout_learner(ql, T, draws=draws).items()}
    host = QLearnerHost(n, env.S, env.A)
    for t in range(T):
        a = host.policy(obs, draws["u_policy"][t])
        assert np.array_equal(a, out["action"][t]), (t, np.nonzero(a != out["action"][t])[0][:4])
        term = out["terminated"][t].astype(bool)
        done = term | out["truncated"][t].astype(bool)
        host.learn(obs, a, np.where(done, out["final_obs"][t], out["obs"][t]), out["reward"][t].astype(np.float64), term)
        obs = out["obs"][t].astype(np.int64)
    assert out["terminated"].sum() > 0 and (cfg != "16x4" or out["truncated"].sum() > 0)
    q, sa, sv = (_np(x) for x in ql.get_state())
    assert np.array_equal(q, host.q)
    assert np.array_equal(sa, host.sa_visits) and np.array_equal(sv, host.s_visits)
    assert env.check_errors() == 0
    ql.close()
    env.close()


def test_rollout_equals_stepping_its_actions():
    """a twin env with the same seed and tasks stepped through step() with the rollout's actions returns the same outputs"""
    n, T = 256, 96
    a_env = _env(_tasks16(), n, seed=9)
    a_env.reset()
    ql = AnyMDPQLearner(a_env)
    ro = {k: _np(v) for k, v in a_env.rollout_learner(ql, T).items()}
    b_env = _env(_tasks16(), n, seed=9)
    b_env.reset()
    for t in range(T):
        obs, r, term, trunc, info = b_env.step(ro["action"][t])
        assert np.array_equal(_np(obs), ro["obs"][t]), t
        assert np.array_equal(_np(r), ro["reward"][t]) and np.array_equal(_np(info["reward_gt"]), ro["reward_gt"][t])
        assert np.array_equal(_np(term).astype(np.uint8), ro["terminated"][t])
        assert np.array_equal(_np(trunc).astype(np.uint8), ro["truncated"][t])
        done = (ro["terminated"][t] | ro["truncated"][t]).astype(bool)
        assert np.array_equal(_np(info["final_obs"])[done], ro["final_obs"][t][done])
    assert len(np.unique(ro["action"])) == 4
    assert a_env.check_errors() == 0 and b_env.check_errors() == 0
    ql.close()
    a_env.close()
    b_env.close()


def test_splitting_T_changes_nothing():
    """two calls of T / 2 equal one call of T bit for bit (free-running draws), agent state included"""
    n, T = 512, 128
    res = []
    for parts in (1, 2):
        env = _env(_tasks16(), n, seed=21)
        env.reset()
        ql = AnyMDPQLearner(env)
        outs = [env.rollout_learner(ql, T // parts) for _ in range(parts)]
        res.append(({k: np.concatenate([_np(o[k]) for o in outs]) for k in outs[0]}, [_np(x) for x in ql.get_state()]))
        assert env.check_errors() == 0
        ql.close()
        env.close()
    (o1, s1), (o2, s2) = res
    for k in o1:
        assert np.array_equal(o1[k], o2[k]), k
    for x, y in zip(s1, s2):
        assert np.array_equal(x, y)


def test_learning_is_real():
    """greedy reward per step after 3,000 steps of learning: far above the random agent, most of the way to the optimal
    teacher.  Thresholds from the host restatement on the same tasks (mean gap closed 0.55-0.74 over 16 runs)"""
    n = 256
    env = _env(_tasks16(), n, seed=3)
    env.reset()
    ql = AnyMDPQLearner(env)
    env.rollout_learner(ql, 3000)
    greedy = float(env.rollout_learner(ql, 1000, greedy=True)["reward_gt"].mean())
    rnd = float(env.rollout_teacher(1000, epsilon=1.0)["reward_gt"].mean())
    opt = float(env.rollout_teacher(1000)["reward_gt"].mean())
    frac = (greedy - rnd) / (opt - rnd)
    print("greedy %.4f random %.4f optimal %.4f: gap closed %.3f" % (greedy, rnd, opt, frac))
    assert opt > rnd + 0.1
    assert frac >= 0.4
    assert env.check_errors() == 0
    ql.close()
    env.close()


def test_state_round_trip_and_masked_reset():
    n = 64
    env = _env(_tasks16(), n, seed=4)
    env.reset()
    ql = AnyMDPQLearner(env, gamma=0.9)
    q0, sa0, sv0 = (_np(x) for x in ql.get_state())
    assert np.all(q0 == 1.0 / (1.0 - 0.9)) and np.all(sa0 == 1) and np.all(sv0 == 1)
    assert q0.shape == (n, 16, 4) and sv0.shape == (n, 16)
    rng = np.random.RandomState(2)
    q, sa, sv = rng.randn(n, 16, 4), rng.randint(1, 10 ** 6, (n, 16, 4)).astype(np.int32), rng.randint(1, 99, (n, 16)).astype(np.int32)
    ql.set_state(q, sa, sv)
    assert all(np.array_equal(_np(x), y) for x, y in zip(ql.get_state(), (q, sa, sv)))
    assert np.array_equal(_np(ql.q), q) and np.array_equal(_np(ql.sa_visits), sa) and np.array_equal(_np(ql.s_visits), sv)
    env.rollout_learner(ql, 16)
    before = [_np(x) for x in ql.get_state()]
    mask = np.zeros(n, bool)
    mask[::3] = True
    ql.reset(mask)
    after = [_np(x) for x in ql.get_state()]
    for b, a in zip(before, after):
        assert np.array_equal(a[~mask], b[~mask])
    assert np.all(after[0][mask] == 1.0 / (1.0 - 0.9)) and np.all(after[1][mask] == 1) and np.all(after[2][mask] == 1)
    with pytest.raises(ValueError):
        ql.reset(np.zeros(n + 1, bool))
    with pytest.raises(ValueError):
        ql.set_state(q=np.zeros((n, 16, 5)))
    assert env.check_errors() == 0
    ql.close()
    env.close()


def test_refusals_before_any_launch():
    tasks = _tasks16()
    # POMDP: the reference asserts task_type == "MDP" (anymdp_solver_q.py:17); the C-ABI refuses as well
    _, ptask = load_anymdp_tok_golden(golden_files("anymdptok_pomdp")[0])
    penv = AnyMDPVecEnv(4, autoreset_mode="same_step")
    penv.set_task(ptask)
    with pytest.raises(AssertionError):
        AnyMDPQLearner(penv)
    h = C.c_void_p()
    assert penv.lib.xv_anymdp_qlearn_create(penv._h, 0.99, 0.5, 4000, C.byref(h)) == _lib.XV_ERR_UNSUPPORTED
    assert not h.value
    penv.close()
    # auto-reset modes other than SAME_STEP
    for mode in ("disabled", "next_step"):
        env = _env(tasks, 8, seed=1, mode=mode)
        env.reset()
        ql = AnyMDPQLearner(env)
        with pytest.raises(ValueError):
            env.rollout_learner(ql, 4)
        ql.close()
        env.close()
    env = _env(tasks, 8, seed=1)
    env.reset()
    ql = AnyMDPQLearner(env)
    tick = env.engine.tick
    # wrong shapes, a missing draw, T < 1, another env's learner
    good = dict(u_policy=np.zeros((4, 8)), u=np.zeros((4, 8)), z=np.zeros((4, 8), np.float32), u_reset=np.zeros((4, 8)))
    for k in good:
        bad = dict(good)
        bad[k] = np.zeros((4, 7))
        with pytest.raises(ValueError):
            env.rollout_learner(ql, 4, draws=bad)
        bad.pop(k)
        with pytest.raises(ValueError):
            env.rollout_learner(ql, 4, draws=bad)
    with pytest.raises(ValueError):
        env.rollout_learner(ql, 0)
    other = _env(tasks, 8, seed=1)
    other.reset()
    oql = AnyMDPQLearner(other)
    with pytest.raises(ValueError):
        env.rollout_learner(oql, 4)
    # sub-batches (split) are refused: learners live on the whole env
    subs = env.split(2)
    with pytest.raises(ValueError):
        AnyMDPQLearner(subs[0])
    with pytest.raises(ValueError):
        subs[0].rollout_learner(ql, 4)
    assert env.engine.tick == tick     # nothing was launched
    q, sa, sv = (_np(x) for x in ql.get_state())
    assert np.all(sa == 1) and np.all(sv == 1)
    # a learner of an env that was given new tasks is refused
    env._drop_views()
    env.set_task(tasks)
    env.reset()
    with pytest.raises(ValueError):
        env.rollout_learner(ql, 4)
    assert env.check_errors() == 0 and other.check_errors() == 0
    oql.close()
    ql.close()
    other.close()
    env.close()


def test_learner_does_not_outlive_its_env_tasks():
    """set_task (twice: a recycled handle address must not revive the learner) and close release the learner before the
    env's handle goes; every later use raises, a new learner works"""
    tasks = _tasks16()
    env = _env(tasks, 8, seed=2)
    env.reset()
    ql = AnyMDPQLearner(env)
    env.rollout_learner(ql, 4)
    for _ in range(2):
        env.set_task(tasks)
        env.reset()
    uses = (lambda: env.rollout_learner(ql, 4), ql.get_state, ql.reset, lambda: ql.q, lambda: ql.s_visits,
            lambda: ql.set_state(q=np.zeros((8, 16, 4))))
    for use in uses:
        with pytest.raises(ValueError, match="new tasks"):
            use()
    ql2 = AnyMDPQLearner(env)
    out = env.rollout_learner(ql2, 8)
    assert out["action"].shape == (8, 8)
    sv = _np(ql2.s_visits)
    assert sv.shape == (8, 16) and int(sv.sum()) == 8 * 16 + 8 * 8      # one visit per env-step on top of the ones
    assert np.array_equal(_np(ql2.sa_visits).sum(axis=(1, 2)), 64 + np.full(8, 8))
    assert env.check_errors() == 0
    env.close()
    for use in (lambda: ql2.get_state(), ql2.reset):
        with pytest.raises(ValueError, match="closed"):
            use()
    ql2.close()
