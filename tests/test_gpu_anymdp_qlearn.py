"""The device Q-learner (csrc/anymdp_qlearn.hip: AnyMDPQLearner, AnyMDPVecEnv.rollout_learner) against the reference's own
training loop (tests/golden/qlearn_anymdp_*.npz), against the host restatement (xenoverse_amd/anymdp/qlearner.py) and
against itself.  The tests that are the same for every learner are in test_gpu_anymdp_learners.py."""
import numpy as np
import pytest

from util import anymdp_env as _env, anymdp_fixture_task as _fixture_task, anymdp_tasks16 as _tasks16, to_np as _np
from util import close_f32, golden_files, load_anymdp_golden
from xenoverse_amd.anymdp import AnyMDPQLearner, QLearnerHost

pytestmark = pytest.mark.gpu
FILES = golden_files("qlearn_anymdp_")
MARGIN = 1e-4


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
