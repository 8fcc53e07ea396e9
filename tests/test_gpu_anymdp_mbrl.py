"""The device model-based learner (csrc/anymdp_mbrl.hip: AnyMDPMBRLLearner, AnyMDPVecEnv.rollout_learner) against the
reference's own training loop (tests/golden/mbrl_anymdp_*.npz), against the host restatement (xenoverse_amd/anymdp/mbrl.py)
and against itself.  The tests that are the same for every learner are in test_gpu_anymdp_learners.py."""
import os

import numpy as np
import pytest

from util import anymdp_env as _env, anymdp_fixture_task as _fixture_task, anymdp_tasks16 as _tasks16, to_np as _np
from util import anymdp_random_task as _random_task
from util import close_f32, golden_files, load_anymdp_golden
from xenoverse_amd.anymdp import AnyMDPMBRLLearner, MBRLHost

pytestmark = pytest.mark.gpu
FILES = golden_files("mbrl_anymdp_")
MARGIN = 1e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# XV_WRITE_PROFILES=1: the replay test also writes its lines to profiles/anymdp_mbrl_replay.txt (otherwise it only prints)
REPLAY_TXT = os.path.join(ROOT, "profiles", "anymdp_mbrl_replay.txt")
_replay_lines = []


def _tasks(cfg):
    if cfg == "16x4":
        return _tasks16()
    if cfg == "64x8":
        return [load_anymdp_golden(golden_files("anymdp_64x8")[0])[1]]
    return [_fixture_task(dict(np.load(f))) for f in FILES if cfg in f]


def _close(a, b):
    return np.all(np.abs(a - b) <= 1e-4 * (1.0 + np.abs(b)))


@pytest.mark.parametrize("path", FILES, ids=lambda p: p.rsplit("/", 1)[-1])
def test_device_replays_reference_training_loop(path):
    """all draws injected: actions equal the reference's at least up to the first step whose recorded margin is below 1e-4
    (the fp32 reward is what limits this; a disagreement is allowed only at such a step); counts equal and est_r, vm, b
    within 1e-4 at every snapshot up to there"""
    g = dict(np.load(path))
    T, A = len(g["action"]), int(g["na"])
    low = np.nonzero(g["margin"] < MARGIN)[0]
    t_first_low = int(low[0]) if len(low) else T
    snap = {int(k): j for j, k in enumerate(g["snap_at"])}
    full = {int(k): j for j, k in enumerate(g["full_at"])}
    is_test = g["is_test"].astype(bool)
    cuts = sorted({0, T} | set(snap) | set(full) | {t for t in range(1, T) if is_test[t] != is_test[t - 1]})
    env = _env(_fixture_task(g), 1, seed=0)
    o0 = env.reset_injected([float(g["init_u"])])
    assert int(_np(o0)[0]) == int(g["init_obs"])
    ml = AnyMDPMBRLLearner(env, gamma=float(g["gamma"]), c=float(g["c"]))
    compared, n_snap = 0, 0
    for t0, t1 in zip(cuts[:-1], cuts[1:]):
        sl = slice(t0, t1)
        draws = dict(u_policy=g["u_policy"][sl, None, :], u=g["u"][sl, None], z=g["z"][sl, None].astype(np.float32),
                     u_reset=g["u_reset"][sl, None])
        out = {k: _np(v)[:, 0] for k, v in env.rollout_learner(ml, t1 - t0, greedy=bool(is_test[t0]), draws=draws).items()}
        bad = np.nonzero(out["action"] != g["action"][sl])[0]
        n_ok = int(bad[0]) if len(bad) else t1 - t0
        if len(bad):
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
        if t1 in snap or t1 in full:
            er, vc, vsa, vm, b = (_np(x)[0] for x in ml.get_state())
            if t1 in snap:
                j = snap[t1]
                assert np.array_equal(vsa, g["snap_vis_cnt_sa"][j]), t1
                assert _close(vm, g["snap_vm"][j]), (t1, np.abs(vm - g["snap_vm"][j]).max())
                assert _close(b, g["snap_b"][j]), t1
            if t1 in full:
                j = full[t1]
                assert np.array_equal(vc, g["snap_vis_cnt"][j]), t1
                assert _close(er, g["snap_est_r"][j]), t1
            n_snap += 1
    line = "%s: %d of %d steps compared (first margin < 1e-4 at %d), %d snapshots" % (
        path.rsplit("/", 1)[-1], compared, T, t_first_low, n_snap)
    print(line)
    _replay_lines.append(line)
    if len(_replay_lines) == len(FILES) and os.environ.get("XV_WRITE_PROFILES") == "1":
        os.makedirs(os.path.dirname(REPLAY_TXT), exist_ok=True)
        with open(REPLAY_TXT, "w") as f:
            f.write("\n".join(sorted(_replay_lines)) + "\n")
    assert compared >= t_first_low
    assert env.check_errors() == 0
    ml.close()
    env.close()


def _device_vs_host(tasks, n, T, seed, c=0.05, sample=None, rng_seed=11):
    env = _env(tasks, n, seed=seed)
    env.reset()
    obs = _np(env.state).astype(np.int64)
    ml = AnyMDPMBRLLearner(env, c=c)
    S, A = env.S, env.A
    rng = np.random.RandomState(rng_seed)
    draws = dict(u_policy=rng.random_sample((T, n, A)), u=rng.random_sample((T, n)),
                 z=rng.standard_normal((T, n)).astype(np.float32), u_reset=rng.random_sample((T, n)))
    out = {k: _np(v) for k, v in env.rollout_learner(ml, T, draws=draws).items()}
    idx = np.arange(n) if sample is None else np.asarray(sample)
    host = MBRLHost(len(idx), S, A, c=c)
    obs = obs[idx]
    most_at_once = 0
    for t in range(T):
        a = host.policy(obs, draws["u_policy"][t][idx])
        assert np.array_equal(a, out["action"][t][idx]), (t, np.nonzero(a != out["action"][t][idx])[0][:4])
        term = out["terminated"][t][idx].astype(bool)
        trunc = out["truncated"][t][idx].astype(bool)
        most_at_once = max(most_at_once, int((term | trunc).sum()))
        host.learn(obs, a, np.where(term | trunc, out["final_obs"][t][idx], out["obs"][t][idx]),
                   out["reward"][t][idx].astype(np.float64), term, trunc)
        obs = out["obs"][t][idx].astype(np.int64)
    dev = [_np(x)[idx] for x in ml.get_state()]
    for name, x, y in zip(("est_r", "vis_cnt", "vis_cnt_sa", "vm", "b"), dev, host.get_state()):
        assert np.array_equal(x, y), (name, np.abs(x - y).max())
    assert env.check_errors() == 0
    ml.close()
    env.close()
    return int(out["terminated"][:, idx].sum()), int(out["truncated"][:, idx].sum()), most_at_once


@pytest.mark.parametrize("cfg,T", [("16x4", 300), ("20x3", 260), ("48x5", 420), ("64x8", 520)])
def test_device_equals_host_restatement(cfg, T):
    """256 envs over the config's tasks, injected draws; the host is fed the device's obs, fp32 rewards and flags: every
    action and all five tables bit-equal"""
    n_term, n_trunc, most = _device_vs_host(_tasks(cfg), 256, T, seed=5, c=1.0 if cfg == "20x3" else 0.05)
    print("%s: %d terminated, %d truncated, at most %d at once" % (cfg, n_term, n_trunc, most))
    # the 20x3 task has no terminal states; the 64x8 task's episodes end by termination within a few steps
    assert (n_term > 0) == (cfg != "20x3") and (n_trunc > 0) == (cfg != "64x8")
    assert most >= 16


@pytest.mark.parametrize("S,A", [(200, 3), (512, 16)])
def test_device_equals_host_long_rows_and_global_products(S, A):
    """rows longer than 128 (numpy's row sum splits into a pairwise tree), and at 512 x 16 the row's products in a global
    slab (they do not fit LDS): 8 envs, every env's episode ended at the first step, then T more steps; the host is fed the
    device's obs, fp32 rewards and flags: every action and all five tables bit-equal"""
    n, T = 8, 12
    env = _env([_random_task(S, A, seed=S + A)], n, seed=6)
    env.reset()
    env.set_state(steps=np.full(n, 49, np.int32))       # max_steps - 1: the first step truncates every episode
    obs = _np(env.state).astype(np.int64)
    ml = AnyMDPMBRLLearner(env, c=1.0)
    rng = np.random.RandomState(S)
    draws = dict(u_policy=rng.random_sample((T, n, A)), u=rng.random_sample((T, n)),
                 z=rng.standard_normal((T, n)).astype(np.float32), u_reset=rng.random_sample((T, n)))
    out = {k: _np(v) for k, v in env.rollout_learner(ml, T, draws=draws).items()}
    assert np.all(out["truncated"][0] == 1)
    host = MBRLHost(n, S, A, c=1.0)
    for t in range(T):
        a = host.policy(obs, draws["u_policy"][t])
        assert np.array_equal(a, out["action"][t]), t
        term, trunc = out["terminated"][t].astype(bool), out["truncated"][t].astype(bool)
        host.learn(obs, a, np.where(term | trunc, out["final_obs"][t], out["obs"][t]),
                   out["reward"][t].astype(np.float64), term, trunc)
        obs = out["obs"][t].astype(np.int64)
    for name, x, y in zip(("est_r", "vis_cnt", "vis_cnt_sa", "vm", "b"), (_np(x) for x in ml.get_state()), host.get_state()):
        assert np.array_equal(x, y), (name, np.abs(x - y).max())
    assert np.any(host.vm != 0.0)
    assert env.check_errors() == 0
    ml.close()
    env.close()


def test_scale_65536_envs_sampled_against_host():
    """65,536 envs of the 64x8 task, injected draws, 512 sampled envs compared bit for bit with the host restatement"""
    rng = np.random.RandomState(3)
    sample = np.sort(rng.choice(65536, 512, replace=False))
    n_term, n_trunc, most = _device_vs_host(_tasks("64x8"), 65536, 300, seed=8, sample=sample, rng_seed=4)
    print("scale: %d terminated, %d truncated in the sample" % (n_term, n_trunc))
    assert n_term + n_trunc > 0


def test_learning_is_real():
    """greedy reward per step over 100 steps, of agents trained for 1,500 steps against that of freshly made ones (vm = 0:
    action 0 until their first episode end), same tasks and seed, on the scale of the random and the optimal teacher.
    c = 1 (the class default; train()'s c = 0.05 explores little on these tasks).  Measured: fresh -0.14, trained 0.095,
    random -0.34, optimal 0.117"""
    n = 256
    res = {}
    for train in (0, 1500):
        env = _env(_tasks16(), n, seed=3)
        env.reset()
        ml = AnyMDPMBRLLearner(env, c=1.0)
        if train:
            env.rollout_learner(ml, train)
        res[train] = float(_np(env.rollout_learner(ml, 100, greedy=True)["reward_gt"]).mean())
        if not train:
            res["rnd"] = float(_np(env.rollout_teacher(600, epsilon=1.0)["reward_gt"]).mean())
            res["opt"] = float(_np(env.rollout_teacher(600)["reward_gt"]).mean())
        assert env.check_errors() == 0
        ml.close()
        env.close()
    gap = res["opt"] - res["rnd"]
    print("greedy reward per step: fresh %.4f, trained %.4f (random %.4f, optimal %.4f)" % (
        res[0], res[1500], res["rnd"], res["opt"]))
    assert gap > 0.1
    assert res[1500] - res[0] >= 0.3 * gap
    assert res[1500] - res["rnd"] >= 0.7 * gap


def test_state_round_trip_and_masked_reset():
    n = 64
    env = _env(_tasks16(), n, seed=4)
    env.reset()
    ml = AnyMDPMBRLLearner(env, gamma=0.9, c=0.5)
    er, vc, vsa, vm, b = (_np(x) for x in ml.get_state())
    assert er.shape == (n, 16, 4, 16) and vm.shape == (n, 16, 4)
    assert np.all(er == 0) and np.all(vc == 0.01) and np.all(vsa == 1) and np.all(vm == 0)
    assert np.all(b == (0.5 / (1.0 - 0.9)) * 0.01)
    rng = np.random.RandomState(2)
    st = [rng.randn(n, 16, 4, 16), rng.random_sample((n, 16, 4, 16)), rng.random_sample((n, 16, 4)) + 1,
          rng.randn(n, 16, 4), rng.random_sample((n, 16, 4))]
    ml.set_state(*st)
    assert all(np.array_equal(_np(x), y) for x, y in zip(ml.get_state(), st))
    assert np.array_equal(_np(ml.vm), st[3]) and np.array_equal(_np(ml.est_r), st[0]) and np.array_equal(_np(ml.b), st[4])
    ml.set_state(vm=np.zeros((n, 16, 4)))
    assert np.all(_np(ml.vm) == 0) and np.array_equal(_np(ml.vis_cnt), st[1])
    env.rollout_learner(ml, 32)
    before = [_np(x) for x in ml.get_state()]
    mask = np.zeros(n, bool)
    mask[::3] = True
    ml.reset(mask)
    after = [_np(x) for x in ml.get_state()]
    for x, y in zip(before, after):
        assert np.array_equal(y[~mask], x[~mask])
    assert np.all(after[1][mask] == 0.01) and np.all(after[3][mask] == 0)
    assert np.all(after[4][mask] == (0.5 / (1.0 - 0.9)) * 0.01)
    with pytest.raises(ValueError):
        ml.reset(np.zeros(n + 1, bool))
    with pytest.raises(ValueError):
        ml.set_state(vm=np.zeros((n, 16, 5)))
    assert env.check_errors() == 0
    ml.close()
    env.close()
