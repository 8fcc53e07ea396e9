"""GPU: what CartPole and Acrobot share (csrc/xv_control.h, metacontrol/base.py) — misuse errors, the fused roll-out, the
copy=False path, the infos of same_step auto-reset and the state round trip — for both families.  The physics is tested
in test_gpu_cartpole.py / test_gpu_acrobot.py."""
import numpy as np
import pytest

from xenoverse_amd.metacontrol import AcrobotVecEnv, CartPoleVecEnv, sample_acrobot, sample_cartpole

pytestmark = pytest.mark.gpu
FAMILIES = {"cartpole": (CartPoleVecEnv, sample_cartpole, 2), "acrobot": (AcrobotVecEnv, sample_acrobot, 3)}   # env, sampler, actions
family = pytest.mark.parametrize("family", sorted(FAMILIES))


def _np(t):
    return t.detach().cpu().numpy()


def _make(family, n, n_task, **kw):
    cls, sample, _ = FAMILIES[family]
    env = cls(n, **kw)
    env.set_task([sample(seed=k) for k in range(n_task)], env_task_index=(np.arange(n) % n_task).astype(np.int32))
    return env


@family
def test_misuse(family):
    cls, sample, _ = FAMILIES[family]
    n = 64
    env = cls(n)
    with pytest.raises(Exception, match="Must call \"set_task\" first"):
        env.reset()
    env.set_task([sample(seed=k) for k in range(n)])
    with pytest.raises(Exception, match="before doing any actions"):
        env.step(np.zeros(n, np.int32))
    env.close()


@family
@pytest.mark.parametrize("mode", ["same_step", "next_step"])
def test_fused_rollout_equals_single_steps(family, mode):
    """xv_*_rollout: T steps in one launch = T calls of xv_*_step bit for bit, through episode ends"""
    n, T, cut, n_task, max_steps = {"cartpole": (1000, 120, 50, 50, 30), "acrobot": (600, 90, 40, 40, 20)}[family]
    acts = np.random.RandomState(1).randint(0, FAMILIES[family][2], (T, n)).astype(np.int32)
    recs = []
    for fused in (False, True):
        env = _make(family, n, n_task, frameskip=2, seed=9, env_id_base=40, autoreset_mode=mode, max_steps=max_steps)
        env.reset()
        if fused:
            a = env.rollout(acts[:cut]); b = env.rollout(acts[cut:])
            rec = {k: np.concatenate([_np(a[k]), _np(b[k])]) for k in a}
        else:
            rows = []
            for t in range(T):
                o, r, te, tr, info = env.step(acts[t])
                rows.append(dict(obs=_np(o), reward=_np(r), terminated=_np(te).astype(np.uint8),
                                 truncated=_np(tr).astype(np.uint8), final_obs=_np(info["final_obs"]) if "final_obs" in info
                                 else None))
            rec = {k: np.stack([row[k] for row in rows]) for k in rows[0] if rows[0][k] is not None}
        st = env.get_state()
        rec.update(state=_np(st[0]), steps=_np(st[1]), tick=np.int64(env.engine.tick))
        recs.append(rec)
        env.close()
    assert recs[0]["truncated"].sum() > 0 and (family != "cartpole" or recs[0]["terminated"].sum() > 0)
    for k in recs[0]:
        assert np.array_equal(recs[0][k], recs[1][k]), k


@family
@pytest.mark.parametrize("mode", ["same_step", "next_step"])
def test_copy_false_steps_equal_fresh_tensor_steps(family, mode):
    """copy=False (persistent outputs, cached pointers and views) returns what copy=True returns: same seed, same actions"""
    n = 300
    envs = [_make(family, n, 10, frameskip=1, autoreset_mode=mode, max_steps=40, seed=5, copy=copy) for copy in (True, False)]
    o = [_np(e.reset()[0]).copy() for e in envs]
    assert np.array_equal(o[0], o[1])
    rng = np.random.RandomState(3)
    ended = 0
    for t in range(120):
        a = rng.randint(0, 2, n).astype(np.int32)
        outs = [e.step(a) for e in envs]
        got = [[_np(x).copy() for x in out[:4]] for out in outs]
        for x, y in zip(*got):
            assert np.array_equal(x, y)
        if mode == "same_step":
            done = got[1][2] | got[1][3]
            assert np.array_equal(_np(outs[1][4]["_final_obs"]), done) and np.array_equal(_np(outs[0][4]["_final_obs"]), done)
            assert np.array_equal(_np(outs[0][4]["final_obs"])[done], _np(outs[1][4]["final_obs"])[done])
            ended += int(done.sum())
    assert mode != "same_step" or ended > 100
    for e in envs:
        e.close()


@family
@pytest.mark.parametrize("copy", [True, False])
@pytest.mark.parametrize("lean", [True, False])
def test_same_step_infos_with_a_partial_last_workgroup(family, copy, lean):
    """n = 300 is no multiple of either family's workgroup size (256 / 64), so the last workgroup is partly idle;
    max_steps = 3 ends every episode at steps 3 and 6.  lean_infos drops `_final_obs` (the mask is terminated | truncated)
    and keeps `final_obs`, in the copying path and in the copy=False path alike."""
    n = 300
    env = _make(family, n, 10, frameskip=1, autoreset_mode="same_step", max_steps=3, seed=11, copy=copy)
    env.lean_infos = lean
    env.reset()
    rng = np.random.RandomState(4)
    count, ended = np.zeros(n, np.int64), 0
    for t in range(8):
        obs, r, term, trunc, info = env.step(rng.randint(0, FAMILIES[family][2], n).astype(np.int32))
        term, trunc, fobs = _np(term), _np(trunc), _np(info["final_obs"])
        count += 1
        assert np.array_equal(trunc, count >= 3)              # every env of the batch, the partial workgroup's included
        done = term | trunc
        count[done] = 0
        ended += int(done.sum())
        assert _np(obs).shape == (n, env.OBS_DIM) and np.isfinite(_np(obs)).all()
        assert fobs.shape == (n, env.OBS_DIM) and fobs[done].any(1).all() and not fobs[~done].any()
        if lean:
            assert "_final_obs" not in info
        else:
            assert np.array_equal(_np(info["_final_obs"]), done)
    assert ended >= 2 * n
    assert env.check_errors() == 0
    env.close()


@family
def test_state_round_trip_replays_bit_equal(family):
    """get_state, 5 steps, set_state of the snapshot with the engine tick set back: the same 5 actions give the same bits
    (max_steps = 4: every env is reset off its Philox stream inside the 5 steps)"""
    n = 300
    env = _make(family, n, 10, frameskip=2, autoreset_mode="same_step", max_steps=4, seed=21)
    env.reset()
    rng = np.random.RandomState(5)
    for t in range(3):
        env.step(rng.randint(0, FAMILIES[family][2], n).astype(np.int32))
    snap, tick = env.get_state(), env.engine.tick
    acts = rng.randint(0, FAMILIES[family][2], (5, n)).astype(np.int32)
    runs = []
    for rep in range(2):
        rows = []
        for a in acts:
            o, r, te, tr, info = env.step(a)
            rows.append([_np(o), _np(r), _np(te), _np(tr), _np(info["final_obs"]), _np(info["_final_obs"])])
        rows.append([_np(x) for x in env.get_state()])
        runs.append(rows)
        env.set_state(*snap)
        env.engine.tick = tick
    assert sum(int(row[3].sum()) for row in runs[0][:5]) >= n
    for x, y in zip(runs[0], runs[1]):
        for p, q in zip(x, y):
            assert np.array_equal(p, q)
    env.close()
