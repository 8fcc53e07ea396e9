"""GPU parity: HIP Acrobot (C-ABI) vs the CPU oracle on seeded batches.  The state is fp64 on both sides with the
same expression order; device sin/cos differ from libm in the last bits, so the pose is compared at 1e-9 and the
oracle is re-synchronised from the device every step (no compounding); flags are compared away from the
termination threshold."""
import numpy as np
import pytest

import oracle
from xenoverse_amd.metacontrol import AcrobotVecEnv, sample_acrobot
from xenoverse_amd.metacontrol.acrobot import TASK_KEYS

pytestmark = pytest.mark.gpu
MODES = {"disabled": 0, "next_step": 1, "same_step": 2}


def _np(t):
    return t.detach().cpu().numpy()


def _params(tasks):
    return np.array([[t[k] for k in TASK_KEYS] for t in tasks], np.float64)


@pytest.mark.parametrize("mode", ["disabled", "next_step", "same_step"])
@pytest.mark.parametrize("frameskip,scale", [(1, 0.10), (5, 0.10), (3, [0.9, 0.8, 0.5, 0.5])])
def test_batch_vs_oracle(mode, frameskip, scale):
    n, n_task = 1000, 50
    tasks = [sample_acrobot(seed=k) for k in range(n_task)]
    env_task = (np.arange(n) % n_task).astype(np.int32)
    env = AcrobotVecEnv(n, frameskip=frameskip, reset_bounds_scale=scale, autoreset_mode=mode, max_steps=40)
    env.set_task(tasks, env_task_index=env_task)
    ora = oracle.AcrobotOracle(_params(tasks), env_task, frameskip=frameskip, max_steps=40, reset_scale=scale)
    rng = np.random.RandomState(1)
    u0 = rng.random_sample((4, n))
    o0 = ora.reset_injected(u0)
    assert np.allclose(_np(env.reset_injected(u0)), o0, rtol=0, atol=2e-7)
    assert np.array_equal(_np(env.get_state()[0]), ora.state)      # the reset state itself is exact
    ended = term_seen = 0
    for t in range(120):
        a = rng.randint(0, 3, n).astype(np.int32)
        u = rng.random_sample((4, n))
        obs, r, term, trunc, info = env.step_injected(a, u)
        o = ora.step_injected(a, u, MODES[mode])
        s, st, nr = env.get_state()
        done_o = (o["terminated"] | o["truncated"]).astype(bool)
        reset_now = done_o if mode == "same_step" else np.zeros(n, bool)
        # With frameskip 1 every env must agree: flags and reward exactly, pose to 1e-9.  With frameskip > 1 the map
        # over 1 s of simulated time is chaotic in part of the task range: a ONE-ULP perturbation of the state moves
        # 0.8 % of the env-steps by more than 1e-9 and 0.1 % completely (measured on the oracle itself), so the
        # device's last-bit sin/cos differences legitimately do the same; those envs are excluded, at most 2 %.
        dev_s = _np(s)
        dst = np.abs(dev_s - ora.state)
        dst[:2] = np.minimum(dst[:2], np.abs(dst[:2] - 2 * np.pi))         # equal up to a wrap at the boundary
        same_flags = _np(term).astype(np.uint8) == o["terminated"]
        tol = 1e-9 if frameskip == 1 else 1e-6
        ok = same_flags & (dst.max(0) < tol)
        if mode == "same_step":     # the pose of an env that ended is visible in final_obs only (its state is the reset)
            fdiff = np.abs(_np(info["final_obs"]) - o["final_obs"]).max(1)
            ok &= ~done_o | (fdiff < (1e-6 if frameskip == 1 else 2e-5))
        assert ok.mean() > (0.999 if frameskip == 1 else 0.98), ok.mean()
        assert np.array_equal(_np(trunc).astype(np.uint8), o["truncated"])
        assert np.array_equal(_np(r)[ok], o["reward"][ok])
        assert np.allclose(_np(obs)[ok], o["obs"][ok], rtol=2e-6, atol=2e-6)
        assert np.array_equal(_np(st)[ok], ora.steps[ok]) and np.array_equal(_np(nr)[ok], ora.need_reset[ok])
        ora.state[:] = _np(s); ora.steps[:] = _np(st); ora.need_reset[:] = _np(nr)   # re-sync: no compounding
        ora.fresh[:] = (_np(st) == 0) & (reset_now | (mode == "next_step"))
        ended += int(done_o.sum()); term_seen += int(o["terminated"].sum())
        if mode == "disabled" and done_o.any():
            ur = rng.random_sample((4, n))
            m = done_o.astype(np.uint8)
            env.reset_injected(ur, mask=m); ora.reset_injected(ur, mask=m)
    assert ended > 500 and (term_seen > 20 or frameskip == 1)
    assert env.check_errors() == 0
    env.close()


def test_free_running_philox_and_misuse():
    n = 256
    tasks = [sample_acrobot(seed=100 + k) for k in range(n)]
    seed, base = 77, 1 << 21
    env = AcrobotVecEnv(n, frameskip=2, seed=seed, env_id_base=base, autoreset_mode="same_step", max_steps=25)
    with pytest.raises(Exception, match="Must call \"set_task\" first"):
        env.reset()
    env.set_task(tasks)
    with pytest.raises(Exception, match="before doing any actions"):
        env.step(np.zeros(n, np.int32))
    ora = oracle.AcrobotOracle(_params(tasks), np.arange(n), frameskip=2, max_steps=25)
    tick = env.engine.tick
    obs, _ = env.reset()
    assert np.allclose(_np(obs), ora.reset(seed, base, tick), rtol=0, atol=2e-7)
    assert np.array_equal(_np(env.get_state()[0]), ora.state)      # same Philox draws, same reset state bits
    rng = np.random.RandomState(2)
    resets = 0
    for t in range(60):
        a = rng.randint(0, 3, n).astype(np.int32)
        tick = env.engine.tick
        obs, r, term, trunc, info = env.step(a)
        if "_final_obs" in info:      # the done mask comes from the step launch (xv_*_step_info)
            assert np.array_equal(_np(info["_final_obs"]), _np(term) | _np(trunc))
        o = ora.step(seed, base, tick, a, 2)
        assert np.array_equal(_np(trunc).astype(np.uint8), o["truncated"])
        agree = _np(term).astype(np.uint8) == o["terminated"]      # marginal terminal tests may differ in the last bit
        assert agree.mean() > 0.99
        s, st, _ = env.get_state()
        s, st = _np(s), _np(st)
        assert np.allclose(s[:, agree], ora.state[:, agree], rtol=1e-9, atol=1e-9)
        done = (o["terminated"] | o["truncated"]).astype(bool) & agree
        assert np.array_equal(s[:, done], ora.state[:, done])      # same Philox draws -> the reset states are exact
        resets += int(done.sum())
        ora.state[:] = s; ora.steps[:] = st
        ora.fresh[:] = (st == 0)
    assert resets > 100
    env.step(np.full(n, 7, np.int32))
    assert env.check_errors() & 1            # action out of range
    env.close()
