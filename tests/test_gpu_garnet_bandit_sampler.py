"""The device Garnet and bandit task samplers (csrc/anymdp_garnet.hip) against their host restatement
(xenoverse_amd/anymdp/sampler_host_garnet.py): bit for bit in everything made of integers and fp64 sums, differences, products
and quotients, within the project's device-sampler tolerance where the device's log, cos and sin enter (they are not
numpy's); one launch against any split of it; nothing written outside the arrays; and the tables end to end in
AnyMDPVecEnv against the same tasks given as dicts.  Settings and seeds: tests/garnet_bandit_util.py."""
import numpy as np
import pytest
import torch

import garnet_bandit_util as U
from xenoverse_amd import _lib
from xenoverse_amd.anymdp import (AnyMDPQLearner, AnyMDPVecEnv, sample_bandit_tasks_device, sample_garnet_tasks_device,
                                  sample_tasks_device, task_dicts_from_device)
from xenoverse_amd.anymdp import device_sampler as ds, sampler_host_garnet as sh
from xenoverse_amd.anymdp.tables import build_tables, row_cdf, row_lines, to_blocked

pytestmark = pytest.mark.gpu

EXACT = ("state_map", "term_mask", "s0_cdf", "s0_ids", "max_steps")


def _np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def eng():
    from xenoverse_amd.engine import Engine
    e = Engine("cuda:0")
    yield e
    e.close()


def _garnet_device(eng, name, **over):
    kw = dict(U.garnet_kwargs(name), engine=eng, dense=True)
    kw.update(over)
    return sample_garnet_tasks_device(U.GARNET[name][3], **kw)


def _share(got, want, what):
    """-> the worst deviation as a share of the tolerance RTOL |want| + ATOL (printed; asserted below 1)"""
    share = float((np.abs(got - want) / (U.RTOL * np.abs(want) + U.ATOL)).max())
    print("%s: worst deviation %.3g of the tolerance" % (what, share))
    return share


def _assert_rows_of_own_dense(dev, S):
    """rows == to_blocked(row_cdf(T_dev), the fp32 pairs of the device's dense tensors), the zero fence and tails included;
    padded states as build_tables pads them (CDF 1.0, zero pairs)"""
    T, R, N = (_np(dev[k]) for k in ("transition", "reward", "reward_noise"))
    n_real = _np(dev["n_real"])
    cdf = np.ones_like(T)
    for i, n in enumerate(n_real):
        cdf[i, :n, :, :n] = row_cdf(T[i, :n, :, :n])
    rs = np.stack([R, N], axis=-1).astype(np.float32)
    rows = _np(dev["rows"])
    assert rows.shape == T.shape[:3] + (row_lines(S), 16)
    assert rows.tobytes() == to_blocked(cdf, rs).tobytes()
    assert (rows[..., 0, :] == 0).all() and (rows[..., 1:, 14:] == 0).all()


# ---- 1. device against host ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(U.GARNET))
def test_garnet_device_equals_host(eng, name):
    S, A, b, n_tasks, m = U.GARNET[name]
    host = U.garnet_host(name)
    real = np.array([t["max_steps"] for t in host["tasks"]])
    assert np.abs(real - np.round(real)).min() > 1e-9      # ceil(max_steps) does not hang on the last bit of the draw
    if name == "ragged":
        assert len(set(host["n_real"].tolist())) >= 2 and host["n_real"].max() == S
    if name == "b_is_n":
        assert (S * A * S) % 2 == 1
    tick = eng.tick
    dev = _garnet_device(eng, name)
    assert eng.tick == tick and eng.error_flags() == 0
    assert (dev["S"], dev["A"], dev["s0_max"]) == (S, A, 4) and dev["stats"]["accepted"] == n_tasks
    for k in EXACT + ("n_real", "transition"):
        got = _np(dev[k])
        want = host[k].view(np.int64) if host[k].dtype == np.uint64 else host[k]
        assert got.dtype == want.dtype and got.shape == want.shape, k
        assert got.tobytes() == want.tobytes(), k
    assert (dev["obs_space"] == host["obs_space"]).all()
    # every CDF entry of the row records
    ent = _np(dev["rows"])[..., 1:, :14].reshape(n_tasks, S, A, -1, 2)[..., 0]
    want = host["rows"][..., 1:, :14].reshape(n_tasks, S, A, -1, 2)[..., 0]
    assert ent.tobytes() == want.tobytes()
    assert _share(_np(dev["reward"]), host["reward"], name + " reward") < 1.0
    assert (_np(dev["reward_noise"]) == 0).all()
    _assert_rows_of_own_dense(dev, S)


@pytest.mark.parametrize("A", U.BANDIT_A)
def test_bandit_device_equals_host(eng, A):
    status, tasks, recs = U.bandit_host(A)
    assert (status == 0).any() and (status == 1).any()
    assert U.bandit_margin(recs) > 1e-9      # no round is decided by the last bits of the device's log
    n, base = U.BANDIT_N, U.BANDIT_CAND_BASE[A]
    dev = ds.sample_bandit_candidates(eng, U.BANDIT_SEED, base, n, A, U.BANDIT_ROUNDS, dense=True)
    eng.sync()
    assert eng.error_flags() == 0
    assert _np(dev["status"]).tobytes() == status.tobytes()
    acc = np.nonzero(status == 0)[0]
    host = sh.bandit_tables([tasks[i] for i in acc])
    for k in EXACT:
        got = _np(dev[k])[acc]
        want = host[k].view(np.int64) if host[k].dtype == np.uint64 else host[k]
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), k
    for k in ("reward", "reward_noise"):
        assert _share(_np(dev[k])[acc], host[k], "bandit A = %d %s" % (A, k)) < 1.0
    # the row records: build_tables' embedding of the device's own dense tensors, bit for bit
    own = [dict(t, reward=_np(dev["reward"])[i], reward_noise=_np(dev["reward_noise"])[i]) for i, t in zip(acc, [tasks[i] for i in acc])]
    assert _np(dev["rows"])[acc].tobytes() == build_tables(own, s0_max=4)["rows"].tobytes()
    ent = _np(dev["rows"])[acc][..., 1, :14].reshape(len(acc), 2, A, 7, 2)[..., 0]
    assert ent.tobytes() == host["rows"][..., 1, :14].reshape(len(acc), 2, A, 7, 2)[..., 0].tobytes()


# ---- 2. one launch against any split of it ------------------------------------------------------------------------------------
KEYS = ("rows",) + EXACT + ("n_real", "transition", "reward", "reward_noise")


@pytest.mark.parametrize("name", ["b_is_n", "ragged"])
def test_garnet_tasks_do_not_depend_on_the_launch_batch(eng, name):
    n = U.GARNET[name][3]
    whole = _garnet_device(eng, name)
    for batch in (1, 3, n):
        part = _garnet_device(eng, name, batch=batch)
        assert part["stats"]["batch"] == batch
        for k in KEYS:
            assert _np(part[k]).tobytes() == _np(whole[k]).tobytes(), (batch, k)
    # a non-zero task_base through the C entry point: tasks 2 .. n - 1 in a launch of their own
    S, A, b, _, m = U.GARNET[name]
    out = ds._table_slots(eng.device, n - 2, S, A, 4)
    out["n_real"] = torch.empty(n - 2, dtype=torch.int32, device=eng.device)
    for k in ("transition", "reward", "reward_noise"):
        out[k] = torch.empty((n - 2, S, A, S), dtype=torch.float64, device=eng.device)
    _lib.check(eng.lib.xv_anymdp_sample_garnet(eng.handle, U.GARNET_SEED[name], 2, n - 2, S, A, m or 0, b, U.SIGMA, 4,
                                               *(_lib.ptr(out[k]) for k in KEYS)))
    eng.sync()
    for k in KEYS:
        assert _np(out[k]).tobytes() == _np(whole[k])[2:].tobytes(), k


def test_bandit_tasks_do_not_depend_on_the_launch_batch(eng):
    kw = dict(action_space=5, seed=U.BANDIT_SEED, max_rounds=U.BANDIT_ROUNDS, engine=eng, dense=True)
    whole = sample_bandit_tasks_device(40, batch=64, **kw)
    assert whole["stats"]["status"]["no_spread"] > 0
    for batch in (1, 3):
        part = sample_bandit_tasks_device(40, batch=batch, **kw)
        assert part["stats"]["status"] == whole["stats"]["status"]
        for k in ("rows",) + EXACT + ("reward", "reward_noise", "transition", "n_real"):
            assert _np(part[k]).tobytes() == _np(whole[k]).tobytes(), (batch, k)


# ---- 3. nothing written outside the arrays --------------------------------------------------------------------------------------
G = 64
FILL = {torch.float64: -7.0, torch.int32: -7, torch.int64: -7}


def _guarded(eng, shapes):
    """name -> (flat tensor with G guard elements on either side, element count)"""
    out = {}
    for k, (shape, dtype) in shapes.items():
        c = int(np.prod(shape))
        out[k] = (torch.full((c + 2 * G,), FILL[dtype], dtype=dtype, device=eng.device), c)
    return out


def _assert_guards(bufs):
    for k, (t, c) in bufs.items():
        h = _np(t)
        assert (h[:G] == -7).all() and (h[G + c:] == -7).all(), k


@pytest.mark.parametrize("name", ["b_is_n", "ragged"])
def test_garnet_writes_nothing_outside_its_arrays(eng, name):
    S, A, b, n, m = U.GARNET[name]
    f64, i32, i64 = torch.float64, torch.int32, torch.int64
    shapes = dict(rows=((n, S, A, row_lines(S), 16), f64), state_map=((n, S), i32), term_mask=((n, (S + 63) // 64), i64),
                  s0_cdf=((n, 4), f64), s0_ids=((n, 4), i32), max_steps=((n,), i32), n_real=((n,), i32),
                  transition=((n, S, A, S), f64), reward=((n, S, A, S), f64), reward_noise=((n, S, A, S), f64))
    bufs = _guarded(eng, shapes)
    _lib.check(eng.lib.xv_anymdp_sample_garnet(eng.handle, U.GARNET_SEED[name], 0, n, S, A, m or 0, b, U.SIGMA, 4,
                                               *(_lib.ptr(bufs[k][0][G:]) for k in KEYS)))
    eng.sync()
    _assert_guards(bufs)
    host = U.garnet_host(name)
    for k in EXACT + ("n_real", "transition"):
        t, c = bufs[k]
        assert _np(t)[G:G + c].tobytes() == host[k].tobytes(), k
    t, c = bufs["reward"]
    np.testing.assert_allclose(_np(t)[G:G + c], host["reward"].reshape(-1), rtol=U.RTOL, atol=U.ATOL)
    t, c = bufs["rows"]      # every element of the records was written (none keeps the fill)
    assert not (_np(t)[G:G + c] == -7).any()


@pytest.mark.parametrize("A", U.BANDIT_A)
def test_bandits_write_nothing_outside_their_arrays(eng, A):
    n, base = U.BANDIT_N - 1, U.BANDIT_CAND_BASE[A]      # 95 candidates: a ragged last workgroup
    f64, i32, i64 = torch.float64, torch.int32, torch.int64
    shapes = dict(rows=((n, 2, A, 2, 16), f64), state_map=((n, 2), i32), term_mask=((n, 1), i64), s0_cdf=((n, 4), f64),
                  s0_ids=((n, 4), i32), max_steps=((n,), i32), reward=((n, A), f64), reward_noise=((n, A), f64),
                  status=((n,), i32))
    bufs = _guarded(eng, shapes)
    _lib.check(eng.lib.xv_anymdp_sample_bandits(eng.handle, U.BANDIT_SEED, base, n, A, U.BANDIT_ROUNDS, 4,
                                                *(_lib.ptr(bufs[k][0][G:]) for k in shapes)))
    eng.sync()
    _assert_guards(bufs)
    status = U.bandit_host(A)[0][:n]
    t, c = bufs["status"]
    assert _np(t)[G:G + c].tobytes() == status.tobytes()
    rows = _np(bufs["rows"][0])[G:G + bufs["rows"][1]].reshape(n, -1)
    assert (rows[status == 1] == -7).all() and not (rows[status == 0] == -7).any()      # rejected slots stay untouched


# ---- 4. end to end ------------------------------------------------------------------------------------------------------------
def _pair_of_envs(eng, tables, envs):
    """one env per task on the tables as they are, one on the same tasks as dicts -> appended to envs"""
    n = int(tables["max_steps"].shape[0])
    for tasks in (tables, task_dicts_from_device(tables)):
        envs.append(AnyMDPVecEnv(n, engine=eng, seed=0))
        envs[-1].set_task(tasks)


def _end_to_end(eng, tables, bandit=False):
    envs = []
    try:      # an env destroys its handle through the engine: a failing check must not leave one to outlive the fixture's engine
        _pair_of_envs(eng, tables, envs)
        _check_end_to_end(eng, tables, envs[0], envs[1], bandit)
    finally:
        for env in envs:
            env.close()


def _check_end_to_end(eng, tables, a_env, b_env, bandit):
    n, A = int(tables["max_steps"].shape[0]), int(tables["A"])
    assert (a_env.S, a_env.A, a_env.ns, a_env.n_task) == (b_env.S, b_env.A, b_env.ns, b_env.n_task)
    actions = torch.from_numpy(np.random.RandomState(0).randint(0, A, size=(64, n)).astype(np.int32)).to(eng.device)
    outs = []
    for env in (a_env, b_env):
        obs, info = env.reset(seed=5)      # the same engine, the same launch ticks from here on
        ro = env.rollout(actions)
        outs.append((_np(obs), {k: _np(v) for k, v in ro.items()}))
    assert outs[0][0].tobytes() == outs[1][0].tobytes()
    assert set(outs[0][1]) == set(outs[1][1])
    for k in outs[0][1]:
        assert outs[0][1][k].tobytes() == outs[1][1][k].tobytes(), k
    if bandit:
        assert outs[0][1]["terminated"].all()      # a single-state task ends every step (anymdp_env.py:107-108)
    sa, sb = a_env.solve(), b_env.solve()
    for x, y in zip(sa, sb):
        assert _np(x).tobytes() == _np(y).tobytes()
    a_env.reset(seed=6)
    te = a_env.rollout_teacher(32)
    assert te["action"].shape == (32, n)
    lr = AnyMDPQLearner(a_env)
    out = a_env.rollout_learner(lr, 32)
    assert out["action"].shape == (32, n)
    eng.sync()
    assert eng.error_flags() == 0
    lr.close()


@pytest.mark.parametrize("name", ["default", "ragged"])
def test_garnet_tables_run_as_the_same_tasks_given_as_dicts(eng, name):
    _end_to_end(eng, _garnet_device(eng, name))


def test_bandit_tables_run_as_the_same_tasks_given_as_dicts(eng):
    tables = sample_bandit_tasks_device(9, 5, seed=U.BANDIT_SEED, max_rounds=U.BANDIT_ROUNDS, engine=eng, dense=True)
    assert tables["S"] == 2 and tables["stats"]["accepted"] == 9 and tables["stats"]["status"]["no_spread"] > 0
    _end_to_end(eng, tables, bandit=True)


def test_task_dicts_need_the_dense_tensors(eng):
    with pytest.raises(ValueError, match="dense=True"):
        task_dicts_from_device(_garnet_device(eng, "minimum", dense=False))
    dicts = task_dicts_from_device(_garnet_device(eng, "ragged"))
    assert [d["transition"].shape[0] for d in dicts] == U.garnet_host("ragged")["n_real"].tolist()
    for d, h in zip(dicts, U.garnet_host("ragged")["tasks"]):
        assert d["transition"].tobytes() == h["transition"].tobytes() and (d["state_mapping"] == h["state_mapping"]).all()


# ---- 5. sample_tasks_device(state_space=1) ------------------------------------------------------------------------------------
def test_sample_tasks_device_with_one_state_is_the_bandit_sampler(eng):
    a = sample_tasks_device(33, state_space=1, action_space=5, seed=3, engine=eng, dense=True)
    b = sample_bandit_tasks_device(33, 5, seed=3, engine=eng, dense=True)
    assert (a["S"], a["A"], a["s0_max"]) == (b["S"], b["A"], b["s0_max"]) == (2, 5, 4)
    assert a["stats"]["status"] == b["stats"]["status"]
    for k in ("rows",) + EXACT + ("reward", "reward_noise", "transition", "n_real"):
        assert _np(a[k]).tobytes() == _np(b[k]).tobytes(), k
    for task_type in ("POMDP", "MTPOMDP"):
        with pytest.raises(ValueError, match="bandit"):
            sample_tasks_device(4, state_space=1, action_space=5, engine=eng, task_type=task_type)


def test_device_refusals_name_the_limit(eng):
    with pytest.raises(ValueError, match="b = 1"):
        sample_garnet_tasks_device(1, 16, 2, b=1, engine=eng)
    with pytest.raises(ValueError, match="state_space"):
        sample_garnet_tasks_device(1, 513, 2, engine=eng)
    z = torch.zeros(4096, dtype=torch.float64, device=eng.device)
    p = _lib.ptr(z)
    rc = eng.lib.xv_anymdp_sample_garnet(eng.handle, 0, 0, 1, 16, 2, 8, 9, 0.1, 4, p, p, p, p, p, p, p, None, None, None)
    assert rc == _lib.XV_ERR_UNSUPPORTED and b"b = 9" in eng.lib.xv_last_error()
    rc = eng.lib.xv_anymdp_sample_bandits(eng.handle, 0, 0, 1, 65, 64, 4, p, p, p, p, p, p, None, None, p)
    assert rc == _lib.XV_ERR_UNSUPPORTED and b"A = 65" in eng.lib.xv_last_error()
