"""The device AnyHVAC task sampler (csrc/anyhvac_sampler.hip) against its numpy restatement
(xenoverse_amd/anyhvac/sampler_host.py), and the path from its tables into HVACVecEnv.set_task.  Cases, seeds and every
bound: anyhvac_sampler_util.py (tests/test_host_anyhvac_sampler.py checks there that the seeds' margins are safe)."""
import ctypes as C

import numpy as np
import pytest
import torch

import anyhvac_sampler_util as U
from xenoverse_amd import _lib
from xenoverse_amd.anyhvac import (HVACVecEnv, build_tables, sample_candidates, sample_tasks_device, sampler_host as sh,
                                   task_dicts_from_device)
from xenoverse_amd.anyhvac import device_sampler as ds
from xenoverse_amd.anyhvac.tables import task_doubles
from xenoverse_amd.engine import Engine

pytestmark = pytest.mark.gpu
MIXED = U.CASES["mixed"]
OBS_KEYS = ("sensor_readings", "heat_readings", "action_temp", "timestep")


@pytest.fixture(scope="module")
def engine():
    e = Engine("cuda:0")
    yield e
    e.close()


def _host(r):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in r.items()}


@pytest.mark.parametrize("case", sorted(U.CASES))
def test_candidates_match_the_restatement(engine, case):
    """every candidate of the case: status, info records and counts equal; an accepted row exact where only arithmetic is
    involved and within the derived bounds elsewhere (check_row); a rejected one all padding.  No candidate is left out."""
    host = U.host_rows(case)
    assert U.margins_safe(host) == (True, True)
    dev = _host(sample_candidates(engine, U.SEEDS[case], 0, U.N_CAND[case], info=True, config=U.CASES[case]))
    dims = dev["dims"]
    assert dims == host["dims"] and dev["table"].shape == (U.N_CAND[case], task_doubles(*dims))
    assert np.array_equal(dev["status"], host["status"])
    for k in sh.INFO_DTYPE.names:
        assert np.array_equal(dev["info"][k], host["info"][k]), (k, dev["info"][k], host["info"][k])
    pad = sh.padding_row(dims)
    for i, c in enumerate(host["candidates"]):
        label = "%s candidate %d:" % (case, i)
        if c["status"]:
            assert np.array_equal(dev["table"][i], pad), label
            assert np.array_equal(dev["extras"][i], c["extras"]), label
            continue
        assert np.array_equal(dev["table"][i, :5].astype(np.int64), [int(c["info"][k]) for k in sh.INFO_DTYPE.names[1:6]])
        U.check_row(dev["table"][i], dev["extras"][i], c, dims, label)
        # padding beyond the task's own counts, exactly as build_tables writes it
        nC, nS, nH = (int(c["info"][k]) for k in ("coolers", "sensors", "heaters"))
        d, p = sh.row_parts(dev["table"][i], dims), sh.row_parts(pad, dims)
        for name, n in (("sensors", nS), ("heaters", nH), ("heat_diffuse", nH), ("coolers", nC), ("cooler_diffuse", nC),
                        ("cooler_vent_diffuse", nC)):
            assert np.array_equal(d[name][n:], p[name][n:]), label + name
        nw, nl = int(c["info"]["n_width"]), int(c["info"]["n_length"])
        mask = np.ones(d["hc"].shape, bool)
        mask[:nw, :nl] = False
        assert (d["hc"][mask] == 1.0).all() and not d["heat_diffuse"][:, mask].any() and not d["cooler_diffuse"][:, mask].any()


def test_bytes_do_not_depend_on_the_launch_geometry(engine):
    """40 `mixed` candidates as one launch, as 7 + 33 and one by one; sample_tasks_device at two batch sizes"""
    kw = dict(config=MIXED, info=True)
    one = _host(sample_candidates(engine, 5, 0, 40, **kw))
    a, b = _host(sample_candidates(engine, 5, 0, 7, **kw)), _host(sample_candidates(engine, 5, 7, 33, **kw))
    singles = [_host(sample_candidates(engine, 5, i, 1, **kw)) for i in range(40)]
    for k in ("table", "extras", "status", "info"):
        assert one[k].tobytes() == np.concatenate([a[k], b[k]]).tobytes(), k
        assert one[k].tobytes() == np.concatenate([s[k] for s in singles]).tobytes(), k
    assert (one["status"] == 0).any()
    t1 = sample_tasks_device(12, seed=5, config=MIXED, engine=engine, batch=5)
    t2 = sample_tasks_device(12, seed=5, config=MIXED, engine=engine, batch=16)
    assert torch.equal(t1["table"], t2["table"]) and torch.equal(t1["extras"], t2["extras"])
    assert torch.equal(t1["counts"], t2["counts"]) and t1["stats"]["candidates"] == t2["stats"]["candidates"]
    assert t1["stats"]["accepted"] == 12 and t1["table"].is_cuda and t1["counts"].dtype == torch.int32
    acc = np.flatnonzero(one["status"] == 0)[:12]
    assert np.array_equal(t1["table"].cpu().numpy(), one["table"][acc])      # task k is the k-th accepted candidate
    with pytest.raises(RuntimeError):
        sample_tasks_device(12, seed=5, config=MIXED, engine=engine, batch=4, max_candidates=8)
    with pytest.raises(ValueError):
        sample_tasks_device(1, control_type="Power", engine=engine)


def test_round_trip_through_task_dicts(engine):
    t = sample_tasks_device(6, seed=9, config=MIXED, engine=engine)
    tasks = task_dicts_from_device(t)
    back = build_tables(tasks, dims=t["dims"])
    dev = t["table"].cpu().numpy()
    off = np.ones(dev.shape[1], bool)
    off[10] = False
    assert np.array_equal(back["table"][:, off], dev[:, off])
    for i, task in enumerate(tasks):
        tol = U.avg_heat_tol(task, back["avg_total_heat"][i])
        assert abs(back["table"][i, 10] - dev[i, 10]) <= tol, (i, back["table"][i, 10], dev[i, 10], tol)
        assert len(task["cooler_loc"]) == int(t["counts"][i, 2]) and task["heat_diffuse"].shape[1:] == tuple(
            int(v) for v in t["counts"][i, :2])
    gen = sample_tasks_device(2, seed=9, config=MIXED, engine=engine, generate_task=True)
    assert (gen["table"][:, 10] == 10000.0).all() and torch.equal(gen["table"][:, off], t["table"][:2][:, off])


def test_set_task_borrows_the_device_tables(engine):
    """16 envs on the sampler's rows (no host copy) and 16 on rows the host rebuilt from task_dicts_from_device: the same
    steps, byte for byte, except the reward — the rebuilt rows carry the host's average heat, which enters energy_cost alone"""
    settings = dict(iter_per_step=20, max_steps=50, autoreset_mode="disabled", seed=4)
    t = sample_tasks_device(16, seed=2, config=MIXED, engine=engine)
    a = HVACVecEnv(16, **settings)
    a.set_task(t)
    assert a._tab["table"].data_ptr() == t["table"].data_ptr() and a._task_list is None
    assert np.array_equal(a.counts["coolers"], t["counts"][:, 2].cpu().numpy())
    tasks = task_dicts_from_device(t)
    back = build_tables(tasks, dims=t["dims"])
    b = HVACVecEnv(16, **settings)
    b.set_task(dict(t, table=torch.from_numpy(back["table"]).to(t["table"].device)))
    assert np.array_equal(a.default_action_value, b.default_action_value) and np.array_equal(a._targets, b._targets)
    # what the device path read back from `counts` and the table columns, against the list-of-flat-dicts path
    c = HVACVecEnv(16, **settings)
    c.set_task(tasks, generate_task=True)      # (no week-long average on the host: only the per-env values are compared)
    assert sorted(a.counts) == sorted(c.counts)
    for key in c.counts:
        assert np.array_equal(a.counts[key], c.counts[key]) and a.counts[key].dtype == c.counts[key].dtype, key
    assert np.array_equal(a._targets, c._targets) and np.array_equal(a.default_action_value, c.default_action_value)
    assert np.array_equal(a._targets, [float(task["target_temperature"]) for task in tasks])
    assert np.array_equal(a.counts["sensors"], [len(task["sensor_loc"]) for task in tasks])
    assert all(x <= y for x, y in zip(c.dims, a.dims)) and list(a.avg_total_heat) == t["table"][:, 10].tolist()
    c.close()
    oa, ob = a.reset()[0], b.reset()[0]
    for key in OBS_KEYS:
        assert torch.equal(torch.as_tensor(oa[key]), torch.as_tensor(ob[key])), key
    rng = np.random.RandomState(0)
    for k in range(5):
        act = rng.uniform(0.2, 0.8, (16, t["dims"][2])).astype(np.float32)
        ra, rb = a.step(act), b.step(act)
        for key in OBS_KEYS:
            assert torch.equal(torch.as_tensor(ra[0][key]), torch.as_tensor(rb[0][key])), (k, key)
        assert torch.equal(torch.as_tensor(ra[2]), torch.as_tensor(rb[2])) and torch.equal(torch.as_tensor(ra[3]),
                                                                                           torch.as_tensor(rb[3]))
        assert torch.equal(torch.as_tensor(ra[4]["cool_power"]), torch.as_tensor(rb[4]["cool_power"]))
        rew_a, rew_b = (np.asarray(torch.as_tensor(r[1]).cpu(), np.float64) for r in (ra, rb))
        ec = np.asarray(torch.as_tensor(rb[4]["energy_cost"]).cpu(), np.float64)
        for i, task in enumerate(tasks):
            avg = back["avg_total_heat"][i]
            tol = U.reward_tol(rew_b[i], ec[i], avg, U.avg_heat_tol(task, avg))
            assert abs(rew_a[i] - rew_b[i]) <= tol, (k, i, rew_a[i], rew_b[i], tol)
    assert a.check_errors() == 0 and b.check_errors() == 0
    # the PID teacher needs flat dicts: made from the device tables on demand
    a.set_pid(kind="gt")
    assert a._task_list is not None and len(a._tasks) == 16
    a.reset()
    out = a.rollout_teacher(3)
    assert torch.isfinite(torch.as_tensor(out[1])).all() and a.check_errors() == 0
    a.close()
    b.close()


def test_default_configuration_structure(engine):
    """four candidates at full size, no comparison with the host (the step kernel at these sizes against the host:
    tests/test_gpu_anyhvac_fullsize.py)"""
    r = sample_candidates(engine, 1, 0, 4, info=True)
    dims = r["dims"]
    assert dims == sh.table_dims() == (15, 15, 303, 607, 607, 4, 7)
    status = r["status"].cpu().numpy()
    assert set(status.tolist()) <= {0, 1, 2, 3} and (status == 0).any()
    table = r["table"].cpu().numpy()
    for i in np.flatnonzero(status == 0):
        p = sh.row_parts(table[i], dims)
        nw, nl, nC, nS, nH = (int(v) for v in p["scalars"][:5])
        assert 5 <= nw <= 15 and 5 <= nl <= 15 and 1 <= nC <= 303 and 1 <= nS <= 607 and 1 <= nH <= 607
        assert int(r["info"]["place_max"][i]) <= sh.PLACE_TRIES
        for name, n in (("heat_diffuse", nH), ("cooler_diffuse", nC)):
            sums = np.array([np.sum(m[:nw, :nl]) for m in p[name][:n]])
            assert np.all(np.abs(sums - 1.0) <= U.sum_one_atol(dims)), (name, np.abs(sums - 1.0).max())
            assert (p[name][:n] >= 0).all()
        assert np.isfinite(table[i]).all() and p["scalars"][10] > 0
    t = sample_tasks_device(2, seed=1, engine=engine)
    env = HVACVecEnv(2, iter_per_step=20, autoreset_mode="disabled")
    env.set_task(t)
    env.reset()
    for _ in range(2):
        out = env.step(np.full((2, dims[2]), 0.5, np.float32))
        assert torch.isfinite(torch.as_tensor(out[1])).all()
        assert torch.isfinite(torch.as_tensor(out[0]["sensor_readings"])).all()
    assert env.check_errors() == 0
    env.close()


def test_bad_arguments_launch_nothing(engine):
    lib = engine.lib
    a = sh.sampler_arguments(config=U.CASES["tiny"])
    dims = a["dims"]
    table = torch.full((2, task_doubles(*dims)), 5.0, dtype=torch.float64, device=engine.device)
    extras = torch.zeros((2, sh.extras_doubles(dims[2], dims[3], dims[4])), dtype=torch.float64, device=engine.device)
    status = torch.full((2,), -7, dtype=torch.int32, device=engine.device)

    def call(dims=dims, null_table=False, n_ambient=None):
        p = ds.params_of(a)
        if n_ambient is not None:
            p.n_ambient = n_ambient
        return lib.xv_anyhvac_sample_tasks(engine.handle, 1, 0, 2, *dims, C.cast(C.byref(p), C.c_void_p),
                                           None if null_table else _lib.ptr(table), _lib.ptr(extras), None, _lib.ptr(status))

    lib.xv_last_error.restype = C.c_char_p
    for kw, word in ((dict(null_table=True), b"table != nullptr"), (dict(dims=(17,) + dims[1:]), b"NW <= HS_MAX_GRID"),
                     (dict(dims=dims[:2] + (321,) + dims[3:]), b"C <= HS_MAX_C"),
                     (dict(dims=dims[:3] + (641,) + dims[4:]), b"S <= HS_MAX_S"), (dict(n_ambient=5), b"n_ambient")):
        assert call(**kw) < 0, kw
        err = lib.xv_last_error()
        assert b"xv_anyhvac_sampler_check: invalid argument" in err and word in err, (kw, err)
    engine.sync()
    assert (status.cpu().numpy() == -7).all() and (table.cpu().numpy() == 5.0).all()      # nothing ran
    assert call() == 0
    engine.sync()
    assert (status.cpu().numpy() != -7).all()


def test_set_task_rejects_tables_of_other_settings(engine):
    t = sample_tasks_device(2, seed=2, config=U.CASES["tiny"], engine=engine)
    env = HVACVecEnv(2, iter_per_step=20)
    with pytest.raises(ValueError):
        env.set_task(t, generate_task=True)
    with pytest.raises(ValueError):
        env.set_task(dict(t, set_upper_bound=30))
    other = HVACVecEnv(2, iter_per_step=20, set_lower_bound=18)
    with pytest.raises(ValueError):
        other.set_task(t)
    gen = sample_tasks_device(2, seed=2, config=U.CASES["tiny"], engine=engine, generate_task=True)
    with pytest.raises(ValueError):
        env.set_task(gen)
    env.set_task(gen, generate_task=True)
    bare = HVACVecEnv(2, iter_per_step=20, device="cuda")      # no index: the tables' cuda:0 is still this env's device
    bare.set_task(t)
    with pytest.raises(ValueError):
        bare.set_task(dict(t, table=t["table"].cpu()))
    bare.close()
    env.close()
    other.close()
