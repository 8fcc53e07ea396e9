"""The host half of the task path, without a device: the accepted-candidate collector the three device samplers share
(xenoverse_amd/device_sampling.py), the env -> task mapping every VecEnv.set_task uses (vector.env_task_map) and the one
LinDS table packer behind build_tables and build_tables_device (linds/tables.py)."""
import numpy as np
import pytest
import torch

from xenoverse_amd.device_sampling import collect_accepted, sampler_stats
from xenoverse_amd.vector import env_task_map

from util import golden_files, load_linds_golden

STATUS = ("accepted", "odd", "even")


def _status(c):
    c = np.asarray(c, np.int64)
    return np.where(((c * 2654435761 % 2**32) >> 7) % 3 == 0, 0, 1 + c % 2).astype(np.int32)


def _fake_launch(calls, with_info):
    """a sampler's sample_candidates on CPU tensors: payload x[c] = c, y[c] = (c, c^2); status in a tensor or in info records"""
    def launch(base, n):
        calls.append((base, n))
        c = np.arange(base, base + n, dtype=np.int64)
        r = dict(x=torch.from_numpy(c.copy()), y=torch.from_numpy(np.stack([c, c * c], 1)))
        if with_info:
            info = np.zeros(n, np.dtype([("status", "<i4"), ("cand", "<i8")]))
            info["status"], info["cand"] = _status(c), c
            r["info"] = info
        else:
            r["status"] = torch.from_numpy(_status(c))
        return r
    return launch


def test_the_fake_statuses_are_what_the_cases_assume():
    st = _status(np.arange(4096))
    assert np.nonzero(st == 0)[0][:5].tolist() == [0, 1, 4, 7, 10]
    assert abs((st == 0).mean() - 0.334) < 0.0005


@pytest.mark.parametrize("with_info", [False, True])
@pytest.mark.parametrize("batch", [1, 5, 7, 64, 1000])
@pytest.mark.parametrize("n_tasks", [1, 10, 23, 200])
def test_collector_returns_the_first_accepted_whatever_the_batch(n_tasks, batch, with_info):
    st = _status(np.arange(4096))
    want = np.nonzero(st == 0)[0][:n_tasks]
    calls = []
    got, info, hist = collect_accepted(_fake_launch(calls, with_info), n_tasks, batch, ("x", "y"), STATUS)
    assert got["x"].dtype == torch.int64 and got["x"].tolist() == want.tolist()
    assert np.array_equal(got["y"].numpy(), np.stack([want, want * want], 1))
    assert np.array_equal(hist, np.bincount(st[: want[-1] + 1], minlength=3)) and hist[0] == n_tasks
    assert calls == [(b, batch) for b in range(0, int(want[-1]) + 1, batch)]      # no launch beyond the batch that completes it
    if with_info:
        assert info["cand"].tolist() == want.tolist() and not info["status"].any()
    else:
        assert info is None
    stats = sampler_stats(hist, STATUS, batch, 0.0, extra=7)
    assert list(stats) == ["candidates", "accepted", "seconds", "status", "batch", "extra"]
    assert (stats["candidates"], stats["accepted"], stats["batch"]) == (int(want[-1]) + 1, n_tasks, batch)
    assert stats["status"] == {k: int(h) for k, h in zip(STATUS, hist)}


@pytest.mark.parametrize("with_info", [False, True])
def test_collector_max_candidates_is_checked_per_batch(with_info):
    with pytest.raises(RuntimeError) as ex:
        collect_accepted(_fake_launch([], with_info), 23, 16, ("x", "y"), STATUS, max_candidates=32)
    assert str(ex.value) == "only 12 of 23 tasks accepted within 32 candidates"
    # the check is batch-granular: 17 candidates allowed, 32 launched, and the 11th accepted (candidate 28) is found
    got, _, _ = collect_accepted(_fake_launch([], with_info), 11, 16, ("x",), STATUS, max_candidates=17)
    assert got["x"][-1] == 28


def test_env_task_default_split_and_checks():
    t = env_task_map(8, 4, None, "cpu")
    assert t.dtype == torch.int32 and t.is_contiguous() and t.tolist() == [0, 0, 1, 1, 2, 2, 3, 3]
    with pytest.raises(ValueError):
        env_task_map(8, 3, None, "cpu")
    for bad in ([0, 1, 2, 3], [[0, 1, 2, 3, 0, 1, 2, 3]], [0, 1, 2, 3, 0, 1, 2, -1], [0, 1, 2, 3, 0, 1, 2, 4]):
        with pytest.raises(ValueError):
            env_task_map(8, 4, bad, "cpu")
    idx = [3, 3, 0, 1, 2, 2, 1, 0]
    strided = torch.tensor([idx, idx], dtype=torch.int64).t().contiguous()[:, 0]      # int64 and not contiguous
    assert not strided.is_contiguous()
    for given in (idx, np.array(idx), np.array(idx, np.int64), strided):
        t = env_task_map(8, 4, given, "cpu")
        assert t.dtype == torch.int32 and t.is_contiguous() and t.device.type == "cpu" and t.tolist() == idx


def test_alloc_follows_its_spec():
    """VectorEnv._alloc on a stand-in with the two attributes it reads: names in spec order, [lead..., N, tail...] shapes,
    filled entries filled (LinDS final_obs: zero rows for envs that go on; AnyMDP token final_obs: -1)"""
    from types import SimpleNamespace
    from xenoverse_amd.vector import VectorEnv
    spec = [("obs", torch.float32, (5,)), ("reward", torch.float64, ()), ("final_obs", torch.float32, (5,), 0),
            ("tok", torch.int32, (2,), -1), ("flag", torch.uint8, ())]
    for lead in ((), (3,), (2, 3)):
        out = VectorEnv._alloc(SimpleNamespace(num_envs=7, device=torch.device("cpu")), spec, lead)
        assert list(out) == [f[0] for f in spec]
        for f in spec:
            assert out[f[0]].shape == lead + (7,) + f[2] and out[f[0]].dtype == f[1] and out[f[0]].is_contiguous()
        assert not out["final_obs"].any() and bool((out["tok"] == -1).all())


class _NoEngine(object):
    def sync(self):
        pass


@pytest.mark.parametrize("pads", [{}, dict(pad_action_dim=16, pad_observation_dim=32, pad_command_dim=32)])
def test_linds_device_builder_packs_what_the_host_builder_packs(pads, monkeypatch):
    """build_tables_device with a host stand-in for its one zero-order-hold launch (the host's own discretisation of each
    task, rounded once to float32, after checking that the launch was given the tasks' matrices zero-padded) returns
    build_tables' arrays exactly, key by key: the two builders share one packer"""
    from xenoverse_amd.linds import build_tables, device_sampler
    from xenoverse_amd.linds.tables import build_dynamics_matrices
    files = golden_files("linds_16x8x8_")[:4] + golden_files("linds_32x8x8_0") + (golden_files("lindswide_") if pads else [])
    assert len(files) == (7 if pads else 5)
    tasks = [load_linds_golden(p)[1] for p in files]
    assert {str(t["target_type"]) for t in tasks} == {"static_target", "dynamic_target"}

    def zoh(engine, A, B, X, ns, dt=0.1, dense=False):
        n, NS, NA = len(tasks), A.shape[1], B.shape[2]
        out = dict(phiT=np.zeros((n, NS, NS), np.float32), gamT=np.zeros((n, NA, NS), np.float32), xt=np.zeros((n, NS), np.float32))
        for i, t in enumerate(tasks):
            s, a = int(t["state_dim"]), int(t["action_dim"])
            a64, b64, x64 = (np.asarray(t[k], np.float64) for k in ("ld_A", "ld_B", "ld_X"))
            assert ns[i] == s
            for given, mine in ((A[i], a64), (B[i], b64), (X[i], x64)):
                padded = np.zeros_like(given)
                padded[tuple(slice(0, k) for k in mine.shape)] = mine
                assert np.array_equal(given, padded)
            phi, gam, xdt = build_dynamics_matrices(a64, b64, x64, dt)
            out["phiT"][i, :s, :s], out["gamT"][i, :a, :s], out["xt"][i, :s] = phi.T, gam.T, xdt
        out["status"] = np.zeros(n, np.int32)
        return {k: torch.from_numpy(v) for k, v in out.items()}

    monkeypatch.setattr(device_sampler, "build_zoh_device", zoh)
    host = build_tables(tasks, **pads)
    dev = device_sampler.build_tables_device(tasks, _NoEngine(), **pads)
    assert list(dev) == list(host)
    for k in host:
        if isinstance(host[k], np.ndarray):
            assert dev[k].dtype == host[k].dtype and np.array_equal(dev[k], host[k]), k
        else:
            assert dev[k] == host[k], k
    assert host["phiT"].any() and host["gamT"].any() and host["four_coef"].any() and host["cmd0"].any()
