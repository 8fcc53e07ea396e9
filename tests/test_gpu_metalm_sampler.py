"""The device MetaLMV3 task sampler (xv_metalm_sample_tasks, csrc/metalm_sampler.hip) against its numpy restatement
(metalang/sampler_host.py), against the existing MetaLMV3 kernels run on its own tables, against itself under other launch
geometries, and end to end through set_task, stream() and the generator.  Shapes, seeds and tolerances:
tests/metalm_sampler_util.py.

What is bit-equal to what: emb to numpy's layer_norm of the device's own enc_w; the fused protocol to
the reset / policy / step kernels on the same tables; one launch to any split of it.  The weights themselves are compared
with the host's within the project's device-sampler tolerance (the device's log, sin and cos are not numpy's), so the host
protocol is run on the DEVICE's tables and compared in the band of tests/test_gpu_metalm.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import metalm_sampler_util as U
from xenoverse_amd import _lib
from xenoverse_amd.metalang import (MetaLMV3VecEnv, device_sampler as ds, generate_data_v3_batch, sample_candidates,
                                    sample_tasks_device, sampler_host as sh, task_dicts_from_device)
from xenoverse_amd.metalang.lm_env import XV_DEVERR_LENGTH
from xenoverse_amd.metalang.lm_host import layer_norm

pytestmark = pytest.mark.gpu

XV_DEVERR_NONFINITE = 2      # include/xeno.h
INFO_KEYS = ("ppl", "query", "query_len", "answer", "answer_len", "flags")
ALL_KEYS = ds.TASK_KEYS + ("status",) + INFO_KEYS


def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else t


@pytest.fixture(scope="module")
def eng():
    from xenoverse_amd.engine import Engine
    e = Engine("cuda:0")
    yield e
    e.close()


_RUNS = {}


def _run(eng, name):
    """the shape's launch, once: every candidate's tables and records"""
    if name not in _RUNS:
        (V, E, H), n = U.SHAPES[name]
        tick = eng.tick
        r = sample_candidates(eng, U.SEEDS[name], U.CAND_BASE, n, V, E, H, U.MAX_LEN, info=True)
        eng.sync()
        assert eng.tick == tick and eng.error_flags() == 0      # the call neither advances the tick nor flags the engine
        _RUNS[name] = r
    return _RUNS[name]


def _protocol(tables, n, max_len, seed, base):
    """reset, policy(1e4), step(cached), policy(1e-6), step(cached) of the existing kernels on the given tables"""
    env = MetaLMV3VecEnv(n, max_len=max_len, seed=seed, env_id_base=base)
    try:
        env.set_task(tables)
        env.engine.tick = 0
        query, query_len = env.reset()
        out = dict(query=query, query_len=query_len, answer=[], answer_len=[], reward=[], ppl=[])
        for T in (1e4, 1e-6):
            answer, answer_len = env.policy(T)
            _, reward, _, _, info = env.step(answer, answer_len, cached=True)
            out["answer"].append(answer)
            out["answer_len"].append(answer_len)
            out["reward"].append(reward)
            out["ppl"].append(torch.stack([info["ppl"], info["ppl_min"], info["ppl_max"]], 1))
        out["flags"] = env.check_errors()
    finally:
        env.close()
    return out


def _assert_protocol_equal(r, p):
    """bit for bit: query, both answers, all six ppls, both rewards"""
    assert torch.equal(r["query"], p["query"]) and torch.equal(r["query_len"], p["query_len"])
    for k in (0, 1):
        assert torch.equal(r["answer"][:, k], p["answer"][k]) and torch.equal(r["answer_len"][:, k], p["answer_len"][k])
        assert torch.equal(r["ppl"][:, k], p["ppl"][k]), k
    assert torch.equal(r["reward_low"], p["reward"][0]) and torch.equal(r["reward_high"], p["reward"][1])
    want = [sh.status_of(lo, hi) for lo, hi in zip(_np(p["reward"][0]), _np(p["reward"][1]))]
    assert _np(r["status"]).tolist() == want
    assert not (p["flags"] & XV_DEVERR_NONFINITE) and not (_np(r["flags"]) & XV_DEVERR_NONFINITE).any()


@pytest.mark.parametrize("name", U.NAMES)
def test_weights_equal_the_host(eng, name):
    r = _run(eng, name)
    (V, E, H), n = U.SHAPES[name]
    hosts = U.host_candidates(name)
    worst = 0.0
    for i, h in enumerate(hosts):
        a = h["arrays"]
        for key, want in (("enc_w", a["enc_w"]), ("w_h_t", a["rnn_w"].T), ("b_h", a["rnn_b"]), ("w_d_t", a["dec_w"].T)):
            got = _np(r[key][i])
            assert got.shape == want.shape
            worst = max(worst, float(np.max(np.abs(got - want) / (U.ATOL + U.RTOL * np.abs(want)))))
            assert np.allclose(got, want, rtol=U.RTOL, atol=U.ATOL), (i, key)
    print("%s: worst deviation of a weight from the host, in units of atol + rtol |w|: %.3e" % (name, worst))
    b_d = _np(r["b_d"])
    assert b_d.shape == (n, V) and not b_d.any() and not np.signbit(b_d).any()
    assert _np(r["candidate"]).tolist() == list(range(U.CAND_BASE, U.CAND_BASE + n))


@pytest.mark.parametrize("name", U.NAMES)
def test_emb_is_numpys_layer_norm_of_the_devices_enc_w(eng, name):
    r = _run(eng, name)
    enc_w, emb = _np(r["enc_w"]), _np(r["emb"])
    for i in range(len(emb)):
        assert np.array_equal(emb[i], layer_norm(np.ascontiguousarray(enc_w[i].T))), i
    assert np.array_equal(emb[0], sh.layer_norm_rows(enc_w[0].T))


@pytest.mark.parametrize("name", U.NAMES)
def test_fused_protocol_is_the_existing_kernels(eng, name):
    r = _run(eng, name)
    (V, E, H), n = U.SHAPES[name]
    p = _protocol(r, n, U.MAX_LEN, U.SEEDS[name], U.CAND_BASE)
    st = _np(r["status"])
    print("%s: status histogram %s" % (name, np.bincount(st, minlength=4).tolist()))
    _assert_protocol_equal(r, p)
    assert (st == 0).any() and (st != 0).any()      # the seed was picked so that both occur


@pytest.mark.parametrize("name", U.NAMES)
def test_host_protocol_on_the_devices_tables(eng, name):
    r = {k: _np(v) for k, v in _run(eng, name).items()}
    (V, E, H), n = U.SHAPES[name]
    hosts = [sh.candidate_host(U.SEEDS[name], U.CAND_BASE + i, V, E, H, U.MAX_LEN, arrays=sh.arrays_of_tables(r, i))
             for i in range(n)]
    r_tol = 1e3 * U.PPL_RTOL
    margin = min(min(h["margin"], h["gap"]) for h in hosts)
    on_threshold = [i for i, h in enumerate(hosts)
                    if abs(h["reward"][0]) <= r_tol or abs(h["reward"][1] - 2.0) <= r_tol * 2.0]
    print("%s: the host's smallest margin / gap %.3e, candidates with a reward on a threshold: %s" % (name, margin, on_threshold))
    assert margin >= U.TAU and not on_threshold      # the cap on left-out candidates is zero
    worst_ppl = worst_r = 0.0
    for i, h in enumerate(hosts):
        assert r["query"][i, :r["query_len"][i]].tolist() == h["query"], i
        for k in (0, 1):
            assert r["answer"][i, k, :r["answer_len"][i, k]].tolist() == h["answer"][k], (i, k)
            worst_ppl = max(worst_ppl, float(np.max(np.abs(r["ppl"][i, k] - h["ppl"][k]) / np.abs(h["ppl"][k]))))
        for got, want in ((r["reward_low"][i], h["reward"][0]), (r["reward_high"][i], h["reward"][1])):
            worst_r = max(worst_r, abs(got - want) / max(1.0, abs(want)))
        assert r["status"][i] == h["status"], i
        assert bool(r["flags"][i] & XV_DEVERR_LENGTH) == h["cut"], i
    print("%s: worst relative deviation of a ppl mean %.3e, of a reward %.3e" % (name, worst_ppl, worst_r))
    assert worst_ppl <= U.PPL_RTOL
    assert worst_r <= r_tol


@pytest.mark.parametrize("name", U.NAMES)
def test_one_launch_equals_two_launches_of_halves(eng, name):
    r = _run(eng, name)
    (V, E, H), n = U.SHAPES[name]
    half = n // 2
    parts = [sample_candidates(eng, U.SEEDS[name], U.CAND_BASE + lo, half, V, E, H, U.MAX_LEN, info=True)
             for lo in (0, half)]
    for k in ALL_KEYS:
        assert torch.equal(torch.cat([p[k] for p in parts]), r[k]), k


def test_tasks_do_not_depend_on_the_batch():
    (V, E, H), _ = U.SHAPES["min_vocab"]      # where most candidates are rejected
    a, b = (sample_tasks_device(24, V, E, H, seed=U.SEEDS["min_vocab"], batch=batch, max_len=U.MAX_LEN) for batch in (7, 64))
    for k in ds.TASK_KEYS:
        assert a[k].shape[0] == 24 and torch.equal(a[k], b[k]), k
    assert a["stats"]["status"] == b["stats"]["status"] and a["stats"]["candidates"] == b["stats"]["candidates"]
    assert a["stats"]["accepted"] == 24 and a["stats"]["candidates"] == int(a["candidate"][-1]) + 1 > 24
    assert (a["stats"]["batch"], b["stats"]["batch"]) == (7, 64)
    assert bool((a["reward_low"] <= 0).all()) and bool((a["reward_high"] >= 2).all())
    assert (a["vocabulary"], a["embedding"], a["hidden"]) == (V, E, H) and a["function_vocabulary"]["s"] == 0
    with pytest.raises(RuntimeError):
        sample_tasks_device(24, V, E, H, seed=U.SEEDS["min_vocab"], batch=8, max_len=U.MAX_LEN, max_candidates=16)


@pytest.mark.parametrize("name", ["min_vocab", "default"])
def test_a_cut_pass_flags_its_candidate_and_not_the_engine(eng, name):
    (V, E, H), n = U.SHAPES[name]
    seed, max_len = U.SEEDS[name], 4
    r = sample_candidates(eng, seed, U.CAND_BASE, n, V, E, H, max_len, info=True)
    eng.sync()
    assert eng.error_flags() == 0
    flags = _np(r["flags"])
    assert not (flags & ~XV_DEVERR_LENGTH).any() and (flags & XV_DEVERR_LENGTH).any()
    host = {k: _np(v) for k, v in r.items()}
    hosts = [sh.candidate_host(seed, U.CAND_BASE + i, V, E, H, max_len, arrays=sh.arrays_of_tables(host, i)) for i in range(n)]
    assert min(min(h["margin"], h["gap"]) for h in hosts) >= U.TAU
    assert [bool(f & XV_DEVERR_LENGTH) for f in flags] == [h["cut"] for h in hosts]
    if name == "min_vocab":
        assert not all(h["cut"] for h in hosts)      # both kinds occur
    p = _protocol(r, n, max_len, seed, U.CAND_BASE)
    assert p["flags"] == XV_DEVERR_LENGTH      # the existing kernels flag their engine
    _assert_protocol_equal(r, p)
    again = sample_candidates(eng, seed, U.CAND_BASE, n, V, E, H, max_len, info=True)      # and the next call works
    for k in ALL_KEYS:
        assert torch.equal(again[k], r[k]), k
    assert eng.error_flags() == 0


def test_end_to_end_tables_equal_task_dicts():
    n, L, max_len = 32, 256, 256
    tables = sample_tasks_device(n, seed=11, max_len=max_len)
    assert tables["stats"]["accepted"] == n and not _np(tables["candidate"] < 0).any()
    tasks = task_dicts_from_device(tables)
    streams = []
    for src in (tables, tasks):
        env = MetaLMV3VecEnv(n, max_len=max_len, seed=5)
        try:
            env.set_task(src)
            if src is tables:      # borrowed as they are
                assert [t.data_ptr() for t in env._tables[:5]] == [tables[k].data_ptr() for k in ds.TABLE_KEYS]
            query, query_len = env.reset()
            data, label, info = env.stream("QAR", L)
            streams.append([query, query_len, data, label, info["filled"], info["rounds"], info["reward"], info["t_index"]])
            assert env.check_errors() & ~XV_DEVERR_LENGTH == 0
        finally:
            env.close()
    for x, y in zip(*streams):
        assert torch.equal(x, y)
    a = generate_data_v3_batch(tables, "QARA", 128, seed=3, max_len=max_len)
    b = generate_data_v3_batch(tasks, "QARA", 128, seed=3, max_len=max_len)
    assert a.shape == (n, 2, 128) and np.array_equal(a, b) and a.any()


def test_refusals_are_those_of_create(eng):
    d = eng.device
    buf = [torch.zeros(64 * 1024, dtype=torch.float64, device=d) for _ in range(6)]
    status = torch.zeros(4, dtype=torch.int32, device=d)
    fun = (C.c_int32 * 10)(*range(1, 11))

    def call(n_cand=4, V=32, E=16, H=32, max_len=64, stop=0, tokens=fun, n_fun=10, base=0):
        return eng.lib.xv_metalm_sample_tasks(eng.handle, 1, base, n_cand, V, E, H, max_len, stop, tokens, n_fun,
                                              *(_lib.ptr(b) for b in buf), _lib.ptr(status), *([None] * 7))
    assert call() == 0
    eng.sync()
    for kw in (dict(V=11), dict(V=257), dict(E=0), dict(E=65), dict(H=0), dict(H=129), dict(max_len=0), dict(max_len=1025)):
        assert call(**kw) == _lib.XV_ERR_UNSUPPORTED, kw
    bad = (C.c_int32 * 10)(*([1] * 9 + [32]))
    for kw in (dict(n_cand=0), dict(stop=32), dict(stop=-1), dict(tokens=bad), dict(tokens=None), dict(n_fun=-1), dict(base=-1)):
        assert call(**kw) == _lib.XV_ERR_INVALID, kw
    with pytest.raises(_lib.XenoError) as ex:
        _lib.check(call(V=300))
    assert "n_vocab = 300 is outside the supported range 12 .. 256" in str(ex.value)
    assert eng.error_flags() == 0
