"""The device MetaLangV2 / MetaLangV1 task samplers (csrc/metalang_sampler.hip) against their numpy restatements
(metalang/sampler_host_v2.py, sampler_host_v1.py), against themselves under other launch batches, and end to end through
set_task(tables), generate() and the generators' command lines.

What is equal to what (DESIGN.md §3.6, §3.9 "Tasks made on the device"): V2's n_gram and zero padding exactly, its normals
within the project's device-sampler tolerance (the device's log, sin and cos are not numpy's); V1's offsets and tokens bit
for bit (integers, and fp64 products, quotients and sums only); one launch to any split of it, bit for bit; generate() on
the device tables to generate() on task_dicts_from_device(tables) through the host path, bit for bit."""
import ctypes as C
import pickle

import numpy as np
import pytest
import torch

from metalm_sampler_util import ATOL, RTOL
from xenoverse_amd import _lib
from xenoverse_amd.metalang import (MetaLangV1Batch, MetaLangV2Batch, device_sampler_v1 as d1, device_sampler_v2 as d2,
                                    generator, generator_v1, sample_tasks_v1_device, sample_tasks_v2_device,
                                    sampler_host_v1 as h1, sampler_host_v2 as h2, task_dicts_from_device)
from xenoverse_amd.metalang.host_v1 import check_task_v1
from xenoverse_amd.metalang.task_sampler import TASK_ARRAYS, check_task

pytestmark = pytest.mark.gpu

# (V, E, H), n_gram, tasks: odd element counts, padded slots and a per-task n; the default size; the limits
V2_SHAPES = {"odd": ((33, 5, 7), [2, 3, 5], 5), "default": ((256, 16, 64), 3, 4), "limits": ((1024, 64, 128), 8, 1)}
# (n_vocab, n_patterns, n_gram): the smallest of everything, the defaults, a wide vocabulary under a list, the largest n_gram
V1_SETTINGS = {"min": (2, 1, 1), "default": (64, 10, 64), "list": (100000, 6, [3, 4, 5, 6]), "max_gram": (64, 2, h1.NGRAM_MAX)}


def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else t


@pytest.fixture(scope="module")
def eng():
    from xenoverse_amd.engine import Engine
    e = Engine("cuda:0")
    yield e
    e.close()


# ---- device against host ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("name", list(V2_SHAPES))
def test_v2_device_equals_host(eng, name, seed):
    (V, E, H), n_gram, n = V2_SHAPES[name]
    tick = eng.tick
    dev = sample_tasks_v2_device(n, n_emb=E, n_hidden=H, n_vocab=V, n_gram=n_gram, _lambda=2.5, seed=seed, engine=eng)
    assert eng.tick == tick and eng.error_flags() == 0
    host = h2.sample_tables(n, n_emb=E, n_hidden=H, n_vocab=V, n_gram=n_gram, _lambda=2.5, seed=seed)
    assert _np(dev["n_gram"]).dtype == np.int32 and (_np(dev["n_gram"]) == host["n_gram"]).all()
    assert (_np(dev["_lambda"]) == 2.5).all() and dev["n_gram_max"] == host["n_gram_max"]
    assert dev["stats"]["accepted"] == dev["stats"]["candidates"] == n
    worst = 0.0
    for k in TASK_ARRAYS:
        got, want = _np(dev[k]), host[k]
        assert got.shape == want.shape and got.dtype == np.float64, k
        assert ((got == 0.0) == (want == 0.0)).all(), k      # the padding is exact zeros, and nothing else is
        worst = max(worst, float(np.max(np.abs(got - want) / (ATOL + RTOL * np.abs(want)))))
    print("%s seed %d: worst deviation %.3g of the tolerance (rtol %g, atol %g)" % (name, seed, worst, RTOL, ATOL))
    assert worst <= 1.0
    if name == "odd":
        assert len(set(host["n_gram"].tolist())) > 1 and host["n_gram"].min() < 5      # padded slots and several n occur


def test_v2_writes_nothing_outside_its_arrays(eng):
    """the C entry point on buffers with a guard on either side of every array: odd element counts (V E = 165, H V = 231,
    V = 33) end in a call whose second half must be dropped"""
    (V, E, H), lst, n = V2_SHAPES["odd"]
    NG, G = max(lst), 64
    counts = [n * V * E, n * NG * E * H, n * NG * H, n * H * V, n * V, n]
    assert counts[0] % 2 == 1 and counts[3] % 2 == 1 and counts[4] % 2 == 1
    bufs = [torch.full((c + 2 * G,), -7.0, dtype=torch.float64, device=eng.device) for c in counts]
    grams = torch.full((n + 2 * G,), -7, dtype=torch.int32, device=eng.device)
    _lib.check(eng.lib.xv_metalang_sample_tasks(eng.handle, 0, 0, n, V, E, H, (C.c_int32 * 3)(*lst), 3, NG, 2.5,
                                                *(_lib.ptr(b[G:]) for b in bufs), _lib.ptr(grams[G:])))
    eng.sync()
    host = h2.sample_tables(n, n_emb=E, n_hidden=H, n_vocab=V, n_gram=lst, _lambda=2.5, seed=0)
    for b, c, k in zip(bufs + [grams], counts + [n], TASK_ARRAYS + ("_lambda", "n_gram")):
        b = _np(b)
        assert (b[:G] == -7).all() and (b[G + c:] == -7).all(), k
        np.testing.assert_allclose(b[G:G + c], host[k].reshape(-1), rtol=RTOL, atol=ATOL, err_msg=k)


def _assert_v1_equal(dev, host):
    for k in d1.TABLE_KEYS + ("n_gram",):
        got = _np(dev[k])
        assert got.dtype == host[k].dtype and got.shape == host[k].shape, k
        assert got.tobytes() == host[k].tobytes(), k


@pytest.mark.parametrize("n_tasks", [1, 257])
@pytest.mark.parametrize("name", list(V1_SETTINGS))
def test_v1_device_equals_host_bit_for_bit(eng, name, n_tasks):
    V, nP, n_gram = V1_SETTINGS[name]
    tick = eng.tick
    dev = sample_tasks_v1_device(n_tasks, n_vocab=V, n_patterns=nP, n_gram=n_gram, error_ratio=0.25, seed=n_tasks, engine=eng)
    assert eng.tick == tick and eng.error_flags() == 0
    host = h1.sample_tables(n_tasks, n_vocab=V, n_patterns=nP, n_gram=n_gram, error_ratio=0.25, seed=n_tasks)
    _assert_v1_equal(dev, host)
    assert dev["stats"]["tokens"] == len(host["tokens"]) and dev["n_patterns"] == nP
    lens = np.diff(host["pattern_token_offset"])
    assert lens.min() >= 3 and host["tokens"].min() >= 0 and host["tokens"].max() < V
    if name == "max_gram" and n_tasks > 1:
        assert abs(lens.mean() - h1.NGRAM_MAX) < 5.0 * np.sqrt(h1.NGRAM_MAX / len(lens))


# ---- batch independence -----------------------------------------------------------------------------------------------
def test_v2_tasks_do_not_depend_on_the_launch_batch(eng):
    kw = dict(n_emb=5, n_hidden=7, n_vocab=33, n_gram=[2, 3, 5], seed=4, engine=eng)
    whole = sample_tasks_v2_device(70, **kw)
    for batch in (2, 64):
        part = sample_tasks_v2_device(70, batch=batch, **kw)
        assert part["stats"]["batch"] == batch
        for k in d2.TABLE_KEYS:
            assert torch.equal(whole[k], part[k]), (batch, k)


def test_v1_tasks_do_not_depend_on_the_launch_batch(eng):
    kw = dict(n_vocab=100, n_patterns=6, n_gram=[3, 4, 5, 6], seed=4, engine=eng)
    whole = sample_tasks_v1_device(70, **kw)
    for batch in (2, 64):
        part = sample_tasks_v1_device(70, batch=batch, **kw)
        for k in d1.TABLE_KEYS + ("n_gram",):
            assert torch.equal(whole[k], part[k]), (batch, k)


# ---- end to end -------------------------------------------------------------------------------------------------------
def _generate_v2(tasks, n_group, index=None, L=64):
    gen = MetaLangV2Batch(n_group, 2, seed=3, env_id_base=7)
    try:
        gen.set_task(tasks, index)
        tokens, logp = gen.generate(L, return_logp=True)
        borrowed = gen._tables[0].data_ptr()
        out = tokens.cpu(), logp.cpu()
        assert gen.check_errors() == 0
        return out, borrowed
    finally:
        gen.close()


def _generate_v1(tasks, n_seq, index=None, L=97):
    gen = MetaLangV1Batch(n_seq, seed=3, env_id_base=7)
    try:
        gen.set_task(tasks, index)
        out = tuple(t.cpu() for t in gen.generate(L, return_kinds=True))
        borrowed = gen._tables[2].data_ptr()
        assert gen.check_errors() == 0
        return out, borrowed
    finally:
        gen.close()


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def tables_v2(eng):
    t = sample_tasks_v2_device(5, n_emb=16, n_hidden=16, n_vocab=64, n_gram=[2, 3, 5], seed=0, engine=eng)
    assert sorted(set(_np(t["n_gram"]).tolist())) == [2, 3, 5]
    return t


@pytest.fixture(scope="module")
def tables_v1(eng):
    return sample_tasks_v1_device(257, n_vocab=32, n_patterns=4, n_gram=[6, 8, 20], error_ratio=0.2, seed=0, engine=eng)


def test_v2_generate_on_device_tables_equals_the_host_path(tables_v2):
    dicts = task_dicts_from_device(tables_v2)
    assert [check_task(t)[3] for t in dicts] == _np(tables_v2["n_gram"]).tolist()
    got, borrowed = _generate_v2(tables_v2, 5)
    want, _ = _generate_v2(dicts, 5)
    assert borrowed == tables_v2["word_emb"].data_ptr()      # no copy
    assert tuple(got[0].shape) == (5, 2, 65) and tuple(got[1].shape) == (5, 2, 64)
    assert _same(got, want)


def test_v1_generate_on_device_tables_equals_the_host_path(tables_v1):
    dicts = task_dicts_from_device(tables_v1)
    assert len(dicts) == 257 and all(len(check_task_v1(t)[0]) == 4 for t in dicts)
    got, borrowed = _generate_v1(tables_v1, 257)
    want, _ = _generate_v1(dicts, 257)
    assert borrowed == tables_v1["tokens"].data_ptr()      # no copy
    assert tuple(got[0].shape) == (257, 97) and got[2].dtype == torch.uint8
    assert _same(got, want)


def test_v2_default_index_rules(eng, tables_v2):
    dicts = task_dicts_from_device(tables_v2)
    one = sample_tasks_v2_device(1, n_emb=16, n_hidden=16, n_vocab=64, n_gram=[2, 3, 5], seed=0, engine=eng)
    assert _same(_generate_v2(one, 5)[0], _generate_v2(dicts[:1], 5)[0])                    # one task: every group's
    assert _same(_generate_v2(tables_v2, 5)[0], _generate_v2(dicts, 5, np.arange(5))[0])    # n_group tasks: task g
    index = [4, 0, 3]
    assert _same(_generate_v2(tables_v2, 3, index)[0], _generate_v2(dicts, 3, index)[0])
    with pytest.raises(ValueError, match="5 tasks for 3 groups: give group_task_index"):
        _generate_v2(tables_v2, 3)
    with pytest.raises(ValueError, match="group_task_index must be"):
        _generate_v2(tables_v2, 3, [0, 1, 5])


def test_v1_default_index_rules(eng, tables_v1):
    dicts = task_dicts_from_device(tables_v1)
    one = sample_tasks_v1_device(1, n_vocab=32, n_patterns=4, n_gram=[6, 8, 20], error_ratio=0.2, seed=0, engine=eng)
    assert _same(_generate_v1(one, 5)[0], _generate_v1(dicts[:1], 5)[0])
    assert _same(_generate_v1(tables_v1, 257)[0], _generate_v1(dicts, 257, np.arange(257))[0])
    index = [256, 0, 100]
    assert _same(_generate_v1(tables_v1, 3, index)[0], _generate_v1(dicts, 3, index)[0])
    with pytest.raises(ValueError, match="257 tasks for 3 sequences: give seq_task_index"):
        _generate_v1(tables_v1, 3)
    with pytest.raises(ValueError, match="seq_task_index must be"):
        _generate_v1(tables_v1, 3, [0, 1, 257])


# ---- command lines ----------------------------------------------------------------------------------------------------
def test_v2_command_line_with_the_device_sampler(tmp_path):
    common = ["--sampler", "device", "--samples", "3", "--sequence_length", "16", "--vocab_size", "32", "--seed", "5"]
    out = str(tmp_path / "seq.npy")
    generator.main(common + ["--output_type", "npy", "--output", out])
    tokens = np.load(out)
    assert tokens.shape == (3, 17) and tokens.dtype == np.int32 and tokens.min() >= 0 and tokens.max() < 32
    generator.main(common + ["--sample_type", "tasks", "--output", str(tmp_path / "tasks")])
    with open(str(tmp_path / "tasks.pkl"), "rb") as f:
        tasks = pickle.load(f)
    assert len(tasks) == 3 and all(isinstance(t["word_emb"], np.ndarray) for t in tasks)
    assert all(check_task(t)[:3] == (32, 16, 16) and check_task(t)[3] in (3, 4, 5, 6) for t in tasks)


def test_v1_command_line_with_the_device_sampler(tmp_path):
    common = ["--sampler", "device", "--samples", "3", "--sequence_length", "16", "--vocab_size", "32", "--seed", "5"]
    out = str(tmp_path / "seq.npy")
    generator_v1.main(common + ["--output_type", "npy", "--output", out])
    data = np.load(out)
    assert data.shape == (3, 2, 16) and data.dtype == np.int32 and data.min() >= 0 and data.max() < 32
    generator_v1.main(common + ["--sample_type", "tasks", "--output", str(tmp_path / "tasks")])
    with open(str(tmp_path / "tasks.pkl"), "rb") as f:
        tasks = pickle.load(f)
    assert len(tasks) == 3
    for t in tasks:
        pats, V, e = check_task_v1(t)
        assert (len(pats), V, e) == (10, 32, 0.20) and t["n_gram"] in (3, 4, 5, 6)
