"""MetaLangV1 on the device (csrc/metalang_v1.hip: MetaLangV1Batch, MetaLangV1) against the reference's recorded runs
(tests/golden/metalang_v1_*.npz), against the host restatement (xenoverse_amd/metalang/host_v1.py) and against itself.
Integer work and two fp64 comparisons: every equality is exact."""
import ctypes as C
import random

import numpy as np
import pytest

from metalang_v1_util import DRAWS, FILES, by_name, draws_of, fixture_id, load
from util import to_np as _np
from xenoverse_amd import _lib
from xenoverse_amd.metalang import MetaLangV1, MetaLangV1Batch, MetaLangV1Host, TaskSamplerV1

pytestmark = pytest.mark.gpu


def _run(gen, L, draws=None):
    f, lab, kinds, n_seg = gen.generate(L, draws=draws, return_kinds=True)
    assert str(f.dtype) == "torch.int32" and str(lab.dtype) == "torch.int32" and str(kinds.dtype) == "torch.uint8"
    assert tuple(f.shape) == tuple(lab.shape) == tuple(kinds.shape) == (gen.n_seq, L)
    return _np(f), _np(lab), _np(kinds), _np(n_seg)


def _equal(dev, host):
    for a, k in zip(dev, ("features", "labels", "kinds", "n_segments")):
        assert np.array_equal(a, host[k]), (k, np.argwhere(a != host[k])[:5])


@pytest.mark.parametrize("path", FILES, ids=fixture_id)
def test_reference_replay(path):
    g, task = load(path)
    B, L = int(g["B"]), int(g["L"])
    gen = MetaLangV1Batch(B)
    gen.set_task(task)
    f, lab, kinds, n_seg = _run(gen, L, draws_of(g))
    assert np.array_equal(f, g["features"]), np.argwhere(f != g["features"])[:5]
    assert np.array_equal(lab, g["labels"]), np.argwhere(lab != g["labels"])[:5]
    assert np.array_equal(n_seg, g["n_segments"])
    _equal((f, lab, kinds, n_seg), MetaLangV1Host(task).run(L, batch=B, draws=draws_of(g)))
    assert gen.check_errors() == 0
    gen.close()


MIXED = [dict(n_vocab=16, n_patterns=3, n_gram=4, error_ratio=0.1), dict(n_vocab=300, n_patterns=7, n_gram=9, error_ratio=0.5),
         dict(n_vocab=70000, n_patterns=1, n_gram=30, error_ratio=0.9)]


def _mixed_case(L=150, seed=40):
    """8 sequences over 3 tasks in a shuffled order, their draws from the host restatement over a RandomState"""
    tasks = [TaskSamplerV1(seed=seed + k, **kw) for k, kw in enumerate(MIXED)]
    sti = np.random.RandomState(seed).permutation(np.arange(8) % 3).astype(np.int32)
    per = [MetaLangV1Host(tasks[t]).run(L, rng=np.random.RandomState(seed + 10 + s)) for s, t in enumerate(sti)]
    n_slot = max(r["draws"]["pattern_index"].shape[1] for r in per)
    draws = {k: np.concatenate([r["draws"][k] for r in per]) for k in DRAWS[1:]}
    draws["pattern_index"] = np.concatenate([np.pad(r["draws"]["pattern_index"], ((0, 0), (0, n_slot - r["draws"]["pattern_index"].shape[1])))
                                             for r in per])
    host = {k: np.concatenate([r[k] for r in per]) for k in ("features", "labels", "kinds", "n_segments")}
    return tasks, sti, draws, host


def test_mixed_tasks_in_one_launch():
    L = 150
    tasks, sti, draws, host = _mixed_case(L)
    gen = MetaLangV1Batch(8)
    gen.set_task(tasks, seq_task_index=sti)
    whole = _run(gen, L, draws)
    _equal(whole, host)
    assert gen.check_errors() == 0
    gen.close()
    for t in range(3):      # the per-task runs
        rows = np.flatnonzero(sti == t)
        part = MetaLangV1Batch(len(rows))
        part.set_task(tasks[t])
        got = _run(part, L, {k: np.ascontiguousarray(v[rows]) for k, v in draws.items()})
        for a, b in zip(got, whole):
            assert np.array_equal(a, b[rows])
        assert part.check_errors() == 0
        part.close()


def _words(engine, seed, ids, tick, purpose, sub):
    """Philox words of the documented layout (include/xeno.h, MetaLangV1): counter = {id lo, id hi, tick lo, purpose | tick hi
    << 8}, key = {seed lo, seed hi ^ (0x80000000 | sub)} -> int64[n, 4] holding uint32 values"""
    n = len(ids)
    ctr = np.stack([ids & 0xFFFFFFFF, ids >> np.uint64(32), np.full(n, tick & 0xFFFFFFFF, np.uint64),
                    np.full(n, purpose | ((tick >> 32) << 8), np.uint64)], axis=1).astype(np.int64)
    key = [seed & 0xFFFFFFFF, ((seed >> 32) & 0xFFFFFFFF) ^ (0x80000000 | sub)]
    return _np(engine.philox(ctr, key)).astype(np.int64) & 0xFFFFFFFF


def _philox_draws(engine, seed, first_seq, tick, L, n_patterns, n_vocab, n_slot):
    """the draws a free-running call makes: purposes 10 (segment k: sub k >> 2, word k & 3), 11 (value of position q: sub
    q >> 2, word q & 3), 12 and 13 (u_noise, u_mask of q: sub q >> 1, words 0,1 or 2,3); integers (w * n) >> 32, uniforms
    ((a >> 5) * 2^26 + (b >> 6)) / 2^53"""
    n = len(n_patterns)
    ids = first_seq + np.arange(n, dtype=np.uint64)
    nP, V = np.asarray(n_patterns, np.uint64), np.asarray(n_vocab, np.uint64)
    pi = np.zeros((n, n_slot), np.int32)
    for sub in range((n_slot + 3) // 4):
        w = _words(engine, seed, ids, tick, 10, sub).astype(np.uint64)
        for j in range(4):
            if 4 * sub + j < n_slot:
                pi[:, 4 * sub + j] = (w[:, j] * nP) >> np.uint64(32)
    nv = np.zeros((n, L + 1), np.int32)
    for sub in range((L + 4) // 4):
        w = _words(engine, seed, ids, tick, 11, sub).astype(np.uint64)
        for j in range(4):
            if 4 * sub + j <= L:
                nv[:, 4 * sub + j] = (w[:, j] * V) >> np.uint64(32)
    u = {12: np.zeros((n, L + 1)), 13: np.zeros((n, L + 1))}
    for purpose in (12, 13):
        for sub in range((L + 2) // 2):
            w = _words(engine, seed, ids, tick, purpose, sub)
            for odd in (0, 1):
                if 2 * sub + odd <= L:
                    a, b = w[:, 2 * odd], w[:, 2 * odd + 1]
                    u[purpose][:, 2 * sub + odd] = ((a >> 5) * 67108864.0 + (b >> 6)) / 9007199254740992.0
    return dict(pattern_index=pi, noise_value=nv, u_noise=u[12], u_mask=u[13])


def _host_rows(tasks, sti, L, draws):
    per = [MetaLangV1Host(tasks[t]).run(L, draws={k: v[s:s + 1] for k, v in draws.items()}) for s, t in enumerate(sti)]
    return {k: np.concatenate([r[k] for r in per]) for k in ("features", "labels", "kinds", "n_segments")}


@pytest.mark.parametrize("L,n_seq", [(70, 6), (1029, 2)])
def test_free_running_draws(L, n_seq):
    seed, base = (7 << 32) | 7654321, 3000
    tasks = [TaskSamplerV1(seed=60 + k, **kw) for k, kw in enumerate(MIXED)]
    sti = (np.arange(n_seq) % 3).astype(np.int32)
    gen = MetaLangV1Batch(n_seq, seed=seed, env_id_base=base)
    gen.set_task(tasks, seq_task_index=sti)
    tick0 = gen.engine.tick
    first = _run(gen, L)
    assert gen.engine.tick == tick0 + 1
    draws = _philox_draws(gen.engine, seed, base, tick0, L, [len(tasks[t]["patterns"]) for t in sti],
                          [tasks[t]["n_vocab"] for t in sti], (L + 1) // 4 + 2)
    assert 0.0 <= draws["u_noise"].min() and draws["u_mask"].max() < 1.0
    _equal(first, _host_rows(tasks, sti, L, draws))
    second = _run(gen, L)      # the tick advanced: other draws
    assert not np.array_equal(first[0], second[0])
    again = MetaLangV1Batch(n_seq, seed=seed, env_id_base=base)      # the same tick and seed repeat
    again.set_task(tasks, seq_task_index=sti)
    again.engine.tick = tick0
    for a, b in zip(first, _run(again, L)):
        assert np.array_equal(a, b)
    cut = n_seq // 2      # sharding: [0, cut) and [cut, n_seq) with the matching env_id_base
    for s0, s1 in ((0, cut), (cut, n_seq)):
        part = MetaLangV1Batch(s1 - s0, seed=seed, env_id_base=base + s0)
        part.set_task(tasks, seq_task_index=sti[s0:s1])
        part.engine.tick = tick0
        for a, b in zip(first, _run(part, L)):
            assert np.array_equal(a[s0:s1], b)
        assert part.check_errors() == 0
        part.close()
    assert gen.check_errors() == 0 and again.check_errors() == 0
    gen.close()
    again.close()


def test_distribution():
    """64 sequences of 1024 under one task, error_ratio 0.2: shares within 5 sigma, sigma from the counts seen.  The patterns
    have the lengths 5, 7, 9, 11 and no token 0, so a segment's pattern is read off its length; the first 80 segments of a
    sequence are whole whatever was drawn (80 * 12 <= 1024)."""
    e, P, L = 0.2, 4, 1024
    rs = np.random.RandomState(5)
    task = dict(patterns=[rs.randint(1, 50, size=n, dtype="int32") for n in (5, 7, 9, 11)], n_vocab=50, n_patterns=P,
                error_ratio=e)
    gen = MetaLangV1Batch(64, seed=99)
    gen.set_task(task)
    f, lab, kinds, n_seg = _run(gen, L)
    assert gen.check_errors() == 0
    gen.close()
    n = int((kinds != 3).sum())
    n_bad = int(((kinds == 1) | (kinds == 2)).sum())
    share = n_bad / n
    print("corrupted share %.5f of %d, sigma %.5f" % (share, n, np.sqrt(e * (1 - e) / n)))
    assert abs(share - e) <= 5 * np.sqrt(e * (1 - e) / n)
    masked = int((kinds == 2).sum()) / n_bad
    print("masked share %.5f of %d, sigma %.5f" % (masked, n_bad, np.sqrt(0.3 * 0.7 / n_bad)))
    assert abs(masked - 0.30) <= 5 * np.sqrt(0.3 * 0.7 / n_bad)
    counts = np.zeros(P)
    for b in range(64):
        seps = np.flatnonzero(kinds[b] == 3)[:80]
        lens = np.diff(np.concatenate([[-1], seps])) - 1
        assert len(lens) == 80 and set(lens.tolist()) <= {5, 7, 9, 11}
        counts += [(lens == m).sum() for m in (5, 7, 9, 11)]
    total = counts.sum()
    print("pattern shares", (counts / total).tolist(), "sigma %.5f" % np.sqrt((1 / P) * (1 - 1 / P) / total))
    assert (np.abs(counts / total - 1 / P) <= 5 * np.sqrt((1 / P) * (1 - 1 / P) / total)).all()
    assert f.min() >= 0 and f.max() < 50 and lab.max() < 50 and (n_seg >= 80).all()


def test_out_of_range_draws_are_clamped_and_flagged():
    g, task = by_name("v16_p3_g4_L64_b4")
    B, L, d = int(g["B"]), int(g["L"]), draws_of(g)
    gen = MetaLangV1Batch(B)
    gen.set_task(task)
    cases = []
    bad = dict(d, pattern_index=d["pattern_index"].copy())
    bad["pattern_index"][1, 2] = 3
    bad["pattern_index"][2, 0] = -5
    cases.append(bad)
    bad = dict(d, noise_value=np.where(g["u_noise"] < 0.1, 1 << 20, -3).astype(np.int32))
    cases.append(bad)
    cases.append(dict(d, pattern_index=np.ascontiguousarray(d["pattern_index"][:, :4])))      # every sequence needs 9 or 10
    for bad in cases:
        assert gen.check_errors() == 0
        f, lab, kinds, n_seg = _run(gen, L, bad)
        assert gen.check_errors() & 1      # XV_DEVERR_ACTION_RANGE
        assert 0 <= f.min() and f.max() < 16 and 0 <= lab.min() and lab.max() < 16 and kinds.max() <= 3
        assert (n_seg >= 1).all() and (n_seg <= L + 1).all()
    _equal(_run(gen, L, d), MetaLangV1Host(task).run(L, batch=B, draws=d))      # and the handle goes on working
    assert gen.check_errors() == 0
    gen.close()


def test_limits_are_refused_with_the_limit_named():
    _, task = by_name("v16_p3_g4_L64_b4")
    gen = MetaLangV1Batch(1)
    gen.set_task(task)
    with pytest.raises(_lib.XenoError, match=r"L = 16777217 is outside the supported range 1 \.\. 16777216"):
        gen.generate((1 << 24) + 1)
    import torch
    buf = torch.zeros(8, dtype=torch.int32, device=gen.device)      # refused before anything is launched
    rc = gen.lib.xv_metalang1_generate(gen._h, (1 << 24) + 1, 0.3, None, 0, None, None, None, _lib.ptr(buf), _lib.ptr(buf), None, None)
    assert rc == -3      # XV_ERR_UNSUPPORTED
    gen.lib.xv_last_error.restype = C.c_char_p
    assert b"L = 16777217 is outside the supported range 1 .. 16777216" in gen.lib.xv_last_error()
    assert gen.check_errors() == 0
    gen.close()


def test_reference_surface(tmp_path):
    task = TaskSamplerV1(seed=8, n_vocab=40, n_patterns=5, n_gram=6, error_ratio=0.2)
    env = MetaLangV1(L=50)
    env.set_task(task)
    f, lab = env.batch_generator(6, seed=3)
    assert isinstance(f, np.ndarray) and f.dtype == np.int32 and lab.dtype == np.int32 and f.shape == lab.shape == (6, 50)
    f2, lab2 = env.batch_generator(6, seed=3)
    assert np.array_equal(f, f2) and np.array_equal(lab, lab2) and not np.array_equal(f, env.batch_generator(6, seed=4)[0])
    one_f, one_l = env.data_generator(seed=3)
    assert one_f.shape == one_l.shape == (50,) and np.array_equal(one_f, f[0]) and np.array_equal(one_l, lab[0])
    out = str(tmp_path / "text.txt")
    env.generate_text(3, out, seed=3)
    lines = open(out).read().splitlines()
    assert len(lines) == 3
    for b, line in enumerate(lines):
        assert [tuple(int(x) for x in pair.split(",")) for pair in line.split("\t")] == list(zip(f[b].tolist(), lab[b].tolist()))
    env.generate_npy(3, str(tmp_path / "both.npy"), seed=3)
    assert np.array_equal(np.load(str(tmp_path / "both.npy")), np.stack([f[:3], lab[:3]]))


def test_generator_v1_cli_round_trip(tmp_path):
    from xenoverse_amd.metalang import generator_v1
    out = str(tmp_path / "seqs.npy")
    kw = ["--vocab_size", "32", "--patterns_number", "4", "--n_gram", "3", "4", "5", "--error_rate", "0.25"]
    generator_v1.main(["--samples", "10", "--sequence_length", "77", "--output_type", "npy", "--output", out, "--seed", "21"] + kw)
    data = np.load(out)
    assert data.dtype == np.int32 and data.shape == (10, 2, 77)
    tasks = [TaskSamplerV1(seed=21 + i, n_vocab=32, n_patterns=4, n_gram=[3, 4, 5], error_ratio=0.25) for i in range(10)]
    random.Random(21).shuffle(tasks)
    gen = MetaLangV1Batch(10, seed=21)
    gen.set_task(tasks)
    f, lab, kinds, _ = _run(gen, 77)
    gen.close()
    assert np.array_equal(data[:, 0], f) and np.array_equal(data[:, 1], lab)
    clean = kinds[:, 1:] == 0
    assert clean.any() and np.array_equal(data[:, 0, 1:][clean], data[:, 1, :-1][clean])
    txt = str(tmp_path / "seqs.txt")
    generator_v1.main(["--samples", "10", "--sequence_length", "77", "--output", txt, "--seed", "21"] + kw)
    rows = [[tuple(int(x) for x in p.split(",")) for p in line.split("\t")] for line in open(txt).read().splitlines()]
    assert rows == [list(zip(a.tolist(), b.tolist())) for a, b in zip(f, lab)]
