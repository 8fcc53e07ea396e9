"""The shared host statement of the samplers' draw constructions (xenoverse_amd/host_draws.py) against the oracle's C
(xo_philox4x32_10, xo_u53, xo_env_draw, xo_env_draw_sub), against csrc/philox.h compiled for the host, and against numpy's
own sum.  No GPU."""
import subprocess

import numpy as np
import pytest

import oracle
from xenoverse_amd import host_draws as hd
from xenoverse_amd.mazeworld import explore_draws_host
from xenoverse_amd.mazeworld.rollout import DRAW_EXPLORE
from xenoverse_amd.metalang.sampler_host import XV_DRAW_METALM, XV_DRAW_METALM_TASK

KATS = [      # Random123's known answers, as tests/test_oracle_philox.py holds them for the oracle
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]
# words at the ends of the range and around the 5-bit and 6-bit shifts of u53
EDGE_WORDS = [0, 1, 31, 32, 33, 63, 64, 65, 0x7FFFFFFF, 0x80000000, 0xFFFFFFDF, 0xFFFFFFE0, 0xFFFFFFBF, 0xFFFFFFC0, 0xFFFFFFFF]
BIG = [(5, 7, 2), (2**64 - 1, 2**40 + 9, 2**33 + 1), (0, 0, 0), (123456789, 63, 4), (0x1122334455667788, 2**32, 2**32),
       (77, 2**63 + 5, 2**56 + 3)]      # (seed, gid, tick)


def test_philox_equals_the_oracle_for_a_scalar_key():
    for ctr, key, exp in KATS:
        w = hd.philox4x32_10(np.array(ctr, np.uint32), np.array(key, np.uint32))
        assert w.shape == (4,) and w.dtype == np.uint32 and tuple(int(x) for x in w) == exp
    rng = np.random.RandomState(7)
    ctr = rng.randint(0, 2**32, (64, 4), dtype=np.uint64).astype(np.uint32)
    ctr[0], ctr[1] = 0, 0xFFFFFFFF
    key = np.array([0xA4093822, 0x299F31D0], np.uint32)
    assert np.array_equal(hd.philox4x32_10(ctr, key), oracle.philox4x32_10(ctr, key))
    assert np.array_equal(hd.philox4x32_10(ctr.reshape(4, 16, 4), key).reshape(64, 4), oracle.philox4x32_10(ctr, key))
    rs = np.random.RandomState(0)
    ctr = rs.randint(0, 2**32, size=(6, 4), dtype=np.uint64).astype(np.uint32)
    key = rs.randint(0, 2**32, size=2, dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(hd.philox4x32_10(ctr, key), oracle.philox4x32_10(ctr, key))


def test_philox_equals_the_oracle_for_a_broadcast_key():
    rng = np.random.RandomState(3)
    ctr = rng.randint(0, 2**32, (5, 7, 4), dtype=np.uint64).astype(np.uint32)
    ctr[0, 0], ctr[0, 1] = 0, 0xFFFFFFFF
    for shape in ((5, 7, 2), (7, 2), (5, 1, 2)):
        key = rng.randint(0, 2**32, shape, dtype=np.uint64).astype(np.uint32)
        key.reshape(-1, 2)[0] = 0xFFFFFFFF
        got = hd.philox4x32_10(ctr, key)
        full = np.broadcast_to(key, (5, 7, 2))
        assert got.shape == (5, 7, 4)
        for i in range(5):
            for j in range(7):
                assert np.array_equal(got[i, j], oracle.philox4x32_10(ctr[i, j], full[i, j])[0]), (shape, i, j)
    for ctr1, key1, exp in KATS:      # one counter under a stack of keys
        keys = np.array([key1, (1, 2)], np.uint32)
        got = hd.philox4x32_10(np.array(ctr1, np.uint32), keys)
        assert got.shape == (2, 4) and tuple(int(x) for x in got[0]) == exp
        assert np.array_equal(got[1], oracle.philox4x32_10(np.array(ctr1, np.uint32), keys[1])[0])


def test_u53_and_k53_are_the_oracles():
    rng = np.random.RandomState(1)
    words = np.array(EDGE_WORDS + list(rng.randint(0, 2**32, 40, dtype=np.uint64)), np.uint64).astype(np.uint32)
    a, b = [v.reshape(-1) for v in np.meshgrid(words, words, indexing="ij")]
    u, k = hd.u53(a, b), hd.k53(a, b)
    assert u.dtype == np.float64 and k.dtype == np.uint64 and int(k.max()) == 2**53 - 1 and int(k.min()) == 0
    assert np.array_equal(u, np.array([oracle.u53(int(x), int(y)) for x, y in zip(a, b)]))
    assert np.array_equal(k.astype(np.float64) / 2.0**53, u)
    assert [int(v) for v in k] == [((int(x) >> 5) << 26) | (int(y) >> 6) for x, y in zip(a, b)]
    assert float(u.max()) < 1.0 and float(u.min()) == 0.0
    w = np.stack([a, b, b, a], axis=-1)
    ua, ub = hd.pair(w)
    assert np.array_equal(ua, u) and np.array_equal(ub, hd.u53(b, a))


def test_env_draw_words_are_the_oracles():
    for purpose in (0, 1, 48, 255):
        for seed, gid, tick in BIG:
            assert np.array_equal(hd.env_draw_words(seed, gid, tick, purpose), oracle.env_draw(seed, gid, tick, purpose))
    # array gid / tick (together, and one against a scalar) are the scalar calls
    seed = 0x1234ABCD5678EF01
    gids = np.array([g for _, g, _ in BIG], np.uint64)
    ticks = np.array([t for _, _, t in BIG], np.uint64)
    want = np.stack([oracle.env_draw(seed, int(g), int(t), 48) for g, t in zip(gids, ticks)])
    assert np.array_equal(hd.env_draw_words(seed, gids, ticks, 48), want)
    assert np.array_equal(hd.env_draw_words(seed, gids, 2**33 + 1, 48),
                          np.stack([oracle.env_draw(seed, int(g), 2**33 + 1, 48) for g in gids]))
    assert np.array_equal(hd.env_draw_words(seed, 2**40 + 9, ticks, 48),
                          np.stack([oracle.env_draw(seed, 2**40 + 9, int(t), 48) for t in ticks]))
    grid = hd.env_draw_words(seed, gids[:, None], ticks[None, :], 1)
    assert grid.shape == (len(gids), len(ticks), 4)
    assert np.array_equal(grid[2, 4], oracle.env_draw(seed, int(gids[2]), int(ticks[4]), 1))


def test_env_draw_sub_words_are_the_oracles_and_the_headers(tmp_path):
    from xenoverse_amd import build as xb
    cases = [(5, 7, 2, XV_DRAW_METALM_TASK, 3), (2**64 - 1, 2**40 + 9, 2**33 + 1, XV_DRAW_METALM, (4 << 16) | 511),
             (0, 0, 0, XV_DRAW_METALM_TASK, 16383), (123456789, 63, 4, XV_DRAW_METALM, (3 << 16) | 0)]
    got = [hd.env_draw_sub_words(*c[:4], [c[4]])[0] for c in cases]
    for (seed, gid, tick, purpose, sub), w in zip(cases, got):      # the oracle's Philox under the documented counter layout
        ctr = np.array([[gid & 0xFFFFFFFF, gid >> 32, tick & 0xFFFFFFFF, purpose | ((tick >> 32) << 8)]], np.uint32)
        key = np.array([seed & 0xFFFFFFFF, (seed >> 32) ^ (0x80000000 | sub)], np.uint32)
        assert np.array_equal(w, oracle.philox4x32_10(ctr, key)[0])
        assert np.array_equal(w, oracle.env_draw_sub(seed, gid, tick, purpose, sub))
    # array sub, gid and tick are the scalar calls
    subs = np.array([0, 1, 511, (4 << 16) | 511, 0x7FFFFFFF], np.uint32)
    for seed, gid, tick in BIG:
        want = np.stack([oracle.env_draw_sub(seed, gid, tick, 9, int(s)) for s in subs])
        assert np.array_equal(hd.env_draw_sub_words(seed, gid, tick, 9, subs), want)
        assert np.array_equal(hd.env_draw_sub_words(seed, gid, tick, 9, int(subs[3])), want[3])
    seed = 2**64 - 1
    gids = np.array([g for _, g, _ in BIG], np.uint64)
    ticks = np.array([t for _, _, t in BIG], np.uint64)
    want = np.stack([oracle.env_draw_sub(seed, int(g), int(t), 14, 77) for g, t in zip(gids, ticks)])
    assert np.array_equal(hd.env_draw_sub_words(seed, gids, ticks, 14, 77), want)
    got2 = hd.env_draw_sub_words(seed, gids[:, None], 2**33 + 1, 14, subs[None, :])
    assert got2.shape == (len(gids), len(subs), 4)
    assert np.array_equal(got2[5, 3], oracle.env_draw_sub(seed, int(gids[5]), 2**33 + 1, 14, int(subs[3])))
    # csrc/philox.h's own host function, compiled for the host alone
    lines = "".join('  w = xv_env_draw_sub(%dull, %dull, %dull, %du, %du); printf("%%u %%u %%u %%u\\n", w.x, w.y, w.z, w.w);\n' % c
                    for c in cases)
    src = tmp_path / "draws.cpp"
    src.write_text('#include "philox.h"\n#include <cstdio>\nint main() {\n  xv_u32x4 w;\n%s  return 0;\n}\n' % lines)
    exe = str(tmp_path / "draws")
    subprocess.check_call([xb._hipcc(), "-x", "hip", "--offload-host-only", "-I", xb.CSRC, str(src), "-o", exe])
    words = np.array(subprocess.check_output([exe]).split(), np.uint64).astype(np.uint32).reshape(len(cases), 4)
    assert np.array_equal(words, np.stack(got))


def test_draws_are_philox_on_the_index_counter():
    """Draws(seed, index): key = seed, counter = {index lo, index hi, sub, purpose | tick << 8}"""
    subs = np.array([0, 1, 2, 1000, 2**31, 2**32 - 1], np.uint32)
    for seed, index, _ in BIG:
        for purpose, tick in ((0, 0), (7, 3), (0x17, 2**24 - 1), (255, 1)):
            ctr = np.array([[index & 0xFFFFFFFF, index >> 32, int(s), purpose | (tick << 8)] for s in subs], np.uint32)
            w = oracle.philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint32))
            d = hd.Draws(seed, index)
            ka, kb = d.ints53(purpose, subs, tick)
            assert ka.dtype == np.uint64 and np.array_equal(ka, hd.k53(w[:, 0], w[:, 1]))
            assert np.array_equal(kb, hd.k53(w[:, 2], w[:, 3]))
            assert [int(v) for v in ka] == [((int(x) >> 5) << 26) | (int(y) >> 6) for x, y in w[:, :2]]
            ua, ub = d.pairs(purpose, subs, tick)
            assert np.array_equal(ua, [oracle.u53(x, y) for x, y in w[:, :2]])
            assert np.array_equal(ub, [oracle.u53(x, y) for x, y in w[:, 2:]])
    d = hd.Draws(11, 5)
    blk = d.block(3, 9, tick=2)
    ua, ub = d.pairs(3, np.arange(5), tick=2)
    assert np.array_equal(blk, [ua[0], ub[0], ua[1], ub[1], ua[2], ub[2], ua[3], ub[3], ua[4]])
    assert np.array_equal(hd.interleave(np.arange(4), np.array([10, 11, 12, 13]), np.array([20, 21, 22, 23])), [10, 21, 12, 23])


def test_box_muller_expo_floor_int_and_uniform():
    rng = np.random.RandomState(2)
    ua = np.concatenate([[0.0, 2.0**-53, 1.0 - 2.0**-53, 0.5], rng.random_sample(200)])
    ub = np.concatenate([[0.0, 0.25, 1.0 - 2.0**-53, 0.5], rng.random_sample(200)])
    zc, zs = hd.box_muller(ua, ub)
    r = np.sqrt(-2.0 * np.log(1.0 - ua))
    assert hd.TWO_PI == 6.283185307179586 == 2.0 * np.pi
    assert np.array_equal(zc, r * np.cos(hd.TWO_PI * ub)) and np.array_equal(zs, r * np.sin(hd.TWO_PI * ub))
    assert zc[0] == 0.0 and zs[0] == 0.0 and np.all(np.isfinite(zc)) and np.all(np.isfinite(zs))
    assert zs[1] > 0.0 and abs(zs[1]) > 1e3 * abs(zc[1])          # angle pi / 2 at index 1: the second member is the sine
    assert hd.box_muller(0.5, 0.0) == (np.sqrt(-2.0 * np.log(0.5)), 0.0)      # angle 0: the first member is the cosine
    z1 = hd.box_muller(0.5, 0.25)
    assert abs(z1[0]) < 1e-15 and z1[1] == pytest.approx(np.sqrt(2.0 * np.log(2.0)), rel=1e-15)
    assert np.array_equal(hd.expo(ua), -np.log(1.0 - ua)) and hd.expo(0.0) == 0.0
    assert hd.floor_int(ua, 7).dtype == np.int64 and np.array_equal(hd.floor_int(ua, 7), np.floor(ua * 7.0))
    assert int(hd.floor_int(1.0 - 2.0**-53, 5)) == 4 and int(hd.floor_int(0.0, 5)) == 0
    assert hd.uniform(0.25, 2, 6) == 3.0 and np.array_equal(hd.uniform(ua, 1.5, 4.5), 1.5 + (4.5 - 1.5) * ua)


def test_np_sum_is_numpys():
    rng = np.random.RandomState(5)
    for n in (1, 7, 8, 25, 64, 127, 128, 129, 135, 225, 249, 255, 256):
        a = rng.random_sample(n) * 10.0 ** rng.randint(-6, 3, n)
        assert hd.np_sum(a) == float(np.sum(a)), n
    for n in list(range(0, 301)) + [1023, 1024, 1025, 1031, 2048, 2049, 4099]:
        a = rng.normal(size=n) * 10.0 ** rng.randint(-6, 3, n)
        assert hd.np_sum(a) == float(np.sum(a)), n
    x = rng.normal(size=(15, 15))
    assert hd.np_sum(x) == float(np.sum(x)) and hd.np_sum([]) == 0.0


def test_explore_draws_host_is_the_oracles_philox():
    """1,000 (env, tick) pairs, ticks beyond 2^32 and env ids beyond 2^32 among them"""
    rng = np.random.RandomState(0)
    seed, eps, na = 0x1234ABCD5678EF01, 0.3, 32
    ticks = np.concatenate([rng.randint(0, 1 << 20, 400), rng.randint(0, 1 << 31, 300).astype(np.int64) << 9,
                            (np.int64(1) << 40) + rng.randint(0, 1000, 300)]).astype(np.uint64)
    gids = np.concatenate([rng.randint(0, 1 << 16, 700), (np.int64(1) << 33) + rng.randint(0, 1 << 16, 300)]).astype(np.uint64)
    hits = 0
    for gid, tick in zip(gids, ticks):
        w = oracle.env_draw(int(seed), int(gid), int(tick), DRAW_EXPLORE)
        ex, a = explore_draws_host(seed, int(gid), int(tick), 1, eps, na)
        assert bool(ex[0]) == (oracle.u53(w[0], w[1]) < eps)
        assert int(a[0]) == int(np.floor(oracle.u53(w[2], w[3]) * na))
        hits += int(ex[0])
    assert 200 < hits < 400
    # a batch is the envs one by one, a tick per env is accepted, and the two ends of epsilon are all-or-nothing
    ex, a = explore_draws_host(seed, 5, 77, 64, eps, na)
    for e in (0, 17, 63):
        e1, a1 = explore_draws_host(seed, 5 + e, 77, 1, eps, na)
        assert ex[e] == e1[0] and a[e] == a1[0]
    exv, av = explore_draws_host(seed, 5, np.full(64, 77), 64, eps, na)
    assert np.array_equal(exv, ex) and np.array_equal(av, a) and a.dtype == np.int32 and 0 <= a.min() and a.max() < na
    assert not explore_draws_host(seed, 0, 1, 256, 0.0, 16)[0].any() and explore_draws_host(seed, 0, 1, 256, 1.0, 16)[0].all()
