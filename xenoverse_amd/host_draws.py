"""The counter-based draw constructions of the task samplers and rollouts, stated once for the host (numpy only).  Every
`sampler_host.py` restates its family's device sampler on top of these; the device states the same constructions in
csrc/philox.h and csrc/xv_draws.h, and the oracle's C (xo_philox4x32_10, xo_u53, xo_env_draw*) is the third, independent
statement that tests/test_host_draws.py pins this module against.
"""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
M64 = 2**64 - 1
TWO_PI = 6.283185307179586


def philox4x32_10(ctr, key):
    """xv_philox4x32_10 (csrc/philox.h; Salmon et al., SC'11): ctr uint32[..., 4], key uint32[2] or [..., 2] broadcast
    against ctr's leading shape -> uint32[..., 4]"""
    c = np.asarray(ctr, np.uint32).astype(np.uint64)
    k = np.asarray(key, np.uint32).astype(np.uint64)
    c0, c1, c2, c3 = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
    k0, k1 = k[..., 0], k[..., 1]
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def k53(a, b):
    """xv_k53 (csrc/xv_draws.h): the 53-bit integer of two words, uint64"""
    a, b = np.asarray(a, np.uint32).astype(np.uint64), np.asarray(b, np.uint32).astype(np.uint64)
    return ((a >> np.uint64(5)) << np.uint64(26)) | (b >> np.uint64(6))


def u53(a, b):
    """xv_u53 (csrc/philox.h): numpy's legacy random_sample of two words, a double in [0, 1); exactly k53 / 2^53"""
    return k53(a, b).astype(np.float64) * (1.0 / 9007199254740992.0)


def pair(w):
    """xv_pair (csrc/xv_draws.h): the two uniforms of the calls w uint32[..., 4], words 0,1 and words 2,3"""
    return u53(w[..., 0], w[..., 1]), u53(w[..., 2], w[..., 3])


def box_muller(ua, ub):
    """xv_normal2 (csrc/xv_draws.h): the fp64 Box-Muller pair, radius from 1 - ua in (0, 1], angle 2 pi ub -> (cos
    member, sin member)"""
    r = np.sqrt(-2.0 * np.log(1.0 - ua))
    ang = TWO_PI * ub
    return r * np.cos(ang), r * np.sin(ang)


def interleave(q, a, b):
    """element q of a block is half q & 1 (a: first, b: second) of call q >> 1; a, b are indexed by q already"""
    return np.where(np.asarray(q) & 1, b, a)


def expo(u):
    """xv_expo (csrc/xv_draws.h): -log(1 - u)"""
    return -np.log(1.0 - u)


def floor_int(u, m):
    """xv_floor_int (csrc/xv_draws.h): floor(u * m) as int64"""
    return np.floor(u * m).astype(np.int64)


def uniform(u, lo, hi):
    """lo + (hi - lo) * u"""
    return float(lo) + (float(hi) - float(lo)) * u


def _u64(v):
    return np.asarray(v & M64 if isinstance(v, int) else v, np.uint64)


def _env_counter(gid, tick, purpose):
    gid, tick = np.broadcast_arrays(_u64(gid), _u64(tick))
    s32 = np.uint64(32)
    return np.stack([gid & M32, gid >> s32, tick & M32,
                     np.uint64(int(purpose) & 0xFF) | (((tick >> s32) << np.uint64(8)) & M32)], axis=-1).astype(np.uint32)


def env_draw_words(seed, gid, tick, purpose):
    """xv_env_draw (csrc/philox.h): counter {gid lo, gid hi, tick lo, purpose | tick hi << 8}, key = seed.  gid and tick:
    ints or arrays below 2^64, broadcast -> uint32[..., 4]"""
    seed = int(seed) & M64
    return philox4x32_10(_env_counter(gid, tick, purpose), np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint32))


def env_draw_sub_words(seed, gid, tick, purpose, sub):
    """xv_env_draw_sub (csrc/philox.h): xv_env_draw's counter, key {seed lo, seed hi ^ (0x80000000 | sub)}.  gid, tick
    and sub: ints or arrays, broadcast -> uint32[..., 4]"""
    seed = int(seed) & M64
    ctr = _env_counter(gid, tick, purpose)
    sub = np.asarray(sub, np.uint32)
    shape = np.broadcast_shapes(ctr.shape[:-1], sub.shape)
    key = np.empty(shape + (2,), np.uint32)
    key[..., 0] = seed & 0xFFFFFFFF
    key[..., 1] = np.uint32(seed >> 32) ^ (np.uint32(0x80000000) | sub)
    return philox4x32_10(np.broadcast_to(ctr, shape + (4,)), key)


class Draws(object):
    """the draws of one (seed, index) in the index layout, xv_index_draw (csrc/xv_draws.h): key = seed, counter =
    {index lo, index hi, sub, purpose | tick << 8}"""

    def __init__(self, seed, index):
        seed, index = int(seed) & M64, int(index) & M64
        self.key = np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint32)
        self.c01 = (index & 0xFFFFFFFF, index >> 32)

    def words(self, purpose, subs, tick=0):
        subs = np.asarray(subs, np.uint32)
        ctr = np.empty(subs.shape + (4,), np.uint32)
        ctr[..., 0], ctr[..., 1] = self.c01
        ctr[..., 2] = subs
        ctr[..., 3] = (int(purpose) & 0xFF) | (int(tick) << 8)
        return philox4x32_10(ctr, self.key)

    def ints53(self, purpose, subs, tick=0):
        """-> (first, second) uint64[...]: the 53-bit integers of the two uniforms of calls `subs`"""
        w = self.words(purpose, subs, tick)
        return k53(w[..., 0], w[..., 1]), k53(w[..., 2], w[..., 3])

    def pairs(self, purpose, subs, tick=0):
        return pair(self.words(purpose, subs, tick))

    def block(self, purpose, n, tick=0):
        """n uniforms: element q is half q & 1 of call q >> 1"""
        q = np.arange(n)
        return interleave(q, *self.pairs(purpose, q >> 1, tick))


def np_sum(a):
    """numpy's pairwise add.reduce over a contiguous float64 array, spelled out in scalar fp64 arithmetic (the device's
    lm_np_sum, hs_np_sum and xv_np_sum and csrc/anymdp_vi_host.hip np_sum follow it): below 8 elements left to right from 0;
    up to 128, eight accumulators over the whole blocks of 8, combined pairwise, then the rest in order; above, the two
    halves (the first a multiple of 8) summed recursively"""
    a = np.asarray(a, np.float64).reshape(-1)
    n = len(a)
    if n > 128:
        half = n // 2
        half -= half % 8
        return np_sum(a[:half]) + np_sum(a[half:])
    x = [float(v) for v in a]
    if n < 8:
        res = 0.0
        for v in x:
            res += v
        return res
    r = x[:8]
    i = 8
    while i < n - (n % 8):
        for k in range(8):
            r[k] += x[i + k]
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for v in x[i:]:
        res += v
    return res
