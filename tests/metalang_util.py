"""what the MetaLang tests share: the fixtures of scripts/gen_golden_metalang.py (tests/golden/metalang_v2_*.npz)"""
import numpy as np

from util import golden_files, to_np as _np

FILES = golden_files("metalang_v2_")
NAMES = ["v256_h64_e16_g3_b1", "v64_h16_e16_g3_b1", "v64_h16_e16_g4_b1", "v64_h16_e16_g5_b1", "v64_h16_e16_g6_b1",
         "v64_h16_e16_g4_b8", "v32_h32_e8_g2_b16", "v64_h64_e16_g3_b4_lam1", "v100_h24_e12_g3_b3"]
ARRAYS = ("word_emb", "weights_inputlayer", "bias_inputlayer", "weights_outputlayer", "bias_outputlayer")
TAU = 1e-9             # a device token may differ from the reference's only at a draw whose margin is below this
PPL_TOL = 5e-7 + 1e-9  # the printed perplexity is rounded by "%f"


def fixture_id(path):
    return path.rsplit("metalang_v2_", 1)[-1][:-4]


def load(path):
    """-> (fixture dict, task dict); u, prob and margin come back as [B, L]"""
    g = dict(np.load(path, allow_pickle=False))
    task = {k: g[k] for k in ARRAYS}
    task.update(_lambda=float(g["_lambda"]), n_emb=int(g["n_emb"]), n_hidden=int(g["n_hidden"]), n_vocab=int(g["n_vocab"]),
                n_gram=int(g["n_gram"]))
    for k in ("u", "prob", "margin"):
        g[k] = np.ascontiguousarray(g[k].T)
    return g, task


def by_name(name):
    return load([p for p in FILES if fixture_id(p) == name][0])


def _philox_uniforms(engine, seed, first_seq, n_seq, tick, L):
    """the uniforms a free-running call draws, from the documented counter layout (csrc/metalang.hip, csrc/philox.h):
    counter = {id lo, id hi, tick lo, 8 | tick hi << 8}, key = {seed lo, seed hi ^ (0x80000000 | t >> 1)}; words 0,1 (t even)
    or 2,3 (t odd); u = ((a >> 5) * 2^26 + (b >> 6)) / 2^53 (xv_u53)"""
    ids = first_seq + np.arange(n_seq, dtype=np.uint64)
    ctr = np.stack([ids & 0xFFFFFFFF, ids >> np.uint64(32), np.full(n_seq, tick & 0xFFFFFFFF, np.uint64),
                    np.full(n_seq, 8 | ((tick >> 32) << 8), np.uint64)], axis=1).astype(np.int64)
    u = np.zeros((n_seq, L))
    for sub in range((L + 1) // 2):
        key = [seed & 0xFFFFFFFF, ((seed >> 32) & 0xFFFFFFFF) ^ (0x80000000 | sub)]
        w = _np(engine.philox(ctr, key)).astype(np.int64) & 0xFFFFFFFF
        for odd in (0, 1):
            t = 2 * sub + odd
            if t < L:
                a, b = w[:, 2 * odd], w[:, 2 * odd + 1]
                u[:, t] = ((a >> 5) * 67108864.0 + (b >> 6)) / 9007199254740992.0
    return u
