"""what the MetaLang tests share: the fixtures of scripts/gen_golden_metalang.py (tests/golden/metalang_v2_*.npz)"""
import numpy as np

from util import golden_files

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
