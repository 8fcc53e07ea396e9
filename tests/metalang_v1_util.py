"""what the MetaLangV1 tests share: the fixtures of scripts/gen_golden_metalang_v1.py (tests/golden/metalang_v1_*.npz)"""
import numpy as np

from util import golden_files

FILES = golden_files("metalang_v1_")
NAMES = ["v64_p10_g64_L256_b3", "v16_p3_g4_L64_b4", "v300_p5_g345_L33_b2", "v8_p2_g3_L400_b2", "v64_p10_g64_L2_b4",
         "v32_p1_g6_L130_b2", "v32_p4_g8_L97_b2_e0", "v32_p4_g8_L97_b2_e1", "v100000_p6_g12_L201_b2", "v12_p3_g3_L1031_b1"]
EVENTS = ("L_not_multiple_of_4", "L_is_2", "more_than_64_segments", "segment_starts_at_L", "separator_at_L_minus_1",
          "separator_at_L", "one_pattern", "error_ratio_0", "error_ratio_1", "pattern_holds_token_0", "pattern_longer_than_L",
          "n_vocab_above_65536")
DRAWS = ("pattern_index", "noise_value", "u_noise", "u_mask")


def fixture_id(path):
    return path.rsplit("metalang_v1_", 1)[-1][:-4]


def load(path):
    """-> (fixture dict, task dict)"""
    g = dict(np.load(path, allow_pickle=False))
    ps = g["pattern_start"]
    task = dict(patterns=[g["pattern_tokens"][ps[i]:ps[i + 1]] for i in range(len(ps) - 1)], n_vocab=int(g["n_vocab"]),
                n_patterns=int(g["n_patterns"]), error_ratio=float(g["error_ratio"]), n_gram=int(g["n_gram"]))
    return g, task


def by_name(name):
    return load([p for p in FILES if fixture_id(p) == name][0])


def draws_of(g):
    return {k: g[k] for k in DRAWS}
