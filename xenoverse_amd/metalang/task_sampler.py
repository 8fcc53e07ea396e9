"""MetaLang tasks: the reference's TaskSamplerV2 and TaskSamplerV1 (xenoverse/metalang/task_sampler.py:22-50, :52-73), bit for
bit.

The reference seeds numpy's process-global legacy generator and draws, in this order, the n-gram choice (only when n_gram is
a list) and five normal arrays (V2), or per pattern a Poisson length and its int32 tokens (V1).  Here the same stream comes
from a private RandomState(seed): equal numbers, and the caller's global generator is left alone."""
import os

import numpy as np

from .._lib import XenoError

# what csrc/metalang.hip supports (xv_metalang_create refuses anything outside as well)
LIMITS = dict(n_vocab=1024, n_hidden=128, n_emb=64, n_gram=8, batch=64)
TASK_ARRAYS = ("word_emb", "weights_inputlayer", "bias_inputlayer", "weights_outputlayer", "bias_outputlayer")


def TaskSamplerV2(seed=None, n_emb=16, n_hidden=64, n_vocab=256, n_gram=3, _lambda=5.0):
    if seed is None:
        seed = int.from_bytes(os.urandom(4), "little")
    rs = np.random.RandomState(seed)
    if isinstance(n_gram, list):
        n_gram = rs.choice(n_gram)
    return {
        "word_emb": rs.normal(0, 1.0, size=(n_vocab, n_emb)),
        "weights_inputlayer": rs.normal(0, 1.0, size=(n_gram, n_emb, n_hidden)),
        "bias_inputlayer": rs.normal(0, 1.0, size=(n_gram, 1, n_hidden)),
        "weights_outputlayer": rs.normal(0, 1.0, size=(n_hidden, n_vocab)),
        "bias_outputlayer": rs.normal(0, 1.0, size=(1, n_vocab)),
        "_lambda": _lambda,
        "n_emb": n_emb,
        "n_hidden": n_hidden,
        "n_vocab": n_vocab,
        "n_gram": n_gram,
    }


def TaskSamplerV1(seed=None, n_vocab=64, n_patterns=10, n_gram=64, error_ratio=0.1):
    """n_patterns patterns of max(3, Poisson(n_gram)) tokens in [0, n_vocab) (token 0, the separator's id, included)"""
    if seed is None:
        seed = int.from_bytes(os.urandom(4), "little")
    rs = np.random.RandomState(seed)
    if isinstance(n_gram, list):
        n_gram = rs.choice(n_gram)
    patterns = []
    for _ in range(n_patterns):
        l_r = max(3, rs.poisson(n_gram))
        patterns.append(rs.randint(0, n_vocab, size=(l_r), dtype="int32"))
    return {"patterns": patterns, "n_vocab": n_vocab, "n_patterns": n_patterns, "error_ratio": error_ratio, "n_gram": n_gram}


def check_limit(name, value):
    """XenoError unless 1 <= value <= LIMITS[name]"""
    if not 1 <= int(value) <= LIMITS[name]:
        raise XenoError("MetaLangV2: %s = %d is outside the supported range 1 .. %d" % (name, int(value), LIMITS[name]))


def check_task(task, what="task"):
    """sizes of one task dict -> (V, E, H, n); ValueError for a malformed dict, XenoError for a size outside LIMITS"""
    for k in TASK_ARRAYS + ("_lambda", "n_emb", "n_hidden", "n_vocab", "n_gram"):
        if k not in task:
            raise ValueError("%s: key %r is missing" % (what, k))
    V, E, H, n = int(task["n_vocab"]), int(task["n_emb"]), int(task["n_hidden"]), int(task["n_gram"])
    for k, v in (("n_vocab", V), ("n_hidden", H), ("n_emb", E), ("n_gram", n)):
        check_limit(k, v)
    shapes = dict(word_emb=(V, E), weights_inputlayer=(n, E, H), bias_inputlayer=(n, 1, H), weights_outputlayer=(H, V),
                  bias_outputlayer=(1, V))
    for k, s in shapes.items():
        if tuple(np.shape(task[k])) != s:
            raise ValueError("%s: %s has shape %s, its sizes say %s" % (what, k, tuple(np.shape(task[k])), s))
    return V, E, H, n
