"""Host restatement (numpy) of the device MetaLangV1 task sampler (csrc/metalang_sampler.hip: xv_metalang1_sample_lengths,
_offsets, _tokens): the same Philox counters and constructions (host_draws.py), in the CSR layout xv_metalang1_set_task
reads.  The device equals it bit for bit (tests/test_gpu_metalang_sampler.py): integers, and fp64 products, quotients and
sums only.  It is also the CPU-side proof that the model is the reference's TaskSamplerV1
(xenoverse/metalang/task_sampler.py:52-73): the n-gram choice when n_gram is a list, then n_patterns patterns of
max(3, Poisson(n_gram)) tokens uniform in [0, n_vocab) (tests/test_host_metalang_sampler.py).

Task k of (seed, arguments) is a pure function of those, whatever the batch — but not the task numpy's stream gives for
that seed (for that, `TaskSamplerV1(seed=...)`).  Every candidate is a task.  The draws (index layout, key = seed, counter
= {k lo, k hi, sub, purpose | tick << 8}):
  purpose 0, tick 0, sub 0: n_gram = list[floor(u m)], u the first uniform of the call
  purpose 6, tick 0, sub = pattern j: the first uniform -> Poisson(n_gram) by inversion, `poisson`
  purpose 7, tick = pattern j, sub = pos >> 1: token pos = floor(u n_vocab), u half pos & 1 of the call
n_gram is an integer in 1 .. NGRAM_MAX = 512: exp(-n_gram) stays a normal double, and the search stays short.
"""
import numpy as np

from ..host_draws import M64, Draws, floor_int, pair, philox4x32_10
from .host_v1 import LIMITS_V1
from .sampler_host_v2 import choice, n_gram_list

P_LENGTH, P_TOKEN = 6, 7                           # csrc/metalang_sampler.hip MS_P_LENGTH, MS_P_TOKEN
NGRAM_MAX = 512                                    # include/xeno.h XV_METALANG1_SAMPLER_NGRAM_MAX
PATTERNS_MAX = 1 << 20                             # include/xeno.h XV_METALANG1_SAMPLER_PATTERNS_MAX


def check_args(n_tasks, n_vocab, n_patterns, n_gram):
    """-> (the n-gram list, exp(-n_gram) per entry: formed ONCE, here, and handed to the device); XenoError with the limit
    named for anything unsupported"""
    from .._lib import XenoError
    if not 1 <= int(n_vocab) <= LIMITS_V1["n_vocab"]:
        raise XenoError("MetaLangV1: n_vocab = %d is outside the supported range 1 .. %d" % (n_vocab, LIMITS_V1["n_vocab"]))
    if not 1 <= int(n_patterns) <= PATTERNS_MAX:
        raise XenoError("MetaLangV1: n_patterns = %d is outside the supported range 1 .. %d" % (n_patterns, PATTERNS_MAX))
    if int(n_tasks) * int(n_patterns) > 2 ** 31 - 2:
        raise XenoError("MetaLangV1: %d patterns are more than the supported %d" % (int(n_tasks) * int(n_patterns), 2 ** 31 - 2))
    lst = n_gram_list(n_gram, NGRAM_MAX, "MetaLangV1")
    return lst, np.exp(-np.asarray(lst, np.float64))


def poisson(u, lam, exp_neg):
    """Poisson(lam) by inversion on the uniforms u: the smallest k with u < sum_{i <= k} p_i, p_0 = exp_neg = exp(-lam),
    p_i = p_{i-1} lam / i, the search cut at k = 2 lam + 64 (ms_poisson).  -> int64, u's shape"""
    u = np.asarray(u, np.float64)
    k = np.zeros(u.shape, np.int64)
    p = float(exp_neg)
    s = p
    lam = int(lam)
    for i in range(1, 2 * lam + 65):
        go = u >= s
        if not go.any():
            break
        k[go] = i
        p = p * float(lam) / float(i)
        s = s + p
    return k


def lengths(seed, k, n_patterns, lam, exp_neg):
    """the pattern lengths of task k -> int64[n_patterns]"""
    u = Draws(seed, k).pairs(P_LENGTH, np.arange(int(n_patterns)))[0]
    return np.maximum(3, poisson(u, lam, exp_neg))


def tokens(seed, k, lens, n_vocab):
    """the tokens of task k's patterns of lengths `lens`, concatenated -> int32[sum(lens)]"""
    lens = np.asarray(lens, np.int64)
    seed, k = int(seed) & M64, int(k) & M64
    j = np.repeat(np.arange(len(lens)), lens)
    pos = np.arange(int(lens.sum())) - np.repeat(np.cumsum(lens) - lens, lens)
    ctr = np.empty((len(j), 4), np.uint32)
    ctr[:, 0], ctr[:, 1] = k & 0xFFFFFFFF, k >> 32
    ctr[:, 2] = pos >> 1
    ctr[:, 3] = P_TOKEN | (j << 8)
    a, b = pair(philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint32)))
    return np.minimum(floor_int(np.where(pos & 1, b, a), int(n_vocab)), int(n_vocab) - 1).astype(np.int32)


def sample_tables(n_tasks, n_vocab=64, n_patterns=10, n_gram=64, error_ratio=0.1, seed=0, task_base=0):
    """tasks task_base .. task_base + n_tasks - 1 -> the numpy tables dict in sample_tasks_v1_device's layout:
    task_pattern_offset int32[n + 1], pattern_token_offset int32[n n_patterns + 1], tokens int32[total], n_vocab int32[n],
    error_ratio float64[n], n_gram int32[n]"""
    from .._lib import XenoError
    n_tasks, V, nP = int(n_tasks), int(n_vocab), int(n_patterns)
    lst, exp_neg = check_args(n_tasks, V, nP, n_gram)
    lens, toks, grams = [], [], np.zeros(n_tasks, np.int32)
    for i in range(n_tasks):
        k = int(task_base) + i
        c = choice(seed, k, len(lst))
        grams[i] = lst[c]
        lens.append(lengths(seed, k, nP, lst[c], exp_neg[c]))
        toks.append(tokens(seed, k, lens[-1], V))
    lens = np.concatenate(lens)
    if lens.sum() > LIMITS_V1["tokens"]:
        raise XenoError("MetaLangV1: %d pattern tokens are more than the supported %d" % (lens.sum(), LIMITS_V1["tokens"]))
    return dict(task_pattern_offset=(np.arange(n_tasks + 1) * nP).astype(np.int32),
                pattern_token_offset=np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), tokens=np.concatenate(toks),
                n_vocab=np.full(n_tasks, V, np.int32), error_ratio=np.full(n_tasks, float(error_ratio)), n_gram=grams,
                n_patterns=nP, seed=int(seed))
