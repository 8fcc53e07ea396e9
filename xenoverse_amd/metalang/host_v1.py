"""MetaLangV1Host: the numpy restatement of the reference's MetaLangV1 (xenoverse/metalang/metalangv1.py:39-74), the
pattern-recovery (denoising) task, with the draws either taken from a numpy generator in the reference's order or handed in
re-indexed by segment slot and stream position.  It is the CPU-side check of csrc/metalang_v1.hip
(tests/test_host_metalang_v1.py pins it to the reference's recorded runs) and the CPU line of scripts/bench_metalang_v1.py;
the product never generates on the CPU.

A task is n_patterns integer patterns.  A sequence is a STREAM of positions q = 0 .. L:
  1. segment k is pattern p_k followed by one separator (token 0); it starts at start_k = sum_{j<k} (len(p_j) + 1), and
     segments are drawn while start_k < L + 1 (:63) — the last one overhangs
  2. a non-separator position holds the pattern's token c; its feature is noise_value where u_noise < error_ratio, and 0
     instead where additionally u_mask < mask_ratio (:43-49; both comparisons strict, fp64); separators are never touched
  3. features = the corrupted stream [0, L), labels = the clean stream [1, L + 1)                      (:74)

The reference's draw order per segment (:64, :43-45): one randint(0, n_patterns), randint(0, n_vocab, size=len, dtype=int32),
two random_sample(len) — all len of them, also where the segment overhangs L + 1.
"""
import numpy as np

from .._lib import XenoError

# what csrc/metalang_v1.hip supports (xv_metalang1_* refuses anything outside as well)
LIMITS_V1 = dict(L=1 << 24, n_vocab=2 ** 31 - 1, tokens=2 ** 31 - 1)
KIND_CLEAN, KIND_REPLACED, KIND_MASKED, KIND_SEPARATOR = 0, 1, 2, 3
DRAW_ARRAYS = ("pattern_index", "noise_value", "u_noise", "u_mask")


def check_length_v1(L):
    L = int(L)
    if not 1 <= L <= LIMITS_V1["L"]:
        raise XenoError("MetaLangV1: L = %d is outside the supported range 1 .. %d" % (L, LIMITS_V1["L"]))
    return L


def check_task_v1(task, what="task"):
    """one task dict -> (patterns as int32 arrays, n_vocab, error_ratio); ValueError for a malformed dict, XenoError for a
    size outside LIMITS_V1"""
    for k in ("patterns", "n_vocab", "error_ratio"):
        if k not in task:
            raise ValueError("%s: key %r is missing" % (what, k))
    V = int(task["n_vocab"])
    if not 1 <= V <= LIMITS_V1["n_vocab"]:
        raise XenoError("MetaLangV1: n_vocab = %d is outside the supported range 1 .. %d" % (V, LIMITS_V1["n_vocab"]))
    patterns = [np.asarray(p) for p in task["patterns"]]
    if not patterns:
        raise ValueError("%s: at least one pattern is needed" % what)
    if "n_patterns" in task and int(task["n_patterns"]) != len(patterns):
        raise ValueError("%s: n_patterns = %d, but there are %d patterns" % (what, int(task["n_patterns"]), len(patterns)))
    for i, p in enumerate(patterns):
        if p.ndim != 1 or p.size < 1 or p.dtype.kind not in "iu":
            raise ValueError("%s: pattern %d must be a non-empty one-dimensional integer array" % (what, i))
        if p.min() < 0 or p.max() >= V:
            raise ValueError("%s: pattern %d has a token outside [0, %d)" % (what, i, V))
    e = float(task["error_ratio"])
    if not e == e:
        raise ValueError("%s: error_ratio is not a number" % what)
    return [p.astype(np.int32) for p in patterns], V, e


class MetaLangV1Host(object):
    def __init__(self, task, mask_ratio=0.30):
        self.patterns, self.V, self.e = check_task_v1(task)
        self.mask_ratio = float(mask_ratio)

    def run(self, L, batch=1, rng=None, draws=None):
        """batch sequences of L positions -> dict(features int32[batch, L], labels int32[batch, L], kinds uint8[batch, L]
        (0 clean, 1 replaced, 2 masked, 3 separator), n_segments int32[batch], draws).

        draws None: the draws come from `rng` (a numpy.random.RandomState; None: numpy's global generator) in the
        reference's order, and come back re-indexed as dict(pattern_index int32[batch, n_slot], noise_value
        int32[batch, L + 1], u_noise, u_mask float64[batch, L + 1]) — what the overhang of the last segment drew beyond
        position L is dropped, entries at separator positions are 0.  draws given (such a dict): they are used instead;
        entries at separator positions are ignored."""
        L = check_length_v1(L)
        if draws is not None:
            pi = np.asarray(draws["pattern_index"])
            nv_in, un_in, um_in = (np.asarray(draws[k]) for k in DRAW_ARRAYS[1:])
            if pi.ndim != 2 or pi.shape[0] != batch or any(a.shape != (batch, L + 1) for a in (nv_in, un_in, um_in)):
                raise ValueError("draws must be pattern_index [batch, n_slot] and three arrays [batch, L + 1]")
        elif rng is None:
            rng = np.random
        nP = len(self.patterns)
        clean = np.zeros((batch, L + 1), np.int32)
        feat = np.zeros((batch, L + 1), np.int32)
        kinds = np.full((batch, L + 1), KIND_SEPARATOR, np.uint8)
        nv = np.zeros((batch, L + 1), np.int32)
        un = np.zeros((batch, L + 1))
        um = np.zeros((batch, L + 1))
        slots = []
        for b in range(batch):
            idx, cur = [], 0
            while cur < L + 1:
                if draws is None:
                    p = int(rng.randint(0, nP))
                else:
                    if len(idx) >= pi.shape[1]:
                        raise ValueError("sequence %d needs more than the %d segment slots given" % (b, pi.shape[1]))
                    p = int(pi[b, len(idx)])
                    if not 0 <= p < nP:
                        raise ValueError("pattern index %d of sequence %d is outside [0, %d)" % (p, b, nP))
                idx.append(p)
                seq = self.patterns[p]
                keep = min(len(seq), L + 1 - cur)
                sl = slice(cur, cur + keep)
                if draws is None:
                    v = rng.randint(0, self.V, size=len(seq), dtype="int32")
                    a = rng.random_sample(len(seq))
                    m = rng.random_sample(len(seq))
                    nv[b, sl], un[b, sl], um[b, sl] = v[:keep], a[:keep], m[:keep]
                else:
                    nv[b, sl], un[b, sl], um[b, sl] = nv_in[b, sl], un_in[b, sl], um_in[b, sl]
                    if keep and (nv[b, sl].min() < 0 or nv[b, sl].max() >= self.V):
                        raise ValueError("a noise value of sequence %d is outside [0, %d)" % (b, self.V))
                rep = un[b, sl] < self.e
                msk = rep & (um[b, sl] < self.mask_ratio)
                clean[b, sl] = seq[:keep]
                feat[b, sl] = np.where(msk, 0, np.where(rep, nv[b, sl], seq[:keep]))
                kinds[b, sl] = np.where(msk, KIND_MASKED, np.where(rep, KIND_REPLACED, KIND_CLEAN))
                cur += len(seq) + 1
            slots.append(idx)
        n_seg = np.array([len(i) for i in slots], np.int32)
        index = np.zeros((batch, int(n_seg.max())), np.int32)
        for b, i in enumerate(slots):
            index[b, :len(i)] = i
        return dict(features=feat[:, :L].copy(), labels=clean[:, 1:].copy(), kinds=kinds[:, :L].copy(), n_segments=n_seg,
                    draws=dict(pattern_index=index, noise_value=nv, u_noise=un, u_mask=um))
