"""Golden fixtures of MetaLangV1: the REFERENCE's own generator (xenoverse/metalang: TaskSamplerV1, MetaLangV1.batch_generator)
on ten configurations.

Build-container tooling, like scripts/gen_golden_metalang.py: the reference is imported read-only through
oracle/_refimport.py; nothing under oracle/ is modified.  Per fixture the file holds the task's patterns (CSR: pattern_start,
pattern_tokens), the sampler's seed and arguments, the call's seed, B, L, the reference's features and labels [B, L], and the
draws it consumed re-indexed by segment slot and stream position: the reference draws from numpy's global generator, which
the script seeds with the call seed first (MetaLangV1 ignores its own seed argument), and the same stream is replayed here
from RandomState(call_seed) in the reference's order — per segment one randint(0, n_patterns), randint(0, n_vocab, size=len,
dtype=int32) and two random_sample(len).  The replay forms features and labels with its own two comparisons and must equal
the reference's arrays, or the script stops.

The fixture set must contain every boundary event the device tests rely on (EVENTS below); a configuration that asks for
events walks its call seed upwards until its sequences show them.

Only data is written: tests/golden/metalang_v1_<name>.npz.

usage: python scripts/gen_golden_metalang_v1.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import _refimport  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
MASK_RATIO = 0.30
EVENTS = ("L_not_multiple_of_4", "L_is_2", "more_than_64_segments", "segment_starts_at_L", "separator_at_L_minus_1",
          "separator_at_L", "one_pattern", "error_ratio_0", "error_ratio_1", "pattern_holds_token_0", "pattern_longer_than_L",
          "n_vocab_above_65536")


def replay(task, call_seed, B, L):
    """the draws of batch_generator(B) after numpy.random.seed(call_seed), by slot and position, and what they give"""
    rs = np.random.RandomState(call_seed)
    pats, V, e = task["patterns"], task["n_vocab"], task["error_ratio"]
    nv = np.zeros((B, L + 1), np.int32)
    un, um = np.zeros((B, L + 1)), np.zeros((B, L + 1))
    clean, feat = np.zeros((B, L + 1), np.int32), np.zeros((B, L + 1), np.int32)
    slots, starts = [], []
    for b in range(B):
        idx, st, cur = [], [], 0
        while cur < L + 1:
            p = int(rs.randint(0, task["n_patterns"]))
            n = len(pats[p])
            v, a, m = rs.randint(0, V, size=n, dtype="int32"), rs.random_sample(n), rs.random_sample(n)
            k = min(n, L + 1 - cur)
            nv[b, cur:cur + k], un[b, cur:cur + k], um[b, cur:cur + k] = v[:k], a[:k], m[:k]
            clean[b, cur:cur + k] = pats[p][:k]
            f = np.where(a < e, v, pats[p])
            feat[b, cur:cur + k] = np.where((a < e) & (m < MASK_RATIO), 0, f)[:k]
            idx.append(p)
            st.append(cur)
            cur += n + 1
        slots.append(idx)
        starts.append(st)
    index = np.zeros((B, max(len(i) for i in slots)), np.int32)
    for b, i in enumerate(slots):
        index[b, :len(i)] = i
    return dict(pattern_index=index, noise_value=nv, u_noise=un, u_mask=um, n_segments=np.array([len(i) for i in slots], np.int32),
                features=feat[:, :L], labels=clean[:, 1:]), slots, starts


def events(task, L, slots, starts):
    ev = set()
    pats = task["patterns"]
    if L % 4:
        ev.add("L_not_multiple_of_4")
    if L == 2:
        ev.add("L_is_2")
    if len(pats) == 1:
        ev.add("one_pattern")
    if task["error_ratio"] == 0.0:
        ev.add("error_ratio_0")
    if task["error_ratio"] == 1.0:
        ev.add("error_ratio_1")
    if task["n_vocab"] > 65536:
        ev.add("n_vocab_above_65536")
    for idx, st in zip(slots, starts):
        if len(idx) > 64:
            ev.add("more_than_64_segments")
        for p, s in zip(idx, st):
            if s == L:
                ev.add("segment_starts_at_L")
            if s + len(pats[p]) == L - 1:
                ev.add("separator_at_L_minus_1")
            if s + len(pats[p]) == L:
                ev.add("separator_at_L")
            if (pats[p] == 0).any():
                ev.add("pattern_holds_token_0")
            if len(pats[p]) > L:
                ev.add("pattern_longer_than_L")
    return ev


def gen(name, sampler_seed, V, P, n_gram, e, B, L, want):
    _refimport.setup()
    from xenoverse.metalang.metalangv1 import MetaLangV1
    from xenoverse.metalang.task_sampler import TaskSamplerV1
    while True:      # what an event asks of the task itself is searched over the sampler's seed
        task = TaskSamplerV1(seed=sampler_seed, n_vocab=V, n_patterns=P, n_gram=n_gram, error_ratio=e)
        if "pattern_holds_token_0" not in want or all((p == 0).any() for p in task["patterns"]):
            break
        sampler_seed += 100
    env = MetaLangV1(L=L)
    env.set_task(task)
    call_seed = sampler_seed + 1000
    while True:
        assert call_seed < sampler_seed + 3000, "no call seed shows %s" % (want,)
        np.random.seed(call_seed)
        features, labels = env.batch_generator(B)
        r, slots, starts = replay(task, call_seed, B, L)
        assert np.array_equal(r["features"], features) and np.array_equal(r["labels"], labels), "the replay left the reference"
        ev = events(task, L, slots, starts)
        if set(want) <= ev:
            break
        call_seed += 1
    lens = np.array([len(p) for p in task["patterns"]], np.int64)
    out = dict(r, pattern_start=np.concatenate([[0], np.cumsum(lens)]).astype(np.int32),
               pattern_tokens=np.concatenate(task["patterns"]).astype(np.int32), n_vocab=np.int64(V), n_patterns=np.int64(P),
               n_gram=np.int64(task["n_gram"]), n_gram_arg=np.atleast_1d(np.asarray(n_gram, np.int64)),
               n_gram_is_list=np.bool_(isinstance(n_gram, list)), error_ratio=np.float64(e), sampler_seed=np.int64(sampler_seed),
               call_seed=np.int64(call_seed), B=np.int64(B), L=np.int64(L), events=np.array(sorted(ev)))
    out["features"], out["labels"] = features.astype(np.int32), labels.astype(np.int32)
    path = os.path.join(GOLD, "metalang_v1_%s.npz" % name)
    np.savez_compressed(path, **out)
    print("%s: call seed %d, segments %s, events %s, %d bytes" % (name, call_seed, r["n_segments"].tolist(), sorted(ev),
                                                                  os.path.getsize(path)))
    return ev


CONFIGS = [  # name, sampler seed, V, P, n_gram, error_ratio, B, L, events the call seed is searched for
    ("v64_p10_g64_L256_b3", 201, 64, 10, 64, 0.1, 3, 256, ()),
    ("v16_p3_g4_L64_b4", 202, 16, 3, 4, 0.1, 4, 64, ("segment_starts_at_L", "separator_at_L_minus_1", "separator_at_L")),
    ("v300_p5_g345_L33_b2", 203, 300, 5, [3, 4, 5], 0.2, 2, 33, ("L_not_multiple_of_4",)),
    ("v8_p2_g3_L400_b2", 204, 8, 2, 3, 0.15, 2, 400, ("more_than_64_segments", "pattern_holds_token_0")),
    ("v64_p10_g64_L2_b4", 205, 64, 10, 64, 0.3, 4, 2, ("L_is_2", "pattern_longer_than_L")),
    ("v32_p1_g6_L130_b2", 206, 32, 1, 6, 0.25, 2, 130, ("one_pattern",)),
    ("v32_p4_g8_L97_b2_e0", 207, 32, 4, 8, 0.0, 2, 97, ("error_ratio_0",)),
    ("v32_p4_g8_L97_b2_e1", 208, 32, 4, 8, 1.0, 2, 97, ("error_ratio_1",)),
    ("v100000_p6_g12_L201_b2", 209, 100000, 6, 12, 0.3, 2, 201, ("n_vocab_above_65536",)),
    ("v12_p3_g3_L1031_b1", 210, 12, 3, 3, 0.2, 1, 1031, ("more_than_64_segments",)),
]


def main():
    seen = set()
    for cfg in CONFIGS:
        seen |= gen(*cfg)
    missing = [e for e in EVENTS if e not in seen]
    assert not missing, "the fixture set lacks %s" % missing


if __name__ == "__main__":
    main()
