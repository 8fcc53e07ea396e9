"""Every instantiation of metalang_kernel (csrc/metalang.hip) against the host restatement (metalang/host.py), across the
seams in time: the refill and write-out every K steps, the 128-position chunks of log_prob, the ragged last block.

csrc/metalang.hip builds 72 kernels — (block 64 | 256) x (W_out column in 16 | 32 | 64 registers | through L2) x (B == 1 |
B > 1) x (generate | teacher forcing) x (input tables in LDS | through L2), and block 1024 with W_out through L2 only — and
picks three run-time layouts on top: the logits of a B > 1 group in LDS or in HBM scratch, K = 64 or 8 steps between two
rounds of I/O, LDS above 64 KiB.  CASES names one set of sizes per variant together with the variant it is MEANT to run;
which one it runs is asked of the library (MetaLangV2Batch.describe, xv_metalang_describe: the selection the launch itself
uses), not worked out here, and test_the_table_covers_every_instantiation_and_layout holds the union to all 72 and to
every layout.  Sizes are the smallest that select the variant, off the tile on purpose: V no multiple of 64, H and E odd.

L = 131 is three K-blocks with a tail of 3 at K = 64, 17 at K = 8, two teacher chunks (the second of 3 positions, its n - 1
tokens of history in the first), and odd (the last Philox pair is half used).  Every case holds two tasks of different n
where n_gram_max > 1, so the table copy and the history offset run with n < n_gram_max.

The band is test_gpu_metalang.py's: every host margin is asserted >= TAU first (the cap on left-out draws is zero), then
every token must be equal and probabilities agree within RTOL_P = 1e-10.  Measured on an MI355X
(profiles/metalang_v2_variants.txt): the worst relative error of a probability over every comparison of this file is
1.02e-14, four orders inside RTOL_P, and no variant stands out (1.6e-15 to 8.9e-15 per variant at L = 131)."""
import functools
import itertools

import numpy as np
import pytest

from metalang_util import TAU, _philox_uniforms
from util import to_np as _np
from xenoverse_amd.metalang import MetaLangV2Batch, MetaLangV2Host, TaskSamplerV2, describe_dispatch

gpu = pytest.mark.gpu
RTOL_P = 1e-10
G, L = 2, 131
SWITCH = "XV_METALANG_TABLES"

# id: (V, E, H, (n of task 0, n of task 1), B, tables forced out of LDS by the environment switch,
#      the variant meant: (block, W_out registers, tables in LDS, K, logits, LDS above 64 KiB))
# TL = false comes from the sizes wherever sizes can do it (V E + (n_max - 1)(E + 1) H > 8192 doubles, or a workgroup that
# would pass 64 KiB); the three "switch" cases at the end reach it with small tables through XV_METALANG_TABLES=l2.
CASES = {
    # ---- block 64 ----
    "64-r16-b1-lds": (33, 5, 15, (3, 1), 1, False, (64, 16, True, 64, "register", False)),
    "64-r16-b1-l2": (33, 63, 15, (8, 2), 1, False, (64, 16, False, 64, "register", False)),
    "64-r16-bn-lds": (50, 5, 15, (3, 2), 2, False, (64, 16, True, 64, "lds", False)),
    "64-r16-bn-l2": (33, 63, 15, (8, 1), 2, False, (64, 16, False, 64, "lds", False)),
    "64-r32-b1-lds": (64, 7, 31, (4, 2), 1, False, (64, 32, True, 64, "register", False)),
    "64-r32-b1-l2": (33, 33, 31, (8, 2), 1, False, (64, 32, False, 64, "register", False)),
    "64-r32-bn-lds-k8": (7, 3, 17, (2, 1), 9, False, (64, 32, True, 8, "lds", False)),
    "64-r32-bn-l2": (33, 33, 31, (8, 2), 2, False, (64, 32, False, 64, "lds", False)),
    "64-r64-b1-lds": (50, 9, 33, (3, 2), 1, False, (64, 64, True, 64, "register", False)),
    "64-r64-b1-l2": (33, 19, 63, (8, 1), 1, False, (64, 64, False, 64, "register", False)),
    "64-r64-bn-lds": (33, 5, 63, (3, 2), 3, False, (64, 64, True, 64, "lds", False)),
    "64-r64-bn-l2": (33, 19, 63, (8, 2), 2, False, (64, 64, False, 64, "lds", False)),
    "64-r0-b1-lds": (33, 5, 65, (3, 1), 1, False, (64, 0, True, 64, "register", False)),
    "64-r0-b1-l2": (33, 17, 65, (8, 2), 1, False, (64, 0, False, 64, "register", False)),
    "64-r0-bn-lds": (64, 5, 127, (2, 1), 2, False, (64, 0, True, 64, "lds", False)),
    "64-r0-bn-l2": (33, 17, 65, (8, 2), 2, False, (64, 0, False, 64, "lds", False)),
    "64-r0-bn-l2-k8-big-lds": (33, 5, 65, (2, 1), 64, False, (64, 0, False, 8, "lds", True)),
    # ---- block 256 ----
    "256-r16-b1-lds": (65, 5, 15, (3, 1), 1, False, (256, 16, True, 64, "register", False)),
    "256-r16-b1-l2": (131, 63, 15, (3, 1), 1, False, (256, 16, False, 64, "register", False)),
    "256-r16-bn-lds-k8": (200, 5, 15, (3, 2), 16, False, (256, 16, True, 8, "lds", False)),
    "256-r16-bn-l2": (131, 63, 15, (2, 1), 2, False, (256, 16, False, 64, "lds", False)),
    "256-r32-b1-lds": (129, 7, 31, (4, 2), 1, False, (256, 32, True, 64, "register", False)),
    "256-r32-b1-l2": (65, 33, 31, (8, 2), 1, False, (256, 32, False, 64, "register", False)),
    "256-r32-bn-lds": (250, 3, 17, (2, 1), 2, False, (256, 32, True, 64, "lds", False)),
    "256-r32-bn-l2-scratch": (65, 33, 31, (8, 1), 17, False, (256, 32, False, 8, "scratch", False)),
    "256-r64-b1-lds": (256, 9, 33, (3, 2), 1, False, (256, 64, True, 64, "register", False)),
    "256-r64-b1-l2": (129, 64, 63, (5, 2), 1, False, (256, 64, False, 64, "register", False)),
    "256-r64-bn-lds-scratch": (100, 5, 63, (3, 1), 64, False, (256, 64, True, 8, "scratch", False)),
    "256-r64-bn-l2": (129, 64, 63, (2, 1), 2, False, (256, 64, False, 64, "lds", False)),
    "256-r0-b1-lds": (65, 5, 65, (3, 1), 1, False, (256, 0, True, 64, "register", False)),
    "256-r0-b1-l2": (200, 41, 65, (2, 1), 1, False, (256, 0, False, 64, "register", False)),
    "256-r0-bn-lds": (129, 5, 127, (2, 1), 4, False, (256, 0, True, 64, "lds", False)),
    "256-r0-bn-l2": (200, 41, 65, (3, 1), 2, False, (256, 0, False, 64, "lds", False)),
    # ---- block 1024 (W_out always through L2) ----
    "1024-b1-lds": (257, 5, 15, (3, 1), 1, False, (1024, 0, True, 64, "register", False)),
    "1024-b1-l2": (257, 33, 65, (3, 1), 1, False, (1024, 0, False, 64, "register", False)),
    "1024-bn-lds": (900, 3, 17, (3, 2), 4, False, (1024, 0, True, 64, "lds", False)),
    "1024-bn-l2": (257, 33, 15, (2, 1), 2, False, (1024, 0, False, 64, "lds", False)),
    "1024-bn-l2-scratch": (257, 33, 31, (3, 1), 5, False, (1024, 0, False, 64, "scratch", False)),
    "1024-bn-lds-scratch-k8": (300, 5, 33, (3, 1), 64, False, (1024, 0, True, 8, "scratch", False)),
    # ---- small tables kept out of LDS by the switch ----
    "64-r16-b1-switch": (33, 5, 15, (3, 1), 1, True, (64, 16, False, 64, "register", False)),
    "256-r32-bn-switch": (65, 5, 31, (3, 2), 2, True, (256, 32, False, 64, "lds", False)),
    "1024-bn-switch": (257, 5, 15, (3, 1), 2, True, (1024, 0, False, 64, "lds", False)),
}
EDGE_CASES = ("64-r32-bn-lds-k8", "256-r64-b1-lds", "1024-bn-l2", "256-r32-bn-l2-scratch")      # one per block, one scratch
NO_CUT_CASES = ("64-r16-bn-l2", "256-r16-bn-lds-k8", "1024-bn-l2-scratch")                       # one per block
SHARED_XCD_CASES = ("256-r64-bn-lds-scratch", "1024-bn-lds-scratch-k8")                        # B = 64, run with G = 8
FREE_CASES = ("64-r32-bn-lds-k8-b16", "1024-b1-lds", "256-r32-bn-l2-scratch-b32")                # see _free_case


def _meant(name, teacher):
    V, E, H, ns, B, _, (block, regs, tl, K, logits, big) = CASES[name]
    return dict(block=block, w_out_regs=regs, single_seq=B == 1, tables_in_lds=tl, steps_per_io=K, logits=logits,
                lds_opt_in=big, teacher_chunk=128 if teacher else 0)


def _agrees(got, meant):
    return all(got[k] == v for k, v in meant.items())


def _set_switch(monkeypatch, on):
    if on:
        monkeypatch.setenv(SWITCH, "l2")
    else:
        monkeypatch.delenv(SWITCH, raising=False)


def _tasks(name):
    """the case's two tasks (group g runs task g) and its B"""
    V, E, H, ns, B = CASES[name][:5]
    seed = 4000 + 10 * sorted(CASES).index(name)
    tasks = [TaskSamplerV2(seed=seed + k, n_vocab=V, n_emb=E, n_hidden=H, n_gram=n) for k, n in enumerate(ns)]
    return tasks, B


def _run_host(tasks, u):
    """group g runs task g % len(tasks)"""
    hosts = [MetaLangV2Host(t) for t in tasks]
    res = [hosts[g % len(hosts)].run(u=u[g]) for g in range(len(u))]
    return tuple(np.stack([r[key] for r in res]) for key in ("tokens", "prob", "margin"))


@functools.lru_cache(maxsize=None)
def _reference(name, length=L, no_cut=False, groups=G):
    """the case's tasks and uniforms and the host's tokens, probabilities and margins, made once and shared.  no_cut: u = 2.0
    (above every cut: token 0) at the last step of a K-block, the first step of the next, and positions 127 and 128"""
    tasks, B = _tasks(name)
    u = np.random.RandomState(77 + sorted(CASES).index(name)).random_sample((groups, B, length))
    if no_cut:
        K = CASES[name][6][3]
        for g, (b, t) in itertools.product(range(groups), ((0, K - 1), (B - 1, K), (0, 127), (B - 1, 128), (0, 128))):
            u[g, b, t] = 2.0
    tokens, prob, margin = _run_host(tasks, u)
    for a in (u, tokens, prob, margin):
        a.setflags(write=False)
    return tasks, u, tokens, prob, margin


def _handle(name, monkeypatch, groups=G):
    tasks, B = _tasks(name)
    _set_switch(monkeypatch, CASES[name][5])
    gen = MetaLangV2Batch(groups, B)
    gen.set_task(tasks, group_task_index=np.arange(groups) % len(tasks))
    for teacher in (False, True):
        got = gen.describe(teacher=teacher)
        assert _agrees(got, _meant(name, teacher)), (name, got)
    return gen


def _check(name, gen, u, h_tokens, h_prob, h_margin):
    """generate and log_prob of the first u.shape[2] steps against the host -> the worst relative probability error"""
    n = u.shape[2]
    assert h_margin[:, :, :n].min() >= TAU, "choose another seed: a draw lies within TAU of a cut"
    tokens, logp = gen.generate(n, draws=np.array(u), return_logp=True)      # (copies: the shared reference is read-only)
    tokens, logp = _np(tokens), _np(logp)
    assert np.array_equal(tokens, h_tokens[:, :, :n + 1]), (name, n, np.argwhere(tokens != h_tokens[:, :, :n + 1])[:5])
    rel_g = np.abs(np.exp(logp) / h_prob[:, :, :n] - 1.0).max()
    rel_t = np.abs(np.exp(_np(gen.log_prob(np.array(h_tokens[:, :, :n + 1])))) / h_prob[:, :, :n] - 1.0).max()
    print("%s L = %d: max relative error of a probability: generate %.2e, log_prob %.2e" % (name, n, rel_g, rel_t))
    assert rel_g <= RTOL_P and rel_t <= RTOL_P, (name, n, rel_g, rel_t)
    assert gen.check_errors() == 0
    return max(rel_g, rel_t)


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_variant_equals_host_across_the_seams(name, monkeypatch):
    tasks, u, h_tokens, h_prob, h_margin = _reference(name)
    gen = _handle(name, monkeypatch)
    rel = _check(name, gen, u, h_tokens, h_prob, h_margin)
    d = gen.describe()
    print("VARIANT block %d regs %d tables_in_lds %d logits %s rel %.3e" % (d["block"], d["w_out_regs"], d["tables_in_lds"],
                                                                          d["logits"], rel))
    gen.close()


@gpu
@pytest.mark.parametrize("name", SHARED_XCD_CASES)
def test_two_chunks_of_a_group_on_one_xcd_keep_their_scratch_slices(name, monkeypatch):
    """log_prob at L = 131 is a grid of (G, 2) workgroups and every one owns a slice of the logit scratch.  Workgroups are
    dealt round-robin over the 8 XCDs and the XCDs' L2s are not coherent with each other, so two workgroups that wrongly
    shared a slice would only disturb each other on one XCD: with G = 8 the chunks of group g are workgroups g and 8 + g,
    the same XCD (with G = 2 all four workgroups sit on XCDs of their own).  Slices of 128 and 512 KiB do not stay in a
    CU's 32 KiB L1"""
    assert CASES[name][4] == 64 and CASES[name][6][4] == "scratch"
    tasks, u, h_tokens, h_prob, h_margin = _reference(name, L, False, 8)
    gen = _handle(name, monkeypatch, 8)
    _check(name, gen, u, h_tokens, h_prob, h_margin)
    gen.close()


def _edge_lengths(name):
    K = CASES[name][6][3]
    return (1, K - 1, K, K + 1, 127, 128, 129)


@gpu
@pytest.mark.parametrize("name, length", [(n, k) for n in EDGE_CASES for k in _edge_lengths(n)])
def test_edge_lengths(name, length, monkeypatch):
    """L = K: a write-out with no ragged tail; L = 129: a teacher chunk of one position whose history lies in the chunk
    before it.  The reference is one host run of 129 steps: a shorter call is its prefix"""
    tasks, u, h_tokens, h_prob, h_margin = _reference(name, 129)
    gen = _handle(name, monkeypatch)
    _check(name, gen, np.ascontiguousarray(u[:, :, :length]), h_tokens, h_prob, h_margin)
    gen.close()


@gpu
@pytest.mark.parametrize("name", NO_CUT_CASES)
def test_no_cut_above_u_at_the_seams(name, monkeypatch):
    tasks, u, h_tokens, h_prob, h_margin = _reference(name, L, True)
    B, K = CASES[name][4], CASES[name][6][3]
    assert B > 1 and (u == 2.0).sum() == 5 * G
    for b, t in ((0, K - 1), (B - 1, K), (0, 127), (B - 1, 128), (0, 128)):
        assert (h_tokens[:, b, t + 1] == 0).all()
    assert (h_tokens[:, :, 1:] != 0).any()
    gen = _handle(name, monkeypatch)
    _check(name, gen, u, h_tokens, h_prob, h_margin)
    gen.close()


def _free_case(name):
    """the variants of the free-running test: a table case, or one with another B ("-b16": K = 8 in one wave; "-b32")"""
    if name in CASES:
        return name, CASES[name]
    base, b = name.rsplit("-b", 1)
    c = CASES[base]
    return base, c[:4] + (int(b),) + c[5:]


@gpu
@pytest.mark.parametrize("name", FREE_CASES)
def test_free_running_draws_of_a_variant(name, monkeypatch):
    """generate(L) draws what the documented counter layout says, in every layout of ubuf: K = 8 with b = i / cnt rows
    (block 64, B = 16), the 1024-thread block, and scratch (block 256, B = 32); a handle split in two draws the same"""
    base, sizes = _free_case(name)
    B, meant = sizes[4], sizes[6]
    tasks, _ = _tasks(base)
    seed, first = (9 << 32) | 424243, 700
    _set_switch(monkeypatch, False)
    gen = MetaLangV2Batch(G, B, seed=seed, env_id_base=first)
    gen.set_task(tasks)
    d = gen.describe()
    assert (d["block"], d["steps_per_io"], d["logits"]) == (meant[0], 64 if B <= 8 else 8, "register" if B == 1 else meant[4])
    tick0 = gen.engine.tick
    free = _np(gen.generate(L))
    u = _philox_uniforms(gen.engine, seed, first, G * B, tick0, L).reshape(G, B, L)
    assert u.min() >= 0.0 and u.max() < 1.0 and len(np.unique(u)) == u.size
    assert np.array_equal(free, _np(gen.generate(L, draws=u)))
    parts = []
    for g in range(G):
        part = MetaLangV2Batch(1, B, seed=seed, env_id_base=first + g * B)
        part.set_task(tasks[g])
        part.engine.tick = tick0
        parts.append(_np(part.generate(L)))
        assert part.check_errors() == 0
        part.close()
    assert np.array_equal(free, np.concatenate(parts))
    assert gen.check_errors() == 0
    gen.close()


def test_the_table_covers_every_instantiation_and_layout(monkeypatch):
    """no GPU: the library's own selection (describe_dispatch makes a handle without an engine) for every case of the table"""
    kernels, layouts, steps, big = set(), set(), set(), set()
    for name, (V, E, H, ns, B, switch, _) in CASES.items():
        _set_switch(monkeypatch, switch)
        for teacher in (False, True):
            d = describe_dispatch(B, V, E, H, max(ns), teacher=teacher)
            assert _agrees(d, _meant(name, teacher)), (name, d)
            kernels.add((d["block"], d["w_out_regs"], d["single_seq"], teacher, d["tables_in_lds"]))
            if B > 1:
                layouts.add((d["block"], d["logits"], teacher))
            steps.add((d["block"], d["steps_per_io"]))
            if d["lds_opt_in"]:
                big.add(teacher)
        if max(ns) > 1:
            assert max(ns) != min(ns) and min(ns) <= 2, name
    columns = [(block, regs) for block in (64, 256) for regs in (16, 32, 64, 0)] + [(1024, 0)]
    every = {c + flags for c in columns for flags in itertools.product((False, True), repeat=3)}
    print("%d of %d instantiations" % (len(kernels & every), len(every)))
    assert len(every) == 72 and kernels == every
    # scratch under teacher forcing at L = 131 is two chunks, so two scratch slices per group
    assert layouts == {(b, w, t) for b, w in ((64, "lds"), (256, "lds"), (256, "scratch"), (1024, "lds"), (1024, "scratch"))
                       for t in (False, True)}
    assert steps == {(b, k) for b in (64, 256, 1024) for k in (64, 8)}
    assert big == {False, True}
    for name in EDGE_CASES + NO_CUT_CASES + SHARED_XCD_CASES + tuple(_free_case(n)[0] for n in FREE_CASES):
        assert name in CASES
    assert {CASES[n][6][0] for n in EDGE_CASES} == {CASES[n][6][0] for n in NO_CUT_CASES} == {64, 256, 1024}
    assert any(CASES[n][6][4] == "scratch" for n in EDGE_CASES)
