"""MetaLangV2 on the device (csrc/metalang.hip: MetaLangV2Batch, MetaLangV2) against the reference's recorded runs
(tests/golden/metalang_v2_*.npz), against the host restatement (xenoverse_amd/metalang/host.py) and against itself.

The band: a device token may differ from the reference's (or the host's) only at a draw whose margin — the distance from u to
the nearest cut of the CDF — is below TAU = 1e-9 (reordered fp64 sums, a tree-ordered scan over <= 1024 terms and a device
exp / tanh a few ulp off move a cut by ~1e-15).  No fixture has a margin below 2.6e-8, and the scale test asserts the same of
its own draws first, so every token must be equal.  Probabilities are compared as probabilities within rtol 1e-10."""
import numpy as np
import pytest

from metalang_util import FILES, PPL_TOL, TAU, _philox_uniforms, by_name, fixture_id, load
from util import to_np as _np
from xenoverse_amd.metalang import MetaLangV2, MetaLangV2Batch, MetaLangV2Host, TaskSamplerV2

pytestmark = pytest.mark.gpu
RTOL_P = 1e-10


def _compare(name, g, tokens, logp):
    """tokens [B, L + 1], logp [B, L] of one group against its fixture"""
    total = g["tokens"][:, 1:].size
    leave_out = g["margin"] < TAU
    same = tokens[:, 1:] == g["tokens"][:, 1:]
    assert (same | leave_out).all(), (name, np.argwhere(~same)[:5])
    compared = int((~leave_out).sum())
    print("%s: compared %d / %d tokens" % (name, compared, total))
    assert compared == total
    assert np.array_equal(tokens[:, 0], np.zeros(len(tokens), np.int32))
    p = np.exp(logp)
    rel = np.abs(p / g["prob"] - 1.0).max()
    print("%s: max relative error of the chosen token's probability %.2e" % (name, rel))
    assert rel <= RTOL_P
    ppl = -logp.mean()
    print("%s: perplexity %.9f, printed %.6f" % (name, ppl, float(g["perplexity"])))
    assert abs(ppl - float(g["perplexity"])) <= PPL_TOL


@pytest.mark.parametrize("path", FILES, ids=fixture_id)
def test_reference_replay(path):
    g, task = load(path)
    gen = MetaLangV2Batch(1, int(g["B"]))
    gen.set_task(task)
    tokens, logp = gen.generate(int(g["L"]), draws=g["u"][None], return_logp=True)
    assert str(tokens.dtype) == "torch.int32" and str(logp.dtype) == "torch.float64" and tuple(tokens.shape) == (1, int(g["B"]), int(g["L"]) + 1)
    _compare(fixture_id(path), g, _np(tokens)[0], _np(logp)[0])
    # log_prob along the reference's own tokens, and along generate's
    lp = _np(gen.log_prob(g["tokens"][None]))[0]
    assert np.abs(np.exp(lp) / g["prob"] - 1.0).max() <= RTOL_P
    assert np.abs(np.exp(_np(gen.log_prob(tokens))[0]) / np.exp(_np(logp)[0]) - 1.0).max() <= RTOL_P
    assert np.allclose(_np(gen.perplexity(logp)), [-_np(logp).mean()], rtol=1e-12)
    assert gen.check_errors() == 0
    gen.close()


def test_reference_replay_four_tasks_in_one_handle():
    """the four V = 64, B = 1 fixtures (n = 3, 4, 5, 6) as four groups of one handle: n_gram is per task"""
    names = ["v64_h16_e16_g%d_b1" % n for n in (3, 4, 5, 6)]
    loaded = [by_name(n) for n in names]
    gen = MetaLangV2Batch(4, 1)
    gen.set_task([t for _, t in loaded])
    assert gen.n_gram_max == 6
    u = np.stack([g["u"] for g, _ in loaded])
    tokens, logp = gen.generate(1024, draws=u, return_logp=True)
    for k, (g, _) in enumerate(loaded):
        _compare(names[k] + " (group %d of 4)" % k, g, _np(tokens)[k], _np(logp)[k])
    lp = _np(gen.log_prob(np.stack([g["tokens"] for g, _ in loaded])))
    for k, (g, _) in enumerate(loaded):
        assert np.abs(np.exp(lp[k]) / g["prob"] - 1.0).max() <= RTOL_P
    assert gen.check_errors() == 0
    gen.close()


def _host(tasks, gti, u):
    """the host restatement group by group -> tokens [G, B, L + 1], prob [G, B, L], margin [G, B, L]"""
    hosts = [MetaLangV2Host(t) for t in tasks]
    res = [hosts[k].run(u=u[g]) for g, k in enumerate(gti)]
    return tuple(np.stack([r[key] for r in res]) for key in ("tokens", "prob", "margin"))


SCALE = {  # name: (generator seed, groups, tasks, B, L, sampler arguments)
    "v64_h16_b1": (7001, 512, 64, 1, 256, dict(n_vocab=64, n_hidden=16, n_emb=16, n_gram=[3, 4, 5, 6])),
    "v64_h16_b8": (7002, 512, 64, 8, 256, dict(n_vocab=64, n_hidden=16, n_emb=16, n_gram=[3, 4, 5, 6])),
    "defaults_b1": (7003, 64, 64, 1, 256, dict()),
}


def scale_case(name):
    seed, G, n_task, B, L, kw = SCALE[name]
    tasks = [TaskSamplerV2(seed=seed + k, **kw) for k in range(n_task)]
    rs = np.random.RandomState(seed)
    gti = rs.permutation(np.arange(G) % n_task).astype(np.int32)
    u = rs.random_sample((G, B, L))
    return tasks, gti, u


@pytest.mark.parametrize("name", sorted(SCALE))
def test_device_equals_host_at_scale(name):
    tasks, gti, u = scale_case(name)
    G, B, L = u.shape
    h_tokens, h_prob, h_margin = _host(tasks, gti, u)
    assert h_margin.min() >= TAU, "choose another generator seed: a draw lies within TAU of a cut"
    gen = MetaLangV2Batch(G, B)
    gen.set_task(tasks, group_task_index=gti)
    tokens, logp = gen.generate(L, draws=u, return_logp=True)
    tokens, logp = _np(tokens), _np(logp)
    print("%s: %d / %d tokens equal, smallest host margin %.2e" % (name, int((tokens == h_tokens).sum()), tokens.size,
                                                                  h_margin.min()))
    assert np.array_equal(tokens, h_tokens)
    rel = np.abs(np.exp(logp) / h_prob - 1.0).max()
    print("%s: max relative error of the chosen token's probability %.2e" % (name, rel))
    assert rel <= RTOL_P
    assert np.abs(np.exp(_np(gen.log_prob(tokens))) / h_prob - 1.0).max() <= RTOL_P
    assert gen.check_errors() == 0
    gen.close()


def test_free_running_draws():
    G, B, L, seed, base = 12, 4, 65, (5 << 32) | 1234567, 1000
    tasks = [TaskSamplerV2(seed=300 + k, n_vocab=100, n_hidden=24, n_emb=12, n_gram=[2, 3, 4]) for k in range(G)]
    gen = MetaLangV2Batch(G, B, seed=seed, env_id_base=base)
    gen.set_task(tasks)
    tick0 = gen.engine.tick
    first = _np(gen.generate(L))
    assert gen.engine.tick == tick0 + 1
    u = _philox_uniforms(gen.engine, seed, base, G * B, tick0, L).reshape(G, B, L)
    assert u.min() >= 0.0 and u.max() < 1.0 and len(np.unique(u)) == u.size
    assert np.array_equal(first, _np(gen.generate(L, draws=u)))
    second = _np(gen.generate(L))      # the tick advanced (the injected call took one too): other draws
    assert not np.array_equal(first, second)
    assert first.min() >= 0 and first.max() < 100 and (first[:, :, 0] == 0).all()
    # a second handle with the same seed at the same tick repeats the first call
    again = MetaLangV2Batch(G, B, seed=seed, env_id_base=base)
    again.set_task(tasks)
    again.engine.tick = tick0
    assert np.array_equal(first, _np(again.generate(L)))
    # the same groups split over two handles with the matching env_id_base
    cut = 5
    parts = []
    for g0, g1 in ((0, cut), (cut, G)):
        part = MetaLangV2Batch(g1 - g0, B, seed=seed, env_id_base=base + g0 * B)
        part.set_task(tasks[g0:g1])
        part.engine.tick = tick0
        parts.append(_np(part.generate(L)))
        assert part.check_errors() == 0
        part.close()
    assert np.array_equal(first, np.concatenate(parts))
    assert gen.check_errors() == 0 and again.check_errors() == 0
    gen.close()
    again.close()


def test_no_cut_above_u_gives_token_0_on_the_device():
    for name in ("v64_h16_e16_g4_b8", "v256_h64_e16_g3_b1"):
        g, task = by_name(name)
        B = int(g["B"])
        u = np.random.RandomState(0).random_sample((1, B, 12))
        u[0, B - 1, 5] = u[0, 0, 0] = 2.0
        gen = MetaLangV2Batch(1, B)
        gen.set_task(task)
        tokens = _np(gen.generate(12, draws=u))[0]
        assert tokens[B - 1, 6] == 0 and tokens[0, 1] == 0
        assert np.array_equal(tokens, MetaLangV2Host(task).run(u=u[0])["tokens"])
        assert gen.check_errors() == 0
        gen.close()


def test_limits_of_the_kernel_against_the_host():
    """the sizes at the edge of what is supported, small L: V = 1024 (the 1024-thread block), H = 128 and E = 64 (W_out
    read through L2), n = 8 and n = 1, B = 64 (logits in HBM scratch at V = 1024, in LDS at V = 48)"""
    cases = [dict(n_vocab=1024, n_hidden=128, n_emb=64, n_gram=8, B=3), dict(n_vocab=1024, n_hidden=32, n_emb=8, n_gram=2, B=64),
             dict(n_vocab=48, n_hidden=128, n_emb=16, n_gram=1, B=64), dict(n_vocab=200, n_hidden=100, n_emb=5, n_gram=8, B=1),
             dict(n_vocab=1000, n_hidden=40, n_emb=16, n_gram=3, B=1)]
    for k, c in enumerate(cases):
        B = c.pop("B")
        task = TaskSamplerV2(seed=900 + k, **c)
        u = np.random.RandomState(k).random_sample((2, B, 10))
        h_tokens, h_prob, h_margin = _host([task], [0, 0], u)
        assert h_margin.min() >= TAU
        gen = MetaLangV2Batch(2, B)
        gen.set_task(task)
        tokens, logp = gen.generate(10, draws=u, return_logp=True)
        assert np.array_equal(_np(tokens), h_tokens), c
        assert np.abs(np.exp(_np(logp)) / h_prob - 1.0).max() <= RTOL_P, c
        assert np.abs(np.exp(_np(gen.log_prob(tokens))) / h_prob - 1.0).max() <= RTOL_P, c
        assert gen.check_errors() == 0
        gen.close()


def test_device_errors_are_flagged():
    _, task = by_name("v64_h16_e16_g3_b1")
    gen = MetaLangV2Batch(1, 1)
    gen.set_task(task)
    bad = np.zeros((1, 1, 9), np.int32)
    bad[0, 0, 4] = 64
    gen.log_prob(bad)
    assert gen.check_errors() & 1      # XV_DEVERR_ACTION_RANGE
    assert gen.check_errors() == 0
    flat = dict(task, weights_outputlayer=np.zeros_like(task["weights_outputlayer"]),
                bias_outputlayer=np.zeros_like(task["bias_outputlayer"]))      # all logits equal: std = 0
    gen.set_task(flat)
    gen.generate(4)
    assert gen.check_errors() & 4      # XV_DEVERR_NONFINITE
    gen.close()


def test_reference_surface():
    _, task = by_name("v64_h16_e16_g4_b8")
    env = MetaLangV2(L=64)
    env.set_task(task)
    one = env.data_generator(seed=3)
    assert isinstance(one, np.ndarray) and one.dtype == np.int32 and one.shape == (65,) and one[0] == 0
    assert np.array_equal(one, env.data_generator(seed=3)) and not np.array_equal(one, env.data_generator(seed=4))
    many = env.batch_generator(8, seed=3)
    assert many.dtype == np.int32 and many.shape == (8, 65) and (many[:, 0] == 0).all()
    assert 0 <= many.min() and many.max() < 64
    assert not np.array_equal(env.data_generator(), env.data_generator())      # unseeded: fresh seeds
    # a batch of 8 is not 8 batches of 1: same uniforms, coupled statistics
    u = np.random.RandomState(9).random_sample((8, 64))
    gen8 = MetaLangV2Batch(1, 8)
    gen8.set_task(task)
    coupled = _np(gen8.generate(64, draws=u[None]))[0]
    gen1 = MetaLangV2Batch(8, 1)
    gen1.set_task(task)
    single = _np(gen1.generate(64, draws=u[:, None]))[:, 0]
    host = MetaLangV2Host(task)
    r8 = host.run(u=u)
    assert r8["margin"].min() >= TAU
    assert np.array_equal(coupled, r8["tokens"])
    r1 = [host.run(u=u[b:b + 1]) for b in range(8)]
    assert min(r["margin"].min() for r in r1) >= TAU
    assert np.array_equal(single, np.concatenate([r["tokens"] for r in r1]))
    assert not np.array_equal(coupled, single)
    assert gen8.check_errors() == 0 and gen1.check_errors() == 0
    gen8.close()
    gen1.close()
