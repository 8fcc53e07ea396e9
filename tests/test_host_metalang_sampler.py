"""The numpy restatements of the device MetaLangV2 / MetaLangV1 task samplers (metalang/sampler_host_v2.py, sampler_host_v1.py)
as statements of the reference's model (task_sampler.py TaskSamplerV2 :22-50, TaskSamplerV1 :52-73), checked statistically:
the draws are Philox, not numpy's stream, so there is nothing to compare bit for bit.  Every bound is 5 standard errors of
the statistic under the model, derived from the element counts below.  Plus: batch independence, the new C symbols and
refusals, and the round trip of the tables through task_dicts_from_device."""
import math
import os
import pickle
import re

import numpy as np
import pytest
import torch

from xenoverse_amd import _lib
from xenoverse_amd.metalang import (sample_tasks_v1_device, sample_tasks_v2_device, sampler_host_v1 as h1,
                                    sampler_host_v2 as h2, task_dicts_from_device)
from xenoverse_amd.metalang.host_v1 import check_task_v1
from xenoverse_amd.metalang.task_sampler import TASK_ARRAYS, check_task

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("xv_metalang_sample_tasks", "xv_metalang1_sample_lengths", "xv_metalang1_sample_offsets",
               "xv_metalang1_sample_tokens")


def _torch(tables):
    return {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in tables.items()}


# ---- V2 -----------------------------------------------------------------------------------------------------------------
def test_v2_normals_have_the_moments_of_standard_normals():
    n_tasks, V, E, H, n = 64, 256, 16, 64, 3
    t = h2.sample_tables(n_tasks, n_emb=E, n_hidden=H, n_vocab=V, n_gram=n, seed=0)
    assert (t["n_gram"] == n).all() and (t["_lambda"] == 5.0).all()
    counts = dict(word_emb=V * E, weights_inputlayer=n * E * H, bias_inputlayer=n * H, weights_outputlayer=H * V,
                  bias_outputlayer=V)
    for name in TASK_ARRAYS:
        z = t[name].reshape(-1)
        N = n_tasks * counts[name]
        assert z.size == N
        # the mean of N standard normals has standard error 1 / sqrt(N), their variance sqrt(2 / N)
        assert abs(z.mean()) < 5.0 / math.sqrt(N), (name, z.mean())
        assert abs(z.var() - 1.0) < 5.0 * math.sqrt(2.0 / N), (name, z.var())


def test_v2_slots_beyond_the_tasks_n_are_exact_zeros():
    t = h2.sample_tables(40, n_emb=5, n_hidden=7, n_vocab=33, n_gram=[2, 3, 5], seed=3)
    assert t["weights_inputlayer"].shape == (40, 5, 5, 7) and t["bias_inputlayer"].shape == (40, 5, 7)
    assert set(t["n_gram"].tolist()) == {2, 3, 5}
    for i, n in enumerate(t["n_gram"]):
        assert (t["weights_inputlayer"][i, n:] == 0.0).all() and (t["bias_inputlayer"][i, n:] == 0.0).all()
        assert (t["weights_inputlayer"][i, :n] != 0.0).all() and (t["bias_inputlayer"][i, :n] != 0.0).all()


def test_v2_n_gram_choice_is_uniform_over_the_list():
    lst, N = [2, 3, 5], 3000
    got = np.array([lst[h2.choice(7, k, len(lst))] for k in range(N)])
    bound = 5.0 * math.sqrt(N / 3.0 * 2.0 / 3.0)
    for g in lst:
        count = int((got == g).sum())
        assert count > 0 and abs(count - N / 3.0) <= bound, (g, count)


# ---- V1 -----------------------------------------------------------------------------------------------------------------
def test_v1_lengths_are_poisson_at_64():
    lam, N = 64, 200000
    k = h1.lengths(1, 0, N, lam, math.exp(-lam)).astype(np.float64)
    assert abs(k.mean() - lam) < 5.0 * math.sqrt(lam / N), k.mean()
    # the sample variance of N Poisson draws has variance (mu4 - sigma^4) / N with mu4 = lam + 3 lam^2
    assert abs(k.var() - lam) < 5.0 * math.sqrt((lam + 2.0 * lam * lam) / N), k.var()


def test_v1_lengths_are_at_least_3_at_1():
    lam, N = 1, 200000
    k = h1.lengths(2, 0, N, lam, math.exp(-lam))
    assert k.min() >= 3
    p = math.exp(-1.0) * (1.0 + 1.0 + 0.5 + 1.0 / 6.0)      # P(Poisson(1) <= 3)
    share = float((k == 3).mean())
    assert abs(share - p) < 5.0 * math.sqrt(p * (1.0 - p) / N), share


def test_v1_tokens_are_uniform():
    from scipy.stats import chi2
    V, N = 16, 160000
    lens = h1.lengths(5, 0, 2700, 64, math.exp(-64.0))
    tok = h1.tokens(5, 0, lens, V)
    assert tok.dtype == np.int32 and len(tok) == lens.sum() >= N
    assert tok.min() >= 0 and tok.max() < V
    count = np.bincount(tok[:N], minlength=V)
    stat = float(((count - N / V) ** 2 / (N / V)).sum())
    assert stat < chi2.ppf(1.0 - 1e-6, V - 1), stat
    big = h1.tokens(5, 1, [50, 51], 100000)
    assert big.min() >= 0 and big.max() < 100000 and big.max() > 65536


def test_v1_a_patterns_tokens_do_not_depend_on_the_patterns_before_it():
    a = h1.tokens(9, 4, [7, 5, 9], 64)
    b = h1.tokens(9, 4, [3, 5, 4], 64)
    assert (a[7:12] == b[3:8]).all() and (a[:3] == b[:3]).all() and (a[12:16] == b[8:12]).all()


# ---- both ---------------------------------------------------------------------------------------------------------------
def _v1_task(t, k):
    nP = t["n_patterns"]
    off = t["pattern_token_offset"]
    return [t["tokens"][off[p]:off[p + 1]] for p in range(k * nP, (k + 1) * nP)], int(t["n_gram"][k])


def test_task_k_does_not_depend_on_the_batch():
    kw2 = dict(n_emb=5, n_hidden=7, n_vocab=33, n_gram=[2, 3, 5], seed=11)
    kw1 = dict(n_vocab=100, n_patterns=6, n_gram=[3, 4, 5, 6], seed=11)
    big2, big1 = h2.sample_tables(257, **kw2), h1.sample_tables(257, **kw1)
    for n in (1, 5):
        t2, t1 = h2.sample_tables(n, **kw2), h1.sample_tables(n, **kw1)
        for name in TASK_ARRAYS + ("n_gram",):
            assert t2[name].shape[1:] == big2[name].shape[1:]
            assert t2[name].tobytes() == big2[name][:n].tobytes(), name
        for k in range(n):
            pa, ga = _v1_task(t1, k)
            pb, gb = _v1_task(big1, k)
            assert ga == gb and all(x.tobytes() == y.tobytes() for x, y in zip(pa, pb))
    # a task made alone, from its own index, is the task of the batch
    one = h2.sample_tables(1, task_base=256, **kw2)
    assert all(one[name][0].tobytes() == big2[name][256].tobytes() for name in TASK_ARRAYS)
    pa, _ = _v1_task(h1.sample_tables(1, task_base=256, **kw1), 0)
    pb, _ = _v1_task(big1, 256)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(pa, pb))


def test_new_symbols_are_declared_and_bound_and_the_abi_stays_12():
    with open(os.path.join(ROOT, "include", "xeno.h")) as f:
        header = f.read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES, name
    assert re.search(r"#define\s+XV_ABI_VERSION\s+12\b", header) and _lib.ABI_VERSION == 12
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert getattr(lib, name) is not None
    assert int(re.search(r"#define\s+XV_METALANG1_SAMPLER_NGRAM_MAX\s+(\d+)", header).group(1)) == h1.NGRAM_MAX
    assert int(re.search(r"#define\s+XV_METALANG_SAMPLER_LIST_MAX\s+(\d+)", header).group(1)) == h2.LIST_MAX


@pytest.mark.parametrize("fn", [sample_tasks_v2_device, h2.sample_tables])
@pytest.mark.parametrize("kw, named", [(dict(n_vocab=1025), "n_vocab = 1025 is outside the supported range 1 .. 1024"),
                                       (dict(n_hidden=129), "n_hidden = 129 is outside the supported range 1 .. 128"),
                                       (dict(n_emb=65), "n_emb = 65 is outside the supported range 1 .. 64"),
                                       (dict(n_gram=9), "n_gram = 9 is outside the supported range 1 .. 8"),
                                       (dict(n_gram=[3, 0]), "n_gram = 0 is outside the supported range 1 .. 8"),
                                       (dict(n_gram=[3] * 17), "17 entries is outside the supported range 1 .. 16")])
def test_v2_refuses_sizes_outside_the_limits_by_name(fn, kw, named):
    with pytest.raises(_lib.XenoError) as ex:      # before anything touches a device
        fn(2, **kw)
    assert named in str(ex.value)


@pytest.mark.parametrize("fn", [sample_tasks_v1_device, h1.sample_tables])
@pytest.mark.parametrize("kw, named", [(dict(n_gram=513), "n_gram = 513 is outside the supported range 1 .. 512"),
                                       (dict(n_gram=[4, 0]), "n_gram = 0 is outside the supported range 1 .. 512"),
                                       (dict(n_vocab=2 ** 31), "outside the supported range 1 .. %d" % (2 ** 31 - 1)),
                                       (dict(n_patterns=(1 << 20) + 1), "outside the supported range 1 .. %d" % (1 << 20)),
                                       (dict(n_patterns=0), "n_patterns = 0 is outside the supported range"),
                                       (dict(n_gram=[3] * 17), "17 entries is outside the supported range 1 .. 16")])
def test_v1_refuses_arguments_outside_the_limits_by_name(fn, kw, named):
    with pytest.raises(_lib.XenoError) as ex:
        fn(2, **kw)
    assert named in str(ex.value)


def test_v2_tables_round_trip_through_task_dicts():
    t = h2.sample_tables(6, n_emb=5, n_hidden=7, n_vocab=33, n_gram=[2, 3, 5], _lambda=2.5, seed=1)
    tasks = task_dicts_from_device(_torch(t))
    assert len(tasks) == 6
    tasks = pickle.loads(pickle.dumps(tasks))
    for i, task in enumerate(tasks):
        V, E, H, n = check_task(task)
        assert (V, E, H, n) == (33, 5, 7, int(t["n_gram"][i])) and task["_lambda"] == 2.5
        assert (task["word_emb"] == t["word_emb"][i]).all() and (task["weights_outputlayer"] == t["weights_outputlayer"][i]).all()
        assert (task["weights_inputlayer"] == t["weights_inputlayer"][i, :n]).all()
        assert (task["bias_inputlayer"][:, 0] == t["bias_inputlayer"][i, :n]).all()
        assert (task["bias_outputlayer"][0] == t["bias_outputlayer"][i]).all()
    assert [d["n_gram"] for d in task_dicts_from_device(_torch(t), index=[4, 1])] == [int(t["n_gram"][4]), int(t["n_gram"][1])]


def test_v1_tables_round_trip_through_task_dicts():
    t = h1.sample_tables(5, n_vocab=100, n_patterns=6, n_gram=[3, 4, 5, 6], error_ratio=0.25, seed=1)
    assert t["task_pattern_offset"].tolist() == [0, 6, 12, 18, 24, 30] and t["pattern_token_offset"][-1] == len(t["tokens"])
    tasks = pickle.loads(pickle.dumps(task_dicts_from_device(_torch(t))))
    assert len(tasks) == 5
    for i, task in enumerate(tasks):
        pats, V, e = check_task_v1(task)
        want, gram = _v1_task(t, i)
        assert (V, e, task["n_patterns"], task["n_gram"]) == (100, 0.25, 6, gram)
        assert all(len(p) >= 3 and p.tobytes() == w.tobytes() for p, w in zip(pats, want))
