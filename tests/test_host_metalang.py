"""MetaLangV2 on the CPU: the host restatement (xenoverse_amd/metalang/host.py) and the task sampler against the reference's
recorded runs (tests/golden/metalang_v2_*.npz), the documented refusals, and the generator CLI's task files."""
import pickle

import numpy as np
import pytest

from metalang_util import ARRAYS, FILES, NAMES, PPL_TOL, by_name, fixture_id, load
from xenoverse_amd._lib import XenoError
from xenoverse_amd.metalang import LIMITS, MetaLangV2, MetaLangV2Batch, MetaLangV2Host, TaskSamplerV2


def test_all_fixtures_are_present():
    assert sorted(fixture_id(p) for p in FILES) == sorted(NAMES)
    for p in FILES:
        g, _ = load(p)
        assert g["margin"].min() >= 1e-8      # so no draw of any fixture may be left out of a comparison (TAU = 1e-9)


@pytest.mark.parametrize("path", FILES, ids=fixture_id)
def test_host_reproduces_the_reference(path):
    g, task = load(path)
    r = MetaLangV2Host(task).run(u=g["u"])
    assert r["tokens"].dtype == np.int32 and r["tokens"].shape == (int(g["B"]), int(g["L"]) + 1)
    assert np.array_equal(r["tokens"], g["tokens"])
    assert np.allclose(r["prob"], g["prob"], rtol=1e-12, atol=0.0)
    assert abs(MetaLangV2Host.perplexity(r["prob"]) - float(g["perplexity"])) <= PPL_TOL
    assert np.allclose(r["margin"], g["margin"], rtol=1e-9, atol=1e-15)
    # teacher forcing along the reference's tokens gives the same probabilities
    assert np.allclose(np.exp(MetaLangV2Host(task).log_prob(g["tokens"])), g["prob"], rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("path", FILES, ids=fixture_id)
def test_task_sampler_is_bit_equal(path):
    g, task = load(path)
    t = TaskSamplerV2(seed=int(g["sampler_seed"]), n_emb=task["n_emb"], n_hidden=task["n_hidden"], n_vocab=task["n_vocab"],
                      n_gram=task["n_gram"], _lambda=task["_lambda"])
    assert set(t) == set(ARRAYS) | {"_lambda", "n_emb", "n_hidden", "n_vocab", "n_gram"}
    for k in ARRAYS:
        assert t[k].dtype == np.float64 and np.array_equal(t[k], task[k]), k
    assert (t["_lambda"], t["n_emb"], t["n_hidden"], t["n_vocab"], t["n_gram"]) == (
        task["_lambda"], task["n_emb"], task["n_hidden"], task["n_vocab"], task["n_gram"])


def test_task_sampler_list_valued_n_gram():
    """the choice is the first draw after seeding, the five arrays follow"""
    seen = set()
    for seed in range(12):
        t = TaskSamplerV2(seed=seed, n_vocab=32, n_hidden=8, n_emb=4, n_gram=[3, 4, 5, 6])
        rs = np.random.RandomState(seed)
        n = rs.choice([3, 4, 5, 6])
        assert t["n_gram"] == n and t["weights_inputlayer"].shape == (n, 4, 8)
        assert np.array_equal(t["word_emb"], rs.normal(0, 1.0, size=(32, 4)))
        seen.add(int(n))
    assert len(seen) > 1
    assert TaskSamplerV2()["word_emb"].shape == (256, 16)      # unseeded: the defaults


def test_no_cut_above_u_gives_token_0():
    _, task = by_name("v64_h16_e16_g4_b8")
    u = np.random.RandomState(0).random_sample((8, 12))
    u[2, 5] = u[7, 0] = 2.0
    r = MetaLangV2Host(task).run(u=u)
    assert r["tokens"][2, 6] == 0 and r["tokens"][7, 1] == 0
    assert (r["tokens"][:, 1:] != 0).any()


def test_n_gram_1_logits_are_the_output_bias():
    t = TaskSamplerV2(seed=5, n_vocab=24, n_hidden=8, n_emb=4, n_gram=1, _lambda=2.0)
    host = MetaLangV2Host(t)
    r = host.run(u=np.random.RandomState(1).random_sample((3, 20)))
    o = np.tile(t["bias_outputlayer"], (3, 1))
    e = np.exp(2.0 * (o - o.mean()) / np.sqrt((o * o).mean() - o.mean() ** 2))
    p = e / e.sum(1, keepdims=True)
    assert np.allclose(host.probabilities(np.zeros((3, 1), np.int64)), p, rtol=1e-12)
    assert np.allclose(r["prob"], p[np.arange(3)[:, None], r["tokens"][:, 1:]], rtol=1e-12)


@pytest.mark.parametrize("key,value", [("n_vocab", 1025), ("n_hidden", 129), ("n_emb", 65), ("n_gram", 9), ("n_gram", 0)])
def test_sizes_outside_the_limits_are_refused(key, value):
    kw = dict(n_vocab=16, n_hidden=8, n_emb=4, n_gram=2)
    kw[key] = value
    task = TaskSamplerV2(seed=1, **kw) if value else dict(TaskSamplerV2(seed=1, **dict(kw, n_gram=1)), n_gram=0)
    with pytest.raises(XenoError, match=r"%s = %d is outside the supported range 1 \.\. %d" % (key, value, LIMITS[key])):
        MetaLangV2().set_task(task)
    with pytest.raises(XenoError, match="outside the supported range"):
        MetaLangV2Host(task)


def test_too_many_sequences_per_group_is_refused():
    with pytest.raises(XenoError, match=r"batch = 65 is outside the supported range 1 \.\. 64"):
        MetaLangV2Batch(1, 65)


def test_describe_reports_the_dispatch_without_a_gpu():
    """xv_metalang_describe on a handle made without an engine: the keys, and four sizes whose variant is plain"""
    from xenoverse_amd.metalang import describe_dispatch
    from xenoverse_amd.metalang.batch import DESCRIBE_KEYS
    d = describe_dispatch(1, 256, 16, 64, 3)      # the sampler's defaults: DESIGN.md §3.6 kernel (a)
    assert tuple(d) == DESCRIBE_KEYS and set(d) == {"block", "w_out_regs", "single_seq", "tables_in_lds", "steps_per_io",
                                                    "logits", "act_seqs", "lds_bytes", "lds_opt_in", "teacher_chunk"}
    assert d == dict(block=256, w_out_regs=64, single_seq=True, tables_in_lds=True, steps_per_io=64, logits="register",
                     act_seqs=1, lds_bytes=d["lds_bytes"], lds_opt_in=False, teacher_chunk=0)
    assert 8 * (256 * 16 + 2 * (16 * 64 + 64)) < d["lds_bytes"] <= 65536      # the tables and a little more
    t = describe_dispatch(1, 256, 16, 64, 3, teacher=True)
    assert t == dict(d, teacher_chunk=128)
    d = describe_dispatch(16, 64, 16, 16, 6)
    assert (d["block"], d["w_out_regs"], d["single_seq"], d["steps_per_io"], d["logits"]) == (64, 16, False, 8, "lds")
    d = describe_dispatch(64, 1024, 8, 32, 2)
    assert (d["block"], d["w_out_regs"], d["logits"], d["lds_opt_in"]) == (1024, 0, "scratch", False)
    # looks like a tables-in-LDS case (784 doubles of tables); hs alone is 64 sequences x 128 doubles = 64 KiB
    d = describe_dispatch(64, 48, 16, 128, 1)
    assert (d["block"], d["tables_in_lds"], d["logits"], d["lds_opt_in"]) == (64, False, "lds", True)
    assert d["lds_bytes"] > 65536
    with pytest.raises(XenoError, match=r"n_vocab = 1025 is outside the supported range 1 \.\. 1024"):
        describe_dispatch(1, 1025, 16, 64, 3)


def test_the_tables_switch_keeps_the_tables_out_of_lds(monkeypatch):
    """XV_METALANG_TABLES=l2 is read when the handle is made"""
    from xenoverse_amd.metalang import describe_dispatch
    monkeypatch.delenv("XV_METALANG_TABLES", raising=False)
    lds = describe_dispatch(4, 64, 16, 16, 3)
    assert lds["tables_in_lds"]
    monkeypatch.setenv("XV_METALANG_TABLES", "l2")
    l2 = describe_dispatch(4, 64, 16, 16, 3)
    assert not l2["tables_in_lds"]
    tab = 64 * 16 + 2 * (16 * 16 + 16)
    assert l2 == dict(lds, tables_in_lds=False, lds_bytes=lds["lds_bytes"] - 8 * tab)
    monkeypatch.setenv("XV_METALANG_TABLES", "lds")
    assert describe_dispatch(4, 64, 16, 16, 3) == lds


def test_no_task_set_raises_the_reference_text():
    env = MetaLangV2(L=16)
    with pytest.raises(Exception, match="Please set task before using data generator"):
        env.data_generator()
    with pytest.raises(Exception, match="Please set task before using data generator"):
        env.batch_generator(4, seed=1)


def test_generator_cli_writes_and_reads_back_a_task_file(tmp_path):
    from xenoverse_amd.metalang import generator
    out = str(tmp_path / "tasks")
    generator.main(["--sample_type", "tasks", "--samples", "7", "--vocab_size", "32", "--hidden_size", "8", "--n_gram", "3",
                    "4", "5", "--lambda_weight", "3.0", "--seed", "11", "--output", out])
    with open(out + ".pkl", "rb") as f:
        tasks = pickle.load(f)
    assert len(tasks) == 7
    for i, t in enumerate(tasks):
        ref = TaskSamplerV2(seed=11 + i, n_vocab=32, n_emb=16, n_hidden=8, n_gram=[3, 4, 5], _lambda=3.0)
        assert t["n_gram"] == ref["n_gram"] and t["_lambda"] == 3.0
        assert all(np.array_equal(t[k], ref[k]) for k in ARRAYS)
        MetaLangV2Host(t).run(u=np.full((1, 4), 0.5))
    with pytest.raises(SystemExit, match="V1 is not provided"):
        generator.main(["--version", "v1", "--sample_type", "tasks", "--output", out])
    with pytest.raises(Exception, match="Must specify --output"):
        generator.main(["--sample_type", "tasks"])
