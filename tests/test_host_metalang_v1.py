"""MetaLangV1 on the CPU: the host restatement (xenoverse_amd/metalang/host_v1.py) and the task sampler against the
reference's recorded runs (tests/golden/metalang_v1_*.npz), and the generator CLI's task files.  All equalities are exact."""
import pickle

import numpy as np
import pytest

from metalang_v1_util import DRAWS, EVENTS, FILES, NAMES, by_name, draws_of, fixture_id, load
from xenoverse_amd.metalang import MetaLangV1, MetaLangV1Host, TaskSamplerV1


def test_all_fixtures_are_present_and_cover_the_boundary_events():
    assert sorted(fixture_id(p) for p in FILES) == sorted(NAMES)
    seen = set()
    for p in FILES:
        seen |= set(load(p)[0]["events"].tolist())
    assert set(EVENTS) <= seen


@pytest.mark.parametrize("path", FILES, ids=fixture_id)
def test_task_sampler_is_bit_equal(path):
    g, task = load(path)
    n_gram = g["n_gram_arg"].tolist() if bool(g["n_gram_is_list"]) else int(g["n_gram_arg"][0])
    t = TaskSamplerV1(seed=int(g["sampler_seed"]), n_vocab=task["n_vocab"], n_patterns=task["n_patterns"], n_gram=n_gram,
                      error_ratio=task["error_ratio"])
    assert set(t) == {"patterns", "n_vocab", "n_patterns", "error_ratio", "n_gram"}
    assert t["n_gram"] == task["n_gram"] and len(t["patterns"]) == task["n_patterns"]
    for a, b in zip(t["patterns"], task["patterns"]):
        assert a.dtype == np.int32 and np.array_equal(a, b)
    assert (t["n_vocab"], t["n_patterns"], t["error_ratio"]) == (task["n_vocab"], task["n_patterns"], task["error_ratio"])


def test_a_list_valued_n_gram_is_among_the_fixtures():
    assert any(bool(load(p)[0]["n_gram_is_list"]) for p in FILES)
    assert len(TaskSamplerV1()["patterns"]) == 10      # unseeded: the defaults


@pytest.mark.parametrize("path", FILES, ids=fixture_id)
def test_host_reproduces_the_reference(path):
    g, task = load(path)
    B, L = int(g["B"]), int(g["L"])
    r = MetaLangV1Host(task).run(L, batch=B, rng=np.random.RandomState(int(g["call_seed"])))
    assert r["features"].dtype == np.int32 and r["labels"].dtype == np.int32 and r["features"].shape == (B, L)
    assert np.array_equal(r["features"], g["features"]) and np.array_equal(r["labels"], g["labels"])
    assert np.array_equal(r["n_segments"], g["n_segments"])
    for k in DRAWS:
        assert np.array_equal(r["draws"][k], g[k]), k
    # the global generator, seeded as the reference's caller would, gives the same
    np.random.seed(int(g["call_seed"]))
    again = MetaLangV1Host(task).run(L, batch=B)
    assert np.array_equal(again["features"], g["features"]) and np.array_equal(again["labels"], g["labels"])


@pytest.mark.parametrize("path", FILES, ids=fixture_id)
def test_host_from_position_indexed_draws(path):
    g, task = load(path)
    B, L = int(g["B"]), int(g["L"])
    r = MetaLangV1Host(task).run(L, batch=B, draws=draws_of(g))
    assert np.array_equal(r["features"], g["features"]) and np.array_equal(r["labels"], g["labels"])
    assert np.array_equal(r["n_segments"], g["n_segments"])
    # kinds against the arrays: the clean token of feature position q is labels[q - 1]
    kinds, f, lab = r["kinds"], r["features"], r["labels"]
    assert kinds.dtype == np.uint8 and kinds.shape == (B, L)
    for b in range(B):
        starts = np.concatenate([[0], np.cumsum([len(task["patterns"][p]) + 1 for p in g["pattern_index"][b, :g["n_segments"][b]]])])
        seps = set((starts[1:] - 1).tolist())
        assert [q for q in range(L) if kinds[b, q] == 3] == [q for q in range(L) if q in seps]
    assert (f[kinds == 3] == 0).all() and (f[kinds == 2] == 0).all()
    assert np.array_equal(f[:, 1:][kinds[:, 1:] == 0], lab[:, :-1][kinds[:, 1:] == 0])
    rep = kinds == 1
    assert np.array_equal(f[rep], g["noise_value"][:, :L][rep])
    e = task["error_ratio"]
    nonsep = kinds != 3
    assert np.array_equal((g["u_noise"][:, :L] < e)[nonsep], (kinds[nonsep] != 0))


def test_host_refuses_draws_it_cannot_use():
    g, task = by_name("v16_p3_g4_L64_b4")
    d = draws_of(g)
    with pytest.raises(ValueError, match="segment slots"):
        MetaLangV1Host(task).run(64, batch=4, draws=dict(d, pattern_index=d["pattern_index"][:, :3]))
    bad = dict(d, pattern_index=d["pattern_index"].copy())
    bad["pattern_index"][0, 0] = 3
    with pytest.raises(ValueError, match="pattern index"):
        MetaLangV1Host(task).run(64, batch=4, draws=bad)


def test_no_task_set_raises_the_reference_text():
    env = MetaLangV1(L=16)
    with pytest.raises(Exception, match="Please set task before using data generator"):
        env.data_generator()
    with pytest.raises(Exception, match="Please set task before using data generator"):
        env.batch_generator(4, seed=1)
    assert (env.SepID, env.MaskID, env.PaddingID) == (0, 0, 0)
    env.set_task(TaskSamplerV1(seed=1, n_vocab=77))
    assert env.VocabSize == 77


def test_generator_v1_cli_writes_and_reads_back_a_task_file(tmp_path):
    from xenoverse_amd.metalang import generator, generator_v1
    out = str(tmp_path / "tasks")
    generator_v1.main(["--sample_type", "tasks", "--samples", "6", "--vocab_size", "32", "--patterns_number", "4", "--n_gram",
                       "3", "4", "5", "--error_rate", "0.25", "--seed", "17", "--output", out])
    with open(out + ".pkl", "rb") as f:
        tasks = pickle.load(f)
    assert len(tasks) == 6
    for i, t in enumerate(tasks):
        ref = TaskSamplerV1(seed=17 + i, n_vocab=32, n_patterns=4, n_gram=[3, 4, 5], error_ratio=0.25)
        assert t["n_gram"] == ref["n_gram"] and t["error_ratio"] == 0.25 and t["n_vocab"] == 32 and t["n_patterns"] == 4
        assert all(np.array_equal(a, b) for a, b in zip(t["patterns"], ref["patterns"]))
        MetaLangV1Host(t).run(20, rng=np.random.RandomState(i))
    with pytest.raises(Exception, match="Must specify --output"):
        generator_v1.main(["--sample_type", "tasks"])
    with pytest.raises(SystemExit, match="V1 is not provided"):      # the V2 CLI is as it was
        generator.main(["--version", "v1", "--sample_type", "tasks", "--output", out])
