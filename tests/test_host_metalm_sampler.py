"""The host half of the device MetaLMV3 task sampler, without a device: the numpy restatement (metalang/sampler_host.py)
against the reference's own constructions, the collector over a fake launch, and the dict form of set_task and of the
generator up to the point where a GPU is needed."""
import ctypes
import os

import numpy as np
import pytest
import torch

import metalm_sampler_util as U
from xenoverse_amd import _lib
from xenoverse_amd.device_sampling import collect_accepted
from xenoverse_amd.metalang import (RandomLMHost, TaskSamplerV3, device_sampler as ds, generator_v3, sample_candidates,
                                    sample_tasks_device, sampler_host as sh, task_dicts_from_device)
from xenoverse_amd.metalang.lm_env import env_task_of, tables_for_set_task
from xenoverse_amd.metalang.lm_host import layer_norm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [U.SHAPES[k][0] for k in U.NAMES]


@pytest.mark.parametrize("shape", SHAPES)
def test_the_three_networks_are_one_normal_stream(shape):
    V, E, H = shape
    for seed in (0, 1, 12345):
        got = sh.arrays_from_normals(np.random.RandomState(seed).normal(size=sh.n_normals(V, E, H)), V, E, H)
        want = RandomLMHost.from_seed(V, E, H, seed).arrays()
        assert sorted(got) == sorted(want)
        for k in want:
            assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (seed, k)
    with pytest.raises(ValueError):
        sh.arrays_from_normals(np.zeros(sh.n_normals(V, E, H) - 1), V, E, H)


def test_layer_norm_rows_is_numpys_for_every_row_length():
    rs = np.random.RandomState(5)
    rows = 0
    for E in range(1, 65):
        x = rs.normal(size=(24, E)) * rs.choice([1e-3, 0.3, 1.0, 40.0], size=(24, 1))
        assert np.array_equal(sh.layer_norm_rows(x), layer_norm(x)), E
        rows += len(x)
    for shape in SHAPES:      # and the rows the sampler forms: the encoder's columns
        V, E, H = shape
        enc_w = sh.arrays_from_normals(sh.task_normals(1, 0, sh.n_normals(V, E, H)), V, E, H)["enc_w"]
        assert np.array_equal(sh.layer_norm_rows(enc_w.T), RandomLMHost(enc_w, np.zeros((H, H + E)), np.zeros(H),
                                                                        np.zeros((V, H))).emb)
    assert rows == 64 * 24


def test_normals_and_uniforms_are_counter_based():
    z = sh.task_normals(9, 4, 1001)
    assert np.array_equal(z[:300], sh.task_normals(9, 4, 300))      # a prefix does not depend on the length asked for
    assert not np.array_equal(z[:300], sh.task_normals(9, 5, 300)) and not np.array_equal(z[:300], sh.task_normals(8, 4, 300))
    assert abs(z.mean()) < 0.15 and abs(z.std() - 1.0) < 0.1
    u = sh.metalm_uniforms(9, 4, 2, sh.LM_GREEDY, 257)
    assert np.array_equal(u[:64], sh.metalm_uniforms(9, 4, 2, sh.LM_GREEDY, 64)) and (u >= 0).all() and (u < 1).all()
    assert not np.array_equal(u, sh.metalm_uniforms(9, 4, 2, sh.LM_LOW, 257))
    assert not np.array_equal(u, sh.metalm_uniforms(9, 4, 4, sh.LM_GREEDY, 257))


def test_candidate_host_is_deterministic_and_independent_of_call_order():
    (V, E, H), _ = U.SHAPES["default"]
    a = [sh.candidate_host(3, c, V, E, H, U.MAX_LEN) for c in (0, 1, 2)]
    b = [sh.candidate_host(3, c, V, E, H, U.MAX_LEN) for c in (2, 1, 0)][::-1]
    for x, y in zip(a, b):
        assert np.array_equal(x["reward"], y["reward"]) and np.array_equal(x["ppl"], y["ppl"])
        assert x["query"] == y["query"] and x["answer"] == y["answer"] and x["label"] == y["label"]
        assert (x["status"], x["margin"], x["gap"]) == (y["status"], y["margin"], y["gap"])
    # the given arrays are used as they are
    c = sh.candidate_host(3, 1, V, E, H, U.MAX_LEN, arrays=a[1]["arrays"])
    assert np.array_equal(c["reward"], a[1]["reward"]) and c["query"] == a[1]["query"]
    assert not np.array_equal(sh.candidate_host(3, 1, V, E, H, U.MAX_LEN, arrays=a[0]["arrays"])["reward"], a[1]["reward"])
    assert [sh.status_of(*r) for r in ((-1.0, 2.5), (np.nan, 2.5), (0.5, 1.0), (0.0, 1.0), (0.0, 2.0), (-1, np.inf))] == \
        [0, 1, 2, 3, 0, 1]
    assert sh.status_of(-1.0, 2.5, nonfinite=True) == 1


def test_the_chosen_seeds_have_accepted_and_rejected_candidates_and_no_close_call():
    for name in ("min_vocab", "default"):      # (the larger shapes' host candidates: tests/test_gpu_metalm_sampler.py)
        hosts = U.host_candidates(name)
        st = np.array([h["status"] for h in hosts])
        assert (st == 0).any() and (st != 0).any()
        assert min(min(h["margin"], h["gap"]) for h in hosts) >= U.TAU


def test_collector_over_a_fake_launch_is_batch_independent():
    (V, E, H), _ = U.SHAPES["min_vocab"]
    n_all = 96
    tables, _ = U.fake_tables(n_all, V, E, H, seed=2)
    status = torch.tensor([sh.candidate_host(2, c, V, E, H, 64)["status"] for c in range(n_all)], dtype=torch.int32)
    accepted = torch.nonzero(status == 0).flatten()
    n_tasks = 9
    assert len(accepted) >= n_tasks and (status != 0).sum() >= n_tasks

    def launch(base, n):
        assert base + n <= n_all
        r = ds.slice_tables(tables, base, base + n)
        r["status"] = status[base:base + n]
        return r
    res = [collect_accepted(launch, n_tasks, batch, list(ds.TASK_KEYS), ds.STATUS) for batch in (7, 64, 1)]
    for got, info, hist in res:
        assert info is None and got["candidate"].tolist() == accepted[:n_tasks].tolist()
        assert np.array_equal(hist, np.bincount(status[:int(accepted[n_tasks - 1]) + 1].numpy(), minlength=4))
        for k in ds.TASK_KEYS:
            assert torch.equal(got[k], res[0][0][k]) and torch.equal(got[k], tables[k][accepted[:n_tasks]])


def test_header_and_binding_have_the_symbol_and_abi_12():
    txt = open(os.path.join(ROOT, "include", "xeno.h")).read()
    assert "int xv_metalm_sample_tasks(xv_engine* e, uint64_t seed, int64_t cand_base, int n_cand" in txt
    assert "#define XV_ABI_VERSION 12" in txt
    assert len(_lib.SIGNATURES["xv_metalm_sample_tasks"]) == 25 and _lib.ABI_VERSION == 12
    lib = _lib.load()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "xv_metalm_sample_tasks") and lib.xv_abi_version() == 12
    for k, v in (("XV_METALM_ACCEPTED", 0), ("XV_METALM_NONFINITE", 1), ("XV_METALM_REWARD_LOW", 2), ("XV_METALM_REWARD_HIGH", 3)):
        assert "#define %s %d" % (k, v) in txt and sh.STATUS[v] == k[len("XV_METALM_"):].lower()
    # a call without an engine is refused, not run
    assert lib.xv_metalm_sample_tasks(None, 0, 0, 1, 32, 16, 32, 64, 0, None, 0, *([None] * 14)) == _lib.XV_ERR_INVALID


def test_refusals_before_any_launch():
    for kw in (dict(vocab_size=11), dict(vocab_size=257), dict(embedding_size=65), dict(embedding_size=0),
               dict(hidden_size=129), dict(hidden_size=0), dict(max_len=1025), dict(max_len=0)):
        args = dict(vocab_size=32, embedding_size=16, hidden_size=32, max_len=64)
        args.update(kw)
        with pytest.raises(_lib.XenoError):
            sample_candidates(None, 0, 0, 4, **args)
    with pytest.raises(ValueError):
        sample_candidates(None, 0, 0, 0, 32, 16, 32)
    with pytest.raises(ValueError):
        sample_candidates(None, 0, -1, 4, 32, 16, 32)
    with pytest.raises(ValueError):
        sample_tasks_device(0)
    with pytest.raises(ValueError):
        sample_tasks_device(4, batch=0)
    with pytest.raises(ValueError):
        task_dicts_from_device(TaskSamplerV3(seed=1))
    assert ds.function_tokens() == (0, list(range(1, 11)))


def test_set_task_takes_the_tables_as_they_are():
    V, E, H = 32, 16, 32
    tables, arrays = U.fake_tables(5, V, E, H)
    assert ds.is_tables(tables) and not ds.is_tables(TaskSamplerV3(seed=1)) and not ds.is_tables([tables])
    dev, n_task, sizes = tables_for_set_task(tables, "cpu")
    assert n_task == 5 and sizes == (V, E, H, 0, tuple(range(1, 11)))
    assert [t.data_ptr() for t in dev] == [tables[k].data_ptr() for k in ds.TABLE_KEYS]      # borrowed: no copy
    assert env_task_of(5, 5).tolist() == [0, 1, 2, 3, 4] and env_task_of(1, 3).tolist() == [0, 0, 0]
    assert env_task_of(5, 3, torch.tensor([4, 0, 4])).tolist() == [4, 0, 4]
    for bad in (dict(n_task=5, num_envs=3), dict(n_task=5, num_envs=3, env_task_index=[0, 1, 5]),
                dict(n_task=5, num_envs=3, env_task_index=[0, 1])):
        with pytest.raises(ValueError):
            env_task_of(**bad)
    for k, t in (("emb", tables["emb"].float()), ("w_h_t", tables["w_h_t"][:, :-1]), ("b_d", tables["b_d"][:4]),
                 ("vocabulary", V + 1), ("emb", tables["emb"].numpy())):
        with pytest.raises(ValueError):
            tables_for_set_task(dict(tables, **{k: t}), "cpu")
    part = ds.slice_tables(tables, 1, 4)
    assert part["emb"].data_ptr() == tables["emb"][1].data_ptr() and part["w_d_t"].shape[0] == 3 and part["vocabulary"] == V
    # the task dicts hold the same networks
    tasks = task_dicts_from_device(tables)
    assert len(tasks) == 5 and [t["lm"].n_vocab for t in tasks] == [V] * 5
    for t, a in zip(tasks, arrays):
        assert sorted(t) == sorted(TaskSamplerV3(seed=1)) and isinstance(t["lm"], RandomLMHost)
        for k, v in a.items():
            assert np.array_equal(t["lm"].arrays()[k], v)
    assert np.array_equal(task_dicts_from_device(tables, index=[3])[0]["lm"].rnn_w, arrays[3]["rnn_w"])
    for t, e in zip(tasks, tables["emb"].numpy()):
        assert np.array_equal(t["lm"].emb, e)


def test_generator_slices_the_tables_per_call(monkeypatch):
    tables, _ = U.fake_tables(7, 32, 16, 32)
    seen = []

    class FakeEnv(object):
        def __init__(self, num_envs, max_len, device, seed, env_id_base):
            self.n, self.base = num_envs, env_id_base

        def set_task(self, tasks):
            assert ds.is_tables(tasks) and tasks["emb"].shape[0] == self.n
            assert tasks["emb"].data_ptr() == tables["emb"][self.base].data_ptr()
            seen.append((self.base, self.n))

        def reset(self):
            pass

        def stream(self, datatype, L, T_choices=None):
            row = torch.arange(self.base, self.base + self.n, dtype=torch.int32)[:, None].repeat(1, L)
            return row, -row, {}

        def check_errors(self):
            return 0

        def close(self):
            pass
    from xenoverse_amd.metalang import lm_env
    monkeypatch.setattr(lm_env, "MetaLMV3VecEnv", FakeEnv)
    monkeypatch.setattr(generator_v3, "MAX_ENVS_PER_CALL", 3)
    out = generator_v3.generate_data_v3_batch(tables, "QAR", 5)
    assert seen == [(0, 3), (3, 3), (6, 1)] and out.shape == (7, 2, 5)
    assert np.array_equal(out[:, 0, 0], np.arange(7)) and np.array_equal(out[:, 1, 4], -np.arange(7))
    ap = generator_v3.metalang_generator_v3
    import inspect
    assert inspect.signature(ap).parameters["sampler"].default is None      # opt-in: the default path is the old one
