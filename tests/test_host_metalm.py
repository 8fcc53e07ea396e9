"""MetaLMV3 on the CPU: the host restatement (xenoverse_amd/metalang/lm_host.py) and TaskSamplerV3 against the reference's
recorded runs (tests/golden/metalm_v3_*.npz), the documented refusals, and the C-ABI's new symbols."""
import os
import re

import numpy as np
import pytest

from metalm_util import (FILES, MAX_LEFT_OUT, NAMES, SCALE, WEIGHTS, draws_of, fixture_id, host_rollout, left_out, load, row,
                         smallest_margin)
from xenoverse_amd import _lib
from xenoverse_amd._lib import XenoError
from xenoverse_amd.metalang import LM_LIMITS, MetaLMV3Env, MetaLMV3VecEnv, RandomLMHost, TaskSamplerV3
from xenoverse_amd.metalang.lm_host import reward

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["xv_metalm_create", "xv_metalm_destroy", "xv_metalm_set_task", "xv_metalm_reset", "xv_metalm_policy",
           "xv_metalm_step", "xv_metalm_get_state", "xv_metalm_set_state"]


def test_all_fixtures_are_present():
    assert sorted(fixture_id(p) for p in FILES) == sorted(NAMES)
    for p in FILES:
        g, _ = load(p)
        assert smallest_margin(g) >= 1e-8      # so no draw of any fixture may be left out of a comparison (TAU = 1e-9)
        assert os.path.getsize(p) <= 811543    # the largest file tests/golden/ held before these


@pytest.mark.parametrize("path", FILES, ids=fixture_id)
def test_host_reproduces_the_reference_bit_for_bit(path):
    """every token, label, ppl and reward of the recorded run; no draw is left out"""
    g, task = load(path)
    lm = task["lm"]
    assert lm.generate_query(u=draws_of(g, "u_query", 0)) == row(g, "query", 0)
    assert np.array_equal(lm.last["margin"], g["m_query"][0, :len(lm.last["margin"])])
    for i in range(len(g["reward"])):
        T = float(g["temperature"][i])
        ans, _ = lm.generate_answer_softmax(T=T, u=draws_of(g, "u_policy", i))
        assert ans == row(g, "action", i)
        label, ppl = lm.label_answer(ans)
        greedy, ppl_min = lm.generate_answer_greedy(u=draws_of(g, "u_greedy", i))
        low, ppl_max = lm.generate_answer_low(u=draws_of(g, "u_low", i))
        assert (label, greedy, low) == (row(g, "label", i), row(g, "greedy", i), row(g, "low", i))
        assert (ppl, ppl_min, ppl_max) == (g["ppl"][i], g["ppl_min"][i], g["ppl_max"][i])
        assert reward(ppl, ppl_min, ppl_max) == g["reward"][i]
        if not g["cached"][i]:
            assert lm.generate_query(u=draws_of(g, "u_query", i + 1)) == row(g, "query", i + 1)
        else:
            assert row(g, "query", i + 1) == row(g, "query", 0)      # the reference hands back the query of reset()


@pytest.mark.parametrize("path", FILES, ids=fixture_id)
def test_task_sampler_is_bit_equal(path):
    g, _ = load(path)
    t = TaskSamplerV3(int(g["n_vocab"]), int(g["n_emb"]), int(g["n_hidden"]), seed=int(g["sampler_seed"]))
    assert set(t) == {"vocabulary", "embedding", "hidden", "function_vocabulary", "lm"}
    assert (t["vocabulary"], t["embedding"], t["hidden"]) == (int(g["n_vocab"]), int(g["n_emb"]), int(g["n_hidden"]))
    assert isinstance(t["lm"], RandomLMHost)
    for k in WEIGHTS:
        a = t["lm"].arrays()[k]
        assert a.dtype == np.float64 and np.array_equal(a, g[k]), k
    assert t["lm"].stop_token == int(g["stop_token"])
    assert t["lm"].function_token_list == [int(x) for x in g["function_tokens"]]
    assert t["function_vocabulary"]["s"] == 0 and t["function_vocabulary"]["r<"] == 10


def test_task_sampler_defaults_and_global_generator():
    np.random.seed(77)
    before = np.random.get_state()
    t = TaskSamplerV3(seed=3)
    lm = t["lm"]
    lm.generate_query()
    lm.generate_answer_softmax(T=0.5)
    lm.generate_answer_greedy()
    lm.generate_answer_low()
    TaskSamplerV3()      # unseeded
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    assert (t["vocabulary"], t["embedding"], t["hidden"]) == (32, 16, 32)
    assert lm.enc_w.shape == (16, 32) and lm.rnn_w.shape == (32, 48) and lm.dec_w.shape == (32, 32)


def test_embedding_table_is_the_layer_norm_of_the_encoder_columns():
    lm = TaskSamplerV3(seed=5)["lm"]
    for tok in (0, 7, 31):
        x = lm.enc_w[:, tok].copy()
        assert np.array_equal(lm.emb[tok], (x - x.mean()) / (x.std() + 1e-8))


def test_from_reference_takes_over_an_object_with_the_reference_attributes():
    class Obj(object):
        pass
    src = TaskSamplerV3(seed=9)["lm"]
    lm, lm.enc, lm.dec, lm.rnn = Obj(), Obj(), Obj(), Obj()
    lm.enc.weights, lm.dec.weights, lm.dec.biases = [src.enc_w], [src.dec_w], [src.dec_b]
    lm.rnn.wh, lm.rnn.bh = src.rnn_w, src.rnn_b
    lm.stop_token, lm.function_token_list = 0, list(range(1, 11))
    host = RandomLMHost.from_reference(lm)
    u = np.random.RandomState(1).random_sample(400)
    assert host.generate_query(u=u) == src.generate_query(u=u)


def test_max_len_cuts_a_pass_and_flags_it():
    lm = TaskSamplerV3(seed=4)["lm"]
    free = lm.generate_query(u=np.random.RandomState(2).random_sample(400))
    assert len(free) > 4 and not lm.overflow
    cut = RandomLMHost(*(lm.arrays()[k] for k in WEIGHTS), max_len=4)
    assert cut.generate_query(u=np.random.RandomState(2).random_sample(400)) == free[:4]
    assert cut.overflow and len(cut.last["u"]) == 5


def test_env_without_a_task_raises_the_reference_text():
    env = MetaLMV3Env()
    with pytest.raises(Exception, match="Task not set"):
        env.reset()
    with pytest.raises(Exception, match="Task not set"):
        env.policy()


def test_symbols_are_declared_and_bound_and_the_abi_version_stays():
    with open(os.path.join(ROOT, "include", "xeno.h")) as f:
        header = f.read()
    for s in SYMBOLS:
        assert re.search(r"^int %s\(" % s, header, re.M), s
        assert s in _lib.SIGNATURES, s
    assert _lib.ABI_VERSION == 12 and re.search(r"#define XV_ABI_VERSION 12\b", header)
    assert re.search(r"#define XV_DEVERR_LENGTH 16u", header)


def test_library_loads_without_a_gpu():
    lib = _lib.load()
    assert lib.xv_abi_version() == 12
    for s in SYMBOLS:
        assert hasattr(lib, s)


@pytest.mark.parametrize("V,E,H,key,value", [(257, 16, 32, "n_vocab", 257), (11, 16, 32, "n_vocab", 11),
                                             (32, 16, 129, "n_hidden", 129), (32, 65, 32, "n_emb", 65)])
def test_sizes_outside_the_limits_are_refused(V, E, H, key, value):
    lo, hi = LM_LIMITS[key]
    with pytest.raises(XenoError, match=r"%s = %d is outside the supported range %d \.\. %d" % (key, value, lo, hi)):
        TaskSamplerV3(V, E, H, seed=1)


def test_max_len_outside_the_limit_is_refused_before_the_device_is_touched():
    with pytest.raises(XenoError, match=r"max_len = 1025 is outside the supported range 1 \.\. 1024"):
        MetaLMV3VecEnv(4, max_len=1025)
    with pytest.raises(XenoError, match=r"max_len = 0 is outside the supported range 1 \.\. 1024"):
        MetaLMV3VecEnv(4, max_len=0)
    assert RandomLMHost.from_seed(256, 64, 128, 1).emb.shape == (256, 64)      # the limits themselves are served


@pytest.mark.parametrize("name", sorted(SCALE))
def test_scale_rollout_host_stays_within_the_left_out_cap(name):
    """the seeds of the GPU scale test (tests/test_gpu_metalm.py) leave the host alone within the cap"""
    res = host_rollout(name)
    frac = left_out(res)
    longest = max(len(s[k]) for r in res for s in r for k in ("query", "policy", "greedy", "low") if k in s)
    print("%s: %.2e of %d sequences lie behind a draw within TAU; longest pass %d tokens" % (
        name, frac, sum(len(r) for r in res), longest))
    assert frac <= MAX_LEFT_OUT
