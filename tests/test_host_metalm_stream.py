"""The MetaLMV3 training streams on the CPU: the host restatement (xenoverse_amd/metalang/stream_host.py) against the
reference's recorded generate_data_v3_single_task_* runs (tests/golden/metalmstream_*.npz), the fixtures' own properties,
the task acceptance test, the generator's command line and the C-ABI's new symbol."""
import os
import re

import numpy as np
import pytest

from metalm_stream_util import FILES, NAMES, fixture_id, host_draws, load, smallest_margin
from xenoverse_amd import _lib
from xenoverse_amd.metalang import (FUNCTION_VOCABULARY, TaskSamplerV3, generate_data_v3_host, metalang_generator_v3,
                                    sample_and_check_task, sample_and_check_tasks)
from xenoverse_amd.metalang import generator_v3
from xenoverse_amd.metalang.stream_host import SHORTEST_ROUND, accepts, check_task_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = FUNCTION_VOCABULARY


def _host(g, task, L=None):
    return generate_data_v3_host(task, str(g["datatype"]), int(g["L"]) if L is None else L, t_index=g["t_index"],
                                 T_choices=g["T_choices"], draws=host_draws(g))


def test_all_fixtures_are_present_and_have_the_stated_properties():
    assert sorted(fixture_id(p) for p in FILES) == sorted(NAMES)
    kinds = sorted((str(g["datatype"]), int(g["n_vocab"]), int(g["n_emb"]), int(g["n_hidden"])) for g, _ in map(load, FILES))
    assert kinds == sorted([("QAR", 32, 16, 32), ("QA", 32, 16, 32), ("QARA", 32, 16, 32), ("QAR", 100, 12, 24),
                            ("QARA", 256, 16, 64)])
    for p in FILES:
        g, _ = load(p)
        L, ends = int(g["L"]), g["round_end"]
        assert os.path.getsize(p) <= 811543      # the cap tests/test_host_metalm.py applies to this family's fixtures
        assert smallest_margin(g) >= 1e-8        # so no token of any fixture may be left out of a comparison (TAU = 1e-9)
        assert float(g["r_dist"].min()) >= 1e-6  # no reward token hangs on the device's last digits (tolerance 5e-9)
        assert g["data"].shape == g["label"].shape == (L,)
        assert int(g["rounds"]) == len(ends) >= 7
        assert ends[5, 0] < L                    # six full rounds
        assert ends[-2, 0] < L < ends[-1, 0]     # and the last one is cut
        per = 2 if str(g["datatype"]) == "QARA" else 1
        assert len(g["reward"]) == len(g["t_index"]) == per * len(ends)


@pytest.mark.parametrize("path", FILES, ids=fixture_id)
def test_host_reproduces_the_reference_streams_exactly(path):
    g, task = load(path)
    data, label, info = _host(g, task)
    assert np.array_equal(data, g["data"]) and np.array_equal(label, g["label"])
    assert np.array_equal(info["reward"], g["reward"]) and np.array_equal(info["r_dist"], g["r_dist"])
    assert np.array_equal(np.array(info["round_end"]), g["round_end"])
    for k, sub in enumerate(info["subs"]):      # every uniform was consumed, none beyond
        for key in ("u_policy", "u_greedy", "u_low", "u_query"):
            assert len(sub[key]) == int(g[key + "_n"][k])


@pytest.mark.parametrize("path", FILES, ids=fixture_id)
def test_label_stream_leads_the_data_stream_by_the_format(path):
    """after n rounds: n tokens in QAR, none in QA, 2 n in QARA; and round by round the layout of the two streams"""
    g, task = load(path)
    datatype = str(g["datatype"])
    lead = {"QAR": 1, "QA": 0, "QARA": 2}[datatype]
    data, full_label, info = _host(g, task, L=int(g["round_end"][-1, 0]))      # the last round's data whole
    for n, (nd, nl) in enumerate(info["round_end"], 1):
        assert nl - nd == lead * n
    d0 = l0 = 0
    per = 2 if datatype == "QARA" else 1
    for n, (nd, nl) in enumerate(info["round_end"]):
        if nl > len(full_label):      # the label stream is cut to the same length: its last round is not whole
            assert n == len(info["round_end"]) - 1 and lead
            break
        subs = info["subs"][per * n:per * n + per]
        assert data[d0] == V["q"] and full_label[nl - 1] == V["q"]
        nq = list(data[d0:nd]).index(V["s"]) - 1      # no query token is a function token
        assert list(data[d0 + 1:d0 + 1 + nq]) == list(full_label[l0:l0 + nq])
        a = subs[0]["action"]
        assert list(data[d0 + nq + 1:d0 + nq + 3]) == [V["s"], V["a"]] == list(full_label[l0 + nq:l0 + nq + 2])
        assert list(data[d0 + nq + 3:d0 + nq + 3 + len(a)]) == a
        want = a if datatype == "QA" else subs[0]["label"]
        assert list(full_label[l0 + nq + 2:l0 + nq + 2 + len(want)]) == want and len(want) == len(a) + (datatype != "QA")
        if datatype == "QAR":
            assert data[nd - 1] == full_label[nl - 2] and V["r1"] <= data[nd - 1] <= V["r5"]
        if datatype == "QARA":
            rt = data[d0 + nq + 4 + len(a)]
            assert rt in (V["r>"], V["r<"]) and data[nd - 1] == V["s"]
            assert list(data[nd - 1 - len(subs[1]["action"]):nd - 1]) == subs[1]["action"]
        d0, l0 = nd, nl


@pytest.mark.parametrize("path", FILES, ids=fixture_id)
@pytest.mark.parametrize("L", [1, 3])
def test_a_length_below_the_first_round_returns_the_prefix(path, L):
    g, task = load(path)
    data, label, info = _host(g, task, L=L)
    assert info["rounds"] == 1 and L < SHORTEST_ROUND[str(g["datatype"])]
    assert np.array_equal(data, g["data"][:L]) and np.array_equal(label, g["label"][:L])


def test_reward_tokens_follow_the_reference_order():
    from xenoverse_amd.metalang.stream_host import qar_reward_token, qara_reward_token
    assert [qar_reward_token(r) for r in (-0.1, 0.0, 0.49, 0.5, 0.99, 1.0, 1.99, 2.0, 50.0)] == [
        V["r1"], V["r2"], V["r2"], V["r3"], V["r3"], V["r4"], V["r4"], V["r5"], V["r5"]]
    assert qara_reward_token(1.0, 0.7) == V["r>"] and qara_reward_token(1.0, 0.8) == V["r<"]
    assert qara_reward_token(0.0, 5.0) == V["r<"] and qara_reward_token(float("nan"), 0.0) == V["r="]


def test_host_rejects_bad_arguments():
    task = TaskSamplerV3(seed=1)
    with pytest.raises(ValueError, match="datatype must be one of"):
        generate_data_v3_host(task, "QR", 10)
    with pytest.raises(ValueError, match="L must be at least 1"):
        generate_data_v3_host(task, "QA", 0)
    with pytest.raises(ValueError, match="indices into the 20 T_choices"):
        generate_data_v3_host(task, "QAR", 10, t_index=[20])
    with pytest.raises(ValueError, match="more than the 1 temperature indices"):
        generate_data_v3_host(task, "QAR", 4000, t_index=[3])


def test_sample_and_check_tasks_accepts_only_tasks_that_meet_both_conditions_and_advances_the_seed():
    verdict = {s: accepts(*check_task_host(TaskSamplerV3(seed=s))) for s in range(100, 116)}
    assert not verdict[103] and verdict[104] and not verdict[107]      # what the cases below stand on
    for s in range(100, 116):
        low, high = check_task_host(TaskSamplerV3(seed=s))
        assert verdict[s] == (high >= 2.0 and low <= 0.0)
    tasks, seeds = sample_and_check_tasks(5, seed=100, backend="host")
    assert seeds == [s for s in range(100, 116) if verdict[s]][:5] and 103 not in seeds
    for t, s in zip(tasks, seeds):
        assert np.array_equal(t["lm"].rnn_w, TaskSamplerV3(seed=s)["lm"].rnn_w)
    # a seeded task that fails: the reference would retry seed 103 forever, here the seed advances
    one = sample_and_check_task(seed=103, backend="host")
    assert np.array_equal(one["lm"].rnn_w, TaskSamplerV3(seed=104)["lm"].rnn_w)
    assert set(one) == {"vocabulary", "embedding", "hidden", "function_vocabulary", "lm"}
    with pytest.raises(ValueError, match="backend must be"):
        sample_and_check_tasks(1, seed=1, backend="numpy")


def test_cli_writes_an_npy_of_samples_by_two_by_length(tmp_path):
    import pickle
    tasks_file = str(tmp_path / "tasks")
    generator_v3.main(["--sample_type", "tasks", "--samples", "3", "--output", tasks_file, "--seed", "100", "--backend",
                       "host"])
    with open(tasks_file + ".pkl", "rb") as f:
        tasks = pickle.load(f)
    assert len(tasks) == 3 and all(accepts(*check_task_host(t)) for t in tasks)
    out = str(tmp_path / "seq.npy")
    for datatype in ("QAR", "QA", "QARA"):
        generator_v3.main(["--sample_type", "sequences", "--datatype", datatype, "--task_file", tasks_file + ".pkl",
                           "--sequence_length", "96", "--output_type", "npy", "--output", out, "--seed", "5", "--backend",
                           "host"])
        a = np.load(out)
        assert a.shape == (3, 2, 96) and a.dtype.kind == "i"
        assert (a[:, 0, 0] == V["q"]).all() and (a >= 0).all() and (a < 32).all()
    txt = str(tmp_path / "seq.txt")
    data = metalang_generator_v3(datatype="QA", samples=3, sequence_length=40, output_type="txt", task_file=tasks_file + ".pkl",
                                 output=txt, seed=5, backend="host")
    assert data.shape == (3, 2, 40) and len(open(txt).read().splitlines()) == 3
    with pytest.raises(Exception, match="Must specify --output"):
        metalang_generator_v3(sample_type="tasks", samples=1, backend="host")


def test_stream_symbol_is_declared_and_bound_and_the_abi_version_stays():
    with open(os.path.join(ROOT, "include", "xeno.h")) as f:
        header = f.read()
    assert re.search(r"^int xv_metalm_stream\(", header, re.M)
    for k, v in (("QA", 0), ("QAR", 1), ("QARA", 2)):
        assert re.search(r"#define XV_METALM_%s %d\b" % (k, v), header)
    assert "xv_metalm_stream" in _lib.SIGNATURES and len(_lib.SIGNATURES["xv_metalm_stream"]) == 18
    assert _lib.ABI_VERSION == 12 and re.search(r"#define XV_ABI_VERSION 12\b", header)
    assert hasattr(_lib.load(), "xv_metalm_stream")
