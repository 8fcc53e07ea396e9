"""The MetaLMV3 training streams on the device (MetaLMV3VecEnv.stream, csrc/metalm.hip metalm_stream_kernel) against the
reference's recorded generate_data_v3_single_task_* runs (tests/golden/metalmstream_*.npz) and, bit for bit, against the
loop of policy() / step() calls spliced in Python — the path the fused label arithmetic and the tick layout are held to.

The band is the one of tests/test_gpu_metalm.py: a device token may differ from the reference's only at a draw whose margin
or an argmax whose gap is below TAU = 1e-9; no fixture has one below 1e-8, so every token must be equal.  The reward is
held to 5e-9 relative to max(1, |r|), as there; the replay prints the worst deviation it finds (measured: 7.8e-15 over
the five fixtures, profiles/metalm_stream_replay.txt)."""
import numpy as np
import pytest

from metalm_stream_util import FILES, PASSES, fixture_id, load, row_of, smallest_margin, splice
from util import to_np as _np
from xenoverse_amd.metalang import MetaLMV3VecEnv, TaskSamplerV3
from xenoverse_amd.metalang.lm_env import XV_DEVERR_LENGTH
from xenoverse_amd.metalang.stream_host import default_T_choices

pytestmark = pytest.mark.gpu
TAU = 1e-9
REWARD_RTOL = 5e-9      # tests/test_gpu_metalm.py: 1e3 PPL_RTOL
MAX_LEN = 640           # the longest pass of any fixture has 609 tokens
STATE = ("query", "query_len", "cache", "steps")


def _per(datatype):
    return 2 if datatype == "QARA" else 1


@pytest.mark.parametrize("path", FILES, ids=fixture_id)
def test_reference_replay(path):
    g, task = load(path)
    assert smallest_margin(g) >= TAU      # nothing is left out
    datatype, L, rounds = str(g["datatype"]), int(g["L"]), int(g["rounds"])
    K = len(g["reward"])
    assert K == rounds * _per(datatype)
    env = MetaLMV3VecEnv(1, max_len=MAX_LEN)
    env.set_task(task)
    u = np.full((1, MAX_LEN + 1), 0.5)
    u[0, :len(g["u_reset"])] = g["u_reset"]
    env.reset(draws=dict(u_query=u))
    draws = {}
    for key in PASSES:
        draws[key] = np.full((1, K, MAX_LEN + 1), 0.5)
        draws[key][0, :, :g[key].shape[1]] = g[key]
    data, label, info = env.stream(datatype, L, T_choices=g["T_choices"], t_index=g["t_index"].reshape(1, K),
                                   max_rounds=rounds, draws=draws)
    assert str(data.dtype) == "torch.int32" and tuple(data.shape) == tuple(label.shape) == (1, L)
    flags = env.check_errors()
    data, label = _np(data)[0], _np(label)[0]
    wrong = [(n, int(np.argmax(a != b))) for n, a, b in (("data", data, g["data"]), ("label", label, g["label"]))
             if not np.array_equal(a, b)]
    r_dev, r_ref = _np(info["reward"])[0], g["reward"]
    if datatype == "QA":
        worst = 0.0
        assert not r_dev.any() and (_np(info["t_index"]) == -1).all()
    else:
        worst = float(np.max(np.abs(r_dev - r_ref) / np.maximum(1.0, np.abs(r_ref))))
        assert np.array_equal(_np(info["t_index"])[0], g["t_index"])
    print("%s: %d + %d tokens compared, differing %s; worst relative deviation of the reward %.3e" % (
        fixture_id(path), L, L, wrong, worst))
    assert not wrong      # the cap on left-out tokens is zero
    assert worst <= REWARD_RTOL
    assert int(_np(info["filled"])[0]) == L and int(_np(info["rounds"])[0]) == rounds
    assert flags == 0
    env.close()


def _stepwise(env, first_query, datatype, L, T_choices, t_index, max_rounds):
    """the path without stream(): rounds of policy() / step() on the whole batch, spliced per env in Python until the env's
    data has L tokens or max_rounds rounds are done -> data, label [N, L], reward [N, K], rounds, filled [N], and every
    env's state (get_state's rows) as its own last round left it.  Envs that are done keep stepping; nothing of that is
    used."""
    n_env, per = env.num_envs, _per(datatype)
    K = max_rounds * per
    obs = [[int(t) for t in _np(first_query[0])[e, :int(_np(first_query[1])[e])]] for e in range(n_env)]
    streams = [([], []) for _ in range(n_env)]
    reward = np.zeros((n_env, K))
    rounds = np.zeros(n_env, np.int32)
    state = {k: [None] * n_env for k in STATE}
    live = list(range(n_env))
    k = 0
    while live:
        subs = [[] for _ in range(n_env)]
        for sub in range(per):
            T = 1.0e-3 if datatype == "QA" else np.asarray(T_choices)[t_index[:, k]]
            answer, answer_len = env.policy(T)
            nxt, r, _, _, info = env.step(answer, answer_len, cached=(per == 2 and sub == 0))
            a, n, lab, r = _np(answer), _np(answer_len), _np(info["label"]), _np(r)
            for e in live:
                subs[e].append(([int(t) for t in a[e, :n[e]]], [int(t) for t in lab[e, :n[e] + 1]], float(r[e])))
                reward[e, k] = r[e]
            k += 1
        q, qn = _np(nxt[0]), _np(nxt[1])
        st = {key: _np(v) for key, v in env.get_state().items() if key != "tick"}
        for e in list(live):
            splice(datatype, obs[e], subs[e], streams[e])
            obs[e] = [int(t) for t in q[e, :qn[e]]]
            rounds[e] += 1
            if len(streams[e][0]) >= L or rounds[e] >= max_rounds:
                live.remove(e)
                for key in STATE:
                    state[key][e] = st[key][e].copy()
    if datatype == "QA":
        reward[:] = 0.0      # stream() forms no reward there
    data = np.stack([row_of(s[0], L) for s in streams])
    label = np.stack([row_of(s[1], L) for s in streams])
    filled = np.array([min(len(s[0]), L) for s in streams], np.int32)
    return data, label, reward, rounds, filled, {key: np.stack(v) for key, v in state.items()}


def _pair(n_env, tasks, eti, max_len, seed, base=0):
    envs = []
    for _ in range(2):
        env = MetaLMV3VecEnv(n_env, max_len=max_len, seed=seed, env_id_base=base)
        env.set_task(tasks, eti)
        envs.append(env)
    return envs


def _fused_against_stepwise(n_env, tasks, eti, max_len, datatype, L, max_rounds=None, seed=31):
    """stream() with drawn temperatures on one env; the same on a second env of the same seed, tasks and starting tick by
    policy() / step().  Everything must be equal by ==.  -> what stream() returned, as numpy, and the flags"""
    fused, plain = _pair(n_env, tasks, eti, max_len, seed)
    choices = default_T_choices()
    fused.reset()
    first = plain.reset()
    tick0 = fused.engine.tick
    assert tick0 == plain.engine.tick
    data, label, info = fused.stream(datatype, L, max_rounds=max_rounds)
    K = int(info["reward"].shape[1])
    assert fused.engine.tick == tick0 + 2 * K      # known on the host, however many rounds an env took
    got = dict(data=_np(data), label=_np(label), **{k: _np(v) for k, v in info.items()})
    want = _stepwise(plain, first, datatype, L, choices, got["t_index"], K // _per(datatype))
    w_data, w_label, w_reward, w_rounds, w_filled, w_state = want
    assert np.array_equal(got["rounds"], w_rounds) and np.array_equal(got["filled"], w_filled)
    assert np.array_equal(got["data"], w_data)
    assert np.array_equal(got["label"], w_label)
    assert np.array_equal(got["reward"], w_reward)      # ==: the fused label pass is the separate one bit for bit
    ran = np.arange(K)[None, :] < (got["rounds"] * _per(datatype))[:, None]
    assert ((got["t_index"] >= 0) == (ran & (datatype != "QA"))).all() and (got["t_index"] < len(choices)).all()
    st = fused.get_state()
    for key in STATE:
        assert np.array_equal(_np(st[key]), w_state[key]), key
    flags = fused.check_errors()
    assert flags == plain.check_errors()
    fused.close()
    plain.close()
    return got, flags


def test_drawn_temperature_index_is_the_documented_philox_draw():
    """min(floor(u n), n - 1) with u = xv_u53 of words 0, 1 of the Philox block keyed by (seed, env_id_base + env, the
    policy's tick of sub-step k = tick + 2 k, purpose 9, sub = pass kind 5 << 16 | position 0), recomputed on the host"""
    import oracle
    seed, base, n_env = 77, 5, 6
    env = MetaLMV3VecEnv(n_env, max_len=256, seed=seed, env_id_base=base)
    env.set_task(TaskSamplerV3(seed=17))
    env.reset()
    tick0 = env.engine.tick
    for choices in (default_T_choices(), np.array([0.5, 1.0, 2.0])):
        tick = env.engine.tick
        data, label, info = env.stream("QARA", 96, T_choices=choices)
        got, rounds = _np(info["t_index"]), _np(info["rounds"])
        for e in range(n_env):
            for k in range(2 * int(rounds[e])):
                w = oracle.env_draw_sub(seed, base + e, tick + 2 * k, 9, 5 << 16)
                u = oracle.u53(w[0], w[1])
                assert got[e, k] == min(int(np.floor(u * len(choices))), len(choices) - 1), (e, k)
            assert (got[e, 2 * int(rounds[e]):] == -1).all()
    assert tick0 + 1 < env.engine.tick and env.check_errors() == 0
    env.close()


@pytest.mark.parametrize("datatype", ["QA", "QAR", "QARA"])
def test_fused_equals_step_by_step_bit_for_bit(datatype):
    tasks = [TaskSamplerV3(seed=900 + k) for k in range(6)]
    got, flags = _fused_against_stepwise(48, tasks, (np.arange(48) % 6).astype(np.int32), 256, datatype, 512)
    assert flags == 0 and (got["filled"] == 512).all() and len(set(got["rounds"].tolist())) > 1
    if datatype != "QA":
        assert len(np.unique(got["t_index"][:, 0])) > 4 and len(np.unique(got["reward"][:, 0])) > 24


@pytest.mark.parametrize("datatype", ["QA", "QAR", "QARA"])
def test_fused_equals_step_by_step_at_an_odd_size(datatype):
    """(100, 12, 24): V is no multiple of 64, so the second vocabulary column is partly masked, and H is below a wave"""
    tasks = [TaskSamplerV3(100, 12, 24, seed=950 + k) for k in range(4)]
    # max_len 1024: no pass is cut, so the envs that step on after their stream is full raise no flag of their own
    got, flags = _fused_against_stepwise(8, tasks, (np.arange(8) % 4).astype(np.int32), 1024, datatype, 256)
    assert flags == 0 and (got["filled"] == 256).all()


def test_wide_vocabulary_fused_equals_step_by_step():
    """(256, 16, 64): all four vocabulary columns, the tables read through L2"""
    got, flags = _fused_against_stepwise(1, [TaskSamplerV3(256, 16, 64, seed=8)], np.zeros(1, np.int32), 1024, "QARA", 1024)
    assert flags == 0 and got["filled"][0] == 1024


def test_an_env_does_not_depend_on_its_batch():
    tasks = [TaskSamplerV3(seed=970 + k) for k in range(16)]
    whole = MetaLMV3VecEnv(16, max_len=256, seed=7)
    whole.set_task(tasks)
    whole.reset()
    data, label, info = whole.stream("QAR", 256)
    assert whole.check_errors() == 0
    for i in (3, 14):
        one = MetaLMV3VecEnv(1, max_len=256, seed=7, env_id_base=i)
        one.set_task(tasks[i])
        one.reset()
        d1, l1, i1 = one.stream("QAR", 256)
        assert np.array_equal(_np(d1)[0], _np(data)[i]) and np.array_equal(_np(l1)[0], _np(label)[i])
        for k in ("filled", "rounds", "reward", "t_index"):
            assert np.array_equal(_np(i1[k])[0], _np(info[k])[i]), k
        one.close()
    whole.close()


@pytest.mark.parametrize("datatype", ["QA", "QAR", "QARA"])
@pytest.mark.parametrize("L", [1, 3])
def test_a_length_below_the_first_round(datatype, L):
    got, flags = _fused_against_stepwise(4, [TaskSamplerV3(seed=12)], np.zeros(4, np.int32), 256, datatype, L)
    assert flags == 0 and (got["rounds"] == 1).all() and (got["filled"] == L).all()
    assert (got["data"][:, 0] == 1).all()      # q


def test_max_rounds_ends_the_stream_early_and_leaves_zeros():
    got, flags = _fused_against_stepwise(4, [TaskSamplerV3(seed=13)], np.zeros(4, np.int32), 256, "QAR", 512, max_rounds=2)
    assert flags == 0 and (got["rounds"] == 2).all() and (got["filled"] < 512).all() and (got["filled"] >= 10).all()
    for e in range(4):
        n = int(got["filled"][e])
        assert (got["data"][e, :n] == 0).sum() == 4      # s twice per round, nothing else is 0
        assert not got["data"][e, n:].any() and not got["label"][e, n + 2:].any()     # the label runs one ahead per round
    assert got["reward"].shape == (4, 2)


def test_cut_passes_are_spliced_as_they_were_cut():
    got, flags = _fused_against_stepwise(8, [TaskSamplerV3(seed=14)], np.zeros(8, np.int32), 8, "QARA", 256)
    assert flags == XV_DEVERR_LENGTH and (got["filled"] == 256).all()


def test_ordinary_calls_go_on_from_the_state_the_stream_left():
    task = TaskSamplerV3(seed=15)
    fused, plain = _pair(1, [task], np.zeros(1, np.int32), 256, 41)
    fused.reset()
    first = plain.reset()
    tick0 = plain.engine.tick
    data, label, info = fused.stream("QAR", 64)
    K = int(info["reward"].shape[1])
    _stepwise(plain, first, "QAR", 64, default_T_choices(), _np(info["t_index"]), K)
    plain.engine.tick = tick0 + 2 * K      # the ticks stream() reserves whatever it uses
    out = []
    for env in (fused, plain):
        answer, answer_len = env.policy(0.7)
        obs, r, _, _, inf = env.step(answer, answer_len)
        out.append([_np(x).copy() for x in (answer, answer_len, obs[0], obs[1], r, inf["label"], inf["steps"])])
        assert env.check_errors() == 0
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    assert int(out[0][6][0]) == int(_np(info["rounds"])[0]) + 1
    fused.close()
    plain.close()


def test_bad_arguments_raise_before_any_launch():
    env = MetaLMV3VecEnv(2, max_len=16, seed=1)
    env.set_task(TaskSamplerV3(seed=16))
    env.reset()
    env.check_errors()      # the query of reset() may be cut at max_len = 16: not this test's matter
    before = env.get_state()
    tick = env.engine.tick
    with pytest.raises(ValueError, match="datatype must be one of"):
        env.stream("QRA", 64)
    for L in (0, -5, 2.5):
        with pytest.raises(ValueError, match="L must be an integer of at least 1"):
            env.stream("QAR", L)
    with pytest.raises(ValueError, match="max_rounds must be an integer of at least 1"):
        env.stream("QAR", 64, max_rounds=0)
    with pytest.raises(ValueError, match=r"t_index must have shape \(2, 3\)"):
        env.stream("QAR", 64, max_rounds=3, t_index=np.zeros((2, 4), np.int32))
    with pytest.raises(ValueError, match=r"t_index must have shape \(2, 6\)"):
        env.stream("QARA", 64, max_rounds=3, t_index=np.zeros((2, 3), np.int32))
    with pytest.raises(ValueError, match="t_index must be an integer array"):
        env.stream("QAR", 64, max_rounds=3, t_index=np.zeros((2, 3)))
    with pytest.raises(ValueError, match="indices into the 20 T_choices"):
        env.stream("QAR", 64, max_rounds=3, t_index=np.full((2, 3), 20, np.int32))
    with pytest.raises(ValueError, match=r"draws\['u_low'\] must have shape \(2, 3, 17\)"):
        env.stream("QAR", 64, max_rounds=3, draws=dict(u_low=np.zeros((2, 17))))
    with pytest.raises(ValueError, match="T_choices must be"):
        env.stream("QAR", 64, T_choices=[1.0, -2.0])
    after = env.get_state()
    assert env.engine.tick == tick and all(np.array_equal(_np(before[k]), _np(after[k])) for k in STATE)
    assert env.check_errors() == 0
    env.close()
