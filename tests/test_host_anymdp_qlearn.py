"""The host restatement of the reference's AnyMDPSolverQ (xenoverse_amd/anymdp/qlearner.py) against the reference's own
training loop (tests/golden/qlearn_anymdp_*.npz, scripts/gen_golden_anymdp_qlearn.py) and on its edge cases.  CPU only."""
import numpy as np
import pytest

from util import golden_files
from xenoverse_amd.anymdp.qlearner import QLearnerHost, np_sum, policy_cdf

FILES = golden_files("qlearn_anymdp_")


def _learner(g, n=1):
    ql = QLearnerHost(n, int(g["ns"]), int(g["na"]), gamma=float(g["gamma"]), alpha=float(g["alpha"]),
                      max_steps=int(g["learner_max_steps"]))
    ql.set_state(g["init_q"][None], g["init_sa"][None], g["init_s"][None])
    return ql


def test_fixtures_present():
    names = [f.rsplit("/", 1)[-1] for f in FILES]
    assert len(FILES) >= 7, names
    assert any("64x8" in n for n in names) and any("m1" in n for n in names)
    assert any(int(np.load(f)["na"]) > 8 for f in FILES), names      # a row the pairwise sum takes in eight partial sums


@pytest.mark.parametrize("path", FILES, ids=lambda p: p.rsplit("/", 1)[-1])
def test_replay_reference_training_loop(path):
    """every action equals the reference's; Q, sa_visits and s_visits are bit-equal at every snapshot"""
    g = dict(np.load(path))
    ql = _learner(g)
    T = len(g["action"])
    snaps = {int(k): j for j, k in enumerate(g["snap_at"])}
    assert int(g["obs"][0]) == int(g["init_obs"])
    for t in range(T):
        s = g["obs"][t:t + 1]
        a = ql.policy(s, g["u_policy"][t:t + 1], greedy=bool(g["is_test"][t]))
        assert int(a[0]) == int(g["action"][t]), t
        ql.learn(s, a, g["next_obs"][t:t + 1], g["r"][t:t + 1], g["terminated"][t:t + 1].astype(bool),
                 g["truncated"][t:t + 1].astype(bool))
        if t + 1 < T and not (g["terminated"][t] or g["truncated"][t]):
            assert g["obs"][t + 1] == g["next_obs"][t]
        if t + 1 in snaps:
            j = snaps[t + 1]
            assert np.array_equal(ql.q[0], g["snap_q"][j]), (t, np.abs(ql.q[0] - g["snap_q"][j]).max())
            assert np.array_equal(ql.sa_visits[0], g["snap_sa"][j])
            assert np.array_equal(ql.s_visits[0], g["snap_s"][j])
    assert len(snaps) >= 3


def test_fixtures_cover_terminal_truncated_greedy_and_caps():
    gs = {f.rsplit("/", 1)[-1]: dict(np.load(f)) for f in FILES}
    assert sum(int(g["terminated"].sum()) for g in gs.values()) > 100
    assert sum(int(g["truncated"].sum()) for g in gs.values()) > 10
    assert sum(int(g["is_test"].sum()) for g in gs.values()) > 500
    m1 = gs["qlearn_anymdp_16x4_m1.npz"]
    assert int(m1["learner_max_steps"]) == 1
    M = 1
    assert (m1["snap_sa"][-1] > 1000 * (M + 1) - M).any()           # lr = sqrt(1e-3) on these pairs
    assert (m1["snap_s"][-1] >= 9 * M + 10).any()                    # stiffness = 10
    assert int(gs["qlearn_anymdp_64x8_seed1.npz"]["na"]) >= 8
    wide = [g for g in gs.values() if int(g["na"]) > 8]
    assert len(wide) >= 1
    for g in wide:
        assert int(g["terminated"].sum()) > 0 and int(g["is_test"].sum()) > 0


def test_np_sum_matches_numpy():
    rng = np.random.RandomState(1)
    for A in range(1, 65):
        x = rng.randn(16, A) * rng.choice([1e-6, 1.0, 1e6], (16, 1))
        s = np_sum(x)
        for i in range(16):
            assert s[i] == np.sum(x[i]) and s[i] / A == np.mean(x[i])


def test_all_equal_row_is_uniform():
    """std = 0 falls to the 1e-2 floor: v = 0 everywhere and every action has probability 1 / A"""
    for A in (2, 4, 8, 13):
        cdf = policy_cdf(np.full((1, A), 7.25), [1], 4000)[0]
        assert np.array_equal(cdf, np.cumsum(np.full(A, 1.0 / A)) / np.cumsum(np.full(A, 1.0 / A))[-1])
        ql = QLearnerHost(3, 5, A)
        u = np.array([0.0, 0.5, 1.0 - 1e-12])
        assert list(ql.policy([0, 1, 2], u)) == [0, A // 2, A - 1]


def test_terminal_row_zeroed_then_revisited():
    ql = QLearnerHost(1, 4, 3, gamma=0.9, alpha=0.5, max_steps=10)
    q0 = 1.0 / (1.0 - 0.9)
    ql.learn([0], [1], [2], [1.5], [True])
    assert np.array_equal(ql.q[0, 2], np.zeros(3))
    lr = np.sqrt(max(11 / 11, 1e-3))
    assert ql.q[0, 0, 1] == q0 + 0.5 * lr * (1.5 - q0)
    # a later non-terminal step into that state bootstraps from the zeroed row
    q01 = ql.q[0, 0, 1]
    ql.learn([0], [1], [2], [0.25], [False])
    lr2 = np.sqrt(max(11 / 12, 1e-3))
    assert ql.q[0, 0, 1] == q01 + 0.5 * lr2 * ((0.25 + 0.9 * 0.0) - q01)
    # revisiting the state itself: its row is learned again from zero
    ql.learn([2], [0], [3], [1.0], [False])
    assert ql.q[0, 2, 0] == 0.0 + 0.5 * 1.0 * ((1.0 + 0.9 * ql.q[0, 3].max()) - 0.0)
    assert ql.sa_visits[0, 0, 1] == 3 and ql.s_visits[0, 0] == 3 and ql.s_visits[0, 2] == 2


def test_truncated_bootstraps():
    a = QLearnerHost(1, 3, 2, gamma=0.5)
    b = QLearnerHost(1, 3, 2, gamma=0.5)
    a.learn([0], [0], [1], [1.0], [False], [True])
    b.learn([0], [0], [1], [1.0], [False], [False])
    assert np.array_equal(a.q, b.q) and a.q[0, 0, 0] == 2.0 + 0.5 * 1.0 * ((1.0 + 0.5 * 2.0) - 2.0)
    assert np.array_equal(a.q[0, 1], [2.0, 2.0])      # truncation does not zero the row


def test_caps():
    """lr floor sqrt(1e-3) once sa_visits > 1000 (M + 1) - M; stiffness 10 once s_visits >= 9 M + 10"""
    ql = QLearnerHost(2, 2, 2, gamma=0.5, alpha=1.0, max_steps=1)
    ql.sa_visits[:, 0, 0] = [1999, 5000]
    ql.learn([0, 0], [0, 0], [1, 1], [0.0, 0.0], [True, True])
    assert ql.q[0, 0, 0] == 2.0 + np.sqrt(2.0 / 2000.0) * (0.0 - 2.0)
    assert ql.q[1, 0, 0] == 2.0 + np.sqrt(1e-3) * (0.0 - 2.0)
    q = np.array([[0.0, 1.0], [0.0, 1.0]])
    c_cap = policy_cdf(q, [19, 10 ** 6], 1)
    assert np.array_equal(c_cap[0], c_cap[1])
    assert not np.array_equal(policy_cdf(q, [18], 1)[0], c_cap[0])


def test_greedy_ties_take_the_first_argmax():
    ql = QLearnerHost(3, 2, 5)
    ql.q[0, 0] = [1.0, 3.0, 3.0, 2.0, 3.0]
    ql.q[1, 1] = [4.0, 4.0, 4.0, 4.0, 4.0]
    ql.q[2, 0] = [-1.0, -2.0, -1.0, -5.0, -1.0]
    assert list(ql.policy([0, 1, 0], greedy=True)) == [1, 0, 0]


def test_reset_mask_and_state_round_trip():
    ql = QLearnerHost(4, 3, 2)
    ql.learn([0] * 4, [1] * 4, [2] * 4, [1.0, 2.0, 3.0, 4.0], [False] * 4)
    st = ql.get_state()
    ql.reset([True, False, True, False])
    assert np.all(ql.q[[0, 2]] == 1.0 / (1.0 - 0.99)) and np.all(ql.sa_visits[[0, 2]] == 1)
    assert np.array_equal(ql.q[[1, 3]], st[0][[1, 3]]) and np.array_equal(ql.sa_visits[[1, 3]], st[1][[1, 3]])
    ql.set_state(*st)
    assert all(np.array_equal(x, y) for x, y in zip(ql.get_state(), st))
