"""The host restatement of the reference's AnyMDPSolverMBRL (xenoverse_amd/anymdp/mbrl.py) against the reference's own
training loop (tests/golden/mbrl_anymdp_*.npz, scripts/gen_golden_anymdp_mbrl.py), against numpy's own sums and against
the reference's update_value_matrix (tests/golden/mbrl_value_sweep.npz).  CPU only."""
import os

import numpy as np
import pytest

from util import GOLD, golden_files
from xenoverse_amd.anymdp.mbrl import MBRLHost, gauss_seidel_sweep, np_rowsum, np_tensor_std, np_tensor_sum

FILES = golden_files("mbrl_anymdp_")


def _host(g, n=1):
    return MBRLHost(n, int(g["ns"]), int(g["na"]), gamma=float(g["gamma"]), c=float(g["c"]))


def test_fixtures_present():
    names = [f.rsplit("/", 1)[-1] for f in FILES]
    assert len(FILES) >= 7, names
    for part in ("16x4", "20x3", "48x5", "64x8", "c1"):
        assert any(part in n for n in names), part
    assert all(os.path.getsize(f) < 1 << 20 for f in FILES)


@pytest.mark.parametrize("path", FILES, ids=lambda p: p.rsplit("/", 1)[-1])
def test_replay_reference_training_loop(path):
    """every action equals the reference's; vm, b, vis_cnt_sa (and est_r, vis_cnt where recorded) are bit-equal"""
    g = dict(np.load(path))
    h = _host(g)
    T = len(g["action"])
    snaps = {int(k): j for j, k in enumerate(g["snap_at"])}
    fulls = {int(k): j for j, k in enumerate(g["full_at"])}
    assert int(g["obs"][0]) == int(g["init_obs"])
    for t in range(T):
        s = g["obs"][t:t + 1]
        a = h.policy(s, g["u_policy"][t:t + 1], greedy=bool(g["is_test"][t]))
        assert int(a[0]) == int(g["action"][t]), t
        h.learn(s, a, g["next_obs"][t:t + 1], g["r"][t:t + 1], g["terminated"][t:t + 1].astype(bool),
                g["truncated"][t:t + 1].astype(bool))
        if t + 1 < T and not (g["terminated"][t] or g["truncated"][t]):
            assert g["obs"][t + 1] == g["next_obs"][t]
        if t + 1 in snaps:
            j = snaps[t + 1]
            assert np.array_equal(h.vm[0], g["snap_vm"][j]), (t, np.abs(h.vm[0] - g["snap_vm"][j]).max())
            assert np.array_equal(h.b[0], g["snap_b"][j]), t
            assert np.array_equal(h.vis_cnt_sa[0], g["snap_vis_cnt_sa"][j]), t
        if t + 1 in fulls:
            j = fulls[t + 1]
            assert np.array_equal(h.est_r[0], g["snap_est_r"][j]), t
            assert np.array_equal(h.vis_cnt[0], g["snap_vis_cnt"][j]), t
    assert len(snaps) >= 3 and len(fulls) >= 2


def test_fixtures_cover_terminal_truncated_greedy_and_both_c():
    gs = {f.rsplit("/", 1)[-1]: dict(np.load(f)) for f in FILES}
    assert sum(int(g["terminated"].sum()) for g in gs.values()) > 50
    assert sum(int(g["truncated"].sum()) for g in gs.values()) > 30
    assert sum(int(g["is_test"].sum()) for g in gs.values()) > 500
    cs = {float(g["c"]) for g in gs.values()}
    assert 0.05 in cs and 1.0 in cs
    for g in gs.values():      # every fixture ends episodes both ways or greedy steps and a two-chunk std where it can
        assert int(g["terminated"].sum() + g["truncated"].sum()) >= 3
    big = [g for g in gs.values() if int(g["ns"]) ** 2 * int(g["na"]) > 8192]
    assert len(big) >= 2


@pytest.mark.parametrize("shape", [(16, 4, 16), (20, 3, 20), (48, 5, 48), (64, 8, 64), (128, 8, 128), (12, 3, 200),
                                   (4, 4, 512)])
def test_std_and_row_sums_equal_numpy(shape):
    """numpy's chunked pairwise std and the pairwise row sums, bit for bit, on tensors of several scales and offsets"""
    rng = np.random.RandomState(sum(shape))
    xs = np.stack([rng.randn(*shape) * rng.choice([1e-4, 1.0, 1e4]) + rng.choice([0.0, 3.0, -250.0])
                   for _ in range(12)])
    xs[0] = 0.0
    xs[1] = xs[1] * (rng.random_sample(shape) < 0.05)       # mostly zero, like est_r
    std, tot, rows = np_tensor_std(xs), np_tensor_sum(xs), np_rowsum(xs)
    for k in range(len(xs)):
        assert std[k] == np.std(xs[k]), k
        assert tot[k] == np.sum(xs[k]), k
        assert np.array_equal(rows[k], np.sum(xs[k], axis=-1)), k


def test_sweep_equals_reference_update_value_matrix():
    g = dict(np.load(os.path.join(GOLD, "mbrl_value_sweep.npz")))
    shapes = set()
    for k in range(int(g["n"])):
        t, r, vm = g["t%d" % k], g["r%d" % k], g["vm%d" % k]
        out = gauss_seidel_sweep(t[None], r[None], float(g["gamma%d" % k]), vm[None])[0]
        assert np.array_equal(out, g["out%d" % k]), (k, np.abs(out - g["out%d" % k]).max())
        shapes.add(vm.shape)
    assert (20, 3) in shapes and (48, 5) in shapes


def test_init_state():
    h = MBRLHost(2, 5, 3, gamma=0.9, c=0.05)
    assert np.all(h.vm == 0.0) and np.all(h.est_r == 0.0) and np.all(h.vis_cnt == 0.01) and np.all(h.vis_cnt_sa == 1.0)
    assert np.all(h.b == (0.05 / (1.0 - 0.9)) * 0.01)


def test_terminal_slab_zeroed_after_the_update():
    """terminated into a state: its slab of vis_cnt and est_r is zeroed after (s, a, ns) was counted, even when s == ns"""
    h = MBRLHost(2, 4, 2, gamma=0.5, c=1.0)
    h.learn([1, 2], [0, 1], [3, 2], [2.0, -1.0], [False, True], [True, False])
    assert h.est_r[0, 1, 0, 3] == 2.0 / 1.01 and h.vis_cnt[0, 1, 0, 3] == 1.01
    assert np.all(h.vis_cnt[1, 2] == 0.0) and np.all(h.est_r[1, 2] == 0.0)
    assert h.vis_cnt_sa[0, 1, 0] == 2.0 and h.vis_cnt_sa[1, 2, 1] == 2.0
    # a zeroed row gives t = 0 (the 0.01 clip) and so exp_q = 0 for every action of that state
    assert np.all(h.vm[1, 2] == 0.0)


def test_b_is_a_snapshot_of_the_episode_end():
    h = MBRLHost(1, 3, 2, gamma=0.9, c=1.0)
    b0 = h.b.copy()
    h.learn([0], [1], [2], [5.0], [False], [False])
    assert np.array_equal(h.b, b0) and h.vis_cnt_sa[0, 0, 1] == 2.0        # no episode end: b stays
    h.learn([2], [0], [1], [1.0], [False], [True])
    assert not np.array_equal(h.b, b0)
    assert h.b[0, 0, 1] == (h._c * max(np.std(h.est_r[0]), 0.01)) / np.sqrt(2.0)


def test_policy_first_argmax_and_bonus():
    h = MBRLHost(3, 2, 4)
    h.vm[0, 0] = [1.0, 3.0, 3.0, 2.0]
    h.vm[1, 1] = [0.0, 0.0, 0.0, 0.0]
    h.vm[2, 0] = [0.0, 0.0, 0.0, 0.0]
    h.b[2, 0] = [1.0, 1.0, 1.0, 1.0]
    assert list(h.policy([0, 1, 0], greedy=True)) == [1, 0, 0]
    u = np.array([[0.0] * 4, [0.0] * 4, [0.1, 0.7, 0.7, 0.2]])
    assert list(h.policy([0, 1, 0], u)) == [1, 0, 1]


def test_reset_mask_and_state_round_trip():
    h = MBRLHost(4, 3, 2)
    h.learn([0] * 4, [1] * 4, [2] * 4, [1.0, 2.0, 3.0, 4.0], [False, True, False, True], [True, False, False, False])
    st = h.get_state()
    h.reset([True, False, True, False])
    assert np.all(h.vis_cnt[[0, 2]] == 0.01) and np.all(h.vis_cnt_sa[[0, 2]] == 1.0) and np.all(h.vm[[0, 2]] == 0.0)
    for x, y in zip(h.get_state(), st):
        assert np.array_equal(x[[1, 3]], y[[1, 3]])
    h.set_state(*st)
    assert all(np.array_equal(x, y) for x, y in zip(h.get_state(), st))
