"""The host restatement of the device Garnet and bandit task samplers (xenoverse_amd/anymdp/sampler_host_garnet.py): the
structure of its tasks, that its model is the reference's (the same statistics over it and over the numpy-stream
GarnetTaskSampler / _bandit, which tests/golden/garnet_8x2_seed3.npz pins to the reference, each within 5 standard errors
of its analytic value), the bandit's bounded rounds, the tables against build_tables, the refusals and the C-ABI's new
symbols.  No GPU."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import garnet_bandit_util as U
from xenoverse_amd import _lib
from xenoverse_amd.anymdp import sampler_host_garnet as sh
from xenoverse_amd.anymdp.tables import build_tables, validate_task
from xenoverse_amd.anymdp.task_sampler import GarnetTaskSampler, _bandit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- structure ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["minimum", "b_is_n", "ragged"])
def test_structure_of_the_host_garnet_tasks(name):
    S, A, b, n_tasks, m = U.GARNET[name]
    tasks = U.garnet_host(name)["tasks"]
    lower, upper = sh.max_steps_bounds(S)
    assert (lower, upper) == (100.0, {8: 101.0, 9: 101.0, 16: 128.0}[S])      # max(4 S, 100), max(min(8 S, 500), lower + 1)
    reals = set()
    for t in tasks:
        validate_task(t)
        n = t["transition"].shape[0]
        reals.add(n)
        assert (S if m is None else m) <= n <= S
        assert t["transition"].shape == t["reward"].shape == t["reward_noise"].shape == (n, A, n)
        assert ((t["transition"] != 0).sum(-1) == b).all()
        assert np.abs(t["transition"].sum(-1) - 1.0).max() < 1e-12 and t["transition"].min() >= 0.0
        sm = t["state_mapping"]
        assert sm.shape == (n,) and len(set(sm.tolist())) == n and sm.min() >= 0 and sm.max() < S
        assert lower <= t["max_steps"] < upper
        assert (t["reward_noise"] == 0).all() and t["s_0"].tolist() == [0] and t["s_0_prob"].tolist() == [1.0]
        assert len(t["s_e"]) == 0 and t["final_goal_terminate"] is False and t["task_type"] == "MDP"
        assert t["ns"] == S and t["na"] == A
    if name == "ragged":
        assert len(reals) >= 2, reals
    else:
        assert reals == {S}


def test_task_k_is_a_function_of_seed_arguments_and_k():
    kw = U.garnet_kwargs("ragged")
    whole = U.garnet_host("ragged")["tasks"]
    for k in (0, 5, 11):
        one = sh.garnet_tasks(1, task_base=k, **kw)[0]
        for key in ("transition", "reward", "state_mapping"):
            assert one[key].tobytes() == whole[k][key].tobytes()
        assert one["max_steps"] == whole[k]["max_steps"]
    other = sh.garnet_tasks(1, **dict(kw, seed=kw["seed"] + 1))[0]
    assert other["max_steps"] != whole[0]["max_steps"]


# ---- the same model as the reference's stream -------------------------------------------------------------------------------
ST_S, ST_A, ST_B, ST_N = 16, 4, 3, 40      # rows: 16 * 4 * 40 = 2,560; rewards: 40,960
ST_SEED_NUMPY, ST_SEED_HOST = 100, 0       # fixed; the numpy-stream sampler passes at its seeds on its own


def _garnet_statistics(tasks, S, A, b, sigma):
    """-> list of (name, value, analytic value, standard error)"""
    T = np.stack([t["transition"] for t in tasks]).reshape(-1, S)      # [rows, S]
    R = np.concatenate([t["reward"].reshape(-1) for t in tasks])
    rows = T.shape[0]
    out = []
    # every next state is in a row's b-subset with probability b / S, rows independent: a binomial share
    p = b / S
    for j, f in enumerate((T != 0).mean(0)):
        out.append(("chosen[%d]" % j, f, p, math.sqrt(p * (1 - p) / rows)))
    # the pieces of a random partition are exchangeable and the successors' order is independent of the cuts: the piece on the
    # row's lowest successor is distributed as the first piece, Beta(1, b - 1): mean 1 / b, variance (b - 1) / (b^2 (b + 1))
    first = T[np.arange(rows), (T != 0).argmax(1)]
    out.append(("first piece", first.mean(), 1.0 / b, math.sqrt((b - 1) / (b * b * (b + 1.0)) / rows)))
    # rewards: N(0, sigma); the sample std of N normals has standard error sigma / sqrt(2 N)
    out.append(("reward mean", R.mean(), 0.0, sigma / math.sqrt(len(R))))
    out.append(("reward std", R.std(), sigma, sigma / math.sqrt(2.0 * len(R))))
    return out


@pytest.mark.parametrize("side", ["numpy_stream", "host_restatement"])
def test_garnet_statistics_match_the_analytic_model(side):
    if side == "numpy_stream":
        tasks = [GarnetTaskSampler(ST_S, ST_A, b=ST_B, sigma=U.SIGMA, seed=ST_SEED_NUMPY + k) for k in range(ST_N)]
    else:
        tasks = sh.garnet_tasks(ST_N, ST_S, ST_A, None, ST_B, U.SIGMA, seed=ST_SEED_HOST)
    for name, value, want, se in _garnet_statistics(tasks, ST_S, ST_A, ST_B, U.SIGMA):
        assert abs(value - want) < 5.0 * se, (side, name, value, want, se)


def test_ragged_real_state_counts_cover_their_range():
    """n = m + floor(u (S - m + 1)): uniform on m .. S"""
    S, m, N = 16, 8, 900
    ns = np.array([sh.garnet_task(3, k, S, 2, m, 2, 0.1)["transition"].shape[0] for k in range(0, N)])
    assert ns.min() == m and ns.max() == S
    p = 1.0 / (S - m + 1)
    for v in range(m, S + 1):
        assert abs((ns == v).mean() - p) < 5.0 * math.sqrt(p * (1 - p) / N), v


# ---- bandits ------------------------------------------------------------------------------------------------------------------
BD_N = 2000


def _bandit_shares(base, noise_base):
    n = len(base)
    p = 1.0 - math.exp(-0.05)
    return [("base == 0.05", float((base == 0.05).mean()), p, math.sqrt(p * (1 - p) / n)),
            ("noise_base == 0", float((noise_base == 0).mean()), 0.5, math.sqrt(0.25 / n))]


class _RecordingStream(object):
    """a RandomState that keeps what `exponential` returned: _bandit's base is not in the task it returns"""

    def __init__(self, rng):
        self.rng, self.exponentials = rng, []

    def exponential(self, scale):
        self.exponentials.append(self.rng.exponential(scale))
        return self.exponentials[-1]

    def uniform(self, *args, **kwargs):
        return self.rng.uniform(*args, **kwargs)


@pytest.mark.parametrize("side", ["numpy_stream", "host_restatement"])
def test_bandit_statistics_match_the_analytic_model(side):
    A = 2      # two arms: the numpy stream's unbounded loop ends quickly whatever base is
    if side == "numpy_stream":
        rng = _RecordingStream(np.random.RandomState(5))
        tasks = [_bandit(rng, A) for _ in range(BD_N)]
        base = np.clip(np.array(rng.exponentials), 0.05, 2.0)      # _bandit's first draw
        assert len(base) == BD_N
        noise_base = np.array([(t["reward_noise"] / t["reward"]).max() for t in tasks])      # reward_noise = noise_base * reward
        stds = [np.std(t["reward"]) for t in tasks]
    else:
        st, tasks, recs = sh.bandit_candidates(1, 0, BD_N, A, 1024)
        assert (st == 0).all()
        base = np.array([r["base"] for r in recs])
        noise_base = np.array([r["noise_base"] for r in recs])
        stds = [np.std(t["reward"]) for t in tasks]
        for t, r in zip(tasks, recs):
            assert t["reward_noise"].tobytes() == (r["noise_base"] * t["reward"]).tobytes()
            assert (t["transition"] == 1).all() and t["transition"].shape == (1, A, 1) and t["max_steps"] == 1
            assert 0.5 * r["base"] <= t["reward"].min() and t["reward"].max() <= r["base"]
    assert min(stds) > 0.01
    for name, value, want, se in _bandit_shares(base, noise_base):
        assert abs(value - want) < 5.0 * se, (side, name, value, want, se)


def test_np_std_is_numpys_std():
    rng = np.random.RandomState(0)
    for A in (2, 5, 7, 8, 9, 16, 63, 64):
        for _ in range(20):
            x = rng.uniform(0.025, 0.05, size=(1, A, 1))
            assert sh.np_std(x) == float(np.std(x)), A


def test_bandit_rounds_are_bounded_and_task_k_does_not_depend_on_the_batch():
    st, tasks, recs = U.bandit_host(5)
    assert (st == 0).any() and (st == 1).any()
    for s, t, r in zip(st, tasks, recs):
        assert (t is None) == (s == 1)
        assert len(r["stds"]) == (U.BANDIT_ROUNDS if s == 1 else r["round"] + 1)
        assert (r["stds"][:-1] <= 0.01).all() and (r["stds"][-1] > 0.01) == (s == 0)
    a, hist_a = sh.bandit_tasks(20, 5, U.BANDIT_SEED, U.BANDIT_ROUNDS, batch=1)
    b, hist_b = sh.bandit_tasks(20, 5, U.BANDIT_SEED, U.BANDIT_ROUNDS, batch=64)
    assert hist_a.tolist() == hist_b.tolist() and hist_a[0] == 20 and hist_a[1] > 0
    for x, y in zip(a, b):
        assert x["reward"].tobytes() == y["reward"].tobytes() and x["reward_noise"].tobytes() == y["reward_noise"].tobytes()


# ---- tables -------------------------------------------------------------------------------------------------------------------
def _assert_tables_equal(got, want):
    for k, v in want.items():
        if isinstance(v, np.ndarray):
            assert got[k].dtype == v.dtype and got[k].shape == v.shape, k
            assert got[k].tobytes() == v.tobytes(), k
        else:
            assert got[k] == v, k


@pytest.mark.parametrize("name", ["minimum", "b_is_n", "ragged"])
def test_sample_tables_equals_build_tables_of_the_dicts(name):
    S, A, b, n_tasks, m = U.GARNET[name]
    tab = U.garnet_host(name)
    tasks = tab["tasks"]
    want = build_tables(tasks, s0_max=4)
    assert want["S"] == S and want["s0_max"] == 4
    _assert_tables_equal(tab, want)
    assert tab["n_real"].tolist() == [t["transition"].shape[0] for t in tasks]
    for key in ("transition", "reward", "reward_noise"):
        assert tab[key].shape == (n_tasks, S, A, S)
        for i, t in enumerate(tasks):
            n = t[key].shape[0]
            assert tab[key][i, :n, :, :n].tobytes() == t[key].tobytes()
            assert (tab[key][i, n:] == 0).all() and (tab[key][i, :, :, n:] == 0).all()


def test_a_batch_without_a_full_size_task_is_padded_to_the_samplers_size():
    kw = dict(U.garnet_kwargs("ragged"))
    k = next(k for k, n in enumerate(U.garnet_host("ragged")["n_real"]) if n < 16)
    tab = sh.sample_tables(1, task_base=k, **kw)
    assert tab["S"] == 16 and tab["rows"].shape[1] == 16
    whole = U.garnet_host("ragged")
    for key in ("rows", "cdf", "rs", "state_map", "term_mask", "max_steps", "transition"):
        assert tab[key][0].tobytes() == whole[key][k].tobytes(), key


def test_bandit_tables_are_the_two_state_embedding_of_build_tables():
    tab = sh.sample_bandit_tables(6, 5, seed=U.BANDIT_SEED, max_rounds=U.BANDIT_ROUNDS)
    tasks, hist = sh.bandit_tasks(6, 5, U.BANDIT_SEED, U.BANDIT_ROUNDS)
    _assert_tables_equal(tab, build_tables(tasks, s0_max=4))
    assert tab["S"] == 2 and tab["rows"].shape == (6, 2, 5, 2, 16) and (tab["obs_space"] == 1).all()
    assert (tab["max_steps"] == 1).all() and (tab["term_mask"] == 2).all()
    assert tab["stats"]["status"] == {"accepted": int(hist[0]), "no_spread": int(hist[1])}
    for t in tasks:
        validate_task(t)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw, word", [
    (dict(state_space=7), "state_space"), (dict(state_space=513), "state_space"), (dict(action_space=1), "action_space"),
    (dict(action_space=65), "action_space"), (dict(b=1), "b = 1"), (dict(b=33), "b = 33"),
    (dict(state_space=16, min_state_space=8, b=9), "b = 9"), (dict(state_space=16, min_state_space=7), "min_state_space")])
def test_garnet_limits_are_refused_by_name(kw, word):
    args = dict(state_space=64, action_space=5, min_state_space=None, b=2)
    args.update(kw)
    with pytest.raises(ValueError, match=word):
        sh.check_garnet_args(**args)


def test_bandit_limits_are_refused_by_name():
    for A in (1, 65):
        with pytest.raises(ValueError, match="action_space"):
            sh.check_bandit_args(A, 64)
    for R in (0, sh.ROUNDS_MAX + 1):
        with pytest.raises(ValueError, match="max_rounds"):
            sh.check_bandit_args(5, R)


def test_public_names_are_exported():
    from xenoverse_amd import anymdp
    for name in ("sample_garnet_tasks_device", "sample_bandit_tasks_device", "task_dicts_from_device", "sample_tasks_device"):
        assert callable(getattr(anymdp, name))


def test_symbols_are_declared_and_bound_and_the_abi_version_stays():
    header = open(os.path.join(ROOT, "include", "xeno.h")).read()
    for name, n_args in (("xv_anymdp_sample_garnet", 20), ("xv_anymdp_sample_bandits", 16)):
        assert re.search(r"\bint %s\(" % name, header) and len(_lib.SIGNATURES[name]) == n_args
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert re.search(r"#define XV_ABI_VERSION 12\b", header) and _lib.ABI_VERSION == 12
    assert re.search(r"#define XV_ANYMDP_GARNET_B_MAX %d\b" % sh.B_MAX, header)
    assert "#define XV_ANYMDP_BANDIT_ROUNDS_MAX (1 << 16)" in header and sh.ROUNDS_MAX == 1 << 16
