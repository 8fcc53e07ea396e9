"""AnyHVAC's episode protocol without a GPU (random episode starts, restart before the failure, no-terminate training
flag): HVACHost / DiffActionHost against the reference's recorded runs (tests/golden/start_anyhvac_*.npz,
scripts/gen_golden_anyhvac_start.py) bit for bit; the choice table against numpy's own choice; the device's bounded
history against the reference's literal list; the setters; the new C-ABI symbols."""
import os
import re

import numpy as np
import pytest

import anyhvac_start_util as SU
import anyhvac_util as U
from xenoverse_amd import _lib
from xenoverse_amd.anyhvac import (HVACEnv, HVACEnvDiffAction, HVACEnvDiscreteAction, HVACHost, HVACVecEnv)
from xenoverse_amd.anyhvac import actions as A
from xenoverse_amd.anyhvac import host as H

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "xeno.h")
NEW_SYMBOLS = ("xv_anyhvac_set_start_mode", "xv_anyhvac_set_start_draws", "xv_anyhvac_start_get_state",
               "xv_anyhvac_start_set_state")
SETTERS = ("set_random_start_t", "set_generate_record", "set_overheat_no_termiated_training_only")
STEP_KEYS = ("grid", "t", "reward", "terminated", "truncated", "cool_power", "heat_power", "rest_idx", "warning_count",
             "over_heat", "over_tolerace", "energy_cost", "target_cost", "timestep", "sensor_readings", "heat_readings",
             "action_temp", "hist_len", "last_fail")


def test_every_fixture_is_there_small_with_its_margins_and_the_other_sets_are_as_they_were():
    assert sorted(SU.FILES) == sorted(SU.RUNS)
    for name in SU.RUNS:
        g = SU.load(name)[0]
        assert os.path.getsize(SU.FILES[name]) <= SU.SIZE_CAP, name
        assert float(g["eer_margin"]) >= U.MIN_EER_MARGIN and float(g["fail_margin"]) >= U.MIN_FAIL_MARGIN, name
        assert int(g["set_iter_per_step"]) == 50 and float(g["set_sec_per_iter"]) == 0.6, name
    assert float(SU.load("rl")[0]["stat_margin"]) >= 1e-4
    assert sorted(U.FILES) == sorted(U.RUNS + U.TASKS_ONLY)


def test_fixtures_reach_what_they_are_there_for():
    g = SU.load("inv")[0]
    assert g["reset_u"][0, 0] < 0.5 and g["reset_t"][0] > 3600 and g["n_steps"] == 6
    g = SU.load("choice")[0]
    assert g["reset_u"][0, 0] >= 0.5 and g["reset_t"][0] > 0 and g["n_steps"] == 6
    g = SU.load("back")[0]
    at = g["reset_at"].tolist()
    assert len(at) == 3 and at[1] > 221 and not g["action"][:250].any() and (g["action"][250:] == 1).all()
    assert not g["over_heat"][:250].any() and g["terminated"][at[1] - 1] and g["terminated"][at[2] - 1]
    assert g["reset_rest_idx"][1] != 0 and g["reset_rest_idx"][1] != g["rest_idx"][at[1] - 1]
    assert g["reset_t"][1] == g["t"][at[1] - 1] - 3000 and g["reset_hist_len"][1] == at[1] - 1
    assert g["reset_hist_len"][2] > g["reset_hist_len"][1] and g["n_steps"] - at[2] == 3      # kept, and goes on growing
    assert g["reset_rest_start"][1][g["reset_rest_idx"][1]] == g["reset_t"][1]
    assert 3 <= g["action"].shape[1] <= 6
    g = SU.load("early")[0]
    at = g["reset_at"].tolist()
    assert g["reset_hist_len"][1] < 100 and 0 < g["reset_last_fail"][1] < 3000 and g["reset_t"][1] == 0 and g["reset_t"][0] > 0
    g = SU.load("trunc")[0]
    at = g["reset_at"].tolist()
    assert g["set_max_steps"] == 40 and g["flag_overheat_no_terminated"] and not g["terminated"].any()
    fails = np.flatnonzero(g["over_tolerace"][:at[1]])
    assert len(fails) > 1 and (g["reward"][fails] == -30).all() and g["truncated"][at[1] - 1] and not g["truncated"][:at[1] - 1].any()
    assert (np.diff(g["last_fail"][fails]) > 0).all()      # every failing step moves last_fail
    assert g["reset_last_fail"][1] > 0 and g["reset_hist_len"][1] == 0 and g["reset_u"][1].any()      # branch 3
    g = SU.load("record")[0]
    assert g["flag_generate_record"] and len(g["reset_at"]) == 3 and not g["reset_hist_len"].any()
    assert ((g["reset_t"] / 30) % 1 == 0).all() and len(set(g["reset_t"].tolist())) == 3
    g = SU.load("rl")[0]
    at = g["reset_at"].tolist()
    assert g["rl"] and g["raw_action"].dtype == np.int32 and g["set_reward_mode"] == 1 and len(at) == 2
    assert g["terminated"][at[1] - 1] and g["stat_fail"][at[1] - 1] == 1 and g["reset_t"][1] == g["reset_last_fail"][1] - 3000


@pytest.mark.parametrize("name", SU.RUNS)
def test_host_replays_the_reference_bit_for_bit(name):
    """every reset's start t, rest index, rest_start row, history length, last_fail and observation; every step's record"""
    g, task, settings, flags = SU.load(name)
    h = SU.host_of(name)
    for kind, i in SU.events(g):
        if kind == "reset":
            obs = h.reset(g["reset_grid"][i], start_u=tuple(g["reset_u"][i]))[0]
            at = "%s reset %d: " % (name, i)
            mine = dict(t=np.float64(h.t), rest_idx=np.int32(h.rest_idx), hist_len=np.int32(len(h.history)),
                        last_fail=np.float64(h.last_fail_timestemp), rest_start=h.rest_start, timestep=obs["timestep"][0],
                        **{q: obs[q] for q in SU.OBS})
            for q, v in mine.items():
                assert U.same_bits(v, g["reset_" + q][i]), at + q
            continue
        a = SU.raw_action(g, i)
        delta = h.map_action(a)[1] if bool(g["rl"]) else None
        obs, r, term, trunc, info = h.step(a)
        at = "%s step %d: " % (name, i + 1)
        mine = dict(grid=h.state, t=np.float64(h.t), reward=np.float64(r), terminated=np.bool_(term), truncated=np.bool_(trunc),
                    cool_power=info["cool_power"], heat_power=info["heat_power"], rest_idx=np.int32(h.rest_idx),
                    warning_count=np.int32(h.warning_count), over_heat=np.int32(info["over_heat"]),
                    over_tolerace=np.int32(info["over_tolerace"]), energy_cost=np.float64(info["energy_cost"]),
                    target_cost=np.float64(info["target_cost"]), timestep=obs["timestep"][0],
                    hist_len=np.int32(len(h.history)), last_fail=np.float64(h.last_fail_timestemp), **{q: obs[q] for q in SU.OBS})
        assert set(mine) == set(STEP_KEYS)
        for q in STEP_KEYS:
            assert U.same_bits(mine[q], g[q][i]), at + q
        if bool(g["rl"]):
            assert U.same_bits(h.value, g["applied_value"][i]) and U.same_bits(delta, g["delta"][i]), at + "mapping"
            for q in ("reward", "cooler_power", "fail") + A.STAT_KEYS:
                assert U.same_bits(np.float64(info["step_stat"][q]), g["stat_" + q][i]), at + q


@pytest.mark.parametrize("max_t", [7, 600, 6000])
def test_choice_table_and_upper_bound_are_numpy_choice(max_t):
    """RandomState(seed).choice(arange(max_t + 1), p=the reference's weights) equals the count of table entries <= u, u the
    next random_sample() of a RandomState of the same seed; 2,000 seeds"""
    cdf = H.start_cdf(max_t)
    weights = 1.0 / ((np.arange(max_t + 1) + 1) ** 2)
    weights = weights / weights.sum()
    assert cdf.dtype == np.float64 and cdf.shape == (max_t + 1,) and cdf[-1] == 1.0 and (np.diff(cdf) > 0).all()
    values = np.arange(max_t + 1)
    seen = set()
    for seed in range(2000):
        want = np.random.RandomState(seed).choice(values, p=weights)
        got = H.choice_from_cdf(cdf, np.random.RandomState(seed).random_sample())
        assert got == int(want), seed
        seen.add(got)
    assert 0 in seen and max(seen) > 1


def test_bounded_history_is_the_capped_list():
    """the ring of 128 and its saturating count against the reference's list capped at 1,000, over 1,300 appends, the
    restore read at the stated counts (and at every count), and again after a clear"""
    for start in (0, 1):      # (a second pass after a clear: the oldest entry is no longer slot 0's first)
        ring, ref = H.BoundedHistory(), H.ListHistory()
        if start:
            for v in range(50):
                ring.append(v)
                ref.append(v)
            ring.clear()
            ref.clear()
        rng = np.random.RandomState(5 + start)
        checked = set()
        for n in range(1301):
            assert len(ring) == len(ref) == min(n, 1000)
            assert ring.restore(100) == ref.restore(100), n
            if n in (0, 1, 99, 100, 101, 999, 1000, 1300):
                checked.add(n)
                assert (ref.restore(100) is None) == (n == 0)
                if n >= 100:
                    assert ref.restore(100) == ref.items[-100]
            v = int(rng.randint(0, 320))
            ring.append(v)
            ref.append(v)
        assert checked == {0, 1, 99, 100, 101, 999, 1000, 1300}
        assert ring.count % H.HISTORY_RING == 1301 % H.HISTORY_RING and 1000 <= ring.count < H.HISTORY_WRAP
        assert ring.ring.dtype == np.int16 and ring.ring.shape == (128,) and H.HISTORY_LENGTH == 1000 and H.STEPS_BACK == 100


def test_setters_exist_on_all_six_classes_and_keywords_are_still_refused():
    for cls in (HVACHost, A.DiffActionHost, A.DiscreteActionHost, HVACVecEnv, HVACEnv, HVACEnvDiscreteAction,
                HVACEnvDiffAction):
        for name in SETTERS:
            assert callable(getattr(cls, name, None)), (cls.__name__, name)
    h = HVACHost()
    assert (h.random_start_t, h.generate_record, h.overheat_no_termiated_training_only, h.last_fail_timestemp) == (False, False, False, -1)
    h.set_random_start_t(True)
    h.set_generate_record(True)
    h.set_overheat_no_termiated_training_only(True)
    assert h.random_start_t and h.generate_record and h.overheat_no_termiated_training_only
    with pytest.raises(ValueError, match="set_random_start_t"):      # the message points to the setter
        HVACHost(random_start_t=True)
    for name in SETTERS:
        with pytest.raises(ValueError, match=name[4:]):
            HVACVecEnv(1, **{name[4:]: True})


def test_vec_env_setters_take_a_bool_or_one_per_env_before_the_device_is_touched():
    env = object.__new__(HVACVecEnv)      # (no engine: the flags are host data until a task is set)
    env.num_envs, env._h, env._start_flags = 3, None, np.zeros(3, np.uint8)
    env.set_random_start_t(True)
    env.set_overheat_no_termiated_training_only([True, False, True])
    assert env._start_flags.tolist() == [5, 1, 5] and env._start_flags.dtype == np.uint8
    env.set_generate_record(np.array([False, True, False]))
    env.set_random_start_t(False)
    assert env._start_flags.tolist() == [4, 2, 4]
    with pytest.raises(ValueError):
        env.set_generate_record([True, False])


def test_new_symbols_are_declared_and_bound_and_the_abi_version_stays():
    text = open(HEADER).read()
    assert re.search(r"#define XV_ABI_VERSION 12\b", text) and _lib.ABI_VERSION == 12
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, text), name
        assert name in _lib.SIGNATURES, name
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NEW_SYMBOLS) and lib.xv_abi_version() == 12
    assert len(_lib.AnyHVACIO.FIELDS) == 15 and len(_lib.AnyHVACState.FIELDS) == 13
    for name, value in (("RANDOM", H.START_RANDOM), ("RECORD", H.START_RECORD), ("NO_TERMINATE", H.START_NO_TERMINATE)):
        assert re.search(r"#define XV_ANYHVAC_START_%s %d\b" % (name, value), text)
    assert re.search(r"#define XV_ANYHVAC_HISTORY %d\b" % H.HISTORY_RING, text)


def test_flags_off_is_the_reset_and_step_of_before():
    """the existing `rot` run: a host whose setters were called with False equals one without, bit for bit, and both the
    recording"""
    g, task, settings, gen = U.load("rot")
    a, b = HVACHost(**settings), HVACHost(**settings)
    for name in SETTERS:
        getattr(b, name)(False)
    outs = []
    for h in (a, b):
        h.set_task(task, generate_task=gen)
        obs = h.reset(g["init_grid"])[0]
        rows = [obs["sensor_readings"], np.float64(h.t), h.rest_start.copy()]
        for k in range(int(g["n_steps"])):
            obs, r, term, trunc, info = h.step(g["action"][k])
            rows += [h.state.copy(), np.float64(h.t), np.float64(r), np.bool_(term), obs["sensor_readings"], info["cool_power"]]
            if h is a:
                assert U.same_bits(h.state, g["grid"][k]) and U.same_bits(np.float64(r), g["reward"][k])
        outs.append(rows)
    assert all(U.same_bits(x, y) for x, y in zip(*outs))
    assert a.t == g["t"][-1] and len(a.history) == int(g["n_steps"]) and a.last_fail_timestemp == -1


def test_start_probability_is_the_mixture_it_says():
    """start_t_probability against an exhaustive count over a small max_t: the inverse-CDF branch on a fine grid of u, the
    choice branch from the table"""
    max_t = 12
    cdf = H.start_cdf(max_t)
    u = (np.arange(200000) + 0.5) / 200000
    inv = np.array([H.inverse_start(x, max_t) for x in u[::40]])
    ch = np.searchsorted(cdf, u, side="right")
    for lo, hi in ((0, 0), (7, 12), (3, 5)):
        want = 0.5 * np.mean((inv >= lo) & (inv <= hi)) + 0.5 * np.mean((ch >= lo) & (ch <= hi))
        assert abs(H.start_t_probability(cdf, max_t, lo, hi) - want) < 1e-3
