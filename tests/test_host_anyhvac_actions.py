"""AnyHVAC's RL action spaces without a GPU: actions.py (DiscreteActionHost, DiffActionHost) against the reference's
recorded runs (tests/golden/act_anyhvac_*.npz, scripts/gen_golden_anyhvac_actions.py), bit for bit; the new C-ABI symbols;
the refusals."""
import os
import re

import numpy as np
import pytest

import anyhvac_act_util as AU
import anyhvac_util as U
from xenoverse_amd import _lib
from xenoverse_amd.anyhvac import HVACHost, HVACVecEnv
from xenoverse_amd.anyhvac import actions as A

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "xeno.h")
NEW_SYMBOLS = ("xv_anyhvac_set_action_mode", "xv_anyhvac_step_mapped", "xv_anyhvac_step_mapped_injected",
               "xv_anyhvac_rollout_mapped", "xv_anyhvac_act_get_state", "xv_anyhvac_act_set_state")


def test_every_fixture_is_there_under_the_cap_with_its_margins():
    assert sorted(AU.FILES) == sorted(AU.RUNS)
    for name in AU.RUNS:
        g = AU.load(name)[0]
        assert os.path.getsize(AU.FILES[name]) <= AU.SIZE_CAP, name
        assert float(g["stat_margin"]) >= AU.MIN_STAT_MARGIN, name
        assert float(g["eer_margin"]) >= U.MIN_EER_MARGIN and float(g["fail_margin"]) >= U.MIN_FAIL_MARGIN, name
        assert AU.same_bits(g["cost_table"], A.COST_TABLE), name
    # the closed sets of the env's and the teachers' fixtures are as they were
    assert sorted(U.FILES) == sorted(U.RUNS + U.TASKS_ONLY)


def test_fixtures_reach_what_they_are_there_for():
    g = AU.load("diff_md")[0]
    target = float(AU.load("diff_md")[1]["target_temperature"])
    temp = g["applied_value"].astype(np.float64) * 16 + 16
    assert g["raw_action"].dtype == np.int32 and (g["rest_idx"] == 0).all()
    assert np.abs(temp[-1, 1] - (target - 3)).max() < 0.051 and (g["raw_action"][:, 1] == 0).all()      # the floor, rounded to 0.1 K
    assert g["applied_value"][-1, 2] == 1.0 and (g["raw_action"][:, 2] == 12).all()                    # the clip
    assert g["n_steps"] > A.WINDOW_LEN + 1 and (g["action_cost"] < 0).all()
    r = AU.load("diff_rot")[0]
    assert r["raw_action"].dtype == np.float32 and set(r["rest_idx"].tolist()) == {0, 1} and not r["action_cost"].any()
    assert AU.load("disc")[0]["raw_action"].dtype == np.float32 and not AU.load("disc")[0]["delta"].any()
    w = AU.load("diff_wide")[0]
    assert w["applied_value"].shape[1] == 92 and w["sensor_readings"].shape[1] == 111


def test_tables_are_the_reference_expressions():
    assert AU.same_bits(A.DISCRETE_VALUES, -3.0 + 0.5 * np.arange(13))      # what the device forms from a bin
    assert A.N_BINS == 13 and A.COST_TABLE[6] == 0.0 and AU.same_bits(A.COST_TABLE, A.COST_TABLE[::-1].copy())
    assert AU.same_bits(A.COST_TABLE, np.array([(abs(d) ** 1.2) * 0.3 for d in np.linspace(-3, 3, 13)]))


@pytest.mark.parametrize("name", AU.RUNS)
def test_host_classes_replay_the_reference(name):
    """from the recorded initial grid with the recorded raw actions: the applied value, the delta, the action cost, every
    step_stat entry, the running averages and the whole env record, bit for bit at every step"""
    g, task, settings, opts = AU.load(name)
    h = AU.host_of(name)
    h.reset(g["init_grid"])
    C = len(task["cooler_loc"])
    for k in range(int(g["n_steps"])):
        a = g["raw_action"][k]
        delta = h.map_action(a)[1] if opts["action_mode"] == "diff" else np.zeros(C)
        obs, r, term, trunc, info = h.step(a)
        at = "%s step %d: " % (name, k + 1)
        assert AU.same_bits(h.value, g["applied_value"][k]) and AU.same_bits(delta, g["delta"][k]), at + "mapping"
        assert AU.same_bits(np.float64(info.get("action_cost", 0.0)), g["action_cost"][k]), at + "action cost"
        for q in AU.STAT_STEP_KEYS:
            assert AU.same_bits(np.float64(info["step_stat"][q]), g["stat_" + q][k]), at + q
        for q in A.RUNNING_KEYS:
            assert AU.same_bits(np.array(getattr(h, q), np.float64), g["run_" + q][k]), at + q
        mine = dict(grid=h.state, t=np.float64(h.t), reward=np.float64(r), terminated=np.bool_(term), truncated=np.bool_(trunc),
                    cool_power=info["cool_power"], heat_power=info["heat_power"], rest_idx=np.int32(h.rest_idx),
                    warning_count=np.int32(h.warning_count), over_heat=np.int32(info["over_heat"]),
                    over_tolerace=np.int32(info["over_tolerace"]), energy_cost=np.float64(info["energy_cost"]),
                    target_cost=np.float64(info["target_cost"]), timestep=obs["timestep"][0],
                    sensor_readings=obs["sensor_readings"], heat_readings=obs["heat_readings"], action_temp=obs["action_temp"])
        assert set(mine) == set(AU.ENV_KEYS)
        for q in AU.ENV_KEYS:
            assert AU.same_bits(mine[q], g[q][k]), at + q
        assert np.array_equal(AU.counts_numpy(obs["sensor_readings"], task["target_temperature"]), AU.recorded_counts(g, k)), at


def test_box_input_of_the_difference_mode_is_the_bin_it_rounds_to():
    """float32 [0, 1] -> clip(round(v * 12), 0, 12), halves to even; the same step as the integer index"""
    g, task, _, _ = AU.load("diff_md")
    C = len(task["cooler_loc"])
    v = np.array([0.0, 1.0, 0.5, 1.0 / 24, 3.0 / 24, 0.49, 1.2, -0.3, 0.51], np.float32)[:C]
    want = np.array([0, 12, 6, 0, 2, 6, 12, 0, 6])[:C]
    ha, hb = AU.host_of("diff_md"), AU.host_of("diff_md")
    ha.reset(g["init_grid"])
    hb.reset(g["init_grid"])
    assert np.array_equal(ha.action_indices(v), want)
    assert all(AU.same_bits(x, y) for x, y in zip(ha.map_action(v), hb.map_action(want)))
    # under the Box space an integer array is a value array, as in the reference
    hc = AU.host_of("diff_md", discretize_rl_action_space=False)
    hc.reset(g["init_grid"])
    assert np.array_equal(hc.action_indices(np.ones(C, np.int64)), np.full(C, 12))


def test_reset_clears_the_history_and_restarts_from_the_default():
    g, task, _, _ = AU.load("diff_md")
    h = AU.host_of("diff_md")
    h.reset(g["init_grid"])
    first = h.step(g["raw_action"][0])[4]["action_cost"]
    for k in range(1, 4):
        h.step(g["raw_action"][k])
    assert h.bins.shape == (4, len(h.value)) and np.array_equal(h.bins, g["raw_action"][:4]) and not AU.same_bits(h.value, np.full_like(h.value, h.default_action_value))
    h.reset(g["init_grid"])
    assert h.bins is None and AU.same_bits(h.value, np.full(len(h.value), h.default_action_value, np.float32))
    assert h.step(g["raw_action"][0])[4]["action_cost"] == first == g["action_cost"][0]


def test_new_symbols_are_declared_and_bound_and_the_abi_version_stays():
    text = open(HEADER).read()
    assert re.search(r"#define XV_ABI_VERSION 12\b", text) and _lib.ABI_VERSION == 12
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, text), name
        assert name in _lib.SIGNATURES, name
    assert "typedef struct xv_anyhvac_act_io" in text
    fields = re.search(r"typedef struct xv_anyhvac_act_io \{(.*?)\} xv_anyhvac_act_io;", text, re.S).group(1)
    assert tuple(re.findall(r"(\w+);", fields)) == _lib.AnyHVACActIO.FIELDS
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NEW_SYMBOLS) and lib.xv_abi_version() == 12
    # the two structs that existed keep their layouts
    assert len(_lib.AnyHVACIO.FIELDS) == 15 and len(_lib.AnyHVACState.FIELDS) == 13


@pytest.mark.parametrize("setting", [dict(no_switch_action=False), dict(action_space_format="dict"),
                                     dict(random_start_t=True), dict(overheat_no_termiated_training_only=True),
                                     dict(return_normilized_obs=True), dict(control_type="Power")])
def test_excluded_settings_are_refused_as_before(setting):
    name = next(iter(setting))
    for cls in (HVACHost, A.DiffActionHost, A.DiscreteActionHost):
        with pytest.raises(ValueError, match=name):
            cls(**setting)
    with pytest.raises(ValueError, match=name):      # (raised before the device is touched, in front of action_mode)
        HVACVecEnv(1, action_mode="diff", **setting)
    with pytest.raises(TypeError):
        A.DiffActionHost(action_mode="diff")


def test_teachers_refuse_a_mapped_mode_before_the_device_is_touched():
    for mode in ("discrete", "diff"):
        env = object.__new__(HVACVecEnv)      # (no engine: the refusals come first)
        env.action_mode = mode
        with pytest.raises(ValueError, match="box"):
            env.set_pid("gt")
        with pytest.raises(ValueError, match="box"):
            env.rollout_teacher(4)
