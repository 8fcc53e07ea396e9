"""AnyHVAC on the device (csrc/anyhvac.hip) against the reference's recorded runs and the host restatement; the bounds are
derived in anyhvac_util.py.  The shapes are the fixtures': rooms of 30-99 cells, 3-92 coolers, and in
test_replays_the_reference the two full-size rooms of 225 and 256 cells (tests/test_gpu_anyhvac_fullsize.py has the rest at
that size)."""
import numpy as np
import pytest
import torch

import anyhvac_util as U
from xenoverse_amd.anyhvac import HVACEnv, HVACHost, HVACVecEnv

pytestmark = pytest.mark.gpu
SAME_SETTINGS = ("rot", "hot", "trunc", "wide")      # the run fixtures of iter_per_step = 200
BATCH_STEPS = 6
_solo = {}


def _env(n, settings, tasks, gen, mode="disabled", index=None, **kw):
    env = HVACVecEnv(n, autoreset_mode=mode, **dict(settings, **kw))
    env.set_task(tasks, env_task_index=index, generate_task=gen)
    return env


@pytest.mark.parametrize("name", U.RUNS)
def test_replays_the_reference(name):
    """num_envs = 1 from the recorded initial grid: every discrete output equal, every continuous one within its bound, at
    every step of every fixture"""
    g, task, settings, gen = U.load(name)
    assert float(g["eer_margin"]) >= U.MIN_EER_MARGIN and float(g["fail_margin"]) >= U.MIN_FAIL_MARGIN
    env = _env(1, settings, [task], gen)
    obs = env.reset_injected(g["init_grid"][None])
    assert np.array_equal(U.grid_of(env, 0), g["init_grid"]) and int(obs["timestep"][0]) == 0
    for k in range(int(g["n_steps"])):
        out = env.step(g["action"][k][None])
        U.check_step(g, k, *U.true_sizes(env, 0, *out), U.grid_of(env, 0), label=name)
    assert env.check_errors() == 0
    env.close()


def _solo_run(name):
    """BATCH_STEPS steps of a fixture's room alone under the common settings: [flat result per step], final grid"""
    if name not in _solo:
        g, task, settings, _ = U.load(name)
        env = _env(1, dict(settings, max_steps=20160), [task], True)
        env.reset_injected(g["init_grid"][None])
        steps = []
        for k in range(BATCH_STEPS):
            steps.append(U.flat_result(*U.true_sizes(env, 0, *env.step(g["action"][k][None]))))
        _solo[name] = (steps, U.grid_of(env, 0))
        env.close()
    return _solo[name]


def _batch_env():
    loaded = [U.load(n) for n in SAME_SETTINGS]
    env = _env(len(loaded), dict(loaded[0][2], max_steps=20160), [x[1] for x in loaded], True)
    env.reset_injected(U.pad_grids(env, [x[0]["init_grid"] for x in loaded]))
    return env, loaded


def test_mixed_batch_is_bit_equal_to_the_solo_runs():
    """four rooms of 30, 30, 35 and 99 cells with 6 to 92 coolers in ONE batch, padded to the largest"""
    env, loaded = _batch_env()
    assert env.dims[:5] == (9, 11, 92, 111, 202)
    assert list(env.counts["coolers"]) == [len(x[1]["cooler_loc"]) for x in loaded]
    for k in range(BATCH_STEPS):
        out = env.step(U.pad_actions(env, [x[0]["action"][k] for x in loaded]))
        for i, name in enumerate(SAME_SETTINGS):
            mine, solo = U.flat_result(*U.true_sizes(env, i, *out)), _solo_run(name)[0][k]
            assert all(U.same_bits(a, b) for a, b in zip(mine, solo)), "%s step %d" % (name, k + 1)
        nC = env.counts["coolers"]
        for i in range(env.num_envs):      # padded columns stay zero
            assert not out[0]["action_temp"][i, int(nC[i]):].any() and not out[4]["cool_power"][i, int(nC[i]):].any()
    for i, name in enumerate(SAME_SETTINGS):
        assert U.same_bits(U.grid_of(env, i), _solo_run(name)[1]), name
    assert env.check_errors() == 0
    env.close()


def test_rollout_is_bit_equal_to_single_steps():
    """trunc and wide (with the two others) in one launch of BATCH_STEPS steps against BATCH_STEPS launches"""
    env, loaded = _batch_env()
    acts = np.stack([U.pad_actions(env, [x[0]["action"][k] for x in loaded]) for k in range(BATCH_STEPS)])
    out = env.rollout(acts)
    for k in range(BATCH_STEPS):
        for i, name in enumerate(SAME_SETTINGS):
            mine = U.flat_result(*U.true_sizes(env, i, *out, lead=(k,)))
            assert all(U.same_bits(a, b) for a, b in zip(mine, _solo_run(name)[0][k])), "%s step %d" % (name, k + 1)
    for i, name in enumerate(SAME_SETTINGS):
        assert U.same_bits(U.grid_of(env, i), _solo_run(name)[1]), name
    env.close()


def test_rest_cooler_wraps_around_and_the_hour_is_strict():
    """two envs of the rot room with the LAST cooler resting: one whose rest expires at the next step (3601 s: cooler 0
    takes over) and one at exactly 3600 s (it goes on resting), against HVACHost"""
    g, task, settings, _ = U.load("rot")
    C = len(task["cooler_loc"])
    env = _env(2, settings, [task], True)
    env.reset_injected(np.stack([g["init_grid"]] * 2))
    hosts = []
    for _ in range(2):
        h = HVACHost(**settings)
        h.set_task(task, generate_task=True)
        h.reset(g["init_grid"])
        hosts.append(h)
    a0, a1 = g["action"][0], g["action"][1]
    env.step(np.stack([a0, a0]))
    for h in hosts:
        h.step(a0)
    assert hosts[0].t == 30
    starts = [30.0 - 3601.0, 30.0 - 3600.0]
    rs = np.zeros((2, C))
    rs[:, C - 1] = starts
    env.set_state(rest_idx=np.array([C - 1, C - 1], np.int32), rest_start=rs)
    for h, s in zip(hosts, starts):
        h.switch[:] = 1
        h.switch[C - 1] = 0
        h.rest_idx = C - 1
        h.rest_start[C - 1] = s
    out = env.step(np.stack([a1, a1]))
    for i, (h, rest) in enumerate(zip(hosts, (0, C - 1))):
        hobs, hr, _, _, hinfo = h.step(a1)
        o, r, _, _, inf = U.true_sizes(env, i, *out)
        assert h.rest_idx == rest and int(inf["rest_idx"]) == rest
        assert U.same_bits(o["action_temp"], hobs["action_temp"]) and o["action_temp"][rest] == -1.0
        assert np.abs(U.grid_of(env, i) - h.state).max() <= U.grid_tol(g, 1)
        assert U.ulps32(o["sensor_readings"], hobs["sensor_readings"]).max() <= 1.0
        assert U.ulps32(inf["cool_power"], hinfo["cool_power"]).max() <= 2.0 and inf["cool_power"][rest] == 0.0
    assert float(env.get_state()["rest_start"][0, 0]) == 30.0
    env.close()


def test_same_step_autoreset_starts_the_episode_the_host_starts():
    """trunc (max_steps = 8) with the reset grid injected: the truncating step hands out the finished episode's last
    observation as final_obs and the new episode's first as obs; the step after it is the host's first step"""
    g, task, settings, gen = U.load("trunc")
    env = _env(1, settings, [task], gen, mode="same_step")
    env.reset_injected(g["init_grid"][None])
    fresh = g["init_grid"][None] + 0.5
    for k in range(8):
        obs, r, term, trunc, info = env.step_injected(g["action"][k][None], fresh)
        assert bool(trunc[0]) == (k == 7) and bool(info["_final_obs"][0]) == (k == 7)
        if k < 7:
            assert not info["final_obs"]["sensor_readings"].any()
    assert U.ulps32(info["final_obs"]["sensor_readings"][0].cpu().numpy(), g["sensor_readings"][7]).max() <= 1.0
    assert int(info["final_obs"]["timestep"][0]) == int(g["timestep"][7]) and float(info["time"][0]) == float(g["t"][7])
    host = HVACHost(**settings)
    host.set_task(task, generate_task=gen)
    hobs, _ = host.reset(fresh[0])
    assert np.array_equal(U.grid_of(env, 0), fresh[0])
    assert U.ulps32(obs["sensor_readings"][0].cpu().numpy(), hobs["sensor_readings"]).max() <= 1.0
    assert U.same_bits(obs["action_temp"][0].cpu().numpy(), hobs["action_temp"]) and int(obs["timestep"][0]) == 0
    st = env.get_state()
    assert float(st["t"][0]) == 0.0 and int(st["episode_step"][0]) == 0 and int(st["tail"][0]) == 0
    assert torch.isnan(st["last_call"][0]) and not st["filter"].any()
    out = env.step_injected(g["action"][0][None], fresh)
    hobs, hr, _, _, hinfo = host.step(g["action"][0])
    o, r, _, _, inf = U.true_sizes(env, 0, *out)
    assert np.abs(U.grid_of(env, 0) - host.state).max() <= U.grid_tol(g, 0)
    assert U.ulps32(o["sensor_readings"], hobs["sensor_readings"]).max() <= 1.0 and inf["episode_step"] == 1
    assert U.ulps32(inf["cool_power"], hinfo["cool_power"]).max() <= 2.0
    env.close()


def test_philox_reset_is_reproducible_and_has_the_reference_spread():
    """reset(): ambient + 2 N(0, 1) per cell from the engine's Philox stream (not numpy's: runs inject the grid)"""
    g, task, settings, _ = U.load("trunc")
    grids = []
    for _ in range(2):
        env = _env(64, settings, [task], True, seed=11)
        obs, _ = env.reset()
        grids.append(torch.stack([env.get_state()["grid"][i] for i in range(64)]).cpu().numpy())
        assert obs["sensor_readings"].shape == (64, len(task["sensor_loc"]))
        env.close()
    assert np.array_equal(grids[0], grids[1])
    z = (grids[0] - float(task["ambient_temp"])) / 2.0      # 64 x 35 draws: mean within 5 / sqrt(n), variance within 5 sqrt(2 / n)
    n = z.size
    assert len(np.unique(z)) > 0.99 * n
    assert abs(z.mean()) < 5 / np.sqrt(n) and abs(z.var() - 1) < 5 * np.sqrt(2 / n)


def test_nan_sets_the_error_flag_and_leaves_the_env_as_it_was():
    g, task, settings, _ = U.load("trunc")
    nan = np.full_like(task["cooler_cooler_eer_base"], np.nan)
    bad = dict(task, cooler_cooler_eer_base=nan, cooler_cooler_eer_reverse=nan)
    env = _env(2, dict(settings, max_steps=20160), [task, bad], True)
    env.reset_injected(np.stack([g["init_grid"]] * 2))
    out = env.step(np.stack([g["action"][0]] * 2))
    assert env.check_errors() & 4      # XV_DEVERR_NONFINITE
    assert np.array_equal(U.grid_of(env, 1), g["init_grid"])
    st = env.get_state()
    assert float(st["t"][1]) == 0.0 and int(st["episode_step"][1]) == 0 and float(st["t"][0]) == 30.0
    assert torch.isnan(out[1][1]) and not bool(out[2][1]) and not bool(out[3][1])
    good = U.flat_result(*U.true_sizes(env, 0, *out))
    assert all(U.same_bits(a, b) for a, b in zip(good, _solo_run("trunc")[0][0]))
    assert env.check_errors() == 0      # reading cleared it
    env.close()


def test_one_env_wrapper_returns_true_sizes_and_the_reference_surface():
    g, task, settings, gen = U.load("mode2")
    env = HVACEnv(**settings)
    env.set_task(task, generate_task=gen)
    obs, info = env.reset(state=g["init_grid"])
    C, S, H = len(task["cooler_loc"]), len(task["sensor_loc"]), len(task["heater_loc"])
    assert obs["sensor_readings"].shape == (S,) and obs["heat_readings"].shape == (H,) and obs["action_temp"].shape == (C,)
    assert obs["action_temp"][0] == -1.0 and obs["timestep"].dtype == np.int32 and obs["timestep"].shape == (1,)
    for k in range(2):
        o, r, term, trunc, info = env.step(g["action"][k])
        assert isinstance(r, float) and abs(r - float(g["reward"][k])) <= U.cost_tols(g, k, S, C)[2]
        assert U.ulps32(o["sensor_readings"], g["sensor_readings"][k]).max() <= 1.0 and info["time"] == g["t"][k]
        assert info["cool_power"].shape == (C,) and info["heat_power"].shape == (H,)
    target = float(task["target_temperature"])
    assert not env.sample_action("max").any() and env.sample_action("max").shape == (C,)
    assert np.array_equal(env.sample_action("constant"), np.full(C, (target - 16) / 16, np.float32))
    assert np.array_equal(env.sample_action("constant_conservative"), np.full(C, (target - 5 - 16) / 16, np.float32))
    with pytest.raises(ValueError):
        env.sample_action("random")
    env.close()
