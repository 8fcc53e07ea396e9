"""AnyHVAC on the device (csrc/anyhvac.hip) at the sizes of the sampler's default configuration: the `full` (15 x 15 cells,
283 coolers, 553 sensors, 366 heaters, 512 wall entries) and `max` (16 x 16 cells, 303 coolers, 469 sensors, 355 heaters, 578
wall entries) rooms, where every count is above the step kernel's 256 lanes — each lane carries a second cooler
(c = tid + 256), the wall loop takes a second and a third pass, hv_obs and hv_pid stride over the sensors and heaters, and
at 16 x 16 every lane is a cell.  Each test holds the device to the reference's recording or to the host restatement
(HVACHost, PIDHost, DiffActionHost) under the bounds of anyhvac_util.py, anyhvac_pid_util.py and anyhvac_act_util.py,
unchanged: they are functions of the counts (cost_tols, gamma) or do not depend on them.  tests/test_gpu_anyhvac.py's
test_replays_the_reference runs both rooms alone against their recordings.

What a skipped pass would break, from the kernel's code (each line was also seen to fail against a library built with that
one pass taken out):
  * the q = 1 cooler pass: coolers >= 256 would keep s_pc = s_pv = s_energy = 0, so cool_power[256:] is 0 where the
    recording and the host have powers (check_step's cool-power bound in every test below), action_temp[256:] misses the
    action (bit-equality with the host), and applied_value / delta / window of test 5 stay 0;
  * the second wall pass: s_chtc[256:] would miss a step's wall coefficients, the stencil of the cells in rows >= 7 reads
    them, and the grid leaves grid_tol (1e-11 K) by whole kelvins within a step (check_step's grid bound);
  * the second sensor pass: sensor_readings[256:] stay 0 (check_step's one-ulp bound), target_cost loses their loss
    (cost_tols), the stat counts of test 5 lose their share, and hv_pid's d_e[256:] = 0 moves every value column of test 4
    far out of the reordering interval.
Tests 1-5 fail under each of the three.  Test 6's rooms are the sampler's own — at most 156 coolers — so it fails under
the second and the third, not under the first.
"""
import numpy as np
import pytest
import torch

import anyhvac_act_util as AU
import anyhvac_pid_util as PU
import anyhvac_util as U
from xenoverse_amd.anyhvac import (DiffActionHost, HVACHost, HVACVecEnv, sample_tasks_device, task_dicts_from_device)
from xenoverse_amd.anyhvac.actions import STAT_KEYS, stat_margin
from xenoverse_amd.anyhvac.pid import PIDHost
from xenoverse_amd.engine import Engine

pytestmark = pytest.mark.gpu
BLOCK = 256      # HV_BLOCK: the step kernel's workgroup
STEPS = 4
BATCH = ("trunc", "full", "max", "wide", "full")
INDEX_SEED = 5       # the bins of test 5: the host alone keeps 2.6e-4 K from every stat threshold over the 4 steps
SAMPLER_SEED = 9     # the rooms of test 6: the host restatement of the sampler leaves out none of its 8
_solo = {}


def _env(n, settings, tasks, gen, mode="disabled", index=None, **kw):
    env = HVACVecEnv(n, autoreset_mode=mode, **dict(settings, **kw))
    env.set_task(tasks, env_task_index=index, generate_task=gen)
    return env


def _np(t):
    return torch.as_tensor(t).cpu().numpy()


def _host(cls, task, settings, grid, **task_kw):
    h = cls(**settings)
    h.set_task(task, generate_task=True, **task_kw)
    h.reset(grid)
    return h


def _counts(task):
    return len(task["cooler_loc"]), len(task["sensor_loc"]), len(task["heater_loc"])


# ---- 1: the padded batch -----------------------------------------------------------------------------------------------
def _solo_run(name):
    """STEPS steps of a fixture's room alone (num_envs = 1) under the common settings: [flat result per step], final grid.
    Where those are the fixture's own settings the run is held to the recording, so that what the batch is bit-equal to is
    itself the reference's run."""
    if name not in _solo:
        g, task, settings, _ = U.load(name)
        env = _env(1, dict(settings, max_steps=20160), [task], True)
        env.reset_injected(g["init_grid"][None])
        steps = []
        for k in range(STEPS):
            out = U.true_sizes(env, 0, *env.step(g["action"][k][None]))
            if settings["max_steps"] == 20160:
                U.check_step(g, k, *out, U.grid_of(env, 0), label=name + " alone")
            steps.append(U.flat_result(*out))
        _solo[name] = (steps, U.grid_of(env, 0))
        env.close()
    return _solo[name]


def _batch_env():
    loaded = [U.load(n) for n in BATCH]
    names = list(dict.fromkeys(BATCH))
    env = _env(len(BATCH), dict(loaded[0][2], max_steps=20160), [U.load(n)[1] for n in names], True,
               index=[names.index(n) for n in BATCH])
    env.reset_injected(U.pad_grids(env, [x[0]["init_grid"] for x in loaded]))
    return env, loaded


def test_padded_batch_and_rollout_are_bit_equal_to_the_solo_runs():
    """rooms of 35, 225, 256, 99 and 225 cells in ONE batch padded to 16 x 16 cells and 303 coolers: every output of every
    env and its final grid bit-equal to the room alone (which check_step holds to its recording), by 4 steps and by ONE
    rollout of the 4; padded columns zero.  The second `full` env sits four rows of the odd stride C = 303 into every
    per-cooler array."""
    env, loaded = _batch_env()
    assert env.dims[:5] == (16, 16, 303, 553, 366)
    assert list(env.counts["coolers"]) == [len(x[1]["cooler_loc"]) for x in loaded]
    acts = np.stack([U.pad_actions(env, [x[0]["action"][k] for x in loaded]) for k in range(STEPS)])

    def check(results):
        for k, out in enumerate(results):
            for i, name in enumerate(BATCH):
                mine, solo = U.flat_result(*out(i)), _solo_run(name)[0][k]
                assert all(U.same_bits(a, b) for a, b in zip(mine, solo)), "%s (env %d) step %d" % (name, i, k + 1)
        for i, name in enumerate(BATCH):
            assert U.same_bits(U.grid_of(env, i), _solo_run(name)[1]), name
        assert env.check_errors() == 0

    outs = []
    for k in range(STEPS):
        out = env.step(acts[k])
        outs.append(lambda i, out=out: U.true_sizes(env, i, *out))
        for i, key in ((i, key) for i in range(env.num_envs) for key in ("coolers", "sensors", "heaters")):
            n = int(env.counts[key][i])
            padded = {"coolers": (out[0]["action_temp"], out[4]["cool_power"]), "sensors": (out[0]["sensor_readings"],),
                      "heaters": (out[0]["heat_readings"], out[4]["heat_power"])}[key]
            assert not any(bool(p[i, n:].any()) for p in padded), "padded %s columns of env %d" % (key, i)
    check(outs)
    env.close()
    env, _ = _batch_env()
    out = env.rollout(acts)
    check([lambda i, k=k: U.true_sizes(env, i, *out, lead=(k,)) for k in range(STEPS)])
    env.close()


# ---- 2: the resting cooler in the second half --------------------------------------------------------------------------
def test_rest_cooler_beyond_the_block_wraps_around_and_rests():
    """`full` (283 coolers) after one step, three envs: the LAST cooler resting for 3601 s (cooler 0 takes over), for exactly
    3600 s (it goes on resting), and cooler 256 — the first of the lanes' second coolers — 100 s into its hour; the next
    step against HVACHost under check_step's bounds"""
    g, task, settings, _ = U.load("full")
    C = len(task["cooler_loc"])
    assert C - 1 > BLOCK
    rests, starts, after = (C - 1, C - 1, BLOCK), (30.0 - 3601.0, 30.0 - 3600.0, 30.0 - 100.0), (0, C - 1, BLOCK)
    env = _env(3, settings, [task], True)
    env.reset_injected(np.stack([g["init_grid"]] * 3))
    recs = [U.HostRecord(_host(HVACHost, task, settings, g["init_grid"])) for _ in rests]
    a0, a1 = g["action"][0], g["action"][1]
    env.step(np.stack([a0] * 3))
    rs = np.zeros((3, C))
    for i, (rec, rest, start) in enumerate(zip(recs, rests, starts)):
        rec.step(a0)
        h = rec.host
        assert h.t == 30
        h.switch[:] = 1
        h.switch[rest] = 0
        h.rest_idx = rest
        h.rest_start[rest] = rs[i, rest] = start
    env.set_state(rest_idx=np.array(rests, np.int32), rest_start=rs)
    out = env.step(np.stack([a1] * 3))
    for i, (rec, rest) in enumerate(zip(recs, after)):
        rec.step(a1)
        o, r, te, tr, inf = U.true_sizes(env, i, *out)
        assert rec.host.rest_idx == rest and int(inf["rest_idx"]) == rest
        assert o["action_temp"][rest] == -1.0 and inf["cool_power"][rest] == 0.0
        assert (o["action_temp"][np.arange(C) != rest] >= 16.0).all()
        U.check_step(rec.g, 1, o, r, te, tr, inf, U.grid_of(env, i), label="env %d" % i)
    st = env.get_state()
    assert float(st["rest_start"][0, 0]) == 30.0 and float(st["rest_start"][1, C - 1]) == starts[1]
    assert float(st["rest_start"][2, BLOCK]) == starts[2]
    assert env.check_errors() == 0
    env.close()


# ---- 3: same-step autoreset ----------------------------------------------------------------------------------------------
def test_same_step_autoreset_at_full_size():
    """`max` (256 cells, 303 coolers, 469 sensors) with max_steps = 2 and the reset grid injected: step 2 truncates, hands
    out the recording's step 2 as final_obs and the host's reset observation as obs, and leaves a new episode's state in
    every column; step 3 is the host's first step"""
    g, task, settings, gen = U.load("max")
    settings = dict(settings, max_steps=2)
    C, S, H = _counts(task)
    env = _env(1, settings, [task], gen, mode="same_step")
    env.reset_injected(g["init_grid"][None])
    fresh = g["init_grid"][None] + 0.5
    for k in range(2):
        obs, r, term, trunc, info = env.step_injected(g["action"][k][None], fresh)
        assert bool(trunc[0]) == (k == 1) and bool(info["_final_obs"][0]) == (k == 1) and not bool(term[0])
        if k == 0:
            assert not any(bool(info["final_obs"][q].any()) for q in ("sensor_readings", "heat_readings", "action_temp"))
            U.check_step(g, 0, *U.true_sizes(env, 0, obs, r, term, trunc, info), U.grid_of(env, 0), label="max")
    fin = info["final_obs"]
    assert fin["sensor_readings"].shape == (1, S) and S > BLOCK
    assert U.ulps32(_np(fin["sensor_readings"][0]), g["sensor_readings"][1]).max() <= 1.0
    assert U.ulps32(_np(fin["heat_readings"][0]), g["heat_readings"][1]).max() <= 1.0
    assert U.same_bits(_np(fin["action_temp"][0]), g["action_temp"][1])
    assert int(fin["timestep"][0]) == int(g["timestep"][1]) and float(info["time"][0]) == float(g["t"][1])
    assert U.ulps32(_np(info["cool_power"][0]), g["cool_power"][1]).max() <= 2.0
    host = HVACHost(**settings)
    host.set_task(task, generate_task=gen)
    hobs, _ = host.reset(fresh[0])
    assert np.array_equal(U.grid_of(env, 0), fresh[0])
    assert U.ulps32(_np(obs["sensor_readings"][0]), hobs["sensor_readings"]).max() <= 1.0
    assert U.ulps32(_np(obs["heat_readings"][0]), hobs["heat_readings"]).max() <= 1.0
    assert U.same_bits(_np(obs["action_temp"][0]), hobs["action_temp"]) and int(obs["timestep"][0]) == 0
    st = env.get_state()
    assert float(st["t"][0]) == 0.0 and int(st["episode_step"][0]) == 0 and int(st["tail"][0]) == 0
    assert torch.isnan(st["last_call"][0]) and not st["filter"].any() and not st["head"].any() and not st["rest_start"].any()
    assert int(st["rest_idx"][0]) == 0 and U.same_bits(_np(st["value"][0]), host.value) and st["value"].shape == (1, C)
    rec = U.HostRecord(host)
    rec.step(g["action"][0])
    out = env.step_injected(g["action"][0][None], fresh)
    o, r, te, tr, inf = U.true_sizes(env, 0, *out)
    assert inf["episode_step"] == 1
    U.check_step(rec.g, 0, o, r, te, tr, inf, U.grid_of(env, 0), label="after the reset")
    assert not any(bool(out[4]["final_obs"][q].any()) for q in ("sensor_readings", "heat_readings", "action_temp"))
    assert env.check_errors() == 0
    env.close()


# ---- 4: the PID teacher ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("gt", "loc"))
def test_pid_teacher_at_full_size(kind):
    """`full` (553 sensors, 283 coolers), the solvers' default gains: pid_action on the recorded readings of steps 1-4
    against PIDHost under anyhvac_pid_util's contract (the host alone keeps every x 3.9e-4 from the switch threshold); then
    rollout_teacher(3) against three rounds of pid_action() + step(), bit for bit"""
    g, task, settings, gen = U.load("full")
    C, S, _ = _counts(task)
    sec = settings["iter_per_step"] * settings["sec_per_iter"]
    host = PIDHost(task, kind, sec_per_step=sec)
    assert host.corr_sensor_cooler.shape == (S, C) and S > 2 * BLOCK and C > BLOCK
    a = _env(1, settings, [task], gen)
    a.set_pid(kind)
    adjacent = 0
    for k in range(STEPS):
        readings = g["sensor_readings"][k]
        act, flat = a.pid_action(readings[None], return_flat=True)
        fl, st = _np(flat[0]), a.get_pid_state()
        d_e = host.advance(readings)
        x = np.matmul(d_e, host.corr_sensor_cooler)
        at = "%s step %d" % (kind, k + 1)
        assert np.abs(x + 0.05).min() >= PU.MIN_SWITCH_MARGIN, at + ": the host's own margin"
        assert PU.same_bits(fl[0], (x > -0.05).astype(np.float32)), at + ": switch columns"
        adjacent += PU.check_value(fl[1], d_e, host.corr_sensor_cooler, at)
        assert PU.same_bits(_np(act[0]), 1 - fl[1]), at + ": the env's action is 1 - value in float32"
        assert PU.same_bits(_np(st["acc_diff"][0]), host.acc_diff), at + ": acc_diff"
        assert PU.same_bits(_np(st["last_obs"][0]), readings), at + ": last observation"
    assert adjacent <= PU.ADJACENT_CAP * STEPS * C, "%d of %d value columns adjacent" % (adjacent, STEPS * C)
    a.reset_injected(g["init_grid"][None])      # (a reset: the controller is a fresh one)
    assert int(a.get_pid_state()["fresh"][0]) == 1 and not a.get_pid_state()["acc_diff"].any()
    rounds = []
    for _ in range(3):
        act = a.pid_action()
        rounds.append((act, a.step(act)))
    b = _env(1, settings, [task], gen)
    b.reset_injected(g["init_grid"][None])
    b.set_pid(kind)
    out = b.rollout_teacher(3)
    for k, (act, step) in enumerate(rounds):
        assert PU.same_bits(_np(out[4]["action"][k]), _np(act)), "action of step %d" % (k + 1)
        mine = U.flat_result(*U.true_sizes(b, 0, *out, lead=(k,)))
        assert all(U.same_bits(p, q) for p, q in zip(mine, U.flat_result(*U.true_sizes(a, 0, *step)))), k
    sa, sb = a.get_state(), b.get_state()
    assert all(PU.same_bits(_np(sa[k]), _np(sb[k])) for k in sa)
    pa, pb = a.get_pid_state(), b.get_pid_state()
    assert all(PU.same_bits(_np(pa[k]), _np(pb[k])) for k in pa)
    # the closed loop's first action is the host's on the device's own first observation
    host.reset()
    first = _np(a.reset_injected(g["init_grid"][None])["sensor_readings"][0])
    PU.check_action(_np(rounds[0][0][0]), host.advance(first), host.corr_sensor_cooler, "the first closed-loop action")
    assert a.check_errors() == 0 and b.check_errors() == 0
    a.close()
    b.close()


# ---- 5: the difference-action mode -------------------------------------------------------------------------------------
def test_difference_actions_at_full_size():
    """`full`, two envs, MultiDiscrete bins with the action cost and the too-cold limit on, the generator of
    scripts/gen_golden_anyhvac_actions.py's random_indices restated (seed 5) — against DiffActionHost: applied_value, delta and
    action_temp bit-equal, the window words of all 283 coolers, the cost within gamma_C |cost|, the eight counts equal, the
    physics within check_step's bounds"""
    g, task, settings, _ = U.load("full")
    C, S, _ = _counts(task)
    opts = dict(action_mode="diff", discretize_rl_action_space=True, add_action_cost=True, too_cold_limit=True)
    raw = np.random.RandomState(INDEX_SEED).randint(0, 13, (STEPS, C))
    env = _env(2, settings, [task], True, **opts)
    env.reset_injected(np.stack([g["init_grid"]] * 2))
    host = _host(DiffActionHost, task, settings, g["init_grid"], discretize_rl_action_space=True, add_action_cost=True,
                 too_cold_limit=True)
    rec = U.HostRecord(host)
    margin = np.inf
    for k in range(STEPS):
        out = env.step(np.stack([raw[k]] * 2).astype(np.int32))
        hdelta = host.map_action(raw[k])[1]
        hobs, hr, _, _, hinfo = rec.step(raw[k])
        margin = min(margin, stat_margin(hobs["sensor_readings"], host.target_temperature))
        window = _np(env.get_act_state()["window"])
        for i in range(2):
            at = "env %d step %d: " % (i, k + 1)
            o, r, te, tr, inf = U.true_sizes(env, i, *out)
            assert U.same_bits(_np(out[4]["applied_value"][i]), host.value), at + "applied value"
            assert U.same_bits(_np(out[4]["delta"][i]), hdelta), at + "delta"
            assert U.same_bits(o["action_temp"], hobs["action_temp"]), at + "action_temp"
            assert ((window[i] & 15) == raw[k] + 1).all() and (window[i] >> (4 * (k + 1)) == 0).all(), at + "the window"
            assert AU.cost_close(out[4]["action_cost"][i], hinfo["action_cost"], C), at + "action cost %r %r" % (
                float(out[4]["action_cost"][i]), hinfo["action_cost"])
            mine = np.array([int(out[4]["step_stat"][q][i]) for q in STAT_KEYS], np.int64)
            assert np.array_equal(mine, [int(hinfo["step_stat"][q]) for q in STAT_KEYS]), at + "counts"
            assert np.array_equal(mine, AU.counts_numpy(o["sensor_readings"], host.target_temperature)), at + "own readings"
            U.check_step(rec.g, k, o, r, te, tr, inf, U.grid_of(env, i), label=at)
    assert margin >= AU.MIN_STAT_MARGIN and host.eer_margin >= U.MIN_EER_MARGIN
    assert env.check_errors() == 0
    env.close()


# ---- 6: rooms of the device sampler --------------------------------------------------------------------------------------
def test_device_sampled_default_rooms_follow_the_host():
    """8 rooms of the default configuration from the device sampler (6 x 11 to 15 x 15 cells, seven of them not square, up
    to 156 coolers, 292 sensors and 518 heaters in tables padded to 15 x 15 x 303 x 607 x 607), set through
    set_task of the device tables; two steps of 20 iterations from an injected grid against HVACHost on the flat dicts made
    from those tables.  An env whose host run comes within 1e-7 K of an EER jump or 1e-4 K of the failure bound is left
    out: at most one of the 8 (the host restatement of the sampler leaves out none at this seed)."""
    settings = dict(max_steps=20160, iter_per_step=20, sec_per_iter=0.15, reward_mode=0)
    engine = Engine("cuda:0")
    t = sample_tasks_device(8, seed=SAMPLER_SEED, generate_task=True, engine=engine)
    assert t["dims"] == (15, 15, 303, 607, 607, 4, 7)
    env = HVACVecEnv(8, autoreset_mode="disabled", **settings)
    env.set_task(t, generate_task=True)
    tasks = task_dicts_from_device(t)
    rng = np.random.RandomState(100 + SAMPLER_SEED)
    recs, grids, acts = [], [], []
    for task in tasks:
        nw, nl, C = int(task["n_width"]), int(task["n_length"]), len(task["cooler_loc"])
        grids.append(float(task["ambient_temp"]) + 2.0 * rng.standard_normal((nw, nl)))
        acts.append(rng.uniform(0, 1, (2, C)).astype(np.float32))
        recs.append(U.HostRecord(_host(HVACHost, task, settings, grids[-1])))
    assert len({g.shape for g in grids}) == 8 and sum(g.shape[0] != g.shape[1] for g in grids) == 7
    nS, nH = max(env.counts["sensors"]), max(env.counts["heaters"])
    assert nS > BLOCK and nH > 2 * BLOCK and env.counts["n_width"][int(np.argmax(env.counts["sensors"]))] < 15
    env.reset_injected(U.pad_grids(env, grids))
    outs, fail = [], np.full(8, np.inf)
    for k in range(2):
        outs.append((env.step(U.pad_actions(env, [a[k] for a in acts])), [U.grid_of(env, i) for i in range(8)]))
        for i, rec in enumerate(recs):
            hobs = rec.step(acts[i][k])[0]
            fail[i] = min(fail[i], np.abs(hobs["sensor_readings"].astype(np.float64) - rec.host.failure_upperbound).min())
    kept = [i for i, rec in enumerate(recs) if rec.host.eer_margin >= U.MIN_EER_MARGIN and fail[i] >= U.MIN_FAIL_MARGIN]
    assert len(kept) >= 7, "left out: %s" % sorted(set(range(8)) - set(kept))
    for k, (out, grid) in enumerate(outs):
        for i in kept:
            U.check_step(recs[i].g, k, *U.true_sizes(env, i, *out), grid[i], label="room %d" % i)
    assert env.check_errors() == 0
    env.close()
    engine.close()
