"""AnyHVAC's episode protocol on the device (csrc/anyhvac.hip: hv_reset's start logic, the history ring, last_fail, the
no-terminate flag) against the reference's recorded runs (tests/golden/start_anyhvac_*.npz) and against itself.  A reset's
start t, rest index, history count and last_fail are exact; every step is held to the derived bounds of anyhvac_util.py
(and anyhvac_act_util.py for `rl`).  Rooms of 30-35 cells, at most 276 steps of 50 iterations.

A handle has ONE max_steps, reward mode and action mode, so the fixtures run as three batches: the five that share the
default settings in one handle of ten envs (each twice, rooms of three sizes padded together), `trunc` (max_steps = 40) and
`rl` (difference actions, reward mode 1) each twice in a handle of their own beside a room of another size."""
import numpy as np
import pytest
import torch

import anyhvac_act_util as AU
import anyhvac_start_util as SU
import anyhvac_util as U
from xenoverse_amd.anyhvac import HVACVecEnv
from xenoverse_amd.anyhvac import host as H
from xenoverse_amd.anyhvac.actions import STAT_KEYS

pytestmark = pytest.mark.gpu
GROUPS = {
    "main": ("inv", "choice", "back", "early", "record", "back", "record", "inv", "early", "choice"),
    "trunc": ("trunc", None, "trunc"),      # None: a room of another size that only fills the batch (the `inv` task)
    "rl": (None, "rl", "rl"),
}
START_KEYS = ("t", "rest_idx", "rest_start", "last_fail", "history_count")


def _flags(flags):
    return (H.START_RANDOM if flags[0] else 0) | (H.START_RECORD if flags[1] else 0) | (H.START_NO_TERMINATE if flags[2] else 0)


def _batch(layout, mode="disabled", seed=0, **kw):
    """an env per entry of layout (fixture names; None: a filler room without flags) -> (env, fixtures per env)"""
    names = [n or "inv" for n in layout]
    uniq = sorted(set(names))
    fx = [SU.load(n) for n in names]
    first = next(f for n, f in zip(layout, fx) if n)
    opts = dict(action_mode="diff", **SU.RL_OPTS) if bool(first[0]["rl"]) else {}
    env = HVACVecEnv(len(layout), autoreset_mode=mode, seed=seed, **dict(first[2], **opts), **kw)
    env.set_task([SU.load(n)[1] for n in uniq], env_task_index=[uniq.index(n) for n in names],
                 generate_task=bool(first[0]["generate_task"]))
    bits = np.array([_flags(f[3]) if n else 0 for n, f in zip(layout, fx)])
    env.set_random_start_t((bits & H.START_RANDOM) != 0)
    env.set_generate_record((bits & H.START_RECORD) != 0)
    env.set_overheat_no_termiated_training_only((bits & H.START_NO_TERMINATE) != 0)
    return env, [f[0] for f in fx]


def _flat(out):
    obs, r, te, tr, info = out
    d = {"obs." + k: v for k, v in obs.items() if k != "counts"}
    d.update(reward=r, terminated=te, truncated=tr)
    for k, v in info.items():
        if isinstance(v, dict):
            d.update({k + "." + q: w for q, w in v.items() if q != "counts"})
        else:
            d[k] = v
    return {k: v.cpu().numpy() for k, v in d.items()}


def _same(a, b, label=""):
    assert set(a) == set(b)
    for k in a:
        assert U.same_bits(a[k], b[k]), label + k


def _sizes(env, i, d, lead=()):
    """env i of a _flat() result -> check_step's arguments in the room's true sizes"""
    nC, nS, nH = (int(env.counts[q][i]) for q in ("coolers", "sensors", "heaters"))
    at = tuple(lead) + (i,)
    o = dict(sensor_readings=d["obs.sensor_readings"][at][:nS], heat_readings=d["obs.heat_readings"][at][:nH],
             action_temp=d["obs.action_temp"][at][:nC], timestep=int(d["obs.timestep"][at]))
    inf = {k: float(d[k][at]) for k in ("over_heat", "over_tolerace", "energy_cost", "target_cost", "time", "rest_idx",
                                        "warning_count", "episode_step")}
    inf["cool_power"], inf["heat_power"] = d["cool_power"][at][:nC], d["heat_power"][at][:nH]
    return o, float(d["reward"][at]), bool(d["terminated"][at]), bool(d["truncated"][at]), inf


def _state(env, keys):
    return {k: v.cpu().numpy() for k, v in env.get_state(only=keys).items()}


def _grids(env):
    NW, NL = env.dims[:2]
    g = env.get_state(only=("grid",))["grid"].cpu().numpy().reshape(env.num_envs, NW, NL)
    return [g[i, :int(env.counts["n_width"][i]), :int(env.counts["n_length"][i])] for i in range(env.num_envs)]


def _check_reset(env, i, g, j, obs, label):
    """reset j of fixture g at env i: exact start t, rest index, timestep, last_fail, history count, rest_start row"""
    st = _state(env, START_KEYS)
    nC, nS = int(env.counts["coolers"][i]), int(env.counts["sensors"][i])
    at = "%s env %d reset %d: " % (label, i, j)
    rest = int(g["reset_rest_idx"][j])
    assert float(st["t"][i]) == float(g["reset_t"][j]), at + "start t %r, recorded %r" % (st["t"][i], g["reset_t"][j])
    assert int(st["rest_idx"][i]) == rest, at + "rest index"
    assert int(obs["timestep"][i]) == int(g["reset_timestep"][j]), at + "timestep"
    assert float(st["last_fail"][i]) == float(g["reset_last_fail"][j]), at + "last_fail"
    assert min(int(st["history_count"][i]), H.HISTORY_LENGTH) == int(g["reset_hist_len"][j]), at + "history count"
    assert float(st["rest_start"][i, rest]) == float(g["reset_t"][j]), at + "rest_start[rest]"
    assert U.same_bits(st["rest_start"][i, :nC], g["reset_rest_start"][j]), at + "rest_start"
    assert U.same_bits(obs["action_temp"][i, :nC].cpu().numpy(), g["reset_action_temp"][j]), at + "action_temp"
    u = float(U.ulps32(obs["sensor_readings"][i, :nS].cpu().numpy(), g["reset_sensor_readings"][j]).max())
    assert u <= 1.0, at + "sensor readings off by %g float32 ulp" % u


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_fixtures_in_one_batch_with_injected_grids_and_draws(group):
    """every env walks its fixture's resets (reset_injected under a mask, the recorded grid and draws) and steps (its
    recorded actions) while the others of the batch walk theirs; envs whose fixture has ended go on stepping unchecked"""
    layout = GROUPS[group]
    env, fx = _batch(layout)
    N, Cc = env.num_envs, env.dims[2]
    rl = env.action_mode == "diff"
    todo = [SU.events(g) if n else [] for n, g in zip(layout, fx)]
    last_grid = [np.zeros((int(env.counts["n_width"][i]), int(env.counts["n_length"][i]))) for i in range(N)]
    n_reset = n_step = 0
    while any(todo):
        mask = np.array([bool(ev) and ev[0][0] == "reset" for ev in todo])
        if env.need_reset:      # (the first reset takes every env: the fillers and all fixtures start with one)
            assert all(not ev or ev[0] == ("reset", 0) for ev in todo)
            mask[:] = True
        if mask.any():
            grids, u = list(last_grid), np.zeros((N, 2))
            for i in np.flatnonzero(mask):
                if todo[i]:
                    grids[i], u[i] = fx[i]["reset_grid"][todo[i][0][1]], fx[i]["reset_u"][todo[i][0][1]]
                else:
                    grids[i] = SU.load("inv")[0]["reset_grid"][0]
            obs = env.reset_injected(U.pad_grids(env, grids), mask=mask.astype(np.uint8), start_u=u)
            for i in np.flatnonzero(mask):
                if todo[i]:
                    _check_reset(env, i, fx[i], todo[i].pop(0)[1], obs, group)
                    n_reset += 1
            continue
        acts = np.full((N, Cc), 6, np.int32) if rl else np.zeros((N, Cc), np.float32)
        for i, ev in enumerate(todo):
            if ev:
                a = SU.raw_action(fx[i], ev[0][1])
                acts[i, :len(a)] = a
        d = _flat(env.step(acts))
        grids = _grids(env)
        st = _state(env, ("last_fail", "history_count"))
        for i, ev in enumerate(todo):
            last_grid[i] = grids[i]
            if not ev:
                continue
            g, k = fx[i], ev.pop(0)[1]
            at = "%s env %d step %d: " % (group, i, k + 1)
            U.check_step(g, k, *_sizes(env, i, d), grids[i], label="%s env %d" % (group, i))
            assert float(st["last_fail"][i]) == float(g["last_fail"][k]), at + "last_fail"
            assert min(int(st["history_count"][i]), H.HISTORY_LENGTH) == int(g["hist_len"][k]), at + "history count"
            n_step += 1
            if rl:
                nC, nS = g["applied_value"].shape[1], g["sensor_readings"].shape[1]
                assert U.same_bits(d["applied_value"][i, :nC], g["applied_value"][k]), at + "applied value"
                assert U.same_bits(d["delta"][i, :nC], g["delta"][k]), at + "delta"
                mine = np.array([d["step_stat." + q][i] for q in STAT_KEYS], np.int64)
                target = float(SU.load("rl")[1]["target_temperature"])
                assert np.array_equal(mine, AU.counts_numpy(d["obs.sensor_readings"][i, :nS], target)), at + "counts (own readings)"
                assert np.array_equal(mine, AU.recorded_counts(g, k)), at + "counts (recorded)"
                assert int(d["step_stat.fail"][i]) == int(g["stat_fail"][k]), at + "fail"
                rec = float(g["stat_cooler_power"][k])      # the bound of test_gpu_anyhvac_actions.py, derived there
                assert abs(float(d["step_stat.cooler_power"][i]) - rec) <= (nC + 7) * float(np.spacing(np.float32(rec))) + 1e-4, at
    assert env.check_errors() == 0
    assert n_reset == sum(len(g["reset_at"]) for n, g in zip(layout, fx) if n)
    assert n_step == sum(int(g["n_steps"]) for n, g in zip(layout, fx) if n)
    env.close()


def test_same_step_autoreset_in_the_kernel_equals_a_masked_reset_across_both_restarts_of_back():
    """`back` under same-step autoreset with the reset grids injected, against autoreset_mode='disabled' followed by
    reset_injected under the step's done mask: the new episode's observation, the finished one's, every other output and
    the whole state are bit-equal, at both restarts (rest index from the history, 100 entries back) and the steps between"""
    g = SU.load("back")[0]
    at = g["reset_at"].tolist()
    T = int(g["n_steps"])
    a, _ = _batch(("back",), mode="same_step")
    b, _ = _batch(("back",), mode="disabled")
    u0 = g["reset_u"][0][None]
    for env in (a, b):
        env.reset_injected(g["reset_grid"][0][None], start_u=u0)
    ra = _flat(a.rollout(g["action"][:250, None]))      # the cool 250 steps: one launch each
    rb = _flat(b.rollout(g["action"][:250, None]))
    assert not ra["terminated"].any()
    _same({k: v for k, v in ra.items() if "final" not in k}, rb, "the first 250 steps: ")
    restarts = 0
    for k in range(250, T):
        fresh = g["reset_grid"][min(restarts + 1, 2)][None]
        da = _flat(a.step_injected(g["action"][k][None], fresh))
        db = _flat(b.step(g["action"][k][None]))
        label = "step %d: " % (k + 1)
        done = bool(db["terminated"][0])
        assert done == bool(da["terminated"][0]) == (k + 1 in at) and bool(da["_final_obs"][0]) == done
        for q in ("reward", "truncated", "cool_power", "heat_power", "time", "rest_idx", "warning_count", "over_tolerace"):
            assert U.same_bits(da[q], db[q]), label + q
        if done:
            restarts += 1
            for q in ("sensor_readings", "heat_readings", "action_temp", "timestep"):
                assert U.same_bits(da["final_obs." + q], db["obs." + q]), label + "final " + q
            obs = b.reset_injected(fresh, mask=db["terminated"].astype(np.uint8))
            for q in ("sensor_readings", "heat_readings", "action_temp", "timestep"):
                assert U.same_bits(da["obs." + q], obs[q].cpu().numpy()), label + "new " + q
            st = _state(a, START_KEYS)
            assert float(st["t"][0]) == float(g["reset_t"][restarts]) and int(st["rest_idx"][0]) == int(g["reset_rest_idx"][restarts])
        else:
            for q in ("sensor_readings", "heat_readings", "action_temp", "timestep"):
                assert U.same_bits(da["obs." + q], db["obs." + q]), label + q
        sa, sb = _state(a, None), _state(b, None)
        assert all(U.same_bits(sa[q], sb[q]) for q in sa), label + "state"
    assert restarts == 2 and a.check_errors() == 0 and b.check_errors() == 0
    a.close()
    b.close()


def _early_pair(n=1, **kw):
    g = SU.load("early")[0]
    envs = []
    for _ in range(2):
        env, _ = _batch(("early",) * n, mode="same_step", seed=7, **kw)
        env.reset_injected(np.repeat(g["reset_grid"][0][None], n, axis=0), start_u=np.repeat(g["reset_u"][0][None], n, axis=0))
        envs.append(env)
    return g, envs


def test_rollout_in_one_launch_equals_step_launches_across_a_failure_and_its_restart():
    """`early` with ones for 25 steps under same-step autoreset, the reset grids from the engine's Philox stream: the
    failure at step 11 (as recorded), the restart at t = 0 from history entry 0, and the steps of the next episode"""
    g, (a, b) = _early_pair()
    T, C = 25, g["action"].shape[1]
    acts = np.ones((T, 1, C), np.float32)
    roll = _flat(a.rollout(acts))
    rows = [_flat(b.step(acts[k])) for k in range(T)]
    steps = {k: np.stack([r[k] for r in rows]) for k in rows[0]}
    _same(steps, roll, "step vs rollout: ")
    fails = np.flatnonzero(roll["terminated"][:, 0])
    assert fails[0] == 10 and roll["obs.timestep"][10, 0] == 0 and roll["time"][11, 0] == 30.0      # restarted at t = 0
    sa, sb = _state(a, None), _state(b, None)
    assert all(U.same_bits(sa[q], sb[q]) for q in sa)
    assert float(sa["last_fail"][0]) == roll["time"][fails[-1], 0] and int(sa["history_count"][0]) == T - len(fails)
    assert a.check_errors() == 0 and b.check_errors() == 0
    a.close()
    b.close()


def test_rollout_teacher_equals_controller_call_and_step_across_a_failure_and_its_restart():
    """the same room under the `gt` PID teacher with the default gains: the room is too hot for it, it fails at step 11"""
    g, (a, b) = _early_pair()
    T = 16
    for env in (a, b):
        env.set_pid("gt")
    out = a.rollout_teacher(T)      # (info["action"]: what the teacher did)
    roll = _flat(out)
    rows = []
    for k in range(T):
        act = b.pid_action()
        r = _flat(b.step(act))
        r["action"] = act.cpu().numpy()
        rows.append(r)
    steps = {k: np.stack([r[k] for r in rows]) for k in rows[0]}
    _same(steps, roll, "controller + step vs rollout_teacher: ")
    assert roll["terminated"][:, 0].any() and not roll["terminated"][-1, 0]
    k = int(np.flatnonzero(roll["terminated"][:, 0])[0])
    assert roll["obs.timestep"][k, 0] == 0 and float(_state(a, ("last_fail",))["last_fail"][0]) == roll["time"][k, 0]
    sa, sb = _state(a, None), _state(b, None)
    assert all(U.same_bits(sa[q], sb[q]) for q in sa)
    pa, pb = a.get_pid_state(), b.get_pid_state()
    assert all(torch.equal(pa[q], pb[q]) for q in pa)
    a.close()
    b.close()


def test_flags_are_per_env_one_copy_goes_on_after_the_failure_the_other_restarts():
    """two copies of `early`'s env, env 1 with overheat_no_terminated: it reports terminated = False and reward -30 on
    every failing step, moves last_fail each time and goes on; env 0 restarts at t = 0"""
    g = SU.load("early")[0]
    env, _ = _batch(("early", "early"), mode="same_step")
    env.set_overheat_no_termiated_training_only([False, True])
    env.reset_injected(np.stack([g["reset_grid"][0]] * 2), start_u=np.stack([g["reset_u"][0]] * 2))
    C = g["action"].shape[1]
    fresh = np.stack([g["reset_grid"][1]] * 2)
    fails = []
    for k in range(16):
        d = _flat(env.step_injected(np.ones((2, C), np.float32), fresh))
        st = _state(env, ("t", "last_fail", "history_count"))
        if k < 10:
            assert not d["terminated"].any() and not d["over_tolerace"].any()
            assert U.same_bits(d["obs.sensor_readings"][0], d["obs.sensor_readings"][1])
        assert not d["terminated"][1] and float(st["t"][1]) == float(g["reset_t"][0]) + 30.0 * (k + 1)
        if k >= 10:      # env 1 fails on every step from the 11th
            assert d["over_tolerace"][1] == 1 and d["reward"][1] == -30.0 and float(st["last_fail"][1]) == d["time"][1]
            assert int(st["history_count"][1]) == 10
            fails.append(float(st["last_fail"][1]))
        if k == 10:
            assert d["terminated"][0] and d["reward"][0] == -30.0 and float(st["t"][0]) == 0.0 and d["_final_obs"][0]
            assert float(st["last_fail"][0]) == float(g["reset_last_fail"][1]) == d["time"][0]
        elif k > 10:
            assert not d["terminated"][0] and float(st["t"][0]) == 30.0 * (k - 10)
    assert len(fails) == 6 and (np.diff(fails) == 30.0).all()
    assert env.check_errors() == 0
    env.close()


def test_state_round_trip_after_a_restart_carries_the_history():
    """14 steps (the restart after step 11), get_state, 20 steps — with the next failure and a restart that reads the
    history — set_state, the same 20 steps: bit-equal in every output and in the state after"""
    g = SU.load("early")[0]
    env, _ = _batch(("early",), mode="same_step")
    env.reset_injected(g["reset_grid"][0][None], start_u=g["reset_u"][0][None])
    C = g["action"].shape[1]
    ones, fresh = np.ones((1, C), np.float32), g["reset_grid"][1][None]
    for k in range(14):
        d = _flat(env.step_injected(ones, fresh))
    snap = env.get_state()
    assert int(snap["history_count"][0]) == 13 and float(snap["last_fail"][0]) > 0 and float(snap["t"][0]) == 90.0
    first = [_flat(env.step_injected(ones, fresh)) for _ in range(20)]
    end = _state(env, None)
    assert sum(bool(r["terminated"][0]) for r in first) >= 1
    env.set_state(**snap)
    second = [_flat(env.step_injected(ones, fresh)) for _ in range(20)]
    for k, (x, y) in enumerate(zip(first, second)):
        _same(x, y, "step %d: " % (k + 1))
    again = _state(env, None)
    assert all(U.same_bits(end[q], again[q]) for q in end)
    # a history that is not carried shows: with the count zeroed the same 20 steps end in another count
    env.set_state(**dict(snap, history_count=torch.zeros_like(snap["history_count"])))
    for _ in range(20):
        env.step_injected(ones, fresh)
    assert int(_state(env, ("history_count",))["history_count"][0]) == int(end["history_count"][0]) - 13
    # a new task is a new reference object: set_task forgets the failure and the history, and keeps the flags
    env.set_task([SU.load("early")[1]], generate_task=bool(g["generate_task"]))
    st = _state(env, ("last_fail", "history_count"))
    assert float(st["last_fail"][0]) == -1.0 and int(st["history_count"][0]) == 0
    env.reset_injected(g["reset_grid"][0][None], start_u=g["reset_u"][0][None])
    assert float(_state(env, ("t",))["t"][0]) == float(g["reset_t"][0]) > 0      # (the choice branch: the table went along)
    env.close()


def test_free_running_start_draws():
    """4,096 envs of `back`'s room (30 cells), resets only.  The same seed gives the same starts; an env's start depends on
    (seed, env_id_base + index, tick) and not on the batch around it; the grids do not depend on the flag; under
    generate_record every t is a whole step below max_steps; in the mixed branch the counts of t = 0 and of t > max_t / 2
    lie within 5 binomial standard deviations of their expectations, which come from the host's table and the inverse-CDF
    formula (host.start_t_probability), not from a device run"""
    n = 4096
    g, task, settings, _ = SU.load("back")
    max_t = int(settings["max_steps"] * settings["iter_per_step"] * settings["sec_per_iter"])

    def make(num, random, base=0, record=False):
        env = HVACVecEnv(num, seed=13, env_id_base=base, **settings)
        env.set_task([task], generate_task=bool(g["generate_task"]))
        env.set_random_start_t(random)
        env.set_generate_record(record)
        env.reset()
        st = _state(env, ("t", "grid", "rest_idx", "rest_start", "history_count"))
        return env, st

    a, sa = make(n, True)
    b, sb = make(n, True)
    assert U.same_bits(sa["t"], sb["t"]) and U.same_bits(sa["grid"], sb["grid"])
    b.close()
    c, sc = make(64, True, base=1000)
    assert U.same_bits(sc["t"], sa["t"][1000:1064]) and U.same_bits(sc["grid"], sa["grid"][1000:1064])
    c.close()
    off, so = make(n, False)
    assert U.same_bits(so["grid"], sa["grid"]) and not so["t"].any()
    off.close()
    t = sa["t"]
    assert (t == np.floor(t)).all() and t.min() >= 0 and t.max() <= max_t and not sa["rest_idx"].any()
    assert U.same_bits(sa["rest_start"][:, 0], t) and not sa["rest_start"][:, 1:].any()
    cdf = H.start_cdf(max_t)
    for what, lo, hi in (("t = 0", 0, 0), ("t > max_t / 2", max_t // 2 + 1, max_t)):
        p = H.start_t_probability(cdf, max_t, lo, hi)
        count = int(((t >= lo) & (t <= hi)).sum())
        assert abs(count - n * p) <= 5 * np.sqrt(n * p * (1 - p)), "%s: %d of %d, expected %.1f" % (what, count, n, n * p)
    a.set_generate_record(True)      # the next reset of the same envs: a uniform step each
    a.reset()
    k = _state(a, ("t",))["t"] / (settings["iter_per_step"] * settings["sec_per_iter"])
    assert (k == np.floor(k)).all() and k.min() >= 0 and k.max() < settings["max_steps"] and len(np.unique(k)) > 0.8 * n
    assert a.check_errors() == 0
    a.close()


def test_one_room_class_runs_the_trainers_configuration_through_a_failure_and_its_restart():
    """HVACEnvDiffAction(reward_mode=1) set up as run_rl.py:38-48 sets it up, on `rl`: the setters, reset()'s time, the
    failure, and the restart 100 steps before it"""
    from xenoverse_amd.anyhvac import HVACEnvDiffAction
    g, task, settings, flags = SU.load("rl")
    at = g["reset_at"].tolist()
    env = HVACEnvDiffAction(**settings)
    env.set_task(task, generate_task=bool(g["generate_task"]), **SU.RL_OPTS)
    env.set_random_start_t(True)
    env.set_generate_record(False)
    env.set_overheat_no_termiated_training_only(False)
    S, C = g["sensor_readings"].shape[1], g["applied_value"].shape[1]
    for kind, i in SU.events(g):
        if kind == "reset":
            obs, info = env.reset(state=g["reset_grid"][i], start_u=g["reset_u"][i])
            assert info["time"] == float(g["reset_t"][i]) and int(obs["timestep"][0]) == int(g["reset_timestep"][i])
            assert U.same_bits(obs["action_temp"], g["reset_action_temp"][i])
            continue
        obs, r, term, trunc, info = env.step(g["raw_action"][i])
        assert term == bool(g["terminated"][i]) == (i + 1 == at[1]) and info["time"] == float(g["t"][i])
        assert U.same_bits(info["last_control"]["value"], g["applied_value"][i])
        assert info["step_stat"]["fail"] == int(g["stat_fail"][i])
        assert [info["step_stat"][q] for q in STAT_KEYS] == AU.recorded_counts(g, i).tolist()
        if term:
            assert r == -30.0
        else:
            assert abs(r - float(g["reward"][i])) <= U.cost_tols(g, i, S, C)[2]
    assert env.check_errors() == 0
    env.close()
