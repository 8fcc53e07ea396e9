"""Golden fixtures of AnyHVAC's RL action spaces: the REFERENCE's own HVACEnvDiffAction and HVACEnvDiscreteAction
(xenoverse/anyhvac/anyhvac_env.py) on the rooms of scripts/gen_golden_anyhvac.py.

Build-container tooling like that script, whose reference import, sampler check, room constants and seeds are reused: the
reference is imported read-only through oracle/_refimport.py, nothing under oracle/ is modified (gymnasium.spaces gets a
MultiDiscrete stand-in in this process only), only data is written.

Per run: the room's task is sampled as there (same constants, first seed, condition), env.set_task(task, ...), env.reset(),
then the run's scripted actions.  DiffActionHost / DiscreteActionHost (xenoverse_amd/anyhvac/actions.py) run alongside from
the recorded initial grid: the applied value, the step delta, the action cost, every step_stat entry, the running averages
and every recorded quantity of the env step must be bit-equal, or the script stops.  stat_margin is the smallest
|reading - target - k| over k in {0, +-2, +-4, +-6} on any step; a seed that leaves it below 1e-4 K, or eer_margin /
fail_margin below their minima, is passed over.

tests/golden/act_anyhvac_<name>.npz (the prefix in front: anyhvac_* and pid_anyhvac_* are closed sets): the flat task
under task_*, settings, seed, init_grid, per step raw_action, applied_value, delta, action_cost, stat_<key>, the running
averages run_* and the env step's record.

usage: python scripts/gen_golden_anyhvac_actions.py
"""
import os
import sys

import numpy as np

import gen_golden_anyhvac as G
import gen_golden_anyhvac_pid as GP

from xenoverse_amd.anyhvac import actions as A  # noqa: E402

MIN_STAT_MARGIN = 1e-4
FAST = dict(G.SLOW, iter_per_step=50, sec_per_iter=0.2, reward_mode=1)
STAT_STEP_KEYS = ("reward", "cooler_power", "fail") + A.STAT_KEYS


def scripted_md(n_steps, C):
    """integer indices from cooler 1 on (cooler 0 rests during the first hour): always 0 (the target - 3 clamp), always 12
    (the 1.0 clip), 2 / 10 alternating (a reversal every step; the window evicts from step 11), 8 / 6 / 4 cycling (a zero
    between opposite signs is no reversal); the other columns random"""
    a = np.zeros((n_steps, C), np.int64)
    for c in range(C):
        a[:, c] = np.random.RandomState(100 + c).randint(0, 13, n_steps)
    k = np.arange(n_steps)
    a[:, 1], a[:, 2], a[:, 3], a[:, 4] = 0, 12, np.where(k % 2 == 0, 2, 10), np.array([8, 6, 4])[k % 3]
    return a


def uniform32(seed):
    return lambda n_steps, C: np.random.RandomState(seed).uniform(0, 1, (n_steps, C)).astype(np.float32)


def random_indices(seed):
    return lambda n_steps, C: np.random.RandomState(seed).randint(0, 13, (n_steps, C))


# name -> (room of gen_golden_anyhvac.RUNS, class, settings, steps, actions(n_steps, C), discretize, cost, too_cold_limit)
RUNS = {
    "diff_md": ("mode1", "diff", FAST, 24, scripted_md, True, True, True),
    "diff_rot": ("rot", "diff", G.SLOW, 125, uniform32(3), False, False, False),
    "disc": ("mode1", "discrete", FAST, 8, uniform32(4), False, False, False),
    "diff_wide": ("wide", "diff", G.SLOW, 6, random_indices(5), True, True, True),
}


def _reference_classes():
    S, _ = G._reference()
    import gymnasium

    class MultiDiscrete(gymnasium.spaces.Space):
        def __init__(self, nvec):
            self.nvec = np.asarray(nvec)
    if not hasattr(gymnasium.spaces, "MultiDiscrete"):
        gymnasium.spaces.MultiDiscrete = MultiDiscrete
    from xenoverse.anyhvac.anyhvac_env import HVACEnvDiffAction, HVACEnvDiscreteAction
    return S, dict(diff=HVACEnvDiffAction, discrete=HVACEnvDiscreteAction)


def record(Env, kind, ref_task, flat, settings, gen, actions, discretize, cost, too_cold):
    env = Env(**settings)
    host = (A.DiffActionHost if kind == "diff" else A.DiscreteActionHost)(**settings)
    with G.quiet():
        if kind == "diff":      # (HVACEnvDiffAction.set_task always forms the week-long heat average)
            env.set_task(ref_task, discretize_rl_action_space=discretize, add_action_cost=cost, too_cold_limit=too_cold)
            host.set_task(flat, discretize_rl_action_space=discretize, add_action_cost=cost, too_cold_limit=too_cold)
            gen = False
        else:
            env.set_task(ref_task, generate_task=gen)
            host.set_task(flat, generate_task=gen)
        env.reset()
    assert host.avg_total_heat == env.avg_total_heat
    init = env.state.copy()
    host.reset(init)
    rows, fail, margin = {}, np.inf, np.inf
    for k, a in enumerate(actions):
        if kind == "diff":
            delta = env._diff_action(a)[1]      # (pure: the env's state is untouched)
            hdelta = host.map_action(a)[1]
        else:
            delta = hdelta = np.zeros(len(a))
        with G.quiet():
            obs, r, term, trunc, info = env.step(a)
        hobs, hr, hterm, htrunc, hinfo = host.step(a)
        rec = GP._row(obs, r, term, trunc, info, env.last_action["value"], env.state, env.t, env.current_rest_cooler_idx,
                      env.warning_count)
        mine = GP._row(hobs, hr, hterm, htrunc, hinfo, host.value, host.state, host.t, host.rest_idx, host.warning_count)
        for d, e, i, dl in ((rec, env, info, delta), (mine, host, hinfo, hdelta)):
            d["applied_value"] = d.pop("action")
            d.update(delta=dl, action_cost=np.float64(i.get("action_cost", 0.0)),
                     **{"stat_" + q: np.float64(i["step_stat"][q]) for q in STAT_STEP_KEYS},
                     **{"run_" + q: np.array(getattr(e, q), np.float64) for q in A.RUNNING_KEYS})
        assert type(info["step_stat"]["cooler_power"]) is type(hinfo["step_stat"]["cooler_power"])
        assert type(env.avg_cooler_power_per_step) is type(host.avg_cooler_power_per_step)
        for q in rec:
            G.same(rec[q], mine[q], q, k + 1)
            rows.setdefault(q, []).append(np.array(rec[q]))
        fail = min(fail, float(np.abs(obs["sensor_readings"].astype(np.float64) - env.failure_upperbound).min()))
        margin = min(margin, A.stat_margin(obs["sensor_readings"], env.target_temperature))
    out = {q: np.array(v) for q, v in rows.items()}
    raw = np.asarray(actions)
    out.update(raw_action=raw.astype(np.int32) if np.issubdtype(raw.dtype, np.integer) else raw, init_grid=init,
               eer_margin=np.float64(host.eer_margin), fail_margin=np.float64(fail), stat_margin=np.float64(margin),
               avg_total_heat=np.float64(env.avg_total_heat), failure_upperbound=np.float64(env.failure_upperbound),
               generate_task=np.bool_(gen), cost_table=A.COST_TABLE)
    return out


def main():
    S, classes = _reference_classes()
    for name, (room, kind, settings, steps, actions, discretize, cost, too_cold) in RUNS.items():
        config, seed0, cond, _, gen = G.RUNS[room][:5]
        for seed in range(seed0, seed0 + 50):
            try:
                ref, flat = G.sample_both(S, seed, config)
            except ValueError:
                continue
            if not cond(ref):
                continue
            out = record(classes[kind], kind, ref, flat, settings, gen, list(actions(steps, len(ref["coolers"]))),
                         discretize, cost, too_cold)
            if (out["eer_margin"] >= G.MIN_EER_MARGIN and out["fail_margin"] >= G.MIN_FAIL_MARGIN
                    and out["stat_margin"] >= MIN_STAT_MARGIN):
                break
            print("%s: seed %d passed over" % (name, seed))
        else:
            raise SystemExit("no seed qualifies for %s" % name)
        out.update(seed=np.int32(seed), kind=np.array(kind), n_steps=np.int32(steps), discretize=np.bool_(discretize),
                   add_action_cost=np.bool_(cost), too_cold_limit=np.bool_(too_cold),
                   **{"set_" + k: np.asarray(v) for k, v in settings.items()})
        out.update({"task_" + k: np.asarray(v) for k, v in flat.items()})
        path = os.path.join(G.GOLD, "act_anyhvac_%s.npz" % name)
        GP.save_npz(path, out)
        print("%-9s %7d bytes  seed %d  stat margin %.3g  rest %s  cost %.3g..%.3g  terminated: %s"
              % (name, os.path.getsize(path), seed, out["stat_margin"], sorted(set(out["rest_idx"].tolist())),
                 out["action_cost"].min(), out["action_cost"].max(), bool(out["terminated"].any())))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
