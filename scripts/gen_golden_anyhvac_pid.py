"""Golden fixtures of the AnyHVAC PID teachers: the REFERENCE's own solvers (xenoverse/anyhvac/anyhvac_solver.py:
HVACSolverGTPID, HVACSolverLOCPID) driving the reference's env closed loop on the rooms of scripts/gen_golden_anyhvac.py.

Build-container tooling like that script, whose reference import, sampler check and room constants are reused: the
reference is imported read-only through oracle/_refimport.py, nothing under oracle/ is modified, only data is written.

Per run: the room's task is sampled as there (same constants, first seed, condition), env.reset(), solver = Solver(env),
then per step  flat = solver.policy(obs["sensor_readings"]); env.step(1 - flat[C:]).  PIDHost + HVACHost run alongside
from the recorded initial grid: the weight matrix, every flat action, acc_diff and every recorded quantity of the env step
must be bit-equal, or the script stops.  Margins taken along a run: eer_margin and fail_margin as in the env's fixtures,
switch_margin (the smallest |x + 0.05| over all switch decisions, x the pre-clip action value) and clip_margin (the
smallest distance of an unsaturated x from 0 or 1).  A seed whose switch margin is below 1e-9 is passed over.

closed_loop_dev_*: HVACHost + PIDHost closed loop 16 times, the readings fed to the controller perturbed per element by
-1, 0 or +1 float32 ulp at every step (what tests/anyhvac_util.py allows the device's readings); per step the largest
deviation from the unperturbed run of the readings fed and of the env action.  A CPU measurement of the host's
sensitivity, the yardstick of the device's closed-loop test.

tests/golden/pid_anyhvac_<name>.npz (the prefix in front, as qlearn_anymdp_* and mbrl_anymdp_*: anyhvac_* is the closed set
of the env's own fixtures): the flat task under task_*, settings, seed, init_grid, weights, gains, per step pid_readings,
pid_flat, pid_acc_diff and the env step's record (f64_rot: a leading axis of three gain triples).

usage: python scripts/gen_golden_anyhvac_pid.py
"""
import os
import sys
import zipfile

import numpy as np

import gen_golden_anyhvac as G

from xenoverse_amd.anyhvac import host as H  # noqa: E402
from xenoverse_amd.anyhvac import pid as P  # noqa: E402

MIN_SWITCH_MARGIN = 1e-9
N_PERTURBED = 16
FAST = dict(G.SLOW, iter_per_step=50, sec_per_iter=0.2)
GAIN_PICKS = ((0, 0, 0), (4, 5, 3), (9, 9, 9))      # indices into the grid search's default linspaces
# name -> (room of gen_golden_anyhvac.RUNS, solver kind, settings, steps, numpy.float64 gains)
RUNS = {"gt_rot": ("rot", "gt", G.SLOW, 40, False), "loc_rot": ("rot", "loc", G.SLOW, 40, False),
        "gt_wide": ("wide", "gt", G.SLOW, 6, False), "f64_rot": ("rot", "gt", FAST, 8, True)}
ENV_KEYS = ("action", "grid", "t", "reward", "terminated", "truncated", "cool_power", "heat_power", "rest_idx",
            "warning_count", "over_heat", "over_tolerace", "energy_cost", "target_cost", "timestep", "sensor_readings",
            "heat_readings", "action_temp")


def _row(obs, r, term, trunc, info, a, grid, t, rest, warn):
    return dict(action=a, grid=grid, t=np.float64(t), reward=np.float64(r), terminated=bool(term), truncated=bool(trunc),
                cool_power=info["cool_power"], heat_power=info["heat_power"], rest_idx=np.int32(rest),
                warning_count=np.int32(warn), over_heat=np.int32(info["over_heat"]),
                over_tolerace=np.int32(info["over_tolerace"]), energy_cost=np.float64(info["energy_cost"]),
                target_cost=np.float64(info["target_cost"]), timestep=obs["timestep"][0],
                **{q: obs[q] for q in ("sensor_readings", "heat_readings", "action_temp")})


def record(HVACEnv, Solver, ref_task, flat, kind, settings, gen, steps, gains, grid_seed):
    """one closed-loop run of the reference with PIDHost + HVACHost alongside -> dict of per-step arrays and margins"""
    env = HVACEnv(**settings)
    with G.quiet():
        env.set_task(ref_task, generate_task=gen)
        np.random.seed(grid_seed)
        obs = env.reset()[0]
        solver = Solver(env)
    init = env.state.copy()
    host = H.HVACHost(**settings)
    host.set_task(flat, generate_task=gen)
    hobs = host.reset(init)[0]
    mode = "python"
    if gains is not None:
        solver.kp, solver.ki, solver.kd = gains
        mode = "float64"
    pid = P.PIDHost(flat, kind, kp=solver.kp, ki=solver.ki, kd=solver.kd, sec_per_step=env.sec_per_step, gains=mode)
    assert type(pid.kp) is type(solver.kp) and pid.delta_t == solver.delta_t
    G.same(solver.corr_sensor_cooler, pid.corr_sensor_cooler, "corr_sensor_cooler", 0)
    G.same(obs["sensor_readings"], hobs["sensor_readings"], "the first observation", 0)
    C = len(ref_task["coolers"])
    rows, fail, switch, clip = {}, np.inf, np.inf, np.inf
    for k in range(steps):
        readings = obs["sensor_readings"]
        with G.quiet():
            fl = solver.policy(readings)
        hfl = pid.policy(hobs["sensor_readings"])
        G.same(fl, hfl, "the flat action", k + 1)
        G.same(solver.acc_diff, pid.acc_diff, "acc_diff", k + 1)
        G.same(solver.last_observation, pid.last_observation, "last_observation", k + 1)
        x = pid.last_x
        switch = min(switch, float(np.abs(x + 0.05).min()))
        inner = x[(x > 0.0) & (x < 1.0)]
        if inner.size:
            clip = min(clip, float(np.minimum(inner, 1.0 - inner).min()))
        a = 1 - fl[C:]
        with G.quiet():
            obs, r, term, trunc, info = env.step(a)
        hobs, hr, hterm, htrunc, hinfo = host.step(1 - hfl[C:])
        rec = _row(obs, r, term, trunc, info, a, env.state, env.t, env.current_rest_cooler_idx, env.warning_count)
        mine = _row(hobs, hr, hterm, htrunc, hinfo, a, host.state, host.t, host.rest_idx, host.warning_count)
        rec.update(pid_readings=readings, pid_flat=fl, pid_acc_diff=solver.acc_diff.copy())
        for q in rec:
            if q in mine:
                G.same(rec[q], mine[q], q, k + 1)
            rows.setdefault(q, []).append(np.array(rec[q]))
        fail = min(fail, float(np.abs(obs["sensor_readings"].astype(np.float64) - env.failure_upperbound).min()))
    out = {q: np.array(v) for q, v in rows.items()}
    out.update(init_grid=init, weights=np.array(solver.corr_sensor_cooler), eer_margin=np.float64(host.eer_margin),
               fail_margin=np.float64(fail), switch_margin=np.float64(switch), clip_margin=np.float64(clip),
               avg_total_heat=np.float64(env.avg_total_heat), failure_upperbound=np.float64(env.failure_upperbound),
               gains=np.array([solver.kp, solver.ki, solver.kd], np.float64))
    return out


def closed_loop_dev(flat, kind, settings, gen, init, steps, gains, mode, seed):
    """-> (readings_dev[steps], action_dev[steps]) of N_PERTURBED perturbed host runs against the unperturbed one"""
    host = H.HVACHost(**settings)
    host.set_task(flat, generate_task=gen)
    weights = P.pid_weights(flat, kind)
    C = weights.shape[1]
    rng = np.random.RandomState(seed)

    def run(perturb):
        obs = host.reset(init)[0]
        pid = P.PIDHost(flat, kp=gains[0], ki=gains[1], kd=gains[2], sec_per_step=host.iter_per_step * host.sec_per_iter,
                        gains=mode, weights=weights)
        fed, acts = [], []
        for _ in range(steps):
            r = obs["sensor_readings"]
            if perturb:
                d = rng.randint(-1, 2, r.shape)
                r = np.where(d == 0, r, np.nextafter(r, np.where(d > 0, np.float32(np.inf), np.float32(-np.inf))))
                r = r.astype(np.float32)
            a = 1 - pid.policy(r)[C:]
            fed.append(r.astype(np.float64))
            acts.append(a.astype(np.float64))
            obs = host.step(a)[0]
        return np.array(fed), np.array(acts)
    base = run(False)
    dev_r, dev_a = np.zeros(steps), np.zeros(steps)
    for _ in range(N_PERTURBED):
        fed, acts = run(True)
        dev_r = np.maximum(dev_r, np.abs(fed - base[0]).max(axis=1))
        dev_a = np.maximum(dev_a, np.abs(acts - base[1]).max(axis=1))
    return dev_r, dev_a


def save_npz(path, arrays):
    """numpy.savez_compressed with the members' timestamps fixed: the same data gives the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w") as f:
                np.lib.format.write_array(f, np.asanyarray(arrays[k]), allow_pickle=False)


def main():
    S, HVACEnv = G._reference()
    from xenoverse.anyhvac.anyhvac_solver import HVACSolverGridSearchPID, HVACSolverGTPID, HVACSolverLOCPID
    solvers = dict(gt=HVACSolverGTPID, loc=HVACSolverLOCPID)
    # the default linspaces, from the reference constructor's own default ranges
    grids = [np.linspace(r[0], r[1], r[2]) for r in HVACSolverGridSearchPID.__init__.__defaults__]
    for name, (room, kind, settings, steps, f64) in RUNS.items():
        config, seed0, cond, _, gen = G.RUNS[room][:5]
        triples = [tuple(g[i] for g, i in zip(grids, pick)) for pick in GAIN_PICKS] if f64 else [None]
        for seed in range(seed0, seed0 + 50):
            try:
                ref, flat = G.sample_both(S, seed, config)
            except ValueError:
                continue
            if not cond(ref):
                continue
            outs = [record(HVACEnv, solvers[kind], ref, flat, kind, settings, gen, steps, t, 7000 + seed) for t in triples]
            if all(o["eer_margin"] >= G.MIN_EER_MARGIN and o["fail_margin"] >= G.MIN_FAIL_MARGIN
                   and o["switch_margin"] >= MIN_SWITCH_MARGIN for o in outs):
                break
            print("%s: seed %d passed over" % (name, seed))
        else:
            raise SystemExit("no seed qualifies for %s" % name)
        devs = [closed_loop_dev(flat, kind, settings, gen, o["init_grid"], steps, o["gains"],
                                "float64" if f64 else "python", 9000 + seed + i) for i, o in enumerate(outs)]
        shared = ("init_grid", "weights", "avg_total_heat", "failure_upperbound")
        if f64:
            assert all(G_same_bits(o[q], outs[0][q]) for o in outs for q in shared)
            out = {q: (outs[0][q] if q in shared else np.array([o[q] for o in outs])) for q in outs[0]}
            out.update(closed_loop_dev_readings=np.array([dv[0] for dv in devs]),
                       closed_loop_dev_action=np.array([dv[1] for dv in devs]))
        else:
            out = outs[0]
            out.update(closed_loop_dev_readings=devs[0][0], closed_loop_dev_action=devs[0][1])
        out.update(seed=np.int32(seed), generate_task=np.bool_(gen), kind=np.array(kind), n_steps=np.int32(steps),
                   gains_float64=np.bool_(f64), **{"set_" + k: np.asarray(v) for k, v in settings.items()})
        out.update({"task_" + k: np.asarray(v) for k, v in flat.items()})
        path = os.path.join(G.GOLD, "pid_anyhvac_%s.npz" % name)
        save_npz(path, out)
        print("%-8s %7d bytes  seed %d  switch margin %.3g  clip margin %.3g  first action all ones: %s  terminated: %s"
              % (name, os.path.getsize(path), seed, np.min(out["switch_margin"]), np.min(out["clip_margin"]),
                 bool((out["action"][..., 0, :] == 1).all()), bool(out["terminated"].any())))
        sys.stdout.flush()


def G_same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


if __name__ == "__main__":
    main()
