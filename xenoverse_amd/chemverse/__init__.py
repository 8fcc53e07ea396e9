"""ChemVerse: the reference's chain-reaction simulator (xenoverse/chemverse/environment/simulator.py) as a batch.

  ChemVerseBatch(worlds, capacity).simulate(...)   N experiments, each under its own world, in one launch -> device tensors
  simulate_chain_reaction(world, ...)              the reference's signature and result dict, backend "device" or "host"
  simulate_chain_reactions(worlds, experiments)    a list of such calls from one launch
  scan(world, amounts, temperatures, durations, equipment, scales)   a Cartesian grid of conditions as one batch

  compute_optimal_cost(world, ...)                 the reference's ground-truth cost oracle (optimal.py): its signature and dict
  compute_optimal_costs(worlds, requests), chain_costs, one_pot_costs, ChemVerseOptimal   batches of it and its parts

The tool-call shell of the reference (sessions, perform_reaction, pathway evaluation, world samplers) is not part of this
package; of its cost and purification models, what the cost oracle calls is (optimal_host.py).
"""
import numpy as np

from . import tables as T
from .batch import ChemVerseBatch, prepare_experiments  # noqa: F401
from .optimal import (ChemVerseOptimal, chain_costs, compute_optimal_cost, compute_optimal_costs,  # noqa: F401
                      one_pot_costs)
from .optimal_host import find_reaction_chains, optimal_conditions, yield_threshold  # noqa: F401
from .host import (FAIL_INIT_P, FAIL_INIT_T, FAIL_NONE, FAIL_RUN_P, FAIL_RUN_T, HISTORY_MAX, LOG_MAX,  # noqa: F401
                   brentq_host, simulate_chain_host, simulate_one)
from .tables import build_tables  # noqa: F401

BACKENDS = ("device", "host")


def result_dict(tab, row, equipment, temperature_C, pressure_atm, duration_s, unknown=()):
    """one experiment's arrays (row: name -> numpy row / scalar, with history and log) -> the reference's dict (:695-716,
    :780-806, :861-880), key for key.  unknown: (id, grams) pairs outside the world, which the reference carries through."""
    ids, rids = tab["chem_ids"], tab["rxn_ids"]
    e = T.equipment_index(tab, equipment)
    spec = tab["equip_specs"][e]
    min_T, max_T, max_P = spec["min_temp_C"], spec["max_temp_C"], spec["max_pressure_atm"]
    name = equipment or "open_beaker"
    if isinstance(name, (int, np.integer)):
        name = tab["equip_names"][int(name)]
    failure = int(row["failure"])
    final_T, final_P = float(row["final_T"]), float(row["final_P"])
    tail = {"equipment": name, "vessel_type": spec["vessel_type"], "thermal_mode": spec["thermal_mode"]}

    def above(a):
        return {ids[c]: float(a[c]) for c in range(len(ids)) if a[c] > 1e-9}

    if failure in (FAIL_INIT_T, FAIL_INIT_P):
        reason = ("Initial temperature %.1f°C outside equipment range [%s, %s]°C" % (final_T, min_T, max_T)
                  if failure == FAIL_INIT_T else
                  "Initial pressure %.2f atm exceeds equipment limit %s atm" % (final_P, max_P))
        out = {"final_pool_g": {}, "consumed_g": {}, "produced_g": {}, "byproduct_g": {}, "net_consumed_g": {},
               "net_produced_g": {}, "gas_lost_g": {}, "reactions_fired": {}, "chain_reaction": False, "num_steps_simulated": 0,
               "converged": False, "final_temperature_C": round(final_T, 2), "final_pressure_atm": round(final_P, 4),
               "temperature_history": [], "reaction_log": []}
        out.update(tail)
        out.update({"equipment_failure": True, "failure_reason": reason})
        return out

    num_steps = int(row["num_steps"])
    dt = duration_s / num_steps
    fired = {rids[r]: int(row["fired"][r]) for r in range(len(rids)) if row["fired"][r] > 0}
    history = [{"step": int(row["hist_step"][i]), "time_s": round((int(row["hist_step"][i]) + 1) * dt, 2),
                "temperature_C": round(float(row["hist_T"][i]), 2), "pressure_atm": round(float(row["hist_P"][i]), 4)}
               for i in range(int(row["hist_count"]))]
    log = [{"step": int(row["log_step"][i]), "time_s": round((int(row["log_step"][i]) + 1) * dt, 2),
            "reactions_active": int(row["log_active"][i]), "temperature_C": round(float(row["log_T"][i]), 2),
            "pressure_atm": round(float(row["log_P"][i]), 4),
            "consumed": {k: round(v, 6) for k, v in above(row["log_consumed"][i]).items()},
            "produced": {k: round(v, 6) for k, v in above(row["log_produced"][i]).items()}}
           for i in range(int(row["log_count"]))]
    if failure in (FAIL_RUN_T, FAIL_RUN_P):
        reason = ("Temperature %.1f°C exceeded equipment limit [%s, %s]°C" % (final_T, min_T, max_T)
                  if failure == FAIL_RUN_T else
                  "Pressure %.2f atm exceeded equipment limit %s atm" % (final_P, max_P))
        out = {"final_pool_g": {}, "consumed_g": above(row["consumed"]), "produced_g": {}, "byproduct_g": {},
               "net_consumed_g": {}, "net_produced_g": {}, "gas_lost_g": {}, "reactions_fired": fired,
               "chain_reaction": len(fired) > 1, "num_steps_simulated": int(row["failure_step"]) + 1, "converged": False,
               "final_temperature_C": round(final_T, 2), "final_pressure_atm": round(final_P, 4),
               "temperature_history": history, "reaction_log": log}
        out.update(tail)
        out.update({"equipment_failure": True, "failure_reason": reason})
        return out

    consumed, produced = row["consumed"], row["produced"]
    net_c = {ids[c]: float(consumed[c] - produced[c]) for c in range(len(ids))
             if consumed[c] != 0 and consumed[c] - produced[c] > 1e-9}
    net_p = {ids[c]: float(produced[c] - consumed[c]) for c in range(len(ids))
             if produced[c] != 0 and produced[c] - consumed[c] > 1e-9}
    pool = above(row["final_pool"])
    for cid, g in unknown:
        if g > 1e-9:
            pool[cid] = g
    out = {"final_pool_g": pool, "consumed_g": above(consumed), "produced_g": above(produced),
           "byproduct_g": above(row["byproduct"]), "net_consumed_g": net_c, "net_produced_g": net_p, "reactions_fired": fired,
           "chain_reaction": len(fired) > 1, "num_steps_simulated": num_steps, "converged": bool(row["converged"]),
           "final_temperature_C": round(final_T, 2), "final_pressure_atm": round(final_P, 4), "temperature_history": history,
           "reaction_log": log, "gas_lost_g": above(row["gas_lost"])}
    out.update(tail)
    return out


def simulate_chain_reactions(world_or_worlds, experiments, backend="device", device="cuda:0"):
    """experiments: dicts of simulate_chain_reaction's arguments (initial_amounts_g, temperature_C, pressure_atm, duration_s,
    equipment, heating_rate_C_per_s, vessel_volume_L, step_seconds — one value for the whole call — and `world`, an index
    into the list of worlds, default 0) -> the reference's result dicts, from ONE launch (backend "device") or from the host
    restatement (backend "host")."""
    if backend not in BACKENDS:
        raise ValueError("backend must be one of %s" % (BACKENDS,))
    worlds = world_or_worlds
    if isinstance(worlds, dict) or hasattr(worlds, "chemicals"):
        worlds = [worlds]
    tabs = [T.build_tables(w) for w in worlds]
    if not experiments:
        return []
    steps = set(float(e.get("step_seconds", 5.0)) for e in experiments)
    if len(steps) != 1:
        raise ValueError("one call takes one step_seconds")
    step_seconds = steps.pop()
    known, unknown, widx = [], [], []
    for e in experiments:
        w = int(e.get("world", 0))
        if not 0 <= w < len(tabs):
            raise ValueError("world %d is outside [0, %d)" % (w, len(tabs)))
        ids = set(tabs[w]["chem_ids"])
        known.append({c: g for c, g in e["initial_amounts_g"].items() if c in ids})
        unknown.append([(c, g) for c, g in e["initial_amounts_g"].items() if c not in ids])
        widx.append(w)
    args = dict(temperature_C=[e["temperature_C"] for e in experiments], pressure_atm=[e["pressure_atm"] for e in experiments],
                duration_s=[e["duration_s"] for e in experiments], equipment=[e.get("equipment") for e in experiments],
                heating_rate_C_per_s=[e.get("heating_rate_C_per_s", 0.0) for e in experiments],
                vessel_volume_L=[e.get("vessel_volume_L", 1.0) for e in experiments], step_seconds=step_seconds)
    if backend == "device":
        batch = ChemVerseBatch(tabs, len(experiments), device=device)
        try:
            res = {k: v.cpu().numpy() for k, v in batch.simulate(widx, known, record="log", **args).items()}
            flags = batch.check_errors()
        finally:
            batch.close()
        if flags:
            from .. import _lib
            raise _lib.XenoError("ChemVerse: device error flags 0x%x (include/xeno.h XV_DEVERR_*)" % flags)
    else:
        x = prepare_experiments(tabs, widx, known, **args)
        exps = [dict(world=widx[i], amounts=[(int(x["order"][i, j]), float(x["grams"][i, x["order"][i, j]]))
                                              for j in range(x["n_initial"][i])],
                     temperature_C=float(x["T"][i]), pressure_atm=float(x["P"][i]), duration_s=float(x["duration"][i]),
                     equipment=int(x["equipment"][i]), heating_rate_C_per_s=float(x["rate"][i]),
                     vessel_volume_L=float(x["volume"][i]), step_seconds=step_seconds) for i in range(x["n"])]
        res = simulate_chain_host(tabs, exps, record="log")
    return [result_dict(tabs[widx[i]], {k: v[i] for k, v in res.items()}, e.get("equipment"), e["temperature_C"],
                        e["pressure_atm"], e["duration_s"], unknown[i]) for i, e in enumerate(experiments)]


def simulate_chain_reaction(world, initial_amounts_g, temperature_C, pressure_atm, duration_s, equipment=None,
                            heating_rate_C_per_s=0.0, vessel_volume_L=1.0, catalyst_ids=None, step_seconds=5.0,
                            backend="device", device="cuda:0"):
    """the reference's simulate_chain_reaction (simulator.py:639-650; catalyst_ids is unused there too)"""
    return simulate_chain_reactions(world, [dict(initial_amounts_g=initial_amounts_g, temperature_C=temperature_C,
                                                 pressure_atm=pressure_atm, duration_s=duration_s, equipment=equipment,
                                                 heating_rate_C_per_s=heating_rate_C_per_s, vessel_volume_L=vessel_volume_L,
                                                 step_seconds=step_seconds)], backend=backend, device=device)[0]


def scan(world, amounts, temperatures, durations, equipment, scales=(1.0,), pressure_atm=1.0, heating_rate_C_per_s=0.0,
         vessel_volume_L=1.0, step_seconds=5.0, batch=None, device="cuda:0"):
    """the Cartesian grid temperatures x durations x equipment x scales of one charge (amounts: dict id -> grams, multiplied by
    the scale) as ONE batch -> dict of device tensors shaped [len(temperatures), len(durations), len(equipment),
    len(scales), ...].  batch: a ChemVerseBatch over this world with room for the grid (default: made and closed here)."""
    temperatures, durations = [float(t) for t in temperatures], [float(d) for d in durations]
    equipment, scales = list(equipment), [float(s) for s in scales]
    grid = (len(temperatures), len(durations), len(equipment), len(scales))
    n = int(np.prod(grid))
    if n < 1:
        raise ValueError("scan needs at least one value on every axis")
    it, idur, ie, isc = (a.reshape(-1) for a in np.indices(grid))
    tab = T.build_tables(world if batch is None else batch.tables[0])
    eq = np.array([T.equipment_index(tab, e) for e in equipment], np.int32)
    charges = [{c: g * s for c, g in amounts.items()} for s in scales]
    own = batch is None
    if own:
        batch = ChemVerseBatch(tab, n, device=device)
    try:
        res = batch.simulate(0, [charges[k] for k in isc], np.array(temperatures)[it], pressure_atm, np.array(durations)[idur],
                             eq[ie], heating_rate_C_per_s, vessel_volume_L, step_seconds)
        flags = batch.check_errors()
    finally:
        if own:
            batch.close()
    if flags:
        from .. import _lib
        raise _lib.XenoError("ChemVerse: device error flags 0x%x (include/xeno.h XV_DEVERR_*)" % flags)
    return {k: v.reshape(grid + tuple(v.shape[1:])) for k, v in res.items()}
