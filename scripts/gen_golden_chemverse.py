"""Golden fixtures of ChemVerse: the REFERENCE's own simulate_chain_reaction (xenoverse/chemverse/environment/simulator.py) on
three of its evaluation worlds, 128 experiments each.

Build-container tooling, like scripts/gen_golden_anyhvac.py: the reference is imported read-only through oracle/_refimport.py;
nothing under oracle/ is modified.  Only data is written, under tests/golden/:
  chemverse_world_{a,b,c}.json   three evaluation-world files, copied byte for byte: the one with the fewest reactions, the
                                 middle one and the one with the most (ordered by reactions, chemicals, file name)
  chemverse_runs_{a,b,c}.npz     the experiments, the reference's results, the sensitivity figures, recorded brentq calls and
                                 (first 32 experiments and the hand-made ones) the reference's own rounded result dicts

Experiments (RandomState(SEED + world)): pick a reaction, give its reactants base * coeff * U(0.5, 1.5) g with base ~ U(2, 40),
its catalysts base * U(0.02, 0.3); with probability 0.85 add base * U(1, 8) of a solvent that lists every non-solvent reactant;
with probability 0.4 add a second reaction's reactants and catalysts; equipment uniform over the world's; T ~ U(-10, 280);
P = 1 for the open beaker, else from {1, 1, 1.4, 3}; duration from {5, 12, 60, 300, 600} s; heating rate ~ U(-0.4, 0.6); volume
from {1, 0.5, 2}.  The last experiments of a fixture are hand-made for what the recipe does not reach: a reaction whose
reactants are all solvents ("__self__"), a strongly exothermic charge in the autoclave (isothermal excess heat), and the
first recipe experiment that the reference runs for all of its 120 steps, again with 175 s: 35 steps, every one of them
sampled, so that temperature_history is cut at 30 entries (the recipe's durations give 24 at most).

Recording: `round` in the simulator module's namespace is the identity (this process only), so temperatures and pressures are
stored unrounded; the rounded dicts come from a second, unpatched run.  The per-step reaction log is kept for the first 32
experiments only.

Sensitivity, measured on the reference: every experiment runs eight more times with numpy's exp and log, as the simulator
module sees them, moved by a random integer in [-2, 2] ulp; and once per further string-hash seed (the reference adds the
reactants' grams in the order of a Python set of id strings, simulator.py:369-371, which follows PYTHONHASHSEED).
  stable[n]      the discrete outcomes (fired counts, steps, converged, failure code and step, species above 1e-9) are the same
                 in all runs; at most 2 % may be unstable, or the script stops
  spread_*       the largest absolute deviation of every recorded float from the base run
  order_free[n]  every recorded value is bit-identical under all hash seeds
The script prints a count per branch and stops if a listed branch has none.

usage: python scripts/gen_golden_chemverse.py            (spawns its workers with fixed PYTHONHASHSEEDs)
"""
import io
import json
import os
import shutil
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import _refimport  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
SEED = 20261
N_EXP = 128
N_LOG = 32
N_HAND = 4
HASH_SEEDS = (0, 1, 2, 3, 4)
N_PERTURBED = 8
BRENT_KEEP = 300
HISTORY_MAX, LOG_MAX = 30, 20
BRANCHES = ("fired", "fired_two_or_more", "fail_initial", "fail_run_T", "fail_run_P", "mode_isothermal_fired",
            "mode_adiabatic_fired", "mode_open_air_fired", "mode_heating_fired", "mode_cooling_fired", "gas_loss",
            "phase_heat_positive", "phase_heat_negative", "sealed_pressure_moved", "byproduct", "catalysed", "solvent_external",
            "solvent_reactant", "solvent_neat", "solvent_none", "equilibrium_root", "equilibrium_zero", "equilibrium_max",
            "reactants_2", "reactants_3", "reactants_4", "coeff_1", "coeff_2", "coeff_3", "steps_1", "steps_3_dt_4", "steps_120",
            "idle_break", "product_appears_mid_run", "history_cut_at_30", "log_cut_at_20")
GAPS = ("solvent_self", "isothermal_excess")      # may be unreachable on these worlds; reported with the reason


def world_files():
    d = os.path.join(_refimport.REF_ROOT, "xenoverse", "chemverse", "worlds")
    rows = []
    for f in sorted(os.listdir(d)):
        if f.startswith("eval_world_") and f.endswith(".json"):
            w = json.load(open(os.path.join(d, f)))
            rows.append((len(w["reactions"]), len(w["chemicals"]), f))
    rows.sort()
    return [os.path.join(d, rows[i][2]) for i in (0, len(rows) // 2, len(rows) - 1)]


def make_experiments(world, rs, simulate):
    chems, rxns = world.chemicals, list(world.reactions.values())
    equip = list(world.equipment.keys())
    exps = []

    def charge(amounts, rxn, base):
        for cid, k in rxn.reactants:
            amounts[cid] = amounts.get(cid, 0.0) + base * k * rs.uniform(0.5, 1.5)
        for cid in rxn.catalysts:
            amounts[cid] = amounts.get(cid, 0.0) + base * rs.uniform(0.02, 0.3)

    for _ in range(N_EXP - N_HAND):
        rxn = rxns[rs.randint(len(rxns))]
        base = rs.uniform(2, 40)
        amounts = {}
        charge(amounts, rxn, base)
        if rs.uniform() < 0.85:
            non_solv = [c for c, _ in rxn.reactants if not chems[c].is_solvent]
            cands = [s for s, c in chems.items() if c.is_solvent and all(s in chems[x].solubility for x in non_solv)]
            if cands:
                s = cands[rs.randint(len(cands))]
                amounts[s] = amounts.get(s, 0.0) + base * rs.uniform(1, 8)
        if rs.uniform() < 0.4:
            charge(amounts, rxns[rs.randint(len(rxns))], base)
        eq = equip[rs.randint(len(equip))]
        exps.append(dict(amounts=amounts, temperature_C=float(rs.uniform(-10, 280)),
                         pressure_atm=1.0 if eq == "open_beaker" else float((1.0, 1.0, 1.4, 3.0)[rs.randint(4)]),
                         duration_s=float((5, 12, 60, 300, 600)[rs.randint(5)]), equipment=eq,
                         heating_rate_C_per_s=float(rs.uniform(-0.4, 0.6)), vessel_volume_L=float((1.0, 0.5, 2.0)[rs.randint(3)])))
    # hand-made: all-solvent reactants; exothermic charges in the autoclave, by delta_H, at two temperatures
    selfs = [r for r in rxns if all(chems[c].is_solvent for c, _ in r.reactants)]
    hot = sorted(rxns, key=lambda r: r.delta_H_kJ)[:2]
    hand = []
    if selfs:
        a = {}
        for cid, k in selfs[0].reactants:
            a[cid] = 20.0 * k
        for cid in selfs[0].catalysts:
            a[cid] = 2.0
        hand.append(dict(amounts=a, temperature_C=60.0, pressure_atm=1.0, duration_s=60.0, equipment="sealed_flask",
                         heating_rate_C_per_s=0.0, vessel_volume_L=1.0))
    for r, temp in zip(hot * 2, (220.0, 320.0, 150.0)):
        if len(hand) >= N_HAND - 1:
            break
        a = {}
        for cid, k in r.reactants:
            a[cid] = 150.0 * k
        for cid in r.catalysts:
            a[cid] = 30.0
        non_solv = [c for c, _ in r.reactants if not chems[c].is_solvent]
        cands = [s for s, c in chems.items() if c.is_solvent and all(s in chems[x].solubility for x in non_solv)]
        if cands:
            a[cands[0]] = a.get(cands[0], 0.0) + 400.0
        hand.append(dict(amounts=a, temperature_C=temp, pressure_atm=1.0, duration_s=60.0, equipment="autoclave",
                         heating_rate_C_per_s=0.0, vessel_volume_L=1.0))
    hand = hand[:N_HAND - 1]
    long_run = None
    for e in exps:
        if e["duration_s"] == 600.0:
            r = simulate(world, dict(e["amounts"]), e["temperature_C"], e["pressure_atm"], 175.0, equipment=e["equipment"],
                         heating_rate_C_per_s=e["heating_rate_C_per_s"], vessel_volume_L=e["vessel_volume_L"])
            if len(r["temperature_history"]) == HISTORY_MAX and r["temperature_history"][-1]["step"] == HISTORY_MAX - 1:
                long_run = dict(e, duration_s=175.0)
                break
    if long_run is None:
        raise SystemExit("no recipe experiment runs 30 sampled steps at 175 s")
    while len(hand) < N_HAND - 1:      # a world without some hand-made case: the long run's charge at other durations
        hand.append(dict(long_run, duration_s=(45.0, 90.0, 135.0)[len(hand)]))
    return exps + hand + [long_run]


class PerturbedNumpy(object):
    """numpy as the simulator module sees it, with exp and log moved by a random integer in [-2, 2] ulp"""

    def __init__(self, rs):
        self._rs = rs

    def __getattr__(self, name):
        return getattr(np, name)

    def _move(self, y):
        y = np.asarray(y, np.float64)
        k = self._rs.randint(-2, 3, size=y.shape)
        out = y.copy()
        for sign in (1, -1):
            for _ in range(2):
                m = (sign * k) > 0
                out = np.where(m, np.nextafter(out, sign * np.inf), out)
                k = k - sign * m
        return out if out.shape else np.float64(out)

    def exp(self, x):
        with np.errstate(all="ignore"):
            return self._move(np.exp(x))

    def log(self, x):
        with np.errstate(all="ignore"):
            return self._move(np.log(x))


def to_arrays(world, exps, results, steps_run):
    cidx = {c: i for i, c in enumerate(world.chemicals)}
    ridx = {r: i for i, r in enumerate(world.reactions)}
    n, C, R = len(exps), len(cidx), len(ridx)
    a = dict(final_pool=np.zeros((n, C)), consumed=np.zeros((n, C)), produced=np.zeros((n, C)), byproduct=np.zeros((n, C)),
             gas_lost=np.zeros((n, C)), fired=np.zeros((n, R), np.int32), num_steps=np.zeros(n, np.int32),
             steps_run=np.array(steps_run, np.int32), converged=np.zeros(n, np.uint8), failure=np.zeros(n, np.uint8),
             failure_step=np.full(n, -1, np.int32), final_T=np.zeros(n), final_P=np.zeros(n),
             hist_step=np.zeros((n, HISTORY_MAX), np.int32), hist_T=np.zeros((n, HISTORY_MAX)), hist_P=np.zeros((n, HISTORY_MAX)),
             hist_count=np.zeros(n, np.int32), log_step=np.zeros((N_LOG, LOG_MAX), np.int32),
             log_active=np.zeros((N_LOG, LOG_MAX), np.int32), log_T=np.zeros((N_LOG, LOG_MAX)), log_P=np.zeros((N_LOG, LOG_MAX)),
             log_consumed=np.zeros((N_LOG, LOG_MAX, C)), log_produced=np.zeros((N_LOG, LOG_MAX, C)),
             log_count=np.zeros(N_LOG, np.int32))
    for i, (e, r) in enumerate(zip(exps, results)):
        for key, src in (("final_pool", "final_pool_g"), ("consumed", "consumed_g"), ("produced", "produced_g"),
                         ("byproduct", "byproduct_g"), ("gas_lost", "gas_lost_g")):
            for cid, g in r[src].items():
                a[key][i, cidx[cid]] = g
        for rid, k in r["reactions_fired"].items():
            a["fired"][i, ridx[rid]] = k
        a["num_steps"][i] = max(1, int(np.ceil(e["duration_s"] / 5.0)))
        a["converged"][i] = r["converged"]
        if r.get("equipment_failure"):
            text = r["failure_reason"]
            a["failure"][i] = (1 if text.startswith("Initial temperature") else 2 if text.startswith("Initial pressure")
                               else 3 if text.startswith("Temperature") else 4)
            if a["failure"][i] >= 3:
                a["failure_step"][i] = r["num_steps_simulated"] - 1
        a["final_T"][i], a["final_P"][i] = r["final_temperature_C"], r["final_pressure_atm"]
        for j, h in enumerate(r["temperature_history"]):
            a["hist_step"][i, j], a["hist_T"][i, j], a["hist_P"][i, j] = h["step"], h["temperature_C"], h["pressure_atm"]
        a["hist_count"][i] = len(r["temperature_history"])
        if i < N_LOG:
            for j, h in enumerate(r["reaction_log"]):
                a["log_step"][i, j], a["log_active"][i, j] = h["step"], h["reactions_active"]
                a["log_T"][i, j], a["log_P"][i, j] = h["temperature_C"], h["pressure_atm"]
                for cid, g in h["consumed"].items():
                    a["log_consumed"][i, j, cidx[cid]] = g
                for cid, g in h["produced"].items():
                    a["log_produced"][i, j, cidx[cid]] = g
            a["log_count"][i] = len(r["reaction_log"])
    return a


FLOATS = ("final_pool", "consumed", "produced", "byproduct", "gas_lost", "final_T", "final_P", "hist_T", "hist_P", "log_T",
          "log_P", "log_consumed", "log_produced")
DISCRETE = ("fired", "num_steps", "steps_run", "converged", "failure", "failure_step", "hist_step", "hist_count", "log_step",
            "log_active", "log_count")


def discrete_equal(a, b):
    """per experiment: the discrete outcomes and the set of species above 1e-9 agree"""
    n = len(a["num_steps"])
    ok = np.ones(n, bool)
    for k in DISCRETE:
        m = min(len(a[k]), n)
        ok[:m] &= (a[k] == b[k]).reshape(m, -1).all(axis=1)
    for k in ("final_pool", "consumed", "produced", "byproduct", "gas_lost"):
        ok &= ((a[k] > 1e-9) == (b[k] > 1e-9)).all(axis=1)
    return ok


def worker(out_path, full):
    _refimport.setup()
    from xenoverse.chemverse.environment import simulator as sim
    from xenoverse.chemverse.world_gen.models import World
    import scipy.optimize as so
    real_brentq = so.brentq
    counts = dict((b, 0) for b in BRANCHES + GAPS)
    blob = {}
    for tag, path in zip("abc", world_files()):
        world = World.load(path)
        exps = make_experiments(world, np.random.RandomState(SEED + ord(tag)), sim.simulate_chain_reaction)
        chems = world.chemicals
        state = dict(calls=0, brent=[], record=False, kinds=None, exp_ev=None)
        orig = dict((k, getattr(sim, k)) for k in ("_find_applicable_reactions", "_find_common_solvent", "_step_single_reaction",
                                                   "solve_equilibrium_extent", "_process_phase_transitions",
                                                   "_update_vessel_state", "_apply_gas_loss"))

        def applicable(*a, **k):
            state["calls"] += 1
            return orig["_find_applicable_reactions"](*a, **k)

        def brentq(f, a, b, **kw):
            root, info = real_brentq(f, a, b, full_output=True, **kw)
            if state["record"]:
                cl = dict(zip(f.__code__.co_freevars, (c.cell_contents for c in f.__closure__)))
                state["brent"].append((cl["K_eq"], list(cl["reactant_amounts_mol"]), list(cl["reactant_coeffs"]),
                                       list(cl["product_amounts_mol"]), list(cl["product_coeffs"]), b, root, info.function_calls))
            state["kinds"] = "root"
            return root

        def solve(K, ra, rc, pa, pc):
            state["kinds"] = None
            xi = orig["solve_equilibrium_extent"](K, ra, rc, pa, pc)
            ev = state["exp_ev"]
            if ev is not None and min(x / c for x, c in zip(ra, rc)) > 0:
                ev.add("equilibrium_" + (state["kinds"] or ("zero" if xi == 0.0 else "max")))
            return xi

        def common(rxn, chemicals, pool, T, P):
            s = orig["_find_common_solvent"](rxn, chemicals, pool, T, P)
            if s is None and state["exp_ev"] is not None:
                state["exp_ev"].add("solvent_none")
            return s

        def single(rxn, chemicals, pool, T, P, dt, solvent_id=None):
            before = set(k for k, g in pool.items())
            res = orig["_step_single_reaction"](rxn, chemicals, pool, T, P, dt, solvent_id=solvent_id)
            ev = state["exp_ev"]
            if ev is not None and sum(res[0].values()) + sum(res[1].values()) >= 1e-12:
                ids = [c for c, _ in rxn.reactants]
                ev.add("solvent_" + ("neat" if solvent_id == "__neat__" else "self" if solvent_id == "__self__" else
                                     "none_on_recheck" if solvent_id is None else "reactant" if solvent_id in ids else "external"))
                ev.add("reactants_%d" % len(ids))
                for _, k in list(rxn.reactants) + list(rxn.products):
                    ev.add("coeff_%d" % k)
                if rxn.catalysts:
                    ev.add("catalysed")
                if any(g > 1e-12 for g in res[2].values()):
                    ev.add("byproduct")
                if state["step_index"] > 0 and any(p not in before for p in res[1]):
                    ev.add("product_appears_mid_run")
            return res

        def phase(*a, **k):
            h = orig["_process_phase_transitions"](*a, **k)
            if state["exp_ev"] is not None and h != 0:
                state["exp_ev"].add("phase_heat_positive" if h > 0 else "phase_heat_negative")
            return h

        def vessel_update(vessel, pool, chemicals, heat, dt, igm, **k):
            T0, P0 = vessel.temperature_C, vessel.pressure_atm
            orig["_update_vessel_state"](vessel, pool, chemicals, heat, dt, igm, **k)
            ev = state["exp_ev"]
            state["step_index"] += 1
            if ev is not None:
                if heat != 0:
                    ev.add("mode_%s_fired" % vessel.thermal_mode)
                if vessel.thermal_mode == "isothermal" and vessel.temperature_C != T0:
                    ev.add("isothermal_excess")
                if vessel.vessel_type == "sealed" and vessel.pressure_atm != P0:
                    ev.add("sealed_pressure_moved")

        def gas_loss(*a, **k):
            lost = orig["_apply_gas_loss"](*a, **k)
            if lost and state["exp_ev"] is not None:
                state["exp_ev"].add("gas_loss")
            return lost

        patched = dict(_find_applicable_reactions=applicable, _find_common_solvent=common, _step_single_reaction=single,
                       solve_equilibrium_extent=solve, _process_phase_transitions=phase, _update_vessel_state=vessel_update,
                       _apply_gas_loss=gas_loss)

        def run_all(track):
            res, steps = [], []
            for e in exps:
                state["calls"], state["step_index"] = 0, 0
                state["exp_ev"] = set() if track else None
                with np.errstate(all="ignore"):
                    r = sim.simulate_chain_reaction(world, dict(e["amounts"]), e["temperature_C"], e["pressure_atm"],
                                                    e["duration_s"], equipment=e["equipment"],
                                                    heating_rate_C_per_s=e["heating_rate_C_per_s"],
                                                    vessel_volume_L=e["vessel_volume_L"])
                res.append(r)
                steps.append(state["calls"])
                if track:
                    ev = state["exp_ev"]
                    fired = sum(r["reactions_fired"].values())
                    if fired:
                        ev.add("fired")
                    if len(r["reactions_fired"]) >= 2:
                        ev.add("fired_two_or_more")
                    if r.get("equipment_failure"):
                        t = r["failure_reason"]
                        ev.add("fail_initial" if t.startswith("Initial") else "fail_run_T" if t.startswith("Temp") else "fail_run_P")
                    ns = max(1, int(np.ceil(e["duration_s"] / 5.0)))
                    if ns == 1:
                        ev.add("steps_1")
                    if ns == 3 and e["duration_s"] / ns == 4.0:
                        ev.add("steps_3_dt_4")
                    if ns == 120 and state["calls"] == 120:
                        ev.add("steps_120")
                    if not fired and not r.get("equipment_failure") and state["calls"] == 3 and ns > 3:
                        ev.add("idle_break")
                    if len(r["temperature_history"]) == HISTORY_MAX and ns > HISTORY_MAX:
                        ev.add("history_cut_at_30")
                    if len(r["reaction_log"]) == LOG_MAX and sum(r["reactions_fired"].values()) > LOG_MAX + 3:
                        ev.add("log_cut_at_20")
                    for b in ev:
                        if b in counts:
                            counts[b] += 1
            return res, steps

        for k, f in patched.items():
            setattr(sim, k, f)
        so.brentq = brentq
        try:
            rounded = None
            if full:      # the reference's own rounded dicts, before `round` is replaced
                rounded, _ = run_all(False)
            sim.round = lambda x, n=None: x
            state["record"] = full
            base_res, base_steps = run_all(full)
            state["record"] = False
            base = to_arrays(world, exps, base_res, base_steps)
            for k, v in base.items():
                blob["%s/%s" % (tag, k)] = v
            if full:
                stable = np.ones(len(exps), bool)
                spread = dict((k, np.zeros_like(base[k])) for k in FLOATS)
                rs = np.random.RandomState(SEED + 7)
                for _ in range(N_PERTURBED):
                    sim.np = PerturbedNumpy(rs)
                    try:
                        res, steps = run_all(False)
                    finally:
                        sim.np = np
                    a = to_arrays(world, exps, res, steps)
                    stable &= discrete_equal(base, a)
                    for k in FLOATS:
                        spread[k] = np.maximum(spread[k], np.abs(a[k] - base[k]))
                blob["%s/stable" % tag] = stable
                for k in FLOATS:
                    blob["%s/spread_%s" % (tag, k)] = spread[k]
                # the experiments themselves
                cidx = {c: i for i, c in enumerate(chems)}
                n, C = len(exps), len(cidx)
                order, grams, n_init = np.full((n, C), -1, np.int8), np.zeros((n, C)), np.zeros(n, np.int32)
                for i, e in enumerate(exps):
                    for j, (cid, g) in enumerate(e["amounts"].items()):
                        order[i, j], grams[i, cidx[cid]] = cidx[cid], g
                    n_init[i] = len(e["amounts"])
                blob.update({tag + "/order": order, tag + "/grams": grams, tag + "/n_initial": n_init,
                             tag + "/equipment": np.array([list(world.equipment).index(e["equipment"]) for e in exps], np.int32)})
                for k in ("temperature_C", "pressure_atm", "duration_s", "heating_rate_C_per_s", "vessel_volume_L"):
                    blob["%s/%s" % (tag, k)] = np.array([e[k] for e in exps])
                keep = list(range(N_LOG)) + list(range(len(exps) - N_HAND, len(exps)))
                keep += [i for i in range(N_LOG, len(exps) - N_HAND) if base["failure"][i]][:12]
                text = json.dumps([[i, rounded[i]] for i in keep])
                blob[tag + "/dicts_json"] = np.frombuffer(text.encode(), np.uint8)
                # brentq calls: distinct ones, the first BRENT_KEEP
                seen, rows = set(), []
                for row in state["brent"]:
                    key = repr(row[:6])
                    if key not in seen:
                        seen.add(key)
                        rows.append(row)
                rows = rows[:BRENT_KEEP]
                m = len(rows)
                b = dict(K_eq=np.zeros(m), r_mol=np.zeros((m, 6)), r_coeff=np.zeros((m, 6), np.int32), n_r=np.zeros(m, np.int32),
                         p_mol=np.zeros((m, 4)), p_coeff=np.zeros((m, 4), np.int32), n_p=np.zeros(m, np.int32),
                         max_extent=np.zeros(m), root=np.zeros(m), calls=np.zeros(m, np.int32))
                for i, (K, ra, rc, pa, pc, mx, root, calls) in enumerate(rows):
                    b["K_eq"][i], b["max_extent"][i], b["root"][i], b["calls"][i] = K, mx, root, calls
                    b["n_r"][i], b["n_p"][i] = len(ra), len(pa)
                    b["r_mol"][i, :len(ra)], b["r_coeff"][i, :len(rc)] = ra, rc
                    b["p_mol"][i, :len(pa)], b["p_coeff"][i, :len(pc)] = pa, pc
                for k, v in b.items():
                    blob["%s/brent_%s" % (tag, k)] = v
        finally:
            for k, f in orig.items():
                setattr(sim, k, f)
            so.brentq = real_brentq
            sim.np = np
            if "round" in sim.__dict__:
                del sim.round
    if full:
        blob["counts_json"] = np.frombuffer(json.dumps(counts).encode(), np.uint8)
    np.savez(out_path, **blob)


def write_npz(path, arrays):
    """a compressed .npz whose bytes depend on the arrays alone (numpy's savez stamps the time of day on every member)"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--worker":
        return worker(sys.argv[2], sys.argv[3] == "full")
    if not _refimport.available():
        raise SystemExit("the reference tree is not present: fixtures are generated in the build container only")
    tmp = tempfile.mkdtemp(prefix="chemverse_golden_")
    try:
        runs = []
        for hs in HASH_SEEDS:
            out = os.path.join(tmp, "h%d.npz" % hs)
            env = dict(os.environ, PYTHONHASHSEED=str(hs))
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--worker", out, "full" if hs == 0 else "base"],
                                  env=env)
            runs.append(np.load(out))
        base = runs[0]
        counts = json.loads(bytes(base["counts_json"]).decode())
        print("branch counts over the three fixtures (experiments that took the branch):")
        for b in BRANCHES + GAPS:
            print("  %-26s %d" % (b, counts[b]))
        missing = [b for b in BRANCHES if not counts[b]]
        if missing:
            raise SystemExit("the fixtures do not reach: %s" % ", ".join(missing))
        for g in GAPS:
            if not counts[g]:
                print("not reached on these worlds: %s (%s)" % (g, {
                    "solvent_self": "no reaction of the three worlds has only solvents as reactants",
                    "isothermal_excess": "no charge within the autoclave's limits releases more than its max_heat_rate_W"}[g]))
        for tag, src in zip("abc", world_files()):
            shutil.copyfile(src, os.path.join(GOLD, "chemverse_world_%s.json" % tag))
            arrays = dict((k.split("/", 1)[1], base[k]) for k in base.files if k.startswith(tag + "/"))
            n = len(arrays["num_steps"])
            stable, order_free = arrays["stable"].copy(), np.ones(n, bool)
            for other in runs[1:]:
                o = dict((k.split("/", 1)[1], other[k]) for k in other.files if k.startswith(tag + "/"))
                stable &= discrete_equal(arrays, o)
                for k in FLOATS:
                    d = np.abs(o[k] - arrays[k])
                    arrays["spread_" + k] = np.maximum(arrays["spread_" + k], d)
                    m = min(len(d), n)
                    order_free[:m] &= (o[k].view(np.uint64) == arrays[k].view(np.uint64)).reshape(m, -1).all(axis=1)
            arrays["stable"], arrays["order_free"] = stable, order_free
            unstable = int((~stable).sum())
            if unstable > 0.02 * n:
                raise SystemExit("fixture %s: %d of %d experiments are unstable (more than 2 %%)" % (tag, unstable, n))
            path = os.path.join(GOLD, "chemverse_runs_%s.npz" % tag)
            write_npz(path, arrays)
            print("fixture %s: %s, %d experiments, %d fired, %d unstable, %d depend on the hash seed, %d brentq calls, %d bytes"
                  % (tag, os.path.basename(src), n, int((arrays["fired"].sum(axis=1) > 0).sum()), unstable,
                     int((~order_free).sum()), len(arrays["brent_root"]), os.path.getsize(path)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
