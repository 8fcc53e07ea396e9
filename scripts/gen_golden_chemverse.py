"""Golden fixtures of ChemVerse: the REFERENCE's own simulate_chain_reaction (xenoverse/chemverse/environment/simulator.py) on
three of its evaluation worlds and on two wide worlds, 128 experiments each, and one experiment of 4,096 steps.

Build-container tooling, like scripts/gen_golden_anyhvac.py: the reference is imported read-only through oracle/_refimport.py;
nothing under oracle/ is modified.  Only data is written, under tests/golden/:
  chemverse_world_{a,b,c}.json   three evaluation-world files, copied byte for byte: the one with the fewest reactions, the
                                 middle one and the one with the most (ordered by reactions, chemicals, file name)
  chemverse_runs_{a,b,c}.npz     the experiments, the reference's results, the sensitivity figures, recorded brentq calls and
                                 (first 32 experiments and the hand-made ones) the reference's own rounded result dicts
  chemverse_world_h.json         the to_dict() of the first WorldSampler(seed, "hard") world, seeds from 0, with more than 64
                                 reactions and more than 32 chemicals, sampled under PYTHONHASHSEED=0 (seed 5: 51 and 95)
  chemverse_world_x.json         a world at every table limit, made by make_world_x below from chemverse_world_c.json alone
  chemverse_runs_{h,x}.npz       as above, and branch_hits[n, branch]: which experiment took which branch of the reference.
                                 Their recipe draws 60 % of the target reactions among the indices 64 and up; world x's
                                 hand-made experiments also charge each widened reaction, sealed and under reflux
  chemverse_runs_long.npz        world a's first reaction charged with 200 g per coefficient at 0 C in the sealed flask for
                                 20,480 s: all 4,096 steps fire

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
The script prints a count per branch and stops if a listed branch has none: BRANCHES over a, b and c, WIDE_BRANCHES over h and x.

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
GAPS = ("isothermal_excess",)      # may be unreachable on these worlds; reported with the reason
# the wide fixtures h and x: every one of these needs an experiment in the two together
WIDE_BRANCHES = ("solvent_self", "reaction_index_ge_64_fired", "chemical_index_ge_32_in_pool", "chemical_63_in_pool",
                 "reactants_6", "products_4", "byproducts_2_or_more", "byproducts_4", "catalysts_2_or_more", "catalysts_4",
                 "coeff_4_to_7", "coeff_8", "external_solvent_index_ge_32", "rescaled_with_byproducts")
WIDE_TAGS = ("h", "x")
N_HAND_X = 7                # world x: the all-solvent charge, two per widened reaction, an exothermic one, the long run
WIDE_SHARE = 0.6            # wide fixtures: this share of the target reactions is drawn among the indices >= 64
LONG_STEPS = 4096
WIDE_THERMO = dict(delta_G_kJ=-5.0, delta_H_kJ=-40.0, activation_energy_kJ=45.0, log_A_factor=9.0)


def world_files():
    d = os.path.join(_refimport.REF_ROOT, "xenoverse", "chemverse", "worlds")
    rows = []
    for f in sorted(os.listdir(d)):
        if f.startswith("eval_world_") and f.endswith(".json"):
            w = json.load(open(os.path.join(d, f)))
            rows.append((len(w["reactions"]), len(w["chemicals"]), f))
    rows.sort()
    return [os.path.join(d, rows[i][2]) for i in (0, len(rows) // 2, len(rows) - 1)]


def make_world_x(c):
    """World x, at the table limits, from fixture world c's JSON dict (27 chemicals, 32 reactions) alone:
      chemicals  0..26  world c's own (C001..C027)
                27..36  E001..E010: copies of C001..C010 (the four solvents and six more), lighter and lower-melting
                37..63  D001..D027: a copy of all of world c, heavier and higher-melting; its solvents are 37..40
      reactions  0..31  world c's own;  32..63  the same on the same chemicals with shifted constants
                64..95  world c's reactions on the D copies;  96..127  those with shifted constants, of which the last three are
                replaced: 125 and 126 are widened to 6 reactants, 4 products, 4 byproducts and 4 catalysts with coefficients up
                to 8 and constants that let them fire, 127 has two solvents as its only reactants and makes chemical 63.
    A copy's solubility entries name its own copy's solvents."""
    src = list(c["chemicals"].items())
    chemicals = {}

    def copy_chem(cid, d, letter, mw, dT):
        new = letter + cid[1:]
        e = dict(d, id=new, name=d["name"] + " " + letter, molecular_weight=round(d["molecular_weight"] * mw, 2),
                 melting_point=round(d["melting_point"] + dT, 2), boiling_point=round(d["boiling_point"] + 1.5 * dT, 2))
        if "solubility" in d:
            e["solubility"] = {letter + s[1:]: v for s, v in d["solubility"].items()}
        chemicals[new] = e

    for cid, d in src:
        chemicals[cid] = dict(d)
    for cid, d in src[:10]:
        copy_chem(cid, d, "E", 0.97, -2.0)
    for cid, d in src:
        copy_chem(cid, d, "D", 1.03, 2.0)
    reactions = {}

    def add(r, letter, shifted):
        rid = "R%03d" % (len(reactions) + 1)
        ren = lambda x: letter + x[1:]      # noqa: E731
        e = dict(r, id=rid, reactants=[[ren(x), k] for x, k in r["reactants"]], catalysts=[ren(x) for x in r["catalysts"]],
                 products=[[ren(x), k] for x, k in r["products"]], byproducts=[[ren(x), k] for x, k in r["byproducts"]])
        if shifted:
            e.update(delta_G_kJ=round(r["delta_G_kJ"] + 0.5, 3), activation_energy_kJ=round(r["activation_energy_kJ"] - 3.0, 3))
        reactions[rid] = e

    for letter in "CD":
        for shifted in (False, True):
            for r in c["reactions"].values():
                add(r, letter, shifted)
    # every reactant of the widened ones lists D004 (world c's C004), so one solvent dissolves them all; R126's products and
    # byproducts outweigh its reactants (2,937 g against 2,579 g per mole of extent: rescaled), R127's do not
    reactions["R126"] = dict(id="R126", reactants=[["D006", 1], ["D007", 2], ["D008", 1], ["D009", 1], ["D010", 1], ["D013", 5]],
                             catalysts=["D011", "D015", "D016", "E005"],
                             products=[["D017", 8], ["D018", 1], ["D020", 2], ["D023", 2]],
                             byproducts=[["D014", 1], ["D021", 2], ["E006", 1], ["E007", 3]], **WIDE_THERMO)
    reactions["R127"] = dict(id="R127", reactants=[["D015", 8], ["D016", 1], ["D017", 1], ["D018", 2], ["D019", 1], ["D020", 1]],
                             catalysts=["D006", "D007", "E008", "E009"],
                             products=[["D022", 1], ["D023", 4], ["D026", 1], ["D027", 1]],
                             byproducts=[["D024", 1], ["D025", 1], ["E008", 2], ["E010", 6]], **WIDE_THERMO)
    reactions["R128"] = dict(id="R128", reactants=[["D001", 1], ["D002", 2]], catalysts=[], products=[["D027", 1]],
                             byproducts=[], **WIDE_THERMO)
    world = dict(world_id="limits_world_x",
                 metadata=dict(num_layers=c["metadata"]["num_layers"], seed=c["metadata"]["seed"],
                               num_chemicals=len(chemicals), num_reactions=len(reactions)),
                 chemicals=chemicals, reactions=reactions, cost_params=c["cost_params"], equipment=c["equipment"])
    assert len(chemicals) == 64 and len(reactions) == 128 and list(chemicals)[63] == "D027"
    return world


def widened(world):
    """the reactions at all four per-reaction limits"""
    return [r for r in world.reactions.values()
            if (len(r.reactants), len(r.products), len(r.byproducts), len(r.catalysts)) == (6, 4, 4, 4)]


def make_experiments(world, rs, simulate, wide=False, n_hand=N_HAND):
    chems, rxns = world.chemicals, list(world.reactions.values())
    equip = list(world.equipment.keys())
    exps = []

    def charge(amounts, rxn, base):
        for cid, k in rxn.reactants:
            amounts[cid] = amounts.get(cid, 0.0) + base * k * rs.uniform(0.5, 1.5)
        for cid in rxn.catalysts:
            amounts[cid] = amounts.get(cid, 0.0) + base * rs.uniform(0.02, 0.3)

    def solvents_for(r):
        non_solv = [c for c, _ in r.reactants if not chems[c].is_solvent]
        return [s for s, c in chems.items() if c.is_solvent and all(s in chems[x].solubility for x in non_solv)]

    targets = []
    for _ in range(N_EXP - n_hand):
        if wide and rs.uniform() < WIDE_SHARE:      # a wide fixture: most targets among the reactions 64 and up
            k = 64 + rs.randint(len(rxns) - 64)
        else:
            k = rs.randint(len(rxns))
        targets.append(k)
        rxn = rxns[k]
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
    if wide:      # every widened reaction: its reactants, catalysts and a solvent for all of them, sealed and open
        for r in widened(world):
            for eq, temp, g in (("sealed_flask", 60.0, 20.0), ("reflux_condenser", 95.0, 6.0)):
                a = {}
                for cid, k in r.reactants:
                    a[cid] = g * k
                for cid in r.catalysts:
                    a[cid] = 2.0
                s = solvents_for(r)[0]
                a[s] = a.get(s, 0.0) + 300.0
                hand.append(dict(amounts=a, temperature_C=temp, pressure_atm=1.0, duration_s=60.0, equipment=eq,
                                 heating_rate_C_per_s=0.0, vessel_volume_L=1.0))
        if sum(k >= 64 for k in targets) * 2 < N_EXP:
            raise SystemExit("fewer than half of the experiments target a reaction with index >= 64")
    for r, temp in zip(hot * 2, (220.0, 320.0, 150.0)):
        if len(hand) >= n_hand - 1:
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
    hand = hand[:n_hand - 1]
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
    while len(hand) < n_hand - 1:      # a world without some hand-made case: the long run's charge at other durations
        hand.append(dict(long_run, duration_s=(45.0, 90.0, 135.0)[len(hand) % 3]))
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
    n_log = min(n, N_LOG)
    a = dict(final_pool=np.zeros((n, C)), consumed=np.zeros((n, C)), produced=np.zeros((n, C)), byproduct=np.zeros((n, C)),
             gas_lost=np.zeros((n, C)), fired=np.zeros((n, R), np.int32), num_steps=np.zeros(n, np.int32),
             steps_run=np.array(steps_run, np.int32), converged=np.zeros(n, np.uint8), failure=np.zeros(n, np.uint8),
             failure_step=np.full(n, -1, np.int32), final_T=np.zeros(n), final_P=np.zeros(n),
             hist_step=np.zeros((n, HISTORY_MAX), np.int32), hist_T=np.zeros((n, HISTORY_MAX)), hist_P=np.zeros((n, HISTORY_MAX)),
             hist_count=np.zeros(n, np.int32), log_step=np.zeros((n_log, LOG_MAX), np.int32),
             log_active=np.zeros((n_log, LOG_MAX), np.int32), log_T=np.zeros((n_log, LOG_MAX)), log_P=np.zeros((n_log, LOG_MAX)),
             log_consumed=np.zeros((n_log, LOG_MAX, C)), log_produced=np.zeros((n_log, LOG_MAX, C)),
             log_count=np.zeros(n_log, np.int32))
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
        if i < n_log:
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


def sample_world_h(out_path):
    """the first WorldSampler(seed, "hard") world, seeds from 0, with more than 64 reactions and more than 32 chemicals, as its
    to_dict() JSON.  The sampler iterates sets of id strings while it draws, so the world is that of PYTHONHASHSEED=0."""
    _refimport.setup()
    from xenoverse.chemverse.world_gen.sampler import WorldSampler
    for seed in range(1000):
        world = WorldSampler(seed, complexity_level="hard").sample_world("hard_world_%d" % seed)
        if len(world.reactions) > 64 and len(world.chemicals) > 32:
            break
    else:
        raise SystemExit("no hard world with more than 64 reactions and 32 chemicals among 1000 seeds")
    print("fixture h: WorldSampler seed %d, %d chemicals, %d reactions" % (seed, len(world.chemicals), len(world.reactions)))
    with open(out_path, "w") as f:
        json.dump(world.to_dict(), f, indent=2)


def long_experiment(world):
    """world a's first reaction charged at 200 g per coefficient, cold and sealed, for 4,096 steps of 5 s"""
    rxn = list(world.reactions.values())[0]
    return dict(amounts={cid: 200.0 * k for cid, k in rxn.reactants}, temperature_C=0.0, pressure_atm=1.0,
                duration_s=5.0 * LONG_STEPS, equipment="sealed_flask", heating_rate_C_per_s=0.0, vessel_volume_L=1.0)


def worker(out_path, full, worlds_dir):
    _refimport.setup()
    from xenoverse.chemverse.environment import simulator as sim
    from xenoverse.chemverse.world_gen.models import World
    import scipy.optimize as so
    real_brentq = so.brentq
    counts = dict((g, dict((b, 0) for b in BRANCHES + GAPS + WIDE_BRANCHES)) for g in ("abc", "wide", "long"))
    blob = {}
    jobs = list(zip("abc", world_files())) + [(t, os.path.join(worlds_dir, "%s.json" % t)) for t in WIDE_TAGS]
    jobs.append(("long", world_files()[0]))
    for tag, path in jobs:
        world = World.load(path)
        wide, group = tag in WIDE_TAGS, ("wide" if tag in WIDE_TAGS else "long" if tag == "long" else "abc")
        n_hand = 1 if tag == "long" else N_HAND_X if tag == "x" else N_HAND
        if tag == "long":
            exps = [long_experiment(world)]
        else:
            exps = make_experiments(world, np.random.RandomState(SEED + ord(tag)), sim.simulate_chain_reaction, wide=wide,
                                    n_hand=n_hand)
        chems = world.chemicals
        cpos = {c: i for i, c in enumerate(chems)}
        rpos = {r: i for i, r in enumerate(world.reactions)}
        hits = []      # per experiment: the branches it took
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
                    if 4 <= k <= 7:
                        ev.add("coeff_4_to_7")
                if rpos[rxn.id] >= 64:
                    ev.add("reaction_index_ge_64_fired")
                if len(rxn.products) == 4:
                    ev.add("products_4")
                byp = [(b, k) for b, k in rxn.byproducts if b in chemicals and res[2].get(b, 0.0) > 1e-12]
                if len(byp) >= 2:
                    ev.add("byproducts_2_or_more")
                if len(byp) == 4:
                    ev.add("byproducts_4")
                if len(rxn.catalysts) >= 2:
                    ev.add("catalysts_2_or_more")
                if len(rxn.catalysts) == 4:
                    ev.add("catalysts_4")
                if solvent_id in cpos and solvent_id not in ids and cpos[solvent_id] >= 32:
                    ev.add("external_solvent_index_ge_32")
                if len(byp) >= 2 and rxn.delta_H_kJ != 0:      # the extent from the heat; the amounts before the rescaling
                    xi = res[4] / (-rxn.delta_H_kJ * 1000.0)
                    made = (sum(k * xi * chemicals[p].molecular_weight for p, k in rxn.products) +
                            sum(k * xi * chemicals[b].molecular_weight * 0.1 for b, k in rxn.byproducts if b in chemicals))
                    used = sum(res[0].values())
                    if made > used * (1.0 + 1e-9) and used > 1e-12:
                        ev.add("rescaled_with_byproducts")
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
                    held = [cpos[c] for c in list(e["amounts"]) + list(r["final_pool_g"]) if c in cpos]
                    if held and max(held) >= 32:
                        ev.add("chemical_index_ge_32_in_pool")
                    if 63 in held:
                        ev.add("chemical_63_in_pool")
                    for b in ev:
                        if b in counts[group]:
                            counts[group][b] += 1
                    hits.append(sorted(ev))
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
                keep = list(range(min(N_LOG, n))) + list(range(max(N_LOG, len(exps) - n_hand), len(exps)))
                keep += [i for i in range(N_LOG, len(exps) - n_hand) if base["failure"][i]][:12]
                text = json.dumps([[i, rounded[i]] for i in keep])
                blob[tag + "/dicts_json"] = np.frombuffer(text.encode(), np.uint8)
                if group != "abc":      # which experiment took which branch, for the tests that assert the coverage
                    names = BRANCHES + GAPS + WIDE_BRANCHES
                    blob[tag + "/branch_names_json"] = np.frombuffer(json.dumps(names).encode(), np.uint8)
                    blob[tag + "/branch_hits"] = np.array([[b in h for b in names] for h in hits], bool)
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
    if len(sys.argv) == 5 and sys.argv[1] == "--worker":
        return worker(sys.argv[2], sys.argv[3] == "full", sys.argv[4])
    if len(sys.argv) == 3 and sys.argv[1] == "--sample-h":
        return sample_world_h(sys.argv[2])
    if not _refimport.available():
        raise SystemExit("the reference tree is not present: fixtures are generated in the build container only")
    tmp = tempfile.mkdtemp(prefix="chemverse_golden_")
    try:
        # the wide worlds, as the JSON files every worker loads: h sampled by the reference, x made here from world c
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--sample-h", os.path.join(tmp, "h.json")],
                              env=dict(os.environ, PYTHONHASHSEED="0"))
        with open(os.path.join(GOLD, "chemverse_world_c.json")) as f:
            world_c = json.load(f)
        with open(os.path.join(tmp, "x.json"), "w") as f:
            json.dump(make_world_x(world_c), f, indent=1)
        runs = []
        for hs in HASH_SEEDS:
            out = os.path.join(tmp, "h%d.npz" % hs)
            env = dict(os.environ, PYTHONHASHSEED=str(hs))
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--worker", out, "full" if hs == 0 else "base",
                                   tmp], env=env)
            runs.append(np.load(out))
        base = runs[0]
        counts = json.loads(bytes(base["counts_json"]).decode())
        print("branch counts over the three fixtures (experiments that took the branch):")
        for b in BRANCHES + GAPS:
            print("  %-26s %d" % (b, counts["abc"][b]))
        missing = [b for b in BRANCHES if not counts["abc"][b]]
        if missing:
            raise SystemExit("the fixtures do not reach: %s" % ", ".join(missing))
        for g in GAPS:
            if not counts["abc"][g] and not counts["wide"][g]:
                print("not reached on these worlds: %s (%s)" % (g, {
                    "isothermal_excess": "no charge within the autoclave's limits releases more than its max_heat_rate_W"}[g]))
        print("branch counts over the wide fixtures h and x:")
        for b in WIDE_BRANCHES + BRANCHES + GAPS:
            print("  %-30s %d" % (b, counts["wide"][b]))
        missing = [b for b in WIDE_BRANCHES if not counts["wide"][b]]
        if missing:
            raise SystemExit("the wide fixtures do not reach: %s" % ", ".join(missing))
        sources = list(zip("abc", world_files())) + [(t, os.path.join(tmp, "%s.json" % t)) for t in WIDE_TAGS]
        for tag, src in sources + [("long", world_files()[0])]:
            if tag != "long":
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
            # 4,096 steps are sampled every 204th: steps 0..4 and 204, 408 .. 4080 make 25 history entries, not HISTORY_MAX
            if tag == "long" and (arrays["steps_run"][0] != LONG_STEPS or arrays["hist_count"][0] != 25 or
                                  arrays["log_count"][0] != LOG_MAX):
                raise SystemExit("the long experiment ran %d steps, %d history and %d log entries"
                                 % (arrays["steps_run"][0], arrays["hist_count"][0], arrays["log_count"][0]))
            path = os.path.join(GOLD, "chemverse_runs_%s.npz" % tag)
            write_npz(path, arrays)
            print("fixture %s: %s, %d experiments, %d fired, %d unstable, %d depend on the hash seed, %d brentq calls, %d bytes"
                  % (tag, os.path.basename(src), n, int((arrays["fired"].sum(axis=1) > 0).sum()), unstable,
                     int((~order_free).sum()), len(arrays["brent_root"]), os.path.getsize(path)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
