"""ChemVerse's ground-truth cost oracle, restated on the host: the reference's ChemistryEnvironment.compute_optimal_cost
(xenoverse/chemverse/environment/api.py:1777-2266) with _find_reaction_chains (:957), _optimal_temp_for_reaction (:992),
_max_solvent_bp_for_reaction (:1029) and the parts of environment/cost_model.py it calls, over the tables of tables.py and
host.simulate_one.  Plain Python, operation for operation: math.log / math.exp, `**`, the builtin sum and Python's round are
the reference's own.  This file is the specification of csrc/chemverse_optimal.hip and what backend="host" runs.

How the work is cut, so that the device can take the middle of it:
  * a PLAN is one candidate in the form the kernel reads: steps of (temperature, duration, charge entries), the equipment,
    the target, which yield counts (the virtual pool's or the last experiment's final pool) and the bisection's range and
    length.  chain_plan makes one from a route, one_pot_plans the (charge, temperature) candidates of a target.
  * run_plan is _simulate_chain's simulation half (:1967-1995, :2067-2074): it charges, simulates and carries the virtual
    pool, and returns the ROWS of one pass: per step the charged grams and the consumed / produced / byproduct totals.
    bisect_plan is the search around it (:1918-1937, :2182-2217).
  * finish_chain / finish_one_pot price one pass from its rows (:2004-2065, :2097-2109; :2229-2264) — the same code for
    rows from run_plan and rows from the device.

Where the reference has no defined order, this file fixes one:
  * _compute_one_pot_cost builds its charge by iterating Python sets of id strings (m1_reactants, catalysts,
    needed_solvents), so the pool's insertion order follows the process's string-hash seed.  Here each of the three groups
    is charged in ascending chemical index.
  * _simulate_chain sums the purification cost over produced_g / byproduct_g in the order the simulator first produced each
    species, and compute_purification_cost over the pool's insertion order; the rows keep no such order, the sums here run
    in ascending chemical index.  With two or more observed species a sum can differ in its last bit before it is rounded
    to two or four decimals.
"""
import math

import numpy as np

from . import tables as T
from .host import R_kJ, _world, simulate_one

DETECTION_THRESHOLD_G = 0.001                   # api.py:260
KIND_SCALE, KIND_TENTH, KIND_FIVE, KIND_POOL = range(4)      # a charge entry: scale, 0.1 scale, 5 scale, max(virtual pool, 0.01)
MODE_VIRTUAL_POOL, MODE_FINAL_POOL = 0, 1
CHAIN_ITERS, CHAIN_LO, CHAIN_HI = 30, 0.1, 1000.0           # :1918-1921
ONE_POT_ITERS, ONE_POT_LO, ONE_POT_HI = 12, 0.5, 200.0       # :2182-2184
BIT_PROBE = 31                                  # the decision bit of the pass at scale_hi
PHASE_NAMES = ("solid", "liquid", "gas")
STEP_SECONDS = 5.0


def chem_index(tab, c):
    if isinstance(c, (int, np.integer)):
        if not 0 <= int(c) < tab["C"]:
            raise ValueError("chemical index %d is outside [0, %d)" % (int(c), tab["C"]))
        return int(c)
    pos = tab.get("_chem_pos")
    if pos is None:
        pos = tab["_chem_pos"] = {k: i for i, k in enumerate(tab["chem_ids"])}
    if c not in pos:
        raise ValueError("%r is not a chemical of this world" % (c,))
    return pos[c]


def rxn_index(tab, r):
    if isinstance(r, (int, np.integer)):
        if not 0 <= int(r) < tab["R"]:
            raise ValueError("reaction index %d is outside [0, %d)" % (int(r), tab["R"]))
        return int(r)
    pos = tab.get("_rxn_pos")
    if pos is None:
        pos = tab["_rxn_pos"] = {k: i for i, k in enumerate(tab["rxn_ids"])}
    if r not in pos:
        raise ValueError("%r is not a reaction of this world" % (r,))
    return pos[r]


def _finite(**kw):
    for k, v in kw.items():
        if not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
            raise ValueError("%s must be a finite number, got %r" % (k, v))


def find_reaction_chains(tab, target, max_routes=5, max_steps=4):
    """_find_reaction_chains :957-990: backward depth-first search from the target -> routes as lists of reaction indices in
    forward order, the reference's routes in the reference's order"""
    w = _world(tab)
    layer = tab["layer"].tolist()
    target = chem_index(tab, target)
    produces = {}
    for r, rxn in enumerate(w.rxn):
        for p, _ in rxn["products"]:
            produces.setdefault(p, []).append(r)
    chains = []

    def dfs(needed, chain_rev, used):
        if len(chains) >= max_routes:
            return
        non_m1 = [c for c in needed if layer[c] > 1]
        if not non_m1:
            chains.append(list(chain_rev))
            return
        if len(chain_rev) >= max_steps:
            return
        resolve = non_m1[0]
        remaining = [c for c in needed if c != resolve]
        for r in produces.get(resolve, []):
            if r in used:
                continue
            new_needed = list(dict.fromkeys(remaining + [c for c, _ in w.rxn[r]["reactants"]]))
            dfs(new_needed, chain_rev + [r], used | {r})

    dfs([target], [], frozenset())
    return [list(reversed(ch)) for ch in chains]


def _max_solvent_bp(tab, w, rxn):      # :1029-1062
    reactants = [c for c, _ in rxn["reactants"]]
    non_solvent = [c for c in reactants if not w.is_solvent[c]]
    if not non_solvent:
        return 600.0
    best_bp = -273.0
    for s in [c for c in reactants if w.is_solvent[c]]:
        if all(w.sol_present[c, s] for c in non_solvent):
            best_bp = max(best_bp, w.bp[s])
    for s in range(w.C):
        if not w.is_solvent[s] or s in reactants:
            continue
        if all(w.sol_present[c, s] for c in non_solvent):
            best_bp = max(best_bp, w.bp[s])
    return best_bp if best_bp > -273.0 else 600.0


def optimal_conditions(tab):
    """_optimal_temp_for_reaction :992-1027 for every reaction -> (T_C, duration_s), two lists of Python floats.  Host only:
    the values are rounded with Python's round(., 1) and are inputs of the device."""
    got = tab.get("_optimal_conditions")
    if got is not None:
        return got
    w = _world(tab)
    temps, durs = [], []
    for rxn in w.rxn:
        A = 10.0 ** rxn["logA"]
        target_k = 0.01
        ratio = A / max(target_k, 1e-30)
        if ratio <= 1.0:
            T_K = 298.15
        else:
            T_K = rxn["Ea"] / (R_kJ * math.log(ratio))
        T_K = max(298.15, min(873.15, T_K))
        max_solvent_bp_C = _max_solvent_bp(tab, w, rxn)
        T_C = T_K - 273.15
        if T_C > max_solvent_bp_C - 5.0:
            T_C = max_solvent_bp_C - 5.0
        min_reactant_bp = min((w.bp[c] for c, _ in rxn["reactants"]), default=9999.0)
        if T_C > min_reactant_bp - 5.0:
            T_C = min_reactant_bp - 5.0
        T_C = max(25.0, T_C)
        T_K = T_C + 273.15
        k_at_T = A * math.exp(-rxn["Ea"] / (R_kJ * T_K))
        duration_s = min(3600.0, max(60.0, 3.0 / max(k_at_T, 1e-30)))
        temps.append(round(T_C, 1))
        durs.append(round(duration_s, 1))
    tab["_optimal_conditions"] = (temps, durs)
    return temps, durs


def yield_threshold(min_yield_g):
    """the smallest double y >= 0 with round(y, 6) >= min_yield_g: the device compares the unrounded yield with it where the
    reference compares the rounded one (:1924).  Found on the ordered doubles with Python's own round: a bisection on the
    bit patterns, then stepped to the boundary and checked there."""
    m = float(min_yield_g)
    _finite(min_yield_g=m)

    def passes(y):
        return round(y, 6) >= m

    if passes(0.0):
        return 0.0
    to_bits = lambda y: int(np.float64(y).view(np.int64))      # noqa: E731: monotone on the non-negative doubles
    to_float = lambda b: float(np.int64(b).view(np.float64))   # noqa: E731
    lo, hi = 0, to_bits(m + 1e-6 + abs(m) * 1e-9)
    if not passes(to_float(hi)):
        raise ValueError("min_yield_g = %r is beyond what round(., 6) can reach" % (m,))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if passes(to_float(mid)):
            hi = mid
        else:
            lo = mid
    y = to_float(hi)
    while passes(math.nextafter(y, -math.inf)):      # round is monotone; the steps are a check that costs nothing
        y = math.nextafter(y, -math.inf)
    return y


# ---- plans -----------------------------------------------------------------------------------------------------------------

def chain_plan(tab, chain, target, conditions=None):
    """a route (reaction indices or ids, forward order) as a plan: _simulate_chain's charges (:1968-1990) — a layer-1
    reactant `scale`, a layer-1 catalyst 0.1 scale, anything else max(virtual pool, 0.01); reactants, then catalysts — at the
    reactions' optimal conditions, in the autoclave.  conditions: {step: (T_C, duration_s)} overrides."""
    w = _world(tab)
    chain = [rxn_index(tab, r) for r in chain]
    if len(chain) > T.CHAIN_MAX:
        raise T._unsupported("reactions per route", len(chain), "CHAIN_MAX", T.CHAIN_MAX)
    if not chain:
        raise ValueError("a route needs at least one reaction")
    layer = tab["layer"]
    temps, durs = optimal_conditions(tab)
    steps = []
    for s, r in enumerate(chain):
        rxn = w.rxn[r]
        entries = [(c, KIND_SCALE if layer[c] == 1 else KIND_POOL) for c, _ in rxn["reactants"]]
        entries += [(c, KIND_TENTH if layer[c] == 1 else KIND_POOL) for c in rxn["catalysts"]]
        T_C, dur = (conditions or {}).get(s, (temps[r], durs[r]))
        _finite(temperature_C=T_C, duration_s=dur)
        if not dur > 0 or not -273.15 <= T_C <= 5000.0:
            raise ValueError("step %d: duration_s must be positive and temperature_C within [-273.15, 5000], got (%r, %r)"
                             % (s, T_C, dur))
        T.num_steps_of(dur, STEP_SECONDS)      # refuses more than STEPS_MAX steps
        steps.append(dict(rxn=r, n_reactants=len(rxn["reactants"]), T=float(T_C), dur=float(dur), entries=entries))
    return dict(kind="chain", steps=steps, equipment=T.equipment_index(tab, "autoclave"), target=chem_index(tab, target),
                mode=MODE_VIRTUAL_POOL, lo=CHAIN_LO, hi=CHAIN_HI, n_iter=CHAIN_ITERS)


def one_pot_plans(tab, target, max_time_seconds):
    """_compute_one_pot_cost :2129-2181: the (charge, temperature) candidates of a target, in the reference's order; [] where
    it returns None before simulating"""
    w = _world(tab)
    layer = tab["layer"]
    target = chem_index(tab, target)
    chains = find_reaction_chains(tab, target, max_routes=5, max_steps=6)
    configs = []
    for chain in chains:
        m1, cats = set(), set()
        for r in chain:
            m1.update(c for c, _ in w.rxn[r]["reactants"] if layer[c] == 1)
            cats.update(c for c in w.rxn[r]["catalysts"] if layer[c] == 1)
        if m1:
            configs.append((sorted(m1), sorted(cats), chain))
    solvents = set()
    for _, _, chain in configs:      # :2154-2167: per reaction, the first solvent every non-solvent reactant lists
        for r in chain:
            non_solvent = [c for c, _ in w.rxn[r]["reactants"] if not w.is_solvent[c]]
            for s in range(w.C):
                if w.is_solvent[s] and all(w.sol_present[c, s] for c in non_solvent):
                    solvents.add(s)
                    break
    temps, _ = optimal_conditions(tab)
    dur = 300.0
    if dur > max_time_seconds:
        dur = max_time_seconds
    plans = []
    for m1, cats, chain in configs:
        entries = [(c, KIND_SCALE) for c in m1] + [(c, KIND_TENTH) for c in cats] + [(c, KIND_FIVE) for c in sorted(solvents)]
        for T_C in sorted(set(temps[r] for r in chain) | {150.0})[:3]:
            plans.append(dict(kind="one_pot", steps=[dict(rxn=chain[0], n_reactants=0, T=float(T_C), dur=float(dur),
                                                          entries=entries)],
                              equipment=T.equipment_index(tab, "sealed_flask"), target=target, mode=MODE_FINAL_POOL,
                              lo=ONE_POT_LO, hi=ONE_POT_HI, n_iter=ONE_POT_ITERS))
    return plans


def plan_widths(plans):
    """-> (steps, charge entries) of the longest plan"""
    return (max(len(p["steps"]) for p in plans), max(1, max(len(s["entries"]) for p in plans for s in p["steps"])))


# ---- one pass and the search ----------------------------------------------------------------------------------------------------

def _update_virtual_pool(vpool, consumed, produced, byproduct):      # :2067-2074, over the result dict's > 1e-9 entries
    for c in np.nonzero(consumed > 1e-9)[0].tolist():
        vpool[c] = max(0.0, vpool.get(c, 0.0) - float(consumed[c]))
    for row in (produced, byproduct):
        for c in np.nonzero(row > 1e-9)[0].tolist():
            if row[c] >= DETECTION_THRESHOLD_G:
                vpool[c] = vpool.get(c, 0.0) + float(row[c])


def run_plan(tab, plan, scale):
    """one pass of a plan at one scale -> its rows: charged [steps][entries], consumed / produced / byproduct [steps][C]
    (unfiltered totals as simulate_one reports them), failure [steps], final_pool [C] of the last step, and `yield`"""
    C = tab["C"]
    n = len(plan["steps"])
    k = max(1, max(len(s["entries"]) for s in plan["steps"]))
    rows = dict(charged=np.zeros((n, k)), consumed=np.zeros((n, C)), produced=np.zeros((n, C)), byproduct=np.zeros((n, C)),
                failure=np.zeros(n, np.uint8), final_pool=np.zeros(C))
    vpool = {}
    for s, step in enumerate(plan["steps"]):
        amounts = {}
        for j, (c, kind) in enumerate(step["entries"]):
            g = (scale if kind == KIND_SCALE else scale * 0.1 if kind == KIND_TENTH else scale * 5.0 if kind == KIND_FIVE
                 else max(vpool.get(c, 0.0), 0.01))
            rows["charged"][s, j] = g
            amounts[c] = amounts[c] + g if c in amounts else g
        sim = simulate_one(tab, list(amounts.items()), step["T"], 1.0, step["dur"], plan["equipment"],
                           step_seconds=STEP_SECONDS)
        for key in ("consumed", "produced", "byproduct"):
            rows[key][s] = sim[key]
        rows["failure"][s] = sim["failure"]
        rows["final_pool"] = sim["final_pool"]
        _update_virtual_pool(vpool, sim["consumed"], sim["produced"], sim["byproduct"])
    rows["yield"] = (vpool.get(plan["target"], 0.0) if plan["mode"] == MODE_VIRTUAL_POOL
                     else float(rows["final_pool"][plan["target"]]))
    return rows


def bisect_plan(tab, plan, passes):
    """_compute_chain_cost :1918-1937 / _compute_one_pot_cost :2182-2227: passes(yield) -> bool is the comparison.
    -> dict(found, best_scale, bits, rows): rows of the pass at best_scale, None when nothing passed"""
    lo, hi = plan["lo"], plan["hi"]
    best, bits = None, 0
    for it in range(plan["n_iter"]):
        mid = (lo + hi) / 2.0
        if passes(run_plan(tab, plan, mid)["yield"]):
            best, hi = mid, mid
            bits |= 1 << it
        else:
            lo = mid
    if best is None and passes(run_plan(tab, plan, hi)["yield"]):
        best = hi
        bits |= 1 << BIT_PROBE
    if best is None:
        return dict(found=False, best_scale=0.0, bits=bits, rows=None)
    return dict(found=True, best_scale=best, bits=bits, rows=run_plan(tab, plan, best))


# ---- pricing a pass from its rows (environment/cost_model.py) ---------------------------------------------------------------------

def _round_sig(value, sig=4):      # api.py:12-18
    if value == 0:
        return 0.0
    digits = sig - int(math.floor(math.log10(abs(value)))) - 1
    return round(value, max(digits, 0))


def _phase_separation_factor(phases):      # cost_model.py:11-28, phases: a set of "solid" / "liquid" / "gas"
    if not phases:
        return 1.0
    if len(phases) == 1:
        phase = next(iter(phases))
        return 0.4 if phase == "solid" else 1.0 if phase == "liquid" else 1.8
    if len(phases) == 3:
        return 3.0
    if "gas" in phases and "liquid" in phases:
        return 2.2
    if "gas" in phases and "solid" in phases:
        return 2.0
    return 0.7


def _purification_cost_per_component(grams, n_components, phase_factor):      # cost_model.py:31-40
    if n_components <= 1:
        return 0.0
    complexity = 1.0 + 0.5 * (n_components - 2) ** 1.3
    base_rate = 6.0
    return base_rate * complexity * phase_factor * grams ** 0.7


def _phase(w, c, T_C, P):
    return PHASE_NAMES[w.state_at(c, T_C, P)]


def process_costs(tab, rxn, amounts, T_C, P, duration_s, equipment=None):
    """calculate_cost :150-224 -> (energy_cost, duration_cost, equipment_cost), each rounded to two decimals as its result
    dict has them.  amounts: [(chemical, grams)] in dict order; rxn: the reaction whose products' toxicities count."""
    w = _world(tab)
    cp = tab["cost_params"]
    total_mass = sum(g for _, g in amounts)
    T_dev = abs(T_C - 25.0)
    if T_C < 25.0:
        energy_temp = cp["cooling_coeff"] * (T_dev / 100.0) ** cp["cooling_exponent"]
    else:
        energy_temp = cp["heating_coeff"] * (T_dev / 100.0) ** cp["heating_exponent"]
    if P < 1.0:
        energy_pressure = cp["pressure_low_coeff"] * (1.0 - P) ** cp["pressure_low_exp"]
    else:
        energy_pressure = cp["pressure_high_coeff"] * (P - 1.0) ** cp["pressure_high_exp"]
    energy_cost = (energy_temp + energy_pressure + 0.1) * total_mass
    duration_cost = cp["duration_coeff"] * (duration_s / 3600.0) * total_mass ** 0.5
    tox = tab["base_toxicity"].tolist()
    all_tox = [tox[c] for c, _ in amounts] + [tox[p] for p, _ in w.rxn[rxn]["products"]]
    max_toxicity = min(10.0, max(all_tox) / 2.0) if all_tox else 0.0
    toxicity_premium = 1.0 + 0.15 * max_toxicity
    e = T.equipment_index(tab, equipment)
    hours = duration_s / 3600.0
    base = float(tab["base_cost_per_hour"][e]) * hours
    equip_cost = base * total_mass ** 0.6 * float(tab["cost_multiplier"][e])
    equip_cost *= toxicity_premium
    return round(energy_cost, 2), round(duration_cost, 2), round(equip_cost, 2)


def _above(row):
    """a row of totals as the simulator's result dict lists it: {chemical: grams} above 1e-9"""
    return {c: float(row[c]) for c in np.nonzero(row > 1e-9)[0].tolist()}


def finish_chain(tab, plan, scale, rows):
    """_simulate_chain's pricing half and its result dict (:2004-2065, :2076-2109) from one pass's rows"""
    w = _world(tab)
    layer, price, names = tab["layer"], tab["price_per_gram"].tolist(), tab["chem_names"]
    vpool = {}
    purchase = process = purification = total_time = 0.0
    details = []
    for s, step in enumerate(plan["steps"]):
        T_C, dur, nr = step["T"], step["dur"], step["n_reactants"]
        charged = [(c, float(rows["charged"][s, j])) for j, (c, _) in enumerate(step["entries"])]
        reactants, catalysts = charged[:nr], charged[nr:]
        consumed, produced, byproduct = _above(rows["consumed"][s]), _above(rows["produced"][s]), _above(rows["byproduct"][s])
        for c, amt in reactants + catalysts:
            if layer[c] == 1:
                purchase += price[c] * amt
        energy, duration, equipment = process_costs(tab, step["rxn"], reactants, T_C, 1.0, dur, equipment=None)
        process_cost = energy + duration + equipment
        process += process_cost
        total_time += dur
        leftover = {}
        for c, original in reactants:
            left = original - consumed.get(c, 0.0)
            if left > DETECTION_THRESHOLD_G:
                leftover[c] = left
        for c, g in catalysts:
            if g > DETECTION_THRESHOLD_G:
                leftover[c] = g
        seen_p = {c: g for c, g in produced.items() if g >= DETECTION_THRESHOLD_G}
        seen_b = {c: g for c, g in byproduct.items() if g >= DETECTION_THRESHOLD_G}
        components = len(leftover) + len(seen_p) + len(seen_b)
        step_purification = 0.0
        if components > 1:
            phases = set(_phase(w, c, T_C, 1.0) for c in list(seen_p) + list(seen_b) + list(leftover))
            factor = _phase_separation_factor(phases)
            for g in seen_p.values():
                step_purification += _purification_cost_per_component(g, components, factor)
            for g in seen_b.values():
                step_purification += _purification_cost_per_component(g, components, factor)
        purification += step_purification
        _update_virtual_pool(vpool, rows["consumed"][s], rows["produced"][s], rows["byproduct"][s])
        details.append({
            "reaction_id": tab["rxn_ids"][step["rxn"]],
            "reactants_g": {names[c]: _round_sig(g) for c, g in reactants},
            "catalysts_g": {names[c]: _round_sig(g) for c, g in catalysts} if catalysts else {},
            "temperature_C": T_C,
            "duration_s": dur,
            "conversion": round(0.0, 4),      # the simulator's dict has no total_conversion (:2000)
            "products_g": {names[c]: _round_sig(g) for c, g in seen_p.items()},
            "purification_cost": round(step_purification, 2),
            "process_cost": round(process_cost, 2),
        })
    target_yield = vpool.get(plan["target"], 0.0)
    total_cost = purchase + process + purification
    return {"target_yield_g": round(target_yield, 6), "total_cost": round(total_cost, 4), "purchase_cost": round(purchase, 4),
            "process_cost": round(process, 4), "purification_cost": round(purification, 4), "total_time": round(total_time, 1),
            "m1_scale_g": round(scale, 4), "steps": details}


def chain_result(tab, plan, solved, max_time_seconds):
    """_compute_chain_cost's answer (:1930-1942) from a solved plan: the result dict, or None — nothing passed, or over the
    time budget by more than its 5 % allowance"""
    if not solved["found"]:
        return None
    result = finish_chain(tab, plan, solved["best_scale"], solved["rows"])
    if result["total_time"] > max_time_seconds:
        return result if result["total_time"] <= max_time_seconds * 1.05 else None
    return result


def finish_one_pot(tab, plan, scale, rows):
    """:2219-2264 from the rows of the pass at best_scale -> (the unrounded total the search compares, the result dict)"""
    w = _world(tab)
    step = plan["steps"][0]
    T_C, dur = step["T"], step["dur"]
    amounts = {}
    for j, (c, _) in enumerate(step["entries"]):
        g = float(rows["charged"][0, j])
        amounts[c] = amounts.get(c, 0) + g
    price = tab["price_per_gram"].tolist()
    purchase_cost = sum(price[c] * g for c, g in amounts.items())
    energy, duration, equipment = process_costs(tab, step["rxn"], list(amounts.items()), T_C, 1.0, dur, equipment="sealed_flask")
    process_cost = energy + duration + equipment
    pool = _above(rows["final_pool"])
    visible = {c: g for c, g in pool.items() if g >= DETECTION_THRESHOLD_G}      # compute_purification_cost :43-62
    purif_cost = 0.0
    if len(visible) > 1:
        factor = _phase_separation_factor(set(_phase(w, c, T_C, 1.0) for c in visible))
        total = 0.0
        for g in visible.values():
            total += _purification_cost_per_component(g, len(visible), factor)
        purif_cost = round(total, 2)
    total_cost = purchase_cost + process_cost + purif_cost
    return total_cost, {"total_cost": round(total_cost, 4), "purchase_cost": round(purchase_cost, 4),
                        "process_cost": round(process_cost, 4), "purification_cost": round(purif_cost, 4), "total_time": dur,
                        "temperature_C": T_C, "m1_scale_g": round(scale, 4),
                        "target_yield_g": round(pool.get(plan["target"], 0.0), 6), "strategy": "one_pot"}


def one_pot_result(tab, plans, solved):
    """the cheapest of a target's one-pot candidates, strict `<` in the reference's order, against the rounded total of the
    best so far as the reference does (:2253); None when none passed"""
    best = None
    for plan, sol in zip(plans, solved):
        if not sol["found"]:
            continue
        total_cost, result = finish_one_pot(tab, plan, sol["best_scale"], sol["rows"])
        if best is None or total_cost < best["total_cost"]:
            best = result
    return best


# ---- the host backend ---------------------------------------------------------------------------------------------------------

def simulate_chain_host(tab, chain, target, scale):
    """_simulate_chain :1944-2109 -> its result dict"""
    plan = chain_plan(tab, chain, target)
    return finish_chain(tab, plan, scale, run_plan(tab, plan, scale))


def solve_plans_host(tabs, worlds, plans, min_yields):
    """every plan's search on the host.  min_yields[i]: the reference's comparison is round(yield, 6) >= min_yield_g for a
    route (:1924) and final_pool >= min_yield_g, unrounded, for a one-pot candidate (:2197)."""
    out = []
    for w, plan, m in zip(worlds, plans, min_yields):
        if plan["mode"] == MODE_VIRTUAL_POOL:
            out.append(bisect_plan(tabs[w], plan, lambda y, m=m: round(y, 6) >= m))
        else:
            out.append(bisect_plan(tabs[w], plan, lambda y, m=m: y >= m))
    return out


def compute_chain_cost_host(tab, chain, target, min_yield_g, max_time_seconds):
    """_compute_chain_cost :1903-1942"""
    _finite(min_yield_g=min_yield_g, max_time_seconds=max_time_seconds)
    plan = chain_plan(tab, chain, target)
    return chain_result(tab, plan, solve_plans_host([tab], [0], [plan], [min_yield_g])[0], max_time_seconds)


def compute_one_pot_cost_host(tab, target, min_yield_g, max_time_seconds):
    """_compute_one_pot_cost :2111-2266"""
    _finite(min_yield_g=min_yield_g, max_time_seconds=max_time_seconds)
    plans = one_pot_plans(tab, target, max_time_seconds)
    return one_pot_result(tab, plans, solve_plans_host([tab], [0] * len(plans), plans, [min_yield_g] * len(plans)))


# ---- the whole request (:1777-1901), cut around the searches ----------------------------------------------------------------------

REQUEST_DEFAULTS = dict(min_medicinal_value=3.0, max_toxicity=4.0, min_yield_g=1.0, max_time_seconds=28800.0,
                        required_phase=None, phase_temp_C=25.0, max_routes_per_target=5, max_steps=6)


def request_plans(tab, request):
    """the candidates of one request -> dict(request, qualifying, chains [(target, plan)], one_pot [(target, [plan])]) in
    the reference's order; the searches are the caller's"""
    unknown = set(request) - set(REQUEST_DEFAULTS) - {"world"}
    if unknown:
        raise ValueError("unknown request keys %s" % sorted(unknown))
    q = dict(REQUEST_DEFAULTS)
    q.update((k, v) for k, v in request.items() if k != "world")
    _finite(min_medicinal_value=q["min_medicinal_value"], max_toxicity=q["max_toxicity"], min_yield_g=q["min_yield_g"],
            max_time_seconds=q["max_time_seconds"], phase_temp_C=q["phase_temp_C"])
    if q["required_phase"] not in (None, "") + PHASE_NAMES:
        raise ValueError("required_phase must be one of %s or None" % (PHASE_NAMES,))
    w = _world(tab)
    med, tox, layer = tab["medicinal_value"].tolist(), tab["base_toxicity"].tolist(), tab["layer"].tolist()
    qualifying = [c for c in range(tab["C"]) if med[c] >= q["min_medicinal_value"] and tox[c] <= q["max_toxicity"]]
    if q["required_phase"]:
        qualifying = [c for c in qualifying if _phase(w, c, q["phase_temp_C"], 1.0) == q["required_phase"]]
    chains, one_pot = [], []
    effective_steps = max(q["max_steps"], tab["num_layers"] * 2)
    for c in qualifying:
        if layer[c] == 1:
            continue
        for chain in find_reaction_chains(tab, c, q["max_routes_per_target"], effective_steps):
            chains.append((c, chain_plan(tab, chain, c)))
    for c in qualifying:
        if layer[c] > 1:
            one_pot.append((c, one_pot_plans(tab, c, q["max_time_seconds"])))
    return dict(request=q, qualifying=qualifying, chains=chains, one_pot=one_pot)


def request_result(tab, planned, chain_solved, one_pot_solved):
    """compute_optimal_cost's dict from the solved candidates of request_plans (same order, one_pot_solved a list per target)"""
    q = planned["request"]
    if not planned["qualifying"]:
        return {"success": False, "found": False, "message": "No qualifying compounds found.", "optimal_cost": None}
    med, tox, layer = tab["medicinal_value"].tolist(), tab["base_toxicity"].tolist(), tab["layer"].tolist()
    names, price = tab["chem_names"], tab["price_per_gram"].tolist()
    best = None

    def offer(c, cost, num_steps, total_time, detail):
        nonlocal best
        if best is None or cost < best["optimal_cost"]:
            best = {"target": names[c], "medicinal_value": med[c], "base_toxicity": tox[c], "optimal_cost": cost,
                    "num_steps": num_steps, "total_time_seconds": total_time, "route_detail": detail}

    solved = iter(zip(planned["chains"], chain_solved))
    pending = next(solved, None)
    for c in planned["qualifying"]:
        if layer[c] == 1:
            offer(c, round(price[c] * q["min_yield_g"], 4), 0, 0.0, {"note": "Direct purchase"})
            continue
        while pending is not None and pending[0][0] == c:
            (_, plan), sol = pending
            result = chain_result(tab, plan, sol, q["max_time_seconds"])
            if result is not None:
                offer(c, result["total_cost"], len(plan["steps"]), result["total_time"], result)
            pending = next(solved, None)
    for (c, plans), sol in zip(planned["one_pot"], one_pot_solved):
        result = one_pot_result(tab, plans, sol)
        if result is not None:
            offer(c, result["total_cost"], 1, result["total_time"], result)
    if best is None:
        return {"success": True, "found": False, "message": "No feasible synthesis route found within constraints.",
                "optimal_cost": None}
    return {"success": True, "found": True, "optimal_cost": best["optimal_cost"], "target": best["target"],
            "medicinal_value": best["medicinal_value"], "base_toxicity": best["base_toxicity"], "num_steps": best["num_steps"],
            "total_time_seconds": best["total_time_seconds"], "route_detail": best["route_detail"],
            "message": ("Optimal cost: %.2f credits to produce %sg of %s (med=%.2f, tox=%.2f) in %d step(s), %.0fs."
                        % (best["optimal_cost"], q["min_yield_g"], best["target"], best["medicinal_value"],
                           best["base_toxicity"], best["num_steps"], best["total_time_seconds"]))}


def compute_optimal_cost_host(tab, **request):
    """compute_optimal_cost :1777-1901 on the host"""
    planned = request_plans(tab, request)
    m = planned["request"]["min_yield_g"]
    plans = [p for _, p in planned["chains"]]
    chain_solved = solve_plans_host([tab], [0] * len(plans), plans, [m] * len(plans))
    one_pot_solved = [solve_plans_host([tab], [0] * len(ps), ps, [m] * len(ps)) for _, ps in planned["one_pot"]]
    return request_result(tab, planned, chain_solved, one_pot_solved)
