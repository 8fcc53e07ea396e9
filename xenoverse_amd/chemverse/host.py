"""ChemVerse host restatement: the reference's simulate_chain_reaction (xenoverse/chemverse/environment/simulator.py:639-880
and what it calls, :34-500, :614-636) over the flat tables of tables.py, one experiment at a time, in plain Python / numpy.

This file is the specification csrc/chemverse.hip follows, and what runs where there is no GPU (backend="host").  It keeps the
reference's arithmetic operation for operation — the same numpy exp / log, the same Python `**`, the same left-to-right sums —
so that its results equal the reference's recorded runs bit for bit.  One sum is the exception: the reference adds the
reactants' grams in the iteration order of a Python set of id strings (:369-371), which changes from process to process with
the string hash seed; here the sum runs in the reaction's own order (three or more reactants can differ in the last bit).

What must be kept, and is easy to lose:
  * the pool is a dict in INSERTION order: initial amounts in the caller's order, products and byproducts as they first
    appear; heat capacity, gas moles, phase heat, the external-solvent search and gas loss run over it in that order
  * the applicable set is computed once per step from the pool at the step's start (:721); each reaction is then evaluated
    against the pool as already changed by the reactions before it in the same step (:737-766), its solvent searched again —
    and a search that now finds none leaves the dissolution factor at 1 (:355-367)
  * an empty applicable set skips the vessel update and the gas loss (:725-729); totals exclude a failing step (:778-806)
"""
import numpy as np

from . import tables as T

R_kJ = 8.314e-3      # simulator.py:10-15
R_J = 8.314
AMBIENT_TEMP_C = 25.0
HISTORY_MAX = 30     # temperature_history[:30]
LOG_MAX = 20         # reaction_log[:20]

SOLV_NONE, SOLV_SELF, SOLV_NEAT = -1, -2, -3      # _find_common_solvent's None, "__self__", "__neat__"; >= 0: a chemical
FAIL_NONE, FAIL_INIT_T, FAIL_INIT_P, FAIL_RUN_T, FAIL_RUN_P = range(5)
SOLID, LIQUID, GAS = 0, 1, 2

BRENT_XTOL = 1e-10
BRENT_RTOL = 4 * np.finfo(float).eps      # scipy.optimize.brentq's default
BRENT_MAXITER = 200


class BrentError(Exception):
    """what scipy raises: a NaN function value, or no convergence within maxiter"""


def brentq_host(f, xa, xb, xtol=BRENT_XTOL, rtol=BRENT_RTOL, maxiter=BRENT_MAXITER):
    """scipy.optimize.brentq(f, xa, xb, xtol=xtol, maxiter=maxiter), step for step -> (root, function evaluations).
    Raises BrentError where scipy raises (a NaN value; no convergence).  f(xa) and f(xb) must differ in sign."""
    def call(x):
        v = float(f(x))
        if v != v:
            raise BrentError("the function value at x=%r is NaN" % x)
        return v

    xpre, xcur = float(xa), float(xb)
    xblk = fblk = spre = scur = 0.0
    fpre = call(xpre)
    fcur = call(xcur)
    calls = 2
    if fpre == 0:
        return xpre, calls
    if fcur == 0:
        return xcur, calls
    if np.signbit(fpre) == np.signbit(fcur):
        raise ValueError("f(a) and f(b) must have different signs")
    for _ in range(maxiter):
        if fpre != 0 and fcur != 0 and np.signbit(fpre) != np.signbit(fcur):
            xblk, fblk = xpre, fpre
            spre = scur = xcur - xpre
        if abs(fblk) < abs(fcur):
            xpre, xcur = xcur, xblk
            xblk = xpre
            fpre, fcur = fcur, fblk
            fblk = fpre
        delta = (xtol + rtol * abs(xcur)) / 2
        sbis = (xblk - xcur) / 2
        if fcur == 0 or abs(sbis) < delta:
            return xcur, calls
        if abs(spre) > delta and abs(fcur) < abs(fpre):
            if xpre == xblk:      # interpolate
                stry = -fcur * (xcur - xpre) / (fcur - fpre)
            else:                 # extrapolate
                dpre = (fpre - fcur) / (xpre - xcur)
                dblk = (fblk - fcur) / (xblk - xcur)
                with np.errstate(all="ignore"):
                    stry = float(-np.float64(fcur) * (np.float64(fblk) * dblk - np.float64(fpre) * dpre)
                                 / (np.float64(dblk) * dpre * (np.float64(fblk) - fpre)))
            if 2 * abs(stry) < min(abs(spre), 3 * abs(sbis) - delta):
                spre, scur = scur, stry
            else:
                spre = scur = sbis
        else:
            spre = scur = sbis
        xpre, fpre = xcur, fcur
        if abs(scur) > delta:
            xcur += scur
        else:
            xcur += delta if sbis > 0 else -delta
        fcur = call(xcur)
        calls += 1
    raise BrentError("failed to converge after %d iterations" % maxiter)


def seq_sum(values):
    """the builtin sum of floats as the reference's Python ran it: left to right from 0"""
    s = 0.0
    for v in values:
        s = s + v
    return s


def equilibrium_objective(K_eq, r_mol, r_coeff, p_mol, p_coeff):
    """solve_equilibrium_extent's objective (:183-190)"""
    def objective(xi):
        products_conc = [p + vp * xi for p, vp in zip(p_mol, p_coeff)]
        reactants_conc = [r - vr * xi for r, vr in zip(r_mol, r_coeff)]
        if any(c <= 0 for c in reactants_conc) or any(c < 0 for c in products_conc):
            return float("inf")
        with np.errstate(all="ignore"):
            Q = np.prod([c ** vp for c, vp in zip(products_conc, p_coeff)])
            Q /= np.prod([c ** vr for c, vr in zip(reactants_conc, r_coeff)])
            return Q - K_eq
    return objective


def solve_equilibrium_extent_host(K_eq, r_mol, r_coeff, p_mol, p_coeff, outcome=None):
    """:170-205.  outcome (a list, optional) receives "root", "zero", "max" or "except"."""
    max_extent = min(a / c for a, c in zip(r_mol, r_coeff))
    max_extent *= 0.9999
    if max_extent <= 0:
        return 0.0
    objective = equilibrium_objective(K_eq, r_mol, r_coeff, p_mol, p_coeff)
    try:
        f0 = objective(0.0)
        f1 = objective(max_extent)
        if f0 * f1 < 0:
            xi_eq, _ = brentq_host(objective, 0.0, max_extent)
            kind = "root"
        elif f0 >= 0:
            xi_eq, kind = 0.0, "zero"
        else:
            xi_eq, kind = max_extent, "max"
    except Exception:
        xi_eq, kind = max_extent * 0.5, "except"
    if outcome is not None:
        outcome.append(kind)
    return float(np.clip(xi_eq, 0.0, max_extent))


class _World(object):
    """one world's tables, unpacked into Python lists once"""

    def __init__(self, tab):
        self.tab = tab
        self.C, self.R = tab["C"], tab["R"]
        f = tab["chem_f"]
        self.mw, self.mp, self.bp = f[:, T.CH_MW].tolist(), f[:, T.CH_MP].tolist(), f[:, T.CH_BP].tolist()
        self.clausius, self.cp = f[:, T.CH_CLAUSIUS].tolist(), f[:, T.CH_CP].tolist()
        self.lfus, self.lvap = f[:, T.CH_LFUS].tolist(), f[:, T.CH_LVAP].tolist()
        self.is_solvent = (f[:, T.CH_SOLVENT] != 0).tolist()
        self.sol_present, self.sol_value = tab["sol_present"], tab["sol_value"]
        self.rxn = []
        for r in range(self.R):
            i, g = tab["rxn_i"][r].tolist(), tab["rxn_f"][r].tolist()
            nr, npr, nb, nc = i[:4]
            self.rxn.append(dict(
                reactants=list(zip(i[T.RX_REAC:T.RX_REAC + nr], i[T.RX_REAC_COEFF:T.RX_REAC_COEFF + nr])),
                products=list(zip(i[T.RX_PROD:T.RX_PROD + npr], i[T.RX_PROD_COEFF:T.RX_PROD_COEFF + npr])),
                byproducts=list(zip(i[T.RX_BYP:T.RX_BYP + nb], i[T.RX_BYP_COEFF:T.RX_BYP_COEFF + nb])),
                catalysts=i[T.RX_CAT:T.RX_CAT + nc], dG=g[T.RF_DG], dH=g[T.RF_DH], Ea=g[T.RF_EA], logA=g[T.RF_LOGA],
                solv_mask=int(tab["rxn_solv"][r])))

    def state_at(self, c, temp_C, pressure_atm):      # :34-41
        bp_adj = self.bp[c] + self.clausius[c] * np.log(max(0.01, pressure_atm))
        if temp_C < self.mp[c]:
            return SOLID
        if temp_C < bp_adj:
            return LIQUID
        return GAS


def _world(tab):
    w = tab.get("_host_world")
    if w is None:
        w = tab["_host_world"] = _World(tab)
    return w


def find_common_solvent(w, rxn, pool, temp_C, pressure_atm):      # :219-278
    reactant_ids = [c for c, _ in rxn["reactants"]]
    solvent_reactants = [c for c in reactant_ids if w.is_solvent[c]]
    non_solvent = [c for c in reactant_ids if not w.is_solvent[c]]
    if not non_solvent:
        return SOLV_SELF
    for s in solvent_reactants:
        if w.state_at(s, temp_C, pressure_atm) != LIQUID:
            continue
        if (rxn["solv_mask"] >> s) & 1:      # every non-solvent reactant lists s
            return s
    has_solid_or_gas = any(w.state_at(c, temp_C, pressure_atm) != LIQUID for c in non_solvent)
    for s, g in pool.items():      # the pool's insertion order
        if (g > 1e-9 and w.is_solvent[s] and s not in reactant_ids
                and w.state_at(s, temp_C, pressure_atm) == LIQUID and (rxn["solv_mask"] >> s) & 1):
            return s
    if not has_solid_or_gas:      # then every non-solvent reactant is liquid (:270-276)
        return SOLV_NEAT
    return SOLV_NONE


def dissolved_fraction(w, c, s, pool):      # :281-305, s a chemical
    if w.is_solvent[c]:
        return 1.0
    max_g_per_100mL = float(w.sol_value[c, s]) if w.sol_present[c, s] else 0.0
    if max_g_per_100mL <= 0:
        return 0.0
    solvent_g = pool.get(s, 0.0)
    if solvent_g < 1e-9:
        return 0.0
    solvent_mL = solvent_g / 0.9
    max_dissolved_g = max_g_per_100mL * (solvent_mL / 100.0)
    chem_g = pool.get(c, 0.0)
    if chem_g <= 0:
        return 0.0
    return min(1.0, max_dissolved_g / chem_g)


def find_applicable(w, pool, temp_C, pressure_atm):      # :308-335
    out = []
    for r, rxn in enumerate(w.rxn):
        needed = [c for c, _ in rxn["reactants"]] + rxn["catalysts"]
        if not all(pool.get(c, 0.0) > 1e-9 for c in needed):
            continue
        if find_common_solvent(w, rxn, pool, temp_C, pressure_atm) == SOLV_NONE:
            continue
        out.append(r)
    return out


def phase_factor(w, rxn, temp_C, pressure_atm):      # :152-167
    factors = [(0.01, 1.0, 8.0)[w.state_at(c, temp_C, pressure_atm)] for c, _ in rxn["reactants"]]
    log_mean = np.mean(np.log(np.array(factors, dtype=float) + 1e-30))
    return float(np.exp(log_mean))


def heterogeneous_rate_factor(w, rxn, pool, temp_C, pressure_atm):      # :111-149
    present = [(c, w.state_at(c, temp_C, pressure_atm)) for c, _ in rxn["reactants"] if pool.get(c, 0.0) > 1e-9]
    phases = set(p for _, p in present)
    if len(phases) <= 1:
        return 1.0
    factor = 1.0
    if SOLID in phases and LIQUID in phases:
        solid_mass = 0.0
        for c, p in present:
            if p == SOLID:
                solid_mass += pool[c]
        factor *= max(0.01, solid_mass ** (2.0 / 3.0) / max(solid_mass, 0.1))
    if GAS in phases and LIQUID in phases:
        gas_mass = 0.0
        for c, p in present:
            if p == GAS:
                gas_mass += pool[c]
        factor *= min(1.0, pressure_atm * 0.5) * max(0.05, gas_mass ** 0.5 / max(gas_mass, 0.1))
    if SOLID in phases and GAS in phases:
        factor *= 0.05 * pressure_atm ** 0.3
    return float(np.clip(factor, 0.001, 2.0))


def step_single_reaction(w, rxn, pool, temp_C, pressure_atm, dt, solvent, outcome=None):      # :338-428
    """-> consumed [(chemical, g)], produced, byproducts (lists in the reaction's order), heat_released_J"""
    T_K = temp_C + 273.15
    K_ref = np.exp(-rxn["dG"] / (R_kJ * 298.0))
    K_eq = float(max(K_ref * np.exp(-rxn["dH"] / R_kJ * (1.0 / T_K - 1.0 / 298.0)), 1e-30))
    k_rate = float(10 ** rxn["logA"] * np.exp(-rxn["Ea"] / (R_kJ * T_K)))
    pf = phase_factor(w, rxn, temp_C, pressure_atm)
    hetero_f = heterogeneous_rate_factor(w, rxn, pool, temp_C, pressure_atm)
    reactant_ids = [c for c, _ in rxn["reactants"]]

    dissolution = 1.0
    if solvent == SOLV_NEAT:
        dissolution = 0.3
    elif solvent >= 0 and solvent not in reactant_ids:
        dissolution = 1.0
        for c in reactant_ids:
            dissolution = min(dissolution, dissolved_fraction(w, c, solvent, pool))
    # SOLV_SELF, a reactant solvent, and SOLV_NONE (a search that finds none after the pool has changed): 1.0

    reactant_g = seq_sum(pool.get(c, 0.0) for c in reactant_ids)      # the reaction's order (see the module text)
    catalyst_g = [pool.get(c, 0.0) for c in rxn["catalysts"] if pool.get(c, 0.0) > 1e-9]
    cat_factor = 1.0
    if catalyst_g and reactant_g > 0:      # :208-216
        cat_factor = 1.0 + 10.0 * (seq_sum(catalyst_g) / reactant_g) ** 0.5
    k_eff = k_rate * pf * hetero_f * cat_factor * dissolution

    r_mol = [pool.get(c, 0.0) / w.mw[c] * dissolution for c in reactant_ids]
    r_coeff = [k for _, k in rxn["reactants"]]
    p_mol = [pool.get(c, 0.0) / w.mw[c] for c, _ in rxn["products"]]
    p_coeff = [k for _, k in rxn["products"]]
    xi_eq = solve_equilibrium_extent_host(K_eq, r_mol, r_coeff, p_mol, p_coeff, outcome)
    if xi_eq <= 1e-30:
        return [], [], [], 0.0
    xi_t = xi_eq * (1.0 - np.exp(-k_eff * dt))
    xi_t = float(np.clip(xi_t, 0.0, xi_eq))

    consumed = [(c, min(k * xi_t, m) * w.mw[c]) for (c, k), m in zip(rxn["reactants"], r_mol)]
    produced = [(c, k * xi_t * w.mw[c]) for c, k in rxn["products"]]
    byproducts = [(c, k * xi_t * w.mw[c] * 0.1) for c, k in rxn["byproducts"]]
    total_consumed = seq_sum(g for _, g in consumed)
    total_produced = seq_sum(g for _, g in produced) + seq_sum(g for _, g in byproducts)
    if total_produced > total_consumed and total_consumed > 1e-12:
        scale = total_consumed / total_produced
        produced = [(c, g * scale) for c, g in produced]
        byproducts = [(c, g * scale) for c, g in byproducts]
    return consumed, produced, byproducts, xi_t * (-rxn["dH"]) * 1000.0


def mixture_heat_capacity(w, pool):      # :57-65
    total = 0.0
    for c, g in pool.items():
        if g > 1e-9:
            total += g * w.cp[c]
    return max(total, 0.1)


def count_gas_moles(w, pool, temp_C, pressure_atm):      # :68-80
    total = 0.0
    for c, g in pool.items():
        if g > 1e-9 and w.state_at(c, temp_C, pressure_atm) == GAS:
            total += g / w.mw[c]
    return total


def phase_transition_heat(w, pool, old_T, new_T, pressure_atm):      # :83-108
    heat = 0.0
    for c, g in pool.items():
        if g < 1e-9:
            continue
        bp_adj = w.bp[c] + w.clausius[c] * np.log(max(0.01, pressure_atm))
        mp = w.mp[c]
        if old_T < mp <= new_T:
            heat += g * w.lfus[c]
        elif new_T < mp <= old_T:
            heat -= g * w.lfus[c]
        if old_T < bp_adj <= new_T:
            heat += g * w.lvap[c]
        elif new_T < bp_adj <= old_T:
            heat -= g * w.lvap[c]
    return heat


def update_vessel(w, v, pool, heat_J, dt, initial_gas_moles, events=None):      # :431-499; v: the vessel dict
    old_T = v["T"]
    mode = v["mode"]
    if mode == 0:      # isothermal
        if v["max_heat_W"] > 0 and dt > 0:
            heat_rate_W = abs(heat_J) / dt
            if heat_rate_W > v["max_heat_W"]:
                excess_J = (heat_rate_W - v["max_heat_W"]) * dt
                excess_heat = excess_J if heat_J > 0 else -excess_J
                Cp = mixture_heat_capacity(w, pool)
                dT = excess_heat / Cp
                phase_heat = phase_transition_heat(w, pool, old_T, old_T + dT, v["P"])
                v["T"] += (excess_heat - phase_heat) / Cp
                if events is not None:
                    events.add("isothermal_excess")
    elif mode == 1:      # adiabatic
        Cp = mixture_heat_capacity(w, pool)
        dT = heat_J / Cp
        phase_heat = phase_transition_heat(w, pool, old_T, old_T + dT, v["P"])
        v["T"] += (heat_J - phase_heat) / Cp
    elif mode == 2:      # open_air
        Cp = mixture_heat_capacity(w, pool)
        heat_loss_J = v["htc"] * Cp * (v["T"] - AMBIENT_TEMP_C) * dt
        net_heat = heat_J - heat_loss_J
        phase_heat = phase_transition_heat(w, pool, old_T, old_T + net_heat / Cp, v["P"])
        v["T"] += (net_heat - phase_heat) / Cp
    else:      # heating, cooling: the same arithmetic
        Cp = mixture_heat_capacity(w, pool)
        total_dT = v["rate"] * dt + heat_J / Cp
        phase_heat = phase_transition_heat(w, pool, old_T, old_T + total_dT, v["P"])
        v["T"] += (heat_J + v["rate"] * dt * Cp - phase_heat) / Cp
    v["T"] = float(np.clip(v["T"], -273.0, 5000.0))
    if v["sealed"]:
        gas = count_gas_moles(w, pool, v["T"], v["P"])
        T_K_now, T_K_init = v["T"] + 273.15, v["T0"] + 273.15
        if initial_gas_moles > 1e-9:
            v["P"] = v["P0"] * (gas / initial_gas_moles) * (T_K_now / T_K_init)
        elif gas > 1e-9:
            v["P"] = gas * R_J * T_K_now / (v["vol"] * 0.001) / 101325.0
        v["P"] = float(np.clip(v["P"], 0.001, 1000.0))


def simulate_one(tab, amounts, temperature_C, pressure_atm, duration_s, equipment, heating_rate=0.0, volume_L=1.0,
                 step_seconds=5.0, events=None):
    """one experiment.  amounts: [(chemical index, grams)] in the caller's order; equipment: an index.  -> dict of arrays and
    scalars named as xv_chem_simulate's outputs (include/xeno.h).  events (a set, optional) collects the branches taken."""
    w = _world(tab)
    C, R = w.C, w.R
    ei, ef = tab["eq_i"][equipment], tab["eq_f"][equipment].tolist()
    v = dict(T=float(temperature_C), P=float(pressure_atm), T0=float(temperature_C), P0=float(pressure_atm),
             sealed=bool(ei[T.EI_SEALED]), mode=int(ei[T.EI_MODE]), rate=float(heating_rate), vol=float(volume_L),
             htc=ef[T.EF_HTC], max_heat_W=ef[T.EF_MAX_HEAT_W])
    max_T, min_T, max_P, retention = ef[T.EF_MAX_T], ef[T.EF_MIN_T], ef[T.EF_MAX_P], ef[T.EF_RETENTION]
    pool = {}
    for c, g in amounts:
        if g > 1e-9:
            pool[int(c)] = float(g)
    initial_gas_moles = count_gas_moles(w, pool, v["T"], v["P"])
    num_steps = T.num_steps_of(duration_s, step_seconds)
    dt = duration_s / num_steps

    out = dict(final_pool=np.zeros(C), consumed=np.zeros(C), produced=np.zeros(C), byproduct=np.zeros(C), gas_lost=np.zeros(C),
               fired=np.zeros(R, np.int32), num_steps=num_steps, steps_run=0, converged=0, failure=FAIL_NONE, failure_step=-1,
               hist_step=np.zeros(HISTORY_MAX, np.int32), hist_T=np.zeros(HISTORY_MAX), hist_P=np.zeros(HISTORY_MAX),
               hist_count=0, log_step=np.zeros(LOG_MAX, np.int32), log_active=np.zeros(LOG_MAX, np.int32),
               log_T=np.zeros(LOG_MAX), log_P=np.zeros(LOG_MAX), log_consumed=np.zeros((LOG_MAX, C)),
               log_produced=np.zeros((LOG_MAX, C)), log_count=0)
    if v["T"] > max_T or v["T"] < min_T or v["P"] > max_P:      # :689-716
        out["failure"] = FAIL_INIT_T if (v["T"] > max_T or v["T"] < min_T) else FAIL_INIT_P
        out["final_T"], out["final_P"] = v["T"], v["P"]
        return out

    total_c, total_p, total_b, total_lost = {}, {}, {}, {}
    converged_steps = 0
    stride = max(1, num_steps // 20)
    for step in range(num_steps):
        out["steps_run"] = step + 1
        applicable = find_applicable(w, pool, v["T"], v["P"])
        if not applicable:
            converged_steps += 1
            if converged_steps >= 3:
                break
            continue
        step_c, step_p, step_b = {}, {}, {}
        step_heat, progress = 0.0, False
        for r in applicable:
            rxn = w.rxn[r]
            solvent = find_common_solvent(w, rxn, pool, v["T"], v["P"])
            outcome = [] if events is not None else None
            consumed, produced, byproducts, heat = step_single_reaction(w, rxn, pool, v["T"], v["P"], dt, solvent, outcome)
            if seq_sum(g for _, g in consumed) + seq_sum(g for _, g in produced) < 1e-12:
                continue
            progress = True
            step_heat += heat
            out["fired"][r] += 1
            if events is not None:
                events.add("solvent_" + {SOLV_NONE: "none_on_recheck", SOLV_SELF: "self", SOLV_NEAT: "neat"}.get(
                    solvent, "reactant" if solvent in [c for c, _ in rxn["reactants"]] else "external"))
                events.update("equilibrium_" + k for k in outcome)
            for c, g in consumed:
                actual = min(g, pool.get(c, 0.0))
                if actual > 1e-12:
                    pool[c] = pool.get(c, 0.0) - actual
                    step_c[c] = step_c.get(c, 0.0) + actual
            for c, g in produced:
                if g > 1e-12:
                    pool[c] = pool.get(c, 0.0) + g
                    step_p[c] = step_p.get(c, 0.0) + g
            for c, g in byproducts:
                if g > 1e-12:
                    pool[c] = pool.get(c, 0.0) + g
                    step_b[c] = step_b.get(c, 0.0) + g
        update_vessel(w, v, pool, step_heat, dt, initial_gas_moles, events)
        bad_T = v["T"] > max_T or v["T"] < min_T
        if bad_T or v["P"] > max_P:      # the batch is destroyed: only what was consumed before this step is reported
            pool.clear()
            total_p, total_b, total_lost = {}, {}, {}
            out["failure"], out["failure_step"] = (FAIL_RUN_T if bad_T else FAIL_RUN_P), step
            break
        if not v["sealed"]:      # _apply_gas_loss :614-636
            for c in list(pool.keys()):
                if pool[c] < 1e-9:
                    continue
                if w.state_at(c, v["T"], v["P"]) == GAS:
                    g = pool[c]
                    escaped = g * (1.0 - retention)
                    if escaped > 1e-12:
                        pool[c] = g - escaped
                        total_lost[c] = total_lost.get(c, 0.0) + escaped
        if not progress:
            converged_steps += 1
            if converged_steps >= 3:
                break
        else:
            converged_steps = 0
        for tot, stp in ((total_c, step_c), (total_p, step_p), (total_b, step_b)):
            for c, g in stp.items():
                tot[c] = tot.get(c, 0.0) + g
        if step < 5 or step % stride == 0:
            n = out["hist_count"]
            if n < HISTORY_MAX:
                out["hist_step"][n], out["hist_T"][n], out["hist_P"][n] = step, v["T"], v["P"]
                out["hist_count"] = n + 1
            n = out["log_count"]
            if progress and n < LOG_MAX:
                out["log_step"][n], out["log_active"][n], out["log_T"][n], out["log_P"][n] = step, len(applicable), v["T"], v["P"]
                for c, g in step_c.items():
                    out["log_consumed"][n, c] = g
                for c, g in step_p.items():
                    out["log_produced"][n, c] = g
                out["log_count"] = n + 1
    if out["failure"] == FAIL_NONE:
        out["converged"] = int(converged_steps >= 3)
    for c, g in pool.items():
        if g > 1e-9:
            out["final_pool"][c] = g
    for key, tot in (("consumed", total_c), ("produced", total_p), ("byproduct", total_b), ("gas_lost", total_lost)):
        for c, g in tot.items():
            out[key][c] = g
    out["final_T"], out["final_P"] = v["T"], v["P"]
    return out


SCALARS = (("num_steps", np.int32), ("steps_run", np.int32), ("converged", np.uint8), ("failure", np.uint8),
           ("failure_step", np.int32), ("final_T", np.float64), ("final_P", np.float64), ("hist_count", np.int32),
           ("log_count", np.int32))
PER_CHEM = ("final_pool", "consumed", "produced", "byproduct", "gas_lost")
HISTORY = ("hist_step", "hist_T", "hist_P", "hist_count")
LOG = ("log_step", "log_active", "log_T", "log_P", "log_consumed", "log_produced", "log_count")


def simulate_chain_host(tables, experiments, record="log"):
    """tables: one world's tables or a list of them; experiments: dicts with world (index, default 0), amounts [(chemical index,
    grams)], temperature_C, pressure_atm, duration_s, equipment (index), heating_rate_C_per_s, vessel_volume_L, step_seconds.
    -> dict of numpy arrays [n, ...] named as the device outputs, rows padded to the widest world."""
    if isinstance(tables, dict):
        tables = [tables]
    cs, rs = max(t["C"] for t in tables), max(1, max(t["R"] for t in tables))
    res = [simulate_one(tables[e.get("world", 0)], e["amounts"], e["temperature_C"], e["pressure_atm"], e["duration_s"],
                        e["equipment"], e.get("heating_rate_C_per_s", 0.0), e.get("vessel_volume_L", 1.0),
                        e.get("step_seconds", 5.0)) for e in experiments]
    n = len(res)
    out = {}
    for k in PER_CHEM:
        out[k] = np.zeros((n, cs))
        for i, r in enumerate(res):
            out[k][i, :len(r[k])] = r[k]
    out["fired"] = np.zeros((n, rs), np.int32)
    for i, r in enumerate(res):
        out["fired"][i, :len(r["fired"])] = r["fired"]
    for k, dt in SCALARS:
        out[k] = np.array([r[k] for r in res], dt)
    if record in ("history", "log"):
        for k in HISTORY[:3]:
            out[k] = np.stack([r[k] for r in res]) if n else np.zeros((0, HISTORY_MAX))
    if record == "log":
        for k in LOG[:4]:
            out[k] = np.stack([r[k] for r in res]) if n else np.zeros((0, LOG_MAX))
        for k in ("log_consumed", "log_produced"):
            out[k] = np.zeros((n, LOG_MAX, cs))
            for i, r in enumerate(res):
                out[k][i, :, :r[k].shape[1]] = r[k]
    if record == "none":
        del out["hist_count"], out["log_count"]
    elif record == "history":
        del out["log_count"]
    return out
