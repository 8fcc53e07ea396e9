"""ChemVerse world tables: the reference's World (xenoverse/chemverse/world_gen/models.py:215-265, or its to_dict() / world-JSON
form) as flat numeric arrays.

Chemical and reaction indices follow the dicts' INSERTION order: the reference iterates world.reactions.values() in that order
and mutates the pool as it goes (environment/simulator.py:318, :737), so reaction order is semantics.  Equipment indices follow
the world's own equipment dict.

build_tables(world) -> dict of numpy arrays (one world); pack_worlds([tables, ...]) -> the concatenated arrays with per-world
offsets that xv_chem_set_worlds borrows (include/xeno.h).
"""
import numpy as np

from .. import _lib

# ---- limits (include/xeno.h XV_CHEM_*) -----------------------------------------------------------------------------------
C_MAX = 64            # chemicals per world
R_MAX = 128           # reactions per world
E_MAX = 16            # equipment entries per world
REACTANTS_MAX = 6     # per reaction
PRODUCTS_MAX = 4
BYPRODUCTS_MAX = 4
CATALYSTS_MAX = 4
COEFF_MAX = 8         # largest stoichiometric coefficient
STEPS_MAX = 4096      # steps per experiment: ceil(duration / step_seconds)
CHAIN_MAX = 16        # reactions per route of the cost oracle (optimal_host.py, csrc/chemverse_optimal.hip)

# columns of chem_f
CH_MW, CH_MP, CH_BP, CH_CLAUSIUS, CH_CP, CH_LFUS, CH_LVAP, CH_SOLVENT = range(8)
CHEM_F = 8
# columns of rxn_i
RX_NREAC, RX_NPROD, RX_NBYP, RX_NCAT = range(4)
RX_REAC = 4
RX_REAC_COEFF = RX_REAC + REACTANTS_MAX
RX_PROD = RX_REAC_COEFF + REACTANTS_MAX
RX_PROD_COEFF = RX_PROD + PRODUCTS_MAX
RX_BYP = RX_PROD_COEFF + PRODUCTS_MAX
RX_BYP_COEFF = RX_BYP + BYPRODUCTS_MAX
RX_CAT = RX_BYP_COEFF + BYPRODUCTS_MAX
RXN_I = RX_CAT + CATALYSTS_MAX      # 36
# columns of rxn_f
RF_DG, RF_DH, RF_EA, RF_LOGA = range(4)
RXN_F = 4
# columns of eq_i / eq_f
EI_SEALED, EI_MODE = range(2)
EQ_I = 2
EF_MAX_T, EF_MIN_T, EF_MAX_P, EF_HTC, EF_MAX_HEAT_W, EF_RETENTION = range(6)
EQ_F = 6

# world_gen/models.py:199-211: a world file's cost_params are laid over these
DEFAULT_COST_PARAMS = dict(heating_coeff=0.8, cooling_coeff=1.2, heating_exponent=1.5, cooling_exponent=1.3,
                           pressure_high_coeff=1.5, pressure_low_coeff=1.5, pressure_high_exp=0.7, pressure_low_exp=0.6,
                           equipment_base=5.0, equipment_pressure_coeff=0.3, duration_coeff=0.05)

THERMAL_MODES = ("isothermal", "adiabatic", "open_air", "heating", "cooling")
GAS_RETENTION_RATES = {"open_beaker": 0.0, "reflux_condenser": 0.75}      # simulator.py:608-611


def _unsupported(what, got, limit_name, limit):
    err = _lib.XenoError("libxeno_hip error %d: chemverse: %s = %d is beyond the supported %s = %d"
                         % (_lib.XV_ERR_UNSUPPORTED, what, got, limit_name, limit))
    err.code = _lib.XV_ERR_UNSUPPORTED
    return err


def _unsupported_text(text):
    err = _lib.XenoError("libxeno_hip error %d: chemverse: %s" % (_lib.XV_ERR_UNSUPPORTED, text))
    err.code = _lib.XV_ERR_UNSUPPORTED
    return err


def _get(obj, key, default=None):
    if isinstance(obj, dict):
        return obj.get(key, default)
    return getattr(obj, key, default)


def _pairs(seq):
    return [(x[0], x[1]) for x in seq]


def build_tables(world):
    """world: World.to_dict() / world JSON, or an object with .chemicals, .reactions, .equipment"""
    if isinstance(world, dict) and "chem_f" in world:
        return world
    chemicals = _get(world, "chemicals")
    reactions = _get(world, "reactions")
    equipment = _get(world, "equipment")
    if chemicals is None or reactions is None or equipment is None:
        raise ValueError("a ChemVerse world needs chemicals, reactions and equipment")
    chem_ids = list(chemicals.keys())
    rxn_ids = list(reactions.keys())
    equip_names = list(equipment.keys())
    C, R, E = len(chem_ids), len(rxn_ids), len(equip_names)
    if C < 1:
        raise ValueError("a ChemVerse world needs at least one chemical")
    if C > C_MAX:
        raise _unsupported("chemicals per world", C, "C_MAX", C_MAX)
    if R > R_MAX:
        raise _unsupported("reactions per world", R, "R_MAX", R_MAX)
    if E > E_MAX:
        raise _unsupported("equipment entries per world", E, "E_MAX", E_MAX)
    if "open_beaker" not in equipment:
        raise ValueError("a ChemVerse world's equipment needs 'open_beaker' (the reference's default, simulator.py:655)")
    cidx = {cid: i for i, cid in enumerate(chem_ids)}

    chem_f = np.zeros((C, CHEM_F), np.float64)
    sol_present = np.zeros((C, C), np.uint8)      # [chemical][solvent]: `sid in chem.solubility`
    sol_value = np.zeros((C, C), np.float64)      # [chemical][solvent]: chem.solubility[sid]
    for i, cid in enumerate(chem_ids):
        c = chemicals[cid]
        chem_f[i] = (_get(c, "molecular_weight"), _get(c, "melting_point"), _get(c, "boiling_point"),
                     _get(c, "clausius_C", 40.0), _get(c, "heat_capacity_J_per_gK", 2.0),
                     _get(c, "latent_heat_fusion_J_per_g", 150.0), _get(c, "latent_heat_vaporization_J_per_g", 800.0),
                     1.0 if _get(c, "is_solvent", False) else 0.0)
        for sid, v in (_get(c, "solubility", None) or {}).items():
            if sid in cidx:      # a solvent id outside the world can never be in a pool the tables describe
                sol_present[i, cidx[sid]] = 1
                sol_value[i, cidx[sid]] = float(v)
    if not np.isfinite(chem_f).all() or not np.isfinite(sol_value).all():
        raise ValueError("a ChemVerse world's chemical properties must be finite")
    if (chem_f[:, CH_MW] <= 0).any():
        raise ValueError("molecular weights must be positive")

    rxn_i = np.zeros((R, RXN_I), np.int32)
    rxn_f = np.zeros((R, RXN_F), np.float64)
    rxn_solv = np.zeros(R, np.uint64)      # bit s: solvent s is listed by every non-solvent reactant (simulator.py:243-246)
    for r, rid in enumerate(rxn_ids):
        x = reactions[rid]
        reac, prod = _pairs(_get(x, "reactants")), _pairs(_get(x, "products"))
        byp = [(b, k) for b, k in _pairs(_get(x, "byproducts", None) or []) if b in cidx]      # simulator.py:415
        cat = list(_get(x, "catalysts", None) or [])
        for what, ids in (("reactant", [c for c, _ in reac]), ("product", [c for c, _ in prod]), ("catalyst", cat)):
            for c in ids:
                if c not in cidx:
                    raise _unsupported_text("reaction %s names %s %s, which is not among the world's chemicals" % (rid, what, c))
        for what, ids in (("reactants", [c for c, _ in reac]), ("products", [c for c, _ in prod]),
                          ("byproducts", [c for c, _ in byp]), ("catalysts", cat)):
            if len(set(ids)) != len(ids):
                raise _unsupported_text("reaction %s lists one of its %s twice" % (rid, what))
        if len(reac) < 1:
            raise _unsupported_text("reaction %s has no reactants" % rid)
        for what, n, name, lim in (("reactants per reaction", len(reac), "REACTANTS_MAX", REACTANTS_MAX),
                                   ("products per reaction", len(prod), "PRODUCTS_MAX", PRODUCTS_MAX),
                                   ("byproducts per reaction", len(byp), "BYPRODUCTS_MAX", BYPRODUCTS_MAX),
                                   ("catalysts per reaction", len(cat), "CATALYSTS_MAX", CATALYSTS_MAX)):
            if n > lim:
                raise _unsupported(what, n, name, lim)
        for _, k in reac + prod + byp:
            if int(k) != k or int(k) < 1:
                raise _unsupported_text("reaction %s has a coefficient %r that is not a positive integer" % (rid, k))
            if int(k) > COEFF_MAX:
                raise _unsupported("largest coefficient", int(k), "COEFF_MAX", COEFF_MAX)
        row = rxn_i[r]
        row[RX_NREAC], row[RX_NPROD], row[RX_NBYP], row[RX_NCAT] = len(reac), len(prod), len(byp), len(cat)
        for base, cbase, lst in ((RX_REAC, RX_REAC_COEFF, reac), (RX_PROD, RX_PROD_COEFF, prod), (RX_BYP, RX_BYP_COEFF, byp)):
            for j, (c, k) in enumerate(lst):
                row[base + j], row[cbase + j] = cidx[c], int(k)
        for j, c in enumerate(cat):
            row[RX_CAT + j] = cidx[c]
        rxn_f[r] = (_get(x, "delta_G_kJ"), _get(x, "delta_H_kJ"), _get(x, "activation_energy_kJ"), _get(x, "log_A_factor"))
        mask = (1 << C) - 1
        for c, _ in reac:
            if chem_f[cidx[c], CH_SOLVENT] == 0.0:
                m = 0
                for s in range(C):
                    if sol_present[cidx[c], s]:
                        m |= 1 << s
                mask &= m
        rxn_solv[r] = mask
    if not np.isfinite(rxn_f).all():
        raise ValueError("a ChemVerse world's reaction constants must be finite")

    eq_i = np.zeros((E, EQ_I), np.int32)
    eq_f = np.zeros((E, EQ_F), np.float64)
    for e, name in enumerate(equip_names):
        spec = equipment[name]
        mode = spec["thermal_mode"]
        if mode not in THERMAL_MODES:
            raise _unsupported_text("equipment %s has thermal mode %r; supported: %s" % (name, mode, ", ".join(THERMAL_MODES)))
        eq_i[e] = (1 if spec["vessel_type"] == "sealed" else 0, THERMAL_MODES.index(mode))
        eq_f[e] = (spec.get("max_temp_C", 5000.0), spec.get("min_temp_C", -273.0), spec.get("max_pressure_atm", 1000.0),
                   spec.get("heat_transfer_coeff", 0.0), spec.get("max_heat_rate_W", 0.0),
                   GAS_RETENTION_RATES.get(name, 0.0))
    if not np.isfinite(eq_f).all():
        raise ValueError("a ChemVerse world's equipment limits must be finite")
    # what the cost oracle reads (optimal_host.py); xv_chem_set_worlds takes none of it.  A missing layer counts as 1, a
    # missing price is NaN (the reference's None: only layer-1 chemicals are bought)
    num = lambda v, d: d if v is None else float(v)      # noqa: E731
    layer = np.array([int(_get(chemicals[c], "layer", 1) or 1) for c in chem_ids], np.int32)
    price = np.array([num(_get(chemicals[c], "price_per_gram", None), np.nan) for c in chem_ids], np.float64)
    medicinal = np.array([num(_get(chemicals[c], "medicinal_value", None), np.nan) for c in chem_ids], np.float64)
    for i, c in enumerate(chem_ids):      # models.py:28: a property of the object, a product of two fields in the JSON
        if np.isnan(medicinal[i]):
            medicinal[i] = num(_get(chemicals[c], "medicinal_expected", None), 0.0) * \
                num(_get(chemicals[c], "medicinal_efficacy", None), 0.0)
    toxicity = np.array([num(_get(chemicals[c], "base_toxicity", None), 0.0) for c in chem_ids], np.float64)
    cost_params = dict(DEFAULT_COST_PARAMS)
    cost_params.update(_get(world, "cost_params", None) or {})
    eq_cost = np.array([(equipment[n].get("base_cost_per_hour", 0.0), equipment[n].get("cost_multiplier", 1.0))
                        for n in equip_names], np.float64).reshape(E, 2)
    return dict(layer=layer, price_per_gram=price, medicinal_value=medicinal, base_toxicity=toxicity,
                num_layers=int(layer.max()), cost_params=cost_params, base_cost_per_hour=eq_cost[:, 0].copy(),
                cost_multiplier=eq_cost[:, 1].copy(), chem_names=[str(_get(chemicals[c], "name", c)) for c in chem_ids],
                C=C, R=R, E=E, chem_ids=chem_ids, rxn_ids=rxn_ids, equip_names=equip_names,
                equip_specs=[dict(vessel_type=equipment[n]["vessel_type"], thermal_mode=equipment[n]["thermal_mode"],
                                  max_temp_C=equipment[n].get("max_temp_C", 5000.0),
                                  min_temp_C=equipment[n].get("min_temp_C", -273.0),
                                  max_pressure_atm=equipment[n].get("max_pressure_atm", 1000.0)) for n in equip_names],
                chem_f=chem_f, sol_present=sol_present, sol_value=sol_value, rxn_i=rxn_i, rxn_f=rxn_f, rxn_solv=rxn_solv,
                eq_i=eq_i, eq_f=eq_f)


def equipment_index(tab, equipment):
    """the reference's `catalog.get(equipment or "open_beaker", catalog["open_beaker"])` (simulator.py:655) as an index"""
    if isinstance(equipment, (int, np.integer)):
        if not 0 <= int(equipment) < tab["E"]:
            raise ValueError("equipment index %d is outside [0, %d)" % (int(equipment), tab["E"]))
        return int(equipment)
    name = equipment or "open_beaker"
    names = tab["equip_names"]
    return names.index(name) if name in names else names.index("open_beaker")


def num_steps_of(duration_s, step_seconds):
    """simulator.py:683; refused beyond STEPS_MAX"""
    if not (np.isfinite(duration_s) and np.isfinite(step_seconds)) or step_seconds <= 0:
        raise ValueError("duration_s and step_seconds must be finite, step_seconds positive")
    n = max(1, int(np.ceil(duration_s / step_seconds)))
    if n > STEPS_MAX:
        raise _unsupported("steps per experiment", n, "STEPS_MAX", STEPS_MAX)
    return n


def pack_worlds(tabs):
    """the worlds' tables concatenated, with world_off int32[n_world + 1][4] = the first (chemical, reaction, equipment,
    solubility entry) of every world; c_stride / r_stride: the widest world's chemicals / reactions"""
    off = np.zeros((len(tabs) + 1, 4), np.int64)
    for w, t in enumerate(tabs):
        off[w + 1] = off[w] + (t["C"], t["R"], t["E"], t["C"] * t["C"])
    if off[-1].max() > 2 ** 31 - 1:
        raise _unsupported_text("the worlds' tables together exceed int32 offsets")
    cat = lambda k, shape, dt: (np.concatenate([t[k].reshape(shape) for t in tabs]).astype(dt)      # noqa: E731
                                if sum(t[k].size for t in tabs) else np.zeros((1,) + tuple(shape[1:]), dt))
    return dict(n_world=len(tabs), c_stride=max(t["C"] for t in tabs), r_stride=max(1, max(t["R"] for t in tabs)),
                world_off=off.astype(np.int32), chem_f=cat("chem_f", (-1, CHEM_F), np.float64),
                sol_present=cat("sol_present", (-1,), np.uint8), sol_value=cat("sol_value", (-1,), np.float64),
                rxn_i=cat("rxn_i", (-1, RXN_I), np.int32), rxn_f=cat("rxn_f", (-1, RXN_F), np.float64),
                rxn_solv=cat("rxn_solv", (-1,), np.uint64).view(np.int64), eq_i=cat("eq_i", (-1, EQ_I), np.int32),
                eq_f=cat("eq_f", (-1, EQ_F), np.float64))
