"""ChemVerse fixtures (scripts/gen_golden_chemverse.py) and the comparison the host and device tests share.

A fixture is one of the reference's evaluation worlds (tests/golden/chemverse_world_<tag>.json, copied byte for byte) and 128
experiments on it with the reference's own results (chemverse_runs_<tag>.npz), recorded unrounded.  The wide fixtures are
made the same way on two larger worlds: h, a world of the reference's "hard" sampler (51 chemicals, 95 reactions), and x, a
world at every table limit built from world c; they also record which experiment took which branch.  `long` is one experiment
of 4,096 steps on world a.

The comparison, and where its figures come from — all measured on the reference, none on the code under test:
  * discrete outcomes (fired counts, step counts, converged, failure code and step, history / log steps and counts, the set of
    species above 1e-9) must be EQUAL for every experiment the fixture marks `stable`: one whose discrete outcomes stayed the
    same when the reference itself ran with exp and log moved by up to 2 ulp, and under other string-hash seeds.  At most 2 %
    of a fixture may be unstable; the tests assert that.
  * floats: the HOST restatement uses the reference's own operations and must be bit-identical on every experiment marked
    `order_free` (its recorded values did not depend on the hash seed, which orders one sum of the reference,
    simulator.py:369-371) and within the device bound elsewhere.  The DEVICE has other exp / log / pow (documented at 1-2 ulp):
    per element |device - reference| <= max(16 * spread, 2^-46 * max(|x|, 1)), spread being the largest deviation the
    reference showed under the perturbed runs.  16: eight random runs underestimate the extreme, `**` could not be perturbed
    in the reference, and the device's functions are themselves 1-2 ulp off; 2^-46 (128 ulp of a value near 1) covers the
    elements whose spread happened to be zero.
  * the reference's result dicts list amounts above 1e-9 only (simulator.py:863-876, :841-842), so the recorded totals and log
    rows are zero at or below it; the arrays under test hold the unfiltered sums and are filtered the same way here first.
"""
import json
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TAGS = ("a", "b", "c")
WIDE_TAGS = ("h", "x")      # a sampled "hard" world beyond 64 reactions and 32 chemicals; a world at every table limit
LONG = "long"               # one experiment of 4,096 steps on world a
PER_CHEM = ("final_pool", "consumed", "produced", "byproduct", "gas_lost")
FLOATS = PER_CHEM + ("final_T", "final_P", "hist_T", "hist_P", "log_T", "log_P", "log_consumed", "log_produced")
DISCRETE = ("fired", "num_steps", "steps_run", "converged", "failure", "failure_step", "hist_step", "hist_count", "log_step",
            "log_active", "log_count")
LOG_KEYS = ("log_step", "log_active", "log_T", "log_P", "log_consumed", "log_produced", "log_count")
N_LOG = 32
_cache = {}


def fixture(tag):
    """-> dict(world=the JSON dict, tab=its tables, runs=the npz as a dict, n)"""
    if tag not in _cache:
        from xenoverse_amd.chemverse import build_tables
        with open(os.path.join(GOLD, "chemverse_world_%s.json" % ("a" if tag == LONG else tag))) as f:
            world = json.load(f)
        with np.load(os.path.join(GOLD, "chemverse_runs_%s.npz" % tag)) as z:
            runs = {k: z[k] for k in z.files}
        for v in runs.values():
            v.setflags(write=False)
        _cache[tag] = dict(world=world, tab=build_tables(world), runs=runs, n=len(runs["num_steps"]))
    return _cache[tag]


def amounts_of(fx, i):
    """experiment i's initial amounts as a dict id -> grams in the recorded key order"""
    r, ids = fx["runs"], fx["tab"]["chem_ids"]
    return {ids[c]: float(r["grams"][i, c]) for c in r["order"][i, :r["n_initial"][i]]}


def host_experiment(fx, i, world=0):
    r = fx["runs"]
    return dict(world=world, amounts=[(int(c), float(r["grams"][i, c])) for c in r["order"][i, :r["n_initial"][i]]],
                temperature_C=float(r["temperature_C"][i]), pressure_atm=float(r["pressure_atm"][i]),
                duration_s=float(r["duration_s"][i]), equipment=int(r["equipment"][i]),
                heating_rate_C_per_s=float(r["heating_rate_C_per_s"][i]), vessel_volume_L=float(r["vessel_volume_L"][i]))


def call_args(fx, i):
    """experiment i as simulate_chain_reaction's keyword arguments"""
    r = fx["runs"]
    return dict(initial_amounts_g=amounts_of(fx, i), temperature_C=float(r["temperature_C"][i]),
                pressure_atm=float(r["pressure_atm"][i]), duration_s=float(r["duration_s"][i]),
                equipment=fx["tab"]["equip_names"][int(r["equipment"][i])],
                heating_rate_C_per_s=float(r["heating_rate_C_per_s"][i]), vessel_volume_L=float(r["vessel_volume_L"][i]))


def recorded_dicts(fx):
    """[(experiment index, the reference's own rounded result dict)]"""
    return json.loads(bytes(fx["runs"]["dicts_json"]).decode())


def rows(key, n):
    """the experiments a recorded array covers: the reaction log is kept for the first N_LOG only"""
    return min(n, N_LOG) if key in LOG_KEYS else n


def branch_hits(fx):
    """the wide fixtures record which experiment took which branch of the reference: -> name -> bool[n]"""
    names = json.loads(bytes(fx["runs"]["branch_names_json"]).decode())
    return {b: fx["runs"]["branch_hits"][:, k] for k, b in enumerate(names)}


def unstable_fraction(fx):
    return float((~fx["runs"]["stable"]).mean())


def compare(fx, got, sel=None, exact=False, keys=None, label=""):
    """got: name -> array [n, ...] (a world's own widths or wider) for the fixture's experiments `sel` (default all, in
    order).  Discrete outcomes equal where stable; floats bit-identical where order_free (exact=True: the host) or within the
    bound.  -> the largest ratio of deviation to bound seen (0 where everything was bit-identical)."""
    r, n = fx["runs"], fx["n"]
    sel = np.arange(n) if sel is None else np.asarray(sel)
    C, R = fx["tab"]["C"], fx["tab"]["R"]
    worst = 0.0
    stable = r["stable"][sel]

    def cut(key, a):      # a wider batch pads chemical / reaction columns with zeros
        a = np.asarray(a)
        width = R if key == "fired" else (C if key in PER_CHEM or key in ("log_consumed", "log_produced") else None)
        if width is not None and a.shape[-1] != width:
            assert not a[..., width:].any(), "%s%s: non-zero beyond the world's columns" % (label, key)
            a = a[..., :width]
        if width is not None and key != "fired":      # the reference reports amounts above 1e-9 only; the arrays hold all
            a = np.where(a > 1e-9, a, 0.0)
        return a

    for key in (keys or DISCRETE + FLOATS):
        if key not in got:
            continue
        m = sel < rows(key, n)
        if not m.any():
            continue
        ref, g = r[key][sel[m]], cut(key, got[key])[m]
        assert g.shape == ref.shape, "%s%s: shape %s, expected %s" % (label, key, g.shape, ref.shape)
        if key in DISCRETE:
            bad = (g != ref).reshape(len(ref), -1).any(axis=1) & stable[m]
            assert not bad.any(), "%s%s differs for experiments %s" % (label, key, sel[m][bad].tolist())
            continue
        above = ((g > 1e-9) != (ref > 1e-9)).reshape(len(ref), -1).any(axis=1) & stable[m]
        if key in PER_CHEM:
            assert not above.any(), "%s%s: other species above 1e-9 for experiments %s" % (label, key, sel[m][above].tolist())
        live = stable[m]
        if exact:
            of = r["order_free"][sel[m]]
            same = (g.view(np.uint64) == ref.view(np.uint64)).reshape(len(ref), -1).all(axis=1)
            bad = ~same & of
            assert not bad.any(), "%s%s is not bit-identical for experiments %s" % (label, key, sel[m][bad].tolist())
            live = live & ~of
        spread = r["spread_" + key][sel[m]]
        bound = np.maximum(16.0 * spread, 2.0 ** -46 * np.maximum(np.abs(ref), 1.0))
        ratio = np.abs(g - ref) / bound
        ratio = ratio.reshape(len(ref), -1).max(axis=1)
        ratio = np.where(live, ratio, 0.0)
        if len(ratio):
            k = int(np.argmax(ratio))
            worst = max(worst, float(ratio[k]))
            assert ratio[k] <= 1.0, "%s%s: experiment %d deviates %.3g times its bound" % (label, key, sel[m][k], ratio[k])
    return worst
