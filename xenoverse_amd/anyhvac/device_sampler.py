"""AnyHVAC task sampling on the GPU: `sample_tasks_device` returns n accepted tasks as the float64 table rows
`HVACVecEnv.set_task` takes as they are (no host copy), made by `xv_anyhvac_sample_tasks` (csrc/anyhvac_sampler.hip), one
256-lane workgroup per candidate.

Same generative model as the reference's HVACTaskSampler with counter-based randomness: task k of (seed, arguments) is the
k-th ACCEPTED candidate in candidate order, a pure function of those arguments whatever the batch size — but not the task
numpy's stream gives for that seed (for that, the host sampler `HVACTaskSampler`).  Departures, counters and statuses:
anyhvac/sampler_host.py (the numpy restatement the device is tested against) and DESIGN.md §3.8.0.
"""
import ctypes as C
import time

import numpy as np
import torch

from .. import _lib
from ..device_sampling import collect_accepted, engine_scope, sampler_stats
from . import sampler_host as sh
from .tables import _COOLER_COLUMNS, task_doubles

STATUS = sh.STATUS
INFO_DTYPE = sh.INFO_DTYPE
KEYS = ("table", "extras")
BATCH_BYTES = 1 << 30      # what one launch's rows may take (a default-configuration row is about 3.2 MB)

# XV_ANYHVAC_R_* (include/xeno.h), in order: (LOW key, HIGH key) of config.DEFAULTS
RANGES = (("CELL_SIZE_LOW", "CELL_SIZE_HIGH"), ("FLOOR_HEIGHT_LOW", "FLOOR_HEIGHT_HIGH"),
          ("INTERNAL_CHTC_LOW", "INTERNAL_CHTC_HIGH"), ("WALL_CHTC_LOW", "WALL_CHTC_HIGH"),
          ("FLOOR_CHTC_LOW", "FLOOR_CHTC_HIGH"), ("GRID_HC_LOW", "GRID_HC_HIGH"), ("EQUIPMENT_HC_LOW", "EQUIPMENT_HC_HIGH"),
          ("SENSOR_DENSITY_LOW", "SENSOR_DENSITY_HIGH"), ("HEATER_DENSITY_LOW", "HEATER_DENSITY_HIGH"),
          ("COOLER_DENSITY_LOW", "COOLER_DENSITY_HIGH"), ("TARGET_TEMPERATURE_LOW", "TARGET_TEMPERATURE_HIGH"),
          ("HEAT_SPACE_INSTANT_DIFFSION_LOW", "HEAT_SPACE_INSTANT_DIFFUSION_HIGH"),
          ("COOLER_SPACE_INSTANT_DIFFUSION_LOW", "COOLER_SPACE_INSTANT_DIFFUSION_HIGH"),
          ("COOLER_VENT_EFFICIENCY_LOW", "COOLER_VENT_EFFICIENCY_HIGH"), ("COOLER_EER_BASE_LOW", "COOLER_EER_BASE_HIGH"),
          ("COOLER_EER_DECAY_START_HIGH", "COOLER_EER_DECAY_START_HIGH"),      # the reference draws uniform(HIGH, HIGH)
          ("COOLER_EER_ZERO_POINT_LOW", "COOLER_EER_ZERO_POINT_HIGH"), ("COOLER_EER_REVERSE_LOW", "COOLER_EER_REVERSE_HIGH"),
          ("COOLER_DIFF_DECAY_UB_LOW", "COOLER_DIFF_DECAY_UB_HIGH"), ("COOLER_DIFF_DECAY_LB_LOW", "COOLER_DIFF_DECAY_LB_HIGH"),
          ("COOLER_MAX_COOLING_POWER_LOW", "COOLER_MAX_COOLING_POWER_HIGH"),
          ("COOLER_POWER_VENT_MIN_LOW", "COOLER_POWER_VENT_MIN_HIGH"),
          ("COOLER_VENT_FIXED_RATIO_LOW", "COOLER_VENT_FIXED_RATIO_HIGH"),
          ("COOLER_VENT_FIXED_POWER_LOW", "COOLER_VENT_FIXED_POWER_HIGH"),
          ("COOLER_SENSOR_DELAY_LOW", "COOLER_SENSOR_DELAY_HIGH"),
          ("HEAT_SOURCE_BASE_FACTOR_LOW", "HEAT_SOURCE_BASE_FACTOR_HIGH"),
          ("HEAT_SOURCE_VARIANT_SCALE_LOW", "HEAT_SOURCE_VARIANT_SCALE_HIGH"),
          ("BASE_HEAT_SOURCE_PERIOD_RANGE_LOW", "BASE_HEAT_SOURCE_PERIOD_RANGE_HIGH"))      # heat_base: kept as the reference has it


class Params(C.Structure):   # xv_anyhvac_sampler_params (include/xeno.h)
    _fields_ = [(k, C.c_int32) for k in ("nw_lo", "nw_hi", "nl_lo", "nl_hi", "n_ambient", "has_target", "generate_task",
                                         "sensor_period_lo", "sensor_period_hi", "heat_period_lo", "heat_period_hi",
                                         "sensor_max_order", "sensor_max_items", "heat_max_order", "heat_max_item",
                                         "reserved")] + \
               [("ambient_low", C.c_double), ("ambient_pt", C.c_double * 4), ("ambient_w", C.c_double * 4)] + \
               [(k, C.c_double) for k in ("target", "set_lower", "set_upper", "sensor_drift_mean", "sensor_drift_ub",
                                          "vent_fixed_factor", "bias_mean", "sign_prob")] + \
               [("range", (C.c_double * 2) * len(RANGES))]


def params_of(a):
    """sampler_host.sampler_arguments' result -> xv_anyhvac_sampler_params"""
    K, p = a["K"], Params()
    p.nw_lo, p.nw_hi = int(K["ROOM_W_GRID_SIZE_LOW"]), int(K["ROOM_W_GRID_SIZE_HIGH"])
    p.nl_lo, p.nl_hi = int(K["ROOM_L_GRID_SIZE_LOW"]), int(K["ROOM_L_GRID_SIZE_HIGH"])
    buckets = list(K["AMBIENT_TEMPERATURE_HIGH"])
    p.n_ambient = len(buckets)
    for q, (pt, w) in enumerate(buckets[:4]):
        p.ambient_pt[q], p.ambient_w[q] = float(pt), float(w)
    p.ambient_low = float(K["AMBIENT_TEMPERATURE_LOW"])
    p.has_target, p.target = (0, 0.0) if a["target"] is None else (1, float(a["target"]))
    p.generate_task = 1 if a["generate_task"] else 0
    p.sensor_period_lo, p.sensor_period_hi = int(K["SENSOR_DRIFT_PERIOD_LOW"]), int(K["SENSOR_DRIFT_PERIOD_HIGH"])
    p.heat_period_lo, p.heat_period_hi = int(K["HEAT_SOURCE_PERIOD_RANGE_LOW"]), int(K["HEAT_SOURCE_PERIOD_RANGE_HIGH"])
    p.sensor_max_order, p.sensor_max_items = int(K["SENSOR_DRIFT_FOURIER_MAX_ORDER"]), int(K["SENSOR_DRIFT_FOURIER_MAX_ITEMS"])
    p.heat_max_order, p.heat_max_item = int(K["HEAT_SOURCE_FOURIER_MAX_ORDER"]), int(K["HEAT_SOURCE_FOURIER_MAX_ITEM"])
    p.set_lower, p.set_upper = float(a["lower"]), float(a["upper"])
    p.sensor_drift_mean, p.sensor_drift_ub = float(K["SENSOR_DRIFT_MEAN"]), float(K["SENSOR_DRIFT_UPPER_BOUND"])
    p.vent_fixed_factor = float(K["COOLER_VENT_FIXED_RATIO_FACTOR"])
    p.bias_mean, p.sign_prob = float(K["COOLER_SENSOR_BIAS_MEAN"]), float(K["COOLER_SENSOR_SIGN_POSITIVE_PROB"])
    for r, (lo, hi) in enumerate(RANGES):
        p.range[r][0], p.range[r][1] = float(K[lo]), float(K[hi])
    return p


def sample_candidates(engine, seed, cand_base, n_cand, info=False, **sampler_kwargs):
    """One launch over candidates [cand_base, cand_base + n_cand).  -> dict with `dims`, `table` float64[n_cand, doubles],
    `extras` float64[n_cand, ...] (device; all padding where status != 0), `status` int32[n_cand] (device) and, with info,
    the per-candidate records on the host.  Keyword arguments: sample_tasks_device's sampler arguments."""
    a = sh.sampler_arguments(**sampler_kwargs)
    d = engine.device
    dims = a["dims"]
    out = dict(dims=dims,
               table=torch.empty((n_cand, task_doubles(*dims)), dtype=torch.float64, device=d),
               extras=torch.empty((n_cand, sh.extras_doubles(dims[2], dims[3], dims[4])), dtype=torch.float64, device=d),
               status=torch.empty(n_cand, dtype=torch.int32, device=d))
    raw = torch.zeros((n_cand, INFO_DTYPE.itemsize), dtype=torch.uint8, device=d) if info else None
    p = params_of(a)
    _lib.check(engine.lib.xv_anyhvac_sample_tasks(engine.handle, int(seed) & (2**64 - 1), int(cand_base), int(n_cand),
                                                  *[int(v) for v in dims], C.cast(C.byref(p), C.c_void_p),
                                                  _lib.ptr(out["table"]), _lib.ptr(out["extras"]), _lib.ptr(raw),
                                                  _lib.ptr(out["status"])))
    engine.sync()
    if info:
        out["info"] = raw.cpu().numpy().view(INFO_DTYPE).reshape(n_cand)
    return out


def default_batch(n_tasks, dims):
    """candidates per launch: bounded by the bytes of their rows"""
    row_bytes = 8 * (task_doubles(*dims) + sh.extras_doubles(dims[2], dims[3], dims[4]))
    return int(max(1, min(4096, max(16, n_tasks), BATCH_BYTES // row_bytes)))


def sample_tasks_device(n_tasks, seed=0, control_type='Temperature', target_temperature=None, config=None,
                        set_lower_bound=16, set_upper_bound=32, generate_task=False, engine=None, device="cuda:0", batch=None,
                        max_candidates=None):
    """n_tasks accepted tasks -> dict(dims, table (device float64 rows), extras, counts (device int32 [n, 5]: n_width,
    n_length, coolers, sensors, heaters), info (host records), stats) + what `HVACVecEnv.set_task` checks against its own
    settings: set_lower_bound, set_upper_bound, generate_task, delay_high (the configuration's COOLER_SENSOR_DELAY_HIGH).
    Task k is the k-th accepted candidate in candidate order, whatever `batch` is."""
    kw = dict(control_type=control_type, target_temperature=target_temperature, config=config,
              set_lower_bound=set_lower_bound, set_upper_bound=set_upper_bound, generate_task=generate_task)
    a = sh.sampler_arguments(**kw)
    if batch is None:
        batch = default_batch(n_tasks, a["dims"])
    with engine_scope(engine, device) as eng:
        t0 = time.perf_counter()
        got, info, hist = collect_accepted(lambda base, n: sample_candidates(eng, seed, base, n, info=True, **kw),
                                           n_tasks, batch, KEYS, STATUS, max_candidates)
        out = dict(dims=a["dims"], **got)
        out["counts"] = got["table"][:, :5].to(torch.int32).contiguous()
        out["info"] = info
        out.update(set_lower_bound=set_lower_bound, set_upper_bound=set_upper_bound, generate_task=bool(generate_task),
                   delay_high=float(a["K"]["COOLER_SENSOR_DELAY_HIGH"]), control_type=control_type)
        eng.sync()
        out["stats"] = sampler_stats(hist, STATUS, batch, t0)
        return out


def task_dicts_from_device(tables):
    """device (or host) tables of sample_tasks_device -> flat task dicts in the task_sampler.py schema, arrays cut back to
    the true counts (Fourier rows keep the tables' KS / KH).  Locations and sigmas come from `extras`, everything else from
    the row; `build_tables(dicts, ..., dims=tables["dims"])` reproduces the rows except for the average-heat scalar."""
    def host(v):
        return v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)

    dims = tuple(int(v) for v in tables["dims"])
    NW, NL, Cd, Sd, Hd, KS, KH = dims
    table, extras = host(tables["table"]), host(tables["extras"])
    tasks = []
    for row, ex in zip(table, extras):
        p = sh.row_parts(row, dims)
        sloc, hloc, cloc, hsig, csig, tail = np.split(ex, np.cumsum([2 * Sd, 2 * Hd, 2 * Cd, Hd, Cd]))
        sc = p["scalars"]
        nw, nl, nC, nS, nH = (int(v) for v in sc[:5])
        cs = float(sc[5])
        t = dict(width=nw * cs, length=nl * cs, n_width=nw, n_length=nl, cell_size=cs, floor_height=float(sc[6]),
                 floorceil_chtc=float(sc[7]), ambient_temp=float(sc[8]), target_temperature=float(sc[9]),
                 control_type=tables.get("control_type", "Temperature"), unify_cooler_coefficent=float(tail[0]),
                 convection_coeffs=p["chtc"][:nw + 1, :nl + 1].copy(), heat_capacity=p["hc"][:nw, :nl].copy())
        s = p["sensors"][:nS]
        t.update(sensor_loc=sloc.reshape(Sd, 2)[:nS].copy(), sensor_period=s[:, 6].copy(), sensor_n_terms=s[:, 7].astype(np.int32),
                 sensor_order=s[:, 8:8 + KS].copy(), sensor_coef=np.stack([s[:, 8 + KS:8 + 2 * KS], s[:, 8 + 2 * KS:]], axis=2))
        t.update(base_heater_heat_base=float(sc[11]), base_heater_period=float(sc[12]), base_heater_n_terms=int(sc[13]),
                 base_heater_order=p["base"][0].copy(), base_heater_coef=np.stack([p["base"][1], p["base"][2]], axis=1))
        h = p["heaters"][:nH]
        t.update(heater_loc=hloc.reshape(Hd, 2)[:nH].copy(), heater_base_factor=h[:, 0].copy(), heater_heat_base=h[:, 1].copy(),
                 heater_period=h[:, 2].copy(), heater_timer=h[:, 2].astype(np.int64), heater_n_terms=h[:, 3].astype(np.int32),
                 heater_order=h[:, 4:4 + KH].copy(), heater_coef=np.stack([h[:, 4 + KH:4 + 2 * KH], h[:, 4 + 2 * KH:]], axis=2),
                 heater_diffuse_sigma=hsig[:nH].copy(), heat_diffuse=p["heat_diffuse"][:nH, :nw, :nl].copy())
        c = p["coolers"][:nC]
        t["cooler_loc"] = cloc.reshape(Cd, 2)[:nC].copy()
        for j, k in enumerate(_COOLER_COLUMNS):
            t["cooler_" + k] = c[:, 8 + j].copy()
        t["cooler_cooler_diffuse_sigma"] = csig[:nC].copy()
        t["cooler_diffuse"] = p["cooler_diffuse"][:nC, :nw, :nl].copy()
        t["cooler_vent_diffuse"] = p["cooler_vent_diffuse"][:nC, :nw + 1, :nl + 1].copy()
        tasks.append(t)
    return tasks
