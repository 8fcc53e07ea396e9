"""Device tables of AnyHVAC tasks: a batch of flat task dicts (task_sampler.py) -> one float64 row per task in the layout
include/xeno.h documents (XV_ANYHVAC_TASK_DOUBLES), padded to the batch's own maxima with the true counts kept.

Nothing is recomputed that the host restatement does not compute the same way: the bilinear read's cells and weights come
from host.bilinear_setup, `avg_total_heat` from host.average_total_heat, and the diffuse matrices are copied value for value
(zeros included: no packing)."""
import numpy as np

from .config import MAX_COOLERS, MAX_GRID, MAX_HEATERS, MAX_SENSORS
from .host import average_total_heat, bilinear_setup, check_settings
from .task_sampler import COOLER_PARAMS

COOLER_ROW = 24
_COOLER_COLUMNS = ("power_eff_vent", "cooler_eer_base", "cooler_eer_decay_start", "cooler_eer_zero_point",
                   "cooler_eer_reverse", "temp_diff_decay_ub", "temp_diff_decay_lb", "max_cooling_power",
                   "min_cooling_power", "power_vent_min", "power_vent_ratio", "base_bias", "delay_seconds")
assert set(_COOLER_COLUMNS) <= set(COOLER_PARAMS)


def task_doubles(NW, NL, C, S, H, KS, KH):
    """XV_ANYHVAC_TASK_DOUBLES"""
    nwall = (NW + 1) * (NL + 1) * 2
    return 16 + 3 * KH + nwall + NW * NL + S * (8 + 3 * KS) + H * (4 + 3 * KH) + H * NW * NL + C * 24 + C * NW * NL + C * nwall


def counts(task):
    return dict(nw=int(task["n_width"]), nl=int(task["n_length"]), C=len(task["cooler_loc"]), S=len(task["sensor_loc"]),
                H=len(task["heater_loc"]), KS=task["sensor_order"].shape[1], KH=task["heater_order"].shape[1])


def _nodes(loc, cell_size, nw, nl):
    sn, dn, k, nloc = bilinear_setup(loc, cell_size, nw, nl)
    return np.concatenate([sn, dn, k], axis=1).astype(np.float64), nloc


def build_tables(tasks, set_lower_bound=16, set_upper_bound=32, generate_task=False, dims=None):
    """-> dict(dims=(NW, NL, C, S, H, KS, KH), table=float64[n_task, task_doubles(*dims)], counts=[per task dict],
    avg_total_heat=[per task]).  dims: pad to these dimensions (the device sampler's) instead of the batch's own maxima."""
    cs = [counts(t) for t in tasks]
    for t in tasks:
        check_settings(control_type=t.get("control_type", "Temperature"))
    NW, NL, C, S, H, KS, KH = (max(c[k] for c in cs) for k in ("nw", "nl", "C", "S", "H", "KS", "KH"))
    if dims is not None:
        if any(a > b for a, b in zip((NW, NL, C, S, H, KS, KH), dims)):
            raise ValueError("a task exceeds the dimensions asked for: %s > %s" % ((NW, NL, C, S, H, KS, KH), tuple(dims)))
        NW, NL, C, S, H, KS, KH = (int(v) for v in dims)
    if NW > MAX_GRID or NL > MAX_GRID or C > MAX_COOLERS or S > MAX_SENSORS or H > MAX_HEATERS:
        raise ValueError("a task exceeds the device tables: %d x %d cells (<= %d), %d coolers (<= %d), %d sensors (<= %d), "
                         "%d heaters (<= %d)" % (NW, NL, MAX_GRID, C, MAX_COOLERS, S, MAX_SENSORS, H, MAX_HEATERS))
    NC, NWALL = NW * NL, (NW + 1) * (NL + 1) * 2
    table = np.zeros((len(tasks), task_doubles(NW, NL, C, S, H, KS, KH)))
    heats = []
    for row, t, c in zip(table, tasks, cs):
        nw, nl, target = c["nw"], c["nl"], float(t["target_temperature"])
        avg = 10000 if generate_task else average_total_heat(t)
        heats.append(avg)
        parts = iter(np.split(row, np.cumsum([16, 3 * KH, NWALL, NC, S * (8 + 3 * KS), H * (4 + 3 * KH), H * NC, C * 24,
                                              C * NC])))
        sc, base, chtc, hc, sens, heat, hd, cool, cd, cv = parts
        sc[:] = [nw, nl, c["C"], c["S"], c["H"], t["cell_size"], t["floor_height"], t["floorceil_chtc"], t["ambient_temp"],
                 target, avg, t["base_heater_heat_base"], t["base_heater_period"], t["base_heater_n_terms"],
                 (target - set_lower_bound) / (set_upper_bound - set_lower_bound), np.mean(target + 6)]
        base = base.reshape(3, KH)
        kh = c["KH"]
        base[0, :kh], base[1, :kh], base[2, :kh] = (t["base_heater_order"], t["base_heater_coef"][:, 0],
                                                    t["base_heater_coef"][:, 1])
        chtc.reshape(NW + 1, NL + 1, 2)[:nw + 1, :nl + 1] = t["convection_coeffs"]
        hc = hc.reshape(NW, NL)
        hc[:] = 1.0
        hc[:nw, :nl] = t["heat_capacity"]
        sens = sens.reshape(S, 8 + 3 * KS)
        n, ks = c["S"], c["KS"]
        sens[:n, :6], _ = _nodes(t["sensor_loc"], float(t["cell_size"]), nw, nl)
        sens[:, 6] = 1.0
        sens[:n, 6], sens[:n, 7] = t["sensor_period"], t["sensor_n_terms"]
        sens[:n, 8:8 + ks] = t["sensor_order"]
        sens[:n, 8 + KS:8 + KS + ks] = t["sensor_coef"][:, :, 0]
        sens[:n, 8 + 2 * KS:8 + 2 * KS + ks] = t["sensor_coef"][:, :, 1]
        heat = heat.reshape(H, 4 + 3 * KH)
        n = c["H"]
        heat[:, 2] = 1.0
        heat[:n, 0], heat[:n, 1], heat[:n, 2] = t["heater_base_factor"], t["heater_heat_base"], t["heater_period"]
        heat[:n, 3] = t["heater_n_terms"]
        heat[:n, 4:4 + kh] = t["heater_order"]
        heat[:n, 4 + KH:4 + KH + kh] = t["heater_coef"][:, :, 0]
        heat[:n, 4 + 2 * KH:4 + 2 * KH + kh] = t["heater_coef"][:, :, 1]
        hd.reshape(H, NW, NL)[:n, :nw, :nl] = t["heat_diffuse"]
        cool = cool.reshape(C, COOLER_ROW)
        n = c["C"]
        cool[:n, :6], nloc = _nodes(t["cooler_loc"], float(t["cell_size"]), nw, nl)
        cool[:n, 6:8] = nloc
        cool[:, 20] = 1.0      # (a padded row's delay: never read, never a division by zero)
        for j, k in enumerate(_COOLER_COLUMNS):
            cool[:n, 8 + j] = t["cooler_" + k]
        cd.reshape(C, NW, NL)[:n, :nw, :nl] = t["cooler_diffuse"]
        cv.reshape(C, NW + 1, NL + 1, 2)[:n, :nw + 1, :nl + 1] = t["cooler_vent_diffuse"]
    return dict(dims=(NW, NL, C, S, H, KS, KH), table=table, counts=cs, avg_total_heat=heats)
