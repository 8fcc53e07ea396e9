"""HVACTaskSampler — the reference's anyhvac task sampler (anyhvac_sampler.py with the node classes of anyhvac_utils.py and
utils/random_nn.py:RandomFourier) restated to return this project's kind of task: a dict of scalars and flat arrays, no
objects.

It draws from numpy's GLOBAL stream and Python's `random` in the reference's order, so after
`numpy.random.seed(s); random.seed(s)` it returns the reference's task bit for bit.  The reference's `print`s are not
reproduced.  Kept as they are in the reference:
  * a cooler's `min_cooling_power` is the FIRST draw of `power_vent_min`, also when `power_vent_min` is drawn again;
  * `cooler_eer_decay_start` is uniform(HIGH, HIGH);
  * a heat curve's `heat_base` is drawn between the BASE_HEAT_SOURCE_PERIOD_RANGE bounds;
  * with ONE cooler and 0.4 <= sample_ratio < 0.8 the unification asks `random.sample` for one of zero coolers and raises
    ValueError (numpy / random seed 5 at a 5 x 5 room of 1.0-1.05 m cells is such a seed).  So does this port.

Task keys (C coolers, S sensors, H heaters, nw x nl cells, KS / KH = most Fourier terms of a sensor / heat curve, the
constant term included; rows are padded with order 0, coefficient 0 up to them and `*_n_terms` keeps the count):
  width, length, n_width, n_length, cell_size, floor_height, floorceil_chtc, ambient_temp, target_temperature,
  control_type, unify_cooler_coefficent, heater_timer[H], convection_coeffs[nw+1, nl+1, 2], heat_capacity[nw, nl],
  sensor_loc[S, 2], sensor_period[S], sensor_n_terms[S], sensor_order[S, KS], sensor_coef[S, KS, 2],
  base_heater_heat_base, base_heater_period, base_heater_n_terms, base_heater_order[KH], base_heater_coef[KH, 2],
  heater_loc[H, 2], heater_base_factor[H], heater_heat_base[H], heater_period[H], heater_n_terms[H],
  heater_order[H, KH], heater_coef[H, KH, 2], heater_diffuse_sigma[H], heat_diffuse[H, nw, nl],
  cooler_loc[C, 2], cooler_<p>[C] for p in COOLER_PARAMS, cooler_diffuse[C, nw, nl], cooler_vent_diffuse[C, nw+1, nl+1, 2].
A heater's `heat_vent_diffuse` is never used by the reference and is left out.
"""
import random

import numpy as np
from numpy import random as rnd

from ..random_nn import RandomFourier
from .config import DEFAULTS

COOLER_PARAMS = ("power_eff_vent", "cooler_eer_base", "cooler_eer_decay_start", "cooler_eer_zero_point",
                 "cooler_eer_reverse", "cooler_diffuse_sigma", "temp_diff_decay_ub", "temp_diff_decay_lb",
                 "max_cooling_power", "min_cooling_power", "power_vent_min", "power_vent_ratio", "base_bias",
                 "delay_seconds")
_UNIFIED = ("max_cooling_power", "power_vent_min", "min_cooling_power", "power_vent_ratio", "power_eff_vent",
            "cooler_eer_base", "cooler_eer_decay_start", "cooler_eer_zero_point", "cooler_eer_reverse",
            "cooler_diffuse_sigma")


def wind_diffuser(cell_wall, src, cell_size, sigma):
    """-> (diffuse[nw, nl], wall_diffuse[nw+1, nl+1, 2]): breadth-first spread of a source at `src` (metres) over the cells
    that no wall separates, with weight exp(-(distance / sigma)^2) per hop times the weight of the cell it came from; a cell
    keeps the largest weight offered and spreads on while it is above 1e-3.  The cell matrix is normalised to sum 1."""
    nx, ny = cell_wall.shape[0], cell_wall.shape[1]
    src_grid = src / cell_size
    mat = np.zeros((nx - 1, ny - 1))
    wall = np.zeros((nx, ny, 2))
    mat[int(src_grid[0]), int(src_grid[1])] = 1.0
    queue = [src_grid]
    while queue:
        loc = queue.pop(0)
        ci, cj = int(loc[0]), int(loc[1])
        for di, dj in ((-1, 0), (0, -1), (1, 0), (0, 1)):
            ni, nj = ci + di, cj + dj
            if ni < 0 or nj < 0 or ni >= nx - 1 or nj >= ny - 1:
                continue
            wi, wj, w = ci + max(di, 0), cj + max(dj, 0), int(di == 0)
            if cell_wall[wi, wj, w]:
                continue
            dist = np.sum(((loc - np.array([ni + 0.5, nj + 0.5])) * cell_size / sigma) ** 2)
            k = np.exp(-dist) * mat[ci, cj]
            if k > mat[ni, nj]:
                mat[ni, nj] = k
                if k > 1.0e-3:
                    queue.append(np.array([ni + 0.5, nj + 0.5]))
            dist = np.sum(((loc - np.array([0.5 * ni + 0.5 * ci, 0.5 * nj + 0.5 * cj])) * cell_size / sigma) ** 2)
            k = np.exp(-dist) * mat[ci, cj]
            if k > wall[wi, wj, w]:
                wall[wi, wj, w] = k
    mat /= np.sum(mat)
    return mat, wall


def _place(dw, dl, others, min_dist):
    """a node's location: redrawn while it is closer than min_dist to one placed before"""
    loc = np.array([rnd.randint(0, dw), rnd.uniform(0, dl)])
    if others:
        while True:
            mdist = 1e+10
            for o in others:
                dist = ((o - loc) ** 2).sum() ** 0.5
                if dist < mdist:
                    mdist = dist
            if mdist < min_dist:
                loc = np.array([rnd.randint(0, dw), rnd.uniform(0, dl)])
            else:
                break
    return loc


def _fourier(max_order, max_item, box_size):
    """RandomFourier(ndim=1) over numpy's global stream: [(order, (a, b))], the first term of order 0"""
    return RandomFourier(ndim=1, max_order=max_order, max_item=max_item, box_size=box_size).coeffs


def _heat_curve(K):
    period = rnd.randint(K["HEAT_SOURCE_PERIOD_RANGE_LOW"] * 60, K["HEAT_SOURCE_PERIOD_RANGE_HIGH"] * 60) * 60
    scale = rnd.uniform(K["HEAT_SOURCE_VARIANT_SCALE_LOW"], K["HEAT_SOURCE_VARIANT_SCALE_HIGH"])
    heat_base = rnd.uniform(K["BASE_HEAT_SOURCE_PERIOD_RANGE_LOW"], K["BASE_HEAT_SOURCE_PERIOD_RANGE_HIGH"])
    terms = _fourier(K["HEAT_SOURCE_FOURIER_MAX_ORDER"], K["HEAT_SOURCE_FOURIER_MAX_ITEM"], scale)
    return dict(period=period, heat_base=heat_base, terms=terms)


def _pack_terms(rows, width):
    n = np.array([len(r) for r in rows], np.int32)
    order = np.zeros((len(rows), width))
    coef = np.zeros((len(rows), width, 2))
    for i, r in enumerate(rows):
        for j, (o, c) in enumerate(r):
            order[i, j] = o
            coef[i, j] = np.asarray(c, np.float64).reshape(2)
    return n, order, coef


def _flatten(room, sensors, base_heater, heaters, coolers):
    ks = max(len(s["terms"]) for s in sensors)
    kh = max([len(base_heater["terms"])] + [len(h["terms"]) for h in heaters])
    t = dict(room)
    t["heater_timer"] = np.array([h["period"] for h in heaters], np.int64)
    t["sensor_loc"] = np.array([s["loc"] for s in sensors], np.float64)
    t["sensor_period"] = np.array([s["period"] for s in sensors], np.float64)
    t["sensor_n_terms"], t["sensor_order"], t["sensor_coef"] = _pack_terms([s["terms"] for s in sensors], ks)
    n, o, c = _pack_terms([base_heater["terms"]], kh)
    t["base_heater_heat_base"] = float(base_heater["heat_base"])
    t["base_heater_period"] = float(base_heater["period"])
    t["base_heater_n_terms"], t["base_heater_order"], t["base_heater_coef"] = int(n[0]), o[0], c[0]
    t["heater_loc"] = np.array([h["loc"] for h in heaters], np.float64)
    for k in ("base_factor", "heat_base", "period", "diffuse_sigma"):
        t["heater_" + k] = np.array([h[k] for h in heaters], np.float64)
    t["heater_n_terms"], t["heater_order"], t["heater_coef"] = _pack_terms([h["terms"] for h in heaters], kh)
    t["heat_diffuse"] = np.array([h["heat_diffuse"] for h in heaters], np.float64)
    t["cooler_loc"] = np.array([c["loc"] for c in coolers], np.float64)
    for k in COOLER_PARAMS:
        t["cooler_" + k] = np.array([c[k] for c in coolers], np.float64)
    t["cooler_diffuse"] = np.array([c["cooler_diffuse"] for c in coolers], np.float64)
    t["cooler_vent_diffuse"] = np.array([c["cooler_vent_diffuse"] for c in coolers], np.float64)
    return t


def HVACTaskSampler(control_type='Temperature', target_temperature=None, config=None):
    """one AnyHVAC task (module docstring).  Raises ValueError for control_type='Power' (not built here) and — as the
    reference does — for a one-cooler room whose `random.uniform` draw falls in [0.4, 0.8)."""
    if str(control_type).lower() != "temperature":
        raise ValueError("control_type=%r is not supported: only control_type='Temperature' is built" % (control_type,))
    K = dict(DEFAULTS)
    for k, v in (config or {}).items():
        if k not in K:
            raise ValueError("unknown sampler constant %r" % (k,))
        K[k] = v
    nw = rnd.randint(K["ROOM_W_GRID_SIZE_LOW"], K["ROOM_W_GRID_SIZE_HIGH"])
    nl = rnd.randint(K["ROOM_L_GRID_SIZE_LOW"], K["ROOM_L_GRID_SIZE_HIGH"])
    cell_size = rnd.uniform(K["CELL_SIZE_LOW"], K["CELL_SIZE_HIGH"])
    floor_height = rnd.uniform(K["FLOOR_HEIGHT_LOW"], K["FLOOR_HEIGHT_HIGH"])
    dw, dl = nw * cell_size, nl * cell_size
    area = dw * dl
    cell_volume = floor_height * cell_size * cell_size
    chtc = rnd.uniform(K["INTERNAL_CHTC_LOW"], K["INTERNAL_CHTC_HIGH"], size=(nw + 1, nl + 1, 2))
    hc = rnd.uniform(K["GRID_HC_LOW"], K["GRID_HC_HIGH"], size=(nw, nl)) * cell_volume
    wall_chtc = rnd.uniform(K["WALL_CHTC_LOW"], K["WALL_CHTC_HIGH"])
    chtc[0, :, 0] = wall_chtc
    chtc[nw, :, 0] = wall_chtc
    chtc[:, 0, 1] = wall_chtc
    chtc[:, nl, 1] = wall_chtc
    cell_walls = chtc < 5.0
    floorceil_chtc = rnd.uniform(K["FLOOR_CHTC_LOW"], K["FLOOR_CHTC_HIGH"])
    n_sensors = max(int(area * rnd.uniform(K["SENSOR_DENSITY_LOW"], K["SENSOR_DENSITY_HIGH"])), 1)
    n_heaters = max(int(area * rnd.uniform(K["HEATER_DENSITY_LOW"], K["HEATER_DENSITY_HIGH"])), 1)
    n_coolers = max(int(area * rnd.uniform(K["COOLER_DENSITY_LOW"], K["COOLER_DENSITY_HIGH"])), 1)

    eps = rnd.uniform(0.0, sum(w for _, w in K["AMBIENT_TEMPERATURE_HIGH"]))
    t_b = K["AMBIENT_TEMPERATURE_LOW"]
    for pt, w in K["AMBIENT_TEMPERATURE_HIGH"]:
        if eps < w:
            t_ambient = rnd.uniform(t_b, pt)
            break
        eps -= w
        t_b = pt
    if target_temperature is None:
        target_temperature = round(rnd.uniform(K["TARGET_TEMPERATURE_LOW"], K["TARGET_TEMPERATURE_HIGH"]) * 2) / 2
    drift_std = rnd.uniform(1, 2)

    sensors, heaters, coolers = [], [], []
    for _ in range(n_sensors):
        loc = _place(dw, dl, [s["loc"] for s in sensors], 1.2)
        period = rnd.randint(K["SENSOR_DRIFT_PERIOD_LOW"] * 60, K["SENSOR_DRIFT_PERIOD_HIGH"] * 60)
        box = min(rnd.exponential(scale=K["SENSOR_DRIFT_MEAN"]), K["SENSOR_DRIFT_UPPER_BOUND"])
        sensors.append(dict(loc=loc, period=period, terms=_fourier(K["SENSOR_DRIFT_FOURIER_MAX_ORDER"],
                                                                    K["SENSOR_DRIFT_FOURIER_MAX_ITEMS"], box)))
    base_heater = _heat_curve(K)
    for _ in range(n_heaters):
        loc = _place(dw, dl, [h["loc"] for h in heaters], 1.2)
        sigma = rnd.uniform(K["HEAT_SPACE_INSTANT_DIFFSION_LOW"], K["HEAT_SPACE_INSTANT_DIFFUSION_HIGH"])
        diffuse, _ = wind_diffuser(cell_walls, loc, cell_size, sigma)
        base_factor = rnd.uniform(K["HEAT_SOURCE_BASE_FACTOR_LOW"], K["HEAT_SOURCE_BASE_FACTOR_HIGH"])
        h = _heat_curve(K)
        h.update(loc=loc, diffuse_sigma=sigma, heat_diffuse=diffuse, base_factor=base_factor)
        heaters.append(h)
        nloc = (loc / cell_size).astype(int)
        hc[nloc[0], nloc[1]] += rnd.uniform(K["EQUIPMENT_HC_LOW"], K["EQUIPMENT_HC_HIGH"])
    for _ in range(n_coolers):
        c = dict(loc=_place(dw, dl, [q["loc"] for q in coolers], min(cell_size, 2.0)))
        c["power_eff_vent"] = rnd.uniform(K["COOLER_VENT_EFFICIENCY_LOW"], K["COOLER_VENT_EFFICIENCY_HIGH"])
        c["cooler_eer_base"] = rnd.uniform(K["COOLER_EER_BASE_LOW"], K["COOLER_EER_BASE_HIGH"])
        c["cooler_eer_decay_start"] = rnd.uniform(K["COOLER_EER_DECAY_START_HIGH"], K["COOLER_EER_DECAY_START_HIGH"])
        c["cooler_eer_zero_point"] = rnd.uniform(K["COOLER_EER_ZERO_POINT_LOW"], K["COOLER_EER_ZERO_POINT_HIGH"])
        c["cooler_eer_reverse"] = rnd.uniform(K["COOLER_EER_REVERSE_LOW"], K["COOLER_EER_REVERSE_HIGH"])
        c["cooler_diffuse_sigma"] = rnd.uniform(K["COOLER_SPACE_INSTANT_DIFFUSION_LOW"],
                                                K["COOLER_SPACE_INSTANT_DIFFUSION_HIGH"])
        c["cooler_diffuse"], c["cooler_vent_diffuse"] = wind_diffuser(cell_walls, c["loc"], cell_size,
                                                                      c["cooler_diffuse_sigma"])
        c["temp_diff_decay_ub"] = rnd.uniform(K["COOLER_DIFF_DECAY_UB_LOW"], K["COOLER_DIFF_DECAY_UB_HIGH"])
        c["temp_diff_decay_lb"] = rnd.uniform(K["COOLER_DIFF_DECAY_LB_LOW"], K["COOLER_DIFF_DECAY_LB_HIGH"])
        c["max_cooling_power"] = rnd.uniform(K["COOLER_MAX_COOLING_POWER_LOW"], K["COOLER_MAX_COOLING_POWER_HIGH"])
        c["power_vent_min"] = rnd.uniform(K["COOLER_POWER_VENT_MIN_LOW"], K["COOLER_POWER_VENT_MIN_HIGH"])
        c["min_cooling_power"] = c["power_vent_min"]
        if rnd.random() < K["COOLER_VENT_FIXED_RATIO_FACTOR"]:
            c["power_vent_ratio"] = rnd.uniform(K["COOLER_VENT_FIXED_RATIO_LOW"], K["COOLER_VENT_FIXED_RATIO_HIGH"])
        else:
            c["power_vent_ratio"] = 0.0
            c["power_vent_min"] = rnd.uniform(K["COOLER_VENT_FIXED_POWER_LOW"], K["COOLER_VENT_FIXED_POWER_HIGH"])
        # the return-air sensor: bias by rejection sampling inside +-bound, then the sign, then the transport delay
        bound = min(32 - target_temperature - 2, 6)
        while True:
            sample = rnd.normal(K["COOLER_SENSOR_BIAS_MEAN"], drift_std)
            if -bound <= sample <= bound:
                c["base_bias"] = abs(sample) if rnd.random() < K["COOLER_SENSOR_SIGN_POSITIVE_PROB"] else -abs(sample)
                break
        c["delay_seconds"] = rnd.uniform(K["COOLER_SENSOR_DELAY_LOW"], K["COOLER_SENSOR_DELAY_HIGH"])
        coolers.append(c)

    def unify(base, c):
        for k in _UNIFIED:
            c[k] = base[k]
        c["cooler_diffuse"], c["cooler_vent_diffuse"] = wind_diffuser(cell_walls, c["loc"], cell_size,
                                                                      c["cooler_diffuse_sigma"])

    unified = 0
    sample_ratio = random.uniform(0.0, 1.0)
    if sample_ratio < 0.4:
        for c in coolers:
            unify(coolers[0], c)
        unified = 1
    elif sample_ratio < 0.8:
        unify_ratio = random.uniform(0.7, 1.0)
        n_to_unify = max(1, int((n_coolers - 1) * unify_ratio))
        for c in random.sample(coolers[1:], n_to_unify):      # one cooler: a sample of 1 from none -> ValueError
            unify(coolers[0], c)
        unified = (n_to_unify + 1) / n_coolers

    room = dict(width=dw, length=dl, n_width=nw, n_length=nl, cell_size=cell_size, floor_height=floor_height,
                floorceil_chtc=floorceil_chtc, convection_coeffs=chtc, heat_capacity=hc, ambient_temp=t_ambient,
                control_type=control_type, target_temperature=target_temperature, unify_cooler_coefficent=unified)
    return _flatten(room, sensors, base_heater, heaters, coolers)


def task_from_reference(task):
    """a task of reference OBJECTS (what the reference's HVACTaskSampler returns) -> this project's flat task dict, by
    attribute access only"""
    def curve(hc):
        return dict(period=hc.period, heat_base=hc.heat_base, terms=list(hc.heat_periodical.coeffs))

    sensors = [dict(loc=s.loc, period=s.drift_periodical.max_steps, terms=list(s.drift_periodical.coeffs))
               for s in task["sensors"]]
    heaters = []
    for h in task["equipments"]:
        d = curve(h.heat_curve)
        d.update(loc=h.loc, diffuse_sigma=h.heat_diffuse_sigma, heat_diffuse=h.heat_diffuse, base_factor=h.base_factor)
        heaters.append(d)
    coolers = []
    for c in task["coolers"]:
        d = {k: getattr(c, k) for k in COOLER_PARAMS[:-2]}
        d.update(loc=c.loc, base_bias=c.cooler_sensor_drift.base_bias, delay_seconds=c.cooler_sensor_drift.delay_seconds,
                 cooler_diffuse=c.cooler_diffuse, cooler_vent_diffuse=c.cooler_vent_diffuse)
        coolers.append(d)
    room = {k: task[k] for k in ("width", "length", "n_width", "n_length", "cell_size", "floor_height", "floorceil_chtc",
                                 "convection_coeffs", "heat_capacity", "ambient_temp", "control_type",
                                 "target_temperature", "unify_cooler_coefficent")}
    return _flatten(room, sensors, curve(task["equipments"][0].base_heater), heaters, coolers)
