"""Host restatement (numpy, fp64) of the device AnyHVAC task sampler (csrc/anyhvac_sampler.hip: xv_anyhvac_sample_tasks):
the same Philox counters, the same draw constructions and the same formulas in the same order.  It is what the device is
compared with (tests/test_gpu_anyhvac_sampler.py), as mazeworld/sampler_host.py and linds/sampler_host.py are for theirs.

The generative model is the reference's HVACTaskSampler (anyhvac_sampler.py, the node classes of anyhvac_utils.py,
utils/random_nn.py RandomFourier; task_sampler.py restates it for numpy's stream) under counter-based randomness: task k of
(seed, arguments) is the k-th ACCEPTED candidate in candidate order whatever the batch size — not the task numpy's stream
gives for that seed.

Departures from the reference:
  * integers, `exponential` (times its scale) and normals are host_draws' floor_int, expo and box_muller;
  * a node's x coordinate stays the reference's integer, floor(u * int(dw)); y is dl * u;
  * placement compares squared distances, d2 < min_dist * min_dist; attempt a of node i of a kind draws from (the kind's
    purpose, tick = i, sub = a) and the lowest passing attempt wins; an attempt whose cell index x / cell_size, y / cell_size
    would fall outside the grid fails; after PLACE_TRIES attempts the candidate has status `placement_cap`;
  * wind_diffuser is the fixed point of the reference's FIFO relaxation (`wind_diffuser_host`): whole-grid passes until
    nothing changes, the wall matrix from the final cell values; a unified cooler runs it once, with the base's sigma;
  * the cooler bias rejection takes at most BIAS_TRIES attempts (sub BIAS_SUB + a; 0.0 after that, never seen);
  * unification: `random.uniform` is one counter uniform; `random.sample(coolers[1:], n)` is "the n coolers of index >= 1
    with the smallest 53-bit keys, ties by index"; one cooler with 0.4 <= ratio < 0.8 is status `unify_empty`;
  * a count above the table dimensions asked for is status `too_big`; `too_big` and `unify_empty` are decided from the head
    draws, before placement;
  * an ambient draw that falls through every bucket (rounding of the running subtraction) takes the last bucket.

Counter layout (include/xeno.h): key = seed; counter = {candidate lo, candidate hi, sub, purpose | tick << 8}.  One call
gives two uniforms (words 0,1 and words 2,3 by xv_u53) or one Box-Muller pair.  Element q of a block of uniforms is half
q & 1 of call q >> 1.  Purposes (tick 0 unless said):
  0 P_HEAD     sub 0 (n_width, n_length), 1 (cell_size, floor_height), 2 (wall chtc, floorceil chtc), 3 (sensor density,
               heater density), 4 (cooler density, ambient bucket), 5 (ambient, target), 6 (drift std, unify ratio draw),
               7 (unify_ratio, -)
  1 P_CHTC     block over walls (i * (nl + 1) + j) * 2 + d of the room's own nw, nl
  2 P_HC       block over cells i * nl + j
  3 P_SENSOR_LOC, 4 P_HEATER_LOC, 5 P_COOLER_LOC   tick = node, sub = attempt: (x, y)
  6 P_SENSOR   tick = sensor: sub 0 (period, box), Fourier block from sub 1
  7 P_BASE     the base heater's curve: sub 0 (period, scale), 1 (heat_base, -), Fourier block from sub 2
  8 P_HEATER   tick = heater: the curve as P_BASE; sub 128 (sigma, base_factor), 129 (equipment heat capacity, -)
  9 P_COOLER   tick = cooler: sub 0 (power_eff_vent, eer_base), 1 (eer_decay_start, eer_zero_point), 2 (eer_reverse, sigma),
               3 (decay_ub, decay_lb), 4 (max_cooling_power, power_vent_min), 5 (fixed-ratio decision, ratio or power),
               6 (sign, delay); sub BIAS_SUB + a: the normal (cos half) of bias attempt a
 10 P_UNIFY    block over coolers: the 53-bit key of cooler q
A Fourier block from sub f: f (n_items, -); term t = 0 ... n_items at f + 1 + 4 t: + 0 (order integer, -), + 1 the order's
normal (cos half), + 2 the coefficients' normals (a: cos, b: sin), + 3 the coefficients' exponentials (a, b).
"""
import numpy as np

from ..host_draws import Draws, box_muller, expo, floor_int, uniform
from .config import DEFAULTS, MAX_COOLERS, MAX_GRID, MAX_HEATERS, MAX_SENSORS
from .host import HEAT_AVG_INTERVAL, HEAT_AVG_MAX_TIME, check_settings
from .tables import _COOLER_COLUMNS, _nodes, task_doubles
from .task_sampler import COOLER_PARAMS

STATUS = ("accepted", "placement_cap", "unify_empty", "too_big")
PLACE_TRIES = 4096
BIAS_TRIES, BIAS_SUB = 256, 16
MAX_TERMS = 16          # KS, KH of the step kernel
MAX_AMBIENT = 4
TICK_MAX = 1 << 24
DIFFUSE_CUT = 1.0e-3
COUNT_CAP = 1.0e6      # a count is capped here before it becomes an integer: far above any table, so too_big
(P_HEAD, P_CHTC, P_HC, P_SENSOR_LOC, P_HEATER_LOC, P_COOLER_LOC, P_SENSOR, P_BASE, P_HEATER, P_COOLER,
 P_UNIFY) = range(11)
PURPOSES = dict(head=P_HEAD, chtc=P_CHTC, hc=P_HC, sensor_loc=P_SENSOR_LOC, heater_loc=P_HEATER_LOC,
                cooler_loc=P_COOLER_LOC, sensor=P_SENSOR, base=P_BASE, heater=P_HEATER, cooler=P_COOLER, unify=P_UNIFY)
HEATER_EXTRA_SUB = 128
INFO_DTYPE = np.dtype([(k, "<i4") for k in ("status", "n_width", "n_length", "coolers", "sensors", "heaters", "place_max",
                                            "passes", "unified", "bias_max")])      # xv_anyhvac_cand_info
DIRS = ((-1, 0), (0, -1), (1, 0), (0, 1))
_UNIFIED = ("max_cooling_power", "power_vent_min", "min_cooling_power", "power_vent_ratio", "power_eff_vent",
            "cooler_eer_base", "cooler_eer_decay_start", "cooler_eer_zero_point", "cooler_eer_reverse",
            "cooler_diffuse_sigma")


def extras_doubles(C, S, H):
    """XV_ANYHVAC_EXTRAS: sensor_loc[S][2], heater_loc[H][2], cooler_loc[C][2], heater sigma[H], cooler sigma[C], the
    unify coefficient, the bias margin, the diffuse margin, 0"""
    return 2 * S + 3 * H + 3 * C + 4


def sampler_config(config=None):
    K = dict(DEFAULTS)
    for k, v in (config or {}).items():
        if k not in K:
            raise ValueError("unknown sampler constant %r" % (k,))
        K[k] = v
    return K


def table_dims(config=None):
    """(NW, NL, C, S, H, KS, KH): the largest counts the configuration can give, capped by what the step kernel holds"""
    K = sampler_config(config)
    NW, NL = int(K["ROOM_W_GRID_SIZE_HIGH"]) - 1, int(K["ROOM_L_GRID_SIZE_HIGH"]) - 1
    area = (NW * float(K["CELL_SIZE_HIGH"])) * (NL * float(K["CELL_SIZE_HIGH"]))
    n = [max(int(area * float(K[k + "_DENSITY_HIGH"])), 1) for k in ("COOLER", "SENSOR", "HEATER")]
    return (min(NW, MAX_GRID), min(NL, MAX_GRID), min(n[0], MAX_COOLERS), min(n[1], MAX_SENSORS), min(n[2], MAX_HEATERS),
            min(int(K["SENSOR_DRIFT_FOURIER_MAX_ITEMS"]) + 1, MAX_TERMS), min(int(K["HEAT_SOURCE_FOURIER_MAX_ITEM"]) + 1, MAX_TERMS))


def sampler_arguments(control_type='Temperature', target_temperature=None, config=None, set_lower_bound=16,
                      set_upper_bound=32, generate_task=False):
    """the arguments of a sampling call, checked: -> dict(K=the constants, dims, target, lower, upper, generate_task)"""
    check_settings(control_type=control_type)
    K = sampler_config(config)
    for k in ("ROOM_W_GRID_SIZE", "ROOM_L_GRID_SIZE"):
        if not (1 <= int(K[k + "_LOW"]) < int(K[k + "_HIGH"]) <= MAX_GRID + 1):
            raise ValueError("%s must give 1 .. %d cells" % (k, MAX_GRID))
    if len(K["AMBIENT_TEMPERATURE_HIGH"]) > MAX_AMBIENT or not K["AMBIENT_TEMPERATURE_HIGH"]:
        raise ValueError("AMBIENT_TEMPERATURE_HIGH must have 1 .. %d buckets" % MAX_AMBIENT)
    if int(K["SENSOR_DRIFT_FOURIER_MAX_ITEMS"]) + 1 > MAX_TERMS or int(K["HEAT_SOURCE_FOURIER_MAX_ITEM"]) + 1 > MAX_TERMS:
        raise ValueError("a Fourier series may have at most %d terms" % MAX_TERMS)
    hi = float(K["TARGET_TEMPERATURE_HIGH"]) if target_temperature is None else float(target_temperature)
    if not (32 - hi - 2 >= 1.0):
        raise ValueError("the target temperature must stay at or below 29 (the cooler bias is drawn within 32 - target - 2)")
    if not float(set_upper_bound) > float(set_lower_bound):
        raise ValueError("set_upper_bound must exceed set_lower_bound")
    return dict(K=K, dims=table_dims(config), target=None if target_temperature is None else float(target_temperature),
                lower=set_lower_bound, upper=set_upper_bound, generate_task=bool(generate_task))


# ---- wind_diffuser as a fixed point ----------------------------------------------------------------------------------
def _edge_weights(loc, ci, cj, cell_size, sigma):
    """exp(-distance^2) of a cell spreading from `loc` (grid units) to its four neighbours' centres and wall midpoints"""
    ec, ew = np.zeros(4), np.zeros(4)
    for d, (di, dj) in enumerate(DIRS):
        ni, nj = ci + di, cj + dj
        tx, ty = (loc[0] - (ni + 0.5)) * cell_size / sigma, (loc[1] - (nj + 0.5)) * cell_size / sigma
        ec[d] = np.exp(-(tx * tx + ty * ty))
        tx = (loc[0] - (0.5 * ni + 0.5 * ci)) * cell_size / sigma
        ty = (loc[1] - (0.5 * nj + 0.5 * cj)) * cell_size / sigma
        ew[d] = np.exp(-(tx * tx + ty * ty))
    return ec, ew


def wind_diffuser_host(cell_wall, src, cell_size, sigma, with_stats=False):
    """task_sampler.wind_diffuser's result without its queue: a cell's value is the largest product over paths from the
    source, a cell spreads iff it is the source or its final value exceeds 1e-3; the source spreads from `src`, every other
    cell from its centre (whose eight weights depend on the direction alone).  Whole-grid passes until nothing changes, then
    the walls from the final values, then numpy's own normalising sum.  -> (diffuse, wall_diffuse[, passes, margin])"""
    nx, ny = cell_wall.shape[0], cell_wall.shape[1]
    nw, nl = nx - 1, ny - 1
    cell_size, sigma = float(cell_size), float(sigma)
    g = np.asarray(src, np.float64) / cell_size
    si, sj = int(g[0]), int(g[1])
    ec_s, ew_s = _edge_weights(g, si, sj, cell_size, sigma)
    ec_c, ew_c = _edge_weights(np.array([0.5, 0.5]), 0, 0, cell_size, sigma)
    is_src = np.zeros((nw, nl), bool)
    is_src[si, sj] = True
    mat = np.zeros((nw, nl))
    mat[si, sj] = 1.0
    sl = []
    for di, dj in DIRS:      # cells c that have a neighbour n = c + (di, dj), and the wall between them
        ci = slice(max(0, -di), nw - max(0, di))
        cj = slice(max(0, -dj), nl - max(0, dj))
        ni = slice(ci.start + di, ci.stop + di)
        nj = slice(cj.start + dj, cj.stop + dj)
        wi = slice(ci.start + max(di, 0), ci.stop + max(di, 0))
        wj = slice(cj.start + max(dj, 0), cj.stop + max(dj, 0))
        sl.append((ci, cj, ni, nj, wi, wj, int(di == 0)))
    passes = 0
    while True:
        passes += 1
        spread = (mat > DIFFUSE_CUT) | is_src
        new = mat.copy()
        for d, (ci, cj, ni, nj, wi, wj, w) in enumerate(sl):
            k = np.where(is_src, ec_s[d], ec_c[d]) * mat
            k = np.where(spread, k, 0.0)[ci, cj]
            k = np.where(cell_wall[wi, wj, w], 0.0, k)
            new[ni, nj] = np.maximum(new[ni, nj], k)
        if np.array_equal(new, mat):
            break
        mat = new
    spread = (mat > DIFFUSE_CUT) | is_src
    wall = np.zeros((nx, ny, 2))
    for d, (ci, cj, ni, nj, wi, wj, w) in enumerate(sl):
        k = np.where(is_src, ew_s[d], ew_c[d]) * mat
        k = np.where(spread, k, 0.0)[ci, cj]
        k = np.where(cell_wall[wi, wj, w], 0.0, k)
        wall[wi, wj, w] = np.maximum(wall[wi, wj, w], k)
    live = mat[(mat > 0) & ~is_src]
    margin = float(np.min(np.abs(live - DIFFUSE_CUT) / DIFFUSE_CUT)) if len(live) else np.inf
    mat = mat / np.sum(mat)
    return (mat, wall, passes, margin) if with_stats else (mat, wall)


# ---- the pieces of a candidate ---------------------------------------------------------------------------------------
def place_host(d, purpose, n, dw, dl, cell_size, nw, nl, min_dist, block=32):
    """-> (loc[n, 2], attempts used per node) or (None, ...) when a node found no place within PLACE_TRIES attempts"""
    loc = np.zeros((n, 2))
    used = np.zeros(n, np.int64)
    idw, md2 = float(int(dw)), min_dist * min_dist
    for i in range(n):
        for base in range(0, PLACE_TRIES, block):
            ux, uy = d.pairs(purpose, np.arange(base, base + block), tick=i)
            x, y = np.floor(ux * idw), dl * uy
            ok = (x / cell_size < nw) & (y / cell_size < nl)
            if i:
                dx, dy = loc[None, :i, 0] - x[:, None], loc[None, :i, 1] - y[:, None]
                ok &= ~((dx * dx + dy * dy) < md2).any(axis=1)
            if ok.any():
                a = int(np.argmax(ok))
                loc[i], used[i] = (x[a], y[a]), base + a + 1
                break
        else:
            return None, used
    return loc, used


def fourier_host(d, purpose, tick, sub, max_order, max_item, box, width):
    """RandomFourier(ndim=1) -> (n_terms, order[width], coef[width, 2]), padded with zeros"""
    ua, ub = d.pairs(purpose, sub + np.arange(1 + 4 * (max_item + 1)), tick=tick)
    n_items = 1 + int(floor_int(ua[0], max_item))
    scale = box / np.sqrt(float(n_items))
    order, coef = np.zeros(width), np.zeros((width, 2))
    for t in range(n_items + 1):
        b = 1 + 4 * t
        if t:
            order[t] = (1 + int(floor_int(ua[b], max_order))) + box_muller(ua[b + 1], ub[b + 1])[0]
        za, zb = box_muller(ua[b + 2], ub[b + 2])
        coef[t] = za * (expo(ua[b + 3]) * scale), zb * (expo(ub[b + 3]) * scale)
    return n_items + 1, order, coef


def heat_curve_host(d, purpose, tick, K, width):
    (up, uh), (us, _) = d.pairs(purpose, [0, 1], tick=tick)
    lo, hi = int(K["HEAT_SOURCE_PERIOD_RANGE_LOW"]) * 60, int(K["HEAT_SOURCE_PERIOD_RANGE_HIGH"]) * 60
    period = (lo + int(floor_int(up, hi - lo))) * 60
    scale = uniform(us, K["HEAT_SOURCE_VARIANT_SCALE_LOW"], K["HEAT_SOURCE_VARIANT_SCALE_HIGH"])
    heat_base = uniform(uh, K["BASE_HEAT_SOURCE_PERIOD_RANGE_LOW"], K["BASE_HEAT_SOURCE_PERIOD_RANGE_HIGH"])
    n, order, coef = fourier_host(d, purpose, tick, 2, int(K["HEAT_SOURCE_FOURIER_MAX_ORDER"]),
                                  int(K["HEAT_SOURCE_FOURIER_MAX_ITEM"]), scale, width)
    return float(period), heat_base, n, order, coef


def _curve_power(ts, heat_base, period, n_terms, order, coef, max_power=20000):
    y = np.zeros(len(ts))
    x = ts / period
    for j in range(int(n_terms)):
        y = y + (coef[j, 0] * np.sin(order[j] * x) + coef[j, 1] * np.cos(order[j] * x))
    return np.clip(heat_base + np.clip(y, 0, None), None, max_power)


def average_heat_host(t):
    """host.average_total_heat value for value (the same operations on the same operands in the same order: heaters added
    in index order from 0, the times one after the other), evaluated heater by heater over a curve's live terms only
    instead of [H, T] passes over all KH columns — a third of the time at 270 heaters"""
    ts = np.arange(0, HEAT_AVG_MAX_TIME, HEAT_AVG_INTERVAL)
    base = _curve_power(ts, t["base_heater_heat_base"], t["base_heater_period"], t["base_heater_n_terms"],
                        t["base_heater_order"], t["base_heater_coef"])
    step_heat = np.zeros(len(ts))
    for h in range(len(t["heater_loc"])):
        own = _curve_power(ts, t["heater_heat_base"][h], t["heater_period"][h], t["heater_n_terms"][h], t["heater_order"][h],
                           t["heater_coef"][h])
        f = t["heater_base_factor"][h]
        step_heat = step_heat + (f * base + (1 - f) * own)
    return float(np.cumsum(step_heat)[-1] / len(ts))


def sample_candidate_host(seed, cand, control_type='Temperature', target_temperature=None, config=None, set_lower_bound=16,
                          set_upper_bound=32, generate_task=False, with_heat=True):
    """candidate `cand` of `seed` -> dict(status, info (an INFO_DTYPE record), task (the flat dict of task_sampler.py, None
    unless accepted), row (the XV_ANYHVAC_TASK_DOUBLES table row; all padding unless accepted), extras, bias_margin,
    diffuse_margin, unified (bool per cooler)).  with_heat=False leaves the average-heat scalar 0 (the slow part)."""
    A = sampler_arguments(control_type, target_temperature, config, set_lower_bound, set_upper_bound, generate_task)
    K, dims = A["K"], A["dims"]
    NW, NL, Cd, Sd, Hd, KS, KH = dims
    d = Draws(seed, cand)
    ua, ub = d.pairs(P_HEAD, np.arange(8))
    nw = int(K["ROOM_W_GRID_SIZE_LOW"]) + int(floor_int(ua[0], int(K["ROOM_W_GRID_SIZE_HIGH"]) - int(K["ROOM_W_GRID_SIZE_LOW"])))
    nl = int(K["ROOM_L_GRID_SIZE_LOW"]) + int(floor_int(ub[0], int(K["ROOM_L_GRID_SIZE_HIGH"]) - int(K["ROOM_L_GRID_SIZE_LOW"])))
    cell_size = uniform(ua[1], K["CELL_SIZE_LOW"], K["CELL_SIZE_HIGH"])
    floor_height = uniform(ub[1], K["FLOOR_HEIGHT_LOW"], K["FLOOR_HEIGHT_HIGH"])
    dw, dl = nw * cell_size, nl * cell_size
    area = dw * dl
    cell_volume = floor_height * cell_size * cell_size
    wall_chtc = uniform(ua[2], K["WALL_CHTC_LOW"], K["WALL_CHTC_HIGH"])
    floorceil_chtc = uniform(ub[2], K["FLOOR_CHTC_LOW"], K["FLOOR_CHTC_HIGH"])
    n_sensors = max(int(min(area * uniform(ua[3], K["SENSOR_DENSITY_LOW"], K["SENSOR_DENSITY_HIGH"]), COUNT_CAP)), 1)
    n_heaters = max(int(min(area * uniform(ub[3], K["HEATER_DENSITY_LOW"], K["HEATER_DENSITY_HIGH"]), COUNT_CAP)), 1)
    n_coolers = max(int(min(area * uniform(ua[4], K["COOLER_DENSITY_LOW"], K["COOLER_DENSITY_HIGH"]), COUNT_CAP)), 1)
    wsum = 0.0
    for _, w in K["AMBIENT_TEMPERATURE_HIGH"]:
        wsum = wsum + float(w)
    eps, t_b = ub[4] * wsum, float(K["AMBIENT_TEMPERATURE_LOW"])
    buckets = list(K["AMBIENT_TEMPERATURE_HIGH"])
    for q, (pt, w) in enumerate(buckets):
        if eps < float(w) or q == len(buckets) - 1:
            t_ambient = uniform(ua[5], t_b, pt)
            break
        eps -= float(w)
        t_b = float(pt)
    target = A["target"]
    if target is None:
        target = float(np.rint(uniform(ub[5], K["TARGET_TEMPERATURE_LOW"], K["TARGET_TEMPERATURE_HIGH"]) * 2.0) / 2.0)
    drift_std = uniform(ua[6], 1.0, 2.0)
    sample_ratio = float(ub[6])

    info = np.zeros((), INFO_DTYPE)
    info["n_width"], info["n_length"] = nw, nl
    info["coolers"], info["sensors"], info["heaters"] = n_coolers, n_sensors, n_heaters
    out = dict(task=None, bias_margin=np.inf, diffuse_margin=np.inf, unified=None)

    def done(status):
        info["status"] = status
        out.update(status=status, info=info)
        if status:
            out["row"], out["extras"] = padding_row(dims), np.zeros(extras_doubles(Cd, Sd, Hd))
            out["extras"][-3:-1] = np.inf
        return out

    if nw > NW or nl > NL or n_coolers > Cd or n_sensors > Sd or n_heaters > Hd:
        return done(3)
    if n_coolers == 1 and 0.4 <= sample_ratio < 0.8:
        return done(2)

    # convection_coeffs / heat_capacity
    nwall = (nw + 1) * (nl + 1) * 2
    chtc = uniform(d.block(P_CHTC, nwall), K["INTERNAL_CHTC_LOW"], K["INTERNAL_CHTC_HIGH"]).reshape(nw + 1, nl + 1, 2)
    hc = uniform(d.block(P_HC, nw * nl), K["GRID_HC_LOW"], K["GRID_HC_HIGH"]).reshape(nw, nl) * cell_volume
    chtc[0, :, 0] = wall_chtc
    chtc[nw, :, 0] = wall_chtc
    chtc[:, 0, 1] = wall_chtc
    chtc[:, nl, 1] = wall_chtc
    cell_walls = chtc < 5.0

    # placement
    locs, place_max = {}, 0
    for kind, purpose, n, md in (("sensor", P_SENSOR_LOC, n_sensors, 1.2), ("heater", P_HEATER_LOC, n_heaters, 1.2),
                                 ("cooler", P_COOLER_LOC, n_coolers, min(cell_size, 2.0))):
        locs[kind], used = place_host(d, purpose, n, dw, dl, cell_size, nw, nl, md)
        place_max = max(place_max, int(used.max()))
        info["place_max"] = place_max
        if locs[kind] is None:
            return done(1)

    t = dict(width=dw, length=dl, n_width=nw, n_length=nl, cell_size=cell_size, floor_height=floor_height,
             floorceil_chtc=floorceil_chtc, convection_coeffs=chtc, heat_capacity=hc, ambient_temp=t_ambient,
             control_type=control_type, target_temperature=target)
    # sensors
    t["sensor_loc"] = locs["sensor"]
    t["sensor_period"], t["sensor_n_terms"] = np.zeros(n_sensors), np.zeros(n_sensors, np.int32)
    t["sensor_order"], t["sensor_coef"] = np.zeros((n_sensors, KS)), np.zeros((n_sensors, KS, 2))
    lo, hi = int(K["SENSOR_DRIFT_PERIOD_LOW"]) * 60, int(K["SENSOR_DRIFT_PERIOD_HIGH"]) * 60
    for i in range(n_sensors):
        (up, ue), = zip(*d.pairs(P_SENSOR, [0], tick=i))
        t["sensor_period"][i] = lo + floor_int(up, hi - lo)
        box = min(expo(ue) * float(K["SENSOR_DRIFT_MEAN"]), float(K["SENSOR_DRIFT_UPPER_BOUND"]))
        t["sensor_n_terms"][i], t["sensor_order"][i], t["sensor_coef"][i] = fourier_host(
            d, P_SENSOR, i, 1, int(K["SENSOR_DRIFT_FOURIER_MAX_ORDER"]), int(K["SENSOR_DRIFT_FOURIER_MAX_ITEMS"]), box, KS)
    # heat curves
    (t["base_heater_period"], t["base_heater_heat_base"], t["base_heater_n_terms"], t["base_heater_order"],
     t["base_heater_coef"]) = heat_curve_host(d, P_BASE, 0, K, KH)
    t["heater_loc"] = locs["heater"]
    for k in ("base_factor", "heat_base", "period", "diffuse_sigma"):
        t["heater_" + k] = np.zeros(n_heaters)
    t["heater_n_terms"] = np.zeros(n_heaters, np.int32)
    t["heater_order"], t["heater_coef"] = np.zeros((n_heaters, KH)), np.zeros((n_heaters, KH, 2))
    t["heat_diffuse"] = np.zeros((n_heaters, nw, nl))
    passes, dmargin = 0, np.inf
    for i in range(n_heaters):
        (t["heater_period"][i], t["heater_heat_base"][i], t["heater_n_terms"][i], t["heater_order"][i],
         t["heater_coef"][i]) = heat_curve_host(d, P_HEATER, i, K, KH)
        (us, uf), (ue, _) = zip(*d.pairs(P_HEATER, [HEATER_EXTRA_SUB, HEATER_EXTRA_SUB + 1], tick=i))
        sigma = uniform(us, K["HEAT_SPACE_INSTANT_DIFFSION_LOW"], K["HEAT_SPACE_INSTANT_DIFFUSION_HIGH"])
        t["heater_diffuse_sigma"][i] = sigma
        t["heater_base_factor"][i] = uniform(uf, K["HEAT_SOURCE_BASE_FACTOR_LOW"], K["HEAT_SOURCE_BASE_FACTOR_HIGH"])
        t["heat_diffuse"][i], _, p, m = wind_diffuser_host(cell_walls, locs["heater"][i], cell_size, sigma, True)
        passes, dmargin = max(passes, p), min(dmargin, m)
        nloc = (locs["heater"][i] / cell_size).astype(int)
        hc[nloc[0], nloc[1]] += uniform(ue, K["EQUIPMENT_HC_LOW"], K["EQUIPMENT_HC_HIGH"])
    t["heater_timer"] = t["heater_period"].astype(np.int64)
    # coolers
    c = {k: np.zeros(n_coolers) for k in COOLER_PARAMS}
    bound = min(32 - target - 2, 6)
    bmargin, bias_max = np.inf, 0
    for i in range(n_coolers):
        ua, ub = d.pairs(P_COOLER, np.arange(7), tick=i)
        c["power_eff_vent"][i] = uniform(ua[0], K["COOLER_VENT_EFFICIENCY_LOW"], K["COOLER_VENT_EFFICIENCY_HIGH"])
        c["cooler_eer_base"][i] = uniform(ub[0], K["COOLER_EER_BASE_LOW"], K["COOLER_EER_BASE_HIGH"])
        c["cooler_eer_decay_start"][i] = uniform(ua[1], K["COOLER_EER_DECAY_START_HIGH"], K["COOLER_EER_DECAY_START_HIGH"])
        c["cooler_eer_zero_point"][i] = uniform(ub[1], K["COOLER_EER_ZERO_POINT_LOW"], K["COOLER_EER_ZERO_POINT_HIGH"])
        c["cooler_eer_reverse"][i] = uniform(ua[2], K["COOLER_EER_REVERSE_LOW"], K["COOLER_EER_REVERSE_HIGH"])
        c["cooler_diffuse_sigma"][i] = uniform(ub[2], K["COOLER_SPACE_INSTANT_DIFFUSION_LOW"],
                                                K["COOLER_SPACE_INSTANT_DIFFUSION_HIGH"])
        c["temp_diff_decay_ub"][i] = uniform(ua[3], K["COOLER_DIFF_DECAY_UB_LOW"], K["COOLER_DIFF_DECAY_UB_HIGH"])
        c["temp_diff_decay_lb"][i] = uniform(ub[3], K["COOLER_DIFF_DECAY_LB_LOW"], K["COOLER_DIFF_DECAY_LB_HIGH"])
        c["max_cooling_power"][i] = uniform(ua[4], K["COOLER_MAX_COOLING_POWER_LOW"], K["COOLER_MAX_COOLING_POWER_HIGH"])
        c["power_vent_min"][i] = uniform(ub[4], K["COOLER_POWER_VENT_MIN_LOW"], K["COOLER_POWER_VENT_MIN_HIGH"])
        c["min_cooling_power"][i] = c["power_vent_min"][i]
        if ua[5] < float(K["COOLER_VENT_FIXED_RATIO_FACTOR"]):
            c["power_vent_ratio"][i] = uniform(ub[5], K["COOLER_VENT_FIXED_RATIO_LOW"], K["COOLER_VENT_FIXED_RATIO_HIGH"])
        else:
            c["power_vent_ratio"][i] = 0.0
            c["power_vent_min"][i] = uniform(ub[5], K["COOLER_VENT_FIXED_POWER_LOW"], K["COOLER_VENT_FIXED_POWER_HIGH"])
        sample = 0.0
        for base in range(0, BIAS_TRIES, 16):
            za, zb = d.pairs(P_COOLER, BIAS_SUB + np.arange(base, base + 16), tick=i)
            s = float(K["COOLER_SENSOR_BIAS_MEAN"]) + drift_std * box_muller(za, zb)[0]
            ok = (-bound <= s) & (s <= bound)
            n_eval = int(np.argmax(ok)) + 1 if ok.any() else 16
            bmargin = min(bmargin, float(np.min(np.abs(np.abs(s[:n_eval]) - bound) / bound)))
            if ok.any():
                sample = float(s[n_eval - 1])
                bias_max = max(bias_max, base + n_eval)
                break
        c["base_bias"][i] = abs(sample) if ua[6] < float(K["COOLER_SENSOR_SIGN_POSITIVE_PROB"]) else -abs(sample)
        c["delay_seconds"][i] = uniform(ub[6], K["COOLER_SENSOR_DELAY_LOW"], K["COOLER_SENSOR_DELAY_HIGH"])
    # unification
    unified, coefficient = np.zeros(n_coolers, bool), 0.0
    if sample_ratio < 0.4:
        unified[:] = True
        coefficient = 1
    elif sample_ratio < 0.8:
        n_to_unify = max(1, int((n_coolers - 1) * uniform(float(d.pairs(P_HEAD, [7])[0][0]), 0.7, 1.0)))
        q = np.arange(n_coolers)
        ka, kb = d.ints53(P_UNIFY, q >> 1)
        keys = np.where(q & 1, kb, ka)
        rank = np.argsort(keys[1:], kind="stable")      # equal keys: the lower index first
        unified[1 + rank[:n_to_unify]] = True
        coefficient = (n_to_unify + 1) / n_coolers
    for k in _UNIFIED:
        c[k][unified] = c[k][0]
    t["unify_cooler_coefficent"] = coefficient
    t["cooler_loc"] = locs["cooler"]
    for k in COOLER_PARAMS:
        t["cooler_" + k] = c[k]
    t["cooler_diffuse"] = np.zeros((n_coolers, nw, nl))
    t["cooler_vent_diffuse"] = np.zeros((n_coolers, nw + 1, nl + 1, 2))
    for i in range(n_coolers):
        t["cooler_diffuse"][i], t["cooler_vent_diffuse"][i], p, m = wind_diffuser_host(
            cell_walls, locs["cooler"][i], cell_size, c["cooler_diffuse_sigma"][i], True)
        passes, dmargin = max(passes, p), min(dmargin, m)
    info["passes"], info["unified"], info["bias_max"] = passes, int(unified.sum()), bias_max
    avg = 10000.0 if generate_task else (average_heat_host(t) if with_heat else 0.0)
    out.update(task=t, bias_margin=bmargin, diffuse_margin=dmargin, unified=unified, avg_total_heat=avg)
    out["row"] = pack_row(t, dims, avg, set_lower_bound, set_upper_bound)
    ex = np.zeros(extras_doubles(Cd, Sd, Hd))
    parts = np.split(ex, np.cumsum([2 * Sd, 2 * Hd, 2 * Cd, Hd, Cd]))
    parts[0][:2 * n_sensors] = locs["sensor"].reshape(-1)
    parts[1][:2 * n_heaters] = locs["heater"].reshape(-1)
    parts[2][:2 * n_coolers] = locs["cooler"].reshape(-1)
    parts[3][:n_heaters], parts[4][:n_coolers] = t["heater_diffuse_sigma"], c["cooler_diffuse_sigma"]
    parts[5][:3] = coefficient, bmargin, dmargin
    out["extras"] = ex
    return done(0)


def _split(row, dims):
    NW, NL, C, S, H, KS, KH = dims
    NC, NWALL = NW * NL, (NW + 1) * (NL + 1) * 2
    sc, base, chtc, hc, sens, heat, hd, cool, cd, cv = np.split(
        row, np.cumsum([16, 3 * KH, NWALL, NC, S * (8 + 3 * KS), H * (4 + 3 * KH), H * NC, C * 24, C * NC]))
    return dict(scalars=sc, base=base.reshape(3, KH), chtc=chtc.reshape(NW + 1, NL + 1, 2), hc=hc.reshape(NW, NL),
                sensors=sens.reshape(S, 8 + 3 * KS), heaters=heat.reshape(H, 4 + 3 * KH), heat_diffuse=hd.reshape(H, NW, NL),
                coolers=cool.reshape(C, 24), cooler_diffuse=cd.reshape(C, NW, NL),
                cooler_vent_diffuse=cv.reshape(C, NW + 1, NL + 1, 2))


def row_parts(row, dims):
    """views of one table row by the layout of include/xeno.h"""
    assert row.shape == (task_doubles(*dims),)
    return _split(row, dims)


def padding_row(dims):
    """what tables.build_tables leaves where a task has nothing: heat capacity 1, periods 1, a cooler's delay 1, zeros"""
    row = np.zeros(task_doubles(*dims))
    p = _split(row, dims)
    p["hc"][:] = 1.0
    p["sensors"][:, 6] = 1.0
    p["heaters"][:, 2] = 1.0
    p["coolers"][:, 20] = 1.0
    return row


def pack_row(t, dims, avg, set_lower_bound=16, set_upper_bound=32):
    """the flat task dict -> its table row at the dimensions `dims` (the layout of include/xeno.h)"""
    row = padding_row(dims)
    p = _split(row, dims)
    nw, nl = int(t["n_width"]), int(t["n_length"])
    nC, nS, nH = len(t["cooler_loc"]), len(t["sensor_loc"]), len(t["heater_loc"])
    KS, KH = dims[5], dims[6]
    target = float(t["target_temperature"])
    p["scalars"][:] = [nw, nl, nC, nS, nH, t["cell_size"], t["floor_height"], t["floorceil_chtc"], t["ambient_temp"], target,
                       avg, t["base_heater_heat_base"], t["base_heater_period"], t["base_heater_n_terms"],
                       (target - set_lower_bound) / (set_upper_bound - set_lower_bound), target + 6]
    p["base"][0], p["base"][1], p["base"][2] = t["base_heater_order"], t["base_heater_coef"][:, 0], t["base_heater_coef"][:, 1]
    p["chtc"][:nw + 1, :nl + 1] = t["convection_coeffs"]
    p["hc"][:nw, :nl] = t["heat_capacity"]
    s = p["sensors"]
    s[:nS, :6], _ = _nodes(t["sensor_loc"], float(t["cell_size"]), nw, nl)
    s[:nS, 6], s[:nS, 7] = t["sensor_period"], t["sensor_n_terms"]
    s[:nS, 8:8 + KS], s[:nS, 8 + KS:8 + 2 * KS] = t["sensor_order"], t["sensor_coef"][:, :, 0]
    s[:nS, 8 + 2 * KS:] = t["sensor_coef"][:, :, 1]
    h = p["heaters"]
    h[:nH, 0], h[:nH, 1], h[:nH, 2], h[:nH, 3] = (t["heater_base_factor"], t["heater_heat_base"], t["heater_period"],
                                                  t["heater_n_terms"])
    h[:nH, 4:4 + KH], h[:nH, 4 + KH:4 + 2 * KH], h[:nH, 4 + 2 * KH:] = (t["heater_order"], t["heater_coef"][:, :, 0],
                                                                        t["heater_coef"][:, :, 1])
    p["heat_diffuse"][:nH, :nw, :nl] = t["heat_diffuse"]
    c = p["coolers"]
    c[:nC, :6], nloc = _nodes(t["cooler_loc"], float(t["cell_size"]), nw, nl)
    c[:nC, 6:8] = nloc
    for j, k in enumerate(_COOLER_COLUMNS):
        c[:nC, 8 + j] = t["cooler_" + k]
    p["cooler_diffuse"][:nC, :nw, :nl] = t["cooler_diffuse"]
    p["cooler_vent_diffuse"][:nC, :nw + 1, :nl + 1] = t["cooler_vent_diffuse"]
    return row


def sample_rows_host(seed, cand_base, n, **kwargs):
    """candidates [cand_base, cand_base + n) -> dict(dims, table[n, doubles], extras[n, ...], info[n], status[n],
    tasks (flat dicts, None where not accepted), bias_margin[n], diffuse_margin[n])"""
    cs = [sample_candidate_host(seed, cand_base + i, **kwargs) for i in range(n)]
    return dict(dims=table_dims(kwargs.get("config")), table=np.stack([c["row"] for c in cs]),
                extras=np.stack([c["extras"] for c in cs]), info=np.array([c["info"] for c in cs], INFO_DTYPE),
                status=np.array([c["status"] for c in cs], np.int32), tasks=[c["task"] for c in cs],
                bias_margin=np.array([c["bias_margin"] for c in cs]),
                diffuse_margin=np.array([c["diffuse_margin"] for c in cs]), candidates=cs)

