"""HVACHost — the reference's base HVACEnv (anyhvac_env.py:8-651, control_type='Temperature', no_switch_action=True, box
actions) restated over this project's flat task dict: numpy and fp64, the reference's arithmetic in the reference's order
and dtypes, one env per object (a batch is a list of them).  It is pinned bit for bit to recorded runs of the reference
(tests/golden/anyhvac_*.npz) and is the yardstick of the device kernel (csrc/anyhvac.hip).

What one step does:
  * the resting cooler rotates when it has rested for MORE than 3600 s (checked with the step's starting t);
  * heater powers, and with them the static heat of every cell, are evaluated once at the step's starting t;
  * `iter_per_step` inner iterations: every cooler reads its return temperature (bilinear read of the grid, then the
    delay queue and low-pass filter of its sensor — they run for the resting cooler too), its proportional controller
    and EER give the cooling and ventilation power, the coolers' effects are added in index order, the 5-point stencil
    advances the grid, and t += sec_per_iter;
  * t is rounded half away from zero; observation, reward and flags follow from the new grid and t.
float32 appears where the reference has it: the clipped action, the set temperature, the energy accumulator, avg_power,
the observations, and the reward's target term.  The accumulator follows numpy's promotion of the reference's operands:
where the controller's ratio is interpolated the power is a numpy.float64 and power * dt is added in fp64, the sum rounded
back to float32; where the ratio is clamped to 0 or 1, or the cooler rests, the power is a Python float (the sampler's
draws are Python floats), which numpy rounds to float32 BEFORE a float32 addition.

The episode protocol of the reference's RL trainer (run_rl.py:38-48) is three setters, as there: set_random_start_t,
set_generate_record, set_overheat_no_termiated_training_only.  reset() then follows anyhvac_env.py:301-323 branch for
branch (see reset), every failing step remembers its time, every other step appends the resting cooler's index to a
history the restart-before-failure branch reads 100 entries back.  BoundedHistory is the device's form of that history
(a ring and a saturating count); tests/test_host_anyhvac_start.py proves it against the literal list.
"""
import numpy as np

from .config import RING_CAPACITY

EXCLUDED = dict(control_type="Temperature", no_switch_action=True, action_space_format="box",
                include_switch_in_observation=False, return_normilized_obs=False, random_start_t=False,
                generate_record=False, overheat_no_termiated_training_only=False)
REST_SECONDS = 3600
FAILURE_REWARD, OVERHEAT_REWARD, ENERGY_WHT, TARGET_WHT, BASE_REWARD, WARNING_TOLERANCE = -30, -10, -3.0, -0.5, 1.0, 5
HEAT_AVG_INTERVAL, HEAT_AVG_MAX_TIME = 30, 604800
HISTORY_LENGTH, STEPS_BACK = 1000, 100      # the reference's cap of the history, and how far a restart goes back
HISTORY_RING = 128                          # what the device keeps of it (include/xeno.h XV_ANYHVAC_HISTORY)
HISTORY_WRAP = 1024 + HISTORY_RING
START_RANDOM, START_RECORD, START_NO_TERMINATE = 1, 2, 4      # include/xeno.h XV_ANYHVAC_START_*
SETTERS = ("random_start_t", "generate_record", "overheat_no_termiated_training_only")


def check_settings(**settings):
    """the settings this project does not build raise a ValueError that names them"""
    for k, v in settings.items():
        if k not in EXCLUDED:
            raise TypeError("unknown setting %r" % (k,))
        ok = EXCLUDED[k]
        same = (str(v).lower() == ok.lower()) if isinstance(ok, str) else (bool(v) == ok)
        if not same:
            hint = " as a keyword (the reference has none either): call set_%s()" % k if k in SETTERS else ""
            raise ValueError("%s=%r is not supported by xenoverse_amd.anyhvac%s (only %s=%r is built)" % (k, v, hint, k, ok))


def check_ring(delay_seconds, sec_per_iter):
    """a cooler's delay queue holds at most delay / sec_per_iter + 2 entries; the device ring has RING_CAPACITY"""
    need = float(np.max(delay_seconds)) / float(sec_per_iter) + 2
    if need > RING_CAPACITY:
        raise ValueError("sec_per_iter=%g needs %d delay-queue entries for a sensor delay of %.3g s; the ring holds %d"
                         % (sec_per_iter, int(need), float(np.max(delay_seconds)), RING_CAPACITY))


def bilinear_setup(loc, cell_size, nw, nl):
    """-> (sn[n, 2], dn[n, 2], k[n, 2], nloc[n, 2]): the clipped cell pairs and weights of the read at cloc - nloc - 0.5"""
    cloc = np.asarray(loc, np.float64) / cell_size
    nloc = cloc.astype(int)
    d_loc = cloc - nloc - 0.5
    sgrid = np.floor(d_loc).astype(int) + nloc
    hi = np.array([nw - 1, nl - 1])
    sn = np.clip(sgrid, 0, hi)
    dn = np.clip(sgrid + 1, 0, hi)
    return sn, dn, d_loc - np.floor(d_loc), nloc


def fourier(order, coef, n_terms, x):
    """rows of Fourier series at x: sum over a row's terms, one after the other from 0, of a sin(order x) + b cos(order x).
    order[R, K], coef[R, K, 2], n_terms[R]; x[R] -> [R], x[R, T] -> [R, T]"""
    x = np.asarray(x, np.float64)
    wide = (slice(None), None) if x.ndim == 2 else (slice(None),)
    n_terms = np.asarray(n_terms)[wide]
    y = np.zeros(x.shape)
    for j in range(order.shape[1]):
        o, a, b = order[:, j][wide], coef[:, j, 0][wide], coef[:, j, 1][wide]
        y = np.where(j < n_terms, y + (a * np.sin(o * x) + b * np.cos(o * x)), y)
    return y


def heat_curve_power(heat_base, period, n_terms, order, coef, t, max_power):
    """rows of heat curves at time(s) t (a scalar or [T]): base + the positive part of the series, capped"""
    t = np.asarray(t)
    wide = (slice(None), None) if t.ndim else (slice(None),)
    heat_base, period = np.asarray(heat_base, np.float64)[wide], np.asarray(period, np.float64)[wide]
    y = fourier(order, coef, n_terms, (t[None] if t.ndim else t) / period)
    return np.clip(heat_base + np.clip(y, 0, None), None, max_power)


def heater_powers(task, t, max_power=20000):
    """the power of every heater at time(s) t: [H] for a scalar t, [H, T] for t[T]"""
    base = heat_curve_power([task["base_heater_heat_base"]], [task["base_heater_period"]], [task["base_heater_n_terms"]],
                            task["base_heater_order"][None], task["base_heater_coef"][None], t, max_power)
    own = heat_curve_power(task["heater_heat_base"], task["heater_period"], task["heater_n_terms"], task["heater_order"],
                           task["heater_coef"], t, max_power)
    f = task["heater_base_factor"]
    if own.ndim == 2:
        f = f[:, None]
    return f * base + (1 - f) * own


def average_total_heat(task):
    """the reference's running sum over arange(0, 604800, 30) in its order of addition: per time the heaters are added in
    index order starting from 0, the times are added one after the other — as H + 1 numpy passes over the 20,160 times"""
    ts = np.arange(0, HEAT_AVG_MAX_TIME, HEAT_AVG_INTERVAL)
    p = heater_powers(task, ts)
    step_heat = np.zeros(len(ts))
    for h in range(p.shape[0]):
        step_heat = step_heat + p[h]
    return float(np.cumsum(step_heat)[-1] / len(ts))      # cumsum adds sequentially


def start_cdf(max_t):
    """the table numpy.random.choice(arange(max_t + 1), p=weights) searches, formed with the reference's own expressions
    (anyhvac_env.py:320-321) and numpy's (cdf = p.cumsum(); cdf /= cdf[-1]): float64 [max_t + 1]"""
    weights = 1.0 / ((np.arange(max_t + 1) + 1) ** 2)
    weights = weights / weights.sum()
    cdf = weights.cumsum()
    cdf /= cdf[-1]
    return cdf


def choice_from_cdf(cdf, u):
    """numpy's choice on its uniform u: the number of entries <= u"""
    return int(np.searchsorted(cdf, u, side="right"))


def inverse_start(u, max_t):
    """anyhvac_env.py:315-317 on its uniform u"""
    start_ratio = 1 - np.sqrt(1 - u)
    return int(start_ratio * max_t)


def start_t_probability(cdf, max_t, lo, hi):
    """P(lo <= t <= hi) of the reference's mixed start draw (no record, no failure behind it): half the inverse-CDF
    branch — t = int((1 - sqrt(1 - u)) max_t) >= a exactly when u >= 1 - (1 - a / max_t)^2, up to a rounding on u's
    2^-53 grid — and half the choice branch, whose probabilities are the table's differences"""
    def inv_at_least(a):
        return 1.0 if a <= 0 else (0.0 if a >= max_t else (1.0 - a / max_t) ** 2)
    below = float(cdf[lo - 1]) if lo > 0 else 0.0
    return 0.5 * (inv_at_least(lo) - inv_at_least(hi + 1)) + 0.5 * (float(cdf[min(hi, len(cdf) - 1)]) - below)


class BoundedHistory(object):
    """the reference's cooler_state_history as the device keeps it.  The reference appends one rest index per step that
    does not fail, pops the oldest beyond 1,000 entries, and reads ONE entry, at index max(0, len - 100): the 100th
    newest once there are 100, the oldest since the last clear before.  Both lie among the last 100 appends, so a ring of
    128 entries (int16: a room has up to 320 coolers) and the number of appends since the clear give the same entry.  The
    count need not run on for ever: from 1152 it steps back by one ring, which keeps count % 128 — the next slot — and
    keeps it >= 1000, so min(count, 1000) is the reference's len."""

    def __init__(self):
        self.ring = np.zeros(HISTORY_RING, np.int16)
        self.count = 0

    def clear(self):
        self.count = 0

    def append(self, rest_idx):
        self.ring[self.count & (HISTORY_RING - 1)] = rest_idx
        self.count = self.count + 1 - HISTORY_RING if self.count + 1 >= HISTORY_WRAP else self.count + 1

    def __len__(self):
        return min(self.count, HISTORY_LENGTH)

    def restore(self, steps_back=STEPS_BACK):
        """-> the entry at max(0, len - steps_back), None when empty"""
        if self.count == 0:
            return None
        at = self.count - steps_back if self.count >= steps_back else 0
        return int(self.ring[at & (HISTORY_RING - 1)])


class ListHistory(object):
    """the reference's list, literally (_save / _restore / _reset_cooler_state_history): what HVACHost keeps"""

    def __init__(self):
        self.items = []

    def clear(self):
        self.items = []

    def append(self, rest_idx):
        self.items.append(rest_idx)
        if len(self.items) > HISTORY_LENGTH:
            self.items.pop(0)

    def __len__(self):
        return len(self.items)

    def restore(self, steps_back=STEPS_BACK):
        if len(self.items) > 0:
            return self.items[max(0, len(self.items) - steps_back)]
        return None


class HVACHost(object):
    def __init__(self, max_steps=20160, iter_per_step=200, sec_per_iter=0.15, set_lower_bound=16, set_upper_bound=32,
                 reward_mode=0, include_heat_in_observation=True, include_last_action_in_observation=True,
                 include_timestep_in_observation=True, **excluded):
        check_settings(**excluded)
        if reward_mode not in (0, 1, 2):
            raise ValueError("reward_mode must be 0, 1 or 2")
        self.max_steps, self.iter_per_step, self.sec_per_iter = max_steps, int(iter_per_step), sec_per_iter
        self.lower_bound, self.upper_bound, self.reward_mode = set_lower_bound, set_upper_bound, reward_mode
        self.include = (bool(include_heat_in_observation), bool(include_last_action_in_observation),
                        bool(include_timestep_in_observation))
        self.task_set = False
        self.random_start_t = self.generate_record = self.overheat_no_termiated_training_only = False
        self.last_fail_timestemp = -1
        self.history = ListHistory()      # cooler_state_history['current_rest_cooler_idx']
        self.t = 0.0                      # (the reference's reset reads self.t only behind last_fail > 0)

    def set_random_start_t(self, random_start_t):
        self.random_start_t = random_start_t

    def set_generate_record(self, generate_record):
        self.generate_record = generate_record

    def set_overheat_no_termiated_training_only(self, overheat_no_termiated_training_only):
        self.overheat_no_termiated_training_only = overheat_no_termiated_training_only

    def _start_cdf(self):
        if getattr(self, "_cdf", (None, None))[0] != self.max_t:
            self._cdf = (self.max_t, start_cdf(self.max_t))
        return self._cdf[1]

    def set_task(self, task, generate_task=False):
        check_settings(control_type=task.get("control_type", "Temperature"))
        check_ring(task["cooler_delay_seconds"], self.sec_per_iter)
        self.task = task
        self.nw, self.nl = int(task["n_width"]), int(task["n_length"])
        for k in ("cell_size", "floor_height", "floorceil_chtc", "ambient_temp", "target_temperature"):
            setattr(self, k, float(task[k]))
        self.convection_coeffs = np.asarray(task["convection_coeffs"], np.float64)
        self.heat_capacity = np.asarray(task["heat_capacity"], np.float64)
        self.n_coolers, self.n_sensors = len(task["cooler_loc"]), len(task["sensor_loc"])
        self.n_heaters = len(task["heater_loc"])
        self.failure_upperbound = np.mean(self.target_temperature + 6)
        self.csa = self.cell_size * self.floor_height
        self.avg_total_heat = 10000 if generate_task else average_total_heat(task)
        self._sensor = bilinear_setup(task["sensor_loc"], self.cell_size, self.nw, self.nl)
        sn, dn, k, nloc = bilinear_setup(task["cooler_loc"], self.cell_size, self.nw, self.nl)
        p = {q: [float(v) for v in task["cooler_" + q]] for q in
             ("power_eff_vent", "cooler_eer_base", "cooler_eer_decay_start", "cooler_eer_zero_point", "cooler_eer_reverse",
              "temp_diff_decay_ub", "temp_diff_decay_lb", "max_cooling_power", "min_cooling_power", "power_vent_min",
              "power_vent_ratio", "base_bias", "delay_seconds")}
        self._cooler = [dict(sn=(int(sn[i, 0]), int(sn[i, 1])), dn=(int(dn[i, 0]), int(dn[i, 1])),
                             k=(float(k[i, 0]), float(k[i, 1])), nloc=(int(nloc[i, 0]), int(nloc[i, 1])),
                             D=np.asarray(task["cooler_diffuse"][i], np.float64),
                             V=np.asarray(task["cooler_vent_diffuse"][i], np.float64),
                             **{q: p[q][i] for q in p}) for i in range(self.n_coolers)]
        self.task_set = True

    # -- episode --------------------------------------------------------------------------------------------------
    def reset(self, state=None, start_u=None):
        """state: the initial grid [nw, nl] (tests inject the recorded one); None draws ambient + 2 N(0, 1) from numpy's
        global stream, as the reference does.  start_u: (u0, u1), the uniforms of the start draw (under generate_record
        u1 alone: k = floor(u1 max_steps)); None takes them from numpy's global stream with the reference's own calls.
        Under random_start_t, anyhvac_env.py:301-323 in its order: generate_record -> a uniform step, the history
        emptied; a failure behind and t < max_t -> 100 steps before it, with the rest index of 100 history entries ago;
        else the history emptied and the mixed draw.  Without it t = 0 and cooler 0 rests; the history is not touched."""
        if state is None:
            state = np.full((self.nw, self.nl), self.ambient_temp) + np.random.normal(0, 2.0, (self.nw, self.nl))
        self.state = np.array(state, np.float64).reshape(self.nw, self.nl)
        self.max_t = int(self.max_steps * self.iter_per_step * self.sec_per_iter)
        rest = 0
        if self.random_start_t:
            if self.generate_record:
                k = np.random.randint(0, self.max_steps) if start_u is None else int(np.floor(start_u[1] * self.max_steps))
                self.t = k * self.iter_per_step * self.sec_per_iter
                self.history.clear()
            elif self.last_fail_timestemp > 0 and self.t < self.max_t:
                self.t = max(0, self.last_fail_timestemp - STEPS_BACK * self.iter_per_step * self.sec_per_iter)
                if len(self.history) > 0:
                    rest = self.history.restore(STEPS_BACK)
            else:
                self.history.clear()
                if (np.random.random() if start_u is None else start_u[0]) < 0.5:
                    self.t = inverse_start(np.random.random() if start_u is None else start_u[1], self.max_t)
                elif start_u is None:
                    weights = 1.0 / ((np.arange(self.max_t + 1) + 1) ** 2)
                    weights = weights / weights.sum()
                    self.t = np.random.choice(np.arange(self.max_t + 1), p=weights)
                else:
                    self.t = choice_from_cdf(self._start_cdf(), start_u[1])
        else:
            self.t = 0.0
        self.episode_step = 0
        self.warning_count = 0
        self.rest_start = np.zeros(self.n_coolers)
        self.rest_idx = rest
        self.rest_start[rest] = self.t
        self.default_action_value = (self.target_temperature - self.lower_bound) / (self.upper_bound - self.lower_bound)
        self.switch = np.ones(self.n_coolers, np.int8)
        self.switch[rest] = 0
        self.value = np.full(self.n_coolers, self.default_action_value, np.float32)
        obs = self._obs()
        self.filter_out = [0.0] * self.n_coolers      # cooler.reset(): last_output = 0.0, the queue empty, no last call
        self.queue = [[] for _ in range(self.n_coolers)]
        self.last_call = None
        self.eer_margin = np.inf      # smallest |ambient - state[nloc]| a cooler saw (the EER jump), for the fixtures
        return obs, {"state": self.state.copy(), "time": self.t}

    def _rotate(self):
        if (self.t - self.rest_start[self.rest_idx]) > REST_SECONDS:
            self.switch[self.rest_idx] = 1
            self.rest_idx = 0 if self.rest_idx + 1 > self.n_coolers - 1 else self.rest_idx + 1
            self.switch[self.rest_idx] = 0
            self.rest_start[self.rest_idx] = self.t

    def _read(self, sn, dn, k):
        s = self.state
        k0, k1 = k[..., 0], k[..., 1]
        return (s[sn[..., 0], sn[..., 1]] * (1 - k0) * (1 - k1) + s[dn[..., 0], sn[..., 1]] * k0 * (1 - k1)
                + s[sn[..., 0], dn[..., 1]] * (1 - k0) * k1 + s[dn[..., 0], dn[..., 1]] * k0 * k1)

    def _obs(self):
        sn, dn, k, _ = self._sensor
        task = self.task
        drift = fourier(task["sensor_order"], task["sensor_coef"], task["sensor_n_terms"], self.t / task["sensor_period"])
        obs = {"sensor_readings": (self._read(sn, dn, k) + drift).astype(np.float32)}
        if self.include[0]:
            obs["heat_readings"] = heater_powers(task, self.t).astype(np.float32)
        if self.include[1]:
            temp = self.value * (self.upper_bound - self.lower_bound) + self.lower_bound
            temp[self.switch == 0] = -1.0
            obs["action_temp"] = temp
        if self.include[2]:
            obs["timestep"] = np.array([self.t / (self.iter_per_step * self.sec_per_iter)], dtype=np.int32)
        return obs

    def _iterate(self, set_temp, dt, n):
        static_heat = np.zeros((self.nw, self.nl))
        equip_heat = heater_powers(self.task, self.t)
        for h in range(self.n_heaters):
            static_heat += self.task["heat_diffuse"][h] * equip_heat[h]
        static_chtc = self.convection_coeffs
        energy = [0.0] * self.n_coolers      # float32 values
        cell_area = self.cell_size * self.cell_size
        amb = self.ambient_temp
        for _ in range(n):
            net_heat = np.copy(static_heat)
            net_chtc = np.copy(static_chtc)
            t = self.t
            call_dt = 0.0 if self.last_call is None else t - self.last_call
            s = self.state
            for i, c in enumerate(self._cooler):
                (a0, a1), (b0, b1), (k0, k1) = c["sn"], c["dn"], c["k"]
                gt = float(s[a0, a1] * (1 - k0) * (1 - k1) + s[b0, a1] * k0 * (1 - k1) + s[a0, b1] * (1 - k0) * k1
                           + s[b0, b1] * k0 * k1)
                cur = gt + c["base_bias"]
                q = self.queue[i]
                q.append((t, cur))
                cutoff = t - c["delay_seconds"]
                while q and q[0][0] < cutoff:
                    q.pop(0)
                delayed = q[0][1] if q else cur
                alpha = float(np.exp(-call_dt / (c["delay_seconds"] / 3.0))) if call_dt > 0 else 1.0
                env_temp = alpha * self.filter_out[i] + (1 - alpha) * delayed
                self.filter_out[i] = env_temp
                diff_amb = amb - float(s[c["nloc"]])
                if abs(diff_amb) < self.eer_margin:
                    self.eer_margin = abs(diff_amb)
                plain = True      # the power is a Python float (resting, or a clamped ratio), not a numpy.float64
                if self.switch[i] == 0:
                    power_cool = power_vent = 0.0
                else:
                    temp_diff = env_temp - set_temp[i]
                    if temp_diff > c["temp_diff_decay_ub"]:
                        ratio = 1
                    elif temp_diff < c["temp_diff_decay_lb"]:
                        ratio = 0
                    else:
                        plain = False
                        ratio = (temp_diff - c["temp_diff_decay_lb"]) / (c["temp_diff_decay_ub"] - c["temp_diff_decay_lb"])
                    power_all = (c["max_cooling_power"] - c["min_cooling_power"]) * ratio + c["min_cooling_power"]
                    power_vent = min(max(c["power_vent_ratio"] * power_all, c["power_vent_min"]), power_all)
                    power_cool = power_all - power_vent
                if diff_amb < 0:
                    eer = c["cooler_eer_reverse"]
                elif diff_amb < c["cooler_eer_decay_start"]:
                    eer = c["cooler_eer_base"]
                elif diff_amb < c["cooler_eer_zero_point"]:
                    eer = c["cooler_eer_base"] * ((c["cooler_eer_zero_point"] - diff_amb)
                                                  / (c["cooler_eer_zero_point"] - c["cooler_eer_decay_start"]))
                else:
                    eer = 0.0
                net_heat += -eer * c["D"] * power_cool
                net_chtc += c["V"] * power_vent * c["power_eff_vent"]
                # energy_costs[i] += power * dt on a float32 array: a numpy.float64 product is added in fp64 and the sum
                # rounded; a Python float is weak, so the product is rounded to float32 first and added in float32
                step_energy = (power_cool + power_vent) * dt
                if plain:
                    energy[i] = float(np.float32(energy[i]) + np.float32(step_energy))
                else:
                    energy[i] = float(np.float32(energy[i] + step_energy))
            self.last_call = t
            se = np.full((self.nw + 2, self.nl + 2), amb)
            se[1:-1, 1:-1] = s
            horizontal = -(se[1:, 1:-1] - se[:-1, 1:-1]) * net_chtc[:, :-1, 0] * self.csa
            vertical = -(se[1:-1, 1:] - se[1:-1, :-1]) * net_chtc[:-1, :, 1] * self.csa
            floor_ceil = self.floorceil_chtc * cell_area * (amb - s)
            net_in = (horizontal[:-1, :] - horizontal[1:, :]) + (vertical[:, :-1] - vertical[:, 1:]) + floor_ceil
            if np.isnan(net_heat).any() or np.isnan(net_in).any():
                raise ValueError("NaN detected in heat calculations.")
            self.state += (net_heat + net_in) / self.heat_capacity * dt
            self.t += dt
        self.t = int(self.t + 0.5) if self.t >= 0 else int(self.t - 0.5)
        return equip_heat, np.array(energy, np.float32) / (dt * n)

    def step(self, action):
        action = np.asarray(action)
        if action.shape != (self.n_coolers,):
            raise ValueError("action must have shape (%d,)" % self.n_coolers)
        self._rotate()
        value = np.clip(action, 0.0, 1.0).astype(np.float32)
        value[self.switch < 0.5] = self.default_action_value
        self.episode_step += 1
        set_temp = np.clip(value, 0.0, 1.0) * (self.upper_bound - self.lower_bound) + self.lower_bound      # float32
        equip_heat, powers = self._iterate([float(v) for v in set_temp], self.sec_per_iter, self.iter_per_step)
        self.value = value
        obs = self._obs()
        average_power = np.mean(powers)
        heat_power = np.sum(np.copy(equip_heat))
        reward, terminated, info = self._reward(obs["sensor_readings"], average_power, heat_power)
        truncated = self.t >= self.max_t
        info.update(time=self.t, heat_power=np.copy(equip_heat), cool_power=powers, state=self.state.copy())
        if self.overheat_no_termiated_training_only:      # (the failure's reward, info and last_fail stand)
            terminated = False
        return obs, reward, terminated, truncated, info

    def _reward(self, obs_arr, power, heat_power):
        obs_dev = np.clip(obs_arr - self.target_temperature, 0.0, 8.0)
        # numpy.maximum's third positional argument is `out`: the d^2 / 8 array is overwritten with max(sqrt(d), d)
        target_loss = np.maximum(np.sqrt(obs_dev), obs_dev, obs_dev ** 2 / 8.0)
        target_cost = TARGET_WHT * np.mean(target_loss)
        energy_cost = ENERGY_WHT * (self.avg_total_heat / heat_power) * (power / 10000)
        if self.reward_mode == 1:
            energy_cost, target_cost = energy_cost * 1.25, target_cost * 0.75
        elif self.reward_mode == 2:
            energy_cost, target_cost = energy_cost * 1.5, target_cost * 0.5
        hard_loss = (obs_arr > self.failure_upperbound).any()
        overheat, overheat_cost = 0, 0
        if hard_loss and self.episode_step > 5:
            overheat, overheat_cost = 1, OVERHEAT_REWARD
            self.warning_count = min(WARNING_TOLERANCE + 1, self.warning_count + 1)
        else:
            self.warning_count = max(self.warning_count - 1, 0)
        info = {"over_heat": overheat, "over_tolerace": 0, "energy_cost": energy_cost, "target_cost": target_cost}
        if self.warning_count > WARNING_TOLERANCE:
            info["over_tolerace"] = 1
            self.last_fail_timestemp = self.t
            return FAILURE_REWARD, True, info
        self.history.append(self.rest_idx)      # _save_cooler_state_history: a failing step returns before it
        return BASE_REWARD + target_cost + 0.0 + energy_cost + 0.0 + overheat_cost, False, info
