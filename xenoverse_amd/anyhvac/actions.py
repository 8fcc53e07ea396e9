"""The reference's two RL action spaces restated over HVACHost (anyhvac_env.py:782-1276), numpy in the reference's own
order and dtypes, pinned bit for bit to recorded runs (tests/golden/act_anyhvac_*.npz) and the yardstick of the mapped
step kernels (csrc/anyhvac.hip, xv_anyhvac_step_mapped).

DiscreteActionHost — HVACEnvDiscreteAction: the value is turned into a set temperature IN THE INPUT'S DTYPE (float32 for
  the Box space), divided by 0.1 in that dtype, rounded half to even, multiplied by 0.1 in fp64 and turned back.
DiffActionHost — HVACEnvDiffAction (flat branches, no_switch_action=True): each input picks one of 13 steps -3 ... +3 K —
  an integer index (MultiDiscrete, discretize_rl_action_space=True) or a float32 in [0, 1] mapped by
  clip(round(v * 12), 0, 12) — which is added IN FP64 to the float32 set temperature the env applied at the step before
  (the resting cooler's column holds the default value there), bounded below by target - 3 under too_cold_limit,
  rounded to 0.1 K as above and turned back.  With add_action_cost the step's reward gets -mean_c(0.5 table[index_c] +
  0.5 * 0.6 * reversals_c), reversals_c the adjacent nonzero sign reversals among cooler c's last <= 10 steps.
Both end in the base step's clip(...).astype(float32), and both return info["step_stat"] from stat(), whose running
averages are kept as the reference keeps them (never cleared, the step index being the episode's).
"""
import numpy as np

from .host import HVACHost

ACTION_RESOLUTION_TEMP = 0.1
DISCRETE_VALUES = np.linspace(-3.0, 3.0, int((3.0 - -3.0) / 0.5) + 1)      # the 13 temperature steps
N_BINS = len(DISCRETE_VALUES)
TARGET_TEMP_OFFSET = 3
WINDOW_LEN = 10
# the non-zero-step term of _calculate_simplified_action_cost per bin, formed with the reference's own expression; the
# device is handed this table and evaluates no pow
COST_TABLE = np.array([(abs(d) ** 1.2) * 0.3 for d in DISCRETE_VALUES])
STAT_THRESHOLDS = (0, 2, 4, 6)
STAT_KEYS = ("hot_0", "hot_2", "hot_4", "hot_6", "cool_0", "cool_-2", "cool_-4", "cool_-6")
ACTION_MODES = ("box", "discrete", "diff")


class RunningStat(object):
    """stat()'s running averages (anyhvac_env.py:684-779) from one step's counts; the device classes feed it the kernel's
    counts, the host classes numpy's"""

    def __init__(self):
        self.avg_cooler_power_per_step = 0.0
        self.avg_reward = 0.0
        self.over_heat_percentage = [0.0, 0.0, 0.0, 0.0]
        self.over_cool_percentage = [0.0, 0.0, 0.0, 0.0]
        self.fail_percentage = 0.0

    def update(self, current_step, n_sensor, count_overheat, count_overcool, cool_power, terminated, reward):
        current_cool_power = round(np.sum(cool_power), 4)
        self.avg_cooler_power_per_step = (self.avg_cooler_power_per_step * (current_step - 1) + current_cool_power) / current_step
        self.avg_reward = (self.avg_reward * (current_step - 1) + reward) / current_step
        last = [p * (current_step - 1) * n_sensor for p in self.over_heat_percentage]
        self.over_heat_percentage = [(a + b) / (current_step * n_sensor) for a, b in zip(last, count_overheat)]
        last = [p * (current_step - 1) * n_sensor for p in self.over_cool_percentage]
        self.over_cool_percentage = [(a + b) / (current_step * n_sensor) for a, b in zip(last, count_overcool)]
        self.fail_percentage = (self.fail_percentage * (current_step - 1) + int(terminated)) / current_step
        return {"reward": reward, "cooler_power": current_cool_power,
                "cool_0": count_overcool[0], "cool_-2": count_overcool[1], "cool_-4": count_overcool[2],
                "cool_-6": count_overcool[3], "hot_0": count_overheat[0], "hot_2": count_overheat[1],
                "hot_4": count_overheat[2], "hot_6": count_overheat[3], "fail": int(terminated)}

    def running(self):
        return dict(avg_reward=self.avg_reward, avg_cooler_power_per_step=self.avg_cooler_power_per_step,
                    over_heat_percentage=list(self.over_heat_percentage),
                    over_cool_percentage=list(self.over_cool_percentage), fail_percentage=self.fail_percentage)


def stat_counts(sensor_reading, target_temperature):
    """-> (hot[4], cool[4]): the readings above target + 0, 2, 4, 6 and below target - 0, 2, 4, 6, with the reference's
    expression (a float32 array minus a Python float: a float32 difference)"""
    d = sensor_reading - target_temperature
    return [np.sum(d > k) for k in STAT_THRESHOLDS], [np.sum(d < -k) for k in STAT_THRESHOLDS]


def stat_margin(sensor_reading, target_temperature):
    """the smallest distance of reading - target from a threshold 0, +-2, +-4, +-6 (fp64, for the fixtures)"""
    d = np.asarray(sensor_reading, np.float64) - float(target_temperature)
    return float(min(np.abs(d - k).min() for k in (0, 2, -2, 4, -4, 6, -6)))


class ActionMapHost(HVACHost):
    """HVACHost + stat(): what the two action classes share"""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.stats = RunningStat()

    def _span(self):
        return self.upper_bound - self.lower_bound

    def _value_from_temp(self, temp, tenth):
        """temp / tenth (in the dtype numpy gives the pair) rounded half to even, times 0.1 in fp64, as a clipped value"""
        snapped = np.round(temp / tenth).astype(int) * ACTION_RESOLUTION_TEMP
        return np.clip((snapped - self.lower_bound) / self._span(), 0.0, 1.0)

    def stat(self, obs, terminated, info, reward):
        hot, cool = stat_counts(obs["sensor_readings"], self.target_temperature)
        return self.stats.update(self.episode_step, self.n_sensors, hot, cool, info.get("cool_power", 0), terminated, reward)

    def _with_stat(self, out):
        obs, reward, terminated, truncated, info = out
        info["step_stat"] = self.stat(obs, terminated, info, reward)
        return obs, reward, terminated, truncated, info


RUNNING_KEYS = ("avg_reward", "avg_cooler_power_per_step", "over_heat_percentage", "over_cool_percentage", "fail_percentage")
for _k in RUNNING_KEYS:      # the running averages, under the reference's attribute names
    setattr(ActionMapHost, _k, property(lambda self, k=_k: getattr(self.stats, k)))


class DiscreteActionHost(ActionMapHost):
    def map_action(self, action):
        """raw values -> the values handed to the base step; the temperature keeps the input's dtype up to the division"""
        raw = np.asarray(action)[:self.n_coolers]
        return self._value_from_temp(raw * self._span() + self.lower_bound, ACTION_RESOLUTION_TEMP)

    def step(self, action):
        return self._with_stat(super().step(self.map_action(action)))


class DiffActionHost(ActionMapHost):
    """bins[n, C] holds the bins of the last n <= WINDOW_LEN steps of the episode, oldest first (the action cost's window)"""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.discrete_rl_action_space, self.add_action_cost, self.too_cold_limit = False, False, True
        self.bins = None

    def set_too_cold_limit(self, too_cold_limit):
        self.too_cold_limit = too_cold_limit

    def set_task(self, task, discretize_rl_action_space=False, add_action_cost=False, too_cold_limit=True,
                 generate_task=False):
        super().set_task(task, generate_task=generate_task)
        self.discrete_rl_action_space = discretize_rl_action_space
        self.add_action_cost = add_action_cost
        self.too_cold_limit = too_cold_limit

    def reset(self, state=None, start_u=None):
        self.bins = None
        return super().reset(state, start_u)

    def action_indices(self, action):
        """the bin per cooler: the integers themselves under the MultiDiscrete space, else round(v * 12) clipped"""
        action = np.asarray(action)
        if self.discrete_rl_action_space and np.issubdtype(action.dtype, np.integer):
            return action.astype(int)
        return np.clip(np.round(action[:self.n_coolers] * (N_BINS - 1)), 0, N_BINS - 1).astype(int)

    def map_action(self, action):
        """-> (the values handed to the base step, the temperature steps taken, the bins)"""
        idx = self.action_indices(action)
        step_k = DISCRETE_VALUES[idx]
        temp = (self.value * self._span() + self.lower_bound) + step_k      # float32 set temperature + fp64 step: fp64
        if self.too_cold_limit:
            floor = self.target_temperature - TARGET_TEMP_OFFSET
            temp[temp < floor] = floor
        return self._value_from_temp(temp, ACTION_RESOLUTION_TEMP), step_k, idx

    def action_cost(self, idx):
        """push this step's bins and price them: per cooler half the table's entry plus half of 0.6 per adjacent pair of
        opposite nonzero signs in its window; the mean over the coolers, never below zero"""
        row = np.asarray(idx, int)[None]
        self.bins = row if self.bins is None else np.concatenate([self.bins, row])[-WINDOW_LEN:]
        sign = np.sign(self.bins - (N_BINS - 1) // 2)
        reversals = (sign[1:] * sign[:-1] < 0).sum(axis=0)
        per_cooler = 0.5 * COST_TABLE[self.bins[-1]] + 0.5 * (reversals * 0.6)
        return max(np.mean(per_cooler), 0.0)

    def step(self, action, call_diff_action=True):
        if not call_diff_action:      # (the values as they are: no step, no cost)
            return self._with_stat(super().step(np.asarray(action)))
        value, _, idx = self.map_action(action)
        obs, reward, terminated, truncated, info = super().step(value)
        if self.add_action_cost:
            info["action_cost"] = -1 * self.action_cost(idx)
            reward = reward + info["action_cost"]
        return self._with_stat((obs, reward, terminated, truncated, info))
