"""The reference's PID teachers (anyhvac_solver.py: HVACSolverGTPID, HVACSolverLOCPID, HVACSolverGridSearchPID) restated
over this project's flat task dict: numpy, the reference's expressions with the reference's dtypes, one env per object.
PIDHost is pinned bit for bit to recorded runs of the reference (tests/golden/pid_anyhvac_*.npz) and is the yardstick of
the device controller (csrc/anyhvac.hip: hv_pid).

One controller call, per sensor s and cooler c (target is a Python float, the readings are float32):
    diff      = target - obs                      float32
    last_diff = target - last_obs                 float32 (last_obs: float32 zeros at the first call and after reset())
    acc_diff += diff                              float64 accumulator of float32 terms
    d_e       = -(kp diff - kd (diff - last_diff) / delta_t + ki acc_diff)
    x         = d_e @ corr_sensor_cooler          float64 [C]
    flat      = [x > -0.05, clip(x, 0, 1)]        float32 [2C]; the env's action is 1 - flat[C:]
With Python-float gains (the solvers' defaults) kp diff and kd (diff - last_diff) / delta_t are float32 expressions (numpy
rounds a Python float to the array's float32) and only ki acc_diff is float64; with numpy.float64 gains (the grid search's
linspace values) all three products are float64.  gains="python" | "float64" selects between the two.

The reference's constructor stores numpy.array(env._get_obs()), a 0-d object array whose shape never matches, so its first
policy() call starts from a float32 zero vector: the derivative term of step 1 is -kd obs / delta_t, a large kick that
saturates the action.  reset() restores exactly that state.  (The grid search's _evaluate_params zeroes last_observation
as float64, which forms step 1's diff - last_diff in float64; the kick saturates either way and PIDHost keeps float32.)
"""
import itertools

import numpy as np

from .host import HVACHost, bilinear_setup

KINDS = ("gt", "loc")
GAINS = ("python", "float64")
DEFAULT_GAINS = dict(kp=5.0e-3, ki=2.0e-2, kd=5.0e-3)
METRICS = ("mean_error", "max_error", "std_error", "error_within_2C", "error_within_1C", "mean_reward", "mean_overshoot")


def _nloc(task, which):
    return bilinear_setup(task[which + "_loc"], float(task["cell_size"]), int(task["n_width"]), int(task["n_length"]))[3]


def pid_weights(task, kind="gt"):
    """corr_sensor_cooler, float64 [S, C]: 'gt' — every cooler's cooler_diffuse at the sensor's cell; 'loc' — the inverse
    distance of the integer cell indices; both scaled up while a row sums below 1e-6 and normalised by the clipped sum"""
    if kind not in KINDS:
        raise ValueError("kind must be one of %s" % (KINDS,))
    sn = _nloc(task, "sensor")
    rows = []
    if kind == "gt":
        diffuse = np.asarray(task["cooler_diffuse"], np.float64)
        for nx, ny in sn:
            w = np.asarray([diffuse[c][nx, ny] for c in range(diffuse.shape[0])])
            while np.sum(w) < 1.0e-6:
                w *= 10.0
                w += 1.0e-12
            rows.append(w)
        return rows / np.clip(np.sum(rows, axis=1, keepdims=True), a_min=1e-6, a_max=None)
    cn = _nloc(task, "cooler")
    dist = np.zeros((len(sn), len(cn)))
    for i, s in enumerate(sn):
        for j, c in enumerate(cn):
            dist[i, j] = np.sqrt((s[0] - c[0]) ** 2 + (s[1] - c[1]) ** 2)
    dist = np.clip(dist, 1e-6, None)
    for i in range(len(sn)):
        w = 1.0 / dist[i, :]
        while np.sum(w) < 1.0e-6:
            w *= 10.0
            w += 1.0e-12
        w /= np.clip(np.sum(w), a_min=1e-6, a_max=None)
        rows.append(w)
    return np.array(rows)


def typed_gains(kp, ki, kd, gains):
    if gains not in GAINS:
        raise ValueError("gains must be one of %s" % (GAINS,))
    cast = float if gains == "python" else np.float64
    return cast(kp), cast(ki), cast(kd)


class PIDHost(object):
    def __init__(self, task, kind="gt", kp=DEFAULT_GAINS["kp"], ki=DEFAULT_GAINS["ki"], kd=DEFAULT_GAINS["kd"],
                 sec_per_step=200 * 0.15, gains="python", weights=None):
        self.target_temperature = float(task["target_temperature"])
        self.corr_sensor_cooler = pid_weights(task, kind) if weights is None else np.asarray(weights, np.float64)
        self.n_sensors, self.n_coolers = self.corr_sensor_cooler.shape
        self.kp, self.ki, self.kd = typed_gains(kp, ki, kd, gains)
        self.delta_t = sec_per_step / 60
        self.reset()

    def reset(self):
        self.acc_diff = np.zeros(self.n_sensors)
        self.last_observation = np.zeros(self.n_sensors, np.float32)

    def advance(self, sensor_readings):
        """ONE controller call up to the per-sensor error signal d_e, float64 [S]: acc_diff and last_observation move on,
        so call it (or policy(), which calls it) exactly once per step"""
        obs = np.array(sensor_readings)[:self.n_sensors]
        if obs.dtype != np.float32 or obs.shape != (self.n_sensors,):
            raise ValueError("sensor_readings must be float32 [%d] (or longer: a time component is cut off)" % self.n_sensors)
        target = self.target_temperature
        diff = target - obs
        last_diff = target - self.last_observation
        self.acc_diff += diff
        d_e = -(self.kp * diff - self.kd * (diff - last_diff) / self.delta_t + self.ki * self.acc_diff)
        self.last_observation = np.copy(obs)
        return d_e

    def flat_from(self, x):
        """the pre-clip action values x, float64 [C] -> the reference's flat float32 [2C] action"""
        flat = np.zeros(2 * self.n_coolers, dtype=np.float32)
        flat[:self.n_coolers] = (x > -0.05).astype(np.float32)
        flat[self.n_coolers:] = np.clip(x, 0.0, 1.0)
        return flat

    def policy(self, sensor_readings):
        self.last_x = np.matmul(self.advance(sensor_readings), self.corr_sensor_cooler)
        return self.flat_from(self.last_x)


def search_score(metrics):
    return 0.5 * metrics["mean_error"] + 0.3 * (100 - metrics["error_within_2C"]) / 10 + 0.2 * metrics["max_error"]


def first_strict_minimum(results):
    """HVACSolverGridSearchPID.search's `if score < best_score` over the candidates in their order"""
    best, best_score = None, float("inf")
    for m in results:
        if m["score"] < best_score:
            best_score, best = m["score"], m.copy()
    return best


def evaluate_host(env, pid, init_grid, max_steps):
    """_evaluate_params for the gains pid holds: the env is driven with 1 - policy(obs)[C:] for max_steps steps, never
    breaking on done; the errors are those of the observation AFTER every step"""
    obs, _ = env.reset(init_grid)
    pid.reset()
    C, target = pid.n_coolers, pid.target_temperature
    errors, rewards, overshoots = [], [], []
    for _ in range(max_steps):
        action = 1 - pid.policy(obs["sensor_readings"])[C:]
        obs, reward, _, _, _ = env.step(action)
        readings = obs["sensor_readings"]
        errors.extend(np.abs(readings - target).tolist())
        overshoots.append(np.sum(readings > target + 2.0))
        rewards.append(reward)
    errors = np.array(errors)
    return {"kp": pid.kp, "ki": pid.ki, "kd": pid.kd, "mean_error": np.mean(errors), "max_error": np.max(errors),
            "std_error": np.std(errors), "error_within_2C": np.mean(errors <= 2.0) * 100,
            "error_within_1C": np.mean(errors <= 1.0) * 100, "mean_reward": np.mean(rewards),
            "mean_overshoot": np.mean(overshoots)}


def pid_search_host(task, kp_values, ki_values, kd_values, max_steps, settings=None, init_grid=None, kind="gt",
                    generate_task=False, evaluate=None):
    """HVACSolverGridSearchPID.search over HVACHost + PIDHost -> (best_params, search_results).  One departure: every
    candidate starts from the SAME initial grid (init_grid, or one draw of HVACHost.reset()), where the reference draws a
    fresh one per candidate — the scores are then comparable.  evaluate(kp, ki, kd) -> metrics replaces the rollout."""
    if evaluate is None:
        settings = dict(settings or {})
        env = HVACHost(**settings)
        env.set_task(task, generate_task=generate_task)
        if init_grid is None:
            init_grid = env.reset()[1]["state"]
        sec_per_step = env.iter_per_step * env.sec_per_iter
        weights = pid_weights(task, kind)

        def evaluate(kp, ki, kd):
            pid = PIDHost(task, kp=kp, ki=ki, kd=kd, sec_per_step=sec_per_step, gains="float64", weights=weights)
            return evaluate_host(env, pid, init_grid, max_steps)
    results = []
    for kp, ki, kd in itertools.product(kp_values, ki_values, kd_values):
        m = evaluate(kp, ki, kd)
        m["score"] = search_score(m)
        results.append(m)
    return first_strict_minimum(results), results
