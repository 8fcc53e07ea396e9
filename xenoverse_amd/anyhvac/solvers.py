"""HVACSolverGTPID / HVACSolverLOCPID / HVACSolverGridSearchPID — the reference-shaped PID teacher classes over the one-room
HVACEnv (single_env.py); the controller runs on the device (HVACVecEnv.set_pid / pid_action / rollout_teacher, vec_env.py)
and the grid search evaluates its candidates as the envs of one batch."""
import itertools

import numpy as np

from .pid import DEFAULT_GAINS, first_strict_minimum, pid_weights, search_score
from .vec_env import HVACVecEnv


class HVACSolverGTPID(object):
    """the reference's HVACSolverGTPID over the one-room HVACEnv (set_task and reset first): .policy(observation) -> the flat
    float32 [2C] action (switch columns, value columns), computed on the device; the env's action is 1 - policy(obs)[C:].
    kp, ki, kd and corr_sensor_cooler are attributes as there; gains that are numpy.float64 scalars take the float64
    arithmetic numpy gives the reference with them."""
    kind = "gt"

    def __init__(self, env):
        if not getattr(env, "task_set", False):
            raise Exception("Must call \"set_task\" first")
        self.env = env
        vec = env.vec
        task = vec._tasks[0]
        self.target_temperature = float(task["target_temperature"])
        self.sec_per_step = vec.iter_per_step * vec.sec_per_iter
        self.lower_bound, self.upper_bound = vec.lower_bound, vec.upper_bound
        self.delta_t = self.sec_per_step / 60
        self.kp, self.ki, self.kd = DEFAULT_GAINS["kp"], DEFAULT_GAINS["ki"], DEFAULT_GAINS["kd"]
        self.corr_sensor_cooler = pid_weights(task, self.kind)
        self.n_sensors, self.n_coolers = self.corr_sensor_cooler.shape
        self._on_device = None
        self._push(keep_state=False)

    def _gains_mode(self):
        kinds = {isinstance(g, np.floating) for g in (self.kp, self.ki, self.kd)}
        if len(kinds) != 1:
            raise ValueError("kp, ki and kd must be all Python floats or all numpy.float64 scalars")
        return "float64" if kinds.pop() else "python"

    def _push(self, keep_state=True):
        """the gains and weights as the attributes have them now -> the device (the controller's state is kept)"""
        want = (float(self.kp), float(self.ki), float(self.kd), self._gains_mode(), self.corr_sensor_cooler.tobytes())
        if want == self._on_device and self.env.vec._pid is not None:
            return
        vec = self.env.vec
        state = vec.get_pid_state() if keep_state and vec._pid is not None else None
        vec.set_pid(kp=self.kp, ki=self.ki, kd=self.kd, gains=want[3], weights=[self.corr_sensor_cooler])
        if state is not None:
            vec.set_pid_state(**state)
        self._on_device = want

    def reset(self):
        self._push()
        self.env.vec.pid_reset()

    def policy(self, observation):
        obs = np.array(observation)[:self.n_sensors]
        if obs.dtype != np.float32 or obs.shape != (self.n_sensors,):
            raise ValueError("the observation must be the env's float32 sensor readings")
        self._push()
        _, flat = self.env.vec.pid_action(obs[None], return_flat=True)
        return flat[0, :, :self.n_coolers].reshape(-1).cpu().numpy()


class HVACSolverLOCPID(HVACSolverGTPID):
    """HVACSolverGTPID with the inverse-distance weight matrix"""
    kind = "loc"


class HVACSolverGridSearchPID(HVACSolverGTPID):
    """the reference's HVACSolverGridSearchPID: .search() evaluates every (kp, ki, kd) of the three linspaces for max_steps
    controller-driven steps and returns the candidate with the lowest score.  Here the candidates are the envs of ONE batch
    (a private HVACVecEnv), each with its own gains, all with the env's task and the SAME initial grid (the reference
    draws a new one per candidate)."""
    MAX_T = 64      # steps per launch

    def __init__(self, env, kp_range=(1e-3, 5e-2, 10), ki_range=(1e-2, 1e-1, 10), kd_range=(1e-3, 2e-2, 10)):
        super().__init__(env)
        self.kp_values, self.ki_values, self.kd_values = (np.linspace(r[0], r[1], r[2]) for r in (kp_range, ki_range, kd_range))
        self.kp_range, self.ki_range, self.kd_range = kp_range, ki_range, kd_range
        self.search_results, self.best_params = [], None
        self.search_rollouts, self.search_stats = [], np.zeros((0, 8))

    @staticmethod
    def metrics_from_stats(st, max_steps):
        """a pid_stats row -> the reference's metrics (std from the two sums)"""
        n = st[7]
        mean = st[0] / n
        return {"mean_error": mean, "max_error": st[1], "std_error": float(np.sqrt(max(st[2] / n - mean * mean, 0.0))),
                "error_within_2C": st[4] / n * 100, "error_within_1C": st[3] / n * 100, "mean_reward": st[6] / max_steps,
                "mean_overshoot": st[5] / max_steps}

    def search(self, max_steps=1000, apply_best=True, chunk=None, init_grid=None, keep_rollouts=False):
        """-> best_params (the reference's dict).  chunk: candidates per batch (default all at once); init_grid [nw, nl]:
        the grid every candidate starts from; without it the caller's env IS RESET (as the reference's search resets it)
        and its new grid taken; keep_rollouts: rollout_teacher()'s tuples, per chunk a list of calls, stay in
        self.search_rollouts.  search_stats: the candidates' pid_stats rows, float64 [n, 8]."""
        vec0 = self.env.vec
        task = vec0._tasks[0]
        nw, nl = int(task["n_width"]), int(task["n_length"])
        if init_grid is None:
            vec0.reset()
            init_grid = vec0.get_state()["grid"][0].reshape(vec0.dims[0], vec0.dims[1])[:nw, :nl].cpu().numpy()
        init_grid = np.asarray(init_grid, np.float64).reshape(nw, nl)
        cands = list(itertools.product(self.kp_values, self.ki_values, self.kd_values))
        chunk = len(cands) if chunk is None else max(1, int(chunk))
        self.search_results, self.search_rollouts, rows = [], [], []
        for lo in range(0, len(cands), chunk):
            part = np.array(cands[lo:lo + chunk])
            vec = HVACVecEnv(len(part), max_steps=vec0.max_steps, iter_per_step=vec0.iter_per_step,
                             sec_per_iter=vec0.sec_per_iter, set_lower_bound=vec0.lower_bound,
                             set_upper_bound=vec0.upper_bound, reward_mode=vec0.reward_mode, device=str(self.env.vec.device),
                             autoreset_mode="disabled")
            vec.set_task([task], generate_task=vec0._generate_task)
            vec.reset_injected(np.repeat(init_grid[None], len(part), axis=0))
            vec.set_pid(kp=part[:, 0], ki=part[:, 1], kd=part[:, 2], gains="float64", weights=[self.corr_sensor_cooler])
            stats, calls = None, []
            for t0 in range(0, max_steps, self.MAX_T):
                out = vec.rollout_teacher(min(self.MAX_T, max_steps - t0), stats=stats, return_stats=True)
                stats = out[4]["pid_stats"]
                if keep_rollouts:
                    calls.append(out)
            rows.append(stats.cpu().numpy())
            self.search_rollouts.append(calls)
            vec.close()
        self.search_stats = np.concatenate(rows)
        for (kp, ki, kd), st in zip(cands, self.search_stats):
            m = dict(kp=kp, ki=ki, kd=kd, **self.metrics_from_stats(st, max_steps))
            m["score"] = search_score(m)
            self.search_results.append(m)
        self.best_params = first_strict_minimum(self.search_results)
        if apply_best and self.best_params:
            self.apply_params(self.best_params["kp"], self.best_params["ki"], self.best_params["kd"])
        return self.best_params

    def apply_params(self, kp=None, ki=None, kd=None):
        if kp is not None:
            self.kp = kp
        if ki is not None:
            self.ki = ki
        if kd is not None:
            self.kd = kd
