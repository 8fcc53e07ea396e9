"""HVACEnv — the one-room wrapper over HVACVecEnv (vec_env.py) with the reference's constructor keywords and numpy outputs of
the room's true sizes; HVACEnvDiscreteAction / HVACEnvDiffAction — the reference-shaped one-room classes of the RL action
spaces, with stat()'s running averages."""
import numpy as np

from .actions import STAT_KEYS, RunningStat
from .vec_env import HVACVecEnv


class HVACEnv(object):
    """one room with the reference's surface: HVACEnv(**keywords); set_task(task, generate_task=False); reset() ->
    (obs, info); step(action[C]) -> (obs, reward, terminated, truncated, info), numpy arrays of the room's true sizes.
    The episode is not reset behind the caller's back (autoreset_mode='disabled')."""
    ACTION_MODE = "box"

    def __init__(self, max_steps=20160, iter_per_step=200, sec_per_iter=0.15, set_lower_bound=16, set_upper_bound=32,
                 verbose=False, action_space_format='box', include_heat_in_observation=True,
                 include_switch_in_observation=False, include_last_action_in_observation=True,
                 include_timestep_in_observation=True, no_switch_action=True, reward_mode=0, device="cuda:0", seed=0):
        self.vec = HVACVecEnv(1, action_mode=self.ACTION_MODE, max_steps=max_steps, iter_per_step=iter_per_step, sec_per_iter=sec_per_iter,
                              set_lower_bound=set_lower_bound, set_upper_bound=set_upper_bound, reward_mode=reward_mode,
                              include_heat_in_observation=include_heat_in_observation,
                              include_last_action_in_observation=include_last_action_in_observation,
                              include_timestep_in_observation=include_timestep_in_observation, device=device, seed=seed,
                              autoreset_mode="disabled", action_space_format=action_space_format,
                              include_switch_in_observation=include_switch_in_observation,
                              no_switch_action=no_switch_action)
        self.verbose = verbose
        self.task_set = False

    def set_task(self, task, generate_task=False):
        self.vec.set_task([task], generate_task=generate_task)
        self.action_space = self.vec.single_action_space
        self.task_set = True

    def set_random_start_t(self, random_start_t):
        self.vec.set_random_start_t(bool(random_start_t))

    def set_generate_record(self, generate_record):
        self.vec.set_generate_record(bool(generate_record))

    def set_overheat_no_termiated_training_only(self, overheat_no_termiated_training_only):
        self.vec.set_overheat_no_termiated_training_only(bool(overheat_no_termiated_training_only))

    def _np(self, obs):
        c = self.vec.counts
        width = dict(sensor_readings=c["sensors"][0], heat_readings=c["heaters"][0], action_temp=c["coolers"][0])
        out = {}
        for k, v in obs.items():
            if k == "counts":
                continue
            v = v[0].cpu().numpy()
            out[k] = v[:width[k]] if k in width else v.reshape(1)
        return out

    def reset(self, *args, state=None, start_u=None, **kwargs):
        """state: the initial grid [n_width, n_length] (otherwise ambient + 2 N(0, 1) from the engine's Philox stream);
        start_u: with it, the uniforms (u0, u1) of the start draw under random_start_t"""
        if state is None:
            obs, _ = self.vec.reset()
        else:
            obs = self.vec.reset_injected(np.asarray(state, np.float64)[None],
                                          start_u=None if start_u is None else np.asarray(start_u, np.float64)[None])
        return self._np(obs), {"time": float(self.vec.time()[0])}

    def step(self, action):
        n = int(self.vec.counts["coolers"][0])
        action = np.asarray(action)
        integer = self.ACTION_MODE == "diff" and self.vec.discretize_rl_action_space and np.issubdtype(action.dtype, np.integer)
        a = np.zeros((1, self.vec.dims[2]), np.int32 if integer else np.float32)
        a[0, :n] = action.reshape(-1)[:n]
        obs, r, term, trunc, info = self.vec.step(a)
        self._last = info
        c = self.vec.counts
        out = {k: float(info[k][0]) for k in ("energy_cost", "target_cost", "time")}
        out.update(over_heat=int(info["over_heat"][0]), over_tolerace=int(info["over_tolerace"][0]),
                   cool_power=info["cool_power"][0, :n].cpu().numpy(),
                   heat_power=info["heat_power"][0, :int(c["heaters"][0])].cpu().numpy())
        return self._np(obs), float(r[0]), bool(term[0]), bool(trunc[0]), out

    def sample_action(self, mode="constant"):
        a = self.vec.sample_action(mode)
        return a[0, :int(self.vec.counts["coolers"][0])].cpu().numpy()

    def check_errors(self, clear=True):
        return self.vec.check_errors(clear)

    def close(self):
        self.vec.close()


class _StatEnv(HVACEnv):
    """HVACEnv + stat(): info["step_stat"] with the reference's keys and its running averages as attributes"""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.stats = RunningStat()

    def _finish(self, out):
        obs, reward, terminated, truncated, info = out
        raw = self._last
        n = int(self.vec.counts["coolers"][0])
        info["last_control"] = {"value": raw["applied_value"][0, :n].cpu().numpy()}
        if self.vec.add_action_cost:
            info["action_cost"] = float(raw["action_cost"][0])
        cnt = [int(raw["step_stat"][k][0]) for k in STAT_KEYS]
        info["step_stat"] = self.stats.update(int(raw["episode_step"][0]), int(self.vec.counts["sensors"][0]), cnt[:4], cnt[4:],
                                              info["cool_power"], terminated, reward)
        return obs, reward, terminated, truncated, info


for _k in ("avg_reward", "avg_cooler_power_per_step", "over_heat_percentage", "over_cool_percentage", "fail_percentage"):
    setattr(_StatEnv, _k, property(lambda self, k=_k: getattr(self.stats, k)))


class HVACEnvDiscreteAction(_StatEnv):
    """the reference's HVACEnvDiscreteAction: absolute actions rounded to 0.1 K on the device, info["step_stat"]"""
    ACTION_MODE = "discrete"

    def step(self, action):
        return self._finish(super().step(action))


class HVACEnvDiffAction(_StatEnv):
    """the reference's HVACEnvDiffAction: each action is one of 13 temperature steps on the cooler's previous set-point"""
    ACTION_MODE = "diff"

    def set_too_cold_limit(self, too_cold_limit):
        self.vec.set_too_cold_limit(too_cold_limit)

    def set_task(self, task, discretize_rl_action_space=False, add_action_cost=False, too_cold_limit=True,
                 generate_task=False):
        vec = self.vec      # (the options go to the device with the handle set_task builds)
        vec.discretize_rl_action_space, vec.add_action_cost = bool(discretize_rl_action_space), bool(add_action_cost)
        vec.too_cold_limit = bool(too_cold_limit)
        super().set_task(task, generate_task=generate_task)

    def step(self, action, call_diff_action=True):
        if not call_diff_action:
            raise ValueError("call_diff_action=False is not supported by xenoverse_amd.anyhvac (the mapping runs on the device)")
        return self._finish(super().step(action))
