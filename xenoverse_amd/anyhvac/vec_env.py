"""HVACVecEnv — batched AnyHVAC rooms on the device (csrc/anyhvac.hip, include/xeno.h xv_anyhvac_*): one launch steps every
room, one workgroup per room.  HVACEnv — the one-room wrapper with the reference's constructor keywords and numpy outputs
of the room's true sizes.

Observations are dicts of tensors padded to the batch's largest room — sensor_readings[N, S], heat_readings[N, H],
action_temp[N, C] (float32), timestep[N] (int32) — with `counts` (per env: coolers, sensors, heaters, n_width, n_length)
beside them; padded columns are zero and padded action columns are ignored.  Rewards are float64.  Same-step autoreset (the
engine's default) hands out the new episode's first observation and the finished one's last under info["final_obs"];
autoreset_mode="disabled" goes on stepping as the reference's env would; "next_step" is not built.
"""
import ctypes as C

import numpy as np
import torch

from .. import _lib
from ..engine import AUTORESET
from ..spaces import Box
from ..vector import VectorEnv
from .config import RING_CAPACITY
from .host import check_ring, check_settings
from .tables import build_tables

OBS_KEYS = ("sensor_readings", "heat_readings", "action_temp", "timestep")
MISC = ("over_heat", "over_tolerace", "energy_cost", "target_cost", "time", "rest_idx", "warning_count", "episode_step")
_STATE_DTYPES = dict(grid=torch.float64, t=torch.float64, last_call=torch.float64, episode_step=torch.int32,
                     warning_count=torch.int32, rest_idx=torch.int32, rest_start=torch.float64, value=torch.float32,
                     filter=torch.float64, ring_t=torch.float64, ring_v=torch.float64, head=torch.int32, tail=torch.int32)


class HVACVecEnv(VectorEnv):
    def __init__(self, num_envs, max_steps=20160, iter_per_step=200, sec_per_iter=0.15, set_lower_bound=16,
                 set_upper_bound=32, reward_mode=0, include_heat_in_observation=True,
                 include_last_action_in_observation=True, include_timestep_in_observation=True, device="cuda:0", seed=0,
                 env_id_base=0, autoreset_mode="same_step", to_numpy=False, engine=None, **excluded):
        check_settings(**excluded)
        if reward_mode not in (0, 1, 2):
            raise ValueError("reward_mode must be 0, 1 or 2")
        if autoreset_mode == "next_step":
            raise ValueError("autoreset_mode='next_step' is not built for AnyHVAC (same_step and disabled are)")
        if int(max_steps) * int(iter_per_step) >= 2 ** 31 - RING_CAPACITY:
            raise ValueError("max_steps * iter_per_step must stay below 2^31 (the delay queues count their entries)")
        super().__init__(num_envs, device=device, seed=seed, env_id_base=env_id_base, autoreset_mode=autoreset_mode,
                         to_numpy=to_numpy, engine=engine)
        self.max_steps, self.iter_per_step, self.sec_per_iter = int(max_steps), int(iter_per_step), float(sec_per_iter)
        self.lower_bound, self.upper_bound, self.reward_mode = set_lower_bound, set_upper_bound, int(reward_mode)
        self.include = dict(heat_readings=bool(include_heat_in_observation),
                            action_temp=bool(include_last_action_in_observation),
                            timestep=bool(include_timestep_in_observation))
        self._h = None
        self.need_reset = True

    # -- tasks ----------------------------------------------------------------------------------------------------
    def set_task(self, tasks, env_task_index=None, generate_task=False):
        """tasks: one flat task dict (task_sampler.py) or a list; envs share tasks through env_task_index (default: equal
        blocks).  generate_task=True takes avg_total_heat = 10000 as the reference does, False forms the reference's
        week-long average (host.average_total_heat)."""
        if isinstance(tasks, dict):
            tasks = [tasks]
        n_task, n, d = len(tasks), self.num_envs, self.device
        for t in tasks:
            check_ring(t["cooler_delay_seconds"], self.sec_per_iter)
        if env_task_index is None:
            if n % n_task != 0:
                raise ValueError("num_envs is not a multiple of the task count; pass env_task_index")
            env_task = np.arange(n, dtype=np.int32) // (n // n_task)
        else:
            env_task = np.asarray(torch.as_tensor(env_task_index).cpu(), np.int32)
            if env_task.shape != (n,) or env_task.min() < 0 or env_task.max() >= n_task:
                raise ValueError("env_task_index must be (num_envs,) with entries in [0, n_task)")
        tab = build_tables(tasks, self.lower_bound, self.upper_bound, generate_task)
        self.dims = NW, NL, Cc, S, H, KS, KH = tab["dims"]
        self.avg_total_heat = tab["avg_total_heat"]
        cs = tab["counts"]
        self.counts = {k: np.array([cs[i][q] for i in env_task], np.int32) for k, q in
                       (("coolers", "C"), ("sensors", "S"), ("heaters", "H"), ("n_width", "nw"), ("n_length", "nl"))}
        self._tab = dict(table=torch.from_numpy(tab["table"]).to(d), env_task=torch.from_numpy(env_task).to(d))
        self.close_extras()
        h = C.c_void_p()
        max_t = int(self.max_steps * self.iter_per_step * self.sec_per_iter)
        _lib.check(self.lib.xv_anyhvac_create(self.engine.handle, n, NW, NL, Cc, S, H, KS, KH, self.iter_per_step,
                                              self.sec_per_iter, float(self.lower_bound), float(self.upper_bound),
                                              float(max_t), self.reward_mode, C.byref(h)))
        self._h = h
        _lib.check(self.lib.xv_anyhvac_set_task(h, n_task, _lib.ptr(self._tab["table"]), _lib.ptr(self._tab["env_task"])))
        self._set_spaces(None, Box(0.0, 1.0, shape=(Cc,), dtype=np.float32))
        self.single_observation_spaces = dict(
            sensor_readings=Box(10, 50, shape=(S,), dtype=np.float32), heat_readings=Box(0.0, 50000.0, shape=(H,)),
            action_temp=Box(-1, 33, shape=(Cc,)), timestep=Box(0, 30000, shape=(1,), dtype=np.int32))
        self.default_action_value = np.array([(float(tasks[i]["target_temperature"]) - self.lower_bound)
                                              / (self.upper_bound - self.lower_bound) for i in env_task])
        self._targets = np.array([float(tasks[i]["target_temperature"]) for i in env_task])
        self.task_set = True
        self.need_reset = True

    def _set_spaces(self, single_obs, single_act):
        self.single_observation_space = self.observation_space = single_obs
        self.single_action_space = single_act
        from ..spaces import batch_space
        self.action_space = batch_space(single_act, self.num_envs)

    # -- buffers --------------------------------------------------------------------------------------------------
    def _buffers(self, lead, final):
        NW, NL, Cc, S, H, _, _ = self.dims
        d, n = self.device, self.num_envs
        shape = tuple(lead) + (n,)
        z = lambda tail, dt: torch.zeros(shape + tail, dtype=dt, device=d)  # noqa: E731
        b = dict(sensor_readings=z((S,), torch.float32), heat_readings=z((H,), torch.float32),
                 action_temp=z((Cc,), torch.float32), timestep=z((), torch.int32), reward=z((), torch.float64),
                 terminated=z((), torch.uint8), truncated=z((), torch.uint8), cool_power=z((Cc,), torch.float32),
                 heat_power=z((H,), torch.float64), misc=z((8,), torch.float64))
        if final:
            for k, dt in zip(OBS_KEYS, (torch.float32, torch.float32, torch.float32, torch.int32)):
                b["final_" + k] = z(b[k].shape[len(shape):], dt)
        return b

    def _io(self, b, action=None):
        io = _lib.AnyHVACIO()
        io.action = _lib.ptr(action)
        for k in _lib.AnyHVACIO.FIELDS[1:]:
            t = b.get(k)
            base = k[6:] if k.startswith("final_") else k
            if t is not None and self.include.get(base, True):
                setattr(io, k, t.data_ptr())
        return io

    def _obs(self, b, prefix=""):
        obs = {k: self._out(b[prefix + k]) for k in OBS_KEYS if self.include.get(k, True) and prefix + k in b}
        obs["counts"] = self.counts
        return obs

    def _result(self, b):
        misc = b["misc"]
        info = {k: self._out(misc[..., i]) for i, k in enumerate(MISC)}
        info["cool_power"], info["heat_power"] = self._out(b["cool_power"]), self._out(b["heat_power"])
        if self.autoreset_mode == "same_step":
            info["final_obs"] = self._obs(b, "final_")
            info["_final_obs"] = self._out((b["terminated"] | b["truncated"]).bool())
        return (self._obs(b), self._out(b["reward"]), self._out(b["terminated"].bool()), self._out(b["truncated"].bool()),
                info)

    def _pad_grid(self, grid):
        """[N, nw, nl] (or already [N, NW, NL]) -> contiguous float64 [N, NW * NL] on the device"""
        NW, NL = self.dims[:2]
        g = torch.as_tensor(grid, dtype=torch.float64)
        if g.dim() != 3 or g.shape[0] != self.num_envs or g.shape[1] > NW or g.shape[2] > NL:
            raise ValueError("a grid must be [num_envs, <= %d, <= %d]" % (NW, NL))
        out = torch.zeros((self.num_envs, NW, NL), dtype=torch.float64, device=self.device)
        out[:, :g.shape[1], :g.shape[2]] = g.to(self.device)
        return out.reshape(self.num_envs, NW * NL)

    def _actions(self, actions, lead=()):
        a = self._dev(actions, torch.float32)
        if a.shape != tuple(lead) + (self.num_envs, self.dims[2]):
            raise ValueError("actions must have shape %s" % (tuple(lead) + (self.num_envs, self.dims[2]),))
        return a

    # -- episode --------------------------------------------------------------------------------------------------
    def reset(self, *, seed=None, options=None):
        self._require_task()
        if seed is not None:
            self.engine.tick = (int(seed) & 0xFFFFFFFF) << 24
        mask = None
        if options is not None and options.get("reset_mask") is not None:
            mask = self._dev(options["reset_mask"], torch.uint8)
        b = self._buffers((), False)
        io = self._io(b)
        _lib.check(self.lib.xv_anyhvac_reset(self._h, _lib.ptr(mask), C.byref(io)))
        self.need_reset = False
        return self._obs(b), {}

    def reset_injected(self, state, mask=None):
        """reset with the initial grid given: state [N, nw, nl] (rooms smaller than the batch's largest: zero-padded)"""
        self._require_task()
        g = self._pad_grid(state)
        m = None if mask is None else self._dev(mask, torch.uint8)
        b = self._buffers((), False)
        io = self._io(b)
        _lib.check(self.lib.xv_anyhvac_reset_injected(self._h, _lib.ptr(m), _lib.ptr(g), C.byref(io)))
        self.need_reset = False
        return self._obs(b)

    def _require_reset(self):
        if (not self.task_set) or self.need_reset:
            raise Exception("Must \"set_task\" and \"reset\" before doing any actions")

    def step(self, actions):
        self._require_reset()
        a = self._actions(actions)
        b = self._buffers((), self.autoreset_mode == "same_step")
        io = self._io(b, a)
        _lib.check(self.lib.xv_anyhvac_step(self._h, C.byref(io), AUTORESET[self.autoreset_mode]))
        return self._result(b)

    def step_injected(self, actions, reset_state):
        self._require_reset()
        a, g = self._actions(actions), self._pad_grid(reset_state)
        b = self._buffers((), self.autoreset_mode == "same_step")
        io = self._io(b, a)
        _lib.check(self.lib.xv_anyhvac_step_injected(self._h, C.byref(io), _lib.ptr(g), AUTORESET[self.autoreset_mode]))
        return self._result(b)

    def rollout(self, actions):
        """actions float32[T, N, C] -> (obs, reward, terminated, truncated, info) with a leading T on every tensor, from ONE
        launch; bit-equal to T calls of step()"""
        self._require_reset()
        T = int(torch.as_tensor(actions).shape[0]) if not torch.is_tensor(actions) else int(actions.shape[0])
        a = self._actions(actions, (T,))
        b = self._buffers((T,), self.autoreset_mode == "same_step")
        io = self._io(b, a)
        _lib.check(self.lib.xv_anyhvac_rollout(self._h, T, C.byref(io), AUTORESET[self.autoreset_mode]))
        return self._result(b)

    # -- state ----------------------------------------------------------------------------------------------------
    def _state_shapes(self):
        NW, NL, Cc = self.dims[:3]
        n, R = self.num_envs, RING_CAPACITY
        return dict(grid=(n, NW * NL), t=(n,), last_call=(n,), episode_step=(n,), warning_count=(n,), rest_idx=(n,),
                    rest_start=(n, Cc), value=(n, Cc), filter=(n, Cc), ring_t=(n, R), ring_v=(n, R, Cc), head=(n, Cc),
                    tail=(n,))

    def get_state(self):
        """-> dict of device tensors: grid [N, NW * NL], t, last_call (NaN: none since the reset), episode_step,
        warning_count, rest_idx, rest_start [N, C], value [N, C] (the current action), filter [N, C], the delay rings
        ring_t [N, 256], ring_v [N, 256, C] with head [N, C] and tail [N].  (The energy accumulator lives within a step.)"""
        self._require_task()
        st = _lib.AnyHVACState()
        out = {}
        for k, shape in self._state_shapes().items():
            out[k] = torch.empty(shape, dtype=_STATE_DTYPES[k], device=self.device)
            setattr(st, k, out[k].data_ptr())
        _lib.check(self.lib.xv_anyhvac_get_state(self._h, C.byref(st)))
        self.engine.sync()
        return out

    def set_state(self, **state):
        """any subset of get_state()'s entries"""
        self._require_task()
        st = _lib.AnyHVACState()
        shapes, keep = self._state_shapes(), []
        for k, v in state.items():
            if k not in shapes:
                raise ValueError("unknown state entry %r" % (k,))
            t = self._dev(v, _STATE_DTYPES[k])
            if tuple(t.shape) != shapes[k]:
                raise ValueError("state entry %s must have shape %s" % (k, shapes[k]))
            keep.append(t)
            setattr(st, k, t.data_ptr())
        _lib.check(self.lib.xv_anyhvac_set_state(self._h, C.byref(st)))
        self.engine.sync()
        self.need_reset = False

    def sample_action(self, mode="constant"):
        """anyhvac_env.py:653-678 for the C value columns: 'max' (all zeros: the lowest set temperature), 'constant' (the
        target temperature), 'constant_conservative' (5 K below it) -> float32 [N, C]"""
        Cc = self.dims[2]
        if mode == "max":
            v = np.zeros(self.num_envs)
        elif mode == "constant":
            v = (self._targets - self.lower_bound) / (self.upper_bound - self.lower_bound)
        elif mode == "constant_conservative":
            v = (self._targets - 5 - self.lower_bound) / (self.upper_bound - self.lower_bound)
        else:
            raise ValueError(f"Unsupported mode: {mode}")
        a = np.repeat(v[:, None], Cc, axis=1).astype(np.float32)
        return self._out(torch.from_numpy(a).to(self.device))

    def close_extras(self, **kwargs):
        if self._h is not None:
            self.lib.xv_anyhvac_destroy(self._h)
            self._h = None


class HVACEnv(object):
    """one room with the reference's surface: HVACEnv(**keywords); set_task(task, generate_task=False); reset() ->
    (obs, info); step(action[C]) -> (obs, reward, terminated, truncated, info), numpy arrays of the room's true sizes.
    The episode is not reset behind the caller's back (autoreset_mode='disabled')."""

    def __init__(self, max_steps=20160, iter_per_step=200, sec_per_iter=0.15, set_lower_bound=16, set_upper_bound=32,
                 verbose=False, action_space_format='box', include_heat_in_observation=True,
                 include_switch_in_observation=False, include_last_action_in_observation=True,
                 include_timestep_in_observation=True, no_switch_action=True, reward_mode=0, device="cuda:0", seed=0):
        self.vec = HVACVecEnv(1, max_steps=max_steps, iter_per_step=iter_per_step, sec_per_iter=sec_per_iter,
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

    def reset(self, *args, state=None, **kwargs):
        """state: the initial grid [n_width, n_length] (otherwise ambient + 2 N(0, 1) from the engine's Philox stream)"""
        if state is None:
            obs, _ = self.vec.reset()
        else:
            obs = self.vec.reset_injected(np.asarray(state, np.float64)[None])
        return self._np(obs), {"time": 0.0}

    def step(self, action):
        a = np.zeros((1, self.vec.dims[2]), np.float32)
        n = int(self.vec.counts["coolers"][0])
        a[0, :n] = np.asarray(action, np.float32).reshape(-1)[:n]
        obs, r, term, trunc, info = self.vec.step(a)
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
