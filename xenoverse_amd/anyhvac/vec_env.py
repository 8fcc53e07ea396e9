"""HVACVecEnv — batched AnyHVAC rooms on the device (csrc/anyhvac.hip, include/xeno.h xv_anyhvac_*): one launch steps every
room, one workgroup per room.  (HVACEnv, the one-room wrapper with the reference's surface: single_env.py.)

Observations are dicts of tensors padded to the batch's largest room — sensor_readings[N, S], heat_readings[N, H],
action_temp[N, C] (float32), timestep[N] (int32) — with `counts` (per env: coolers, sensors, heaters, n_width, n_length)
beside them; padded columns are zero and padded action columns are ignored.  Rewards are float64.  Same-step autoreset (the
engine's default) hands out the new episode's first observation and the finished one's last under info["final_obs"];
autoreset_mode="disabled" goes on stepping as the reference's env would; "next_step" is not built.

The PID teachers (pid.py restates the reference's solvers on the host): set_pid() puts a controller with per-env gains on
the device, pid_action() makes one controller call, rollout_teacher(T) runs T controller-driven steps in ONE launch.
HVACSolverGTPID / HVACSolverLOCPID / HVACSolverGridSearchPID (solvers.py) are the reference-shaped classes over the one-room
HVACEnv; the grid search evaluates its candidates as the envs of one batch.

The RL action spaces (actions.py restates the reference's classes on the host): HVACVecEnv(action_mode="discrete" | "diff")
maps every step's raw actions inside the step kernel — float32 [N, C], or under action_mode="diff" with
discretize_rl_action_space=True an integer tensor of bins 0...12 — and adds info["applied_value"], info["delta"],
info["action_cost"] (with add_action_cost) and info["step_stat"].  HVACEnvDiscreteAction / HVACEnvDiffAction
(single_env.py) are the reference-shaped one-room classes.

The episode protocol of the reference's RL trainer: set_random_start_t, set_generate_record and
set_overheat_no_termiated_training_only take a bool or a bool[num_envs] and hold from the next reset (the last: the next
step) on; the start logic runs inside every reset the device makes, same-step autoresets included (host.py restates it).
"""
import ctypes as C

import numpy as np
import torch

from .. import _lib
from ..engine import AUTORESET
from ..spaces import Box, MultiDiscrete
from ..vector import VectorEnv
from .actions import ACTION_MODES, COST_TABLE, N_BINS, STAT_KEYS
from .config import RING_CAPACITY
from .host import (HISTORY_RING, START_NO_TERMINATE, START_RANDOM, START_RECORD, check_ring, check_settings, start_cdf)
from .pid import DEFAULT_GAINS, GAINS, pid_weights
from .tables import build_tables, task_doubles

OBS_KEYS = ("sensor_readings", "heat_readings", "action_temp", "timestep")
MISC = ("over_heat", "over_tolerace", "energy_cost", "target_cost", "time", "rest_idx", "warning_count", "episode_step")
_COST_TABLE = np.ascontiguousarray(COST_TABLE, np.float64)
_f64, _f32, _i64, _i32, _i16 = torch.float64, torch.float32, torch.int64, torch.int32, torch.int16
# Every entry of the handle's state: name -> (group, dtype, shape behind [num_envs] from dims d = (NW, NL, C, S, H, KS, KH)).
# Within a group the entries stand in the order of the C call's pointers: xv_anyhvac_state's fields for "env", the
# arguments of xv_anyhvac_<group>_get_state / _set_state for "start", "act" and "pid".
_STATE = {
    "grid": ("env", _f64, lambda d: (d[0] * d[1],)), "t": ("env", _f64, lambda d: ()), "last_call": ("env", _f64, lambda d: ()),
    "episode_step": ("env", _i32, lambda d: ()), "warning_count": ("env", _i32, lambda d: ()),
    "rest_idx": ("env", _i32, lambda d: ()), "rest_start": ("env", _f64, lambda d: (d[2],)),
    "value": ("env", _f32, lambda d: (d[2],)), "filter": ("env", _f64, lambda d: (d[2],)),
    "ring_t": ("env", _f64, lambda d: (RING_CAPACITY,)), "ring_v": ("env", _f64, lambda d: (RING_CAPACITY, d[2])),
    "head": ("env", _i32, lambda d: (d[2],)), "tail": ("env", _i32, lambda d: ()),
    "last_fail": ("start", _f64, lambda d: ()), "history": ("start", _i16, lambda d: (HISTORY_RING,)),
    "history_count": ("start", _i32, lambda d: ()),
    "window": ("act", _i64, lambda d: (d[2],)),
    "acc_diff": ("pid", _f64, lambda d: (d[3],)), "last_obs": ("pid", _f32, lambda d: (d[3],)), "fresh": ("pid", _i32, lambda d: ()),
}
assert tuple(k for k, v in _STATE.items() if v[0] == "env") == _lib.AnyHVACState.FIELDS


class HVACVecEnv(VectorEnv):
    def __init__(self, num_envs, max_steps=20160, iter_per_step=200, sec_per_iter=0.15, set_lower_bound=16,
                 set_upper_bound=32, reward_mode=0, include_heat_in_observation=True,
                 include_last_action_in_observation=True, include_timestep_in_observation=True, device="cuda:0", seed=0,
                 env_id_base=0, autoreset_mode="same_step", to_numpy=False, engine=None, action_mode="box",
                 discretize_rl_action_space=False, add_action_cost=False, too_cold_limit=True, **excluded):
        check_settings(**excluded)
        if action_mode not in ACTION_MODES:
            raise ValueError("action_mode must be one of %s" % (ACTION_MODES,))
        if action_mode != "diff" and (discretize_rl_action_space or add_action_cost):
            raise ValueError("discretize_rl_action_space and add_action_cost belong to action_mode='diff'")
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
        self.action_mode = action_mode
        self.discretize_rl_action_space, self.add_action_cost = bool(discretize_rl_action_space), bool(add_action_cost)
        self.too_cold_limit = bool(too_cold_limit)
        self._h = None
        self._pid = None
        self._task_list = self._task_tables = None
        self.need_reset = True
        self._start_flags = np.zeros(self.num_envs, np.uint8)
        self._start_cdf = self._start_u = None

    # -- the episode start ----------------------------------------------------------------------------------------
    def _set_start_flag(self, bit, on):
        on = np.broadcast_to(np.asarray(on, bool), (self.num_envs,))
        self._start_flags = np.where(on, self._start_flags | bit, self._start_flags & ~np.uint8(bit)).astype(np.uint8)
        if self._h is not None:
            self._push_start_mode()

    def set_random_start_t(self, random_start_t):
        """a bool or bool[num_envs]: from the next reset on an episode starts as the reference's does under random_start_t
        (100 steps before the last failure, else at a random time of the week)"""
        self._set_start_flag(START_RANDOM, random_start_t)

    def set_generate_record(self, generate_record):
        """a bool or bool[num_envs]: with random_start_t, every reset starts at a uniform step and forgets the history"""
        self._set_start_flag(START_RECORD, generate_record)

    def set_overheat_no_termiated_training_only(self, overheat_no_termiated_training_only):
        """a bool or bool[num_envs]: a failing step still returns -30 and over_tolerace = 1 but terminated = False"""
        self._set_start_flag(START_NO_TERMINATE, overheat_no_termiated_training_only)

    def _push_start_mode(self):
        """the flags, and with the first env that may take the choice branch the table of numpy's choice (once per
        handle: max_t + 1 doubles, shared among the envs), to the handle"""
        cdf, n = None, 0
        if ((self._start_flags & (START_RANDOM | START_RECORD)) == START_RANDOM).any() and not self._cdf_on_handle:
            if self._start_cdf is None:
                self._start_cdf = np.ascontiguousarray(start_cdf(int(self.max_steps * self.iter_per_step * self.sec_per_iter)))
            cdf, n = self._start_cdf.ctypes.data_as(C.c_void_p), len(self._start_cdf)
        flags = np.ascontiguousarray(self._start_flags)
        _lib.check(self.lib.xv_anyhvac_set_start_mode(self._h, flags.ctypes.data_as(C.c_void_p), self.max_steps, cdf, n))
        self._cdf_on_handle = self._cdf_on_handle or cdf is not None

    def _start_draws(self, start_u):
        """start_u float64 [N, 2] (u0, u1) or None -> the handle's injected start draws for the next *_injected call"""
        u = None
        if start_u is not None:
            u = self._dev(start_u, torch.float64)
            if tuple(u.shape) != (self.num_envs, 2):
                raise ValueError("start_u must have shape %s" % ((self.num_envs, 2),))
            u = u.contiguous()
        if u is not None or self._start_u is not None:
            _lib.check(self.lib.xv_anyhvac_set_start_draws(self._h, _lib.ptr(u)))
        self._start_u = u      # (borrowed by the handle: alive until the next call replaces it)

    # -- tasks ----------------------------------------------------------------------------------------------------
    def set_task(self, tasks, env_task_index=None, generate_task=False):
        """tasks: one flat task dict (task_sampler.py) or a list; envs share tasks through env_task_index (default: equal
        blocks).  generate_task=True takes avg_total_heat = 10000 as the reference does, False forms the reference's
        week-long average (host.average_total_heat).
        A dict with a `table` key is the result of anyhvac.sample_tasks_device: its device rows are borrowed as they are (no
        host copy); its set bounds and generate_task must be this call's, and flat dicts are made from it only when
        something asks for them (set_pid(weights=None), the solver classes)."""
        if isinstance(tasks, dict) and "table" in tasks:
            return self._set_task_device(tasks, env_task_index, generate_task)
        if isinstance(tasks, dict):
            tasks = [tasks]
        n_task, d = len(tasks), self.device
        for t in tasks:
            check_ring(t["cooler_delay_seconds"], self.sec_per_iter)
        env_task_dev = self._env_task(n_task, env_task_index)
        tab = build_tables(tasks, self.lower_bound, self.upper_bound, generate_task)
        targets = np.array([float(t["target_temperature"]) for t in tasks])
        self._finish_task(tab["dims"], torch.from_numpy(tab["table"]).to(d), env_task_dev,
                          {k: np.array([c[q] for c in tab["counts"]], np.int32) for k, q in
                           (("coolers", "C"), ("sensors", "S"), ("heaters", "H"), ("n_width", "nw"), ("n_length", "nl"))},
                          targets, np.array([(v - self.lower_bound) / (self.upper_bound - self.lower_bound) for v in targets]),
                          tab["avg_total_heat"], generate_task)
        self._task_list, self._task_tables = list(tasks), None

    def _finish_task(self, dims, table, env_task_dev, counts, targets, default_action_value, avg_total_heat, generate_task):
        """what both set_task paths end with.  counts {name: int32 [n_task]}, targets and default_action_value float64
        [n_task], avg_total_heat [n_task]: per task; the per-env attributes are read off them through the env -> task map"""
        env_task = env_task_dev.cpu().numpy()      # (the per-env counts and targets are host arrays)
        self.dims = dims
        self.avg_total_heat = avg_total_heat
        self.counts = {k: v[env_task] for k, v in counts.items()}
        self._tab = dict(table=table, env_task=env_task_dev)
        self._bind_tables(int(table.shape[0]))
        self.default_action_value, self._targets = default_action_value[env_task], targets[env_task]
        self._generate_task = bool(generate_task)
        self.task_set = True
        self.need_reset = True

    def _bind_tables(self, n_task):
        """a handle for self.dims over self._tab, the spaces"""
        NW, NL, Cc, S, H, KS, KH = self.dims
        self.close_extras()
        h = C.c_void_p()
        max_t = int(self.max_steps * self.iter_per_step * self.sec_per_iter)
        _lib.check(self.lib.xv_anyhvac_create(self.engine.handle, self.num_envs, NW, NL, Cc, S, H, KS, KH, self.iter_per_step,
                                              self.sec_per_iter, float(self.lower_bound), float(self.upper_bound),
                                              float(max_t), self.reward_mode, C.byref(h)))
        self._h = h
        self._cdf_on_handle = False      # (a new handle: no failure behind any env, empty histories, no table)
        self._push_start_mode()
        _lib.check(self.lib.xv_anyhvac_set_task(h, n_task, _lib.ptr(self._tab["table"]), _lib.ptr(self._tab["env_task"])))
        self._push_action_mode()
        if self.action_mode == "diff" and self.discretize_rl_action_space:
            self._set_spaces(None, MultiDiscrete([N_BINS] * Cc))
        else:
            self._set_spaces(None, Box(0.0, 1.0, shape=(Cc,), dtype=np.float32))
        self.single_observation_spaces = dict(
            sensor_readings=Box(10, 50, shape=(S,), dtype=np.float32), heat_readings=Box(0.0, 50000.0, shape=(H,)),
            action_temp=Box(-1, 33, shape=(Cc,)), timestep=Box(0, 30000, shape=(1,), dtype=np.int32))

    def _set_task_device(self, tables, env_task_index, generate_task):
        """set_task over the device tables of anyhvac.sample_tasks_device"""
        table = tables["table"]
        dims = tuple(int(v) for v in tables["dims"])
        # (self.device is the engine's: a torch.device with its index resolved, also when the env was built with 'cuda')
        if not torch.is_tensor(table) or table.dtype != torch.float64 or table.device != self.device \
                or not table.is_contiguous() or table.ndim != 2 or table.shape[1] != task_doubles(*dims):
            raise ValueError("tables['table'] must be a contiguous float64 tensor [n_task, %d] on %s"
                             % (task_doubles(*dims), self.device))
        check_settings(control_type=tables.get("control_type", "Temperature"))
        if float(tables["set_lower_bound"]) != float(self.lower_bound) or \
                float(tables["set_upper_bound"]) != float(self.upper_bound):
            raise ValueError("the tables were sampled for set bounds (%g, %g), this env has (%g, %g)"
                             % (tables["set_lower_bound"], tables["set_upper_bound"], self.lower_bound, self.upper_bound))
        if bool(tables["generate_task"]) != bool(generate_task):
            raise ValueError("the tables were sampled with generate_task=%r, set_task was called with generate_task=%r"
                             % (bool(tables["generate_task"]), bool(generate_task)))
        check_ring(float(tables["delay_high"]), self.sec_per_iter)
        env_task_dev = self._env_task(int(table.shape[0]), env_task_index)
        # one small read-back: the counts, and the target / average heat / default action columns of the rows
        small = torch.cat([tables["counts"].to(torch.float64), table[:, [9, 10, 14]]], dim=1).cpu().numpy()
        self._finish_task(dims, table, env_task_dev,
                          {k: small[:, j].astype(np.int32) for j, k in
                           enumerate(("n_width", "n_length", "coolers", "sensors", "heaters"))},
                          small[:, 5], small[:, 7], [float(v) for v in small[:, 6]], generate_task)
        self._task_list, self._task_tables = None, tables

    @property
    def _tasks(self):
        """the flat task dicts; made from device tables the first time something needs them"""
        if self._task_list is None and self._task_tables is not None:
            from .device_sampler import task_dicts_from_device
            self._task_list = task_dicts_from_device(self._task_tables)
        return self._task_list

    @_tasks.setter
    def _tasks(self, tasks):
        self._task_list = tasks

    def _push_action_mode(self):
        if self.action_mode == "box":
            return
        flags = 0
        if self.action_mode == "diff":
            flags = (1 if self.add_action_cost else 0) | (2 if self.too_cold_limit else 0)
        _lib.check(self.lib.xv_anyhvac_set_action_mode(self._h, ACTION_MODES.index(self.action_mode), flags,
                                                       _COST_TABLE.ctypes.data_as(C.c_void_p)))

    def set_too_cold_limit(self, too_cold_limit):
        """the reference's setter: from the next step on; the action windows are kept"""
        if self.action_mode != "diff":
            raise ValueError("too_cold_limit belongs to action_mode='diff'")
        self.too_cold_limit = bool(too_cold_limit)
        if self._h is not None:
            self._push_action_mode()      # (the mode stays: only the flags change)

    def _set_spaces(self, single_obs, single_act):
        self.single_observation_space = self.observation_space = single_obs
        self.single_action_space = single_act
        from ..spaces import batch_space
        self.action_space = batch_space(single_act, self.num_envs)

    # -- buffers --------------------------------------------------------------------------------------------------
    def _buffers(self, lead, final):
        NW, NL, Cc, S, H, _, _ = self.dims
        f32, f64, i32, u8 = torch.float32, torch.float64, torch.int32, torch.uint8
        spec = [("sensor_readings", f32, (S,)), ("heat_readings", f32, (H,)), ("action_temp", f32, (Cc,)), ("timestep", i32, ()),
                ("reward", f64, ()), ("terminated", u8, ()), ("truncated", u8, ()), ("cool_power", f32, (Cc,)),
                ("heat_power", f64, (H,)), ("misc", f64, (8,))]      # (the first four: OBS_KEYS)
        if self.action_mode != "box":
            spec += [("applied_value", f32, (Cc,)), ("delta", f64, (Cc,)), ("action_cost", f64, ()),
                     ("stat_counts", i32, (len(STAT_KEYS),))]
        if final:
            spec += [("final_" + f[0],) + f[1:] for f in spec[:len(OBS_KEYS)]]
        return self._alloc([f + (0,) for f in spec], lead)      # zero-filled: the padded columns are never written

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
        if self.action_mode != "box":
            info["applied_value"], info["delta"] = self._out(b["applied_value"]), self._out(b["delta"])
            if self.add_action_cost:
                info["action_cost"] = self._out(b["action_cost"])
            stat = {k: self._out(b["stat_counts"][..., i]) for i, k in enumerate(STAT_KEYS)}
            stat.update(fail=self._out(b["terminated"].to(torch.int32)), reward=self._out(b["reward"]),
                        cooler_power=self._out(torch.round(b["cool_power"].sum(-1), decimals=4)))
            info["step_stat"] = stat
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

    def _run(self, actions=None, rollout=False, injected=False, reset_state=None, start_u=None, teacher=None):
        """THE step-family call, one launch: step(), step_injected() (injected), rollout() (actions [T, N, C]) or
        rollout_teacher() (teacher = (T, action_out, stats): the controller acts, there are no actions)"""
        a = idx = g = None
        if teacher is not None:
            lead = (teacher[0],)
        else:
            integer = self.action_mode != "box" and (
                (actions.dtype in (torch.int32, torch.int64)) if torch.is_tensor(actions) else
                np.issubdtype(np.asarray(actions).dtype, np.integer))
            if integer and not (self.action_mode == "diff" and self.discretize_rl_action_space):
                raise ValueError("integer actions need action_mode='diff' with discretize_rl_action_space=True")
            a = self._dev(actions, torch.int32 if integer else torch.float32)
            lead = (int(a.shape[0]),) if rollout else ()
            if a.shape != lead + (self.num_envs, self.dims[2]):
                raise ValueError("actions must have shape %s" % (lead + (self.num_envs, self.dims[2]),))
            if integer:
                a, idx = None, a
        if injected:
            g = self._pad_grid(reset_state)
            self._start_draws(start_u)
        b = self._buffers(lead, self.autoreset_mode == "same_step")
        io = self._io(b, a)
        name, args = "rollout" if lead else "step", list(lead) + [C.byref(io)]
        if self.action_mode != "box":
            act = _lib.AnyHVACActIO()
            act.action_index = _lib.ptr(idx)
            for k in _lib.AnyHVACActIO.FIELDS[1:]:
                setattr(act, k, b[k].data_ptr())
            name, args = name + "_mapped", args + [C.byref(act)]
        elif teacher is not None:
            name, args = name + "_pid", args + [_lib.ptr(teacher[1]), _lib.ptr(teacher[2])]
        if injected:
            name, args = name + "_injected", args + [_lib.ptr(g)]
        _lib.check(getattr(self.lib, "xv_anyhvac_" + name)(self._h, *args, AUTORESET[self.autoreset_mode]))
        if teacher is None:
            self._pid_follow(b)      # (box mode alone has a controller to follow)
        return self._result(b)

    # -- state ----------------------------------------------------------------------------------------------------
    def _state_call(self, verb, ts):
        """one xv_anyhvac_[<group>_]<verb>_state call per group that has an entry in ts (name -> tensor), then a sync"""
        for group in dict.fromkeys(_STATE[k][0] for k in ts):
            names = [k for k, v in _STATE.items() if v[0] == group]
            if group == "env":
                st = _lib.AnyHVACState()
                for k in names:
                    setattr(st, k, _lib.ptr(ts.get(k)))
                _lib.check(getattr(self.lib, "xv_anyhvac_%s_state" % verb)(self._h, C.byref(st)))
            else:
                _lib.check(getattr(self.lib, "xv_anyhvac_%s_%s_state" % (group, verb))(self._h, *[_lib.ptr(ts.get(k)) for k in names]))
        self.engine.sync()

    def _get_state(self, groups, only=None):
        out = {k: torch.empty((self.num_envs,) + shape(self.dims), dtype=dtype, device=self.device)
               for k, (group, dtype, shape) in _STATE.items() if group in groups and (only is None or k in only)}
        self._state_call("get", out)
        return out

    def _set_state(self, groups, what, state):
        """what: how the error texts call an entry of these groups"""
        ts = {}
        for k, v in state.items():
            if k not in _STATE or _STATE[k][0] not in groups:
                raise ValueError("unknown %s%r" % (what, k))
            ts[k] = self._dev(v, _STATE[k][1])
            shape = (self.num_envs,) + _STATE[k][2](self.dims)
            if tuple(ts[k].shape) != shape:
                raise ValueError("%s%s must have shape %s" % (what, k, shape))
        self._state_call("set", ts)

    def _require_act_state(self):
        self._require_task()
        if self.action_mode == "box":
            raise ValueError("action_mode='box' keeps no action state")

    def get_act_state(self):
        """-> dict(window int64 [N, C]): per cooler the last <= 10 bins of the action cost's window, 4 bits per entry holding
        bin + 1, the newest lowest, 0 = empty"""
        self._require_act_state()
        return self._get_state(("act",))

    def set_act_state(self, window):
        self._require_act_state()
        self._set_state(("act",), "", dict(window=window))

    # -- episode --------------------------------------------------------------------------------------------------
    def reset(self, *, seed=None, options=None):
        mask = self._reset_prelude(seed, options)
        b = self._buffers((), False)
        io = self._io(b)
        _lib.check(self.lib.xv_anyhvac_reset(self._h, _lib.ptr(mask), C.byref(io)))
        self.need_reset = False
        if self._pid is not None:
            self.pid_reset(mask)
        return self._obs(b), {}

    def reset_injected(self, state, mask=None, start_u=None):
        """reset with the initial grid given: state [N, nw, nl] (rooms smaller than the batch's largest: zero-padded);
        start_u float64 [N, 2]: the uniforms (u0, u1) of the start draw under random_start_t (default: the engine's)"""
        self._require_task()
        g = self._pad_grid(state)
        self._start_draws(start_u)
        m = None if mask is None else self._dev(mask, torch.uint8)
        b = self._buffers((), False)
        io = self._io(b)
        _lib.check(self.lib.xv_anyhvac_reset_injected(self._h, _lib.ptr(m), _lib.ptr(g), C.byref(io)))
        self.need_reset = False
        if self._pid is not None:
            self.pid_reset(m)
        return self._obs(b)

    def step(self, actions):
        self._require_reset()
        return self._run(actions)

    def step_injected(self, actions, reset_state, start_u=None):
        self._require_reset()
        return self._run(actions, injected=True, reset_state=reset_state, start_u=start_u)

    def rollout(self, actions):
        """actions float32[T, N, C] -> (obs, reward, terminated, truncated, info) with a leading T on every tensor, from ONE
        launch; bit-equal to T calls of step()"""
        self._require_reset()
        return self._run(actions, rollout=True)

    # -- the PID teacher -------------------------------------------------------------------------------------------
    def set_pid(self, kind="gt", kp=DEFAULT_GAINS["kp"], ki=DEFAULT_GAINS["ki"], kd=DEFAULT_GAINS["kd"], gains="python",
                weights=None):
        """put the reference's PID controller on the device.  kind: 'gt' (HVACSolverGTPID's weights) or 'loc'
        (HVACSolverLOCPID's); weights: one float64 [S_task, C_task] matrix per task instead.  kp, ki, kd: scalars or [N]
        arrays, one triple per env.  gains: 'python' (the arithmetic of Python-float gains, the solvers' defaults) or
        'float64' (of numpy.float64 gains, the grid search's).  The controllers start as new solvers do."""
        if self.action_mode != "box":
            raise ValueError("the PID teachers put out box actions: set_pid needs action_mode='box'")
        self._require_task()
        if gains not in GAINS:
            raise ValueError("gains must be one of %s" % (GAINS,))
        Cc, S = self.dims[2], self.dims[3]
        if weights is None:
            weights = [pid_weights(t, kind) for t in self._tasks]
        elif isinstance(weights, np.ndarray) and weights.ndim == 2:
            weights = [weights]
        if len(weights) != len(self._tasks):
            raise ValueError("weights: one [sensors, coolers] matrix per task")
        w = np.zeros((len(self._tasks), S, Cc))
        for i, (m, t) in enumerate(zip(weights, self._tasks)):
            m = np.asarray(m, np.float64)
            if m.shape != (len(t["sensor_loc"]), len(t["cooler_loc"])):
                raise ValueError("weights of task %d must have shape %s" % (i, (len(t["sensor_loc"]), len(t["cooler_loc"]))))
            w[i, :m.shape[0], :m.shape[1]] = m
        g = np.stack([np.broadcast_to(np.asarray(v, np.float64), (self.num_envs,)) for v in (kp, ki, kd)], axis=1)
        pid = dict(weights=torch.from_numpy(w).to(self.device), gains=torch.from_numpy(np.ascontiguousarray(g)).to(self.device))
        _lib.check(self.lib.xv_anyhvac_set_pid(self._h, _lib.ptr(pid["weights"]), _lib.ptr(pid["gains"]),
                                               1 if gains == "float64" else 0))
        self.engine.sync()
        self._pid = pid      # (the handle borrows both tensors)

    def _require_pid(self):
        self._require_task()
        if self._pid is None:
            raise Exception("Must \"set_pid\" before asking the teacher")

    def pid_action(self, sensor_readings=None, return_flat=False):
        """one controller call per env, no step -> the env's action float32 [N, C] (1 - value; padded columns 0).
        sensor_readings: float32 [N, S], default the envs' current observation.  return_flat: also the reference's flat
        action as float32 [N, 2, C] (switch row, value row).  The controllers' state advances."""
        self._require_pid()
        Cc, S = self.dims[2], self.dims[3]
        r = None
        if sensor_readings is not None:
            r = self._dev(sensor_readings, torch.float32)
            if r.shape != (self.num_envs, S):
                raise ValueError("sensor_readings must have shape %s" % ((self.num_envs, S),))
        else:
            self._require_reset()
        act = torch.zeros((self.num_envs, Cc), dtype=torch.float32, device=self.device)
        flat = torch.zeros((self.num_envs, 2, Cc), dtype=torch.float32, device=self.device) if return_flat else None
        _lib.check(self.lib.xv_anyhvac_pid_action(self._h, _lib.ptr(r), _lib.ptr(act), _lib.ptr(flat)))
        if r is not None:
            self.engine.sync()      # (r may be a temporary)
        return (self._out(act), self._out(flat)) if return_flat else self._out(act)

    def rollout_teacher(self, T, return_stats=False, stats=None):
        """T controller-driven steps in ONE launch -> rollout()'s tuple with info["action"] float32 [T, N, C] (what the
        teacher did); bit-equal to T rounds of pid_action() + step().  return_stats: info["pid_stats"] float64 [N, 8] over
        the T steps' resulting readings of the real sensors, e = reading - target in float32: sum |e|, max |e|, sum e^2,
        count(|e| <= 1), count(|e| <= 2), count(reading > target + 2), sum of rewards, sample count.  stats: a tensor
        of an earlier call to go on accumulating into."""
        if self.action_mode != "box":
            raise ValueError("the PID teachers put out box actions: rollout_teacher needs action_mode='box'")
        self._require_pid()
        self._require_reset()
        T = int(T)
        act = torch.zeros((T, self.num_envs, self.dims[2]), dtype=torch.float32, device=self.device)
        if stats is None and return_stats:
            stats = torch.zeros((self.num_envs, 8), dtype=torch.float64, device=self.device)
        if stats is not None and (stats.shape != (self.num_envs, 8) or stats.dtype != torch.float64
                                  or stats.device != self.device or not stats.is_contiguous()):
            raise ValueError("stats must be a contiguous float64 [num_envs, 8] tensor on the env's device")
        out = self._run(teacher=(T, act, stats))
        out[4]["action"] = self._out(act)
        if stats is not None:
            out[4]["pid_stats"] = self._out(stats)
        return out

    def pid_reset(self, mask=None):
        """acc_diff = 0, last observation = 0 for the envs of mask (default all): a new solver's state"""
        self._require_pid()
        m = None if mask is None else self._dev(mask, torch.uint8)
        _lib.check(self.lib.xv_anyhvac_pid_reset(self._h, _lib.ptr(m)))
        self._pid["mask"] = m      # (kept alive until the next call's replaces it)

    def _pid_follow(self, b):
        """after step() / rollout() under same-step autoreset: an env that was reset gets a fresh controller, as inside
        rollout_teacher()"""
        if self._pid is not None and self.autoreset_mode == "same_step":
            done = b["terminated"] | b["truncated"]
            self.pid_reset(done if done.dim() == 1 else done.amax(0))

    def get_pid_state(self):
        """-> dict of device tensors: acc_diff float64 [N, S], last_obs float32 [N, S], fresh int32 [N] (1 from a reset
        to the first controller call)"""
        self._require_pid()
        return self._get_state(("pid",))

    def set_pid_state(self, **state):
        """any subset of get_pid_state()'s entries"""
        self._require_pid()
        self._set_state(("pid",), "PID state entry ", state)

    def get_state(self, only=None):
        """only: a subset of the entries' names (default all).  -> dict of device tensors: grid [N, NW * NL], t, last_call
        (NaN: none since the reset), episode_step,
        warning_count, rest_idx, rest_start [N, C], value [N, C] (the current action), filter [N, C], the delay rings
        ring_t [N, 256], ring_v [N, 256, C] with head [N, C] and tail [N]; last_fail [N] (-1: none yet), history int16
        [N, 128] — the rest indices of the last steps that did not fail, a ring whose next slot is history_count % 128 — and
        history_count [N] (min(count, 1000) is the reference's history length).  (The energy accumulator lives within a
        step.)"""
        self._require_task()
        return self._get_state(("env", "start"), only)

    def set_state(self, **state):
        """any subset of get_state()'s entries"""
        self._require_task()
        self._set_state(("env", "start"), "state entry ", state)
        self.need_reset = False

    def time(self):
        """-> the envs' t as a float64 numpy array [N] (one small read-back)"""
        return self.get_state(only=("t",))["t"].cpu().numpy()

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
        self._pid = None
