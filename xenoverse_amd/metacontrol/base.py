"""ControlVecEnv — what the one-lane-per-env control families (cartpole.py, acrobot.py) share: everything around the
physics.  The native side is csrc/xv_control.h; a family states its C prefix, observation width, task keys and how it
reads `reset_bounds_scale`, and passes its spaces to the constructor.
"""
import ctypes as C

import numpy as np
import torch

from .. import _lib
from ..engine import AUTORESET
from ..vector import VectorEnv

_CALLS = ("create", "destroy", "reset", "reset_injected", "rollout", "step_injected", "get_state", "set_state")


def _versatile(setting, default_range, default_value, rng):
    # utils/tools.py:47-54
    if isinstance(setting, (tuple, list)):
        assert len(setting) == 2, f"Setting must be a tuple or list of length 2, got {len(setting)}"
        return float(rng.uniform(setting[0], setting[1]))
    if setting:
        return float(rng.uniform(default_range[0], default_range[1]))
    return default_value


class ControlVecEnv(VectorEnv):
    PREFIX = None        # "xv_<family>": the family's entry points in include/xeno.h
    OBS_DIM = None
    TASK_KEYS = ()       # the columns of a parameter row, as keys of a task dict

    def __init__(self, num_envs, frameskip, reset_bounds_scale, max_steps, observation_space, action_space, **kwargs):
        super().__init__(num_envs, **kwargs)
        self.frameskip = int(frameskip)
        self.reset_bounds_scale = self._read_scale(reset_bounds_scale)
        self.max_steps = int(max_steps)
        self._set_spaces(observation_space, action_space)
        for name in _CALLS:
            setattr(self, "_c_" + name, getattr(self.lib, "%s_%s" % (self.PREFIX, name)))
        self._h = None

    def _read_scale(self, scale):
        """reset_bounds_scale as the constructor received it -> float64[4]"""
        raise NotImplementedError

    def _create_extras(self):
        """the family's own arguments of xv_*_create, between reset_scale and env_task"""
        return ()

    def set_task(self, tasks, env_task_index=None):
        if isinstance(tasks, dict):
            tasks = [tasks]
        params = np.array([[t[k] for k in self.TASK_KEYS] for t in tasks], np.float64)
        d = self.device
        n_task = len(tasks)
        self._tab = dict(params=torch.from_numpy(params).to(d), scale=torch.from_numpy(self.reset_bounds_scale).to(d),
                         env_task=self._env_task(n_task, env_task_index))
        self.close_extras()
        h = C.c_void_p()
        _lib.check(self._c_create(self.engine.handle, self.num_envs, n_task, self.frameskip, self.max_steps,
                                  _lib.ptr(self._tab["params"]), _lib.ptr(self._tab["scale"]), *self._create_extras(),
                                  _lib.ptr(self._tab["env_task"]), C.byref(h)))
        self._h = h
        f32, u8, w = torch.float32, torch.uint8, self.OBS_DIM
        fields = [("obs", f32, (w,)), ("fobs", f32, (w,)), ("reward", f32, ()), ("term", u8, ()), ("trunc", u8, ()), ("done", u8, ())]
        self._plain_buffers(fields)
        self._make_step_outputs(fields, ("obs", "reward", "term", "trunc", "fobs", "done"), as_bool=("term", "trunc", "done"))
        self._step_fn = self.PREFIX + "_step_info"
        self.task_set = True
        self.need_reset = True

    def reset(self, *, seed=None, options=None):
        mask = self._reset_prelude(seed, options)
        self._adopt_latest(_obs="obs")
        self._detach("_obs")
        _lib.check(self._c_reset(self._h, _lib.ptr(mask), _lib.ptr(self._obs)))
        self.need_reset = False
        return self._o(self._obs), {}

    def reset_injected(self, u, mask=None):
        self._require_task()
        u = self._dev(u, torch.float64)
        m = None if mask is None else self._dev(mask, torch.uint8)
        self._adopt_latest(_obs="obs")
        self._detach("_obs")
        _lib.check(self._c_reset_injected(self._h, _lib.ptr(m), _lib.ptr(u), _lib.ptr(self._obs)))
        self.need_reset = False
        return self._o(self._obs)

    def _finish(self, s):
        """the output set a step launch has written (all of it, for every env) -> step()'s return value"""
        t = s.t
        infos = {}
        if self._auto == 2:      # same_step
            infos["final_obs"] = t["fobs"]
            if not self.lean_infos:
                infos["_final_obs"] = t["done"]
        if self.to_numpy:
            return self._numpy(t["obs"], t["reward"], t["term"], t["trunc"], infos)
        return t["obs"], t["reward"], t["term"], t["trunc"], infos

    def step(self, actions):
        self._require_reset()
        a = self._dev(actions, torch.int32)
        assert a.shape == (self.num_envs,)
        s = self._outputs.next()
        _lib.step_call(self._step_fn, self._h, a, s, self._auto)      # one launch: the done mask comes from the step kernel
        return self._finish(s)

    def rollout(self, actions, out=None):
        """Fused open-loop roll-out: actions int32[T, N] -> dict of [T, N(, OBS_DIM)] device tensors from one launch with
        the state in registers between the steps; equals T calls of step() bit for bit."""
        self._require_reset()
        a = self._dev(actions, torch.int32).contiguous()
        T, w, f32, u8 = int(a.shape[0]), self.OBS_DIM, torch.float32, torch.uint8
        assert a.shape == (T, self.num_envs)
        if out is None:
            out = self._alloc((("obs", f32, (w,)), ("reward", f32, ()), ("terminated", u8, ()), ("truncated", u8, ()),
                               ("final_obs", f32, (w,))), (T,))
        _lib.check(self._c_rollout(self._h, T, _lib.ptr(a), _lib.ptr(out["obs"]), _lib.ptr(out["reward"]),
                                   _lib.ptr(out["terminated"]), _lib.ptr(out["truncated"]),
                                   _lib.ptr(out.get("final_obs")), AUTORESET[self.autoreset_mode]))
        return out

    def step_injected(self, actions, u_reset):
        a = self._dev(actions, torch.int32)
        u = self._dev(u_reset, torch.float64)
        s = self._outputs.next()
        _lib.check(self._c_step_injected(self._h, _lib.ptr(a), _lib.ptr(u), *s.args[:5], AUTORESET[self.autoreset_mode]))
        if not self.lean_infos:      # the done mask by an op of its own
            torch.bitwise_or(s.t["term"], s.t["trunc"], out=s.t["done"])
        return self._finish(s)

    def get_state(self):
        n, d = self.num_envs, self.device
        s = torch.empty((4, n), dtype=torch.float64, device=d)
        st = torch.empty(n, dtype=torch.int32, device=d)
        nr = torch.empty(n, dtype=torch.uint8, device=d)
        _lib.check(self._c_get_state(self._h, _lib.ptr(s), _lib.ptr(st), _lib.ptr(nr)))
        return s, st, nr

    def set_state(self, state=None, steps=None, need_reset=None):
        s = None if state is None else self._dev(state, torch.float64)
        st = None if steps is None else self._dev(steps, torch.int32)
        nr = None if need_reset is None else self._dev(need_reset, torch.uint8)
        _lib.check(self._c_set_state(self._h, _lib.ptr(s), _lib.ptr(st), _lib.ptr(nr)))
        self.engine.sync()
        self.need_reset = False

    def close_extras(self, **kwargs):
        if self._h is not None:
            self._c_destroy(self._h)
            self._h = None
