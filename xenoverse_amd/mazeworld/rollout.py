"""Fused MazeWorld rollouts: T vector steps issued by one C call (xv_maze_rollout / xv_maze_rollout_agent,
csrc/maze_rollout.hip), every result a device tensor stacked over T.  MazeWorldVecEnv.rollout / rollout_teacher are
thin wrappers over the two functions here; `explore_draws_host` restates the exploration draws on the host."""
import ctypes as C
import math

import numpy as np
import torch

from .. import _lib
from ..engine import AUTORESET
from ..host_draws import env_draw_words, u53

DRAW_EXPLORE = 48      # XV_DRAW_EXPLORE (csrc/maze_common.h)

# name, dtype, trailing shape — in the member order of xv_maze_rollout_out (include/xeno.h)
RECORD = (("reward", torch.float32, ()), ("terminated", torch.uint8, ()), ("truncated", torch.uint8, ()),
          ("steps", torch.int32, ()), ("command", torch.float32, (3,)), ("pos", torch.float64, (2,)),
          ("ori", torch.float64, ()), ("grid", torch.int32, (2,)), ("cmd_idx", torch.int32, ()),
          ("cmd_age", torch.int32, ()), ("collision", torch.float64, ()), ("target", torch.int32, ()),
          ("episode", torch.int32, ()))
TEACHER = (("action", torch.int32, ()), ("action_label", torch.int32, ()), ("explored", torch.uint8, ()))
BOOLS = ("terminated", "truncated", "explored")


class _RolloutOut(C.Structure):   # xv_maze_rollout_out
    _fields_ = [(k, C.c_void_p) for k in [f[0] for f in RECORD] + ["final_pose", "frames", "final_frames"] +
                [f[0] for f in TEACHER]]


def explore_draws_host(seed, gid_base, tick, n_env, epsilon, n_actions):
    """The exploration draws of rollout_teacher for envs gid_base .. gid_base + n_env - 1 at `tick` (the tick of the behaviour
    agent's act; a scalar or one per env): w = xv_env_draw(seed, env id, tick, 48); -> (explored bool[n_env] = u53(w0, w1) <
    epsilon, random_action int32[n_env] = floor(u53(w2, w3) * n_actions))."""
    gid = np.uint64(int(gid_base)) + np.arange(int(n_env), dtype=np.uint64)
    w = env_draw_words(seed, gid, tick, DRAW_EXPLORE)
    explored = u53(w[:, 0], w[:, 1]) < float(epsilon)
    return explored, np.floor(u53(w[:, 2], w[:, 3]) * float(n_actions)).astype(np.int32)


def _frame_stride(frames):
    if frames is None:
        return 0
    if isinstance(frames, bool) or not isinstance(frames, (int, np.integer)) or int(frames) < 1:
        raise ValueError("frames must be None (no frame is painted) or an int >= 1 (every frames-th step is painted)")
    return int(frames)


def _outputs(env, T, stride, teacher, given):
    """the [T, N, ...] device tensors of one call: those of `given` (checked) where it has them, else fresh ones"""
    n, d = env.num_envs, env.device
    W, H = env.resolution
    spec = list(RECORD) + (list(TEACHER) if teacher else [])
    same = env.autoreset_mode == "same_step"
    if same:
        spec.append(("final_pose", torch.float64, (3,)))
    lead = {}
    if stride and T // stride > 0:
        spec.append(("frames", torch.uint8, (W, H, 3)))
        lead["frames"] = T // stride
        if same and env.with_final_obs:
            spec.append(("final_obs", torch.uint8, (W, H, 3)))
            lead["final_obs"] = T // stride
    given = {} if given is None else given
    if not isinstance(given, dict):
        raise ValueError("out must be a dict of tensors (as a former call returned it)")
    raw = {}
    for name, dt, tail in spec:
        shape = (lead.get(name, T), n) + tuple(tail)
        t = given.get(name)
        if t is None:
            # final_obs is written only where an episode ended
            raw[name] = (torch.zeros if name == "final_obs" else torch.empty)(shape, dtype=dt, device=d)
            continue
        if not torch.is_tensor(t) or t.device != d or tuple(t.shape) != shape or not t.is_contiguous() or \
                (t.dtype != dt and not (name in BOOLS and t.dtype == torch.bool)):
            raise ValueError("out[%r] must be a contiguous %s tensor of shape %s on %s" % (name, dt, shape, d))
        raw[name] = t.view(torch.uint8) if t.dtype == torch.bool else t
    return raw


def _struct(raw):
    return _RolloutOut(**{k: _lib.ptr(raw.get("final_obs" if k == "final_frames" else k)) for k, _ in _RolloutOut._fields_})


def _finish(env, raw):
    return {k: env._out(v.view(torch.bool) if k in BOOLS else v) for k, v in raw.items()}


def _require_ready(env):
    if env._h is None:
        raise Exception("Must call \"set_task\" before reset")
    if env.need_reset:
        raise Exception("Must \"reset\" before doing any actions")   # maze_env.py:51-52


def rollout(env, actions, frames=None, out=None):
    mode = env.ACTION_MODES[env.action_space_type]
    want, tail = (torch.float64, (2,)) if mode == 0 else (torch.int32, ())
    if not torch.is_tensor(actions):
        actions = torch.as_tensor(np.asarray(actions))
    if actions.dtype != want:
        raise ValueError("actions must be %s for a %s action space, not %s" % (want, env.action_space_type, actions.dtype))
    if actions.dim() != 2 + len(tail) or tuple(actions.shape[1:]) != (env.num_envs,) + tail:
        raise ValueError("actions must have shape (T, %d%s)" % (env.num_envs, ", 2" if tail else ""))
    T = int(actions.shape[0])
    if T < 1:
        raise ValueError("a rollout needs T >= 1 steps")
    stride = _frame_stride(frames)
    _require_ready(env)
    a = env._dev(actions, want)
    raw = _outputs(env, T, stride, False, out)
    _lib.check(env.lib.xv_maze_rollout(env._h, _lib.ptr(a), mode, T, stride, AUTORESET[env.autoreset_mode],
                                       C.byref(_struct(raw))))
    return _finish(env, raw)


def _agent_handle(env, agent, what):
    from .agents import AgentBase
    if not isinstance(agent, AgentBase) or agent.maze_env is not env:
        raise ValueError("%s must be an agent created with maze_env= this env" % what)
    if agent._h is None or env._h is None or agent._env_handle != env._h.value:
        raise ValueError("%s is closed (the env's task changed, or close() was called); create a new agent" % what)
    return agent._h


def rollout_teacher(env, agent, T, epsilon=0.0, label_agent=None, frames=None, out=None):
    if env.ACTION_MODES[env.action_space_type] == 0:
        raise ValueError("rollout_teacher needs a Discrete16 or Discrete32 action space (the agents choose from its table)")
    if env.autoreset_mode != "same_step":
        raise ValueError("rollout_teacher needs autoreset_mode=\"same_step\"")
    if isinstance(T, bool) or not isinstance(T, (int, np.integer)) or int(T) < 1:
        raise ValueError("a rollout needs T >= 1 steps")
    eps = float(epsilon)
    if math.isnan(eps) or eps < 0.0 or eps > 1.0:
        raise ValueError("epsilon must be within [0, 1]")
    stride = _frame_stride(frames)
    g = _agent_handle(env, agent, "agent")
    lab = None if label_agent is None else _agent_handle(env, label_agent, "label_agent")
    if label_agent is agent:
        raise ValueError("label_agent must be another agent than the behaviour agent (it would update its memory twice per step)")
    _require_ready(env)
    raw = _outputs(env, int(T), stride, True, out)
    _lib.check(env.lib.xv_maze_rollout_agent(g, lab, int(T), eps, stride, C.byref(_struct(raw))))
    return _finish(env, raw)
