"""MixedBatch — several environment families stepped concurrently on one GPU (BASELINE.json config 5: anymdp +
linds + metacontrol, 262,144 envs sharded over 8 GPUs = per GPU 16,384 anymdp + 8,192 linds + 8,192 cartpole).

Each family keeps its own engine.  `streams="shared"` (default) launches all families on the caller's stream;
`streams="separate"` gives every family a private HIP stream so that their step kernels can overlap, with
`sync()` making the caller's stream wait for all of them.  Measured on one MI355X at the config-5 share
(`scripts/bench_families.py --families mixed`): the three step kernels take 16.4 us back to back on one stream and
47.6 us on three streams — they are 4-8 us each, so the cross-stream event waits a dependent step loop needs
(actions in, observations out) cost more than the overlap saves; separate streams pay off only when a family's
step is long (MazeWorld frames) or the consumer does not need all families at every step.  A family's trajectory
is identical either way and identical to what it would be stepped alone: engines share nothing (no global RNG).
Across GPUs each rank owns a contiguous slice of every family (`distributed.shard_range`).

Round 3: `step_fused` advances one AnyMDP, one LinDS and one CartPole family with ONE kernel launch (`xv_mixed_step`:
the families' own step bodies share a grid) — same results as `step`, one launch latency instead of three.
"""
import ctypes as C

import torch

from . import _lib
from .engine import AUTORESET, Engine


class _MixedIO(C.Structure):   # xv_mixed_io (include/xeno.h)
    _fields_ = [(k, C.c_void_p) for k in (
        "a_action", "a_obs", "a_reward", "a_reward_gt", "a_terminated", "a_truncated", "a_final_obs",
        "l_action", "l_obs", "l_reward", "l_terminated", "l_truncated", "l_cmd", "l_error", "l_final_obs",
        "c_action", "c_obs", "c_reward", "c_terminated", "c_truncated", "c_final_obs",
        "a_steps", "a_done", "l_steps", "l_done", "c_done")]      # ABI 12: steps / done masks from the fused launch (nullable)


def _io_outputs(prefix, **fields):
    return tuple((prefix + k, v) for k, v in fields.items())


# xv_mixed_io field -> the field of the family's output set (AnyMDPVecEnv, LinDSVecEnv, ControlVecEnv: set_task) it points at
_IO_OUTPUTS = (
    _io_outputs("a_", obs="obs", reward="reward", reward_gt="reward_gt", terminated="term", truncated="trunc",
                final_obs="final_obs", steps="steps", done="done"),
    _io_outputs("l_", obs="obs", reward="reward", terminated="term", truncated="trunc", cmd="cmd", error="error",
                final_obs="fobs", steps="steps", done="done"),
    _io_outputs("c_", obs="obs", reward="reward", terminated="term", truncated="trunc", final_obs="fobs", done="done"))


class MixedBatch(object):
    def __init__(self, device="cuda:0", seed=0, streams="shared"):
        assert streams in ("shared", "separate")
        self.device = torch.device(device)
        self.seed = int(seed)
        self.separate = streams == "separate"
        self.envs = {}
        self.streams = {}
        self._trio = None          # (_fused_trio result, cached until add())
        self._fast = {}            # step_fused: three persistent output sets -> [xv_mixed_io filled for them, its byref, the sets, the return value]

    def add(self, name, env_cls, num_envs, env_id_base=0, **kwargs):
        """Create `env_cls(num_envs, engine=<engine on a private stream>, **kwargs)` under `name`."""
        st = torch.cuda.Stream(device=self.device) if self.separate else torch.cuda.current_stream(self.device)
        eng = Engine(self.device, seed=self.seed, env_id_base=env_id_base, stream=st)
        env = env_cls(num_envs, engine=eng, **kwargs)
        env._own_engine = True   # closed with the env
        self.envs[name] = env
        self.streams[name] = st
        self._trio, self._fast = None, {}
        return env

    def _on(self, name):
        st = self.streams[name]
        if self.separate:
            st.wait_stream(torch.cuda.current_stream(self.device))   # inputs produced on the caller's stream
        return torch.cuda.stream(st)

    def set_task(self, tasks):
        for name, t in tasks.items():
            with self._on(name):
                if isinstance(t, tuple):
                    self.envs[name].set_task(t[0], env_task_index=t[1])
                else:
                    self.envs[name].set_task(t)

    def reset(self):
        out = {}
        for name, env in self.envs.items():
            with self._on(name):
                out[name] = env.reset()
        self.sync()
        return out

    def step(self, actions):
        """actions: dict name -> batched action.  Launches every family's step on its own stream, then makes the
        caller's stream wait for all of them.  -> dict name -> (obs, reward, terminated, truncated, infos)"""
        out = {}
        for name, env in self.envs.items():
            with self._on(name):
                out[name] = env.step(actions[name])
        self.sync()
        return out

    def _fused_trio(self):
        if self._trio is not None:
            return self._trio
        self._trio = self._fused_trio_uncached()
        return self._trio

    def _fused_trio_uncached(self):
        from .anymdp import AnyMDPVecEnv
        from .linds import LinDSVecEnv
        from .metacontrol import CartPoleVecEnv
        pick = {}
        for name, env in self.envs.items():
            for key, cls in (("a", AnyMDPVecEnv), ("l", LinDSVecEnv), ("c", CartPoleVecEnv)):
                if isinstance(env, cls):
                    if key in pick:
                        raise ValueError("step_fused takes one env of each family (anymdp, linds, cartpole)")
                    pick[key] = (name, env)
        if len(pick) != 3 or len(self.envs) != 3:
            raise ValueError("step_fused needs exactly one AnyMDPVecEnv, one LinDSVecEnv and one CartPoleVecEnv")
        if self.separate:
            raise ValueError("step_fused launches one kernel: build the batch with streams='shared'")
        modes = {e.autoreset_mode for _, e in pick.values()}
        if len(modes) != 1:
            raise ValueError("the three families must use one autoreset_mode")
        return pick, modes.pop()

    def step_fused(self, actions):
        """One launch for the whole mixed batch (xv_mixed_step).  actions: dict name -> batched action, as for step().
        -> dict name -> (obs, reward, terminated, truncated, infos), bit for bit what step() returns.  Handles without a
        fused instantiation (AnyMDP on the per-lane search or S > 112, LinDS on the scalar path or other pads) are stepped
        by step() — three launches, same results.

        Each env hands out its next output set, the fused kernel writes all three (info["steps"] and the done masks included,
        ABI 12), and each env turns its set into what its own step() returns."""
        pick, mode = self._fused_trio()
        (na, ea), (nl, el), (nc, ec) = pick["a"], pick["l"], pick["c"]
        if ea._tok is not None:
            raise ValueError("step_fused serves MDP tasks")
        ea._check_step(); el._check_step(); ec._require_reset()
        if not ea.lib.xv_mixed_supported(ea._h, el._h, ec._h):      # asked BEFORE any output set is taken
            return self.step(actions)
        aa = ea._dev(actions[na], torch.int32)
        al = el._action(actions[nl])
        ac = ec._dev(actions[nc], torch.int32)
        if aa.shape != (ea.num_envs,) or ac.shape != (ec.num_envs,):
            raise AssertionError("action batch shapes do not match the env counts")
        oa, ol, oc = ea._outputs or ea._make_outputs(), el._outputs, ec._outputs
        sets = (oa.next(), ol.next(), oc.next())
        # persistent sets (copy=False, to_numpy): the struct filled for a combination of sets is kept with them — and so is what
        # the envs return for it, where that is the same objects every time (no conversion, no launch of its own)
        key = None
        if oa.persistent and ol.persistent and oc.persistent:
            key = (id(sets[0]), id(sets[1]), id(sets[2]), ea.lean_infos, el.lean_infos, ec.lean_infos)
        hit = self._fast.get(key)
        if hit is None:
            io = _MixedIO()
            for s, names in zip(sets, _IO_OUTPUTS):
                for field, name in names:
                    setattr(io, field, s.ptr[name])
            hit = [io, C.byref(io), sets, None]
            if key is not None:
                if len(self._fast) >= 8:      # (sets of tasks long replaced: an env makes new ones at every set_task)
                    self._fast.clear()
                self._fast[key] = hit
        io, ref, _, out = hit
        io.a_action, io.l_action, io.c_action = aa.data_ptr(), al.data_ptr(), ac.data_ptr()
        _lib.check(ea.lib.xv_mixed_step(ea._h, el._h, ec._h, ref, AUTORESET[mode]))
        if out is None:
            out = {na: ea._finish(sets[0], aa), nl: el._finish(sets[1]), nc: ec._finish(sets[2])}
            if key is not None and not (ea.to_numpy or el.to_numpy or ec.to_numpy or ea.with_transition_gt):
                hit[3] = out
        return out

    def capture(self, policy_fn, obs, unroll=1, warmup=1, lean=True):
        """[policy_fn(obs dict) -> actions dict; step_fused(actions)] captured in a torch.cuda.graph (capture.py):
        one graph launch per `unroll` vector steps of the whole mixed batch.  obs: dict name -> the observation the family
        returned last.  The envs must be built with copy=False."""
        from .capture import CapturedLoop
        pick, _ = self._fused_trio()
        envs = [e for _, e in pick.values()]
        if any(e.copy or e.to_numpy for e in envs):
            raise ValueError("capture() needs the three envs built with copy=False and to_numpy=False")
        for e in envs:
            e._lean_saved, e._lean_wanted = e.lean_infos, bool(lean) or e.lean_infos

        def hold(on):
            for e in envs:
                e._capture_hold(on)

        def step(actions):
            out = self.step_fused(actions)
            return ({k: v[0] for k, v in out.items()}, out)

        return CapturedLoop(step, [e.engine for e in envs], policy_fn, obs, unroll=unroll, warmup=warmup, device=self.device,
                            hold=hold)

    def sync(self):
        if not self.separate:
            return
        cur = torch.cuda.current_stream(self.device)
        for st in self.streams.values():
            cur.wait_stream(st)

    @property
    def num_envs(self):
        return sum(e.num_envs for e in self.envs.values())

    def close(self):
        for env in self.envs.values():
            env.close()
