"""VectorEnv base: the gymnasium >= 1.0 `VectorEnv` surface over a device
engine.  gymnasium's class is generic over the array type; these envs return torch tensors that live on
the GPU (`to_numpy=True` converts for NumPy consumers)."""
import math

import torch

from . import _lib
from .engine import AUTORESET, Engine
from .spaces import batch_space


try:      # gymnasium >= 1.0 present: be a gymnasium.vector.VectorEnv (isinstance checks of wrappers / trainers hold)
    from gymnasium.vector import VectorEnv as _GymVectorEnv
except Exception:      # not installed: the same surface on a plain class
    _GymVectorEnv = object


class OutputSet(object):
    """What one step writes: `t` name -> tensor (bool views and derived views included), the device pointers in the order the
    C call takes them as ctypes objects (`args`) and as ints (`ints`, for _xvfast.icall), and `ptr` name -> int."""
    __slots__ = ("t", "args", "ints", "ptr", "after")

    def __init__(self, t, ptr, order):
        self.t, self.ptr = t, {k: p.value for k, p in ptr.items()}
        self.args = tuple(ptr[k] for k in order)
        self.ints = tuple(self.ptr[k] for k in order)


class OutputSlabs(object):
    """Fresh output tensors for every step() at the cost of none: the outputs of K consecutive steps are carved out of ONE
    allocation per dtype (K x fields x N), the per-step tensors and their device pointers are made when the slab is, and a
    step takes the next precomputed set.  What a step hands out is never written again WHILE ANYBODY CAN SEE IT — copy=True
    semantics, as gymnasium's SyncVectorEnv(copy=True) — and a tensor the caller keeps keeps its slab alive (torch counts
    references on the storage).  (One torch.empty_like per output per step cost ~10 us of the 22-us eager step of 65,536
    envs.)

    Round 6: slabs are RECYCLED, with their tensor objects.  Up to `keep` slabs stay cached; when a slab is used up, the oldest
    cached one that nobody outside this object can reach any more is handed out again — the very same Python tensor objects,
    so a step creates and destroys no object at all (14.2 -> ~10 us per eager copy=True step of 65,536 AnyMDP envs).  "Nobody
    can reach it" is checked, not assumed, once per slab (K steps):
      * every cached tensor object has exactly the Python references this cache holds (sys.getrefcount): no caller variable,
        list or dict holds one of them;
      * every cached tensor's TensorImpl has one owner (Tensor._use_count() == 1): no C++ holder such as a DLPack capsule;
      * every slab storage is shared by exactly the tensors made here (torch._C._storage_Use_Count): no view, .detach(),
        .numpy() or reshaped alias of a handed-out tensor is alive.
    A slab that fails any of the three is left alone (and dropped from the cache when `keep` newer ones exist: it lives on
    for as long as its holders do).

    fields: [(name, torch dtype, trailing shape)], uint8 fields named in `as_bool` are handed out as bool views."""

    def __init__(self, fields, n, device, K=64, as_bool=(), order=None, keep=3, derived=None, zero_on_refill=()):
        """order: field names in the order the C call takes its pointers — next() then returns them as a ready tuple
        derived: {name: (field, fn)} — further views made once per slab, e.g. the user's columns of a padded observation;
        zero_on_refill: fields whose whole [K, ...] block is zeroed when a slab is (re)issued — for outputs a step writes only
        in part (LinDS final_obs: rows of finished envs), ONE fill per K steps instead of one per step"""
        self.fields, self.n, self.device, self.K = list(fields), int(n), device, int(K)
        self.derived = dict(derived or {})
        self.zero_on_refill = tuple(zero_on_refill)
        self.as_bool = set(as_bool)
        self.order = list(order) if order is not None else [f[0] for f in self.fields]
        self.keep = max(1, int(keep))
        self._sets, self._pos = [], 0
        self.last = None         # the set handed out last (it counts as a holder of its slab)
        self._cached = []          # cached slabs, oldest first; the last one is the slab in use
        self.made = 0            # slabs allocated so far (tests, diagnostics)
        self.recycled = 0        # slabs handed out again

    def _make(self, alloc=torch.empty):
        import ctypes as C
        by = {}
        for name, dt, tail in self.fields:
            by.setdefault(dt, []).append((name, tuple(tail)))
        per_step = [dict() for _ in range(self.K)]
        ptrs = [dict() for _ in range(self.K)]
        storages, zero_blocks = [], []
        for dt, fl in by.items():
            # [field][step][n * tail]: two unbind() calls hand out every per-step tensor (slicing K x fields views one by one
            # in Python cost more than the allocations it was meant to save)
            width = max(self.n * math.prod(t) for _, t in fl)
            slab = alloc((len(fl), self.K, width), dtype=dt, device=self.device)
            storages.append(slab.untyped_storage())
            base, esz = slab.data_ptr(), slab.element_size()
            fields = (slab.view(torch.bool) if dt == torch.uint8 else slab).unbind(0)
            plain = slab.unbind(0)
            for f, (name, tail) in enumerate(fl):
                src = fields[f] if name in self.as_bool else plain[f]
                sz = self.n * math.prod(tail)
                if sz != width:
                    src = src[:, :sz]
                if name in self.zero_on_refill:
                    zero_blocks.append(src)
                if tail:
                    src = src.view((self.K, self.n) + tail)
                rows = src.unbind(0)
                for k in range(self.K):
                    per_step[k][name] = rows[k]
                    ptrs[k][name] = C.c_void_p(base + ((f * self.K + k) * width) * esz)
        for name, (field, fn) in self.derived.items():
            for k in range(self.K):
                per_step[k][name] = fn(per_step[k][field])
        sets = [OutputSet(per_step[k], ptrs[k], self.order) for k in range(self.K)]
        rec = {"zero": zero_blocks, "sets": sets,
               "flat": [t for d in per_step for t in d.values()] + per_step + sets, "tensors": [t for d in per_step for t in d.values()],
               "storages": storages}      # (`flat` counts the per-step dicts and sets too: next() / next_set() hand them out)
        self.made += 1
        return rec

    @staticmethod
    def _counts(rec):
        import sys
        return (sum(map(sys.getrefcount, rec["flat"])), sum(map(torch.Tensor._use_count, rec["tensors"])),
                tuple(torch._C._storage_Use_Count(st._cdata) for st in rec["storages"]))

    def _refill(self):
        # the oldest cached slab nobody outside can reach, else a new one.  (The slab just used up is the newest: the
        # caller usually still holds its last outputs, so it is looked at last.)
        pick = None
        for i, rec in enumerate(self._cached):
            if self._counts(rec) == rec["idle"]:
                pick = self._cached.pop(i)
                self.recycled += 1
                break
        if pick is None:
            pick = self._make()
            pick["idle"] = None
        self._cached.append(pick)
        for blk in pick["zero"]:
            blk.zero_()
        if pick["idle"] is None:      # (taken with every temporary of _make gone: the slab is referenced exactly as when it idles)
            pick["idle"] = self._counts(pick)
        while len(self._cached) > self.keep:
            self._cached.pop(0)
        self._sets = pick["sets"]
        self._pos = 0

    def next(self):
        """-> (dict name -> tensor, tuple of ctypes pointers in `order`) of a set no earlier step has written — or one whose
        earlier contents nobody can reach any more"""
        s = self.next_set()
        return s.t, s.args

    def next_set(self):
        """the same set as an OutputSet (pointers also as ints and by name)"""
        if self._pos >= len(self._sets):
            self._refill()
        s = self.last = self._sets[self._pos]
        self._pos += 1
        return s


class StepOutputs(object):
    """Where a family's step() writes, and who owns that memory afterwards — decided here and nowhere else.  An env builds one
    per set_task from its field list and takes `next()` before every step launch: an OutputSet.

      copy=True                 sets of recycled 64-step slabs (OutputSlabs): nothing handed out is ever written again while
                                anybody can see it;
      copy=False                `n_sets` persistent sets used round robin — what a step returned is valid until the step
                                `n_sets` calls later; `hold(True)` pins the current set (captured loops: the policy reads the
                                observation where the step writes it), `hold(False)` resumes; `zero_on_refill` fields are
                                NOT zeroed again (rows a step leaves alone keep what an earlier step wrote);
      to_numpy=True             one persistent set, `zero_on_refill` fields zeroed before every step; the env converts on the
                                way out.

    fields: [(name, torch dtype, trailing shape[, fill])] — `fill` is what a persistent set holds before its first step
    (default 0); order / as_bool / derived / zero_on_refill: as OutputSlabs."""

    def __init__(self, fields, n, device, order, copy=True, to_numpy=False, n_sets=1, as_bool=(), derived=None,
                 zero_on_refill=(), K=64):
        self.persistent = bool(to_numpy) or not copy
        plain = [f[:3] for f in fields]
        if not self.persistent:
            self._slabs = OutputSlabs(plain, n, device, K=K, as_bool=as_bool, order=order, derived=derived,
                                      zero_on_refill=zero_on_refill)
            self.next = self._slabs.next_set      # (slabs are made at the first step: 64 steps of outputs are not small)
            return
        rec = OutputSlabs(plain, n, device, K=1 if to_numpy else n_sets, as_bool=as_bool, order=order, derived=derived,
                          zero_on_refill=zero_on_refill)._make(alloc=torch.zeros)      # never refilled, never checked for holders
        sets = rec["sets"]
        for s, after in zip(sets, sets[1:] + sets[:1]):      # a ring: `after` is the set of the following step
            s.after = after
            for f in fields:
                if len(f) > 3 and f[3]:
                    s.t[f[0]].fill_(f[3])
        self._cur, self.last, self._held = sets[0], None, False
        if to_numpy:
            self._zero, self.next = rec["zero"], self._next_zeroed

    def hold(self, on):
        """True: next() keeps returning the set it would return now; False: sets alternate again"""
        self._held = bool(on)

    def next(self):
        s = self.last = self._cur
        if not self._held:
            self._cur = s.after
        return s

    def _next_zeroed(self):
        for blk in self._zero:
            blk.zero_()
        self.last = self._cur
        return self._cur

    def take_last(self):
        """the set next() returned last — the latest outputs — once: None when nothing was stepped since the last call"""
        own = self if self.persistent else self._slabs
        s, own.last = own.last, None
        return s


def env_task_map(num_envs, n_task, index=None, device="cpu"):
    """The task of every env as a contiguous int32[num_envs] tensor on `device`.  index None: the envs split evenly and
    contiguously over the tasks (num_envs must be a multiple of n_task); else `index` (tensor / ndarray / list), checked:
    the kernels read their task's tables by it."""
    if index is None:
        if num_envs % n_task != 0:
            raise ValueError("num_envs is not a multiple of the task count; pass env_task_index")
        return torch.arange(num_envs, device=device, dtype=torch.int32) // (num_envs // n_task)
    t = torch.as_tensor(index).to(device=device, dtype=torch.int32).contiguous()
    if t.shape != (num_envs,) or int(t.min()) < 0 or int(t.max()) >= n_task:
        raise ValueError("env_task_index must be (num_envs,) with entries in [0, n_task)")
    return t


class VectorEnv(_GymVectorEnv):
    metadata = {"autoreset_mode": "same_step"}
    render_mode = None
    spec = None

    def __init__(self, num_envs, device="cuda:0", seed=0, env_id_base=0, autoreset_mode="same_step",
                 to_numpy=False, engine=None, copy=True):
        if autoreset_mode not in AUTORESET:
            raise ValueError("autoreset_mode must be one of %s" % sorted(AUTORESET))
        self.num_envs = int(num_envs)
        self.engine = engine if engine is not None else Engine(device, seed=seed, env_id_base=env_id_base)
        self._own_engine = engine is None
        self.device = self.engine.device
        self.lib = self.engine.lib
        self.autoreset_mode = autoreset_mode
        self._auto = AUTORESET[autoreset_mode]      # as the C-ABI takes it (XV_AUTORESET_*)
        self.metadata = dict(type(self).metadata, autoreset_mode=autoreset_mode)
        self.to_numpy = bool(to_numpy)
        # copy (as gymnasium's SyncVectorEnv(copy=...)): True returns fresh tensors from every call; False returns
        # views of engine-owned output buffers, valid until the next step()/reset() (no per-step device copies)
        self.copy = bool(copy)
        # lean_infos: step() returns only the infos that cost no extra launch (captured loops: xenoverse_amd/capture.py)
        self.lean_infos = False
        self._outputs = None      # StepOutputs of the families that step through output sets (_make_step_outputs)
        self._holding = False
        self.closed = False
        self.task_set = False
        self.single_observation_space = None
        self.single_action_space = None
        self.observation_space = None
        self.action_space = None

    # -- helpers ------------------------------------------------------------------------------------
    def _set_spaces(self, single_obs, single_act):
        self.single_observation_space = single_obs
        self.single_action_space = single_act
        self.observation_space = batch_space(single_obs, self.num_envs)
        self.action_space = batch_space(single_act, self.num_envs)

    def _dev(self, x, dtype):
        """Bring `x` (tensor / ndarray / list) to a contiguous device tensor of `dtype` without copying
        when it already is one."""
        if torch.is_tensor(x):
            if x.device != self.device or x.dtype != dtype:
                x = x.to(device=self.device, dtype=dtype)
            return x.contiguous()
        return torch.as_tensor(x).to(device=self.device, dtype=dtype).contiguous()

    def _out(self, t):
        return t.cpu().numpy() if self.to_numpy else t

    def _o(self, t):
        """an output buffer -> what the caller receives (a copy unless copy=False)"""
        return self._out(t.clone() if (self.copy and not self.to_numpy) else t)

    def _renew(self, *names):
        """copy=True without copies: before a launch that fully overwrites these output buffers, swap in fresh
        ones — the tensors handed out by the previous call are then never written again (use with _of / _obf)"""
        if self.copy and not self.to_numpy:
            for name in names:
                t = getattr(self, name)
                if t is not None:
                    setattr(self, name, torch.empty_like(t))

    def _detach(self, *names):
        """copy=True before a launch that overwrites output buffers only in part (masked reset, render of the
        current state): the launch writes into private clones, so tensors handed out earlier keep their values
        and the entries the launch does not touch keep theirs"""
        if self.copy and not self.to_numpy:
            for name in names:
                t = getattr(self, name, None)
                if t is not None:
                    setattr(self, name, t.clone())

    def _plain_buffers(self, fields):
        """one engine-owned buffer per field as `self._<name>`: what reset() writes (_adopt_latest rebinds those to the latest
        step's outputs), and fixed memory for callers that time bare kernels (scripts/bench_families.py)"""
        for f in fields:
            setattr(self, "_" + f[0], torch.full((self.num_envs,) + tuple(f[2]), f[3] if len(f) > 3 else 0, dtype=f[1],
                                                 device=self.device))

    def _adopt_latest(self, **names):
        """before reset() writes its buffers: when steps were made since the last reset, `self.<attr>` becomes field `name` of
        the latest step's output set — a masked reset then keeps the other envs' last observation"""
        s = self._outputs.take_last() if self._outputs is not None else None
        if s is not None:
            for attr, name in names.items():
                setattr(self, attr, s.t[name])

    def _make_step_outputs(self, fields, order, **kw):
        """-> this env's StepOutputs for `fields` (set_task, or the first step after it)"""
        self._outputs = StepOutputs(fields, self.num_envs, self.device, order, copy=self.copy, to_numpy=self.to_numpy, **kw)
        self._outputs.hold(self._holding)
        return self._outputs

    def _numpy(self, obs, reward, term, trunc, infos):
        """to_numpy: what a step hands out is converted here, on the way out"""
        return (self._out(obs), self._out(reward), self._out(term), self._out(trunc), {k: self._out(v) for k, v in infos.items()})

    def _of(self, t):
        """an output buffer that was renewed before the launch (or copy=False): handed out as it is"""
        return self._out(t)

    def _obf(self, t):
        return self._out(t.bool() if self.to_numpy else t.view(torch.bool))

    def _require_task(self):
        if not self.task_set:
            # reference: raise Exception("Must call \"set_task\" first") (anymdp_env.py:83, linds_env.py:110)
            raise Exception("Must call \"set_task\" first")

    def _require_reset(self):
        if (not self.task_set) or self.need_reset:
            # reference message (anymdp_env.py:93-94, linds_env.py:134-135)
            raise Exception("Must \"set_task\" and \"reset\" before doing any actions")

    def _env_task(self, n_task, env_task_index):
        """set_task's env -> task mapping on this env's device (env_task_map above)"""
        return env_task_map(self.num_envs, n_task, env_task_index, self.device)

    def _reset_mask(self, options):
        """reset(options={"reset_mask": ...}) -> uint8[N] device tensor, or None: every env"""
        if options is not None and options.get("reset_mask") is not None:
            return self._dev(options["reset_mask"], torch.uint8)
        return None

    def _reset_prelude(self, seed, options):
        """the head of reset(): a task must be set; `seed` (int) re-keys the engine's Philox stream position; -> the mask"""
        self._require_task()
        if seed is not None:
            self.engine.tick = (int(seed) & 0xFFFFFFFF) << 24
        return self._reset_mask(options)

    def _alloc(self, spec, lead=()):
        """spec: [(name, torch dtype, trailing shape[, fill])] -> {name: tensor[lead..., N, trailing...]} on the device, in
        spec order.  Without `fill` the tensor is uninitialised (the launch writes every entry); with it, filled (outputs a
        launch writes only in part)."""
        shape, out = tuple(lead) + (self.num_envs,), {}
        for f in spec:
            size = shape + tuple(f[2])
            if len(f) < 4:
                out[f[0]] = torch.empty(size, dtype=f[1], device=self.device)
            elif f[3] == 0:
                out[f[0]] = torch.zeros(size, dtype=f[1], device=self.device)
            else:
                out[f[0]] = torch.full(size, f[3], dtype=f[1], device=self.device)
        return out

    def _capture_hold(self, on):
        """while a captured loop exists: pins whatever the family alternates between step() calls (output sets) and,
        when asked, leaves out the infos that need a launch of their own"""
        self._holding = bool(on)
        if self._outputs is not None:
            self._outputs.hold(on)
        self.lean_infos = self._lean_wanted if on else self._lean_saved

    AUTO_UNROLL = 8      # one hipGraphLaunch costs the host about what it replaces; 8 iterations per launch: 15 -> 7.3 us per step

    def capture(self, policy_fn, obs, unroll=1, warmup=1, lean=True):
        """[policy_fn(obs) -> actions; step(actions)] captured in a torch.cuda.graph -> CapturedLoop (capture.py): one
        graph launch per `unroll` vector steps, same trajectory as the eager calls.  Needs copy=False, to_numpy=False.
        unroll="auto": AUTO_UNROLL iterations per graph launch (`loop.unroll` says how many steps one replay() makes).
        `warmup` eager iterations run first and are real steps.  lean: step() skips the infos that need a launch of
        their own (AnyMDP / LinDS `steps`, the `_final_obs` mask) while the loop exists."""
        from .capture import CapturedLoop
        if self.copy or self.to_numpy:
            raise ValueError("capture() needs an env built with copy=False and to_numpy=False (fixed output buffers)")
        self._lean_saved, self._lean_wanted = self.lean_infos, bool(lean) or self.lean_infos
        if unroll == "auto":
            unroll = self.AUTO_UNROLL
        return CapturedLoop(self.step, [self.engine], policy_fn, obs, unroll=unroll, warmup=warmup, device=self.device,
                            hold=self._capture_hold)

    def check_errors(self, clear=True):
        """Device-side range errors are sticky bits, read on demand (one stream sync)."""
        return self.engine.error_flags(clear)

    def close(self, **kwargs):
        if self.closed:
            return
        self.close_extras(**kwargs)
        if self._own_engine:
            self.engine.close()
        self.closed = True

    def close_extras(self, **kwargs):
        pass

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


XenoError = _lib.XenoError
