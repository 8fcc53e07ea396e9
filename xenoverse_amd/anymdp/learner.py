"""What the AnyMDP learners (qlearner.py, mbrl.py) share: numpy's pairwise sum for the host restatements, and
`_DeviceLearner`, the scaffold of a learner on the device (csrc/anymdp_learner.h is its C++ counterpart)."""
import numpy as np


def pairwise_sum(x):
    """numpy's pairwise_sum of each row of x[..., n] (any n): a plain loop below 8 elements, eight partial sums up to 128,
    above that split at n / 2 rounded down to a multiple of 8"""
    n = x.shape[-1]
    if n < 8:
        res = np.zeros(x.shape[:-1])
        for i in range(n):
            res = res + x[..., i]
        return res
    if n <= 128:
        r = [x[..., j].copy() for j in range(8)]
        i = 8
        while i < n - (n % 8):
            for j in range(8):
                r[j] = r[j] + x[..., i + j]
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for k in range(i, n):
            res = res + x[..., k]
        return res
    n2 = n // 2
    n2 -= n2 % 8
    if 2 * n2 == n:      # two equal halves: one call over both
        h = pairwise_sum(x.reshape(x.shape[:-1] + (2, n2)))
        return h[..., 0] + h[..., 1]
    return pairwise_sum(x[..., :n2]) + pairwise_sum(x[..., n2:])


def np_rowsum(x):
    """numpy.sum(x, axis=-1) of a contiguous x: add.reduce of each row onto the identity 0"""
    return 0.0 + pairwise_sum(x)


class _DeviceLearner(object):
    """One agent per env of an AnyMDPVecEnv, on the device, driven by `env.rollout_learner(learner, T)`.  A subclass declares
    its C-ABI and its tables and writes __init__: `_check_env(env)`, its own argument checks, `_create(env, *arguments)`.
    Every table becomes a property that returns a device copy of it taken when read; `get_state` copies all of them and
    `set_state` writes any.  The learner lives as long as its env's tasks: `env.set_task` and `env.close` close it (any
    later use raises)."""
    _ABI = None          # "xv_anymdp_qlearn": the prefix of _create, _destroy, _reset, _get_state, _set_state
    _ROLLOUT = None      # the rollout entry point rollout_learner calls
    _TABLES = ()         # (name, torch dtype name, dims of "NSA") in the order of the C-ABI's get_state / set_state
    _U_POLICY = "TN"     # dims of draws["u_policy"]
    _NOT_MDP = (ValueError, "MDP tasks only")
    _h = None

    def __init_subclass__(cls, **kwargs):
        super().__init_subclass__(**kwargs)
        for j, (name, _, _) in enumerate(cls._TABLES):
            setattr(cls, name, property(lambda self, j=j: self._get((j,))[j]))

    def _check_env(self, env):
        env._require_task()
        if getattr(env, "_parent", None) is not None:
            raise ValueError("%s: a sub-batch made by split() cannot carry learners; "
                             "make them on the env it was split from" % type(self).__name__)
        if env.task_type != "MDP":
            raise self._NOT_MDP[0](self._NOT_MDP[1])

    def _create(self, env, *args):
        import ctypes as C

        from .. import _lib
        self.env, self.lib = env, env.lib
        self.num_envs, self.S, self.A = env.num_envs, env.S, env.A
        # the env's handle object itself: set_task makes a new one, and holding it keeps `is` from ever matching a recycled one
        self._env_h = env._h
        self._closed_why = "%s: closed" % type(self).__name__
        h = C.c_void_p()
        _lib.check(self._fn("create")(env._h, *args, C.byref(h)))
        self._h = h
        env._learners.add(self)      # released before the env's handle goes (set_task, close)
        env._learner_handles[h.value] = (self._fn("destroy"), h)

    def _fn(self, op):
        return getattr(self.lib, "%s_%s" % (self._ABI, op))

    def _shape(self, dims, T=None):
        sizes = dict(T=T, N=self.num_envs, S=self.S, A=self.A)
        return tuple(sizes[d] for d in dims)

    def _live(self):
        if self._h is None:
            raise ValueError(self._closed_why)
        if self.env._h is not self._env_h:
            raise ValueError("%s: its env was closed or given new tasks; make a new learner" % type(self).__name__)

    def reset(self, mask=None):
        """__init__'s state for the agents where mask (bool[N]) is set (None: all)"""
        import torch

        from .. import _lib
        self._live()
        m = None if mask is None else self.env._dev(mask, torch.uint8)
        if m is not None and tuple(m.shape) != (self.num_envs,):
            raise ValueError("reset mask must have shape (num_envs,)")
        _lib.check(self._fn("reset")(self._h, _lib.ptr(m)))
        self.env.engine.sync()

    def _get(self, which):
        import torch

        from .. import _lib
        self._live()
        out = [torch.empty(self._shape(dims), dtype=getattr(torch, dt), device=self.env.device) if j in which else None
               for j, (_, dt, dims) in enumerate(self._TABLES)]
        _lib.check(self._fn("get_state")(self._h, *(_lib.ptr(t) for t in out)))
        self.env.engine.sync()
        return out

    def get_state(self):
        """-> device tensors (copies) of every table, in the order of _TABLES"""
        return tuple(self._get(range(len(self._TABLES))))

    def set_state(self, *tables, **named):
        """writes the tables given, by position in the order of _TABLES or by name; None or absent: left as it is"""
        import torch

        from .. import _lib
        self._live()
        names = [t[0] for t in self._TABLES]
        if len(tables) > len(names) or set(named) - set(names[len(tables):]):
            raise TypeError("set_state takes %s" % ", ".join(names))
        named.update(zip(names, tables))
        args = []
        for name, dt, dims in self._TABLES:
            t = named.get(name)
            if t is not None:
                t = self.env._dev(t, getattr(torch, dt))
                if tuple(t.shape) != self._shape(dims):
                    raise ValueError("set_state: expected shape %s, got %s" % (self._shape(dims), tuple(t.shape)))
            args.append(t)
        _lib.check(self._fn("set_state")(self._h, *(_lib.ptr(t) for t in args)))
        self.env.engine.sync()      # the temporaries above must outlive the copies

    def close(self, why=None):
        if self._h is not None:
            # the C learner borrows the env's handle and, through it, the engine: destroying it reads both.  When the env's
            # handle went first (only a learner collected together with its env sees that: vec_env.py, _release_learners)
            # the env has destroyed the C learner already
            env = self.env
            if env._h is self._env_h and env.engine.handle is not None:
                self._fn("destroy")(self._h)
                env._learner_handles.pop(self._h.value, None)
            self._h = None
            self._closed_why = why or self._closed_why

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
