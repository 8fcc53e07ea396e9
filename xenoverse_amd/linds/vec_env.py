"""LinDSVecEnv — N randomised LTI control environments stepped per kernel launch on one MI355X.

Mirrors the reference's per-env interface (xenoverse/linds/linds_env.py: LinearDSEnv.__init__ :16-38,
set_task :40-65, reset :108-131, step :133-169, get_future_inner_cmds :171-183, state :185-187) behind the
gymnasium VectorEnv surface.  Same task dicts, same info keys (`steps`, `command`,
`command_type` on reset, `error`), same exception messages for misuse.
"""
import ctypes as C

import numpy as np
import torch

from .. import _lib
from ..engine import AUTORESET
from ..spaces import Box
from ..vector import VectorEnv
from .tables import _Tables, build_tables, pad_tables

_F32 = ("phiT", "gamT", "cT", "xt", "y0", "valid", "cmd0", "four_coef", "scal", "init")
_F64 = ("four_omega", "four_period")


class _MPCTables(C.Structure):   # xv_linds_mpc_tables (include/xeno.h)
    _fields_ = [("n_pad", C.c_int), ("n_in", C.c_int), ("NOc", C.c_int)] + \
        [(k, C.c_void_p) for k in ("mfrag", "gfrag", "g0", "rho", "mnorm", "nu")] + \
        [(k, C.c_float) for k in ("sigma", "alpha", "eps_abs", "eps_rel")]


class LinDSVecEnv(VectorEnv):
    def __init__(self, num_envs, dt=0.1, max_steps=1000, pad_observation_dim=16, pad_command_dim=16,
                 pad_action_dim=8, device="cuda:0", seed=0, env_id_base=0, autoreset_mode="same_step",
                 to_numpy=False, engine=None, copy=True):
        super().__init__(num_envs, device=device, seed=seed, env_id_base=env_id_base,
                         autoreset_mode=autoreset_mode, to_numpy=to_numpy, engine=engine, copy=copy)
        self.dt = dt
        self.max_steps = max_steps
        self.pad_observation_dim = pad_observation_dim
        self.pad_command_dim = pad_command_dim
        self.pad_action_dim = pad_action_dim
        self._set_spaces(Box(-np.inf, np.inf, shape=(pad_observation_dim,), dtype=np.float32),
                         Box(-1, 1, shape=(pad_action_dim,), dtype=np.float32))
        self._h = None

    def set_task(self, tasks, env_task_index=None):
        """tasks: one reference task dict, a list of them, or prebuilt tables (linds.tables.build_tables)."""
        self._drop_mpc()
        if isinstance(tasks, dict) and "phiT" in tasks:
            tab = tasks
            self._mpc_src = None if any(torch.is_tensor(tab[k]) for k in ("phiT", "gamT", "cT", "xt", "y0", "valid", "scal")) \
                else tab
        else:
            self._mpc_src = [tasks] if isinstance(tasks, dict) else list(tasks)
            tab = build_tables(tasks, dt=self.dt, pad_observation_dim=self.pad_observation_dim,
                               pad_action_dim=self.pad_action_dim, pad_command_dim=self.pad_command_dim)
        self.user_dims = (int(tab["NA"]), int(tab["NO"]))
        tab = pad_tables(tab)
        dev = {k: self._dev(tab[k], torch.float32) for k in _F32}
        dev.update((k, self._dev(tab[k], torch.float64)) for k in _F64)
        dev["ints"] = self._dev(tab["ints"], torch.int32)
        n_task = int(dev["phiT"].shape[0])
        dev["env_task"] = self._env_task(n_task, env_task_index)
        self.NS, self.NA, self.NO, self.NI = int(tab["NS"]), int(tab["NA"]), int(tab["NO"]), int(tab["NI"])
        if self._h is not None:
            self.lib.xv_linds_destroy(self._h)
            self._h = None
        ct = _Tables(*[_lib.ptr(dev[k]) for k, _ in _Tables._fields_])
        h = C.c_void_p()
        _lib.check(self.lib.xv_linds_create(self.engine.handle, self.num_envs, n_task, self.NS, self.NA, self.NO,
                                            self.NI, C.byref(ct), _lib.ptr(dev["env_task"]), C.byref(h)))
        self._h = h
        self._tab = dev
        self.n_task = n_task
        f32, u8, i32, NO, uo = torch.float32, torch.uint8, torch.int32, self.NO, self.user_dims[1]
        cut = (lambda t: t[:, :uo]) if uo != NO else (lambda t: t)      # the user's columns of a padded row
        fields = [("obs", f32, (NO,)), ("cmd", f32, (NO,)), ("fobs", f32, (NO,)), ("reward", f32, ()), ("error", f32, ()),
                  ("steps", i32, ()), ("term", u8, ()), ("trunc", u8, ()), ("done", u8, ())]
        self._plain_buffers(fields)
        # a step writes final_obs rows of FINISHED envs only (64 B per env-step that ~93 % of the envs do not need): copy=True /
        # to_numpy hand out zero rows elsewhere (zero_on_refill); with copy=False the rows of unfinished envs keep whatever an
        # earlier episode end left there — read them under info["_final_obs"]
        self._make_step_outputs(fields, ("obs", "reward", "term", "trunc", "cmd", "error", "fobs", "steps", "done"),
                                as_bool=("term", "trunc", "done"), zero_on_refill=("fobs",),
                                derived={"obs_u": ("obs", cut), "cmd_u": ("cmd", cut), "fobs_u": ("fobs", cut)})
        self._path_name = "auto"
        self._command_type = np.where(tab["ints"][:, 3] > 0, "dynamic_target", "static_target") \
            if not torch.is_tensor(tab["ints"]) else None
        self.task_set = True
        self.need_reset = True

    PATH = {"auto": 0, "mfma": 1, "scalar": 2}

    def set_path(self, path):
        """Select the step kernel ("auto", "mfma", "scalar"); results are identical (include/xeno.h)."""
        _lib.check(self.lib.xv_linds_set_path(self._h, self.PATH[path]))
        self._path_name = path

    def set_command_table(self, enable):
        """Use the per-task table of get_inner_cmd values built at set_task (default) or evaluate the Fourier
        terms in every step; the results are identical."""
        _lib.check(self.lib.xv_linds_set_command_table(self._h, 1 if enable else 0))

    # -- helpers ------------------------------------------------------------------------------------
    def _user_obs(self, t):
        return t[:, :self.user_dims[1]]

    def _action(self, actions, lead=()):
        """actions float[lead..., N, na_user] (lead: () for one step, (P,) for a ring or a roll-out) -> contiguous
        float32[lead..., N, NA] on the device, zero in the padded columns"""
        a = self._dev(actions, torch.float32)
        na_user = self.user_dims[0]
        want = tuple(lead) + (self.num_envs, na_user)
        if a.shape != want:
            # reference: assert numpy.shape(action) == (self.pad_action_dim,) (linds_env.py:137)
            raise AssertionError(f"Action shape mismatch: expected {want}, got {tuple(a.shape)}")
        if na_user != self.NA:
            p = torch.zeros(want[:-1] + (self.NA,), dtype=torch.float32, device=self.device)
            p[..., :na_user] = a
            a = p
        return a.contiguous()

    def _rollout_spec(self):
        """what a roll-out / step_many slot holds per step, as _alloc takes it: the first four without infos.  final_obs is
        zero-filled: the kernels write the rows of finished envs only"""
        f32, u8, NO = torch.float32, torch.uint8, self.NO
        return [("obs", f32, (NO,)), ("reward", f32, ()), ("terminated", u8, ()), ("truncated", u8, ()),
                ("command", f32, (NO,)), ("error", f32, ()), ("final_obs", f32, (NO,), 0)]

    def _steps_now(self):
        st = torch.empty(self.num_envs, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.xv_linds_get_state(self._h, None, _lib.ptr(st), None))
        return st

    def _reset_infos(self):
        return {"steps": self._out(self._steps_now()), "command": self._o(self._user_obs(self._cmd)), "error": self._o(self._error)}

    # -- API ----------------------------------------------------------------------------------------
    def reset(self, *, seed=None, options=None):
        mask = self._reset_prelude(seed, options)
        self._adopt_latest(_obs="obs", _cmd="cmd", _error="error")
        self._detach("_obs", "_cmd", "_error")
        _lib.check(self.lib.xv_linds_reset(self._h, _lib.ptr(mask), _lib.ptr(self._obs), _lib.ptr(self._cmd),
                                           _lib.ptr(self._error)))
        self.need_reset = False
        infos = self._reset_infos()
        if self._command_type is not None:
            infos["command_type"] = self._command_type[self._tab["env_task"].cpu().numpy()]
        return self._o(self._user_obs(self._obs)), infos

    def reset_injected(self, init_index, mask=None):
        self._require_task()
        idx = self._dev(init_index, torch.int32)
        m = None if mask is None else self._dev(mask, torch.uint8)
        self._adopt_latest(_obs="obs", _cmd="cmd", _error="error")
        self._detach("_obs", "_cmd", "_error")
        _lib.check(self.lib.xv_linds_reset_injected(self._h, _lib.ptr(m), _lib.ptr(idx), _lib.ptr(self._obs),
                                                    _lib.ptr(self._cmd), _lib.ptr(self._error)))
        self.need_reset = False
        return self._o(self._user_obs(self._obs)), self._reset_infos()

    _check_step = VectorEnv._require_reset

    def _steps_and_done(self, s):
        """after a launch that writes the first seven outputs only (the scalar test kernel, step_injected): `steps` and the done
        mask by a launch / an op of their own — left out, with their infos, when lean_infos asks for no extra launches"""
        if not self.lean_infos:
            _lib.check(self.lib.xv_linds_get_state(self._h, None, s.ptr["steps"], None))
            torch.bitwise_or(s.t["term"], s.t["trunc"], out=s.t["done"])
        return self._finish(s, not self.lean_infos)

    def _finish(self, s, full=True):
        """the output set a step launch has written -> step()'s return value"""
        t = s.t
        infos = {"command": t["cmd_u"], "error": t["error"]}
        if full:
            infos["steps"] = t["steps"]
        if self._auto == 2:      # same_step
            infos["final_obs"] = t["fobs_u"]
            if full:
                infos["_final_obs"] = t["done"]
        if self.to_numpy:
            return self._numpy(t["obs_u"], t["reward"], t["term"], t["trunc"], infos)
        return t["obs_u"], t["reward"], t["term"], t["trunc"], infos

    def step(self, actions):
        self._check_step()
        a = self._action(actions)
        s = self._outputs.next()
        if self._path_name == "scalar":      # the test kernel
            _lib.check(self.lib.xv_linds_step(self._h, _lib.ptr(a), *s.args[:7], AUTORESET[self.autoreset_mode]))
            return self._steps_and_done(s)
        # ONE launch: the step kernel writes info["steps"] and the terminated | truncated mask itself
        _lib.step_call("xv_linds_step_info", self._h, a, s, self._auto)
        return self._finish(s)

    def step_injected(self, actions, z, init_index):
        """Parity hook: z float[NS, N] standard normals (process noise), init_index int[N] (used on reset)."""
        self._check_step()
        a = self._action(actions)
        z = self._dev(z, torch.float32)
        if z.shape[0] != self.NS:
            p = torch.zeros((self.NS, self.num_envs), dtype=torch.float32, device=self.device)
            p[:z.shape[0]] = z
            z = p
        idx = self._dev(init_index, torch.int32)
        s = self._outputs.next()
        _lib.check(self.lib.xv_linds_step_injected(self._h, _lib.ptr(a), _lib.ptr(z.contiguous()), _lib.ptr(idx), *s.args[:7],
                                                   AUTORESET[self.autoreset_mode]))
        return self._steps_and_done(s)

    def step_many(self, n_steps, actions, out=None):
        """n_steps vector steps issued from C (xv_linds_step_many): actions float32[P, N, na] is a ring of P action sets,
        step k uses slot k % P and writes slot k % P of the returned dict of [P, N(, NO)] device tensors.  Equals n_steps
        calls of step(); `final_obs` rows are written for finished envs only."""
        self._check_step()
        P = len(actions)
        a = self._action(actions, (P,))
        if out is None:
            out = self._alloc(self._rollout_spec(), (P,))
        _lib.check(self.lib.xv_linds_step_many(self._h, int(n_steps), P, _lib.ptr(a), _lib.ptr(out["obs"]),
                                               _lib.ptr(out["reward"]), _lib.ptr(out["terminated"]),
                                               _lib.ptr(out["truncated"]), _lib.ptr(out["command"]), _lib.ptr(out["error"]),
                                               _lib.ptr(out.get("final_obs")), AUTORESET[self.autoreset_mode]))
        return out

    def rollout(self, actions, out=None, with_info=True):
        """Fused open-loop roll-out: actions float32[T, N, na] -> dict of [T, N(, NO)] device tensors, one launch with the
        state resident in registers between the steps.  Equals T calls of step() with SAME_STEP auto-reset, bit for bit."""
        self._check_step()
        T = len(actions)
        a = self._action(actions, (T,))
        if out is None:      # (a caller-supplied `out` keeps the final_obs rows of unfinished envs)
            out = self._alloc(self._rollout_spec() if with_info else self._rollout_spec()[:4], (T,))
        _lib.check(self.lib.xv_linds_rollout(self._h, T, _lib.ptr(a), _lib.ptr(out["obs"]), _lib.ptr(out["reward"]),
                                             _lib.ptr(out["terminated"]), _lib.ptr(out["truncated"]),
                                             _lib.ptr(out.get("command")), _lib.ptr(out.get("error")),
                                             _lib.ptr(out.get("final_obs"))))
        return out

    @property
    def state(self):
        """env.state (linds_env.py:185-187): float[N, NS]"""
        x = torch.empty((self.NS, self.num_envs), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.xv_linds_get_state(self._h, _lib.ptr(x), None, None))
        return self._out(x.t().contiguous())

    def get_future_inner_cmds(self, K):
        """the next K inner commands of every env, starting with the one tracked at the next step
        (linds_env.py:171-183): float32[N, K, NO] on the host; command(t) = cmd_fn(t) * target_valid."""
        st = self._steps_now().cpu().numpy()
        t = self._tab
        task = t["env_task"].cpu().numpy()
        ints = t["ints"].cpu().numpy()[task]
        delay, nf = ints[:, 1], ints[:, 3]
        tt = st[:, None] - delay[:, None] + np.arange(K)[None, :]                     # [N, K]
        om = t["four_omega"].cpu().numpy()[task]                                       # [N, KMAX]
        per = t["four_period"].cpu().numpy()[task]
        co = t["four_coef"].cpu().numpy()[task].astype(np.float64)                     # [N, KMAX, NO, 2]
        ang = om[:, None, :] * (tt[:, :, None] / per[:, None, None])                   # [N, K, KMAX]
        live = (np.arange(om.shape[1])[None, :] < nf[:, None])[:, None, :, None]
        dyn = ((np.sin(ang)[..., None] * co[:, None, :, :, 0] + np.cos(ang)[..., None] * co[:, None, :, :, 1]) * live).sum(2)
        static = t["cmd0"].cpu().numpy()[task][:, None, :].astype(np.float64)
        cmd = np.where((nf > 0)[:, None, None], dyn, static) * t["valid"].cpu().numpy()[task][:, None, :]
        return cmd[..., :self.user_dims[1]].astype(np.float32)

    def get_state(self):
        x = torch.empty((self.NS, self.num_envs), dtype=torch.float32, device=self.device)
        st = torch.empty(self.num_envs, dtype=torch.int32, device=self.device)
        nr = torch.empty(self.num_envs, dtype=torch.uint8, device=self.device)
        _lib.check(self.lib.xv_linds_get_state(self._h, _lib.ptr(x), _lib.ptr(st), _lib.ptr(nr)))
        return x, st, nr

    def set_state(self, x=None, steps=None, need_reset=None):
        """x float[NS_user or NS, N] component-major"""
        xs = None
        if x is not None:
            xs = self._dev(x, torch.float32)
            if xs.shape[0] != self.NS:
                p = torch.zeros((self.NS, self.num_envs), dtype=torch.float32, device=self.device)
                p[:xs.shape[0]] = xs
                xs = p
            xs = xs.contiguous()
        st = None if steps is None else self._dev(steps, torch.int32)
        nr = None if need_reset is None else self._dev(need_reset, torch.uint8)
        _lib.check(self.lib.xv_linds_set_state(self._h, _lib.ptr(xs), _lib.ptr(st), _lib.ptr(nr)))
        self.engine.sync()
        self.need_reset = False

    # -- MPC teacher (linds/teacher.py, csrc/linds_mpc.hip) --------------------------------------------
    MPC_MAX_ITER = 4000

    def mpc_models(self):
        """the fp64 LTI model of every task (linds.teacher._Model): from the task dicts given to set_task, or from host
        tables (their fp32 values)"""
        from . import teacher
        src = getattr(self, "_mpc_src", None)
        if src is None:
            raise ValueError("the MPC teacher needs the task dicts or host (numpy) tables given to set_task")
        if isinstance(src, dict):
            return [teacher.model_from_tables(src, t) for t in range(self.n_task)]
        memo = {}      # a task dict repeated over many task indices is discretised once
        for t in src:
            if id(t) not in memo:
                memo[id(t)] = teacher.model_from_task(t, dt=self.dt, pad_action_dim=self.pad_action_dim)
        return [memo[id(t)] for t in src]

    def _drop_mpc(self):
        c = getattr(self, "_mpc_cache", None)
        if c is not None and getattr(self, "lib", None) is not None:
            self.lib.xv_linds_mpc_destroy(c[1])
        self._mpc_cache = None

    def _mpc(self, K, gamma, max_iter=None):
        """the device teacher's handle for (K, gamma), built once per set_task (cached like AnyMDP's greedy table)"""
        from . import teacher
        max_iter = self.MPC_MAX_ITER if max_iter is None else int(max_iter)
        key = (id(self._tab), int(K), float(gamma), max_iter)
        c = getattr(self, "_mpc_cache", None)
        if c is not None and c[0] == key:
            return c[1], c[2]
        self._drop_mpc()
        dt = teacher.device_tables(self.mpc_models(), K, gamma, self.NS, self.NO)
        ct = _MPCTables(dt["n_pad"], dt["n_in"], dt["NOc"], dt["mfrag"].ctypes.data, dt["gfrag"].ctypes.data,
                        dt["g0"].ctypes.data, dt["rho"].ctypes.data, dt["mnorm"].ctypes.data, dt["nu"].ctypes.data, teacher.SIGMA, teacher.ALPHA,
                        teacher.EPS_ABS, teacher.EPS_REL)
        h = C.c_void_p()
        _lib.check(self.lib.xv_linds_mpc_create(self._h, int(K), float(gamma), C.byref(ct), max_iter, C.byref(h)))
        info = dict(n_pad=dt["n_pad"], n_in=dt["n_in"], NOc=dt["NOc"], nu=dt["nu"], rho=dt["rho"])
        self._mpc_cache = (key, h, info)
        return h, info

    def mpc_action(self, K=20, gamma=0.99, return_info=False, max_iter=None):
        """The reference's MPC teacher (LTISystemMPC(env, K, gamma).solve(env.state, env.get_future_inner_cmds(K)),
        xenoverse/linds/solver.py:94-125) for every env, on the device, without stepping: float32[N, action_dim]
        (+ dict(status=int32[N] 1 converged / 0 max_iter, iters=int32[N], U=float32[N, n_pad] the whole plan U[k * Nu + a])
        with return_info)."""
        self._check_step()
        h, info = self._mpc(K, gamma, max_iter)
        n, d = self.num_envs, self.device
        a = torch.empty((n, self.NA), dtype=torch.float32, device=d)
        st = torch.empty(n, dtype=torch.int32, device=d)
        it = torch.empty(n, dtype=torch.int32, device=d)
        U = torch.empty((n, info["n_pad"]), dtype=torch.float32, device=d) if return_info else None
        _lib.check(self.lib.xv_linds_mpc_action(h, _lib.ptr(a), _lib.ptr(U), _lib.ptr(st), _lib.ptr(it)))
        a = a[:, :self.user_dims[0]]
        return (a, dict(status=st, iters=it, U=U)) if return_info else a

    def mpc_solve(self, x, ref, K=20, gamma=0.99, max_iter=None):
        """Parity hook (xv_linds_mpc_solve): x float[N, <=NS], ref float[N, K, <=NO] -> (U float32[N, n_pad] with
        U[k * Nu + a], status int32[N], iters int32[N]) for each env's task"""
        self._require_task()
        h, _ = self._mpc(K, gamma, max_iter)
        n, d = self.num_envs, self.device
        xs = torch.zeros((n, self.NS), dtype=torch.float32, device=d)
        xi = self._dev(x, torch.float32)
        xs[:, :xi.shape[1]] = xi
        rs = torch.zeros((n, K, self.NO), dtype=torch.float32, device=d)
        ri = self._dev(ref, torch.float32)
        rs[:, :, :ri.shape[2]] = ri
        info = self._mpc_cache[2]
        U = torch.empty((n, info["n_pad"]), dtype=torch.float32, device=d)
        st = torch.empty(n, dtype=torch.int32, device=d)
        it = torch.empty(n, dtype=torch.int32, device=d)
        _lib.check(self.lib.xv_linds_mpc_solve(h, _lib.ptr(xs), _lib.ptr(rs), _lib.ptr(U), _lib.ptr(st), _lib.ptr(it)))
        return U, st, it

    def rollout_teacher(self, T, K=20, gamma=0.99, max_iter=None):
        """T steps driven by the device MPC teacher (xv_linds_rollout_mpc), SAME_STEP auto-reset: dict of [T, N(, ...)]
        device tensors — the outputs of rollout() plus "action" [T, N, NA], "status" and "iters" [T, N].  Equals T x
        (mpc_action(K, gamma) + step) bit for bit."""
        self._check_step()
        T = int(T)
        h, _ = self._mpc(K, gamma, max_iter)
        i32 = torch.int32
        out = self._alloc([("action", torch.float32, (self.NA,))] + self._rollout_spec() + [("status", i32, ()), ("iters", i32, ())],
                          (T,))
        _lib.check(self.lib.xv_linds_rollout_mpc(h, T, *[_lib.ptr(out[k]) for k in (
            "action", "obs", "reward", "terminated", "truncated", "command", "error", "final_obs", "status", "iters")]))
        return out

    def close_extras(self, **kwargs):
        self._drop_mpc()
        if self._h is not None:
            self.lib.xv_linds_destroy(self._h)
            self._h = None
        self._tab = None
