"""LinDS task sampling on the GPU: `sample_tasks_device` returns n accepted tasks as the device tables
`LinDSVecEnv.set_task` takes as they are, generated, searched and discretised by `xv_linds_sample_tasks`
(csrc/linds_sampler.hip), one workgroup per candidate; `build_tables_device` is `linds.tables.build_tables` with the
per-task `scipy.linalg.expm` replaced by one `xv_linds_build_zoh` launch.

Same generative model as the reference's LinearDSSampler / LinearDSSamplerRandomDim (xenoverse/linds/task_sampler.py:12-154,
RandomFourier utils/random_nn.py:346-368) with counter-based randomness: task k of (seed, dims arguments) is the k-th
ACCEPTED candidate in candidate order, a pure function of those arguments whatever the batch size — but not the task
NumPy's stream gives for that seed (for that, the host sampler `LinearDSSampler(seed=...)`).  Three documented departures
(DESIGN.md §3.2): no rank test on B and C, a start attempt with more than `max_init` initial states fails, and a candidate
without a passing attempt below `max_draws` is dropped as `exhausted` (the host sampler's shrinking fallback is not
reproduced: the population is the reference's, conditioned on passing within max_draws).  The numpy restatement the device
is tested against is linds/sampler_host.py.
"""
import ctypes as C
import time

import numpy as np
import torch

from .. import _lib
from ..device_sampling import collect_accepted, engine_scope, sampler_stats
from . import sampler_host as sh
from .tables import KMAX, _Tables, _pack, _pad_to

STATUS = sh.STATUS

INFO_DTYPE = np.dtype([("status", "<i4"), ("attempt", "<i4"), ("ns", "<i4"), ("na", "<i4"), ("no", "<i4"), ("a_scale", "<i4"),
                       ("x_scale", "<i4"), ("trim", "<i4"), ("width", "<i4"), ("max_steps", "<i4"), ("n_init", "<i4"),
                       ("n_terms", "<i4"), ("delay", "<i4"), ("type", "<i4"), ("valid_rounds", "<i4"), ("zoh_s", "<i4"),
                       ("target_valid", "i1", 32), ("action_cost", "<f8"), ("reward_base", "<f8"), ("terminate_punish", "<f8"),
                       ("reward_factor", "<f8"), ("noise_drift", "<f8"), ("eps", "<f8")], align=True)   # xv_linds_cand_info

TABLE_KEYS = ("phiT", "gamT", "cT", "xt", "y0", "valid", "cmd0", "four_coef", "four_omega", "four_period", "scal", "ints", "init")
DENSE_KEYS = ("A", "B", "C", "X", "Y", "init64", "phi", "gam", "four_order", "four_coef64", "cmd064")


class _Dense(C.Structure):   # xv_linds_dense (include/xeno.h)
    _fields_ = [(k, C.c_void_p) for k in ("A", "B", "C", "X", "Y", "init", "phi", "gam", "four_order", "four_coef", "cmd0")]


def _table_shapes(n, NS, NA, NO, NI):
    f32, f64, i32 = torch.float32, torch.float64, torch.int32
    return dict(phiT=((n, NS, NS), f32), gamT=((n, NA, NS), f32), cT=((n, NS, NO), f32), xt=((n, NS), f32), y0=((n, NO), f32),
                valid=((n, NO), f32), cmd0=((n, NO), f32), four_coef=((n, KMAX, NO, 2), f32), four_omega=((n, KMAX), f64),
                four_period=((n,), f64), scal=((n, 8), f32), ints=((n, 4), i32), init=((n, NI, NS), f32))


def _dense_shapes(n, NS, NA, NO, NI):
    return dict(A=(n, NS, NS), B=(n, NS, NA), C=(n, NO, NS), X=(n, NS), Y=(n, NO), init64=(n, NI, NS), phi=(n, NS, NS),
                gam=(n, NS, NA), four_order=(n, KMAX), four_coef64=(n, KMAX, NO, 2), cmd064=(n, NO))


def default_pads(state_dim, action_dim, observation_dim, random_dim, pad_action_dim, pad_observation_dim):
    """(NS, NA, NO) the step engine is compiled for that hold every dim the arguments can give"""
    ns, na, no = int(state_dim), int(action_dim), int(observation_dim)
    if random_dim:      # LinearDSSamplerRandomDim raises the caller's maxima to its own minima
        na, no = max(na, (ns + 1) // 2), max(no, ns // 4)
    return _pad_to(ns, (16, 32)), _pad_to(max(na, int(pad_action_dim)), (8, 16)), _pad_to(max(no, int(pad_observation_dim)), (16, 32))


def sample_candidates(engine, seed, cand_base, n_cand, state_dim=16, action_dim=8, observation_dim=8, random_dim=False,
                      dt=0.1, pad_observation_dim=16, pad_action_dim=8, max_init=8, max_draws=1 << 20, tables=True,
                      dense=False, info=False, pad_state_dim=None):
    """One launch over candidates [cand_base, cand_base + n_cand).  -> dict with `status` int32[n_cand] (device), NS / NA /
    NO / NI, and, as requested, the table slots (zero where status != 0), the dense fp64 tensors (A, B, C, X, Y for every
    candidate; init64, phi, gam, four_order, four_coef64, cmd064 for accepted ones) and the info records.
    With random_dim the three dims are LinearDSSamplerRandomDim's maxima."""
    d = engine.device
    NS, NA, NO = default_pads(state_dim, action_dim, observation_dim, random_dim, pad_action_dim, pad_observation_dim)
    if pad_state_dim is not None:
        NS = int(pad_state_dim)
    NI = int(max_init)
    out = dict(status=torch.empty(n_cand, dtype=torch.int32, device=d), NS=NS, NA=NA, NO=NO, NI=NI, dt=float(dt))
    ct = dn = None
    if tables or dense:
        for k, (shape, dtype) in _table_shapes(n_cand, NS, NA, NO, NI).items():
            out[k] = torch.zeros(shape, dtype=dtype, device=d)
        out["four_period"].fill_(1.0)
        ct = _Tables(*[_lib.ptr(out[k]) for k in TABLE_KEYS])
    if dense:
        for k, shape in _dense_shapes(n_cand, NS, NA, NO, NI).items():
            out[k] = torch.zeros(shape, dtype=torch.float64, device=d)
        dn = _Dense(*[_lib.ptr(out[k]) for k in DENSE_KEYS])
    if info:
        out["info_raw"] = torch.zeros((n_cand, INFO_DTYPE.itemsize), dtype=torch.uint8, device=d)
    _lib.check(engine.lib.xv_linds_sample_tasks(
        engine.handle, int(seed) & (2**64 - 1), int(cand_base), int(n_cand), 1 if random_dim else 0, int(state_dim),
        int(action_dim), int(observation_dim), NS, NA, NO, NI, float(dt), int(max_draws),
        None if ct is None else C.cast(C.byref(ct), C.c_void_p), None if dn is None else C.cast(C.byref(dn), C.c_void_p),
        _lib.ptr(out.get("info_raw")), _lib.ptr(out["status"])))
    if info:
        engine.sync()
        out["info"] = out.pop("info_raw").cpu().numpy().view(INFO_DTYPE).reshape(n_cand)
    return out


def sample_tasks_device(n_tasks, state_dim=16, action_dim=8, observation_dim=8, random_dim=False, seed=0, dt=0.1,
                        pad_observation_dim=16, pad_action_dim=8, max_draws=1 << 20, engine=None, device="cuda:0", batch=None,
                        dense=False, max_init=8, max_candidates=None):
    """n_tasks accepted tasks -> the tables dict of linds.tables.build_tables with device tensors (NS, NA, NO, NI, dt, phiT,
    gamT, cT, xt, y0, valid, cmd0, four_coef, four_omega, four_period, scal, ints, init; action_dims and `info` on the
    host; with dense=True also the fp64 tensors) + "stats": candidates tried, status histogram, histogram of the accepted
    attempt index (bin b: attempts in [2^b - 1, 2^(b+1) - 1)), seconds.  Task k is the k-th accepted candidate in candidate
    order, whatever `batch` is.  `LinDSVecEnv.set_task(tables)` takes the result as it is."""
    if batch is None:
        batch = int(max(64, min(4096, 2 * n_tasks)))
    keys = list(TABLE_KEYS) + (list(DENSE_KEYS) if dense else [])
    NS, NA, NO = default_pads(state_dim, action_dim, observation_dim, random_dim, pad_action_dim, pad_observation_dim)
    with engine_scope(engine, device) as eng:
        t0 = time.perf_counter()
        got, info, hist = collect_accepted(
            lambda base, n: sample_candidates(eng, seed, base, n, state_dim, action_dim, observation_dim, random_dim, dt,
                                              pad_observation_dim, pad_action_dim, max_init, max_draws, tables=True,
                                              dense=dense, info=True),
            n_tasks, batch, keys, STATUS, max_candidates)
        out = dict(NS=NS, NA=NA, NO=NO, NI=int(max_init), dt=float(dt), **got)      # as sample_candidates has them
        out["info"] = info
        out["action_dims"] = info["na"].astype(np.int32)
        eng.sync()
        attempts = info["attempt"]
        out["stats"] = sampler_stats(
            hist, STATUS, batch, t0, attempts_total=int(attempts.astype(np.int64).sum() + len(info)),
            attempts_log2=np.bincount(np.floor(np.log2(attempts.astype(np.float64) + 1.0)).astype(np.int64), minlength=1).tolist())
        return out


def task_dicts_from_device(out):
    """a dense=True result of sample_tasks_device (or the accepted rows of sample_candidates) -> reference-schema task dicts
    (SURVEY.md §8(a) L1): what dump_task, the host build_tables and the MPC teacher take.  A dynamic task's command is an
    object with `coeffs` and `max_steps`, as `linds.tables.fourier_terms` expects."""
    if "A" not in out or "info" not in out:
        raise ValueError("task_dicts_from_device needs a dense=True result with its info records")
    info = out["info"]
    g = {k: out[k].detach().cpu().numpy() for k in DENSE_KEYS}
    tasks = []
    for i, r in enumerate(info):
        if r["status"] != 0:
            raise ValueError("candidate %d was not accepted (status %s)" % (i, STATUS[int(r["status"])]))
        ns, na, no = int(r["ns"]), int(r["na"]), int(r["no"])
        head = dict(ns=ns, na=na, no=no, max_steps=int(r["max_steps"]), A=g["A"][i, :ns, :ns], B=g["B"][i, :ns, :na],
                    C=g["C"][i, :no, :ns], X=g["X"][i, :ns], Y=g["Y"][i, :no], action_cost=r["action_cost"],
                    reward_base=r["reward_base"], terminate_punish=r["terminate_punish"], reward_factor=r["reward_factor"],
                    target_valid=r["target_valid"][:no], type=int(r["type"]))
        tasks.append(sh.task_dict(head, r["n_init"], r["noise_drift"], r["delay"], g["init64"][i], cmd0=g["cmd064"][i],
                                  orders=g["four_order"][i], coef=g["four_coef64"][i], n_terms=r["n_terms"]))
    return tasks


def build_zoh_device(engine, A, B, X, ns, dt=0.1, dense=False):
    """xv_linds_build_zoh: A float64[n, NS, NS], B float64[n, NS, NA], X float64[n, NS] (zero-padded beyond ns[t]; numpy or
    device tensors) -> dict(phiT, gamT, xt float32 device tensors, status int32[n] (0 ok, 1 non-finite, 2 scale cap),
    and with dense the fp64 phi, gam)"""
    d = engine.device
    A, B, X = (torch.as_tensor(np.ascontiguousarray(v, np.float64)).to(d) if not torch.is_tensor(v)
               else v.to(d, torch.float64).contiguous() for v in (A, B, X))
    n, NS, NA = int(A.shape[0]), int(A.shape[1]), int(B.shape[2])
    if A.shape != (n, NS, NS) or B.shape != (n, NS, NA) or X.shape != (n, NS):
        raise ValueError("shapes: A [n, NS, NS], B [n, NS, NA], X [n, NS]")
    nst = torch.as_tensor(np.ascontiguousarray(ns, np.int32)).to(d) if not torch.is_tensor(ns) else ns.to(d, torch.int32).contiguous()
    out = dict(phiT=torch.empty((n, NS, NS), dtype=torch.float32, device=d), gamT=torch.empty((n, NA, NS), dtype=torch.float32, device=d),
               xt=torch.empty((n, NS), dtype=torch.float32, device=d), status=torch.empty(n, dtype=torch.int32, device=d))
    if dense:
        out.update(phi=torch.empty((n, NS, NS), dtype=torch.float64, device=d), gam=torch.empty((n, NS, NA), dtype=torch.float64, device=d))
    _lib.check(engine.lib.xv_linds_build_zoh(engine.handle, n, _lib.ptr(nst), NS, NA, _lib.ptr(A), _lib.ptr(B), _lib.ptr(X),
                                             float(dt), _lib.ptr(out["phiT"]), _lib.ptr(out["gamT"]), _lib.ptr(out["xt"]),
                                             _lib.ptr(out.get("phi")), _lib.ptr(out.get("gam")), _lib.ptr(out["status"])))
    return out


def build_tables_device(tasks, engine, dt=0.1, pad_observation_dim=16, pad_action_dim=8, pad_command_dim=16):
    """`linds.tables.build_tables` (same arguments, same dict of host arrays) with its per-task expm replaced by one
    xv_linds_build_zoh launch over all tasks.  Opt-in: `LinDSVecEnv.set_task` keeps using the host builder."""
    _, tab, (A, B, X, nsv) = _pack(tasks, dt, pad_observation_dim, pad_action_dim, pad_command_dim)
    z = build_zoh_device(engine, A, B, X, nsv, dt)
    engine.sync()
    status = z["status"].cpu().numpy()
    if status.any():
        bad = np.nonzero(status)[0]
        raise ValueError("zero-order hold failed for task(s) %s (status %s: 1 non-finite, 2 scale cap)"
                         % (bad.tolist(), status[bad].tolist()))
    tab.update(phiT=z["phiT"].cpu().numpy(), gamT=z["gamT"].cpu().numpy(), xt=z["xt"].cpu().numpy())
    return tab
