"""ChemVerse's ground-truth cost oracle (the reference's ChemistryEnvironment.compute_optimal_cost, environment/api.py:1777-2266)
for one world or a batch of (world, constraints) requests.

  compute_optimal_cost(world, ...)            the reference's signature and result dict
  compute_optimal_costs(worlds, requests)     every request's candidates through ONE set of launches
  chain_costs(worlds, candidates)             _compute_chain_cost for chosen routes
  one_pot_costs(worlds, requests)             _compute_one_pot_cost for chosen (world, target)
  ChemVerseOptimal(worlds, capacity)          the handle behind them: worlds and workspace kept across calls

backend "device": the searches run in csrc/chemverse_optimal.hip (xv_chem_optimal), a lane per candidate; "host": in
optimal_host.py.  Route search, optimal conditions, rounding and pricing are optimal_host's for both.
"""
import ctypes as C

import numpy as np

from .. import _lib
from . import optimal_host as H
from . import tables as T
from .batch import LANES, ChemVerseBatch, group_by_world

BACKENDS = ("device", "host")


def _tables(worlds):
    if isinstance(worlds, dict) or hasattr(worlds, "chemicals"):
        worlds = [worlds]
    if not len(worlds):
        raise ValueError("at least one world is needed")
    return [T.build_tables(w) for w in worlds]


class ChemVerseOptimal(object):
    """worlds as ChemVerseBatch takes them; capacity: the most candidates one call takes (a request is 5 to 50)"""

    def __init__(self, worlds, capacity=4096, engine=None, device="cuda:0"):
        self.batch = ChemVerseBatch(_tables(worlds), capacity, engine=engine, device=device)
        self.capacity = self.batch.capacity
        self.time_launches = False      # True: solve() times every launch (scripts/bench_chemverse_optimal.py)
        self.last_launch_ms = None
        self.last_launches = 0

    @property
    def tables(self):
        return self.batch.tables

    def set_worlds(self, worlds):
        self.batch.set_worlds(_tables(worlds))

    def solve(self, worlds, plans, thresholds):
        """plans (optimal_host.chain_plan / one_pot_plans) of the worlds worlds[i], each passing at yield >= thresholds[i]
        -> per plan dict(found, best_scale, bits, yield, rows) as optimal_host.bisect_plan gives it"""
        import torch
        b = self.batch
        n = len(plans)
        if n < 1:
            return []
        if n > self.capacity:
            raise ValueError("%d candidates are more than this handle's capacity %d" % (n, self.capacity))
        world = np.asarray(worlds, np.int32)
        if world.shape != (n,) or world.min() < 0 or world.max() >= len(b.tables):
            raise ValueError("worlds must be %d indices in [0, %d)" % (n, len(b.tables)))
        ls, ks = H.plan_widths(plans)
        if ls > T.CHAIN_MAX:
            raise T._unsupported("reactions per route", ls, "CHAIN_MAX", T.CHAIN_MAX)
        cs = b.c_stride
        total_steps = np.array([sum(T.num_steps_of(s["dur"], H.STEP_SECONDS) for s in p["steps"]) for p in plans], np.int64)
        slot_of, cand_of = group_by_world(world, total_steps)
        n_pad = len(cand_of)
        a = dict(world=np.full(n_pad, -1, np.int32), n_step=np.zeros(n_pad, np.int32), equipment=np.zeros(n_pad, np.int32),
                 target=np.zeros(n_pad, np.int32), mode=np.zeros(n_pad, np.int32), n_iter=np.zeros(n_pad, np.int32),
                 threshold=np.zeros(n_pad), lo=np.zeros(n_pad), hi=np.zeros(n_pad), step_T=np.full((n_pad, ls), 25.0),
                 step_dur=np.ones((n_pad, ls)), n_charge=np.zeros((n_pad, ls), np.int32),
                 charge=np.zeros((n_pad, ls, ks), np.int32))
        for i, p in enumerate(plans):
            k = slot_of[i]
            tab = b.tables[world[i]]
            if not (0 <= p["target"] < tab["C"] and 0 <= p["equipment"] < tab["E"]):
                raise ValueError("candidate %d: target or equipment outside its world" % i)
            if not (1 <= p["n_iter"] <= H.CHAIN_ITERS and 1e-7 < p["lo"] <= p["hi"] < 1e12):
                raise ValueError("candidate %d: the bisection needs 1 to %d iterations on a positive range" % (i, H.CHAIN_ITERS))
            thr = float(thresholds[i])
            if not np.isfinite(thr):
                raise ValueError("candidate %d: the yield threshold must be finite" % i)
            a["world"][k], a["n_step"][k], a["equipment"][k] = world[i], len(p["steps"]), p["equipment"]
            a["target"][k], a["mode"][k], a["n_iter"][k] = p["target"], p["mode"], p["n_iter"]
            a["threshold"][k], a["lo"][k], a["hi"][k] = thr, p["lo"], p["hi"]
            for s, step in enumerate(p["steps"]):
                a["step_T"][k, s], a["step_dur"][k, s], a["n_charge"][k, s] = step["T"], step["dur"], len(step["entries"])
                for j, (c, kind) in enumerate(step["entries"]):
                    if not (0 <= c < tab["C"] and 0 <= kind <= 3):
                        raise ValueError("candidate %d: a charge entry outside its world" % i)
                    a["charge"][k, s, j] = c | (kind << 8)
        order = ("world", "n_step", "equipment", "target", "mode", "n_iter", "threshold", "lo", "hi", "step_T", "step_dur",
                 "n_charge", "charge")
        ins = [torch.from_numpy(np.ascontiguousarray(a[k])).to(b.device) for k in order]
        f64, u8 = torch.float64, torch.uint8
        shapes = dict(best_scale=((), f64), found=((), u8), bits=((), torch.int32), charged=((ls, ks), f64),
                      consumed=((ls, cs), f64), produced=((ls, cs), f64), byproduct=((ls, cs), f64), final_pool=((cs,), f64),
                      failure=((ls,), u8))
        shapes["yield"] = ((), f64)
        # zeros, not empty: rows of padding lanes and of candidates not found are never written
        raw = dict((k, torch.zeros((n_pad,) + shapes[k][0], dtype=shapes[k][1], device=b.device)) for k in _lib.ChemOptOut.FIELDS)
        out = _lib.ChemOptOut(**dict((k, _lib.ptr(raw[k])) for k in _lib.ChemOptOut.FIELDS))
        n_pass = int(max(p["n_iter"] for p in plans))
        ms = (C.c_float * (n_pass + 2))() if self.time_launches else None
        _lib.check(b.lib.xv_chem_optimal(b._h, n_pad, ls, ks, n_pass, *(_lib.ptr(t) for t in ins), H.STEP_SECONDS,
                                         C.byref(out), ms))
        res = dict((k, raw[k].cpu().numpy()[slot_of]) for k in _lib.ChemOptOut.FIELDS)      # .cpu() waits for the stream
        b.engine.sync()      # the inputs must outlive the launches
        self.last_launches = n_pass + 2
        self.last_launch_ms = list(ms) if ms is not None else None
        flags = b.check_errors()
        if flags:
            raise _lib.XenoError("ChemVerse: device error flags 0x%x (include/xeno.h XV_DEVERR_*)" % flags)
        solved = []
        for i, p in enumerate(plans):
            found = bool(res["found"][i])
            C_w, n, k = b.tables[world[i]]["C"], len(p["steps"]), max(1, max(len(s["entries"]) for s in p["steps"]))
            rows = None
            if found:
                rows = dict(charged=res["charged"][i, :n, :k], consumed=res["consumed"][i, :n, :C_w],
                            produced=res["produced"][i, :n, :C_w], byproduct=res["byproduct"][i, :n, :C_w],
                            failure=res["failure"][i, :n], final_pool=res["final_pool"][i, :C_w])
                rows["yield"] = float(res["yield"][i])
            solved.append({"found": found, "best_scale": float(res["best_scale"][i]),
                           "bits": int(res["bits"][i]) & 0xffffffff, "yield": float(res["yield"][i]), "rows": rows})
        return solved

    def check_errors(self, clear=True):
        return self.batch.check_errors(clear)

    def close(self):
        if getattr(self, "batch", None) is not None:
            self.batch.close()
            self.batch = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _solve(tabs, worlds, plans, min_yields, backend, handle, device):
    """every plan's search: min_yields[i] is the request's min_yield_g"""
    if backend not in BACKENDS:
        raise ValueError("backend must be one of %s" % (BACKENDS,))
    if not plans:
        return []
    if backend == "host":
        return H.solve_plans_host(tabs, worlds, plans, min_yields)
    cache = {}

    def threshold(plan, m):      # a route compares the rounded yield (:1924), a one-pot candidate the unrounded (:2197)
        if plan["mode"] != H.MODE_VIRTUAL_POOL:
            return float(m)
        if m not in cache:
            cache[m] = H.yield_threshold(m)
        return cache[m]

    thresholds = [threshold(p, m) for p, m in zip(plans, min_yields)]
    own = handle is None
    if own:
        handle = ChemVerseOptimal(tabs, len(plans), device=device)
    try:
        return handle.solve(worlds, plans, thresholds)
    finally:
        if own:
            handle.close()


def _world_of(item, n_world):
    w = int(item.get("world", 0))
    if not 0 <= w < n_world:
        raise ValueError("world %d is outside [0, %d)" % (w, n_world))
    return w


def chain_costs(worlds, candidates, backend="device", handle=None, device="cuda:0", details=False):
    """candidates: dicts with world (index, default 0), target, chain (reaction ids or indices, forward order), min_yield_g,
    max_time_seconds (default 28800) and, optionally, conditions {step: (T_C, duration_s)} in place of the optimal ones
    -> _compute_chain_cost's result dict or None per candidate.  details=True: (results, solved) with every candidate's
    found, best_scale, decision bits and rows."""
    tabs = handle.tables if handle is not None else _tables(worlds)
    ws, plans, ms = [], [], []
    for cand in candidates:
        w = _world_of(cand, len(tabs))
        H._finite(min_yield_g=cand["min_yield_g"], max_time_seconds=cand.get("max_time_seconds", 28800.0))
        plans.append(H.chain_plan(tabs[w], cand["chain"], cand["target"], cand.get("conditions")))
        ws.append(w)
        ms.append(float(cand["min_yield_g"]))
    solved = _solve(tabs, ws, plans, ms, backend, handle, device)
    results = [H.chain_result(tabs[w], p, s, float(c.get("max_time_seconds", 28800.0)))
               for w, p, s, c in zip(ws, plans, solved, candidates)]
    return (results, solved) if details else results


def one_pot_costs(worlds, requests, backend="device", handle=None, device="cuda:0", details=False):
    """requests: dicts with world, target, min_yield_g, max_time_seconds -> _compute_one_pot_cost's dict or None each.
    details=True: (results, [(plans, solved) per request])"""
    tabs = handle.tables if handle is not None else _tables(worlds)
    ws, plans, ms, cut = [], [], [], [0]
    for req in requests:
        w = _world_of(req, len(tabs))
        max_time = float(req.get("max_time_seconds", 28800.0))
        H._finite(min_yield_g=req["min_yield_g"], max_time_seconds=max_time)
        ps = H.one_pot_plans(tabs[w], req["target"], max_time)
        plans += ps
        ws += [w] * len(ps)
        ms += [float(req["min_yield_g"])] * len(ps)
        cut.append(len(plans))
    solved = _solve(tabs, ws, plans, ms, backend, handle, device)
    parts = [(plans[cut[i]:cut[i + 1]], solved[cut[i]:cut[i + 1]]) for i in range(len(requests))]
    results = [H.one_pot_result(tabs[_world_of(req, len(tabs))], ps, ss) for req, (ps, ss) in zip(requests, parts)]
    return (results, parts) if details else results


def compute_optimal_costs(worlds, requests, backend="device", handle=None, device="cuda:0"):
    """requests: dicts of compute_optimal_cost's keyword arguments and `world` (index, default 0) -> the reference's dict
    each; on the device every candidate of every request — routes and one-pot charges — shares one set of launches"""
    tabs = handle.tables if handle is not None else _tables(worlds)
    planned, ws, plans, ms = [], [], [], []
    for req in requests:
        w = _world_of(req, len(tabs))
        pl = H.request_plans(tabs[w], req)
        mine = [p for _, p in pl["chains"]] + [p for _, ps in pl["one_pot"] for p in ps]
        planned.append((w, pl, len(plans), len(mine)))
        plans += mine
        ws += [w] * len(mine)
        ms += [float(pl["request"]["min_yield_g"])] * len(mine)
    solved = _solve(tabs, ws, plans, ms, backend, handle, device)
    out = []
    for w, pl, first, _ in planned:
        k = first + len(pl["chains"])
        chain_solved = solved[first:k]
        one_pot_solved = []
        for _, ps in pl["one_pot"]:
            one_pot_solved.append(solved[k:k + len(ps)])
            k += len(ps)
        out.append(H.request_result(tabs[w], pl, chain_solved, one_pot_solved))
    return out


def compute_optimal_cost(world, min_medicinal_value=3.0, max_toxicity=4.0, min_yield_g=1.0, max_time_seconds=28800.0,
                         required_phase=None, phase_temp_C=25.0, max_routes_per_target=5, max_steps=6, backend="device",
                         device="cuda:0"):
    """the reference's compute_optimal_cost (api.py:1777-1901) for one world"""
    return compute_optimal_costs([world], [dict(min_medicinal_value=min_medicinal_value, max_toxicity=max_toxicity,
                                                min_yield_g=min_yield_g, max_time_seconds=max_time_seconds,
                                                required_phase=required_phase, phase_temp_C=phase_temp_C,
                                                max_routes_per_target=max_routes_per_target, max_steps=max_steps)],
                                 backend=backend, device=device)[0]
