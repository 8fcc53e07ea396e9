"""ChemVerse on the device (csrc/chemverse.hip, C-ABI xv_chem_*): ChemVerseBatch runs the reference's simulate_chain_reaction for
many experiments, each under its own world, in one launch."""
import ctypes as C

import numpy as np

from .. import _lib
from . import tables as T
from .host import HISTORY, LOG, SCALARS

LANES = 64
RECORD = ("none", "history", "log")


def prepare_experiments(tabs, world_index, amounts, temperature_C, pressure_atm, duration_s, equipment,
                        heating_rate_C_per_s=0.0, vessel_volume_L=1.0, step_seconds=5.0):
    """the arguments of ChemVerseBatch.simulate, checked, as host arrays: dict(n, world int32[n], grams float64[n, cs], order
    int32[n, cs], n_initial, T, P, duration, equipment, rate, volume, num_steps).  Refuses what the kernel would only clamp:
    indices out of range, non-finite inputs, more than STEPS_MAX steps."""
    cs = max(t["C"] for t in tabs)
    if isinstance(amounts, (list, tuple)) and len(amounts) and isinstance(amounts[0], dict):
        n = len(amounts)
    else:
        amounts = np.asarray(amounts.detach().cpu().numpy() if hasattr(amounts, "detach") else amounts, np.float64)
        if amounts.ndim != 2:
            raise ValueError("amounts must be [n, C] or a list of dicts")
        n = amounts.shape[0]
    if n < 1:
        raise ValueError("simulate needs at least one experiment")

    def vec(x, dtype, name):
        a = np.asarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x)
        a = np.broadcast_to(a.astype(dtype), (n,)).copy() if a.ndim == 0 else np.ascontiguousarray(a, dtype)
        if a.shape != (n,):
            raise ValueError("%s must be a scalar or have shape (%d,), got %s" % (name, n, a.shape))
        if dtype == np.float64 and not np.isfinite(a).all():
            raise ValueError("%s must be finite" % name)
        return a

    world = vec(world_index, np.int32, "world_index")
    if world.min() < 0 or world.max() >= len(tabs):
        raise ValueError("world_index must be in [0, %d)" % len(tabs))
    if isinstance(equipment, str) or equipment is None:
        equipment = [equipment] * n
    eq = np.asarray(equipment)
    if eq.dtype.kind in "iu":
        eq = vec(eq, np.int32, "equipment")
        for i in range(n):
            T.equipment_index(tabs[world[i]], int(eq[i]))
    else:
        if len(equipment) != n:
            raise ValueError("equipment must name one entry per experiment")
        eq = np.array([T.equipment_index(tabs[world[i]], equipment[i]) for i in range(n)], np.int32)
    out = dict(n=n, world=world, equipment=eq, T=vec(temperature_C, np.float64, "temperature_C"),
               P=vec(pressure_atm, np.float64, "pressure_atm"), duration=vec(duration_s, np.float64, "duration_s"),
               rate=vec(heating_rate_C_per_s, np.float64, "heating_rate_C_per_s"),
               volume=vec(vessel_volume_L, np.float64, "vessel_volume_L"))
    step_seconds = float(step_seconds)
    out["num_steps"] = np.array([T.num_steps_of(d, step_seconds) for d in out["duration"]], np.int32)
    grams, order, n_init = np.zeros((n, cs)), np.zeros((n, cs), np.int32), np.zeros(n, np.int32)
    if isinstance(amounts, np.ndarray):
        if amounts.shape[1] > cs or not np.isfinite(amounts).all():
            raise ValueError("amounts must be finite and at most %d wide" % cs)
        for i in range(n):
            if (amounts[i, tabs[world[i]]["C"]:] != 0).any():
                raise ValueError("experiment %d has amounts beyond its world's %d chemicals" % (i, tabs[world[i]]["C"]))
            idx = np.nonzero(amounts[i] > 1e-9)[0]
            order[i, :len(idx)], n_init[i] = idx, len(idx)
        grams[:, :amounts.shape[1]] = amounts
    else:
        for i, a in enumerate(amounts):
            ids = tabs[world[i]]["chem_ids"]
            pos = tabs[world[i]].get("_chem_pos")
            if pos is None:
                pos = tabs[world[i]]["_chem_pos"] = {c: k for k, c in enumerate(ids)}
            for j, (cid, g) in enumerate(a.items()):
                c = cid if isinstance(cid, (int, np.integer)) else pos.get(cid)
                if c is None or not 0 <= c < len(ids):
                    raise ValueError("experiment %d: %r is not a chemical of its world" % (i, cid))
                if not np.isfinite(g):
                    raise ValueError("experiment %d: the amount of %r is not finite" % (i, cid))
                grams[i, c], order[i, j] = g, c
            n_init[i] = len(a)
    out.update(grams=grams, order=order, n_initial=n_init, step_seconds=step_seconds)
    return out


def group_by_world(world, num_steps):
    """-> (slot_of int64[n], exp_of int32[n_pad]): the experiments sorted by (world, steps) — fewer divergent lanes — and cut
    into workgroups of 64 of ONE world, the last one of a world padded with -1"""
    perm = np.lexsort((num_steps, world))
    slot_of = np.zeros(len(world), np.int64)
    exp_of = []
    i = 0
    while i < len(perm):
        j = i
        while j < len(perm) and world[perm[j]] == world[perm[i]]:
            j += 1
        slot_of[perm[i:j]] = len(exp_of) + np.arange(j - i)
        exp_of.extend(perm[i:j].tolist())
        exp_of.extend([-1] * (-(j - i) % LANES))
        i = j
    return slot_of, np.array(exp_of, np.int64)


class ChemVerseBatch(object):
    """worlds: the reference's World objects, their to_dict() / JSON form, or tables of build_tables; capacity: the most
    experiments one simulate() takes.  The call is a pure function of its arguments: no random draws, no tick."""

    def __init__(self, worlds, capacity, engine=None, device="cuda:0"):
        from ..engine import Engine
        if int(capacity) < 1:
            raise ValueError("capacity must be at least 1")
        self.capacity = int(capacity)
        self._h = None
        self._dev = None
        self._own_engine = engine is None
        self.engine = engine if engine is not None else Engine(device)
        self.lib, self.device = self.engine.lib, self.engine.device
        h = C.c_void_p()
        _lib.check(self.lib.xv_chem_create(self.engine.handle, self.capacity, C.byref(h)))
        self._h = h
        self.time_kernel = False      # True: simulate() brackets the launch with the engine's timing events
        self.last_kernel_ms = None    # -> the launch's milliseconds (scripts/bench_chemverse.py)
        self.set_worlds(worlds)

    def set_worlds(self, worlds):
        import torch
        if isinstance(worlds, dict) or hasattr(worlds, "chemicals"):
            worlds = [worlds]
        if not len(worlds):
            raise ValueError("set_worlds needs at least one world")
        tabs = [T.build_tables(w) for w in worlds]
        p = T.pack_worlds(tabs)
        keys = ("world_off", "chem_f", "sol_present", "sol_value", "rxn_i", "rxn_f", "rxn_solv", "eq_i", "eq_f")
        dev = [torch.from_numpy(np.ascontiguousarray(p[k])).to(self.device) for k in keys]
        self.engine.sync()      # the tables a running call reads are let go below
        _lib.check(self.lib.xv_chem_set_worlds(self._h, p["n_world"], p["c_stride"], p["r_stride"], *(_lib.ptr(t) for t in dev)))
        self._dev = dev         # borrowed by the handle
        self.tables, self.c_stride, self.r_stride = tabs, p["c_stride"], p["r_stride"]

    def simulate(self, world_index, amounts, temperature_C, pressure_atm, duration_s, equipment, heating_rate_C_per_s=0.0,
                 vessel_volume_L=1.0, step_seconds=5.0, record="none"):
        """-> dict of device tensors named as xv_chem_simulate's outputs (include/xeno.h), one row per experiment in the
        caller's order.  record: "none", "history" (+ hist_*) or "log" (+ hist_* and log_*)."""
        import torch
        if record not in RECORD:
            raise ValueError("record must be one of %s" % (RECORD,))
        x = prepare_experiments(self.tables, world_index, amounts, temperature_C, pressure_atm, duration_s, equipment,
                                heating_rate_C_per_s, vessel_volume_L, step_seconds)
        n = x["n"]
        if n > self.capacity:
            raise ValueError("%d experiments are more than this batch's capacity %d" % (n, self.capacity))
        slot_of, exp_of = group_by_world(x["world"], x["num_steps"])
        n_pad, live = len(exp_of), exp_of >= 0
        src = np.where(live, exp_of, 0)

        def padded(a, fill=0):
            b = a[src].copy()
            b[~live] = fill
            return torch.from_numpy(np.ascontiguousarray(b)).to(self.device)

        ins = [padded(x["world"], -1), padded(x["grams"]), padded(x["order"]), padded(x["n_initial"]), padded(x["T"], 25.0),
               padded(x["P"], 1.0), padded(x["duration"], 1.0), padded(x["equipment"]), padded(x["rate"]), padded(x["volume"], 1.0)]
        cs, rs = self.c_stride, self.r_stride
        f64, i32, u8 = torch.float64, torch.int32, torch.uint8
        shapes = dict(final_pool=((cs,), f64), consumed=((cs,), f64), produced=((cs,), f64), byproduct=((cs,), f64),
                      gas_lost=((cs,), f64), fired=((rs,), i32))
        shapes.update((k, ((), {np.int32: i32, np.uint8: u8, np.float64: f64}[dt])) for k, dt in SCALARS)
        shapes.update(hist_step=((30,), i32), hist_T=((30,), f64), hist_P=((30,), f64), log_step=((20,), i32),
                      log_active=((20,), i32), log_T=((20,), f64), log_P=((20,), f64), log_consumed=((20, cs), f64),
                      log_produced=((20, cs), f64))
        want = [k for k in _lib.ChemOut.FIELDS
                if not (k in HISTORY and record == "none") and not (k in LOG and record != "log")]
        # zeros, not empty: the rows of padding lanes are never written
        raw = dict((k, torch.zeros((n_pad,) + shapes[k][0], dtype=shapes[k][1], device=self.device)) for k in want)
        out = _lib.ChemOut(**dict((k, _lib.ptr(raw[k])) for k in want))
        if self.time_kernel:
            self.engine.event_record(0)
        _lib.check(self.lib.xv_chem_simulate(self._h, n_pad, *(_lib.ptr(t) for t in ins), float(x["step_seconds"]),
                                             C.byref(out)))
        if self.time_kernel:
            self.engine.event_record(1)
        back = torch.from_numpy(slot_of).to(self.device)
        res = dict((k, raw[k].index_select(0, back)) for k in want)
        self.engine.sync()      # the padded inputs must outlive the launch
        if self.time_kernel:
            self.last_kernel_ms = self.engine.event_elapsed_ms()
        return res

    def check_errors(self, clear=True):
        """the engine's sticky device error word (0: none)"""
        return self.engine.error_flags(clear)

    def close(self):
        if getattr(self, "_h", None) is not None:
            self.lib.xv_chem_destroy(self._h)
            self._h = None
            self._dev = None
        if getattr(self, "engine", None) is not None and self._own_engine:
            self.engine.close()
        self.engine = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
