"""Throughput task sampling on the GPU: `sample_tasks_device` returns n accepted AnyMDP tasks as device tables that
`AnyMDPVecEnv.set_task` takes as they are (no host round trip), generated, repaired and accepted by
`xv_anymdp_sample_tasks` (csrc/anymdp_sampler.hip), one workgroup per candidate.

Same generative model and acceptance test as the reference's AnyMDPTaskSampler (xenoverse/anymdp/task_sampler.py:15-65,
task_sampler_utils.py:65-256, solver.py:84-148) with counter-based randomness: task k of (seed, state_space,
action_space) is the k-th ACCEPTED candidate in candidate order — a pure function of those arguments, independent of
the batch size used to find it — but not the task NumPy's stream would give for that seed (for that, the host sampler
`AnyMDPTaskSampler(seed=...)`).  Supported sizes: 8 <= state_space <= 64 with state_space * action_space <= 512 (a
candidate's transition tensor lives in registers) and, round 4, state_space <= 256 with state_space * action_space <= 4096
(rows in a transposed global scratch: the defaults of the reference's Garnet (128) and multi-token (256) samplers).

The reference's other two task makers are here as well (csrc/anymdp_garnet.hip; numpy restatement sampler_host_garnet.py):
`sample_garnet_tasks_device` (GarnetTaskSampler: every index is a task, up to 512 states) and `sample_bandit_tasks_device`
(the single-state task, which `sample_tasks_device(..., state_space=1)` delegates to).
"""
import ctypes as C
import time

import numpy as np
import torch

from .. import _lib
from ..device_sampling import collect_accepted, engine_scope, sampler_stats
from .tables import row_lines

STATUS = ("accepted", "unrepairable", "value_gap", "occupancy", "no_convergence")

INFO_DTYPE = np.dtype([("status", "<i4"), ("goal", "<i4"), ("n_s0", "<i4"), ("repair_rounds", "<i4"), ("s0", "<i4", 4),
                       ("sweeps", "<i4", 8), ("band_lo", "<i4", 256), ("band_hi", "<i4", 256), ("state_map", "<i4", 256),
                       ("s_e", "u1", 256), ("max_steps", "<f8"), ("gini", "<f8"), ("ent", "<f8"), ("gap_min", "<f8"),
                       ("s0_prob", "<f8", 4)], align=True)     # xv_anymdp_cand_info (include/xeno.h)


def sample_candidates(engine, seed, cand_base, n_cand, S, A, s0_max=4, tables=True, dense=False, info=False):
    """One launch over candidates [cand_base, cand_base + n_cand).  -> dict with `status` int32[n_cand] (device) and,
    as requested, the table slots (written where status == 0), dense fp64 tensors and the per-candidate info records."""
    d = engine.device
    out = {"status": torch.empty(n_cand, dtype=torch.int32, device=d)}
    if tables:
        out.update(rows=torch.empty((n_cand, S, A, row_lines(S), 16), dtype=torch.float64, device=d),
                   state_map=torch.empty((n_cand, S), dtype=torch.int32, device=d),
                   term_mask=torch.empty((n_cand, (S + 63) // 64), dtype=torch.int64, device=d),
                   s0_cdf=torch.empty((n_cand, s0_max), dtype=torch.float64, device=d),
                   s0_ids=torch.empty((n_cand, s0_max), dtype=torch.int32, device=d),
                   max_steps=torch.empty(n_cand, dtype=torch.int32, device=d))
    if dense:
        for k in ("transition", "reward", "reward_noise"):
            out[k] = torch.empty((n_cand, S, A, S), dtype=torch.float64, device=d)
    if info:
        out["info_raw"] = torch.zeros((n_cand, INFO_DTYPE.itemsize), dtype=torch.uint8, device=d)
    p = lambda k: _lib.ptr(out.get(k))
    _lib.check(engine.lib.xv_anymdp_sample_tasks(
        engine.handle, int(seed) & (2**64 - 1), int(cand_base), int(n_cand), S, A, s0_max, p("rows"), p("state_map"),
        p("term_mask"), p("s0_cdf"), p("s0_ids"), p("max_steps"), p("transition"), p("reward"), p("reward_noise"),
        p("info_raw"), p("status")))
    if info:
        engine.sync()
        out["info"] = out.pop("info_raw").cpu().numpy().view(INFO_DTYPE).reshape(n_cand)
    return out


def sample_observation_model_device(engine, seed, n_tasks, state_space, observation_space=64, observation_tokens=1,
                                    density=0.20, maximum_distribution=4, task_base=0):
    """Observation models of AnyPOMDPTaskSampler / MultiTokensAnyPOMDPTaskSampler (task_sampler.py:78-87, :103-117) for
    n_tasks tasks on the device -> obs_cdf float64[n_tasks, observation_tokens, state_space, observation_space] (device):
    sparse random rows (exactly round(density * S * n_obs) cells per matrix), empty rows fixed, normalised, as CDFs."""
    out = torch.empty((n_tasks, observation_tokens, state_space, observation_space), dtype=torch.float64, device=engine.device)
    _lib.check(engine.lib.xv_anymdp_sample_observation_model(
        engine.handle, int(seed) & (2**64 - 1), int(task_base), int(n_tasks), int(state_space), int(observation_space),
        int(observation_tokens), float(density), float(maximum_distribution), _lib.ptr(out)))
    return out


def launch_batch(S, A, dense=False):
    """candidates per launch that memory allows (6 GiB of outputs and scratch), 8192 at the most"""
    per = S * A * row_lines(S) * 128 + (3 * S * A * S * 8 if dense else 0)
    if S > 64 or S * A > 512:      # the candidate's scratch: transposed transition rows + two S x S matrices
        per += ((S * A + 63) // 64 * 64 * S + 2 * S * S) * 8
    return int(min(8192, (6 << 30) // per))


def sample_tasks_device(n_tasks, state_space=64, action_space=5, seed=0, device="cuda:0", engine=None, batch=None,
                        s0_max=4, dense=False, max_candidates=None, task_type="MDP", observation_space=64,
                        observation_tokens=4, action_tokens=2, density=0.20, maximum_distribution=4):
    """n_tasks accepted tasks -> dict of device tensors (keys as anymdp.tables.build_tables: S, A, s0_max, rows,
    state_map, term_mask, s0_cdf, s0_ids, max_steps; with dense=True also transition / reward / reward_noise fp64 and
    max_steps_real) + "stats" (candidates tried, status histogram, seconds).
    state_space = 1, the multi-armed bandit, is `sample_bandit_tasks_device` (task_type "MDP" only).
    task_type "POMDP" / "MTPOMDP" (the reference's AnyPOMDPTaskSampler / MultiTokensAnyPOMDPTaskSampler, whose arguments
    observation_space, observation_tokens, action_tokens, density, maximum_distribution are taken as they are) adds the
    observation model of every task, sampled on the device too: obs_cdf, n_obs, d_obs, d_act, task_type — the dict
    `AnyMDPVecEnv.set_task` takes as it is."""
    if task_type not in ("MDP", "POMDP", "MTPOMDP"):
        raise NotImplementedError(f"Unknown task type: {task_type}")
    S, A = int(state_space), int(action_space)
    if S == 1:      # the multi-armed bandit (task_sampler.py:30-31, task_sampler_utils.py:258-272)
        if task_type != "MDP":
            raise ValueError("state_space = 1 (the multi-armed bandit) has no %s form: the reference's observation model needs "
                             "at least 8 states; use task_type=\"MDP\"" % task_type)
        return sample_bandit_tasks_device(n_tasks, A, seed=seed, device=device, engine=engine, batch=batch, s0_max=s0_max,
                                          dense=dense, max_candidates=max_candidates)
    if batch is None:
        batch = max(64, min(launch_batch(S, A, dense), 4 * n_tasks + 64))
    keys = ["rows", "state_map", "term_mask", "s0_cdf", "s0_ids", "max_steps"] + \
        (["transition", "reward", "reward_noise"] if dense else [])
    with engine_scope(engine, device) as eng:
        t0 = time.perf_counter()
        # (no info records: one is ~4 KB per candidate; the status comes back as one int32 per candidate)
        got, _, hist = collect_accepted(
            lambda base, n: sample_candidates(eng, seed, base, n, S, A, s0_max, tables=True, dense=dense),
            n_tasks, batch, keys, STATUS, max_candidates)
        out = dict(S=S, A=A, s0_max=s0_max, **got)
        if task_type != "MDP":
            d_obs, d_act = (int(observation_tokens), int(action_tokens)) if task_type == "MTPOMDP" else (1, 1)
            out.update(task_type=task_type, n_obs=int(observation_space), d_obs=d_obs, d_act=d_act,
                       obs_cdf=sample_observation_model_device(eng, seed, n_tasks, S, observation_space, d_obs, density,
                                                               maximum_distribution))
        eng.sync()
        out["stats"] = sampler_stats(hist, STATUS, batch, t0)
        return out


def task_dict_from_dense(transition, reward, reward_noise, info_row, S, A):
    """one candidate's dense tensors + info record -> the reference's task dict"""
    n0 = int(info_row["n_s0"])
    return dict(ns=S, na=A, max_steps=float(info_row["max_steps"]), state_mapping=np.array(info_row["state_map"][:S], np.int64),
                task_type="MDP", s_0=np.array(info_row["s0"][:n0], np.int64), s_0_prob=np.array(info_row["s0_prob"][:n0]),
                s_e=np.nonzero(info_row["s_e"][:S])[0].astype(np.int64), transition=np.asarray(transition, np.float64),
                reward=np.asarray(reward, np.float64), reward_noise=np.asarray(reward_noise, np.float64),
                final_goal_terminate=bool(info_row["goal"]))


# ---- Garnet and bandit tasks (csrc/anymdp_garnet.hip; the model: sampler_host_garnet.py) ------------------

GARNET_STATUS = ("accepted",)


def _table_slots(d, n, S, A, s0_max):
    return dict(rows=torch.empty((n, S, A, row_lines(S), 16), dtype=torch.float64, device=d),
                state_map=torch.empty((n, S), dtype=torch.int32, device=d),
                term_mask=torch.empty((n, (S + 63) // 64), dtype=torch.int64, device=d),
                s0_cdf=torch.empty((n, s0_max), dtype=torch.float64, device=d),
                s0_ids=torch.empty((n, s0_max), dtype=torch.int32, device=d),
                max_steps=torch.empty(n, dtype=torch.int32, device=d))


def sample_garnet_tasks_device(n_tasks, state_space=128, action_space=5, min_state_space=None, b=2, sigma=0.1, seed=0,
                               device="cuda:0", engine=None, batch=None, s0_max=4, dense=False):
    """n_tasks Garnet tasks (the reference's GarnetTaskSampler, its arguments taken as they are) -> the table dict of
    sample_tasks_device (S, A, s0_max, rows, state_map, term_mask, s0_cdf, s0_ids, max_steps; with dense=True also transition /
    reward / reward_noise fp64 [n, S, A, S], zero outside a task's real states) + n_real int32[n] (the real state counts:
    with min_state_space they differ, and states past a task's count are padded as build_tables pads them), obs_space and
    "stats".  Every index is a task; task k is the same bits whatever `batch` (tasks per launch; default: what 6 GiB take).
    `AnyMDPVecEnv.set_task(tables)` takes the result as it is; `task_dicts_from_device` turns a dense one into the
    reference's dicts.  Limits: sampler_host_garnet.check_garnet_args (ValueError naming the limit)."""
    from . import sampler_host_garnet as sh
    n_tasks = int(n_tasks)
    if n_tasks < 1:
        raise ValueError("n_tasks must be at least 1")
    if int(s0_max) < 1:
        raise ValueError("s0_max smaller than the longest s_0 list")
    S, A, _ = sh.check_garnet_args(state_space, action_space, min_state_space, b)
    if batch is None:
        per = S * A * row_lines(S) * 128 + (3 * S * A * S * 8 if dense else 0)
        batch = int(max(1, min(n_tasks, (6 << 30) // per)))
    batch = int(batch)
    if batch < 1:
        raise ValueError("batch must be at least 1")
    seed64 = int(seed) & (2**64 - 1)
    with engine_scope(engine, device) as eng:
        t0 = time.perf_counter()
        d = eng.device
        out = _table_slots(d, n_tasks, S, A, int(s0_max))
        out["n_real"] = torch.empty(n_tasks, dtype=torch.int32, device=d)
        if dense:
            for k in ("transition", "reward", "reward_noise"):
                out[k] = torch.empty((n_tasks, S, A, S), dtype=torch.float64, device=d)
        for lo in range(0, n_tasks, batch):
            hi = min(lo + batch, n_tasks)
            p = lambda k: _lib.ptr(out[k][lo:hi]) if k in out else None
            _lib.check(eng.lib.xv_anymdp_sample_garnet(
                eng.handle, seed64, lo, hi - lo, S, A, 0 if min_state_space is None else int(min_state_space), int(b),
                float(sigma), int(s0_max), p("rows"), p("state_map"), p("term_mask"), p("s0_cdf"), p("s0_ids"), p("max_steps"),
                p("n_real"), p("transition"), p("reward"), p("reward_noise")))
        eng.sync()
        out.update(S=S, A=A, s0_max=int(s0_max), obs_space=np.full(n_tasks, S, np.int32), sampler="garnet")
        out["stats"] = sampler_stats(np.array([n_tasks], np.int64), GARNET_STATUS, batch, t0)
        return out


def sample_bandit_candidates(engine, seed, cand_base, n_cand, A, max_rounds=1024, s0_max=4, tables=True, dense=False):
    """One launch over bandit candidates [cand_base, cand_base + n_cand).  -> dict with `status` int32[n_cand] (device) and,
    as requested, the table slots at S = 2 and the dense reward / reward_noise fp64 [n_cand, 1, A, 1] (written where
    status == 0)"""
    d = engine.device
    out = {"status": torch.empty(n_cand, dtype=torch.int32, device=d)}
    if tables:
        out.update(_table_slots(d, n_cand, 2, A, s0_max))
    if dense:
        for k in ("reward", "reward_noise"):
            out[k] = torch.empty((n_cand, 1, A, 1), dtype=torch.float64, device=d)
    p = lambda k: _lib.ptr(out.get(k))
    _lib.check(engine.lib.xv_anymdp_sample_bandits(
        engine.handle, int(seed) & (2**64 - 1), int(cand_base), int(n_cand), int(A), int(max_rounds), int(s0_max), p("rows"),
        p("state_map"), p("term_mask"), p("s0_cdf"), p("s0_ids"), p("max_steps"), p("reward"), p("reward_noise"), p("status")))
    return out


def sample_bandit_tasks_device(n_tasks, action_space=5, seed=0, max_rounds=1024, device="cuda:0", engine=None, batch=None,
                               s0_max=4, dense=False, max_candidates=None):
    """n_tasks multi-armed bandits (the reference's AnyMDPTaskSampler(state_space=1)) -> the table dict of
    sample_tasks_device at S = 2, build_tables' embedding of a single-state task in two inner states (with dense=True also
    transition (ones) / reward / reward_noise fp64 [n, 1, A, 1]) + n_real (ones), obs_space (ones) and "stats".  Task k is
    the k-th candidate with a round of std(reward) > 0.01 within max_rounds, whatever `batch` (candidates per launch); the
    others have status "no_spread" and are skipped (the reference draws rounds without bound)."""
    from . import sampler_host_garnet as sh
    n_tasks = int(n_tasks)
    if n_tasks < 1:
        raise ValueError("n_tasks must be at least 1")
    if int(s0_max) < 1:
        raise ValueError("s0_max smaller than the longest s_0 list")
    A, R = sh.check_bandit_args(action_space, max_rounds)
    batch = int(max(64, min(1 << 20, n_tasks + n_tasks // 8 + 64))) if batch is None else int(batch)
    if batch < 1:
        raise ValueError("batch must be at least 1")
    keys = ["rows", "state_map", "term_mask", "s0_cdf", "s0_ids", "max_steps"] + (["reward", "reward_noise"] if dense else [])
    with engine_scope(engine, device) as eng:
        t0 = time.perf_counter()
        got, _, hist = collect_accepted(
            lambda base, n: sample_bandit_candidates(eng, seed, base, n, A, R, int(s0_max), tables=True, dense=dense),
            n_tasks, batch, keys, sh.BANDIT_STATUS, max_candidates)
        out = dict(S=2, A=A, s0_max=int(s0_max), **got)
        if dense:
            out["transition"] = torch.ones((n_tasks, 1, A, 1), dtype=torch.float64, device=eng.device)
        out.update(n_real=torch.ones(n_tasks, dtype=torch.int32, device=eng.device), obs_space=np.ones(n_tasks, np.int32),
                   sampler="bandit")
        eng.sync()
        out["stats"] = sampler_stats(hist, sh.BANDIT_STATUS, batch, t0)
        return out


def task_dicts_from_device(tables, index=None):
    """the tasks of a Garnet or bandit tables dict made with dense=True (all, or those of `index`) -> the reference's task
    dicts of numpy arrays, ragged tasks sliced to their real state count: what pickles, and what
    set_task takes as a list.  max_steps is the integer the tables hold, ceil of the real draw: `steps >= max_steps` on
    integer steps is the same test."""
    if not (isinstance(tables, dict) and tables.get("sampler") in ("garnet", "bandit")):
        raise ValueError("task_dicts_from_device needs the dict sample_garnet_tasks_device / sample_bandit_tasks_device returns")
    if any(tables.get(k) is None for k in ("transition", "reward", "reward_noise")):
        raise ValueError("task_dicts_from_device needs the dense tensors: sample with dense=True")
    host = {k: tables[k].detach().cpu().numpy() for k in ("transition", "reward", "reward_noise", "state_map", "max_steps",
                                                           "n_real")}
    bandit = tables["sampler"] == "bandit"
    index = range(len(host["n_real"])) if index is None else [int(i) for i in np.asarray(index).reshape(-1)]
    out = []
    for i in index:
        n = int(host["n_real"][i])
        task = {"ns": 1 if bandit else int(tables["S"]), "na": int(tables["A"]), "max_steps": float(host["max_steps"][i]),
                "state_mapping": host["state_map"][i, :n].astype(np.int64), "task_type": "MDP", "s_0": np.array([0]),
                "s_0_prob": np.array([1.0]), "s_e": np.array([], dtype=int), "final_goal_terminate": False}
        for k in ("transition", "reward", "reward_noise"):
            task[k] = np.array(host[k][i, :n, :, :n])
        out.append(task)
    return out
