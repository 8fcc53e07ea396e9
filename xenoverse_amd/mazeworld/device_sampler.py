"""MazeWorld task sampling on the GPU: `sample_tasks_device` returns n accepted tasks as the device tables
`MazeWorldVecEnv.set_task` takes as they are, made by `xv_maze_sample_tasks` (csrc/maze_sampler.hip), one wave per
candidate; `resample_tasks_device` is the reference's Resampler over such tables (`xv_maze_resample_tasks`).

Same generative model as the reference's MazeTaskManager.sample_task / resample_task (mazeworld/envs/task_sampler.py:92-225,
utils/grid_ops.py:49-162) with counter-based randomness: task k of (seed, arguments) is the k-th ACCEPTED candidate in
candidate order, a pure function of those arguments whatever the batch size — but not the task NumPy's stream gives for
that seed (for that, the host sampler `MazeTaskSampler(seed=...)`).  Departures: integers are
floor(u * m), the wall release runs at most 4 (n-2)^2 passes (`pass_cap`), and a candidate with fewer open cells than
landmarks + 1 is dropped (`no_room`).  The numpy restatement the device is tested against is mazeworld/sampler_host.py.
"""
import ctypes as C
import time

import numpy as np
import torch

from .. import _lib
from ..device_sampling import collect_accepted, engine_scope, sampler_stats
from . import sampler_host as sh
from .tables import LMAX

STATUS = sh.STATUS
INFO_DTYPE = sh.INFO_DTYPE
SLOT_KEYS = ("walls", "texts", "landmarks", "ints", "dbl", "commands", "lm_coord")
RESAMPLE_CMD, RESAMPLE_START, RESAMPLE_LANDMARKS, RESAMPLE_COLOR = 1, 2, 4, 8


class _Params(C.Structure):   # xv_maze_sampler_params (include/xeno.h)
    _fields_ = [(k, C.c_int32) for k in ("n_lo", "n_hi", "allow_loops", "landmarks_lo", "landmarks_hi", "n_cmd",
                                         "n_wall_textures", "n_ground_textures", "n_ceiling_textures",
                                         "has_goal_reward")] + \
               [(k, C.c_double * 2) for k in ("cell_size", "wall_height", "agent_height", "wall_density", "fol_angle")] + \
               [(k, C.c_double) for k in ("step_reward", "collision_reward", "goal_reward")]


class _Slots(C.Structure):   # xv_maze_task_slots
    _fields_ = [(k, C.c_void_p) for k in SLOT_KEYS]


def _params(a):
    p = _Params()
    p.n_lo, p.n_hi = int(a["n_range"][0]), int(a["n_range"][1])
    p.allow_loops = 1 if a["allow_loops"] else 0
    p.landmarks_lo, p.landmarks_hi = int(a["landmarks_number_range"][0]), int(a["landmarks_number_range"][1])
    p.n_cmd = int(a["commands_sequence"])
    p.n_wall_textures, p.n_ground_textures, p.n_ceiling_textures = (a["n_wall_textures"], a["n_ground_textures"],
                                                                    a["n_ceiling_textures"])
    p.has_goal_reward = 0 if a["goal_reward"] is None else 1
    for k in ("cell_size", "wall_height", "agent_height", "wall_density", "fol_angle"):
        getattr(p, k)[0], getattr(p, k)[1] = float(a[k + "_range"][0]), float(a[k + "_range"][1])
    p.step_reward, p.collision_reward = float(a["step_reward"]), float(a["collision_reward"])
    p.goal_reward = 0.0 if a["goal_reward"] is None else float(a["goal_reward"])
    return p


def _slot_tensors(n, NG, n_cmd, device):
    return dict(walls=torch.empty((n, NG, NG), dtype=torch.int8, device=device),
                texts=torch.empty((n, NG, NG), dtype=torch.int32, device=device),
                landmarks=torch.empty((n, NG, NG), dtype=torch.int8, device=device),
                ints=torch.empty((n, 8), dtype=torch.int32, device=device),
                dbl=torch.empty((n, 8), dtype=torch.float64, device=device),
                commands=torch.empty((n, n_cmd), dtype=torch.int32, device=device),
                lm_coord=torch.empty((n, LMAX, 2), dtype=torch.int32, device=device))


def _fill_tan(dbl):
    """dbl[:, 7] = numpy.tan(fol_angle / 2) on the host, as build_tables has it: the ray caster's bytes depend on it"""
    t = np.array([np.tan(float(f) / 2) for f in dbl[:, 3].cpu().numpy()], np.float64)      # build_tables' expression
    dbl[:, 7] = torch.from_numpy(t).to(dbl.device)


def sample_candidates(engine, seed, cand_base, n_cand, info=False, **sampler_kwargs):
    """One launch over candidates [cand_base, cand_base + n_cand).  -> dict with NG, n_cmd, the seven table slots
    ([n_cand]-leading device tensors; all padding where status != 0), `status` int32[n_cand] (device) and, with info, the
    per-candidate records (status, n, rooms, passes, idle, released) on the host.  Keyword arguments: MazeTaskSampler's."""
    a = sh.sampler_arguments(**sampler_kwargs)
    d = engine.device
    NG, n_cmd = sh.grid_pitch(a["n_range"]), int(a["commands_sequence"])
    out = dict(NG=NG, n_cmd=n_cmd, **_slot_tensors(n_cand, NG, n_cmd, d))
    out["status"] = torch.empty(n_cand, dtype=torch.int32, device=d)
    raw = torch.zeros((n_cand, INFO_DTYPE.itemsize), dtype=torch.uint8, device=d) if info else None
    p, slots = _params(a), _Slots(*[_lib.ptr(out[k]) for k in SLOT_KEYS])
    _lib.check(engine.lib.xv_maze_sample_tasks(engine.handle, int(seed) & (2**64 - 1), int(cand_base), int(n_cand), NG,
                                               C.cast(C.byref(p), C.c_void_p), C.cast(C.byref(slots), C.c_void_p),
                                               _lib.ptr(raw), _lib.ptr(out["status"])))
    engine.sync()
    _fill_tan(out["dbl"])
    if info:
        out["info"] = raw.cpu().numpy().view(INFO_DTYPE).reshape(n_cand)
    return out


def sample_tasks_device(n_tasks, seed=0, engine=None, device="cuda:0", batch=None, max_candidates=None, **sampler_kwargs):
    """n_tasks accepted tasks -> the tables dict of mazeworld.tables.build_tables with device tensors (NG, n_cmd, walls,
    texts, landmarks, ints, dbl, commands, lm_coord) + `info` (host records) and `stats`: candidates tried, status
    histogram, seconds.  Task k is the k-th accepted candidate in candidate order, whatever `batch` is.
    `MazeWorldVecEnv.set_task(tables)` takes the result as it is.  Keyword arguments: MazeTaskSampler's."""
    if batch is None:
        batch = int(max(64, min(4096, n_tasks)))
    a = sh.sampler_arguments(**sampler_kwargs)
    with engine_scope(engine, device) as eng:
        t0 = time.perf_counter()
        got, info, hist = collect_accepted(
            lambda base, n: sample_candidates(eng, seed, base, n, info=True, **sampler_kwargs),
            n_tasks, batch, SLOT_KEYS, STATUS, max_candidates)
        out = dict(NG=sh.grid_pitch(a["n_range"]), n_cmd=int(a["commands_sequence"]), **got)      # as sample_candidates has them
        out["info"] = info
        eng.sync()
        out["stats"] = sampler_stats(hist, STATUS, batch, t0)
        return out


def resample_tasks_device(tables, seed=0, episode=0, resample_cmd=True, resample_start=True, resample_landmarks=False,
                          resample_landmarks_color=False, engine=None, index_base=0):
    """The reference's Resampler over device tables: -> a new tables dict whose landmarks, lm_coord, ints and commands are
    new tensors and whose other entries are the given ones.  Draws are a function of (seed, index_base + task, episode)."""
    w = tables["walls"]
    if not torch.is_tensor(w) or not w.is_cuda:
        raise ValueError("resample_tasks_device takes tables whose entries are device tensors")
    n_task, NG, n_cmd = int(w.shape[0]), int(tables["NG"]), int(tables["n_cmd"])
    shapes = dict(walls=(n_task, NG, NG), landmarks=(n_task, NG, NG), ints=(n_task, 8), commands=(n_task, n_cmd),
                  lm_coord=(n_task, LMAX, 2))
    dtypes = dict(walls=torch.int8, landmarks=torch.int8, ints=torch.int32, commands=torch.int32, lm_coord=torch.int32)
    for k, shape in shapes.items():      # the kernel addresses the tables by these pitches
        if tuple(tables[k].shape) != shape or tables[k].dtype != dtypes[k] or tables[k].device != w.device:
            raise ValueError("table %r must be %s%s on %s" % (k, dtypes[k], list(shape), w.device))
    with engine_scope(engine, str(w.device)) as eng:
        new = dict(tables)
        for k in ("landmarks", "lm_coord", "ints", "commands"):
            new[k] = tables[k].contiguous().clone()
        new["walls"] = w.contiguous()
        flags = (RESAMPLE_CMD if resample_cmd else 0) | (RESAMPLE_START if resample_start else 0) | \
                (RESAMPLE_LANDMARKS if resample_landmarks else 0) | (RESAMPLE_COLOR if resample_landmarks_color else 0)
        slots = _Slots(_lib.ptr(new["walls"]), None, _lib.ptr(new["landmarks"]), _lib.ptr(new["ints"]), None,
                       _lib.ptr(new["commands"]), _lib.ptr(new["lm_coord"]))
        _lib.check(eng.lib.xv_maze_resample_tasks(eng.handle, int(seed) & (2**64 - 1), int(index_base), int(episode),
                                                  n_task, NG, n_cmd, flags,
                                                  C.cast(C.byref(slots), C.c_void_p)))
        eng.sync()
        return new


def task_dicts_from_device(tables):
    """device (or host) tables -> reference-schema task dicts: arrays cut back to n x n, `start` a
    tuple, `landmarks_coordinates` a list of tuples.  `MazeWorldVecEnv.set_task` and the reference's env both take them."""
    g = {k: (tables[k].detach().cpu().numpy() if torch.is_tensor(tables[k]) else np.asarray(tables[k])) for k in SLOT_KEYS}
    tasks = []
    for i in range(g["ints"].shape[0]):
        n, si, sj, gt, ct, k = (int(v) for v in g["ints"][i, :6])
        cs, wh, ah, fol, sr, gr, cr = (float(v) for v in g["dbl"][i, :7])
        tasks.append({"start": (si, sj), "cell_walls": g["walls"][i, :n, :n].copy(),
                      "cell_texts": g["texts"][i, :n, :n].astype(np.int64), "cell_size": cs, "ground_text": gt,
                      "ceiling_text": ct, "step_reward": sr, "goal_reward": gr, "collision_reward": cr, "wall_height": wh,
                      "agent_height": ah, "fol_angle": fol, "commands_sequence": g["commands"][i].astype(np.int64),
                      "landmarks_coordinates": [(int(a), int(b)) for a, b in g["lm_coord"][i, :k]],
                      "cell_landmarks": g["landmarks"][i, :n, :n].copy()})
    return tasks
