"""MetaLangV2 task sampling on the GPU: `sample_tasks_v2_device` returns n tasks as the device tables
`MetaLangV2Batch.set_task` takes as they are, written by `xv_metalang_sample_tasks` (csrc/metalang_sampler.hip) in one launch
per batch (by default one launch for all of them).

Same generative model as the reference's TaskSamplerV2 (xenoverse/metalang/task_sampler.py:22-50: the n-gram choice when
n_gram is a list, then five arrays of standard normals), with counter-based randomness: task k of (seed, sizes, n_gram) is
a pure function of those arguments whatever the batch size — but not the task NumPy's stream gives for that seed (for
that, `TaskSamplerV2(seed=...)`).  The reference has no acceptance test for these tasks: every candidate is a task.  The
numpy restatement the device is tested against is metalang/sampler_host_v2.py.
"""
import ctypes as C
import time

import numpy as np
import torch

from .. import _lib
from ..device_sampling import engine_scope, sampler_stats
from . import sampler_host_v2 as sh
from .task_sampler import LIMITS, TASK_ARRAYS, check_limit

STATUS = ("accepted",)
TABLE_KEYS = TASK_ARRAYS + ("_lambda", "n_gram")      # xv_metalang_set_task's, in its order


def _table_shapes(n, V, E, H, NG):
    return dict(word_emb=(n, V, E), weights_inputlayer=(n, NG, E, H), bias_inputlayer=(n, NG, H),
                weights_outputlayer=(n, H, V), bias_outputlayer=(n, V))


def sample_tasks_v2_device(n_tasks, n_emb=16, n_hidden=64, n_vocab=256, n_gram=3, _lambda=5.0, seed=0, device="cuda:0",
                           engine=None, batch=None):
    """n_tasks tasks -> dict: word_emb [n, V, E], weights_inputlayer [n, NG, E, H], bias_inputlayer [n, NG, H] (NG = the
    largest entry of n_gram; exact zeros at and beyond a task's own n), weights_outputlayer [n, H, V], bias_outputlayer
    [n, V], _lambda [n] as float64 device tensors and n_gram int32 [n]; n_vocab, n_emb, n_hidden, n_gram_max, seed; "stats".
    n_gram: an int, or a list a task draws its n from.  Task k is the same bits whatever `batch` (tasks per launch;
    default: all) is.  `MetaLangV2Batch.set_task(tables)` takes the result as it is; `task_dicts_from_device_v2` turns it
    into TaskSamplerV2's dicts."""
    n_tasks, V, E, H = int(n_tasks), int(n_vocab), int(n_emb), int(n_hidden)
    if n_tasks < 1:
        raise ValueError("n_tasks must be at least 1")
    batch = n_tasks if batch is None else int(batch)
    if batch < 1:
        raise ValueError("batch must be at least 1")
    sh.check_sizes(V, E, H)
    lst = sh.n_gram_list(n_gram, LIMITS["n_gram"])
    NG = max(lst)
    c_list = (C.c_int32 * len(lst))(*lst)
    with engine_scope(engine, device) as eng:
        t0 = time.perf_counter()
        d = eng.device
        out = {k: torch.empty(s, dtype=torch.float64, device=d) for k, s in _table_shapes(n_tasks, V, E, H, NG).items()}
        out["_lambda"] = torch.empty(n_tasks, dtype=torch.float64, device=d)
        out["n_gram"] = torch.empty(n_tasks, dtype=torch.int32, device=d)
        for lo in range(0, n_tasks, batch):
            hi = min(n_tasks, lo + batch)
            _lib.check(eng.lib.xv_metalang_sample_tasks(
                eng.handle, int(seed) & (2**64 - 1), lo, hi - lo, V, E, H, c_list, len(lst), NG, float(_lambda),
                *(_lib.ptr(out[k][lo:hi]) for k in TABLE_KEYS)))
        eng.sync()
        out.update(n_vocab=V, n_emb=E, n_hidden=H, n_gram_max=NG, seed=int(seed))
        out["stats"] = sampler_stats(np.array([n_tasks], np.int64), STATUS, batch, t0)
        return out


def is_tables_v2(tasks):
    """a tables dict of sample_tasks_v2_device (and not a TaskSamplerV2 task dict, whose arrays have no task axis)"""
    return (isinstance(tasks, dict) and all(k in tasks for k in TABLE_KEYS) and torch.is_tensor(tasks["word_emb"])
            and tasks["word_emb"].dim() == 3)


def check_tables_v2(tables):
    """shapes, dtypes and limits of a tables dict -> (n_task, V, E, H, NG); ValueError for a malformed one, XenoError for
    a size outside LIMITS"""
    emb = tables["word_emb"]
    n, V, E = (int(s) for s in emb.shape)
    w_in = tables["weights_inputlayer"]
    if w_in.dim() != 4:
        raise ValueError("tables: weights_inputlayer must be [n_task, n_gram_max, n_emb, n_hidden]")
    NG, H = int(w_in.shape[1]), int(w_in.shape[3])
    for k, v in (("n_vocab", V), ("n_hidden", H), ("n_emb", E), ("n_gram", NG)):
        check_limit(k, v)
    shapes = dict(_table_shapes(n, V, E, H, NG), _lambda=(n,), n_gram=(n,))
    for k in TABLE_KEYS:
        t = tables[k]
        want = torch.int32 if k == "n_gram" else torch.float64
        if not torch.is_tensor(t) or tuple(t.shape) != shapes[k] or t.dtype != want or t.device != emb.device:
            raise ValueError("tables: %s must be a %s tensor of shape %s on %s" % (k, want, shapes[k], emb.device))
    return n, V, E, H, NG


def task_dicts_from_device_v2(tables, index=None):
    """the tasks of a tables dict (all, or those of `index`) -> TaskSamplerV2-shaped dicts of numpy arrays: what pickles,
    what MetaLangV2Host takes, and what set_task takes as a list"""
    if not is_tables_v2(tables):
        raise ValueError("task_dicts_from_device_v2 needs the dict sample_tasks_v2_device returns")
    n, V, E, H, _ = check_tables_v2(tables)
    host = {k: tables[k].detach().cpu().numpy() for k in TABLE_KEYS}
    index = range(n) if index is None else [int(i) for i in np.asarray(index).reshape(-1)]
    out = []
    for i in index:
        g = int(host["n_gram"][i])
        out.append({"word_emb": host["word_emb"][i].copy(), "weights_inputlayer": host["weights_inputlayer"][i, :g].copy(),
                    "bias_inputlayer": host["bias_inputlayer"][i, :g].reshape(g, 1, H).copy(),
                    "weights_outputlayer": host["weights_outputlayer"][i].copy(),
                    "bias_outputlayer": host["bias_outputlayer"][i].reshape(1, V).copy(),
                    "_lambda": float(host["_lambda"][i]), "n_emb": E, "n_hidden": H, "n_vocab": V, "n_gram": g})
    return out
