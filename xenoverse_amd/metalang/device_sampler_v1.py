"""MetaLangV1 task sampling on the GPU: `sample_tasks_v1_device` returns n tasks as the CSR device tables
`MetaLangV1Batch.set_task` takes as they are, written by xv_metalang1_sample_lengths / _offsets / _tokens
(csrc/metalang_sampler.hip): lengths are variable, so a lengths launch, a prefix sum and a tokens launch.

Same generative model as the reference's TaskSamplerV1 (xenoverse/metalang/task_sampler.py:52-73: the n-gram choice when
n_gram is a list, then n_patterns patterns of max(3, Poisson(n_gram)) tokens uniform in [0, n_vocab)), with counter-based
randomness: task k of (seed, arguments) is a pure function of those arguments whatever the batch size — but not the task
NumPy's stream gives for that seed (for that, `TaskSamplerV1(seed=...)`).  The reference has no acceptance test for these
tasks: every candidate is a task.  n_gram: an integer (or a list of them) in 1 .. 512, sampler_host_v1.NGRAM_MAX; anything
else is refused by name.  The numpy restatement the device equals bit for bit is metalang/sampler_host_v1.py.
"""
import ctypes as C
import time

import numpy as np
import torch

from .. import _lib
from ..device_sampling import engine_scope, sampler_stats
from . import sampler_host_v1 as sh
from .host_v1 import LIMITS_V1

STATUS = ("accepted",)
TABLE_KEYS = ("task_pattern_offset", "pattern_token_offset", "tokens", "n_vocab", "error_ratio")   # xv_metalang1_set_task's


def sample_tasks_v1_device(n_tasks, n_vocab=64, n_patterns=10, n_gram=64, error_ratio=0.1, seed=0, device="cuda:0",
                           engine=None, batch=None):
    """n_tasks tasks -> dict of device tensors: task_pattern_offset int32[n + 1] (task t owns patterns
    [t n_patterns, (t + 1) n_patterns)), pattern_token_offset int32[n n_patterns + 1], tokens int32[total], n_vocab int32[n],
    error_ratio float64[n], n_gram int32[n] (the mean length each task drew from the list); n_patterns, seed; "stats".
    Task k is the same bits whatever `batch` (tasks per launch; default: all) is.  `MetaLangV1Batch.set_task(tables)` takes
    the result as it is; `task_dicts_from_device_v1` turns it into TaskSamplerV1's dicts."""
    n_tasks, V, nP = int(n_tasks), int(n_vocab), int(n_patterns)
    if n_tasks < 1:
        raise ValueError("n_tasks must be at least 1")
    batch = n_tasks if batch is None else int(batch)
    if batch < 1:
        raise ValueError("batch must be at least 1")
    lst, exp_neg = sh.check_args(n_tasks, V, nP, n_gram)
    c_list = (C.c_int32 * len(lst))(*lst)
    c_exp = (C.c_double * len(lst))(*[float(v) for v in exp_neg])
    seed64 = int(seed) & (2**64 - 1)
    with engine_scope(engine, device) as eng:
        t0 = time.perf_counter()
        d = eng.device
        lengths = torch.empty(n_tasks * nP, dtype=torch.int32, device=d)
        out = dict(task_pattern_offset=torch.empty(n_tasks + 1, dtype=torch.int32, device=d),
                   pattern_token_offset=torch.empty(n_tasks * nP + 1, dtype=torch.int32, device=d),
                   n_vocab=torch.full((n_tasks,), V, dtype=torch.int32, device=d),
                   error_ratio=torch.full((n_tasks,), float(error_ratio), dtype=torch.float64, device=d),
                   n_gram=torch.empty(n_tasks, dtype=torch.int32, device=d))
        total = torch.empty(1, dtype=torch.int64, device=d)
        cuts = list(range(0, n_tasks, batch)) + [n_tasks]
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            _lib.check(eng.lib.xv_metalang1_sample_lengths(eng.handle, seed64, lo, hi - lo, nP, c_list, c_exp, len(lst),
                                                           _lib.ptr(out["n_gram"][lo:hi]), _lib.ptr(lengths[lo * nP:hi * nP])))
        off = out["pattern_token_offset"]
        _lib.check(eng.lib.xv_metalang1_sample_offsets(eng.handle, n_tasks, nP, _lib.ptr(lengths),
                                                       _lib.ptr(out["task_pattern_offset"]), _lib.ptr(off), _lib.ptr(total)))
        eng.sync()
        # one read-back: the total sizes `tokens`, the offsets at the batches' cuts say which tokens a launch writes
        n_token = int(total.item())
        if n_token > LIMITS_V1["tokens"]:
            raise _lib.XenoError("MetaLangV1: %d pattern tokens are more than the supported %d" % (n_token, LIMITS_V1["tokens"]))
        at = off[torch.tensor([c * nP for c in cuts], device=d)].tolist()
        out["tokens"] = torch.empty(n_token, dtype=torch.int32, device=d)
        for lo, hi, t_lo, t_hi in zip(cuts[:-1], cuts[1:], at[:-1], at[1:]):
            _lib.check(eng.lib.xv_metalang1_sample_tokens(eng.handle, seed64, lo, hi - lo, nP, V,
                                                          _lib.ptr(off[lo * nP:hi * nP + 1]), t_lo, t_hi - t_lo,
                                                          _lib.ptr(out["tokens"])))
        eng.sync()
        out.update(n_patterns=nP, seed=int(seed))
        out["stats"] = sampler_stats(np.array([n_tasks], np.int64), STATUS, batch, t0, tokens=n_token)
        return out


def is_tables_v1(tasks):
    """a tables dict of sample_tasks_v1_device (and not a TaskSamplerV1 task dict)"""
    return isinstance(tasks, dict) and "patterns" not in tasks and all(k in tasks for k in TABLE_KEYS)


def check_tables_v1(tables):
    """shapes and dtypes of a tables dict -> (n_task, n_pattern_total, n_token_total); ValueError for a malformed one"""
    tpo, pto, tok = (tables[k] for k in TABLE_KEYS[:3])
    n = int(tpo.shape[0]) - 1
    shapes = dict(task_pattern_offset=(n + 1,), pattern_token_offset=(int(pto.shape[0]),), tokens=(int(tok.shape[0]),),
                  n_vocab=(n,), error_ratio=(n,))
    for k in TABLE_KEYS:
        t = tables[k]
        want = torch.float64 if k == "error_ratio" else torch.int32
        if not torch.is_tensor(t) or t.dim() != 1 or tuple(t.shape) != shapes[k] or t.dtype != want or t.device != tok.device:
            raise ValueError("tables: %s must be a %s tensor of shape %s on %s" % (k, want, shapes[k], tok.device))
    if n < 1 or pto.shape[0] < 2 or tok.shape[0] < 1:
        raise ValueError("tables: at least one task, one pattern and one token are needed")
    return n, int(pto.shape[0]) - 1, int(tok.shape[0])


def task_dicts_from_device_v1(tables, index=None):
    """the tasks of a tables dict (all, or those of `index`) -> TaskSamplerV1-shaped dicts of numpy arrays: what pickles,
    what MetaLangV1Host takes, and what set_task takes as a list"""
    if not is_tables_v1(tables):
        raise ValueError("task_dicts_from_device_v1 needs the dict sample_tasks_v1_device returns")
    n, _, _ = check_tables_v1(tables)
    host = {k: tables[k].detach().cpu().numpy() for k in TABLE_KEYS}
    grams = tables["n_gram"].detach().cpu().numpy() if torch.is_tensor(tables.get("n_gram")) else None
    index = range(n) if index is None else [int(i) for i in np.asarray(index).reshape(-1)]
    tpo, pto, tok = (host[k] for k in TABLE_KEYS[:3])
    out = []
    for i in index:
        pats = [tok[pto[p]:pto[p + 1]].copy() for p in range(tpo[i], tpo[i + 1])]
        task = {"patterns": pats, "n_vocab": int(host["n_vocab"][i]), "n_patterns": len(pats),
                "error_ratio": float(host["error_ratio"][i])}
        if grams is not None:
            task["n_gram"] = int(grams[i])
        out.append(task)
    return out
