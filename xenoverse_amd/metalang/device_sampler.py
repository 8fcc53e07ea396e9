"""MetaLMV3 task sampling on the GPU: `sample_tasks_device` returns n accepted tasks as the device tables
`MetaLMV3VecEnv.set_task` takes as they are, generated AND tested by `xv_metalm_sample_tasks` (csrc/metalm_sampler.hip), one
workgroup per candidate and one launch per batch.

Same generative model as the reference's TaskSamplerV3 (xenoverse/metalang/task_sampler.py:86-98: three networks from one
seed, so one stream of normals under three scales) and the same acceptance test as its sample_and_check_task
(generator_v3.py:25-46), with counter-based randomness: task k of (seed, sizes, max_len) is the k-th ACCEPTED candidate in
candidate order, a pure function of those arguments whatever the batch size — but not the task NumPy's stream gives for
that seed (for that, `TaskSamplerV3(seed=...)`).  One documented departure: a candidate with a
non-finite reward is rejected (`nonfinite`), where the reference's loop would let a NaN through.  The numpy restatement
the device is tested against is metalang/sampler_host.py.
"""
import ctypes as C
import time

import numpy as np
import torch

from .. import _lib
from ..device_sampling import collect_accepted, engine_scope, sampler_stats
from . import sampler_host as sh
from .lm_host import FUNCTION_VOCABULARY, RandomLMHost, check_lm_limit

STATUS = sh.STATUS
TABLE_KEYS = ("emb", "w_h_t", "b_h", "w_d_t", "b_d")      # xv_metalm_set_task's, in its order
TASK_KEYS = TABLE_KEYS + ("enc_w", "reward_low", "reward_high", "candidate")


def function_tokens(function_vocabulary=None):
    """(stop token, the sorted function tokens) of a function vocabulary (default: the reference's)"""
    vocab = FUNCTION_VOCABULARY if function_vocabulary is None else function_vocabulary
    return int(vocab["s"]), sorted(int(v) for k, v in vocab.items() if k != "s")


def _table_shapes(n, V, E, H):
    return dict(emb=(n, V, E), w_h_t=(n, H + E, H), b_h=(n, H), w_d_t=(n, H, V), b_d=(n, V), enc_w=(n, E, V))


def sample_candidates(engine, seed, cand_base, n_cand, vocab_size, embedding_size, hidden_size, max_len=1024, info=False):
    """One launch over candidates [cand_base, cand_base + n_cand).  -> dict of device tensors, [n_cand] leading, for EVERY
    candidate, accepted or not: the five tables and enc_w (float64), `status` int32 (an index into STATUS), reward_low /
    reward_high float64, `candidate` int64; with info also ppl float64 [n_cand, 2, 3] (per answer: ppl, ppl_min, ppl_max),
    query int32 [n_cand, max_len] with query_len, answer int32 [n_cand, 2, max_len] with answer_len [n_cand, 2] (the
    T = 1e4 and the T = 1e-6 answer) and flags int32 [n_cand], the XV_DEVERR_* bits the candidate's passes raised."""
    V, E, H, n, max_len = int(vocab_size), int(embedding_size), int(hidden_size), int(n_cand), int(max_len)
    for k, v in (("n_vocab", V), ("n_hidden", H), ("n_emb", E), ("max_len", max_len)):
        check_lm_limit(k, v)
    if n < 1 or int(cand_base) < 0:
        raise ValueError("n_cand must be at least 1 and cand_base non-negative")
    d = engine.device
    stop, fun = function_tokens()
    out = {k: torch.empty(s, dtype=torch.float64, device=d) for k, s in _table_shapes(n, V, E, H).items()}
    out["status"] = torch.empty(n, dtype=torch.int32, device=d)
    reward = torch.empty((n, 2), dtype=torch.float64, device=d)
    extra = {}
    if info:
        extra = dict(ppl=torch.empty((n, 2, 3), dtype=torch.float64, device=d),
                     query=torch.empty((n, max_len), dtype=torch.int32, device=d),
                     query_len=torch.empty(n, dtype=torch.int32, device=d),
                     answer=torch.empty((n, 2, max_len), dtype=torch.int32, device=d),
                     answer_len=torch.empty((n, 2), dtype=torch.int32, device=d),
                     flags=torch.empty(n, dtype=torch.int32, device=d))
    ft = (C.c_int32 * max(len(fun), 1))(*fun)
    _lib.check(engine.lib.xv_metalm_sample_tasks(
        engine.handle, int(seed) & (2**64 - 1), int(cand_base), n, V, E, H, max_len, stop, ft, len(fun),
        *(_lib.ptr(out[k]) for k in TABLE_KEYS), _lib.ptr(out["enc_w"]), _lib.ptr(out["status"]), _lib.ptr(reward),
        *(_lib.ptr(extra.get(k)) for k in ("ppl", "query", "query_len", "answer", "answer_len", "flags"))))
    out.update(extra)
    out["reward_low"], out["reward_high"] = reward[:, 0], reward[:, 1]
    out["candidate"] = torch.arange(int(cand_base), int(cand_base) + n, dtype=torch.int64, device=d)
    return out


def sample_tasks_device(n_tasks, vocab_size=32, embedding_size=16, hidden_size=32, seed=0, device="cuda:0", engine=None,
                        batch=None, max_len=1024, max_candidates=None):
    """n_tasks accepted tasks -> dict: the five tables of xv_metalm_set_task and enc_w as device tensors ([n_tasks]
    leading), reward_low / reward_high float64 and `candidate` int64 (the candidate each task was), vocabulary / embedding /
    hidden, function_vocabulary, max_len, seed, and "stats": candidates tried, status histogram, seconds.  Task k is the
    k-th accepted candidate in candidate order, whatever `batch` is.  `MetaLMV3VecEnv.set_task(tables)` takes the result
    as it is; `task_dicts_from_device` turns it into TaskSamplerV3's dicts."""
    n_tasks = int(n_tasks)
    if n_tasks < 1:
        raise ValueError("n_tasks must be at least 1")
    if batch is None:
        batch = int(max(64, min(4096, 2 * n_tasks)))
    batch = int(batch)
    if batch < 1:
        raise ValueError("batch must be at least 1")
    with engine_scope(engine, device) as eng:
        t0 = time.perf_counter()
        got, _, hist = collect_accepted(
            lambda base, n: sample_candidates(eng, seed, base, n, vocab_size, embedding_size, hidden_size, max_len),
            n_tasks, batch, list(TASK_KEYS), STATUS, max_candidates)
        eng.sync()
        out = dict(got, vocabulary=int(vocab_size), embedding=int(embedding_size), hidden=int(hidden_size),
                   function_vocabulary=dict(FUNCTION_VOCABULARY), max_len=int(max_len), seed=int(seed))
        out["stats"] = sampler_stats(hist, STATUS, batch, t0)
        return out


def is_tables(tasks):
    """a tables dict of sample_tasks_device / sample_candidates (and not a TaskSamplerV3 task dict)"""
    return isinstance(tasks, dict) and "lm" not in tasks and all(k in tasks for k in TABLE_KEYS)


def slice_tables(tables, lo, hi):
    """tasks [lo, hi) of a tables dict: views of its tensors, everything else as it is"""
    n = int(tables["emb"].shape[0])
    return {k: (v[lo:hi] if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == n else v) for k, v in tables.items()}


def task_dicts_from_device(tables, index=None):
    """the tasks of a tables dict (all, or those of `index`) -> TaskSamplerV3-shaped dicts whose "lm" is a RandomLMHost made
    from the device's arrays: what pickles, what the host generator takes, and what set_task takes as a list"""
    if not is_tables(tables) or "enc_w" not in tables:
        raise ValueError("task_dicts_from_device needs the dict sample_tasks_device returns")
    host = {k: tables[k].detach().cpu().numpy() for k in TABLE_KEYS + ("enc_w",)}
    n = host["emb"].shape[0]
    index = range(n) if index is None else [int(i) for i in np.asarray(index).reshape(-1)]
    vocab = dict(tables.get("function_vocabulary") or FUNCTION_VOCABULARY)
    stop, fun = function_tokens(vocab)
    V, E, H = host["emb"].shape[1], host["emb"].shape[2], host["b_h"].shape[1]
    return [{"vocabulary": V, "embedding": E, "hidden": H, "function_vocabulary": dict(vocab),
             "lm": RandomLMHost(function_tokens=fun, stop_token=stop, **sh.arrays_of_tables(host, i))} for i in index]
