"""What the device task samplers (anymdp / linds / mazeworld `device_sampler.py`) share: the engine they launch on, the loop
that collects the first n ACCEPTED candidates in candidate order, and the `stats` entry of their result.

The loop is where the samplers' common promise is kept: task k is the k-th accepted candidate and the status histogram
stops at the last candidate needed, so neither depends on the batch size the candidates were launched in.  It touches
tensors through torch only (no engine, no device assumed): tests/test_host_task_path.py runs it on CPU tensors.
"""
import time

import numpy as np
import torch

from .engine import Engine


class engine_scope(object):
    """`with engine_scope(engine, device) as eng`: `engine` when the caller passed one, else an Engine(device) that this
    scope owns and closes when it ends.  (A plain class: entering it costs well under a microsecond, a generator-based
    context manager several — a resample call over 16,384 tasks takes 200.)"""
    __slots__ = ("engine", "own")

    def __init__(self, engine, device):
        self.own = engine is None
        self.engine = Engine(device) if self.own else engine

    def __enter__(self):
        return self.engine

    def __exit__(self, *exc):
        if self.own:
            self.engine.close()


def collect_accepted(launch, n_tasks, batch, keys, status_names, max_candidates=None):
    """launch(cand_base, n_cand) -> dict: one launch over candidates [cand_base, cand_base + n_cand) with `[n_cand]`-leading
    tensors under `keys` and the candidates' status (0 = accepted, else an index into status_names) either in host records
    `info["status"]` or, when the launch fetches none, in a tensor `status` (one read-back per batch, for the histogram).
    -> (tensors of the first n_tasks accepted candidates, their info records or None, status histogram int64[len(status_names)]
    over candidates 0 ... the n_tasks-th accepted one).  max_candidates is checked before each batch: RuntimeError when that
    many candidates were launched and tasks are still missing."""
    got = {k: [] for k in keys}
    infos = []
    hist = np.zeros(len(status_names), np.int64)
    n_acc = base = 0
    while n_acc < n_tasks:
        if max_candidates is not None and base >= max_candidates:
            raise RuntimeError("only %d of %d tasks accepted within %d candidates" % (n_acc, n_tasks, base))
        r = launch(base, batch)
        info = r.get("info")
        # (with records the status is on the host already; without, the search for the accepted runs where the launch left it)
        st = r["status"] if info is None else torch.from_numpy(np.ascontiguousarray(info["status"]))
        acc = torch.nonzero(st == 0).flatten()[: n_tasks - n_acc]
        last = int(acc[-1]) + 1 if len(acc) and n_acc + len(acc) >= n_tasks else batch
        hist += np.bincount(st[:last].cpu().numpy(), minlength=len(status_names))[: len(status_names)]
        sel = acc.to(r[keys[0]].device)
        for k in keys:
            got[k].append(r[k].index_select(0, sel))
        if info is not None:
            infos.append(info[acc.numpy()])
        n_acc += int(len(acc))
        base += batch
    return {k: torch.cat(v) for k, v in got.items()}, (np.concatenate(infos) if infos else None), hist


def sampler_stats(hist, status_names, batch, t0, **extra):
    """the `stats` entry of a sample_tasks_device result; t0: time.perf_counter() when the sampling began"""
    return dict(candidates=int(hist.sum()), accepted=int(hist[0]), seconds=time.perf_counter() - t0,
                status={name: int(h) for name, h in zip(status_names, hist)}, batch=batch, **extra)
