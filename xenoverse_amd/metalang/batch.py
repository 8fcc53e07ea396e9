"""MetaLangV2 on the device (csrc/metalang.hip, C-ABI xv_metalang_*): MetaLangV2Batch generates, and scores, many groups of
sequences in one launch; MetaLangV2 puts the reference's surface (xenoverse/metalang/metalangv2.py:79-110) on one group."""
import ctypes as C
import os

import numpy as np

from .. import _lib
from .task_sampler import TASK_ARRAYS, check_limit, check_task


DESCRIBE_KEYS = ("block", "w_out_regs", "single_seq", "tables_in_lds", "steps_per_io", "logits", "act_seqs", "lds_bytes",
                 "lds_opt_in", "teacher_chunk")      # xv_metalang_describe's out[0 .. 9] (include/xeno.h)
LOGITS_WHERE = ("register", "lds", "scratch")


def _describe(lib, h, teacher):
    out = (C.c_int32 * len(DESCRIBE_KEYS))()
    _lib.check(lib.xv_metalang_describe(h, 1 if teacher else 0, out))
    d = dict(zip(DESCRIBE_KEYS, (int(v) for v in out)))
    for k in ("single_seq", "tables_in_lds", "lds_opt_in"):
        d[k] = bool(d[k])
    d["logits"] = LOGITS_WHERE[d["logits"]]
    return d


def describe_dispatch(seqs_per_group, n_vocab, n_emb, n_hidden, n_gram_max, teacher=False):
    """what a MetaLangV2Batch of these sizes would launch (MetaLangV2Batch.describe), from the library's own selection, without
    a GPU: the handle is made without an engine and can do nothing else"""
    lib = _lib.load()
    h = C.c_void_p()
    _lib.check(lib.xv_metalang_create(None, 1, int(seqs_per_group), int(n_vocab), int(n_emb), int(n_hidden), int(n_gram_max),
                                      C.byref(h)))
    try:
        return _describe(lib, h, teacher)
    finally:
        lib.xv_metalang_destroy(h)


class MetaLangV2Batch(object):
    """n_group groups of seqs_per_group sequences.  A group is one call of the reference's forward(L, batch=seqs_per_group)
    under one task: its sequences share the mean and the standard deviation of the logits at every step.  Every task of a
    handle has the same n_vocab, n_emb and n_hidden; n_gram is per task.

    Free-running draws are Philox, keyed by (seed, env_id_base + group * seqs_per_group + b, the engine's tick at the call,
    position): a handle over groups [g0, g1) made with env_id_base + g0 * seqs_per_group draws what the whole batch draws
    there.  Every generate() advances the tick by one."""

    def __init__(self, n_group, seqs_per_group=1, device="cuda:0", seed=0, env_id_base=0):
        from ..engine import Engine
        if int(n_group) < 1:
            raise ValueError("n_group must be at least 1")
        check_limit("batch", seqs_per_group)
        self.n_group, self.seqs_per_group = int(n_group), int(seqs_per_group)
        self._h = None
        self.engine = Engine(device, seed=seed, env_id_base=env_id_base)
        self.lib, self.device = self.engine.lib, self.engine.device
        self._tables = None
        self.n_vocab = None

    # ---- tasks ----------------------------------------------------------------------------------------------------
    def set_task(self, tasks, group_task_index=None):
        """tasks: one task dict (TaskSamplerV2), a list of them, or the device tables of sample_tasks_v2_device (borrowed as
        they are: keep them unchanged while the handle uses them); group_task_index int[n_group]: the task of every group
        (default: the only task; task g for group g when there are n_group tasks)"""
        import torch
        from .device_sampler_v2 import TABLE_KEYS, check_tables_v2, is_tables_v2
        if is_tables_v2(tasks):      # the device tables of sample_tasks_v2_device: borrowed as they are, no host copy
            n_task, V, E, H, NG = check_tables_v2(tasks)
            gti = self._group_task_index(n_task, group_task_index)
            dev = [tasks[k] if tasks[k].is_contiguous() else tasks[k].contiguous() for k in TABLE_KEYS]
            if dev[0].device != torch.device(self.device):
                raise ValueError("the tables are on %s, this handle on %s" % (dev[0].device, self.device))
            return self._set_tables(dev + [torch.from_numpy(gti).to(self.device)], n_task, V, E, H, NG)
        if isinstance(tasks, dict):
            tasks = [tasks]
        if not len(tasks):
            raise ValueError("set_task needs at least one task")
        sizes = [check_task(t, "task %d" % k) for k, t in enumerate(tasks)]
        V, E, H = sizes[0][:3]
        for k, s in enumerate(sizes):
            if s[:3] != (V, E, H):
                raise ValueError("task %d has (n_vocab, n_emb, n_hidden) = %s, task 0 has %s: one handle holds one size"
                                 % (k, s[:3], (V, E, H)))
        n_task, NG = len(tasks), max(s[3] for s in sizes)
        gti = self._group_task_index(n_task, group_task_index)
        w_in = np.zeros((n_task, NG, E, H))
        b_in = np.zeros((n_task, NG, H))
        for k, (t, s) in enumerate(zip(tasks, sizes)):
            w_in[k, :s[3]] = t["weights_inputlayer"]
            b_in[k, :s[3]] = np.asarray(t["bias_inputlayer"]).reshape(s[3], H)
        host = [np.stack([np.asarray(t["word_emb"], np.float64) for t in tasks]), w_in, b_in,
                np.stack([np.asarray(t["weights_outputlayer"], np.float64) for t in tasks]),
                np.stack([np.asarray(t["bias_outputlayer"], np.float64).reshape(V) for t in tasks]),
                np.array([float(t["_lambda"]) for t in tasks], np.float64),
                np.array([s[3] for s in sizes], np.int32), gti]
        self._set_tables([torch.from_numpy(np.ascontiguousarray(a)).to(self.device) for a in host], n_task, V, E, H, NG)

    def _group_task_index(self, n_task, group_task_index):
        """the task of every group -> int32[n_group]; default: the only task, task g for group g when there are n_group"""
        if group_task_index is None:
            if n_task == 1:
                group_task_index = np.zeros(self.n_group, np.int32)
            elif n_task == self.n_group:
                group_task_index = np.arange(self.n_group, dtype=np.int32)
            else:
                raise ValueError("%d tasks for %d groups: give group_task_index" % (n_task, self.n_group))
        if hasattr(group_task_index, "detach"):
            group_task_index = group_task_index.detach().cpu().numpy()
        gti = np.ascontiguousarray(group_task_index, dtype=np.int32)
        if gti.shape != (self.n_group,) or gti.min() < 0 or gti.max() >= n_task:
            raise ValueError("group_task_index must be int[n_group] with values in [0, %d)" % n_task)
        return gti

    def _set_tables(self, dev, n_task, V, E, H, NG):
        """dev: the eight device tensors of xv_metalang_set_task, in its order; the handle borrows them"""
        if self._h is not None and (V, E, H, NG) != (self.n_vocab, self.n_emb, self.n_hidden, self.n_gram_max):
            self._destroy()
        if self._h is None:
            h = C.c_void_p()
            _lib.check(self.lib.xv_metalang_create(self.engine.handle, self.n_group, self.seqs_per_group, V, E, H, NG,
                                                   C.byref(h)))
            self._h = h
        self.engine.sync()      # the tables a running call reads are let go below
        _lib.check(self.lib.xv_metalang_set_task(self._h, n_task, *(_lib.ptr(t) for t in dev)))
        self._tables = dev      # borrowed by the handle
        self.n_vocab, self.n_emb, self.n_hidden, self.n_gram_max, self.n_task = V, E, H, NG, n_task

    def _live(self):
        if self._h is None:
            raise Exception("Please set task before using data generator")      # the reference's text (metalangv2.py:102)

    # ---- generation -----------------------------------------------------------------------------------------------
    def generate(self, L, draws=None, return_logp=False):
        """L steps of every group -> tokens int32[n_group, seqs_per_group, L + 1] on the device (token 0 first), and with
        return_logp the log-probability of every chosen token, float64[n_group, seqs_per_group, L].  draws: the uniforms,
        float64[n_group, seqs_per_group, L] (the parity path); None: Philox."""
        import torch
        self._live()
        L = int(L)
        if L < 1:
            raise ValueError("L must be at least 1")
        shape = (self.n_group, self.seqs_per_group, L)
        u = None
        if draws is not None:
            u = torch.as_tensor(draws, dtype=torch.float64).to(self.device).contiguous()
            if tuple(u.shape) != shape:
                raise ValueError("draws must have shape %s, got %s" % (shape, tuple(u.shape)))
        tokens = torch.empty(shape[:2] + (L + 1,), dtype=torch.int32, device=self.device)
        logp = torch.empty(shape, dtype=torch.float64, device=self.device) if return_logp else None
        _lib.check(self.lib.xv_metalang_generate(self._h, L, _lib.ptr(u), _lib.ptr(tokens), _lib.ptr(logp)))
        if u is not None:
            self.engine.sync()      # a converted copy of the draws must outlive the launch
        return (tokens, logp) if return_logp else tokens

    def log_prob(self, tokens):
        """teacher forcing: tokens int[n_group, seqs_per_group, L + 1] -> float64[n_group, seqs_per_group, L], the
        log-probability of every token after the first given its predecessors (with the group's statistics)"""
        import torch
        self._live()
        t = torch.as_tensor(tokens).to(self.device, torch.int32).contiguous()
        if t.dim() != 3 or tuple(t.shape[:2]) != (self.n_group, self.seqs_per_group) or t.shape[2] < 2:
            raise ValueError("tokens must have shape (%d, %d, L + 1)" % (self.n_group, self.seqs_per_group))
        L = int(t.shape[2]) - 1
        logp = torch.empty((self.n_group, self.seqs_per_group, L), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.xv_metalang_log_prob(self._h, L, _lib.ptr(t), _lib.ptr(logp)))
        self.engine.sync()
        return logp

    def describe(self, teacher=False):
        """which kernel variant and layouts generate (teacher=False) or log_prob (teacher=True) launches for the task set
        (xv_metalang_describe) -> dict with DESCRIBE_KEYS: block 64 / 256 / 1024; w_out_regs 16 / 32 / 64, 0: W_out through
        L2; single_seq; tables_in_lds; steps_per_io; logits "register" / "lds" / "scratch"; act_seqs; lds_bytes; lds_opt_in
        (above 64 KiB); teacher_chunk (0: one workgroup runs the whole call)"""
        self._live()
        return _describe(self.lib, self._h, teacher)

    @staticmethod
    def perplexity(logp):
        """the reference's "Ground Truth Sequence Perplexity" of every group: the mean of -log p over its draws -> [n_group]"""
        return -logp.mean(dim=(1, 2))

    def check_errors(self, clear=True):
        """the engine's sticky device error word (0: none)"""
        return self.engine.error_flags(clear)

    def _destroy(self):
        if self._h is not None:
            self.lib.xv_metalang_destroy(self._h)
            self._h = None
            self._tables = None

    def close(self):
        self._destroy()
        if getattr(self, "engine", None) is not None:
            self.engine.close()
            self.engine = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MetaLangV2(object):
    """The reference's MetaLangV2 (metalangv2.py:79-110) on the device: one task, sequences of L + 1 tokens.  `seed` keys the
    Philox stream of the call (the reference seeds numpy's global generator with it: other numbers, same distribution);
    None draws a seed from the OS."""

    def __init__(self, L=4096, device="cuda:0"):
        self.L = int(L)
        assert L > 1
        self.device = device
        self.task_set = False

    def set_task(self, task):
        check_task(task)
        self.task = task
        self.task_set = True

    def _generate(self, batch_size, seed):
        if not self.task_set:
            raise Exception("Please set task before using data generator")
        if seed is None:
            seed = int.from_bytes(os.urandom(8), "little")
        gen = MetaLangV2Batch(1, batch_size, device=self.device, seed=seed)
        try:
            gen.set_task(self.task)
            tokens = gen.generate(self.L)[0].cpu().numpy()
            flags = gen.check_errors()
        finally:
            gen.close()
        if flags:
            raise _lib.XenoError("MetaLangV2: device error flags 0x%x (include/xeno.h XV_DEVERR_*)" % flags)
        return tokens

    def data_generator(self, seed=None):
        """-> int32[L + 1]"""
        return self._generate(1, seed)[0]

    def batch_generator(self, batch_size, seed=None):
        """-> int32[batch_size, L + 1]; the sequences of one call are one group"""
        return self._generate(batch_size, seed)
