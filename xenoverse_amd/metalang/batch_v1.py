"""MetaLangV1 on the device (csrc/metalang_v1.hip, C-ABI xv_metalang1_*): MetaLangV1Batch generates many sequences, each under
its own task, in one launch; MetaLangV1 puts the reference's surface (xenoverse/metalang/metalangv1.py:20-118) on it."""
import ctypes as C
import os
import sys

import numpy as np

from .. import _lib
from .host_v1 import DRAW_ARRAYS, check_length_v1, check_task_v1


class MetaLangV1Batch(object):
    """n_seq sequences.  Free-running draws are Philox, keyed by (seed, env_id_base + sequence, the engine's tick at the
    call, kind, segment or position): a handle over sequences [s0, s1) made with env_id_base + s0 draws what the whole batch
    draws there.  Every generate() advances the tick by one."""

    def __init__(self, n_seq, device="cuda:0", seed=0, env_id_base=0):
        from ..engine import Engine
        if int(n_seq) < 1:
            raise ValueError("n_seq must be at least 1")
        self.n_seq = int(n_seq)
        self._h = None
        self._tables = None
        self.engine = Engine(device, seed=seed, env_id_base=env_id_base)
        self.lib, self.device = self.engine.lib, self.engine.device
        h = C.c_void_p()
        _lib.check(self.lib.xv_metalang1_create(self.engine.handle, self.n_seq, C.byref(h)))
        self._h = h

    # ---- tasks ----------------------------------------------------------------------------------------------------
    def set_task(self, tasks, seq_task_index=None):
        """tasks: one task dict (TaskSamplerV1), a list of them, or the device tables of sample_tasks_v1_device (borrowed as
        they are: keep them unchanged while the handle uses them); seq_task_index int[n_seq]: the task of every sequence
        (default: the only task; task i for sequence i when there are n_seq tasks)"""
        import torch
        from .device_sampler_v1 import TABLE_KEYS, check_tables_v1, is_tables_v1
        if is_tables_v1(tasks):      # the device tables of sample_tasks_v1_device: no host copy
            n_task, n_pattern, n_token = check_tables_v1(tasks)
            sti = self._seq_task_index(n_task, seq_task_index)
            dev = [tasks[k] if tasks[k].is_contiguous() else tasks[k].contiguous() for k in TABLE_KEYS]
            if dev[0].device != torch.device(self.device):
                raise ValueError("the tables are on %s, this handle on %s" % (dev[0].device, self.device))
            return self._set_tables(dev + [torch.from_numpy(sti).to(self.device)], n_task, n_pattern, n_token)
        if isinstance(tasks, dict):
            tasks = [tasks]
        if not len(tasks):
            raise ValueError("set_task needs at least one task")
        checked = [check_task_v1(t, "task %d" % k) for k, t in enumerate(tasks)]
        n_task = len(tasks)
        sti = self._seq_task_index(n_task, seq_task_index)
        lens = np.array([len(p) for pats, _, _ in checked for p in pats], np.int64)
        if lens.sum() > 2 ** 31 - 1:
            raise _lib.XenoError("MetaLangV1: %d pattern tokens are more than the supported %d" % (lens.sum(), 2 ** 31 - 1))
        host = [np.concatenate([[0], np.cumsum([len(pats) for pats, _, _ in checked])]).astype(np.int32),
                np.concatenate([[0], np.cumsum(lens)]).astype(np.int32),
                np.concatenate([p for pats, _, _ in checked for p in pats]).astype(np.int32),
                np.array([V for _, V, _ in checked], np.int32), np.array([e for _, _, e in checked], np.float64), sti]
        self._set_tables([torch.from_numpy(np.ascontiguousarray(a)).to(self.device) for a in host], n_task, len(lens),
                         int(lens.sum()))

    def _seq_task_index(self, n_task, seq_task_index):
        """the task of every sequence -> int32[n_seq]; default: the only task, task i for sequence i when there are n_seq"""
        if seq_task_index is None:
            if n_task == 1:
                seq_task_index = np.zeros(self.n_seq, np.int32)
            elif n_task == self.n_seq:
                seq_task_index = np.arange(self.n_seq, dtype=np.int32)
            else:
                raise ValueError("%d tasks for %d sequences: give seq_task_index" % (n_task, self.n_seq))
        if hasattr(seq_task_index, "detach"):
            seq_task_index = seq_task_index.detach().cpu().numpy()
        sti = np.ascontiguousarray(seq_task_index, dtype=np.int32)
        if sti.shape != (self.n_seq,) or sti.min() < 0 or sti.max() >= n_task:
            raise ValueError("seq_task_index must be int[n_seq] with values in [0, %d)" % n_task)
        return sti

    def _set_tables(self, dev, n_task, n_pattern, n_token):
        """dev: the six device tensors of xv_metalang1_set_task, in its order; the handle borrows them"""
        self.engine.sync()      # the tables a running call reads are let go below
        _lib.check(self.lib.xv_metalang1_set_task(self._h, n_task, n_pattern, n_token, *(_lib.ptr(t) for t in dev)))
        self._tables = dev      # borrowed by the handle
        self.n_task = n_task

    # ---- generation -----------------------------------------------------------------------------------------------
    def generate(self, L, draws=None, return_kinds=False, mask_ratio=0.30):
        """-> features, labels int32[n_seq, L] on the device; with return_kinds also kinds uint8[n_seq, L] (0 clean, 1 replaced,
        2 masked, 3 separator) and n_segments int32[n_seq].  draws: dict(pattern_index int32[n_seq, n_slot], noise_value
        int32[n_seq, L + 1], u_noise, u_mask float64[n_seq, L + 1]) (the parity path); None: Philox."""
        import torch
        if self._tables is None:
            raise Exception("Please set task before using data generator")      # the reference's text (metalangv1.py:59)
        L = check_length_v1(L)
        d, n_slot = [None] * 4, 0
        if draws is not None:
            kinds_ = (torch.int32, torch.int32, torch.float64, torch.float64)
            d = [torch.as_tensor(np.asarray(draws[k]) if not torch.is_tensor(draws[k]) else draws[k]).to(self.device, t).contiguous()
                 for k, t in zip(DRAW_ARRAYS, kinds_)]
            if d[0].dim() != 2 or d[0].shape[0] != self.n_seq or d[0].shape[1] < 1:
                raise ValueError("pattern_index must have shape (%d, n_slot), n_slot >= 1" % self.n_seq)
            for k, a in zip(DRAW_ARRAYS[1:], d[1:]):
                if tuple(a.shape) != (self.n_seq, L + 1):
                    raise ValueError("%s must have shape %s, got %s" % (k, (self.n_seq, L + 1), tuple(a.shape)))
            n_slot = int(d[0].shape[1])
        features = torch.empty((self.n_seq, L), dtype=torch.int32, device=self.device)
        labels = torch.empty((self.n_seq, L), dtype=torch.int32, device=self.device)
        kinds = torch.empty((self.n_seq, L), dtype=torch.uint8, device=self.device) if return_kinds else None
        n_seg = torch.empty((self.n_seq,), dtype=torch.int32, device=self.device) if return_kinds else None
        _lib.check(self.lib.xv_metalang1_generate(self._h, L, float(mask_ratio), _lib.ptr(d[0]), n_slot, _lib.ptr(d[1]),
                                                  _lib.ptr(d[2]), _lib.ptr(d[3]), _lib.ptr(features), _lib.ptr(labels),
                                                  _lib.ptr(kinds), _lib.ptr(n_seg)))
        if draws is not None:
            self.engine.sync()      # converted copies of the draws must outlive the launch
        return (features, labels, kinds, n_seg) if return_kinds else (features, labels)

    def check_errors(self, clear=True):
        """the engine's sticky device error word (0: none)"""
        return self.engine.error_flags(clear)

    def close(self):
        if getattr(self, "_h", None) is not None:
            self.lib.xv_metalang1_destroy(self._h)
            self._h = None
            self._tables = None
        if getattr(self, "engine", None) is not None:
            self.engine.close()
            self.engine = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MetaLangV1(object):
    """The reference's MetaLangV1 (metalangv1.py:20-118) on the device: one task, (features, labels) of L tokens.  `seed` keys
    the Philox stream of the call, as for MetaLangV2 here (the reference ignores it in V1 and draws from numpy's global
    generator); None draws a seed from the OS."""

    def __init__(self, L=2048, device="cuda:0"):
        self.L = int(L)
        self.mask_ratio = 0.30
        self.device = device
        self.task_set = False
        assert self.L > 1

    def set_task(self, task):
        check_task_v1(task)
        for key, val in task.items():
            self.__dict__[key] = val
        self.task = task
        self.task_set = True

    def _generate(self, batch_size, seed):
        if not self.task_set:
            raise Exception("Please set task before using data generator")
        if seed is None:
            seed = int.from_bytes(os.urandom(8), "little")
        gen = MetaLangV1Batch(batch_size, device=self.device, seed=seed)
        try:
            gen.set_task(self.task)
            features, labels = (t.cpu().numpy() for t in gen.generate(self.L, mask_ratio=self.mask_ratio))
            flags = gen.check_errors()
        finally:
            gen.close()
        if flags:
            raise _lib.XenoError("MetaLangV1: device error flags 0x%x (include/xeno.h XV_DEVERR_*)" % flags)
        return features, labels

    def data_generator(self, seed=None):
        """-> (features int32[L], labels int32[L])"""
        features, labels = self._generate(1, seed)
        return features[0], labels[0]

    def batch_generator(self, batch_size, seed=None):
        """-> (features, labels) int32[batch_size, L]: one launch"""
        return self._generate(batch_size, seed)

    def generate_text(self, size, output_stream, seed=None):
        """one line per sequence: tab-separated "feature,label" pairs (metalangv1.py:87-98)"""
        features, labels = self.batch_generator(size, seed=seed)
        need_close = isinstance(output_stream, str)
        stream = open(output_stream, "w") if need_close else (output_stream if output_stream is not None else sys.stdout)
        for f, l in zip(features.tolist(), labels.tolist()):
            stream.write("\t".join("%d,%d" % fl for fl in zip(f, l)))
            stream.write("\n")
        if need_close:
            stream.close()

    def generate_npy(self, size, file_name, seed=None):
        """int32[2, size, L] (features, labels) to file_name — the reference's own (metalangv1.py:100-102) saves to an
        undefined name `file` and raises NameError"""
        feas, labs = self.batch_generator(size, seed=seed)
        np.save(file_name, np.stack([feas, labs], axis=0))

    @property
    def VocabSize(self):
        return self.n_vocab

    @property
    def SepID(self):
        return 0

    @property
    def MaskID(self):
        return 0

    @property
    def PaddingID(self):
        return 0
