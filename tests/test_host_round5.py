"""Host-side pieces added in round 5 (no GPU): output slabs, the device table builder's eligibility rule, the rendezvous
store selection of the RCCL communicator, the mixed workload's fabricated records."""
import ctypes as C
import os
import sys

import numpy as np
import torch

from xenoverse_amd.anymdp.tables import device_buildable
from xenoverse_amd.vector import OutputSlabs, StepOutputs


def test_output_slabs_hand_out_disjoint_tensors_with_matching_pointers():
    fields = [("obs", torch.int32, ()), ("steps", torch.int32, ()), ("reward", torch.float32, ()), ("frame", torch.float32, (3, 2)),
              ("term", torch.uint8, ()), ("done", torch.uint8, ())]
    sl = OutputSlabs(fields, 7, "cpu", K=4, as_bool=("term", "done"), order=("obs", "reward", "term", "frame"))
    seen, kept = set(), []
    for step in range(11):                       # three slabs
        t, p = sl.next()
        assert [x.value for x in p] == [t[k].data_ptr() for k in ("obs", "reward", "term", "frame")]
        assert t["obs"].shape == (7,) and t["frame"].shape == (7, 3, 2) and t["term"].dtype == torch.bool
        for k, v in t.items():
            lo = v.data_ptr()
            span = (lo, lo + v.numel() * v.element_size())
            for a, b in seen:                    # no tensor overlaps any tensor handed out before
                assert span[1] <= a or span[0] >= b, (step, k)
            seen.add(span)
            v.fill_(1 if v.dtype == torch.bool else step + 1)
        kept.append(t)
    for step, t in enumerate(kept):              # what a step got is never written again
        assert int(t["obs"][0]) == step + 1 and float(t["frame"][6, 2, 1]) == step + 1 and bool(t["done"][3])


def test_output_slabs_are_recycled_only_when_nobody_can_reach_them():
    """round 6: a used-up slab is handed out again — the same tensor objects — once no Python reference, no C++ holder (DLPack)
    and no alias of its storage (view, detach, numpy) is left; anything the caller still holds keeps its values"""
    import torch.utils.dlpack as dl
    fields = [("obs", torch.int32, ()), ("reward", torch.float32, ()), ("term", torch.uint8, ())]
    sl = OutputSlabs(fields, 5, "cpu", K=4, as_bool=("term",), order=("obs", "reward", "term"))
    last = None
    ids = set()
    for step in range(48):                       # the usual loop: only the latest observation is kept
        t, p = sl.next()
        t["obs"].fill_(step)
        last = t["obs"]
        ids.add(id(t["obs"]))
    assert sl.made == 2 and sl.recycled == 10 and len(ids) == 8      # two slabs alternate: no new objects after the first two
    assert int(last[0]) == 47
    holders = {}
    for step in range(64):
        t, p = sl.next()
        for k, v in t.items():
            v.fill_(1 if v.dtype == torch.bool else step + 100)
        if step == 3:
            holders["tensor"] = (t["reward"], lambda x: float(x[0]), 103.0)
        if step == 9:
            holders["view"] = (t["obs"][1:3], lambda x: int(x[0]), 109)
        if step == 14:
            holders["detach"] = (t["reward"].detach(), lambda x: float(x[4]), 114.0)
        if step == 21:
            holders["numpy"] = (t["obs"].numpy(), lambda x: int(x[2]), 121)
        if step == 26:
            holders["dlpack"] = (dl.to_dlpack(t["obs"]), None, 126)
    for _ in range(64):                          # plenty of further steps: every free slab is recycled and overwritten
        t, p = sl.next()
        for v in t.values():
            v.fill_(0)
    for name, (h, get, want) in holders.items():
        if name == "dlpack":
            h = dl.from_dlpack(h)
            get = lambda x: int(x[0])           # noqa: E731
        assert get(h) == want, name
    made = sl.made
    holders.clear()
    del h
    for _ in range(64):
        sl.next()
    assert sl.made == made                       # once the holders are gone their slabs serve again: nothing new is allocated


_FIELDS = [("obs", torch.float32, (4,)), ("fobs", torch.float32, (4,)), ("final", torch.int32, (), -1), ("reward", torch.float32, ()),
           ("term", torch.uint8, ()), ("done", torch.uint8, ())]
_ORDER = ("obs", "reward", "term", "fobs", "final", "done")


def _step_outputs(**kw):
    return StepOutputs(_FIELDS, 5, "cpu", _ORDER, as_bool=("term", "done"), zero_on_refill=("fobs",),
                       derived={"obs_u": ("obs", lambda t: t[:, :3]), "first": ("fobs", lambda t: t[:, 0])}, **kw)


def _check_set(s):
    """pointers by name, in the C call's order, and views: all of one set agree"""
    names = [f[0] for f in _FIELDS]
    for k in names:
        assert s.ptr[k] == s.t[k].data_ptr(), k
    assert s.ints == tuple(s.ptr[k] for k in _ORDER)
    assert tuple(p.value for p in s.args) == s.ints
    assert s.t["term"].dtype == torch.bool and s.t["done"].dtype == torch.bool and s.t["reward"].dtype == torch.float32
    assert s.t["obs"].shape == (5, 4) and s.t["obs_u"].shape == (5, 3) and s.t["first"].shape == (5,)
    s.t["obs"].fill_(3.0); s.t["fobs"].fill_(4.0)
    assert s.t["obs_u"].data_ptr() == s.ptr["obs"] and float(s.t["obs_u"][4, 2]) == 3.0      # derived views alias their field
    assert s.t["first"].data_ptr() == s.ptr["fobs"] and float(s.t["first"][4]) == 4.0
    raw = torch.frombuffer((C.c_uint8 * 5).from_address(s.ptr["term"]), dtype=torch.uint8)
    s.t["term"].fill_(True)
    assert raw.tolist() == [1] * 5                                                           # a bool view aliases its bytes


def test_persistent_output_sets_alternate_hold_and_start_filled():
    so = _step_outputs(copy=False, n_sets=2)
    assert so.persistent
    a, b = so.next(), so.next()
    assert a is not b
    for s in (a, b):                                  # a fresh set: zeros, and the fill value where one is declared
        assert int(s.t["final"].min()) == -1 == int(s.t["final"].max())
        assert float(s.t["obs"].abs().max()) == 0.0 and float(s.t["fobs"].abs().max()) == 0.0 and not bool(s.t["done"].any())
        _check_set(s)
    seq = [so.next() for _ in range(6)]
    assert [x is a for x in seq] == [True, False] * 3 and all(x is a or x is b for x in seq)
    for k in [f[0] for f in _FIELDS]:                  # every field's memory repeats with period 2
        p = [x.t[k].data_ptr() for x in seq]
        assert p[0] != p[1] and p == p[:2] * 3, k
    so.hold(True)
    held = [so.next() for _ in range(5)]
    assert all(x is held[0] for x in held) and held[0] is a          # the set that was next stays
    so.hold(False)
    seq = [so.next() for _ in range(4)]
    assert seq[0] is a and seq[1] is b and seq[2] is a and seq[3] is b
    a.t["fobs"].fill_(7.0)                            # copy=False: a zero_on_refill field keeps what the caller (a step) left there
    assert [so.next() is a for _ in range(3)] == [True, False, True] and float(a.t["fobs"].min()) == 7.0


def test_one_persistent_output_set_is_the_same_objects_every_time():
    so = _step_outputs(copy=False)
    s = so.next()
    t = dict(s.t)
    _check_set(s)
    for _ in range(5):
        s2 = so.next()
        assert s2 is s and all(s2.t[k] is v for k, v in t.items())
    so.hold(True)
    assert so.next() is s
    so.hold(False)
    assert so.next() is s


def test_to_numpy_output_set_zeroes_partly_written_fields_before_every_step():
    so = _step_outputs(copy=True, to_numpy=True, n_sets=2)      # to_numpy: one set whatever copy and n_sets say
    assert so.persistent
    s = so.next()
    _check_set(s)
    for k in range(4):
        s2 = so.next()
        assert s2 is s
        assert float(s.t["fobs"].abs().max()) == 0.0 and float(s.t["first"].abs().max()) == 0.0
        assert float(s.t["obs"].min()) == 3.0                        # (only the declared fields are cleared)
        s.t["fobs"].fill_(k + 1.0)                                   # what a step would leave behind


def test_copy_true_output_sets_come_from_slabs():
    so = _step_outputs(copy=True, K=4)
    assert not so.persistent
    seen, kept = set(), []
    for step in range(11):                            # three slabs
        s = so.next()
        assert float(s.t["fobs"].abs().max()) == 0.0                 # zeroed once per slab, before any of its sets is handed out
        _check_set(s)
        assert s.ptr["obs"] not in seen
        seen.add(s.ptr["obs"])
        s.t["obs"].fill_(step)
        kept.append(s.t["obs"])
    so.hold(True)                                     # nothing to pin: every step still gets memory of its own
    assert so.next().ptr["obs"] not in seen
    for step, t in enumerate(kept):
        assert float(t[4, 3]) == step


def test_device_buildable_rule():
    def task(n, a, extra=None):
        d = dict(transition=np.zeros((n, a, n)), reward=np.zeros((n, a, n)), reward_noise=np.zeros((n, a, n)), na=a)
        d.update(extra or {})
        return d
    assert device_buildable([task(8, 3), task(8, 3)])
    assert not device_buildable([task(8, 3), task(9, 3)])            # ragged: host builder pads
    assert not device_buildable([task(1, 3)])                        # bandits are embedded by the host builder
    assert not device_buildable([task(8, 3, {"na": 4})])
    assert not device_buildable(task(8, 3)) and not device_buildable([])
    assert not device_buildable([task(8, 3, {"reward": np.zeros((8, 3, 7))})])


def test_rendezvous_store_prefers_the_callers_store():
    from xenoverse_amd.distributed import _rendezvous_store

    class Store(dict):
        def set(self, k, v):
            self[k] = v

        def get(self, k):
            return self[k]
    st = Store()
    assert _rendezvous_store(0, 2, st, None, None, 5) is st


def test_mixed_workload_fabricated_records_are_functions_of_global_ids():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    import bench_mixed
    from xenoverse_amd.distributed import MixedChunk
    ch = MixedChunk(4, 256, 128, 64, 2)
    whole = bench_mixed.fabricate(torch, ch, 4, {"anymdp": (0, 256), "linds": (0, 128), "cartpole": (0, 64)})
    for r in range(2):
        part = bench_mixed.fabricate(torch, ch, 4, {f: ch.share[f][r] for f in ch.rec})
        for f in ch.rec:
            lo, hi = ch.share[f][r]
            for k in part[f]:
                assert torch.equal(part[f][k], whole[f][k][:, lo:hi]), (f, k)
    assert ch.bytes_per_rank == 4 * (128 * 8 + 64 * 72 + 32 * 24)


def test_profile_hash_covers_the_kernel_section_only(tmp_path, monkeypatch):
    """xenoverse_amd.build.source_hash ties a committed counter profile to the KERNEL source it measured: a .hip file counts
    up to its `#ifndef XV_KERNELS_ONLY` line, headers whole — host-side edits behind the marker leave the hash alone"""
    from xenoverse_amd import build as xb
    d = tmp_path / "csrc"
    d.mkdir()
    (d / "k.hip").write_text("__global__ void k() {}\n#ifndef XV_KERNELS_ONLY\nint host_a;\n#endif\n")
    (d / "h.h").write_text("#define X 1\n")
    monkeypatch.setattr(xb, "CSRC", str(d))
    h0 = xb.source_hash(("k.hip", "h.h"))
    (d / "k.hip").write_text("__global__ void k() {}\n#ifndef XV_KERNELS_ONLY\nint host_b; int more;\n#endif\n")
    assert xb.source_hash(("k.hip", "h.h")) == h0                      # host part changed: same hash
    (d / "k.hip").write_text("__global__ void k() { }\n#ifndef XV_KERNELS_ONLY\nint host_b;\n#endif\n")
    assert xb.source_hash(("k.hip", "h.h")) != h0                      # kernel part changed
    (d / "k.hip").write_text("__global__ void k() {}\n#ifndef XV_KERNELS_ONLY\nint host_a;\n#endif\n")
    (d / "h.h").write_text("#define X 2\n")
    assert xb.source_hash(("k.hip", "h.h")) != h0                      # a header counts whole
    # the committed profile of the step kernel is keyed to the source in the tree
    monkeypatch.undo()
    import json, glob, os
    import bench
    prof = sorted(glob.glob(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r0*pmc_traffic_anymdp_2a*.json")))
    assert prof and json.load(open(prof[-1]))["bench_key"]["kernel_source_sha16"] == bench.kernel_source_hash()
