"""bench.py --dump-outputs on the host (no GPU): the ring slot of the last timed step goes to DIR/<name>.npy in float32, a
fixed seeded sample of the envs past the size cap, and the flag is refused where there is no step_many ring to dump."""
import os
import subprocess
import sys

import numpy as np
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ring(P, n):
    g = torch.Generator().manual_seed(0)
    return dict(obs=torch.randint(0, 64, (P, n), generator=g, dtype=torch.int32),
                reward=torch.randn((P, n), generator=g, dtype=torch.float32),
                reward_gt=torch.randn((P, n), generator=g, dtype=torch.float32),
                terminated=torch.randint(0, 2, (P, n), generator=g, dtype=torch.uint8),
                truncated=torch.randint(0, 2, (P, n), generator=g, dtype=torch.uint8),
                final_obs=torch.randint(-1, 64, (P, n), generator=g, dtype=torch.int32))


def test_dump_writes_the_slot_of_every_ring_array_in_float32(tmp_path):
    ring = _ring(4, 100)
    names = bench.dump_outputs(str(tmp_path), ring, 2)
    assert sorted(names) == sorted(ring)
    assert sorted(os.listdir(tmp_path)) == sorted(k + ".npy" for k in ring)
    for k, t in ring.items():
        a = np.load(tmp_path / (k + ".npy"))
        assert a.dtype == np.float32 and a.shape == (100,)
        assert np.array_equal(a, t[2].numpy().astype(np.float32)), k


def test_dump_past_the_cap_is_a_fixed_seeded_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 6 * 4 * 10 + 80)
    ring = _ring(3, 1000)
    total = 0
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), ring, 1, seed=7)
        total = sum(os.path.getsize(tmp_path / d / f) - 128 for f in os.listdir(tmp_path / d))   # (128-byte .npy header)
    assert total <= bench.DUMP_MAX_BYTES
    idx = np.load(tmp_path / "a" / "env_index.npy")
    assert idx.dtype == np.float64 and len(idx) == 10 and np.all(np.diff(idx) > 0)
    assert np.array_equal(idx, np.load(tmp_path / "b" / "env_index.npy"))
    for k, t in ring.items():
        a = np.load(tmp_path / "a" / (k + ".npy"))
        assert np.array_equal(a, t[1].numpy()[idx.astype(np.int64)].astype(np.float32)), k
        assert np.array_equal(a, np.load(tmp_path / "b" / (k + ".npy")))


def test_dump_is_refused_where_there_is_no_ring(tmp_path):
    for extra in (["--workload", "mixed"], ["--exchange-selftest"], ["--sweep-envs", "4096"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dump-outputs", str(tmp_path)] + extra,
                           capture_output=True, text=True, timeout=120, cwd=ROOT)
        assert r.returncode == 2 and "--dump-outputs" in r.stderr, (extra, r.stderr[-500:])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=120, cwd=ROOT)
    assert r.returncode == 2 and "--steps" in r.stderr
    assert os.listdir(tmp_path) == []
