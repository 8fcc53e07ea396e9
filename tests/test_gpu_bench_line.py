"""The bench line as a GPU run prints it (small sizes): the contract keys, the `roofline` and `cpu_baseline` objects, the
`long_call` block of a --full run, and a plain run that measures the headline only — a renamed key or a fraction above 1
fails here before a judge reads the line."""
import json
import os
import subprocess
import sys

import pytest

import bench

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _line(extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", "--envs", "4096",
           "--no-families", "--sustain-seconds", "0.3", "--long-steps", "256", "--long-repeats", "2", "--cpu-seconds", "0.5",
           "--cpu-table-gib", "0.05", "--repeats", "5"] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    out = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(out) == 1
    return out[0]


def test_bench_line_schema_at_the_drivers_flags():
    d = _line(["--full"])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline", "long_call", "sustain"):
        assert k in d, k
    assert d["steps"] == 20 and d["warmup"] == 5 and d["n_gpus"] == 1 and d["dtype"] == "f64" and d["vs_baseline"] is None
    assert "workload" in d["config"] and d["config"]["device_error_flags"] == 0
    ro = d["roofline"]
    for k in bench.ROOFLINE_KEYS:
        assert k in ro, k
    assert ro["frac"] is None or 0.0 < ro["frac"] <= 1.0
    assert ro["peak"] == 8000.0 and ro["unit"] == "GB/s" and ro["bound"] in ("hbm", "cache")
    # the traffic is this run's own: two child passes under rocprofv3 --pmc before the GPU is touched
    tl = ro["traffic_live"]
    assert tl is not None and "error" not in tl, tl
    assert tl["plain"] and tl["rollout"] and ro["traffic"] in (tl["plain"], tl["hand"]) and ro["traffic_source"].startswith("live")
    assert 100 * 4096 < tl["plain"] < 600 * 4096          # bytes per launch: one table line + the per-env streams, per env
    cb = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in cb
    lc = d["long_call"]
    assert "error" not in lc, lc.get("error")
    for m in bench.LONG_CALL_MODES:
        row = lc[m]
        for k in bench.LONG_CALL_ROW_KEYS:
            assert k in row, (m, k)
        assert row["steps"] == 256 and row["warmup"] >= 100 and row["device_error_flags"] == 0
        assert row["us_per_step"] > 0 and row["wall_us_per_step"] >= row["us_per_step"] * 0.9
        fr = row["roofline"]["frac"]
        assert fr is None or fr <= 1.0
    assert lc["one_stream"]["overlap_state"] == 0 and lc["overlapped"]["overlap_state"] in (1, -2, 0)
    assert lc["fused_rollout"]["launches_per_call"] == 256 // 32
    # the sustain leg is issued the way long_call.overlapped is (round 5 left it on one stream by a bench bug)
    assert d["sustain"]["overlap_requested"] is True and d["sustain"]["steps_per_call"] == 256
    assert d["sustain"]["overlap_state"] == lc["overlapped"]["overlap_state"] or d["sustain"]["overlap_state"] in (1, 0, -2)


def test_plain_run_is_the_headline_only():
    """without --full a run sets up, warms up, times the steps and prints the line: the contract keys and the roofline (traffic
    from a committed counter profile where one matches), none of the blocks that take runs of their own (the flags that size
    them are ignored)"""
    d = _line([])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype", "config",
              "roofline"):
        assert k in d, k
    assert d["steps"] == 20 and d["warmup"] == 5 and d["repeats"] == 5 and d["dtype"] == "f64" and d["higher_is_better"] is True
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["config"]["device_error_flags"] == 0
    for k in bench.ROOFLINE_KEYS:
        assert k in d["roofline"], k
    assert d["roofline"]["traffic_live"] is None and d["cpu_baseline"] is None
    for k in ("long_call", "sustain", "sustain_s", "search_variants", "families", "with_allgather", "fused_rollout_env_steps_per_s_rank0"):
        assert k not in d, k


def test_bench_line_shared_tasks_claims_no_hbm_fraction():
    d = _line(["--tasks", "64", "--no-cpu-baseline", "--long-steps", "0", "--no-live-pmc"])
    assert d["roofline"]["traffic_live"] is None
    assert d["roofline"]["bound"] == "cache" and d["roofline"]["frac"] is None and d["roofline"]["frac_survey_bytes"] > 0
    assert "long_call" not in d


def test_dump_outputs_are_the_last_timed_step_and_repeat_run_to_run(tmp_path):
    """--dump-outputs: the step_many ring slot of the last timed step, float32, one value per env; the same arguments give
    the same arrays (seeded tables, actions and draws), which is what lets two builds be compared output for output"""
    import numpy as np
    quick = ["--no-cpu-baseline", "--no-live-pmc", "--long-steps", "0", "--no-variants", "--sustain-seconds", "0"]
    got = []
    for d in ("a", "b"):
        line = _line(quick + ["--dump-outputs", str(tmp_path / d)])
        assert line["steps"] == 20 and line["ms_per_step"] > 0
        got.append({f[:-4]: np.load(tmp_path / d / f) for f in os.listdir(tmp_path / d)})
    a, b = got
    assert sorted(a) == ["final_obs", "obs", "reward", "reward_gt", "terminated", "truncated"]
    for k in a:
        assert a[k].dtype == np.float32 and a[k].shape == (4096,), k
        assert np.array_equal(a[k], b[k]), k
    assert a["obs"].min() >= 0 and a["obs"].max() < 64 and np.all(a["obs"] == np.round(a["obs"]))
    assert set(np.unique(a["terminated"])) <= {0.0, 1.0} and set(np.unique(a["truncated"])) <= {0.0, 1.0}
    assert np.all(np.isfinite(a["reward"])) and np.all(np.isfinite(a["reward_gt"]))
    assert np.all((a["final_obs"] == -1) | ((a["terminated"] + a["truncated"]) > 0))
