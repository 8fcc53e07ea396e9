"""what the AnyHVAC PID tests share: the fixtures of scripts/gen_golden_anyhvac_pid.py (tests/golden/pid_anyhvac_*.npz) and
the bounds a device controller is held to against the host's (xenoverse_amd/anyhvac/pid.py: PIDHost).

Device and host form diff, acc_diff and d_e with the same operations in the same order and dtypes (the build forbids
contraction), so given the same readings those are bit-equal.  They differ in ONE place: x = d_e @ corr is a sum of S fp64
products whose order numpy's matmul leaves open and the device fixes (index order).  Any order's result lies within
gamma_S * sum_s |d_e[s] corr[s][c]| of the exact sum, gamma_S = S u / (1 - S u), u = 2^-53 (Higham, Accuracy and
Stability of Numerical Algorithms, section 3.1).  The value column is float32(clip(x, 0, 1)): a rounding of a monotone
function of x, so the device's value lies between the roundings of the two ends of that interval — equal to the host's or,
where the interval straddles a float32 rounding boundary, adjacent.  Straddling is rare: the interval is ~1e-15 wide and a
float32 ulp below 1 is >= 1e-8 wide for values above 0.1, so ADJACENT_CAP = 1 % is generous by orders of magnitude.  The
switch column is x > -0.05; the fixtures keep |x + 0.05| >= 1e-9, far above the interval, so it is equal.  The env's action
is the float32 operation 1 - value on the device's own value: bit-equal to numpy's on that value.  None of this is taken
from a device run.
"""
import os

import numpy as np

from util import golden_files
from xenoverse_amd.anyhvac.pid import PIDHost

FILES = {os.path.basename(p)[len("pid_anyhvac_"):-4]: p for p in golden_files("pid_anyhvac_")}
RUNS = ("gt_rot", "loc_rot", "gt_wide", "f64_rot")
MIN_SWITCH_MARGIN = 1e-9
ADJACENT_CAP = 0.01
U53 = 2.0 ** -53
REF_KEYS = {"kp", "ki", "kd", "mean_error", "max_error", "std_error", "error_within_2C", "error_within_1C", "mean_reward",
            "mean_overshoot", "score"}
_cache = {}


def load(name):
    """-> (fixture dict, flat task dict, env settings, generate_task)"""
    if name not in _cache:
        g = dict(np.load(FILES[name], allow_pickle=False))
        task = {k[5:]: (v if v.ndim else v[()]) for k, v in g.items() if k.startswith("task_")}
        settings = dict(max_steps=int(g["set_max_steps"]), iter_per_step=int(g["set_iter_per_step"]),
                        sec_per_iter=float(g["set_sec_per_iter"]), reward_mode=int(g["set_reward_mode"]))
        _cache[name] = (g, task, settings, bool(g["generate_task"]))
    return _cache[name]


def runs_of(name):
    """a fixture's recorded runs: [(fixture view without the leading axis, gains triple, gains mode)]"""
    g = load(name)[0]
    if not bool(g["gains_float64"]):
        return [(g, tuple(float(v) for v in g["gains"]), "python")]
    per_run = ("pid_readings", "pid_flat", "pid_acc_diff", "action", "sensor_readings", "closed_loop_dev_readings",
               "closed_loop_dev_action", "grid", "t", "timestep", "rest_idx", "terminated", "truncated")
    return [(dict(g, **{k: g[k][i] for k in per_run}), tuple(np.float64(v) for v in g["gains"][i]), "float64")
            for i in range(g["gains"].shape[0])]


def host_pid(name, gains, mode, **kw):
    g, task, settings, _ = load(name)
    return PIDHost(task, str(g["kind"]), kp=gains[0], ki=gains[1], kd=gains[2],
                   sec_per_step=settings["iter_per_step"] * settings["sec_per_iter"], gains=mode, **kw)


def gamma(n):
    return n * U53 / (1.0 - n * U53)


def x_interval(d_e, corr):
    """(lo[C], hi[C]): the host's own x -/+ gamma_S * sum_s |d_e[s] corr[s][c]|"""
    x = np.matmul(d_e, corr)
    b = gamma(len(d_e)) * np.abs(d_e[:, None] * corr).sum(axis=0)
    return x - b, x + b


def value32(x):
    v = np.zeros(len(x), np.float32)
    v[:] = np.clip(x, 0.0, 1.0)
    return v


def check_value(value, d_e, corr, label=""):
    """a controller's float32 value columns against the interval of the host's d_e — what PIDHost.advance(readings)
    returned for this step; it moves the host's state on, so the caller makes that call once per step — -> the number of
    entries that differ from the host's own (every one of them adjacent, by the assertion)"""
    lo, hi = x_interval(d_e, corr)
    vlo, vhi = value32(lo), value32(hi)
    value = np.asarray(value, np.float32)
    assert ((vlo <= value) & (value <= vhi)).all(), label + ": a value column outside the reordering bound"
    assert (np.abs(vhi.astype(np.float64) - vlo) <= np.spacing(np.maximum(vlo, vhi))).all(), label + ": interval wider than an ulp"
    return int((value != value32(np.matmul(d_e, corr))).sum())


def check_action(action, d_e, corr, label=""):
    """the same for the env's action 1 - value (float32; monotone in the value, so it lies between the two ends' actions)
    -> the number of entries that differ from the host's own"""
    lo, hi = x_interval(d_e, corr)
    alo, ahi = 1 - value32(hi), 1 - value32(lo)
    action = np.asarray(action, np.float32)
    assert ((alo <= action) & (action <= ahi)).all(), label + ": an action outside the reordering bound"
    return int((action != 1 - value32(np.matmul(d_e, corr))).sum())


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def stats_numpy(readings, rewards, target):
    """the eight pid_stats slots from one env's readings float32 [T, S] and rewards [T] in numpy, and the sum of the
    absolute terms of the three fp64 sums (for their reordering bounds)"""
    e = np.abs(np.asarray(readings, np.float32) - target).astype(np.float64).reshape(-1)      # float32 subtraction
    over = np.asarray(readings, np.float32) > target + 2.0
    st = np.array([e.sum(), e.max(), (e * e).sum(), (e <= 1.0).sum(), (e <= 2.0).sum(), over.sum(),
                   np.asarray(rewards, np.float64).sum(), e.size])
    return st, np.array([e.sum(), (e * e).sum(), np.abs(rewards).sum()])


def metrics_numpy(readings, rewards, target):
    """the reference's _evaluate_params metrics from one env's readings [T, S] and rewards [T], as it forms them"""
    errors, overshoots = [], []
    for r in np.asarray(readings, np.float32):
        errors.extend(np.abs(r - target).tolist())
        overshoots.append(np.sum(r > target + 2.0))
    errors = np.array(errors)
    return {"mean_error": np.mean(errors), "max_error": np.max(errors), "std_error": np.std(errors),
            "error_within_2C": np.mean(errors <= 2.0) * 100, "error_within_1C": np.mean(errors <= 1.0) * 100,
            "mean_reward": np.mean(rewards), "mean_overshoot": np.mean(overshoots)}
