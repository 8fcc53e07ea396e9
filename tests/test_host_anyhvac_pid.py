"""The AnyHVAC PID teachers without a GPU: pid.py (pid_weights, PIDHost, pid_search_host) against the reference's recorded
closed-loop runs (tests/golden/pid_anyhvac_*.npz, scripts/gen_golden_anyhvac_pid.py), bit for bit."""
import itertools

import numpy as np
import pytest

import anyhvac_pid_util as PU
from xenoverse_amd.anyhvac.pid import (PIDHost, evaluate_host, first_strict_minimum, pid_search_host, pid_weights,
                                       search_score)
from xenoverse_amd.anyhvac.host import HVACHost


def test_every_fixture_is_there_with_its_margins():
    assert sorted(PU.FILES) == sorted(PU.RUNS)
    for name in PU.RUNS:
        g = PU.load(name)[0]
        assert float(np.min(g["switch_margin"])) >= PU.MIN_SWITCH_MARGIN, name
        assert not g["terminated"].any() and not g["truncated"].any(), name
        assert (g["action"][..., 0, :] == 1.0).all(), name      # the derivative kick of the first call saturates


@pytest.mark.parametrize("name", PU.RUNS)
def test_weights_are_the_recorded_matrices(name):
    g, task, _, _ = PU.load(name)
    w = pid_weights(task, str(g["kind"]))
    assert PU.same_bits(w, g["weights"])
    assert w.shape == (len(task["sensor_loc"]), len(task["cooler_loc"]))
    other = pid_weights(task, "loc" if str(g["kind"]) == "gt" else "gt")
    assert not np.array_equal(other, w) and np.abs(other.sum(axis=1) - 1).max() < 1e-12
    with pytest.raises(ValueError):
        pid_weights(task, "nearest")


@pytest.mark.parametrize("name", PU.RUNS)
def test_host_controller_replays_the_reference(name):
    """fed the recorded readings: the recorded flat actions and acc_diff, bit for bit; the other gains path gives other
    pre-clip values"""
    for g, gains, mode in PU.runs_of(name):
        pid = PU.host_pid(name, gains, mode)
        assert type(pid.kp) is (float if mode == "python" else np.float64)
        other = PU.host_pid(name, gains, "float64" if mode == "python" else "python")
        differs = False
        for k in range(int(g["n_steps"])):
            flat = pid.policy(g["pid_readings"][k])
            assert flat.dtype == np.float32 and PU.same_bits(flat, g["pid_flat"][k]), (name, k)
            assert PU.same_bits(pid.acc_diff, g["pid_acc_diff"][k]), (name, k)
            C = pid.n_coolers
            assert PU.same_bits(1 - flat[C:], g["action"][k])
            other.policy(g["pid_readings"][k])
            differs = differs or not PU.same_bits(other.last_x, pid.last_x)
        assert differs, "the two gains paths must round differently somewhere on " + name


def test_reset_gives_a_fresh_solvers_first_call():
    g, gains, mode = PU.runs_of("gt_rot")[0]
    pid = PU.host_pid("gt_rot", gains, mode)
    first = pid.policy(g["pid_readings"][0])
    for k in range(1, 5):
        pid.policy(g["pid_readings"][k])
    assert pid.acc_diff.any() and pid.last_observation.any()
    pid.reset()
    assert not pid.acc_diff.any() and pid.last_observation.dtype == np.float32 and not pid.last_observation.any()
    assert PU.same_bits(pid.policy(g["pid_readings"][0]), first) and PU.same_bits(first, g["pid_flat"][0])
    with pytest.raises(ValueError):
        pid.policy(g["pid_readings"][0].astype(np.float64))


@pytest.mark.parametrize("name", PU.RUNS)
def test_reversed_summation_stays_inside_the_bound_and_the_cap(name):
    """the bound the device is held to (anyhvac_pid_util.py), tried on the CPU with the opposite order of summation"""
    adjacent = total = 0
    for g, gains, mode in PU.runs_of(name):
        pid = PU.host_pid(name, gains, mode)
        corr = pid.corr_sensor_cooler
        for k in range(int(g["n_steps"])):
            d_e = pid.advance(g["pid_readings"][k])
            x = np.zeros(corr.shape[1])
            for s in range(len(d_e) - 1, -1, -1):
                x = x + d_e[s] * corr[s]
            adjacent += PU.check_value(PU.value32(x), d_e, corr, "%s step %d" % (name, k + 1))
            total += corr.shape[1]
            assert np.array_equal(x > -0.05, g["pid_flat"][k][:corr.shape[1]] > 0)
    assert adjacent <= PU.ADJACENT_CAP * total, (adjacent, total)


def test_score_is_the_formula_and_the_first_strict_minimum_wins():
    m = dict(mean_error=1.5, error_within_2C=80.0, max_error=4.0)
    assert search_score(m) == 0.5 * 1.5 + 0.3 * (100 - 80.0) / 10 + 0.2 * 4.0
    # a hand-made tie: candidates 1 and 5 share the lowest score; product order decides
    table = {c: dict(mean_error=2.0, error_within_2C=50.0, max_error=3.0, std_error=0.0, error_within_1C=0.0, mean_reward=0.0,
                     mean_overshoot=0.0) for c in itertools.product((1.0, 2.0), (3.0, 4.0), (5.0, 6.0))}
    for c in ((1.0, 3.0, 6.0), (2.0, 3.0, 6.0)):
        table[c] = dict(table[c], mean_error=1.0)
    best, results = pid_search_host(None, (1.0, 2.0), (3.0, 4.0), (5.0, 6.0), 0,
                                    evaluate=lambda kp, ki, kd: dict(table[(kp, ki, kd)], kp=kp, ki=ki, kd=kd))
    assert [(r["kp"], r["ki"], r["kd"]) for r in results] == list(itertools.product((1.0, 2.0), (3.0, 4.0), (5.0, 6.0)))
    assert (best["kp"], best["ki"], best["kd"]) == (1.0, 3.0, 6.0) and set(best) == PU.REF_KEYS
    assert all(r["score"] == search_score(r) for r in results)
    assert first_strict_minimum(results)["score"] == min(r["score"] for r in results)


def test_host_search_runs_every_candidate_from_the_same_grid():
    """2 x 2 x 2 on the rot room, 3 steps of 50 iterations: the metrics are the reference's expressions over the run a
    PIDHost with those numpy.float64 gains makes from the given grid"""
    g, task, settings, gen = PU.load("f64_rot")
    kp, ki, kd = np.linspace(1e-3, 5e-2, 2), np.linspace(1e-2, 1e-1, 2), np.linspace(1e-3, 2e-2, 2)
    best, results = pid_search_host(task, kp, ki, kd, 3, settings=settings, init_grid=g["init_grid"], generate_task=True)
    assert len(results) == 8 and set(best) == PU.REF_KEYS and all(type(r["kp"]) is np.float64 for r in results)
    assert best["score"] == min(r["score"] for r in results)
    env = HVACHost(**settings)
    env.set_task(task, generate_task=True)
    sec = settings["iter_per_step"] * settings["sec_per_iter"]
    mine = evaluate_host(env, PIDHost(task, kp=kp[1], ki=ki[0], kd=kd[1], sec_per_step=sec, gains="float64"), g["init_grid"], 3)
    assert all(mine[k] == results[5][k] for k in mine)
    assert 0.0 <= mine["error_within_1C"] <= mine["error_within_2C"] <= 100.0 and mine["max_error"] >= mine["mean_error"]
