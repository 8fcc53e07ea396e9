"""AnyHVAC without a GPU: the sampler port and the host restatement against the reference's recorded tasks and runs
(tests/golden/anyhvac_*.npz, scripts/gen_golden_anyhvac.py), bit for bit; the padded device tables; the settings that are
not built."""
import os
import random

import numpy as np
import pytest

import anyhvac_util as U
from xenoverse_amd.anyhvac import HVACTaskSampler, wind_diffuser
from xenoverse_amd.anyhvac.host import HVACHost, check_ring
from xenoverse_amd.anyhvac.tables import build_tables, task_doubles


def test_every_fixture_is_there_with_its_margins():
    assert sorted(U.FILES) == sorted(U.RUNS + U.TASKS_ONLY)
    for name in U.RUNS:
        g = U.load(name)[0]
        assert float(g["eer_margin"]) >= U.MIN_EER_MARGIN and float(g["fail_margin"]) >= U.MIN_FAIL_MARGIN, name
    for name in U.FULL_SIZE:
        assert os.path.getsize(U.FILES[name]) <= U.SIZE_CAP, name


@pytest.mark.parametrize("name", U.TASKS_ONLY + U.RUNS)
def test_sampler_port_returns_the_reference_task(name):
    g, task, _, _ = U.load(name)
    seed = int(g["seed"])
    np.random.seed(seed)
    random.seed(seed)
    mine = HVACTaskSampler(config=U.sampler_config(g) if name in U.RUNS else None)
    assert set(mine) == set(task)
    for k in task:
        assert U.same_bits(mine[k], g["task_" + k]), k
    if name == "task_s0":
        assert (mine["n_width"], mine["n_length"], len(mine["cooler_loc"])) == (10, 5, 21)
    if name == "task_s1":
        assert (mine["n_width"], mine["n_length"], len(mine["cooler_loc"])) == (10, 13, 16)


def test_one_cooler_room_raises_as_the_reference_does():
    np.random.seed(5)
    random.seed(5)
    with pytest.raises(ValueError):
        HVACTaskSampler(config=dict(ROOM_W_GRID_SIZE_LOW=5, ROOM_W_GRID_SIZE_HIGH=6, ROOM_L_GRID_SIZE_LOW=5,
                                    ROOM_L_GRID_SIZE_HIGH=6, CELL_SIZE_LOW=1.0, CELL_SIZE_HIGH=1.05))


@pytest.mark.parametrize("name", ("trunc", "wide", "task_s1"))
def test_wind_diffuser_gives_the_recorded_matrices(name):
    task = U.load(name)[1]
    walls = task["convection_coeffs"] < 5.0
    for i, loc in enumerate(task["cooler_loc"]):
        d, v = wind_diffuser(walls, loc, float(task["cell_size"]), task["cooler_cooler_diffuse_sigma"][i])
        assert U.same_bits(d, task["cooler_diffuse"][i]) and U.same_bits(v, task["cooler_vent_diffuse"][i]), i
    for i, loc in enumerate(task["heater_loc"][:40]):
        d, _ = wind_diffuser(walls, loc, float(task["cell_size"]), task["heater_diffuse_sigma"][i])
        assert U.same_bits(d, task["heat_diffuse"][i]), i


@pytest.mark.parametrize("name", U.RUNS)
def test_host_replays_the_reference_bit_for_bit(name):
    g, task, settings, gen = U.load(name)
    host = HVACHost(**settings)
    host.set_task(task, generate_task=gen)
    assert np.float64(host.avg_total_heat) == g["avg_total_heat"]
    host.reset(g["init_grid"])
    n = int(g["n_steps"])
    for k in range(n):
        obs, r, term, trunc, info = host.step(g["action"][k])
        got = dict(grid=host.state, t=np.float64(host.t), reward=np.float64(r), terminated=np.bool_(term),
                   truncated=np.bool_(trunc), cool_power=info["cool_power"], heat_power=info["heat_power"],
                   rest_idx=np.int32(host.rest_idx), warning_count=np.int32(host.warning_count),
                   energy_cost=np.float64(info["energy_cost"]), target_cost=np.float64(info["target_cost"]),
                   sensor_readings=obs["sensor_readings"], heat_readings=obs["heat_readings"], action_temp=obs["action_temp"],
                   timestep=obs["timestep"][0])
        for q, v in got.items():
            assert U.same_bits(v, g[q][k]), "%s at step %d" % (q, k + 1)
    assert float(host.eer_margin) == float(g["eer_margin"])
    if name == "rot":      # the first rotation of the resting cooler: 122 steps of 30 s are the first MORE than 3600 s
        assert list(g["rest_idx"][:121]) == [0] * 121 and list(g["rest_idx"][121:]) == [1] * (n - 121)
    if name == "hot":
        assert n == 11 and g["terminated"][10] and g["reward"][10] == -30 and not g["terminated"][:10].any()
        assert list(g["warning_count"]) == [0] * 5 + [1, 2, 3, 4, 5, 6]
    if name == "trunc":
        assert n == 8 and g["truncated"][7] and not g["truncated"][:7].any()
    if name in ("mode1", "mode2"):
        assert list(g["t"]) == [10.0 * (k + 1) for k in range(n)]
    if name in U.FULL_SIZE:      # what these two are for: every lane-strided loop of the step kernel takes a second pass
        assert host.nw * host.nl == {"full": 225, "max": 256}[name] and n == 4
        assert host.n_coolers > 256 and host.n_sensors > 256 and host.n_heaters > 256


def test_host_raises_on_nan_like_the_reference():
    g, task, settings, gen = U.load("trunc")
    nan = np.full_like(task["cooler_cooler_eer_base"], np.nan)
    bad = dict(task, cooler_cooler_eer_base=nan, cooler_cooler_eer_reverse=nan)
    host = HVACHost(**settings)
    host.set_task(bad, generate_task=True)
    host.reset(g["init_grid"])
    with pytest.raises(ValueError, match="NaN"):
        host.step(g["action"][0])


def test_padding_of_a_mixed_batch_keeps_the_true_counts():
    small, wide = U.load("trunc")[1], U.load("wide")[1]
    tab = build_tables([small, wide], generate_task=True)
    NW, NL, C, S, H, KS, KH = tab["dims"]
    assert (NW, NL, C, S, H) == (9, 11, 92, 111, 202)
    assert tab["table"].shape == (2, task_doubles(*tab["dims"]))
    assert [(c["nw"], c["nl"], c["C"], c["S"], c["H"]) for c in tab["counts"]] == [
        (5, 7, len(small["cooler_loc"]), len(small["sensor_loc"]), len(small["heater_loc"])), (9, 11, 92, 111, 202)]
    for row, t in zip(tab["table"], (small, wide)):
        nw, nl = int(t["n_width"]), int(t["n_length"])
        assert list(row[:5]) == [nw, nl, len(t["cooler_loc"]), len(t["sensor_loc"]), len(t["heater_loc"])]
        assert row[10] == 10000 and row[15] == float(t["target_temperature"]) + 6
        nwall = (NW + 1) * (NL + 1) * 2
        chtc = row[16 + 3 * KH:16 + 3 * KH + nwall].reshape(NW + 1, NL + 1, 2)
        assert np.array_equal(chtc[:nw + 1, :nl + 1], t["convection_coeffs"])
        assert not chtc[nw + 1:].any() and not chtc[:, nl + 1:].any()
        cd = row[len(row) - C * nwall - C * NW * NL:len(row) - C * nwall].reshape(C, NW, NL)
        n = len(t["cooler_loc"])
        assert np.array_equal(cd[:n, :nw, :nl], t["cooler_diffuse"]) and not cd[n:].any() and not cd[:, nw:].any()
        cv = row[len(row) - C * nwall:].reshape(C, NW + 1, NL + 1, 2)
        assert np.array_equal(cv[:n, :nw + 1, :nl + 1], t["cooler_vent_diffuse"]) and not cv[n:].any()


@pytest.mark.parametrize("setting", [dict(no_switch_action=False), dict(action_space_format="dict"),
                                     dict(include_switch_in_observation=True), dict(return_normilized_obs=True),
                                     dict(random_start_t=True), dict(generate_record=True),
                                     dict(overheat_no_termiated_training_only=True), dict(control_type="Power")])
def test_excluded_settings_raise_and_name_the_setting(setting):
    from xenoverse_amd.anyhvac import HVACVecEnv
    name = next(iter(setting))
    with pytest.raises(ValueError, match=name):
        HVACHost(**setting)
    with pytest.raises(ValueError, match=name):      # (raised before the device is touched)
        HVACVecEnv(1, **setting)


def test_power_control_is_refused_by_the_sampler_and_by_set_task():
    with pytest.raises(ValueError, match="control_type"):
        HVACTaskSampler(control_type="Power")
    task = dict(U.load("trunc")[1], control_type="Power")
    with pytest.raises(ValueError, match="control_type"):
        HVACHost().set_task(task)
    with pytest.raises(ValueError, match="control_type"):
        build_tables([task])


def test_ring_capacity_check_raises_at_a_tenth_of_a_second():
    task = U.load("wide")[1]
    assert task["cooler_delay_seconds"].max() > 25.4      # 25.4 / 0.1 + 2 = 256
    with pytest.raises(ValueError, match="sec_per_iter"):
        HVACHost(sec_per_iter=0.1).set_task(task, generate_task=True)
    check_ring(task["cooler_delay_seconds"], 0.12)      # the delay is at most 30 s: 0.12 always fits
    check_ring(np.array([30.0]), 0.12)


def _replay_from_table(row, dims, settings, g):
    """a step loop that knows NOTHING but one task's device table in the layout include/xeno.h documents, with the kernel's
    data structures (padded strides, one ring of time stamps per env, a ring of values and a head per cooler): numpy's
    exp / sin / cos in the host's order, so grid, t, sensor readings and cool_power must be the recording's bit for bit"""
    NW, NL, C, S, H, KS, KH = dims
    NC, NWALL, R = NW * NL, (NW + 1) * (NL + 1) * 2, 256
    sc, base, chtc, hc, sens, heat, hd, cool, cd, cv = np.split(row, np.cumsum(
        [16, 3 * KH, NWALL, NC, S * (8 + 3 * KS), H * (4 + 3 * KH), H * NC, C * 24, C * NC]))
    nw, nl, nC, nS, nH = (int(v) for v in sc[:5])
    sens, heat, cool = sens.reshape(S, -1), heat.reshape(H, -1), cool.reshape(C, 24)
    hd, cd, cv = hd.reshape(H, NC), cd.reshape(C, NC), cv.reshape(C, NWALL)
    amb, csa, fcc_area = sc[8], sc[5] * sc[6], sc[7] * (sc[5] * sc[5])
    dt, iters = settings["sec_per_iter"], settings["iter_per_step"]
    cells = [(i, j, i * NL + j) for i in range(nw) for j in range(nl)]

    def series(r, K, n, x):
        y = 0.0
        for j in range(int(n)):
            y = y + (r[K + j] * np.sin(r[j] * x) + r[2 * K + j] * np.cos(r[j] * x))
        return y

    def curve(hb, period, n, r, t):
        return min(hb + max(series(r, KH, n, t / period), 0.0), 20000.0)

    def heater(h, t):
        r = heat[h]
        return r[0] * curve(sc[11], sc[12], sc[13], base, t) + (1.0 - r[0]) * curve(r[1], r[2], r[3], r[4:], t)

    def read(grid, r):
        at = lambda a, b: grid[int(a) * NL + int(b)]  # noqa: E731
        k0, k1 = r[4], r[5]
        return (at(r[0], r[1]) * (1.0 - k0) * (1.0 - k1) + at(r[2], r[1]) * k0 * (1.0 - k1)
                + at(r[0], r[3]) * (1.0 - k0) * k1 + at(r[2], r[3]) * k0 * k1)

    grid = np.zeros(NC)
    for i, j, idx in cells:
        grid[idx] = g["init_grid"][i, j]
    t, last_call, rest, rest_since, tail = 0.0, None, 0, 0.0, 0
    filt, head = [0.0] * nC, [0] * nC
    ring_t, ring_v = np.zeros(R), np.zeros((R, C))
    for k in range(int(g["n_steps"])):
        if t - rest_since > 3600.0:
            rest, rest_since = (0 if rest + 1 > nC - 1 else rest + 1), t
        powers = [heater(h, t) for h in range(nH)]
        static = np.zeros(NC)
        for _, _, idx in cells:
            for h in range(nH):
                static[idx] += hd[h, idx] * powers[h]
        value = np.clip(g["action"][k], 0, 1).astype(np.float32)
        value[rest] = np.float32(sc[14])
        set_temp = value * np.float32(settings["set_upper_bound"] - settings["set_lower_bound"]) \
            + np.float32(settings["set_lower_bound"])
        energy = np.zeros(nC, np.float32)
        for _ in range(iters):
            call_dt = 0.0 if last_call is None else t - last_call
            ne, pc, pv = np.zeros(nC), np.zeros(nC), np.zeros(nC)
            slot = tail & (R - 1)
            ring_t[slot] = t
            for c in range(nC):
                r = cool[c]
                cur = read(grid, r) + r[19]
                ring_v[slot, c] = cur
                while head[c] < tail and ring_t[head[c] & (R - 1)] < t - r[20]:
                    head[c] += 1
                delayed = ring_v[head[c] & (R - 1), c] if head[c] < tail else cur
                alpha = np.exp(-call_dt / (r[20] / 3.0)) if call_dt > 0 else 1.0
                filt[c] = alpha * filt[c] + (1.0 - alpha) * delayed
                plain = True
                if c != rest:
                    diff = filt[c] - float(set_temp[c])
                    if diff > r[13]:
                        pall = (r[15] - r[16]) * 1.0 + r[16]
                    elif diff < r[14]:
                        pall = (r[15] - r[16]) * 0.0 + r[16]
                    else:
                        pall, plain = (r[15] - r[16]) * ((diff - r[14]) / (r[13] - r[14])) + r[16], False
                    m = r[17] if r[17] > r[18] * pall else r[18] * pall
                    pv[c] = pall if pall < m else m
                    pc[c] = pall - pv[c]
                d_amb = amb - grid[int(r[6]) * NL + int(r[7])]
                eer = r[12] if d_amb < 0 else r[9] if d_amb < r[10] else \
                    r[9] * ((r[11] - d_amb) / (r[11] - r[10])) if d_amb < r[11] else 0.0
                ne[c] = -eer
                e = (pc[c] + pv[c]) * dt
                energy[c] = energy[c] + np.float32(e) if plain else np.float32(np.float64(energy[c]) + e)
            last_call, tail = t, tail + 1
            wall = chtc.copy()
            for c in range(nC):
                wall += (cv[c] * pv[c]) * cool[c, 8]
            new = grid.copy()
            for i, j, idx in cells:
                nh = static[idx]
                for c in range(nC):
                    nh += (ne[c] * cd[c, idx]) * pc[c]
                s0 = grid[idx]
                up, down = (grid[idx - NL] if i > 0 else amb), (grid[idx + NL] if i < nw - 1 else amb)
                left, right = (grid[idx - 1] if j > 0 else amb), (grid[idx + 1] if j < nl - 1 else amb)
                w = (i * (NL + 1) + j) * 2
                h0, h1 = (-(s0 - up)) * wall[w] * csa, (-(down - s0)) * wall[w + 2 * (NL + 1)] * csa
                v0, v1 = (-(s0 - left)) * wall[w + 1] * csa, (-(right - s0)) * wall[w + 3] * csa
                net_in = ((h0 - h1) + (v0 - v1)) + fcc_area * (amb - s0)
                new[idx] = s0 + (nh + net_in) / hc[idx] * dt
            grid = new
            t += dt
        t = float(int(t + 0.5))
        got = np.array([[grid[i * NL + j] for j in range(nl)] for i in range(nw)])
        assert U.same_bits(got, g["grid"][k]) and t == g["t"][k], k
        sensors = np.array([read(grid, sens[s]) + series(sens[s][8:], KS, sens[s][7], t / sens[s][6]) for s in range(nS)])
        assert U.same_bits(sensors.astype(np.float32), g["sensor_readings"][k]), k
        assert U.same_bits(energy / np.float32(dt * iters), g["cool_power"][k]), k
        assert rest == g["rest_idx"][k]


@pytest.mark.parametrize("name", ("mode1", "hot"))
def test_device_table_alone_replays_a_recording(name):
    """the table of the small room inside a batch padded to the wide room's sizes carries the whole task, where the header
    says it does"""
    g, task, settings, gen = U.load(name)
    tab = build_tables([U.load("wide")[1], task], generate_task=gen)
    _replay_from_table(tab["table"][1], tab["dims"], dict(settings, set_lower_bound=16, set_upper_bound=32), g)


def test_the_package_keeps_its_names_and_the_moved_classes_say_where_they_live():
    """every public name of xenoverse_amd.anyhvac before the one-room and solver classes left vec_env.py"""
    import xenoverse_amd.anyhvac as pkg
    names = ("ActionMapHost", "DEFAULTS", "DiffActionHost", "DiscreteActionHost", "HVACEnv", "HVACEnvDiffAction",
             "HVACEnvDiscreteAction", "HVACHost", "HVACSolverGTPID", "HVACSolverGridSearchPID", "HVACSolverLOCPID",
             "HVACTaskSampler", "HVACVecEnv", "PIDHost", "actions", "average_total_heat", "build_tables", "check_settings",
             "config", "device_sampler", "heater_powers", "host", "pid", "pid_search_host", "pid_weights",
             "sample_candidate_host", "sample_candidates", "sample_rows_host", "sample_tasks_device", "sampler_host",
             "table_dims", "tables", "task_dicts_from_device", "task_from_reference", "task_sampler", "vec_env",
             "wind_diffuser", "wind_diffuser_host")
    for k in names:
        assert hasattr(pkg, k), k
    where = {"vec_env": ("HVACVecEnv",), "single_env": ("HVACEnv", "HVACEnvDiscreteAction", "HVACEnvDiffAction"),
             "solvers": ("HVACSolverGTPID", "HVACSolverLOCPID", "HVACSolverGridSearchPID")}
    for module, classes in where.items():
        for k in classes:
            assert getattr(pkg, k).__module__ == "xenoverse_amd.anyhvac." + module, k
    from xenoverse_amd.anyhvac.single_env import _StatEnv
    assert _StatEnv.__module__ == "xenoverse_amd.anyhvac.single_env"
