"""The numpy restatement of the device AnyHVAC task sampler (xenoverse_amd/anyhvac/sampler_host.py), without a GPU: its
diffuser against the reference's FIFO walk, its tasks against build_tables and HVACHost, its candidate order, its counters,
the C-ABI's declaration, and the promises the GPU test (tests/test_gpu_anyhvac_sampler.py) relies on for its seeds."""
import os
import re

import numpy as np
import pytest
import torch

import anyhvac_sampler_util as U
from xenoverse_amd import _lib
from xenoverse_amd.anyhvac import HVACHost, build_tables, sampler_host as sh
from xenoverse_amd.anyhvac.task_sampler import wind_diffuser
from xenoverse_amd.device_sampling import collect_accepted

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_jacobi_diffuser_equals_the_fifo_walk_byte_for_byte():
    """random wall patterns, square and oblong grids (one above 128 cells: numpy's sum splits there), sources anywhere"""
    rng = np.random.RandomState(11)
    for nw, nl, density in ((5, 5, 0.3), (5, 8, 0.5), (9, 6, 0.2), (15, 15, 0.35), (1, 7, 0.2), (12, 11, 0.0)):
        for _ in range(4):
            walls = rng.random_sample((nw + 1, nl + 1, 2)) < density
            cell_size, sigma = rng.uniform(1.0, 3.0), rng.uniform(0.5, 4.0)
            src = np.array([float(rng.randint(0, int(nw * cell_size))), rng.uniform(0, nl * cell_size)])
            mat, wall = wind_diffuser(walls, src, cell_size, sigma)
            m2, w2, passes, margin = sh.wind_diffuser_host(walls, src, cell_size, sigma, with_stats=True)
            assert m2.tobytes() == mat.tobytes() and w2.tobytes() == wall.tobytes(), (nw, nl)
            assert 1 <= passes <= nw * nl + 1 and margin > 0


def test_tasks_are_accepted_by_build_tables_and_the_host_env():
    rows = U.host_rows("tiny")
    done = 0
    for c in rows["candidates"]:
        if c["status"] == 0 and done < 3:
            done += 1
            tab = build_tables([c["task"]])
            assert tab["counts"][0]["C"] == int(c["info"]["coolers"])
            env = HVACHost(iter_per_step=5)
            env.set_task(c["task"])
            obs, _ = env.reset()
            obs, reward, terminated, truncated, info = env.step(np.full(env.n_coolers, 0.5, np.float32))
            assert np.isfinite(reward) and np.isfinite(obs["sensor_readings"]).all()
    assert done == 3


@pytest.mark.parametrize("case", ["tiny", "mixed"])
def test_row_equals_build_tables_of_its_own_dict(case):
    rows = U.host_rows(case, with_heat=False)      # (the week-long average is the slow part: formed for three candidates)
    dims = rows["dims"]
    acc = [sh.sample_candidate_host(U.SEEDS[case], int(i), config=U.CASES[case])
           for i in np.flatnonzero(rows["status"] == 0)[:3]]
    tab = build_tables([c["task"] for c in acc], dims=dims)
    assert tab["dims"] == dims
    for c, row, avg in zip(acc, tab["table"], tab["avg_total_heat"]):
        assert np.array_equal(row, c["row"])      # the average heat too: both are host.average_total_heat
        assert avg == c["avg_total_heat"] == c["row"][10]
    for c in rows["candidates"]:
        if c["status"]:
            assert np.array_equal(c["row"], sh.padding_row(dims)) and c["task"] is None
    gen = sh.sample_candidate_host(U.SEEDS[case], int(np.flatnonzero(rows["status"] == 0)[0]), config=U.CASES[case],
                                   generate_task=True)
    assert gen["row"][10] == 10000.0
    off = np.ones(len(gen["row"]), bool)
    off[10] = False
    assert np.array_equal(gen["row"][off], acc[0]["row"][off])


def test_candidate_order_does_not_depend_on_the_batch():
    def launch(base, n):
        r = sh.sample_rows_host(U.SEEDS["tiny"], base, n, config=U.CASES["tiny"], with_heat=False)
        return dict(table=torch.from_numpy(r["table"]), extras=torch.from_numpy(r["extras"]), info=r["info"])

    a, ia, ha = collect_accepted(launch, 9, 4, ("table", "extras"), sh.STATUS)
    b, ib, hb = collect_accepted(launch, 9, 11, ("table", "extras"), sh.STATUS)
    assert torch.equal(a["table"], b["table"]) and torch.equal(a["extras"], b["extras"])
    assert np.array_equal(ia, ib) and np.array_equal(ha, hb) and ha[0] == 9


def test_counter_purposes_never_collide():
    values = list(sh.PURPOSES.values())
    assert len(set(values)) == len(values) == 11 and all(0 <= v < 256 for v in values)
    # within a purpose: the Fourier block of a sensor / heat curve ends before the next sub in use
    assert 1 + 1 + 4 * sh.MAX_TERMS <= 128 and 2 + 1 + 4 * sh.MAX_TERMS <= sh.HEATER_EXTRA_SUB
    assert 7 <= sh.BIAS_SUB and sh.PLACE_TRIES < 2 ** 32 and max(U.sh.table_dims()[2:5]) < sh.TICK_MAX
    # two candidates, two purposes, two ticks, two subs: all different words
    d0, d1 = sh.Draws(1, 0), sh.Draws(1, 1)
    seen = set()
    for d in (d0, d1):
        for purpose in (sh.P_SENSOR, sh.P_HEATER):
            for tick in (0, 1):
                a, b = d.ints53(purpose, [0, 1], tick)
                seen.update(int(v) for v in a)
                seen.update(int(v) for v in b)
    assert len(seen) == 2 * 2 * 2 * 4


def test_symbol_is_declared_bound_and_the_abi_version_stays():
    with open(os.path.join(ROOT, "include", "xeno.h")) as f:
        header = f.read()
    assert re.search(r"int xv_anyhvac_sample_tasks\(xv_engine\* e, uint64_t seed, int64_t cand_base, int n_cand", header)
    assert "xv_anyhvac_sampler_params" in header and "xv_anyhvac_cand_info" in header and "XV_ANYHVAC_EXTRAS" in header
    assert re.search(r"#define XV_ABI_VERSION 12\b", header)
    assert _lib.ABI_VERSION == 12
    assert len(_lib.SIGNATURES["xv_anyhvac_sample_tasks"]) == 16 and "xv_anyhvac_sampler_check" in _lib.SIGNATURES
    from xenoverse_amd.anyhvac import device_sampler as ds
    assert len(ds.RANGES) == 28 and C_sizeof(ds.Params) == 16 * 4 + (9 + 8) * 8 + 28 * 16
    assert sh.INFO_DTYPE.itemsize == 40 and sh.extras_doubles(3, 5, 7) == 2 * 5 + 3 * 7 + 3 * 3 + 4


def C_sizeof(struct):
    import ctypes
    return ctypes.sizeof(struct)


def test_table_dims_follow_the_configuration():
    assert sh.table_dims() == (15, 15, 303, 607, 607, 4, 7)
    assert sh.table_dims(U.CASES["tiny"])[:2] == (5, 5) and sh.table_dims(U.CASES["many"])[3:5] == (270, 270)
    with pytest.raises(ValueError):
        sh.sampler_arguments(control_type="Power")
    with pytest.raises(ValueError):
        sh.sampler_arguments(config=dict(AMBIENT_TEMPERATURE_HIGH=[(30 + i, 0.2) for i in range(5)]))
    with pytest.raises(ValueError):
        sh.sampler_arguments(config=dict(NO_SUCH_CONSTANT=1))


@pytest.mark.parametrize("case", sorted(U.CASES))
def test_the_gpu_tests_seeds_keep_their_promises(case):
    """at least one accepted candidate, every margin safe (so the GPU test leaves no candidate out), placement far from its
    cap where rooms are dense, and a unify_empty in `tiny`"""
    rows = U.host_rows(case, with_heat=False)
    status = rows["status"]
    assert (status == 0).sum() >= 1 and set(status.tolist()) <= {0, 2}
    assert U.margins_safe(rows) == (True, True), (rows["bias_margin"].min(), rows["diffuse_margin"].min())
    if case in ("many", "wide"):
        assert int(rows["info"]["place_max"].max()) <= 1024
    if case == "tiny":
        assert (status == 2).sum() >= 1
        assert int(rows["info"]["coolers"][status == 0].min()) == 1      # a one-node kind among the accepted
    if case == "many":
        assert int(rows["info"]["sensors"].min()) > 256
    if case == "mixed":
        assert len(set(rows["info"]["n_width"].tolist())) > 1
