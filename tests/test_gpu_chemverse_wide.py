"""ChemVerse on the device at its table limits (goldens only): world x has 64 chemicals and 128 reactions, two of them with 6
reactants, 4 products, 4 byproducts, 4 catalysts and coefficients up to 8, and one whose reactants are all solvents; world h is
a sampled "hard" world of 51 chemicals and 95 reactions; world a (14 and 9) rides in the same handle, so its rows are mostly
padding.  tests/test_host_chemverse.py asserts, without a GPU, which branches these fixtures reach; tests/chemverse_util.py
states the comparison and where its bound comes from.  One run of XV_CHEM_STEPS_MAX steps on world a."""
import time

import numpy as np
import pytest

import chemverse_util as cu

pytestmark = pytest.mark.gpu

ORDER = ("x", "h", "a")      # the handle's worlds; the widest first
N_TAG = len(ORDER)
WIDTH = dict(fired="R", final_pool="C", consumed="C", produced="C", byproduct="C", gas_lost="C", log_consumed="C",
             log_produced="C")


def interleaved():
    """x0 h0 a0 x1 ...: (world index, fixture row) per batch entry"""
    n = cu.fixture("a")["n"]
    assert all(cu.fixture(t)["n"] == n for t in ORDER)
    k = np.arange(N_TAG * n)
    return k % N_TAG, k // N_TAG


def args_of(world, row, tags=ORDER):
    fxs = [cu.fixture(t) for t in tags]
    pick = lambda key: np.array([fxs[w]["runs"][key][i] for w, i in zip(world, row)])      # noqa: E731
    return dict(world_index=np.asarray(world, np.int32), amounts=[cu.amounts_of(fxs[w], i) for w, i in zip(world, row)],
                temperature_C=pick("temperature_C"), pressure_atm=pick("pressure_atm"), duration_s=pick("duration_s"),
                equipment=pick("equipment"), heating_rate_C_per_s=pick("heating_rate_C_per_s"),
                vessel_volume_L=pick("vessel_volume_L"))


def run(b, **args):
    res = {k: v.cpu().numpy() for k, v in b.simulate(record="log", **args).items()}
    assert b.check_errors() == 0
    return res


def _same(a, b, sel=None):
    for k in b:
        x = a[k] if sel is None else a[k][sel]
        assert np.array_equal(x.view(np.uint8), b[k].view(np.uint8)), k


@pytest.fixture(scope="module")
def batch():
    from xenoverse_amd.chemverse import ChemVerseBatch
    from xenoverse_amd.chemverse import tables as T
    b = ChemVerseBatch([cu.fixture(t)["world"] for t in ORDER], N_TAG * 128)
    assert b.c_stride == T.C_MAX and b.r_stride == T.R_MAX
    yield b
    b.close()


@pytest.fixture(scope="module")
def whole(batch):
    """the interleaved batch of 384 with the reaction log, once; left unchanged"""
    res = run(batch, **args_of(*interleaved()))
    for v in res.values():
        v.setflags(write=False)
    return res


def test_device_equals_the_reference_at_the_limits(whole):
    world, row = interleaved()
    for w, tag in enumerate(ORDER):
        fx = cu.fixture(tag)
        assert cu.unstable_fraction(fx) <= 0.02
        m = world == w
        assert np.array_equal(row[m], np.arange(fx["n"]))
        ratio = cu.compare(fx, {k: v[m] for k, v in whole.items()}, label="device %s: " % tag)
        print("fixture %s in the 64 x 128 handle: largest deviation / bound = %.4g" % (tag, ratio))
        assert ratio <= 1.0
    # the shapes the fixtures were made for ran on the device, not only on the reference
    x = {k: v[world == 0] for k, v in whole.items()}
    stable = cu.fixture("x")["runs"]["stable"]
    ri = cu.fixture("x")["tab"]["rxn_i"]
    full = np.nonzero((ri[:, :4] == (6, 4, 4, 4)).all(axis=1))[0]
    assert len(full) >= 2 and full.min() >= 64
    assert all((x["fired"][stable][:, r] > 0).any() for r in full)
    assert (x["fired"][:, 127] > 0).any() and (x["final_pool"][:, 63] > 1e-9).any() and (x["log_produced"][..., 63] > 0).any()


def test_padding_columns_are_zero_and_narrow_rows_do_not_depend_on_the_stride(whole):
    from xenoverse_amd.chemverse import ChemVerseBatch
    world, row = interleaved()
    for w, tag in enumerate(ORDER):
        tab = cu.fixture(tag)["tab"]
        for key, dim in WIDTH.items():
            assert not whole[key][world == w][..., tab[dim]:].any(), (tag, key)
    fx = cu.fixture("a")
    b = ChemVerseBatch([fx["world"]], fx["n"])
    try:
        assert (b.c_stride, b.r_stride) == (fx["tab"]["C"], fx["tab"]["R"])
        alone = run(b, **args_of(np.zeros(fx["n"], np.int32), np.arange(fx["n"]), tags=("a",)))
    finally:
        b.close()
    m = world == ORDER.index("a")
    for key, v in alone.items():
        wide = whole[key][m]
        if key in WIDTH:
            wide = wide[..., :fx["tab"][WIDTH[key]]]
        assert np.array_equal(np.ascontiguousarray(wide).view(np.uint8), v.view(np.uint8)), key


def test_limit_experiments_are_independent_of_their_batch(batch, whole):
    """an experiment that fired a reaction past 63, one holding chemical 63, one that took `__self__` and one that fired a
    6 / 4 / 4 / 4 reaction: alone, and among 65 experiments of world x (two workgroups), bit-equal to the whole batch"""
    fx = cu.fixture("x")
    hits, stable = cu.branch_hits(fx), fx["runs"]["stable"]
    wide = hits["reactants_6"] & hits["products_4"] & hits["byproducts_4"] & hits["catalysts_4"]
    picks = []
    for m in (hits["reaction_index_ge_64_fired"] & ~wide, hits["chemical_63_in_pool"], hits["solvent_self"], wide):
        picks.append(next(int(i) for i in np.nonzero(m & stable)[0] if int(i) not in picks))
    rows = picks + [i for i in range(fx["n"]) if i not in picks][:65 - len(picks)]
    at = lambda r: np.asarray(r) * N_TAG + ORDER.index("x")      # noqa: E731
    _same(whole, run(batch, **args_of(np.zeros(65, np.int32), rows)), at(rows))
    for i in picks:
        alone = run(batch, **args_of([0], [i]))
        assert alone["fired"].sum() > 0
        _same(whole, alone, at([i]))


def test_the_longest_run(whole):
    """XV_CHEM_STEPS_MAX steps beside two short experiments: 25 history entries (steps 0..4, then every 204th), the log cut at
    20, the values within the bound of the recorded run"""
    from xenoverse_amd.chemverse import ChemVerseBatch
    from xenoverse_amd.chemverse import tables as T
    long, a = cu.fixture(cu.LONG), cu.fixture("a")
    b = ChemVerseBatch([a["world"]], 3)
    try:
        args = args_of([0, 1, 1], [0, 0, 1], tags=(cu.LONG, "a"))
        args["world_index"] = np.zeros(3, np.int32)
        t0 = time.perf_counter()
        res = run(b, **args)
        seconds = time.perf_counter() - t0
    finally:
        b.close()
    print("%d steps beside two short experiments: %.2f s" % (T.STEPS_MAX, seconds))
    assert res["steps_run"][0] == T.STEPS_MAX and res["num_steps"][0] == T.STEPS_MAX
    assert res["hist_count"][0] == 25 and res["log_count"][0] == 20
    assert np.array_equal(res["hist_step"][0], long["runs"]["hist_step"][0])
    assert long["runs"]["stable"][0]
    ratio = cu.compare(long, {k: v[:1] for k, v in res.items()}, label="device long: ")
    print("the longest run: largest deviation / bound = %.4g" % ratio)
    assert ratio <= 1.0
    world, row = interleaved()
    k = np.nonzero((world == ORDER.index("a")) & (row < 2))[0]
    for key, v in res.items():      # the short ones beside it: as in the wide handle
        wide = whole[key][k]
        if key in WIDTH:
            wide = wide[..., :a["tab"][WIDTH[key]]]
        assert np.array_equal(wide, v[1:]), key
    assert seconds < 10.0


def test_strides_beyond_the_limits_are_refused_and_the_handle_lives_on(batch, whole):
    from xenoverse_amd import _lib
    from xenoverse_amd.chemverse import tables as T
    ptrs = [_lib.ptr(t) for t in batch._dev]
    for cs, rs in ((T.C_MAX + 1, T.R_MAX), (T.C_MAX, T.R_MAX + 1)):
        rc = batch.lib.xv_chem_set_worlds(batch._h, N_TAG, cs, rs, *ptrs)
        assert rc == _lib.XV_ERR_UNSUPPORTED, (cs, rs, rc)
    batch.set_worlds([cu.fixture(t)["world"] for t in ORDER])
    sel = np.arange(70)
    world, row = interleaved()
    _same(whole, run(batch, **args_of(world[sel], row[sel])), sel)
