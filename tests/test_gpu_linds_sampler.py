"""The device LinDS task sampler and zero-order-hold builder (xv_linds_sample_tasks, xv_linds_build_zoh,
csrc/linds_sampler.hip) against their numpy restatement (linds/sampler_host.py), the host table builder, a 50-digit
yardstick, and end to end through the step engine.  The inputs are those of tests/linds_sampler_util.py, which
tests/test_host_linds_sampler.py shows to exercise every branch."""
import numpy as np
import pytest
import torch

import linds_sampler_util as U
from util import golden_files, load_linds_golden

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-9, 1e-12      # the project's device-sampler tolerance (tests/test_gpu_sampler.py)


def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else t


@pytest.fixture(scope="module")
def eng():
    from xenoverse_amd.engine import Engine
    e = Engine("cuda:0")
    yield e
    e.close()


def _run(eng, case, base=None, n=None):
    from xenoverse_amd.linds import device_sampler as ds
    r = ds.sample_candidates(eng, case["seed"], case["cand_base"] if base is None else base, case["n"] if n is None else n,
                             max_draws=case["max_draws"], max_init=U.MAX_INIT, tables=True, dense=True, info=True,
                             **U.dims_kw(case))
    eng.sync()
    return r


_RUNS = {}


def _case_run(eng, name):
    if name not in _RUNS:
        _RUNS[name] = _run(eng, U.CASES[name])
    return _RUNS[name]


def _accepted(r):
    """the accepted rows of a sample_candidates result, as task_dicts_from_device takes them"""
    acc = np.nonzero(r["info"]["status"] == 0)[0]
    sel = torch.as_tensor(acc, device=r["status"].device)
    out = {k: (v.index_select(0, sel) if torch.is_tensor(v) else v) for k, v in r.items()}
    out["info"] = r["info"][acc]
    return out


def _close(a, b):
    return np.allclose(a, b, rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("name", sorted(U.CASES))
def test_candidates_equal_the_host(eng, name):
    """every candidate, accepted or not: status, accepted attempt and every discrete choice exact, fp64 arrays to 1e-9"""
    r = _case_run(eng, name)
    st = _np(r["status"])
    g = {k: _np(r[k]) for k in ("A", "B", "C", "X", "Y", "init64", "phi", "gam", "four_order", "four_coef64", "cmd064")}
    hosts = U.host_candidates(name)
    for i, h in enumerate(hosts):
        inf, hd = r["info"][i], h["head"]
        assert st[i] == inf["status"] == h["status"], (i, st[i], h["status"])
        assert inf["attempt"] == h["attempt"], (i, inf["attempt"], h["attempt"])
        ns, na, no = hd["ns"], hd["na"], hd["no"]
        assert (inf["ns"], inf["na"], inf["no"]) == (ns, na, no)
        for k in ("a_scale", "x_scale", "trim", "width", "max_steps", "type", "valid_rounds"):
            assert inf[k] == hd[k], (i, k, inf[k], hd[k])
        assert np.array_equal(inf["target_valid"][:no], hd["target_valid"]) and not inf["target_valid"][no:].any()
        for k in ("action_cost", "reward_base", "terminate_punish", "reward_factor", "eps"):
            assert _close(inf[k], hd[k]), (i, k)
        assert _close(g["A"][i, :ns, :ns], hd["A"]) and _close(g["B"][i, :ns, :na], hd["B"])
        assert _close(g["C"][i, :no, :ns], hd["C"]) and _close(g["X"][i, :ns], hd["X"]) and not g["Y"][i].any()
        assert np.array_equal(g["A"][i, :ns, :ns] == 0.0, hd["A"] == 0.0)      # the trim pattern
        assert np.linalg.matrix_rank(g["B"][i, :ns, :na]) == min(ns, na)       # the rank test the device leaves out
        assert np.linalg.matrix_rank(g["C"][i, :no, :ns]) == min(ns, no)
        if h["status"] != 0:
            continue
        t = h["task"]
        assert (inf["n_init"], inf["n_terms"], inf["delay"]) == (h["n_init"], h["n_terms"], h["delay"])
        assert _close(inf["noise_drift"], t["noise_drift"])
        assert _close(g["init64"][i, :h["n_init"], :ns], np.stack(t["initial_states"])) and not g["init64"][i, h["n_init"]:].any()
        if hd["type"] == 0:
            assert _close(g["cmd064"][i, :no], t["command"])
        else:
            orders = np.array([o for o, _ in t["command"].coeffs])
            coefs = np.stack([c for _, c in t["command"].coeffs])
            assert _close(g["four_order"][i, :h["n_terms"]], orders) and _close(g["four_coef64"][i, :h["n_terms"], :no], coefs)
            assert not g["four_coef64"][i, h["n_terms"]:].any()
        assert _close(g["phi"][i, :ns, :ns], h["Phi"]) and _close(g["gam"][i, :ns, :na], h["Gamma"])
    assert (st == 0).sum() >= 1 and (st == 1).sum() >= 1


_BITWISE = ("status", "phiT", "gamT", "cT", "xt", "y0", "valid", "cmd0", "four_coef", "four_omega", "four_period", "scal", "ints",
            "init", "A", "B", "C", "X", "init64", "phi", "gam", "four_order", "four_coef64", "cmd064")


def test_results_do_not_depend_on_launch_geometry(eng):
    """one launch of 48 candidates = three launches of 16 with shifted cand_base; another `batch` = the same tasks"""
    from xenoverse_amd.linds import device_sampler as ds
    g = U.GEOMETRY
    whole = _run(eng, g)
    parts = [_run(eng, g, base=g["cand_base"] + 16 * k, n=16) for k in range(3)]
    assert (whole["info"]["status"] == 0).sum() >= 4
    for k in _BITWISE:
        assert torch.equal(whole[k], torch.cat([p[k] for p in parts])), k
    assert whole["info"].tobytes() == np.concatenate([p["info"] for p in parts]).tobytes()
    kw = dict(state_dim=16, action_dim=8, observation_dim=8, seed=g["seed"], max_draws=g["max_draws"], engine=eng, dense=True)
    a = ds.sample_tasks_device(10, batch=16, **kw)
    b = ds.sample_tasks_device(10, batch=7, **kw)
    for k in _BITWISE[1:]:
        assert a[k].shape[0] == 10 and torch.equal(a[k], b[k]), k
    assert a["info"].tobytes() == b["info"].tobytes() and a["stats"]["candidates"] == b["stats"]["candidates"]
    assert a["stats"]["accepted"] == 10 and sum(a["stats"]["status"].values()) == a["stats"]["candidates"]


def _check_tables(dev, ref, what):
    """criterion 3: every field exact but phiT / gamT, which are equal or adjacent fp32 values — at most 1e-3 of an array's
    entries adjacent, none further than 1 ulp unless below 2^-20 of the array's largest.  -> all bit-equal?"""
    NS, NI = ref["NS"], ref["NI"]
    same = True
    for k in ("cT", "xt", "y0", "valid", "cmd0", "four_coef", "four_omega", "four_period", "scal", "ints", "init", "phiT", "gamT"):
        d, r = _np(dev[k]), ref[k]
        if k in ("phiT", "cT"):
            full, d = d, d[:, :NS]
            assert not full[:, NS:].any(), (what, k)
        if k in ("gamT", "xt"):
            full, d = d, d[..., :NS]
            assert not full[..., NS:].any(), (what, k)
        if k == "phiT":
            assert not d[:, :, NS:].any()
            d = d[:, :, :NS]
        if k == "init":
            assert not d[:, NI:].any() and not d[:, :, NS:].any()
            d = d[:, :NI, :NS]
        assert d.shape == r.shape and d.dtype == r.dtype, (what, k, d.shape, r.shape)
        if k in ("phiT", "gamT"):
            share, ok = U.f32_ulp_report(d, r)
            print("%s %s: share of adjacent entries %.2e" % (what, k, share))
            assert ok and share <= 1e-3, (what, k, share)
            same = same and np.array_equal(d, r)
        else:
            assert np.array_equal(d, r), (what, k)
    return same


@pytest.mark.parametrize("name", sorted(U.CASES))
def test_tables_equal_the_host_builder(eng, name):
    """build_tables(task_dicts_from_device(out)) = the device's tables, for the accepted candidates of every case"""
    from xenoverse_amd.linds import build_tables, task_dicts_from_device
    acc = _accepted(_case_run(eng, name))
    tasks = task_dicts_from_device(acc)
    assert len(tasks) >= 1
    ref = build_tables(tasks, dt=0.1, pad_observation_dim=acc["NO"], pad_action_dim=acc["NA"], pad_command_dim=acc["NO"])
    _check_tables(acc, ref, name)
    assert np.array_equal(ref["action_dims"], acc["info"]["na"])


def _yardstick_inputs():
    y = U.yardstick()
    return y, y["A"], y["B"], np.zeros(y["A"].shape[:2]), y["ns"]


def test_zoh_against_the_yardstick(eng):
    """xv_linds_build_zoh under the bound of the host test: per case, relative to the largest entry,
    max(2^-44, 8 x the error of build_dynamics_matrices on that case)"""
    from xenoverse_amd.linds import build_zoh_device
    from xenoverse_amd.linds import sampler_host as sh
    y, A, B, X, ns = _yardstick_inputs()
    n = len(ns)
    outs = {}
    for dt in sorted(set(y["dt"])):      # dt is one argument of the launch
        sel = np.nonzero(y["dt"] == dt)[0]
        z = build_zoh_device(eng, A[sel], B[sel], X[sel], ns[sel], dt=float(dt), dense=True)
        eng.sync()
        assert not _np(z["status"]).any()
        for j, c in enumerate(sel):
            outs[int(c)] = (_np(z["phi"][j]), _np(z["gam"][j]), _np(z["phiT"][j]), _np(z["gamT"][j]))
    for c in range(n):
        k, na = int(ns[c]), int(y["na"][c])
        phi, gam, phiT, gamT = outs[c]
        e_phi = U.rel_err(phi[:k, :k], y["phi_hi"][c, :k, :k], y["phi_lo"][c, :k, :k])
        e_gam = U.rel_err(gam[:k, :na], y["gam_hi"][c, :k, :na], y["gam_lo"][c, :k, :na])
        s_phi, s_gam = U.scipy_rel_err(y, c)
        hp, hg, _, s = sh.zoh_host(A[c, :k, :k], B[c, :k, :na], float(y["dt"][c]))
        print("case %d ns %d scale %g s %d: device %.2e %.2e scipy %.2e %.2e; bits equal zoh_host: %s"
              % (c, k, y["scale"][c], s, e_phi, e_gam, s_phi, s_gam, np.array_equal(phi[:k, :k], hp) and np.array_equal(gam[:k, :na], hg)))
        assert e_phi <= U.zoh_bound(s_phi) and e_gam <= U.zoh_bound(s_gam), (c, e_phi, e_gam)
        assert not phi[k:].any() and not phi[:, k:].any() and not gam[k:].any()      # padding stays zero
        assert np.array_equal(phiT, phi.T.astype(np.float32)) and np.array_equal(gamT, gam.T.astype(np.float32))


def test_zoh_bad_inputs_set_a_status_and_spare_the_rest(eng):
    from xenoverse_amd.linds import build_zoh_device
    y, A, B, X, ns = _yardstick_inputs()
    sel = np.array([4, 5, 6, 7])      # four ns = 16 cases at dt = 0.1
    good = build_zoh_device(eng, A[sel], B[sel], X[sel], ns[sel], dt=0.1, dense=True)
    A2 = A[sel].copy()
    A2[1, 3, 2] = np.nan
    A2[3] = A2[3] * 1e15      # |A dt|_inf needs more than 40 halvings
    bad = build_zoh_device(eng, A2, B[sel], X[sel], ns[sel], dt=0.1, dense=True)
    eng.sync()
    assert _np(good["status"]).tolist() == [0, 0, 0, 0] and _np(bad["status"]).tolist() == [0, 1, 0, 2]
    for k in ("phiT", "gamT", "xt", "phi", "gam"):
        assert torch.equal(bad[k][0], good[k][0]) and torch.equal(bad[k][2], good[k][2]), k
        assert not _np(bad[k][1]).any() and not _np(bad[k][3]).any(), k      # a failed task's tables are zero, never NaN


def test_build_tables_device_on_the_golden_tasks(eng):
    from xenoverse_amd.linds import build_tables, build_tables_device
    files = golden_files("linds_16x8x8_")[:4] + golden_files("linds_32x8x8_0")
    assert len(files) == 5
    tasks = [load_linds_golden(p)[1] for p in files]
    ref = build_tables(tasks)
    dev = build_tables_device(tasks, eng)
    assert set(dev) == set(ref) and (dev["NS"], dev["NA"], dev["NO"], dev["NI"]) == (ref["NS"], ref["NA"], ref["NO"], ref["NI"])
    _check_tables(dev, ref, "golden")
    assert np.array_equal(dev["action_dims"], ref["action_dims"])


def test_device_tasks_step_like_the_same_tasks_from_the_host(eng):
    """8 device-sampled (16, 8, 8) tasks x 16 envs through set_task as device tables, and through task dicts and the host
    builder into a second env: same injected resets, actions and noise -> the same trajectories"""
    from xenoverse_amd.linds import LinDSVecEnv, build_tables, sample_tasks_device, task_dicts_from_device
    e = U.END_TO_END
    out = sample_tasks_device(e["n_tasks"], e["state_dim"], e["action_dim"], e["observation_dim"], seed=e["seed"],
                              max_draws=e["max_draws"], batch=e["batch"], engine=eng, dense=True)
    assert out["phiT"].shape == (8, 16, 16) and out["stats"]["accepted"] == 8
    tasks = task_dicts_from_device(out)
    ref = build_tables(tasks)
    bit_equal = _check_tables(out, ref, "end to end")
    # which case this is: the banded / triangular tasks among the eight have Phi entries below 2^-20 of the largest, where the
    # kernel's Taylor series and scipy's Pade approximant round differently (every larger entry is bit-equal)
    assert not bit_equal
    eq_task = np.array([np.array_equal(_np(out["phiT"][t]), ref["phiT"][t]) and np.array_equal(_np(out["gamT"][t]), ref["gamT"][t])
                        for t in range(e["n_tasks"])])
    eq_env = np.repeat(eq_task, 16)      # envs of a task whose two table sets are bit-equal must step bit-equal
    print("tasks with bit-equal tables:", eq_task.tolist())
    n = 16 * e["n_tasks"]
    env_d = LinDSVecEnv(n, seed=5, engine=eng)
    env_h = LinDSVecEnv(n, seed=5, engine=eng)
    env_d.set_task(out)
    env_h.set_task(tasks)
    rng = np.random.RandomState(3)
    idx = np.zeros(n, np.int32)
    od, _ = env_d.reset_injected(idx)
    oh, _ = env_h.reset_injected(idx)
    assert torch.equal(od, oh)
    for _ in range(8):
        a = rng.uniform(-1, 1, (n, 8)).astype(np.float32)
        z = rng.randn(16, n).astype(np.float32)
        d, h = env_d.step_injected(a, z, idx), env_h.step_injected(a, z, idx)
        for x, yv in zip(d[:4], h[:4]):
            x, yv = _np(x), _np(yv)
            assert np.array_equal(x[eq_env], yv[eq_env])
            assert np.allclose(x.astype(np.float64), yv.astype(np.float64), rtol=1e-5, atol=1e-5)      # the LinDS suite's 1e-5
        assert torch.isfinite(d[0]).all()
    with pytest.raises(ValueError):      # device tables carry no fp64 model: the teacher asks for the dicts
        env_d.mpc_action(K=4)
    act = env_h.mpc_action(K=4)
    assert act.shape == (n, 8) and torch.isfinite(act).all()
    env_d.close()
    env_h.close()
