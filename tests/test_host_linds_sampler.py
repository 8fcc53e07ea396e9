"""The numpy restatement of the LinDS device sampler (xenoverse_amd/linds/sampler_host.py) on its own: the
validity of what it accepts, the statistics of its heads, the fixed inputs the GPU tests use, its zero-order hold against
a 50-digit yardstick, and the C-ABI declarations.  No GPU."""
import os
import re

import numpy as np
import pytest

import linds_sampler_util as U
from xenoverse_amd.linds import sampler_host as sh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check_task(c):
    """an accepted candidate against the reference's rules, recomputed with plain numpy from the emitted dict"""
    t, h = c["task"], c["head"]
    ns, na, no = t["state_dim"], t["action_dim"], t["observation_dim"]
    A, B, Cm, Y, tv = t["ld_A"], t["ld_B"], t["ld_C"], t["ld_Y"], t["target_valid"]
    assert A.shape == (ns, ns) and B.shape == (ns, na) and Cm.shape == (no, ns) and t["ld_X"].shape == (ns,) and Y.shape == (no,)
    cmd = t["command"] if t["target_type"] == "static_target" else t["command"](-t["target_delay"])
    assert 1 <= len(t["initial_states"]) <= U.MAX_INIT
    for x0 in t["initial_states"]:      # task_sampler.py:123-128
        assert np.linalg.norm((cmd - Cm @ x0 - Y) * tv) <= 3.0 and np.linalg.norm(x0) <= 10.0
    assert np.linalg.matrix_rank(B) == min(na, ns) and np.linalg.matrix_rank(Cm) == min(no, ns)
    i, j = np.indices((ns, ns))
    zero = np.zeros((ns, ns), bool)
    if h["trim"] == 0 and h["width"] < ns:
        zero = np.abs(i - j) > h["width"]
    elif h["trim"] == 1 and h["width"] < ns:
        zero = j < i + h["width"]
    assert np.array_equal(A == 0.0, zero)
    assert tv.sum() >= 1 and set(np.unique(tv)) <= {0, 1}
    assert 100 <= t["max_steps"] < 1000 and 0.0 <= t["noise_drift"] <= 0.02 and 0 <= t["target_delay"] < 30
    if t["target_type"] == "dynamic_target":
        assert 2 <= len(t["command"].coeffs) <= 6 and t["command"].coeffs[0][0] == 0.0 and t["command"].max_steps == 1000
    return t


@pytest.mark.parametrize("name", sorted(U.CASES))
def test_accepted_tasks_are_valid(name):
    from xenoverse_amd.linds import LinearDSSampler
    ref = LinearDSSampler(4, 2, 2, seed=1)
    n_acc = 0
    for c in U.host_candidates(name):
        if c["status"] != 0:
            assert c["attempt"] == -1 and c["task"] is None
            continue
        n_acc += 1
        t = _check_task(c)
        assert set(t) == set(ref)
        for k, v in ref.items():      # the keys and dtypes of LinearDSSampler's dict
            if k == "command":
                continue
            assert type(t[k]) is type(v) or np.asarray(t[k]).dtype.kind == np.asarray(v).dtype.kind, k
            if isinstance(v, np.ndarray):
                assert t[k].dtype == v.dtype and t[k].ndim == v.ndim, k
        assert all(x.dtype == np.float64 and x.ndim == 1 for x in t["initial_states"])
        if U.CASES[name]["random_dim"]:
            ns = t["state_dim"]
            assert 1 <= ns <= 16 and max(1, (ns + 1) // 2) <= t["action_dim"] <= max(min(8, ns * 3 // 2), (ns + 1) // 2)
            assert max(1, ns // 4) <= t["observation_dim"] <= max(min(16, ns * 3 // 2), ns // 4, 1)
    assert n_acc >= 1
    if U.CASES[name]["random_dim"]:
        assert len({c["head"]["ns"] for c in U.host_candidates(name)}) >= 4


def test_head_statistics():
    """4,096 heads: the discrete choices are uniform (2:1 for the target type) and target_valid has the mean of
    binomial(1, min(U(0.2, 1.2), 1)) conditioned on a non-zero sum, each to 4 standard errors"""
    n, no = 4096, 2
    heads = [sh.sample_head(31, c, 4, 2, no) for c in range(n)]

    def shares(key, k):
        return np.bincount([h[key] for h in heads], minlength=k) / n
    for key, k in (("a_scale", 5), ("x_scale", 3), ("trim", 3)):
        p = 1.0 / k
        assert np.all(np.abs(shares(key, k) - p) <= 4 * np.sqrt(p * (1 - p) / n)), (key, shares(key, k))
    dyn = np.mean([h["type"] for h in heads])
    assert abs(dyn - 2 / 3) <= 4 * np.sqrt(2 / 9 / n), dyn
    # E[tv_j | sum > 0] = E_eps[ eps / (1 - (1 - eps)^no) ], eps = min(U(0.2, 1.2), 1): 0.2 of the mass sits at eps = 1
    e = np.linspace(0.2, 1.0, 200001)
    f = e / (1.0 - (1.0 - e) ** no)
    want = np.sum((f[1:] + f[:-1]) * 0.5) * (e[1] - e[0]) + 0.2
    tv = np.array([h["target_valid"].mean() for h in heads])
    assert abs(tv.mean() - want) <= 4 * tv.std(ddof=1) / np.sqrt(n), (tv.mean(), want)
    assert all(h["target_valid"].sum() >= 1 for h in heads) and max(h["valid_rounds"] for h in heads) > 1
    ms = np.array([h["max_steps"] for h in heads])
    assert ms.min() >= 100 and ms.max() <= 999 and abs(ms.mean() - 549.5) <= 4 * np.sqrt((900**2 - 1) / 12 / n)


def test_fixed_gpu_inputs_exercise_every_branch():
    """what tests/test_gpu_linds_sampler.py relies on, asserted where no GPU is needed"""
    static = dynamic = multi = 0
    for name, case in U.CASES.items():
        cs = U.host_candidates(name)
        st = np.array([c["status"] for c in cs])
        assert (st == 0).sum() >= 1 and (st == 1).sum() >= 1, (name, st)
        acc = [c for c in cs if c["status"] == 0]
        static += sum(c["head"]["type"] == 0 for c in acc)
        dynamic += sum(c["head"]["type"] == 1 for c in acc)
        multi += sum(c["n_init"] > 1 for c in acc)
        for i in range(case["n"]):
            m = sh.start_margins(case["seed"], case["cand_base"] + i, NI=U.MAX_INIT, max_draws=case["max_draws"], **U.dims_kw(case))
            assert m >= 1e-6, (name, i, m)
    assert static >= 1 and dynamic >= 1 and multi >= 1


def test_candidate_does_not_depend_on_chunking():
    case = U.CASES["16x8x8"]
    for i in (0, 3):
        a = U.host_candidates("16x8x8")[i]
        b = sh.sample_candidate_host(case["seed"], case["cand_base"] + i, max_draws=case["max_draws"], NI=U.MAX_INIT, chunk=37,
                                     **U.dims_kw(case))
        assert a["status"] == b["status"] and a["attempt"] == b["attempt"]
        if a["status"] == 0:
            assert all(np.array_equal(x, y) for x, y in zip(a["task"]["initial_states"], b["task"]["initial_states"]))


def test_zoh_host_against_the_yardstick():
    """zoh_host against (Phi, Gamma) to 50 digits: per case, relative to the largest entry, within
    max(2^-44, 8 x the error of build_dynamics_matrices on that case).  Measured: scipy 4e-19 .. 6.4e-16, zoh_host
    1.6e-19 .. 7.3e-15 (the largest at ns = 16, scale 50, s = 6)."""
    y = U.yardstick()
    n = len(y["ns"])
    assert n == 10 and set(y["ns"]) == {5, 16, 32}
    ss = []
    for c in range(n):
        ns, na = int(y["ns"][c]), int(y["na"][c])
        phi, gam, st, s = sh.zoh_host(y["A"][c, :ns, :ns], y["B"][c, :ns, :na], float(y["dt"][c]))
        assert st == sh.ZOH_OK
        ss.append(s)
        e_phi = U.rel_err(phi, y["phi_hi"][c, :ns, :ns], y["phi_lo"][c, :ns, :ns])
        e_gam = U.rel_err(gam, y["gam_hi"][c, :ns, :na], y["gam_lo"][c, :ns, :na])
        s_phi, s_gam = U.scipy_rel_err(y, c)
        print("case %d ns %d scale %g s %d: zoh_host %.2e %.2e scipy %.2e %.2e" % (c, ns, y["scale"][c], s, e_phi, e_gam, s_phi, s_gam))
        assert e_phi <= U.zoh_bound(s_phi) and e_gam <= U.zoh_bound(s_gam), (c, e_phi, e_gam)
    assert min(ss) == 0 and max(ss) >= 6


def test_zoh_host_reports_bad_inputs():
    A = np.eye(3)
    B = np.ones((3, 2))
    bad = A.copy()
    bad[1, 2] = np.nan
    assert sh.zoh_host(bad, B, 0.1)[2] == sh.ZOH_NONFINITE
    assert sh.zoh_host(A * 1e14, B, 0.1)[2] == sh.ZOH_SCALE_CAP
    phi, gam, st, _ = sh.zoh_host(A * 0.0, B, 0.1)
    assert st == sh.ZOH_OK and np.array_equal(phi, np.eye(3)) and np.allclose(gam, 0.1 * B, rtol=1e-15)


def test_zoh_host_rounds_like_scipy_on_the_sampled_tasks():
    """in fp32, zoh_host and build_dynamics_matrices give the same table entries on the accepted tasks of the fixed inputs
    (entries below 2^-20 of an array's largest aside): so the cap the GPU test puts on adjacent entries hides nothing"""
    from xenoverse_amd.linds.tables import build_dynamics_matrices
    for name in U.CASES:
        for c in U.host_candidates(name):
            if c["status"] != 0:
                continue
            t = c["task"]
            phi, gam, _ = build_dynamics_matrices(t["ld_A"], t["ld_B"], t["ld_X"], 0.1)
            for a, b in ((c["Phi"], phi), (c["Gamma"], gam)):
                a32, b32 = a.astype(np.float32), b.astype(np.float32)
                big = np.abs(b32) >= 2.0 ** -20 * np.abs(b32).max()
                assert np.array_equal(a32[big], b32[big])


def test_header_and_bindings():
    from xenoverse_amd import _lib
    txt = open(os.path.join(ROOT, "include", "xeno.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for sym in ("xv_linds_sample_tasks", "xv_linds_build_zoh"):
        assert re.search(r"\bint\s+%s\s*\(" % sym, code) and sym in _lib.SIGNATURES
    assert "xv_linds_cand_info" in code and "xv_linds_dense" in code
    assert re.search(r"#define\s+XV_ABI_VERSION\s+12\b", txt) and _lib.ABI_VERSION == 12
    from xenoverse_amd.linds import device_sampler as ds
    assert ds.INFO_DTYPE.itemsize == 144 and ds.INFO_DTYPE.fields["action_cost"][1] == 96
    import xenoverse_amd.linds as L
    for name in ("sample_tasks_device", "sample_candidates", "task_dicts_from_device", "build_tables_device"):
        assert callable(getattr(L, name))
