"""The host restatement of the reference's LinDS MPC teacher (xenoverse_amd/linds/teacher.py) against the QPs the reference
itself poses (tests/golden/mpc_linds_*.npz, scripts/gen_golden_linds_mpc.py), and the device teacher's tables (CPU only)."""
import glob
import os
import re

import numpy as np
import pytest

from xenoverse_amd.linds import teacher

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "mpc_linds_*.npz")))
IDS = [os.path.basename(p)[len("mpc_linds_"):-4] for p in GOLDEN]


def load(path):
    z = np.load(path, allow_pickle=False)
    g = {k: z[k] for k in z.files}
    task = {k[5:]: g[k] for k in g if k.startswith("task_")}
    for k in ("state_dim", "action_dim", "observation_dim", "max_steps", "target_delay"):
        task[k] = int(task[k])
    for k in ("action_cost", "reward_factor"):
        task[k] = float(task[k])
    task["target_type"] = str(task["target_type"])
    return g, task


def mpc_of(g, task):
    return teacher.LTISystemMPC(teacher.model_from_task(task, dt=float(g["dt"]), pad_action_dim=int(g["pad_action_dim"])),
                                K=int(g["K"]), gamma=float(g["gamma"]))


def test_golden_cover_the_cases():
    assert len(GOLDEN) >= 10
    ks = {int(np.load(p)["K"]) for p in GOLDEN}
    assert ks == {20, 50}
    kinds = {str(np.load(p)["ref_kind"]) for p in GOLDEN}
    assert {"full", "vector", "short"} <= kinds
    zs = [np.load(p) for p in GOLDEN]
    assert any(int(z["task_target_delay"]) + 1 > int(z["K"]) for z in zs)
    assert any(float(z["task_action_cost"]) == 0.0 for z in zs) and any(float(z["task_action_cost"]) > 0.0 for z in zs)
    assert any(str(z["task_target_type"]) == "static_target" for z in zs)
    assert any(int(z["steps"]) == 0 for z in zs) and any(int(z["steps"]) >= int(z["task_max_steps"]) - 2 for z in zs)


@pytest.mark.parametrize("path", GOLDEN, ids=IDS)
def test_qp_matches_the_reference(path):
    g, task = load(path)
    mpc = mpc_of(g, task)
    P, q, lb, ub = mpc.qp(g["x"], g["ref"])
    assert P.shape == g["P"].shape
    assert np.abs(P - g["P"]).max() <= 1e-10 * np.abs(g["P"]).max()
    assert np.abs(q - g["q"]).max() <= 1e-10 * max(np.abs(g["q"]).max(), 1e-300)
    assert np.array_equal(lb, g["l"]) and np.array_equal(ub, g["u"])


@pytest.mark.parametrize("path", GOLDEN, ids=IDS)
def test_solve_is_the_optimum(path):
    g, task = load(path)
    mpc = mpc_of(g, task)
    P, q = g["P"], g["q"]
    U = mpc.solve_qp(g["x"], g["ref"])
    J, Js = 0.5 * U @ P @ U + q @ U, float(g["J_opt"])
    assert np.all(np.abs(U) <= 1.0)
    assert abs(J - Js) <= 1e-9 * (1.0 + abs(Js)), (J, Js)
    # KKT on the box: the gradient vanishes inside, pushes outward on an active bound
    grad = P @ U + q
    tol = 1e-7 * (np.abs(P).max() + np.abs(q).max())
    inner = np.abs(U) < 1.0 - 1e-9
    assert np.all(np.abs(grad[inner]) <= tol)
    assert np.all(grad[U >= 1.0 - 1e-9] <= tol) and np.all(grad[U <= -1.0 + 1e-9] >= -tol)


@pytest.mark.parametrize("path", GOLDEN[:3], ids=IDS[:3])
def test_solve_pads_the_action(path):
    g, task = load(path)
    mpc = mpc_of(g, task)
    u = mpc.solve(g["x"], g["ref"])
    nu = int(task["action_dim"])
    assert u.shape == (int(g["pad_action_dim"]),)
    assert np.all(u[nu:] == 0.0)
    assert np.array_equal(u[:nu], mpc.solve_qp(g["x"], g["ref"])[:nu])


def test_y_ref_quirks():
    """ref[i] -> row block K-1-i; a 1-D ref repeats; a short ref repeats its last row (solver.py:98-110)"""
    _, task = load(GOLDEN[0])
    mpc = teacher.LTISystemMPC(task, K=4)
    Ny = mpc.Ny
    r = np.arange(3 * Ny, dtype=np.float64).reshape(3, Ny)
    y = mpc.y_ref(r).reshape(4, Ny)
    assert np.array_equal(y[3], r[0]) and np.array_equal(y[2], r[1]) and np.array_equal(y[1], r[2])
    assert np.array_equal(y[0], r[2])
    assert np.array_equal(mpc.y_ref(r[1]).reshape(4, Ny), np.tile(r[1], (4, 1)))


@pytest.mark.parametrize("path", GOLDEN, ids=IDS)
def test_device_maps_reproduce_q(path):
    g, task = load(path)
    K = int(g["K"])
    model = teacher.model_from_task(task, dt=float(g["dt"]), pad_action_dim=int(g["pad_action_dim"]))
    NS = 16 if model.Nx <= 16 else 32
    dt = teacher.device_tables([model], K, float(g["gamma"]), NS, 16)
    NOc, n = dt["NOc"], model.Nu * K
    # the commands as the device reads them: ref[j] for j < K (after the reference's 1-D / short-ref padding)
    r = np.asarray(g["ref"], np.float64)
    rows = np.tile(r, (K, 1)) if r.ndim == 1 else r[np.minimum(np.arange(K), r.shape[0] - 1)]
    w = np.zeros((K, NOc))
    c = min(rows.shape[1], NOc)
    w[:, :c] = rows[:, :c]
    x = np.zeros(NS)
    x[:model.Nx] = g["x"]
    q = dt["G_x"][0] @ x[:model.Nx] + dt["g_0"][0] - dt["G_r"][0] @ w.reshape(-1)
    assert np.abs(q - g["q"]).max() <= 1e-9 * max(np.abs(g["q"]).max(), 1e-300)
    # the fp32 fragments are the padded operators in the kernel's A-operand order
    npad, nin = dt["n_pad"], dt["n_in"]
    assert npad % 16 == 0 and nin % 16 == 0 and npad >= n and nin >= NS + K * NOc
    Gfull = np.zeros((npad, nin))
    Gfull[:n, :model.Nx] = dt["G_x"][0]
    Gfull[:n, NS:NS + K * NOc] = -dt["G_r"][0]
    unf = dt["gfrag"][0].reshape(npad // 16, nin // 16, 4, 16, 4).transpose(0, 3, 1, 2, 4).reshape(npad, nin)
    assert np.array_equal(unf, Gfull.astype(np.float32))
    q32 = unf.astype(np.float64) @ np.concatenate([x, w.reshape(-1), np.zeros(nin - NS - K * NOc)]) + dt["g0"][0]
    assert np.abs(q32[:n] - g["q"]).max() <= 1e-4 * max(np.abs(g["q"]).max(), 1.0)
    assert np.all(q32[n:] == 0.0)
    M = dt["mfrag"][0].reshape(npad // 16, npad // 16, 4, 16, 4).transpose(0, 3, 1, 2, 4).reshape(npad, npad)
    rho = float(dt["rho"][0])
    Pp = g["P"] + (teacher.SIGMA + rho) * np.eye(n)
    assert np.abs(M[:n, :n].astype(np.float64) @ Pp - np.eye(n)).max() < 1e-3
    assert np.all(M[n:] == 0.0) and np.all(M[:, n:] == 0.0)


def test_device_tables_refuse_n_over_512():
    _, task = load(GOLDEN[0])
    model = teacher.model_from_task(task)
    K = 512 // model.Nu + 1
    with pytest.raises(ValueError):
        teacher.device_tables([model], K, 0.99, 16, 16)


def test_mpc_abi_is_declared_and_bound():
    from xenoverse_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "xeno.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(xv_[a-z0-9_]+)\s*\(", txt))
    for s in ("xv_linds_mpc_create", "xv_linds_mpc_destroy", "xv_linds_mpc_action", "xv_linds_mpc_solve",
              "xv_linds_rollout_mpc"):
        assert s in declared and s in _lib.SIGNATURES
    assert _lib.ABI_VERSION == 12
    if os.path.exists(_lib.LIB_PATH):
        import ctypes
        lib = ctypes.CDLL(_lib.LIB_PATH)
        assert hasattr(lib, "xv_linds_mpc_solve") and hasattr(lib, "xv_linds_rollout_mpc")


def test_tables_carry_action_dim():
    """the teacher built from host tables poses the task-dict QP: action_dim comes from the tables, not from Gamma"""
    from xenoverse_amd.linds import build_tables
    g, task = load([p for p in GOLDEN if "static_start" in p][0])
    task = dict(task, initial_states=list(g["task_initial_states"]), command=g["task_command"])
    tab = build_tables([task], dt=float(g["dt"]))
    assert int(tab["action_dims"][0]) == task["action_dim"]
    m = teacher.model_from_tables(tab, 0)
    assert m.Nu == task["action_dim"]
    P = teacher.LTISystemMPC(m, K=int(g["K"])).W_H
    assert P.shape == g["P"].shape
    assert np.abs(P - g["P"]).max() <= 1e-5 * np.abs(g["P"]).max()      # fp32 tables
    tab.pop("action_dims")
    with pytest.raises(ValueError):
        teacher.model_from_tables(tab, 0)
