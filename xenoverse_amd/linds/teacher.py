"""LinDS MPC teacher: the host restatement of the reference's `LTISystemMPC` (xenoverse/linds/solver.py:16-125) and the
per-task tables of the device teacher (csrc/linds_mpc.hip, xv_linds_mpc_*).

The reference poses, per task and per env-step, the box-constrained QP

    min_U  1/2 U^T W_H U + f^T U    s.t.  -1 <= U <= 1,      U = [u_0; ...; u_{K-1}],  u_k in R^Nu

with (solver.py:36-92, quirks kept):
    W_Q = kron(diag(gamma^arange(K)), diag(target_valid)),   W_P = kron(eye(K) action_cost / max(reward_factor, 1e-6), eye(Nu))
    block (i, k) of H = C Phi^{K+1-i} Gamma for k < K - i (independent of k: row block K-1 holds C Phi^2 Gamma)
    block i of F1 = C Phi^{K-i},  block i of F2 = C Phi^{K+1-i} Xt + Y
    W_H = H^T W_Q H + W_P,   f = H^T W_Q (F1 x + F2 - Y_ref),  ref[i] in row block K-1-i of Y_ref (solver.py:98-110)
and hands it to OSQP (cold start, eps 1e-3).  Here `solve` returns the exact optimum instead (a bounded least-squares
solve on a factor of W_H), which is what OSQP approximates; when W_H is singular (action_cost = 0) the optimal U need not be
unique, the optimal objective is.

Device tables (`device_tables`): the teacher runs OSQP's ADMM with A = I on the device,
    x~ = M (sigma x - q + rho z - y),   M = (P + (sigma + rho) I)^-1   (factored here in fp64, stored fp32)
    x <- alpha x~ + (1 - alpha) x,  z <- clip(alpha x~ + (1 - alpha) z + y / rho),  y <- y + rho (alpha x~ + (1 - alpha) z_old - z)
with a per-task rho = sqrt(lambda_min lambda_max) of P (lambda_min floored at 1e-6 lambda_max), and forms the linear term
on the device as q = G_x x + g_0 - G_r vec(ref), the row-block reversal of Y_ref folded into G_r.
"""
import numpy as np

from .tables import build_dynamics_matrices

SIGMA = 1e-6
ALPHA = 1.6
EPS_ABS = 3e-6       # residual test of the device iteration (OSQP's default, 1e-3, leaves u_0 far from the optimum)
EPS_REL = 3e-6
RHO_FLOOR = 1e-6
N_MAX = 512          # n = K * Nu the device kernel supports


class _Model(object):
    """one task's LTI model in fp64: phi (Nx, Nx), gam (Nx, Nu), C (Ny, Nx), Xt (Nx,), Y (Ny,), valid (Ny,)"""

    def __init__(self, phi, gam, C, Xt, Y, valid, action_cost, reward_factor, pad_action_dim=8):
        self.phi, self.gam, self.C = np.asarray(phi, np.float64), np.asarray(gam, np.float64), np.asarray(C, np.float64)
        self.Xt, self.Y = np.asarray(Xt, np.float64).reshape(-1), np.asarray(Y, np.float64).reshape(-1)
        self.valid = np.asarray(valid, np.float64).reshape(-1)
        self.Nx, self.Nu, self.Ny = self.phi.shape[0], self.gam.shape[1], self.C.shape[0]
        self.action_cost, self.reward_factor = float(action_cost), float(reward_factor)
        self.Na = int(pad_action_dim)


def model_from_task(task, dt=0.1, pad_action_dim=8):
    """a reference task dict -> _Model, ZOH-discretised as LinearDSEnv.build_dynamics_matrices"""
    phi, gam, xt = build_dynamics_matrices(np.asarray(task["ld_A"], np.float64), np.asarray(task["ld_B"], np.float64),
                                           np.asarray(task["ld_X"], np.float64), dt)
    return _Model(phi, gam, task["ld_C"], xt, task["ld_Y"], task["target_valid"], task["action_cost"],
                  task["reward_factor"], pad_action_dim)


def model_from_env(env):
    """a reference-style env after set_task (attributes ld_phi, ld_gamma, ld_C, ld_Xt, ld_Y, target_valid, ...)"""
    return _Model(env.ld_phi, env.ld_gamma, env.ld_C, env.ld_Xt, env.ld_Y, env.target_valid, env.action_cost,
                  env.reward_factor, env.action_space.shape[0])


def model_from_tables(tab, t):
    """task t of the host tables of linds.tables.build_tables (fp32 values).  Nu is the task's action_dim, which the tables
    carry as `action_dims` (n = K Nu and W_P depend on it); Nx / Ny are the padded sizes (zero rows and columns change
    neither W_H nor f: padded observation rows carry target_valid = 0)."""
    if "action_dims" not in tab:
        raise ValueError("the MPC teacher needs the tables' `action_dims` (linds.tables.build_tables writes them)")
    phi = np.asarray(tab["phiT"][t], np.float64).T
    gam = np.asarray(tab["gamT"][t], np.float64).T
    nu = int(np.asarray(tab["action_dims"])[t])
    sc = np.asarray(tab["scal"][t], np.float64)
    return _Model(phi, gam[:, :nu], np.asarray(tab["cT"][t], np.float64).T, tab["xt"][t], tab["y0"][t], tab["valid"][t],
                  sc[0], sc[3], int(tab["NA"]))


def _model_of(env_or_task, task_index=0):
    if isinstance(env_or_task, _Model):
        return env_or_task
    if isinstance(env_or_task, dict) and "phiT" in env_or_task:
        return model_from_tables(env_or_task, task_index)
    if isinstance(env_or_task, dict):
        return model_from_task(env_or_task)
    if hasattr(env_or_task, "ld_phi"):
        return model_from_env(env_or_task)
    if hasattr(env_or_task, "mpc_models"):      # LinDSVecEnv
        return env_or_task.mpc_models()[task_index]
    raise TypeError("LTISystemMPC: expected a task dict, host tables, a reference-style env or a LinDSVecEnv")


class LTISystemMPC(object):
    """reference: xenoverse/linds/solver.py LTISystemMPC (:16-125), same signature and `solve`; the QP's exact optimum"""

    def __init__(self, env, K=20, gamma=0.99, task_index=0):
        m = _model_of(env, task_index)
        self.model = m
        self.Na, self.Nx, self.Nu, self.Ny = m.Na, m.Nx, m.Nu, m.Ny
        self.K, self.gamma = int(K), float(gamma)
        K, Nu, Ny = self.K, self.Nu, self.Ny
        # weights (:36-45), kept as diagonals
        self.wq = np.kron(gamma ** np.arange(K), m.valid)                          # diag of W_Q
        self.wp = np.full(K * Nu, m.action_cost / max(m.reward_factor, 1.0e-6))  # diag of W_P
        self.u_lb, self.u_ub = -np.ones(K * Nu), np.ones(K * Nu)
        # prediction model (:52-92): power p = K + 1 - i for row block i
        pw = [np.eye(self.Nx)]
        for _ in range(K + 1):
            pw.append(pw[-1] @ m.phi)
        p_row = K + 1 - np.arange(K)                                              # [K]
        CP = np.stack([m.C @ pw[p] for p in range(K + 2)])                       # C Phi^p
        CPG = CP[p_row] @ m.gam                                                   # [K, Ny, Nu]
        live = (np.arange(K)[None, :] < (K - np.arange(K))[:, None])              # block (i, k): k < K - i
        self.H = (CPG[:, :, None, :] * live[:, None, :, None]).reshape(K * Ny, K * Nu)
        self.F1 = CP[p_row - 1].reshape(K * Ny, self.Nx)
        self.F2 = (CP[p_row] @ m.Xt + m.Y[None, :]).reshape(K * Ny)
        self.HtWq = self.H.T * self.wq[None, :]                                   # H^T W_Q
        self.W_H = self.HtWq @ self.H + np.diag(self.wp)

    @property
    def n(self):
        return self.K * self.Nu

    def y_ref(self, ref_trajectory):
        """Y_ref of solve (:98-110): ref[i] -> row block K-1-i; 1-D: repeated; shorter than K: its last row repeats"""
        r = np.asarray(ref_trajectory, np.float64)
        K, Ny = self.K, self.Ny
        if r.ndim == 1:
            return np.tile(r[:Ny], K)
        idx = np.minimum(np.arange(K), r.shape[0] - 1)
        rows = r[idx, :Ny]                         # rows[i] = ref[min(i, len - 1)]
        return rows[::-1].reshape(K * Ny)          # row block K-1-i holds rows[i]

    def qp(self, x_current, ref_trajectory):
        """(P, q, lb, ub) of the QP solve() poses (:112-118)"""
        x = np.asarray(x_current, np.float64).reshape(-1)[:self.Nx]
        f = self.F1 @ x + self.F2 - self.y_ref(ref_trajectory)
        return self.W_H.copy(), self.HtWq @ f, self.u_lb.copy(), self.u_ub.copy()

    def objective(self, U, P=None, q=None, x_current=None, ref_trajectory=None):
        if P is None:
            P, q, _, _ = self.qp(x_current, ref_trajectory)
        U = np.asarray(U, np.float64)
        return 0.5 * U @ P @ U + q @ U

    def solve_qp(self, x_current, ref_trajectory):
        """the exact optimum U* (K * Nu) of the QP: bounded least squares min 1/2 |A U - b|^2, A^T A = W_H, A^T b = -q, with
        A = [W_Q^1/2 H; W_P^1/2] (the factor the QP is built from, so f lies in the range of A^T even when W_H is singular)"""
        from scipy.optimize import lsq_linear
        x = np.asarray(x_current, np.float64).reshape(-1)[:self.Nx]
        r = self.F1 @ x + self.F2 - self.y_ref(ref_trajectory)
        sq = np.sqrt(self.wq)
        A = np.vstack([self.H * sq[:, None], np.diag(np.sqrt(self.wp))])
        b = np.concatenate([-sq * r, np.zeros(self.n)])
        keep = np.any(A != 0.0, axis=1)
        res = lsq_linear(A[keep], b[keep], bounds=(self.u_lb, self.u_ub), method="bvls", tol=1e-13, max_iter=50 * self.n)
        return np.clip(res.x, -1.0, 1.0)

    def solve(self, x_current, ref_trajectory):
        """u = U*[:Nu], zero-padded to the env's padded action dim (:119-125)"""
        U = self.solve_qp(x_current, ref_trajectory)
        u = np.zeros(self.Na)
        u[:self.Nu] = U[:self.Nu]
        return u


def admm_params(P):
    """(rho, M) of the device iteration for one task's P (fp64)"""
    n = P.shape[0]
    lam = np.linalg.eigvalsh(P)
    lmax = float(lam[-1])
    if not lmax > 0.0:
        rho = 1.0
    else:
        rho = float(np.sqrt(max(float(lam[0]), RHO_FLOOR * lmax) * lmax))
    M = np.linalg.inv(P + (SIGMA + rho) * np.eye(n))
    return rho, 0.5 * (M + M.T)


def _frag(A):
    """A (rows, cols), both multiples of 16 -> the A-operand fragments of v_mfma_f32_16x16x4_f32 the kernel reads:
    [rows / 16][cols / 16][lane][4], lane (n, g) = 16 g + n, element r = A[16 mt + n][16 q + 4 g + r]"""
    R, Cc = A.shape
    return np.ascontiguousarray(A.reshape(R // 16, 16, Cc // 16, 4, 4).transpose(0, 2, 3, 1, 4).reshape(R // 16, Cc // 16, 64, 4))


def _up16(v):
    return (int(v) + 15) // 16 * 16


def device_tables(models, K, gamma, NS, NO):
    """per-task tables of the device teacher for `models` (one _Model per task), the env's padded NS and NO.

    Returns a dict: n_pad (n = K Nu padded to 16), n_in (input rows: NS state rows then K x NOc command rows, padded to 16),
    NOc (command columns the teacher reads: the live observation columns rounded up to 4), nu int32[n_task],
    rho / inv_rho float32[n_task], mnorm float32[n_task] (|M|_inf of the fp32 operator),
    mfrag float32[n_task][n_pad/16][n_pad/16][64][4] (M), gfrag float32[n_task][n_pad/16]
    [n_in/16][64][4] ([G_x | -G_r]), g0 float32[n_task][n_pad], and the fp64 maps G_x, g_0, G_r (unpadded, per task lists)
    the host tests check."""
    memo = {}      # a model object repeated over many task indices is built and factored once
    for m in models:
        if id(m) not in memo:
            memo[id(m)] = LTISystemMPC(m, K=K, gamma=gamma)
    mpcs = [memo[id(m)] for m in models]
    n_task = len(mpcs)
    n_max = max(p.n for p in mpcs)
    if n_max > N_MAX:
        raise ValueError("K * action_dim = %d exceeds the device teacher's maximum %d" % (n_max, N_MAX))
    ny_max = max(p.Ny for p in mpcs)
    NOc = min((max(int(np.nonzero(p.model.valid)[0][-1]) + 1 if np.any(p.model.valid) else 1 for p in mpcs) + 3) // 4 * 4,
              (ny_max + 3) // 4 * 4)
    NOc = max(NOc, 4)
    if NOc > NO:
        raise ValueError("observation dim exceeds the env's padded NO")
    n_pad, n_in = _up16(n_max), _up16(NS + K * NOc)
    mfrag = np.zeros((n_task, n_pad // 16, n_pad // 16, 64, 4), np.float32)
    gfrag = np.zeros((n_task, n_pad // 16, n_in // 16, 64, 4), np.float32)
    g0 = np.zeros((n_task, n_pad), np.float32)
    rho = np.zeros(n_task, np.float64)
    mnorm = np.zeros(n_task, np.float32)
    nu = np.zeros(n_task, np.int32)
    Gx, G0, Gr = [], [], []
    done = {}
    for t, p in enumerate(mpcs):
        n = p.n
        if id(p) in done:      # the same task again: copy its rows
            s = done[id(p)]
            mfrag[t], gfrag[t], g0[t], rho[t], mnorm[t], nu[t] = mfrag[s], gfrag[s], g0[s], rho[s], mnorm[s], nu[s]
            Gx.append(Gx[s]); G0.append(G0[s]); Gr.append(Gr[s])
            continue
        done[id(p)] = t
        r_t, M = admm_params(p.W_H)
        rho[t], nu[t] = r_t, p.Nu
        Mp = np.zeros((n_pad, n_pad))
        Mp[:n, :n] = M
        M32 = Mp.astype(np.float32)
        mfrag[t] = _frag(M32)
        mnorm[t] = np.abs(M32).sum(axis=1, dtype=np.float64).max()
        gx = p.HtWq @ p.F1                                     # [n, Nx]
        gz = p.HtWq @ p.F2                                     # [n]
        # vec(ref)[j * NOc + c] = ref[j][c] enters Y_ref row (K-1-j) Ny + c
        gr = np.zeros((n, K, NOc))
        hw = p.HtWq.reshape(n, K, p.Ny)[:, ::-1, :]           # [n, j, c] = (H^T W_Q)[:, (K-1-j) Ny + c]
        nc = min(p.Ny, NOc)
        gr[:, :, :nc] = hw[:, :, :nc]
        Gx.append(gx); G0.append(gz); Gr.append(gr.reshape(n, K * NOc))
        A = np.zeros((n_pad, n_in))
        A[:n, :p.Nx] = gx
        A[:n, NS:NS + K * NOc] = -gr.reshape(n, K * NOc)
        gfrag[t] = _frag(A.astype(np.float32))
        g0[t, :n] = gz
    return dict(K=int(K), gamma=float(gamma), n_pad=n_pad, n_in=n_in, NOc=NOc, NS=int(NS), NO=int(NO), nu=nu,
                rho=rho.astype(np.float32), inv_rho=(1.0 / rho).astype(np.float32), mnorm=mnorm, mfrag=mfrag, gfrag=gfrag, g0=g0,
                G_x=Gx, g_0=G0, G_r=Gr)
