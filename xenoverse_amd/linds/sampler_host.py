"""Host restatement (numpy, fp64) of the device LinDS task sampler and zero-order-hold builder
(csrc/linds_sampler.hip: xv_linds_sample_tasks, xv_linds_build_zoh): the same Philox counters, the same draw
constructions and the same formulas in the same order, vectorised over start attempts.  It is what the device is
compared with (tests/test_gpu_linds_sampler.py), as MetaLangV1Host and HVACHost are for their families.

Counter layout (include/xeno.h): key = seed; counter = {candidate lo, candidate hi, stream, draw}.  stream 0 is the
candidate's head, stream 1 + a is start attempt a.  One Philox call `draw` gives two uniforms (words 0,1 and words 2,3 by
xv_u53) or one Box-Muller pair (radius from the first uniform, angle from the second).  Element n of a block of normals
is member n & 1 of call base + (n >> 1); element q of a block of uniforms is half q & 1 of call base + (q >> 1).
"""
import numpy as np

from ..host_draws import box_muller, expo, floor_int, interleave, pair, philox4x32_10
from .tables import KMAX

STATUS = ("accepted", "exhausted", "zoh_failed")
A_SCALES = (0.01, 0.02, 0.05, 0.1, 0.2)
X_SCALES = (0.0, 0.05, 0.1)

# head stream (stream 0): draw indices
H_DIMS, H_DIMS2, H_SCALE, H_TRIM, H_COST, H_REWARD, H_PUNISH, H_TARGET = 0, 1, 2, 3, 4, 5, 6, 7
H_AB, H_X, H_C, H_VALID = 0x1000, 0x2000, 0x3000, 0x10000      # blocks; H_VALID + 16 * round
VALID_ROUNDS = 1 << 16
# attempt stream (stream 1 + a)
S_BORN, S_CMD, S_ORDER_INT, S_ORDER_Z, S_STATIC, S_FOURIER, S_STATES = 0, 1, 2, 8, 16, 64, 1024
# S_FOURIER + 64 k: 32 calls of normals then 32 calls of uniforms (exponentials) of term k; S_STATES + 16 i: state i

ZOH_TERMS = 18          # S(h) = sum_{k < 18} A^k h^{k+1} / (k+1)!
ZOH_THETA = 0.25        # |A h|_inf <= 0.25 after scaling
ZOH_S_CAP = 40          # more halvings than this: status, not a table
ZOH_OK, ZOH_NONFINITE, ZOH_SCALE_CAP = 0, 1, 2


class _Stream(object):
    """draws of one (seed, candidate) over an array of streams"""

    def __init__(self, seed, cand, streams):
        seed, cand = int(seed) & (2**64 - 1), int(cand)
        self.key = np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint32)
        self.c01 = (cand & 0xFFFFFFFF, (cand >> 32) & 0xFFFFFFFF)
        self.streams = np.asarray(streams, np.uint32).reshape(-1)

    def pairs(self, draws):
        """draws int[...] -> (u_a, u_b) float64[n_streams, ...]"""
        d = np.asarray(draws, np.uint32)
        ctr = np.empty((len(self.streams),) + d.shape + (4,), np.uint32)
        ctr[..., 0], ctr[..., 1] = self.c01
        ctr[..., 2] = self.streams.reshape((-1,) + (1,) * d.ndim)
        ctr[..., 3] = d
        return pair(philox4x32_10(ctr, self.key))

    def uniforms(self, base, n):
        """block of n uniforms -> float64[n_streams, n]"""
        q = np.arange(n)
        return interleave(q, *self.pairs(base + (q >> 1)))

    def normals(self, base, n):
        """block of n normals (fp64 Box-Muller) -> float64[n_streams, n]"""
        q = np.arange(n)
        return interleave(q, *box_muller(*self.pairs(base + (q >> 1))))


def random_dims(u_ns, u_na, u_no, max_ns, max_no, max_na):
    """LinearDSSamplerRandomDim's dims (task_sampler.py:134-154) from three uniforms"""
    ns = 1 + int(np.floor(u_ns * max_ns))
    min_na = max(1, (ns + 1) // 2)
    hi_na = max(min(max_na, ns * 3 // 2), min_na)
    min_no = max(1, ns // 4)
    hi_no = max(min(max_no, ns * 3 // 2), min_no)
    na = min_na + int(np.floor(u_na * (hi_na - min_na + 1)))
    no = min_no + int(np.floor(u_no * (hi_no - min_no + 1)))
    return ns, na, no


def sample_head(seed, cand, ns=16, na=8, no=8, random_dim=False):
    """the candidate's head: sample_variants_ and lines 86-105 of the reference's LinearDSSampler.
    With random_dim, (ns, na, no) are the maxima (max_ns, max_na, max_no)."""
    st = _Stream(seed, cand, [0])
    ua, ub = st.pairs(np.arange(8))
    ua, ub = ua[0], ub[0]
    if random_dim:
        ns, na, no = random_dims(ua[H_DIMS], ub[H_DIMS], ua[H_DIMS2], ns, no, na)
    h = dict(ns=int(ns), na=int(na), no=int(no))
    h["max_steps"] = 100 + int(np.floor(ub[H_DIMS2] * 900))
    h["a_scale"], h["x_scale"] = int(np.floor(ua[H_SCALE] * 5)), int(np.floor(ub[H_SCALE] * 3))
    h["trim"] = int(np.floor(ua[H_TRIM] * 3))
    if h["trim"] == 0:
        h["width"] = 2 + int(np.floor(ub[H_TRIM] * (max(ns // 2, 3) - 1)))
    elif h["trim"] == 1:
        h["width"] = -1 + int(np.floor(ub[H_TRIM] * (max(ns // 4, 2) + 2)))
    else:
        h["width"] = 0
    std_ab = np.sqrt(2.0 / (2 * ns + na))
    AB = (st.normals(H_AB, ns * (ns + na))[0] * std_ab * 3.0).reshape(ns, ns + na)
    X = (0.1 * st.normals(H_X, ns)[0]) * X_SCALES[h["x_scale"]]
    C = (st.normals(H_C, no * ns)[0] * np.sqrt(2.0 / (ns + no)) * 3.0).reshape(no, ns)
    A = AB[:, :ns] * A_SCALES[h["a_scale"]]
    i, j = np.indices((ns, ns))
    if h["trim"] == 0 and h["width"] < ns:
        A = np.where(np.abs(i - j) > h["width"], 0.0, A)
    elif h["trim"] == 1 and h["width"] < ns:
        A = np.where(j < i + h["width"], 0.0, A)
    h.update(A=A, B=np.ascontiguousarray(AB[:, ns:]), C=C, X=X, Y=np.zeros(no))
    h["action_cost"] = max((-1.0 + 2.0 * ua[H_COST]) * (expo(ub[H_COST]) * 0.05), 0.0)
    h["reward_base"] = expo(ua[H_REWARD]) * 0.10
    h["terminate_punish"] = (expo(ub[H_REWARD]) * 5.0) * (0.0 if int(np.floor(ua[H_PUNISH] * 3)) == 0 else 1.0)
    h["reward_factor"] = expo(ub[H_PUNISH]) * 0.50
    h["eps"] = min(0.2 + ua[H_TARGET], 1.0)
    h["type"] = 1 if int(np.floor(ub[H_TARGET] * 3)) < 2 else 0          # 1 dynamic_target, 0 static_target
    for rnd in range(VALID_ROUNDS):
        tv = (st.uniforms(H_VALID + 16 * rnd, no)[0] < h["eps"]).astype(np.int64)
        if tv.sum() > 0:
            break
    h["target_valid"], h["valid_rounds"] = tv, rnd + 1
    return h


def eval_attempts(seed, cand, head, attempts, NI=8):
    """start attempts (array of indices) of one candidate -> dict of arrays over attempts: born_loc, noise_drift, the command
    (static values or Fourier terms), the initial states, the two norms of every live state and `ok`"""
    ns, no = head["ns"], head["no"]
    attempts = np.asarray(attempts, np.int64)
    n = len(attempts)
    st = _Stream(seed, cand, 1 + attempts)
    ua, ub = st.pairs(np.arange(2))
    e = expo(ua[:, S_BORN])
    born = np.maximum(e, 1.0).astype(np.int64)
    r = dict(attempt=attempts, born_e=e, born_loc=born, noise_drift=np.clip(-0.02 + 0.04 * ub[:, S_BORN], 0.0, 0.02))
    if head["type"] == 0:
        gate = floor_int(ua[:, S_CMD], 2).astype(np.float64)
        cmd0 = st.normals(S_STATIC, no) * gate[:, None]
        r.update(cmd0=cmd0, delay=np.zeros(n, np.int64), n_terms=np.zeros(n, np.int64))
        cmd = cmd0
    else:
        n_items = 1 + floor_int(ua[:, S_CMD], 5)
        delay = np.maximum(-10 + floor_int(ub[:, S_CMD], 40), 0)
        k = np.arange(1, KMAX)
        oi, _ = st.pairs(S_ORDER_INT + k)
        za, zb = st.pairs(S_ORDER_Z + k)
        orders = np.zeros((n, KMAX))
        orders[:, 1:] = (1 + floor_int(oi, 16)) + box_muller(za, zb)[0]
        scale = 2.0 / np.sqrt(n_items.astype(np.float64))
        coef = np.empty((n, KMAX, no, 2))
        for t in range(KMAX):
            z = st.normals(S_FOURIER + 64 * t, 2 * no)
            ex = expo(st.uniforms(S_FOURIER + 64 * t + 32, 2 * no)) * scale[:, None]
            coef[:, t] = (z * ex).reshape(n, no, 2)
        live = np.arange(KMAX)[None, :] <= n_items[:, None]
        orders = np.where(live, orders, 0.0)
        coef = np.where(live[:, :, None, None], coef, 0.0)
        x = -delay.astype(np.float64) / 1000.0
        cmd = np.zeros((n, no))
        for t in range(KMAX):      # fixed order of the sum; dead terms contribute exactly 0
            ang = orders[:, t] * x
            term = coef[:, t, :, 0] * np.sin(ang)[:, None] + coef[:, t, :, 1] * np.cos(ang)[:, None]
            cmd = np.where(live[:, t, None], cmd + term, cmd)
        r.update(orders=orders, coef=coef, delay=delay, n_terms=1 + n_items)
    states = np.zeros((n, NI, ns))
    for i in range(NI):
        states[:, i] = st.normals(S_STATES + 16 * i, ns)
    C, Y, tv = head["C"], head["Y"], head["target_valid"].astype(np.float64)
    dev2 = np.zeros((n, NI))
    x2 = np.zeros((n, NI))
    for o in range(no):
        y = np.zeros((n, NI))
        for j in range(ns):
            y = y + C[o, j] * states[:, :, j]
        d = (cmd[:, None, o] - y - Y[o]) * tv[o]
        dev2 = dev2 + d * d
    for j in range(ns):
        x2 = x2 + states[:, :, j] * states[:, :, j]
    dev_norm, x_norm = np.sqrt(dev2), np.sqrt(x2)
    live_state = np.arange(NI)[None, :] < born[:, None]
    bad = ((dev_norm > 3.0) | (x_norm > 10.0)) & live_state
    r.update(states=states, dev_norm=dev_norm, x_norm=x_norm, live_state=live_state,
             ok=(born <= NI) & ~bad.any(axis=1))
    return r


def zoh_host(A, B, dt):
    """the kernel's zero-order hold: Phi = e^{A dt}, Gamma = (int_0^dt e^{A tau} d tau) B on ns x ns matrices.
    M = A h, h = dt / 2^s with |M|_inf <= 0.25; P = Horner form of sum_{k<18} M^k / (k+1)!; S = h P; Phi = I + M P;
    s doublings S <- S + Phi S, Phi <- Phi Phi; Gamma = S B.  Every product sums k = 0, 1, ... in order with separate
    multiply and add.  -> (Phi, Gamma, status, s)"""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    ns = A.shape[0]
    zero = (np.zeros((ns, ns)), np.zeros((ns, B.shape[1])))
    if not (np.all(np.isfinite(A)) and np.all(np.isfinite(B)) and np.isfinite(dt)):
        return zero + (ZOH_NONFINITE, 0)
    norm = 0.0
    for i in range(ns):
        row = 0.0
        for j in range(ns):
            row = row + abs(A[i, j])
        norm = max(norm, row)
    norm = norm * abs(dt)
    s = 0
    while norm > ZOH_THETA and s <= ZOH_S_CAP:
        norm, s = norm * 0.5, s + 1
    if s > ZOH_S_CAP:
        return zero + (ZOH_SCALE_CAP, s)
    h = dt * 0.5 ** s

    def mm(a, b):
        acc = np.zeros((a.shape[0], b.shape[1]))
        for k in range(a.shape[1]):
            acc = acc + a[:, k, None] * b[None, k, :]
        return acc
    eye = np.eye(ns)
    M = A * h
    P = eye.copy()
    for k in range(ZOH_TERMS, 1, -1):
        P = eye + mm(M, P) / float(k)
    S = P * h
    Phi = eye + mm(M, P)
    for _ in range(s):
        S = S + mm(Phi, S)
        Phi = mm(Phi, Phi)
    Gam = mm(S, B)
    if not (np.all(np.isfinite(Phi)) and np.all(np.isfinite(Gam))):
        return zero + (ZOH_NONFINITE, s)
    return Phi, Gam, ZOH_OK, s


class FourierCommand(object):
    """the command of a dynamic task as `linds.tables.fourier_terms` and the reference env read it: `coeffs` is a list of
    (order, ndarray[no, 2]), `max_steps` the period (RandomFourier, utils/random_nn.py:346-368)"""

    def __init__(self, orders, coefs, max_steps=1000):
        self.coeffs = [(float(o), np.array(c, np.float64)) for o, c in zip(orders, coefs)]
        self.max_steps = max_steps

    def __call__(self, t):
        x = t / self.max_steps
        y = 0
        for order, coeff in self.coeffs:
            y = y + coeff[:, 0] * np.sin(order * x) + coeff[:, 1] * np.cos(order * x)
        return y


def task_dict(head, born_loc, noise_drift, delay, states, cmd0=None, orders=None, coef=None, n_terms=0):
    """reference-schema task dict (keys and dtypes of LinearDSSampler's)"""
    ns, na, no = head["ns"], head["na"], head["no"]
    t = dict(state_dim=ns, observation_dim=no, action_dim=na, max_steps=int(head["max_steps"]),
             ld_A=np.array(head["A"], np.float64), ld_B=np.array(head["B"], np.float64), ld_C=np.array(head["C"], np.float64),
             ld_X=np.array(head["X"], np.float64), ld_Y=np.array(head["Y"], np.float64),
             action_cost=float(head["action_cost"]), reward_base=float(head["reward_base"]),
             terminate_punish=float(head["terminate_punish"]), reward_factor=float(head["reward_factor"]),
             target_valid=np.array(head["target_valid"], np.int64),
             target_type="dynamic_target" if head["type"] else "static_target",
             noise_drift=float(noise_drift), target_delay=int(delay),
             initial_states=[np.array(states[i][:ns], np.float64) for i in range(int(born_loc))])
    if head["type"]:
        n_terms = int(n_terms)
        t["command"] = FourierCommand(orders[:n_terms], coef[:n_terms, :no])
    else:
        t["command"] = np.array(cmd0[:no], np.float64)
    return t


def sample_candidate_host(seed, cand, state_dim=16, action_dim=8, observation_dim=8, random_dim=False, dt=0.1,
                          max_draws=1 << 20, NI=8, chunk=512, with_zoh=True, keep_evaluated=False):
    """candidate `cand` of (seed, dims arguments) as the kernel makes it -> dict(status, attempt, head, task (reference
    task dict, accepted only), Phi, Gamma, zoh_s, evaluated (with keep_evaluated: the eval_attempts records up to the
    accepted attempt))"""
    head = sample_head(seed, cand, state_dim, action_dim, observation_dim, random_dim)
    out = dict(status=1, attempt=-1, head=head, task=None)
    kept = []
    for base in range(0, int(max_draws), chunk):
        r = eval_attempts(seed, cand, head, np.arange(base, min(base + chunk, int(max_draws))), NI)
        hit = np.nonzero(r["ok"])[0]
        if keep_evaluated:
            cut = len(r["ok"]) if len(hit) == 0 else hit[0] + 1
            kept.append({k: v[:cut] for k, v in r.items()})
        if len(hit):
            w = hit[0]
            out.update(status=0, attempt=int(r["attempt"][w]))
            kw = dict(cmd0=r["cmd0"][w]) if head["type"] == 0 else dict(orders=r["orders"][w], coef=r["coef"][w],
                                                                        n_terms=r["n_terms"][w])
            out["task"] = task_dict(head, r["born_loc"][w], r["noise_drift"][w], r["delay"][w], r["states"][w], **kw)
            out["n_init"], out["n_terms"], out["delay"] = int(r["born_loc"][w]), int(r["n_terms"][w]), int(r["delay"][w])
            break
    if keep_evaluated:
        out["evaluated"] = kept
    if out["status"] == 0 and with_zoh:
        out["Phi"], out["Gamma"], zst, out["zoh_s"] = zoh_host(head["A"], head["B"], dt)
        if zst != ZOH_OK:
            out["status"] = 2
    return out


def start_margins(seed, cand, NI=8, max_draws=1 << 20, chunk=512, **dims):
    """the smallest distance, over every evaluated attempt of the candidate (those up to the accepted one), of the two norms
    of a live start state from their thresholds 3 and 10, and of -log(1-u) from an integer where born_loc is formed:
    how far the accept / reject decisions are from depending on the last bits of log, sin and cos"""
    c = sample_candidate_host(seed, cand, NI=NI, max_draws=max_draws, chunk=chunk, with_zoh=False, keep_evaluated=True, **dims)
    m = np.inf
    for r in c["evaluated"]:
        e = r["born_e"][r["born_e"] >= 1.0]
        if len(e):
            m = min(m, float(np.min(np.abs(e - np.round(e))[np.round(e) >= 2.0], initial=np.inf)))
        live = r["live_state"] & (r["born_loc"] <= NI)[:, None]
        if live.any():
            m = min(m, float(np.min(np.abs(r["dev_norm"][live] - 3.0))), float(np.min(np.abs(r["x_norm"][live] - 10.0))))
    return m
