"""Writes tests/golden/zoh_linds_yardstick.npz: the zero-order-hold pair (Phi, Gamma) of ten LinDS dynamics to ~32
digits, the yardstick `zoh_host` (linds/sampler_host.py) and xv_linds_build_zoh are measured against.

Cases: five sampled (A, B) — the reference's sample_variants_ as linds.task_sampler restates it, ns in {5, 5, 16, 16, 32},
na = 8 (4 at ns = 5) — each at scale 1 and with A scaled by 50, so that the kernel's halving count s runs from
0 to about 7.  dt = 0.1, one task at 0.05.  Exact values: the reference's own block formula (linds_env.py:67-76:
E = expm([[A, I], [0, 0]] dt), Phi = E[:ns, :ns], Gamma = E[:ns, ns:] B) evaluated with mpmath at 50 digits and stored
as hi + lo fp64 pairs (hi = the value rounded to fp64, lo = the remainder rounded to fp64).  The file name does not start
with `linds_`: that prefix is what the LinDS task fixtures are globbed by.

    python scripts/gen_linds_zoh_yardstick.py          (about a minute)
"""
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from xenoverse_amd.linds.task_sampler import _sample_variants  # noqa: E402

NS_PAD, NA_PAD = 32, 8
CASES = [(5, 4, 11, 0.1), (5, 4, 12, 0.05), (16, 8, 13, 0.1), (16, 8, 14, 0.1), (32, 8, 15, 0.1)]   # ns, na, seed, dt
SCALES = (1.0, 50.0)


def exact_zoh(A, B, dt):
    ns = A.shape[0]
    M = mp.zeros(2 * ns, 2 * ns)
    for i in range(ns):
        for j in range(ns):
            M[i, j] = mp.mpf(float(A[i, j])) * mp.mpf(float(dt))
        M[i, ns + i] = mp.mpf(float(dt))
    E = mp.expm(M)
    phi = E[:ns, :ns]
    gam = E[:ns, ns:] * mp.matrix(B.tolist())
    return phi, gam


def split(m):
    hi = np.array([[float(m[i, j]) for j in range(m.cols)] for i in range(m.rows)])
    lo = np.array([[float(m[i, j] - mp.mpf(hi[i, j])) for j in range(m.cols)] for i in range(m.rows)])
    return hi, lo


def main():
    mp.mp.dps = 50
    n = len(CASES) * len(SCALES)
    out = dict(ns=np.zeros(n, np.int32), na=np.zeros(n, np.int32), dt=np.zeros(n), scale=np.zeros(n),
               A=np.zeros((n, NS_PAD, NS_PAD)), B=np.zeros((n, NS_PAD, NA_PAD)),
               phi_hi=np.zeros((n, NS_PAD, NS_PAD)), phi_lo=np.zeros((n, NS_PAD, NS_PAD)),
               gam_hi=np.zeros((n, NS_PAD, NA_PAD)), gam_lo=np.zeros((n, NS_PAD, NA_PAD)))
    c = 0
    for ns, na, seed, dt in CASES:
        A0, B, _, _, _ = _sample_variants(np.random.RandomState(seed), ns, na, 8)
        for scale in SCALES:
            A = A0 * scale
            phi, gam = exact_zoh(A, B, dt)
            out["ns"][c], out["na"][c], out["dt"][c], out["scale"][c] = ns, na, dt, scale
            out["A"][c, :ns, :ns], out["B"][c, :ns, :na] = A, B
            out["phi_hi"][c, :ns, :ns], out["phi_lo"][c, :ns, :ns] = split(phi)
            out["gam_hi"][c, :ns, :na], out["gam_lo"][c, :ns, :na] = split(gam)
            print("case %d: ns %d scale %g dt %g |A|inf dt %.3g" % (c, ns, scale, dt, np.abs(A).sum(1).max() * dt))
            c += 1
    path = os.path.join(ROOT, "tests", "golden", "zoh_linds_yardstick.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
