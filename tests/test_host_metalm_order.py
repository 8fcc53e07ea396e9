"""What csrc/metalm.hip relies on to follow the host bit for bit, checked on the CPU against numpy itself:
the table and polynomial of its lm_tanh are numpy's float64 tanh, and the summation order of its hidden-row dot product is
the one of the matrix-vector product behind numpy's `@`.  FMAs are formed exactly (fractions) and rounded once.

What these two tests, and with them the device's parity with the host (tests/test_gpu_metalm.py, test_gpu_metalm_order.py),
require of the numpy under them — they were written against numpy 2.2.6 from its wheel, which brings OpenBLAS 0.3.29
(DYNAMIC_ARCH) along:
* `@` of a float64 matrix and vector goes to OpenBLAS dgemv on a core where OpenBLAS picks its Haswell, Zen or SkylakeX
  kernels (any x86-64 with AVX2 and FMA3: these targets share the dgemv_t micro-kernel whose order matvec_row restates).
  A numpy linked against another BLAS (MKL, Accelerate, the reference BLAS), or an OpenBLAS target with another dgemv
  micro-kernel (aarch64, pre-AVX2 x86), sums in another order: test_the_devices_dot_product_order_is_numpys then FAILS
  here on the CPU, and that failure, not a change in csrc/metalm.hip, is why the GPU parity tests fail beside it.
* `np.tanh` of float64 goes to numpy's own SIMD loop (a table-driven polynomial; numpy 2.x takes it where the CPU has
  AVX512_SKX or AVX2 + FMA3), not to the C library's tanh: test_the_devices_tanh_is_numpys is its canary.
The recorded fixtures (tests/golden/metalm_v3_*.npz) were made under the same numpy; the host restatement cannot sum in a
fixed order of its own, because it must stay the reference's `@` to reproduce the reference bit for bit."""
import os
import re
from fractions import Fraction

import numpy as np

HIP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "xenoverse_amd", "csrc", "metalm.hip")


def fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def tanh_table():
    text = open(HIP).read()
    body = text[text.index("lm_tanh_tab[18 * 16] = {"):]
    body = body[:body.index("};")]
    words = [int(w, 16) for w in re.findall(r"0x([0-9a-f]{16})ull", body)]
    assert len(words) == 18 * 16
    return np.array(words, np.uint64).view(np.float64).reshape(18, 16)


def lm_tanh(x, tab):
    """lm_tanh of csrc/metalm.hip, operation for operation"""
    bits = int(np.float64(x).view(np.int64))
    i = (bits & 0x7ff8000000000000) - 0x3fc0000000000000
    i = min(max(i, 0), 0x0078000000000000) >> 51
    c = tab[:, i]
    y = abs(float(x)) - float(c[0])
    r = fma(c[17], y, c[16])
    for k in range(15, 0, -1):
        r = fma(r, y, c[k])
    return -r if bits < 0 else r


def test_the_devices_tanh_is_numpys():
    tab = tanh_table()
    rs = np.random.RandomState(11)
    x = np.concatenate([rs.normal(0, 2, 1500), rs.normal(0, 0.05, 300), rs.normal(0, 15, 300),
                        [0.0, 1e-300, 0.125, -0.1875, 0.999, 1.0, 1.5, 23.9, 24.0, 31.0, 40.0, -700.0]])
    want = np.tanh(x)
    got = np.array([lm_tanh(v, tab) for v in x])
    assert got.tobytes() == want.tobytes()


def matvec_row(a, x):
    """one hidden row as csrc/metalm.hip sums it: chain k mod 4 over the first 4 * (K // 4) terms, (0 + 2) + (1 + 3), then
    the last K mod 4 terms"""
    K = len(a)
    K4 = K & ~3
    acc = [0.0, 0.0, 0.0, 0.0]
    for q in range(K4):
        acc[q & 3] = fma(a[q], x[q], acc[q & 3])
    s = (acc[0] + acc[2]) + (acc[1] + acc[3])
    m3 = K - K4
    if m3 == 1:
        return fma(a[K4], x[K4], s)
    if m3 >= 2:
        t = fma(a[K4], x[K4], float(a[K4 + 1]) * float(x[K4 + 1]))
        if m3 == 3:
            t = fma(a[K4 + 2], x[K4 + 2], t)
        s += t
    return s


def test_the_devices_dot_product_order_is_numpys():
    rs = np.random.RandomState(12)
    for H, E in ((32, 16), (64, 16), (64, 32), (24, 12), (128, 64), (20, 13), (20, 10), (24, 7)):
        w = rs.normal(size=(H, H + E))
        x = rs.normal(size=H + E)
        want = w @ x
        got = np.array([matvec_row(w[r], x) for r in range(H)])
        assert got.tobytes() == want.tobytes(), (H, E)
