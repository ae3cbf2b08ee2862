"""Host model of the elementwise part of the block Gram-Schmidt kernels (csrc/blas1.hip: multi_axpy_kernel,
multi_axpy_dev_kernel): x_i <- fma(c_j, V_j[i], x_i) in the order j = 0 .. k - 1, every fma correctly rounded.

Python 3.10 has no math.fma, so one fma is built from the error-free product of tests/exact_reduction.py
(p + e == c * v exactly) and math.fsum([p, e, s]), which rounds the exact sum of its three terms once: that IS fma(c, v, s).
tests/test_gram_schmidt_model_host.py holds it equal to oracle.axpy (the C fma of the oracle) on random data.

Elements with a non-finite operand are outside two_product's window; for them fma(c, v, s) is c * v + s in IEEE arithmetic
(a NaN or an infinity propagates the same way through both), which keeps the rest of the vector on the exact path.
"""
import math

import numpy as np

from exact_reduction import two_product


def fma(c, v, s):
    """fma(c, v_i, s_i) elementwise, correctly rounded (c a scalar; v, s float64 arrays of one length)"""
    v = np.ascontiguousarray(v, dtype=np.float64)
    s = np.ascontiguousarray(s, dtype=np.float64)
    c = float(c)
    out = np.empty_like(s)
    fin = np.isfinite(v) & np.isfinite(s) & bool(np.isfinite(c))
    if not fin.all():
        with np.errstate(invalid="ignore", over="ignore"):
            out[~fin] = c * v[~fin] + s[~fin]
    if fin.any():
        p, e = two_product(np.full(int(fin.sum()), c), v[fin])
        out[fin] = [math.fsum(t) for t in zip(p.tolist(), e.tolist(), s[fin].tolist())]
    return out


def multi_axpy(coef, V, x):
    """x + sum_j coef[j] V[j] as the kernels compute it: one fma per (j, element), j = 0 .. k - 1 in order"""
    s = np.array(x, dtype=np.float64)
    for c, v in zip(coef, V):
        s = fma(c, v, s)
    return s
