"""tests/gram_schmidt_model.py against the oracle's axpy (C fma, oracle/krylov_oracle.c): no device.  The model is what
tests/test_gpu_gram_schmidt_exact.py holds multi_axpy_kernel and multi_axpy_dev_kernel to, so it is pinned first."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gram_schmidt_model as gm  # noqa: E402


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def test_fma_model_equals_the_oracle_axpy(oracle):
    rng = np.random.default_rng(11)
    for n in (1, 2, 3, 257, 4099):
        for scale in (0, 30, 200):
            c = float(rng.standard_normal() * 2.0 ** int(rng.integers(-scale, scale + 1)))
            v = rng.standard_normal(n) * np.exp2(rng.integers(-scale, scale + 1, n))
            s = rng.standard_normal(n) * np.exp2(rng.integers(-scale, scale + 1, n))
            assert _bits(gm.fma(c, v, s)) == _bits(oracle.axpy(c, v.copy(), s.copy())), (n, scale)
    # cancellation: s = -(c v) rounded, so the fma returns the rounding error of the product, which c * v + s loses
    v = rng.standard_normal(1000)
    c = float(rng.standard_normal())
    s = -(c * v)
    got = gm.fma(c, v, s)
    assert _bits(got) == _bits(oracle.axpy(c, v.copy(), s.copy()))
    assert np.count_nonzero(got) > 900 and not np.array_equal(got, c * v + s)


def test_multi_axpy_model_is_the_chain_of_oracle_axpys(oracle):
    rng = np.random.default_rng(12)
    n, k = 513, 9
    V = [rng.standard_normal(n) for _ in range(k)]
    coef = rng.standard_normal(k)
    x = rng.standard_normal(n)
    ref = x.copy()
    for c, v in zip(coef, V):
        oracle.axpy(float(c), v.copy(), ref)
    assert _bits(gm.multi_axpy(coef, V, x)) == _bits(ref)
    assert not np.array_equal(gm.multi_axpy(coef[::-1], V[::-1], x), ref)        # the order is part of the model


def test_special_values_follow_the_fma():
    v = np.array([1.0, np.nan, 3.0, np.inf])
    s = np.array([0.5, 0.5, 0.5, 0.5])
    out = gm.fma(2.0, v, s)
    assert out[0] == 2.5 and np.isnan(out[1]) and out[2] == 6.5 and out[3] == np.inf
    out = gm.fma(-0.0, np.array([1.0, -2.0, 7.0]), np.array([0.5, -0.25, 3.0]))
    assert _bits(out) == _bits(np.array([0.5, -0.25, 3.0]))
