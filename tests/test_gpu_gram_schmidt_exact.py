"""The three kernels only gmres! reaches -- multi_dot4_kernel, multi_axpy_dev_kernel (variant = 1 / 2) and divcopy_dev_kernel
(the look-ahead) -- and multi_axpy_kernel, each against an exact reference, through the test-only entry points of
include/krylov_hip_test.h that launch them the way csrc/solvers.cpp does (scalars in the device ring).

  multi_dot4_kernel      every output against the exactly rounded dot of the operands read back from the device
                         (tests/exact_reduction.py): the Dot2 bound with compensated = 1, the classical bound
                         gamma_n sum|x_i y_i| with compensated = 0 (which must break the Dot2 bound somewhere); an output must not
                         depend on where its basis vector stands in the table; q may be an entry of the table.
  multi_axpy*_kernel     bit for bit the correctly rounded fma chain of tests/gram_schmidt_model.py and k sequential kaxpy_ calls,
                         across the chunk edge kMultiMax = 32 and with one misaligned vector in either chunk.
  divcopy_dev_kernel     x / sqrt(sumsq): bit for bit where the root is exact, within 1 ulp of NumPy's otherwise.

Lengths: 511 and 513 have one workgroup and its odd tail element, 1025 two workgroups on the 16-byte path, 4099 many.  Every case
runs on vectors carved at element offset 0 (16-byte path) and 1 (8-byte path) and with nt_min_elems at its default and at 1.

Not checked: that nothing beyond the (k + 3) & ~3 reserved slots of the ring is written -- no entry point reads the ring back.
"""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_reduction as er  # noqa: E402
import gram_schmidt_model as gm  # noqa: E402
from exact_reduction import Tally, ulp  # noqa: E402
from test_gpu_vec_dispatch import _Options, _carved  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 255, 257, 511, 513, 1025, 4099]
DOT_K = [1, 2, 3, 4, 5, 6, 7, 8, 9, 64]
AXPY_K = [1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 64, 65]
CONDS = (1.0, 1e8, 1e16)
PLACES = ("ends", "tail")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def _nt_settings(ctx):
    default = ctx.get_option("nt_min_elems")
    assert default > max(SIZES)                         # the default launches nothing non-temporal at these sizes
    return (default, 1)


# ---- multi_dot4_kernel -------------------------------------------------------------------------------------------------------------
_DOT_DATA = {}


def _dot_data(n):
    """q and 64 basis vectors of length n: vector i has condition CONDS[i % 3] against q with its cancelling partners at
    PLACES[(i // 3) % 2] -- with "ends" and "tail" the last element (the scalar tail branch at odd n) decides the result"""
    if n not in _DOT_DATA:
        rng = np.random.default_rng(4000 + n)
        q = rng.standard_normal(n) * np.exp2(rng.integers(-8, 9, n))
        V, conds = [], []
        for i in range(max(DOT_K)):
            cond, place = (CONDS[i % 3], PLACES[(i // 3) % 2]) if n >= 255 else (1.0, "ends")
            x, _, got = er.gen_dot(n, cond, rng, place, y=q)
            assert cond == 1.0 or got >= cond / 2, (n, i, cond, got)
            V.append(x)
            conds.append(got)
        _DOT_DATA[n] = (q, V, conds)
    return _DOT_DATA[n]


def _dot_setup(ctx, n, first):
    """the table on the device, carved at element offset `first`; the exact dots of what the device holds, read back"""
    q, V, conds = _dot_data(n)
    names = ["q"] + [f"V{i}" for i in range(len(V))]
    buf, v = _carved(ctx, n, names, first)
    v["q"].copy_from_host(q)
    for i, x in enumerate(V):
        v[f"V{i}"].copy_from_host(x)
    dq, dV = v["q"], [v[f"V{i}"] for i in range(len(V))]
    qd = dq.to_host()
    Vd = [u.to_host() for u in dV]
    exact = [(er.exact_dot(x, qd), er.absum(x, qd)) for x in Vd]
    return buf, dq, dV, qd, Vd, exact, conds


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("first", [0, 1])
def test_multi_dot_meets_the_bounds(K, ctx, parity_log, n, first):
    buf, dq, dV, qd, Vd, exact, conds = _dot_setup(ctx, n, first)
    g = er.gamma(n)
    for nt in _nt_settings(ctx):
        for comp in (1, 0):
            worst = 0.0
            with _Options(ctx, nt_min_elems=nt, compensated=comp):
                for k in DOT_K:
                    out = K.test_multi_dot(n, dV[:k], dq)
                    assert len(out) == k
                    for i, d in enumerate(out):
                        s, a = exact[i]
                        bound = er.dot2_bound(n, s, a) if comp else g * a
                        ratio = abs(d - s) / bound if bound > 0 else (0.0 if d == s else math.inf)
                        worst = max(worst, ratio)
                        assert abs(d - s) <= bound, (n, first, nt, comp, k, i, conds[i], d, s, bound)
            parity_log(test="gram_schmidt_exact", family="multi_dot", n=n, offset=first, nt_min_elems=nt, compensated=comp,
                       worst_ratio_of_bound=worst)
            print(f"multi_dot n={n} offset={first} nt_min_elems={nt} compensated={comp}: worst |d - s| = {worst:.3e} of its bound")


@pytest.mark.parametrize("n", [513, 4099])
@pytest.mark.parametrize("first", [0, 1])
def test_uncompensated_multi_dot_breaks_the_dot2_bound(K, ctx, n, first):
    """compensated = 0 is plain fma accumulation on the same tree: on the ill-conditioned vectors the Dot2 bound must fail, so
    test_multi_dot_meets_the_bounds tells the two modes apart"""
    buf, dq, dV, qd, Vd, exact, conds = _dot_setup(ctx, n, first)
    with _Options(ctx, compensated=0):
        out = K.test_multi_dot(n, dV[:9], dq)
    broke = [i for i, d in enumerate(out) if abs(d - exact[i][0]) > er.dot2_bound(n, *exact[i])]
    assert broke, (n, first)
    assert all(conds[i] > 1e7 for i in broke), (broke, [conds[i] for i in broke])     # never a well-conditioned one


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("first", [0, 1])
def test_multi_dot_output_does_not_depend_on_the_table_position(K, ctx, n, first):
    """each of the four outputs of a group has its own accumulator, and wave_publish<4> / reduce_finish_kernel<4> treat all four
    alike: output i of a k = 9 call equals, bit for bit, output 0 of a k = 1 call on (V_i, q)"""
    buf, dq, dV, qd, Vd, exact, conds = _dot_setup(ctx, n, first)
    for nt in _nt_settings(ctx):
        for comp in (1, 0):
            with _Options(ctx, nt_min_elems=nt, compensated=comp):
                nine = K.test_multi_dot(n, dV[:9], dq)
                alone = [K.test_multi_dot(n, [dV[i]], dq)[0] for i in range(9)]
            differ = [i for i in range(9) if _bits([nine[i]]) != _bits([alone[i]])]
            assert not differ, (n, first, nt, comp, differ, [(nine[i], alone[i]) for i in differ])


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("first", [0, 1])
def test_multi_dot_with_q_in_the_table(K, ctx, parity_log, n, first):
    """the s-step QR calls launch_multi_dot(..., V + k, V[k + j], ...): q is entry j of the table, and out[j] its sum of squares"""
    tally = Tally(parity_log, "multi_dot")
    buf, dq, dV, qd, Vd, exact, conds = _dot_setup(ctx, n, first)
    for nt in _nt_settings(ctx):
        with _Options(ctx, nt_min_elems=nt, compensated=1):
            for k, j in ((1, 0), (4, 3), (5, 4), (6, 1), (9, 8)):
                out = K.test_multi_dot(n, dV[:k], dV[j])
                ok, info = tally.sq(f"multi_dot.alias k={k} j={j}", out[j], Vd[j])
                assert ok, (n, first, nt, info)
                for i in range(k):
                    if i != j:
                        s, a = er.exact_dot(Vd[i], Vd[j]), er.absum(Vd[i], Vd[j])
                        assert abs(out[i] - s) <= er.dot2_bound(n, s, a), (n, first, nt, k, j, i, out[i], s)


# ---- multi_axpy_dev_kernel, multi_axpy_kernel --------------------------------------------------------------------------------------
_AXPY_DATA = {}


def _axpy_data(n):
    """x, 65 vectors, 65 coefficients, and the model's x after every prefix length of AXPY_K (one chain serves them all)"""
    if n not in _AXPY_DATA:
        rng = np.random.default_rng(7000 + n)
        x = rng.standard_normal(n)
        V = [rng.standard_normal(n) * np.exp2(rng.integers(-3, 4, n)) for _ in range(max(AXPY_K))]
        coef = rng.standard_normal(max(AXPY_K)) * np.exp2(rng.integers(-3, 4, max(AXPY_K)))
        model, s = {}, x.copy()
        for j in range(max(AXPY_K)):
            s = gm.fma(-coef[j], V[j], s)
            if j + 1 in AXPY_K:
                model[j + 1] = s.copy()
        _AXPY_DATA[n] = (x, V, coef, model)
    return _AXPY_DATA[n]


def _axpy_setup(ctx, n, first):
    x, V, coef, model = _axpy_data(n)
    buf, v = _carved(ctx, n, ["x"] + [f"V{i}" for i in range(len(V))], first)
    for i, u in enumerate(V):
        v[f"V{i}"].copy_from_host(u)
    return buf, v["x"], [v[f"V{i}"] for i in range(len(V))]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("first", [0, 1])
def test_multi_axpy_equals_the_fma_chain(K, ctx, n, first):
    """x - sum_j coef_j V_j: the device-coefficient form with coef, the host-coefficient form with -coef, k kaxpy_ calls with
    -coef_j and the model are the same fma chain, so the same bits -- also past the chunk edge (k = 33, 64, 65)"""
    x, V, coef, model = _axpy_data(n)
    buf, dx, dV = _axpy_setup(ctx, n, first)
    dx.copy_from_host(x)
    seq = {}
    for j in range(max(AXPY_K)):
        K.kaxpy_(n, -coef[j], dV[j], dx)
        if j + 1 in AXPY_K:
            seq[j + 1] = dx.to_host()
    for k in AXPY_K:
        assert _bits(seq[k]) == _bits(model[k]), ("kaxpy_ chain", n, first, k)
    for nt in _nt_settings(ctx):
        with _Options(ctx, nt_min_elems=nt):
            for k in AXPY_K:
                dx.copy_from_host(x)
                K.test_multi_axpy_dev_(n, coef[:k], dV[:k], dx)
                assert _bits(dx.to_host()) == _bits(model[k]), ("multi_axpy_dev", n, first, nt, k)
                dx.copy_from_host(x)
                K.multi_axpy_(n, -coef[:k], dV[:k], dx)
                assert _bits(dx.to_host()) == _bits(model[k]), ("multi_axpy", n, first, nt, k)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("where", [2, 40])
def test_multi_axpy_with_one_misaligned_vector(K, ctx, n, where):
    """x and the table 16-byte aligned except the vector at table position `where`: its chunk of 32 takes the 8-byte path (at
    position 40 the first chunk keeps the 16-byte path) -- the same bits as the all-aligned run, which is the model's"""
    x, V, coef, model = _axpy_data(n)
    buf, dx, dV = _axpy_setup(ctx, n, 0)
    odd = ctx.zeros(n + 3).slice(1, n + 1)
    assert odd.ptr % 16 == 8 and dx.ptr % 16 == 0
    odd.copy_from_host(V[where])
    table = dV[:where] + [odd] + dV[where + 1:]
    for nt in _nt_settings(ctx):
        with _Options(ctx, nt_min_elems=nt):
            for k in (64, 65):
                dx.copy_from_host(x)
                K.test_multi_axpy_dev_(n, coef[:k], table[:k], dx)
                assert _bits(dx.to_host()) == _bits(model[k]), ("multi_axpy_dev", n, where, nt, k)
                dx.copy_from_host(x)
                K.multi_axpy_(n, -coef[:k], table[:k], dx)
                assert _bits(dx.to_host()) == _bits(model[k]), ("multi_axpy", n, where, nt, k)


@pytest.mark.parametrize("n", [3, 511, 513, 1025])
@pytest.mark.parametrize("first", [0, 1])
def test_multi_axpy_special_values(K, ctx, n, first):
    """a -0.0 coefficient leaves x as the fma chain leaves it; a NaN in one entry of a basis vector (the last element: the
    scalar tail at odd n; and an inner one) reaches that element of x and no other"""
    x, V, coef, _ = _axpy_data(n)
    k = 9
    coef = coef[:k].copy()
    coef[3] = -0.0
    V = [u.copy() for u in V[:k]]
    V[5][n - 1] = np.nan
    V[6][n // 2] = np.nan
    want = {}
    for sign in (-1.0, 1.0):                                   # the device form negates its coefficients, the host form does not
        want[sign] = gm.multi_axpy(sign * coef, V, x)
        nan = np.isnan(want[sign])
        assert sorted(np.flatnonzero(nan).tolist()) == sorted({n - 1, n // 2})
    buf, v = _carved(ctx, n, ["x"] + [f"V{i}" for i in range(k)], first)
    dV = [v[f"V{i}"].copy_from_host(V[i]) for i in range(k)]
    dx = v["x"]

    def same(got, ref):
        nan = np.isnan(ref)
        return np.array_equal(np.isnan(got), nan) and _bits(got[~nan]) == _bits(ref[~nan])

    for nt in _nt_settings(ctx):
        with _Options(ctx, nt_min_elems=nt):
            dx.copy_from_host(x)
            K.test_multi_axpy_dev_(n, coef, dV, dx)
            assert same(dx.to_host(), want[-1.0]), ("multi_axpy_dev", n, first, nt)
            dx.copy_from_host(x)
            K.multi_axpy_(n, coef, dV, dx)
            assert same(dx.to_host(), want[1.0]), ("multi_axpy", n, first, nt)


# ---- divcopy_dev_kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("first", [0, 1])
def test_divcopy_dev(K, ctx, parity_log, n, first):
    rng = np.random.default_rng(9000 + n)
    x = rng.standard_normal(n) * np.exp2(rng.integers(-20, 21, n))
    buf, v = _carved(ctx, n, ["x", "y"], first)
    v["x"].copy_from_host(x)
    for nt in _nt_settings(ctx):
        with _Options(ctx, nt_min_elems=nt):
            for sumsq in (4.0, 2.25, 9.0 * 2.0 ** -40):       # exact squares: the root is exact, the quotient correctly rounded
                root = math.sqrt(sumsq)
                assert root * root == sumsq
                K.kfill_(v["y"], -7.0)
                K.test_divcopy_dev_(n, sumsq, v["x"], v["y"])
                assert _bits(v["y"].to_host()) == _bits(x / root), (n, first, nt, sumsq)
            for sumsq in (3.0, 0.1, float(np.dot(x, x)), 1e-30, 7e40):
                K.kfill_(v["y"], -7.0)
                K.test_divcopy_dev_(n, sumsq, v["x"], v["y"])
                got, ref = v["y"].to_host(), x / np.sqrt(sumsq)
                err = float(np.max(np.abs(got - ref) / np.array([ulp(r) for r in ref])))
                parity_log(test="gram_schmidt_exact", family="divcopy_dev", n=n, offset=first, nt_min_elems=nt, sumsq=sumsq,
                           max_ulps=err, bit_equal=bool(_bits(got) == _bits(ref)))
                assert err <= 1.0, (n, first, nt, sumsq, err)
            assert np.array_equal(v["x"].to_host(), x)
