"""The MFMA panel kernels of block_gmres! (csrc/panel.hip) against exact references, at every width and at the edges of their
launch geometry.  The model -- geometry, rounding counts, references, input families, and the host proof that the comparisons
used here reject a wrong kernel -- is tests/panel_model.py / tests/test_panel_model_host.py.

Two kinds of comparison, no tolerance picked by hand:
  * integer panels (panel_model.int_panels): every partial sum in every order is an integer below 2^53, so the device result
    EQUALS the float64 matmul bit for bit at any size;
  * real panels (normal / scaled over 2^+-300 / cancelling at condition 1e8): |d| <= gamma(m) * sum of magnitudes per entry, m
    from panel_model.tn_roundings (V'Q, against exact_reduction.exact_dot) or 2 p + 2 (the update, against a double-double sum
    of error-free products).  max |d| / bound goes to the parity log per case with the launch counts of tn_geometry.
The fused kernels (khip_panel_mgs, the QR's SELF pass, khip_panel_multi_nn) are tied bit for bit to the primitives pinned that
way, on the same grid of sizes and widths.

Contracts written down here (and in include/krylov_hip.h):
  * khip_panel_from_colmajor zeroes the padding rows itself (a memset; its kernel writes rows < n only), so the caller may hand it
    a buffer that held anything.  Every other entry relies on zero padding and keeps it zero FOR FINITE FACTORS: the kernels
    compute the padding rows like any other (0 * psi = 0).  A factor with an Inf or NaN turns them into NaN (0 * Inf) -- but
    then the same column of EVERY real row is non-finite too, so the padding adds nothing to what V'Q or the norm would
    report.  The kernels do not mask rows >= n.
  * n = 0: khip_panel_gemm_nn / _multi_nn launch nothing; khip_panel_gemm_tn launches one workgroup without rows and returns
    Psi = 0.
Measured on an MI355X (largest max |d| / bound per family): V'Q 0.095 normal, 0.091 scaled, 0.052 cancelling, 0.003 at the two
mid sizes over every width; the update 0.44 in every family (p = 1, where the count 2 p + 2 = 4 is nearly attained); no integer
entry differed at any size.  The file takes about 70 s, most of it the exact dots at 65 536 / 65 537 rows.
Not covered here: row-partitioned panels (the rank sum of Psi), the TSQR tree, the SpMM tile kernel (own tests)."""
import ctypes
import gc
import math
import os
import sys
from contextlib import contextmanager

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_reduction as er  # noqa: E402
import panel_model as pm  # noqa: E402

pytestmark = pytest.mark.gpu

PAIRS = ((-1.0, 1.0), (2.0, 0.0), (1.0, 1.0), (0.3, -1.7), (0.0, 1.0), (0.0, 0.0))
GRID = [(n, p) for n in pm.EDGE_SIZES for p in pm.EDGE_WIDTHS]
GRID3 = GRID + [(pm.THREE_LEVEL, 16), (pm.THREE_LEVEL, 17)]
ROW_GRID = [(n, p) for n in pm.ROW_EDGES for p in pm.EDGE_WIDTHS]


def _up(K, ctx, M):
    return K.Panel.from_host(ctx, M)


def _raw(P):
    """The whole buffer, padding rows included: n_pad x p."""
    return P.buf.to_host().reshape(P.n_pad, P.p)


def _padding_zero(P):
    return not _raw(P)[P.n:].any()


@contextmanager
def _options(ctx, **kw):
    saved = {k: ctx.get_option(k) for k in kw}
    try:
        for k, v in kw.items():
            ctx.set_option(k, v)
        yield
    finally:
        for k, v in saved.items():
            ctx.set_option(k, v)


def _geo(n, p):
    g = pm.tn_geometry(n, p)
    return dict(n=n, p=p, workgroups=g["workgroups"], reduce_launches=len(g["reduce"]), reduce_tiles=g["reduce"])


def _entries(n, p):
    return pm.all_entries(p) if n <= pm.ALL_ENTRIES_UP_TO else pm.sample_entries(p)


# ------------------------------------------------------------------------------------------------ Psi = V'Q
@pytest.mark.parametrize("p", range(1, 33))
@pytest.mark.parametrize("n", pm.MID_SIZES)
def test_gemm_tn_every_width(K, ctx, parity_log, n, p):
    """Every p in 1..32: all p^2 entries, V != Q and V'Q unsymmetric (an A / B or transpose swap shows), integers for equality
    and standard normal against exact dots."""
    V, Q = pm.int_panels(n, p)
    ref = V.T @ Q
    assert p == 1 or not np.array_equal(ref, ref.T)
    assert np.array_equal(K.panel_gemm_tn(_up(K, ctx, V), _up(K, ctx, Q)), ref)
    V, Q = pm.real_panels("normal", n, p)
    ratio = pm.tn_ratio(K.panel_gemm_tn(_up(K, ctx, V), _up(K, ctx, Q)), V, Q)
    parity_log(test="panel_gemm_tn_every_width", family="normal", ratio=ratio, m=pm.tn_roundings(n, p) + 1, **_geo(n, p))
    print(f"V'Q n={n} p={p} normal: max|d|/bound {ratio:.4f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("n,p", GRID3)
def test_gemm_tn_edges_integer(K, ctx, parity_log, n, p):
    """The edge sizes (one tile ... three reduce launches), every entry, equality."""
    V, Q = pm.int_panels(n, p)
    ref = V.T @ Q
    dV, dQ = _up(K, ctx, V), _up(K, ctx, Q)
    try:
        Psi = K.panel_gemm_tn(dV, dQ)
        wrong = int((Psi != ref).sum())
        parity_log(test="panel_gemm_tn_edges_integer", family="int", entries_wrong=wrong, **_geo(n, p))
        assert wrong == 0, (n, p, np.argwhere(Psi != ref)[:8].tolist())
        assert np.array_equal(K.panel_gemm_tn(dQ, dV), ref.T)            # the operands the other way round
    finally:
        del dV, dQ
        gc.collect()


@pytest.mark.parametrize("n,p", GRID)
def test_gemm_tn_edges_real(K, ctx, parity_log, n, p):
    """Real families at the edge sizes: every entry up to 70 000 rows, the fixed sample of panel_model.sample_entries above."""
    entries = _entries(n, p)
    for fam in pm.families_for(n):
        V, Q = pm.real_panels(fam, n, p)
        ratio = pm.tn_ratio(K.panel_gemm_tn(_up(K, ctx, V), _up(K, ctx, Q)), V, Q, entries)
        parity_log(test="panel_gemm_tn_edges_real", family=fam, ratio=ratio, entries=len(entries), m=pm.tn_roundings(n, p) + 1,
                   **_geo(n, p))
        print(f"V'Q n={n} p={p} {fam}: max|d|/bound {ratio:.4f} over {len(entries)} entries")
        assert ratio <= 1.0, (n, p, fam, ratio)


# ------------------------------------------------------------------------------------------------ Q <- beta Q + alpha V Psi
@pytest.mark.parametrize("n,p", ROW_GRID)
def test_gemm_nn_edges(K, ctx, parity_log, n, p):
    """All entries, per-entry bound gamma(2 p + 2) (integers with integer scalars: equality), both launch paths with the same
    bits, the padding rows still zero; where beta = 0 the old panel is all NaN and must not be read."""
    for fam in ("int",) + pm.families_for(n):
        V, Q = pm.int_panels(n, p) if fam == "int" else pm.real_panels(fam, n, p)
        Psi = pm.int_factor(p) if fam == "int" else pm.real_factor(p)
        dV = _up(K, ctx, V)
        prod = pm.exact_product(V, Psi)
        worst = 0.0
        for alpha, beta in PAIRS:
            outs = []
            for tiles in (2, 0):
                with _options(ctx, panel_multi_tiles=tiles):
                    dQ = _up(K, ctx, np.full((n, p), np.nan) if beta == 0.0 else Q)
                    K.panel_gemm_nn_(alpha, dV, Psi, beta, dQ)
                    outs.append(dQ.to_host())
                    assert _padding_zero(dQ), (n, p, fam, alpha, beta, tiles)
            assert np.array_equal(outs[0], outs[1], equal_nan=True), (n, p, fam, alpha, beta)
            if fam == "int" and alpha == int(alpha) and beta == int(beta):
                assert np.array_equal(outs[0], beta * Q + alpha * (V @ Psi)), (n, p, alpha, beta)
            else:
                worst = max(worst, pm.nn_ratio(outs[0], alpha, V, Psi, beta, Q, prod))
            if (alpha, beta) == (0.0, 1.0):
                assert np.array_equal(outs[0], Q)
        parity_log(test="panel_gemm_nn_edges", family=fam, ratio=worst, m=pm.nn_roundings(p) + 1, n=n, p=p)
        print(f"update n={n} p={p} {fam}: max|d|/bound {worst:.4f}")
        assert worst <= 1.0, (n, p, fam, worst)


@pytest.mark.parametrize("n,p", ROW_GRID)
def test_gemm_nn_in_place_equals_out_of_place(K, ctx, n, p):
    """V may alias Q with beta = 0 (the documented in-place Q <- Q Psi): same bits as out of place, on both launch paths."""
    V, _ = pm.real_panels("normal", n, p)
    Psi = pm.real_factor(p)
    for tiles in (2, 0):
        with _options(ctx, panel_multi_tiles=tiles):
            dV, dOut = _up(K, ctx, V), K.Panel(ctx, n, p)
            K.panel_gemm_nn_(1.5, dV, Psi, 0.0, dOut)
            K.panel_gemm_nn_(1.5, dV, Psi, 0.0, dV)
            assert np.array_equal(_raw(dV), _raw(dOut)), (n, p, tiles)
    Vi, _ = pm.int_panels(n, p)
    dV = _up(K, ctx, Vi)
    K.panel_gemm_nn_(1.0, dV, pm.int_factor(p), 0.0, dV)
    assert np.array_equal(dV.to_host(), Vi @ pm.int_factor(p))


@pytest.mark.parametrize("n,p", [(1025, 17), (1040, 32), (272, 16)])
def test_gemm_nn_tiles_per_wave_same_bits(K, ctx, n, p):
    V, Q = pm.real_panels("normal", n, p)
    Psi = pm.real_factor(p)
    dV = _up(K, ctx, V)
    outs = {}
    for tiles in (0, 1, 2, 4, 8):
        with _options(ctx, panel_multi_tiles=tiles):
            dQ = _up(K, ctx, Q)
            K.panel_gemm_nn_(0.3, dV, Psi, -1.7, dQ)
            outs[tiles] = _raw(dQ)
    assert all(np.array_equal(outs[0], o) for o in outs.values())


# ------------------------------------------------------------------------------------------------ the fused family
def _mgs_case(K, ctx, n, p, ks):
    """khip_panel_mgs against the khip_panel_gemm_tn / khip_panel_gemm_nn sequence issued call by call: Q (padding included) and
    every Psi_i bit for bit, with the fused sweep on and off, the A operand through LDS or not, streaming accesses forced
    off and on.  panel_a_lds only acts at p = 16; at 15 and 17 it is run to show that nothing changes."""
    rng = np.random.default_rng(131 * p + n)
    distinct = 1 if n > 1_000_000 else 2                   # three-level panels: 0.55 GB each, four of them at most at a time
    dVs = [_up(K, ctx, rng.standard_normal((n, p)) / math.sqrt(n)) for _ in range(distinct)]
    dQ0 = _up(K, ctx, rng.standard_normal((n, p)))
    dQ = K.Panel(ctx, n, p)
    combos = [dict(panel_fuse=0), dict(panel_fuse=1, panel_a_lds=1, panel_nt=0), dict(panel_fuse=1, panel_a_lds=1, panel_nt=2)]
    if p in (15, 16, 17):
        combos += [dict(panel_fuse=1, panel_a_lds=0, panel_nt=0), dict(panel_fuse=1, panel_a_lds=0, panel_nt=2)]
    try:
        for k in ks:
            V = [dVs[i % distinct] for i in range(k)]
            K.kcopy_(dQ.n_pad * p, dQ.buf, dQ0.buf)
            prim = []
            for i in range(k):
                prim.append(K.panel_gemm_tn(V[i], dQ))
                K.panel_gemm_nn_(-1.0, V[i], prim[i], 1.0, dQ)
            Qref = _raw(dQ)
            assert np.isfinite(Qref).all() and not Qref[n:].any()
            for combo in combos:
                with _options(ctx, **combo):
                    K.kcopy_(dQ.n_pad * p, dQ.buf, dQ0.buf)
                    blocks = K.panel_mgs_(V, dQ)
                    assert all(np.array_equal(b, r) for b, r in zip(blocks, prim)), (n, p, k, combo)
                    assert np.array_equal(_raw(dQ), Qref), (n, p, k, combo)
    finally:
        del dVs, dQ0, dQ
        gc.collect()


@pytest.mark.parametrize("n,p", GRID3)
def test_mgs_equals_the_pinned_primitives(K, ctx, n, p):
    _mgs_case(K, ctx, n, p, (1, 2, 5))


@pytest.mark.parametrize("p", [16, 17])
def test_mgs_at_the_end_of_the_factor_ring(K, ctx, p):
    """The fused sweep keeps Psi_i in a ring of PSI_SLOTS slots: k = 61 is the last fused count, k = 62 the first that falls
    back to the two-kernel sequence."""
    assert 61 + 2 < pm.PSI_SLOTS <= 62 + 2
    _mgs_case(K, ctx, 272, p, (61, 62))


@pytest.mark.parametrize("n,p", [(65537, 16), (65537, 17), (100 * 1024 + 1, 16), (100 * 1024 + 1, 31), (pm.THREE_LEVEL, 16), (pm.THREE_LEVEL, 17)])
def test_qr_scaling_pass_fused_or_not_same_bits(K, ctx, n, p):
    """khip_panel_qr: the scaling of round 1 fused with the Gram matrix of round 2 (panel_nn_tn_kernel, SELF) against the
    gemm_nn + gemm_tn sequence at the sizes with two and three reduce launches: R and Q bit for bit."""
    rng = np.random.default_rng(n + p)
    A = rng.standard_normal((n, p)) @ (np.eye(p) + 0.3 * rng.standard_normal((p, p)))
    res = []
    for fuse in (1, 0):
        with _options(ctx, panel_fuse=fuse):
            dQ = _up(K, ctx, A)
            R = K.panel_qr_(dQ)
            res.append((R, _raw(dQ)))
            del dQ
            gc.collect()
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    assert np.isfinite(res[0][1]).all() and not res[0][1][n:].any()


@pytest.mark.parametrize("n", [272, 1025])
@pytest.mark.parametrize("p,k,path", [(16, 24, "lds"), (32, 6, "lds"), (16, 25, "reread"), (32, 7, "reread"), (17, 22, "reread"),
                                      (16, 33, "sequence")])
def test_multi_nn_three_paths(K, ctx, n, p, k, path):
    """khip_panel_multi_nn with the factors in LDS (k p^2 8 <= 48 KB), re-read per tile, and as k gemm_nn calls (k > 32): the
    k pinned khip_panel_gemm_nn calls bit for bit, and the integer result at integer inputs."""
    assert pm.multi_path(p, k, tiles=ctx.get_option("panel_multi_tiles")) == path
    rng = np.random.default_rng(n + p + k)
    Vh = [rng.standard_normal((n, p)) for _ in range(3)]
    Yh = [rng.standard_normal((p, p)) for _ in range(k)]
    X0 = rng.standard_normal((n, p))
    dV3 = [_up(K, ctx, v) for v in Vh]
    Vs = [dV3[i % 3] for i in range(k)]
    for beta in (1.0, 0.0, -0.5):
        ref = _up(K, ctx, X0)
        for i in range(k):
            K.panel_gemm_nn_(1.0, Vs[i], Yh[i], beta if i == 0 else 1.0, ref)
        X = _up(K, ctx, np.full((n, p), np.nan) if beta == 0.0 else X0)
        K.panel_multi_nn_(Vs, Yh, beta, X)
        assert np.array_equal(_raw(X), _raw(ref)), (n, p, k, beta)
    Vi = [pm.int_panels(n, p, seed=s)[0] for s in range(3)]
    Yi = [pm.int_factor(p, seed=i, lo=2) for i in range(k)]
    Xi = pm.int_panels(n, p)[1]
    dV3 = [_up(K, ctx, v) for v in Vi]
    X = _up(K, ctx, Xi)
    K.panel_multi_nn_([dV3[i % 3] for i in range(k)], Yi, 1.0, X)
    assert np.array_equal(X.to_host(), Xi + sum(Vi[i % 3] @ Yi[i] for i in range(k)))
    assert _padding_zero(X)


# ------------------------------------------------------------------------------------------------ padding rows
def _tridiagonal(K, ctx, n):
    rowptr, col, val = [0], [], []
    for r in range(n):
        for c, v in ((r - 1, -1.0), (r, 4.0), (r + 1, -1.5)):
            if 0 <= c < n:
                col.append(c)
                val.append(v)
        rowptr.append(len(col))
    return K.CsrMatrix.from_host(ctx, np.array(rowptr, dtype=np.int64), np.array(col, dtype=np.int64), np.array(val), (n, n))


@pytest.mark.parametrize("p", [3, 16, 17])
@pytest.mark.parametrize("n", [1, 17, 1001])
def test_padding_rows_stay_zero(K, ctx, n, p):
    """Rows n .. n_pad of the raw buffer after every entry that writes a panel (finite inputs), and khip_panel_norm, which
    reads them, against exact_norm."""
    rng = np.random.default_rng(n * 37 + p)
    A = rng.standard_normal((n, p))
    # from-colmajor into a buffer that held garbage: the ENTRY zeroes the padding (its kernel does not write rows >= n)
    P = K.Panel(ctx, n, p)
    K.kfill_(P.buf, 7.0)
    col = ctx.array(np.asfortranarray(A).ravel(order="F"))
    assert K.lib().khip_panel_from_colmajor(ctx._h, n, p, col.ptr, P.buf.ptr) == 0
    assert _padding_zero(P) and np.array_equal(P.to_host(), A)
    nrm, ref = K.panel_norm(P), er.exact_norm(A.ravel())
    assert abs(nrm - ref) <= 4 * er.U * ref
    Q = _up(K, ctx, rng.standard_normal((n, p)))
    K.panel_gemm_nn_(-1.0, P, rng.standard_normal((p, p)), 1.0, Q)
    assert _padding_zero(Q)
    X = _up(K, ctx, A)
    K.panel_multi_nn_([P, Q, P], [rng.standard_normal((p, p)) for _ in range(3)], 1.0, X)
    assert _padding_zero(X)
    for fuse in (1, 0):
        with _options(ctx, panel_fuse=fuse):
            W = _up(K, ctx, rng.standard_normal((n, p)))
            K.panel_mgs_([P, Q], W)
            assert _padding_zero(W) and _padding_zero(P) and _padding_zero(Q)
    if n >= p:
        for dependent in (False, True):
            B = rng.standard_normal((n, p))
            if dependent and p >= 3:
                B[:, 1] = B[:, 0]
                B[:, 2] = 0.0
            for qr in (K.panel_qr_, K.panel_qr_tau_):
                W = _up(K, ctx, B)
                try:
                    qr(W)
                except K.KhipError:                        # a small dependent block may be refused as rank deficient
                    assert dependent
                assert _padding_zero(W), (n, p, dependent, qr.__name__)
    dA = _tridiagonal(K, ctx, n)
    Y = K.Panel(ctx, n, p)
    K.spmm_(dA, P, Y)
    assert _padding_zero(Y)
    nrm, ref = K.panel_norm(Y), er.exact_norm(Y.to_host().ravel())
    assert abs(nrm - ref) <= 4 * er.U * ref
    if n >= 4 * p:
        # a block_gmres! solve on adopted panels: every tall block of the workspace afterwards
        ws = K.BlockGmresWorkspace(ctx, n, n, p, memory=3, adopt=True)
        Bp = _up(K, ctx, A)
        K.block_gmres_(ws, dA, Bp, restart=True, itmax=7, history=True)
        panels = list(ws._pan.items()) + [(f"V{i}", v) for i, v in enumerate(ws.V)] + [("B", Bp)]
        assert {"X", "W", "dX"} <= set(ws._pan)
        for name, pan in panels:
            assert _padding_zero(pan), (n, p, name)


def test_padding_rows_after_the_qr_fills_dependent_columns(K, ctx):
    """The size at which dependent columns survive the shifted pass and khip_panel_qr puts stand-in directions there
    (panel_fill_columns, tests/test_gpu_block.py::test_panel_qr_dependent_columns_get_stand_in_directions): rows >= n stay zero."""
    rng = np.random.default_rng(41)
    n, p = 200_001, 8
    A = rng.standard_normal((n, p))
    A[:, 3] = A[:, 1]
    A[:, 5] = 2.0 * A[:, 0] - 0.5 * A[:, 2]
    A[:, 6] = 0.0
    for qr in (K.panel_qr_, K.panel_qr_tau_):
        W = _up(K, ctx, A)
        qr(W)
        raw = _raw(W)
        assert np.isfinite(raw).all() and raw[:n, 6].any() and not raw[n:].any()


# ------------------------------------------------------------------------------------------------ non-finite inputs
def _cls(x):
    """0 finite, 1 +Inf, -1 -Inf, 2 NaN."""
    x = np.asarray(x, dtype=np.float64)
    return np.where(np.isnan(x), 2, np.where(np.isposinf(x), 1, np.where(np.isneginf(x), -1, 0)))


def _cls_of_sum(products):
    """Class of the IEEE sum of `products` along axis 0 when the finite part does not overflow: NaN if a NaN or both
    infinities occur, else the infinity that occurs, else finite."""
    c = _cls(products)
    nan = (c == 2).any(axis=0) | ((c == 1).any(axis=0) & (c == -1).any(axis=0))
    return np.where(nan, 2, np.where((c == 1).any(axis=0), 1, np.where((c == -1).any(axis=0), -1, 0)))


NONFINITE_KINDS = ("+inf", "-inf", "nan", "inf*0", "+inf and -inf")


def _poison(M, Other, rows, kind, col):
    """Put the special values of `kind` into column `col` of M at rows[0] (and rows[1] for the pair); 'inf*0': the partner
    entries Other[rows[0], 2 % p] and [.., 0] are exact zeros."""
    p = M.shape[1]
    if kind == "+inf":
        M[rows[0], col] = np.inf
    elif kind == "-inf":
        M[rows[0], col] = -np.inf
    elif kind == "nan":
        M[rows[0], col] = np.nan
    elif kind == "inf*0":
        M[rows[0], col] = np.inf
        Other[rows[0], 2 % p] = 0.0
        Other[rows[0], 0] = 0.0
    else:
        M[rows[0], col] = np.inf
        M[rows[1], col] = -np.inf


@pytest.mark.parametrize("p", [16, 17])
@pytest.mark.parametrize("kind", NONFINITE_KINDS)
def test_nonfinite_inputs_give_the_ieee_classes(K, ctx, kind, p):
    """Specials in the first row, the last real row (next to the padding) and a row of the last wave of the first reduce
    group: every entry of V'Q and of V Psi has the class of the IEEE result (float64 NumPy products of the same operands, summed
    by class), and entries whose operands are all finite stay finite."""
    n = pm.NONFINITE_SIZE
    rows3 = pm.NONFINITE_ROWS
    Psi = pm.real_factor(p)
    Psi[1 % p, 3 % p] = 0.0                                # V Psi: the special of V meets an exact zero of the factor there
    for at in range(3):
        rows = (rows3[at], rows3[(at + 1) % 3])
        V, Q = pm.real_panels("normal", n, p)
        _poison(Q, V, rows, kind, 1 % p)
        touched = sorted(set(rows))
        with np.errstate(invalid="ignore"):
            want = _cls_of_sum(V[touched][:, :, None] * Q[touched][:, None, :])
            got = K.panel_gemm_tn(_up(K, ctx, V), _up(K, ctx, Q))
        assert np.array_equal(_cls(got), want), (kind, p, rows, _cls(got).tolist(), want.tolist())
        assert (want != 0).any() and (p == 1 or (want == 0).any())
        # the update: the special sits in V, the panel's other rows stay finite, the padding zero (the factor is finite)
        V, Q = pm.real_panels("normal", n, p)
        _poison(V, Q, rows, kind, 1 % p)
        want = np.zeros((n, p), dtype=np.int64)
        with np.errstate(invalid="ignore"):
            for r in touched:                              # q + sum_k v_k psi_k: the p products and the old entry
                want[r] = _cls_of_sum(np.concatenate([V[r][:, None] * Psi, Q[r][None, :]]))
        for tiles in (2, 0):
            with _options(ctx, panel_multi_tiles=tiles):
                dQ = _up(K, ctx, Q)
                K.panel_gemm_nn_(1.0, _up(K, ctx, V), Psi, 1.0, dQ)
                assert np.array_equal(_cls(dQ.to_host()), want), (kind, p, rows, tiles)
                assert _padding_zero(dQ)
        assert (want != 0).any() and (kind != "inf*0" or want[rows[0], 3 % p] == 2)


@pytest.mark.parametrize("p", [5, 16, 17])
def test_nonfinite_factor_reaches_every_row_and_the_padding(K, ctx, p):
    """An Inf in Psi: column c of every real row gets v * Inf (the IEEE class of the float64 product), and the padding rows
    0 * Inf = NaN -- the written contract is 'padding stays zero for FINITE factors' (module docstring): with such a factor
    the column is non-finite in every real row already."""
    n = 1001
    V, Q = pm.real_panels("normal", n, p)
    V[7, 2 % p] = 0.0
    Psi = pm.real_factor(p)
    Psi[2 % p, 0] = np.inf
    with np.errstate(invalid="ignore"):
        want = np.stack([_cls_of_sum(V[r][:, None] * Psi) for r in range(n)])
    for tiles in (2, 0):
        with _options(ctx, panel_multi_tiles=tiles):
            dQ = _up(K, ctx, Q)
            K.panel_gemm_nn_(1.0, _up(K, ctx, V), Psi, 1.0, dQ)
            raw = _raw(dQ)
            assert np.array_equal(_cls(raw[:n]), want)
            assert want[7, 0] == 2 and (want[:, 0] != 0).all() and (want[:, 1:] == 0).all()
            assert np.isnan(raw[n:, 0]).all() and not raw[n:, 1:].any()


# ------------------------------------------------------------------------------------------------ argument checks
def test_argument_checks_and_empty_panels(K, ctx):
    L = K.lib()
    buf, buf2 = ctx.zeros(32 * 33), ctx.zeros(32 * 33)
    host = np.zeros(4096)
    hp = host.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ptrs = (ctypes.c_void_p * 2)(buf.ptr, buf.ptr)
    out = ctypes.c_double()

    def refused(rc, text):
        assert rc == -1 and text in L.khip_last_error().decode(), (rc, L.khip_last_error())

    for p in (0, 33):
        refused(L.khip_panel_gemm_tn(ctx._h, 16, p, buf.ptr, buf2.ptr, hp), "panel_gemm_tn: bad argument (1 <= p <= 32)")
        refused(L.khip_panel_gemm_nn(ctx._h, 16, p, 1.0, buf.ptr, hp, 1.0, buf2.ptr), "panel_gemm_nn: bad argument (1 <= p <= 32)")
        refused(L.khip_panel_mgs(ctx._h, 16, p, 1, ptrs, buf2.ptr, hp, 0), "panel_mgs: bad argument (1 <= p <= 32)")
        refused(L.khip_panel_multi_nn(ctx._h, 16, p, 1, ptrs, hp, 1.0, buf2.ptr), "panel_multi_nn: bad argument (1 <= p <= 32)")
        refused(L.khip_panel_from_colmajor(ctx._h, 16, p, buf.ptr, buf2.ptr), "panel_from_colmajor: bad argument (1 <= p <= 32)")
        refused(L.khip_panel_to_colmajor(ctx._h, 16, p, buf.ptr, buf2.ptr), "panel_to_colmajor: bad argument (1 <= p <= 32)")
        refused(L.khip_panel_qr(ctx._h, 16, p, buf2.ptr, hp), "panel_qr: bad argument (1 <= p <= 32)")
        refused(L.khip_panel_qr_tau(ctx._h, 16, p, buf2.ptr, hp, hp), "panel_qr: bad argument (1 <= p <= 32)")
    refused(L.khip_panel_norm(ctx._h, 16, 0, buf.ptr, ctypes.byref(out)), "panel_norm: bad argument")
    refused(L.khip_panel_mgs(ctx._h, 16, 4, -1, ptrs, buf2.ptr, hp, 0), "panel_mgs: bad argument (1 <= p <= 32)")
    refused(L.khip_panel_multi_nn(ctx._h, 16, 4, -1, ptrs, hp, 1.0, buf2.ptr), "panel_multi_nn: bad argument (1 <= p <= 32)")
    # n = 0: Psi is defined (zero: one workgroup without rows is launched), the update and the sum launch nothing
    K.kfill_(buf2, 3.0)
    for p in (1, 16, 17, 32):
        host[:] = np.nan
        assert L.khip_panel_gemm_tn(ctx._h, 0, p, buf.ptr, buf2.ptr, hp) == 0
        assert not host[:p * p].any() and np.isnan(host[p * p:]).all()
        host[:] = 1.0
        assert L.khip_panel_gemm_nn(ctx._h, 0, p, 1.0, buf.ptr, hp, 1.0, buf2.ptr) == 0
        assert L.khip_panel_multi_nn(ctx._h, 0, p, 2, ptrs, hp, 1.0, buf2.ptr) == 0
        assert L.khip_panel_multi_nn(ctx._h, 16, p, 0, ptrs, hp, 0.0, buf2.ptr) == 0      # k = 0: nothing to add, X untouched
        ctx.sync()
        assert np.array_equal(buf2.to_host(), np.full(32 * 33, 3.0))
        assert K.panel_rows(0) == 0
