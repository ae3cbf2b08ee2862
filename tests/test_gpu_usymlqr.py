"""usymlqr! on the GPU: its fused third pass alone against the NumPy expressions (bit for bit), and the three loops against the
NumPy restatement of src/usymlqr.jl (tests/usymlqr_reference.py) and against each other, at (ls, ln) = (true, true), (true, false)
and (false, true).

Budgets (tests/test_usymlqr_host.py holds the functions and shows that they reject the injected faults):
  * path 0 (one launch per primitive) against the restatement: same niter, status and flags; both histories within budget() =
    max(1e-8, 10 x the case's own np.dot-versus-exact deviation) of each entry, plus the absolute floor 1e-12 x the first entry;
    y within the same budget of max|y| and x of max(max|x|, max|b₀|).  Only cases the project's rule admits are in the list.
  * path 1 (host-driven, fused kernels) against path 0: elementwise values are the same expressions, the dots differ by <= 1 ulp:
    the same budget.
  * path 2 (device-resident) against path 1 (same kernels, same scalar code): np.array_equal everywhere: x, y, both histories, the
    flags, the status and every role of khip_usymlqr_vector.
"q" and "p" are left out of the role comparisons against path 0 and the restatement, as for trimr!: near the end of a solve they
are βₖ₊₁ vₖ₊₁ and γₖ₊₁ uₖ₊₁ with tiny norms, quotients of rounding errors relative to their own size.
None of these tests reads the reference tree."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import usymlqr_reference as ur  # noqa: E402
from test_bilq_host import other_c  # noqa: E402
from test_gpu_trimr import _fma, _same  # noqa: E402  (the exactly rounded fma and the bitwise comparison)
from test_usymlqr_host import (BOTH, CASES, EXPECTED, FLAGS, NAN_SYSTEMS, PARITY_CASE, PARITY_ITMAX, RECT_CASES, RECT_EXPECTED,  # noqa: E402
                               SMALL_EXPECTED, SMALL_SIZES, SOLVED, STAGGERED, TIRED, budget, case_keywords, case_system, dense_pair,
                               deviation, mismatches, nonsymmetric_definite, pair_budget, rect_system, reference_pair, role_deviation,
                               roles_budget, summary)

ROLES = ur.VECTORS
NVEC = len(ROLES)
COMPARED = tuple(r for r in ROLES if r not in ("q", "p"))
W_ROLES = ("w_m2", "w_m1", "v_prev", "u_prev")                        # what a wrong parity of the rotations would swap


def _device(K, ctx, S):
    S = sp.csr_matrix(S)
    S.sort_indices()
    return K.CsrMatrix.from_host(ctx, S.indptr, S.indices, S.data, S.shape)


def _dense(K, ctx, M):
    return _device(K, ctx, sp.csr_matrix(np.asarray(M, dtype=np.float64)))


def _solve(K, ctx, A, b, c, fused=2, x0=None, y0=None, adopt=None, vectors=None, **kw):
    ws = K.UsymlqrWorkspace(ctx, len(b), len(c), adopt=adopt, vectors=vectors)
    if x0 is not None:
        ws.warm_start_(ctx.array(x0), ctx.array(y0))
    K.usymlqr_(ws, A, ctx.array(b), ctx.array(c), fused=fused, history=True, **kw)
    return ws


def _xy(ws):
    return ws.x.to_host(), ws.y.to_host()


def _roles(ws):
    return {name: ws.vector(name).to_host() for name in ROLES}


def _flags(s):
    return (s.niter, s.status, s.solved, s.inconsistent)


def _same_bits(w1, w2):
    s1, s2 = w1.stats, w2.stats
    assert _flags(s1) == _flags(s2)
    assert np.array_equal(s1.residuals, s2.residuals, equal_nan=True)
    assert np.array_equal(s1.Aresiduals, s2.Aresiduals, equal_nan=True)
    if s2.niter > 0:                                            # (before the first iteration q and p are not defined)
        r1, r2 = _roles(w1), _roles(w2)
        for name in ROLES:
            assert np.array_equal(r1[name], r2[name], equal_nan=True), name
    for a, b in zip(_xy(w1), _xy(w2)):
        assert np.array_equal(a, b, equal_nan=True)


def _against(ws, ref, bud):
    """mismatches of a workspace's solve against a restatement triple or another workspace (x is measured against the
    restatement's floor max|b₀|; between two workspaces the floor is max|b| of the solve, passed through `ref`)."""
    if isinstance(ref, tuple) and len(ref) == 3:
        xr, yr, sr = ref
    else:
        w, floor = ref
        (xr, yr), sr = _xy(w), w.stats
        sr.x_floor = floor
    x, y = _xy(ws)
    return mismatches(ws.stats, sr, bud, x, xr, y, yr)


def _roles_close(got, want, bud, floor, names=COMPARED):
    for name in names:
        d = role_deviation(got, want, name, floor)
        assert d <= bud, (name, d)


_OPS = {}


@pytest.fixture(scope="module")
def ops(K, ctx, oracle):
    """(scipy operator, device operator, b, c) of a case of the list, built once per module (cases on one system share it)."""
    def get(name):
        base = CASES[name][0]
        if base not in _OPS:
            S, b, c = case_system(oracle, name)
            _OPS[base] = (S, _device(K, ctx, S), b, c)
        return _OPS[base]
    yield get
    _OPS.clear()


# ---- 0. the fused third pass alone, through the test export: every stream bit for bit ----------------------------------------------
KERNEL_SIZES = (1, 2, 3, 255, 256, 257, 1027)                         # 1027: three blocks of 512 elements and an odd tail
STREAMS = ("x", "r", "dbar", "y", "z", "w_m2", "w_m1", "v", "u", "q", "p", "v_next", "u_next")
# -ϵₖ₋₂, -λₖ₋₁, δₖ, ϕₖ, the r coefficient, |sₖ|², ζₖ₋₁cₖ₋₁, ζₖ₋₁sₖ₋₁, -ζₖ₋₁, -cₖ₋₁, sₖ₋₁ (βₖ₊₁, γₖ₊₁ and 1 / δₖ follow)
COEF = (-0.37, 1.25, -2.3, 0.81, -0.45, 0.36, 1.31, -0.92, 0.63, 0.8, -0.6)
FLAG_PAIRS = ((1, 1), (1, 0), (0, 1), (0, 0))


def _kernel_vectors(ctx, n, seed, odd):
    """Host and device copies of the thirteen streams of P3: random, NaN-free values everywhere, so that a stream the kernel must
    not touch comes back as the sentinel it went in as.  odd: every vector starts at an odd 8-byte offset (an adopted workspace
    carved from one buffer), which takes the VEC = 1 path."""
    rng = np.random.default_rng(seed)
    host = {k: rng.standard_normal(n) for k in STREAMS}
    dev = {}
    for k in STREAMS:
        if odd:
            dev[k] = ctx.zeros(n + 1).slice(1, n + 1).copy_from_host(host[k])      # (the slice keeps its buffer alive)
            assert dev[k].ptr % 16 == 8
        else:
            dev[k] = ctx.array(host[k])
    return host, dev


def _coef14(coef, bn, gn):
    return (C.c_double * 14)(*coef, bn, gn, float(np.float64(1.0) / np.float64(coef[2])))


def _expected_p3(stage, ls, ln, h, coef, bn, gn):
    """The NumPy expressions of P3 on host copies (the roundings of the path-0 primitives: fma for kaxpy!, fma(a, x, b y) for
    kaxpby!, a x for kscal!, x (1 / a) for kdiv!, / for kdivcopy!); returns the dict of every stream afterwards."""
    ne, nl, dl, phi, rc, s2, zc, zs, nz, nc, sn = [np.float64(t) for t in coef]
    idl = np.float64(1.0) / dl
    e = {k: a.copy() for k, a in h.items()}
    n = len(h["x"])
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if stage == 1:
            w = h["u"] / dl
            e["w_m1"] = w
        else:
            t = ne * h["w_m2"] if stage >= 3 else h["w_m2"]
            t = _fma(nl, h["w_m1"], t)
            t = _fma(np.float64(1.0), h["u"], t)
            w = t * idl
            e["w_m2"] = w
        if ls:
            e["y"] = _fma(phi, w, h["y"])
            e["r"] = _fma(rc, h["q"], s2 * h["r"])
        if ln:
            if stage == 1:
                e["dbar"] = h["v"].copy()
            else:
                e["x"] = _fma(zs, h["v"], _fma(zc, h["dbar"], h["x"]))
                e["dbar"] = _fma(nc, h["v"], sn * h["dbar"])
                e["z"] = _fma(nz, h["w_m1"], h["z"])                    # the OLD wₖ₋₁
        e["v_next"] = h["q"] / np.float64(bn) if bn != 0 else np.zeros(n)
        e["u_next"] = h["p"] / np.float64(gn) if gn != 0 else np.zeros(n)
    return e


def _run_p3(K, ctx, n, stage, ls, ln, coef, bn, gn, dev):
    rc = K.lib().khip_test_usymlqr_p3(ctx._h, n, stage, ls, ln, _coef14(coef, bn, gn), *[dev[k].ptr for k in STREAMS])
    assert rc == 0, K.lib().khip_last_error().decode()


@pytest.mark.parametrize("odd", (False, True))
@pytest.mark.parametrize("stage", (1, 2, 3))
@pytest.mark.parametrize("n", KERNEL_SIZES)
def test_p3_kernel_is_the_numpy_expression(K, ctx, n, stage, odd):
    """usymlqr_p3_kernel at each stage and each of the four pairs of activity flags, on random vectors with chosen coefficients:
    every output stream bit-identical to the NumPy expression, every other stream -- the inputs, and ALL streams of a side that is
    not active -- equal to what went in.  odd: the VEC = 1 path."""
    for i, (ls, ln) in enumerate(FLAG_PAIRS):
        host, dev = _kernel_vectors(ctx, n, 1000 * n + 10 * stage + i, odd)
        _run_p3(K, ctx, n, stage, ls, ln, COEF, 2.5, 0.7, dev)
        want = _expected_p3(stage, ls, ln, host, COEF, 2.5, 0.7)
        for k in STREAMS:
            assert _same(dev[k].to_host(), want[k]), (k, stage, n, odd, ls, ln)
        if not ls:
            assert all(np.array_equal(dev[k].to_host(), host[k]) for k in ("y", "r"))
        if not ln:
            assert all(np.array_equal(dev[k].to_host(), host[k]) for k in ("x", "z", "dbar"))


@pytest.mark.parametrize("stage", (1, 2, 3))
def test_p3_kernel_zero_norms_give_zero_vectors(K, ctx, stage):
    """βₖ₊₁ = 0: vₖ₊₁ = 0 (a fill in the reference), γₖ₊₁ = 0: uₖ₊₁ = 0; the two guards are independent."""
    for n in (3, 257):
        for bn, gn in ((0.0, 0.7), (2.5, 0.0), (0.0, 0.0)):
            host, dev = _kernel_vectors(ctx, n, 17 * n + stage, False)
            _run_p3(K, ctx, n, stage, 0, 1, COEF, bn, gn, dev)
            want = _expected_p3(stage, 0, 1, host, COEF, bn, gn)
            for k in STREAMS:
                assert _same(dev[k].to_host(), want[k]), (k, stage, n, bn, gn)


@pytest.mark.parametrize("stage", (2, 3))
def test_p3_kernel_frozen_side_keeps_its_bits_beside_nan_and_inf(K, ctx, stage):
    """A side that is not active touches none of its streams: with the other side's coefficients NaN or Inf (the 0 / 0 r
    coefficient; an overflowed ζ), the frozen y, r or x, z, d̅ come back bit for bit."""
    n = 257
    nan_ls = list(COEF)
    nan_ls[3], nan_ls[4] = np.inf, np.nan                       # ϕₖ, the r coefficient
    host, dev = _kernel_vectors(ctx, n, 5 + stage, False)
    _run_p3(K, ctx, n, stage, 1, 0, nan_ls, 2.5, 0.7, dev)
    assert all(_same(dev[k].to_host(), host[k]) for k in ("x", "z", "dbar"))
    assert np.isnan(dev["r"].to_host()).all() and np.isinf(dev["y"].to_host()).all()
    nan_ln = list(COEF)
    nan_ln[6], nan_ln[7], nan_ln[8] = np.inf, np.nan, np.inf    # ζₖ₋₁cₖ₋₁, ζₖ₋₁sₖ₋₁, -ζₖ₋₁
    host, dev = _kernel_vectors(ctx, n, 50 + stage, False)
    _run_p3(K, ctx, n, stage, 0, 1, nan_ln, 2.5, 0.7, dev)
    assert all(_same(dev[k].to_host(), host[k]) for k in ("y", "r"))
    assert np.isnan(dev["x"].to_host()).all() and np.isinf(dev["z"].to_host()).all()


def test_p3_kernel_non_temporal_instantiation(K, ctx):
    """The same comparison with the non-temporal instantiation forced (nt_min_elems = 1), at the sizes with a tail and without."""
    keep = ctx.get_option("nt_min_elems")
    ctx.set_option("nt_min_elems", 1)
    try:
        for n in (256, 257, 1027):
            for stage in (1, 2, 3):
                host, dev = _kernel_vectors(ctx, n, 7 * n + stage, False)
                _run_p3(K, ctx, n, stage, 1, 1, COEF, 2.5, 0.7, dev)
                want = _expected_p3(stage, 1, 1, host, COEF, 2.5, 0.7)
                for k in STREAMS:
                    assert _same(dev[k].to_host(), want[k]), (k, stage, n)
    finally:
        ctx.set_option("nt_min_elems", keep)


# ---- 1. path 0 against the restatement, path 1 against path 0, path 2 against path 1: every case, all three settings ---------------
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("name", list(CASES))
def test_three_paths_on_every_case(K, ctx, oracle, ops, name, flags):
    S, A, b, c = ops(name)
    ref = reference_pair(oracle, name, flags)[0]
    bud = budget(oracle, name, flags)
    kw = case_keywords(name, flags)
    w0 = _solve(K, ctx, A, b, c, fused=0, **kw)
    w1 = _solve(K, ctx, A, b, c, fused=1, **kw)
    w2 = _solve(K, ctx, A, b, c, fused=2, **kw)
    assert (w0.last_path, w1.last_path, w2.last_path) == (0, 1, 2)
    s0, s1 = w0.stats, w1.stats
    print(f"{name} (ls, ln) = {flags}: budget {bud:.2e}; path 0 against the restatement "
          f"{deviation(s0.residuals, ref[2].residuals, 1e-12):.2e}; path 1 against path 0 {deviation(s1.residuals, s0.residuals, 1e-12):.2e}")
    assert summary(s0) == EXPECTED[name][FLAGS.index(flags)]
    assert not s0.inconsistent
    assert _against(w0, ref, bud) == []
    assert _against(w1, (w0, ref[2].x_floor), bud) == []
    _same_bits(w1, w2)
    _roles_close(_roles(w2), _roles(w0), bud, ref[2].x_floor, W_ROLES)
    assert len(s0.Aresiduals) == len(ref[2].Aresiduals) and len(s0.residuals) == len(ref[2].residuals)
    if name in STAGGERED and flags == BOTH:                     # each history ends with the iteration that solved its side
        k_ls, k_ln = STAGGERED[name]
        for s in (s0, s1, w2.stats):
            assert len(s.Aresiduals) == k_ls and len(s.residuals) == k_ls + k_ln


# ---- 2. the first iterations: every named vector holds the restatement's variable --------------------------------------------------
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("itmax", PARITY_ITMAX)
def test_roles_hold_the_reference_variables(K, ctx, oracle, ops, itmax, flags):
    """After k iterations every name of khip_usymlqr_vector but "q" and "p" holds what the reference's variable of that name holds
    at the end of the loop, on paths 0, 1 and 2 (1 and 2 bit-identical to each other): k = 1, 2, 3, 4, 7, 8 walks the three stages
    of P3 and both parities of the rotation of (wₖ₋₂, wₖ₋₁).  n = 343 is odd: the tail lane does every branch."""
    S, A, b, c = ops(PARITY_CASE)
    pair = reference_pair(oracle, PARITY_CASE, flags, itmax=itmax)
    bud = roles_budget(pair, COMPARED)
    assert bud <= 1e-6
    sr = pair[0][2]
    kw = dict(ls=flags[0], ln=flags[1], itmax=itmax)
    w0, w1, w2 = (_solve(K, ctx, A, b, c, fused=f, **kw) for f in (0, 1, 2))
    assert (w0.last_path, w1.last_path, w2.last_path) == (0, 1, 2) and summary(w2.stats) == (itmax, TIRED)
    _same_bits(w1, w2)
    for w in (w0, w2):
        _roles_close(_roles(w), sr.vectors, bud, sr.x_floor)
        assert _against(w, pair[0], bud) == []
    r0, r2 = _roles(w0), _roles(w2)
    for name in ("q", "p"):                                     # early in a solve q and p are ordinary vectors on every path
        assert role_deviation(r0, sr.vectors, name) <= bud and role_deviation(r2, sr.vectors, name) <= bud


# ---- 3. small, rectangular and degenerate systems -------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("n", SMALL_SIZES)
def test_small_dense_systems(K, ctx, n, flags):
    """n = 1, 2, 3 end in stages 1, 2 and 3 of P3; 63, 64, 65 sit around the wave size.  n = 1 with `ls` is the 0 / 0 case: r and x
    are NaN on every path, as in the restatement."""
    M, b = nonsymmetric_definite(n)
    c = other_c(n)
    pair = dense_pair(M, b, c, ls=flags[0], ln=flags[1])
    bud = pair_budget(pair)
    A = _dense(K, ctx, M)
    w0, w1, w2 = (_solve(K, ctx, A, b, c, fused=f, ls=flags[0], ln=flags[1]) for f in (0, 1, 2))
    assert (w0.last_path, w1.last_path, w2.last_path) == (0, 1, 2)
    assert _against(w0, pair[0], bud) == []
    assert _against(w1, (w0, pair[0][2].x_floor), bud) == []
    _same_bits(w1, w2)
    assert w2.stats.solved and w2.stats.niter == SMALL_EXPECTED[n][FLAGS.index(flags)]
    if n == 1 and flags[0]:
        assert all(np.isnan(w.x.to_host()).all() and np.isnan(w.vector("r").to_host()).all() for w in (w0, w1, w2))


@pytest.mark.parametrize("name", list(NAN_SYSTEMS))
def test_beta_zero_makes_r_and_x_nan_on_every_path(K, ctx, name):
    """βₖ₊₁ = 0 exactly in an active least-squares step: the r coefficient is 0 / 0; r, then x, are NaN and the solve ends `solved`,
    on all three loops as in the restatement (equal_nan); y and both histories are finite and equal.  Kept, not fixed."""
    M, b, c = NAN_SYSTEMS[name]
    xr, yr, sr = ur.usymlqr(M, b, c)
    A = _dense(K, ctx, M)
    ws = [_solve(K, ctx, A, b, c, fused=f) for f in (0, 1, 2)]
    assert [w.last_path for w in ws] == [0, 1, 2]
    for w in ws:
        x, y = _xy(w)
        st = w.stats
        assert (st.niter, st.status, st.solved, st.inconsistent) == (sr.niter, SOLVED, True, False)
        assert np.array_equal(np.isnan(x), np.isnan(xr)) and np.isnan(x).all()
        assert np.array_equal(np.isnan(w.vector("r").to_host()), np.isnan(sr.vectors["r"]))
        assert np.abs(y - yr).max() <= 1e-14 * np.abs(yr).max()
        assert np.allclose(st.residuals, sr.residuals, rtol=1e-14, atol=1e-300) and np.allclose(st.Aresiduals, sr.Aresiduals, rtol=1e-14)
    _same_bits(ws[1], ws[2])


@pytest.mark.parametrize("shape", list(RECT_CASES))
def test_rectangular_runs_the_primitive_sequence(K, ctx, shape):
    """m ≠ n: loop 0 whatever `fused` says, x of m entries and y of n, within budget of the restatement."""
    M, b, c = rect_system(*shape)
    kw, settings = RECT_CASES[shape]
    A = _dense(K, ctx, M)
    for flags in settings:
        pair = dense_pair(M, b, c, ls=flags[0], ln=flags[1], **kw)
        for fused in (2, 0):
            ws = _solve(K, ctx, A, b, c, fused=fused, ls=flags[0], ln=flags[1], **kw)
            assert ws.last_path == 0 and summary(ws.stats) == RECT_EXPECTED[(shape, flags)]
            assert len(ws.x) == shape[0] and len(ws.y) == shape[1]
            assert _against(ws, pair[0], pair_budget(pair)) == []
    assert K.UsymlqrWorkspace(ctx, shape[0], shape[1], adopt=False).nbytes == 8 * (6 * shape[0] + 7 * shape[1])


def test_inconsistent_exit_leaves_the_status_unknown(K, ctx):
    """b ⟂ range(A): the least-squares side ends by ‖Aᴴrₖ₋₁‖ <= κ in one iteration; the status stays "unknown", solved and
    stats.inconsistent are false, as in the reference."""
    M = np.array([[1.0, 0.0], [0.0, 1.0], [0.0, 0.0]])
    b, c = np.array([0.0, 0.0, 1.0]), np.array([1.0, 2.0])
    xr, yr, sr = ur.usymlqr(M, b, c)
    ws = _solve(K, ctx, _dense(K, ctx, M), b, c)
    st = ws.stats
    assert sr.inconsistent_exit and (st.niter, st.status, st.solved, st.inconsistent) == (1, "unknown", False, False)
    x, y = _xy(ws)
    assert np.abs(x - xr).max() <= 1e-14 and np.abs(y - yr).max() <= 1e-14


# ---- 4. adopted vectors, warm start, callback, paths, history windows -----------------------------------------------------------
def _carved(K, ctx, n, first):
    """The thirteen vectors of a workspace inside one buffer, starting at element `first` with an even stride: first = 1 puts every
    vector at an odd element offset (8-byte but not 16-byte aligned), first = 0 keeps them 16-byte aligned."""
    stride = n + 2 - (n & 1) + 2
    buf = ctx.zeros(first + NVEC * stride)
    assert buf.ptr % 16 == 0
    vec = {k: buf.slice(first + i * stride, first + i * stride + n) for i, k in enumerate(K.UsymlqrWorkspace.VECTORS)}
    assert all(v.ptr % 16 == 8 * first for v in vec.values())
    return buf, vec


@pytest.mark.parametrize("name", ["kron8_sinc_it60", "kron7_it60"])
def test_adopted_vectors_at_odd_offsets(K, ctx, oracle, ops, name):
    """The 8-byte kernel path (and, with n = 343, the 16-byte path's tail element beside it): bit-identical to an owned workspace
    and to a 16-byte-aligned adoption under path 2, within budget of path 0; nothing is written between the carved vectors."""
    S, A, b, c = ops(name)
    n = len(b)
    kw = case_keywords(name, BOTH)
    wo = _solve(K, ctx, A, b, c, adopt=False, **kw)
    buf1, odd = _carved(K, ctx, n, 1)
    w1 = _solve(K, ctx, A, b, c, vectors=odd, **kw)
    buf0, even = _carved(K, ctx, n, 0)
    w0 = _solve(K, ctx, A, b, c, vectors=even, **kw)
    assert (wo.last_path, w1.last_path, w0.last_path) == (2, 2, 2)
    _same_bits(wo, w1)
    _same_bits(wo, w0)
    wp = _solve(K, ctx, A, b, c, fused=0, **kw)
    assert wp.last_path == 0 and _against(w1, (wp, float(np.abs(b).max())), budget(oracle, name, BOTH)) == []
    stride = n + 2 - (n & 1) + 2
    for first, buf in ((1, buf1), (0, buf0)):
        h = buf.to_host()
        gaps = np.ones(len(h), dtype=bool)
        for i in range(NVEC):
            gaps[first + i * stride:first + i * stride + n] = False
        assert not h[gaps].any(), "a kernel wrote outside its vectors"


def test_adopted_workspace_and_the_generic_entries(K, ctx, ops):
    name = "kron8_sinc_it60"
    S, A, b, c = ops(name)
    n = len(b)
    vec = {k: ctx.empty(n) for k in K.UsymlqrWorkspace.VECTORS}
    ws = K.UsymlqrWorkspace(ctx, n, n, vectors=vec)
    K.usymlqr_(ws, A, ctx.array(b), ctx.array(c), history=True, itmax=60)
    assert ws.x is vec["x"] and ws.y is vec["y"] and ws.last_path == 2      # solution(ws) is the caller's x and y
    wo = _solve(K, ctx, A, b, c, adopt=False, itmax=60)
    _same_bits(wo, ws)
    assert K.UsymlqrWorkspace(ctx, n, n, adopt=False).nbytes == 8 * 13 * n
    x, y, st, ws2 = K.usymlqr(A, ctx.array(b), ctx.array(c), history=True, itmax=60)
    assert ws2.last_path == 2                                  # the out-of-place entry forwards the default callback
    assert np.array_equal(x.to_host(), wo.x.to_host()) and np.array_equal(y.to_host(), wo.y.to_host())
    assert np.array_equal(st.residuals, wo.stats.residuals) and np.array_equal(st.Aresiduals, wo.stats.Aresiduals)
    ws3 = K.krylov_workspace("usymlqr", A, ctx.array(b), ctx.array(c))
    assert isinstance(ws3, K.UsymlqrWorkspace)
    K.krylov_solve_(ws3, A, ctx.array(b), c=ctx.array(c), history=True, itmax=60)
    assert ws3.last_path == 2 and np.array_equal(ws3.y.to_host(), wo.y.to_host())
    x4, y4, st4, ws4 = K.krylov_solve("usymlqr", A, ctx.array(b), c=ctx.array(c), history=True, itmax=60)
    assert ws4.last_path == 2 and np.array_equal(x4.to_host(), wo.x.to_host()) and np.array_equal(y4.to_host(), wo.y.to_host())


@pytest.mark.parametrize("adopt", [False, True])
@pytest.mark.parametrize("fused", [0, 1, 2])
def test_warm_start_with_x0_and_y0(K, ctx, oracle, ops, fused, adopt):
    """From a truncated solve to the same solution, within budget of the restatement's warm start; the warm start is used up."""
    name = "kron8_shift24_sinc"
    S, A, b, c = ops(name)
    full = _solve(K, ctx, A, b, c, fused=fused)
    xf, yf = _xy(full)
    part = _solve(K, ctx, A, b, c, fused=fused, itmax=5)
    x0, y0 = _xy(part)
    ws = _solve(K, ctx, A, b, c, fused=fused, x0=x0, y0=y0, adopt=adopt)
    assert ws.last_path == fused
    pair = reference_pair(oracle, name, BOTH, x0=x0, y0=y0)
    assert _against(ws, pair[0], pair_budget(pair)) == []
    x, y = _xy(ws)
    assert ws.stats.solved
    assert np.abs(x - xf).max() <= 1e-6 * np.abs(xf).max() and np.abs(y - yf).max() <= 1e-6 * np.abs(yf).max()
    again = _solve(K, ctx, A, b, c, fused=fused)                 # the warm start is used up: a second solve equals a fresh workspace's
    K.usymlqr_(ws, A, ctx.array(b), ctx.array(c), fused=fused, history=True)
    _same_bits(again, ws)


@pytest.mark.parametrize("fused", [0, 1])
def test_callback_sees_the_history_and_stops(K, ctx, ops, fused):
    S, A, b, c = ops("kron4_sinc")
    seen = []

    def cb(w):
        seen.append(len(w.stats.residuals))
        return len(seen) == 3
    ws = _solve(K, ctx, A, b, c, fused=fused, callback=cb)
    st = ws.stats
    assert ws.last_path == fused
    assert seen == [2, 4, 6]                                     # nothing is pushed before iteration 1; two entries per iteration
    assert st.niter == 3 and st.status == "user-requested exit" and not st.solved
    xr, yr, sr = ur.usymlqr(S, b, c, itmax=3)
    assert deviation(st.residuals, sr.residuals, 1e-12) <= 1e-10 and deviation(st.Aresiduals, sr.Aresiduals, 1e-12) <= 1e-10
    x, y = _xy(ws)
    assert np.abs(x - xr).max() <= 1e-10 * np.abs(xr).max() and np.abs(y - yr).max() <= 1e-10 * np.abs(yr).max()


def test_last_path(K, ctx, ops):
    """2 by default, 1 for a callback or a user operator, 0 for fused = 0 and for every m ≠ n; a loop that never starts reports 1."""
    S, A, b, c = ops("poisson8")
    n = len(b)
    path = lambda **kw: _solve(K, ctx, A, b, c, **kw).last_path  # noqa: E731
    assert path() == 2
    assert path(callback=lambda w: False) == 1
    assert path(At=lambda x, y: A._adjoint.matvec(x, y)) == 1   # a user operator
    assert path(fused=0) == 0
    zero = _solve(K, ctx, A, np.zeros(n), np.zeros(n))
    assert zero.last_path == 1 and zero.stats.niter == 0 and zero.stats.solved and len(zero.stats.residuals) == 0
    M, br, cr = rect_system(20, 12)
    assert _solve(K, ctx, _dense(K, ctx, M), br, cr, itmax=12).last_path == 0


def test_both_false_is_the_reference_error(K, ctx, ops):
    S, A, b, c = ops("poisson8")
    with pytest.raises(K.KhipError, match="can't be both `false`"):
        _solve(K, ctx, A, b, c, ls=False, ln=False)
    with pytest.raises(K.KhipError, match="warm_start needs x0 and y0"):
        K.UsymlqrWorkspace(ctx, len(b), len(c)).warm_start_(ctx.array(b))


def test_path2_history_window_drain(K, ctx, ops):
    """A solve longer than the history window, with the three streams ending at different iterations."""
    S, A, b, c = ops("poisson16")
    ctx.set_option("hist_window", 8)
    try:
        w2 = _solve(K, ctx, A, b, c, fused=2)
    finally:
        ctx.set_option("hist_window", 1 << 14)
    w1 = _solve(K, ctx, A, b, c, fused=1)
    assert (w1.last_path, w2.last_path) == (1, 2) and summary(w2.stats) == (74, SOLVED)
    assert len(w2.stats.Aresiduals) == 62 and len(w2.stats.residuals) == 62 + 74
    _same_bits(w1, w2)


def test_nt_and_compensated_instantiations(K, ctx, oracle, ops):
    name = "kron8_sinc_it60"
    S, A, b, c = ops(name)
    kw = case_keywords(name, BOTH)
    wd = _solve(K, ctx, A, b, c, **kw)
    keep = ctx.get_option("nt_min_elems")
    ctx.set_option("nt_min_elems", 1)
    try:
        wn = _solve(K, ctx, A, b, c, **kw)
        assert wn.last_path == 2
        _same_bits(wd, wn)
    finally:
        ctx.set_option("nt_min_elems", keep)


def test_no_device_memory_growth(K, ctx, ops):
    S, A, b, c = ops("kron8_sinc_it60")
    bd, cd = ctx.array(b), ctx.array(c)
    ws = K.UsymlqrWorkspace(ctx, len(b), len(c), adopt=False)

    def solve(i):
        K.usymlqr_(ws, A, bd, cd, fused=(2, 1, 0)[i % 3], history=True, itmax=20)
    for i in range(3):
        solve(i)
    ctx.sync()
    free0 = ctx.mem_info()[0]
    for i in range(20):
        solve(i)
    ctx.sync()
    assert ctx.mem_info()[0] >= free0 - (4 << 20)


def test_profile_bracket_counts_one_p3_per_iteration(K, ctx, ops):
    """The `usymlqr_p3` bracket: one launch per iteration on the host-driven loop and per enqueued iteration on the device-resident
    one (itmax = 8 is two full chunks), beside one of each shared pass; the siblings' P3 brackets stay empty."""
    S, A, b, c = ops("kron8_sinc_it60")
    for fused, itmax in ((1, 7), (2, 8)):
        ctx.set_option("profile_spmv", 1)
        try:
            ctx.profile_kernels()
            ws = _solve(K, ctx, A, b, c, fused=fused, itmax=itmax)
            prof = ctx.profile_kernels()
        finally:
            ctx.set_option("profile_spmv", 0)
        assert ws.last_path == fused and ws.stats.niter == itmax
        assert prof["usymlqr_p3"][0] == itmax and prof["usymlqr_p3"][1] > 0.0, prof
        assert prof["ssy_p1"][0] == itmax and prof["ssy_p2"][0] == itmax, prof
        assert prof["trimr_p3"][0] == 0 and prof["usymqr_p3"][0] == 0 and prof["usymlq_p3"][0] == 0, prof
