"""trimr! on the GPU: its two vector kernels alone against the NumPy expressions (bit for bit), and the three loops against the
NumPy restatement of src/trimr.jl (tests/trimr_reference.py) and against each other, at (τ, ν) = (1, −1), (1, 1), (1, 0) and (0, 0).

Budgets (tests/test_trimr_host.py holds the functions and shows that they reject the injected faults):
  * path 0 (one launch per primitive) against the restatement: same niter, status and flags; the history within budget() =
    max(1e-8, 10 x the case's own np.dot-versus-exact deviation) of each entry, plus the absolute floor 1e-12 x the first entry;
    x and y within the same budget of max|x| and max|y|.  Only cases whose own deviation is <= 1e-6 are in the list.
  * path 1 (host-driven, fused kernels) against path 0: elementwise values are the same expressions, the dots differ by <= 1 ulp:
    the same budget.
  * path 2 (device-resident) against path 1 (same kernels, same scalar code): np.array_equal everywhere: x, y, the history, the
    flags, the status and every role of khip_trimr_vector.
"q" and "p" are the two names that differ between path 0 and the fused paths after an iteration (the fused P3 does not write the
quotient back): the role comparisons against path 0 and against the restatement leave them out.
"""
import ctypes as C
import os
import sys
import threading
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trimr_reference as tm  # noqa: E402
import test_usymqr_host as qr_host  # noqa: E402
from test_bilq_host import other_c, rhs  # noqa: E402
from test_trimr_host import (ADJ, BREAKDOWN_B, BREAKDOWN_C, BREAKDOWNS, CASES, EXPECTED, INCONSISTENT, PARAMS, RECT_EXPECTED,  # noqa: E402,F401
                             RECT_KEYWORDS, RECT_SHAPES, SMALL_EXPECTED, SMALL_SIZES, SOLVED, SP, SPD, SQD, TIRED, _breakdown, budget,
                             case_keywords, case_system, dense_pair, deviation, mismatches, nonsymmetric_definite, pair_budget,
                             rect_system, reference_pair, rel_residual, role_deviation, roles_budget, summary)

ROLES = tm.VECTORS
NVEC = len(ROLES)
COMPARED = tuple(r for r in ROLES if r not in ("q", "p"))
G8 = ("gx_m3", "gx_m2", "gx_m1", "gx", "gy_m3", "gy_m2", "gy_m1", "gy")
G_ROLES = G8 + ("v_prev", "u_prev")                                  # what a wrong parity of the rotations would swap
BTOL = tm.BTOL


def _run_ranks(K, world, hub_id, body):
    """In-process ranks on one device, one thread each (the pattern of tests/test_gpu_dist.py)."""
    results, errors = [None] * world, []

    def worker(rank):
        try:
            c = K.Context(0)
            c.comm_init_local(rank, world, hub_id)
            results[rank] = body(c, rank)
            c.barrier()
            c.close()
        except Exception as e:  # pragma: no cover
            import traceback
            errors.append(f"rank {rank}: {e}\n{traceback.format_exc()}")
    ts = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=300)
    assert not errors, errors
    assert all(not t.is_alive() for t in ts), "a rank is stuck (collective mismatch)"
    return results


def _device(K, ctx, S):
    S = sp.csr_matrix(S)
    S.sort_indices()
    return K.CsrMatrix.from_host(ctx, S.indptr, S.indices, S.data, S.shape)


def _dense(K, ctx, M):
    return _device(K, ctx, sp.csr_matrix(np.asarray(M, dtype=np.float64)))


def _kw(kw):
    """The restatement's tau / nu as the mirror's τ / ν."""
    kw = dict(kw)
    for a, g in (("tau", "τ"), ("nu", "ν")):
        if a in kw:
            kw[g] = kw.pop(a)
    return kw


def _solve(K, ctx, A, b, c, fused=2, x0=None, y0=None, adopt=None, vectors=None, **kw):
    ws = K.TrimrWorkspace(ctx, len(b), len(c), adopt=adopt, vectors=vectors)
    if x0 is not None:
        ws.warm_start_(ctx.array(x0), ctx.array(y0))
    K.trimr_(ws, A, ctx.array(b), ctx.array(c), fused=fused, history=True, **_kw(kw))
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
    assert len(s2.residuals) == s2.niter + 1
    if s2.niter > 0:                                            # (before the first iteration q and p are not defined)
        r1, r2 = _roles(w1), _roles(w2)
        for name in ROLES:
            assert np.array_equal(r1[name], r2[name], equal_nan=True), name
    for a, b in zip(_xy(w1), _xy(w2)):
        assert np.array_equal(a, b, equal_nan=True)


def _against(ws, ref, bud):
    """mismatches of a workspace's solve against a restatement triple or another workspace."""
    if isinstance(ref, tuple):
        xr, yr, sr = ref
    else:
        (xr, yr), sr = _xy(ref), ref.stats
    x, y = _xy(ws)
    return mismatches(ws.stats, sr, bud, x, xr, y, yr)


def _roles_close(got, want, bud, names=COMPARED):
    """Every named vector within `bud` of the largest entry of its family (tests/test_trimr_host.py: role_deviation)."""
    for name in names:
        d = role_deviation(got, want, name)
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


# ---- 0. the two vector kernels alone, through the test exports: every output bit for bit ------------------------------------------
def _fma(a, b, c):
    """fma(a, b, c) per element, exactly rounded (rational arithmetic); a is a scalar."""
    out = np.empty(len(b))
    for i in range(len(b)):
        prod = Fraction(float(a)) * Fraction(float(b[i]))
        s = prod + Fraction(float(c[i]))
        if s != 0:
            out[i] = float(s)
        else:                                                   # an exact zero: −0 only from (−0) + (−0)
            pneg = (np.signbit(a) != np.signbit(b[i])) if prod == 0 else False
            out[i] = -0.0 if (prod == 0 and pneg and c[i] == 0 and np.signbit(c[i])) else 0.0
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


KERNEL_SIZES = (1, 2, 3, 63, 64, 65, 130)
# row one (μ₂ₖ₋₅, λ₂ₖ₋₄, η₂ₖ₋₃, σ₂ₖ₋₂, δ₂ₖ₋₁), row two (μ₂ₖ₋₄, λ₂ₖ₋₃, η₂ₖ₋₂, σ₂ₖ₋₁, δ₂ₖ): one coefficient is 0 (η₂ₖ₋₃), several are negative
ROW1 = (0.37, -1.25, 0.0, 0.81, -2.3)
ROW2 = (-0.11, 0.63, -0.92, 1.7, 3.1)
PI = (-0.45, 1.31)
FIRST_SCALE = -ROW2[3] / ROW2[4]


def _kernel_vectors(ctx, n, seed, odd):
    """Host and device copies of the sixteen streams of P3 (v_next / u_next start as NaN-free garbage).  odd: x starts at an odd
    8-byte offset, which takes the VEC = 1 path for the whole launch."""
    rng = np.random.default_rng(seed)
    names = ("x", "y") + G8 + ("v", "u", "q", "p", "v_next", "u_next")
    host = {k: rng.standard_normal(n) for k in names}
    dev = {}
    for k in names:
        if odd and k == "x":
            dev[k] = ctx.zeros(n + 1).slice(1, n + 1).copy_from_host(host[k])      # (the slice keeps its buffer alive)
            assert dev[k].ptr % 16 == 8
        else:
            dev[k] = ctx.array(host[k])
    return host, dev


def _expected_p3(stage, h, beta_next, gamma_next):
    """The NumPy expressions of P3 on host copies; returns the dict of every stream afterwards."""
    r1, r2 = [np.float64(t) for t in ROW1], [np.float64(t) for t in ROW2]
    pi1, pi2 = np.float64(PI[0]), np.float64(PI[1])
    e = {k: a.copy() for k, a in h.items()}
    n = len(h["x"])
    if stage == 1:
        e["gx_m1"] = h["v"] / r1[4]
        e["gx"] = np.float64(FIRST_SCALE) * e["gx_m1"]
        e["gy"] = h["u"] / r2[4]
        e["x"] = _fma(pi2, e["gx"], _fma(pi1, e["gx_m1"], np.zeros(n)))
        e["y"] = _fma(pi2, e["gy"], _fma(pi1, np.zeros(n), np.zeros(n)))
    else:
        for side, w in (("gx", h["v"]), ("gy", h["u"])):
            o1, o2, n1, n2 = h[side + "_m3"], h[side + "_m2"], h[side + "_m1"], h[side]
            w1, w2 = (w, None) if side == "gx" else (None, w)
            if stage == 2:
                a = tm.g_value(w1, [(r1[2], n1), (r1[3], n2)], r1[4])
                b = tm.g_value(w2, [(r2[1], n1), (r2[2], n2), (r2[3], a)], r2[4])
            else:
                a = tm.g_value(w1, [(r1[0], o1), (r1[1], o2), (r1[2], n1), (r1[3], n2)], r1[4])
                b = tm.g_value(w2, [(r2[0], o2), (r2[1], n1), (r2[2], n2), (r2[3], a)], r2[4])
            e[side + "_m3"], e[side + "_m2"] = a, b
            xy = "x" if side == "gx" else "y"
            e[xy] = _fma(pi2, b, _fma(pi1, a, h[xy]))
    e["v_next"] = h["q"] * (np.float64(1.0) / np.float64(beta_next)) if beta_next > BTOL else h["q"].copy()
    e["u_next"] = h["p"] * (np.float64(1.0) / np.float64(gamma_next)) if gamma_next > BTOL else h["p"].copy()
    return e


@pytest.mark.parametrize("odd", (False, True))
@pytest.mark.parametrize("stage", (1, 2, 3))
@pytest.mark.parametrize("n", KERNEL_SIZES)
def test_p3_kernel_is_the_numpy_expression(K, ctx, n, stage, odd):
    """trimr_p3_kernel at each stage on random vectors with chosen coefficients: every output stream bit-identical to the NumPy
    expression (g, x, y, vₖ₊₁ and uₖ₊₁ on both sides of the btol guard), every input stream unchanged.  odd: the VEC = 1 path."""
    for guards, (bn, gn) in enumerate(((2.5, 1e-13), (1e-13, 0.7))):
        host, dev = _kernel_vectors(ctx, n, 100 * n + 10 * stage + guards, odd)
        coef = (C.c_double * 16)(*ROW1, *ROW2, FIRST_SCALE, *PI, bn, gn, BTOL)
        g8 = (C.c_void_p * 8)(*[dev[k].ptr for k in G8])
        rc = K.lib().khip_test_trimr_p3(ctx._h, n, stage, coef, dev["x"].ptr, dev["y"].ptr, g8, dev["v"].ptr, dev["u"].ptr,
                                        dev["q"].ptr, dev["p"].ptr, dev["v_next"].ptr, dev["u_next"].ptr)
        assert rc == 0, K.lib().khip_last_error().decode()
        want = _expected_p3(stage, host, bn, gn)
        for k in want:
            assert _same(dev[k].to_host(), want[k]), (k, stage, n, odd, guards)


def test_p3_kernel_non_temporal_instantiation(K, ctx):
    """The same comparison with the non-temporal instantiation forced (nt_min_elems = 1), at the sizes with a tail and without."""
    keep = ctx.get_option("nt_min_elems")
    ctx.set_option("nt_min_elems", 1)
    try:
        for n in (64, 65, 130):
            for stage in (1, 2, 3):
                host, dev = _kernel_vectors(ctx, n, 7 * n + stage, False)
                coef = (C.c_double * 16)(*ROW1, *ROW2, FIRST_SCALE, *PI, 2.5, 1e-13, BTOL)
                g8 = (C.c_void_p * 8)(*[dev[k].ptr for k in G8])
                rc = K.lib().khip_test_trimr_p3(ctx._h, n, stage, coef, dev["x"].ptr, dev["y"].ptr, g8, dev["v"].ptr, dev["u"].ptr,
                                                dev["q"].ptr, dev["p"].ptr, dev["v_next"].ptr, dev["u_next"].ptr)
                assert rc == 0, K.lib().khip_last_error().decode()
                want = _expected_p3(stage, host, 2.5, 1e-13)
                for k in want:
                    assert _same(dev[k].to_host(), want[k]), (k, stage, n)
    finally:
        ctx.set_option("nt_min_elems", keep)


@pytest.mark.parametrize("n", KERNEL_SIZES)
def test_g_kernel_is_the_numpy_expression(K, ctx, n):
    """trimr_g_kernel, the four launches of an iteration of the primitive sequence at k = 2 and at k ≥ 3 (one output vector each,
    the k ≥ 3 ones in place), bit-identical to the NumPy expression and therefore to P3's g (which the P3 test holds to the same)."""
    r1, r2 = [np.float64(t) for t in ROW1], [np.float64(t) for t in ROW2]
    for stage in (2, 3):
        host, dev = _kernel_vectors(ctx, n, 31 * n + stage, False)
        want = _expected_p3(stage, host, 2.5, 0.7)
        for side, w in (("gx", "v"), ("gy", "u")):
            o1, o2, n1, n2 = (dev[side + s] for s in ("_m3", "_m2", "_m1", ""))
            w1, w2 = (dev[w].ptr, None) if side == "gx" else (None, dev[w].ptr)
            if stage == 2:
                calls = ((o1, w1, 2, (r1[2], r1[3], 0.0, 0.0), (n1, n2, None, None), r1[4]),
                         (o2, w2, 3, (r2[1], r2[2], r2[3], 0.0), (n1, n2, o1, None), r2[4]))
            else:
                calls = ((o1, w1, 4, r1[:4], (o1, o2, n1, n2), r1[4]), (o2, w2, 4, r2[:4], (o2, n1, n2, o1), r2[4]))
            for out, wp, nterm, cf, a, delta in calls:
                rc = K.lib().khip_test_trimr_g(ctx._h, n, out.ptr, wp, nterm, (C.c_double * 4)(*cf), *[v.ptr if v is not None else None for v in a],
                                               float(delta))
                assert rc == 0, K.lib().khip_last_error().decode()
        for k in G8 + ("v", "u"):
            assert _same(dev[k].to_host(), want[k]), (k, stage, n)


# ---- 1. path 0 against the restatement, path 1 against path 0, path 2 against path 1: every case, all four (τ, ν) -----------------
@pytest.mark.parametrize("params", PARAMS)
@pytest.mark.parametrize("name", list(CASES))
def test_three_paths_on_every_case(K, ctx, oracle, ops, name, params):
    S, A, b, c = ops(name)
    ref = reference_pair(oracle, name, params)[0]
    bud = budget(oracle, name, params)
    kw = case_keywords(name, params)
    w0 = _solve(K, ctx, A, b, c, fused=0, **kw)
    w1 = _solve(K, ctx, A, b, c, fused=1, **kw)
    w2 = _solve(K, ctx, A, b, c, fused=2, **kw)
    assert (w0.last_path, w1.last_path, w2.last_path) == (0, 1, 2)
    s0, s1 = w0.stats, w1.stats
    print(f"{name} (τ, ν) = {params}: budget {bud:.2e}; path 0 against the restatement "
          f"{deviation(s0.residuals, ref[2].residuals, 1e-12):.2e}; path 1 against path 0 {deviation(s1.residuals, s0.residuals, 1e-12):.2e}")
    assert summary(s0) == EXPECTED[name][PARAMS.index(params)]
    assert _against(w0, ref, bud) == []
    assert _against(w1, w0, bud) == []
    _same_bits(w1, w2)
    _roles_close(_roles(w2), _roles(w0), bud, G_ROLES)
    if s0.solved:
        x, y = _xy(w2)
        assert rel_residual(S, b, c, x, y, *params) <= 1e-6


# ---- 2. the first iterations: every named vector holds the restatement's variable ------------------------------------------------
@pytest.mark.parametrize("params", (SQD, SP))
@pytest.mark.parametrize("itmax", [1, 2, 3, 4, 5, 6])
def test_roles_hold_the_reference_variables(K, ctx, oracle, ops, itmax, params):
    """After k iterations every name of khip_trimr_vector but "q" and "p" holds what the reference's variable of that name holds at
    the end of the loop, on paths 0, 1 and 2 (1 and 2 bit-identical to each other): k = 1 … 6 walks the three stages of P3 and both
    parities of the rotation.  n = 343 is odd: the tail lane does every branch.  On path 0 "q" and "p" hold the reference's as well.
    (1, 0): σ₂ₖ₋₁ ≠ 0, so the new g₂ₖ₋₁ counts in g₂ₖ."""
    S, A, b, c = ops("kron7_it60")
    pair = reference_pair(oracle, "kron7_it60", params, itmax=itmax)
    bud = roles_budget(pair, COMPARED)
    assert bud <= 1e-6
    sr = pair[0][2]
    kw = dict(tau=params[0], nu=params[1])
    w = {f: _solve(K, ctx, A, b, c, fused=f, itmax=itmax, **kw) for f in (0, 1, 2)}
    _same_bits(w[1], w[2])
    for fused in (0, 1, 2):
        assert w[fused].last_path == fused and w[fused].stats.niter == itmax
        got = _roles(w[fused])
        _roles_close(got, sr.vectors, bud, ROLES if fused == 0 else COMPARED)
        if itmax == 1:
            assert not got["gy_m1"].any() and not any(got[k].any() for k in ("gx_m3", "gx_m2", "gy_m3", "gy_m2"))
        assert len({w[fused].vector(name).ptr for name in ROLES}) == NVEC
    # the fused paths leave q and p undivided: q = βₖ₊₁ vₖ₊₁ up to the rounding of the quotient
    got = _roles(w[2])
    coef = float(got["q"] @ got["v"]) / float(got["v"] @ got["v"])
    assert abs(coef - 1.0) > 1e-3 and np.abs(got["q"] - coef * got["v"]).max() <= 1e-12 * np.abs(got["q"]).max()
    assert np.array_equal(_roles(w[0])["q"], _roles(w[0])["v"])      # path 0: kdiv!(q) in place, then kcopy!(v, q)


# ---- 3. path 2 bit-identical to path 1 on every ending ---------------------------------------------------------------------------
def _square_breakdown():
    """ssy_mo_breakdown with a third, stored but zero, row: the same process (the third entry of every vₖ is zero), m = n = 3, so
    the fused loops run it.  At τ = ν = 1 the block matrix is singular: `inconsistent` after two iterations."""
    indptr = np.array([0, 2, 4, 5], dtype=np.int64)
    indices = np.array([0, 2, 0, 1, 2], dtype=np.int32)
    data = np.array([1.0, -1.0, -1.0, 1.0, 0.0])
    return sp.csr_matrix((data, indices, indptr), shape=(3, 3)), np.array([1.0, 1.0, 0.0]), np.ones(3)


def _endings(K, ctx, ops):
    S, A, b, c = ops("kron4_sinc")
    S8, A8, b8, c8 = ops("poisson8")
    z = np.zeros(len(b))
    Sb, bb, cb = _square_breakdown()
    Ab = K.CsrMatrix.from_host(ctx, Sb.indptr, Sb.indices, Sb.data, Sb.shape)
    M1, r1 = nonsymmetric_definite(1)
    M2, r2 = nonsymmetric_definite(2)
    return {  # ending -> (A, b, c, keywords, (niter, status), last_path of fused = 2)
        "solved_even": (A8, b8, c8, {}, (26, SOLVED), 2),
        "solved_odd": (A8, b8, c8, dict(tau=1.0, nu=1.0), (21, SOLVED), 2),
        "solved_even_sp": (A8, b8, c8, dict(tau=1.0, nu=0.0), (32, SOLVED), 2),
        "tired_even": (A, b, c, dict(itmax=40), (40, TIRED), 2),
        "tired_odd": (A, b, c, dict(itmax=7, tau=1.0, nu=0.0), (7, TIRED), 2),
        "timemax": (A, b, c, dict(timemax=1e-9), (1, "time limit exceeded"), 2),
        "inconsistent": (Ab, bb, cb, dict(tau=1.0, nu=1.0), (2, INCONSISTENT), 2),
        "solved_in_one": (_dense(K, ctx, M1), r1, other_c(1), {}, (1, SOLVED), 2),
        "solved_in_two": (_dense(K, ctx, M2), r2, other_c(2), {}, (2, SOLVED), 2),
        "b_zero": (A, z, c, dict(itmax=6), (6, TIRED), 2),
        "c_zero": (A, b, z, dict(itmax=6), (6, TIRED), 2),
        "b_and_c_zero": (A, z, z, {}, (0, SOLVED), 1),
    }


ENDINGS = ["solved_even", "solved_odd", "solved_even_sp", "tired_even", "tired_odd", "timemax", "inconsistent", "solved_in_one",
           "solved_in_two", "b_zero", "c_zero", "b_and_c_zero"]


@pytest.mark.parametrize("ending", ENDINGS)
def test_path2_is_bit_identical_to_path1(K, ctx, ops, ending):
    A, b, c, kw, want, path2 = _endings(K, ctx, ops)[ending]
    w1 = _solve(K, ctx, A, b, c, fused=1, **kw)
    w2 = _solve(K, ctx, A, b, c, fused=2, **kw)
    assert w1.last_path == 1 and w2.last_path == path2
    _same_bits(w1, w2)
    assert summary(w2.stats) == want, summary(w2.stats)
    if ending.startswith("solved") or ending.startswith("tired") or ending == "inconsistent":
        # the device loop's host enqueued more iterations than ran: the names of the g still follow the parity of niter
        w0 = _solve(K, ctx, A, b, c, fused=0, **kw)
        assert summary(w0.stats) == want
        _roles_close(_roles(w2), _roles(w0), 1e-6, G_ROLES)
    if ending == "inconsistent":
        st = w2.stats
        assert st.inconsistent and not st.solved and all(np.isfinite(a).all() for a in _xy(w2))
    if ending == "b_and_c_zero":
        assert not w2.x.to_host().any() and not w2.y.to_host().any() and list(w2.stats.residuals) == [0.0] and w2.stats.solved


@pytest.mark.parametrize("ending", ["b_zero", "c_zero"])
def test_zero_right_hand_side_is_an_ordinary_solve(K, ctx, ops, ending):
    """v₁ = 0 (or u₁ = 0) by a fill, not 0 / 0: finite everywhere, and the restatement's values on all three paths."""
    A, b, c, kw, want, _ = _endings(K, ctx, ops)[ending]
    S = ops("kron4_sinc")[0]
    pair = dense_pair(S.toarray(), b, c, **kw)
    bud = pair_budget(pair)
    for fused in (0, 1, 2):
        ws = _solve(K, ctx, A, b, c, fused=fused, **kw)
        assert ws.last_path == fused and np.isfinite(ws.stats.residuals).all()
        assert _against(ws, pair[0], bud) == [], fused


@pytest.mark.parametrize("transpose", (False, True))
def test_inconsistent_ending_on_the_breakdown_system(K, ctx, transpose):
    """ssy_mo_breakdown with τ = ν = 1 (K is singular): two iterations, `inconsistent`, x and y finite; rectangular, so path 0
    whatever `fused` says.  At (1, −1) it is solved after two."""
    M, b, c = _breakdown(transpose)
    A = _dense(K, ctx, M)
    for fused in (0, 2):
        ws = _solve(K, ctx, A, b, c, fused=fused, tau=1.0, nu=1.0)
        st = ws.stats
        assert ws.last_path == 0 and summary(st) == (2, INCONSISTENT) and st.inconsistent and not st.solved
        assert all(np.isfinite(a).all() for a in _xy(ws))
        ws = _solve(K, ctx, A, b, c, fused=fused)
        x, y = _xy(ws)
        assert summary(ws.stats) == (2, SOLVED) and rel_residual(M, b, c, x, y, 1.0, -1.0) <= 1e-6


@pytest.mark.parametrize("name", list(BREAKDOWNS))
def test_breakdown_on_one_side(K, ctx, name):
    """BREAKDOWNS: one side of the process breaks down exactly, the undivided zero vector is taken over; the same on all three
    paths."""
    M = BREAKDOWNS[name]
    A = _dense(K, ctx, M)
    pair = dense_pair(M, BREAKDOWN_B, BREAKDOWN_C)
    w = {f: _solve(K, ctx, A, BREAKDOWN_B, BREAKDOWN_C, fused=f) for f in (0, 1, 2)}
    for f in (0, 1, 2):
        assert w[f].last_path == f and _against(w[f], pair[0], pair_budget(pair)) == [], f
        assert w[f].stats.niter in (1, 3) and w[f].stats.solved
    _same_bits(w[1], w[2])
    ref1 = tm.trimr(M, BREAKDOWN_B, BREAKDOWN_C, itmax=1)[2].vectors
    first = {f: _roles(_solve(K, ctx, A, BREAKDOWN_B, BREAKDOWN_C, fused=f, itmax=1)) for f in (0, 1, 2)}
    for f in (0, 1, 2):
        for role in ("v", "u"):
            assert np.array_equal(first[f][role], ref1[role]), (f, role)
        assert not first[f]["v"].any() or not first[f]["u"].any()       # taken over undivided: the zero vector


# ---- 4. shapes where the pass can go wrong -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SMALL_SIZES)
def test_small_dense_systems(K, ctx, n):
    """nonsymmetric_definite(n) at (1, −1): one lane, one pair, a pair and the tail lane, one wave less one, one wave, one wave and
    the tail.  n = 1, 2, 3 end in stage 1, 2 and 3 of P3."""
    M, b = nonsymmetric_definite(n)
    c = other_c(n)
    pair = dense_pair(M, b, c)
    bud = pair_budget(pair)
    A = _dense(K, ctx, M)
    w0, w1, w2 = (_solve(K, ctx, A, b, c, fused=f) for f in (0, 1, 2))
    assert (w0.last_path, w1.last_path, w2.last_path) == (0, 1, 2)
    assert _against(w0, pair[0], bud) == []
    assert _against(w1, w0, bud) == []
    _same_bits(w1, w2)
    assert w2.stats.solved and w2.stats.niter == SMALL_EXPECTED[n]


def _carved(K, ctx, n, first):
    """The sixteen vectors of a workspace inside one buffer, starting at element `first` with an even stride: first = 1 puts every
    vector at an odd element offset (8-byte but not 16-byte aligned), first = 0 keeps them 16-byte aligned."""
    stride = n + 2 - (n & 1) + 2
    buf = ctx.zeros(first + NVEC * stride)
    assert buf.ptr % 16 == 0
    vec = {k: buf.slice(first + i * stride, first + i * stride + n) for i, k in enumerate(K.TrimrWorkspace.VECTORS)}
    assert all(v.ptr % 16 == 8 * first for v in vec.values())
    return buf, vec


@pytest.mark.parametrize("name", ["kron8_sinc_it60", "kron7_it60"])
def test_adopted_vectors_at_odd_offsets(K, ctx, oracle, ops, name):
    """The 8-byte kernel path (and, with n = 343, the 16-byte path's tail element beside it): bit-identical to an owned workspace
    and to a 16-byte-aligned adoption under path 2, within budget of path 0; nothing is written between the carved vectors."""
    S, A, b, c = ops(name)
    n = len(b)
    kw = case_keywords(name, SP)
    wo = _solve(K, ctx, A, b, c, adopt=False, **kw)
    buf1, odd = _carved(K, ctx, n, 1)
    w1 = _solve(K, ctx, A, b, c, vectors=odd, **kw)
    buf0, even = _carved(K, ctx, n, 0)
    w0 = _solve(K, ctx, A, b, c, vectors=even, **kw)
    assert (wo.last_path, w1.last_path, w0.last_path) == (2, 2, 2)
    _same_bits(wo, w1)
    _same_bits(wo, w0)
    wp = _solve(K, ctx, A, b, c, fused=0, **kw)
    assert wp.last_path == 0 and _against(w1, wp, budget(oracle, name, SP)) == []
    stride = n + 2 - (n & 1) + 2
    for first, buf in ((1, buf1), (0, buf0)):
        h = buf.to_host()
        gaps = np.ones(len(h), dtype=bool)
        for i in range(NVEC):
            gaps[first + i * stride:first + i * stride + n] = False
        assert not h[gaps].any(), "a kernel wrote outside its vectors"


def test_nt_and_compensated_instantiations(K, ctx, oracle, ops):
    name = "kron8_sinc_it60"
    S, A, b, c = ops(name)
    kw = case_keywords(name, SP)
    wd = _solve(K, ctx, A, b, c, **kw)
    keep = ctx.get_option("nt_min_elems")
    assert keep > len(b)
    ctx.set_option("nt_min_elems", 1)
    try:
        wn = _solve(K, ctx, A, b, c, **kw)
        assert wn.last_path == 2
        _same_bits(wd, wn)
    finally:
        ctx.set_option("nt_min_elems", keep)
    keep = ctx.get_option("compensated")
    ctx.set_option("compensated", 0)
    try:
        w1 = _solve(K, ctx, A, b, c, fused=1, **kw)
        w2 = _solve(K, ctx, A, b, c, fused=2, **kw)
        _same_bits(w1, w2)
        assert _against(w2, wd, budget(oracle, name, SP)) == []
    finally:
        ctx.set_option("compensated", keep)


def test_adopted_workspace_and_the_generic_entries(K, ctx, ops):
    name = "kron8_sinc_it60"
    S, A, b, c = ops(name)
    n = len(b)
    vec = {k: ctx.empty(n) for k in K.TrimrWorkspace.VECTORS}
    ws = K.TrimrWorkspace(ctx, n, n, vectors=vec)
    K.trimr_(ws, A, ctx.array(b), ctx.array(c), history=True, itmax=60)
    assert ws.x is vec["x"] and ws.y is vec["y"] and ws.last_path == 2      # solution(ws) is the caller's x and y
    wo = _solve(K, ctx, A, b, c, adopt=False, itmax=60)
    _same_bits(wo, ws)
    assert K.TrimrWorkspace(ctx, n, n, adopt=False).nbytes == 8 * 16 * n
    assert A._adjoint is not None and K._adjoint_of(A) is A._adjoint     # A' is taken once and kept on the matrix
    x, y, st, ws2 = K.trimr(A, ctx.array(b), ctx.array(c), history=True, itmax=60)
    assert ws2.last_path == 2                                  # the out-of-place entry forwards the default callback
    assert np.array_equal(x.to_host(), wo.x.to_host()) and np.array_equal(y.to_host(), wo.y.to_host())
    assert np.array_equal(st.residuals, wo.stats.residuals)
    ws3 = K.krylov_workspace("trimr", A, ctx.array(b), ctx.array(c))
    assert isinstance(ws3, K.TrimrWorkspace)
    K.krylov_solve_(ws3, A, ctx.array(b), c=ctx.array(c), history=True, itmax=60)
    assert ws3.last_path == 2 and np.array_equal(ws3.y.to_host(), wo.y.to_host())
    x4, y4, st4, ws4 = K.krylov_solve("trimr", A, ctx.array(b), c=ctx.array(c), history=True, itmax=60)
    assert ws4.last_path == 2 and np.array_equal(x4.to_host(), wo.x.to_host()) and np.array_equal(y4.to_host(), wo.y.to_host())


# ---- 5. parameters -------------------------------------------------------------------------------------------------------------------
def test_flags_equal_their_tau_and_nu(K, ctx, ops):
    S, A, b, c = ops("poisson8")
    for flag, params in (("flip", (-1.0, 1.0)), ("spd", (1.0, 1.0)), ("snd", (-1.0, -1.0)), ("sp", (1.0, 0.0))):
        wf = _solve(K, ctx, A, b, c, tau=3.0, nu=4.0, **{flag: True})
        wp = _solve(K, ctx, A, b, c, tau=params[0], nu=params[1])
        assert wf.last_path == 2 and wf.stats.solved
        _same_bits(wf, wp)
        x, y = _xy(wf)
        assert rel_residual(S, b, c, x, y, *params) <= 1e-6


def test_the_six_pair_errors(K, ctx, ops):
    S, A, b, c = ops("poisson8")
    assert len(tm.PAIR_ERRORS) == 6
    for pair, msg in tm.PAIR_ERRORS.items():
        with pytest.raises(K.KhipError) as e:
            _solve(K, ctx, A, b, c, **{k: True for k in pair})
        assert msg in str(e.value), (pair, str(e.value))
        assert "-1" in str(e.value) or getattr(e.value, "code", None) == -1


@pytest.mark.parametrize("name,params", [("kron7_shift24_sinc", (12.0, -0.7)), ("poisson8", (0.0, 1.0))])
def test_other_parameters(K, ctx, oracle, ops, name, params):
    S, A, b, c = ops(name)
    pair = reference_pair(oracle, name, params)
    bud = pair_budget(pair)
    w0, w1, w2 = (_solve(K, ctx, A, b, c, fused=f, **case_keywords(name, params)) for f in (0, 1, 2))
    assert (w0.last_path, w1.last_path, w2.last_path) == (0, 1, 2)
    print(f"{name} (τ, ν) = {params}: {summary(w0.stats)}, budget {bud:.2e}")
    assert _against(w0, pair[0], bud) == [] and _against(w1, w0, bud) == []
    _same_bits(w1, w2)
    if w2.stats.solved:
        x, y = _xy(w2)
        assert rel_residual(S, b, c, x, y, *params) <= 1e-6


# ---- 6. rectangular ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("itmax", [5, 0])
@pytest.mark.parametrize("shape", RECT_SHAPES)
def test_rectangular_runs_the_primitive_sequence(K, ctx, shape, itmax):
    """m ≠ n runs path 0 whatever `fused` says; x has m entries and y has n; every named vector has its side's length and the
    restatement's values.  itmax = 0 stands for the shape's keywords of the list ((33, 65) enters under its cap)."""
    m, n = shape
    M, b, c = rect_system(m, n)
    kw = dict(itmax=itmax) if itmax else RECT_KEYWORDS[shape]
    pair = dense_pair(M, b, c, **kw)
    bud = pair_budget(pair)
    A = _dense(K, ctx, M)
    for fused in (0, 2):
        ws = _solve(K, ctx, A, b, c, fused=fused, **kw)
        assert ws.last_path == 0 and summary(ws.stats) == summary(pair[0][2])
        assert summary(ws.stats) == ((5, TIRED) if itmax else RECT_EXPECTED[shape])
        assert _against(ws, pair[0], bud) == []
        x, y = _xy(ws)
        assert len(x) == m and len(y) == n and ws.nbytes == 8 * (8 * m + 8 * n)
        got = _roles(ws)
        for role in ROLES:
            assert len(got[role]) == len(pair[0][2].vectors[role]) == (m if role in K.TrimrWorkspace.ROW_SIDE else n), role
        # (at convergence βₖ₊₁ and γₖ₊₁ are rounding and vₖ₊₁, uₖ₊₁ quotients of rounding errors: roles_budget follows their own deviation)
        rbud = roles_budget(pair)
        print(f"{shape} itmax={itmax}: budget {bud:.1e}, for the work vectors {rbud:.1e}")
        _roles_close(got, pair[0][2].vectors, rbud, ROLES if not ws.stats.solved else ("x", "y"))
        if ws.stats.solved:
            assert rel_residual(M, b, c, x, y, 1.0, -1.0) <= 1e-6


def test_rectangular_warm_start(K, ctx):
    """Δx over m entries and Δy over n, with τ and ν terms in both right-hand sides."""
    m, n = 12, 20
    M, b, c = rect_system(m, n)
    x0, y0 = np.linspace(-0.5, 0.5, m), np.linspace(0.25, -0.25, n)
    pair = dense_pair(M, b, c, x0=x0, y0=y0, tau=12.0, nu=-0.7)
    for adopt in (False, True):
        ws = _solve(K, ctx, _dense(K, ctx, M), b, c, x0=x0, y0=y0, adopt=adopt, tau=12.0, nu=-0.7)
        assert ws.last_path == 0 and _against(ws, pair[0], pair_budget(pair)) == []
        x, y = _xy(ws)
        assert ws.stats.solved and rel_residual(M, b, c, x, y, 12.0, -0.7) <= 1e-6
        assert len(ws.vector("dx").to_host()) == m and len(ws.vector("dy").to_host()) == n
        assert ws.nbytes == 8 * (9 * m + 9 * n)


def test_row_partitioned_rectangular_handle_is_refused(K, oracle):
    M, b, c = qr_host.known_system("over_consistent")              # 25 x 10

    def body(cx, rank):
        r0, r1 = (0, 13) if rank == 0 else (13, 25)
        S = sp.csr_matrix(M[r0:r1])
        S.sort_indices()
        A = K.CsrMatrix.from_host(cx, S.indptr, S.indices, S.data, (r1 - r0, 25), dist_rows=(r0, r1), n_global=25)
        ws = K.TrimrWorkspace(cx, r1 - r0, 10)
        with pytest.raises(K.KhipError, match="row-partitioned rectangular system") as e:
            K.trimr_(ws, A, cx.array(b[r0:r1]), cx.array(c), At=lambda x, y: None)
        return e.value.code if hasattr(e.value, "code") else str(e.value)

    res = _run_ranks(K, 2, 35001, body)
    assert all(r == -3 or "error -3" in str(r) for r in res), res


# ---- 7. behaviour around the solve ---------------------------------------------------------------------------------------------------
def test_argument_errors(K, ctx, ops):
    S, A, b, c = ops("kron4_sinc")
    n = len(b)
    ws = K.TrimrWorkspace(ctx, n, n)
    keep = []
    op = K._make_operator(ctx, A, n, keep)
    bd, cd = ctx.array(b), ctx.array(c)
    rc = K.lib().khip_trimr_solve(ws._h, op, None, bd.ptr, cd.ptr, None, None)
    assert rc == -1 and "At" in K.lib().khip_last_error().decode()
    rc = K.lib().khip_trimr_solve(ws._h, op, K._make_operator(ctx, A.transpose(), n, keep), bd.ptr, None, None, None)
    assert rc == -1 and "c is required" in K.lib().khip_last_error().decode()
    with pytest.raises(K.KhipError, match="c .* is required"):
        K.trimr_(ws, A, bd)
    small = K.TrimrWorkspace(ctx, n - 1, n - 1)
    with pytest.raises(K.KhipError, match="inconsistent with size"):
        K.trimr_(small, A, ctx.array(rhs(n - 1)), ctx.array(rhs(n - 1)))
    with pytest.raises(K.KhipError, match="Inconsistent problem size"):
        K.trimr_(ws, A, ctx.array(rhs(n - 1)), cd)
    with pytest.raises(K.KhipError, match="Inconsistent problem size"):
        K.trimr_(ws, A, bd, ctx.array(rhs(n - 1)))
    with pytest.raises(K.KhipError, match="warm_start needs x0 and y0"):
        ws.warm_start_(bd)
    with pytest.raises(K.KhipError, match="warm_start needs x0 and y0"):
        K.trimr(A, bd, cd, y0=cd)
    assert K.lib().khip_trimr_warm_start(ws._h, bd.ptr, None) == -1
    v = [ctx.empty(n) for _ in range(NVEC)]
    v[12] = v[2]
    with pytest.raises(K.KhipError, match="must be distinct"):
        K.TrimrWorkspace(ctx, n, n, vectors=dict(zip(K.TrimrWorkspace.VECTORS, v)))
    for kw in (dict(M=A), dict(N=A)):
        with pytest.raises(K.KhipError, match="M and N other than I") as e:
            K.trimr_(ws, A, bd, cd, **kw)
        assert "-5" in str(e.value) or getattr(e.value, "code", None) == -5
    g8 = (C.c_void_p * 8)(*[bd.ptr] * 8)
    coef = (C.c_double * 16)(*[1.0] * 16)
    assert K.lib().khip_test_trimr_p3(ctx._h, n, 4, coef, bd.ptr, bd.ptr, g8, bd.ptr, bd.ptr, bd.ptr, bd.ptr, bd.ptr, bd.ptr) == -1
    assert K.lib().khip_test_trimr_g(ctx._h, n, bd.ptr, None, 5, (C.c_double * 4)(), bd.ptr, bd.ptr, bd.ptr, bd.ptr, 1.0) == -1


@pytest.mark.parametrize("adopt", [False, True])
@pytest.mark.parametrize("fused", [0, 1, 2])
def test_warm_start_with_x0_and_y0(K, ctx, oracle, ops, fused, adopt):
    """From a truncated solve to the same solution; from the solution, zero iterations.  (12, −0.7): both the τ and the ν term of
    the warm start's right-hand sides count."""
    name = "kron8_shift24_sinc"
    S, A, b, c = ops(name)
    params = (12.0, -0.7)
    kw = dict(tau=params[0], nu=params[1])
    full = _solve(K, ctx, A, b, c, fused=fused, **kw)
    xf, yf = _xy(full)
    part = _solve(K, ctx, A, b, c, fused=fused, itmax=5, **kw)
    x0, y0 = _xy(part)
    ws = _solve(K, ctx, A, b, c, fused=fused, x0=x0, y0=y0, adopt=adopt, **kw)
    assert ws.last_path == fused
    pair = reference_pair(oracle, name, params, x0=x0, y0=y0)
    assert _against(ws, pair[0], pair_budget(pair)) == []
    x, y = _xy(ws)
    assert ws.stats.solved and rel_residual(S, b, c, x, y, *params) <= 1e-6
    assert np.abs(x - xf).max() <= 1e-6 * np.abs(xf).max() and np.abs(y - yf).max() <= 1e-6 * np.abs(yf).max()
    again = _solve(K, ctx, A, b, c, fused=fused, **kw)            # the warm start is used up: a second solve equals a fresh workspace's
    K.trimr_(ws, A, ctx.array(b), ctx.array(c), fused=fused, history=True, τ=params[0], ν=params[1])
    _same_bits(again, ws)
    done = _solve(K, ctx, A, b, c, fused=fused, x0=xf, y0=yf, atol=1e-6, rtol=0.0, **kw)
    assert done.stats.niter == 0 and done.stats.solved and done.last_path == (1 if fused else 0)
    assert np.array_equal(done.x.to_host(), xf) and np.array_equal(done.y.to_host(), yf)


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
    assert seen == [2, 3, 4]
    assert st.niter == 3 and st.status == "user-requested exit" and not st.solved
    xr, yr, sr = tm.trimr(S, b, c, itmax=3)
    assert deviation(st.residuals, sr.residuals, 1e-12) <= 1e-10
    x, y = _xy(ws)
    assert np.abs(x - xr).max() <= 1e-10 * np.abs(xr).max() and np.abs(y - yr).max() <= 1e-10 * np.abs(yr).max()


def test_last_path_and_verbose(K, ctx, ops, tmp_path):
    S, A, b, c = ops("poisson8")
    n = len(b)
    path = lambda **kw: _solve(K, ctx, A, b, c, **kw).last_path  # noqa: E731
    assert path() == 2
    assert path(callback=lambda w: False) == 1
    assert path(At=lambda x, y: A._adjoint.matvec(x, y)) == 1   # a user operator
    assert path(fused=0) == 0
    zero = lambda **kw: _solve(K, ctx, A, np.zeros(n), np.zeros(n), **kw).last_path  # noqa: E731
    assert zero() == 1 and zero(fused=0) == 0                    # a loop that never starts reports 1
    log = tmp_path / "trimr.log"
    with open(log, "w") as f:
        ws = _solve(K, ctx, A, b, c, verbose=1, iostream=f)
    st = ws.stats
    assert ws.last_path == 1 and summary(st) == (26, SOLVED)
    lines = open(log, encoding="utf-8").read().splitlines()
    assert lines[0] == f"TriMR: system of {2 * n} equations in {2 * n} variables"
    assert lines[1] == "%5s  %7s  %7s  %7s  %5s" % ("k", "‖rₖ‖", "βₖ₊₁", "γₖ₊₁", "timer")
    rows = [ln for ln in lines[2:] if ln.strip()]
    assert [int(r.split()[0]) for r in rows] == list(range(0, 27))
    assert rows[0].startswith("    0  %7.1e  %7.1e  %7.1e  " % (st.residuals[0], np.linalg.norm(b), np.linalg.norm(c)))
    assert rows[10].startswith("   10  %7.1e  " % st.residuals[10]) and rows[26].startswith("   26  %7.1e  " % st.residuals[26])


def test_path2_history_window_drain(K, ctx, ops):
    """A solve longer than the history window."""
    S, A, b, c = ops("poisson16")
    ctx.set_option("hist_window", 8)
    try:
        w2 = _solve(K, ctx, A, b, c, fused=2, tau=1.0, nu=0.0)
    finally:
        ctx.set_option("hist_window", 1 << 14)
    w1 = _solve(K, ctx, A, b, c, fused=1, tau=1.0, nu=0.0)
    assert (w1.last_path, w2.last_path) == (1, 2) and summary(w2.stats) == (69, SOLVED)
    _same_bits(w1, w2)


def test_row_partitioned(K, ctx, oracle, ops):
    name = "kron8_sinc_it60"
    world = 2
    S, A0, b, c = ops(name)
    n = len(b)
    ref = _solve(K, ctx, A0, b, c, itmax=60)
    xref, yref = _xy(ref)
    bud = budget(oracle, name)
    starts = K.row_partition(n, world)

    def body(cx, rank):
        r0, r1 = starts[rank], starts[rank + 1]
        sl = sp.csr_matrix(S[r0:r1])
        sl.sort_indices()
        A = K.CsrMatrix.from_host(cx, sl.indptr, sl.indices, sl.data, (r1 - r0, n), dist_rows=(r0, r1), n_global=n)
        At = A.transpose()                                  # collective: the same partition
        out = {}
        for fused in (2, 1, 0):
            ws = K.TrimrWorkspace(cx, r1 - r0, r1 - r0)
            K.trimr_(ws, A, cx.array(b[r0:r1]), cx.array(c[r0:r1]), At=At, fused=fused, history=True, itmax=60)
            out[fused] = (ws.stats, ws.last_path, ws.x.to_host(), ws.y.to_host())
        return out

    res = _run_ranks(K, world, 35002, body)
    for out in res:
        for fused in (2, 1, 0):
            st, path = out[fused][:2]
            assert path == fused
            assert mismatches(st, ref.stats, bud) == []
        assert np.array_equal(out[2][0].residuals, out[1][0].residuals)
        assert np.array_equal(out[2][0].residuals, res[0][2][0].residuals)
    for fused in (2, 1):
        x = np.concatenate([out[fused][2] for out in res])
        y = np.concatenate([out[fused][3] for out in res])
        assert np.abs(x - xref).max() <= bud * np.abs(xref).max() and np.abs(y - yref).max() <= bud * np.abs(yref).max()
    assert all(np.array_equal(out[2][2], out[1][2]) and np.array_equal(out[2][3], out[1][3]) for out in res)


def test_no_device_memory_growth(K, ctx, ops):
    S, A, b, c = ops("kron8_sinc_it60")
    bd, cd = ctx.array(b), ctx.array(c)
    ws = K.TrimrWorkspace(ctx, len(b), len(c), adopt=False)

    def solve(i):
        K.trimr_(ws, A, bd, cd, fused=(2, 1, 0)[i % 3], history=True, itmax=20)
    for i in range(3):
        solve(i)
    ctx.sync()
    free0 = ctx.mem_info()[0]
    for i in range(20):
        solve(i)
    ctx.sync()
    assert ctx.mem_info()[0] >= free0 - (4 << 20)


def test_profile_bracket_counts_one_p3_per_iteration(K, ctx, ops):
    """The `trimr_p3` bracket: one launch per iteration on the host-driven loop and per enqueued iteration on the device-resident
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
        assert prof["trimr_p3"][0] == itmax and prof["trimr_p3"][1] > 0.0, prof
        assert prof["ssy_p1"][0] == itmax and prof["ssy_p2"][0] == itmax, prof
        assert all(prof[k][0] == 0 for k in ("usymqr_p3", "usymlq_p3", "trilqr_p3", "tricg_p3")), prof
