"""symmlq! on the GPU: the three loops against the NumPy restatement of src/symmlq.jl (tests/symmlq_reference.py) and against each
other.

Budgets:
  * path 0 (one launch per primitive) against the restatement: same niter, status and solved; residuals, residualscg (NaN for NaN:
    the reference's `missing`) and x within _budget(): the two runs differ only in the rounding of the dots (compensated on the
    device, plain np.dot in NumPy) and of the axpys (fma on the device).  The budget is MEASURED per case on the restatement itself:
    its histories with np.dot against its histories with exactly summed dots (math.fsum), times 10, at least 1e-8, plus a floor of
    1e-12 ‖r₀‖.  Only cases whose own deviation is <= 1e-6 are in the history-parity list (tests/test_symmlq_host.py).
  * path 1 against path 0: elementwise values are the same expressions, the dots differ by <= 1 ulp: the same budget.
  * path 2 (device-resident) against path 1 (host-driven, same kernels, same scalar code): np.array_equal(equal_nan=True) everywhere:
    x, both histories, Anorm, Acond and every name of khip_symmlq_vector, on EVERY case.
The reference's rNorm is the residual of the LQ iterate BEFORE the iteration that reports it, and with λ ≠ 0 its recurrence does not
solve the shifted system (tests/test_symmlq_host.py, CASES): the true-residual checks are made where they hold, on λ = 0, for the CG
point against residualscg[end] and for the LQ iterate of a run one iteration shorter against residuals[k].
"""
import ctypes as C
import math
import os
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import symmlq_reference as sr  # noqa: E402
from test_bilq_host import rhs  # noqa: E402
from test_symmlq_host import (CASES, EXPECTED_NITER, PARITY_CASES, _cg, case_matrix, case_rhs, deviation,  # noqa: E402
                              reference_pair)

HIST_RTOL = 1e-8
HIST_FLOOR = 1e-12
CORE = ("x", "Mvold", "Mv", "Mv_next", "wbar")
LAZY = ("dx", "v")
KW = {"lam": "λ", "lam_est": "λest"}                      # the restatement's ASCII keywords -> the mirror's


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


def _budget(name_or_pair, oracle=None, **extra):
    """10 x the restatement's own sensitivity to the rounding of its dots (at least HIST_RTOL)."""
    (_, s1), (_, s2) = reference_pair(oracle, name_or_pair, **extra) if isinstance(name_or_pair, str) else name_or_pair
    return max(HIST_RTOL, 10.0 * deviation(s1, s2))


def _hist_ok(a, b, rtol, r0):
    """|a - b| <= rtol |b| + 1e-12 ‖r₀‖ entry by entry, NaN exactly where b has NaN."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        print(f"history: shapes {a.shape} {b.shape} or the places of NaN differ")
        return False
    m = ~np.isnan(b)
    a, b = a[m], b[m]
    with np.errstate(invalid="ignore", divide="ignore"):
        dev = np.nan_to_num(np.abs(a - b) / np.abs(b), nan=0.0, posinf=0.0) if len(b) else np.zeros(1)
    print(f"history: {len(a)} finite entries, largest relative deviation {dev.max():.3e}, budget {rtol:.3e}")
    return bool(np.all(np.abs(a - b) <= rtol * np.abs(b) + HIST_FLOOR * r0))


def _x_ok(x, xr, rtol):
    if not np.array_equal(np.isnan(x), np.isnan(xr)):
        return False
    m = ~np.isnan(xr)
    if not m.any():
        return True
    print(f"x: largest deviation {np.abs(x[m] - xr[m]).max():.3e} of {np.abs(xr[m]).max():.3e}, budget {rtol:.3e}")
    return bool(np.all(np.abs(x[m] - xr[m]) <= rtol * np.abs(xr[m]).max()))


def _scalar_ok(a, b, rtol):
    return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= rtol * abs(b)


def _solve(K, ctx, A, b, fused=2, x0=None, adopt=None, vectors=None, history=True, window=5, **kw):
    n = len(b)
    ws = K.SymmlqWorkspace(ctx, n, n, window=window, adopt=adopt, vectors=vectors)
    if x0 is not None:
        ws.warm_start_(ctx.array(x0))
    K.symmlq_(ws, A, ctx.array(b), fused=fused, history=history, **{KW.get(k, k): v for k, v in kw.items()})
    return ws


def _vectors(ws):
    return {name: ws.vector(name).to_host() for name in CORE}


def _same_bits(w1, w2, after_loop=True):
    """last_path is the caller's to assert first; then the stats, the histories, the norms, x and every named vector."""
    s1, s2 = w1.stats, w2.stats
    assert s1.niter == s2.niter and s1.status == s2.status and s1.solved == s2.solved
    for k in ("residuals", "residualscg", "errors", "errorscg"):
        assert np.array_equal(getattr(s1, k), getattr(s2, k), equal_nan=True), k
    assert np.array_equal([s1.Anorm, s1.Acond], [s2.Anorm, s2.Acond], equal_nan=True)
    assert np.array_equal(w1.x.to_host(), w2.x.to_host(), equal_nan=True)
    if after_loop:
        v1, v2 = _vectors(w1), _vectors(w2)
        for name in CORE:
            assert np.array_equal(v1[name], v2[name], equal_nan=True), name


def _device(K, ctx, S):
    return K.CsrMatrix.from_host(ctx, S.indptr, S.indices, S.data, S.shape)


_OPS = {}


@pytest.fixture(scope="module")
def ops(K, ctx, oracle):
    """(SciPy operator, device operator) of a case's (kind, size), built once per module."""
    def get(kind, size):
        if (kind, size) not in _OPS:
            S = case_matrix(oracle, kind, size)
            _OPS[(kind, size)] = (S, _device(K, ctx, S))
        return _OPS[(kind, size)]
    yield get
    _OPS.clear()


def _case(ops, name):
    kind, size, kw = CASES[name]
    S, A = ops(kind, size)
    return S, A, case_rhs(kind, S.shape[0]), dict(kw)


def _mv_is_defined(sr_, rtol):
    """Mv = Mv_next / β carries the rounding of Mv_next, about eps ‖A‖ in absolute terms, divided by β.  Where that alone may exceed
    the budget (β at rounding level: the Krylov space is exhausted, or a Lanczos breakdown) the direction of Mv is not defined
    and is not compared, nor is Mv_next = β Mv."""
    return not math.isnan(sr_.beta) and sr_.beta * rtol >= 10.0 * sr.EPS * sr_.Anorm


def _against(ws, pair, rtol, names=("Mvold", "Mv", "wbar")):
    """A solve against the restatement: the stats, both histories, the norms, x and the named vectors within the budget."""
    (xr, sr_), _ = pair
    st = ws.stats
    assert st.niter == sr_.niter and st.status == sr_.status and st.solved == sr_.solved, (st.niter, sr_.niter, st.status, sr_.status)
    assert len(st.residuals) == len(st.residualscg) == st.niter + 1
    r0 = sr_.residuals[0]
    assert _hist_ok(st.residuals, sr_.residuals, rtol, r0)
    assert _hist_ok(st.residualscg, sr_.residualscg, rtol, r0)
    assert _scalar_ok(st.Anorm, sr_.Anorm, rtol) and _scalar_ok(st.Acond, sr_.Acond, rtol)
    assert _x_ok(ws.x.to_host(), xr, rtol)
    if st.niter > 0:
        for name in names:
            if name in ("Mv", "Mv_next") and not _mv_is_defined(sr_, rtol):
                print(f"{name} is not compared: β = {sr_.beta:.3e} against ‖A‖ = {sr_.Anorm:.3e}")
                continue
            assert _x_ok(ws.vector(name).to_host(), sr_.vectors[name], rtol), name


# ---- 1. path 0 against the restatement, path 1 against path 0 --------------------------------------------------------------------
@pytest.mark.parametrize("name", PARITY_CASES)
def test_path0_against_the_restatement(K, ctx, oracle, ops, name):
    """The Lanczos breakdowns among them (breakdown, tri1): NaN for NaN, and the loop ends."""
    S, A, b, kw = _case(ops, name)
    ws = _solve(K, ctx, A, b, fused=0, **kw)
    assert ws.last_path == 0
    assert ws.stats.niter == EXPECTED_NITER[name]
    _against(ws, reference_pair(oracle, name), _budget(name, oracle), names=("Mvold", "Mv", "Mv_next", "wbar"))


@pytest.mark.parametrize("name", PARITY_CASES)
def test_path1_against_path0(K, ctx, oracle, ops, name):
    S, A, b, kw = _case(ops, name)
    w0 = _solve(K, ctx, A, b, fused=0, **kw)
    w1 = _solve(K, ctx, A, b, fused=1, **kw)
    assert (w0.last_path, w1.last_path) == (0, 1)
    s0, s1 = w0.stats, w1.stats
    assert s0.niter == s1.niter and s0.status == s1.status and s0.solved == s1.solved
    rtol = _budget(name, oracle)
    r0 = s0.residuals[0]
    assert _hist_ok(s1.residuals, s0.residuals, rtol, r0) and _hist_ok(s1.residualscg, s0.residualscg, rtol, r0)
    assert _scalar_ok(s1.Anorm, s0.Anorm, rtol) and _scalar_ok(s1.Acond, s0.Acond, rtol)
    assert _x_ok(w1.x.to_host(), w0.x.to_host(), rtol)
    (_, sr_), _ = reference_pair(oracle, name)
    for vname in ("Mvold", "Mv", "wbar"):                  # (Mv_next is scratch: the fused loops leave vₖ₋₁ there, the reference β Mv)
        if vname == "Mv" and not _mv_is_defined(sr_, rtol):
            continue
        assert _x_ok(w1.vector(vname).to_host(), w0.vector(vname).to_host(), rtol), vname


# ---- 2. path 2 bit-identical to path 1 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_path2_is_bit_identical_to_path1(K, ctx, ops, name):
    """Every case: n = 1, 2, 3, 63, 64, 65, odd n = 729 (the tail element, three workgroups), the indefinite ones, the breakdowns."""
    S, A, b, kw = _case(ops, name)
    w1 = _solve(K, ctx, A, b, fused=1, **kw)
    w2 = _solve(K, ctx, A, b, fused=2, **kw)
    assert w1.last_path == 1 and w2.last_path == 2
    _same_bits(w1, w2)
    st = w2.stats
    print(f"{name}: {st.niter} iterations (restatement {EXPECTED_NITER[name]}), {st.status}")
    assert len(st.residuals) == len(st.residualscg) == st.niter + 1
    if name in PARITY_CASES:
        assert st.niter == EXPECTED_NITER[name]


def test_lanczos_breakdown(K, ctx, oracle, ops):
    """symmetric_breakdown (test/test_utils.jl:188-192): γbar₁ = 0, so residualscg starts with NaN (missing); β₃ = 0, so Mv ends as
    0 / 0; x = [0, 1] exactly, on every path."""
    S, A, b, kw = _case(ops, "breakdown")
    (xr, sr_), _ = reference_pair(oracle, "breakdown")
    for fused in (0, 1, 2):
        ws = _solve(K, ctx, A, b, fused=fused)
        st = ws.stats
        assert ws.last_path == fused
        assert st.niter == 1 and st.solved and st.status == sr.SOLVED_CG
        assert np.array_equal(ws.x.to_host(), [0.0, 1.0])
        assert np.array_equal(st.residuals, sr_.residuals) and np.array_equal(st.residualscg, sr_.residualscg, equal_nan=True)
        assert np.isnan(st.residualscg[0]) and st.residualscg[1] == 0.0
        assert np.isnan(ws.vector("Mv").to_host()).all()


# ---- 3. alignments and instantiations --------------------------------------------------------------------------------------------
def _carved(K, ctx, n, first):
    """The five vectors of a workspace inside one buffer, starting at element `first` with an even stride: first = 1 puts every
    vector at an odd element offset (8-byte but not 16-byte aligned), first = 0 keeps them 16-byte aligned."""
    stride = n + 2 - (n & 1) + 2
    buf = ctx.zeros(first + 5 * stride)
    assert buf.ptr % 16 == 0
    vec = {k: buf.slice(first + i * stride, first + i * stride + n) for i, k in enumerate(K.SymmlqWorkspace.VECTORS)}
    assert all(v.ptr % 16 == 8 * first for v in vec.values())
    return buf, vec


@pytest.mark.parametrize("name", ["poisson8", "poisson9"])
def test_adopted_vectors_at_odd_offsets(K, ctx, ops, name):
    """Vectors offset by one double: the VEC = 1 instantiations run (with n = 729 the 16-byte path's tail element beside them):
    bit-identical to an owned workspace and to a 16-byte-aligned adoption, under path 2; nothing is written between the vectors."""
    S, A, b, kw = _case(ops, name)
    n = S.shape[0]
    wo = _solve(K, ctx, A, b, adopt=False)
    buf1, odd = _carved(K, ctx, n, 1)
    w1 = _solve(K, ctx, A, b, vectors=odd)
    buf0, even = _carved(K, ctx, n, 0)
    w0 = _solve(K, ctx, A, b, vectors=even)
    assert (wo.last_path, w1.last_path, w0.last_path) == (2, 2, 2)
    _same_bits(w1, wo)
    _same_bits(w0, wo)
    assert w1.x is odd["x"] and np.array_equal(odd["x"].to_host(), wo.x.to_host())
    stride = n + 2 - (n & 1) + 2
    for first, buf in ((1, buf1), (0, buf0)):
        h = buf.to_host()
        gaps = np.ones(len(h), dtype=bool)
        for i in range(5):
            gaps[first + i * stride:first + i * stride + n] = False
        assert not h[gaps].any(), "a kernel wrote outside its vectors"


@pytest.mark.parametrize("name", ["poisson8", "poisson9"])
def test_nontemporal_instantiations(K, ctx, ops, name):
    """nt_min_elems = 1: the NT instantiations of the two passes run; their results are bit-equal to the default's."""
    S, A, b, kw = _case(ops, name)
    wd = _solve(K, ctx, A, b)
    keep = ctx.get_option("nt_min_elems")
    assert keep > S.shape[0]                                     # the default is the cacheable instantiation at these sizes
    ctx.set_option("nt_min_elems", 1)
    try:
        w2 = _solve(K, ctx, A, b)
        w1 = _solve(K, ctx, A, b, fused=1)
    finally:
        ctx.set_option("nt_min_elems", keep)
    assert (wd.last_path, w2.last_path, w1.last_path) == (2, 2, 1)
    _same_bits(w2, wd)
    _same_bits(w1, wd)


def test_plain_accumulation(K, ctx, oracle, ops):
    """compensated = 0: the COMP = false instantiation of P2; path 2 equals its own path 1 bit for bit and stays within the case's
    budget of the compensated run."""
    S, A, b, kw = _case(ops, "poisson8")
    wd = _solve(K, ctx, A, b)
    keep = ctx.get_option("compensated")
    ctx.set_option("compensated", 0)
    try:
        w2 = _solve(K, ctx, A, b)
        w1 = _solve(K, ctx, A, b, fused=1)
    finally:
        ctx.set_option("compensated", keep)
    assert (w2.last_path, w1.last_path) == (2, 1)
    _same_bits(w1, w2)
    assert w2.stats.niter == wd.stats.niter
    rtol = _budget("poisson8", oracle)
    assert _hist_ok(w2.stats.residuals, wd.stats.residuals, rtol, wd.stats.residuals[0])
    assert _x_ok(w2.x.to_host(), wd.x.to_host(), rtol)


# ---- 4. endings ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("itmax", [1, 3])
def test_itmax(K, ctx, oracle, ops, itmax):
    """itmax = 1 and 3: after the stop Mvold, Mv and w̅ are the reference's variables on every path (the roles were rotated itmax
    times and Mv got its last kscal!), and path 2 equals path 1 in every bit."""
    S, A, b, kw = _case(ops, "poisson9")
    w = {f: _solve(K, ctx, A, b, fused=f, itmax=itmax) for f in (0, 1, 2)}
    assert [w[f].last_path for f in (0, 1, 2)] == [0, 1, 2]
    _same_bits(w[1], w[2])
    pair = reference_pair(oracle, "poisson9", itmax=itmax)
    rtol = _budget(pair)
    for f in (0, 1, 2):
        st = w[f].stats
        assert st.niter == itmax and st.status == sr.TIRED and not st.solved
        _against(w[f], pair, rtol)
        assert abs(np.linalg.norm(w[f].vector("Mv").to_host()) - 1.0) <= 1e-12          # v is normalised


@pytest.mark.parametrize("fused", [0, 1, 2])
def test_zero_right_hand_side(K, ctx, ops, fused):
    S, A = ops("poisson", 8)
    ws = _solve(K, ctx, A, np.zeros(512), fused=fused)
    st = ws.stats
    assert ws.last_path == min(fused, 1)
    assert st.niter == 0 and st.solved and st.status == "x is a zero-residual solution" and not ws.x.to_host().any()
    assert list(st.residuals) == [0.0] and list(st.residualscg) == [0.0] and math.isnan(st.Anorm) and math.isnan(st.Acond)


def test_loop_that_never_starts_reports_path_1(K, ctx, ops):
    S, A, b, kw = _case(ops, "poisson8")
    ws = _solve(K, ctx, A, b, rtol=1.0)
    st = ws.stats
    assert ws.last_path == 1 and st.niter == 0 and st.status == sr.SOLVED_LQ and st.solved and not ws.x.to_host().any()


@pytest.mark.parametrize("fused", [0, 1, 2])
def test_transfer_to_cg(K, ctx, oracle, ops, fused):
    """tiny_spd_sym.mtx ends at the CG point: with the transfer x = xᶜ = xᴸ + ζbar w̅ and ‖b - A x‖ is residualscg[end]; without it
    x = xᴸ, the status is the LQ one, and residuals[k] is the true residual of the run stopped after k - 1 iterations."""
    S, A, b, kw = _case(ops, "mtx")
    won = _solve(K, ctx, A, b, fused=fused)
    woff = _solve(K, ctx, A, b, fused=fused, transfer_to_cg=False)
    assert (won.last_path, woff.last_path) == (fused, fused)
    pair_on, pair_off = reference_pair(oracle, "mtx"), reference_pair(oracle, "mtx_lq")
    rtol = max(_budget(pair_on), _budget(pair_off))
    _against(won, pair_on, rtol)
    _against(woff, pair_off, rtol)
    assert won.stats.status == sr.SOLVED_CG and woff.stats.status == sr.SOLVED
    xc, xl = won.x.to_host(), woff.x.to_host()
    assert not np.array_equal(xc, xl)
    assert _x_ok(xl, pair_on[0][1].xlq, rtol)                                 # the same LQ iterate under both
    nb = np.linalg.norm(b)
    true_cg = np.linalg.norm(b - S @ xc)
    print(f"||b - A xc|| {true_cg:.6e}, residualscg[end] {won.stats.residualscg[-1]:.6e}")
    assert abs(true_cg - won.stats.residualscg[-1]) <= rtol * nb
    k = 6
    wk = _solve(K, ctx, A, b, fused=fused, transfer_to_cg=False, itmax=k - 1)
    true_lq = np.linalg.norm(b - S @ wk.x.to_host())
    print(f"||b - A xl(k - 1)|| {true_lq:.6e}, residuals[k] {woff.stats.residuals[k]:.6e}")
    assert abs(true_lq - woff.stats.residuals[k]) <= rtol * nb


def test_indefinite_solve_converges(K, ctx, oracle, ops):
    """A - 0.5 I assembled (one negative eigenvalue): the reference's own bound on the true residual, under path 2."""
    S, A, b, kw = _case(ops, "poisson8_shifted")
    ws = _solve(K, ctx, A, b, **kw)
    assert ws.last_path == 2 and ws.stats.solved
    x = ws.x.to_host()
    import scipy.sparse.linalg as spla
    resid = np.linalg.norm(b - S @ x) / np.linalg.norm(b)
    print(f"resid {resid:.3e}, bound {1e-6 * spla.norm(S) * np.linalg.norm(x):.3e}")
    assert resid <= 1e-6 * spla.norm(S) * np.linalg.norm(x)


@pytest.mark.parametrize("window", [1, 5, 70])
def test_error_estimates_run_the_host_driven_loop(K, ctx, oracle, ops, window):
    """λest ≠ 0 (test/test_symmlq.jl:46-62 on get_div_grad(8, 8, 8), b = ones): path 1 whatever was asked for; ‖x* - xᴸ‖ ≤
    errors[end] and ‖x* - xᶜ‖ ≤ errorscg[end]; the four histories follow the restatement, the window's rewrites included."""
    S, A = ops("poisson", 8)
    b = np.ones(512)
    dense = S.toarray()
    lam_est = (1 - 1e-10) * float(np.linalg.eigvalsh(dense)[0])
    x_exact = np.linalg.solve(dense, b)
    pair = (sr.symmlq(S, b, lam_est=lam_est, window=window, transfer_to_cg=False),
            sr.symmlq(S, b, lam_est=lam_est, window=window, transfer_to_cg=False, dot=sr.fsum_dot))
    (xr, sr_), (_, sf) = pair
    rtol = max(_budget(pair), 10.0 * sr.history_deviation(sr_.errors, sf.errors), 10.0 * sr.history_deviation(sr_.errorscg, sf.errorscg))
    print(f"window {window}: budget {rtol:.3e}")
    errcg = np.linalg.norm(x_exact - _cg(S, b))
    for fused in (2, 0):
        ws = _solve(K, ctx, A, b, fused=fused, window=window, lam_est=lam_est, transfer_to_cg=False)
        st = ws.stats
        assert ws.last_path == min(fused, 1)
        _against(ws, pair, rtol)
        assert len(st.errors) == len(st.errorscg) == st.niter + 1
        assert _hist_ok(st.errors, sr_.errors, rtol, sr_.errors[0]) and _hist_ok(st.errorscg, sr_.errorscg, rtol, sr_.errors[0])
        err = np.linalg.norm(x_exact - ws.x.to_host())
        print(f"path {ws.last_path}: ||x* - xl|| {err:.3e} <= {st.errors[-1]:.3e}; ||x* - xc|| {errcg:.3e} <= {st.errorscg[-1]:.3e}")
        assert err <= st.errors[-1] and errcg <= st.errorscg[-1]


@pytest.mark.parametrize("lam", [0.0, -0.5])
def test_warm_start(K, ctx, oracle, ops, lam):
    """x0 with and without λ (:168-172, :453): every path against the restatement, path 2 = path 1."""
    S, A, b, kw = _case(ops, "poisson8")
    x0 = np.linspace(-0.5, 0.5, 512)
    pair = reference_pair(oracle, "poisson8", x0=x0, lam=lam)
    rtol = _budget(pair)
    assert rtol <= 10 * 1e-6                                     # the warm-started runs qualify for history parity
    w = {f: _solve(K, ctx, A, b, fused=f, x0=x0, lam=lam) for f in (0, 1, 2)}
    assert [w[f].last_path for f in (0, 1, 2)] == [0, 1, 2]
    for f in (0, 1, 2):
        _against(w[f], pair, rtol)
    _same_bits(w[1], w[2])
    assert w[2].vector("dx") is not None


@pytest.mark.parametrize("fused", [0, 1, 2])
def test_without_history(K, ctx, ops, fused):
    S, A, b, kw = _case(ops, "poisson8")
    wh = _solve(K, ctx, A, b, fused=fused)
    wn = _solve(K, ctx, A, b, fused=fused, history=False)
    sn = wn.stats
    assert wn.last_path == fused
    assert len(sn.residuals) == len(sn.residualscg) == 0 and sn.niter == wh.stats.niter and sn.status == wh.stats.status
    assert np.array_equal(wn.x.to_host(), wh.x.to_host()) and sn.Anorm == wh.stats.Anorm


def test_history_window_drain(K, ctx, ops):
    S, A, b, kw = _case(ops, "poisson8_shifted")
    ctx.set_option("hist_window", 8)
    try:
        w2 = _solve(K, ctx, A, b, fused=2, **kw)
    finally:
        ctx.set_option("hist_window", 1 << 14)
    w1 = _solve(K, ctx, A, b, fused=1, **kw)
    assert (w1.last_path, w2.last_path) == (1, 2)
    assert w2.stats.niter > 8 and len(w2.stats.residuals) == len(w2.stats.residualscg) == w2.stats.niter + 1
    _same_bits(w1, w2)


def test_time_limit_already_used_up(K, ctx, ops):
    S, A, b, kw = _case(ops, "poisson8")
    for fused in (0, 1, 2):
        ws = _solve(K, ctx, A, b, fused=fused, timemax=1e-9)
        st = ws.stats
        assert ws.last_path == fused and st.niter == 1 and st.status == "time limit exceeded" and not st.solved


# ---- 5. bindings, preconditioners, callback, verbose -----------------------------------------------------------------------------
def test_out_of_place_entry_generic_interface_and_reuse(K, ctx, ops):
    """K.symmlq(A, b), as the README spells it, forwards the default callback and still runs the device-resident loop; 5n doubles;
    solution === x on an adopted workspace; one workspace serves two solves."""
    S, A, b, kw = _case(ops, "poisson8")
    n = 512
    wo = _solve(K, ctx, A, b, adopt=False)
    assert wo.last_path == 2 and wo.nbytes == 5 * 8 * n
    x, st, ws = K.symmlq(A, ctx.array(b), history=True, window=3)
    assert ws.last_path == 2 and ws.window == 3
    assert np.array_equal(x.to_host(), wo.x.to_host()) and np.array_equal(st.residuals, wo.stats.residuals)
    assert np.array_equal(st.residualscg, wo.stats.residualscg) and st.Anorm == wo.stats.Anorm and st.Acond == wo.stats.Acond
    ws3 = K.krylov_workspace("symmlq", A, ctx.array(b))
    assert isinstance(ws3, K.SymmlqWorkspace) and ws3.window == 5
    K.krylov_solve_(ws3, A, ctx.array(b), history=True)
    assert ws3.last_path == 2 and np.array_equal(ws3.x.to_host(), wo.x.to_host())
    vec = {k: ctx.empty(n) for k in K.SymmlqWorkspace.VECTORS}
    wa = K.SymmlqWorkspace(ctx, n, n, vectors=vec)
    K.symmlq_(wa, A, ctx.array(b), history=True)
    assert wa.x is vec["x"] and np.array_equal(vec["x"].to_host(), wo.x.to_host())
    first = wa.stats
    K.symmlq_(wa, A, ctx.array(b), history=True)                  # the second solve starts from the rotated roles
    second = wa.stats
    assert wa.last_path == 2 and np.array_equal(vec["x"].to_host(), wo.x.to_host())
    assert np.array_equal(first.residuals, second.residuals) and np.array_equal(first.residualscg, second.residualscg)
    assert wa.nbytes == 5 * 8 * n
    assert sorted(wa.vector(k).ptr for k in ("Mvold", "Mv", "Mv_next")) == sorted(vec[k].ptr for k in ("Mvold", "Mv", "Mv_next"))


def test_argument_errors(K, ctx, ops):
    S, A = ops("poisson", 8)
    n = 512
    small = K.SymmlqWorkspace(ctx, n - 1, n - 1)
    with pytest.raises(K.KhipError, match="inconsistent with size"):
        K.symmlq_(small, A, ctx.array(rhs(n - 1)))
    ws = K.SymmlqWorkspace(ctx, n, n)
    with pytest.raises(K.KhipError, match="Inconsistent problem size"):
        K.symmlq_(ws, A, ctx.array(rhs(n - 1)))
    with pytest.raises(K.KhipError, match="symmlq: options.variant must be 0"):
        K.symmlq_(ws, A, ctx.array(rhs(n)), variant=1)
    rect = K.SymmlqWorkspace(ctx, n, n + 1, adopt=False)
    with pytest.raises(K.KhipError, match="System must be square"):
        K.symmlq_(rect, lambda x, y: None, ctx.array(rhs(n + 1)))


def test_jacobi_preconditioner(K, ctx, oracle, ops):
    """Jacobi M on the assembled indefinite operator's SPD neighbour (tiny_spd_sym.mtx, whose diagonal is not constant): the
    host-driven loop and the primitive sequence against the restatement with v -> v / d; v appears only with M."""
    S, A, b, kw = _case(ops, "mtx")
    d = np.array(S.diagonal())
    jac = lambda v: v / d  # noqa: E731
    pair = (sr.symmlq(S, b, M=jac), sr.symmlq(S, b, M=jac, dot=sr.fsum_dot))
    rtol = _budget(pair)
    assert rtol <= 10 * 1e-6
    J = K.Jacobi(A)
    for fused, want in ((2, 1), (0, 0)):
        ws = _solve(K, ctx, A, b, fused=fused, M=J)
        assert ws.last_path == want and ws.vector("v") is not None
        _against(ws, pair, rtol, names=("Mvold", "Mv", "wbar", "v"))
    assert _solve(K, ctx, A, b).vector("v") is None


def test_ilu0_preconditioner_runs_the_host_driven_loop(K, ctx, ops):
    """ILU(0) of an SPD matrix is its IC(0), positive definite: accepted as M, path 1, and the solve meets the reference's own
    bound on the true residual (test/test_symmlq.jl:64-70)."""
    S, A, b, kw = _case(ops, "poisson8")
    ws = _solve(K, ctx, A, b, M=K.Ilu0(A))
    st = ws.stats
    x = ws.x.to_host()
    import scipy.sparse.linalg as spla
    resid = np.linalg.norm(b - S @ x) / np.linalg.norm(b)
    print(f"ILU(0) as M: {st.niter} iterations, {st.status}, resid {resid:.3e}, bound {1e-6 * spla.norm(S) * np.linalg.norm(x):.3e}")
    assert ws.last_path == 1 and st.solved and ws.vector("v") is not None
    assert resid <= 1e-6 * spla.norm(S) * np.linalg.norm(x)


def test_preconditioner_not_positive_definite(K, ctx, ops):
    S, A, b, kw = _case(ops, "poisson8")
    n = 512
    for fused in (2, 0):
        ws = K.SymmlqWorkspace(ctx, n, n)
        with pytest.raises(K.KhipError, match="Preconditioner is not positive definite") as e:
            K.symmlq_(ws, A, ctx.array(b), M=lambda x, y: K.kscalcopy_(n, y, -1.0, x), fused=fused)
        assert e.value.code == -1                                     # KHIP_ERR_INVALID
    # ⟨b, M b⟩ > 0 but ⟨v₂, M v₂⟩ < 0: the reference's own check (:205), the example of tests/test_symmlq_host.py
    import scipy.sparse as sp
    A2 = _device(K, ctx, sp.csr_matrix(np.array([[0.0, 1.0], [1.0, 0.0]])))
    sign = ctx.array(np.array([1.0, -1.0]))
    ws = K.SymmlqWorkspace(ctx, 2, 2)
    with pytest.raises(K.KhipError, match="Preconditioner is not positive definite"):
        K.symmlq_(ws, A2, ctx.array(np.array([1.0, 0.25])), M=lambda x, y: K.kvmul_(2, y, sign, x))


@pytest.mark.parametrize("fused", [0, 1])
def test_callback_stops_at_iteration_2(K, ctx, oracle, ops, fused):
    S, A, b, kw = _case(ops, "poisson8")
    seen = []

    def cb(w):
        seen.append(len(w.stats.residuals))
        return len(seen) == 2
    ws = _solve(K, ctx, A, b, fused=fused, callback=cb)
    st = ws.stats
    assert ws.last_path == fused
    assert seen == [2, 3]
    assert st.niter == 2 and st.status == "user-requested exit" and len(st.residuals) == len(st.residualscg) == 3
    (_, sr_), _ = reference_pair(oracle, "poisson8", itmax=2)
    assert np.all(np.abs(st.residuals - sr_.residuals) <= 1e-10 * sr_.residuals)


def test_last_path_and_verbose(K, ctx, ops, tmp_path):
    S, A, b, kw = _case(ops, "poisson8")
    assert _solve(K, ctx, A, b).last_path == 2
    assert _solve(K, ctx, A, b, window=70).last_path == 2                          # the window lists are not read with λest = 0
    assert _solve(K, ctx, A, b, callback=lambda w: False).last_path == 1
    assert _solve(K, ctx, lambda x, y: A.matvec(x, y), b).last_path == 1           # a user operator
    assert _solve(K, ctx, A, b, lam_est=0.1).last_path == 1
    assert _solve(K, ctx, A, b, fused=0).last_path == 0
    log = tmp_path / "symmlq.log"
    with open(log, "w") as f:
        ws = _solve(K, ctx, A, b, verbose=10, iostream=f)
    assert ws.last_path == 1
    lines = open(log, encoding="utf-8").read().splitlines()
    assert lines[0] == "SYMMLQ: system of size 512"
    assert lines[1] == "%5s  %7s  %7s  %8s  %8s  %7s  %7s  %7s  %5s" % ("k", "‖r‖", "β", "cos", "sin", "‖A‖", "κ(A)", "test1", "timer")
    rows = [ln for ln in lines[2:] if ln.strip()]
    assert [int(r.split()[0]) for r in rows] == list(range(0, ws.stats.niter + 1, 10))
    assert "✗ ✗ ✗ ✗" in rows[0] and all(r.endswith("s") for r in rows)


# ---- 6. row-partitioned ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_row_partitioned(K, ctx, oracle, ops, world):
    S, A0, b, kw = _case(ops, "poisson9")
    n = S.shape[0]
    ref_ws = _solve(K, ctx, A0, b)
    ref, xref = ref_ws.stats, ref_ws.x.to_host()
    rtol = _budget("poisson9", oracle)
    starts = K.row_partition(n, world)

    def body(cx, rank):
        r0, r1 = starts[rank], starts[rank + 1]
        sl = S[r0:r1].tocsr()
        sl.sort_indices()
        A = K.CsrMatrix.from_host(cx, sl.indptr, sl.indices, sl.data, (r1 - r0, n), dist_rows=(r0, r1), n_global=n)
        out = {}
        for fused in (2, 1):
            ws = K.SymmlqWorkspace(cx, r1 - r0, r1 - r0)
            K.symmlq_(ws, A, cx.array(b[r0:r1]), fused=fused, history=True)
            st = ws.stats
            out[fused] = (st.niter, st.status, st.residuals, st.residualscg, (st.Anorm, st.Acond), ws.last_path,
                          {k: ws.vector(k).to_host() for k in CORE})
        return out

    res = _run_ranks(K, world, 970 + world, body)
    for out in res:
        for fused in (2, 1):
            niter, status, hist, histcg, norms, path, _ = out[fused]
            assert path == fused
            assert niter == ref.niter and status == ref.status
            assert _hist_ok(hist, ref.residuals, rtol, ref.residuals[0]) and _hist_ok(histcg, ref.residualscg, rtol, ref.residuals[0])
            assert _scalar_ok(norms[0], ref.Anorm, rtol) and _scalar_ok(norms[1], ref.Acond, rtol)
        for i in (2, 3, 4):                                             # path 2 = path 1 per rank: the histories, the norms ...
            assert np.array_equal(out[2][i], out[1][i], equal_nan=True)
        for k in CORE:                                                  # ... and every vector
            assert np.array_equal(out[2][6][k], out[1][6][k]), k
        for i in (2, 3, 4):                                             # every rank has the same histories and norms
            assert np.array_equal(out[2][i], res[0][2][i], equal_nan=True)
    for fused in (2, 1):
        assert _x_ok(np.concatenate([out[fused][6]["x"] for out in res]), xref, rtol)


# ---- 7. the workspace table through the raw C entry points -----------------------------------------------------------------------
N5 = 5


def _adopt(K, ctx, n, ptrs, window=5):
    h = C.c_void_p()
    return K.lib().khip_symmlq_workspace_adopt(ctx._h, n, n, window, *ptrs, C.byref(h)), h


def test_workspace_table(K, ctx):
    L = K.lib()
    vec = {k: ctx.empty(N5) for k in CORE + LAZY}
    rc, h = _adopt(K, ctx, N5, [vec[k].ptr for k in CORE])
    assert rc == 0
    for k in CORE:
        assert L.khip_symmlq_vector(h, k.encode()) == vec[k].ptr, k
    for k in LAZY + ("nope", ""):                                        # lazy vectors are empty until needed
        assert L.khip_symmlq_vector(h, k.encode()) is None, k
    assert L.khip_symmlq_workspace_bytes(h) == len(CORE) * 8 * N5
    assert L.khip_symmlq_solution(h) == vec["x"].ptr
    for i, k in enumerate(LAZY):
        assert L.khip_symmlq_workspace_adopt_vector(h, k.encode(), vec[k].ptr) == 0, k
        assert L.khip_symmlq_workspace_bytes(h) == (len(CORE) + i + 1) * 8 * N5
        assert L.khip_symmlq_vector(h, k.encode()) == vec[k].ptr, k
    for k in CORE:                                                       # a core vector comes with khip_symmlq_workspace_adopt only
        assert L.khip_symmlq_workspace_adopt_vector(h, k.encode(), ctx.empty(N5).ptr) == -1
        assert L.khip_last_error() == f"symmlq_workspace_adopt_vector: unknown vector '{k}' ({', '.join(LAZY)})".encode()
    assert L.khip_symmlq_workspace_adopt_vector(h, b"v", vec["wbar"].ptr) == -1
    assert L.khip_last_error() == (b"symmlq_workspace_adopt_vector: the pointer for 'v' already is the workspace's 'wbar' "
                                   b"(every vector needs its own storage)")
    assert L.khip_symmlq_workspace_destroy(h) == 0
    for v in vec.values():                                               # nothing of the caller's was freed
        K.kfill_(v, 1.0)
    assert K.knorm(N5, vec["wbar"]) == pytest.approx(N5 ** 0.5)


def test_workspace_adopt_refusals_and_null_handles(K, ctx):
    L = K.lib()
    vec = [ctx.empty(N5) for _ in CORE]
    ptrs = [v.ptr for v in vec]
    ptrs[0] = ptrs[1]
    rc, _ = _adopt(K, ctx, N5, ptrs)
    assert rc == -1 and L.khip_last_error() == b"symmlq_workspace_adopt: x, Mvold, Mv, Mv_next, wbar must be distinct"
    ptrs = [v.ptr for v in vec]
    ptrs[3] = None
    rc, _ = _adopt(K, ctx, N5, ptrs)
    assert rc == -1 and L.khip_last_error() == b"symmlq_workspace_adopt: x, Mvold, Mv, Mv_next, wbar must be device vectors of n entries"
    rc, _ = _adopt(K, ctx, N5, [v.ptr for v in vec], window=-1)
    assert rc == -1 and L.khip_last_error() == b"symmlq_workspace_adopt: window must not be negative"
    rc, h = _adopt(K, ctx, 0, [None] * len(CORE))                        # n = 0: nothing to hand over
    assert rc == 0 and L.khip_symmlq_workspace_bytes(h) == 0 and L.khip_symmlq_workspace_destroy(h) == 0
    assert L.khip_symmlq_workspace_destroy(None) == 0 and L.khip_symmlq_workspace_bytes(None) == 0
    assert L.khip_symmlq_vector(None, b"x") is None and L.khip_symmlq_last_path(None) == -1


def test_created_workspace_and_lazy_vectors(K, ctx, ops):
    S, A, b, kw = _case(ops, "poisson8")
    n = 512
    ws = K.SymmlqWorkspace(ctx, n, n, adopt=False)
    assert ws.nbytes == 5 * 8 * n and ws.last_path == -1
    assert len({ws.vector(k).ptr for k in CORE}) == 5 and all(ws.vector(k) is None for k in LAZY)
    K.symmlq_(ws, A, ctx.array(b))
    assert ws.nbytes == 5 * 8 * n                                        # M = I, no warm start: nothing was added
    K.symmlq_(ws, A, ctx.array(b), M=K.Jacobi(A))
    assert ws.nbytes == 6 * 8 * n and ws.vector("v") is not None and ws.vector("dx") is None
    ws.warm_start_(ctx.array(np.zeros(n)))
    assert ws.nbytes == 7 * 8 * n and ws.vector("dx") is not None


# ---- 8. no device-memory growth --------------------------------------------------------------------------------------------------
def test_no_device_memory_growth(K, ctx, ops):
    S, A, b, kw = _case(ops, "poisson8")
    bd = ctx.array(b)
    ws = K.SymmlqWorkspace(ctx, 512, 512, adopt=False)

    def solve(i):
        K.symmlq_(ws, A, bd, fused=(2, 1, 0)[i % 3], history=True)
    for i in range(3):
        solve(i)
    ctx.sync()
    free0 = ctx.mem_info()[0]
    for i in range(20):
        solve(i)
    ctx.sync()
    assert ctx.mem_info()[0] >= free0 - (4 << 20)
