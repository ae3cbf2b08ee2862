"""cgs! on the GPU: the three loops against the NumPy restatement of src/cgs.jl (tests/cgs_reference.py) and against each other.

Budgets:
  * path 0 (one launch per primitive) against the restatement: same niter, status and solved; the whole residual history and x
    within _budget(): the two runs differ only in the rounding of the dots (compensated on the device, plain np.dot in NumPy) and
    of the axpys (fma on the device), and CGS, which squares the residual polynomial, carries such differences on amplified.  The
    budget is MEASURED per case on the restatement itself: its history with np.dot against its history with exactly summed dots
    (math.fsum), times 10, at least 1e-8, plus a floor of 1e-12 ‖r₀‖.  Only cases whose own deviation is <= 1e-6 are in the
    history-parity list (tests/test_cgs_host.py: kron7, kron8, kron8_negc, poisson8).
  * path 1 against path 0: elementwise values are the same expressions, the dots differ by <= 1 ulp: the same budget.
  * path 2 (device-resident) against path 1 (host-driven, same kernels, same scalar code): np.array_equal everywhere: x, the
    history and every name of khip_cgs_vector, on EVERY case (the other four need no budget for this).
  * the true residual ‖b - A x‖ <= 1e-6 ‖b‖ on every converging case: the reference's own test bound.
"""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cgs_reference as cr  # noqa: E402
from test_bilq_host import case_operator, case_vectors, rhs  # noqa: E402
from test_cgs_host import CASES, EXPECTED_NITER, PARITY_CASES, SOLVED, reference_pair  # noqa: E402

HIST_RTOL = 1e-8
HIST_FLOOR = 1e-12
TIRED = cr.TIRED
CORE = ("x", "r", "u", "p", "q", "ts")
LAZY = ("dx", "yz", "vw")
BREAKDOWN_A = [[1.0, 0.0], [1.0, 2.0]]


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
    return max(HIST_RTOL, 10.0 * cr.history_deviation(s1.residuals, s2.residuals))


def _hist_ok(a, b, rtol):
    """|a - b| <= rtol |b| + 1e-12 ‖r₀‖ entry by entry (b[0] = ‖r₀‖)."""
    a, b = np.asarray(a), np.asarray(b)
    with np.errstate(invalid="ignore", divide="ignore"):       # (a zero entry of the reference is judged by the floor below)
        dev = np.nan_to_num(np.abs(a - b) / np.abs(b), nan=0.0, posinf=0.0) if a.shape == b.shape else np.array([np.inf])
    print(f"history: {len(a)} entries, largest relative deviation {dev.max():.3e}, budget {rtol:.3e}")
    return a.shape == b.shape and bool(np.all(np.abs(a - b) <= rtol * np.abs(b) + HIST_FLOOR * b[0]))


def _x_ok(x, xr, rtol):
    print(f"x: largest deviation {np.abs(x - xr).max():.3e} of {np.abs(xr).max():.3e}, budget {rtol:.3e}")
    return bool(np.all(np.abs(x - xr) <= rtol * np.abs(xr).max()))


def _solve(K, ctx, A, b, c=None, fused=2, x0=None, adopt=None, vectors=None, history=True, **kw):
    n = len(b)
    ws = K.CgsWorkspace(ctx, n, n, adopt=adopt, vectors=vectors)
    if x0 is not None:
        ws.warm_start_(ctx.array(x0))
    K.cgs_(ws, A, ctx.array(b), c=None if c is None else ctx.array(c), fused=fused, history=history, **kw)
    return ws


def _run(K, ctx, A, b, **kw):
    ws = _solve(K, ctx, A, b, **kw)
    return ws.x.to_host(), ws.stats, ws.last_path


def _vectors(ws):
    return {name: ws.vector(name).to_host() for name in CORE}


def _same_bits(w1, w2, after_loop=True):
    """last_path is the caller's to assert first; then the stats, the history, x and every named vector."""
    s1, s2 = w1.stats, w2.stats
    assert s1.niter == s2.niter and s1.status == s2.status and s1.solved == s2.solved and s1.inconsistent == s2.inconsistent
    assert np.array_equal(s1.residuals, s2.residuals, equal_nan=True)
    assert np.array_equal(w1.x.to_host(), w2.x.to_host(), equal_nan=True)
    if after_loop:                                              # (before the first iteration u, p, q, ts are not defined)
        v1, v2 = _vectors(w1), _vectors(w2)
        for name in CORE:
            assert np.array_equal(v1[name], v2[name], equal_nan=True), name


def _device(K, ctx, A_cpu):
    return K.CsrMatrix.from_host(ctx, A_cpu.rowptr, A_cpu.col, A_cpu.val, (A_cpu.n, A_cpu.n))


def _dense(K, ctx, M):
    import scipy.sparse as sp
    S = sp.csr_matrix(np.asarray(M, dtype=np.float64))
    S.sort_indices()
    return K.CsrMatrix.from_host(ctx, S.indptr, S.indices, S.data, S.shape)


_OPS = {}


@pytest.fixture(scope="module")
def ops(K, ctx, oracle):
    """(host operator, device operator) of a case's (kind, n1), built once per module."""
    def get(kind, n1):
        if (kind, n1) not in _OPS:
            A_cpu = case_operator(oracle, kind, n1)
            _OPS[(kind, n1)] = (A_cpu, _device(K, ctx, A_cpu))
        return _OPS[(kind, n1)]
    yield get
    _OPS.clear()


def _case(ops, name):
    kind, n1, cname, kw = CASES[name]
    A_cpu, A = ops(kind, n1)
    b, c = case_vectors(A_cpu.n, cname)
    return A_cpu, A, b, c, dict(kw)


# ---- 1. path 0 against the restatement, path 1 against path 0 --------------------------------------------------------------------
@pytest.mark.parametrize("name", PARITY_CASES)
def test_path0_against_the_restatement(K, ctx, oracle, ops, name):
    A_cpu, A, b, c, kw = _case(ops, name)
    x, st, path = _run(K, ctx, A, b, c=c, fused=0, **kw)
    assert path == 0
    (xr, sr), _ = reference_pair(oracle, name)
    assert st.niter == sr.niter == EXPECTED_NITER[name] and st.status == sr.status, (st.niter, sr.niter, st.status, sr.status)
    assert st.solved == sr.solved and st.solved
    assert len(st.residuals) == st.niter + 1
    rtol = _budget(name, oracle)
    assert _hist_ok(st.residuals, sr.residuals, rtol)
    assert _x_ok(x, xr, rtol)


@pytest.mark.parametrize("name", PARITY_CASES)
def test_path1_against_path0(K, ctx, oracle, ops, name):
    A_cpu, A, b, c, kw = _case(ops, name)
    x0_, s0, p0 = _run(K, ctx, A, b, c=c, fused=0, **kw)
    x1, s1, p1 = _run(K, ctx, A, b, c=c, fused=1, **kw)
    assert (p0, p1) == (0, 1)
    assert s0.niter == s1.niter and s0.status == s1.status and s0.solved == s1.solved
    rtol = _budget(name, oracle)
    assert _hist_ok(s1.residuals, s0.residuals, rtol)
    assert _x_ok(x1, x0_, rtol)


# ---- 2. path 2 bit-identical to path 1, the true residual, niter -----------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_path2_is_bit_identical_to_path1(K, ctx, ops, name):
    """Every case, kron12 (4 workgroups of 16-byte accesses) and poisson16 (8 workgroups) among them."""
    A_cpu, A, b, c, kw = _case(ops, name)
    w1 = _solve(K, ctx, A, b, c=c, fused=1, **kw)
    w2 = _solve(K, ctx, A, b, c=c, fused=2, **kw)
    assert w1.last_path == 1 and w2.last_path == 2
    _same_bits(w1, w2)
    st = w2.stats
    assert st.status == SOLVED and st.solved and len(st.residuals) == st.niter + 1
    print(f"{name}: {st.niter} iterations (restatement {EXPECTED_NITER[name]})")
    assert st.niter == EXPECTED_NITER[name]         # no residual of the restatement is within 10 x its deviation of ε (test_cgs_host.py)
    true_res = np.linalg.norm(b - A_cpu.matvec(w2.x.to_host()))
    print(f"true residual {true_res / np.linalg.norm(b):.3e} ||b||")
    assert true_res <= 1e-6 * np.linalg.norm(b)


# ---- 3. the smallest shapes ------------------------------------------------------------------------------------------------------
def test_one_by_one(K, ctx):
    A = _dense(K, ctx, [[2.0]])
    xr, sr = cr.cgs(np.array([[2.0]]), np.array([3.0]))
    for fused in (0, 1, 2):
        x, st, path = _run(K, ctx, A, np.array([3.0]), fused=fused)
        assert path == fused and st.niter == sr.niter == 1 and st.status == sr.status and st.solved
        assert x[0] == 1.5 and np.array_equal(st.residuals, sr.residuals)


def test_alpha_breakdown_on_every_path(K, ctx):
    """n = 2, A = [[1, 0], [1, 2]], b = c = e₁: ρ₁ = 0 exactly, then σ₂ = 0, α₂ = NaN: two iterations, "breakdown αₖ == 0", the history
    [1, 1, NaN], x NaN; u, p, q of the last iteration are NaN too (its P3 ran)."""
    A = _dense(K, ctx, BREAKDOWN_A)
    e1 = np.array([1.0, 0.0])
    xr, sr = cr.cgs(np.array(BREAKDOWN_A), e1)
    assert sr.niter == 2 and sr.status == cr.BREAKDOWN
    for fused in (0, 1, 2):
        ws = _solve(K, ctx, A, e1, fused=fused)
        st = ws.stats
        assert ws.last_path == fused
        assert st.niter == 2 and st.status == sr.status and not st.solved
        assert np.array_equal(st.residuals, sr.residuals, equal_nan=True) and np.isnan(st.residuals[2])
        assert list(st.residuals[:2]) == [1.0, 1.0]
        assert np.isnan(ws.x.to_host()).all()
        for name in ("u", "p", "q", "r"):
            assert np.isnan(ws.vector(name).to_host()).all(), name


def test_odd_length(K, ctx, oracle, ops):
    """n = 343: the 16-byte kernels' scalar tail element; path 2 against path 0."""
    A_cpu, A, b, c, kw = _case(ops, "kron7")
    assert A_cpu.n == 343
    x0_, s0, p0 = _run(K, ctx, A, b, fused=0)
    x2, s2, p2 = _run(K, ctx, A, b, fused=2)
    assert (p0, p2) == (0, 2)
    assert s0.niter == s2.niter and s0.status == s2.status
    rtol = _budget("kron7", oracle)
    assert _hist_ok(s2.residuals, s0.residuals, rtol)
    assert _x_ok(x2, x0_, rtol)


def _carved(K, ctx, n, first):
    """The six vectors of a workspace inside one buffer, starting at element `first` with an even stride: first = 1 puts every
    vector at an odd element offset (8-byte but not 16-byte aligned), first = 0 keeps them 16-byte aligned."""
    stride = n + 2 - (n & 1) + 2
    buf = ctx.zeros(first + 6 * stride)
    assert buf.ptr % 16 == 0
    vec = {k: buf.slice(first + i * stride, first + i * stride + n) for i, k in enumerate(K.CgsWorkspace.VECTORS)}
    assert all(v.ptr % 16 == 8 * first for v in vec.values())
    return buf, vec


@pytest.mark.parametrize("name", ["kron8", "kron7"])
def test_adopted_vectors_at_odd_offsets(K, ctx, ops, name):
    """The 8-byte kernel path (and, with n = 343, the 16-byte path's tail element beside it): bit-identical to an owned workspace
    and to a 16-byte-aligned adoption, under path 2; nothing is written between the carved vectors."""
    A_cpu, A, b, c, kw = _case(ops, name)
    n = A_cpu.n
    wo = _solve(K, ctx, A, b, adopt=False)
    buf1, odd = _carved(K, ctx, n, 1)
    w1 = _solve(K, ctx, A, b, vectors=odd)
    buf0, even = _carved(K, ctx, n, 0)
    w0 = _solve(K, ctx, A, b, vectors=even)
    assert (wo.last_path, w1.last_path, w0.last_path) == (2, 2, 2)
    _same_bits(w1, wo)
    _same_bits(w0, wo)
    assert np.array_equal(odd["x"].to_host(), wo.x.to_host())
    stride = n + 2 - (n & 1) + 2
    for first, buf in ((1, buf1), (0, buf0)):
        h = buf.to_host()
        gaps = np.ones(len(h), dtype=bool)
        for i in range(6):
            gaps[first + i * stride:first + i * stride + n] = False
        assert not h[gaps].any(), "a kernel wrote outside its vectors"


@pytest.mark.parametrize("name", ["kron7", "kron12"])
def test_nontemporal_instantiations(K, ctx, ops, name):
    """nt_min_elems = 1: the NT instantiations of the three passes run; their results are bit-equal to the default's."""
    A_cpu, A, b, c, kw = _case(ops, name)
    wd = _solve(K, ctx, A, b)
    keep = ctx.get_option("nt_min_elems")
    assert keep > A_cpu.n                                        # the default is the cacheable instantiation at these sizes
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
    """compensated = 0: the COMP = false instantiation of P2; path 2 equals its own path 1 bit for bit and stays within the
    case's budget of the compensated run."""
    A_cpu, A, b, c, kw = _case(ops, "kron8")
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
    rtol = _budget("kron8", oracle)
    assert _hist_ok(w2.stats.residuals, wd.stats.residuals, rtol)
    assert _x_ok(w2.x.to_host(), wd.x.to_host(), rtol)


# ---- 4. endings ------------------------------------------------------------------------------------------------------------------
def test_itmax_runs_the_last_p3(K, ctx, oracle, ops):
    """itmax = 3: u, p and q after the stop are path 1's (P3 of the last iteration ran on the device-resident loop) and, within
    the budget, the reference's variables on every path."""
    A_cpu, A, b, c, kw = _case(ops, "kron7")
    w = {f: _solve(K, ctx, A, b, fused=f, itmax=3) for f in (0, 1, 2)}
    assert [w[f].last_path for f in (0, 1, 2)] == [0, 1, 2]
    _same_bits(w[1], w[2])
    pair = reference_pair(oracle, "kron7", itmax=3)
    rtol = _budget(pair)
    (xr, sr), _ = pair
    for f in (0, 1, 2):
        st = w[f].stats
        assert st.niter == 3 and st.status == TIRED and not st.solved and len(st.residuals) == 4
        for name in ("u", "p", "q", "r"):
            got, want = w[f].vector(name).to_host(), sr.vectors[name]
            dev = np.abs(got - want).max() / np.abs(want).max()
            print(f"path {f} {name}: largest deviation {dev:.3e} of its largest entry")
            assert dev <= rtol, (f, name)
    # P3 did run: u differs from r (u = r + β q)
    assert not np.array_equal(w[2].vector("u").to_host(), w[2].vector("r").to_host())


@pytest.mark.parametrize("fused", [0, 1, 2])
def test_zero_right_hand_side(K, ctx, ops, fused):
    A_cpu, A = ops("kron", 8)
    x, st, path = _run(K, ctx, A, np.zeros(A_cpu.n), fused=fused)
    assert path == min(fused, 1)
    assert st.niter == 0 and st.solved and st.status == "x is a zero-residual solution" and not x.any()
    assert list(st.residuals) == [0.0]


@pytest.mark.parametrize("fused", [0, 1, 2])
def test_c_orthogonal_to_b(K, ctx, ops, fused):
    A_cpu, A = ops("kron", 8)
    b = rhs(A_cpu.n)
    c = np.zeros(A_cpu.n)
    c[0], c[1] = b[1], -b[0]                                    # cᴴb = b₁b₀ - b₀b₁ = 0 exactly
    x, st, path = _run(K, ctx, A, b, c=c, fused=fused)
    assert path == min(fused, 1)
    assert st.niter == 0 and not st.solved and st.status == "Breakdown bᴴc = 0" and not x.any()
    assert len(st.residuals) == 1


def test_loop_that_never_starts_reports_path_1(K, ctx, ops):
    A_cpu, A, b, c, kw = _case(ops, "kron8")
    x, st, path = _run(K, ctx, A, b, rtol=1.0)
    assert path == 1 and st.niter == 0 and st.status == SOLVED and st.solved and not x.any()


@pytest.mark.parametrize("fused", [0, 1, 2])
def test_warm_start(K, ctx, oracle, ops, fused):
    A_cpu, A, b, c, kw = _case(ops, "kron8")
    x0 = np.linspace(-0.5, 0.5, A_cpu.n)
    x, st, path = _run(K, ctx, A, b, fused=fused, x0=x0)
    assert path == fused
    pair = reference_pair(oracle, "kron8", x0=x0)
    (xr, sr), _ = pair
    rtol = _budget(pair)
    assert rtol <= 10 * 1e-6                                     # the warm-started run qualifies for history parity (1.8e-10 of its own)
    assert st.niter == sr.niter and st.solved and st.status == sr.status
    assert _hist_ok(st.residuals, sr.residuals, rtol)
    assert _x_ok(x, xr, rtol)
    assert np.linalg.norm(b - A_cpu.matvec(x)) <= 1e-6 * np.linalg.norm(b)


def test_warm_start_path2_equals_path1(K, ctx, ops):
    A_cpu, A, b, c, kw = _case(ops, "kron8")
    x0 = np.linspace(-0.5, 0.5, A_cpu.n)
    w1 = _solve(K, ctx, A, b, fused=1, x0=x0)
    w2 = _solve(K, ctx, A, b, fused=2, x0=x0)
    assert (w1.last_path, w2.last_path) == (1, 2)
    _same_bits(w1, w2)
    assert w2.vector("dx") is not None


@pytest.mark.parametrize("fused", [0, 1, 2])
def test_without_history(K, ctx, ops, fused):
    A_cpu, A, b, c, kw = _case(ops, "kron8")
    wh = _solve(K, ctx, A, b, fused=fused)
    wn = _solve(K, ctx, A, b, fused=fused, history=False)
    assert wn.last_path == fused
    assert len(wn.stats.residuals) == 0 and wn.stats.niter == wh.stats.niter and wn.stats.status == SOLVED
    assert np.array_equal(wn.x.to_host(), wh.x.to_host())


def test_history_window_drain(K, ctx, ops):
    A_cpu, A, b, c, kw = _case(ops, "kron8_rtol12")
    ctx.set_option("hist_window", 8)
    try:
        w2 = _solve(K, ctx, A, b, fused=2, **kw)
    finally:
        ctx.set_option("hist_window", 1 << 14)
    w1 = _solve(K, ctx, A, b, fused=1, **kw)
    assert (w1.last_path, w2.last_path) == (1, 2)
    assert w2.stats.niter > 8 and len(w2.stats.residuals) == w2.stats.niter + 1
    _same_bits(w1, w2)


def test_time_limit(K, ctx, ops):
    A_cpu, A, b, c, kw = _case(ops, "kron8")
    for fused in (1, 2):
        x, st, path = _run(K, ctx, A, b, fused=fused, timemax=1e-9)
        assert path == fused and st.niter == 1 and st.status == "time limit exceeded" and not st.solved


# ---- 5. bindings, preconditioners, callback, verbose -----------------------------------------------------------------------------
def test_out_of_place_entry_and_generic_interface(K, ctx, ops):
    """K.cgs(A, b), as the README spells it, forwards the default callback and still runs the device-resident loop."""
    A_cpu, A, b, c, kw = _case(ops, "kron8")
    wo = _solve(K, ctx, A, b, adopt=False)
    assert wo.last_path == 2 and wo.nbytes == 6 * 8 * A_cpu.n
    x, st, ws = K.cgs(A, ctx.array(b), history=True)
    assert ws.last_path == 2
    assert np.array_equal(x.to_host(), wo.x.to_host()) and np.array_equal(st.residuals, wo.stats.residuals)
    ws3 = K.krylov_workspace("cgs", A, ctx.array(b))
    assert isinstance(ws3, K.CgsWorkspace)
    K.krylov_solve_(ws3, A, ctx.array(b), history=True)
    assert ws3.last_path == 2 and np.array_equal(ws3.x.to_host(), wo.x.to_host())
    vec = {k: ctx.empty(A_cpu.n) for k in K.CgsWorkspace.VECTORS}
    wa = K.CgsWorkspace(ctx, A_cpu.n, A_cpu.n, vectors=vec)
    K.cgs_(wa, A, ctx.array(b))
    assert wa.x is vec["x"] and np.array_equal(vec["x"].to_host(), wo.x.to_host())


def test_argument_errors(K, ctx, ops):
    A_cpu, A = ops("kron", 8)
    n = A_cpu.n
    small = K.CgsWorkspace(ctx, n - 1, n - 1)
    with pytest.raises(K.KhipError, match="inconsistent with size"):
        K.cgs_(small, A, ctx.array(rhs(n - 1)))
    ws = K.CgsWorkspace(ctx, n, n)
    with pytest.raises(K.KhipError, match="Inconsistent problem size"):
        K.cgs_(ws, A, ctx.array(rhs(n - 1)))
    with pytest.raises(K.KhipError, match="cgs: options.variant must be 0"):
        K.cgs_(ws, A, ctx.array(rhs(n)), variant=1)
    rect = K.CgsWorkspace(ctx, n, n + 1, adopt=False)
    with pytest.raises(K.KhipError, match="System must be square"):
        K.cgs_(rect, lambda x, y: None, ctx.array(rhs(n + 1)))


@pytest.mark.parametrize("which", ["M", "N", "MN"])
def test_jacobi_preconditioners(K, ctx, oracle, ops, which):
    """Jacobi M, Jacobi N, both: the host-driven loop (and the primitive sequence) against the restatement with v -> v / d; vw and
    yz appear only where M and N need them.  The restatement's own deviations are 6.8e-8, 4.7e-8 and 3.6e-7: all three qualify."""
    A_cpu, A, b, c, kw = _case(ops, "kron8")
    S = A_cpu.to_scipy()
    d = np.array(S.diagonal())
    jac = lambda v: v / d  # noqa: E731
    ref_kw = {k: jac for k in which}
    pair = (cr.cgs(S, b, **ref_kw), cr.cgs(S, b, dot=cr.fsum_dot, **ref_kw))
    rtol = _budget(pair)
    assert rtol <= 10 * 1e-6
    (xr, sr), _ = pair
    J = K.Jacobi(A)
    for fused, want in ((2, 1), (0, 0)):
        ws = _solve(K, ctx, A, b, fused=fused, **{k: J for k in which})
        x, st = ws.x.to_host(), ws.stats
        assert ws.last_path == want
        assert (ws.vector("vw") is not None) == ("M" in which) and (ws.vector("yz") is not None) == ("N" in which)
        assert st.niter == sr.niter and st.status == sr.status and st.solved
        assert _hist_ok(st.residuals, sr.residuals, rtol)
        assert _x_ok(x, xr, rtol)
        assert np.linalg.norm(b - A_cpu.matvec(x)) <= 1e-6 * np.linalg.norm(b)


@pytest.mark.parametrize("which", ["M", "N"])
def test_ilu0_preconditioner_runs_the_host_driven_loop(K, ctx, ops, which):
    """ILU(0) needs no adjoint here (cgs! is transpose-free): it is accepted on either side, runs path 1 and converges to the
    reference's true-residual bound (with N the residual the loop tests is that of A N⁻¹, the same vector)."""
    A_cpu, A, b, c, kw = _case(ops, "kron8")
    ws = _solve(K, ctx, A, b, **{which: K.Ilu0(A)})
    st = ws.stats
    print(f"ILU(0) as {which}: {st.niter} iterations")
    assert ws.last_path == 1 and st.solved and st.status == SOLVED
    if which == "N":
        assert np.linalg.norm(b - A_cpu.matvec(ws.x.to_host())) <= 1e-6 * np.linalg.norm(b)


@pytest.mark.parametrize("fused", [0, 1])
def test_callback_sees_the_history_and_stops(K, ctx, ops, fused):
    A_cpu, A, b, c, kw = _case(ops, "kron8")
    seen = []

    def cb(w):
        seen.append(len(w.stats.residuals))
        return len(seen) == 3
    x, st, path = _run(K, ctx, A, b, fused=fused, callback=cb)
    assert path == fused
    assert seen == [2, 3, 4]
    assert st.niter == 3 and st.status == "user-requested exit" and len(st.residuals) == 4
    _, sr = cr.cgs(A_cpu.to_scipy(), b, itmax=3)
    assert np.all(np.abs(st.residuals - sr.residuals) <= 1e-10 * sr.residuals)


def test_last_path_and_verbose(K, ctx, ops, tmp_path):
    A_cpu, A, b, c, kw = _case(ops, "kron8")
    assert _run(K, ctx, A, b)[2] == 2
    assert _run(K, ctx, A, b, callback=lambda w: False)[2] == 1
    assert _run(K, ctx, lambda x, y: A.matvec(x, y), b)[2] == 1                    # a user operator
    assert _run(K, ctx, A, b, fused=0)[2] == 0
    log = tmp_path / "cgs.log"
    with open(log, "w") as f:
        x, st, path = _run(K, ctx, A, b, verbose=10, iostream=f)
    assert path == 1
    lines = open(log, encoding="utf-8").read().splitlines()
    assert lines[0] == f"CGS: system of size {A_cpu.n}"
    assert lines[1] == "%5s  %7s  %5s" % ("k", "‖rₖ‖", "timer")
    rows = [ln for ln in lines[2:] if ln.strip()]
    assert [int(r.split()[0]) for r in rows] == list(range(0, st.niter + 1, 10))
    assert all(len(r.split()) == 3 and r.endswith("s") for r in rows)


# ---- 6. row-partitioned ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_row_partitioned(K, ctx, oracle, ops, world):
    A_cpu, A0, b, c, kw = _case(ops, "kron8")
    n = A_cpu.n
    xref, ref, _ = _run(K, ctx, A0, b)
    rtol = _budget("kron8", oracle)
    starts = K.row_partition(n, world)

    def body(cx, rank):
        r0, r1 = starts[rank], starts[rank + 1]
        sl = A_cpu.row_slice(r0, r1)
        A = K.CsrMatrix.from_host(cx, sl.rowptr, sl.col, sl.val, (r1 - r0, n), dist_rows=(r0, r1), n_global=n)
        out = {}
        for fused in (2, 1):
            ws = K.CgsWorkspace(cx, r1 - r0, r1 - r0)
            K.cgs_(ws, A, cx.array(b[r0:r1]), fused=fused, history=True)
            st = ws.stats
            out[fused] = (st.niter, st.status, st.residuals, ws.last_path, {k: ws.vector(k).to_host() for k in CORE})
        return out

    res = _run_ranks(K, world, 960 + world, body)
    for out in res:
        for fused in (2, 1):
            niter, status, hist, path, _ = out[fused]
            assert path == fused
            assert niter == ref.niter and status == ref.status
            assert _hist_ok(hist, ref.residuals, rtol)
        assert np.array_equal(out[2][2], out[1][2])                     # path 2 = path 1 per rank: the history ...
        for k in CORE:                                                  # ... and every vector
            assert np.array_equal(out[2][4][k], out[1][4][k]), k
        assert np.array_equal(out[2][2], res[0][2][2])                  # every rank has the same history
    for fused in (2, 1):
        assert _x_ok(np.concatenate([out[fused][4]["x"] for out in res]), xref, rtol)


# ---- 7. the workspace table through the raw C entry points -----------------------------------------------------------------------
N5 = 5


def _adopt(K, ctx, n, ptrs):
    h = C.c_void_p()
    return K.lib().khip_cgs_workspace_adopt(ctx._h, n, n, *ptrs, C.byref(h)), h


def test_workspace_table(K, ctx):
    L = K.lib()
    vec = {k: ctx.empty(N5) for k in CORE + LAZY}
    rc, h = _adopt(K, ctx, N5, [vec[k].ptr for k in CORE])
    assert rc == 0
    for k in CORE:
        assert L.khip_cgs_vector(h, k.encode()) == vec[k].ptr, k
    for k in LAZY + ("nope", ""):                                        # lazy vectors are empty until needed
        assert L.khip_cgs_vector(h, k.encode()) is None, k
    assert L.khip_cgs_workspace_bytes(h) == len(CORE) * 8 * N5
    assert L.khip_cgs_solution(h) == vec["x"].ptr
    for i, k in enumerate(LAZY):
        assert L.khip_cgs_workspace_adopt_vector(h, k.encode(), vec[k].ptr) == 0, k
        assert L.khip_cgs_workspace_bytes(h) == (len(CORE) + i + 1) * 8 * N5
        assert L.khip_cgs_vector(h, k.encode()) == vec[k].ptr, k
    for k in CORE:                                                       # a core vector comes with khip_cgs_workspace_adopt only
        assert L.khip_cgs_workspace_adopt_vector(h, k.encode(), ctx.empty(N5).ptr) == -1
        assert L.khip_last_error() == f"cgs_workspace_adopt_vector: unknown vector '{k}' ({', '.join(LAZY)})".encode()
    assert L.khip_cgs_workspace_adopt_vector(h, b"yz", vec["ts"].ptr) == -1
    assert L.khip_last_error() == (b"cgs_workspace_adopt_vector: the pointer for 'yz' already is the workspace's 'ts' "
                                   b"(every vector needs its own storage)")
    assert L.khip_cgs_workspace_destroy(h) == 0
    for v in vec.values():                                               # nothing of the caller's was freed
        K.kfill_(v, 1.0)
    assert K.knorm(N5, vec["ts"]) == pytest.approx(N5 ** 0.5)


def test_workspace_adopt_refusals(K, ctx):
    L = K.lib()
    vec = [ctx.empty(N5) for _ in CORE]
    for i in (0, len(CORE) - 1):
        ptrs = [v.ptr for v in vec]
        ptrs[i] = ptrs[(i + 1) % len(CORE)]
        rc, _ = _adopt(K, ctx, N5, ptrs)
        assert rc == -1 and L.khip_last_error() == b"cgs_workspace_adopt: x, r, u, p, q, ts must be distinct"
    for i in (0, 3, len(CORE) - 1):
        ptrs = [v.ptr for v in vec]
        ptrs[i] = None
        rc, _ = _adopt(K, ctx, N5, ptrs)
        assert rc == -1 and L.khip_last_error() == b"cgs_workspace_adopt: x, r, u, p, q, ts must be device vectors of n entries"


def test_created_workspace_and_lazy_vectors(K, ctx, ops):
    L = K.lib()
    rc, h = _adopt(K, ctx, 0, [None] * len(CORE))                        # n = 0: nothing to hand over
    assert rc == 0 and L.khip_cgs_workspace_bytes(h) == 0 and L.khip_cgs_workspace_destroy(h) == 0
    assert L.khip_cgs_workspace_destroy(None) == 0 and L.khip_cgs_workspace_bytes(None) == 0
    assert L.khip_cgs_vector(None, b"x") is None and L.khip_cgs_last_path(None) == -1
    A_cpu, A, b, c, kw = _case(ops, "kron8")
    n = A_cpu.n
    ws = K.CgsWorkspace(ctx, n, n, adopt=False)
    assert ws.nbytes == 6 * 8 * n and ws.last_path == -1
    ptrs = [ws.vector(k).ptr for k in CORE]
    assert len(set(ptrs)) == 6 and all(ws.vector(k) is None for k in LAZY)
    K.cgs_(ws, A, ctx.array(b))
    assert ws.nbytes == 6 * 8 * n                                        # M = N = I, no warm start: nothing was added
    K.cgs_(ws, A, ctx.array(b), M=K.Jacobi(A))
    assert ws.nbytes == 7 * 8 * n and ws.vector("vw") is not None and ws.vector("yz") is None
    K.cgs_(ws, A, ctx.array(b), N=K.Jacobi(A))
    assert ws.nbytes == 8 * 8 * n and ws.vector("yz") is not None
    ws.warm_start_(ctx.array(np.zeros(n)))
    assert ws.nbytes == 9 * 8 * n and ws.vector("dx") is not None


# ---- 8. no device-memory growth --------------------------------------------------------------------------------------------------
def test_no_device_memory_growth(K, ctx, ops):
    A_cpu, A, b, c, kw = _case(ops, "kron8")
    bd = ctx.array(b)
    ws = K.CgsWorkspace(ctx, A_cpu.n, A_cpu.n, adopt=False)

    def solve(i):
        K.cgs_(ws, A, bd, fused=(2, 1, 0)[i % 3], history=True)
    for i in range(3):
        solve(i)
    ctx.sync()
    free0 = ctx.mem_info()[0]
    for i in range(20):
        solve(i)
    ctx.sync()
    assert ctx.mem_info()[0] >= free0 - (4 << 20)
