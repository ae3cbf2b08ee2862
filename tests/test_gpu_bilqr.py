"""bilqr! on the GPU: the three loops against the NumPy restatement of src/bilqr.jl (tests/bilqr_reference.py) and against each
other.

Budgets, those of tests/test_gpu_qmr.py, applied to BOTH histories and to x and y:
  * path 0 (one launch per primitive) against the restatement: same niter, full status, solved_primal, solved_dual and both history
    lengths; both residual histories within _budget(): the two runs differ only in the rounding of the dots (compensated on the
    device, plain np.dot in NumPy) and of the axpys (fma on the device), and the two-sided Lanczos recurrence carries such
    differences on undamped.  The budget is MEASURED per case on the restatement itself: the larger deviation of its two histories
    with np.dot against exactly summed dots (math.fsum), times 10, at least 1e-8, plus 1e-12 beta_1 with beta_1 = sqrt(|c.r_0|).
    Only cases whose own deviation is <= 1e-6 are in the list (tests/test_bilqr_host.py).
  * path 2 (device-resident) against path 1 (host-driven, same kernels, same scalar code): np.array_equal everywhere: x, y, both
    histories and every role of khip_bilqr_vector.
  * path 1 against path 0: elementwise values are the same expressions, the dots differ by <= 1 ulp: the same budget.
"""
import os
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bilqr_reference as qq  # noqa: E402
from test_bilq_host import case_operator, other_c, rhs  # noqa: E402
from test_bilqr_host import CASES, EXPECTED, VECTORS, case_vectors, pair_deviation, reference_pair  # noqa: E402

HIST_RTOL = 1e-8
HIST_FLOOR = 1e-12
ROLES = VECTORS


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
    pair = reference_pair(oracle, name_or_pair, **extra) if isinstance(name_or_pair, str) else name_or_pair
    return max(HIST_RTOL, 10.0 * pair_deviation(pair))


def _beta1(oracle, name):
    return reference_pair(oracle, name)[0][2].beta1


def _hist_ok(a, b, beta1, rtol, what="history"):
    a, b = np.asarray(a), np.asarray(b)
    same_nan = a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b))
    a, b = np.nan_to_num(a, nan=0.0), np.nan_to_num(b, nan=0.0)             # (a NaN entry must be a NaN entry: same_nan)
    with np.errstate(invalid="ignore", divide="ignore"):       # (a zero entry of the reference is judged by the floor below)
        dev = np.nan_to_num(np.abs(a - b) / np.abs(b), nan=0.0, posinf=0.0) if a.shape == b.shape else np.array([np.inf])
    print(f"{what}: {len(a)} entries, largest relative deviation {dev.max():.3e}, budget {rtol:.3e}")
    return same_nan and bool(np.all(np.abs(a - b) <= rtol * np.abs(b) + HIST_FLOOR * beta1))


def _both_hist_ok(st, sr, beta1, rtol):
    return (_hist_ok(st.residuals_primal, sr.residuals_primal, beta1, rtol, "primal history")
            and _hist_ok(st.residuals_dual, sr.residuals_dual, beta1, rtol, "dual history"))


def _x_ok(x, xr, rtol, what="x"):
    print(f"{what}: largest deviation {np.abs(x - xr).max():.3e} of {np.abs(xr).max():.3e}, budget {rtol:.3e}")
    return bool(np.all(np.abs(x - xr) <= max(1e-8, rtol) * max(np.abs(xr).max(), 1e-300)))


def _solve(K, ctx, A, b, c, fused=2, x0=None, y0=None, adopt=None, vectors=None, **kw):
    n = len(b)
    ws = K.BilqrWorkspace(ctx, n, n, adopt=adopt, vectors=vectors)
    if x0 is not None:
        ws.warm_start_(ctx.array(x0), ctx.array(y0))
    K.bilqr_(ws, A, ctx.array(b), ctx.array(c), fused=fused, history=True, **kw)
    return ws


def _run(K, ctx, A, b, c, **kw):
    ws = _solve(K, ctx, A, b, c, **kw)
    return ws.x.to_host(), ws.y.to_host(), ws.stats, ws.last_path


def _roles(ws):
    return {name: ws.vector(name).to_host() for name in ROLES}


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


def _same_stats(s1, s2):
    return (s1.niter == s2.niter and s1.status == s2.status and s1.solved_primal == s2.solved_primal
            and s1.solved_dual == s2.solved_dual and len(s1.residuals_primal) == len(s2.residuals_primal)
            and len(s1.residuals_dual) == len(s2.residuals_dual))


# ---- 1. path 0 against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_path0_against_the_restatement(K, ctx, oracle, ops, name):
    A_cpu, A, b, c, kw = _case(ops, name)
    x, y, st, path = _run(K, ctx, A, b, c, fused=0, **kw)
    assert path == 0
    (xr, yr, sr), _ = reference_pair(oracle, name)
    print(f"niter {st.niter} / {sr.niter}, histories {len(st.residuals_primal)} / {len(st.residuals_dual)}, {st.status}")
    assert _same_stats(st, sr), (st.niter, sr.niter, st.status, sr.status)
    assert (st.niter, len(st.residuals_primal), len(st.residuals_dual)) == EXPECTED[name]
    rtol = _budget(name, oracle)
    assert _both_hist_ok(st, sr, sr.beta1, rtol)
    assert _x_ok(x, xr, rtol) and _x_ok(y, yr, rtol, "y")
    assert st.solved_primal and st.solved_dual and st.solved
    S = A_cpu.to_scipy()
    assert np.linalg.norm(b - S @ x) <= 1e-6 * np.linalg.norm(b) and np.linalg.norm(c - S.T @ y) <= 1e-6 * np.linalg.norm(c)


# ---- 2. path 2 bit-identical to path 1 -------------------------------------------------------------------------------------------
def _endings(K, ctx, ops):
    A_cpu, A = ops("kron", 8)
    A7_cpu, A7 = ops("kron", 7)
    n = A_cpu.n
    b, cs = rhs(n), other_c(n)
    b7, c7 = rhs(A7_cpu.n), other_c(A7_cpu.n)
    ident = _dense(K, ctx, np.eye(5))
    b5 = np.arange(1.0, 6.0)
    two = _dense(K, ctx, [[0.0, 1.0], [-1.0, 0.0]])
    diag = _dense(K, ctx, [[1.0, 0.0], [0.0, 2.0]])
    one = _dense(K, ctx, [[2.0]])
    c_orth = np.zeros(n)
    c_orth[0], c_orth[1] = b[1], -b[0]                       # cᴴb = b₁b₀ - b₀b₁ = 0 exactly
    out = {  # ending -> (A, b, c, keywords, status, niter or None, runs the loop)
        "both": (A, b, b, {}, qq.BOTH_C, 40, True),
        "lq": (A7, b7, c7, dict(transfer_to_bicg=False), qq.BOTH_L, 39, True),
        "primal_first": (A7, b7, c7, {}, qq.BOTH_C, 39, True),          # P3 goes on without its primal part for 4 iterations
        "dual_first": (A, b, cs, {}, qq.BOTH_C, 41, True),              # ... and without its dual part for 2
        "b_zero": (A, np.zeros(n), b, {}, qq.BC_BREAKDOWN, 0, False),
        "timemax": (A, b, cs, dict(timemax=1e-9), "time limit exceeded", 1, True),
        "identity": (ident, b5, b5, {}, qq.BREAKDOWN, 1, True),
        "two_by_two": (two, np.array([1.0, 0.0]), np.array([-1.0, 0.0]), {}, qq.BREAKDOWN, 2, True),
        "diag": (diag, np.array([1.0, 1.0]), np.array([1.0, 2.0]), {}, None, 3, True),
        "one_by_one": (one, np.array([3.0]), np.array([5.0]), {}, None, 2, True),
        "mach": (A, b, cs, dict(atol=0.0, rtol=0.0), None, None, True),              # ε = 0: the mach tests or itmax
        "cb_zero": (A, b, c_orth, {}, qq.BC_BREAKDOWN, 0, False),
    }
    for k in (1, 2, 3, 4, 5, 7):                              # every stage of w, both parities of the rotations
        out[f"itmax{k}"] = (A, b, cs, dict(itmax=k), qq.TIRED, k, True)
    return out


ENDINGS = ["both", "lq", "primal_first", "dual_first", "itmax1", "itmax2", "itmax3", "itmax4", "itmax5", "itmax7", "b_zero", "timemax",
           "identity", "two_by_two", "diag", "one_by_one", "mach", "cb_zero"]


@pytest.mark.parametrize("ending", ENDINGS)
def test_path2_is_bit_identical_to_path1(K, ctx, ops, ending):
    A, b, c, kw, status, niter, loops = _endings(K, ctx, ops)[ending]
    w1 = _solve(K, ctx, A, b, c, fused=1, **kw)
    w2 = _solve(K, ctx, A, b, c, fused=2, **kw)
    s1, s2 = w1.stats, w2.stats
    print(f"{ending}: niter {s2.niter}, histories {len(s2.residuals_primal)} / {len(s2.residuals_dual)}, {s2.status}")
    assert w1.last_path == 1 and w2.last_path == (2 if loops else 1)
    assert _same_stats(s1, s2) and s1.solved == s2.solved, (s1, s2)
    assert np.array_equal(s1.residuals_primal, s2.residuals_primal, equal_nan=True)
    assert np.array_equal(s1.residuals_dual, s2.residuals_dual, equal_nan=True)
    cst = K.lib().khip_bilqr_stats(w2._h).contents               # khip_stats: the primal history, both sides solved
    assert cst.nres == len(s2.residuals_primal) and bool(cst.solved) == (s2.solved_primal and s2.solved_dual)
    if s2.niter > 0:                                            # (before the first iteration only x and y are defined)
        r1, r2 = _roles(w1), _roles(w2)
        for name in ROLES:
            assert np.array_equal(r1[name], r2[name], equal_nan=True), name
    assert np.array_equal(w1.x.to_host(), w2.x.to_host(), equal_nan=True)
    assert np.array_equal(w1.y.to_host(), w2.y.to_host(), equal_nan=True)
    if status is not None:
        assert s2.status == status, s2.status
    if niter is not None:
        assert s2.niter == niter, s2.niter
    x, y = w2.x.to_host(), w2.y.to_host()
    if ending == "primal_first":
        assert (len(s2.residuals_primal), len(s2.residuals_dual)) == EXPECTED["kron7_sinc"][1:]
    if ending == "dual_first":
        assert (len(s2.residuals_primal), len(s2.residuals_dual)) == EXPECTED["kron8_sinc"][1:]
    if ending == "identity":
        assert not x.any() and not y.any() and not s2.solved_primal and not s2.solved_dual
    if ending == "two_by_two":
        assert np.allclose(x, [0.0, 1.0], rtol=0, atol=1e-15) and np.allclose(y, [0.0, 0.0], rtol=0, atol=1e-15)
        assert np.array_equal(s2.residuals_primal, [1.0, 1.0, np.nan], equal_nan=True)
        assert np.allclose(s2.residuals_dual, [1.0, 1.0, np.sqrt(2.0)], rtol=0, atol=1e-15)
    if ending == "diag":
        assert s2.solved_primal and s2.solved_dual and s2.solved
        assert np.allclose(x, [1.0, 0.5], rtol=0, atol=1e-15) and np.allclose(y, [1.0, 1.0], rtol=0, atol=1e-15)
        # which of the tol and mach tests fire on this 2 x 2 system depends on the last bit of the estimates: any "both" status
        assert s2.status in qq.STATUSES and ("Both" in s2.status or "Found" in s2.status)
        short = K.lib().khip_bilqr_stats(w2._h).contents.status.decode("utf-8")   # the copy in khip_stats is valid UTF-8
        assert len(short.encode()) <= 95 and s2.status.startswith(short)
    if ending == "one_by_one":
        assert abs(x[0] - 1.5) <= 8 * qq.EPS * 1.5 and abs(y[0] - 2.5) <= 8 * qq.EPS * 2.5
    if ending == "timemax":
        assert (len(s2.residuals_primal), len(s2.residuals_dual)) == (2, 2)
    if ending == "mach":
        print(f"rtol = atol = 0: {s2.niter} iterations, {s2.status}")
        # ε = 0: only the mach tests can solve a side; otherwise the loop ends at itmax = 2n or in a breakdown
        assert s2.status in qq.STATUSES and 40 <= s2.niter <= 2 * len(b)
        if s2.solved_primal:
            assert "zero-residual primal" in s2.status
        if s2.solved_dual:
            assert s2.residuals_dual[-1] + 1.0 <= 1.0
    if ending in ("cb_zero", "b_zero"):
        assert not s2.solved and not s2.solved_primal and not s2.solved_dual
        assert (len(s2.residuals_primal), len(s2.residuals_dual)) == (1, 1)


@pytest.mark.parametrize("itmax", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("fused", [0, 1, 2])
def test_roles_hold_the_reference_variables(K, ctx, oracle, ops, itmax, fused):
    """After k iterations every name of khip_bilqr_vector holds what the reference's variable of that name holds at the end of the
    loop, on every path, for every stage of w and both parities of the rotations."""
    A_cpu, A, b, c, kw = _case(ops, "kron7_sinc")
    ws = _solve(K, ctx, A, b, c, fused=fused, itmax=itmax)
    assert ws.last_path == fused and ws.stats.niter == itmax
    pair = reference_pair(oracle, "kron7_sinc", itmax=itmax)
    rtol = _budget(pair)
    (xr, yr, sr), _ = pair
    got = _roles(ws)
    for name in ROLES:
        want = {"x": xr, "y": yr}.get(name)
        want = sr.vectors[name] if want is None else want
        scale = max(np.abs(want).max(), 1e-300)
        dev = np.abs(got[name] - want).max() / scale
        print(f"{name}: largest deviation {dev:.3e} of its largest entry")
        assert dev <= rtol, name
    if itmax == 1:
        assert not got["w_prev2"].any() and not got["w_prev3"].any() and not got["y"].any()
    if itmax == 2:
        assert not got["w_prev3"].any() and got["w_prev2"].any()
    assert len({ws.vector(name).ptr for name in ROLES}) == len(ROLES)


# ---- 3. path 1 against path 0 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["kron7_sinc", "kron8_sinc"])
def test_path1_against_path0(K, ctx, oracle, ops, name):
    """A primal-first and a dual-first case."""
    A_cpu, A, b, c, kw = _case(ops, name)
    x0_, y0_, s0, p0 = _run(K, ctx, A, b, c, fused=0, **kw)
    x1, y1, s1, p1 = _run(K, ctx, A, b, c, fused=1, **kw)
    assert (p0, p1) == (0, 1)
    assert _same_stats(s0, s1)
    rtol = _budget(name, oracle)
    assert _both_hist_ok(s1, s0, _beta1(oracle, name), rtol)
    assert _x_ok(x1, x0_, rtol) and _x_ok(y1, y0_, rtol, "y")


# ---- 4. histories longer than the device window, of different final lengths ------------------------------------------------------
@pytest.mark.parametrize("name", ["kron8_sinc", "poisson16_sinc"])
def test_path2_history_window_drain(K, ctx, ops, name):
    A_cpu, A, b, c, kw = _case(ops, name)
    ctx.set_option("hist_window", 8)
    try:
        x2, y2, s2, p2 = _run(K, ctx, A, b, c, fused=2, **kw)
    finally:
        ctx.set_option("hist_window", 1 << 14)
    x1, y1, s1, p1 = _run(K, ctx, A, b, c, fused=1, **kw)
    assert (p1, p2) == (1, 2)
    assert _same_stats(s1, s2)
    assert (s2.niter, len(s2.residuals_primal), len(s2.residuals_dual)) == EXPECTED[name]
    assert np.array_equal(s1.residuals_primal, s2.residuals_primal) and np.array_equal(s1.residuals_dual, s2.residuals_dual)
    assert np.array_equal(x1, x2) and np.array_equal(y1, y2)


# ---- 5. kernel shapes ----------------------------------------------------------------------------------------------------------
def test_odd_length(K, ctx, oracle, ops):
    """n = 343: the 16-byte kernels' scalar tail element, path 2 against path 0."""
    A_cpu, A, b, c, kw = _case(ops, "kron7_sinc")
    assert A_cpu.n == 343
    x0_, y0_, s0, p0 = _run(K, ctx, A, b, c, fused=0)
    x2, y2, s2, p2 = _run(K, ctx, A, b, c, fused=2)
    assert (p0, p2) == (0, 2)
    assert _same_stats(s0, s2)
    rtol = _budget("kron7_sinc", oracle)
    assert _both_hist_ok(s2, s0, _beta1(oracle, "kron7_sinc"), rtol)
    assert _x_ok(x2, x0_, rtol) and _x_ok(y2, y0_, rtol, "y")


def _carved(K, ctx, n, first):
    """The eleven vectors of a workspace inside one buffer, starting at element `first` with an even stride: first = 1 puts every
    vector at an odd element offset (8-byte but not 16-byte aligned), first = 0 keeps them 16-byte aligned."""
    stride = n + 2 - (n & 1) + 2
    buf = ctx.zeros(first + len(VECTORS) * stride)
    assert buf.ptr % 16 == 0
    vec = {k: buf.slice(first + i * stride, first + i * stride + n) for i, k in enumerate(VECTORS)}
    assert all(v.ptr % 16 == 8 * first for v in vec.values())
    return buf, vec


@pytest.mark.parametrize("name", ["kron8_sinc", "kron7_sinc"])
def test_adopted_vectors_at_odd_offsets(K, ctx, ops, name):
    """The 8-byte kernel path (and, with n = 343, the 16-byte path's tail element beside it): bit-identical to an owned workspace
    and to a 16-byte-aligned adoption, under path 2; nothing is written between the carved vectors."""
    A_cpu, A, b, c, kw = _case(ops, name)
    n = A_cpu.n
    xo, yo, so, po = _run(K, ctx, A, b, c, adopt=False)
    buf1, odd = _carved(K, ctx, n, 1)
    x1, y1, s1, p1 = _run(K, ctx, A, b, c, vectors=odd)
    buf0, even = _carved(K, ctx, n, 0)
    x0_, y0_, s0, p0 = _run(K, ctx, A, b, c, vectors=even)
    assert (po, p1, p0) == (2, 2, 2)
    for x, y, s in ((x1, y1, s1), (x0_, y0_, s0)):
        assert _same_stats(s, so)
        assert np.array_equal(s.residuals_primal, so.residuals_primal) and np.array_equal(s.residuals_dual, so.residuals_dual)
        assert np.array_equal(x, xo) and np.array_equal(y, yo)
    assert np.array_equal(odd["x"].to_host(), xo) and np.array_equal(odd["y"].to_host(), yo)
    stride = n + 2 - (n & 1) + 2
    for first, buf in ((1, buf1), (0, buf0)):
        h = buf.to_host()
        gaps = np.ones(len(h), dtype=bool)
        for i in range(len(VECTORS)):
            gaps[first + i * stride:first + i * stride + n] = False
        assert not h[gaps].any(), "a kernel wrote outside its vectors"


# ---- 6. bindings ---------------------------------------------------------------------------------------------------------------
def test_adopted_workspace_is_bit_identical_to_owned(K, ctx, ops):
    A_cpu, A, b, c, kw = _case(ops, "kron8_sinc")
    n = A_cpu.n
    vec = {k: ctx.empty(n) for k in VECTORS}
    ws = K.BilqrWorkspace(ctx, n, n, vectors=vec)
    K.bilqr_(ws, A, ctx.array(b), ctx.array(c), history=True)
    assert ws.x is vec["x"] and ws.y is vec["y"] and ws.last_path == 2
    xo, yo, so, _ = _run(K, ctx, A, b, c, adopt=False)
    assert np.array_equal(vec["x"].to_host(), xo) and np.array_equal(vec["y"].to_host(), yo)
    assert np.array_equal(ws.stats.residuals_dual, so.residuals_dual) and ws.stats.niter == so.niter
    owned = K.BilqrWorkspace(ctx, n, n, adopt=False)
    assert owned.nbytes == 11 * 8 * n
    owned.warm_start_(ctx.array(b), ctx.array(c))
    assert owned.nbytes == 13 * 8 * n
    assert A._adjoint is not None and K._adjoint_of(A) is A._adjoint     # A' is taken once and kept on the matrix
    x, y, st, ws2 = K.bilqr(A, ctx.array(b), ctx.array(c), history=True)
    assert ws2.last_path == 2                                  # the out-of-place entry forwards the default callback
    assert np.array_equal(x.to_host(), xo) and np.array_equal(y.to_host(), yo)
    assert np.array_equal(st.residuals_primal, so.residuals_primal) and st.status == so.status
    ws3 = K.krylov_workspace("bilqr", A, ctx.array(b))
    assert isinstance(ws3, K.BilqrWorkspace)
    K.krylov_solve_(ws3, A, ctx.array(b), c=ctx.array(c), history=True)
    assert ws3.last_path == 2 and np.array_equal(ws3.x.to_host(), xo) and np.array_equal(ws3.y.to_host(), yo)


def test_argument_errors(K, ctx, ops):
    A_cpu, A = ops("kron", 8)
    n = A_cpu.n
    with pytest.raises(K.KhipError, match="Systems must be square"):
        K.BilqrWorkspace(ctx, n, n + 1, adopt=False)
    ws = K.BilqrWorkspace(ctx, n, n)
    keep = []
    bd = ctx.array(rhs(n))
    opA = K._make_operator(ctx, A, n, keep)
    rc = K.lib().khip_bilqr_solve(ws._h, opA, None, bd.ptr, bd.ptr, None, None)
    assert rc == -1 and "At" in K.lib().khip_last_error().decode()
    rc = K.lib().khip_bilqr_solve(ws._h, opA, K._make_operator(ctx, K._adjoint_of(A), n, keep), bd.ptr, None, None, None)
    assert rc == -1 and "c (the right-hand side of the dual system) is required" in K.lib().khip_last_error().decode()
    with pytest.raises(K.KhipError, match="c .* is required"):
        K.bilqr_(ws, A, bd)
    small = K.BilqrWorkspace(ctx, n - 1, n - 1)
    with pytest.raises(K.KhipError, match="inconsistent with size"):
        K.bilqr_(small, A, ctx.array(rhs(n - 1)), ctx.array(rhs(n - 1)))
    with pytest.raises(K.KhipError, match="Inconsistent problem size"):
        K.bilqr_(ws, A, ctx.array(rhs(n - 1)), bd)
    v = [ctx.empty(n) for _ in range(11)]
    v[10] = v[2]
    with pytest.raises(K.KhipError, match="must be distinct"):
        K.BilqrWorkspace(ctx, n, n, vectors=dict(zip(VECTORS, v)))
    with pytest.raises(K.KhipError, match="x0 and y0"):
        ws.warm_start_(bd)
    assert K.lib().khip_bilqr_warm_start(ws._h, bd.ptr, None) == -1
    assert "x0 and y0 are both required" in K.lib().khip_last_error().decode()


@pytest.mark.parametrize("fused", [0, 1, 2])
def test_warm_start(K, ctx, oracle, ops, fused):
    A_cpu, A, b, c, kw = _case(ops, "kron8_sinc")
    n = A_cpu.n
    x0, y0 = np.linspace(-0.5, 0.5, n), np.linspace(0.3, -0.2, n)
    x, y, st, path = _run(K, ctx, A, b, c, fused=fused, x0=x0, y0=y0)
    assert path == fused
    pair = reference_pair(oracle, "kron8_sinc", x0=x0, y0=y0)
    (xr, yr, sr), (_, _, se) = pair
    assert _same_stats(sr, se) and pair_deviation(pair) <= 1e-6       # the admission condition (measured: 3.5e-9)
    assert _same_stats(st, sr), (st.niter, sr.niter, st.status, sr.status)
    rtol = _budget(pair)
    assert _both_hist_ok(st, sr, sr.beta1, rtol)
    assert _x_ok(x, xr, rtol) and _x_ok(y, yr, rtol, "y")


@pytest.mark.parametrize("fused", [0, 1])
def test_callback_sees_both_histories_and_stops(K, ctx, ops, fused):
    A_cpu, A, b, c, kw = _case(ops, "kron8_sinc")
    seen = []

    def cb(w):
        st = w.stats
        seen.append((len(st.residuals_primal), len(st.residuals_dual)))
        return len(seen) == 3
    x, y, st, path = _run(K, ctx, A, b, c, fused=fused, callback=cb)
    assert path == fused
    assert seen == [(2, 2), (3, 3), (4, 4)]
    assert st.niter == 3 and st.status == "user-requested exit"
    _, _, sr = qq.bilqr(A_cpu.to_scipy(), b, c, itmax=3)
    assert np.all(np.abs(st.residuals_primal - sr.residuals_primal) <= 1e-10 * sr.residuals_primal)
    assert np.all(np.abs(st.residuals_dual - sr.residuals_dual) <= 1e-10 * sr.residuals_dual)


def test_last_path_and_verbose(K, ctx, ops, tmp_path):
    A_cpu, A, b, c, kw = _case(ops, "kron7_sinc")                  # primal-first: rows with ✗ ✗ ✗ ✗ in the primal column
    assert _run(K, ctx, A, b, c)[3] == 2
    assert _run(K, ctx, A, b, c, callback=lambda w: False)[3] == 1
    assert _run(K, ctx, A, b, c, At=lambda x, y: A._adjoint.matvec(x, y))[3] == 1     # a user operator
    assert _run(K, ctx, A, b, c, fused=0)[3] == 0
    log = tmp_path / "bilqr.log"
    with open(log, "w") as f:
        x, y, st, path = _run(K, ctx, A, b, c, verbose=1, iostream=f)
    assert path == 1
    lines = open(log, encoding="utf-8").read().splitlines()
    assert lines[0] == f"BILQR: systems of size {A_cpu.n}"
    assert lines[1] == "%5s  %7s  %7s  %5s" % ("k", "‖rₖ‖", "‖sₖ‖", "timer")
    rows = [ln for ln in lines[2:] if ln.strip()]
    np_, nd = len(st.residuals_primal), len(st.residuals_dual)
    assert (st.niter, np_, nd) == EXPECTED["kron7_sinc"]
    # a row is printed while a side is unsolved AFTER the iteration's tests: k = 0 .. the last iteration but one
    assert [int(r.split()[0]) for r in rows] == list(range(0, st.niter))
    crossed = [r for r in rows if "✗ ✗ ✗ ✗" in r]
    assert len(crossed) == nd - np_                                # from the iteration that solved the primal side on
    assert all(r.split()[1:5] == ["✗", "✗", "✗", "✗"] for r in crossed)


def test_loop_that_never_starts_reports_path_1(K, ctx, ops):
    """cᴴb = 0 is the early return: no iteration runs, and last_path says 1."""
    A_cpu, A = ops("kron", 8)
    n = A_cpu.n
    b = rhs(n)
    c = np.zeros(n)
    c[0], c[1] = b[1], -b[0]
    x, y, st, path = _run(K, ctx, A, b, c)
    assert path == 1 and st.niter == 0 and st.status == qq.BC_BREAKDOWN and not x.any() and not y.any()


# ---- 7. row-partitioned ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_row_partitioned(K, ctx, oracle, ops, world):
    A_cpu, A0, b, c, kw = _case(ops, "kron8_bb")
    n = A_cpu.n
    xref, yref, ref, _ = _run(K, ctx, A0, b, c)
    rtol = _budget("kron8_bb", oracle)
    starts = K.row_partition(n, world)

    def body(cx, rank):
        r0, r1 = starts[rank], starts[rank + 1]
        sl = A_cpu.row_slice(r0, r1)
        A = K.CsrMatrix.from_host(cx, sl.rowptr, sl.col, sl.val, (r1 - r0, n), dist_rows=(r0, r1), n_global=n)
        At = A.transpose()                                  # collective: the same partition
        out = {}
        for fused in (2, 1, 0):
            ws = K.BilqrWorkspace(cx, r1 - r0, r1 - r0)
            K.bilqr_(ws, A, cx.array(b[r0:r1]), cx.array(c[r0:r1]), At=At, fused=fused, history=True)
            st = ws.stats
            out[fused] = (st, ws.last_path, ws.x.to_host(), ws.y.to_host())
        return out

    res = _run_ranks(K, world, 960 + world, body)
    for out in res:
        for fused in (2, 1, 0):
            st, path, _, _ = out[fused]
            assert _same_stats(st, ref) and path == fused
            assert _both_hist_ok(st, ref, _beta1(oracle, "kron8_bb"), rtol)
        for a in ("residuals_primal", "residuals_dual"):
            assert np.array_equal(getattr(out[2][0], a), getattr(out[1][0], a))
            assert np.array_equal(getattr(out[2][0], a), getattr(res[0][2][0], a))
    for fused in (2, 1):
        assert _x_ok(np.concatenate([out[fused][2] for out in res]), xref, rtol)
        assert _x_ok(np.concatenate([out[fused][3] for out in res]), yref, rtol, "y")
    assert all(np.array_equal(out[2][2], out[1][2]) and np.array_equal(out[2][3], out[1][3]) for out in res)


# ---- 8. no device-memory growth --------------------------------------------------------------------------------------------------
def test_no_device_memory_growth(K, ctx, ops):
    A_cpu, A, b, c, kw = _case(ops, "kron8_sinc")
    bd, cd = ctx.array(b), ctx.array(c)
    ws = K.BilqrWorkspace(ctx, A_cpu.n, A_cpu.n, adopt=False)

    def solve(i):
        K.bilqr_(ws, A, bd, cd, fused=(2, 1, 0)[i % 3], history=True)
    for i in range(3):
        solve(i)
    ctx.sync()
    free0 = ctx.mem_info()[0]
    for i in range(20):
        solve(i)
    ctx.sync()
    assert ctx.mem_info()[0] >= free0 - (4 << 20)
