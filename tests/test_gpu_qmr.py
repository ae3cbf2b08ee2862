"""qmr! on the GPU: the three loops against the NumPy restatement of src/qmr.jl (tests/qmr_reference.py) and against each other.

Budgets, those of tests/test_gpu_bilq.py:
  * path 0 (one launch per primitive) against the restatement: same niter and status; the whole residual history within
    _budget(): the two runs differ only in the rounding of the dots (compensated on the device, plain np.dot in NumPy) and of the
    axpys (fma on the device), and the two-sided Lanczos recurrence carries such differences on undamped.  The budget is MEASURED
    per case on the restatement itself: its history with np.dot against its history with exactly summed dots (math.fsum), times 10,
    at least 1e-8, plus 1e-12 beta_1 with beta_1 = sqrt(|c.r_0|) (the restatement reports it as stats.beta1).  Only cases whose
    own deviation is <= 1e-6 are in the list (tests/test_qmr_host.py).
  * path 2 (device-resident) against path 1 (host-driven, same kernels, same scalar code): np.array_equal everywhere: x, the
    history and every role of khip_qmr_vector.
  * path 1 against path 0: elementwise values are the same expressions, the dots differ by <= 1 ulp: the same budget.
"""
import os
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qmr_reference as qr  # noqa: E402
from test_bilq_host import case_operator, case_vectors, rhs  # noqa: E402
from test_qmr_host import CASES, EXPECTED_NITER, SOLVED, reference_pair  # noqa: E402

HIST_RTOL = 1e-8
HIST_FLOOR = 1e-12
TIRED = qr.TIRED
ROLES = ("u_prev", "u", "q", "v_prev", "v", "p", "x", "w_prev2", "w_prev")


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
    return max(HIST_RTOL, 10.0 * qr.history_deviation(s1.residuals, s2.residuals))


def _beta1(oracle, name):
    """β₁ = sqrt(|cᴴr₀|) of a case of the list, from the restatement."""
    return reference_pair(oracle, name)[0][1].beta1


def _hist_ok(a, b, beta1, rtol):
    a, b = np.asarray(a), np.asarray(b)
    with np.errstate(invalid="ignore", divide="ignore"):       # (a zero entry of the reference is judged by the floor below)
        dev = np.nan_to_num(np.abs(a - b) / np.abs(b), nan=0.0, posinf=0.0) if a.shape == b.shape else np.array([np.inf])
    print(f"history: {len(a)} entries, largest relative deviation {dev.max():.3e}, budget {rtol:.3e}")
    return a.shape == b.shape and bool(np.all(np.abs(a - b) <= rtol * np.abs(b) + HIST_FLOOR * beta1))


def _x_ok(x, xr, rtol):
    print(f"x: largest deviation {np.abs(x - xr).max():.3e} of {np.abs(xr).max():.3e}, budget {rtol:.3e}")
    return bool(np.all(np.abs(x - xr) <= max(1e-8, rtol) * np.abs(xr).max()))


def _solve(K, ctx, A, b, c=None, fused=2, x0=None, adopt=None, vectors=None, **kw):
    n = len(b)
    ws = K.QmrWorkspace(ctx, n, n, adopt=adopt, vectors=vectors)
    if x0 is not None:
        ws.warm_start_(ctx.array(x0))
    K.qmr_(ws, A, ctx.array(b), c=None if c is None else ctx.array(c), fused=fused, history=True, **kw)
    return ws


def _run(K, ctx, A, b, **kw):
    ws = _solve(K, ctx, A, b, **kw)
    return ws.x.to_host(), ws.stats, ws.last_path


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


# ---- 1. path 0 against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_path0_against_the_restatement(K, ctx, oracle, ops, name):
    A_cpu, A, b, c, kw = _case(ops, name)
    x, st, path = _run(K, ctx, A, b, c=c, fused=0, **kw)
    assert path == 0
    (xr, sr), _ = reference_pair(oracle, name)
    assert st.niter == sr.niter == EXPECTED_NITER[name] and st.status == sr.status, (st.niter, sr.niter, st.status, sr.status)
    assert len(st.residuals) == st.niter + 1
    assert _hist_ok(st.residuals, sr.residuals, sr.beta1, _budget(name, oracle))
    assert st.solved
    true_res = np.linalg.norm(b - A_cpu.matvec(x))
    print(f"true residual {true_res / np.linalg.norm(b):.3e} ||b||")
    assert true_res <= 1e-6 * np.linalg.norm(b)


# ---- 2. path 2 bit-identical to path 1 -------------------------------------------------------------------------------------------
def _endings(K, ctx, ops):
    A_cpu, A = ops("kron", 8)
    n = A_cpu.n
    b = rhs(n)
    ident = _dense(K, ctx, np.eye(5))
    b5 = np.arange(1.0, 6.0)
    two = _dense(K, ctx, [[0.0, 1.0], [-1.0, 0.0]])
    c_orth = np.zeros(n)
    c_orth[0], c_orth[1] = b[1], -b[0]                       # cᴴb = b₁b₀ - b₀b₁ = 0 exactly
    return {  # ending -> (A, b, c, keywords, status, niter or None, runs the loop)
        "rtol": (A, b, None, {}, SOLVED, 39, True),
        "itmax1": (A, b, None, dict(itmax=1), TIRED, 1, True),          # stage 1; v, u rotated once, w not
        "itmax2": (A, b, None, dict(itmax=2), TIRED, 2, True),          # stage 2; w rotated once
        "itmax3": (A, b, None, dict(itmax=3), TIRED, 3, True),          # stage 3; w rotated twice
        "itmax7": (A, b, None, dict(itmax=7), TIRED, 7, True),
        "b_zero": (A, np.zeros(n), None, {}, "x is a zero-residual solution", 0, False),
        "timemax": (A, b, None, dict(timemax=1e-9), "time limit exceeded", 1, True),
        "identity": (ident, b5, None, {}, SOLVED, 1, True),
        "two_by_two": (two, np.array([1.0, 0.0]), np.array([-1.0, 0.0]), {}, SOLVED, 2, True),      # pᴴq = 0 at the solution
        "mach": (A, b, None, dict(atol=0.0, rtol=0.0), None, None, True),                            # ε = 0: resid_decrease_mach
        "cb_zero": (A, b, c_orth, {}, "Breakdown bᴴc = 0", 0, False),
    }


@pytest.mark.parametrize("ending", ["rtol", "itmax1", "itmax2", "itmax3", "itmax7", "b_zero", "timemax", "identity", "two_by_two",
                                    "mach", "cb_zero"])
def test_path2_is_bit_identical_to_path1(K, ctx, ops, ending):
    A, b, c, kw, status, niter, loops = _endings(K, ctx, ops)[ending]
    w1 = _solve(K, ctx, A, b, c=c, fused=1, **kw)
    w2 = _solve(K, ctx, A, b, c=c, fused=2, **kw)
    s1, s2 = w1.stats, w2.stats
    assert w1.last_path == 1 and w2.last_path == (2 if loops else 1)
    assert s1.niter == s2.niter and s1.status == s2.status and s1.solved == s2.solved and s1.inconsistent == s2.inconsistent
    assert np.array_equal(s1.residuals, s2.residuals) and len(s2.residuals) == s2.niter + 1
    if s2.niter > 0:                                            # (before the first iteration only x is defined)
        r1, r2 = _roles(w1), _roles(w2)
        for name in ROLES:
            assert np.array_equal(r1[name], r2[name], equal_nan=True), name
    assert np.array_equal(w1.x.to_host(), w2.x.to_host())
    if status is not None:
        assert s2.status == status, s2.status
        assert s2.niter == niter, s2.niter
    if ending == "identity":
        assert np.array_equal(w2.x.to_host(), b) and s2.residuals[1] == 0.0
    if ending == "two_by_two":
        assert np.allclose(w2.x.to_host(), [0.0, 1.0], rtol=0, atol=1e-15)
        assert np.allclose(s2.residuals, [1.0, np.sqrt(2.0), 0.0], rtol=0, atol=1e-15)
    if ending == "mach":
        print(f"rtol = atol = 0: {s2.niter} iterations, {s2.status}, last bound {s2.residuals[-1]:.3e}")
        # ε = 0: only resid_decrease_mach can end the loop as solved (the restatement takes 64 iterations to get there)
        assert s2.status == SOLVED and s2.solved and 40 <= s2.niter < 2 * len(b)
        assert s2.residuals[-1] + 1.0 <= 1.0 and s2.residuals[-2] + 1.0 > 1.0
    if ending == "cb_zero":
        assert not s2.solved


@pytest.mark.parametrize("itmax", [1, 2, 3, 4, 7])
@pytest.mark.parametrize("fused", [0, 1, 2])
def test_roles_hold_the_reference_variables(K, ctx, oracle, ops, itmax, fused):
    """After k iterations every name of khip_qmr_vector holds what the reference's variable of that name holds at the end of the
    loop (w_prev = wₖ, w_prev2 = wₖ₋₁ or zeros after one iteration), on every path and for both parities of the rotations."""
    A_cpu, A, b, c, kw = _case(ops, "kron7")
    ws = _solve(K, ctx, A, b, fused=fused, itmax=itmax)
    assert ws.last_path == fused and ws.stats.niter == itmax
    pair = reference_pair(oracle, "kron7", itmax=itmax)
    rtol = _budget(pair)
    (xr, sr), _ = pair
    got = _roles(ws)
    for name in ROLES:
        want = xr if name == "x" else sr.vectors[name]
        scale = max(np.abs(want).max(), 1e-300)
        dev = np.abs(got[name] - want).max() / scale
        print(f"{name}: largest deviation {dev:.3e} of its largest entry")
        assert dev <= rtol, name
    if itmax == 1:
        assert not got["w_prev2"].any()
    assert len({ws.vector(name).ptr for name in ROLES}) == len(ROLES)


# ---- 3. path 1 against path 0 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["kron8", "kron8_sinc", "poisson16", "kron8_rtol12"])
def test_path1_against_path0(K, ctx, oracle, ops, name):
    A_cpu, A, b, c, kw = _case(ops, name)
    x0_, s0, p0 = _run(K, ctx, A, b, c=c, fused=0, **kw)
    x1, s1, p1 = _run(K, ctx, A, b, c=c, fused=1, **kw)
    assert (p0, p1) == (0, 1)
    assert s0.niter == s1.niter and s0.status == s1.status
    rtol = _budget(name, oracle)
    assert _hist_ok(s1.residuals, s0.residuals, _beta1(oracle, name), rtol)
    assert _x_ok(x1, x0_, rtol)


# ---- 4. a history longer than the device window ----------------------------------------------------------------------------------
def test_path2_history_window_drain(K, ctx, ops):
    A_cpu, A, b, c, kw = _case(ops, "kron8_rtol12")
    ctx.set_option("hist_window", 8)
    try:
        x2, s2, p2 = _run(K, ctx, A, b, fused=2, **kw)
    finally:
        ctx.set_option("hist_window", 1 << 14)
    x1, s1, p1 = _run(K, ctx, A, b, fused=1, **kw)
    assert (p1, p2) == (1, 2)
    assert s2.niter == s1.niter == 51 and s2.status == s1.status
    assert len(s2.residuals) == s2.niter + 1 and np.array_equal(s1.residuals, s2.residuals)
    assert np.array_equal(x1, x2)


# ---- 5. kernel shapes: path 2 against path 0 -------------------------------------------------------------------------------------
def test_odd_length(K, ctx, oracle, ops):
    """n = 343: the 16-byte kernels' scalar tail element."""
    A_cpu, A, b, c, kw = _case(ops, "kron7")
    assert A_cpu.n == 343
    x0_, s0, p0 = _run(K, ctx, A, b, fused=0)
    x2, s2, p2 = _run(K, ctx, A, b, fused=2)
    assert (p0, p2) == (0, 2)
    assert s0.niter == s2.niter and s0.status == s2.status
    rtol = _budget("kron7", oracle)
    assert _hist_ok(s2.residuals, s0.residuals, _beta1(oracle, "kron7"), rtol)
    assert _x_ok(x2, x0_, rtol)


def test_two_by_two_breakdown_system(K, ctx):
    """unsymmetric_breakdown (test/test_utils.jl:196-201): x = [0, 1] after two iterations on every path, history [1, √2, 0]."""
    A = _dense(K, ctx, [[0.0, 1.0], [-1.0, 0.0]])
    b, c = np.array([1.0, 0.0]), np.array([-1.0, 0.0])
    xr, sr = qr.qmr(np.array([[0.0, 1.0], [-1.0, 0.0]]), b, c=c)
    _, se = qr.qmr(np.array([[0.0, 1.0], [-1.0, 0.0]]), b, c=c, dot=qr.fsum_dot)
    rtol = _budget(((xr, sr), (None, se)))
    for fused in (0, 1, 2):
        x, st, path = _run(K, ctx, A, b, c=c, fused=fused)
        assert path == fused and st.niter == 2 and st.status == SOLVED and st.solved
        assert np.allclose(x, [0.0, 1.0], rtol=0, atol=1e-15)
        assert _hist_ok(st.residuals, sr.residuals, sr.beta1, rtol)


def test_one_by_one(K, ctx):
    A = _dense(K, ctx, [[2.0]])
    xr, sr = qr.qmr(np.array([[2.0]]), np.array([3.0]))
    for fused in (0, 1, 2):
        x, st, path = _run(K, ctx, A, np.array([3.0]), fused=fused)
        assert path == fused and st.niter == sr.niter == 1 and st.status == sr.status and st.solved
        assert x[0] == 1.5
        assert _hist_ok(st.residuals, sr.residuals, sr.beta1, HIST_RTOL)


def _carved(K, ctx, n, first):
    """The nine vectors of a workspace inside one buffer, starting at element `first` with an even stride: first = 1 puts every
    vector at an odd element offset (8-byte but not 16-byte aligned), first = 0 keeps them 16-byte aligned."""
    stride = n + 2 - (n & 1) + 2
    buf = ctx.zeros(first + 9 * stride)
    assert buf.ptr % 16 == 0
    vec = {k: buf.slice(first + i * stride, first + i * stride + n) for i, k in enumerate(K.QmrWorkspace.VECTORS)}
    assert all(v.ptr % 16 == 8 * first for v in vec.values())
    return buf, vec


@pytest.mark.parametrize("name", ["kron8", "kron7"])
def test_adopted_vectors_at_odd_offsets(K, ctx, ops, name):
    """The 8-byte kernel path (and, with n = 343, the 16-byte path's tail element beside it): bit-identical to an owned workspace
    and to a 16-byte-aligned adoption, under path 2; nothing is written between the carved vectors."""
    A_cpu, A, b, c, kw = _case(ops, name)
    n = A_cpu.n
    xo, so, po = _run(K, ctx, A, b, adopt=False)
    buf1, odd = _carved(K, ctx, n, 1)
    x1, s1, p1 = _run(K, ctx, A, b, vectors=odd)
    buf0, even = _carved(K, ctx, n, 0)
    x0_, s0, p0 = _run(K, ctx, A, b, vectors=even)
    assert (po, p1, p0) == (2, 2, 2)
    for x, s in ((x1, s1), (x0_, s0)):
        assert s.niter == so.niter and s.status == so.status
        assert np.array_equal(s.residuals, so.residuals) and np.array_equal(x, xo)
    assert np.array_equal(odd["x"].to_host(), xo)
    stride = n + 2 - (n & 1) + 2
    for first, buf in ((1, buf1), (0, buf0)):
        h = buf.to_host()
        gaps = np.ones(len(h), dtype=bool)
        for i in range(9):
            gaps[first + i * stride:first + i * stride + n] = False
        assert not h[gaps].any(), "a kernel wrote outside its vectors"


# ---- 6. bindings and preconditioners ---------------------------------------------------------------------------------------------
def test_adopted_workspace_is_bit_identical_to_owned(K, ctx, ops):
    A_cpu, A, b, c, kw = _case(ops, "kron8")
    n = A_cpu.n
    vec = {k: ctx.empty(n) for k in K.QmrWorkspace.VECTORS}
    ws = K.QmrWorkspace(ctx, n, n, vectors=vec)
    K.qmr_(ws, A, ctx.array(b), history=True)
    assert ws.x is vec["x"] and ws.last_path == 2              # solution(ws) is the caller's x
    xo, so, _ = _run(K, ctx, A, b, adopt=False)
    assert np.array_equal(vec["x"].to_host(), xo) and np.array_equal(ws.stats.residuals, so.residuals) and ws.stats.niter == so.niter
    owned = K.QmrWorkspace(ctx, n, n, adopt=False)
    assert owned.nbytes == 9 * 8 * n
    assert A._adjoint is not None and K._adjoint_of(A) is A._adjoint     # A' is taken once and kept on the matrix
    x, st, ws2 = K.qmr(A, ctx.array(b), history=True)
    assert ws2.last_path == 2                                  # the out-of-place entry forwards the default callback
    assert np.array_equal(x.to_host(), xo) and np.array_equal(st.residuals, so.residuals)
    ws3 = K.krylov_workspace("qmr", A, ctx.array(b))
    assert isinstance(ws3, K.QmrWorkspace)
    K.krylov_solve_(ws3, A, ctx.array(b), history=True)
    assert ws3.last_path == 2 and np.array_equal(ws3.x.to_host(), xo)


def test_argument_errors(K, ctx, ops):
    A_cpu, A = ops("kron", 8)
    n = A_cpu.n
    with pytest.raises(K.KhipError, match="square"):
        K.QmrWorkspace(ctx, n, n + 1, adopt=False)
    ws = K.QmrWorkspace(ctx, n, n)
    keep = []
    rc = K.lib().khip_qmr_solve(ws._h, K._make_operator(ctx, A, n, keep), None, None, None, ctx.array(rhs(n)).ptr, None, None, None)
    assert rc == -1 and "At" in K.lib().khip_last_error().decode()
    small = K.QmrWorkspace(ctx, n - 1, n - 1)
    with pytest.raises(K.KhipError, match="inconsistent with size"):
        K.qmr_(small, A, ctx.array(rhs(n - 1)))
    with pytest.raises(K.KhipError, match="Inconsistent problem size"):
        K.qmr_(ws, A, ctx.array(rhs(n - 1)))
    v = [ctx.empty(n) for _ in range(9)]
    v[8] = v[2]
    with pytest.raises(K.KhipError, match="must be distinct"):
        K.QmrWorkspace(ctx, n, n, vectors=dict(zip(K.QmrWorkspace.VECTORS, v)))


def test_preconditioner_without_its_adjoint_is_refused(K, ctx, ops):
    """ILU(0) of a nonsymmetric A (or a callable) is not its own adjoint: without Mt / Nt the solve would run N A' M in place of
    N' A' M' and report convergence on a wrong x, so the binding refuses it before anything is launched; Jacobi stays accepted."""
    A_cpu, A, b, c, kw = _case(ops, "kron8")
    ilu = K.Ilu0(A)
    for key in ("M", "N"):
        with pytest.raises(K.KhipError, match="qmr: . = Ilu0 is not known to be its own adjoint"):
            _run(K, ctx, A, b, **{key: ilu})
        with pytest.raises(K.KhipError, match="own adjoint"):
            _run(K, ctx, A, b, **{key: lambda x, y: K.kcopy_(len(x), y, x)})
    with pytest.raises(K.KhipError, match="own adjoint"):
        K.qmr(A, ctx.array(b), M=ilu)
    ident = lambda x, y: K.kcopy_(len(x), y, x)  # noqa: E731
    x, st, path = _run(K, ctx, A, b, M=ident, Mt=ident)          # an explicit adjoint is taken
    assert path == 1 and st.solved


def test_loop_that_never_starts_reports_path_1(K, ctx, ops):
    """‖r₀‖ <= atol + rtol ‖r₀‖ at set-up: no iteration runs, and last_path says so, as after the early returns."""
    A_cpu, A, b, c, kw = _case(ops, "kron8")
    x, st, path = _run(K, ctx, A, b, rtol=1.0)
    assert path == 1 and st.niter == 0 and st.status == SOLVED and st.solved and not x.any()
    assert len(st.residuals) == 1


@pytest.mark.parametrize("fused", [0, 1, 2])
def test_warm_start(K, ctx, oracle, ops, fused):
    A_cpu, A, b, c, kw = _case(ops, "kron8")
    x0 = np.linspace(-0.5, 0.5, A_cpu.n)
    x, st, path = _run(K, ctx, A, b, fused=fused, x0=x0)
    assert path == fused
    pair = reference_pair(oracle, "kron8", x0=x0)
    (xr, sr), _ = pair
    assert st.niter == sr.niter and st.status == sr.status
    rtol = _budget(pair)
    assert _hist_ok(st.residuals, sr.residuals, sr.beta1, rtol)
    assert _x_ok(x, xr, rtol)


@pytest.mark.parametrize("which", ["M", "N", "MN"])
def test_jacobi_preconditioners(K, ctx, oracle, ops, which):
    """Jacobi M, Jacobi N, both: the host-driven loop (and the primitive sequence) against the restatement with v -> v / d."""
    A_cpu, A, b, c, kw = _case(ops, "kron8")
    d = np.array(A_cpu.to_scipy().diagonal())
    S = A_cpu.to_scipy()
    St = S.T.tocsr()
    jac = lambda v: v / d  # noqa: E731
    ref_kw = {k: jac for k in which}
    sr = qr.qmr(S, b, At=St, **ref_kw)
    se = qr.qmr(S, b, At=St, dot=qr.fsum_dot, **ref_kw)
    rtol = _budget((sr, se))
    xr, sr = sr
    J = K.Jacobi(A)
    for fused, want in ((2, 1), (0, 0)):
        x, st, path = _run(K, ctx, A, b, fused=fused, **{k: J for k in which})
        assert path == want
        assert st.niter == sr.niter and st.status == sr.status
        assert _hist_ok(st.residuals, sr.residuals, sr.beta1, rtol)
        assert _x_ok(x, xr, rtol)
        assert np.linalg.norm(b - A_cpu.matvec(x)) <= 1e-6 * np.linalg.norm(b)


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
    _, sr = qr.qmr(A_cpu.to_scipy(), b, itmax=3)
    assert np.all(np.abs(st.residuals - sr.residuals) <= 1e-10 * sr.residuals)


def test_last_path_and_verbose(K, ctx, ops, tmp_path):
    A_cpu, A, b, c, kw = _case(ops, "kron8")
    assert _run(K, ctx, A, b)[2] == 2
    assert _run(K, ctx, A, b, callback=lambda w: False)[2] == 1
    assert _run(K, ctx, A, b, At=lambda x, y: A._adjoint.matvec(x, y))[2] == 1     # a user operator
    assert _run(K, ctx, A, b, fused=0)[2] == 0
    log = tmp_path / "qmr.log"
    with open(log, "w") as f:
        x, st, path = _run(K, ctx, A, b, verbose=10, iostream=f)
    assert path == 1
    lines = open(log, encoding="utf-8").read().splitlines()
    assert lines[0] == f"QMR: system of size {A_cpu.n}"
    assert lines[1] == "%5s  %8s  %7s  %5s" % ("k", "αₖ", "‖rₖ‖", "timer")
    rows = [ln for ln in lines[2:] if ln.strip()]
    assert [int(r.split()[0]) for r in rows] == list(range(0, st.niter + 1, 10))


# ---- 7. row-partitioned ----------------------------------------------------------------------------------------------------------
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
        At = A.transpose()                                  # collective: the same partition
        out = {}
        for fused in (2, 1, 0):
            ws = K.QmrWorkspace(cx, r1 - r0, r1 - r0)
            K.qmr_(ws, A, cx.array(b[r0:r1]), At=At, fused=fused, history=True)
            st = ws.stats
            out[fused] = (st.niter, st.status, st.residuals, ws.last_path, ws.x.to_host())
        return out

    res = _run_ranks(K, world, 940 + world, body)
    for out in res:
        for fused in (2, 1, 0):
            niter, status, hist, path, _ = out[fused]
            assert niter == ref.niter and status == ref.status and path == fused
            assert _hist_ok(hist, ref.residuals, _beta1(oracle, "kron8"), rtol)
        assert np.array_equal(out[2][2], out[1][2])
        assert np.array_equal(out[2][2], res[0][2][2])
    for fused in (2, 1):
        assert _x_ok(np.concatenate([out[fused][4] for out in res]), xref, rtol)
    assert all(np.array_equal(out[2][4], out[1][4]) for out in res)


# ---- 8. no device-memory growth --------------------------------------------------------------------------------------------------
def test_no_device_memory_growth(K, ctx, ops):
    A_cpu, A, b, c, kw = _case(ops, "kron8")
    bd = ctx.array(b)
    ws = K.QmrWorkspace(ctx, A_cpu.n, A_cpu.n, adopt=False)

    def solve(i):
        K.qmr_(ws, A, bd, fused=(2, 1, 0)[i % 3], history=True)
    for i in range(3):
        solve(i)
    ctx.sync()
    free0 = ctx.mem_info()[0]
    for i in range(20):
        solve(i)
    ctx.sync()
    assert ctx.mem_info()[0] >= free0 - (4 << 20)
