"""minres! on the GPU: the three loops against the NumPy restatement of src/minres.jl (tests/minres_reference.py) and against
each other.

Budgets:
  * path 0 (one launch per primitive) against the restatement: same niter and status; the first 20 residual estimates within
    1e-12 relative; the whole history within _budget(): the two runs differ only in the rounding of the dots (compensated on
    the device, plain np.dot in NumPy), and once the Lanczos vectors lose orthogonality the recurrence carries such
    differences on undamped -- strongly so for indefinite operators.  The budget is MEASURED per case on the restatement
    itself: its history with np.dot against its history with exactly summed dots (math.fsum), times 10, plus 1e-12 beta_1.
  * path 2 (device-resident) against path 1 (host-driven, same kernels, same scalar code): np.array_equal everywhere.
  * path 1 against path 0: elementwise values are the same expressions, the dots differ by <= 1 ulp: the same kind of budget.
"""
import math
import os
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import minres_reference as mr  # noqa: E402

EPS = np.finfo(float).eps
HIST_RTOL = 1e-8
HIST_FLOOR = 1e-12


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


def _hist_ok(a, b, beta1, rtol=HIST_RTOL):
    n = min(len(a), len(b))
    return bool(np.all(np.abs(a[:n] - b[:n]) <= rtol * np.abs(b[:n]) + HIST_FLOOR * beta1))


def _fsum_dot(x, y):
    return math.fsum(np.multiply(x, y))


def _budget(plain, exact):
    """10 x the restatement's own sensitivity to the rounding of its dots (at least HIST_RTOL)."""
    n = min(len(plain), len(exact))
    dev = float(np.max(np.abs(plain[:n] - exact[:n]) / np.abs(exact[:n])))
    return max(HIST_RTOL, 10.0 * dev)


def _run(K, ctx, A, b, fused=2, window=5, x0=None, adopt=None, **kw):
    ws = K.MinresWorkspace(ctx, len(b), len(b), window=window, adopt=adopt)
    if x0 is not None:
        ws.warm_start_(ctx.array(x0))
    K.minres_(ws, A, ctx.array(b), fused=fused, history=True, **kw)
    st = ws.stats
    return ws.x.to_host(), st, ws.last_path


def _operator(K, ctx, oracle, kind, n1):
    if kind in ("poisson", "shifted"):
        A_cpu = oracle.poisson3d(n1)
    else:
        A_cpu = oracle.banded_random(n1 ** 3, half_band=13, links=3, seed=7)
    A = K.CsrMatrix.from_host(ctx, A_cpu.rowptr, A_cpu.col, A_cpu.val, (A_cpu.n, A_cpu.n))
    return A_cpu, A


CASES = [  # kind, n1, lam, warm, jacobi, itmax
    ("poisson", 32, 0.0, False, False, 0),
    ("poisson", 64, 0.0, False, False, 0),
    ("shifted", 32, -1.0, False, False, 300),
    ("banded", 24, 0.0, False, False, 300),
    ("poisson", 32, 0.75, False, False, 0),
    ("poisson", 32, 0.0, True, False, 0),
    ("poisson", 32, 0.0, False, True, 0),
]


@pytest.mark.parametrize("kind,n1,lam,warm,jacobi,itmax", CASES)
def test_path0_against_the_restatement(K, ctx, oracle, kind, n1, lam, warm, jacobi, itmax):
    A_cpu, A = _operator(K, ctx, oracle, kind, n1)
    n = A_cpu.n
    b = np.cos(0.37 * np.arange(n)) + 0.5
    x0 = np.linspace(-0.5, 0.5, n) if warm else None
    kw = dict(λ=lam, itmax=itmax)
    ref_kw = dict(lam=lam, itmax=itmax)
    if jacobi:
        d = np.array(A_cpu.to_scipy().diagonal())
        kw["M"] = K.Jacobi(A)
        ref_kw["M"] = lambda v: v / d
    x, st, path = _run(K, ctx, A, b, fused=0, x0=x0, **kw)
    assert path == 0
    xr, sr = mr.minres(A_cpu.matvec, b, x0=x0, **ref_kw)
    assert st.niter == sr.niter and st.status == sr.status, (st.niter, sr.niter, st.status, sr.status)
    k = min(20, len(sr.residuals))
    assert np.all(np.abs(st.residuals[:k] - sr.residuals[:k]) <= 1e-12 * sr.residuals[:k])
    beta1 = sr.residuals[0]
    _, se = mr.minres(A_cpu.matvec, b, x0=x0, dot=_fsum_dot, **ref_kw)
    rtol = _budget(sr.residuals, se.residuals)
    assert _hist_ok(st.residuals, sr.residuals, beta1, rtol), rtol
    assert _hist_ok(st.Aresiduals, sr.Aresiduals, sr.Aresiduals.max(), max(rtol, _budget(sr.Aresiduals[1:], se.Aresiduals[1:])))
    assert len(st.residuals) == len(st.Aresiduals) == len(st.Acond) == st.niter + 1
    # the final true residual is consistent with the last reported one (MINRES's estimate of ||b - (A + lam I) x||)
    true_res = np.linalg.norm(b - (A_cpu.matvec(x) + lam * x))
    if jacobi:   # the estimate is the M^-1 norm of the residual
        r = b - A_cpu.matvec(x)
        true_res = math.sqrt(float(np.dot(r, r / d)))
    assert abs(true_res - st.residuals[-1]) <= 1e-6 * beta1 + 1e-3 * st.residuals[-1], (true_res, st.residuals[-1])


def _endings(K, ctx, oracle):
    A_cpu, A = _operator(K, ctx, oracle, "poisson", 16)
    n = A_cpu.n
    b = np.cos(0.37 * np.arange(n)) + 0.5
    i = np.arange(16) + 1
    s = np.sin(np.pi * i / 17)
    eig = np.einsum("i,j,k->ijk", s, s, s).ravel()           # an eigenvector of the Dirichlet Laplacian
    return A, {
        "rtol": (b, dict()),
        "itmax": (b, dict(itmax=7)),
        "etol": (b, dict(window=2, etol=1e-2)),
        "conlim": (b, dict(conlim=3.0, atol=0.0, rtol=0.0, etol=0.0)),   # no tolerance test fires first
        "b_zero": (np.zeros(n), dict()),
        "eigenvector": (eig, dict()),
        "timemax": (b, dict(timemax=1e-9)),
    }


# product options of a context: "plain" = no sliced copy (the staged kernel; the Lanczos step P1 is a pass of its own);
# "sell8" / "sell32" = the sliced SpMV on the 8-bit-coded / int32 sliced copy, which carries P1 as an epilogue of the product
# (the session context of tests/conftest.py codes small operators too: it takes "sell8")
PRODUCTS = {"plain": {"spmv_codes": 0, "spmv_sell": 0}, "sell8": {"spmv_codes": 2}, "sell32": {"spmv_codes": 0, "spmv_sell": 3}}


@pytest.fixture(scope="module", params=list(PRODUCTS))
def pctx(K, request):
    c = K.Context(0)
    for k, v in PRODUCTS[request.param].items():
        c.set_option(k, v)
    yield request.param, c
    c.close()


@pytest.mark.parametrize("ending", ["rtol", "itmax", "etol", "conlim", "b_zero", "eigenvector", "timemax"])
def test_path2_is_bit_identical_to_path1(K, pctx, oracle, ending):
    product, ctx = pctx
    A, table = _endings(K, ctx, oracle)
    b, kw = table[ending]
    window = kw.pop("window", 5)
    x1, s1, p1 = _run(K, ctx, A, b, fused=1, window=window, **kw)
    x2, s2, p2 = _run(K, ctx, A, b, fused=2, window=window, **kw)
    assert p1 == 1 and (p2 == 2 or ending == "b_zero")
    assert s1.niter == s2.niter and s1.status == s2.status and s1.solved == s2.solved and s1.inconsistent == s2.inconsistent
    for f in ("residuals", "Aresiduals", "Acond"):
        assert np.array_equal(getattr(s1, f), getattr(s2, f)), f
    assert np.array_equal(x1, x2)
    expect = {"itmax": "maximum number of iterations exceeded", "etol": "truncated forward error small enough",
              "conlim": "condition number exceeds tolerance", "b_zero": "x is a zero-residual solution",
              "eigenvector": "x is a minimum least-squares solution", "timemax": "time limit exceeded"}
    if ending in expect:
        assert s2.status == expect[ending], s2.status
    if ending in ("eigenvector", "timemax"):
        assert s2.niter == 1


def test_path2_history_window_drain(K, ctx, oracle):
    """A history longer than the device window (ctx option hist_window): the three histories are drained in pieces and stay
    identical to the host-driven loop's, and so does x."""
    A_cpu, A = _operator(K, ctx, oracle, "poisson", 16)
    b = np.cos(0.37 * np.arange(A_cpu.n)) + 0.5
    kw = dict(atol=0.0, rtol=1e-12, etol=0.0)         # no forward-error exit: > 40 iterations
    ctx.set_option("hist_window", 8)
    try:
        x2, s2, p2 = _run(K, ctx, A, b, fused=2, **kw)
    finally:
        ctx.set_option("hist_window", 1 << 14)
    x1, s1, p1 = _run(K, ctx, A, b, fused=1, **kw)
    assert (p1, p2) == (1, 2)
    assert s2.niter == s1.niter > 40 and s2.status == s1.status
    for f in ("residuals", "Aresiduals", "Acond"):
        assert len(getattr(s2, f)) == s2.niter + 1 and np.array_equal(getattr(s1, f), getattr(s2, f)), f
    assert np.array_equal(x1, x2)


def test_fused_product(K, pctx, oracle):
    """The Lanczos step rides on the product exactly where the sliced kernel runs; its elementwise values are those of path 0's
    primitives (the residual estimates agree to the dots' rounding), and a warm start and Jacobi M take the same product."""
    product, ctx = pctx
    A_cpu, A = _operator(K, ctx, oracle, "poisson", 16)
    n = A_cpu.n
    b = np.cos(0.37 * np.arange(n)) + 0.5
    ws = K.MinresWorkspace(ctx, n, n)
    K.minres_(ws, A, ctx.array(b), λ=-0.3, history=True, itmax=60)
    assert ws.last_path == 2 and ws.fused_product == (product != "plain")
    s2 = ws.stats
    x0_, s0, p0 = _run(K, ctx, A, b, fused=0, λ=-0.3, itmax=60)
    assert s0.niter == s2.niter and s0.status == s2.status
    assert np.all(np.abs(s2.residuals[:20] - s0.residuals[:20]) <= 1e-12 * s0.residuals[:20])
    _, sp_ = mr.minres(A_cpu.matvec, b, lam=-0.3, itmax=60)
    _, se = mr.minres(A_cpu.matvec, b, lam=-0.3, itmax=60, dot=_fsum_dot)
    assert _hist_ok(s2.residuals, s0.residuals, s0.residuals[0], _budget(sp_.residuals, se.residuals))
    ws = K.MinresWorkspace(ctx, n, n)
    ws.warm_start_(ctx.array(np.linspace(-0.5, 0.5, n)))
    K.minres_(ws, A, ctx.array(b), M=K.Jacobi(A), history=True)
    assert ws.last_path == 1 and ws.fused_product == (product != "plain") and ws.stats.solved


@pytest.mark.parametrize("fused", [0, 1])
def test_callback_sees_the_history_and_stops(K, ctx, oracle, fused):
    """callback(workspace) runs after every iteration with stats.residuals published (k + 1 entries after iteration k);
    returning true ends the solve with "user-requested exit" (src/minres.jl:446, :467)."""
    A_cpu, A = _operator(K, ctx, oracle, "poisson", 16)
    b = np.cos(0.37 * np.arange(A_cpu.n)) + 0.5
    seen = []

    def cb(w):
        seen.append(len(w.stats.residuals))
        return len(seen) == 3
    x, st, path = _run(K, ctx, A, b, fused=fused, callback=cb)
    assert path == fused
    assert seen == [2, 3, 4]
    assert st.niter == 3 and st.status == "user-requested exit" and len(st.residuals) == 4
    _, sr = mr.minres(A_cpu.matvec, b, itmax=3)
    assert np.all(np.abs(st.residuals - sr.residuals) <= 1e-12 * sr.residuals)


def test_path1_against_path0(K, ctx, oracle):
    A_cpu, A = _operator(K, ctx, oracle, "shifted", 32)
    b = np.cos(0.37 * np.arange(A_cpu.n)) + 0.5
    x0_, s0, _ = _run(K, ctx, A, b, fused=0, λ=-1.0, itmax=200)
    x1, s1, _ = _run(K, ctx, A, b, fused=1, λ=-1.0, itmax=200)
    assert s0.niter == s1.niter and s0.status == s1.status
    _, sp_ = mr.minres(A_cpu.matvec, b, lam=-1.0, itmax=200)
    _, se = mr.minres(A_cpu.matvec, b, lam=-1.0, itmax=200, dot=_fsum_dot)
    rtol = _budget(sp_.residuals, se.residuals)
    assert _hist_ok(s1.residuals, s0.residuals, s0.residuals[0], rtol), rtol
    assert np.allclose(x1, x0_, rtol=0, atol=max(1e-8, rtol) * np.abs(x0_).max())


def test_last_path(K, ctx, oracle):
    A_cpu, A = _operator(K, ctx, oracle, "poisson", 8)
    b = np.ones(A_cpu.n)
    assert _run(K, ctx, A, b)[2] == 2
    ws = K.minres(A, ctx.array(b))[2]
    assert ws.last_path == 2                                  # the out-of-place entry forwards the default callback
    assert _run(K, ctx, A, b, M=K.Jacobi(A))[2] == 1
    assert _run(K, ctx, A, b, callback=lambda w: False)[2] == 1
    assert _run(K, ctx, A, b, verbose=1)[2] == 1
    assert _run(K, ctx, A, b, fused=0)[2] == 0


def test_adopted_workspace_is_bit_identical_to_owned(K, ctx, oracle):
    A_cpu, A = _operator(K, ctx, oracle, "poisson", 24)
    b = np.cos(0.37 * np.arange(A_cpu.n))
    xa, sa, _ = _run(K, ctx, A, b, adopt=True)
    xo, so, _ = _run(K, ctx, A, b, adopt=False)
    assert np.array_equal(xa, xo) and np.array_equal(sa.residuals, so.residuals) and sa.niter == so.niter
    ws = K.MinresWorkspace(ctx, A_cpu.n, A_cpu.n, adopt=False)
    assert ws.nbytes == 6 * 8 * A_cpu.n


def test_linesearch_is_refused(K, ctx, oracle):
    A_cpu, A = _operator(K, ctx, oracle, "poisson", 8)
    with pytest.raises(K.KhipError, match="linesearch"):
        _run(K, ctx, A, np.ones(A_cpu.n), linesearch=True)


@pytest.mark.parametrize("world,codes", [(2, 1), (3, 1), (2, 2)])
def test_row_partitioned(K, ctx, oracle, world, codes):
    n1 = 16
    A_cpu = oracle.poisson3d(n1)
    n = A_cpu.n
    b = np.cos(0.37 * np.arange(n)) + 0.5
    A0 = K.CsrMatrix.from_host(ctx, A_cpu.rowptr, A_cpu.col, A_cpu.val, (n, n))
    _, ref, _ = _run(K, ctx, A0, b, λ=-0.5, itmax=120)
    _, sp_ = mr.minres(A_cpu.matvec, b, lam=-0.5, itmax=120)
    _, se = mr.minres(A_cpu.matvec, b, lam=-0.5, itmax=120, dot=_fsum_dot)
    rtol = _budget(sp_.residuals, se.residuals)
    starts = K.row_partition(n, world)

    def body(c, rank):
        r0, r1 = starts[rank], starts[rank + 1]
        c.set_option("spmv_codes", codes)                   # 2: the sliced kernel with the Lanczos epilogue on every rank
        A = K.CsrMatrix.stencil(c, "poisson", n1, rows=(r0, r1), distributed=True)
        out = {}
        for fused in (2, 1, 0):
            ws = K.MinresWorkspace(c, r1 - r0, r1 - r0)
            K.minres_(ws, A, c.array(b[r0:r1]), fused=fused, history=True, λ=-0.5, itmax=120)
            st = ws.stats
            out[fused] = (st.niter, st.status, st.residuals, ws.last_path)
            out[f"fp{fused}"] = ws.fused_product
        return out

    res = _run_ranks(K, world, 700 + world, body)
    for out in res:
        for fused in (2, 1, 0):
            niter, status, hist, path = out[fused]
            assert niter == ref.niter and status == ref.status and path == fused
            assert _hist_ok(hist, ref.residuals, ref.residuals[0], rtol), rtol
        assert np.array_equal(out[2][2], out[1][2])
        assert np.array_equal(out[2][2], res[0][2][2])
        assert out["fp2"] == out["fp1"] == (codes == 2) and not out["fp0"]


def test_512_cubed_forty_iterations(K, ctx):
    n1 = 512
    A = K.CsrMatrix.stencil(ctx, "poisson", n1)
    n = n1 ** 3
    b = ctx.empty(n)
    K.kfill_(b, 1.0)
    hist = {}
    for fused in (2, 0):
        ws = K.MinresWorkspace(ctx, n, n)
        K.minres_(ws, A, b, fused=fused, history=True, itmax=40, atol=0.0, rtol=0.0)   # (b = ones passes test2 <= atol + rtol beta_1 at once)
        st = ws.stats
        hist[fused] = st.residuals
        assert ws.fused_product == (fused == 2)            # at this size the default product is the sliced kernel
        assert st.niter == 40 and st.status == "maximum number of iterations exceeded"
        if fused == 2:
            r = A.matvec(ws.x)
            K.kaxpby_(n, 1.0, b, -1.0, r)
            true_res = K.knorm(n, r)
        del ws
    assert _hist_ok(hist[2], hist[0], hist[0][0])
    assert abs(true_res - hist[2][-1]) <= 1e-6 * hist[2][-1]


def test_no_device_memory_growth(K, ctx, oracle):
    A_cpu, A = _operator(K, ctx, oracle, "poisson", 32)
    b = ctx.array(np.ones(A_cpu.n))

    def cycle():
        for fused in (2, 1, 0):
            ws = K.MinresWorkspace(ctx, A_cpu.n, A_cpu.n, adopt=False)
            K.minres_(ws, A, b, fused=fused, history=True)
            del ws
    cycle()
    ctx.sync()
    free0 = ctx.mem_info()[0]
    for _ in range(5):
        cycle()
    ctx.sync()
    assert ctx.mem_info()[0] >= free0 - (4 << 20)
