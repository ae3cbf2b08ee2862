"""cg_lanczos_shift! on the GPU: the three loops against the NumPy restatement of src/cg_lanczos_shift.jl
(tests/lanczos_shift_reference.py), against each other and against the true residuals.

Budgets, as for minres! (tests/test_gpu_minres.py):
  * path 0 against the restatement: same niter, status, converged / indefinite and history lengths; the histories within
    _budget(), 10 x the restatement's own sensitivity to the rounding of its dots (np.dot against math.fsum);
  * path 2 against path 1 (same kernels, same scalar code): np.array_equal everywhere;
  * path 1 against path 0: the same elementwise expressions, dots within one ulp: the same kind of budget.
"""
import io
import math
import os
import sys
import tempfile
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lanczos_shift_reference as lr  # noqa: E402

HIST_RTOL = 1e-8
HIST_FLOOR = 1e-12
SQRT_EPS = math.sqrt(np.finfo(float).eps)
SHIFTS = [0.0, 1e-3, 1e-2, 0.1, 1.0, 10.0]


def _fsum_dot(x, y):
    return math.fsum(np.multiply(x, y))


def _budget(plain, exact):
    dev = 0.0
    for a, e in zip(plain, exact):
        k = min(len(a), len(e))
        if k:
            dev = max(dev, float(np.max(np.abs(np.array(a[:k]) - np.array(e[:k])) / np.abs(np.array(e[:k])))))
    return max(HIST_RTOL, 10.0 * dev)


def _hist_ok(a, b, beta1, rtol):
    a, b = np.asarray(a), np.asarray(b)
    return len(a) == len(b) and bool(np.all(np.abs(a - b) <= rtol * np.abs(b) + HIST_FLOOR * beta1))


def _run(K, ctx, A, b, shifts, fused=2, adopt=None, **kw):
    ws = K.CgLanczosShiftWorkspace(ctx, len(b), len(b), len(shifts), adopt=adopt)
    K.cg_lanczos_shift_(ws, A, ctx.array(b), shifts, fused=fused, history=True, **kw)
    return ws


def _state(ws):
    st = ws.stats
    return dict(x=[v.to_host() for v in ws.x], p=[v.to_host() for v in ws.p], st=st, arrays=ws.arrays(), path=ws.last_path)


def _identical(a, b):
    assert a["st"].niter == b["st"].niter and a["st"].status == b["st"].status and a["st"].solved == b["st"].solved
    for i in range(len(a["x"])):
        assert np.array_equal(a["x"][i], b["x"][i]), i
        assert np.array_equal(a["p"][i], b["p"][i]), i
        assert a["st"].residuals[i] == b["st"].residuals[i], i
    for k in a["arrays"]:
        assert np.array_equal(a["arrays"][k], b["arrays"][k]), k


def _poisson(K, ctx, oracle, n1):
    A_cpu = oracle.poisson3d(n1)
    return A_cpu, K.CsrMatrix.from_host(ctx, A_cpu.rowptr, A_cpu.col, A_cpu.val, (A_cpu.n, A_cpu.n))


def _rhs(n):
    return np.cos(0.37 * np.arange(n)) + 0.5


def _check_true_residuals(A_cpu, b, shifts, xs, atol=SQRT_EPS, rtol=SQRT_EPS):
    nb = np.linalg.norm(b)
    for s, x in zip(shifts, xs):
        r = b - A_cpu.matvec(x) - s * x
        assert np.linalg.norm(r) <= 10 * (atol + rtol * nb), (s, np.linalg.norm(r))


# ---- true answers --------------------------------------------------------------------------------------------------------------
def test_true_answers_poisson48(K, ctx, oracle):
    A_cpu = oracle.poisson3d(48)
    A = K.CsrMatrix.stencil(ctx, "poisson", 48)
    b = _rhs(A_cpu.n)
    x, st, ws = K.cg_lanczos_shift(A, ctx.array(b), SHIFTS)
    assert ws.last_path == 2 and st.solved and st.status == "solution good enough given atol and rtol"
    _check_true_residuals(A_cpu, b, SHIFTS, [v.to_host() for v in x])


@pytest.mark.parametrize("product", ["int32", "sell32"])
def test_true_answers_irregular(K, oracle, product):
    c = K.Context(0)
    try:
        if product == "sell32":
            c.set_option("spmv_codes", 0)
            c.set_option("spmv_sell", 3)
        A_cpu = oracle.banded_random(30000, half_band=13, links=3, seed=7)
        A = K.CsrMatrix.from_host(c, A_cpu.rowptr, A_cpu.col, A_cpu.val, (A_cpu.n, A_cpu.n))
        S = A_cpu.to_scipy()
        shifts = [float(abs(S).sum(axis=1).max()) + s for s in (0.0, 1.0, 10.0)]      # SPD by diagonal dominance
        b = _rhs(A_cpu.n)
        x, st, ws = K.cg_lanczos_shift(A, c.array(b), shifts)
        assert ws.last_path == 2 and st.solved
        _check_true_residuals(A_cpu, b, shifts, [v.to_host() for v in x])
    finally:
        c.close()


# ---- the reference's five cases (test/test_cg_lanczos_shift.jl) through the mirror ---------------------------------------------
def _dense(K, ctx, D):
    n = D.shape[0]
    rowptr = np.arange(0, n * n + 1, n, dtype=np.int32)
    col = np.tile(np.arange(n, dtype=np.int32), n)
    return K.CsrMatrix.from_host(ctx, rowptr, col, np.ascontiguousarray(D, dtype=np.float64).ravel(), (n, n))


def test_reference_cases(K, ctx):
    n = 10
    T = np.diag(np.full(n, 4.0)) + np.diag(np.ones(n - 1), 1) + np.diag(np.ones(n - 1), -1)
    b = T @ np.arange(1.0, n + 1)
    A = _dense(K, ctx, T)
    shifts = [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]
    x, st, _ = K.cg_lanczos_shift(A, ctx.array(b), shifts, itmax=n)
    for s, xi in zip(shifts, x):
        assert np.linalg.norm(b - T @ xi.to_host() - s * xi.to_host()) / np.linalg.norm(b) <= 1e-6
    assert st.solved
    _, st, _ = K.cg_lanczos_shift(A, ctx.array(b), [-4.0, -3.0, 2.0], check_curvature=True, itmax=n)
    assert st.indefinite == [True, True, False]
    R = np.random.default_rng(3).random((n, n))
    x, st, _ = K.cg_lanczos_shift(_dense(K, ctx, R), ctx.array(np.zeros(n)), [-4.0, -3.0, 2.0])
    assert all(np.linalg.norm(xi.to_host()) == 0 for xi in x) and st.status == "x is a zero-residual solution"
    D = np.ones((n, n)) + (n - 1) * np.eye(n)
    bp = 10.0 * np.arange(1.0, n + 1)

    def Minv(xv, yv):                                 # M⁻¹ = (1/n) I as an operator
        K.kscalcopy_(n, yv, 1.0 / n, xv)
    x, st, ws = K.cg_lanczos_shift(_dense(K, ctx, D), ctx.array(bp), shifts, M=Minv)
    assert ws.last_path == 1 and st.solved
    for s, xi in zip(shifts, x):
        assert np.linalg.norm(bp - D @ xi.to_host() - s * xi.to_host()) / np.linalg.norm(bp) <= 1e-6
    ws = K.CgLanczosShiftWorkspace(ctx, n, n, len(shifts))

    def cb_n2(w):                                     # TestCallbackN2Shifts, tol = 0.1
        return all(np.linalg.norm(b - T @ xi.to_host() - s * xi.to_host()) <= 0.1 for s, xi in zip(shifts, w.x))
    K.cg_lanczos_shift_(ws, A, ctx.array(b), shifts, atol=0.0, rtol=0.0, callback=cb_n2)
    assert ws.stats.status == "user-requested exit" and cb_n2(ws)


# ---- path 0 against the restatement; paths 2 / 1 / 0 against each other -------------------------------------------------------
CASES = {  # name: (n1, shifts, kwargs)
    "poisson": (24, SHIFTS, {}),
    "spread": (24, [1e3, 1.0, 0.0], {}),                                # converge many iterations apart
    "curvature": (16, [-1.0, -0.05, 0.5, 2.0], dict(check_curvature=True, itmax=60)),
    "indefinite": (16, [-0.05, 0.5], dict(itmax=40)),
    "itmax": (24, SHIFTS, dict(itmax=17)),
}


@pytest.mark.parametrize("case", list(CASES))
def test_path0_against_the_restatement(K, ctx, oracle, case):
    n1, shifts, kw = CASES[case]
    A_cpu, A = _poisson(K, ctx, oracle, n1)
    b = _rhs(A_cpu.n)
    s0 = _state(_run(K, ctx, A, b, shifts, fused=0, **kw))
    assert s0["path"] == 0
    xr, sr, wr = lr.cg_lanczos_shift(A_cpu.matvec, b, shifts, **kw)
    _, se, _ = lr.cg_lanczos_shift(A_cpu.matvec, b, shifts, dot=_fsum_dot, vectors=False, **kw)
    st = s0["st"]
    assert st.niter == sr.niter and st.status == sr.status, (st.niter, sr.niter, st.status, sr.status)
    assert list(s0["arrays"]["converged"]) == list(wr.converged) and st.indefinite == sr.indefinite
    assert [len(h) for h in st.residuals] == [len(h) for h in sr.residuals]
    rtol = _budget(sr.residuals, se.residuals)
    for i in range(len(shifts)):
        assert _hist_ok(st.residuals[i], sr.residuals[i], sr.residuals[i][0], rtol), (i, rtol)
        assert np.allclose(s0["x"][i], xr[i], rtol=1e-6, atol=1e-9 * np.abs(xr[i]).max()), i
    # paths 1 and 2: same kernels, same scalar code
    s1 = _state(_run(K, ctx, A, b, shifts, fused=1, **kw))
    s2 = _state(_run(K, ctx, A, b, shifts, fused=2, **kw))
    assert (s1["path"], s2["path"]) == (1, 2)
    _identical(s1, s2)
    assert s1["st"].niter == st.niter and s1["st"].status == st.status
    for i in range(len(shifts)):
        assert _hist_ok(s1["st"].residuals[i], st.residuals[i], st.residuals[i][0], rtol), i


def test_frozen_shift_equals_the_restatement(K, ctx, oracle):
    A_cpu, A = _poisson(K, ctx, oracle, 24)
    b = _rhs(A_cpu.n)
    shifts = [1e3, 0.0]
    s2 = _state(_run(K, ctx, A, b, shifts))
    xr, sr, _ = lr.cg_lanczos_shift(A_cpu.matvec, b, shifts)
    assert len(s2["st"].residuals[0]) < len(s2["st"].residuals[1]) == s2["st"].niter + 1
    assert len(s2["st"].residuals[0]) == len(sr.residuals[0])
    assert np.allclose(s2["x"][0], xr[0], rtol=1e-12, atol=0)


# ---- shapes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,path", [(1, 2), (64, 2), (65, 1)])
def test_shift_counts(K, ctx, oracle, p, path):
    A_cpu, A = _poisson(K, ctx, oracle, 12)
    b = _rhs(A_cpu.n)
    shifts = list(np.linspace(0.0, 5.0, p))
    ws = _run(K, ctx, A, b, shifts)
    assert ws.last_path == path and ws.stats.solved
    _check_true_residuals(A_cpu, b, shifts, [v.to_host() for v in ws.x])
    if p == 65:
        s1 = _state(ws)
        s1b = _state(_run(K, ctx, A, b, shifts, fused=1))
        _identical(s1, s1b)


def test_duplicated_shifts_are_bit_identical(K, ctx, oracle):
    A_cpu, A = _poisson(K, ctx, oracle, 16)
    s2 = _state(_run(K, ctx, A, _rhs(A_cpu.n), [0.5, 2.0, 0.5, 0.5]))
    assert np.array_equal(s2["x"][0], s2["x"][2]) and np.array_equal(s2["x"][0], s2["x"][3])
    assert s2["st"].residuals[0] == s2["st"].residuals[2]


def test_negative_shifts_with_curvature_on_path2(K, ctx, oracle):
    A_cpu, A = _poisson(K, ctx, oracle, 16)
    b = _rhs(A_cpu.n)
    shifts = [-3.0, -0.2, 1.0]
    ws = _run(K, ctx, A, b, shifts, check_curvature=True)
    _, sr, _ = lr.cg_lanczos_shift(A_cpu.matvec, b, shifts, check_curvature=True, vectors=False)
    assert ws.last_path == 2 and ws.stats.indefinite == sr.indefinite and sr.indefinite[:2] == [True, True]
    assert ws.stats.niter == sr.niter and [len(h) for h in ws.stats.residuals] == [len(h) for h in sr.residuals]


@pytest.mark.parametrize("fused", [2, 1, 0])
def test_zero_rhs(K, ctx, oracle, fused):
    A_cpu, A = _poisson(K, ctx, oracle, 8)
    ws = _run(K, ctx, A, np.zeros(A_cpu.n), [0.0, 1.0], fused=fused)
    st = ws.stats
    assert st.niter == 0 and st.solved and st.status == "x is a zero-residual solution"
    assert st.residuals == [[0.0], [0.0]] and all(not v.to_host().any() for v in ws.x)


def test_history_across_a_drained_window(K, ctx, oracle):
    A_cpu, A = _poisson(K, ctx, oracle, 16)
    b = _rhs(A_cpu.n)
    shifts = [1e2, 1.0, 0.0]
    kw = dict(atol=0.0, rtol=1e-12)
    ctx.set_option("hist_window", 8)
    try:
        s2 = _state(_run(K, ctx, A, b, shifts, **kw))
    finally:
        ctx.set_option("hist_window", 1 << 14)
    s1 = _state(_run(K, ctx, A, b, shifts, fused=1, **kw))
    assert s2["path"] == 2 and s2["st"].niter > 40 and len(s2["st"].residuals[0]) < len(s2["st"].residuals[2])
    _identical(s1, s2)


# ---- operator kinds and preconditioners --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["stencil", "int32", "template", "callback"])
def test_operator_kinds(K, ctx, oracle, kind):
    n1 = 16
    A_cpu = oracle.poisson3d(n1)
    b = _rhs(A_cpu.n)
    if kind == "stencil":
        A = K.CsrMatrix.stencil(ctx, "poisson", n1)
    else:
        A = K.CsrMatrix.from_host(ctx, A_cpu.rowptr, A_cpu.col, A_cpu.val, (A_cpu.n, A_cpu.n))
        if kind == "template":
            assert A.compress() > 0
        if kind == "callback":
            D = A

            def A(xv, yv):
                D.matvec(xv, yv)
    s2 = _state(_run(K, ctx, A, b, SHIFTS))
    assert s2["path"] == (1 if kind == "callback" else 2) and s2["st"].solved
    _check_true_residuals(A_cpu, b, SHIFTS, s2["x"])
    _, sr, _ = lr.cg_lanczos_shift(A_cpu.matvec, b, SHIFTS, vectors=False)
    assert s2["st"].niter == sr.niter


@pytest.mark.parametrize("prec", ["jacobi", "ic0"])
def test_preconditioners(K, ctx, oracle, prec):
    A_cpu, A = _poisson(K, ctx, oracle, 16)
    n = A_cpu.n
    b = _rhs(n)
    shifts = [0.0, 0.1, 1.0]
    if prec == "jacobi":
        M = K.Jacobi(A)
        d = np.array(A_cpu.to_scipy().diagonal())
        Mh = lambda v: v / d                                          # noqa: E731
    else:
        M = K.Ilu0(A)

        def Mh(v):                                    # the device factor applied on the host: the same operator
            dv, dy = ctx.array(v), ctx.empty(n)
            M(dv, dy)
            return dy.to_host()
    s0 = _state(_run(K, ctx, A, b, shifts, fused=0, M=M))
    s1 = _state(_run(K, ctx, A, b, shifts, fused=1, M=M))
    s2 = _state(_run(K, ctx, A, b, shifts, fused=2, M=M))
    assert (s0["path"], s1["path"], s2["path"]) == (0, 1, 1)
    _identical(s1, s2)
    xr, sr, _ = lr.cg_lanczos_shift(A_cpu.matvec, b, shifts, M=Mh)
    _, se, _ = lr.cg_lanczos_shift(A_cpu.matvec, b, shifts, M=Mh, dot=_fsum_dot, vectors=False)
    rtol = _budget(sr.residuals, se.residuals)
    for s in (s0, s1):
        assert s["st"].niter == sr.niter and s["st"].status == sr.status
        for i in range(len(shifts)):
            assert _hist_ok(s["st"].residuals[i], sr.residuals[i], sr.residuals[i][0], rtol), (i, rtol)
    if prec == "jacobi":
        # the shift enters as s_i ‖v‖² (:214-218): the iterates solve (A + s_i I) x_i = b where M is a multiple of I -- as Jacobi
        # is on this operator (constant diagonal) -- and not for IC(0), where only the agreement with the restatement holds
        _check_true_residuals(A_cpu, b, shifts, s1["x"])


# ---- callback, verbose, adoption -----------------------------------------------------------------------------------------------
def test_callback_sees_current_iterates_and_stops(K, ctx, oracle):
    A_cpu, A = _poisson(K, ctx, oracle, 16)
    b = _rhs(A_cpu.n)
    seen = []

    def cb(w):
        st = w.stats
        xs = [v.to_host() for v in w.x]
        seen.append((st.niter, [len(h) for h in st.residuals], np.linalg.norm(b - A_cpu.matvec(xs[1]) - 1.0 * xs[1])))
        return seen[-1][2] <= 1e-3 * np.linalg.norm(b)
    ws = _run(K, ctx, A, b, [0.0, 1.0], callback=cb)
    assert ws.last_path == 1 and ws.stats.status == "user-requested exit"
    k = ws.stats.niter
    assert len(seen) == k and seen[-1][2] <= 1e-3 * np.linalg.norm(b) and seen[-2][2] > 1e-3 * np.linalg.norm(b)
    assert [s[1] for s in seen] == [[j + 2, j + 2] for j in range(k)]    # the history so far, as the reference's callbacks read it


def test_verbose_layout(K, ctx, oracle):
    A_cpu, A = _poisson(K, ctx, oracle, 8)
    b = _rhs(A_cpu.n)
    shifts = [0.0, 1.0]
    with tempfile.TemporaryFile("w+") as f:
        ws = _run(K, ctx, A, b, shifts, verbose=2, iostream=f)
        f.flush()
        f.seek(0)
        got = f.read()
    ref = io.StringIO()
    lr.cg_lanczos_shift(A_cpu.matvec, b, shifts, verbose=2, iostream=ref)
    assert ws.last_path == 1

    def strip(t):                                     # timings differ
        return [ln.rsplit("  ", 1)[0] if ln.endswith("s") else ln for ln in t.split("\n")]
    assert strip(got) == strip(ref.getvalue()), (got, ref.getvalue())


def test_adopted_workspace_is_bit_identical_to_owned(K, ctx, oracle):
    A_cpu, A = _poisson(K, ctx, oracle, 16)
    b = _rhs(A_cpu.n)
    _identical(_state(_run(K, ctx, A, b, SHIFTS, adopt=True)), _state(_run(K, ctx, A, b, SHIFTS, adopt=False)))


def test_adoption_refusals(K, ctx, oracle):
    import ctypes as C
    A_cpu, A = _poisson(K, ctx, oracle, 8)
    n = A_cpu.n
    L = K.lib()
    vs = [ctx.empty(n) for _ in range(7)]
    h = C.c_void_p()
    xs = (C.c_void_p * 2)(vs[3].ptr, vs[4].ptr)
    ps = (C.c_void_p * 2)(vs[5].ptr, vs[3].ptr)                            # p[2] is x[1]
    assert L.khip_cg_lanczos_shift_workspace_adopt(ctx._h, n, n, 2, vs[0].ptr, vs[1].ptr, vs[2].ptr, C.cast(xs, K.c_void_pp),
                                                   C.cast(ps, K.c_void_pp), C.byref(h)) != 0
    assert "distinct" in L.khip_last_error().decode()
    ws = K.CgLanczosShiftWorkspace(ctx, n, n, 2)
    with pytest.raises(K.KhipError, match="already is the workspace's 'x"):
        ws._adopt_vector("v", ws.x[1])
    with pytest.raises(K.KhipError, match="inconsistent with length"):
        K.cg_lanczos_shift_(ws, A, ctx.array(np.ones(n)), [1.0, 2.0, 3.0])
    with pytest.raises(K.KhipError, match="Inconsistent problem size"):
        K.cg_lanczos_shift_(ws, A, ctx.array(np.ones(n + 1)), [1.0, 2.0])
    ws2 = K.CgLanczosShiftWorkspace(ctx, n + 1, n + 1, 2)
    with pytest.raises(K.KhipError, match="is inconsistent with size"):
        K.cg_lanczos_shift_(ws2, A, ctx.array(np.ones(n + 1)), [1.0, 2.0])


# ---- row-partitioned handles -------------------------------------------------------------------------------------------------
def _run_ranks(K, world, hub_id, body):
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


@pytest.mark.parametrize("world", [2, 3])
def test_row_partitioned(K, ctx, oracle, world):
    n1 = 16
    A_cpu, A0 = _poisson(K, ctx, oracle, n1)
    n = A_cpu.n
    b = _rhs(n)
    shifts = [0.0, 0.5, 5.0]
    ref = _run(K, ctx, A0, b, shifts).stats
    _, sr, _ = lr.cg_lanczos_shift(A_cpu.matvec, b, shifts, vectors=False)
    _, se, _ = lr.cg_lanczos_shift(A_cpu.matvec, b, shifts, dot=_fsum_dot, vectors=False)
    rtol = _budget(sr.residuals, se.residuals)
    starts = K.row_partition(n, world)

    def body(c, rank):
        r0, r1 = starts[rank], starts[rank + 1]
        A = K.CsrMatrix.stencil(c, "poisson", n1, rows=(r0, r1), distributed=True)
        out = {}
        for fused in (2, 1, 0):
            ws = K.CgLanczosShiftWorkspace(c, r1 - r0, r1 - r0, len(shifts))
            K.cg_lanczos_shift_(ws, A, c.array(b[r0:r1]), shifts, fused=fused, history=True)
            out[fused] = (ws.stats.niter, ws.stats.status, ws.stats.residuals, ws.last_path, [v.to_host() for v in ws.x])
        return out

    res = _run_ranks(K, world, 760 + world, body)
    for out in res:
        for fused in (2, 1, 0):
            niter, status, hist, path, _ = out[fused]
            assert niter == ref.niter and status == ref.status and path == fused
            for i in range(len(shifts)):
                assert _hist_ok(hist[i], ref.residuals[i], ref.residuals[i][0], rtol), (fused, i)
        assert out[2][2] == out[1][2]
        for i in range(len(shifts)):
            assert np.array_equal(out[2][4][i], out[1][4][i])
    xs = [np.concatenate([res[r][2][4][i] for r in range(world)]) for i in range(len(shifts))]
    _check_true_residuals(A_cpu, b, shifts, xs)


# ---- a larger size ---------------------------------------------------------------------------------------------------------------
def test_256_cubed_eight_shifts(K, ctx, oracle):
    n1 = 256
    A_cpu = oracle.poisson3d(n1)
    A = K.CsrMatrix.stencil(ctx, "poisson", n1)
    b = np.ones(A_cpu.n)
    shifts = [0.0, 1e-3, 1e-2, 0.03, 0.1, 0.3, 1.0, 3.0]
    ws = _run(K, ctx, A, b, shifts, itmax=50, atol=0.0, rtol=0.0)
    st = ws.stats
    assert ws.last_path == 2 and st.niter == 50 and st.status == "maximum number of iterations exceeded"
    _, sr, _ = lr.cg_lanczos_shift(A_cpu.matvec, b, shifts, itmax=50, atol=0.0, rtol=0.0, vectors=False)
    for i in range(len(shifts)):
        assert _hist_ok(st.residuals[i], sr.residuals[i], sr.residuals[i][0], 1e-6), i
    x = ws.x[0].to_host()
    r = b - A_cpu.matvec(x)
    assert abs(np.linalg.norm(r) - st.residuals[0][-1]) <= 1e-6 * np.linalg.norm(b)
