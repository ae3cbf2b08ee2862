"""minres_qlp! on the GPU: the three loops against the NumPy restatement of src/minres_qlp.jl (tests/minres_qlp_reference.py) and
against each other.

Budgets:
  * path 0 (one launch per primitive) against the restatement: same niter, status, solved and inconsistent; x and the histories of
    the case that qualify (tests/test_minres_qlp_host.py, PARITY) within case_budget(): the two runs differ only in the rounding of
    the dots (compensated on the device, plain np.dot in NumPy) and of the axpys (fma on the device).  The budget is MEASURED per
    case on the restatement itself: its histories and x with np.dot against those with exactly summed dots (math.fsum), times 10,
    at least 1e-8, plus a floor of 1e-12 × the history's first entry.  A history is in a case's list when that deviation, measured
    relative to no less than 1e-9 × the first entry, is <= 1e-6; niter, status, flags and x are checked on every case.
  * path 1 against path 0: elementwise values are the same expressions, the dots differ by <= 1 ulp: the same budget.
  * path 2 (device-resident) against path 1 (host-driven, same kernels, same scalar code): np.array_equal(equal_nan=True) everywhere:
    x, the three histories and every name of khip_minres_qlp_vector, on EVERY case.
The C client path is not covered here: tests/test_gpu_entry_points.py builds its clients from a list inside that file.
"""
import os
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import minres_qlp_reference as mr  # noqa: E402
from test_bilq_host import rhs  # noqa: E402
from test_minres_qlp_host import (CASES, CORE, EXPECTED_NITER, EXPECTED_STATUS, HIST_FLOOR, HISTORIES, INCONSISTENT,  # noqa: E402
                                  PARITY, SINGULAR, case_budget, case_matrix, case_rhs, history_floor, null_vector, pair_budget,
                                  reference_pair)

LAZY = ("dx", "vk")
KW = {"lam": "λ"}                                        # the restatement's ASCII keywords -> the mirror's


def _run_ranks(K, world, hub_id, body):
    """In-process ranks on one device, one thread each (the pattern of tests/test_gpu_symmlq.py)."""
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


def _hist_ok(a, b, rtol, floor, what="history"):
    """|a - b| <= rtol |b| + floor entry by entry, NaN exactly where b has NaN."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        print(f"{what}: shapes {a.shape} {b.shape} or the places of NaN differ")
        return False
    m = ~np.isnan(b)
    a, b = a[m], b[m]
    with np.errstate(invalid="ignore", divide="ignore"):
        dev = np.nan_to_num(np.abs(a - b) / np.abs(b), nan=0.0, posinf=0.0) if len(b) else np.zeros(1)
    print(f"{what}: {len(a)} finite entries, largest relative deviation {dev.max():.3e}, budget {rtol:.3e} + {floor:.3e}")
    return bool(np.all(np.abs(a - b) <= rtol * np.abs(b) + floor))


def _x_ok(x, xr, rtol, what="x"):
    if not np.array_equal(np.isnan(x), np.isnan(xr)):
        return False
    m = ~np.isnan(xr)
    if not m.any():
        return True
    print(f"{what}: largest deviation {np.abs(x[m] - xr[m]).max():.3e} of {np.abs(xr[m]).max():.3e}, budget {rtol:.3e}")
    return bool(np.all(np.abs(x[m] - xr[m]) <= rtol * np.abs(xr[m]).max()))


def _solve(K, ctx, A, b, fused=2, x0=None, adopt=None, vectors=None, history=True, **kw):
    n = len(b)
    ws = K.MinresQlpWorkspace(ctx, n, n, adopt=adopt, vectors=vectors)
    if x0 is not None:
        ws.warm_start_(ctx.array(x0))
    K.minres_qlp_(ws, A, ctx.array(b), fused=fused, history=history, **{KW.get(k, k): v for k, v in kw.items()})
    return ws


def _vectors(ws):
    return {name: ws.vector(name).to_host() for name in CORE}


def _same_bits(w1, w2):
    """last_path is the caller's to assert first; then the stats, the three histories, x and every named vector."""
    s1, s2 = w1.stats, w2.stats
    assert (s1.niter, s1.status, s1.solved, s1.inconsistent) == (s2.niter, s2.status, s2.solved, s2.inconsistent)
    for k in HISTORIES:
        assert np.array_equal(getattr(s1, k), getattr(s2, k), equal_nan=True), k
    assert np.array_equal(w1.x.to_host(), w2.x.to_host(), equal_nan=True)
    if s1.niter == 0 and s1.status == mr.ZERO_RESIDUAL:   # the early return (:193-201) comes before the work vectors are set up (:212-219)
        return
    v1, v2 = _vectors(w1), _vectors(w2)
    for name in CORE:
        if name == "p":                                   # scratch: the next product overwrites it
            continue
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
    kind, size, which, kw = CASES[name]
    S, A = ops(kind, size)
    return S, A, case_rhs(S, which), dict(kw)


def _stats_against(st, sr_, rtol, keys):
    assert (st.niter, st.status, st.solved, st.inconsistent) == (sr_.niter, sr_.status, sr_.solved, sr_.inconsistent), \
        (st.niter, sr_.niter, st.status, sr_.status)
    assert len(st.residuals) == len(st.Acond) == st.niter + 1 and len(st.Aresiduals) == st.niter
    for k in keys:
        assert _hist_ok(getattr(st, k), getattr(sr_, k), rtol, history_floor(sr_, k), k), k


def _against(ws, pair, rtol, keys=HISTORIES, names=()):
    """A solve against the restatement: the stats, the histories `keys`, x and the named vectors within the budget."""
    (xr, sr_), _ = pair
    _stats_against(ws.stats, sr_, rtol, keys)
    assert _x_ok(ws.x.to_host(), xr, rtol)
    for name in names:
        assert _x_ok(ws.vector(name).to_host(), sr_.vectors[name], rtol, name), name


# ---- 1. path 0 against the restatement, path 1 against path 0 --------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_path0_against_the_restatement(K, ctx, oracle, ops, name):
    S, A, b, kw = _case(ops, name)
    ws = _solve(K, ctx, A, b, fused=0, **kw)
    assert ws.last_path == 0
    st = ws.stats
    print(f"{name}: {st.niter} iterations, {st.status}")
    assert st.niter == EXPECTED_NITER[name] and st.status == EXPECTED_STATUS[name] and st.inconsistent == (name in INCONSISTENT)
    _against(ws, reference_pair(oracle, name), case_budget(oracle, name), PARITY[name])


@pytest.mark.parametrize("name", list(CASES))
def test_path1_against_path0(K, ctx, oracle, ops, name):
    S, A, b, kw = _case(ops, name)
    w0 = _solve(K, ctx, A, b, fused=0, **kw)
    w1 = _solve(K, ctx, A, b, fused=1, **kw)
    assert (w0.last_path, w1.last_path) == (0, 1)
    rtol = case_budget(oracle, name)
    _stats_against(w1.stats, w0.stats, rtol, PARITY[name])
    assert _x_ok(w1.x.to_host(), w0.x.to_host(), rtol)


# ---- 2. path 2 bit-identical to path 1 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_path2_is_bit_identical_to_path1(K, ctx, ops, name):
    """Every case: n = 1, 2, 3, 4, 10, 63, 64, 65, odd n = 729 (the tail element, three workgroups), the indefinite and the singular
    ones, the breakdowns."""
    S, A, b, kw = _case(ops, name)
    w1 = _solve(K, ctx, A, b, fused=1, **kw)
    w2 = _solve(K, ctx, A, b, fused=2, **kw)
    assert w1.last_path == 1 and w2.last_path == (1 if name == "zero_rhs" else 2)      # an early return reports no device loop
    assert w1.fused_product == w2.fused_product
    _same_bits(w1, w2)
    st = w2.stats
    print(f"{name}: {st.niter} iterations (restatement {EXPECTED_NITER[name]}), {st.status}, fused product {w2.fused_product}")
    assert st.niter == EXPECTED_NITER[name] and st.status == EXPECTED_STATUS[name]
    assert len(st.residuals) == len(st.Acond) == st.niter + 1 and len(st.Aresiduals) == st.niter


# ---- 3. the product with and without the Lanczos step ----------------------------------------------------------------------------
# context options as in tests/test_gpu_minres.py: "plain" = no sliced copy (the step is a pass of its own), "sell8" / "sell32" = the
# sliced SpMV on the 8-bit-coded / int32 sliced copy, which carries the step as an epilogue of the product
PRODUCTS = {"plain": {"spmv_codes": 0, "spmv_sell": 0}, "sell8": {"spmv_codes": 2}, "sell32": {"spmv_codes": 0, "spmv_sell": 3}}


@pytest.mark.parametrize("name", ["poisson9_lam", "poisson8_singular"])
def test_fused_product_both_ways(K, oracle, name):
    """fused_product is 1 exactly where the plan carries the epilogue.  The elementwise expressions are the same either way and α
    comes from a different reduction (the product's fused dot or the pass's), so the runs agree within the case's budget; each is
    bit-identical between paths 1 and 2."""
    kind, size, which, kw = CASES[name]
    S = case_matrix(oracle, kind, size)
    b = case_rhs(S, which)
    rtol = case_budget(oracle, name)
    runs = {}
    for product, options in PRODUCTS.items():
        c = K.Context(0)
        try:
            for k, v in options.items():
                c.set_option(k, v)
            A = _device(K, c, S)
            w2 = _solve(K, c, A, b, fused=2, **kw)
            w1 = _solve(K, c, A, b, fused=1, **kw)
            w0 = _solve(K, c, A, b, fused=0, **kw)
            assert (w2.last_path, w1.last_path, w0.last_path) == (2, 1, 0)
            assert w2.fused_product == w1.fused_product == (product != "plain"), product
            assert not w0.fused_product
            _same_bits(w1, w2)
            runs[product] = (w2.stats, w2.x.to_host())
        finally:
            c.close()
    for product in ("sell8", "sell32"):
        _stats_against(runs[product][0], runs["plain"][0], rtol, PARITY[name])
        assert _x_ok(runs[product][1], runs["plain"][1], rtol)
    _stats_against(runs["plain"][0], reference_pair(oracle, name)[0][1], rtol, PARITY[name])


# ---- 4. what the answers mean ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["poisson8", "poisson9", "poisson8_lam", "poisson9_lam", "poisson8_tight", "sym_indef10_lam2",
                                  "neumann64_cons"])
def test_true_residual_where_solved(K, ctx, ops, name):
    """‖b − (A + λI) x‖ is residuals[end] (to 1e-8 ‖b‖: the estimate and the recurrence's rounding), under path 2: with λ ≠ 0 it is
    the SHIFTED system that is solved."""
    S, A, b, kw = _case(ops, name)
    ws = _solve(K, ctx, A, b, **kw)
    assert ws.last_path == 2 and ws.stats.solved and not ws.stats.inconsistent
    x = ws.x.to_host()
    lam = kw.get("lam", 0.0)
    true = np.linalg.norm(b - S @ x - lam * x)
    print(f"{name}: ||b - (A + λI) x|| {true:.6e}, residuals[end] {ws.stats.residuals[-1]:.6e}")
    assert abs(true - ws.stats.residuals[-1]) <= 1e-8 * np.linalg.norm(b)


@pytest.mark.parametrize("fused", [0, 1, 2])
@pytest.mark.parametrize("name,m", list(zip(SINGULAR, (8, 9))))
def test_singular_poisson_gives_the_minimum_length_solution(K, ctx, ops, name, m, fused):
    S, A, b, kw = _case(ops, name)
    ws = _solve(K, ctx, A, b, fused=fused, **kw)
    st = ws.stats
    assert ws.last_path == fused
    assert st.inconsistent and not st.solved and st.status == mr.INCONSISTENT
    x = ws.x.to_host()
    lam = kw["lam"]
    r = b - S @ x - lam * x
    Ar, Ab = S @ r + lam * r, S @ b + lam * b
    u = null_vector(m)
    cos = abs(x @ u) / (np.linalg.norm(x) * np.linalg.norm(u))
    print(f"{name}, path {fused}: ||(A+λI) r|| {np.linalg.norm(Ar):.3e} of ||(A+λI) b|| {np.linalg.norm(Ab):.3e}; x.u {cos:.3e}")
    assert np.linalg.norm(Ar) <= 1e-6 * np.linalg.norm(Ab)                 # the reference's acceptance condition
    assert cos <= 1e-12                                                     # orthogonal to the null vector: the minimum-length one


@pytest.mark.parametrize("fused", [0, 1, 2])
@pytest.mark.parametrize("n", [63, 64, 65])
def test_neumann_inconsistent_ends_by_breakdown(K, ctx, ops, n, fused):
    S, A, b, kw = _case(ops, f"neumann{n}_inc")
    ws = _solve(K, ctx, A, b, fused=fused)
    st = ws.stats
    assert ws.last_path == fused and st.inconsistent and not st.solved
    x = ws.x.to_host()
    r = b - S @ x
    print(f"neumann{n}_inc, path {fused}: Σx {x.sum():.3e} of {np.abs(x).sum():.3e}, ||A r|| {np.linalg.norm(S @ r):.3e}")
    assert abs(x.sum()) <= 1e-6 * np.abs(x).sum()
    assert np.linalg.norm(S @ r) <= 1e-6 * np.linalg.norm(S @ b)


# ---- 5. endings and the roles after them -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("itmax", [1, 2, 3, 4])
def test_itmax_and_the_roles(K, ctx, oracle, ops, itmax):
    """itmax = 1 ... 4: after the stop wₖ₋₁, wₖ, M⁻¹vₖ₋₁ and M⁻¹vₖ are the reference's variables on every path (the roles were
    rotated itmax times, swapped itmax − 1 times, and M⁻¹vₖ got its last kscal!), and path 2 equals path 1 in every bit."""
    S, A, b, kw = _case(ops, "poisson9_lam")
    w = {f: _solve(K, ctx, A, b, fused=f, itmax=itmax, **kw) for f in (0, 1, 2)}
    assert [w[f].last_path for f in (0, 1, 2)] == [0, 1, 2]
    _same_bits(w[1], w[2])
    pair = reference_pair(oracle, "poisson9_lam", itmax=itmax)
    rtol = pair_budget(pair)
    for f in (0, 1, 2):
        st = w[f].stats
        assert st.niter == itmax and st.status == mr.TIRED and not st.solved
        _against(w[f], pair, rtol, names=("wkm1", "wk", "Mvkm1", "Mvk"))
        assert abs(np.linalg.norm(w[f].vector("Mvk").to_host()) - 1.0) <= 1e-12        # vₖ₊₁ is normalised


@pytest.mark.parametrize("fused", [0, 1, 2])
def test_zero_right_hand_side(K, ctx, ops, fused):
    S, A = ops("poisson", 8)
    ws = _solve(K, ctx, A, np.zeros(512), fused=fused)
    st = ws.stats
    assert ws.last_path == min(fused, 1)
    assert st.niter == 0 and st.solved and not st.inconsistent and st.status == mr.ZERO_RESIDUAL and not ws.x.to_host().any()
    assert list(st.residuals) == [0.0] and list(st.Acond) == [0.0] and len(st.Aresiduals) == 0


def test_loop_that_never_starts_reports_path_1(K, ctx, ops):
    S, A, b, kw = _case(ops, "poisson8")
    ws = _solve(K, ctx, A, b, rtol=1.0)
    st = ws.stats
    assert ws.last_path == 1 and st.niter == 0 and st.status == mr.SOLVED and st.solved and not ws.x.to_host().any()


@pytest.mark.parametrize("fused", [0, 1, 2])
def test_symmetric_breakdown(K, ctx, oracle, ops, fused):
    """[0 1; 1 0], b = e₁ (test/test_utils.jl:188-192): β₃ ≤ btol ends the loop without the division; x = [0, 1]."""
    S, A, b, kw = _case(ops, "breakdown")
    ws = _solve(K, ctx, A, b, fused=fused)
    st = ws.stats
    assert ws.last_path == fused
    assert st.niter == 2 and st.solved and not st.inconsistent and st.status == mr.SOLVED
    assert np.allclose(ws.x.to_host(), [0.0, 1.0], rtol=0, atol=1e-15)
    assert not np.isnan(ws.vector("Mvk").to_host()).any()                    # no 0 / 0: the division was skipped


@pytest.mark.parametrize("lam", [0.0, -0.5])
def test_warm_start(K, ctx, oracle, ops, lam):
    """x0 with and without λ (:168-172, :527): every path against the restatement, path 2 = path 1."""
    S, A, b, kw = _case(ops, "poisson8")
    x0 = np.linspace(-0.5, 0.5, 512)
    pair = reference_pair(oracle, "poisson8", x0=x0, lam=lam)
    rtol = pair_budget(pair)
    assert rtol <= 10 * 1e-6                                     # the warm-started runs qualify for history parity
    w = {f: _solve(K, ctx, A, b, fused=f, x0=x0, lam=lam) for f in (0, 1, 2)}
    assert [w[f].last_path for f in (0, 1, 2)] == [0, 1, 2]
    for f in (0, 1, 2):
        _against(w[f], pair, rtol)
    _same_bits(w[1], w[2])
    assert w[2].vector("dx") is not None
    x = w[2].x.to_host()
    assert np.linalg.norm(b - S @ x - lam * x) <= 1e-6 * np.linalg.norm(b)


@pytest.mark.parametrize("fused", [0, 1, 2])
def test_without_history(K, ctx, ops, fused):
    S, A, b, kw = _case(ops, "poisson8")
    wh = _solve(K, ctx, A, b, fused=fused)
    wn = _solve(K, ctx, A, b, fused=fused, history=False)
    sn = wn.stats
    assert wn.last_path == fused
    assert len(sn.residuals) == len(sn.Aresiduals) == len(sn.Acond) == 0
    assert sn.niter == wh.stats.niter and sn.status == wh.stats.status and np.array_equal(wn.x.to_host(), wh.x.to_host())


def test_history_window_drain(K, ctx, ops):
    S, A, b, kw = _case(ops, "poisson8_singular")
    ctx.set_option("hist_window", 8)
    try:
        w2 = _solve(K, ctx, A, b, fused=2, **kw)
    finally:
        ctx.set_option("hist_window", 1 << 14)
    w1 = _solve(K, ctx, A, b, fused=1, **kw)
    assert (w1.last_path, w2.last_path) == (1, 2)
    assert w2.stats.niter > 8 and len(w2.stats.residuals) == len(w2.stats.Acond) == w2.stats.niter + 1
    _same_bits(w1, w2)


def test_time_limit_already_used_up(K, ctx, ops):
    S, A, b, kw = _case(ops, "poisson8")
    for fused in (0, 1, 2):
        ws = _solve(K, ctx, A, b, fused=fused, timemax=1e-9)
        st = ws.stats
        assert ws.last_path == fused and st.niter == 1 and st.status == mr.OVERTIMED and not st.solved


def test_nontemporal_and_plain_accumulation_instantiations(K, ctx, oracle, ops):
    """nt_min_elems = 1: the NT instantiations of the passes run, bit-equal to the default's.  compensated = 0: the COMP = false
    instantiations; path 2 equals its own path 1 bit for bit and stays within the case's budget of the compensated run."""
    S, A, b, kw = _case(ops, "poisson9_lam")
    wd = _solve(K, ctx, A, b, **kw)
    keep = ctx.get_option("nt_min_elems")
    assert keep > S.shape[0]
    ctx.set_option("nt_min_elems", 1)
    try:
        w2 = _solve(K, ctx, A, b, **kw)
        w1 = _solve(K, ctx, A, b, fused=1, **kw)
    finally:
        ctx.set_option("nt_min_elems", keep)
    assert (wd.last_path, w2.last_path, w1.last_path) == (2, 2, 1)
    _same_bits(w2, wd)
    _same_bits(w1, wd)
    keep = ctx.get_option("compensated")
    ctx.set_option("compensated", 0)
    try:
        p2 = _solve(K, ctx, A, b, **kw)
        p1 = _solve(K, ctx, A, b, fused=1, **kw)
    finally:
        ctx.set_option("compensated", keep)
    assert (p2.last_path, p1.last_path) == (2, 1)
    _same_bits(p1, p2)
    rtol = case_budget(oracle, "poisson9_lam")
    _stats_against(p2.stats, wd.stats, rtol, HISTORIES)
    assert _x_ok(p2.x.to_host(), wd.x.to_host(), rtol)


# ---- 6. path selection: M, a user operator, a callback, verbose ------------------------------------------------------------------
def test_jacobi_preconditioner(K, ctx, oracle, ops):
    """Jacobi M on the Neumann operator shifted to be definite has a diagonal that is not constant: the host-driven loop and the
    primitive sequence against the restatement with v -> v / d; vk appears only with M."""
    S, A, b, kw = _case(ops, "neumann65_cons")
    lam = 0.75
    d = np.array(S.diagonal())
    jac = lambda v: v / d  # noqa: E731
    pair = (mr.minres_qlp(S, b, M=jac, lam=lam), mr.minres_qlp(S, b, M=jac, lam=lam, dot=mr.fsum_dot))
    rtol = pair_budget(pair)
    assert rtol <= 10 * 1e-6 and pair[0][1].solved
    J = K.Jacobi(A)
    for fused, want in ((2, 1), (0, 0)):
        ws = _solve(K, ctx, A, b, fused=fused, M=J, lam=lam)
        assert ws.last_path == want and ws.vector("vk") is not None and not ws.fused_product
        _against(ws, pair, rtol)
    assert _solve(K, ctx, A, b, lam=lam).vector("vk") is None


def test_preconditioner_not_positive_definite(K, ctx, ops):
    S, A, b, kw = _case(ops, "poisson8")
    for fused in (2, 0):
        ws = K.MinresQlpWorkspace(ctx, 512, 512)
        with pytest.raises(K.KhipError, match="Preconditioner is not positive definite"):
            K.minres_qlp_(ws, A, ctx.array(b), M=lambda x, y: K.kscalcopy_(512, y, -1.0, x), fused=fused)


@pytest.mark.parametrize("fused", [0, 1, 2])
def test_callback_stops_at_iteration_3(K, ctx, oracle, ops, fused):
    """The callback runs on path 1 (or 0) and finds the named vectors in the reference's state of that point: wₖ₋₁, wₖ, M⁻¹vₖ₋₁ and
    M⁻¹vₖ (normalised: the division is not carried forward with a callback) against the restatement's at the same call."""
    S, A, b, kw = _case(ops, "poisson9_lam")
    seen, got, want = [], {}, {}

    def cb(w):
        seen.append(len(w.stats.residuals))
        if len(seen) == 3:
            got.update({k: w.vector(k).to_host() for k in ("wkm1", "wk", "Mvkm1", "Mvk")}, x=w.x.to_host())
        return len(seen) == 3

    def cb_ref(w):
        if w.stats.niter == 3:
            want.update({k: np.array(v) for k, v in w.stats.vectors.items()}, x=np.array(w.x))
        return w.stats.niter == 3
    ws = _solve(K, ctx, A, b, fused=fused, callback=cb, **kw)
    st = ws.stats
    assert ws.last_path == min(fused, 1)
    assert seen == [2, 3, 4]
    assert st.niter == 3 and st.status == mr.USER_EXIT and len(st.residuals) == len(st.Acond) == 4 and len(st.Aresiduals) == 3
    xr, sr_ = mr.minres_qlp(S, b, callback=cb_ref, **kw)
    assert sr_.status == mr.USER_EXIT
    for k in ("wkm1", "wk", "Mvkm1", "Mvk", "x"):
        assert _x_ok(got[k], want[k], 1e-8, k), k
    assert _hist_ok(st.residuals, sr_.residuals, 1e-8, HIST_FLOOR * sr_.residuals[0])
    assert _x_ok(ws.x.to_host(), xr, 1e-8)


def test_last_path_and_verbose(K, ctx, ops, tmp_path):
    S, A, b, kw = _case(ops, "poisson8")
    assert _solve(K, ctx, A, b).last_path == 2
    assert _solve(K, ctx, A, b, callback=lambda w: False).last_path == 1
    wu = _solve(K, ctx, lambda x, y: A.matvec(x, y), b)                            # a user operator
    assert wu.last_path == 1 and not wu.fused_product
    assert _solve(K, ctx, A, b, fused=0).last_path == 0
    ref = _solve(K, ctx, A, b)
    assert wu.stats.niter == ref.stats.niter and _x_ok(wu.x.to_host(), ref.x.to_host(), 1e-8)
    log = tmp_path / "minres_qlp.log"
    with open(log, "w") as f:
        ws = _solve(K, ctx, A, b, verbose=5, iostream=f)
    assert ws.last_path == 1
    lines = open(log, encoding="utf-8").read().splitlines()
    assert lines[0] == "MINRES-QLP: system of size 512"
    assert lines[1] == "%5s  %7s  %7s  %7s  %7s  %8s  %7s  %7s  %8s  %5s" % ("k", "‖rₖ‖", "‖Arₖ₋₁‖", "βₖ₊₁", "Rₖ.ₖ", "Lₖ.ₖ", "‖A‖", "κ(A)",
                                                                           "backward", "timer")
    rows = [ln for ln in lines[2:] if ln.strip()]
    assert [int(r.split()[0]) for r in rows] == list(range(0, ws.stats.niter + 1, 5))
    assert rows[0].count("✗ ✗ ✗ ✗") == 4 and all(r.endswith("s") for r in rows)
    assert all(len(r.split()) == 10 for r in rows[1:])
    assert np.array_equal(ws.x.to_host(), ref.x.to_host())                        # path 1 = path 2


# ---- 7. bindings ---------------------------------------------------------------------------------------------------------------------
def test_out_of_place_entry_generic_interface_adopt_and_reuse(K, ctx, ops):
    """K.minres_qlp(A, b), as the README spells it, forwards the default callback and still runs the device-resident loop; 6n
    doubles; an adopted workspace gives the bits of a created one and solution === x; one workspace serves two solves of two
    different systems: the stats and the roles are reset."""
    S, A, b, kw = _case(ops, "poisson8")
    n = 512
    wo = _solve(K, ctx, A, b, adopt=False)
    assert wo.last_path == 2 and wo.nbytes == 6 * 8 * n
    x, st, ws = K.minres_qlp(A, ctx.array(b), history=True)
    assert ws.last_path == 2
    assert np.array_equal(x.to_host(), wo.x.to_host()) and np.array_equal(st.residuals, wo.stats.residuals)
    assert np.array_equal(st.Aresiduals, wo.stats.Aresiduals) and np.array_equal(st.Acond, wo.stats.Acond)
    ws3 = K.krylov_workspace("minres_qlp", A, ctx.array(b))
    assert isinstance(ws3, K.MinresQlpWorkspace)
    K.krylov_solve_(ws3, A, ctx.array(b), history=True)
    assert ws3.last_path == 2 and np.array_equal(ws3.x.to_host(), wo.x.to_host())
    vec = {k: ctx.empty(n) for k in K.MinresQlpWorkspace.VECTORS}
    wa = K.MinresQlpWorkspace(ctx, n, n, vectors=vec)
    K.minres_qlp_(wa, A, ctx.array(b), history=True)
    assert wa.x is vec["x"] and wa.nbytes == 6 * 8 * n
    _same_bits(wa, wo)
    bs = case_rhs(S, "sin")
    lam = CASES["poisson8_singular"][3]["lam"]
    K.minres_qlp_(wa, A, ctx.array(bs), history=True, λ=lam)                       # a second, different solve on the rotated roles
    fresh = _solve(K, ctx, A, bs, lam=lam)
    assert wa.last_path == 2 and wa.stats.inconsistent and wa.stats.niter == EXPECTED_NITER["poisson8_singular"]
    _same_bits(wa, fresh)
    K.minres_qlp_(wa, A, ctx.array(b), history=True)                              # and back: inconsistent is reset
    assert not wa.stats.inconsistent and wa.stats.solved
    _same_bits(wa, wo)
    assert sorted(wa.vector(k).ptr for k in CORE) == sorted(vec[k].ptr for k in CORE)


def test_argument_errors(K, ctx, ops):
    S, A = ops("poisson", 8)
    n = 512
    small = K.MinresQlpWorkspace(ctx, n - 1, n - 1)
    with pytest.raises(K.KhipError, match="inconsistent with size"):
        K.minres_qlp_(small, A, ctx.array(rhs(n - 1)))
    ws = K.MinresQlpWorkspace(ctx, n, n)
    with pytest.raises(K.KhipError, match="Inconsistent problem size"):
        K.minres_qlp_(ws, A, ctx.array(rhs(n - 1)))
    with pytest.raises(K.KhipError, match="minres_qlp: options.variant must be 0"):
        K.minres_qlp_(ws, A, ctx.array(rhs(n)), variant=1)
    with pytest.raises(K.KhipError, match="linesearch") as e:
        K.minres_qlp_(ws, A, ctx.array(rhs(n)), linesearch=True)
    assert e.value.code == -3                                                     # KHIP_ERR_UNSUPPORTED
    rect = K.MinresQlpWorkspace(ctx, n, n + 1, adopt=False)
    with pytest.raises(K.KhipError, match="System must be square"):
        K.minres_qlp_(rect, lambda x, y: None, ctx.array(rhs(n + 1)))
    K.minres_qlp_(ws, A, ctx.array(rhs(n)))                                       # the workspace still serves a solve
    assert ws.stats.solved and ws.last_path == 2


def test_workspace_table(K, ctx):
    import ctypes as C
    L = K.lib()
    N5 = 5
    vec = {k: ctx.empty(N5) for k in CORE + LAZY}
    h = C.c_void_p()
    assert L.khip_minres_qlp_workspace_adopt(ctx._h, N5, N5, *[vec[k].ptr for k in CORE], C.byref(h)) == 0
    for k in CORE:
        assert L.khip_minres_qlp_vector(h, k.encode()) == vec[k].ptr, k
    for k in LAZY + ("nope", ""):
        assert L.khip_minres_qlp_vector(h, k.encode()) is None, k
    assert L.khip_minres_qlp_workspace_bytes(h) == len(CORE) * 8 * N5
    assert L.khip_minres_qlp_solution(h) == vec["x"].ptr and L.khip_minres_qlp_last_path(h) == -1
    for i, k in enumerate(LAZY):
        assert L.khip_minres_qlp_workspace_adopt_vector(h, k.encode(), vec[k].ptr) == 0, k
        assert L.khip_minres_qlp_workspace_bytes(h) == (len(CORE) + i + 1) * 8 * N5
    assert L.khip_minres_qlp_workspace_adopt_vector(h, b"wk", ctx.empty(N5).ptr) == -1
    assert L.khip_last_error() == f"minres_qlp_workspace_adopt_vector: unknown vector 'wk' ({', '.join(LAZY)})".encode()
    assert L.khip_minres_qlp_workspace_destroy(h) == 0
    ptrs = [vec[k].ptr for k in CORE]
    ptrs[0] = ptrs[1]
    assert L.khip_minres_qlp_workspace_adopt(ctx._h, N5, N5, *ptrs, C.byref(h)) == -1
    assert L.khip_last_error() == b"minres_qlp_workspace_adopt: x, wkm1, wk, Mvkm1, Mvk, p must be distinct"
    assert L.khip_minres_qlp_workspace_destroy(None) == 0 and L.khip_minres_qlp_workspace_bytes(None) == 0
    assert L.khip_minres_qlp_vector(None, b"x") is None and L.khip_minres_qlp_fused_product(None) == -1


# ---- 8. row-partitioned ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_row_partitioned(K, ctx, oracle, ops, world):
    """2 and 3 in-process ranks against the single-rank result within the case's budget; per rank path 2 = path 1 in every bit;
    itmax = 0 means 2n of the GLOBAL system on every rank (the singular case runs 49 iterations whatever the local size)."""
    name = "poisson9_singular"
    S, A0, b, kw = _case(ops, name)
    n = S.shape[0]
    ref_ws = _solve(K, ctx, A0, b, **kw)
    ref, xref = ref_ws.stats, ref_ws.x.to_host()
    rtol = case_budget(oracle, name)
    starts = K.row_partition(n, world)

    def body(cx, rank):
        r0, r1 = starts[rank], starts[rank + 1]
        sl = S[r0:r1].tocsr()
        sl.sort_indices()
        A = K.CsrMatrix.from_host(cx, sl.indptr, sl.indices, sl.data, (r1 - r0, n), dist_rows=(r0, r1), n_global=n)
        out = {}
        for fused in (2, 1):
            ws = K.MinresQlpWorkspace(cx, r1 - r0, r1 - r0)
            K.minres_qlp_(ws, A, cx.array(b[r0:r1]), fused=fused, history=True, λ=kw["lam"])
            st = ws.stats
            out[fused] = ((st.niter, st.status, st.solved, st.inconsistent), st, ws.last_path,
                          {k: ws.vector(k).to_host() for k in CORE if k != "p"})
        return out

    res = _run_ranks(K, world, 960 + world, body)
    for out in res:
        for fused in (2, 1):
            flags, st, path, _ = out[fused]
            assert path == fused
            _stats_against(st, ref, rtol, PARITY[name])
        assert out[2][0] == out[1][0]
        for k in HISTORIES:                                             # path 2 = path 1 per rank, and every rank has the same
            assert np.array_equal(getattr(out[2][1], k), getattr(out[1][1], k), equal_nan=True), k
            assert np.array_equal(getattr(out[2][1], k), getattr(res[0][2][1], k), equal_nan=True), k
        for k, v in out[2][3].items():
            assert np.array_equal(v, out[1][3][k]), k
    for fused in (2, 1):
        assert _x_ok(np.concatenate([out[fused][3]["x"] for out in res]), xref, rtol)


# ---- 9. no device-memory growth --------------------------------------------------------------------------------------------------
def test_no_device_memory_growth(K, ctx, ops):
    S, A, b, kw = _case(ops, "poisson8")
    bd = ctx.array(b)
    ws = K.MinresQlpWorkspace(ctx, 512, 512, adopt=False)

    def solve(i):
        K.minres_qlp_(ws, A, bd, fused=(2, 1, 0)[i % 3], history=True)
    for i in range(3):
        solve(i)
    ctx.sync()
    free0 = ctx.mem_info()[0]
    for i in range(20):
        solve(i)
    ctx.sync()
    assert ctx.mem_info()[0] >= free0 - (4 << 20)
