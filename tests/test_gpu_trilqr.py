"""trilqr! on the GPU: the three loops against the NumPy restatement of src/trilqr.jl (tests/trilqr_reference.py) and against each
other, with the transfer to the USYMCG point on and off.

Budgets (tests/test_trilqr_host.py holds the functions and shows that they reject the injected faults):
  * path 0 (one launch per primitive) against the restatement: same niter, status and flags; both histories within budget() =
    max(1e-8, 10 x the case's own np.dot-versus-exact deviation) of each entry, plus the absolute floor 1e-12 x the first entry;
    x and t within the same budget of max|x| and max|t|.  Only cases whose own deviation is <= 1e-6 are in the list.
  * path 1 (host-driven, fused kernels) against path 0: elementwise values are the same expressions, the dots differ by <= 1 ulp:
    the same budget.
  * path 2 (device-resident) against path 1 (same kernels, same scalar code): np.array_equal everywhere: x, t, both histories,
    the flags, the status and every role of khip_trilqr_vector.
"""
import os
import sys
import threading

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trilqr_reference as tr  # noqa: E402
import test_usymlq_host as lq_host  # noqa: E402
import test_usymqr_host as qr_host  # noqa: E402
from test_bilq_host import other_c, rhs  # noqa: E402
from test_trilqr_host import (BOTH_C, BOTH_L, BREAKDOWN_B, BREAKDOWN_C, BREAKDOWNS, CASES, EXPECTED, ONLY_T, SMALL_SIZES, TIRED,  # noqa: E402
                              TRANSFERS, UNSYM_BREAKDOWN, _sign_matrix, adjoint_system, budget, case_keywords, case_system, dense_pair, deviation,
                              mismatches, nonsymmetric_definite, pair_budget, reference_pair, summary)

ROLES = tr.VECTORS
NVEC = len(ROLES)


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


def _solve(K, ctx, A, b, c, fused=2, x0=None, y0=None, adopt=None, vectors=None, **kw):
    ws = K.TrilqrWorkspace(ctx, len(b), len(c), adopt=adopt, vectors=vectors)
    if x0 is not None:
        ws.warm_start_(ctx.array(x0), ctx.array(y0))
    K.trilqr_(ws, A, ctx.array(b), ctx.array(c), fused=fused, history=True, **kw)
    return ws


def _xt(ws):
    return ws.x.to_host(), ws.y.to_host()


def _roles(ws):
    return {name: ws.vector(name).to_host() for name in ROLES}


def _flags(s):
    return (s.niter, s.status, s.solved, s.solved_primal, s.solved_dual, s.inconsistent)


def _same_bits(w1, w2):
    s1, s2 = w1.stats, w2.stats
    assert _flags(s1) == _flags(s2)
    assert np.array_equal(s1.residuals_primal, s2.residuals_primal, equal_nan=True)
    assert np.array_equal(s1.residuals_dual, s2.residuals_dual, equal_nan=True)
    assert len(s2.residuals_primal) <= s2.niter + 1 and len(s2.residuals_dual) <= s2.niter + 1
    if s2.niter > 0:                                            # (before the first iteration only x and t are defined)
        r1, r2 = _roles(w1), _roles(w2)
        for name in ROLES:
            assert np.array_equal(r1[name], r2[name], equal_nan=True), name
    for a, b in zip(_xt(w1), _xt(w2)):
        assert np.array_equal(a, b, equal_nan=True)


def _against(ws, ref, bud):
    """mismatches of a workspace's solve against a restatement triple or another workspace."""
    if isinstance(ref, tuple):
        xr, t_r, sr = ref
    else:
        (xr, t_r), sr = _xt(ref), ref.stats
    x, t = _xt(ws)
    return mismatches(ws.stats, sr, bud, x, xr, t, t_r)


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


# ---- 1. path 0 against the restatement, path 1 against path 0, path 2 against path 1: every case, both transfers ------------------
@pytest.mark.parametrize("transfer", TRANSFERS)
@pytest.mark.parametrize("name", list(CASES))
def test_three_paths_on_every_case(K, ctx, oracle, ops, name, transfer):
    S, A, b, c = ops(name)
    ref = reference_pair(oracle, name, transfer)[0]
    bud = budget(oracle, name, transfer)
    kw = case_keywords(name, transfer)
    w0 = _solve(K, ctx, A, b, c, fused=0, **kw)
    w1 = _solve(K, ctx, A, b, c, fused=1, **kw)
    w2 = _solve(K, ctx, A, b, c, fused=2, **kw)
    assert (w0.last_path, w1.last_path, w2.last_path) == (0, 1, 2)
    s0, s1 = w0.stats, w1.stats
    print(f"{name} transfer={transfer}: budget {bud:.2e}; path 0 against the restatement: primal "
          f"{deviation(s0.residuals_primal, ref[2].residuals_primal, 1e-12):.2e}, dual "
          f"{deviation(s0.residuals_dual, ref[2].residuals_dual, 1e-12):.2e}; path 1 against path 0: primal "
          f"{deviation(s1.residuals_primal, s0.residuals_primal, 1e-12):.2e}, dual "
          f"{deviation(s1.residuals_dual, s0.residuals_dual, 1e-12):.2e}")
    assert summary(s0) == EXPECTED[name][0 if transfer else 1]
    assert _against(w0, ref, bud) == []
    assert _against(w1, w0, bud) == []
    _same_bits(w1, w2)
    x, t = _xt(w2)
    if s0.solved_primal:
        assert np.linalg.norm(b - S @ x) <= 1e-6 * np.linalg.norm(b)
    if s0.solved_dual:
        assert np.linalg.norm(c - S.T @ t) <= 1e-6 * np.linalg.norm(c)


# ---- 2. the first iterations: every named vector holds the restatement's variable ------------------------------------------------
@pytest.mark.parametrize("itmax", [1, 2, 3, 4, 5])
def test_roles_hold_the_reference_variables(K, ctx, oracle, ops, itmax):
    """After k iterations every name of khip_trilqr_vector holds what the reference's variable of that name holds at the end of the
    loop, on paths 1 and 2 (bit-identical to each other): k = 1 … 5 walks the stage 1, 2, 3 and >= 4 branches of P3 and the first
    rotation of (wₖ₋₃, wₖ₋₂).  n = 343 is odd: the tail lane does both blocks."""
    S, A, b, c = ops("kron7_it60")
    pair = reference_pair(oracle, "kron7_it60", True, itmax=itmax)
    bud = pair_budget(pair)
    xr, t_r, sr = pair[0]
    w = {f: _solve(K, ctx, A, b, c, fused=f, itmax=itmax) for f in (1, 2)}
    _same_bits(w[1], w[2])
    for fused in (1, 2):
        assert w[fused].last_path == fused and w[fused].stats.niter == itmax
        got = _roles(w[fused])
        for name in ROLES:
            want = sr.vectors[name]
            dev = np.abs(got[name] - want).max() / max(np.abs(want).max(), 1e-300)
            print(f"itmax {itmax} path {fused} {name}: largest deviation {dev:.3e} of its largest entry")
            assert dev <= bud, (fused, name)
        if itmax == 1:
            assert np.array_equal(got["dbar"], got["u_prev"]) and not got["x"].any() and not got["y"].any()
            assert not got["w_prev2"].any() and not got["w_prev3"].any()
        assert len({w[fused].vector(name).ptr for name in ROLES}) == NVEC


# ---- 3. path 2 bit-identical to path 1 on every ending ---------------------------------------------------------------------------
def _endings(K, ctx, ops):
    S, A, b, c = ops("kron4_sinc")
    S8, A8, b8, c8 = ops("poisson8")
    S16, A16, b16, c16 = ops("poisson16")
    Ab, bb, cb = UNSYM_BREAKDOWN
    off = dict(transfer_to_usymcg=False)
    return {  # ending -> (A, b, c, keywords, (niter, status, nprimal, ndual), runs the loop)
        "primal_first": (A8, b8, c8, {}, (31, BOTH_C, 30, 31), True),
        "dual_first_odd_gap": (A8, b8, c8, off, (36, BOTH_L, 36, 31), True),
        "dual_first_even_gap": (A8, b8, c8, dict(off, itmax=35), (35, ONLY_T, 35, 31), True),       # only one side solved at itmax
        "dual_first_odd_gap_16": (A16, b16, c16, off, (74, BOTH_L, 74, 63), True),
        "dual_first_even_gap_16": (A16, b16, c16, dict(off, itmax=71), (71, ONLY_T, 71, 63), True),
        "same_iteration": (A16, b16, c16, {}, (63, BOTH_C, 63, 63), True),
        "tired": (A, b, c, dict(itmax=40), (40, TIRED, 40, 40), True),
        "timemax": (A, b, c, dict(timemax=1e-9), (1, "time limit exceeded", 1, 1), True),
        "unsymmetric_breakdown": (_dense(K, ctx, Ab), bb, cb, {}, None, True),
        "unsymmetric_breakdown_lq": (_dense(K, ctx, Ab), bb, cb, off, None, True),
        "b_zero": (A, np.zeros(len(b)), c, dict(itmax=6), (6, TIRED, 0, 6), True),
        "c_zero": (A, b, np.zeros(len(c)), dict(itmax=6), (6, TIRED, 6, 0), True),
        "b_and_c_zero": (A, np.zeros(len(b)), np.zeros(len(c)), {}, (0, "unknown", 0, 0), False),
    }


@pytest.mark.parametrize("ending", ["primal_first", "dual_first_odd_gap", "dual_first_even_gap", "dual_first_odd_gap_16",
                                    "dual_first_even_gap_16", "same_iteration", "tired", "timemax", "unsymmetric_breakdown",
                                    "unsymmetric_breakdown_lq", "b_zero", "c_zero", "b_and_c_zero"])
def test_path2_is_bit_identical_to_path1(K, ctx, ops, ending):
    A, b, c, kw, want, loops = _endings(K, ctx, ops)[ending]
    w1 = _solve(K, ctx, A, b, c, fused=1, **kw)
    w2 = _solve(K, ctx, A, b, c, fused=2, **kw)
    assert w1.last_path == 1 and w2.last_path == (2 if loops else 1)
    _same_bits(w1, w2)
    if want is not None:
        assert summary(w2.stats) == want, summary(w2.stats)
    if ending.startswith("dual_first"):
        # the dual block stopped rotating (wₖ₋₃, wₖ₋₂) at iteration ndual, the device loop's host went on: the names still follow
        w0 = _solve(K, ctx, A, b, c, fused=0, **kw)
        for name in ("w_prev3", "w_prev2", "y"):
            a0, a2 = w0.vector(name).to_host(), w2.vector(name).to_host()
            assert np.abs(a2 - a0).max() <= 1e-6 * np.abs(a0).max(), name


@pytest.mark.parametrize("ending", ["b_zero", "c_zero"])
def test_zero_right_hand_side_follows_the_reference(K, ctx, ops, ending):
    """No early return: the side whose right-hand side is zero starts solved, the other one runs on 0 / 0 to itmax.  Compared with
    the restatement NaN for NaN, on all three paths."""
    A, b, c, kw, want, _ = _endings(K, ctx, ops)[ending]
    S = ops("kron4_sinc")[0]
    ref = tr.trilqr(S, b, c, **kw)
    def close(a, r):                                             # NaN where the restatement has NaN, 1e-8 of the largest entry elsewhere
        a, r = np.asarray(a), np.asarray(r)
        assert a.shape == r.shape and np.array_equal(np.isnan(a), np.isnan(r))
        f = np.isfinite(r)
        assert not f.any() or np.abs(a[f] - r[f]).max() <= 1e-8 * max(np.abs(r[f]).max(), 1e-300)
    for fused in (0, 1, 2):
        ws = _solve(K, ctx, A, b, c, fused=fused, **kw)
        st = ws.stats
        assert ws.last_path == fused and summary(st) == want and summary(ref[2]) == want
        assert (st.solved_primal, st.solved_dual, st.inconsistent) == (ref[2].solved_primal, ref[2].solved_dual, ref[2].inconsistent)
        for a, r in zip(_xt(ws) + (st.residuals_primal, st.residuals_dual), ref[:2] + (ref[2].residuals_primal, ref[2].residuals_dual)):
            close(a, r)
        assert (st.solved_primal, st.solved_dual) == ((True, False) if ending == "b_zero" else (False, True))


@pytest.mark.parametrize("fused", [0, 1, 2])
@pytest.mark.parametrize("transfer", TRANSFERS)
def test_unsymmetric_breakdown(K, ctx, fused, transfer):
    """A = [0 1; −1 0], b = e₁, c = −e₁: δbar₁ = 0 exactly, so the guard skips the transfer at k = 1 (no ζbar = 1 / 0); finite
    everywhere, x = e₂."""
    Ab, bb, cb = UNSYM_BREAKDOWN
    pair = dense_pair(Ab, bb, cb, transfer_to_usymcg=transfer)
    ws = _solve(K, ctx, _dense(K, ctx, Ab), bb, cb, fused=fused, transfer_to_usymcg=transfer)
    assert ws.last_path == fused
    assert _against(ws, pair[0], pair_budget(pair)) == []
    x, t = _xt(ws)
    assert np.isfinite(x).all() and np.isfinite(t).all() and np.allclose(x, [0.0, 1.0], atol=1e-15, rtol=0.0)


@pytest.mark.parametrize("name", list(BREAKDOWNS))
def test_breakdown_on_one_side(K, ctx, name):
    """β₂ = 0 exactly keeps vₖ, γ₂ = 0 exactly keeps uₖ, each without the other: the same on all three paths."""
    M = BREAKDOWNS[name]
    A = _dense(K, ctx, M)
    pair = dense_pair(M, BREAKDOWN_B, BREAKDOWN_C)
    w = {f: _solve(K, ctx, A, BREAKDOWN_B, BREAKDOWN_C, fused=f) for f in (0, 1, 2)}
    for f in (0, 1, 2):
        assert w[f].last_path == f and _against(w[f], pair[0], pair_budget(pair)) == [], f
    _same_bits(w[1], w[2])
    first = {f: _roles(_solve(K, ctx, A, BREAKDOWN_B, BREAKDOWN_C, fused=f, itmax=1)) for f in (0, 1, 2)}
    for f in (0, 1, 2):
        kept, moved = ("v", "u") if name == "beta2_zero" else ("u", "v")
        assert np.array_equal(first[f][kept], first[f][kept + "_prev"]) and np.array_equal(first[f][kept], [1.0, 0.0]), (f, kept)
        assert np.array_equal(first[f][moved], [0.0, 1.0]), (f, moved)


# ---- 4. shapes where the pass can go wrong -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("transfer", TRANSFERS)
@pytest.mark.parametrize("n", SMALL_SIZES)
def test_small_dense_systems(K, ctx, n, transfer):
    """nonsymmetric_definite(n): one lane, one pair, one wave less one (odd: the tail lane does both blocks), one wave, one wave
    and the tail."""
    M, b = nonsymmetric_definite(n)
    c = other_c(n)
    pair = dense_pair(M, b, c, transfer_to_usymcg=transfer)
    bud = pair_budget(pair)
    A = _dense(K, ctx, M)
    w0, w1, w2 = (_solve(K, ctx, A, b, c, fused=f, transfer_to_usymcg=transfer) for f in (0, 1, 2))
    assert (w0.last_path, w1.last_path, w2.last_path) == (0, 1, 2)
    assert _against(w0, pair[0], bud) == []
    assert _against(w1, w0, bud) == []
    _same_bits(w1, w2)
    assert w2.stats.solved_primal and w2.stats.solved_dual and w2.stats.solved


def test_sizes_of_the_case_list():
    sizes = {lq_host.CASES[CASES[k][0]][1] ** 3 for k in CASES}
    assert {343, 729, 1331, 512, 1728, 4096} <= sizes and max(sizes) <= 4096 and len(CASES) >= 14


def _carved(K, ctx, n, first):
    """The eleven vectors of a workspace inside one buffer, starting at element `first` with an even stride: first = 1 puts every
    vector at an odd element offset (8-byte but not 16-byte aligned), first = 0 keeps them 16-byte aligned."""
    stride = n + 2 - (n & 1) + 2
    buf = ctx.zeros(first + NVEC * stride)
    assert buf.ptr % 16 == 0
    vec = {k: buf.slice(first + i * stride, first + i * stride + n) for i, k in enumerate(K.TrilqrWorkspace.VECTORS)}
    assert all(v.ptr % 16 == 8 * first for v in vec.values())
    return buf, vec


@pytest.mark.parametrize("name", ["kron8_sinc_it60", "kron7_it60"])
def test_adopted_vectors_at_odd_offsets(K, ctx, oracle, ops, name):
    """The 8-byte kernel path (and, with n = 343, the 16-byte path's tail element beside it): bit-identical to an owned workspace
    and to a 16-byte-aligned adoption under path 2, within budget of path 0; nothing is written between the carved vectors."""
    S, A, b, c = ops(name)
    n = len(b)
    kw = case_keywords(name, True)
    wo = _solve(K, ctx, A, b, c, adopt=False, **kw)
    buf1, odd = _carved(K, ctx, n, 1)
    w1 = _solve(K, ctx, A, b, c, vectors=odd, **kw)
    buf0, even = _carved(K, ctx, n, 0)
    w0 = _solve(K, ctx, A, b, c, vectors=even, **kw)
    assert (wo.last_path, w1.last_path, w0.last_path) == (2, 2, 2)
    _same_bits(wo, w1)
    _same_bits(wo, w0)
    wp = _solve(K, ctx, A, b, c, fused=0, **kw)
    assert wp.last_path == 0 and _against(w1, wp, budget(oracle, name)) == []
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
    kw = case_keywords(name, True)
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
        assert _against(w2, wd, budget(oracle, name)) == []
    finally:
        ctx.set_option("compensated", keep)


def test_adopted_workspace_is_bit_identical_to_owned(K, ctx, ops):
    name = "kron8_sinc_it60"
    S, A, b, c = ops(name)
    n = len(b)
    vec = {k: ctx.empty(n) for k in K.TrilqrWorkspace.VECTORS}
    ws = K.TrilqrWorkspace(ctx, n, n, vectors=vec)
    K.trilqr_(ws, A, ctx.array(b), ctx.array(c), history=True, itmax=60)
    assert ws.x is vec["x"] and ws.y is vec["y"] and ws.last_path == 2      # solution(ws) is the caller's x and t
    wo = _solve(K, ctx, A, b, c, adopt=False, itmax=60)
    _same_bits(wo, ws)
    assert K.TrilqrWorkspace(ctx, n, n, adopt=False).nbytes == 8 * 11 * n
    assert K.TrilqrWorkspace(ctx, 25, 10, adopt=False).nbytes == 8 * (5 * 10 + 6 * 25)
    assert K.TrilqrWorkspace(ctx, 10, 25, adopt=False).nbytes == 8 * (5 * 25 + 6 * 10)
    assert A._adjoint is not None and K._adjoint_of(A) is A._adjoint     # A' is taken once and kept on the matrix
    x, t, st, ws2 = K.trilqr(A, ctx.array(b), ctx.array(c), history=True, itmax=60)
    assert ws2.last_path == 2                                  # the out-of-place entry forwards the default callback
    assert np.array_equal(x.to_host(), wo.x.to_host()) and np.array_equal(t.to_host(), wo.y.to_host())
    assert np.array_equal(st.residuals_dual, wo.stats.residuals_dual)
    ws3 = K.krylov_workspace("trilqr", A, ctx.array(b), ctx.array(c))
    assert isinstance(ws3, K.TrilqrWorkspace)
    K.krylov_solve_(ws3, A, ctx.array(b), c=ctx.array(c), history=True, itmax=60)
    assert ws3.last_path == 2 and np.array_equal(ws3.y.to_host(), wo.y.to_host())


# ---- 5. rectangular ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [0, 2])
def test_rectangular_adjoint_runs_the_primitive_sequence(K, ctx, fused):
    """rectangular_adjoint of the reference's tests (A is 10 x 25; the dual system is inconsistent and ends by ‖A s‖): m ≠ n runs
    path 0 whatever `fused` says; the residual tests of test/test_trilqr.jl at 1e-6; khip_stats.inconsistent carries the flag and
    the status stays the reference's."""
    M, b, c = adjoint_system("rectangular_adjoint")
    pair = dense_pair(M, b, c)
    ws = _solve(K, ctx, _dense(K, ctx, M), b, c, fused=fused)
    assert ws.last_path == 0 and ws.m == 10 and ws.n == 25
    assert _against(ws, pair[0], pair_budget(pair)) == []
    x, t = _xt(ws)
    st = ws.stats
    assert len(x) == 25 and len(t) == 10 and st.solved_primal and st.solved_dual and st.inconsistent
    assert np.linalg.norm(b - M @ x) <= 1e-6 * np.linalg.norm(b)
    assert np.linalg.norm(M @ (c - M.T @ t)) <= 1e-6 * np.linalg.norm(M @ c)
    assert st.status == pair[0][2].status


@pytest.mark.parametrize("itmax", [5, 0])
@pytest.mark.parametrize("shape", [(12, 20), (20, 12), (33, 65)])
def test_rectangular_vectors_have_their_sides_lengths(K, ctx, shape, itmax):
    """underdetermined_adjoint / overdetermined_adjoint of test/test_utils.jl at small sizes (at their own sizes, 100 x 200, the
    restatement's dot modes disagree on niter): five iterations and a full solve.  Every named vector has its side's length and the
    restatement's values (the w recurrence and t run on m entries, x and d̅ on n)."""
    m, n = shape
    M = _sign_matrix(m, n)
    b, c = M @ np.arange(1.0, n + 1), M.T @ np.arange(-float(m), 0.0)
    pair = dense_pair(M, b, c, itmax=itmax)
    bud = pair_budget(pair)
    assert bud <= 1e-6
    ws = _solve(K, ctx, _dense(K, ctx, M), b, c, fused=2, itmax=itmax)
    assert ws.last_path == 0 and summary(ws.stats) == summary(pair[0][2])
    assert _against(ws, pair[0], bud) == []
    for role in ROLES:
        got, want = ws.vector(role).to_host(), pair[0][2].vectors[role]
        assert len(got) == len(want) == (m if role in K.TrilqrWorkspace.ROW_SIDE else n), role
        if itmax or role in ("x", "y"):                          # (at convergence βₖ₊₁ and γₖ₊₁ are rounding: vₖ₊₁, uₖ₊₁ are not compared)
            assert np.abs(got - want).max() <= bud * max(np.abs(want).max(), 1e-300), role
    if itmax == 0:
        x, t = _xt(ws)
        assert np.linalg.norm(b - M @ x) <= 1e-6 * np.linalg.norm(b) and np.linalg.norm(c - M.T @ t) <= 1e-6 * np.linalg.norm(c)


def test_row_partitioned_rectangular_handle_is_refused(K, oracle):
    M, b, c = qr_host.known_system("over_consistent")              # 25 x 10

    def body(cx, rank):
        r0, r1 = (0, 13) if rank == 0 else (13, 25)
        S = sp.csr_matrix(M[r0:r1])
        S.sort_indices()
        A = K.CsrMatrix.from_host(cx, S.indptr, S.indices, S.data, (r1 - r0, 25), dist_rows=(r0, r1), n_global=25)
        ws = K.TrilqrWorkspace(cx, r1 - r0, 10)
        with pytest.raises(K.KhipError, match="row-partitioned rectangular system") as e:
            K.trilqr_(ws, A, cx.array(b[r0:r1]), cx.array(c), At=lambda x, y: None)
        return e.value.code if hasattr(e.value, "code") else str(e.value)

    res = _run_ranks(K, 2, 33001, body)
    assert all(r == -3 or "error -3" in str(r) for r in res), res


# ---- 6. behaviour around the solve ---------------------------------------------------------------------------------------------------
def test_argument_errors(K, ctx, ops):
    S, A, b, c = ops("kron4_sinc")
    n = len(b)
    ws = K.TrilqrWorkspace(ctx, n, n)
    keep = []
    op = K._make_operator(ctx, A, n, keep)
    bd, cd = ctx.array(b), ctx.array(c)
    rc = K.lib().khip_trilqr_solve(ws._h, op, None, bd.ptr, cd.ptr, None, None)
    assert rc == -1 and "At" in K.lib().khip_last_error().decode()
    rc = K.lib().khip_trilqr_solve(ws._h, op, K._make_operator(ctx, A.transpose(), n, keep), bd.ptr, None, None, None)
    assert rc == -1 and "c is required" in K.lib().khip_last_error().decode()
    with pytest.raises(K.KhipError, match="c .* is required"):
        K.trilqr_(ws, A, bd)
    small = K.TrilqrWorkspace(ctx, n - 1, n - 1)
    with pytest.raises(K.KhipError, match="inconsistent with size"):
        K.trilqr_(small, A, ctx.array(rhs(n - 1)), ctx.array(rhs(n - 1)))
    with pytest.raises(K.KhipError, match="Inconsistent problem size"):
        K.trilqr_(ws, A, ctx.array(rhs(n - 1)), cd)
    with pytest.raises(K.KhipError, match="Inconsistent problem size"):
        K.trilqr_(ws, A, bd, ctx.array(rhs(n - 1)))
    with pytest.raises(K.KhipError, match="warm_start needs x0 and y0"):
        ws.warm_start_(bd)
    assert K.lib().khip_trilqr_warm_start(ws._h, bd.ptr, None) == -1
    v = [ctx.empty(n) for _ in range(NVEC)]
    v[10] = v[2]
    with pytest.raises(K.KhipError, match="must be distinct"):
        K.TrilqrWorkspace(ctx, n, n, vectors=dict(zip(K.TrilqrWorkspace.VECTORS, v)))


@pytest.mark.parametrize("adopt", [False, True])
@pytest.mark.parametrize("fused", [0, 1, 2])
def test_warm_start_with_x0_and_y0(K, ctx, oracle, ops, fused, adopt):
    name = "kron8_shift24_sinc"
    S, A, b, c = ops(name)
    n = len(b)
    x0, y0 = np.linspace(-0.5, 0.5, n), np.linspace(0.25, -0.25, n)
    ws = _solve(K, ctx, A, b, c, fused=fused, x0=x0, y0=y0, adopt=adopt)
    assert ws.last_path == fused
    pair = reference_pair(oracle, name, True, x0=x0, y0=y0)
    assert _against(ws, pair[0], pair_budget(pair)) == []
    x, t = _xt(ws)
    assert ws.stats.solved_primal and np.linalg.norm(b - S @ x) <= 1e-6 * np.linalg.norm(b)
    assert ws.stats.solved_dual and np.linalg.norm(c - S.T @ t) <= 1e-6 * np.linalg.norm(c)
    again = _solve(K, ctx, A, b, c, fused=fused)                 # the warm start is used up: a fresh workspace agrees with a second solve
    K.trilqr_(ws, A, ctx.array(b), ctx.array(c), fused=fused, history=True)
    _same_bits(again, ws)


@pytest.mark.parametrize("fused", [0, 1])
def test_callback_sees_both_histories_and_stops(K, ctx, ops, fused):
    S, A, b, c = ops("kron4_sinc")
    seen = []

    def cb(w):
        st = w.stats
        seen.append((len(st.residuals_primal), len(st.residuals_dual)))
        return len(seen) == 3
    ws = _solve(K, ctx, A, b, c, fused=fused, callback=cb)
    st = ws.stats
    assert ws.last_path == fused
    assert seen == [(2, 2), (3, 3), (4, 4)]
    assert st.niter == 3 and st.status == "user-requested exit" and not st.solved
    xr, t_r, sr = tr.trilqr(S, b, c, itmax=3)
    assert deviation(st.residuals_primal, sr.residuals_primal, 1e-12) <= 1e-10
    assert deviation(st.residuals_dual, sr.residuals_dual, 1e-12) <= 1e-10
    x, t = _xt(ws)
    assert np.abs(x - xr).max() <= 1e-10 * np.abs(xr).max() and np.abs(t - t_r).max() <= 1e-10 * np.abs(t_r).max()


def test_last_path_and_verbose(K, ctx, ops, tmp_path):
    S, A, b, c = ops("poisson8")
    n = len(b)
    path = lambda **kw: _solve(K, ctx, A, b, c, **kw).last_path  # noqa: E731
    assert path() == 2
    assert path(callback=lambda w: False) == 1
    assert path(At=lambda x, y: A._adjoint.matvec(x, y)) == 1   # a user operator
    assert path(fused=0) == 0
    zero = lambda **kw: _solve(K, ctx, A, np.zeros(n), np.zeros(n), **kw).last_path  # noqa: E731
    assert zero() == 1 and zero(fused=0) == 0                    # a loop that never starts (both sides solved at once) reports 1
    assert path(rtol=1.0) == 2                                   # no test before the loop (:190-196): one iteration runs
    log = tmp_path / "trilqr.log"
    with open(log, "w") as f:
        ws = _solve(K, ctx, A, b, c, verbose=1, iostream=f, transfer_to_usymcg=False)
    st = ws.stats
    assert ws.last_path == 1 and summary(st) == (36, BOTH_L, 36, 31)
    lines = open(log, encoding="utf-8").read().splitlines()
    assert lines[0] == f"TRILQR: primal system of {n} equations in {n} variables"
    assert lines[1] == f"TRILQR: dual system of {n} equations in {n} variables"
    assert lines[2] == "%5s  %7s  %7s  %5s" % ("k", "‖rₖ‖", "‖sₖ‖", "timer")
    rows = [ln for ln in lines[3:] if ln.strip()]
    # both sides unsolved up to k = 30; the dual side is solved in iteration 31 and the rows show ✗ in its column; the row of the
    # iteration that solves the second side is not printed (:417-419)
    assert [int(r.split()[0]) for r in rows] == list(range(0, 36))
    assert rows[0].startswith("    0  %7.1e  %7.1e  " % (st.residuals_primal[0], st.residuals_dual[0]))
    assert rows[10].startswith("   10  %7.1e  %7.1e  " % (st.residuals_primal[10], st.residuals_dual[10]))
    assert rows[31].startswith("   31  %7.1e  ✗ ✗ ✗ ✗  " % st.residuals_primal[31]) and rows[35].startswith("   35  %7.1e  ✗ ✗ ✗ ✗  " % st.residuals_primal[35])
    with open(log, "w") as f:
        ws = _solve(K, ctx, A, b, c, verbose=1, iostream=f)
    rows = [ln for ln in open(log, encoding="utf-8").read().splitlines()[3:] if ln.strip()]
    assert summary(ws.stats) == (31, BOTH_C, 30, 31) and len(rows) == 31
    assert rows[30].startswith("   30  ✗ ✗ ✗ ✗  %7.1e  " % ws.stats.residuals_dual[30])


def test_full_status_and_its_cut(K, ctx):
    """khip_stats.status holds 95 bytes; the adjoint stats carry the whole string (the 1 x 1 system ends with one of the long ones)."""
    M, b = nonsymmetric_definite(1)
    pair = dense_pair(M, b, other_c(1))
    ws = _solve(K, ctx, _dense(K, ctx, M), b, other_c(1))
    full = ws.stats.status
    assert full == pair[0][2].status and len(full.encode()) > 95
    short = K.lib().khip_trilqr_stats(ws._h).contents.status.decode("utf-8")      # decodes: cut at a character boundary
    assert full.startswith(short) and 90 <= len(short.encode()) <= 95


def test_path2_history_window_drain(K, ctx, ops):
    """A solve longer than the window, with histories of different lengths: the dual side of poisson16 ends at 63, the primal at 74."""
    S, A, b, c = ops("poisson16")
    kw = dict(transfer_to_usymcg=False)
    ctx.set_option("hist_window", 8)
    try:
        w2 = _solve(K, ctx, A, b, c, fused=2, **kw)
    finally:
        ctx.set_option("hist_window", 1 << 14)
    w1 = _solve(K, ctx, A, b, c, fused=1, **kw)
    assert (w1.last_path, w2.last_path) == (1, 2) and summary(w2.stats) == (74, BOTH_L, 74, 63)
    _same_bits(w1, w2)


def test_row_partitioned(K, ctx, oracle, ops):
    name = "kron8_sinc_it60"
    world = 2
    S, A0, b, c = ops(name)
    n = len(b)
    ref = _solve(K, ctx, A0, b, c, itmax=60)
    xref, tref = _xt(ref)
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
            ws = K.TrilqrWorkspace(cx, r1 - r0, r1 - r0)
            K.trilqr_(ws, A, cx.array(b[r0:r1]), cx.array(c[r0:r1]), At=At, fused=fused, history=True, itmax=60)
            out[fused] = (ws.stats, ws.last_path, ws.x.to_host(), ws.y.to_host())
        return out

    res = _run_ranks(K, world, 33002, body)
    for out in res:
        for fused in (2, 1, 0):
            st, path = out[fused][:2]
            assert path == fused
            assert mismatches(st, ref.stats, bud) == []
        for h in ("residuals_primal", "residuals_dual"):
            assert np.array_equal(getattr(out[2][0], h), getattr(out[1][0], h))
            assert np.array_equal(getattr(out[2][0], h), getattr(res[0][2][0], h))
    for fused in (2, 1):
        x = np.concatenate([out[fused][2] for out in res])
        t = np.concatenate([out[fused][3] for out in res])
        assert np.abs(x - xref).max() <= bud * np.abs(xref).max() and np.abs(t - tref).max() <= bud * np.abs(tref).max()
    assert all(np.array_equal(out[2][2], out[1][2]) and np.array_equal(out[2][3], out[1][3]) for out in res)


def test_no_device_memory_growth(K, ctx, ops):
    S, A, b, c = ops("kron8_sinc_it60")
    bd, cd = ctx.array(b), ctx.array(c)
    ws = K.TrilqrWorkspace(ctx, len(b), len(c), adopt=False)

    def solve(i):
        K.trilqr_(ws, A, bd, cd, fused=(2, 1, 0)[i % 3], history=True, itmax=20)
    for i in range(3):
        solve(i)
    ctx.sync()
    free0 = ctx.mem_info()[0]
    for i in range(20):
        solve(i)
    ctx.sync()
    assert ctx.mem_info()[0] >= free0 - (4 << 20)


def test_profile_bracket_counts_one_p3_per_iteration(K, ctx, ops):
    """The `trilqr_p3` bracket: one launch per iteration on the host-driven loop and per enqueued iteration on the device-resident
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
        assert prof["trilqr_p3"][0] == itmax and prof["trilqr_p3"][1] > 0.0, prof
        assert prof["ssy_p1"][0] == itmax and prof["ssy_p2"][0] == itmax, prof
        assert prof["usymqr_p3"][0] == 0 and prof["usymlq_p3"][0] == 0, prof


# ---- 7. the siblings on the same driver still give what they gave ------------------------------------------------------------------
def test_siblings_are_unchanged(K, ctx, oracle, ops):
    """usymlq! and usymqr! on kron7_shift24_sinc: the niter and status their own tests pin (tests/test_usymlq_host.py,
    tests/test_usymqr_host.py), on all three paths, and path 1 = path 2 in every bit.  Guards the move of usymlq_xd into a header
    and the begin_iteration hook of SsyPolicy."""
    name = "kron7_shift24_sinc"
    S, A, b, c = ops(name)
    bd, cd = ctx.array(b), ctx.array(c)
    lq, qr = {}, {}
    for fused in (0, 1, 2):
        ws = K.UsymlqWorkspace(ctx, len(b), len(c))
        K.usymlq_(ws, A, bd, cd, fused=fused, history=True)
        lq[fused] = ws
        assert ws.last_path == fused and (ws.stats.niter, ws.stats.status) == lq_host.EXPECTED[name][0]
        ws = K.UsymqrWorkspace(ctx, len(b), len(c))
        K.usymqr_(ws, A, bd, cd, fused=fused, history=True)
        qr[fused] = ws
        assert ws.last_path == fused and ws.stats.niter == qr_host.EXPECTED_NITER[name] and ws.stats.solved
    for w, roles in ((lq, K.UsymlqWorkspace.VECTORS), (qr, K.UsymqrWorkspace.VECTORS)):
        assert np.array_equal(w[1].stats.residuals, w[2].stats.residuals)
        for role in roles:
            assert np.array_equal(w[1].vector(role).to_host(), w[2].vector(role).to_host()), role
        assert lq_host.mismatches(w[1].stats, w[0].stats, 1e-8, w[1].x.to_host(), w[0].x.to_host()) == []
    assert np.array_equal(qr[1].stats.Aresiduals, qr[2].stats.Aresiduals)
