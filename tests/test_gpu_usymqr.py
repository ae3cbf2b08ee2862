"""usymqr! on the GPU: the three loops against the NumPy restatement of src/usymqr.jl (tests/usymqr_reference.py) and against each
other.

Budgets (tests/test_usymqr_host.py holds the functions and shows that they reject the injected faults):
  * path 0 (one launch per primitive) against the restatement: same niter, status and flags; both histories within budget() =
    max(1e-8, 10 x the case's own np.dot-versus-exact deviation) of each entry, plus the absolute floor 1e-12 x the first entry;
    x within the same budget of max|x|.  Only cases whose own deviation is <= 1e-6 are in the list.
  * path 1 (host-driven, fused kernels) against path 0: elementwise values are the same expressions, the dots differ by <= 1 ulp:
    the same budget.
  * path 2 (device-resident) against path 1 (same kernels, same scalar code): np.array_equal everywhere: x, both histories and
    every role of khip_usymqr_vector.
"""
import os
import sys
import threading

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import usymqr_reference as ur  # noqa: E402
from test_bilq_host import other_c, rhs  # noqa: E402
from test_usymqr_host import (BREAKDOWN_B, BREAKDOWN_C, BREAKDOWNS, CASES, CONSISTENT, EXPECTED_NITER, INCONSISTENT,  # noqa: E402
                              RECTANGULAR, SOLVED, TIRED, budget, case_system, deviation, known_system, mismatches,
                              nonsymmetric_definite, pair_budget, reference_pair)

ROLES = ("v_prev", "v", "q", "x", "w_prev2", "w_prev", "u_prev", "u", "p")


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


_pair_budget = pair_budget


def _dense_pair(A, b, c, **kw):
    A = np.asarray(A, dtype=np.float64)
    return ur.usymqr(A, b, c, **kw), ur.usymqr(A, b, c, dot=ur.fsum_dot, **kw)


def _device(K, ctx, S):
    S = sp.csr_matrix(S)
    S.sort_indices()
    return K.CsrMatrix.from_host(ctx, S.indptr, S.indices, S.data, S.shape)


def _dense(K, ctx, M):
    return _device(K, ctx, sp.csr_matrix(np.asarray(M, dtype=np.float64)))


def _solve(K, ctx, A, b, c, fused=2, x0=None, adopt=None, vectors=None, **kw):
    ws = K.UsymqrWorkspace(ctx, len(b), len(c), adopt=adopt, vectors=vectors)
    if x0 is not None:
        ws.warm_start_(ctx.array(x0))
    K.usymqr_(ws, A, ctx.array(b), ctx.array(c), fused=fused, history=True, **kw)
    return ws


def _run(K, ctx, A, b, c, **kw):
    ws = _solve(K, ctx, A, b, c, **kw)
    return ws.x.to_host(), ws.stats, ws.last_path


def _roles(ws):
    return {name: ws.vector(name).to_host() for name in ROLES}


def _same_bits(w1, w2):
    s1, s2 = w1.stats, w2.stats
    assert (s1.niter, s1.status, s1.solved, s1.inconsistent) == (s2.niter, s2.status, s2.solved, s2.inconsistent)
    assert np.array_equal(s1.residuals, s2.residuals, equal_nan=True) and len(s2.residuals) == s2.niter + 1
    assert np.array_equal(s1.Aresiduals, s2.Aresiduals, equal_nan=True) and len(s2.Aresiduals) == s2.niter
    if s2.niter > 0:                                            # (before the first iteration only x is defined)
        r1, r2 = _roles(w1), _roles(w2)
        for name in ROLES:
            assert np.array_equal(r1[name], r2[name], equal_nan=True), name
    assert np.array_equal(w1.x.to_host(), w2.x.to_host(), equal_nan=True)


_OPS = {}


@pytest.fixture(scope="module")
def ops(K, ctx, oracle):
    """(scipy operator, device operator, b, c) of a case of the list, built once per module."""
    def get(name):
        if name not in _OPS:
            S, b, c = case_system(oracle, name)
            _OPS[name] = (S, _device(K, ctx, S), b, c)
        return _OPS[name]
    yield get
    _OPS.clear()


def _kw(name):
    return dict(CASES[name][4])


# ---- 1. path 0 against the restatement, path 1 against path 0, path 2 against path 1: every case ----------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_three_paths_on_every_case(K, ctx, oracle, ops, name):
    S, A, b, c = ops(name)
    (xr, sr), _ = reference_pair(oracle, name)
    bud = budget(oracle, name)
    w0 = _solve(K, ctx, A, b, c, fused=0, **_kw(name))
    w1 = _solve(K, ctx, A, b, c, fused=1, **_kw(name))
    w2 = _solve(K, ctx, A, b, c, fused=2, **_kw(name))
    assert (w0.last_path, w1.last_path, w2.last_path) == (0, 1, 2)
    x0_, x1 = w0.x.to_host(), w1.x.to_host()
    s0, s1 = w0.stats, w1.stats
    print(f"{name}: budget {bud:.2e}; path 0 against the restatement: residuals {deviation(s0.residuals, sr.residuals, 1e-12):.2e}, "
          f"Aresiduals {deviation(s0.Aresiduals, sr.Aresiduals, 1e-12):.2e}, x {np.abs(x0_ - xr).max() / np.abs(xr).max():.2e}; path 1 "
          f"against path 0: residuals {deviation(s1.residuals, s0.residuals, 1e-12):.2e}, x {np.abs(x1 - x0_).max() / np.abs(x0_).max():.2e}")
    assert s0.niter == EXPECTED_NITER[name]
    assert mismatches(s0, sr, bud, x0_, xr) == []
    assert mismatches(s1, s0, bud, x1, x0_) == []
    _same_bits(w1, w2)
    if "itmax" not in CASES[name][4]:
        assert s0.solved and np.linalg.norm(b - S @ x0_) <= 1e-6 * np.linalg.norm(b)


# ---- 2. path 2 bit-identical to path 1 on every ending ---------------------------------------------------------------------------
def _endings(K, ctx, ops):
    S, A, b, c = ops("kron4_sinc")
    Ai, bi, ci = known_system("square_inconsistent")
    out = {  # ending -> (A, b, c, keywords, status, niter or None, runs the loop)
        "solved": (A, b, c, {}, SOLVED, 50, True),
        "inconsistent": (_dense(K, ctx, Ai), bi, ci, {}, "unknown", 2, True),
        "b_zero": (A, np.zeros(len(b)), c, {}, "x is a zero-residual solution", 0, False),
        "timemax": (A, b, c, dict(timemax=1e-9), "time limit exceeded", 1, True),
    }
    for k in (1, 2, 3, 4, 5, 9):                                 # both sides of the chunk of four enqueued iterations
        out[f"itmax{k}"] = (A, b, c, dict(itmax=k), TIRED, k, True)
    return out


@pytest.mark.parametrize("ending", ["solved", "inconsistent", "b_zero", "timemax", "itmax1", "itmax2", "itmax3", "itmax4", "itmax5",
                                    "itmax9"])
def test_path2_is_bit_identical_to_path1(K, ctx, ops, ending):
    A, b, c, kw, status, niter, loops = _endings(K, ctx, ops)[ending]
    w1 = _solve(K, ctx, A, b, c, fused=1, **kw)
    w2 = _solve(K, ctx, A, b, c, fused=2, **kw)
    assert w1.last_path == 1 and w2.last_path == (2 if loops else 1)
    _same_bits(w1, w2)
    s2 = w2.stats
    assert s2.status == status and s2.niter == niter, (s2.status, s2.niter)
    assert s2.inconsistent == (ending == "inconsistent") and s2.solved == (ending in ("solved", "b_zero"))


@pytest.mark.parametrize("itmax", [1, 2, 3, 7])
@pytest.mark.parametrize("fused", [1, 2])
def test_roles_hold_the_reference_variables(K, ctx, oracle, ops, itmax, fused):
    """After k iterations every name of khip_usymqr_vector holds what the reference's variable of that name holds at the end of the
    loop (w_prev = wₖ, w_prev2 = wₖ₋₁ or zeros after one iteration), for both parities of the rotations."""
    S, A, b, c = ops("kron7_it60")
    ws = _solve(K, ctx, A, b, c, fused=fused, itmax=itmax)
    assert ws.last_path == fused and ws.stats.niter == itmax
    pair = reference_pair(oracle, "kron7_it60", itmax=itmax)
    bud = _pair_budget(pair)
    (xr, sr), _ = pair
    got = _roles(ws)
    for name in ROLES:
        want = xr if name == "x" else sr.vectors[name]
        dev = np.abs(got[name] - want).max() / max(np.abs(want).max(), 1e-300)
        print(f"{name}: largest deviation {dev:.3e} of its largest entry")
        assert dev <= bud, name
    if itmax == 1:
        assert not got["w_prev2"].any()
    assert len({ws.vector(name).ptr for name in ROLES}) == len(ROLES)


# ---- 3. shapes where the passes can go wrong -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65])
def test_small_dense_systems(K, ctx, n):
    """nonsymmetric_definite(n): one lane, one pair, one wave less one, one wave, one wave and the tail."""
    M, b = nonsymmetric_definite(n)
    c = other_c(n)
    pair = _dense_pair(M, b, c)
    (xr, sr), _ = pair
    bud = _pair_budget(pair)
    A = _dense(K, ctx, M)
    w0, w1, w2 = (_solve(K, ctx, A, b, c, fused=f) for f in (0, 1, 2))
    assert (w0.last_path, w1.last_path, w2.last_path) == (0, 1, 2)
    assert mismatches(w0.stats, sr, bud, w0.x.to_host(), xr) == []
    assert mismatches(w1.stats, w0.stats, bud, w1.x.to_host(), w0.x.to_host()) == []
    _same_bits(w1, w2)
    assert w2.stats.solved


def test_sizes_of_the_case_list():
    """343 (one workgroup of pairs plus the odd tail), 729 and 1331 (several plus the tail), 512 (exactly one), 1728, 4096 are all
    in the list that test_three_paths_on_every_case walks."""
    sizes = {CASES[k][1] ** 3 for k in CASES if CASES[k][0] != "nsd"}
    assert {343, 729, 1331, 512, 1728, 4096} <= sizes and max(sizes) <= 4096


# ---- 4. instantiations -------------------------------------------------------------------------------------------------------------
def _carved(K, ctx, n, first):
    """The nine vectors of a workspace inside one buffer, starting at element `first` with an even stride: first = 1 puts every
    vector at an odd element offset (8-byte but not 16-byte aligned), first = 0 keeps them 16-byte aligned."""
    stride = n + 2 - (n & 1) + 2
    buf = ctx.zeros(first + 9 * stride)
    assert buf.ptr % 16 == 0
    vec = {k: buf.slice(first + i * stride, first + i * stride + n) for i, k in enumerate(K.UsymqrWorkspace.VECTORS)}
    assert all(v.ptr % 16 == 8 * first for v in vec.values())
    return buf, vec


@pytest.mark.parametrize("name", ["kron8_sinc_it60", "kron7_it60"])
def test_adopted_vectors_at_odd_offsets(K, ctx, oracle, ops, name):
    """The 8-byte kernel path (and, with n = 343, the 16-byte path's tail element beside it): bit-identical to an owned workspace
    and to a 16-byte-aligned adoption under path 2, within budget of path 0; nothing is written between the carved vectors."""
    S, A, b, c = ops(name)
    n = len(b)
    kw = _kw(name)
    xo, so, po = _run(K, ctx, A, b, c, adopt=False, **kw)
    buf1, odd = _carved(K, ctx, n, 1)
    x1, s1, p1 = _run(K, ctx, A, b, c, vectors=odd, **kw)
    buf0, even = _carved(K, ctx, n, 0)
    x0_, s0, p0 = _run(K, ctx, A, b, c, vectors=even, **kw)
    assert (po, p1, p0) == (2, 2, 2)
    for x, s in ((x1, s1), (x0_, s0)):
        assert s.niter == so.niter and s.status == so.status
        assert np.array_equal(s.residuals, so.residuals) and np.array_equal(s.Aresiduals, so.Aresiduals) and np.array_equal(x, xo)
    xp, sp0, pp = _run(K, ctx, A, b, c, fused=0, **kw)
    assert pp == 0 and mismatches(s1, sp0, budget(oracle, name), x1, xp) == []
    stride = n + 2 - (n & 1) + 2
    for first, buf in ((1, buf1), (0, buf0)):
        h = buf.to_host()
        gaps = np.ones(len(h), dtype=bool)
        for i in range(9):
            gaps[first + i * stride:first + i * stride + n] = False
        assert not h[gaps].any(), "a kernel wrote outside its vectors"


def test_eight_byte_path_after_one_iteration(K, ctx, ops):
    """One iteration from the same state, on 16-byte vectors and on vectors carved at element offset 1 (the 8-byte instantiations):
    the two fused runs agree in every bit of every role; against path 0 the roles that pass through no reduction (vₖ₋₁ = v₁ and
    uₖ₋₁ = u₁) are bit-identical, and the others (q, p through αₖ; vₖ₊₁, uₖ₊₁, w₁, x through βₖ₊₁, γₖ₊₁, δ₁, ζ₁) are the same expressions
    of scalars that differ by the reductions' last bit at most: 4 eps of the largest entry."""
    S, A, b, c = ops("kron4_sinc")
    w0 = _solve(K, ctx, A, b, c, fused=0, itmax=1)
    w1 = _solve(K, ctx, A, b, c, fused=1, itmax=1)
    _, odd = _carved(K, ctx, len(b), 1)
    w8 = _solve(K, ctx, A, b, c, fused=1, itmax=1, vectors=odd)
    r0, r1, r8 = _roles(w0), _roles(w1), _roles(w8)
    for name in ROLES:
        assert np.array_equal(r1[name], r8[name]), name
    for name in ("v_prev", "u_prev"):
        assert np.array_equal(r0[name], r1[name]), name
    for name in ("q", "p", "v", "u", "w_prev", "x"):
        dev = np.abs(r0[name] - r1[name]).max() / np.abs(r0[name]).max()
        print(f"{name}: path 1 against path 0 {dev:.2e} of the largest entry ({'same bits' if dev == 0 else 'not the same bits'})")
        assert dev <= 4 * np.finfo(float).eps, name


def test_nt_and_compensated_instantiations(K, ctx, oracle, ops):
    name = "kron8_sinc_it60"
    S, A, b, c = ops(name)
    kw = _kw(name)
    xd, sd, _ = _run(K, ctx, A, b, c, **kw)
    keep = ctx.get_option("nt_min_elems")
    assert keep > len(b)
    ctx.set_option("nt_min_elems", 1)
    try:
        xn, sn, pn = _run(K, ctx, A, b, c, **kw)
    finally:
        ctx.set_option("nt_min_elems", keep)
    assert pn == 2 and np.array_equal(xn, xd) and np.array_equal(sn.residuals, sd.residuals) and np.array_equal(sn.Aresiduals, sd.Aresiduals)
    keep = ctx.get_option("compensated")
    ctx.set_option("compensated", 0)
    try:
        w1 = _solve(K, ctx, A, b, c, fused=1, **kw)
        w2 = _solve(K, ctx, A, b, c, fused=2, **kw)
        _same_bits(w1, w2)
        assert mismatches(w2.stats, sd, budget(oracle, name), w2.x.to_host(), xd) == []
    finally:
        ctx.set_option("compensated", keep)


def test_adopted_workspace_is_bit_identical_to_owned(K, ctx, ops):
    name = "kron8_sinc_it60"
    S, A, b, c = ops(name)
    n = len(b)
    vec = {k: ctx.empty(n) for k in K.UsymqrWorkspace.VECTORS}
    ws = K.UsymqrWorkspace(ctx, n, n, vectors=vec)
    K.usymqr_(ws, A, ctx.array(b), ctx.array(c), history=True, itmax=60)
    assert ws.x is vec["x"] and ws.last_path == 2              # solution(ws) is the caller's x
    xo, so, _ = _run(K, ctx, A, b, c, adopt=False, itmax=60)
    assert np.array_equal(vec["x"].to_host(), xo) and np.array_equal(ws.stats.residuals, so.residuals)
    assert np.array_equal(ws.stats.Aresiduals, so.Aresiduals) and ws.stats.niter == so.niter
    assert K.UsymqrWorkspace(ctx, n, n, adopt=False).nbytes == 9 * 8 * n
    assert K.UsymqrWorkspace(ctx, 25, 10, adopt=False).nbytes == 8 * (3 * 25 + 6 * 10)
    assert A._adjoint is not None and K._adjoint_of(A) is A._adjoint     # A' is taken once and kept on the matrix
    x, st, ws2 = K.usymqr(A, ctx.array(b), ctx.array(c), history=True, itmax=60)
    assert ws2.last_path == 2                                  # the out-of-place entry forwards the default callback
    assert np.array_equal(x.to_host(), xo) and np.array_equal(st.residuals, so.residuals)
    ws3 = K.krylov_workspace("usymqr", A, ctx.array(b), ctx.array(c))
    assert isinstance(ws3, K.UsymqrWorkspace)
    K.krylov_solve_(ws3, A, ctx.array(b), c=ctx.array(c), history=True, itmax=60)
    assert ws3.last_path == 2 and np.array_equal(ws3.x.to_host(), xo)


# ---- 5. breakdown on one side -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(BREAKDOWNS))
def test_breakdown_on_one_side(K, ctx, name):
    """β₂ = 0 exactly keeps vₖ, γ₂ = 0 exactly keeps uₖ, each without the other: the same on all three paths."""
    M = BREAKDOWNS[name]
    A = _dense(K, ctx, M)
    pair = _dense_pair(M, BREAKDOWN_B, BREAKDOWN_C)
    (xr, sr), _ = pair
    w = {f: _solve(K, ctx, A, BREAKDOWN_B, BREAKDOWN_C, fused=f) for f in (0, 1, 2)}
    for f in (0, 1, 2):
        assert w[f].last_path == f
        assert mismatches(w[f].stats, sr, _pair_budget(pair), w[f].x.to_host(), xr) == [], f
    _same_bits(w[1], w[2])
    first = {f: _roles(_solve(K, ctx, A, BREAKDOWN_B, BREAKDOWN_C, fused=f, itmax=1)) for f in (0, 1, 2)}
    for f in (0, 1, 2):
        kept, moved = ("v", "u") if name == "beta2_zero" else ("u", "v")
        assert np.array_equal(first[f][kept], first[f][kept + "_prev"]) and np.array_equal(first[f][kept], [1.0, 0.0]), (f, kept)
        assert np.array_equal(first[f][moved], [0.0, 1.0]), (f, moved)


# ---- 6. rectangular ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RECTANGULAR + ("square_consistent", "square_inconsistent"))
def test_rectangular_and_square_systems_of_the_reference(K, ctx, name):
    M, b, c = known_system(name)
    A = _dense(K, ctx, M)
    pair = _dense_pair(M, b, c)
    (xr, sr), _ = pair
    x, st, path = _run(K, ctx, A, b, c, fused=2)
    if name in RECTANGULAR:
        assert M.shape[0] != M.shape[1] and path == 0            # m ≠ n: the primitive sequence, whatever `fused` says
    else:
        assert path == 2
    assert mismatches(st, sr, _pair_budget(pair), x, xr) == []
    assert st.inconsistent == (name in INCONSISTENT)
    if name in CONSISTENT:
        assert st.solved and np.linalg.norm(b - M @ x) <= 1e-6 * np.linalg.norm(b)


def test_row_partitioned_rectangular_handle_is_refused(K, oracle):
    M, b, c = known_system("over_consistent")                      # 25 x 10

    def body(cx, rank):
        r0, r1 = (0, 13) if rank == 0 else (13, 25)
        S = sp.csr_matrix(M[r0:r1])
        S.sort_indices()
        A = K.CsrMatrix.from_host(cx, S.indptr, S.indices, S.data, (r1 - r0, 25), dist_rows=(r0, r1), n_global=25)
        ws = K.UsymqrWorkspace(cx, r1 - r0, 10)
        with pytest.raises(K.KhipError, match="row-partitioned rectangular system") as e:
            K.usymqr_(ws, A, cx.array(b[r0:r1]), cx.array(c), At=lambda x, y: None)
        return e.value.code if hasattr(e.value, "code") else str(e.value)

    res = _run_ranks(K, 2, 977, body)
    assert all(r == -3 or "error -3" in str(r) for r in res), res


# ---- 7. behaviour around the solve ---------------------------------------------------------------------------------------------------
def test_argument_errors(K, ctx, ops):
    S, A, b, c = ops("kron4_sinc")
    n = len(b)
    ws = K.UsymqrWorkspace(ctx, n, n)
    keep = []
    op = K._make_operator(ctx, A, n, keep)
    bd, cd = ctx.array(b), ctx.array(c)
    rc = K.lib().khip_usymqr_solve(ws._h, op, None, bd.ptr, cd.ptr, None)
    assert rc == -1 and "At" in K.lib().khip_last_error().decode()
    rc = K.lib().khip_usymqr_solve(ws._h, op, K._make_operator(ctx, A.transpose(), n, keep), bd.ptr, None, None)
    assert rc == -1 and "c is required" in K.lib().khip_last_error().decode()
    with pytest.raises(K.KhipError, match="c .* is required"):
        K.usymqr_(ws, A, bd)
    small = K.UsymqrWorkspace(ctx, n - 1, n - 1)
    with pytest.raises(K.KhipError, match="inconsistent with size"):
        K.usymqr_(small, A, ctx.array(rhs(n - 1)), ctx.array(rhs(n - 1)))
    with pytest.raises(K.KhipError, match="Inconsistent problem size"):
        K.usymqr_(ws, A, ctx.array(rhs(n - 1)), cd)
    v = [ctx.empty(n) for _ in range(9)]
    v[8] = v[2]
    with pytest.raises(K.KhipError, match="must be distinct"):
        K.UsymqrWorkspace(ctx, n, n, vectors=dict(zip(K.UsymqrWorkspace.VECTORS, v)))


@pytest.mark.parametrize("fused", [0, 1, 2])
def test_warm_start(K, ctx, oracle, ops, fused):
    name = "kron8_shift24_sinc"
    S, A, b, c = ops(name)
    x0 = np.linspace(-0.5, 0.5, len(b))
    x, st, path = _run(K, ctx, A, b, c, fused=fused, x0=x0)
    assert path == fused
    pair = reference_pair(oracle, name, x0=x0)
    (xr, sr), _ = pair
    assert mismatches(st, sr, _pair_budget(pair), x, xr) == []
    assert st.solved


@pytest.mark.parametrize("fused", [0, 1])
def test_callback_sees_both_histories_and_stops(K, ctx, ops, fused):
    S, A, b, c = ops("kron4_sinc")
    seen = []

    def cb(w):
        st = w.stats
        seen.append((len(st.residuals), len(st.Aresiduals)))
        return len(seen) == 3
    x, st, path = _run(K, ctx, A, b, c, fused=fused, callback=cb)
    assert path == fused
    assert seen == [(2, 1), (3, 2), (4, 3)]
    assert st.niter == 3 and st.status == "user-requested exit" and len(st.residuals) == 4 and len(st.Aresiduals) == 3
    _, sr = ur.usymqr(S, b, c, itmax=3)
    assert deviation(st.residuals, sr.residuals, 1e-12) <= 1e-10 and deviation(st.Aresiduals, sr.Aresiduals, 1e-12) <= 1e-10


def test_last_path_and_verbose(K, ctx, ops, tmp_path):
    S, A, b, c = ops("kron4_sinc")
    n = len(b)
    assert _run(K, ctx, A, b, c)[2] == 2
    assert _run(K, ctx, A, b, c, callback=lambda w: False)[2] == 1
    assert _run(K, ctx, A, b, c, At=lambda x, y: A._adjoint.matvec(x, y))[2] == 1     # a user operator
    assert _run(K, ctx, A, b, c, fused=0)[2] == 0
    assert _run(K, ctx, A, b, c, rtol=1.0)[2] == 1               # a loop that never starts reports 1
    log = tmp_path / "usymqr.log"
    with open(log, "w") as f:
        x, st, path = _run(K, ctx, A, b, c, verbose=10, iostream=f)
    assert path == 1
    lines = open(log, encoding="utf-8").read().splitlines()
    assert lines[0] == f"USYMQR: system of {n} equations in {n} variables"
    assert lines[1] == "%5s  %7s  %8s  %5s" % ("k", "‖rₖ‖", "‖Aᴴrₖ₋₁‖", "timer")
    rows = [ln for ln in lines[2:] if ln.strip()]
    assert [int(r.split()[0]) for r in rows] == list(range(0, st.niter + 1, 10))
    assert rows[0].startswith("    0  %7.1e  %8s  " % (st.residuals[0], " ✗ ✗ ✗ ✗"))
    assert rows[1].startswith("   10  %7.1e  %8.1e  " % (st.residuals[10], st.Aresiduals[9]))


def test_path2_history_window_drain(K, ctx, ops):
    name = "kron8_sinc_it60"
    S, A, b, c = ops(name)
    ctx.set_option("hist_window", 8)
    try:
        w2 = _solve(K, ctx, A, b, c, fused=2, itmax=60)
    finally:
        ctx.set_option("hist_window", 1 << 14)
    w1 = _solve(K, ctx, A, b, c, fused=1, itmax=60)
    assert (w1.last_path, w2.last_path) == (1, 2) and w2.stats.niter == 60
    _same_bits(w1, w2)


@pytest.mark.parametrize("world", [2, 3])
def test_row_partitioned(K, ctx, oracle, ops, world):
    name = "kron8_sinc_it60"
    S, A0, b, c = ops(name)
    n = len(b)
    xref, ref, _ = _run(K, ctx, A0, b, c, itmax=60)
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
            ws = K.UsymqrWorkspace(cx, r1 - r0, r1 - r0)
            K.usymqr_(ws, A, cx.array(b[r0:r1]), cx.array(c[r0:r1]), At=At, fused=fused, history=True, itmax=60)
            out[fused] = (ws.stats, ws.last_path, ws.x.to_host())
        return out

    res = _run_ranks(K, world, 960 + world, body)
    for out in res:
        for fused in (2, 1, 0):
            st, path, _ = out[fused]
            assert path == fused
            assert mismatches(st, ref, bud) == []
        assert np.array_equal(out[2][0].residuals, out[1][0].residuals) and np.array_equal(out[2][0].Aresiduals, out[1][0].Aresiduals)
        assert np.array_equal(out[2][0].residuals, res[0][2][0].residuals)
    for fused in (2, 1):
        x = np.concatenate([out[fused][2] for out in res])
        assert np.abs(x - xref).max() <= bud * np.abs(xref).max()
    assert all(np.array_equal(out[2][2], out[1][2]) for out in res)


def test_default_itmax_is_m_plus_n_of_the_global_system(K, ctx):
    """atol = rtol = 0 on gamma2_zero, whose process has broken down: only itmax = m + n = 4 ends the loop."""
    A = _dense(K, ctx, BREAKDOWNS["gamma2_zero"])
    _, sr = ur.usymqr(BREAKDOWNS["gamma2_zero"], BREAKDOWN_B, BREAKDOWN_C, atol=0.0, rtol=0.0)
    for fused in (0, 1, 2):
        x, st, path = _run(K, ctx, A, BREAKDOWN_B, BREAKDOWN_C, fused=fused, atol=0.0, rtol=0.0)
        assert st.niter == sr.niter and st.status == sr.status


def test_no_device_memory_growth(K, ctx, ops):
    S, A, b, c = ops("kron8_sinc_it60")
    bd, cd = ctx.array(b), ctx.array(c)
    ws = K.UsymqrWorkspace(ctx, len(b), len(c), adopt=False)

    def solve(i):
        K.usymqr_(ws, A, bd, cd, fused=(2, 1, 0)[i % 3], history=True, itmax=20)
    for i in range(3):
        solve(i)
    ctx.sync()
    free0 = ctx.mem_info()[0]
    for i in range(20):
        solve(i)
    ctx.sync()
    assert ctx.mem_info()[0] >= free0 - (4 << 20)
