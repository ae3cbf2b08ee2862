"""usymlq! on the GPU: the three loops against the NumPy restatement of src/usymlq.jl (tests/usymlq_reference.py) and against each
other, with the transfer to the USYMCG point on and off.

Budgets (tests/test_usymlq_host.py holds the functions and shows that they reject the injected faults):
  * path 0 (one launch per primitive) against the restatement: same niter, status and flag; the history within budget() =
    max(1e-8, 10 x the case's own np.dot-versus-exact deviation) of each entry, plus the absolute floor 1e-12 x the first entry;
    x within the same budget of max|x|.  Only cases whose own deviation is <= 1e-6 are in the list.
  * path 1 (host-driven, fused kernels) against path 0: elementwise values are the same expressions, the dots differ by <= 1 ulp:
    the same budget.
  * path 2 (device-resident) against path 1 (same kernels, same scalar code): np.array_equal everywhere: x, the history and every
    role of khip_usymlq_vector.
"""
import os
import sys
import threading

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import usymlq_reference as ul  # noqa: E402
from test_bilq_host import other_c, rhs  # noqa: E402
from test_usymlq_host import (BREAKDOWN_B, BREAKDOWN_C, BREAKDOWNS, CASES, EXPECTED, RECTANGULAR, SMALL_SIZES, SOLVED_CG,  # noqa: E402
                              SOLVED_LQ, TIRED, TRANSFERS, UNSYM_BREAKDOWN, budget, case_keywords, case_system, dense_pair, deviation,
                              known_system, mismatches, nonsymmetric_definite, pair_budget, reference_pair)

ROLES = ("u_prev", "u", "p", "x", "dbar", "v_prev", "v", "q")


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


def _solve(K, ctx, A, b, c, fused=2, x0=None, adopt=None, vectors=None, **kw):
    ws = K.UsymlqWorkspace(ctx, len(b), len(c), adopt=adopt, vectors=vectors)
    if x0 is not None:
        ws.warm_start_(ctx.array(x0))
    K.usymlq_(ws, A, ctx.array(b), ctx.array(c), fused=fused, history=True, **kw)
    return ws


def _run(K, ctx, A, b, c, **kw):
    ws = _solve(K, ctx, A, b, c, **kw)
    return ws.x.to_host(), ws.stats, ws.last_path


def _roles(ws):
    return {name: ws.vector(name).to_host() for name in ROLES}


def _same_bits(w1, w2):
    s1, s2 = w1.stats, w2.stats
    assert (s1.niter, s1.status, s1.solved, s1.inconsistent) == (s2.niter, s2.status, s2.solved, s2.inconsistent)
    assert not s2.inconsistent
    assert np.array_equal(s1.residuals, s2.residuals, equal_nan=True) and len(s2.residuals) == s2.niter + 1
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


# ---- 1. path 0 against the restatement, path 1 against path 0, path 2 against path 1: every case, both transfers ------------------
@pytest.mark.parametrize("transfer", TRANSFERS)
@pytest.mark.parametrize("name", list(CASES))
def test_three_paths_on_every_case(K, ctx, oracle, ops, name, transfer):
    S, A, b, c = ops(name)
    (xr, sr), _ = reference_pair(oracle, name, transfer)
    bud = budget(oracle, name, transfer)
    kw = case_keywords(name, transfer)
    w0 = _solve(K, ctx, A, b, c, fused=0, **kw)
    w1 = _solve(K, ctx, A, b, c, fused=1, **kw)
    w2 = _solve(K, ctx, A, b, c, fused=2, **kw)
    assert (w0.last_path, w1.last_path, w2.last_path) == (0, 1, 2)
    x0_, x1 = w0.x.to_host(), w1.x.to_host()
    s0, s1 = w0.stats, w1.stats
    print(f"{name} transfer={transfer}: budget {bud:.2e}; path 0 against the restatement: residuals "
          f"{deviation(s0.residuals, sr.residuals, 1e-12):.2e}, x {np.abs(x0_ - xr).max() / np.abs(xr).max():.2e}; path 1 against path 0: "
          f"residuals {deviation(s1.residuals, s0.residuals, 1e-12):.2e}, x {np.abs(x1 - x0_).max() / np.abs(x0_).max():.2e}")
    assert (s0.niter, s0.status) == EXPECTED[name][0 if transfer else 1]
    assert mismatches(s0, sr, bud, x0_, xr) == []
    assert mismatches(s1, s0, bud, x1, x0_) == []
    _same_bits(w1, w2)
    if "itmax" not in kw:
        assert s0.solved and np.linalg.norm(b - S @ x0_) <= 1e-6 * np.linalg.norm(b)


# ---- 2. path 2 bit-identical to path 1 on every ending ---------------------------------------------------------------------------
def _endings(K, ctx, ops):
    S, A, b, c = ops("kron4_sinc")
    S7, A7, b7, c7 = ops("kron7_shift24_sinc")
    Ab, bb, cb = UNSYM_BREAKDOWN
    out = {  # ending -> (A, b, c, keywords, status, niter, runs the loop)
        "solved_lq": (A7, b7, c7, dict(transfer_to_usymcg=False), SOLVED_LQ, 28, True),
        "solved_cg": (A, b, c, {}, SOLVED_CG, 50, True),
        "b_zero": (A, np.zeros(len(b)), c, {}, "x is a zero-residual solution", 0, False),
        "timemax": (A, b, c, dict(timemax=1e-9), "time limit exceeded", 1, True),
        "unsymmetric_breakdown": (_dense(K, ctx, Ab), bb, cb, {}, SOLVED_CG, 2, True),
        "unsymmetric_breakdown_lq": (_dense(K, ctx, Ab), bb, cb, dict(transfer_to_usymcg=False), SOLVED_LQ, 2, True),
    }
    for k in (1, 2, 3, 4, 5, 9):                                 # both sides of the chunk of four enqueued iterations
        out[f"itmax{k}"] = (A, b, c, dict(itmax=k), TIRED, k, True)
    return out


@pytest.mark.parametrize("ending", ["solved_lq", "solved_cg", "b_zero", "timemax", "unsymmetric_breakdown", "unsymmetric_breakdown_lq",
                                    "itmax1", "itmax2", "itmax3", "itmax4", "itmax5", "itmax9"])
def test_path2_is_bit_identical_to_path1(K, ctx, ops, ending):
    A, b, c, kw, status, niter, loops = _endings(K, ctx, ops)[ending]
    w1 = _solve(K, ctx, A, b, c, fused=1, **kw)
    w2 = _solve(K, ctx, A, b, c, fused=2, **kw)
    assert w1.last_path == 1 and w2.last_path == (2 if loops else 1)
    _same_bits(w1, w2)
    s2 = w2.stats
    assert s2.status == status and s2.niter == niter, (s2.status, s2.niter)
    assert s2.solved == (ending in ("solved_lq", "solved_cg", "b_zero") or ending.startswith("unsymmetric"))


@pytest.mark.parametrize("fused", [0, 1, 2])
@pytest.mark.parametrize("transfer", TRANSFERS)
def test_unsymmetric_breakdown(K, ctx, fused, transfer):
    """A = [0 1; −1 0], b = e₁, c = −e₁: δbar₁ = 0 exactly, so the guard skips the transfer at k = 1 (no ζbar = 1 / 0); the solve ends
    at k = 2 with x = e₂, finite everywhere."""
    Ab, bb, cb = UNSYM_BREAKDOWN
    pair = dense_pair(Ab, bb, cb, transfer_to_usymcg=transfer)
    (xr, sr), _ = pair
    x, st, path = _run(K, ctx, _dense(K, ctx, Ab), bb, cb, fused=fused, transfer_to_usymcg=transfer)
    assert path == fused and st.niter == 2 and st.solved
    assert mismatches(st, sr, pair_budget(pair), x, xr) == []
    assert np.isfinite(x).all() and np.isfinite(st.residuals).all()
    assert np.allclose(x, [0.0, 1.0], atol=1e-15, rtol=0.0)


@pytest.mark.parametrize("itmax", [1, 2, 3, 7])
@pytest.mark.parametrize("fused", [1, 2])
def test_roles_hold_the_reference_variables(K, ctx, oracle, ops, itmax, fused):
    """After k iterations every name of khip_usymlq_vector holds what the reference's variable of that name holds at the end of the
    loop (dbar = d̅ₖ, which is u₁ after one iteration), for both parities of the rotations."""
    S, A, b, c = ops("kron7_it60")
    ws = _solve(K, ctx, A, b, c, fused=fused, itmax=itmax)
    assert ws.last_path == fused and ws.stats.niter == itmax
    pair = reference_pair(oracle, "kron7_it60", True, itmax=itmax)
    bud = pair_budget(pair)
    (xr, sr), _ = pair
    got = _roles(ws)
    for name in ROLES:
        want = xr if name == "x" else sr.vectors[name]
        dev = np.abs(got[name] - want).max() / max(np.abs(want).max(), 1e-300)
        print(f"{name}: largest deviation {dev:.3e} of its largest entry")
        assert dev <= bud, name
    if itmax == 1:
        assert np.array_equal(got["dbar"], got["u_prev"]) and not got["x"].any()          # d̅₁ = u₁, x₁ = 0
    assert len({ws.vector(name).ptr for name in ROLES}) == len(ROLES)


# ---- 3. shapes where the passes can go wrong -------------------------------------------------------------------------------------
@pytest.mark.parametrize("transfer", TRANSFERS)
@pytest.mark.parametrize("n", SMALL_SIZES)
def test_small_dense_systems(K, ctx, n, transfer):
    """nonsymmetric_definite(n): one lane, one pair, one wave less one, one wave, one wave and the tail.  n = 1 ends at k = 1 by
    the transfer with β₂ = γ₂ = 0: both guards keep v and u."""
    M, b = nonsymmetric_definite(n)
    c = other_c(n)
    pair = dense_pair(M, b, c, transfer_to_usymcg=transfer)
    (xr, sr), _ = pair
    bud = pair_budget(pair)
    A = _dense(K, ctx, M)
    w0, w1, w2 = (_solve(K, ctx, A, b, c, fused=f, transfer_to_usymcg=transfer) for f in (0, 1, 2))
    assert (w0.last_path, w1.last_path, w2.last_path) == (0, 1, 2)
    assert mismatches(w0.stats, sr, bud, w0.x.to_host(), xr) == []
    assert mismatches(w1.stats, w0.stats, bud, w1.x.to_host(), w0.x.to_host()) == []
    _same_bits(w1, w2)
    assert w2.stats.solved
    if n == 1 and transfer:
        for w in (w0, w1, w2):
            r = _roles(w)
            assert w.stats.niter == 1 and w.stats.status == SOLVED_CG
            assert np.array_equal(r["v"], r["v_prev"]) and np.array_equal(r["u"], r["u_prev"])
            assert np.array_equal(r["v"], [1.0]) and np.array_equal(r["u"], [1.0]) and np.array_equal(r["dbar"], [1.0])


def test_sizes_of_the_case_list():
    """343 (one workgroup of pairs plus the odd tail), 729 and 1331 (several plus the tail), 512 (exactly one), 1728, 4096 are all
    in the list that test_three_paths_on_every_case walks."""
    sizes = {CASES[k][1] ** 3 for k in CASES}
    assert {343, 729, 1331, 512, 1728, 4096} <= sizes and max(sizes) <= 4096 and len(CASES) >= 12


# ---- 4. instantiations -------------------------------------------------------------------------------------------------------------
NVEC = 8


def _carved(K, ctx, n, first):
    """The eight vectors of a workspace inside one buffer, starting at element `first` with an even stride: first = 1 puts every
    vector at an odd element offset (8-byte but not 16-byte aligned), first = 0 keeps them 16-byte aligned."""
    stride = n + 2 - (n & 1) + 2
    buf = ctx.zeros(first + NVEC * stride)
    assert buf.ptr % 16 == 0
    vec = {k: buf.slice(first + i * stride, first + i * stride + n) for i, k in enumerate(K.UsymlqWorkspace.VECTORS)}
    assert all(v.ptr % 16 == 8 * first for v in vec.values())
    return buf, vec


@pytest.mark.parametrize("name", ["kron8_sinc_it60", "kron7_it60"])
def test_adopted_vectors_at_odd_offsets(K, ctx, oracle, ops, name):
    """The 8-byte kernel path (and, with n = 343, the 16-byte path's tail element beside it): bit-identical to an owned workspace
    and to a 16-byte-aligned adoption under path 2, within budget of path 0; nothing is written between the carved vectors."""
    S, A, b, c = ops(name)
    n = len(b)
    kw = case_keywords(name, True)
    xo, so, po = _run(K, ctx, A, b, c, adopt=False, **kw)
    buf1, odd = _carved(K, ctx, n, 1)
    x1, s1, p1 = _run(K, ctx, A, b, c, vectors=odd, **kw)
    buf0, even = _carved(K, ctx, n, 0)
    x0_, s0, p0 = _run(K, ctx, A, b, c, vectors=even, **kw)
    assert (po, p1, p0) == (2, 2, 2)
    for x, s in ((x1, s1), (x0_, s0)):
        assert s.niter == so.niter and s.status == so.status
        assert np.array_equal(s.residuals, so.residuals) and np.array_equal(x, xo)
    xp, sp0, pp = _run(K, ctx, A, b, c, fused=0, **kw)
    assert pp == 0 and mismatches(s1, sp0, budget(oracle, name), x1, xp) == []
    stride = n + 2 - (n & 1) + 2
    for first, buf in ((1, buf1), (0, buf0)):
        h = buf.to_host()
        gaps = np.ones(len(h), dtype=bool)
        for i in range(NVEC):
            gaps[first + i * stride:first + i * stride + n] = False
        assert not h[gaps].any(), "a kernel wrote outside its vectors"


def test_eight_byte_path_after_two_iterations(K, ctx, oracle, ops):
    """Two iterations from the same state (the second runs the x and d̅ updates), on 16-byte vectors and on vectors carved at
    element offset 1 (the 8-byte instantiations): the two fused runs agree in every bit of every role.  Against path 0, after one
    iteration the roles that pass through no reduction of the loop (v₁, u₁, d̅₁, x₁) are bit-identical; after two every role is the
    same expression of scalars that differ by the reductions' last bit, and lies within the budget of the two-iteration case."""
    S, A, b, c = ops("kron4_sinc")
    _, odd1 = _carved(K, ctx, len(b), 1)
    f0, f1, f8 = (_roles(_solve(K, ctx, A, b, c, itmax=1, **kw)) for kw in (dict(fused=0), dict(fused=1), dict(fused=1, vectors=odd1)))
    for name in ROLES:
        assert np.array_equal(f1[name], f8[name]), name
    for name in ("v_prev", "u_prev", "dbar", "x"):                 # v₁, u₁, d̅₁ = u₁ and x₁ = 0 pass through no reduction of the loop
        assert np.array_equal(f0[name], f1[name]), name
    w0 = _solve(K, ctx, A, b, c, fused=0, itmax=2)
    w1 = _solve(K, ctx, A, b, c, fused=1, itmax=2)
    _, odd = _carved(K, ctx, len(b), 1)
    w8 = _solve(K, ctx, A, b, c, fused=1, itmax=2, vectors=odd)
    r0, r1, r8 = _roles(w0), _roles(w1), _roles(w8)
    bud = pair_budget(reference_pair(oracle, "kron4_sinc", True, itmax=2))
    for name in ROLES:
        assert np.array_equal(r1[name], r8[name]), name
        dev = np.abs(r0[name] - r1[name]).max() / np.abs(r0[name]).max()
        print(f"{name}: path 1 against path 0 {dev:.2e} of the largest entry ({'same bits' if dev == 0 else 'not the same bits'})")
        assert dev <= bud, name


def test_nt_and_compensated_instantiations(K, ctx, oracle, ops):
    name = "kron8_sinc_it60"
    S, A, b, c = ops(name)
    kw = case_keywords(name, True)
    xd, sd, _ = _run(K, ctx, A, b, c, **kw)
    keep = ctx.get_option("nt_min_elems")
    assert keep > len(b)
    ctx.set_option("nt_min_elems", 1)
    try:
        wn = _solve(K, ctx, A, b, c, **kw)
        xn, sn, pn = wn.x.to_host(), wn.stats, wn.last_path
        dn = wn.vector("dbar").to_host()
    finally:
        ctx.set_option("nt_min_elems", keep)
    assert pn == 2 and np.array_equal(xn, xd) and np.array_equal(sn.residuals, sd.residuals)
    assert np.array_equal(dn, _solve(K, ctx, A, b, c, **kw).vector("dbar").to_host())
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
    vec = {k: ctx.empty(n) for k in K.UsymlqWorkspace.VECTORS}
    ws = K.UsymlqWorkspace(ctx, n, n, vectors=vec)
    K.usymlq_(ws, A, ctx.array(b), ctx.array(c), history=True, itmax=60)
    assert ws.x is vec["x"] and ws.last_path == 2              # solution(ws) is the caller's x
    xo, so, _ = _run(K, ctx, A, b, c, adopt=False, itmax=60)
    assert np.array_equal(vec["x"].to_host(), xo) and np.array_equal(ws.stats.residuals, so.residuals)
    assert ws.stats.niter == so.niter
    assert K.UsymlqWorkspace(ctx, n, n, adopt=False).nbytes == 8 * 8 * n
    assert K.UsymlqWorkspace(ctx, 25, 10, adopt=False).nbytes == 8 * (5 * 10 + 3 * 25)
    assert K.UsymlqWorkspace(ctx, 10, 25, adopt=False).nbytes == 8 * (5 * 25 + 3 * 10)
    assert A._adjoint is not None and K._adjoint_of(A) is A._adjoint     # A' is taken once and kept on the matrix
    x, st, ws2 = K.usymlq(A, ctx.array(b), ctx.array(c), history=True, itmax=60)
    assert ws2.last_path == 2                                  # the out-of-place entry forwards the default callback
    assert np.array_equal(x.to_host(), xo) and np.array_equal(st.residuals, so.residuals)
    ws3 = K.krylov_workspace("usymlq", A, ctx.array(b), ctx.array(c))
    assert isinstance(ws3, K.UsymlqWorkspace)
    K.krylov_solve_(ws3, A, ctx.array(b), c=ctx.array(c), history=True, itmax=60)
    assert ws3.last_path == 2 and np.array_equal(ws3.x.to_host(), xo)
    x, st, ws4 = K.krylov_solve("usymlq", A, ctx.array(b), c=ctx.array(c), history=True, itmax=40, transfer_to_usymcg=False)
    assert ws4.last_path == 2 and st.niter == 40
    assert np.array_equal(x.to_host(), _run(K, ctx, A, b, c, itmax=40, transfer_to_usymcg=False)[0])


# ---- 5. breakdown on one side -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(BREAKDOWNS))
def test_breakdown_on_one_side(K, ctx, name):
    """β₂ = 0 exactly keeps vₖ, γ₂ = 0 exactly keeps uₖ, each without the other: the same on all three paths."""
    M = BREAKDOWNS[name]
    A = _dense(K, ctx, M)
    for transfer in TRANSFERS:
        pair = dense_pair(M, BREAKDOWN_B, BREAKDOWN_C, transfer_to_usymcg=transfer)
        (xr, sr), _ = pair
        w = {f: _solve(K, ctx, A, BREAKDOWN_B, BREAKDOWN_C, fused=f, transfer_to_usymcg=transfer) for f in (0, 1, 2)}
        for f in (0, 1, 2):
            assert w[f].last_path == f
            assert mismatches(w[f].stats, sr, pair_budget(pair), w[f].x.to_host(), xr) == [], (f, transfer)
        _same_bits(w[1], w[2])
    first = {f: _roles(_solve(K, ctx, A, BREAKDOWN_B, BREAKDOWN_C, fused=f, itmax=1, transfer_to_usymcg=False)) for f in (0, 1, 2)}
    for f in (0, 1, 2):
        kept, moved = ("v", "u") if name == "beta2_zero" else ("u", "v")
        assert np.array_equal(first[f][kept], first[f][kept + "_prev"]) and np.array_equal(first[f][kept], [1.0, 0.0]), (f, kept)
        assert np.array_equal(first[f][moved], [0.0, 1.0]), (f, moved)
        assert np.array_equal(first[f]["dbar"], [1.0, 0.0]), f


# ---- 6. rectangular ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RECTANGULAR + ("square_consistent",))
def test_rectangular_and_square_systems_of_the_reference(K, ctx, name):
    M, b, c = known_system(name)
    A = _dense(K, ctx, M)
    pair = dense_pair(M, b, c)
    (xr, sr), _ = pair
    x, st, path = _run(K, ctx, A, b, c, fused=2)
    if name in RECTANGULAR:
        assert M.shape[0] != M.shape[1] and path == 0            # m ≠ n: the primitive sequence, whatever `fused` says
    else:
        assert path == 2
    assert mismatches(st, sr, pair_budget(pair), x, xr) == []
    assert st.solved and not st.inconsistent and np.linalg.norm(b - M @ x) <= 1e-6 * np.linalg.norm(b)
    if name in RECTANGULAR:                                      # without the transfer only itmax = m + n ends the loop
        x, st, path = _run(K, ctx, A, b, c, fused=2, transfer_to_usymcg=False)
        assert path == 0 and st.niter == sum(M.shape) and st.status == TIRED and not st.inconsistent


def test_row_partitioned_rectangular_handle_is_refused(K, oracle):
    M, b, c = known_system("over_consistent")                      # 25 x 10

    def body(cx, rank):
        r0, r1 = (0, 13) if rank == 0 else (13, 25)
        S = sp.csr_matrix(M[r0:r1])
        S.sort_indices()
        A = K.CsrMatrix.from_host(cx, S.indptr, S.indices, S.data, (r1 - r0, 25), dist_rows=(r0, r1), n_global=25)
        ws = K.UsymlqWorkspace(cx, r1 - r0, 10)
        with pytest.raises(K.KhipError, match="row-partitioned rectangular system") as e:
            K.usymlq_(ws, A, cx.array(b[r0:r1]), cx.array(c), At=lambda x, y: None)
        return e.value.code if hasattr(e.value, "code") else str(e.value)

    res = _run_ranks(K, 2, 978, body)
    assert all(r == -3 or "error -3" in str(r) for r in res), res


# ---- 7. behaviour around the solve ---------------------------------------------------------------------------------------------------
def test_argument_errors(K, ctx, ops):
    S, A, b, c = ops("kron4_sinc")
    n = len(b)
    ws = K.UsymlqWorkspace(ctx, n, n)
    keep = []
    op = K._make_operator(ctx, A, n, keep)
    bd, cd = ctx.array(b), ctx.array(c)
    rc = K.lib().khip_usymlq_solve(ws._h, op, None, bd.ptr, cd.ptr, None, None)
    assert rc == -1 and "At" in K.lib().khip_last_error().decode()
    rc = K.lib().khip_usymlq_solve(ws._h, op, K._make_operator(ctx, A.transpose(), n, keep), bd.ptr, None, None, None)
    assert rc == -1 and "c is required" in K.lib().khip_last_error().decode()
    with pytest.raises(K.KhipError, match="c .* is required"):
        K.usymlq_(ws, A, bd)
    with pytest.raises(K.KhipError, match="c .* is required"):
        K.krylov_solve("usymlq", A, bd)
    small = K.UsymlqWorkspace(ctx, n - 1, n - 1)
    with pytest.raises(K.KhipError, match="inconsistent with size"):
        K.usymlq_(small, A, ctx.array(rhs(n - 1)), ctx.array(rhs(n - 1)))
    with pytest.raises(K.KhipError, match="Inconsistent problem size"):
        K.usymlq_(ws, A, ctx.array(rhs(n - 1)), cd)
    with pytest.raises(K.KhipError, match="Inconsistent problem size"):
        K.usymlq_(ws, A, bd, ctx.array(rhs(n - 1)))
    v = [ctx.empty(n) for _ in range(NVEC)]
    v[7] = v[2]
    with pytest.raises(K.KhipError, match="must be distinct"):
        K.UsymlqWorkspace(ctx, n, n, vectors=dict(zip(K.UsymlqWorkspace.VECTORS, v)))


@pytest.mark.parametrize("fused", [0, 1, 2])
def test_warm_start(K, ctx, oracle, ops, fused):
    name = "kron8_shift24_sinc"
    S, A, b, c = ops(name)
    x0 = np.linspace(-0.5, 0.5, len(b))
    x, st, path = _run(K, ctx, A, b, c, fused=fused, x0=x0)
    assert path == fused
    pair = reference_pair(oracle, name, True, x0=x0)
    (xr, sr), _ = pair
    assert mismatches(st, sr, pair_budget(pair), x, xr) == []
    assert st.solved and np.linalg.norm(b - S @ x) <= 1e-6 * np.linalg.norm(b)


@pytest.mark.parametrize("fused", [0, 1])
def test_callback_sees_the_history_and_stops(K, ctx, ops, fused):
    S, A, b, c = ops("kron4_sinc")
    seen = []

    def cb(w):
        seen.append(len(w.stats.residuals))
        return len(seen) == 3
    x, st, path = _run(K, ctx, A, b, c, fused=fused, callback=cb)
    assert path == fused
    assert seen == [2, 3, 4]
    assert st.niter == 3 and st.status == "user-requested exit" and len(st.residuals) == 4 and not st.solved
    xr, sr = ul.usymlq(S, b, c, itmax=3)
    assert deviation(st.residuals, sr.residuals, 1e-12) <= 1e-10 and np.abs(x - xr).max() <= 1e-10 * np.abs(xr).max()


def test_last_path_and_verbose(K, ctx, ops, tmp_path):
    S, A, b, c = ops("kron4_sinc")
    n = len(b)
    assert _run(K, ctx, A, b, c)[2] == 2
    assert _run(K, ctx, A, b, c, callback=lambda w: False)[2] == 1
    assert _run(K, ctx, A, b, c, At=lambda x, y: A._adjoint.matvec(x, y))[2] == 1     # a user operator
    assert _run(K, ctx, A, b, c, fused=0)[2] == 0
    assert _run(K, ctx, A, b, c, rtol=1.0)[2] == 1               # a loop that never starts reports 1
    assert _run(K, ctx, A, b, c, rtol=1.0, fused=0)[2] == 0
    log = tmp_path / "usymlq.log"
    with open(log, "w") as f:
        x, st, path = _run(K, ctx, A, b, c, verbose=10, iostream=f)
    assert path == 1
    lines = open(log, encoding="utf-8").read().splitlines()
    assert lines[0] == f"USYMLQ: system of {n} equations in {n} variables"
    assert lines[1] == "%5s  %7s  %5s" % ("k", "‖rₖ‖", "timer")
    rows = [ln for ln in lines[2:] if ln.strip()]
    assert [int(r.split()[0]) for r in rows] == list(range(0, st.niter + 1, 10))
    assert rows[0].startswith("    0  %7.1e  " % st.residuals[0]) and rows[0].endswith("s")
    assert rows[1].startswith("   10  %7.1e  " % st.residuals[10]) and len(rows[1].split()) == 3


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
            ws = K.UsymlqWorkspace(cx, r1 - r0, r1 - r0)
            K.usymlq_(ws, A, cx.array(b[r0:r1]), cx.array(c[r0:r1]), At=At, fused=fused, history=True, itmax=60)
            out[fused] = (ws.stats, ws.last_path, ws.x.to_host())
        return out

    res = _run_ranks(K, world, 970 + world, body)
    for out in res:
        for fused in (2, 1, 0):
            st, path, _ = out[fused]
            assert path == fused
            assert mismatches(st, ref, bud) == []
        assert np.array_equal(out[2][0].residuals, out[1][0].residuals)
        assert np.array_equal(out[2][0].residuals, res[0][2][0].residuals)
    for fused in (2, 1):
        x = np.concatenate([out[fused][2] for out in res])
        assert np.abs(x - xref).max() <= bud * np.abs(xref).max()
    assert all(np.array_equal(out[2][2], out[1][2]) for out in res)


def test_default_itmax_is_m_plus_n_of_the_global_system(K, ctx, ops):
    """atol = rtol = 0: only itmax = m + n ends the loop, on gamma2_zero (4, whose process has broken down) and on kron4 (128)."""
    A = _dense(K, ctx, BREAKDOWNS["gamma2_zero"])
    _, sr = ul.usymlq(BREAKDOWNS["gamma2_zero"], BREAKDOWN_B, BREAKDOWN_C, atol=0.0, rtol=0.0)
    assert sr.niter == 4 and sr.status == TIRED
    for fused in (0, 1, 2):
        x, st, path = _run(K, ctx, A, BREAKDOWN_B, BREAKDOWN_C, fused=fused, atol=0.0, rtol=0.0)
        assert st.niter == sr.niter and st.status == sr.status
    S, A4, b, c = ops("kron4_sinc")
    x, st, path = _run(K, ctx, A4, b, c, atol=0.0, rtol=0.0, transfer_to_usymcg=False)
    assert path == 2 and st.niter == 2 * len(b) and st.status == TIRED


def test_no_device_memory_growth(K, ctx, ops):
    S, A, b, c = ops("kron8_sinc_it60")
    bd, cd = ctx.array(b), ctx.array(c)
    ws = K.UsymlqWorkspace(ctx, len(b), len(c), adopt=False)

    def solve(i):
        K.usymlq_(ws, A, bd, cd, fused=(2, 1, 0)[i % 3], history=True, itmax=20)
    for i in range(3):
        solve(i)
    ctx.sync()
    free0 = ctx.mem_info()[0]
    for i in range(20):
        solve(i)
    ctx.sync()
    assert ctx.mem_info()[0] >= free0 - (4 << 20)


def test_profile_bracket_counts_one_p3_per_iteration(K, ctx, ops):
    """The `usymlq_p3` bracket: one launch per iteration on the host-driven loop and per enqueued iteration on the device-resident
    one (itmax = 8 is two full chunks), beside one of each shared pass; usymqr!'s P3 bracket stays empty."""
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
        assert prof["usymlq_p3"][0] == itmax and prof["usymlq_p3"][1] > 0.0, prof
        assert prof["ssy_p1"][0] == itmax and prof["ssy_p2"][0] == itmax and prof["usymqr_p3"][0] == 0, prof
