"""The opt-in loops cg!(variant = 1 | 2) and gmres!(variant = 1 | 2) against their own recurrences.

cg!(variant = 1), cg!(variant = 2) and gmres!(variant = 1) are held to the NumPy restatements of tests/variants_reference.py
(pinned to the oracle in tests/test_variants_host.py) on the case lists of that file.  The budget is the convention of
tests/test_gpu_qmr.py, MEASURED per case on the restatement itself: its history with np.dot against its history with exactly
summed dots, times 10, at least 1e-8, plus 1e-12 r_0; x (and every work vector) within that of its own max|.|.  Every comparison
prints the observed deviation and its budget and sends both to parity_log.

What the even lengths and library-owned vectors of the first tests of the variants never ran: n = 343, 511, 513 on workspaces
adopted on vectors carved at element offset 0 and 1 (the odd tail element and the 8-byte instantiation of cgcg_update_kernel,
pcg_update_kernel, multi_dot4_kernel, multi_axpy_dev_kernel), the work vectors role by role after 1, 2, 3 and 6 iterations, the
ways a solve ends, and for CGS2 the orthogonality of the basis it leaves, with every entry of V'V an exactly summed dot: a tail
element lost in both passes leaves an error of order 1 / n, ten orders of magnitude above the bound.

gmres!(variant = 2) (s-step) has no restatement (its Hessenberg recovery is host code): it is held to its own bits under cache
hints, to the 16-byte path at odd offsets (tests/test_gpu_vec_dispatch.py) and to the true residual of a converged solve."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_reduction as er  # noqa: E402
import variants_reference as vr  # noqa: E402
from test_gpu_vec_dispatch import _Options, _carved, _check_solver  # noqa: E402
from test_variants_host import CG_CASES, GMRES_CASES, RESTATEMENT, case_matrix, case_rhs, reference_pair  # noqa: E402

HIST_RTOL = 1e-8
HIST_FLOOR = 1e-12
CG_ROLES = ("x", "r", "p", "Ap", "z")
ODD = {343: ("poisson", 7), 511: ("tridiagonal", 511), 513: ("tridiagonal", 513)}       # n -> operator of the odd-length runs
_DEV = {}


def _upload(K, ctx, oracle, kind, size):
    if (kind, size) not in _DEV:
        S = case_matrix(oracle, kind, size)
        _DEV[(kind, size)] = K.CsrMatrix.from_host(ctx, S.indptr.astype(np.int64), S.indices.astype(np.int32), S.data, S.shape)
    return _DEV[(kind, size)]


def _from_dense(K, ctx, M):
    import scipy.sparse as sp
    S = sp.csr_matrix(np.asarray(M, dtype=np.float64))
    S.sort_indices()
    return K.CsrMatrix.from_host(ctx, S.indptr.astype(np.int64), S.indices.astype(np.int32), S.data, S.shape)


def _budget(pair):
    """10 x the restatement's own sensitivity to the rounding of its dots (at least HIST_RTOL)"""
    (_, s1), (_, s2) = pair
    return max(HIST_RTOL, 10.0 * vr.history_deviation(s1.residuals, s2.residuals))


def _hist_ok(log, what, a, b, rtol):
    a, b = np.asarray(a), np.asarray(b)
    with np.errstate(invalid="ignore", divide="ignore"):       # (a zero entry of the reference is judged by the floor below)
        dev = np.nan_to_num(np.abs(a - b) / np.abs(b), nan=0.0, posinf=0.0) if a.shape == b.shape else np.array([np.inf])
    print(f"{what}: history of {len(a)} entries, largest relative deviation {dev.max():.3e}, budget {rtol:.3e}")
    log(test="variants", what=what, quantity="history", deviation=float(dev.max()), budget=float(rtol))
    return a.shape == b.shape and bool(np.all(np.abs(a - b) <= rtol * np.abs(b) + HIST_FLOOR * b[0]))


def _vec_ok(log, what, role, v, vr_, rtol):
    scale = float(np.abs(vr_).max())
    dev = float(np.abs(v - vr_).max())
    print(f"{what}: {role} largest deviation {dev:.3e} of max {scale:.3e}, budget {max(1e-8, rtol):.3e}")
    log(test="variants", what=what, quantity=role, deviation=dev / scale if scale else dev, budget=float(max(1e-8, rtol)))
    return bool(np.all(np.abs(v - vr_) <= max(1e-8, rtol) * scale))


def _cg_workspace(K, ctx, n, first=None):
    """first = None: the mirror's own workspace; else x, r, p, Ap and z on vectors carved at element offset `first` (the
    pipelined variant's pz / pq stay library-owned: its pass then sees mixed alignment and takes the 8-byte path)"""
    if first is None:
        return K.CgWorkspace(ctx, n, n)
    buf, v = _carved(ctx, n, CG_ROLES, first)
    ws = K.CgWorkspace.__new__(K.CgWorkspace)
    ws.ctx, ws.m, ws.n, ws.adopted, ws._alloc_s, ws._h, ws._buf = ctx, n, n, True, 0.0, C.c_void_p(), buf
    ws._vec = {k: v[k] for k in ("x", "r", "p", "Ap")}
    assert K.lib().khip_cg_workspace_adopt(ctx._h, n, n, *[v[k].ptr for k in ("x", "r", "p", "Ap")], C.byref(ws._h)) == 0
    ws._adopt_vector("z", v["z"])
    return ws


def _cg(K, ctx, dA, b, variant, first=None, x0=None, **kw):
    """one solve -> (workspace, stats, x on the host)"""
    ws = _cg_workspace(K, ctx, len(b), first)
    if x0 is not None:
        ws.warm_start_(ctx.array(x0))
    K.cg_(ws, dA, ctx.array(b), variant=variant, history=True, **kw)
    st = ws.stats
    assert ws.last_path == (-1 if st.status == vr.ZERO_RESIDUAL else 1)      # b = 0 returns before a loop is chosen: "none yet"
    return ws, st, ws.x.to_host()


# ---- cg!(variant = 1 | 2) -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CG_CASES))
@pytest.mark.parametrize("variant", [1, 2])
def test_cg_variant_against_its_restatement(K, ctx, oracle, parity_log, variant, name):
    kind, size, which, kw = CG_CASES[name]
    pair = reference_pair(oracle, variant, name)
    (xr, sr), _ = pair
    rtol = _budget(pair)
    dA = _upload(K, ctx, oracle, kind, size)
    ws, st, x = _cg(K, ctx, dA, case_rhs(dA.shape[0], which), variant)
    what = f"cg variant {variant} {name}"
    assert (st.niter, st.status, st.solved) == (sr.niter, sr.status, sr.solved), (what, st.niter, st.status, sr.niter, sr.status)
    assert _hist_ok(parity_log, what, st.residuals, sr.residuals, rtol)
    assert _vec_ok(parity_log, what, "x", x, xr, rtol)


@pytest.mark.parametrize("variant", [1, 2])
def test_cg_variant_warm_start(K, ctx, oracle, parity_log, variant):
    S = case_matrix(oracle, "poisson", 7)
    b = case_rhs(S.shape[0], "cos")
    (xs, _), _ = reference_pair(oracle, variant, "poisson7_cos")
    x0 = xs * (1 + 1e-3 * np.cos(np.arange(xs.size)))
    pair = (RESTATEMENT[variant](S, b, x0=x0), RESTATEMENT[variant](S, b, x0=x0, dot=vr.fsum_dot))
    (xr, sr), _ = pair
    ws, st, x = _cg(K, ctx, _upload(K, ctx, oracle, "poisson", 7), b, variant, x0=x0)
    what = f"cg variant {variant} warm start"
    assert (st.niter, st.status, st.solved) == (sr.niter, sr.status, sr.solved)
    assert _hist_ok(parity_log, what, st.residuals, sr.residuals, _budget(pair))
    assert _vec_ok(parity_log, what, "x", x, xr, _budget(pair))


@pytest.mark.parametrize("itmax", [1, 2, 3, 6])
@pytest.mark.parametrize("variant", [1, 2])
def test_cg_variant_roles(K, ctx, oracle, parity_log, variant, itmax):
    """x, r, p, Ap (= s) and z (= w) of khip_cg_vector after `itmax` iterations against the restatement's vectors of those
    names.  Variant 2's pz / pq have no accessor: an error in its z reaches w one iteration later, which itmax = 6 covers."""
    for name in ("poisson7_cos", "tridiagonal513_cos"):
        kind, size, which, kw = CG_CASES[name]
        pair = reference_pair(oracle, variant, name, itmax=itmax)
        (xr, sr), _ = pair
        rtol = _budget(pair)
        dA = _upload(K, ctx, oracle, kind, size)
        ws, st, x = _cg(K, ctx, dA, case_rhs(dA.shape[0], which), variant, itmax=itmax)
        what = f"cg variant {variant} {name} itmax={itmax}"
        assert (st.niter, st.status, st.solved) == (itmax, vr.TIRED, False) == (sr.niter, sr.status, sr.solved)
        assert _hist_ok(parity_log, what, st.residuals, sr.residuals, rtol)
        for role in CG_ROLES:
            assert _vec_ok(parity_log, what, role, ws.vector(role).to_host(), sr.vectors[role], rtol), (what, role)


@pytest.mark.parametrize("n", sorted(ODD))
@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("variant", [1, 2])
def test_cg_variant_on_odd_lengths_and_offsets(K, ctx, oracle, parity_log, variant, first, n):
    kind, size = ODD[n]
    name = f"{kind}{size}_cos"
    dA = _upload(K, ctx, oracle, kind, size)
    b = case_rhs(n, "cos")
    what = f"cg variant {variant} {name} offset {first}"
    # a whole solve and six iterations, each held to the restatement; after six iterations role by role (at convergence r, p, s
    # and w are 1e-7 of what they were and carry the rounding of the early iterations, which the history's sensitivity does
    # not measure: the pipelined variant recurs r and w instead of recomputing them)
    for extra in (dict(), dict(itmax=6)):
        pair = reference_pair(oracle, variant, name, **extra)
        (xr, sr), _ = pair
        rtol = _budget(pair)
        ws, st, x = _cg(K, ctx, dA, b, variant, first=first, **extra)
        assert all(ws.vector(k).ptr % 16 == 8 * first for k in CG_ROLES)
        assert (st.niter, st.status, st.solved) == (sr.niter, sr.status, sr.solved), (what, extra)
        assert _hist_ok(parity_log, f"{what} {extra}", st.residuals, sr.residuals, rtol)
        for role in (CG_ROLES if extra else ("x",)):
            assert _vec_ok(parity_log, f"{what} {extra}", role, ws.vector(role).to_host(), sr.vectors[role], rtol), (what, extra, role)
        # cache hints change no arithmetic: the same bits
        with _Options(ctx, nt_min_elems=1):
            ws2, st2, x2 = _cg(K, ctx, dA, b, variant, first=first, **extra)
        assert (st2.niter, st2.status) == (st.niter, st.status) and x2.tobytes() == x.tobytes(), (what, extra)
        assert np.asarray(st2.residuals).tobytes() == np.asarray(st.residuals).tobytes(), (what, extra)
        for role in CG_ROLES:
            assert ws2.vector(role).to_host().tobytes() == ws.vector(role).to_host().tobytes(), (what, extra, role)
    # plain accumulation of the dots: against the restatement with np.dot
    pair = reference_pair(oracle, variant, name)
    (xr, sr), _ = pair
    with _Options(ctx, compensated=0):
        ws, st, x = _cg(K, ctx, dA, b, variant, first=first)
    assert (st.niter, st.status, st.solved) == (sr.niter, sr.status, sr.solved), what
    assert _hist_ok(parity_log, what + " compensated=0", st.residuals, sr.residuals, _budget(pair))
    assert _vec_ok(parity_log, what + " compensated=0", "x", x, xr, _budget(pair))


@pytest.mark.parametrize("variant", [1, 2])
def test_cg_variant_endings(K, ctx, parity_log, variant):
    """a 2 x 2 system and n = 1: itmax reached after one iteration, a zero right-hand side, an indefinite diagonal operator
    refused at the delta_0 test (KHIP_ERR_NUMERIC) and the breakdown flag in the middle of a solve -- status and x as the
    restatement's"""
    cg = RESTATEMENT[variant]
    A2 = np.array([[4.0, 1.0], [1.0, 3.0]])
    runs = [(A2, [1.0, 2.0], dict(itmax=1)), (A2, [1.0, 2.0], dict()), (A2, [0.0, 0.0], dict()),
            ([[2.0]], [3.0], dict(itmax=1)), ([[2.0]], [3.0], dict()), ([[2.0]], [0.0], dict()),
            (np.diag([1.0, -0.25]), [1.0, 1.0], dict())]
    for M, b, kw in runs:
        M, b = np.asarray(M), np.asarray(b)
        xr, sr = cg(M, b, **kw)
        assert sr.error is None
        ws, st, x = _cg(K, ctx, _from_dense(K, ctx, M), b, variant, **kw)
        what = f"cg variant {variant} ending n={len(b)} b={b.tolist()} {kw} diag={np.diag(M).tolist()}"
        assert (st.niter, st.status, st.solved, st.inconsistent) == (sr.niter, sr.status, sr.solved, sr.inconsistent), (what, st.status)
        assert _hist_ok(parity_log, what, st.residuals, sr.residuals, HIST_RTOL)
        assert np.all(np.abs(x - xr) <= 1e-8 * max(np.abs(xr).max(), 1e-300)), (what, x, xr)
    assert cg(np.diag([1.0, -0.25]), np.array([1.0, 1.0]))[1].status == vr.ZERO_CURVATURE             # the breakdown flag mid-solve
    for M, b in ((np.diag([1.0, -2.0]), [1.0, 1.0]), ([[-1.0]], [1.0])):
        M, b = np.asarray(M), np.asarray(b)
        xr, sr = cg(M, b)
        assert sr.error == vr.NOT_SPD and not xr.any()
        ws = _cg_workspace(K, ctx, len(b))
        with pytest.raises(K.KhipError) as e:
            K.cg_(ws, _from_dense(K, ctx, M), ctx.array(b), variant=variant, history=True)
        assert e.value.code == -5 and "not symmetric positive definite" in str(e.value)               # KHIP_ERR_NUMERIC
        assert not ws.x.to_host().any()


# ---- gmres!(variant = 1) ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GMRES_CASES))
def test_cgs2_against_its_restatement(K, ctx, oracle, parity_log, name):
    kind, size, which, kw = GMRES_CASES[name]
    pair = reference_pair(oracle, "gmres", name)
    (xr, sr), _ = pair
    rtol = _budget(pair)
    dA = _upload(K, ctx, oracle, kind, size)
    x, st, ws = K.gmres(dA, ctx.array(case_rhs(dA.shape[0], which)), history=True, variant=1, **kw)
    what = f"gmres variant 1 {name}"
    assert ws.last_path == 1
    assert (st.niter, st.status, st.solved, st.inconsistent) == (sr.niter, sr.status, sr.solved, sr.inconsistent), (what, st.niter, st.status)
    assert _hist_ok(parity_log, what, st.residuals, sr.residuals, rtol)
    assert _vec_ok(parity_log, what, "x", x.to_host(), xr, rtol)


def _gmres_workspace(K, ctx, n, first, mem):
    """x, w and the basis on vectors carved at element offset `first`; two spare vectors for the grow callback"""
    names = ("x", "w") + tuple(f"V{i}" for i in range(mem + 2))
    buf, v = _carved(ctx, n, names, first)
    ws = K.GmresWorkspace.__new__(K.GmresWorkspace)
    ws.ctx, ws.m, ws.n, ws.adopted, ws._alloc_s, ws._h, ws._buf = ctx, n, n, True, 0.0, C.c_void_p(), buf
    ws._vec, ws.memory = {"x": v["x"], "w": v["w"]}, mem
    ws.V = [v[f"V{i}"] for i in range(mem)]
    spare = [v[f"V{i}"] for i in range(mem, mem + 2)]
    ptrs = (C.c_void_p * mem)(*[u.ptr for u in ws.V])
    assert K.lib().khip_gmres_workspace_adopt(ctx._h, n, n, mem, v["x"].ptr, v["w"].ptr, ptrs, C.byref(ws._h)) == 0

    def grow(_ud):
        ws.V.append(spare.pop(0))
        return ws.V[-1].ptr
    ws._grow = K.GROW_FN(grow)
    assert K.lib().khip_gmres_workspace_set_grow(ws._h, ws._grow, None) == 0
    return ws


def _orthogonality(V):
    """max |V'V - I| with every entry an exactly summed, correctly rounded dot"""
    k = len(V)
    return max(abs(er.exact_dot(V[i], V[j]) - (1.0 if i == j else 0.0)) for i in range(k) for j in range(i, k))


@pytest.mark.parametrize("n", sorted(ODD))
@pytest.mark.parametrize("first", [0, 1])
def test_cgs2_leaves_an_orthonormal_basis(K, ctx, oracle, parity_log, n, first):
    """itmax = memory = 6 on an adopted basis, read back after the solve: max |V'V - I| at most 10 x the same quantity of the
    restatement's basis (the project's factor), never held below n 2^-52 (the first-order bound of normalising an n-term vector)"""
    kind, size = ODD[n]
    S = case_matrix(oracle, kind, size)
    b = case_rhs(n, "cos")
    kw = dict(memory=6, itmax=6, atol=0.0, rtol=0.0)
    pair = (vr.gmres_cgs2(S, b, **kw), vr.gmres_cgs2(S, b, dot=vr.fsum_dot, **kw))
    (xr, sr), _ = pair
    assert len(sr.vectors["V"]) == 6 and sr.niter == 6
    ref = _orthogonality(sr.vectors["V"])
    bound = max(10.0 * ref, n * 2.0 ** -52)
    rtol = _budget(pair)
    for nt in (None, 1):
        for comp in (1, 0):
            ws = _gmres_workspace(K, ctx, n, first, 6)
            with _Options(ctx, compensated=comp, **({} if nt is None else dict(nt_min_elems=nt))):
                K.gmres_(ws, _upload(K, ctx, oracle, kind, size), ctx.array(b), variant=1, history=True, itmax=6, atol=0.0, rtol=0.0)
            st = ws.stats
            what = f"gmres variant 1 n={n} offset {first} nt_min_elems={nt} compensated={comp}"
            assert ws.last_path == 1 and len(ws.V) == 6 and all(u.ptr % 16 == 8 * first for u in ws.V)
            assert (st.niter, st.status) == (6, vr.TIRED) == (sr.niter, sr.status)
            got = _orthogonality([u.to_host() for u in ws.V])
            print(f"{what}: max |V'V - I| = {got:.3e}, restatement {ref:.3e}, bound {bound:.3e}")
            parity_log(test="variants", what=what, quantity="orthogonality", deviation=got, restatement=ref, budget=bound)
            assert got <= bound, (what, got, ref, bound)
            assert _hist_ok(parity_log, what, st.residuals, sr.residuals, rtol)
            assert _vec_ok(parity_log, what, "x", ws.x.to_host(), xr, rtol)


# ---- cache hints and odd offsets for all four; the s-step form's true residual ------------------------------------------------------
@pytest.mark.parametrize("solver,kw,opts", [("cg", dict(variant=1), {}), ("cg", dict(variant=2), {}), ("gmres", dict(variant=1), {}),
                                            ("gmres", dict(variant=2, restart=True), dict(gmres_sstep=1)),
                                            ("gmres", dict(variant=2, restart=True), dict(gmres_sstep=4))])
def test_variant_bits_do_not_depend_on_cache_hints(K, ctx, solver, kw, opts):
    """non-temporal equals default to the bit, offset 1 against offset 0 within the tolerances of tests/test_gpu_vec_dispatch.py;
    every variant reports the host-driven path"""
    with _Options(ctx, **opts):
        _check_solver(K, ctx, solver, last_path=1, **kw)


@pytest.mark.parametrize("n", [511, 513])
@pytest.mark.parametrize("sstep", [1, 4])
def test_sstep_true_residual(K, ctx, oracle, parity_log, n, sstep):
    """a converged s-step solve: ||b - A x|| / ||b|| <= 3e-8, the figure of test_gmres_sstep_variant_parity_budget"""
    S = case_matrix(oracle, "tridiagonal", n)
    b = case_rhs(n, "cos")
    dA = _upload(K, ctx, oracle, "tridiagonal", n)
    with _Options(ctx, gmres_sstep=sstep):
        x, st, ws = K.gmres(dA, ctx.array(b), memory=20, restart=True, history=True, variant=2)
        runs = [("library-owned", x.to_host(), st)]
        for first in (0, 1):
            ws = _gmres_workspace(K, ctx, n, first, 8)
            K.gmres_(ws, dA, ctx.array(b), variant=2, restart=True, history=True)
            runs.append((f"offset {first}", ws.x.to_host(), ws.stats))
    for tag, xh, st in runs:
        res = float(np.linalg.norm(b - S @ xh) / np.linalg.norm(b))
        print(f"gmres variant 2 n={n} s={sstep} {tag}: niter {st.niter}, true residual {res:.3e}")
        parity_log(test="variants", what=f"gmres variant 2 n={n} s={sstep} {tag}", quantity="true residual", deviation=res, budget=3e-8)
        assert st.solved and st.status == vr.SOLVED, (tag, st.status)
        assert res <= 3e-8, (tag, res)
