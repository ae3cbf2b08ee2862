"""cg!, gmres! and bicgstab! on the GPU at tiny shapes and on every ending: the case table of tests/first_solvers_cases.py on the
three loops (`fused` = False / True / 2 is path 0 / 1 / 2).  Every test asserts `last_path` first, so a silent fallback cannot
pass as a device-loop test.

  * path 0 (one launch per primitive) against the CPU oracle: `judge` with the project's tolerance for these solvers
    (tests/test_gpu_solvers.py): |Δr_k| <= 1e-10 r_k + 100 eps r_0, x within 1e-9 max|x|, non-finite entries in the same places.
    On cases in the history-parity list (tests/test_first_solvers_cases_host.py) only; the six chaotic bicgstab! cases must be
    solved and meet the reference's bicgstab_tol on the true residual.
  * path 1 against path 0: the same judge and tolerance, on every case.
  * path 2 against path 1: np.array_equal(equal_nan=True) on x, the history and every vector the workspace exposes, equality of
    niter, status and every flag, on EVERY case -- the same kernels and the same scalar code.
  * against the case's A in NumPy, whatever the oracle says: the reference's 1e-6 on the residual of solved cases, on the normal
    equations of gmres!'s least-squares endings, on |radius - ‖x‖| where the reference asserts it.
"""
import os
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import first_solvers_cases as fc  # noqa: E402
from first_solvers_cases import (BREAKDOWN, CASES, ENDING_CASES, LSQ, NPC, SOLVED, SOLVERS, TOL, ZERO_CURVATURE, Record,  # noqa: E402
                                 case_c, case_ids, flags, judge, oracle_run, qualifies, solver_kwargs, system)

ALL = case_ids()
IDS = [f"{s}-{n}" for s, n in ALL]
# the vectors a workspace exposes by name: khip_cg_vector; the adopted vectors of the Python mirror's Gmres / BicgstabWorkspace.
# gmres!: x here, and the basis V[0 .. inner_iter - 1] of the last cycle beside the host state (Record.basis).  Its w and
# V[inner_iter] are left out: when the loop stops, the look-ahead has already enqueued the abandoned step's q / sqrt(‖q‖²) and its
# product into them, which the plain sequence never forms.
VECTORS = {"cg": ("x", "r", "p", "Ap"), "gmres": ("x",), "bicgstab": ("x", "r", "p", "v", "s", "qd")}
# A qualifying case whose path 0 or path 1 exceeds 1e-10 gets 10 x the oracle's own dot-mode deviation, at least 1e-8, here and
# in profiles/first_solvers_cases.md: (solver, case) -> rtol.  None needed it.
BUDGET = {}


def _tol(solver, name):
    return dict(TOL, rtol=BUDGET.get((solver, name), TOL["rtol"]))


# ---- running a case ----------------------------------------------------------------------------------------------------------------
_DEV, _GPU_RUNS = {}, {}


@pytest.fixture(scope="module")
def run(K, ctx, oracle):
    """run(solver, case, fused, history=True) -> Record of that solve (flags, history, x, last_path, the named vectors), made
    once and shared by the tests; run.device(op) is the case's operator on the device."""
    def device(op):
        if op not in _DEV:
            S = system(oracle, op)
            _DEV[op] = K.CsrMatrix.from_host(ctx, S.rowptr, S.col, S.val, (S.n, S.n))
        return _DEV[op]

    def solve(solver, name, fused, history=True, ws=None):
        case = CASES[solver][name]
        S = system(oracle, case.op)
        kw = solver_kwargs(solver, name)
        b = ctx.array(S.b)
        if solver == "cg":
            ws = ws or K.CgWorkspace(ctx, S.n, S.n)
            K.cg_(ws, device(case.op), b, fused=fused, history=history, **kw)
        elif solver == "gmres":
            ws = ws or K.GmresWorkspace(ctx, S.n, S.n, memory=kw["memory"], adopt=True)
            kw.pop("memory")
            K.gmres_(ws, device(case.op), b, fused=fused, history=history, **kw)
        else:
            ws = ws or K.BicgstabWorkspace(ctx, S.n, S.n, adopt=True)
            c = case_c(S, case)
            K.bicgstab_(ws, device(case.op), b, c=None if c is None else ctx.array(c), fused=fused, history=history, **kw)
        return ws

    def get(solver, name, fused, history=True):
        key = (solver, name, fused, history)
        if key not in _GPU_RUNS:
            ws = solve(solver, name, fused, history)
            path = ws.last_path
            vec = {v: (ws.vector(v) if solver == "cg" else ws._vec[v]).to_host() for v in VECTORS[solver]}
            extra = {}
            if solver == "gmres":
                c, s, z, R, inner = ws.host_state()
                extra = dict(host_state=(c, s, z, R, np.array([inner])), basis=[ws.V[i].to_host() for i in range(inner)])
            if solver == "cg" and ws.stats.indefinite:           # npc_dir is written only when pᵀAp <= 0 was met (src/cg.jl:205, :233)
                extra = dict(npc_dir=ws.vector("npc_dir").to_host())
            _GPU_RUNS[key] = Record(ws.stats, x=ws.x.to_host(), path=path, vectors=vec, **extra)
        return _GPU_RUNS[key]

    get.device, get.solve = device, solve
    yield get
    _DEV.clear()
    _GPU_RUNS.clear()


def _expected_path(solver, name, fused):
    case = CASES[solver][name]
    if case.path2 == -1:                       # bicgstab! on bᴴc = 0: no loop is chosen (case.why)
        return -1
    return {0: 0, 1: 1, 2: case.path2}[int(fused)]


def _line(solver, name, rec):
    print(f"{solver} {name}: path {rec.path}, niter {rec.niter}, {rec.status}, solved {rec.solved}, inconsistent {rec.inconsistent}")


def _true_residual(oracle, solver, name, x):
    S = system(oracle, CASES[solver][name].op)
    return float(np.linalg.norm(S.b - S.A @ x) / np.linalg.norm(S.b))


def _written(solver, rec):
    """The named vectors a solve has written: all of them once a loop was chosen; bicgstab! on bᴴc = 0 returns before it touches
    qd, which is then whatever the allocation held."""
    return VECTORS[solver] if rec.path >= 0 else ("x",)


def _same_bits(a, b, solver, what):
    assert flags(solver, a) == flags(solver, b), (what, flags(solver, a), flags(solver, b))
    assert (a.indefinite, a.npcCount) == (b.indefinite, b.npcCount), what
    assert np.array_equal(a.residuals, b.residuals, equal_nan=True), (what, a.residuals, b.residuals)
    assert np.array_equal(a.x, b.x, equal_nan=True), (what, "x")


# ---- 1. path 0 against the oracle, path 1 against path 0 ---------------------------------------------------------------------------
@pytest.mark.parametrize("solver,name", ALL, ids=IDS)
def test_path0_against_the_oracle(oracle, run, parity_log, solver, name):
    got = run(solver, name, 0)
    assert got.path == _expected_path(solver, name, 0)
    _line(solver, name, got)
    want = Record(oracle_run(oracle, solver, name))
    ok, own = qualifies(oracle, solver, name)
    if ok:
        units = judge(got, want, _tol(solver, name), solver, x=got.x, x_want=want.x)
        print(f"largest deviation {units:.3e} of the tolerance; the oracle's own dot-mode deviation {own:.3e}")
        parity_log(test="first_solvers_cases", solver=solver, case=name, path=0, against="oracle", niter=got.niter, status=got.status,
                   tol_units=units, oracle_dot_mode_dev=own)
    else:
        res = _true_residual(oracle, solver, name, got.x)
        print(f"not in the history-parity list (oracle niter {want.niter}): niter {got.niter}, ||b - A x|| / ||b|| = {res:.3e}")
        parity_log(test="first_solvers_cases", solver=solver, case=name, path=0, against="true residual", niter=got.niter,
                   status=got.status, resid=res)
        assert got.solved and got.status == SOLVED and res <= fc.RESID_TOL


@pytest.mark.parametrize("solver,name", ALL, ids=IDS)
def test_path1_against_path0(oracle, run, parity_log, solver, name):
    """Every case, the six chaotic ones included: both loops run on the device's own dots."""
    p0, p1 = run(solver, name, 0), run(solver, name, 1)
    assert (p0.path, p1.path) == (_expected_path(solver, name, 0), _expected_path(solver, name, 1))
    _line(solver, name, p1)
    _, own = qualifies(oracle, solver, name)
    units = judge(p1, p0, _tol(solver, name), solver, x=p1.x, x_want=p0.x)
    print(f"largest deviation {units:.3e} of the tolerance")
    parity_log(test="first_solvers_cases", solver=solver, case=name, path=1, against="path 0", niter=p1.niter, status=p1.status,
               tol_units=units, oracle_dot_mode_dev=own if np.isfinite(own) else None)


# ---- 2. path 2 bit-identical to path 1 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,name", ALL, ids=IDS)
def test_path2_is_bit_identical_to_path1(oracle, run, parity_log, solver, name):
    """Every case: n = 1, 2, 3, 63, 64, 65, the odd n = 729 over three workgroups, the chaotic six, and every ending -- the NaN
    histories of "breakdown αₖ == 0", the least-squares and zero-curvature endings, the breakdown Hbis <= btol among them.
    After the stop nothing more ran: the workspace's vectors are the same bits, gmres!'s host state too."""
    p1, p2 = run(solver, name, 1), run(solver, name, 2)
    assert (p1.path, p2.path) == (_expected_path(solver, name, 1), _expected_path(solver, name, 2)), CASES[solver][name].why
    _line(solver, name, p2)
    parity_log(test="first_solvers_cases", solver=solver, case=name, path=2, against="path 1", niter=p2.niter, status=p2.status,
               last_path=p2.path)
    _same_bits(p2, p1, solver, name)
    assert len(p2.residuals) == p2.niter + 1
    for v in _written(solver, p2):
        assert np.array_equal(p2.vectors[v], p1.vectors[v], equal_nan=True), (name, v)
    if solver == "gmres":
        for a, b, what in zip(p2.host_state, p1.host_state, ("c", "s", "z", "R", "inner_iter")):
            assert np.array_equal(a, b, equal_nan=True), (name, what)
        assert len(p2.basis) == len(p1.basis) == int(p2.host_state[4][0]) >= 1
        for k, (a, b) in enumerate(zip(p2.basis, p1.basis)):
            assert np.array_equal(a, b, equal_nan=True), (name, f"V[{k}]")
    if solver == "cg":
        # r is the residual of the returned x (tests/test_gpu_solvers.py:138-140): nothing ran after the stop
        S = system(oracle, CASES[solver][name].op)
        # (linesearch with pᵀAp <= 0 at iteration 0 returns the direction itself, x = p = b, src/cg.jl:206-207: r stays b)
        x_is_direction = p2.status == NPC and p2.niter == 0
        for p in (p1, p2):
            want_r = S.b if x_is_direction else S.b - S.A @ p.x
            assert np.allclose(p.vectors["r"], want_r, rtol=0, atol=1e-9 * np.linalg.norm(S.b)), name
        if hasattr(p1, "npc_dir"):
            assert np.array_equal(p2.npc_dir, p1.npc_dir)
    ok, _ = qualifies(oracle, solver, name)
    if ok:                                                           # and the device loop ends where the oracle ends
        want = oracle_run(oracle, solver, name)
        assert flags(solver, p2) == flags(solver, want), (flags(solver, p2), flags(solver, want))


# ---- 3. independent of the oracle --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,name", ALL, ids=IDS)
def test_results_against_the_operator_in_numpy(oracle, run, solver, name):
    case = CASES[solver][name]
    S = system(oracle, case.op)
    for fused in (0, 1, 2):
        got = run(solver, name, fused)
        assert got.path == _expected_path(solver, name, fused)
        if case.ending is not None:
            assert got.status == case.ending, (fused, got.status)
        if got.status == SOLVED:
            res = float(np.linalg.norm(S.b - S.A @ got.x) / np.linalg.norm(S.b))
            print(f"path {got.path}: ||b - A x|| / ||b|| = {res:.3e}")
            assert got.solved and res <= fc.RESID_TOL, (fused, res)
        if got.status == LSQ:                                        # test/test_gmres.jl:49-53
            normal = float(np.linalg.norm(S.A.T @ (S.b - S.A @ got.x)))
            print(f"path {got.path}: ||A'(b - A x)|| = {normal:.3e}")
            assert got.inconsistent and normal <= 1e-6, (fused, normal)
        if case.boundary:                                            # test/test_cg.jl:16-19
            radius = case.kw["radius"]
            assert got.solved and abs(radius - np.linalg.norm(got.x)) <= 1e-6 * radius, fused
        if got.status == NPC:                                        # test/test_cg.jl:56-62, :93-96
            assert got.solved and got.indefinite and got.npcCount == 1 and not got.inconsistent
            assert got.npc_dir @ S.A @ got.npc_dir <= 0
            if got.niter == 0:
                assert np.array_equal(got.npc_dir, S.b) and np.array_equal(got.x, S.b)
        if got.status == ZERO_CURVATURE:
            assert got.inconsistent and not got.solved
        if got.status == BREAKDOWN:
            assert not got.solved and not np.isfinite(got.residuals[-1])


# ---- 4. history off ----------------------------------------------------------------------------------------------------------------
def _history_off_cases():
    out = []
    for s in SOLVERS:
        rest = [n for n in CASES[s] if n not in ENDING_CASES[s]]
        out += [(s, n) for n in ENDING_CASES[s]] + [(s, n) for n in rest[::5]]
    return out


@pytest.mark.parametrize("solver,name", _history_off_cases(), ids=lambda v: v)
def test_history_off_changes_nothing_but_the_history(run, solver, name):
    for fused in (0, 1, 2):
        on, off = run(solver, name, fused), run(solver, name, fused, history=False)
        assert off.path == on.path == _expected_path(solver, name, fused)
        assert len(off.residuals) == 0 and len(on.residuals) == on.niter + 1
        assert flags(solver, off) == flags(solver, on) and (off.indefinite, off.npcCount) == (on.indefinite, on.npcCount), fused
        assert np.array_equal(off.x, on.x, equal_nan=True), fused
        for v in _written(solver, on):
            assert np.array_equal(off.vectors[v], on.vectors[v], equal_nan=True), (fused, v)


# ---- 5. workspace reuse ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("restart", [False, True])
@pytest.mark.parametrize("first", ["diag3", "eye"])
def test_gmres_look_ahead_leaves_nothing_behind_after_a_breakdown(K, ctx, oracle, run, first, restart):
    """The look-ahead loop enqueues V[k+1] = q / sqrt(‖q‖²) and A V[k+1] before the host sees Hbis; at an exact breakdown that is
    a division by zero.  The abandoned step must never be read: an ordinary solve (kron7, n = 343) on the SAME workspace equals a
    fresh workspace's in every bit."""
    n = 343
    S = system(oracle, (first, n))
    kron = system(oracle, ("kron", 7))
    kw = dict(restart=restart, history=True)
    ws = K.GmresWorkspace(ctx, n, n, memory=20)
    K.gmres_(ws, run.device((first, n)), ctx.array(S.b), fused=2, **kw)
    st = ws.stats
    assert ws.last_path == 2
    want = oracle.gmres(S.csr(oracle), S.b, memory=20, history=True, restart=restart)
    print(f"{first}: niter {st.niter}, {st.status}; history {st.residuals}")
    assert (st.niter, st.status, st.solved) == (want.niter, want.status, True) and st.niter == (3 if first == "diag3" else 1)
    assert np.abs(ws.x.to_host() - np.linalg.solve(S.A, S.b)).max() <= 1e-12 * n
    K.gmres_(ws, run.device(("kron", 7)), ctx.array(kron.b), fused=2, **kw)
    fresh = K.GmresWorkspace(ctx, n, n, memory=20)
    K.gmres_(fresh, run.device(("kron", 7)), ctx.array(kron.b), fused=2, **kw)
    assert ws.last_path == fresh.last_path == 2
    a, b = Record(ws.stats, x=ws.x.to_host()), Record(fresh.stats, x=fresh.x.to_host())
    _same_bits(a, b, "gmres", "reused against fresh")
    assert a.solved and np.isfinite(a.x).all() and np.isfinite(a.residuals).all()
    for u, v in zip(ws.host_state(), fresh.host_state()):
        assert np.array_equal(u, v)
    judge(a, Record(oracle.gmres(kron.csr(oracle), kron.b, memory=20, history=True, restart=restart)), TOL, "gmres")


@pytest.mark.parametrize("fused", [1, 2])
@pytest.mark.parametrize("second_linesearch", [True, False])
def test_cg_workspace_reuse_resets_the_npc_state(K, ctx, oracle, run, fused, second_linesearch):
    """test/test_cg.jl:136-170: an npc solve (linesearch on diag(10, 8, 5, -1)), then diag(10, 8, 5, 1) on the same workspace:
    npcCount and indefinite are reset.  With linesearch again the gate keeps the host-driven loop; without it `fused = 2` runs the
    device-resident loop on the reused workspace."""
    S1, S2 = system(oracle, ("npc4",)), system(oracle, ("npc4", 1.0))
    ws = K.CgWorkspace(ctx, 4, 4)
    K.cg_(ws, run.device(("npc4",)), ctx.array(S1.b), linesearch=True, fused=fused, history=True)
    assert ws.last_path == 1
    st = ws.stats
    assert st.npcCount == 1 and st.indefinite and st.status == NPC
    K.cg_(ws, run.device(("npc4", 1.0)), ctx.array(S2.b), linesearch=second_linesearch, fused=fused, history=True)
    assert ws.last_path == (1 if second_linesearch else fused)
    st = ws.stats
    assert st.npcCount == 0 and st.indefinite is False and st.solved and st.status == SOLVED
    assert np.abs(ws.x.to_host() - S2.b / np.diag(S2.A)).max() <= 1e-6
    want = oracle.cg(S2.csr(oracle), S2.b, linesearch=second_linesearch, history=True)
    judge(Record(st), Record(want), TOL, "cg", x=ws.x.to_host(), x_want=want.x)


def test_bicgstab_workspace_reuse_after_a_breakdown(K, ctx, oracle, run):
    """After "breakdown αₖ == 0" every vector of the workspace holds NaN: the next solve on it equals a fresh workspace's."""
    ws = K.BicgstabWorkspace(ctx, 10, 10, adopt=True)
    S = system(oracle, ("eye", 10))
    K.bicgstab_(ws, run.device(("eye", 10)), ctx.array(S.b), fused=2, history=True)
    assert ws.last_path == 2 and ws.stats.status == BREAKDOWN and np.isnan(ws._vec["p"].to_host()).all()
    S = system(oracle, ("nd", 10))
    K.bicgstab_(ws, run.device(("nd", 10)), ctx.array(S.b), fused=2, history=True)
    assert ws.last_path == 2
    _same_bits(Record(ws.stats, x=ws.x.to_host()), run("bicgstab", "nd10", 2), "bicgstab", "reused against fresh")


# ---- 6. row-partitioned ------------------------------------------------------------------------------------------------------------
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


PARTITIONED = [("cg", "sd65"), ("gmres", "sd65"), ("bicgstab", "sd65"), ("gmres", "sq_inc10"), ("cg", "sq_inc10"), ("bicgstab", "eye10")]


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("solver,name", PARTITIONED, ids=lambda v: v)
def test_row_partitioned(K, oracle, run, parity_log, solver, name, world):
    """Rows split over 2 and 3 in-process ranks: the stop decision comes from all-reduced scalars, so every rank ends with the same
    niter, status and flags and bit-equal histories; against the single-device device loop, the judge's tolerance (NaN by place)."""
    case = CASES[solver][name]
    S = system(oracle, case.op)
    single = run(solver, name, 2)
    assert single.path == 2
    n = S.n
    starts = K.row_partition(n, world)

    def body(cx, rank):
        r0, r1 = starts[rank], starts[rank + 1]
        lo, hi = S.rowptr[r0], S.rowptr[r1]
        A = K.CsrMatrix.from_host(cx, S.rowptr[r0:r1 + 1] - lo, S.col[lo:hi], S.val[lo:hi], (r1 - r0, n), dist_rows=(r0, r1), n_global=n)
        b = cx.array(S.b[r0:r1])
        kw = solver_kwargs(solver, name)
        if solver == "cg":
            ws = K.CgWorkspace(cx, r1 - r0, r1 - r0)
            K.cg_(ws, A, b, fused=2, history=True, **kw)
        elif solver == "gmres":
            ws = K.GmresWorkspace(cx, r1 - r0, r1 - r0, memory=kw.pop("memory"))
            K.gmres_(ws, A, b, fused=2, history=True, **kw)
        else:
            ws = K.BicgstabWorkspace(cx, r1 - r0, r1 - r0)
            K.bicgstab_(ws, A, b, fused=2, history=True, **kw)
        return Record(ws.stats, x=ws.x.to_host(), path=ws.last_path)

    res = _run_ranks(K, world, 818100 + 10 * world + PARTITIONED.index((solver, name)), body)
    for rec in res:
        assert rec.path == 2
    x = np.concatenate([rec.x for rec in res])
    for rank, rec in enumerate(res):
        _line(solver, f"{name} rank {rank} of {world}", rec)
        assert flags(solver, rec) == flags(solver, res[0]), rank
        assert np.array_equal(rec.residuals, res[0].residuals, equal_nan=True), rank
    units = judge(res[0], single, TOL, solver, x=x, x_want=single.x)
    parity_log(test="first_solvers_cases", solver=solver, case=name, path=2, against="single device", world=world, tol_units=units)
    assert res[0].status == case.ending
