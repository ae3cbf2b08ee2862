"""What surrounds the iterations of every single-vector solver (csrc/solve_frame.hpp), the same four behaviours for each of them and
for both fused loops: the shape check's message, the callback's exit with stats.residuals visible inside the callback, the time
limit's exit after one iteration, and a warm start that is used up by the solve.  The numerics of each solver have their own
files; here only the frame is checked, on operators of a few hundred rows."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SYMMETRIC = ("cg", "minres", "symmlq", "minres_qlp", "cg_lanczos_shift")
SOLVERS = SYMMETRIC + ("bicgstab", "cgs", "bilq", "qmr", "bilqr")
LONG_MESSAGE = ("symmlq", "minres_qlp", "cgs", "cg_lanczos_shift", "bilq", "qmr", "bilqr")      # cg!, minres!: the short form
FIRST_CHUNK_OF_ONE = tuple(s for s in SOLVERS if s not in ("cg", "bicgstab"))
SHIFTS = [0.5, 2.0]
_CACHE = {}


def _rhs(n):
    return np.cos(0.37 * np.arange(n)) + 0.5


def _other(n):
    return np.sin(0.11 * np.arange(n)) + 1.2


def _operator(K, ctx, oracle, solver):
    key = solver in SYMMETRIC
    if key not in _CACHE:
        Ac = oracle.poisson3d(8) if key else oracle.kron_unsymmetric(7)
        _CACHE[key] = (Ac, K.CsrMatrix.from_host(ctx, Ac.rowptr, Ac.col, Ac.val, (Ac.n, Ac.n)))
    return _CACHE[key]


def _workspace(K, ctx, solver, n):
    cls = getattr(K, "".join(w.capitalize() for w in solver.split("_")) + "Workspace")
    return cls(ctx, n, n, len(SHIFTS)) if solver == "cg_lanczos_shift" else cls(ctx, n, n)


def _solve(K, ctx, solver, ws, A, n, b=None, **kw):
    args = [ws, A, ctx.array(_rhs(n)) if b is None else b]
    if solver == "cg_lanczos_shift":
        args.append(SHIFTS)
    if solver == "bilqr":
        args.append(ctx.array(_other(n)))
    getattr(K, solver + "_")(*args, **kw)
    return ws


def _residuals(solver, st):
    return st.residuals[0] if solver == "cg_lanczos_shift" else st.residuals


@pytest.fixture(scope="module", autouse=True)
def _drop_operators():
    yield
    _CACHE.clear()


@pytest.mark.parametrize("fused", [1, 2])
@pytest.mark.parametrize("solver", [s for s in SOLVERS if s != "bicgstab"])       # bicgstab! has no shape check
def test_inconsistent_shape_message(K, ctx, oracle, solver, fused):
    Ac, A = _operator(K, ctx, oracle, solver)
    n = Ac.n
    ws = _workspace(K, ctx, solver, n + 1)
    with pytest.raises(K.KhipError) as e:
        _solve(K, ctx, solver, ws, A, n + 1, fused=fused)
    want = (f"(workspace.m, workspace.n) = ({n + 1}, {n + 1}) is inconsistent with size(A) = ({n}, {n})" if solver in LONG_MESSAGE
            else "(workspace.m, workspace.n) is inconsistent with size(A)")
    assert want in str(e.value)
    assert ws.stats.error == want


@pytest.mark.parametrize("fused", [1, 2])
@pytest.mark.parametrize("solver", SOLVERS)
def test_callback_exit_sees_the_history(K, ctx, oracle, solver, fused):
    """The callback runs on the host-driven loop whatever `fused` asks for; at its k-th call the history has k + 1 entries."""
    Ac, A = _operator(K, ctx, oracle, solver)
    seen = []

    def cb(w):
        seen.append(len(_residuals(solver, w.stats)))
        return len(seen) >= 2
    ws = _solve(K, ctx, solver, _workspace(K, ctx, solver, Ac.n), A, Ac.n, fused=fused, history=True, callback=cb)
    st = ws.stats
    assert seen == [2, 3]
    assert (st.niter, st.status, ws.last_path) == (2, "user-requested exit", 1)
    assert len(_residuals(solver, st)) == 3


@pytest.mark.parametrize("fused", [1, 2])
@pytest.mark.parametrize("solver", SOLVERS)
def test_time_limit_already_used_up(K, ctx, oracle, solver, fused):
    """timemax = 1 ns is over when it is first looked at: after iteration 1 on the host-driven loop and, where the device loop's
    first chunk is one iteration, there too; cg! and bicgstab! enqueue a chunk of four before they look."""
    Ac, A = _operator(K, ctx, oracle, solver)
    ws = _solve(K, ctx, solver, _workspace(K, ctx, solver, Ac.n), A, Ac.n, fused=fused, history=True, timemax=1e-9)
    st = ws.stats
    assert st.status == "time limit exceeded" and ws.last_path == fused
    if fused == 1 or solver in FIRST_CHUNK_OF_ONE:
        assert st.niter == 1
    else:
        assert 1 <= st.niter <= 4
    assert len(_residuals(solver, st)) == st.niter + 1


@pytest.mark.parametrize("fused", [1, 2])
@pytest.mark.parametrize("solver", [s for s in SOLVERS if s != "cg_lanczos_shift"])
def test_warm_start_is_added_and_used_up(K, ctx, oracle, solver, fused):
    """The solve starts from r0 = b - A x0: the history's first entry is its norm (a sum of n = 343 or 512 squares: 1e-12 relative is
    a thousand roundings' room).  The next solve on the same workspace starts from zero again: bit for bit a fresh workspace's."""
    Ac, A = _operator(K, ctx, oracle, solver)
    n = Ac.n
    b = _rhs(n)
    x0 = 0.01 * np.sin(0.3 * np.arange(n))
    ws = _workspace(K, ctx, solver, n)
    if solver == "bilqr":
        ws.warm_start_(ctx.array(x0), ctx.array(0.02 * np.cos(0.2 * np.arange(n))))
    else:
        ws.warm_start_(ctx.array(x0))
    _solve(K, ctx, solver, ws, A, n, fused=fused, history=True)
    assert ws.last_path == fused and ws.stats.niter > 0
    r0 = np.linalg.norm(b - Ac.matvec(x0))
    assert abs(ws.stats.residuals[0] - r0) <= 1e-12 * r0
    again = _solve(K, ctx, solver, ws, A, n, fused=fused, history=True)
    fresh = _solve(K, ctx, solver, _workspace(K, ctx, solver, n), A, n, fused=fused, history=True)
    assert again.stats.niter == fresh.stats.niter
    assert np.array_equal(again.stats.residuals, fresh.stats.residuals)
    assert np.array_equal(again.x.to_host(), fresh.x.to_host())


@pytest.mark.parametrize("fused", [1, 2])
@pytest.mark.parametrize("solver", [s for s in SOLVERS if s != "cg_lanczos_shift"])
def test_warm_start_from_the_solution_returns_it(K, ctx, oracle, solver, fused):
    """b = A x0 from the product the solver itself runs, so r0 = b - A x0 is zero in every bit: the solve ends before its loop and
    x = 0 + Δx is x0 in every bit.  bilqr! has no zero-residual return: bᴴc = 0 ends it the same way."""
    Ac, A = _operator(K, ctx, oracle, solver)
    n = Ac.n
    x0 = 1.0 + 0.01 * np.sin(0.3 * np.arange(n))
    b = A.matvec(ctx.array(x0))
    ws = _workspace(K, ctx, solver, n)
    if solver == "bilqr":
        ws.warm_start_(ctx.array(x0), ctx.array(x0))
    else:
        ws.warm_start_(ctx.array(x0))
    _solve(K, ctx, solver, ws, A, n, b=b, fused=fused, history=True)
    st = ws.stats
    assert np.array_equal(ws.x.to_host(), x0)
    assert st.niter == (1 if solver == "minres" else 0)
    assert st.status == ("Breakdown bᴴc = 0" if solver == "bilqr" else "x is a zero-residual solution")
    assert st.residuals[0] == 0.0
