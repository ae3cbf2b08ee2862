"""The workspaces of the six solvers on the Saunders-Simon-Yip process at m = 5, n = 3: the vector table of the C core (which side
a vector is on: ws_len, ws_bytes, ws_warm_start, ws_warm_start2 of csrc/solver_host.hpp) against ROW_SIDE of the Python classes,
which the host tests hold against the reference's struct; the two-vector warm start of _TwoSidedWorkspace; and _ssy_solve /
_solve_pair against the dispatcher.  At a rectangular shape a vector on the wrong side has the wrong length."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_tricg_host import rect_system  # noqa: E402

M, N = 5, 3
SOLVERS = ("usymqr", "usymlq", "trilqr", "tricg", "trimr", "usymlqr")
PAIRS = ("trilqr", "tricg", "trimr", "usymlqr")                 # two solutions, warm start with (x0, y0)


def _cls(K, name):
    return getattr(K, name.capitalize() + "Workspace")


def _lazy(cls):
    return ("dx", "dy") if cls.SOLUTIONS == ("x", "y") else ("dx",)


def _side(cls, name):
    return M if name in cls.ROW_SIDE else N


def _starts(cls):
    """x0 / y0 of the lengths of Δx / Δy, with distinct entries."""
    return [np.arange(1.0, _side(cls, name) + 1) * (k + 1) + 0.25 for k, name in enumerate(_lazy(cls))]


def _system(K, ctx):
    """_sign_matrix(5, 3) with the right-hand sides of the solvers' rectangular cases (tests/test_tricg_host.py)."""
    A, b, c = rect_system(M, N)
    S = sp.csr_matrix(A)
    S.sort_indices()
    return K.CsrMatrix.from_host(ctx, S.indptr, S.indices, S.data, S.shape), ctx.array(b), ctx.array(c)


def _lengths_and_bytes(K, ctx, name, adopt):
    """Checks every vector's length; returns nbytes before and after the warm start."""
    cls = _cls(K, name)
    ws = cls(ctx, M, N, adopt=adopt)
    for v in cls.VECTORS:
        assert len(ws.vector(v)) == _side(cls, v), (name, v)
    before = ws.nbytes
    ws.warm_start_(*[ctx.array(s) for s in _starts(cls)])
    for v in _lazy(cls):
        assert len(ws.vector(v)) == _side(cls, v), (name, v)
    return before, ws.nbytes


@pytest.mark.parametrize("name", SOLVERS)
def test_every_vector_has_its_sides_length(K, ctx, name):
    cls = _cls(K, name)
    core = sum(_side(cls, v) for v in cls.VECTORS)
    lazy = sum(_side(cls, v) for v in _lazy(cls))
    owned = _lengths_and_bytes(K, ctx, name, adopt=False)
    assert owned == (8 * core, 8 * (core + lazy))
    assert _lengths_and_bytes(K, ctx, name, adopt=True) == owned


@pytest.mark.parametrize("adopt", [False, True])
@pytest.mark.parametrize("name", PAIRS)
def test_warm_start_copies_each_start_at_its_own_length(K, ctx, name, adopt):
    cls = _cls(K, name)
    x0, y0 = _starts(cls)
    ws = cls(ctx, M, N, adopt=adopt)
    ws.warm_start_(ctx.array(x0), ctx.array(y0))
    assert np.array_equal(ws.vector("dx").to_host(), x0)
    assert np.array_equal(ws.vector("dy").to_host(), y0)


@pytest.mark.parametrize("adopt", [False, True])
def test_trilqr_warm_start_refuses_a_wrong_length(K, ctx, adopt):
    """Δx of trilqr! has n entries and Δy has m: x0 of m entries is refused before anything is copied, and the workspace goes on."""
    A, b, c = _system(K, ctx)
    ws = K.TrilqrWorkspace(ctx, M, N, adopt=adopt)
    with pytest.raises(K.KhipError, match="Inconsistent problem size"):
        ws.warm_start_(ctx.array(np.ones(M)), ctx.array(np.ones(M)))
    with pytest.raises(K.KhipError, match="Inconsistent problem size"):
        ws.warm_start_(ctx.array(np.ones(N)), ctx.array(np.ones(N)))
    ws.warm_start_(ctx.array(np.zeros(N)), ctx.array(np.zeros(M)))
    K.trilqr_(ws, A, b, c)
    assert ws.last_path == 0


@pytest.mark.parametrize("name", SOLVERS)
def test_entry_points_agree_with_the_dispatcher(K, ctx, name):
    """The in-place entry (_ssy_solve) and, with two solutions, the out-of-place entry (_solve_pair) give the bits of
    krylov_solve(method, ...)."""
    A, b, c = _system(K, ctx)
    ws = _cls(K, name)(ctx, M, N)
    getattr(K, name + "_")(ws, A, b, c)
    got = [ws]
    if name in PAIRS:
        got.append(getattr(K, name)(A, b, c)[-1])
    want = K.krylov_solve(name, A, b, c=c)[-1]
    assert (want.m, want.n) == (M, N)
    for w in got:
        for s in w.SOLUTIONS:
            assert len(getattr(w, s)) == _side(type(w), s)
            assert np.array_equal(getattr(w, s).to_host(), getattr(want, s).to_host()), (name, s)
