"""cg_lanczos_shift! without a GPU: the NumPy restatement (tests/lanczos_shift_reference.py) against the reference's own known
answers (test/test_cg_lanczos_shift.jl) and against SciPy, the Python mirror's tables against src/cg_lanczos_shift.jl, and the
Julia specialisation's fallback gate."""
import math
import os
import re
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lanczos_shift_reference as lr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_SRC = "/root/reference/src"
JULIA_SRC = os.path.join(ROOT, "julia", "KrylovHIP", "src", "KrylovHIP.jl")
ref_tree = pytest.mark.skipif(not os.path.isdir(REFERENCE_SRC), reason="the reference tree is only present in the build container")


# ---- the reference's fixtures (test/test_utils.jl), restated -----------------------------------------------------------------
def symmetric_definite(n=10):
    A = sp.diags([np.ones(n - 1), np.full(n, 4.0), np.ones(n - 1)], [-1, 0, 1], format="csr")
    return A, A @ np.arange(1.0, n + 1)


def square_preconditioned(n=10):
    A = np.ones((n, n)) + (n - 1) * np.eye(n)
    return A, 10.0 * np.arange(1.0, n + 1), (1.0 / n) * np.eye(n)


def residuals(A, b, shifts, x):
    return [b - A @ x[i] - shifts[i] * x[i] for i in range(len(shifts))]


# ---- test/test_cg_lanczos_shift.jl, Float64 ------------------------------------------------------------------------------------
def test_cubic_splines_six_shifts():
    A, b = symmetric_definite()
    shifts = [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]
    x, st, _ = lr.cg_lanczos_shift(A, b, shifts, itmax=10)
    resids = np.array([np.linalg.norm(r) for r in residuals(A, b, shifts, x)]) / np.linalg.norm(b)
    assert np.all(resids <= 1e-6) and st.solved, resids


def test_negative_curvature_detection():
    A, b = symmetric_definite()
    _, st, _ = lr.cg_lanczos_shift(A, b, [-4.0, -3.0, 2.0], check_curvature=True, itmax=10)
    assert st.indefinite == [True, True, False]


def test_zero_right_hand_side():
    rng = np.random.default_rng(0)
    A = rng.random((10, 10))
    x, st, _ = lr.cg_lanczos_shift(A, np.zeros(10), [-4.0, -3.0, 2.0])
    assert all(np.linalg.norm(xi) == 0 for xi in x)
    assert st.status == "x is a zero-residual solution" and st.niter == 0 and st.solved
    assert st.residuals == [[0.0], [0.0], [0.0]]


def test_square_preconditioned():
    A, b, Minv = square_preconditioned()
    shifts = [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]
    x, st, _ = lr.cg_lanczos_shift(A, b, shifts, M=Minv)
    resids = np.array([np.linalg.norm(r) for r in residuals(A, b, shifts, x)]) / np.linalg.norm(b)
    assert np.all(resids <= 1e-6) and st.solved, resids


def test_callback_exit():
    A, b = symmetric_definite()
    shifts = [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]

    def cb_n2(ws):                                   # TestCallbackN2Shifts (test/callback_utils.jl:80-91), tol = 0.1
        return all(np.linalg.norm(r) <= 0.1 for r in residuals(A, b, shifts, ws.x))
    x, st, ws = lr.cg_lanczos_shift(A, b, shifts, atol=0.0, rtol=0.0, callback=cb_n2)
    assert st.status == "user-requested exit" and cb_n2(ws)


# ---- against SciPy -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,seed", [(60, 1), (200, 2)])
def test_restatement_agrees_with_spsolve(n, seed):
    rng = np.random.default_rng(seed)
    B = sp.random(n, n, density=0.05, random_state=seed, format="csr")
    A = (B + B.T + sp.identity(n) * (2.0 + abs(B).sum(axis=1).max())).tocsr()       # SPD by diagonal dominance
    b = rng.standard_normal(n)
    shifts = [0.0, 0.5, 3.0, 40.0]
    x, st, _ = lr.cg_lanczos_shift(A, b, shifts, atol=1e-12, rtol=1e-12)
    assert st.solved, st.status
    for i, s in enumerate(shifts):
        ref = spla.spsolve((A + s * sp.identity(n)).tocsc(), b)
        assert np.linalg.norm(x[i] - ref) <= 1e-9 * np.linalg.norm(ref), (s, np.linalg.norm(x[i] - ref))


def test_frozen_shift_keeps_its_history_and_iterate():
    """A shift that leaves not_cv keeps x_i and its history for the rest of the solve (:222-249)."""
    A, b = symmetric_definite(200)
    snap = {}

    def cb(ws):
        snap.setdefault(ws.stats.niter, [xi.copy() for xi in ws.x])
        return False
    x, st, ws = lr.cg_lanczos_shift(A, b, [1000.0, 0.0], callback=cb)
    k0 = len(st.residuals[0]) - 1                    # the large shift converged first, at iteration k0
    assert k0 < st.niter and len(st.residuals[1]) == st.niter + 1
    assert np.array_equal(snap[k0][0], x[0])


# ---- the Python mirror's tables against the reference --------------------------------------------------------------------------
@ref_tree
def test_forwarded_defaults_equal_the_reference():
    import krylov_jl_amd as K
    src = open(os.path.join(REFERENCE_SRC, "cg_lanczos_shift.jl")).read()
    names = re.findall(r":(\w+)", re.search(r"^kwargs_cg_lanczos_shift = \((.*?)\)", src, flags=re.M).group(1))
    table = re.search(r"^def_kwargs_cg_lanczos_shift = \((.*?)\)\n\n", src, flags=re.M | re.S).group(1)
    defaults = {m.group(1): m.group(2) for m in re.finditer(r":\(;\s*(\w+)(?:::[^=]+?)?\s*=\s*(.*?)\s*\)\s*[,)]?\s*$", table, flags=re.M)}
    assert list(defaults) == names
    mine = K.FORWARDED_DEFAULTS["cg_lanczos_shift"]
    assert list(mine) == names, (list(mine), names)
    values = {"I": None, "false": False, "true": True, "√eps(T)": math.sqrt(np.finfo(np.float64).eps), "Inf": math.inf,
              "kstdout": None, "0": 0}
    for k, expr in defaults.items():
        if expr == "workspace -> false":
            assert mine[k] is K.default_callback and K._user_callback(mine[k]) is None
        else:
            want = values[expr]
            assert mine[k] == want and type(mine[k]) is type(want), (k, mine[k], want)
    assert "cg_lanczos_shift" not in K.WORKSPACE_KWARGS


def test_python_mirror_exports_cg_lanczos_shift():
    import krylov_jl_amd as K
    for sym in ("khip_cg_lanczos_shift_workspace_create", "khip_cg_lanczos_shift_workspace_adopt", "khip_cg_lanczos_shift_solve",
                "khip_cg_lanczos_shift_residuals", "khip_cg_lanczos_shift_arrays", "khip_cg_lanczos_shift_last_path"):
        assert sym in K.SIGNATURES and hasattr(K.lib(), sym), sym
    assert K._INPLACE[K.CgLanczosShiftWorkspace] == ("cg_lanczos_shift", K.cg_lanczos_shift_)


# ---- the Julia specialisation (no Julia here: its gate evaluated as in tests/test_abi.py) ---------------------------------------
def test_julia_gate_takes_the_native_branch_for_the_forwarded_defaults():
    glue = open(JULIA_SRC).read()
    m = re.search(r"function Krylov\.cg_lanczos_shift!\(ws::CgLanczosShiftWs, A::HIPCsr, b::HIPVector, shifts::AbstractVector\{Float64\};"
                  r"(.*?)\)\n  if (.*?)\n(.*?)\nend\n", glue, flags=re.S)
    assert m, "no specialised cg_lanczos_shift! method"
    sig, gate, body = m.groups()
    for kw in ("M", "ldiv", "check_curvature", "atol", "rtol", "itmax", "timemax", "verbose", "history", "callback", "iostream"):
        assert re.search(r"\b" + kw + r"\b", sig), kw
    assert "callback" not in gate
    assert "const CgLanczosShiftWs = CgLanczosShiftWorkspace{Float64,Float64,HIPVector}" in glue
    assert "invoke(Krylov.cg_lanczos_shift!, Tuple{CgLanczosShiftWs,Any,AbstractVector{Float64},AbstractVector{Float64}}" in body
    assert "user_callback(callback)" in body and "NATIVE_SOLVES[] += 1" in body and "khip_cg_lanczos_shift_last_path" in body
    I, kstdout = object(), object()
    env = {"native_precond": lambda M: M is I, "native_log": lambda verbose, io: verbose <= 0 or io is kstdout}
    py = gate.replace("||", " or ").replace("&&", " and ").replace("!==", " is not ").replace("===", " is ")
    py = re.sub(r"!(?=[\w(])", " not ", py)
    scope = dict(env, M=I, ldiv=False, verbose=0, iostream=kstdout)
    assert eval(py, {"__builtins__": {}}, scope) is False, gate
    for k, v in (("ldiv", True), ("M", object()), ("verbose", 1)):
        s2 = dict(scope)
        s2[k] = v
        if k == "verbose":
            s2["iostream"] = object()                # an IOBuffer: no file descriptor
        assert eval(py, {"__builtins__": {}}, s2) is True, (k, gate)
    rt = open(os.path.join(ROOT, "julia", "KrylovHIP", "test", "runtests.jl")).read()
    for entry in ("cg_lanczos_shift(A_gpu, b, shifts)", "krylov_solve(Val(:cg_lanczos_shift), A_gpu, b, shifts)"):
        assert re.search(r"native\(2\) do; " + re.escape(entry), rt), entry
