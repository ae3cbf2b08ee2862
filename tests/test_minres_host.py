"""minres! without a GPU: the NumPy restatement (tests/minres_reference.py) against the reference's own known answers and
against SciPy, the Python mirror's tables against src/minres.jl, and the Julia specialisation's shape."""
import math
import os
import re
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import minres_reference as mr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_SRC = "/root/reference/src"
JULIA_SRC = os.path.join(ROOT, "julia", "KrylovHIP", "src", "KrylovHIP.jl")
ref_tree = pytest.mark.skipif(not os.path.isdir(REFERENCE_SRC), reason="the reference tree is only present in the build container")


def _tridiag(n, diag=2.0, off=-1.0):
    return sp.diags([np.full(n - 1, off), np.full(n, diag), np.full(n - 1, off)], [-1, 0, 1], format="csr")


def _err_ones(x):
    return np.linalg.norm(x - 1.0) / math.sqrt(len(x))


# ---- the reference's known answers, restated as data ---------------------------------------------------------------------
def test_spd_tridiagonal_of_the_c_interface_suite():
    """interfaces/test/C/test_all_solvers.c:134,264-275: A = tridiag(-1, 2, -1), n = 20, b = A ones, default options."""
    A = _tridiag(20)
    x, st = mr.minres(A, A @ np.ones(20))
    assert st.solved and _err_ones(x) <= 1e-6, (st.status, _err_ones(x))


def test_shifted_problem_of_the_c_api_suite():
    """interfaces/test/C/test_api.c:392-400: (A + 0.5 I) x = A ones + 0.5, n = 32, atol = rtol = 1e-10."""
    A = _tridiag(32)
    x, st = mr.minres(A, A @ np.ones(32) + 0.5, lam=0.5, atol=1e-10, rtol=1e-10)
    assert st.solved and _err_ones(x) < 1e-6


def test_window_one_of_the_c_api_suite():
    """interfaces/test/C/test_api.c:324-340: window = 1, n = 24, atol = rtol = 1e-10."""
    A = _tridiag(24)
    x, st = mr.minres(A, A @ np.ones(24), atol=1e-10, rtol=1e-10, window=1)
    assert st.solved and _err_ones(x) < 1e-6


def test_restatement_agrees_with_scipy_on_an_indefinite_matrix():
    """A symmetric indefinite matrix (shifted 2-D Laplacian, shift inside the spectrum): same solution as scipy's MINRES."""
    n1 = 12
    L = sp.kronsum(_tridiag(n1), _tridiag(n1)).tocsr()
    A = (L - 2.3 * sp.identity(n1 * n1)).tocsr()
    b = np.cos(np.arange(n1 * n1))
    x, st = mr.minres(A, b, atol=0.0, rtol=1e-13, itmax=2000)
    xs, info = spla.minres(A, b, rtol=1e-13, maxiter=2000)
    assert info == 0
    x_exact = spla.spsolve(A.tocsc(), b)
    assert np.linalg.norm(x - xs) <= 1e-10 * np.linalg.norm(x_exact)
    assert np.linalg.norm(x - x_exact) <= 1e-9 * np.linalg.norm(x_exact)
    assert st.residuals.size == st.niter + 1 == st.Aresiduals.size == st.Acond.size


def test_restatement_exits():
    """b = 0 and an eigenvector right-hand side end where the reference says (:233-244, :410-419)."""
    A = _tridiag(16)
    x, st = mr.minres(A, np.zeros(16))
    assert st.niter == 1 and st.status == "x is a zero-residual solution" and not x.any()
    x, st = mr.minres(sp.identity(8, format="csr") * 0.0, np.ones(8))
    assert st.niter == 1 and st.status == "x is a minimum least-squares solution" and st.inconsistent


# ---- the Python mirror's tables --------------------------------------------------------------------------------------------
def test_python_mirror_exports_minres():
    """The mirror has the whole MINRES surface (fails before the feature: K.minres did not exist)."""
    import krylov_jl_amd as K
    for name in ("minres", "minres_", "MinresWorkspace"):
        assert hasattr(K, name), name
    for sym in ("khip_minres_workspace_create", "khip_minres_workspace_adopt", "khip_minres_workspace_adopt_vector",
                "khip_minres_workspace_destroy", "khip_minres_warm_start", "khip_minres_solve", "khip_minres_solution",
                "khip_minres_stats", "khip_minres_histories", "khip_minres_last_path", "khip_minres_vector",
                "khip_minres_workspace_bytes", "khip_minres_default_params"):
        assert sym in K.SIGNATURES, sym
    assert K.MINRES_WORKSPACE_KWARGS == {"window": 5}
    assert "minres" not in K.WORKSPACE_KWARGS


@ref_tree
def test_forwarded_defaults_equal_the_reference():
    """FORWARDED_DEFAULTS["minres"] = kwargs_minres / def_kwargs_minres of src/minres.jl, names in order, defaults as values."""
    import krylov_jl_amd as K
    src = open(os.path.join(REFERENCE_SRC, "minres.jl")).read()
    names = re.findall(r":(\w+)", re.search(r"^kwargs_minres = \((.*?)\)", src, flags=re.M).group(1))
    table = re.search(r"^def_kwargs_minres = \((.*?)\)\n\n", src, flags=re.M | re.S).group(1)
    defaults = {m.group(1): m.group(2) for m in
                re.finditer(r":\(;\s*(\w+)(?:::[^=]+?)?\s*=\s*(.*?)\s*\)\s*[,)]?\s*$", table, flags=re.M)}
    assert list(defaults) == names
    mine = K.FORWARDED_DEFAULTS["minres"]
    assert list(mine) == names
    sq = math.sqrt(np.finfo(np.float64).eps)
    value = {"I": None, "false": False, "zero(T)": 0.0, "√eps(T)": sq, "1/√eps(T)": 1 / sq, "0": 0, "Inf": math.inf,
             "kstdout": None}
    for k, expr in defaults.items():
        if k == "callback":
            assert expr == "workspace -> false" and mine[k] is K.default_callback
        else:
            assert mine[k] == value[expr], (k, expr, mine[k])
    wk = re.search(r"^kwargs_workspace_minres = \((.*?)\)", src, flags=re.M).group(1)
    assert re.findall(r":(\w+)", wk) == list(K.MINRES_WORKSPACE_KWARGS)


@ref_tree
def test_julia_minres_specialisation():
    """The Julia minres! has every reference keyword, an invoke fallback, the MinresWs alias, and reads only fields of
    MinresWorkspace (src/krylov_workspaces.jl:77-91)."""
    glue = open(JULIA_SRC).read()
    assert "const MinresWs = MinresWorkspace{Float64,Float64,HIPVector}" in glue
    m = re.search(r"function Krylov\.minres!\(ws::MinresWs, A::HIPCsr, b::HIPVector;(.*?)\)\n(.*?)\nend\n", glue, flags=re.S)
    assert m, "no specialised Krylov.minres!"
    sig, body = m.group(1), m.group(2)
    src = open(os.path.join(REFERENCE_SRC, "minres.jl")).read()
    names = re.findall(r":(\w+)", re.search(r"^kwargs_minres = \((.*?)\)", src, flags=re.M).group(1))
    for kw in names:
        assert re.search(r"(?<![\w])" + kw + r"(?![\w])", sig), f"minres!: keyword {kw} of the reference is missing"
    assert "invoke(Krylov.minres!, Tuple{MinresWs,Any,AbstractVector{Float64}}, ws, A, b;" in body
    assert "NATIVE_SOLVES[] += 1" in body and "khip_minres_last_path" in body
    ws_src = open(os.path.join(REFERENCE_SRC, "krylov_workspaces.jl")).read()
    struct = re.search(r"mutable struct MinresWorkspace\{T,FC,S\}.*?\nend", ws_src, flags=re.S).group(0)
    fields = set(re.findall(r"^\s+(\w+)\s+::", struct, flags=re.M))
    used = set(re.findall(r"\bws\.(\w+)", body))
    assert used <= fields, used - fields
