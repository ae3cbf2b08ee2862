"""symmlq! without a GPU: the NumPy restatement (tests/symmlq_reference.py) against the reference's own test problems
(test/test_symmlq.jl) and its error estimates, the case list of the GPU tests with the condition that admits a case to their
history-parity list, the Python mirror's tables and the header against src/symmlq.jl, and the Julia specialisation's shape (as text:
Julia does not run here)."""
import math
import os
import re
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import symmlq_reference as sr  # noqa: E402
from test_bilq_host import rhs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_SRC = "/root/reference/src"
JULIA_SRC = os.path.join(ROOT, "julia", "KrylovHIP", "src", "KrylovHIP.jl")
GOLD = os.path.join(ROOT, "tests", "golden")
ref_tree = pytest.mark.skipif(not os.path.isdir(REFERENCE_SRC), reason="the reference tree is only present in the build container")


@pytest.fixture(autouse=True)
def _the_feature_is_there():
    """The restatement checks symmlq!: without the mirror's entry points there is nothing for it to check, and every test here fails."""
    import krylov_jl_amd as K
    assert hasattr(K, "symmlq") and hasattr(K, "symmlq_") and hasattr(K, "SymmlqWorkspace")


# ---- operators -------------------------------------------------------------------------------------------------------------------
def tridiag(n, diag=2.0, off=-1.0):
    return sp.diags([np.full(max(n - 1, 0), off), np.full(n, diag), np.full(max(n - 1, 0), off)], [-1, 0, 1], format="csr")


_SP = {}


def case_matrix(oracle, kind, size):
    """The SciPy CSR operator of a case, built once."""
    if (kind, size) not in _SP:
        if kind == "poisson":                                         # get_div_grad(size, size, size)
            S = oracle.poisson3d(size).to_scipy()
        elif kind == "poisson_shifted":                               # A - 0.5 I assembled: one negative eigenvalue (6 - 6 cos(π/9) = 0.36)
            S = (oracle.poisson3d(size).to_scipy() - 0.5 * sp.identity(size ** 3)).tocsr()
        elif kind == "tridiag":
            S = tridiag(size)
        elif kind == "mtx":
            from scipy.io import mmread
            S = sp.csr_matrix(mmread(os.path.join(GOLD, "tiny_spd_sym.mtx")))
        else:                                                         # symmetric_breakdown (test/test_utils.jl:188-192)
            S = sp.csr_matrix(np.array([[0.0, 1.0], [1.0, 0.0]]))
        S.sort_indices()
        _SP[(kind, size)] = S
    return _SP[(kind, size)]


def case_rhs(kind, n):
    return np.array([1.0, 0.0]) if kind == "breakdown" else rhs(n)


# ---- the GPU tests' case list (tests/test_gpu_symmlq.py imports it) --------------------------------------------------------------
# name -> (operator, size parameter, keywords of symmlq).  λ = -0.5 lies inside the spectrum of get_div_grad(8³) (0.36 ... 11.6) and of
# get_div_grad(9³) (0.29 ... 11.7): A + λI is indefinite.  The reference's recurrence subtracts α v with α = vᴴAv + λ (:300-303) from
# A v, not from (A + λI) v, so with λ ≠ 0 its iterates do not solve the shifted system (true residual 0.69 ‖b‖ on poisson8_lam):
# the λ cases pin the restated recurrence, poisson8_shifted (the same operator assembled) is the indefinite solve with a true residual.
CASES = {
    "poisson8": ("poisson", 8, {}),                                   # n = 512
    "poisson9": ("poisson", 9, {}),                                   # n = 729: odd, the tail element
    "poisson8_lam": ("poisson", 8, dict(lam=-0.5)),
    "poisson9_lam": ("poisson", 9, dict(lam=-0.5)),
    "poisson8_shifted": ("poisson_shifted", 8, dict(atol=0.0, rtol=1e-10)),
    "poisson8_lq": ("poisson", 8, dict(transfer_to_cg=False)),
    "mtx": ("mtx", 0, {}),                                            # tiny_spd_sym.mtx, n = 42: ends at the CG point
    "mtx_lq": ("mtx", 0, dict(transfer_to_cg=False)),
    "tri1": ("tridiag", 1, {}),                                       # n = 1: β₂ = 0, the Lanczos breakdown in its smallest form
    "tri2": ("tridiag", 2, {}),
    "tri3": ("tridiag", 3, {}),
    "tri63": ("tridiag", 63, {}),
    "tri64": ("tridiag", 64, {}),
    "tri65": ("tridiag", 65, {}),
    "breakdown": ("breakdown", 2, {}),
}
INDEFINITE = ("poisson8_lam", "poisson9_lam", "poisson8_shifted", "breakdown")
# recorded from the restatement (np.dot and math.fsum dots agree on every one)
EXPECTED_NITER = {"poisson8": 21, "poisson9": 22, "poisson8_lam": 33, "poisson9_lam": 36, "poisson8_shifted": 35, "poisson8_lq": 21,
                  "mtx": 19, "mtx_lq": 19, "tri1": 2, "tri2": 1, "tri3": 2, "tri63": 62, "tri64": 63, "tri65": 62, "breakdown": 1}
# tri63 and tri64 end when the Krylov space is exhausted (n - 1 iterations): their last history entries are rounding noise (the
# restatement's own deviation is 0.2 ... 0.5), so they serve path 1 = path 2 only
PARITY_CAP = 1e-6
PARITY_CASES = ("poisson8", "poisson9", "poisson8_lam", "poisson9_lam", "poisson8_shifted", "poisson8_lq", "mtx", "mtx_lq", "tri1",
                "tri2", "tri3", "tri65", "breakdown")


def deviation(s1, s2):
    """Largest relative difference of the residuals and residualscg histories of two runs; inf when the lengths or the places of
    the NaN (missing) entries differ."""
    out = 0.0
    for k in ("residuals", "residualscg"):
        a, b = np.asarray(getattr(s1, k)), np.asarray(getattr(s2, k))
        if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
            return math.inf
        m = ~np.isnan(a)
        if m.any():
            out = max(out, sr.history_deviation(a[m], b[m]))
    return out


_PAIRS = {}


def reference_pair(oracle, name, **extra):
    """(restatement with np.dot, restatement with exactly summed dots) of a case, as (x, stats) pairs; computed once."""
    key = (name, tuple(sorted((k, id(v) if callable(v) else repr(v)) for k, v in extra.items())))
    if key not in _PAIRS:
        kind, size, kw = CASES[name]
        S = case_matrix(oracle, kind, size)
        b = case_rhs(kind, S.shape[0])
        kw = dict(kw, **extra)
        _PAIRS[key] = (sr.symmlq(S, b, **kw), sr.symmlq(S, b, dot=sr.fsum_dot, **kw))
    return _PAIRS[key]


@pytest.mark.parametrize("name", list(CASES))
def test_case_list(oracle, name):
    """Every case ends in the recorded number of iterations with the same status whichever way the dots are rounded; its
    np.dot-against-fsum deviation is printed."""
    (x1, s1), (x2, s2) = reference_pair(oracle, name)
    dev = deviation(s1, s2)
    print(f"{name}: np.dot against fsum, largest relative history deviation {dev:.3e}; {s1.niter} iterations, {s1.status}")
    assert s1.niter == s2.niter == EXPECTED_NITER[name], (s1.niter, s2.niter)
    assert s1.status == s2.status and s1.solved == s2.solved
    assert len(s1.residuals) == len(s1.residualscg) == s1.niter + 1
    assert len(s1.errors) == len(s1.errorscg) == 0                     # λest = 0: no error estimates


def test_parity_list_condition(oracle):
    """Only cases whose own np.dot-against-fsum history deviation is <= 1e-6 are in the history-parity list; no case that
    qualifies was left out; the list is not empty and holds an indefinite case."""
    assert len(PARITY_CASES) > 0 and set(PARITY_CASES) <= set(CASES)
    assert set(PARITY_CASES) & set(INDEFINITE)
    for name in CASES:
        (_, s1), (_, s2) = reference_pair(oracle, name)
        dev = deviation(s1, s2)
        assert (dev <= PARITY_CAP) == (name in PARITY_CASES), (name, dev)


def test_indefinite_cases_are_indefinite(oracle):
    for name in ("poisson8_lam", "poisson9_lam", "poisson8_shifted"):
        kind, size, kw = CASES[name]
        S = case_matrix(oracle, kind, size)
        lo = spla.eigsh(S, k=2, which="SA", return_eigenvectors=False)
        hi = spla.eigsh(S, k=1, which="LA", return_eigenvectors=False)
        lam = kw.get("lam", 0.0)
        assert min(lo) + lam < 0 < max(lo) + lam < hi[0] + lam, (name, lo, hi)


def test_true_residuals_of_the_case_list(oracle):
    """What the histories mean, on the restatement: residualscg[end] is the true residual of the CG point (mtx); residuals[k] is the
    true residual of the LQ iterate BEFORE iteration k (the reference's rNorm lags one iterate), so a run stopped after k - 1
    iterations has that residual; the indefinite solve converges."""
    (x, s), _ = reference_pair(oracle, "mtx")
    S = case_matrix(oracle, "mtx", 0)
    b = rhs(S.shape[0])
    assert s.status == sr.SOLVED_CG and s.solved_cg
    assert abs(np.linalg.norm(b - S @ x) - s.residualscg[-1]) <= 1e-8 * np.linalg.norm(b)
    (xl, sl), _ = reference_pair(oracle, "mtx_lq")
    assert sl.status == sr.SOLVED and not np.array_equal(xl, x) and np.array_equal(xl, s.xlq)
    k = 6
    (x5, s5), _ = reference_pair(oracle, "mtx_lq", itmax=k - 1)
    assert abs(np.linalg.norm(b - S @ x5) - sl.residuals[k]) <= 1e-10 * np.linalg.norm(b)
    (xs, ss), _ = reference_pair(oracle, "poisson8_shifted")
    Ss = case_matrix(oracle, "poisson_shifted", 8)
    bs = rhs(512)
    assert ss.solved and _reference_bound(Ss, bs, xs)                  # the reference's bound: resid ≤ 1e-6 ‖A‖ ‖x‖


# ---- the reference's own test problems (test/test_symmlq.jl, test/test_utils.jl), Float64 ---------------------------------------
def _reference_bound(A, b, x):
    """resid ≤ symmlq_tol ‖A‖ ‖x‖ with resid = ‖b - A x‖ / ‖b‖ (test/test_symmlq.jl:11-13); Julia's norm(A) of a matrix is the
    Frobenius norm."""
    fro = spla.norm(A) if sp.issparse(A) else np.linalg.norm(np.asarray(A))
    resid = np.linalg.norm(b - A @ x) / np.linalg.norm(b)
    print(f"resid {resid:.3e}, bound {1.0e-6 * fro * np.linalg.norm(x):.3e}")
    return resid <= 1.0e-6 * fro * np.linalg.norm(x)


def test_symmetric_definite():
    A = tridiag(10, 4.0, 1.0)
    b = A @ np.arange(1.0, 11.0)
    x, st = sr.symmlq(A, b)
    assert st.solved and _reference_bound(A, b, x)


def test_symmetric_indefinite():
    A = tridiag(10, 1.0, 1.0)
    b = A @ np.arange(1.0, 11.0)
    assert min(np.linalg.eigvalsh(A.toarray())) < 0
    x, st = sr.symmlq(A, b)
    assert st.solved and _reference_bound(A, b, x)


def test_sparse_laplacian(oracle):
    A = oracle.poisson3d(16).to_scipy()
    b = np.ones(16 ** 3)
    x, st = sr.symmlq(A, b)
    assert st.solved and _reference_bound(A, b, x)


def test_symmetric_breakdown():
    A = np.array([[0.0, 1.0], [1.0, 0.0]])
    b = np.array([1.0, 0.0])
    x, st = sr.symmlq(A, b)
    assert st.solved and _reference_bound(A, b, x) and np.array_equal(x, [0.0, 1.0])
    assert np.isnan(st.residualscg[0]) and not np.isnan(st.residualscg[1])          # γbar₁ = 0: no CG point before iteration 1
    assert np.isnan(st.vectors["Mv"]).all()                                          # β₃ = 0: v₃ = 0 / 0


def test_zero_right_hand_side():
    x, st = sr.symmlq(np.random.default_rng(0).random((10, 10)), np.zeros(10))
    assert np.linalg.norm(x) == 0 and st.status == "x is a zero-residual solution" and st.niter == 0 and st.solved
    assert list(st.residuals) == [0.0] and list(st.residualscg) == [0.0] and math.isnan(st.Anorm) and math.isnan(st.Acond)


def test_square_preconditioned():
    n = 10
    A = np.ones((n, n)) + (n - 1) * np.eye(n)
    b = 10.0 * np.arange(1.0, n + 1)
    x, st = sr.symmlq(A, b, M=(1.0 / n) * np.eye(n))
    assert st.solved and _reference_bound(A, b, x)
    # M = -I: β₁² = ⟨b, M b⟩ < 0, and the reference takes its square root before any check (:193: a DomainError there)
    with pytest.raises(ValueError, match="math domain error"):
        sr.symmlq(A, b, M=-np.eye(n))
    # ⟨b, M b⟩ > 0 but ⟨v₂, M v₂⟩ < 0: the reference's own check (:205)
    with pytest.raises(ValueError, match="Preconditioner is not positive definite"):
        sr.symmlq(np.array([[0.0, 1.0], [1.0, 0.0]]), np.array([1.0, 0.25]), M=np.diag([1.0, -1.0]))


def _cg(A, b):
    """cg(A, b) with the reference's default tolerances (src/cg.jl), for test/test_symmlq.jl:52."""
    x, r = np.zeros_like(b), b.copy()
    p, g = r.copy(), float(r @ r)
    eps = math.sqrt(sr.EPS) * (1.0 + math.sqrt(g))
    while math.sqrt(g) > eps:
        Ap = A @ p
        a = g / float(p @ Ap)
        x, r = x + a * p, r - a * Ap
        g, g0 = float(r @ r), g
        p = r + (g / g0) * p
    return x


def test_error_estimates(oracle):
    """test/test_symmlq.jl:46-62: on get_div_grad(8, 8, 8) with λest = (1 - 1e-10) eigmin(A), ‖x* - xᴸ‖ ≤ errors[end] and
    ‖x* - xᶜ‖ ≤ errorscg[end], with the default window, window = 1 and window = 5."""
    A = oracle.poisson3d(8).to_scipy()
    b = np.ones(512)
    dense = A.toarray()
    lam_est = (1 - 1e-10) * float(np.linalg.eigvalsh(dense)[0])
    x_exact = np.linalg.solve(dense, b)
    xlq, st = sr.symmlq(A, b, lam_est=lam_est, transfer_to_cg=False)
    err = np.linalg.norm(x_exact - xlq)
    errcg = np.linalg.norm(x_exact - _cg(A, b))
    assert len(st.errors) == len(st.errorscg) == st.niter + 1
    assert err <= st.errors[-1] and errcg <= st.errorscg[-1]
    for window in (1, 5):
        x, st = sr.symmlq(A, b, lam_est=lam_est, window=window)
        print(f"window {window}: {st.niter} iterations, errors[end] {st.errors[-1]:.3e} >= {err:.3e}, errorscg[end] "
              f"{st.errorscg[-1]:.3e} >= {errcg:.3e}")
        assert err <= st.errors[-1] and errcg <= st.errorscg[-1]
        assert np.all(np.diff(st.errors) <= 0)                          # the bound on the LQ error decreases


def test_warm_start_and_callback_of_the_restatement(oracle):
    S = case_matrix(oracle, "poisson", 8)
    b = rhs(512)
    x0 = np.linspace(-0.5, 0.5, 512)
    for lam in (0.0, -0.5):
        x, st = sr.symmlq(S, b, x0=x0, lam=lam)
        _, s0 = sr.symmlq(S, b - S @ x0 - lam * x0, lam=lam)
        assert st.niter == s0.niter and np.allclose(st.residuals, s0.residuals, rtol=1e-12, atol=0)
    seen = []
    x, st = sr.symmlq(S, b, callback=lambda w: (seen.append(len(w.stats.residuals)), len(seen) == 2)[1])
    assert seen == [2, 3] and st.niter == 2 and st.status == "user-requested exit"


# ---- the Python mirror's tables and the header -----------------------------------------------------------------------------------
SYMMLQ_SYMBOLS = ("khip_symmlq_default_params", "khip_symmlq_workspace_create", "khip_symmlq_workspace_adopt",
                  "khip_symmlq_workspace_adopt_vector", "khip_symmlq_workspace_destroy", "khip_symmlq_warm_start", "khip_symmlq_solve",
                  "khip_symmlq_solution", "khip_symmlq_stats", "khip_symmlq_histories", "khip_symmlq_norms", "khip_symmlq_last_path",
                  "khip_symmlq_vector", "khip_symmlq_workspace_bytes")


def test_python_mirror_exports_symmlq():
    """The mirror has the whole SYMMLQ surface (fails before the feature: K.symmlq did not exist)."""
    import krylov_jl_amd as K
    for name in ("symmlq", "symmlq_", "SymmlqWorkspace"):
        assert hasattr(K, name), name
    for sym in SYMMLQ_SYMBOLS:
        assert sym in K.SIGNATURES, sym
        assert hasattr(K.lib(), sym), sym
    assert K._INPLACE[K.SymmlqWorkspace] == ("symmlq", K.symmlq_)
    assert K.SYMMLQ_WORKSPACE_KWARGS == {"window": 5} and "symmlq" not in K.WORKSPACE_KWARGS
    assert K.SymmlqWorkspace.VECTORS == ("x", "Mvold", "Mv", "Mv_next", "wbar")
    assert len(K.SIGNATURES["khip_symmlq_workspace_adopt"][1]) == 4 + 5 + 1
    assert [f[0] for f in K.CSymmlqParams._fields_] == ["lambda_", "lambda_est", "etol", "conlim", "transfer_to_cg"]
    prm = K.lib().khip_symmlq_default_params()
    assert prm.lambda_ == 0.0 and prm.lambda_est == 0.0 and math.isnan(prm.etol) and math.isnan(prm.conlim) and prm.transfer_to_cg == 1


def test_header_declares_the_symmlq_entries():
    """include/krylov_hip.h: every entry once, adopt with the five core vectors in the order of SymmlqWorkspace, the parameter
    struct's fields in the mirror's order, `missing` = NaN said, the ABI version untouched."""
    header = open(os.path.join(ROOT, "include", "krylov_hip.h"), encoding="utf-8").read()
    for sym in SYMMLQ_SYMBOLS:
        assert len(re.findall(r"^[\w ]+\*?" + sym + r"\(", header, flags=re.M)) == 1, sym
    adopt = re.search(r"int khip_symmlq_workspace_adopt\(khip_ctx \*ctx, int64_t m, int64_t n, int window, (.*?),\s*"
                      r"khip_symmlq_workspace \*\*out\);", header, flags=re.S)
    assert adopt and re.findall(r"double \*(\w+)", adopt.group(1)) == ["x", "Mvold", "Mv", "Mv_next", "wbar"]
    struct = re.search(r"typedef struct \{([^{}]*?)\} khip_symmlq_params;", header, flags=re.S).group(1)
    struct = re.sub(r"/\*.*?\*/", "", struct, flags=re.S)
    assert re.findall(r"(double|int) (\w+);", struct) == [("double", "lambda"), ("double", "lambda_est"), ("double", "etol"),
                                                          ("double", "conlim"), ("int", "transfer_to_cg")]
    solve = re.search(r"int khip_symmlq_solve\((.*?)\);", header, flags=re.S).group(1)
    assert re.findall(r"\*(\w+)(?:,|$)", solve) == ["ws", "A", "M", "b", "opts", "params"]
    assert '"x", "Mvold", "Mv", "Mv_next", "wbar", "dx", "v"' in header
    assert "`missing`" in header and "NaN" in header
    assert "#define KHIP_VERSION_MINOR 4" in header
    for status in (sr.SOLVED_LQ, sr.SOLVED_CG):
        assert status in header


@ref_tree
def test_forwarded_defaults_equal_the_reference():
    """FORWARDED_DEFAULTS["symmlq"] = kwargs_symmlq / def_kwargs_symmlq of src/symmlq.jl, names in order, defaults as values; the
    workspace keyword is kwargs_workspace_symmlq."""
    import krylov_jl_amd as K
    src = open(os.path.join(REFERENCE_SRC, "symmlq.jl")).read()
    names = re.findall(r":(\w+)", re.search(r"^kwargs_symmlq = \((.*?)\)", src, flags=re.M).group(1))
    table = re.search(r"^def_kwargs_symmlq = \((.*?)\)\n\n", src, flags=re.M | re.S).group(1)
    defaults = {m.group(1): m.group(2) for m in
                re.finditer(r":\(;\s*(\w+)(?:::[^=]+?)?\s*=\s*(.*?)\s*\)\s*[,)]?\s*$", table, flags=re.M)}
    assert list(defaults) == names
    mine = K.FORWARDED_DEFAULTS["symmlq"]
    assert list(mine) == names
    sq = math.sqrt(np.finfo(np.float64).eps)
    value = {"I": None, "false": False, "true": True, "zero(T)": 0.0, "√eps(T)": sq, "1/√eps(T)": 1 / sq, "0": 0, "Inf": math.inf,
             "kstdout": None}
    for k, expr in defaults.items():
        if k == "callback":
            assert expr == "workspace -> false" and mine[k] is K.default_callback
        else:
            assert mine[k] == value[expr] and type(mine[k]) is type(value[expr]), (k, expr, mine[k])
    wk = re.search(r"^kwargs_workspace_symmlq = \((.*?)\)", src, flags=re.M).group(1)
    assert re.findall(r":(\w+)", wk) == list(K.SYMMLQ_WORKSPACE_KWARGS)
    assert "def_kwargs_workspace_symmlq = (:(; window::Int = 5),)" in src
    # the restatement's own defaults are the same
    import inspect
    sig = inspect.signature(sr.symmlq).parameters
    for k, mk in (("transfer_to_cg", "transfer_to_cg"), ("lam", "λ"), ("lam_est", "λest"), ("atol", "atol"), ("rtol", "rtol"),
                  ("etol", "etol"), ("conlim", "conlim"), ("itmax", "itmax"), ("timemax", "timemax")):
        assert sig[k].default == mine[mk], k
    assert sig["window"].default == 5


# ---- the Julia glue, as text -----------------------------------------------------------------------------------------------------
def _julia_symmlq():
    glue = open(JULIA_SRC, encoding="utf-8").read()
    m = re.search(r"function Krylov\.symmlq!\(ws::SymmlqWs, A::HIPCsr, b::HIPVector;(.*?)\)\n(.*?)\nend\n", glue, flags=re.S)
    assert m, "no specialised Krylov.symmlq!"
    return glue, m.group(1), m.group(2)


def test_julia_symmlq_specialisation_shape():
    """The Julia symmlq!: the SymmlqWs alias, the five adopted vectors in the order of khip_symmlq_workspace_adopt with the window's
    length, the lazy vectors handed over by name, the fallback gate, the forwarded default callback, LAST_PATH, the parameter
    struct in the header's order, NaN back to missing, and test/symmlq.jl reached from runtests.jl."""
    glue, sig, body = _julia_symmlq()
    assert "const SymmlqWs = SymmlqWorkspace{Float64,Float64,HIPVector}" in glue
    adopt = re.search(r"ccall\(\(:khip_symmlq_workspace_adopt, lib\), Cint,\s*\((.*?)\),\n\s+CTX\[\]\.h, ws\.m, ws\.n, (.*?), r\)\)", glue,
                      flags=re.S)
    assert adopt, "symmlq_handle does not adopt the workspace's vectors"
    assert adopt.group(1).count("Ptr{Cdouble}") == 5
    assert [a.strip() for a in adopt.group(2).split(",")] == ["length(ws.clist)"] + [f"ws.{f}.ptr" for f in
                                                                                     ("x", "Mvold", "Mv", "Mv_next", "w̅")]
    assert re.search(r"struct SymmlqParams[^\n]*\n\s+lambda::Cdouble; lambda_est::Cdouble; etol::Cdouble; conlim::Cdouble; "
                     r"transfer_to_cg::Cint\nend", glue)
    assert "SymmlqParams(λ, λest, etol, conlim, transfer_to_cg)" in body
    assert 'for (name, v) in (("v", ws.v), ("dx", ws.Δx))\n    symmlq_adopt(h, name, v)' in body
    assert "if ldiv || !native_precond(M) || !native_log(verbose, iostream)" in body
    assert "invoke(Krylov.symmlq!, Tuple{SymmlqWs,Any,AbstractVector{Float64}}, ws, A, b;" in body
    assert "callback = callback === nothing ? (w -> false) : callback" in body
    assert "callback_args(user_callback(callback), ws, sp, history)" in body
    assert "NATIVE_SOLVES[] += 1" in body and "LAST_PATH[] = ccall((:khip_symmlq_last_path, lib)" in body
    assert "khip_symmlq_warm_start" in body and "ws.warm_start = false" in body
    assert "khip_symmlq_histories" in body and "khip_symmlq_norms" in body
    assert "isnan(v) ? missing : v" in body and "ws.stats.Anorm" in body and "ws.stats.Acond" in body
    assert "callback = nothing" in sig and "fused::Int = 2" in sig
    assert ("ccall((:khip_symmlq_solve, lib), Cint,\n" in body and
            "(Ptr{Cvoid}, Ref{Operator}, Ptr{Operator}, Ptr{Cdouble}, Ref{Options}, Ptr{Cvoid})" in body)
    tests = os.path.join(ROOT, "julia", "KrylovHIP", "test")
    symmlq_jl = open(os.path.join(tests, "symmlq.jl"), encoding="utf-8").read()
    for piece in ("SymmlqWorkspace(n, n, S)", "native(2) do; symmlq!(ws, A_gpu, b; history = true); end", "generic_symmlq(ws2, A_gpu, b;",
                  "symmetric_breakdown()", "SYMMLQ: system of size $n", "λest = λest", "ismissing"):
        assert piece in symmlq_jl, piece
    runtests = open(os.path.join(tests, "runtests.jl"), encoding="utf-8").read()
    assert 'include("symmlq.jl")' in runtests


@ref_tree
def test_julia_symmlq_specialisation():
    """Against the reference tree: every keyword of kwargs_symmlq is in the signature and forwarded to the generic method, and the
    glue reads only fields of SymmlqWorkspace (src/krylov_workspaces.jl:461-476), all seven vectors among them."""
    glue, sig, body = _julia_symmlq()
    src = open(os.path.join(REFERENCE_SRC, "symmlq.jl")).read()
    names = re.findall(r":(\w+)", re.search(r"^kwargs_symmlq = \((.*?)\)", src, flags=re.M).group(1))
    fallback = re.search(r"invoke\(Krylov\.symmlq!, Tuple\{SymmlqWs,Any,AbstractVector\{Float64\}\}, ws, A, b;(.*?)\)\n  end", body,
                         flags=re.S).group(1)
    for kw in names:
        assert re.search(r"(?<![\w])" + kw + r"(?![\w])", sig), f"symmlq!: keyword {kw} of the reference is missing"
        assert re.search(r"(?<![\w])" + kw + r"(?![\w])", fallback), f"symmlq!: keyword {kw} is not forwarded to the generic method"
    ws_src = open(os.path.join(REFERENCE_SRC, "krylov_workspaces.jl")).read()
    struct = re.search(r"mutable struct SymmlqWorkspace\{T,FC,S\}.*?\nend", ws_src, flags=re.S).group(0)
    fields = set(re.findall(r"^\s+(\S+)\s+::", struct, flags=re.M))
    used = set(re.findall(r"\bws\.([^\s.,;()\[\]]+)", body))
    handle = re.search(r"function symmlq_handle\(ws::SymmlqWs\)\n(.*?)\nend\n", glue, flags=re.S).group(1)
    used |= set(re.findall(r"\bws\.([^\s.,;()\[\]]+)", handle))
    assert used <= fields, used - fields
    assert {"x", "Mvold", "Mv", "Mv_next", "w̅", "Δx", "v", "clist"} <= used
    stats_src = open(os.path.join(REFERENCE_SRC, "krylov_stats.jl")).read()
    sstruct = re.search(r"mutable struct SymmlqStats\{T\}.*?\nend", stats_src, flags=re.S).group(0)
    for f in ("residuals", "residualscg", "errors", "errorscg", "Anorm", "Acond"):
        assert re.search(r"^\s+" + f + r"\s+::", sstruct, flags=re.M), f
        assert f"ws.stats.{f}" in body or f == "residuals", f
