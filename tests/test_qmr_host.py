"""qmr! without a GPU: the NumPy restatement (tests/qmr_reference.py) against the reference's own known answers, against SciPy and,
on a symmetric operator, against the restatement of minres!; the condition that admits a case to the GPU tests' case list; the
Python mirror's tables against src/qmr.jl; and the Julia specialisation's shape."""
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
import qmr_reference as qr  # noqa: E402
from test_bilq_host import case_operator, case_vectors, other_c, rhs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_SRC = "/root/reference/src"
JULIA_SRC = os.path.join(ROOT, "julia", "KrylovHIP", "src", "KrylovHIP.jl")
ref_tree = pytest.mark.skipif(not os.path.isdir(REFERENCE_SRC), reason="the reference tree is only present in the build container")

SOLVED = qr.SOLVED

# ---- the GPU tests' case list (tests/test_gpu_qmr.py imports it) ----------------------------------------------------------------
# name -> (operator, size parameter, c: None | "neg" | "sin", keywords of qmr)
CASES = {
    "kron7": ("kron", 7, None, {}),
    "kron8": ("kron", 8, None, {}),
    "kron8_negc": ("kron", 8, "neg", {}),
    "kron8_sinc": ("kron", 8, "sin", {}),
    "kron12": ("kron", 12, None, {}),
    "poisson16": ("poisson", 16, None, {}),
    "poisson16_sinc": ("poisson", 16, "sin", {}),
    "kron8_rtol12": ("kron", 8, None, dict(atol=0.0, rtol=1e-12)),
}
EXPECTED_NITER = {"kron7": 34, "kron8": 39, "kron8_negc": 39, "kron8_sinc": 42, "kron12": 56, "poisson16": 66, "poisson16_sinc": 71,
                  "kron8_rtol12": 51}

_PAIRS = {}


def reference_pair(oracle, name, **extra):
    """(restatement with np.dot, restatement with exactly summed dots) of a case, as (x, stats) pairs; computed once."""
    key = (name, tuple(sorted((k, id(v) if callable(v) else repr(v)) for k, v in extra.items())))
    if key not in _PAIRS:
        kind, n1, cname, kw = CASES[name]
        A_cpu = case_operator(oracle, kind, n1)
        S = A_cpu.to_scipy()
        St = S.T.tocsr()
        b, c = case_vectors(A_cpu.n, cname)
        kw = dict(kw, **extra)
        _PAIRS[key] = (qr.qmr(S, b, c=c, At=St, **kw), qr.qmr(S, b, c=c, At=St, dot=qr.fsum_dot, **kw))
    return _PAIRS[key]


@pytest.mark.parametrize("name", list(CASES))
def test_case_list_condition(oracle, name):
    """A case may be in the list only if the restatement with np.dot and with math.fsum dots agree on niter and status and their
    whole residual histories agree to <= 1e-6 relative.  Measured deviations: kron7 2.6e-10, kron8 and kron8_negc 5.2e-12,
    kron8_sinc 8.3e-7, kron12 2.3e-8, poisson16 4.1e-10, poisson16_sinc 3.2e-8, kron8_rtol12 1.2e-9."""
    (x1, s1), (_, s2) = reference_pair(oracle, name)
    dev = qr.history_deviation(s1.residuals, s2.residuals)
    kind, n1, cname, kw = CASES[name]
    A_cpu = case_operator(oracle, kind, n1)
    b = rhs(A_cpu.n)
    true_res = np.linalg.norm(b - A_cpu.matvec(x1)) / np.linalg.norm(b)
    print(f"{name}: n = {A_cpu.n}, niter = {s1.niter} / {s2.niter}, deviation {dev:.1e}, true residual {true_res:.1e} ||b||")
    assert s1.niter == s2.niter == EXPECTED_NITER[name], (s1.niter, s2.niter)
    assert s1.status == s2.status == SOLVED and s1.solved
    assert len(s1.residuals) == s1.niter + 1
    assert dev <= 1e-6
    assert true_res <= 1e-8


# ---- the reference's known answers, restated as data ------------------------------------------------------------------------------
def test_unsymmetric_breakdown():
    """test/test_utils.jl:196-201 with test/test_qmr.jl: x = [0, 1] after two iterations, residual history [1, sqrt(2), 0]."""
    A = np.array([[0.0, 1.0], [-1.0, 0.0]])
    x, st = qr.qmr(A, np.array([1.0, 0.0]), c=np.array([-1.0, 0.0]))
    assert st.niter == 2 and st.status == SOLVED and st.solved
    assert np.allclose(x, [0.0, 1.0], rtol=0, atol=1e-15)
    assert np.allclose(st.residuals, [1.0, math.sqrt(2.0), 0.0], rtol=0, atol=1e-15)


def test_bc_breakdown():
    """test/test_utils.jl:204-209: cᴴb = 0 ends before the first iteration."""
    A = np.array([[1.0, 2.0], [3.0, 4.0]])
    x, st = qr.qmr(A, np.array([0.0, 1.0]), c=np.array([1.0, 0.0]))
    assert st.niter == 0 and st.status == "Breakdown bᴴc = 0" and not st.solved and not x.any()


def test_identity():
    """A = I: the Krylov space ends after one step (pᴴq = 0, βₖ₊₁ = 0, so ζbarₖ₊₁ = 0 and the bound is zero): x = b, solved."""
    b = np.arange(1.0, 6.0)
    x, st = qr.qmr(np.eye(5), b)
    assert st.niter == 1 and st.status == SOLVED and st.solved and np.array_equal(x, b)
    assert st.residuals[1] == 0.0
    assert np.array_equal(st.vectors["v"], st.vectors["v_prev"])            # pᴴq = 0: vₖ and uₖ are left as they are (:344-347)
    assert not st.vectors["w_prev2"].any() and st.vectors["w_prev"].any()   # w₁ sits in wₖ₋₁, wₖ₋₂ is still zero


def test_one_by_one():
    x, st = qr.qmr(np.array([[2.0]]), np.array([3.0]))
    assert st.niter == 1 and st.solved and x[0] == 1.5


def test_zero_right_hand_side():
    x, st = qr.qmr(np.eye(4) * 2.0, np.zeros(4))
    assert st.niter == 0 and st.solved and st.status == "x is a zero-residual solution" and not x.any()
    assert list(st.residuals) == [0.0]


def test_negative_c_gives_a_negative_gamma(oracle):
    """c = -b: β₁ = sqrt(|cᴴb|) > 0, γ₁ = cᴴb / β₁ < 0, and the iterates are those of c = b."""
    (x1, s1), _ = reference_pair(oracle, "kron8")
    (x2, s2), _ = reference_pair(oracle, "kron8_negc")
    assert s1.niter == s2.niter and s1.status == s2.status
    assert qr.history_deviation(s1.residuals, s2.residuals) <= 1e-8


def test_restatement_agrees_with_spsolve(oracle):
    S = oracle.kron_unsymmetric(8).to_scipy()
    b = rhs(S.shape[0])
    (x, st), _ = reference_pair(oracle, "kron8_rtol12")
    assert st.solved
    assert np.linalg.norm(x - spla.spsolve(sp.csc_matrix(S), b)) <= 1e-6 * np.linalg.norm(b)


@pytest.mark.parametrize("k", [1, 2, 3, 10, 40])
def test_symmetric_operator_gives_the_minres_iterates(oracle, k):
    """A symmetric and c = b: u₁ = v₁, the two Lanczos sequences coincide and are orthonormal, so the quasi-minimal residual is the
    minimal one and x_k is the iterate of minres!.  The tolerance is measured on the two restatements themselves: 10 x the sum of
    their own sensitivities to the rounding of the dots (np.dot against math.fsum), plus 16 eps for a sensitivity that measures
    zero; all relative to max|x_k|."""
    S = oracle.poisson3d(16).to_scipy()
    b = rhs(S.shape[0])
    xq, sq = qr.qmr(S, b, At=S, itmax=k)
    xqe, _ = qr.qmr(S, b, At=S, itmax=k, dot=qr.fsum_dot)
    xm, sm = mr.minres(S, b, itmax=k)
    xme, _ = mr.minres(S, b, itmax=k, dot=qr.fsum_dot)
    assert sq.niter == sm.niter == k
    scale = np.abs(xm).max()
    tol = 10.0 * (np.abs(xq - xqe).max() + np.abs(xm - xme).max()) / scale + 16 * qr.EPS
    dev = np.abs(xq - xm).max() / scale
    print(f"k = {k}: qmr against minres {dev:.2e}, tolerance {tol:.2e}")
    assert dev <= tol


def test_roles_after_one_two_and_three_iterations(oracle):
    """The names of the work vectors at the end of the loop: w_prev = wₖ, w_prev2 = wₖ₋₁ (zeros after one iteration), and
    x_k - x_k-1 = ζₖ wₖ is parallel to w_prev."""
    S = oracle.kron_unsymmetric(7).to_scipy()
    b = rhs(S.shape[0])
    prev = None
    for k in (1, 2, 3, 4):
        x, st = qr.qmr(S, b, itmax=k)
        w = st.vectors["w_prev"]
        if k == 1:
            assert not st.vectors["w_prev2"].any()
            step = x
        else:
            assert np.array_equal(st.vectors["w_prev2"], prev[1])
            step = x - prev[0]
        zeta = float(step @ w) / float(w @ w)
        assert np.linalg.norm(step - zeta * w) <= 1e-12 * np.linalg.norm(step)
        prev = (x, w)


def test_warm_start_and_preconditioners_of_the_restatement(oracle):
    S = oracle.kron_unsymmetric(8).to_scipy()
    n = S.shape[0]
    b = rhs(n)
    d = S.diagonal()
    jac = lambda v: v / d  # noqa: E731
    for kw in (dict(x0=np.linspace(-0.5, 0.5, n)), dict(M=jac), dict(N=jac), dict(M=jac, N=jac)):
        x, st = qr.qmr(S, b, **kw)
        assert st.solved and np.linalg.norm(b - S @ x) <= 1e-6 * np.linalg.norm(b), kw.keys()


def test_callback_of_the_restatement(oracle):
    S = oracle.kron_unsymmetric(7).to_scipy()
    seen = []
    x, st = qr.qmr(S, rhs(S.shape[0]), callback=lambda w: (seen.append(len(w.stats.residuals)), len(seen) == 3)[1])
    assert seen == [2, 3, 4] and st.niter == 3 and st.status == "user-requested exit"


# ---- the Python mirror's tables -----------------------------------------------------------------------------------------------------
def test_python_mirror_exports_qmr():
    """The mirror has the whole QMR surface (fails before the feature: K.qmr did not exist)."""
    import krylov_jl_amd as K
    for name in ("qmr", "qmr_", "QmrWorkspace"):
        assert hasattr(K, name), name
    for sym in ("khip_qmr_default_params", "khip_qmr_workspace_create", "khip_qmr_workspace_adopt",
                "khip_qmr_workspace_adopt_vector", "khip_qmr_workspace_destroy", "khip_qmr_warm_start", "khip_qmr_solve",
                "khip_qmr_solution", "khip_qmr_stats", "khip_qmr_last_path", "khip_qmr_vector", "khip_qmr_workspace_bytes"):
        assert sym in K.SIGNATURES, sym
        assert hasattr(K.lib(), sym), sym
    assert K._INPLACE[K.QmrWorkspace] == ("qmr", K.qmr_)
    assert "qmr" not in K.WORKSPACE_KWARGS
    assert K.QmrWorkspace.VECTORS == ("u_prev", "u", "q", "v_prev", "v", "p", "x", "w_prev2", "w_prev")
    assert len(K.SIGNATURES["khip_qmr_workspace_adopt"][1]) == 3 + 9 + 1
    prm = K.lib().khip_qmr_default_params()
    assert not prm.Mt and not prm.Nt


def test_preconditioner_adjoint_rule_names_the_solver():
    """Only the identity and Jacobi are their own adjoint; the refusal names the solver that was called."""
    import krylov_jl_amd as K
    f = lambda x, y: y  # noqa: E731
    assert K._bilq_precond_adjoint("M", None, None, solver="qmr") is None
    assert K._bilq_precond_adjoint("M", f, f, solver="qmr") is f
    assert K._bilq_precond_adjoint("N", object.__new__(K.Jacobi), None, solver="qmr") is None
    for op in (f, object.__new__(K.Ilu0)):
        with pytest.raises(K.KhipError, match=r"error -1: qmr: M = \w+ is not known to be its own adjoint"):
            K._bilq_precond_adjoint("M", op, None, solver="qmr")
        with pytest.raises(K.KhipError, match=r"error -1: bilq: M = \w+ is not known to be its own adjoint"):
            K._bilq_precond_adjoint("M", op, None)
    with pytest.raises(K.KhipError, match="error -1: qmr: a matrix-free A"):
        K._adjoint_of(f, solver="qmr")


def test_restatement_reports_beta1(oracle):
    """stats.beta1 = sqrt(|cᴴr₀|), which is not ‖r₀‖ when c differs from r₀ (the floor of the GPU tests' history bound)."""
    (_, s), _ = reference_pair(oracle, "kron8_sinc")
    n = 512
    assert s.beta1 == math.sqrt(abs(float(np.dot(other_c(n), rhs(n))))) and s.beta1 < 0.95 * s.residuals[0]
    (_, s), _ = reference_pair(oracle, "kron8")
    assert abs(s.beta1 - s.residuals[0]) <= 1e-12 * s.residuals[0]


@ref_tree
def test_forwarded_defaults_equal_the_reference():
    """FORWARDED_DEFAULTS["qmr"] = kwargs_qmr / def_kwargs_qmr of src/qmr.jl, names in order, defaults as values."""
    import krylov_jl_amd as K
    src = open(os.path.join(REFERENCE_SRC, "qmr.jl")).read()
    names = re.findall(r":(\w+)", re.search(r"^kwargs_qmr = \((.*?)\)", src, flags=re.M).group(1))
    table = re.search(r"^def_kwargs_qmr = \((.*?)\)\n\n", src, flags=re.M | re.S).group(1)
    defaults = {m.group(1): m.group(2) for m in
                re.finditer(r":\(;\s*(\w+)(?:::[^=]+?)?\s*=\s*(.*?)\s*\)\s*[,)]?\s*$", table, flags=re.M)}
    assert list(defaults) == names
    mine = K.FORWARDED_DEFAULTS["qmr"]
    assert list(mine) == names
    sq = math.sqrt(np.finfo(np.float64).eps)
    value = {"I": None, "b": None, "false": False, "true": True, "√eps(T)": sq, "0": 0, "Inf": math.inf, "kstdout": None}
    for k, expr in defaults.items():
        if k == "callback":
            assert expr == "workspace -> false" and mine[k] is K.default_callback
        else:
            assert mine[k] == value[expr] and type(mine[k]) is type(value[expr]), (k, expr, mine[k])


def _julia_qmr():
    glue = open(JULIA_SRC).read()
    m = re.search(r"function Krylov\.qmr!\(ws::QmrWs, A::HIPCsr, b::HIPVector;(.*?)\)\n(.*?)\nend\n", glue, flags=re.S)
    assert m, "no specialised Krylov.qmr!"
    return glue, m.group(1), m.group(2)


def test_julia_qmr_specialisation_shape():
    """The Julia qmr! (checked as text: Julia does not run here): the QmrWs alias, the nine adopted vectors in the order of
    khip_qmr_workspace_adopt, the fallback gate (ldiv, a foreign M or N, an IO without a descriptor), the default callback's
    recognition, LAST_PATH, A' taken once, and test/qmr.jl beside test/bilq.jl, reached from runtests.jl."""
    glue, sig, body = _julia_qmr()
    assert "const QmrWs = QmrWorkspace{Float64,Float64,HIPVector}" in glue
    adopt = re.search(r"ccall\(\(:khip_qmr_workspace_adopt, lib\), Cint, \((.*?)\),\n\s+CTX\[\]\.h, ws\.m, ws\.n, (.*?), r\)\)", glue,
                      flags=re.S)
    assert adopt, "qmr_handle does not adopt the workspace's vectors"
    assert adopt.group(1).count("Ptr{Cdouble}") == 9
    assert [a.strip() for a in adopt.group(2).split(",")] == [f"ws.{f}.ptr" for f in
                                                              ("uₖ₋₁", "uₖ", "q", "vₖ₋₁", "vₖ", "p", "x", "wₖ₋₂", "wₖ₋₁")]
    assert 'for (name, v) in (("t", ws.t), ("s", ws.s), ("dx", ws.Δx))\n    qmr_adopt(h, name, v)' in body
    assert "if ldiv || !self_adjoint_precond(M) || !self_adjoint_precond(N) || !native_log(verbose, iostream)" in body
    assert "invoke(Krylov.qmr!, Tuple{QmrWs,Any,AbstractVector{Float64}}, ws, A, b;" in body
    assert "callback = callback === nothing ? (w -> false) : callback" in body
    assert "P.kind !== :jacobi) &&\n      error(\"qmr!:" in body
    assert "callback_args(user_callback(callback), ws, sp, history)" in body
    assert "NATIVE_SOLVES[] += 1" in body and "LAST_PATH[] = ccall((:khip_qmr_last_path, lib)" in body
    assert "khip_qmr_warm_start" in body and "ws.warm_start = false" in body
    assert len(re.findall(r"(?<![\w])A'", body)) == 1, "A' is taken once per solve (and cached on the matrix by Base.adjoint)"
    assert "callback = nothing" in sig and "fused::Int = 2" in sig
    # struct QmrParams mirrors khip_qmr_params: two operator pointers
    assert re.search(r"struct QmrParams[^\n]*\n\s+Mt::Ptr\{Operator\}; Nt::Ptr\{Operator\}\nend", glue)
    header = open(os.path.join(ROOT, "include", "krylov_hip.h")).read()
    assert re.search(r"typedef struct \{\s*const khip_operator \*Mt, \*Nt;[^}]*\} khip_qmr_params;", header)
    tests = os.path.join(ROOT, "julia", "KrylovHIP", "test")
    assert os.path.isfile(os.path.join(tests, "qmr.jl"))
    qmr_jl = open(os.path.join(tests, "qmr.jl")).read()
    for piece in ("QmrWorkspace(n, n, S)", "native(2) do; qmr!(ws, A_gpu, b; history = true); end", "generic(qmr!, ws2, A_gpu, b;",
                  "unsymmetric_breakdown()", "bc_breakdown()", "QMR: system of size $n"):
        assert piece in qmr_jl, piece
    assert "qmr(U_gpu, S(bu_cpu))" in open(os.path.join(tests, "runtests.jl")).read()


@ref_tree
def test_julia_qmr_specialisation():
    """Against the reference tree: every keyword of kwargs_qmr is in the signature, and the body reads only fields of QmrWorkspace
    (src/krylov_workspaces.jl)."""
    glue, sig, body = _julia_qmr()
    src = open(os.path.join(REFERENCE_SRC, "qmr.jl")).read()
    names = re.findall(r":(\w+)", re.search(r"^kwargs_qmr = \((.*?)\)", src, flags=re.M).group(1))
    for kw in names:
        assert re.search(r"(?<![\w])" + kw + r"(?![\w])", sig), f"qmr!: keyword {kw} of the reference is missing"
    ws_src = open(os.path.join(REFERENCE_SRC, "krylov_workspaces.jl")).read()
    struct = re.search(r"mutable struct QmrWorkspace\{T,FC,S\}.*?\nend", ws_src, flags=re.S).group(0)
    fields = set(re.findall(r"^\s+(\S+)\s+::", struct, flags=re.M))
    used = set(re.findall(r"\bws\.([^\s.,;()\[\]]+)", body))
    handle = re.search(r"function qmr_handle\(ws::QmrWs\)\n(.*?)\nend\n", glue, flags=re.S).group(1)
    used |= set(re.findall(r"\bws\.([^\s.,;()\[\]]+)", handle))
    assert used <= fields, used - fields
    assert {"uₖ₋₁", "uₖ", "q", "vₖ₋₁", "vₖ", "p", "x", "wₖ₋₂", "wₖ₋₁", "Δx", "t", "s"} <= used
