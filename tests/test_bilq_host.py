"""bilq! without a GPU: the NumPy restatement (tests/bilq_reference.py) against the reference's own known answers and against
SciPy, the condition that admits a case to the GPU tests' case list, the Python mirror's tables against src/bilq.jl, and the Julia
specialisation's shape."""
import math
import os
import re
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bilq_reference as br  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_SRC = "/root/reference/src"
JULIA_SRC = os.path.join(ROOT, "julia", "KrylovHIP", "src", "KrylovHIP.jl")
ref_tree = pytest.mark.skipif(not os.path.isdir(REFERENCE_SRC), reason="the reference tree is only present in the build container")

XC = "solution xᶜ good enough given atol and rtol"
XL = "solution xᴸ good enough given atol and rtol"


# ---- the GPU tests' case list (tests/test_gpu_bilq.py imports it) ---------------------------------------------------------------
def rhs(n):
    return np.cos(0.37 * np.arange(n)) + 0.5


def other_c(n):
    return np.sin(0.11 * np.arange(n)) + 1.2


# name -> (operator, size parameter, c: None | "neg" | "sin", keywords of bilq)
CASES = {
    "kron7": ("kron", 7, None, {}),
    "kron7_lq": ("kron", 7, None, dict(transfer_to_bicg=False)),
    "kron8": ("kron", 8, None, {}),
    "kron8_lq": ("kron", 8, None, dict(transfer_to_bicg=False)),
    "kron8_negc": ("kron", 8, "neg", {}),
    "kron8_sinc": ("kron", 8, "sin", {}),
    "kron12": ("kron", 12, None, {}),
    "poisson16": ("poisson", 16, None, {}),
    "poisson16_sinc": ("poisson", 16, "sin", {}),
    "kron8_rtol12": ("kron", 8, None, dict(atol=0.0, rtol=1e-12)),
}
EXPECTED_NITER = {"kron7": 33, "kron7_lq": 38, "kron8": 39, "kron8_lq": 41, "kron8_negc": 39, "kron8_sinc": 41, "kron12": 53,
                  "poisson16": 63, "poisson16_sinc": 65, "kron8_rtol12": 50}


def case_operator(oracle, kind, n1):
    return oracle.kron_unsymmetric(n1) if kind == "kron" else oracle.poisson3d(n1)


def case_vectors(n, cname):
    b = rhs(n)
    c = None if cname is None else (-b if cname == "neg" else other_c(n))
    return b, c


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
        _PAIRS[key] = (br.bilq(S, b, c=c, At=St, **kw), br.bilq(S, b, c=c, At=St, dot=br.fsum_dot, **kw))
    return _PAIRS[key]


@pytest.mark.parametrize("name", list(CASES))
def test_case_list_condition(oracle, name):
    """A case may be in the list only if the restatement with np.dot and with math.fsum dots agree on niter and status and their
    whole residual histories agree to <= 1e-6 relative."""
    (_, s1), (_, s2) = reference_pair(oracle, name)
    assert s1.niter == s2.niter == EXPECTED_NITER[name], (s1.niter, s2.niter)
    assert s1.status == s2.status and s1.solved
    assert len(s1.residuals) == s1.niter + 1
    assert br.history_deviation(s1.residuals, s2.residuals) <= 1e-6


# ---- the reference's known answers, restated as data ------------------------------------------------------------------------------
def test_unsymmetric_breakdown():
    """test/test_utils.jl:196-201 with test/test_bilq.jl: x = [0, 1] after two iterations, at the BiCG point."""
    A = np.array([[0.0, 1.0], [-1.0, 0.0]])
    x, st = br.bilq(A, np.array([1.0, 0.0]), c=np.array([-1.0, 0.0]))
    assert st.niter == 2 and st.status == XC and st.solved
    assert np.allclose(x, [0.0, 1.0], rtol=0, atol=1e-15)


def test_bc_breakdown():
    """test/test_utils.jl:204-209: cᴴb = 0 ends before the first iteration."""
    A = np.array([[1.0, 2.0], [3.0, 4.0]])
    x, st = br.bilq(A, np.array([0.0, 1.0]), c=np.array([1.0, 0.0]))
    assert st.niter == 0 and st.status == "Breakdown bᴴc = 0" and not st.solved and not x.any()


def test_identity():
    """A = I: the Krylov space ends after one step (pᴴq = 0); the BiCG point is b, without the transfer it is a breakdown."""
    b = np.arange(1.0, 6.0)
    x, st = br.bilq(np.eye(5), b)
    assert st.niter == 1 and st.status == XC and np.array_equal(x, b)
    x, st = br.bilq(np.eye(5), b, transfer_to_bicg=False)
    assert st.niter == 1 and st.status == "Breakdown ⟨uₖ₊₁,vₖ₊₁⟩ = 0" and not st.solved


def test_one_by_one():
    x, st = br.bilq(np.array([[2.0]]), np.array([3.0]))
    assert st.niter == 1 and st.solved and x[0] == 1.5


def test_zero_right_hand_side():
    x, st = br.bilq(np.eye(4) * 2.0, np.zeros(4))
    assert st.niter == 0 and st.solved and st.status == "x is a zero-residual solution" and not x.any()
    assert list(st.residuals) == [0.0]


def test_negative_c_gives_a_negative_gamma(oracle):
    """c = -b: β₁ = sqrt(|cᴴb|) > 0, γ₁ = cᴴb / β₁ < 0, and the iterates are those of c = b."""
    (x1, s1), _ = reference_pair(oracle, "kron8")
    (x2, s2), _ = reference_pair(oracle, "kron8_negc")
    assert s1.niter == s2.niter and s1.status == s2.status
    assert br.history_deviation(s1.residuals, s2.residuals) <= 1e-8


def test_restatement_agrees_with_spsolve(oracle):
    S = oracle.kron_unsymmetric(8).to_scipy()
    b = rhs(S.shape[0])
    (x, st), _ = reference_pair(oracle, "kron8_rtol12")
    assert st.solved
    assert np.linalg.norm(x - spla.spsolve(sp.csc_matrix(S), b)) <= 1e-6 * np.linalg.norm(b)


def test_warm_start_and_preconditioners_of_the_restatement(oracle):
    S = oracle.kron_unsymmetric(8).to_scipy()
    n = S.shape[0]
    b = rhs(n)
    d = S.diagonal()
    jac = lambda v: v / d  # noqa: E731
    for kw in (dict(x0=np.linspace(-0.5, 0.5, n)), dict(M=jac), dict(N=jac), dict(M=jac, N=jac)):
        x, st = br.bilq(S, b, **kw)
        assert st.solved and np.linalg.norm(b - S @ x) <= 1e-6 * np.linalg.norm(b), kw.keys()


# ---- the Python mirror's tables -----------------------------------------------------------------------------------------------------
def test_python_mirror_exports_bilq():
    """The mirror has the whole BiLQ surface (fails before the feature: K.bilq did not exist)."""
    import krylov_jl_amd as K
    for name in ("bilq", "bilq_", "BilqWorkspace"):
        assert hasattr(K, name), name
    for sym in ("khip_bilq_default_params", "khip_bilq_workspace_create", "khip_bilq_workspace_adopt",
                "khip_bilq_workspace_adopt_vector", "khip_bilq_workspace_destroy", "khip_bilq_warm_start", "khip_bilq_solve",
                "khip_bilq_solution", "khip_bilq_stats", "khip_bilq_last_path", "khip_bilq_vector", "khip_bilq_workspace_bytes"):
        assert sym in K.SIGNATURES, sym
        assert hasattr(K.lib(), sym), sym
    assert K._INPLACE[K.BilqWorkspace] == ("bilq", K.bilq_)
    assert "bilq" not in K.WORKSPACE_KWARGS
    prm = K.lib().khip_bilq_default_params()
    assert prm.transfer_to_bicg == 1 and not prm.Mt and not prm.Nt


def test_preconditioner_adjoint_rule():
    """Only the identity and Jacobi are their own adjoint; anything else needs Mt / Nt or is refused."""
    import krylov_jl_amd as K
    f = lambda x, y: y  # noqa: E731
    assert K._bilq_precond_adjoint("M", None, None) is None
    assert K._bilq_precond_adjoint("M", f, f) is f
    jac = object.__new__(K.Jacobi)
    assert K._bilq_precond_adjoint("N", jac, None) is None
    for op in (f, object.__new__(K.Ilu0)):
        with pytest.raises(K.KhipError, match="own adjoint"):
            K._bilq_precond_adjoint("M", op, None)


def test_restatement_reports_beta1(oracle):
    """stats.beta1 = sqrt(|cᴴr₀|), which is not ‖r₀‖ when c differs from r₀ (the floor of the GPU tests' history bound)."""
    (_, s), _ = reference_pair(oracle, "kron8_sinc")
    n = 512
    assert s.beta1 == math.sqrt(abs(float(np.dot(other_c(n), rhs(n))))) and s.beta1 < 0.95 * s.residuals[0]
    (_, s), _ = reference_pair(oracle, "kron8")
    assert abs(s.beta1 - s.residuals[0]) <= 1e-12 * s.residuals[0]


def test_sym_givens_is_one_source():
    """khip_test_sym_givens (host) runs the function the device epilogues run; it agrees with the restatement's to the bit on the
    branches bilq! reaches."""
    import ctypes as C

    import krylov_jl_amd as K
    for a, b in ((3.0, 4.0), (4.0, -3.0), (0.0, 2.0), (-1.5, 0.0), (0.0, 0.0), (1e-300, 1e300), (-0.3, 0.7)):
        c, s, rho = C.c_double(), C.c_double(), C.c_double()
        assert K.lib().khip_test_sym_givens(a, b, C.byref(c), C.byref(s), C.byref(rho)) == 0
        assert (c.value, s.value, rho.value) == br.sym_givens(a, b), (a, b)


@ref_tree
def test_forwarded_defaults_equal_the_reference():
    """FORWARDED_DEFAULTS["bilq"] = kwargs_bilq / def_kwargs_bilq of src/bilq.jl, names in order, defaults as values."""
    import krylov_jl_amd as K
    src = open(os.path.join(REFERENCE_SRC, "bilq.jl")).read()
    names = re.findall(r":(\w+)", re.search(r"^kwargs_bilq = \((.*?)\)", src, flags=re.M).group(1))
    table = re.search(r"^def_kwargs_bilq = \((.*?)\)\n\n", src, flags=re.M | re.S).group(1)
    defaults = {m.group(1): m.group(2) for m in
                re.finditer(r":\(;\s*(\w+)(?:::[^=]+?)?\s*=\s*(.*?)\s*\)\s*[,)]?\s*$", table, flags=re.M)}
    assert list(defaults) == names
    mine = K.FORWARDED_DEFAULTS["bilq"]
    assert list(mine) == names
    sq = math.sqrt(np.finfo(np.float64).eps)
    value = {"I": None, "b": None, "false": False, "true": True, "√eps(T)": sq, "0": 0, "Inf": math.inf, "kstdout": None}
    for k, expr in defaults.items():
        if k == "callback":
            assert expr == "workspace -> false" and mine[k] is K.default_callback
        else:
            assert mine[k] == value[expr] and type(mine[k]) is type(value[expr]), (k, expr, mine[k])


@ref_tree
def test_julia_bilq_specialisation():
    """The Julia bilq! has every reference keyword, an invoke fallback, the BilqWs alias, takes A' once, and reads only fields of
    BilqWorkspace (src/krylov_workspaces.jl)."""
    glue = open(JULIA_SRC).read()
    assert "const BilqWs = BilqWorkspace{Float64,Float64,HIPVector}" in glue
    m = re.search(r"function Krylov\.bilq!\(ws::BilqWs, A::HIPCsr, b::HIPVector;(.*?)\)\n(.*?)\nend\n", glue, flags=re.S)
    assert m, "no specialised Krylov.bilq!"
    sig, body = m.group(1), m.group(2)
    src = open(os.path.join(REFERENCE_SRC, "bilq.jl")).read()
    names = re.findall(r":(\w+)", re.search(r"^kwargs_bilq = \((.*?)\)", src, flags=re.M).group(1))
    for kw in names:
        assert re.search(r"(?<![\w])" + kw + r"(?![\w])", sig), f"bilq!: keyword {kw} of the reference is missing"
    assert "invoke(Krylov.bilq!, Tuple{BilqWs,Any,AbstractVector{Float64}}, ws, A, b;" in body
    assert "callback_args(user_callback(callback), ws, sp, history)" in body
    assert "NATIVE_SOLVES[] += 1" in body and "khip_bilq_last_path" in body
    # only I and Jacobi are their own adjoint: ILU(0) is refused, anything foreign takes the generic method (which calls M')
    assert "self_adjoint_precond(M) = M === I || (M isa HIPOperator && M.kind === :jacobi)" in glue
    assert "!self_adjoint_precond(M) || !self_adjoint_precond(N)" in body and "P.kind !== :jacobi) &&\n      error(" in body
    assert len(re.findall(r"(?<![\w])A'", body)) == 1, "A' is taken once per solve (and cached on the matrix by Base.adjoint)"
    ws_src = open(os.path.join(REFERENCE_SRC, "krylov_workspaces.jl")).read()
    struct = re.search(r"mutable struct BilqWorkspace\{T,FC,S\}.*?\nend", ws_src, flags=re.S).group(0)
    fields = set(re.findall(r"^\s+(\S+)\s+::", struct, flags=re.M))
    used = set(re.findall(r"\bws\.([^\s.,;()\[\]]+)", body))
    assert used <= fields, used - fields
    assert os.path.isfile(os.path.join(ROOT, "julia", "KrylovHIP", "test", "bilq.jl"))
