"""cgs! without a GPU: the NumPy restatement (tests/cgs_reference.py) against known answers, the condition that admits a case
to the GPU tests' history-parity list, the Python mirror's tables and the header against src/cgs.jl, and the Julia specialisation's
shape (as text: Julia does not run here)."""
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cgs_reference as cr  # noqa: E402
from test_bilq_host import case_operator, case_vectors, rhs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_SRC = "/root/reference/src"
JULIA_SRC = os.path.join(ROOT, "julia", "KrylovHIP", "src", "KrylovHIP.jl")
ref_tree = pytest.mark.skipif(not os.path.isdir(REFERENCE_SRC), reason="the reference tree is only present in the build container")

SOLVED = cr.SOLVED

# ---- the GPU tests' case list (tests/test_gpu_cgs.py imports it) ----------------------------------------------------------------
# name -> (operator, size parameter, c: None | "neg" | "sin", keywords of cgs)
CASES = {
    "kron7": ("kron", 7, None, {}),                                   # n = 343
    "kron8": ("kron", 8, None, {}),                                   # n = 512
    "kron8_negc": ("kron", 8, "neg", {}),
    "poisson8": ("poisson", 8, None, {}),                             # n = 512
    "kron8_rtol12": ("kron", 8, None, dict(atol=0.0, rtol=1e-12)),
    "kron12": ("kron", 12, None, {}),                                 # n = 1728
    "kron8_sinc": ("kron", 8, "sin", {}),
    "poisson16": ("poisson", 16, None, {}),                           # n = 4096
}
# recorded from the restatement (np.dot and math.fsum dots agree on every one)
EXPECTED_NITER = {"kron7": 22, "kron8": 24, "kron8_negc": 24, "poisson8": 21, "kron8_rtol12": 31, "kron12": 33, "kron8_sinc": 26,
                  "poisson16": 63}
# CGS squares the residual polynomial: the history of the other cases moves by 6.6e-5 ... 1.2e-2 with the rounding of the dots
# alone, so only these enter the comparisons that need a history budget; the others serve path 1 = path 2, the true residual, niter
PARITY_CAP = 1e-6
PARITY_CASES = ("kron7", "kron8", "kron8_negc", "poisson8")

_PAIRS = {}


def reference_pair(oracle, name, **extra):
    """(restatement with np.dot, restatement with exactly summed dots) of a case, as (x, stats) pairs; computed once."""
    key = (name, tuple(sorted((k, id(v) if callable(v) else repr(v)) for k, v in extra.items())))
    if key not in _PAIRS:
        kind, n1, cname, kw = CASES[name]
        A_cpu = case_operator(oracle, kind, n1)
        S = A_cpu.to_scipy()
        b, c = case_vectors(A_cpu.n, cname)
        kw = dict(kw, **extra)
        _PAIRS[key] = (cr.cgs(S, b, c=c, **kw), cr.cgs(S, b, c=c, dot=cr.fsum_dot, **kw))
    return _PAIRS[key]


@pytest.mark.parametrize("name", list(CASES))
def test_case_list(oracle, name):
    """Every case converges in the recorded number of iterations whichever way the dots are rounded, and to a true residual of
    1e-6 ‖b‖ (the reference's own test bound)."""
    (x1, s1), (x2, s2) = reference_pair(oracle, name)
    assert s1.niter == s2.niter == EXPECTED_NITER[name], (s1.niter, s2.niter)
    assert s1.status == s2.status == SOLVED and s1.solved
    assert len(s1.residuals) == s1.niter + 1
    kind, n1, cname, kw = CASES[name]
    S = case_operator(oracle, kind, n1).to_scipy()
    b = rhs(S.shape[0])
    assert np.linalg.norm(b - S @ x1) <= 1e-6 * np.linalg.norm(b)
    dev = cr.history_deviation(s1.residuals, s2.residuals)
    print(f"{name}: np.dot against fsum, largest relative history deviation {dev:.3e}")
    # niter is robust: no residual is within 10 x that deviation of ε, so the GPU tests may ask for the same count on every case
    eps = kw.get("atol", math.sqrt(cr.EPS)) + kw.get("rtol", math.sqrt(cr.EPS)) * s1.residuals[0]
    assert np.all(s1.residuals[:-1] > (1 + 10 * dev) * eps) and s1.residuals[-1] < (1 - 10 * dev) * eps


def test_parity_list_condition(oracle):
    """Only cases whose own np.dot-against-fsum history deviation is <= 1e-6 are in the history-parity list; the list is not
    empty, and no case that qualifies was left out."""
    assert len(PARITY_CASES) > 0 and set(PARITY_CASES) <= set(CASES)
    for name in CASES:
        (_, s1), (_, s2) = reference_pair(oracle, name)
        dev = cr.history_deviation(s1.residuals, s2.residuals)
        assert (dev <= PARITY_CAP) == (name in PARITY_CASES), (name, dev)


# ---- known answers ---------------------------------------------------------------------------------------------------------------
def test_zero_right_hand_side():
    x, st = cr.cgs(np.eye(4) * 2.0, np.zeros(4))
    assert st.niter == 0 and st.solved and st.status == "x is a zero-residual solution" and not x.any()
    assert list(st.residuals) == [0.0]


def test_bc_breakdown():
    """c ⟂ b ends before the first iteration (test/test_utils.jl:204-209)."""
    A = np.array([[1.0, 2.0], [3.0, 4.0]])
    x, st = cr.cgs(A, np.array([0.0, 1.0]), c=np.array([1.0, 0.0]))
    assert st.niter == 0 and st.status == "Breakdown bᴴc = 0" and not st.solved and not x.any()


def test_itmax_exhaustion(oracle):
    S = oracle.kron_unsymmetric(7).to_scipy()
    x, st = cr.cgs(S, rhs(S.shape[0]), itmax=3)
    assert st.niter == 3 and not st.solved and st.status == cr.TIRED and len(st.residuals) == 4


def test_callback_of_the_restatement(oracle):
    S = oracle.kron_unsymmetric(7).to_scipy()
    seen = []
    x, st = cr.cgs(S, rhs(S.shape[0]), callback=lambda w: (seen.append(len(w.stats.residuals)), len(seen) == 3)[1])
    assert seen == [2, 3, 4] and st.niter == 3 and st.status == "user-requested exit"


def test_alpha_breakdown():
    """A = [[1, 0], [1, 2]], b = c = e₁: ρ₁ = 0 exactly after one iteration, then σ₂ = 0 and α₂ = 0 / 0 is NaN.  The loop ends
    with "breakdown αₖ == 0" after two iterations, the history is [1, 1, NaN] and x is NaN."""
    A = np.array([[1.0, 0.0], [1.0, 2.0]])
    e1 = np.array([1.0, 0.0])
    _, s1 = cr.cgs(A, e1, itmax=1)
    assert float(np.dot(e1, s1.vectors["r"])) == 0.0 and list(s1.residuals) == [1.0, 1.0]
    assert float(np.dot(e1, A @ s1.vectors["p"])) == 0.0                    # σ₂
    x, st = cr.cgs(A, e1)
    assert st.niter == 2 and not st.solved and st.status == "breakdown αₖ == 0"
    assert list(st.residuals[:2]) == [1.0, 1.0] and math.isnan(st.residuals[2]) and len(st.residuals) == 3
    assert np.isnan(x).all()


def test_one_by_one():
    x, st = cr.cgs(np.array([[2.0]]), np.array([3.0]))
    assert st.niter == 1 and st.solved and x[0] == 1.5


def test_negative_c_changes_nothing(oracle):
    """c = -b: ρ and σ change sign together; α, β and every iterate are those of c = b."""
    (x1, s1), _ = reference_pair(oracle, "kron8")
    (x2, s2), _ = reference_pair(oracle, "kron8_negc")
    assert s1.niter == s2.niter and np.array_equal(s1.residuals, s2.residuals) and np.array_equal(x1, x2)


def test_warm_start_and_preconditioners_of_the_restatement(oracle):
    S = oracle.kron_unsymmetric(8).to_scipy()
    n = S.shape[0]
    b = rhs(n)
    d = S.diagonal()
    jac = lambda v: v / d  # noqa: E731
    for kw in (dict(x0=np.linspace(-0.5, 0.5, n)), dict(M=jac), dict(N=jac), dict(M=jac, N=jac)):
        x, st = cr.cgs(S, b, **kw)
        assert st.solved and np.linalg.norm(b - S @ x) <= 1e-6 * np.linalg.norm(b), kw.keys()


# ---- the Python mirror's tables and the header -----------------------------------------------------------------------------------
CGS_SYMBOLS = ("khip_cgs_workspace_create", "khip_cgs_workspace_adopt", "khip_cgs_workspace_adopt_vector", "khip_cgs_workspace_destroy",
               "khip_cgs_warm_start", "khip_cgs_solve", "khip_cgs_solution", "khip_cgs_stats", "khip_cgs_last_path", "khip_cgs_vector",
               "khip_cgs_workspace_bytes")


def test_python_mirror_exports_cgs():
    """The mirror has the whole CGS surface (fails before the feature: K.cgs did not exist)."""
    import krylov_jl_amd as K
    for name in ("cgs", "cgs_", "CgsWorkspace"):
        assert hasattr(K, name), name
    for sym in CGS_SYMBOLS:
        assert sym in K.SIGNATURES, sym
        assert hasattr(K.lib(), sym), sym
    assert K._INPLACE[K.CgsWorkspace] == ("cgs", K.cgs_)
    assert "cgs" not in K.WORKSPACE_KWARGS
    assert K.CgsWorkspace.VECTORS == ("x", "r", "u", "p", "q", "ts")
    assert len(K.SIGNATURES["khip_cgs_workspace_adopt"][1]) == 3 + 6 + 1
    assert len(K.SIGNATURES["khip_cgs_solve"][1]) == len(K.SIGNATURES["khip_bicgstab_solve"][1]) == 7


def test_header_declares_the_cgs_entries():
    """include/krylov_hip.h: every entry once, adopt with the six core vectors in the order x, r, u, p, q, ts, solve with the
    arguments of khip_bicgstab_solve; the ABI version is untouched by this header section."""
    header = open(os.path.join(ROOT, "include", "krylov_hip.h"), encoding="utf-8").read()
    for sym in CGS_SYMBOLS:
        assert len(re.findall(r"^[\w ]+\*?" + sym + r"\(", header, flags=re.M)) == 1, sym
    adopt = re.search(r"int khip_cgs_workspace_adopt\(khip_ctx \*ctx, int64_t m, int64_t n, (.*?),\s*khip_cgs_workspace \*\*out\);", header,
                      flags=re.S)
    assert adopt and re.findall(r"double \*(\w+)", adopt.group(1)) == ["x", "r", "u", "p", "q", "ts"]
    solve = re.search(r"int khip_cgs_solve\((.*?)\);", header, flags=re.S).group(1)
    assert re.findall(r"\*(\w+)(?:,|$)", solve) == ["ws", "A", "M", "N", "b", "c", "opts"]
    assert '"x", "r", "u", "p", "q", "ts", "dx", "yz", "vw"' in header


@ref_tree
def test_forwarded_defaults_equal_the_reference():
    """FORWARDED_DEFAULTS["cgs"] = kwargs_cgs / def_kwargs_cgs of src/cgs.jl, names in order, defaults as values."""
    import krylov_jl_amd as K
    src = open(os.path.join(REFERENCE_SRC, "cgs.jl")).read()
    names = re.findall(r":(\w+)", re.search(r"^kwargs_cgs = \((.*?)\)", src, flags=re.M).group(1))
    table = re.search(r"^def_kwargs_cgs = \((.*?)\)\n\n", src, flags=re.M | re.S).group(1)
    defaults = {m.group(1): m.group(2) for m in
                re.finditer(r":\(;\s*(\w+)(?:::[^=]+?)?\s*=\s*(.*?)\s*\)\s*[,)]?\s*$", table, flags=re.M)}
    assert list(defaults) == names
    mine = K.FORWARDED_DEFAULTS["cgs"]
    assert list(mine) == names
    assert mine == K.FORWARDED_DEFAULTS["bicgstab"]                     # "the keywords of the reference and the stats of bicgstab"
    sq = math.sqrt(np.finfo(np.float64).eps)
    value = {"I": None, "b": None, "false": False, "true": True, "√eps(T)": sq, "0": 0, "Inf": math.inf, "kstdout": None}
    for k, expr in defaults.items():
        if k == "callback":
            assert expr == "workspace -> false" and mine[k] is K.default_callback
        else:
            assert mine[k] == value[expr] and type(mine[k]) is type(value[expr]), (k, expr, mine[k])


# ---- the Julia glue, as text -----------------------------------------------------------------------------------------------------
def _julia_cgs():
    glue = open(JULIA_SRC, encoding="utf-8").read()
    m = re.search(r"function Krylov\.cgs!\(ws::CgsWs, A::HIPCsr, b::HIPVector;(.*?)\)\n(.*?)\nend\n", glue, flags=re.S)
    assert m, "no specialised Krylov.cgs!"
    return glue, m.group(1), m.group(2)


def test_julia_cgs_specialisation_shape():
    """The Julia cgs!: the CgsWs alias, the six adopted vectors in the order of khip_cgs_workspace_adopt, the lazy vectors handed
    over by name, the fallback gate (ldiv, a foreign M or N, an IO without a descriptor), the forwarded default callback,
    LAST_PATH, no adjoint anywhere, and test/cgs.jl reached from runtests.jl."""
    glue, sig, body = _julia_cgs()
    assert "const CgsWs = CgsWorkspace{Float64,Float64,HIPVector}" in glue
    adopt = re.search(r"ccall\(\(:khip_cgs_workspace_adopt, lib\), Cint,\s*\((.*?)\),\n\s+CTX\[\]\.h, ws\.m, ws\.n, (.*?), r\)\)", glue,
                      flags=re.S)
    assert adopt, "cgs_handle does not adopt the workspace's vectors"
    assert adopt.group(1).count("Ptr{Cdouble}") == 6
    assert [a.strip() for a in adopt.group(2).split(",")] == [f"ws.{f}.ptr" for f in ("x", "r", "u", "p", "q", "ts")]
    assert 'for (name, v) in (("vw", ws.vw), ("yz", ws.yz), ("dx", ws.Δx))\n    cgs_adopt(h, name, v)' in body
    assert "if ldiv || !native_precond(M) || !native_precond(N) || !native_log(verbose, iostream)" in body
    assert "invoke(Krylov.cgs!, Tuple{CgsWs,Any,AbstractVector{Float64}}, ws, A, b;" in body
    assert "callback = callback === nothing ? (w -> false) : callback" in body
    assert "callback_args(user_callback(callback), ws, sp, history)" in body
    assert "NATIVE_SOLVES[] += 1" in body and "LAST_PATH[] = ccall((:khip_cgs_last_path, lib)" in body
    assert "khip_cgs_warm_start" in body and "ws.warm_start = false" in body
    assert not re.search(r"(?<![\w])A'", body), "cgs! is transpose-free"
    assert "callback = nothing" in sig and "fused::Int = 2" in sig
    # the ccall of the solve has the argument types of khip_cgs_solve: ws, A, M, N, b, c, opts
    assert ("ccall((:khip_cgs_solve, lib), Cint,\n" in body and
            "(Ptr{Cvoid}, Ref{Operator}, Ptr{Operator}, Ptr{Operator}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Options})" in body)
    tests = os.path.join(ROOT, "julia", "KrylovHIP", "test")
    cgs_jl = open(os.path.join(tests, "cgs.jl"), encoding="utf-8").read()
    for piece in ("CgsWorkspace(n, n, S)", "native(2) do; cgs!(ws, A_gpu, b; history = true); end", "generic_cgs(ws2, A_gpu, b;",
                  "bc_breakdown()", "CGS: system of size $n", "breakdown αₖ == 0"):
        assert piece in cgs_jl, piece
    runtests = open(os.path.join(tests, "runtests.jl"), encoding="utf-8").read()
    assert 'include("cgs.jl")' in runtests and "cgs(U_gpu, S(bu_cpu))" in runtests


@ref_tree
def test_julia_cgs_specialisation():
    """Against the reference tree: every keyword of kwargs_cgs is in the signature, and the glue reads only fields of CgsWorkspace
    (src/krylov_workspaces.jl), all nine vectors among them."""
    glue, sig, body = _julia_cgs()
    src = open(os.path.join(REFERENCE_SRC, "cgs.jl")).read()
    names = re.findall(r":(\w+)", re.search(r"^kwargs_cgs = \((.*?)\)", src, flags=re.M).group(1))
    for kw in names:
        assert re.search(r"(?<![\w])" + kw + r"(?![\w])", sig), f"cgs!: keyword {kw} of the reference is missing"
    ws_src = open(os.path.join(REFERENCE_SRC, "krylov_workspaces.jl")).read()
    struct = re.search(r"mutable struct CgsWorkspace\{T,FC,S\}.*?\nend", ws_src, flags=re.S).group(0)
    fields = set(re.findall(r"^\s+(\S+)\s+::", struct, flags=re.M))
    used = set(re.findall(r"\bws\.([^\s.,;()\[\]]+)", body))
    handle = re.search(r"function cgs_handle\(ws::CgsWs\)\n(.*?)\nend\n", glue, flags=re.S).group(1)
    used |= set(re.findall(r"\bws\.([^\s.,;()\[\]]+)", handle))
    assert used <= fields, used - fields
    assert {"x", "r", "u", "p", "q", "ts", "Δx", "yz", "vw"} <= used
