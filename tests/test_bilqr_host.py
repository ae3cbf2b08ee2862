"""bilqr! without a GPU: the NumPy restatement (tests/bilqr_reference.py) against the reference's own known answers, against a
sparse direct solve of both systems and against the restatements of bilq! and qmr! it combines; the condition that admits a case to
the GPU tests' case list; the Python mirror's tables against src/bilqr.jl; and the Julia specialisation's shape."""
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
import bilqr_reference as qq  # noqa: E402
import qmr_reference as qr  # noqa: E402
from test_bilq_host import case_operator, other_c, rhs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_SRC = "/root/reference/src"
JULIA_SRC = os.path.join(ROOT, "julia", "KrylovHIP", "src", "KrylovHIP.jl")
ref_tree = pytest.mark.skipif(not os.path.isdir(REFERENCE_SRC), reason="the reference tree is only present in the build container")

VECTORS = ("u_prev", "u", "q", "v_prev", "v", "p", "x", "y", "dbar", "w_prev3", "w_prev2")

# ---- the GPU tests' case list (tests/test_gpu_bilqr.py imports it) --------------------------------------------------------------
# name -> (operator, size parameter, c: "b" | "neg" | "sin", keywords of bilqr)
CASES = {
    "kron7_sinc": ("kron", 7, "sin", {}),
    "kron7_bb": ("kron", 7, "b", {}),
    "kron7_sinc_lq": ("kron", 7, "sin", dict(transfer_to_bicg=False)),
    "kron8_sinc": ("kron", 8, "sin", {}),
    "kron8_bb": ("kron", 8, "b", {}),
    "kron8_negc": ("kron", 8, "neg", {}),
    "kron12_bb": ("kron", 12, "b", {}),
    "poisson16_sinc": ("poisson", 16, "sin", {}),
    "poisson16_bb": ("poisson", 16, "b", {}),
    "poisson16_sinc_lq": ("poisson", 16, "sin", dict(transfer_to_bicg=False)),
}
# name -> (niter, entries of the primal history, entries of the dual history), from the restatement
EXPECTED = {"kron7_sinc": (39, 36, 40), "kron7_bb": (36, 34, 37), "kron7_sinc_lq": (39, 40, 40), "kron8_sinc": (41, 42, 40),
            "kron8_bb": (40, 40, 41), "kron8_negc": (40, 40, 41), "kron12_bb": (57, 54, 58), "poisson16_sinc": (73, 66, 74),
            "poisson16_bb": (67, 64, 68), "poisson16_sinc_lq": (79, 80, 74)}
EXPECTED_NITER = {k: v[0] for k, v in EXPECTED.items()}
PRIMAL_FIRST = ("kron7_sinc", "poisson16_sinc")        # the primal side is solved before the dual one
DUAL_FIRST = ("kron8_sinc", "poisson16_sinc_lq")


def case_vectors(n, cname):
    b = rhs(n)
    return b, {"b": b, "neg": -b, "sin": other_c(n)}[cname]


_PAIRS = {}


def reference_pair(oracle, name, **extra):
    """(restatement with np.dot, restatement with exactly summed dots) of a case, as (x, y, stats) triples; computed once."""
    key = (name, tuple(sorted((k, id(v) if callable(v) else repr(v)) for k, v in extra.items())))
    if key not in _PAIRS:
        kind, n1, cname, kw = CASES[name]
        A_cpu = case_operator(oracle, kind, n1)
        S = A_cpu.to_scipy()
        St = S.T.tocsr()
        b, c = case_vectors(A_cpu.n, cname)
        kw = dict(kw, **extra)
        _PAIRS[key] = (qq.bilqr(S, b, c, At=St, **kw), qq.bilqr(S, b, c, At=St, dot=qq.fsum_dot, **kw))
    return _PAIRS[key]


def pair_deviation(pair):
    """The larger of the two histories' deviations between the two restatements of a pair."""
    (_, _, s1), (_, _, s2) = pair
    return max(qq.history_deviation(s1.residuals_primal, s2.residuals_primal),
               qq.history_deviation(s1.residuals_dual, s2.residuals_dual))


@pytest.mark.parametrize("name", list(CASES))
def test_case_list_condition(oracle, name):
    """A case may be in the list only if the restatement with np.dot and with math.fsum dots agree on niter, status and both
    history lengths, and BOTH residual histories agree to <= 1e-6 relative.  Measured (the larger of the two): kron7_sinc 1.2e-10,
    kron7_bb 6.4e-10, kron7_sinc_lq 3.9e-10, kron8_sinc 1.6e-7, kron8_bb and kron8_negc 8.2e-12, kron12_bb 2.6e-8, poisson16_sinc
    and poisson16_sinc_lq 5.3e-8, poisson16_bb 3.7e-9."""
    pair = reference_pair(oracle, name)
    (_, _, s1), (_, _, s2) = pair
    dev = pair_deviation(pair)
    print(f"{name}: niter = {s1.niter} / {s2.niter}, histories {len(s1.residuals_primal)} / {len(s1.residuals_dual)}, "
          f"deviation {dev:.1e}")
    assert (s1.niter, len(s1.residuals_primal), len(s1.residuals_dual)) == EXPECTED[name]
    assert (s2.niter, len(s2.residuals_primal), len(s2.residuals_dual)) == EXPECTED[name]
    assert s1.status == s2.status == (qq.BOTH_L if "lq" in name else qq.BOTH_C)
    assert s1.solved_primal and s1.solved_dual and s2.solved_primal and s2.solved_dual
    assert dev <= 1e-6


def test_the_list_has_both_orders_of_ending():
    for name in PRIMAL_FIRST:
        assert EXPECTED[name][1] < EXPECTED[name][2]
    for name in DUAL_FIRST:
        assert EXPECTED[name][2] < EXPECTED[name][1]


# ---- the reference's known answers, restated as data ------------------------------------------------------------------------------
def test_bc_breakdown():
    """test/test_utils.jl:204-209: cᴴb = 0 ends before the first iteration."""
    A = np.array([[1.0, 2.0], [3.0, 4.0]])
    x, y, st = qq.bilqr(A, np.array([0.0, 1.0]), np.array([1.0, 0.0]))
    assert st.niter == 0 and st.status == qq.BC_BREAKDOWN and not st.solved_primal and not st.solved_dual
    assert not x.any() and not y.any()
    assert list(st.residuals_primal) == [1.0] and list(st.residuals_dual) == [1.0]


def test_zero_right_hand_side():
    """b = 0: cᴴb = 0 is tested before anything looks at solved_lq = (‖r₀‖ == 0), so the status is the breakdown's."""
    x, y, st = qq.bilqr(np.eye(4) * 2.0, np.zeros(4), np.ones(4))
    assert st.niter == 0 and st.status == qq.BC_BREAKDOWN and not x.any() and not y.any()
    assert list(st.residuals_primal) == [0.0] and list(st.residuals_dual) == [2.0]


def test_unsymmetric_breakdown():
    """test/test_utils.jl:196-201: two iterations, pᴴq = 0 with neither primal point accepted: β₃ = 0 divides ⟨v₂, q⟩ and ‖q‖ (both
    zero), the primal estimate is NaN and the loop ends in the breakdown."""
    A = np.array([[0.0, 1.0], [-1.0, 0.0]])
    x, y, st = qq.bilqr(A, np.array([1.0, 0.0]), np.array([-1.0, 0.0]))
    assert st.niter == 2 and st.status == qq.BREAKDOWN and not st.solved_primal and not st.solved_dual
    assert np.array_equal(x, [0.0, 1.0]) and np.array_equal(y, [0.0, 0.0])
    assert np.array_equal(st.residuals_primal, [1.0, 1.0, math.nan], equal_nan=True)
    assert np.allclose(st.residuals_dual, [1.0, 1.0, math.sqrt(2.0)], rtol=0, atol=1e-15)


def test_identity():
    """A = I: pᴴq = 0 after one step; ‖r₁‖ of the LQ point is ‖b‖ and the CG estimate is NaN (β₂ = 0): breakdown, x = 0."""
    b = np.arange(1.0, 6.0)
    x, y, st = qq.bilqr(np.eye(5), b, b)
    assert st.niter == 1 and st.status == qq.BREAKDOWN and not x.any() and not y.any()
    assert np.array_equal(st.vectors["v"], st.vectors["v_prev"]) and np.array_equal(st.vectors["u"], st.vectors["u_prev"])


def test_diagonal_two_by_two():
    """diag(1, 2), b = [1, 1], c = [1, 2]: three iterations, x = [1, 1/2], y = [1, 1], both solved."""
    x, y, st = qq.bilqr(np.diag([1.0, 2.0]), np.array([1.0, 1.0]), np.array([1.0, 2.0]))
    assert st.niter == 3 and st.solved_primal and st.solved_dual
    assert np.allclose(x, [1.0, 0.5], rtol=0, atol=1e-15) and np.allclose(y, [1.0, 1.0], rtol=0, atol=1e-15)
    assert len(st.residuals_primal) == 3 and len(st.residuals_dual) == 4
    assert st.status in qq.STATUSES and len(st.status.encode()) > 95       # one of the four strings khip_stats.status cannot hold


def test_one_by_one():
    x, y, st = qq.bilqr(np.array([[2.0]]), np.array([3.0]), np.array([5.0]))
    assert st.niter == 2 and st.solved_primal and st.solved_dual
    # β₁ = √15 is rounded, and x and y come from it through a handful of products and quotients: a few ulps
    assert abs(x[0] - 1.5) <= 8 * qq.EPS * 1.5 and abs(y[0] - 2.5) <= 8 * qq.EPS * 2.5


def test_restatement_agrees_with_spsolve(oracle):
    """Both systems of an admitted case against a sparse direct solve: relative residuals <= 1e-6, the reference's bilqr_tol."""
    S = oracle.kron_unsymmetric(8).to_scipy()
    n = S.shape[0]
    b, c = rhs(n), other_c(n)
    (x, y, st), _ = reference_pair(oracle, "kron8_sinc")
    assert st.solved_primal and st.solved_dual
    xs = spla.spsolve(sp.csc_matrix(S), b)
    ys = spla.spsolve(sp.csc_matrix(S.T), c)
    assert np.linalg.norm(b - S @ x) <= 1e-6 * np.linalg.norm(b) and np.linalg.norm(c - S.T @ y) <= 1e-6 * np.linalg.norm(c)
    assert np.linalg.norm(x - xs) <= 1e-6 * np.linalg.norm(xs) and np.linalg.norm(y - ys) <= 1e-6 * np.linalg.norm(ys)


# ---- the two solvers it combines -----------------------------------------------------------------------------------------------
def _measured(oracle):
    """The case's own budget, as in the GPU tests: 10 x its np.dot-against-fsum deviation, at least 1e-8."""
    return max(1e-8, 10.0 * pair_deviation(reference_pair(oracle, "kron8_sinc")))


def test_primal_side_is_bilq(oracle):
    """While both run, x and the primal history are those of bilq!(A, b; c).  On kron8_sinc the primal side ends last, with bilq!'s
    own niter.  (The estimates differ in form: ⟨vₖ, q⟩ / βₖ₊₁ here, ⟨vₖ, vₖ₊₁⟩ there.)"""
    S = oracle.kron_unsymmetric(8).to_scipy()
    n = S.shape[0]
    (x, _, st), _ = reference_pair(oracle, "kron8_sinc")
    xb, sb = br.bilq(S, rhs(n), c=other_c(n), At=S.T.tocsr())
    assert sb.niter == st.niter == 41 and len(sb.residuals) == len(st.residuals_primal)
    tol = _measured(oracle)
    dev = qq.history_deviation(st.residuals_primal, sb.residuals)
    xdev = np.abs(x - xb).max() / np.abs(xb).max()
    print(f"primal history against bilq! {dev:.1e}, x {xdev:.1e}, budget {tol:.1e}")
    assert dev <= tol and xdev <= tol


def test_dual_side_is_qmr_on_the_adjoint_one_iteration_behind(oracle):
    """residuals_dual[1:] is the history of qmr!(A', c; c = b), and y its x after len - 2 iterations."""
    S = oracle.kron_unsymmetric(8).to_scipy()
    n = S.shape[0]
    (_, y, st), _ = reference_pair(oracle, "kron8_sinc")
    L = len(st.residuals_dual)
    xq, sq = qr.qmr(S.T.tocsr(), other_c(n), c=rhs(n), At=S, itmax=L - 2)
    assert len(sq.residuals) == L - 1
    tol = _measured(oracle)
    dev = qq.history_deviation(st.residuals_dual[1:], sq.residuals)
    ydev = np.abs(y - xq).max() / np.abs(xq).max()
    print(f"dual history against qmr! {dev:.1e}, y {ydev:.1e}, budget {tol:.1e}")
    assert dev <= tol and ydev <= tol


# ---- roles, warm start, callback -----------------------------------------------------------------------------------------------
def test_roles_after_one_to_five_iterations(oracle):
    """The names of the work vectors at the end of the loop: w₁ is written into w_prev2 at iteration 2 with no swap; from iteration 3
    on wₖ₋₁ is written over w_prev3 and the two are swapped, so w_prev2 is the newest w and w_prev3 the one before.  y_k - y_k-1 is
    parallel to w_prev2.  v, u hold vₖ₊₁, uₖ₊₁ and v_prev, u_prev the vectors before them."""
    S = oracle.kron_unsymmetric(7).to_scipy()
    n = S.shape[0]
    b, c = rhs(n), other_c(n)
    prev = None
    for k in (1, 2, 3, 4, 5):
        x, y, st = qq.bilqr(S, b, c, itmax=k)
        v = st.vectors
        assert st.niter == k
        if k == 1:
            assert not v["w_prev3"].any() and not v["w_prev2"].any() and not y.any()
            assert np.array_equal(v["v_prev"], b / st.beta1)
        else:
            assert np.array_equal(v["w_prev3"], prev["w_prev2"])
            assert np.array_equal(v["v_prev"], prev["v"]) and np.array_equal(v["u_prev"], prev["u"])
            step = y - prev["y"]
            w = v["w_prev2"]
            psi = float(step @ w) / float(w @ w)
            assert np.linalg.norm(step - psi * w) <= 1e-12 * np.linalg.norm(step)
        prev = dict(v, y=y)


def test_warm_start_of_the_restatement(oracle):
    S = oracle.kron_unsymmetric(8).to_scipy()
    n = S.shape[0]
    b, c = rhs(n), other_c(n)
    x, y, st = qq.bilqr(S, b, c, x0=np.linspace(-0.5, 0.5, n), y0=np.linspace(0.3, -0.2, n))
    assert st.solved_primal and st.solved_dual
    assert np.linalg.norm(b - S @ x) <= 1e-6 * np.linalg.norm(b) and np.linalg.norm(c - S.T @ y) <= 1e-6 * np.linalg.norm(c)


def test_callback_of_the_restatement(oracle):
    S = oracle.kron_unsymmetric(7).to_scipy()
    n = S.shape[0]
    seen = []

    def cb(w):
        seen.append((len(w.stats.residuals_primal), len(w.stats.residuals_dual)))
        return len(seen) == 3
    x, y, st = qq.bilqr(S, rhs(n), other_c(n), callback=cb)
    assert seen == [(2, 2), (3, 3), (4, 4)] and st.niter == 3 and st.status == "user-requested exit"


# ---- the Python mirror's tables -----------------------------------------------------------------------------------------------------
def test_python_mirror_exports_bilqr():
    """The mirror has the whole BiLQR surface (fails before the feature: K.bilqr did not exist)."""
    import krylov_jl_amd as K
    for name in ("bilqr", "bilqr_", "BilqrWorkspace", "AdjointStats"):
        assert hasattr(K, name), name
    for sym in ("khip_bilqr_default_params", "khip_bilqr_workspace_create", "khip_bilqr_workspace_adopt",
                "khip_bilqr_workspace_adopt_vector", "khip_bilqr_workspace_destroy", "khip_bilqr_warm_start", "khip_bilqr_solve",
                "khip_bilqr_solution_x", "khip_bilqr_solution_y", "khip_bilqr_stats", "khip_bilqr_adjoint_stats",
                "khip_bilqr_last_path", "khip_bilqr_vector", "khip_bilqr_workspace_bytes"):
        assert sym in K.SIGNATURES, sym
        assert hasattr(K.lib(), sym), sym
    assert K._INPLACE[K.BilqrWorkspace] == ("bilqr", K.bilqr_)
    assert "bilqr" not in K.WORKSPACE_KWARGS
    assert K.BilqrWorkspace.VECTORS == VECTORS
    assert len(K.SIGNATURES["khip_bilqr_workspace_adopt"][1]) == 3 + 11 + 1
    assert K.lib().khip_bilqr_default_params().transfer_to_bicg == 1
    header = open(os.path.join(ROOT, "include", "krylov_hip.h")).read()
    adopt = re.search(r"int khip_bilqr_workspace_adopt\(khip_ctx \*ctx, int64_t m, int64_t n, (.*?),\s*khip_bilqr_workspace \*\*out\);",
                      header, flags=re.S).group(1)
    assert tuple(re.findall(r"double \*(\w+)", adopt)) == VECTORS
    assert re.search(r"typedef struct \{\s*int transfer_to_bicg;[^}]*\} khip_bilqr_params;", header)


def test_no_status_string_is_lost():
    """Every status of src/bilqr.jl is in csrc/bilqr.cpp in full (khip_bilqr_adjoint_stats hands it over whole); the copy in
    khip_stats.status[96] is cut at a UTF-8 character boundary, so it decodes and is a prefix of the full string."""
    text = open(os.path.join(ROOT, "krylov.jl_amd", "csrc", "bilqr.cpp"), encoding="utf-8").read()
    lits = text
    for macro, chars in (("XL", "xᴸ"), ("XC", "xᶜ")):                       # the two macros the file spells xᴸ and xᶜ with
        lits = lits.replace(f'" {macro} "', chars).replace(f'" {macro};', chars + '";')
    lits = re.sub(r'"\s+"', "", lits)                                       # adjacent literals
    lits = re.sub(r"((?:\\x[0-9a-f]{2})+)", lambda m: bytes.fromhex(m.group(1).replace("\\x", "")).decode("utf-8"), lits)
    long_ones = 0
    for status in qq.STATUSES:
        assert status in lits, status
        raw = status.encode("utf-8")
        cut = raw[:95]
        while len(cut) < len(raw) and (raw[len(cut)] & 0xC0) == 0x80:      # the rule of copy_status
            cut = cut[:-1]
        assert status.startswith(cut.decode("utf-8"))                      # valid UTF-8 and a prefix
        long_ones += len(raw) > 95
    assert long_ones == 4 and len(qq.STATUSES[14].encode()) == 107 and max(len(s.encode()) for s in qq.STATUSES) == 110


def test_the_library_cuts_a_long_status_at_a_character_boundary():
    """khip_test_bilqr_status runs the product's status_of and copy_status on the host: every combination of the six solved flags
    (with and without tired / breakdown) ends in a string of the reference, handed over whole, and its char[96] copy is valid
    UTF-8, a prefix of it, and as long as fits; all four long strings are reached."""
    import ctypes as C

    import krylov_jl_amd as K
    seen = set()
    for mask in range(1 << 8):
        cut, full = C.create_string_buffer(96), C.c_char_p()
        assert K.lib().khip_test_bilqr_status(mask, cut, C.byref(full)) == 0
        whole, short = full.value.decode("utf-8"), cut.value.decode("utf-8")
        assert whole in qq.STATUSES and whole.startswith(short)
        raw = whole.encode("utf-8")
        assert len(cut.value) == len(raw) if len(raw) <= 95 else 92 < len(cut.value) <= 95
        seen.add(whole)
    assert {s for s in qq.STATUSES if len(s.encode()) > 95} <= seen and len(seen) >= 16
    xl = qq.STATUSES[14]                                                     # ᴸ sits at bytes 52-54: not where the cut falls
    cut, full = C.create_string_buffer(96), C.c_char_p()
    K.lib().khip_test_bilqr_status(0b010010, cut, C.byref(full))            # solved_lq_mach and solved_qr_tol
    assert full.value.decode("utf-8") == xl and cut.value == xl.encode("utf-8")[:95]


@ref_tree
def test_status_strings_are_the_reference_s():
    src = open(os.path.join(REFERENCE_SRC, "bilqr.jl")).read()
    assert set(re.findall(r'status = "([^"]*)"', src)) == set(qq.STATUSES)


@ref_tree
def test_forwarded_defaults_equal_the_reference():
    """FORWARDED_DEFAULTS["bilqr"] = kwargs_bilqr / def_kwargs_bilqr of src/bilqr.jl, names in order, defaults as values."""
    import krylov_jl_amd as K
    src = open(os.path.join(REFERENCE_SRC, "bilqr.jl")).read()
    names = re.findall(r":(\w+)", re.search(r"^kwargs_bilqr = \((.*?)\)", src, flags=re.M).group(1))
    table = re.search(r"^def_kwargs_bilqr = \((.*?)\)\n\n", src, flags=re.M | re.S).group(1)
    defaults = {m.group(1): m.group(2) for m in
                re.finditer(r":\(;\s*(\w+)(?:::[^=]+?)?\s*=\s*(.*?)\s*\)\s*[,)]?\s*$", table, flags=re.M)}
    assert list(defaults) == names
    mine = K.FORWARDED_DEFAULTS["bilqr"]
    assert list(mine) == names
    sq = math.sqrt(np.finfo(np.float64).eps)
    value = {"false": False, "true": True, "√eps(T)": sq, "0": 0, "Inf": math.inf, "kstdout": None}
    for k, expr in defaults.items():
        if k == "callback":
            assert expr == "workspace -> false" and mine[k] is K.default_callback
        else:
            assert mine[k] == value[expr] and type(mine[k]) is type(value[expr]), (k, expr, mine[k])


# ---- the Julia specialisation, as text (Julia does not run here) ---------------------------------------------------------------
JULIA_FIELDS = ("uₖ₋₁", "uₖ", "q", "vₖ₋₁", "vₖ", "p", "x", "y", "d̅", "wₖ₋₃", "wₖ₋₂")


def _julia_bilqr():
    glue = open(JULIA_SRC).read()
    m = re.search(r"function Krylov\.bilqr!\(ws::BilqrWs, A::HIPCsr, b::HIPVector, c::HIPVector;(.*?)\)\n(.*?)\nend\n", glue, flags=re.S)
    assert m, "no specialised Krylov.bilqr!"
    return glue, m.group(1), m.group(2)


def test_julia_bilqr_specialisation_shape():
    glue, sig, body = _julia_bilqr()
    assert "const BilqrWs = BilqrWorkspace{Float64,Float64,HIPVector}" in glue
    adopt = re.search(r"ccall\(\(:khip_bilqr_workspace_adopt, lib\), Cint, \((.*?)\),\n\s+CTX\[\]\.h, ws\.m, ws\.n, (.*?), r\)\)", glue,
                      flags=re.S)
    assert adopt, "bilqr_handle does not adopt the workspace's vectors"
    assert adopt.group(1).count("Ptr{Cdouble}") == 11
    assert [a.strip() for a in adopt.group(2).split(",")] == [f"ws.{f}.ptr" for f in JULIA_FIELDS]
    assert 'for (name, v) in (("dx", ws.Δx), ("dy", ws.Δy))\n    bilqr_adopt(h, name, v)' in body
    assert "invoke(Krylov.bilqr!, Tuple{BilqrWs,Any,AbstractVector{Float64},AbstractVector{Float64}}, ws, A, b, c;" in body
    # both histories reach a user's callback through khip_bilqr_adjoint_stats; the shared trampoline (stats.residuals) stays out
    assert "callback_args(bilqr_callback(user_callback(callback), h, sp, history), ws, sp, false)" in body
    assert "fill_adjoint_stats!(w.stats, h, sp, history); cb(w)" in glue
    assert "NATIVE_SOLVES[] += 1" in body and "LAST_PATH[] = ccall((:khip_bilqr_last_path, lib)" in body
    assert "khip_bilqr_warm_start" in body and "ws.warm_start = false" in body
    assert "st = fill_adjoint_stats!(ws.stats, h, sp, history)" in body
    assert "khip_bilqr_adjoint_stats" in glue and "stats.status = unsafe_string(Ptr{UInt8}(status[]))" in glue
    assert len(re.findall(r"(?<![\w])A'", body)) == 1, "A' is taken once per solve (and cached on the matrix by Base.adjoint)"
    tests = os.path.join(ROOT, "julia", "KrylovHIP", "test")
    bilqr_jl = open(os.path.join(tests, "bilqr.jl")).read()
    for piece in ("BilqrWorkspace(n, n, S)", "bilqr!(ws, A_gpu, b, c; history = true)", "unsymmetric_breakdown()", "bc_breakdown()",
                  "BILQR: systems of size $n"):
        assert piece in bilqr_jl, piece
    assert 'include("bilqr.jl")' in open(os.path.join(tests, "runtests.jl")).read()


@ref_tree
def test_julia_bilqr_specialisation():
    """Against the reference tree: every keyword of kwargs_bilqr is in the signature, and the glue reads only fields of
    BilqrWorkspace (src/krylov_workspaces.jl), the eleven vectors in the struct's order."""
    glue, sig, body = _julia_bilqr()
    src = open(os.path.join(REFERENCE_SRC, "bilqr.jl")).read()
    names = re.findall(r":(\w+)", re.search(r"^kwargs_bilqr = \((.*?)\)", src, flags=re.M).group(1))
    for kw in names:
        assert re.search(r"(?<![\w])" + kw + r"(?![\w])", sig), f"bilqr!: keyword {kw} of the reference is missing"
    ws_src = open(os.path.join(REFERENCE_SRC, "krylov_workspaces.jl")).read()
    struct = re.search(r"mutable struct BilqrWorkspace\{T,FC,S\}.*?\nend", ws_src, flags=re.S).group(0)
    ordered = re.findall(r"^\s+(\S+)\s+::", struct, flags=re.M)
    fields = set(ordered)
    assert tuple(f for f in ordered if f in JULIA_FIELDS) == JULIA_FIELDS
    used = set(re.findall(r"\bws\.([^\s.,;()\[\]]+)", body))
    handle = re.search(r"function bilqr_handle\(ws::BilqrWs\)\n(.*?)\nend\n", glue, flags=re.S).group(1)
    used |= set(re.findall(r"\bws\.([^\s.,;()\[\]]+)", handle))
    assert used <= fields, used - fields
    assert set(JULIA_FIELDS) | {"Δx", "Δy"} <= used
