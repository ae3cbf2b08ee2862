"""usymqr! without a GPU: the NumPy restatement (tests/usymqr_reference.py) against independent answers (the restatement of
minres! on a symmetric operator, the true residuals ‖b − A xₖ‖ and ‖Aᵀ rₖ₋₁‖, the reference's own known answers, numpy's least
squares); the condition that admits a case to the GPU tests' case list; the injected faults that the GPU tests' comparison rejects;
the Python mirror's tables against src/usymqr.jl; and the Julia specialisation's shape (as text: Julia does not run here)."""
import math
import os
import re
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import minres_reference as mr  # noqa: E402
import usymqr_reference as ur  # noqa: E402
from test_bilq_host import other_c, rhs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_SRC = "/root/reference/src"
JULIA_SRC = os.path.join(ROOT, "julia", "KrylovHIP", "src", "KrylovHIP.jl")
ref_tree = pytest.mark.skipif(not os.path.isdir(REFERENCE_SRC), reason="the reference tree is only present in the build container")

SOLVED, TIRED = ur.SOLVED, ur.TIRED


# ---- the systems of test/test_utils.jl that test/test_usymqr.jl solves, restated as data ----------------------------------------
def _ratio(rows, cols):
    i = np.arange(1.0, rows + 1)[:, None]
    j = np.arange(1.0, cols + 1)[None, :]
    return i / j - j / i


def _triangular_sign(n, diag):
    i = np.arange(n)[:, None]
    j = np.arange(n)[None, :]
    return np.where(i == j, diag, np.where(i < j, 1.0, -1.0))


def symmetric_definite(n=10):
    A = 4.0 * np.eye(n) + np.eye(n, k=1) + np.eye(n, k=-1)
    return A, A @ np.arange(1.0, n + 1)


def symmetric_indefinite(n=10):
    A = np.eye(n) + np.eye(n, k=1) + np.eye(n, k=-1)
    return A, A @ np.arange(1.0, n + 1)


def nonsymmetric_definite(n=10):
    A = _triangular_sign(n, float(n))
    return A, A @ np.arange(1.0, n + 1)


def nonsymmetric_indefinite(n=10):
    i = np.arange(1, n + 1)
    A = _triangular_sign(n, 0.0) + np.diag(n * (-1.0) ** (i * i))
    return A, A @ np.arange(1.0, n + 1)


def known_system(name):
    """(A, b, c) of a case of test/test_usymqr.jl; A is dense but for sparse_laplacian."""
    if name == "symmetric_definite":
        A, b = symmetric_definite()
        return A, b, b.copy()
    if name == "symmetric_indefinite":
        A, b = symmetric_indefinite()
        return A, b, b.copy()
    if name == "nonsymmetric_definite":
        A, b = nonsymmetric_definite()
        return A, b, b.copy()
    if name == "nonsymmetric_indefinite":
        A, b = nonsymmetric_indefinite()
        return A, b, b.copy()
    if name == "under_consistent":
        A = _ratio(10, 25)
        return A, A @ np.ones(25), np.ones(25)
    if name == "under_inconsistent":
        b = np.arange(1.0, 11.0)
        b[0] = -1.0
        return np.ones((10, 25)), b, np.array([1.0 if i % 2 == 0 else -1.0 for i in range(1, 26)])
    if name == "square_consistent":
        A = _ratio(10, 10)
        return A, A @ np.ones(10), np.ones(10)
    if name == "square_inconsistent":
        A = np.eye(10)
        A[0, 0] = 0.0
        return A, np.ones(10), np.ones(10)
    if name == "over_consistent":
        A = _ratio(25, 10)
        return A, A @ np.ones(10), np.ones(10)
    if name == "over_inconsistent":
        b = np.arange(1.0, 26.0)
        b[0] = -1.0
        return np.ones((25, 10)), b, np.array([2.0 ** i * (1.0 if i % 2 == 0 else -1.0) for i in range(1, 11)])
    raise KeyError(name)


CONSISTENT = ("symmetric_definite", "symmetric_indefinite", "nonsymmetric_definite", "nonsymmetric_indefinite", "square_consistent",
              "under_consistent", "over_consistent")
INCONSISTENT = ("square_inconsistent", "under_inconsistent", "over_inconsistent")
RECTANGULAR = ("under_consistent", "under_inconsistent", "over_consistent", "over_inconsistent")

# two 2 x 2 systems whose process breaks down on ONE side after the first step, in exact arithmetic and in floating point alike
# (every product and difference below is exact): with b = e₁ and c = 2 e₁, v₁ = u₁ = e₁ and α₁ = 2;
#   beta2_zero:  q = A e₁ − 2 e₁ = 0 (β₂ = 0, vₖ₊₁ = vₖ is kept), p = Aᵀe₁ − 2 e₁ = e₂ (γ₂ = 1); solved after one iteration
#   gamma2_zero: q = e₂ (β₂ = 1), p = 0 (γ₂ = 0, uₖ₊₁ = uₖ is kept); the loop goes on to itmax = m + n = 4 or to a test
BREAKDOWNS = {"beta2_zero": np.array([[2.0, 1.0], [0.0, 3.0]]), "gamma2_zero": np.array([[2.0, 0.0], [1.0, 3.0]])}
BREAKDOWN_B, BREAKDOWN_C = np.array([1.0, 0.0]), np.array([2.0, 0.0])


# ---- the GPU tests' case list (tests/test_gpu_usymqr.py imports it) ---------------------------------------------------------------
# name -> (operator, size parameter, shift added to the diagonal, c: None (c = b) | "neg" | "sin", keywords of usymqr)
# USYMQR loses orthogonality fast on these operators (a full solve of kron8 deviates by more than 10 % between np.dot and exact
# dots), so the long cases enter with an itmax.  24 = the largest absolute row sum of kron_unsymmetric.
CASES = {
    "kron4_it40": ("kron", 4, 0.0, None, dict(itmax=40)),         # the full solves (52 iterations) deviate by 1.2e-5 in their last
    "kron4_sinc": ("kron", 4, 0.0, "sin", {}),                    # entries, 4e-9 of the first: not admitted; this one (50) is
    "kron4_negc_it40": ("kron", 4, 0.0, "neg", dict(itmax=40)),
    "poisson8": ("poisson", 8, 0.0, None, {}),
    "poisson16": ("poisson", 16, 0.0, None, {}),
    "kron7_shift24_sinc": ("kron", 7, 24.0, "sin", {}),
    "kron8_shift24_sinc": ("kron", 8, 24.0, "sin", {}),
    "nsd10": ("nsd", 10, 0.0, None, {}),
    "kron7_it60": ("kron", 7, 0.0, None, dict(itmax=60)),
    "kron8_it60": ("kron", 8, 0.0, None, dict(itmax=60)),
    "kron8_sinc_it60": ("kron", 8, 0.0, "sin", dict(itmax=60)),
    "kron9_sinc_it60": ("kron", 9, 0.0, "sin", dict(itmax=60)),
    "kron11_sinc_it60": ("kron", 11, 0.0, "sin", dict(itmax=60)),
    "kron12_it60": ("kron", 12, 0.0, None, dict(itmax=60)),
    "poisson16_sinc_it100": ("poisson", 16, 0.0, "sin", dict(itmax=100)),
}
EXPECTED_NITER = {"kron4_it40": 40, "kron4_sinc": 50, "kron4_negc_it40": 40, "poisson8": 30, "poisson16": 62, "kron7_shift24_sinc": 28,
                  "kron8_shift24_sinc": 28, "nsd10": 9, "kron7_it60": 60, "kron8_it60": 60, "kron8_sinc_it60": 60, "kron9_sinc_it60": 60,
                  "kron11_sinc_it60": 60, "kron12_it60": 60, "poisson16_sinc_it100": 100}


def case_system(oracle, name):
    """(A as scipy CSR, b, c) of a case of the list."""
    kind, n1, shift, cname, _ = CASES[name]
    if kind == "nsd":
        A, b = nonsymmetric_definite(n1)
        return sp.csr_matrix(A), b, b.copy()
    S = (oracle.kron_unsymmetric(n1) if kind == "kron" else oracle.poisson3d(n1)).to_scipy().tocsr()
    n = S.shape[0]
    if shift:
        S = (S + shift * sp.identity(n)).tocsr()
    b = rhs(n)
    c = b.copy() if cname is None else (-b if cname == "neg" else other_c(n))
    return S, b, c


def deviation(h, ref, floor):
    """Largest difference of two histories relative to the reference's entry, an entry counting for no less than floor x the
    reference's first one (inf when the lengths differ)."""
    h, ref = np.asarray(h, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if h.shape != ref.shape:
        return math.inf
    if ref.size == 0:
        return 0.0
    if not (np.isfinite(h).all() and np.isfinite(ref).all()):
        return 0.0 if np.array_equal(h, ref, equal_nan=True) else math.inf
    return float(np.max(np.abs(h - ref) / np.maximum(np.abs(ref), floor * abs(ref[0]))))


HIST_FLOOR = 1e-12                                                    # x the history's first entry: the absolute part of a comparison
MEASURE_FLOOR = 1e-9                                                  # x the first entry: the floor of a case's own deviation


def history_excess(h, ref, budget):
    """0.0 when every entry of h is within budget x |entry of ref| + HIST_FLOOR x |ref's first entry| (tests/test_gpu_qmr.py's
    _hist_ok), else the largest deviation in units of that allowance, times budget; inf when the lengths differ."""
    h, ref = np.asarray(h, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if h.shape != ref.shape:
        return math.inf
    if ref.size == 0:
        return 0.0
    if not (np.isfinite(h).all() and np.isfinite(ref).all()):
        return 0.0 if np.array_equal(h, ref, equal_nan=True) else math.inf
    diff = np.abs(h - ref)
    with np.errstate(invalid="ignore", divide="ignore"):       # (a zero allowance admits a zero difference only)
        worst = float(np.max(np.where(diff == 0.0, 0.0, diff / (budget * np.abs(ref) + HIST_FLOOR * abs(ref[0])))))
    return 0.0 if worst <= 1.0 else worst * budget


def mismatches(got, ref, budget, x=None, x_ref=None):
    """What the GPU tests hold a solve to, as the list of what differs: niter, status, the two flags, both histories within `budget`
    of each entry plus the absolute floor 1e-12 x the first entry and, where given, x within `budget` of max|x|."""
    bad = []
    if got.niter != ref.niter:
        bad.append(f"niter {got.niter} != {ref.niter}")
    if got.status != ref.status:
        bad.append(f"status {got.status!r} != {ref.status!r}")
    if bool(got.solved) != bool(ref.solved) or bool(got.inconsistent) != bool(ref.inconsistent):
        bad.append(f"flags ({got.solved}, {got.inconsistent}) != ({ref.solved}, {ref.inconsistent})")
    for name in ("residuals", "Aresiduals"):
        d = history_excess(getattr(got, name), getattr(ref, name), budget)
        if d > 0.0:
            bad.append(f"{name} deviate by {d:.2e} > {budget:.2e}")
    if x is not None:
        x, x_ref = np.asarray(x), np.asarray(x_ref)
        both_nan = not np.isfinite(x_ref).all() and np.array_equal(np.isnan(x), np.isnan(x_ref))
        d = 0.0 if both_nan else (math.inf if not np.isfinite(x).all() else
                                  float(np.abs(x - x_ref).max() / max(np.abs(x_ref).max(), np.finfo(float).tiny)))
        if not d <= budget:
            bad.append(f"x deviates by {d:.2e} > {budget:.2e}")
    return bad


def pair_budget(pair):
    """max(1e-8, 10 x a system's own np.dot-versus-exact deviation): the library's dots are as far from the exact ones as np.dot's
    are, in another order, and ten of those distances bound what the recurrences make of them.  The own deviation is measured
    on both histories, an entry counting for no less than MEASURE_FLOOR x the first one (what lies below is covered by HIST_FLOOR:
    an admitted case deviates by <= 1e-6 x 1e-9 = 1e-15 of the first entry there), and on x relative to max|x|."""
    (x1, s1), (x2, s2) = pair
    own = max(deviation(s1.residuals, s2.residuals, MEASURE_FLOOR), deviation(s1.Aresiduals, s2.Aresiduals, MEASURE_FLOOR))
    if np.isfinite(x1).all() and np.isfinite(x2).all():
        own = max(own, float(np.abs(x1 - x2).max() / max(np.abs(x2).max(), np.finfo(float).tiny)))
    return max(1e-8, 10.0 * own)


_PAIRS = {}


def reference_pair(oracle, name, **extra):
    """(restatement with np.dot, restatement with exactly summed dots) of a case, as (x, stats) pairs; computed once."""
    key = (name, tuple(sorted((k, repr(v)) for k, v in extra.items())))
    if key not in _PAIRS:
        S, b, c = case_system(oracle, name)
        St = S.T.tocsr()
        kw = dict(CASES[name][4], **extra)
        _PAIRS[key] = (ur.usymqr(S, b, c, At=St, **kw), ur.usymqr(S, b, c, At=St, dot=ur.fsum_dot, **kw))
    return _PAIRS[key]


def budget(oracle, name, **extra):
    """pair_budget of a case of the list."""
    return pair_budget(reference_pair(oracle, name, **extra))


@pytest.mark.parametrize("name", list(CASES))
def test_case_list_condition(oracle, name):
    """A case may be in the list only if the restatement with np.dot and with math.fsum dots agree on niter, status, the flags and
    on both histories to <= 1e-6 relative, an entry counting for no less than 1e-9 x the first one."""
    (x1, s1), (_, s2) = reference_pair(oracle, name)
    dr = deviation(s1.residuals, s2.residuals, MEASURE_FLOOR)
    da = deviation(s1.Aresiduals, s2.Aresiduals, MEASURE_FLOOR)
    print(f"{name}: niter = {s1.niter} / {s2.niter}, deviation {dr:.1e} (residuals) {da:.1e} (Aresiduals), budget {budget(oracle, name):.1e}")
    assert s1.niter == s2.niter == EXPECTED_NITER[name], (s1.niter, s2.niter)
    assert s1.status == s2.status == (TIRED if "itmax" in CASES[name][4] else SOLVED)
    assert (s1.solved, s1.inconsistent) == (s2.solved, s2.inconsistent) == ("itmax" not in CASES[name][4], False)
    assert len(s1.residuals) == s1.niter + 1 and len(s1.Aresiduals) == s1.niter
    assert dr <= 1e-6 and da <= 1e-6


# ---- the restatement against independent answers ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n1", [8, 16])
def test_symmetric_operator_and_c_equal_b_give_minres(oracle, n1):
    """A symmetric and c = b: uₖ = vₖ, the tridiagonalisation is Lanczos' and usymqr! is MINRES: the residual history of the
    restatement of minres! (another recurrence for the same iterates), to rounding: 1e-8 of the first entry, the distance of two
    recurrences after up to 62 steps on histories that span nine decades."""
    S = oracle.poisson3d(n1).to_scipy()
    b = rhs(S.shape[0])
    _, su = ur.usymqr(S, b, b.copy(), At=S)
    _, sm = mr.minres(S, b, itmax=su.niter, atol=0.0, rtol=0.0)
    k = min(len(su.residuals), len(sm.residuals))
    assert k >= su.niter
    dev = float(np.max(np.abs(su.residuals[:k] - np.asarray(sm.residuals)[:k])) / su.residuals[0])
    print(f"poisson{n1}: {su.niter} iterations, usymqr against minres {dev:.2e} of the first entry")
    assert dev <= 1e-8


@pytest.mark.parametrize("name", list(CASES))
def test_histories_are_the_true_residuals(oracle, name):
    """residuals[k] = ‖b − A xₖ‖ and Aresiduals[k − 1] = ‖Aᵀ rₖ₋₁‖ over the first 20 iterations, xₖ from runs with itmax = k; 1e-10
    relative to each history's first entry."""
    S, b, c = case_system(oracle, name)
    St = S.T.tocsr()
    x_prev = np.zeros(S.shape[1])
    worst_r = worst_a = 0.0
    for k in range(1, min(20, EXPECTED_NITER[name]) + 1):
        x, st = ur.usymqr(S, b, c, At=St, itmax=k)
        assert st.niter == k
        worst_r = max(worst_r, abs(st.residuals[k] - np.linalg.norm(b - S @ x)) / st.residuals[0])
        worst_a = max(worst_a, abs(st.Aresiduals[k - 1] - np.linalg.norm(St @ (b - S @ x_prev))) / st.Aresiduals[0])
        x_prev = x
    print(f"{name}: residuals {worst_r:.1e}, Aresiduals {worst_a:.1e}")
    assert worst_r <= 1e-10 and worst_a <= 1e-10


@pytest.mark.parametrize("name", CONSISTENT)
def test_known_answers_consistent(name):
    """test/test_usymqr.jl: relative residual <= 1e-6 (and solved) on the consistent systems."""
    A, b, c = known_system(name)
    x, st = ur.usymqr(A, b, c)
    assert np.linalg.norm(b - A @ x) <= 1e-6 * np.linalg.norm(b)
    assert st.solved and not st.inconsistent and st.status == SOLVED


def test_known_answer_sparse_laplacian(oracle):
    S = oracle.poisson3d(16).to_scipy()
    b = np.ones(S.shape[0])
    x, st = ur.usymqr(S, b, b.copy(), At=S)
    assert st.solved and np.linalg.norm(b - S @ x) <= 1e-6 * np.linalg.norm(b)


@pytest.mark.parametrize("name", INCONSISTENT)
def test_known_answers_inconsistent(name):
    A, b, c = known_system(name)
    _, st = ur.usymqr(A, b, c)
    assert st.inconsistent and not st.solved and st.status == "unknown"


def test_zero_right_hand_side():
    x, st = ur.usymqr(np.eye(4) * 2.0, np.zeros(4), np.zeros(4))
    assert st.niter == 0 and st.solved and st.status == "x is a zero-residual solution" and not x.any()
    assert list(st.residuals) == [0.0] and len(st.Aresiduals) == 0


def test_over_consistent_is_the_least_squares_solution():
    """over_consistent's x against numpy.linalg.lstsq's, to 1e-8 of max|x|.  A[i, j] = i / j − j / i has rank 2, so the least-squares
    solutions form an affine space: lstsq returns the one of minimum norm, usymqr! the one in the span of c (here x = c = ones after
    one iteration, the system's own solution; it differs from lstsq's by 0.22 of max|x|).  What can be equal is the part of x in
    the row space of A, which is all of x whenever A has full column rank: that part equals lstsq's solution, and A x = A x_lstsq."""
    A, b, c = known_system("over_consistent")
    assert np.linalg.matrix_rank(A) == 2
    x, st = ur.usymqr(A, b, c)
    xl = np.linalg.lstsq(A, b, rcond=None)[0]
    row_part = np.linalg.lstsq(A, A @ x, rcond=None)[0]          # pinv(A) A x: the projection of x onto the row space
    print(f"over_consistent: x against lstsq {np.abs(x - xl).max() / np.abs(xl).max():.2e}, its row-space part "
          f"{np.abs(row_part - xl).max() / np.abs(xl).max():.2e}")
    assert st.solved and np.abs(row_part - xl).max() <= 1e-8 * np.abs(xl).max()
    assert np.linalg.norm(A @ x - A @ xl) <= 1e-8 * np.linalg.norm(b)


@pytest.mark.parametrize("name", list(BREAKDOWNS))
def test_breakdown_on_one_side(name):
    """β₂ = 0 keeps vₖ and γ₂ = 0 keeps uₖ, each without the other (:312-317)."""
    A = BREAKDOWNS[name]
    x, st = ur.usymqr(A, BREAKDOWN_B, BREAKDOWN_C, itmax=1)
    v = st.vectors
    if name == "beta2_zero":
        assert np.array_equal(v["v"], v["v_prev"]) and np.array_equal(v["u"], [0.0, 1.0]) and st.solved
        assert np.array_equal(x, [0.5, 0.0])
    else:
        assert np.array_equal(v["u"], v["u_prev"]) and np.array_equal(v["v"], [0.0, 1.0]) and not st.solved
    x, st = ur.usymqr(A, BREAKDOWN_B, BREAKDOWN_C)
    assert np.isfinite(x).all() and np.isfinite(st.residuals).all()


def test_roles_after_the_first_iterations(oracle):
    """The names of the work vectors at the end of the loop: w_prev = wₖ, w_prev2 = wₖ₋₁ (zeros after one iteration), and
    x_k - x_k-1 = ζₖ wₖ is parallel to w_prev."""
    S, b, c = case_system(oracle, "kron4_sinc")
    prev = None
    for k in (1, 2, 3, 4):
        x, st = ur.usymqr(S, b, c, itmax=k)
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


def test_callback_and_warm_start_of_the_restatement(oracle):
    S, b, c = case_system(oracle, "kron4_sinc")
    seen = []
    _, st = ur.usymqr(S, b, c, callback=lambda w: (seen.append((len(w.stats.residuals), len(w.stats.Aresiduals))), len(seen) == 3)[1])
    assert seen == [(2, 1), (3, 2), (4, 3)] and st.niter == 3 and st.status == "user-requested exit"
    x, st = ur.usymqr(S, b, c, x0=np.linspace(-0.5, 0.5, S.shape[0]))
    assert st.solved and np.linalg.norm(b - S @ x) <= 1e-6 * np.linalg.norm(b)


# ---- injected faults the comparison rejects ---------------------------------------------------------------------------------------
# fault -> the c ≠ b system that shows it.  With c = b on a symmetric operator "alpha_u" stays silent (uₖ = vₖ), which is why the
# case list has _sinc cases; "w_from_v" changes x alone, which is why the comparison includes x; "one_guard" needs γ₂ = 0 ≠ β₂;
# "kappa_k2" needs a system that ends as inconsistent, with atol = 0 (κ = rtol ‖Aᴴr₁‖ is never reached by ‖Aᴴr₁‖ itself).
FAULT_SYSTEMS = {"alpha_u": "kron4_sinc", "c_k": "kron4_sinc", "w_from_v": "kron4_sinc", "one_guard": "gamma2_zero",
                 "kappa_k2": "over_inconsistent"}
FAULT_KEYWORDS = {"kappa_k2": dict(atol=0.0)}


def _fault_system(oracle, where):
    if where in CASES:
        S, b, c = case_system(oracle, where)
        return S, b, c, budget(oracle, where)
    if where in BREAKDOWNS:
        return BREAKDOWNS[where], BREAKDOWN_B, BREAKDOWN_C, 1e-8
    A, b, c = known_system(where)
    return A, b, c, 1e-8


@pytest.mark.parametrize("fault", ur.FAULTS)
def test_comparison_rejects_injected_fault(oracle, fault):
    A, b, c, bud = _fault_system(oracle, FAULT_SYSTEMS[fault])
    assert not np.array_equal(b, c)
    kw = FAULT_KEYWORDS.get(fault, {})
    x, st = ur.usymqr(A, b, c, **kw)
    xf, sf = ur.usymqr(A, b, c, fault=fault, **kw)
    assert mismatches(st, st, bud, x, x) == []
    bad = mismatches(sf, st, bud, xf, x)
    print(f"{fault} on {FAULT_SYSTEMS[fault]} (budget {bud:.1e}): {bad}")
    assert bad, f"the comparison does not see {fault}"


def test_alpha_fault_is_silent_with_c_equal_b_on_a_symmetric_operator(oracle):
    S, b, c = case_system(oracle, "poisson8")
    x, st = ur.usymqr(S, b, c)
    xf, sf = ur.usymqr(S, b, c, fault="alpha_u")
    assert mismatches(sf, st, budget(oracle, "poisson8"), xf, x) == []


# ---- the Python mirror's tables -----------------------------------------------------------------------------------------------------
USYMQR_SYMBOLS = ("khip_usymqr_workspace_create", "khip_usymqr_workspace_adopt", "khip_usymqr_workspace_adopt_vector",
                  "khip_usymqr_workspace_destroy", "khip_usymqr_warm_start", "khip_usymqr_solve", "khip_usymqr_solution",
                  "khip_usymqr_stats", "khip_usymqr_aresiduals", "khip_usymqr_last_path", "khip_usymqr_vector",
                  "khip_usymqr_workspace_bytes")


def test_python_mirror_exports_usymqr():
    """The mirror has the whole USYMQR surface (fails before the feature: K.usymqr did not exist)."""
    import krylov_jl_amd as K
    for name in ("usymqr", "usymqr_", "UsymqrWorkspace"):
        assert hasattr(K, name), name
    for sym in USYMQR_SYMBOLS:
        assert sym in K.SIGNATURES, sym
        assert hasattr(K.lib(), sym), sym
    header = open(os.path.join(ROOT, "include", "krylov_hip.h")).read()
    assert sorted(set(re.findall(r"\b(khip_usymqr_[a-z_]+)\s*\(", header))) == sorted(USYMQR_SYMBOLS)
    assert K._INPLACE[K.UsymqrWorkspace] == ("usymqr", K.usymqr_)
    assert "usymqr" not in K.WORKSPACE_KWARGS
    assert K.UsymqrWorkspace.VECTORS == ("v_prev", "v", "q", "x", "w_prev2", "w_prev", "u_prev", "u", "p")
    assert K.UsymqrWorkspace.ROW_SIDE == ("v_prev", "v", "q")
    assert len(K.SIGNATURES["khip_usymqr_workspace_adopt"][1]) == 3 + 9 + 1
    assert "runs the primitive sequence" in K.UsymqrWorkspace.__doc__ and "reports 0" in K.UsymqrWorkspace.__doc__
    assert "last_path reports 0" in header


@ref_tree
def test_workspace_vectors_follow_the_reference_struct():
    ws_src = open(os.path.join(REFERENCE_SRC, "krylov_workspaces.jl")).read()
    struct = re.search(r"mutable struct UsymqrWorkspace\{T,FC,Sm,Sn\}.*?\nend", ws_src, flags=re.S).group(0)
    fields = re.findall(r"^\s+(\S+)\s+::\s+(Sm|Sn)\s*$", struct, flags=re.M)
    names = {"vₖ₋₁": "v_prev", "vₖ": "v", "q": "q", "Δx": "dx", "x": "x", "wₖ₋₂": "w_prev2", "wₖ₋₁": "w_prev", "uₖ₋₁": "u_prev",
             "uₖ": "u", "p": "p"}
    import krylov_jl_amd as K
    assert tuple(names[f] for f, _ in fields if f != "Δx") == K.UsymqrWorkspace.VECTORS
    assert tuple(names[f] for f, side in fields if side == "Sm") == K.UsymqrWorkspace.ROW_SIDE


@ref_tree
def test_forwarded_defaults_equal_the_reference():
    """FORWARDED_DEFAULTS["usymqr"] = kwargs_usymqr / def_kwargs_usymqr of src/usymqr.jl, names in order, defaults as values."""
    import krylov_jl_amd as K
    src = open(os.path.join(REFERENCE_SRC, "usymqr.jl")).read()
    names = re.findall(r":(\w+)", re.search(r"^kwargs_usymqr = \((.*?)\)", src, flags=re.M).group(1))
    table = re.search(r"^def_kwargs_usymqr = \((.*?)\)\n\n", src, flags=re.M | re.S).group(1)
    defaults = {m.group(1): m.group(2) for m in
                re.finditer(r":\(;\s*(\w+)(?:::[^=]+?)?\s*=\s*(.*?)\s*\)\s*[,)]?\s*$", table, flags=re.M)}
    assert list(defaults) == names
    mine = K.FORWARDED_DEFAULTS["usymqr"]
    assert list(mine) == names
    sq = math.sqrt(np.finfo(np.float64).eps)
    value = {"false": False, "true": True, "√eps(T)": sq, "0": 0, "Inf": math.inf, "kstdout": None}
    for k, expr in defaults.items():
        if k == "callback":
            assert expr == "workspace -> false" and mine[k] is K.default_callback
        else:
            assert mine[k] == value[expr] and type(mine[k]) is type(value[expr]), (k, expr, mine[k])
    assert re.search(r"^args_usymqr = \(:A, :b, :c\)$", src, flags=re.M) and re.search(r"^optargs_usymqr = \(:x0,\)$", src, flags=re.M)


# ---- the Julia specialisation, as text ----------------------------------------------------------------------------------------------
def _julia_usymqr():
    glue = open(JULIA_SRC).read()
    m = re.search(r"function Krylov\.usymqr!\(ws::UsymqrWs, A::HIPCsr, b::HIPVector, c::HIPVector;(.*?)\)\n(.*?)\nend\n", glue, flags=re.S)
    assert m, "no specialised Krylov.usymqr!"
    return glue, m.group(1), m.group(2)


def test_julia_usymqr_specialisation_shape():
    """The Julia usymqr! (checked as text: Julia does not run here): the UsymqrWs alias, the nine adopted vectors in the order of
    khip_usymqr_workspace_adopt, the fallback gate, the default callback's recognition, LAST_PATH, A' taken once, Aresiduals
    copied into the stats, and test/usymqr.jl reached from runtests.jl."""
    glue, sig, body = _julia_usymqr()
    assert "const UsymqrWs = UsymqrWorkspace{Float64,Float64,HIPVector,HIPVector}" in glue
    adopt = re.search(r"ccall\(\(:khip_usymqr_workspace_adopt, lib\), Cint, \((.*?)\),\n\s+CTX\[\]\.h, ws\.m, ws\.n, (.*?), r\)\)", glue,
                      flags=re.S)
    assert adopt, "usymqr_handle does not adopt the workspace's vectors"
    assert adopt.group(1).count("Ptr{Cdouble}") == 9
    assert [a.strip() for a in adopt.group(2).split(",")] == [f"ws.{f}.ptr" for f in
                                                              ("vₖ₋₁", "vₖ", "q", "x", "wₖ₋₂", "wₖ₋₁", "uₖ₋₁", "uₖ", "p")]
    assert "if !native_log(verbose, iostream)" in body
    assert "invoke(Krylov.usymqr!, Tuple{UsymqrWs,Any,AbstractVector{Float64},AbstractVector{Float64}}, ws, A, b, c;" in body
    assert "callback = callback === nothing ? (w -> false) : callback" in body
    assert "callback_args(user_callback(callback), ws, sp, history)" in body
    assert "NATIVE_SOLVES[] += 1" in body and "LAST_PATH[] = ccall((:khip_usymqr_last_path, lib)" in body
    assert "khip_usymqr_warm_start" in body and "ws.warm_start = false" in body
    assert "khip_usymqr_aresiduals" in body and "ws.stats.Aresiduals" in body
    assert len(re.findall(r"(?<![\w])A'", body)) == 1, "A' is taken once per solve (and cached on the matrix by Base.adjoint)"
    assert "callback = nothing" in sig and "fused::Int = 2" in sig
    tests = os.path.join(ROOT, "julia", "KrylovHIP", "test")
    usymqr_jl = open(os.path.join(tests, "usymqr.jl")).read()
    for piece in ("UsymqrWorkspace(n, n, S, S)", "native(2) do; usymqr!(ws, A_gpu, b, c; history = true); end",
                  "generic(usymqr!, ws2, A_gpu, b, c;", "USYMQR: system of $n equations in $n variables"):
        assert piece in usymqr_jl, piece
    assert 'include("usymqr.jl")' in open(os.path.join(tests, "runtests.jl")).read()


@ref_tree
def test_julia_usymqr_specialisation():
    """Against the reference tree: every keyword of kwargs_usymqr is in the signature, and the glue reads only fields of
    UsymqrWorkspace (src/krylov_workspaces.jl)."""
    glue, sig, body = _julia_usymqr()
    src = open(os.path.join(REFERENCE_SRC, "usymqr.jl")).read()
    names = re.findall(r":(\w+)", re.search(r"^kwargs_usymqr = \((.*?)\)", src, flags=re.M).group(1))
    for kw in names:
        assert re.search(r"(?<![\w])" + kw + r"(?![\w])", sig), f"usymqr!: keyword {kw} of the reference is missing"
    ws_src = open(os.path.join(REFERENCE_SRC, "krylov_workspaces.jl")).read()
    struct = re.search(r"mutable struct UsymqrWorkspace\{T,FC,Sm,Sn\}.*?\nend", ws_src, flags=re.S).group(0)
    fields = set(re.findall(r"^\s+(\S+)\s+::", struct, flags=re.M))
    used = set(re.findall(r"\bws\.([^\s.,;()\[\]]+)", body))
    handle = re.search(r"function usymqr_handle\(ws::UsymqrWs\)\n(.*?)\nend\n", glue, flags=re.S).group(1)
    used |= set(re.findall(r"\bws\.([^\s.,;()\[\]]+)", handle))
    assert used <= fields, used - fields
    assert {"vₖ₋₁", "vₖ", "q", "x", "wₖ₋₂", "wₖ₋₁", "uₖ₋₁", "uₖ", "p", "Δx"} <= used
