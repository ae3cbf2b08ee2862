"""usymlq! without a GPU: the NumPy restatement (tests/usymlq_reference.py) against independent answers (the restatement of bilq!
on a symmetric operator with c = b, the true residuals ‖b − A xₖ‖, the residual of the USYMCG point, the reference's own known
systems); the condition that admits a case to the GPU tests' case list; the injected faults that the GPU tests' comparison
rejects; the Python mirror's tables against src/usymlq.jl; and the Julia specialisation's shape (as text: Julia does not run
here)."""
import math
import os
import re
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bilq_reference as br  # noqa: E402
import usymlq_reference as ul  # noqa: E402
from test_bilq_host import other_c, rhs  # noqa: E402
from test_usymqr_host import (BREAKDOWN_B, BREAKDOWN_C, BREAKDOWNS, HIST_FLOOR, MEASURE_FLOOR, deviation, history_excess,  # noqa: E402,F401
                              known_system, nonsymmetric_definite)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_SRC = "/root/reference/src"
JULIA_SRC = os.path.join(ROOT, "julia", "KrylovHIP", "src", "KrylovHIP.jl")
ref_tree = pytest.mark.skipif(not os.path.isdir(REFERENCE_SRC), reason="the reference tree is only present in the build container")

SOLVED_LQ, SOLVED_CG, TIRED = ul.SOLVED_LQ, ul.SOLVED_CG, ul.TIRED

# the systems of test/test_usymlq.jl that tests/test_usymqr_host.py's known_system restates, and the one it adds
KNOWN = ("symmetric_definite", "symmetric_indefinite", "nonsymmetric_definite", "nonsymmetric_indefinite", "square_consistent",
         "under_consistent", "over_consistent")
RECTANGULAR = ("under_consistent", "over_consistent")
# unsymmetric_breakdown of test/test_utils.jl: α₁ = ⟨v₁, A u₁⟩ = 0, so δbar₁ = 0 exactly and the transfer is skipped at k = 1;
# the solve ends at k = 2 with x = e₂
UNSYM_BREAKDOWN = (np.array([[0.0, 1.0], [-1.0, 0.0]]), np.array([1.0, 0.0]), np.array([-1.0, 0.0]))
# a 1 x 1 system whose pivot δbar₁ = 1e-17 is below eps: guarded, the transfer is skipped and the LQ point of k = 2 solves it;
# unguarded, the USYMCG test fires at k = 1 (β₂ = 0 makes ρ₁ = 0)
TINY_PIVOT = (np.array([[1e-17]]), np.array([1.0]), np.array([2.0]))


# ---- the GPU tests' case list (tests/test_gpu_usymlq.py imports it) ---------------------------------------------------------------
# name -> (operator, size parameter, shift added to the diagonal, c: None (c = b) | "sin", keywords with the transfer on, keywords
# with the transfer off).  USYMLQ loses orthogonality as fast as USYMQR on the unshifted kron operators (the iteration counts of
# full solves of kron7 and kron8 differ between np.dot and exact dots), so the long cases enter with an itmax.  kron4 with c = sin
# is a full solve with the transfer (3.0e-7) and stops at 40 without it (8.4e-4 otherwise).  24 = the largest absolute row sum
# of kron_unsymmetric.
_IT60, _IT30, _IT100 = dict(itmax=60), dict(itmax=30), dict(itmax=100)
CASES = {
    "kron4_sinc": ("kron", 4, 0.0, "sin", {}, dict(itmax=40)),
    "poisson8": ("poisson", 8, 0.0, None, {}, {}),
    "poisson16": ("poisson", 16, 0.0, None, {}, {}),
    "kron7_shift24_sinc": ("kron", 7, 24.0, "sin", {}, {}),
    "kron8_shift24_sinc": ("kron", 8, 24.0, "sin", {}, {}),
    "kron7_it60": ("kron", 7, 0.0, None, _IT60, _IT60),
    "kron8_it60": ("kron", 8, 0.0, None, _IT60, _IT60),
    "kron8_sinc_it60": ("kron", 8, 0.0, "sin", _IT60, _IT60),
    "kron9_sinc_it60": ("kron", 9, 0.0, "sin", _IT60, _IT60),
    "kron11_sinc_it60": ("kron", 11, 0.0, "sin", _IT60, _IT60),
    "kron12_it60": ("kron", 12, 0.0, None, _IT60, _IT60),
    "kron16_sinc_it30": ("kron", 16, 0.0, "sin", _IT30, _IT30),
    "poisson16_sinc_it100": ("poisson", 16, 0.0, "sin", _IT100, _IT100),
}
TRANSFERS = (True, False)
# (niter, status) with the transfer on and off, pinned from the committed restatement
EXPECTED = {
    "kron4_sinc": ((50, SOLVED_CG), (40, TIRED)),
    "poisson8": ((30, SOLVED_CG), (36, SOLVED_LQ)),
    "poisson16": ((63, SOLVED_CG), (74, SOLVED_LQ)),
    "kron7_shift24_sinc": ((28, SOLVED_CG), (28, SOLVED_LQ)),
    "kron8_shift24_sinc": ((30, SOLVED_CG), (30, SOLVED_LQ)),
    "kron7_it60": ((60, TIRED), (60, TIRED)),
    "kron8_it60": ((60, TIRED), (60, TIRED)),
    "kron8_sinc_it60": ((60, TIRED), (60, TIRED)),
    "kron9_sinc_it60": ((60, TIRED), (60, TIRED)),
    "kron11_sinc_it60": ((60, TIRED), (60, TIRED)),
    "kron12_it60": ((60, TIRED), (60, TIRED)),
    "kron16_sinc_it30": ((30, TIRED), (30, TIRED)),
    "poisson16_sinc_it100": ((100, TIRED), (100, TIRED)),
}
SMALL_SIZES = (1, 2, 63, 64, 65)                                     # nonsymmetric_definite(n) with c = other_c(n)


def case_keywords(name, transfer):
    return dict(CASES[name][4 if transfer else 5], transfer_to_usymcg=transfer)


def case_system(oracle, name):
    """(A as scipy CSR, b, c) of a case of the list."""
    kind, n1, shift, cname = CASES[name][:4]
    S = (oracle.kron_unsymmetric(n1) if kind == "kron" else oracle.poisson3d(n1)).to_scipy().tocsr()
    n = S.shape[0]
    if shift:
        S = (S + shift * sp.identity(n)).tocsr()
    b = rhs(n)
    return S, b, (b.copy() if cname is None else other_c(n))


def mismatches(got, ref, budget, x=None, x_ref=None):
    """What the GPU tests hold a solve to, as the list of what differs: niter, status, solved, the history within `budget` of each
    entry plus the absolute floor 1e-12 x the first entry and, where given, x within `budget` of max|x|."""
    bad = []
    if got.niter != ref.niter:
        bad.append(f"niter {got.niter} != {ref.niter}")
    if got.status != ref.status:
        bad.append(f"status {got.status!r} != {ref.status!r}")
    if bool(got.solved) != bool(ref.solved) or bool(got.inconsistent):
        bad.append(f"flags ({got.solved}, {got.inconsistent}) != ({ref.solved}, False)")
    d = history_excess(got.residuals, ref.residuals, budget)
    if d > 0.0:
        bad.append(f"residuals deviate by {d:.2e} > {budget:.2e}")
    if x is not None:
        x, x_ref = np.asarray(x), np.asarray(x_ref)
        both_nan = not np.isfinite(x_ref).all() and np.array_equal(np.isnan(x), np.isnan(x_ref))
        dx = 0.0 if both_nan else (math.inf if not np.isfinite(x).all() else
                                   float(np.abs(x - x_ref).max() / max(np.abs(x_ref).max(), np.finfo(float).tiny)))
        if not dx <= budget:
            bad.append(f"x deviates by {dx:.2e} > {budget:.2e}")
    return bad


def own_deviation(pair):
    """A system's own np.dot-versus-exact deviation: on the history, an entry counting for no less than MEASURE_FLOOR x the first
    one, and on x relative to max|x|."""
    (x1, s1), (x2, s2) = pair
    own = deviation(s1.residuals, s2.residuals, MEASURE_FLOOR)
    if np.isfinite(x1).all() and np.isfinite(x2).all():
        own = max(own, float(np.abs(x1 - x2).max() / max(np.abs(x2).max(), np.finfo(float).tiny)))
    return own


def pair_budget(pair):
    """max(1e-8, 10 x own_deviation): the library's dots are as far from the exact ones as np.dot's are, in another order, and ten
    of those distances bound what the recurrences make of them (the rule of tests/test_usymqr_host.py)."""
    return max(1e-8, 10.0 * own_deviation(pair))


def dense_pair(A, b, c, **kw):
    A = np.asarray(A, dtype=np.float64)
    return ul.usymlq(A, b, c, **kw), ul.usymlq(A, b, c, dot=ul.fsum_dot, **kw)


_PAIRS = {}


def reference_pair(oracle, name, transfer=True, **extra):
    """(restatement with np.dot, restatement with exactly summed dots) of a case, as (x, stats) pairs; computed once."""
    key = (name, transfer, tuple(sorted((k, repr(v)) for k, v in extra.items())))
    if key not in _PAIRS:
        S, b, c = case_system(oracle, name)
        St = S.T.tocsr()
        kw = dict(case_keywords(name, transfer), **extra)
        _PAIRS[key] = (ul.usymlq(S, b, c, At=St, **kw), ul.usymlq(S, b, c, At=St, dot=ul.fsum_dot, **kw))
    return _PAIRS[key]


def budget(oracle, name, transfer=True, **extra):
    """pair_budget of a case of the list."""
    return pair_budget(reference_pair(oracle, name, transfer, **extra))


@pytest.mark.parametrize("transfer", TRANSFERS)
@pytest.mark.parametrize("name", list(CASES))
def test_case_list_condition(oracle, name, transfer):
    """A case may be in the list only if the restatement with np.dot and with math.fsum dots agree on niter, status and the flag
    and on the history to <= 1e-6 relative, an entry counting for no less than 1e-9 x the first one."""
    (x1, s1), (x2, s2) = pair = reference_pair(oracle, name, transfer)
    dr = deviation(s1.residuals, s2.residuals, MEASURE_FLOOR)
    print(f"{name} transfer={transfer}: niter = {s1.niter} / {s2.niter}, status {s1.status!r}, deviation {dr:.1e} (residuals) "
          f"{own_deviation(pair):.1e} (with x), budget {pair_budget(pair):.1e}")
    assert (s1.niter, s1.status) == (s2.niter, s2.status) == EXPECTED[name][0 if transfer else 1], (s1.niter, s1.status, s2.niter)
    limited = "itmax" in case_keywords(name, transfer)
    assert (s1.status == TIRED) == limited and s1.solved == s2.solved == (not limited)
    assert not (s1.solved_cg and not transfer)
    assert len(s1.residuals) == s1.niter + 1
    assert dr <= 1e-6


def test_case_list_keeps_its_size_and_sizes():
    assert len(CASES) >= 12
    assert {343, 512, 729, 1331, 1728, 4096} <= {CASES[k][1] ** 3 for k in CASES}
    assert max(CASES[k][1] ** 3 for k in CASES) <= 4096
    assert set(EXPECTED) == set(CASES)


@pytest.mark.parametrize("transfer", TRANSFERS)
@pytest.mark.parametrize("n", SMALL_SIZES)
def test_small_systems_are_admitted(n, transfer):
    M, b = nonsymmetric_definite(n)
    (x1, s1), (x2, s2) = dense_pair(M, b, other_c(n), transfer_to_usymcg=transfer)
    assert (s1.niter, s1.status) == (s2.niter, s2.status) and s1.solved
    assert deviation(s1.residuals, s2.residuals, MEASURE_FLOOR) <= 1e-6
    if n == 1:                                     # β₂ = γ₂ = 0: the transfer ends it at k = 1, the LQ point at k = 2
        assert (s1.niter, s1.status) == ((1, SOLVED_CG) if transfer else (2, SOLVED_LQ))
        assert np.array_equal(s1.vectors["v"], s1.vectors["v_prev"]) and np.array_equal(s1.vectors["u"], s1.vectors["u_prev"])


@pytest.mark.parametrize("transfer", TRANSFERS)
def test_unshifted_full_solves_are_not_admitted(oracle, transfer):
    """Why kron7 and kron8 enter with an itmax: their full solves do not pass the condition."""
    for n1 in (7, 8):
        S = oracle.kron_unsymmetric(n1).to_scipy().tocsr()
        b = rhs(S.shape[0])
        _, s1 = ul.usymlq(S, b, b.copy(), transfer_to_usymcg=transfer)
        _, s2 = ul.usymlq(S, b, b.copy(), transfer_to_usymcg=transfer, dot=ul.fsum_dot)
        print(f"kron{n1} transfer={transfer}: niter {s1.niter} / {s2.niter}, deviation {deviation(s1.residuals, s2.residuals, MEASURE_FLOOR):.1e}")
        assert not (s1.niter == s2.niter and deviation(s1.residuals, s2.residuals, MEASURE_FLOOR) <= 1e-6)


def test_kron4_sinc_without_the_transfer_needs_its_itmax(oracle):
    S, b, c = case_system(oracle, "kron4_sinc")
    _, s1 = ul.usymlq(S, b, c, transfer_to_usymcg=False)
    _, s2 = ul.usymlq(S, b, c, transfer_to_usymcg=False, dot=ul.fsum_dot)
    dev = deviation(s1.residuals, s2.residuals, MEASURE_FLOOR)
    print(f"kron4_sinc, transfer off, full solve: niter {s1.niter} / {s2.niter}, deviation {dev:.1e}")
    assert not (s1.niter == s2.niter and dev <= 1e-6)


# ---- the restatement against independent answers ------------------------------------------------------------------------------------
@pytest.mark.parametrize("transfer", TRANSFERS)
@pytest.mark.parametrize("n1", [8, 16])
def test_symmetric_operator_and_c_equal_b_give_bilq(oracle, n1, transfer):
    """A symmetric and c = b: uₖ = vₖ, both processes are Lanczos' and usymlq! is bilq! (whose residual formula carries ‖vₖ‖ = 1
    and ⟨vₖ, vₖ₊₁⟩ = 0 explicitly): the same niter, status and x, and the residual history of the restatement of bilq! to
    rounding: 1e-8 of the first entry, the distance of two recurrences after up to 60 steps (what
    test_usymqr_host.py allows usymqr! against minres!)."""
    S = oracle.poisson3d(n1).to_scipy()
    b = rhs(S.shape[0])
    xu, su = ul.usymlq(S, b, b.copy(), At=S, transfer_to_usymcg=transfer)
    xb, sb = br.bilq(S, b, c=b.copy(), At=S, transfer_to_bicg=transfer)
    dev = float(np.max(np.abs(su.residuals - np.asarray(sb.residuals))) / su.residuals[0])
    dx = np.abs(xu - xb).max() / np.abs(xb).max()
    print(f"poisson{n1} transfer={transfer}: {su.niter} iterations, usymlq against bilq {dev:.2e} of the first entry, x {dx:.2e}")
    assert su.niter == sb.niter and su.status == sb.status and su.solved
    assert dev <= 1e-8 and dx <= 1e-8


@pytest.mark.parametrize("name", list(CASES))
def test_history_is_the_true_residual(oracle, name):
    """With the transfer off, residuals[k] = ‖b − A xₖ‖ over the first 20 iterations, xₖ from runs with itmax = k; 1e-10 relative to
    the history's first entry."""
    S, b, c = case_system(oracle, name)
    St = S.T.tocsr()
    worst = 0.0
    for k in range(1, 20):
        x, st = ul.usymlq(S, b, c, At=St, itmax=k, transfer_to_usymcg=False)
        assert st.niter == k
        worst = max(worst, abs(st.residuals[k] - np.linalg.norm(b - S @ x)) / st.residuals[0])
    print(f"{name}: residuals {worst:.1e}")
    assert worst <= 1e-10


@pytest.mark.parametrize("name", ["poisson8", "poisson16", "kron7_shift24_sinc", "kron8_shift24_sinc", "kron4_sinc"])
def test_cg_ending_meets_the_tolerance(oracle, name):
    """On a `cg` ending the returned point is xᶜ = xᴸ + ζbarₖ d̅ₖ, whose residual is what the test bounded: ‖b − A x‖ ≤ ε, to the
    rounding of the recurrence (1e-10 ‖b‖, as above)."""
    S, b, c = case_system(oracle, name)
    x, st = ul.usymlq(S, b, c)
    eps = math.sqrt(ul.EPS) * (1.0 + np.linalg.norm(b))
    assert st.status == SOLVED_CG and st.solved_cg
    res = np.linalg.norm(b - S @ x)
    print(f"{name}: ‖b − A xᶜ‖ = {res:.3e}, ε = {eps:.3e}, the LQ point {np.linalg.norm(b - S @ st.vectors['x_lq']):.3e}")
    assert res <= eps + 1e-10 * np.linalg.norm(b)


@pytest.mark.parametrize("name,transfer", [(k, True) for k in KNOWN] + [(k, False) for k in KNOWN if k not in RECTANGULAR])
def test_known_answers(name, transfer):
    """test/test_usymlq.jl: relative residual <= 1e-6 on its systems, which it solves with the defaults (the transfer on); the
    square ones reach it without the transfer too (the LQ point of a rectangular consistent system need not: under_consistent
    ends at itmax with a residual of 5 %)."""
    A, b, c = known_system(name)
    x, st = ul.usymlq(A, b, c, transfer_to_usymcg=transfer)
    assert np.linalg.norm(b - A @ x) <= 1e-6 * np.linalg.norm(b)
    assert not st.inconsistent
    if name not in RECTANGULAR and name != "square_consistent":
        assert st.solved


def test_known_answer_sparse_laplacian(oracle):
    S = oracle.poisson3d(16).to_scipy()
    b = np.ones(S.shape[0])
    x, st = ul.usymlq(S, b, b.copy(), At=S)
    assert st.solved and np.linalg.norm(b - S @ x) <= 1e-6 * np.linalg.norm(b)


@pytest.mark.parametrize("transfer", TRANSFERS)
def test_unsymmetric_breakdown(transfer):
    """δbar₁ = 0 exactly: the guard skips the transfer at k = 1 (no 1 / 0), and k = 2 ends the solve with x = e₂."""
    A, b, c = UNSYM_BREAKDOWN
    x, st = ul.usymlq(A, b, c, transfer_to_usymcg=transfer)
    assert st.niter == 2 and st.solved and np.isfinite(st.residuals).all()
    assert np.allclose(x, [0.0, 1.0], atol=1e-15, rtol=0) and np.linalg.norm(b - A @ x) <= 1e-6


def test_zero_right_hand_side():
    x, st = ul.usymlq(np.eye(4) * 2.0, np.zeros(4), np.zeros(4))
    assert st.niter == 0 and st.solved and st.status == "x is a zero-residual solution" and not x.any()
    assert list(st.residuals) == [0.0]


@pytest.mark.parametrize("name", list(BREAKDOWNS))
def test_breakdown_on_one_side(name):
    """β₂ = 0 keeps vₖ and γ₂ = 0 keeps uₖ, each without the other (:297-302)."""
    A = BREAKDOWNS[name]
    x, st = ul.usymlq(A, BREAKDOWN_B, BREAKDOWN_C, itmax=1, transfer_to_usymcg=False)
    v = st.vectors
    if name == "beta2_zero":
        assert np.array_equal(v["v"], v["v_prev"]) and np.array_equal(v["u"], [0.0, 1.0])
    else:
        assert np.array_equal(v["u"], v["u_prev"]) and np.array_equal(v["v"], [0.0, 1.0])
    assert np.array_equal(v["dbar"], [1.0, 0.0])
    x, st = ul.usymlq(A, BREAKDOWN_B, BREAKDOWN_C)
    assert np.isfinite(x).all() and np.isfinite(st.residuals).all()


def test_roles_after_the_first_iterations(oracle):
    """dbar = d̅ₖ: u₁ after one iteration; afterwards the LQ step xₖ − xₖ₋₁ = ζₖ₋₁ dₖ₋₁ lies in span(d̅ₖ₋₁, uₖ) and d̅ₖ in the same plane,
    orthogonal to the step (dₖ₋₁ = cₖ d̅ₖ₋₁ + sₖ uₖ, d̅ₖ = sₖ d̅ₖ₋₁ − cₖ uₖ, with d̅ₖ₋₁ ⟂ uₖ of unit length)."""
    S, b, c = case_system(oracle, "kron4_sinc")
    prev = None
    for k in (1, 2, 3, 4):
        x, st = ul.usymlq(S, b, c, itmax=k, transfer_to_usymcg=False)
        d = st.vectors["dbar"]
        if k == 1:
            assert np.array_equal(d, c / math.sqrt(float(c @ c))) and np.array_equal(d, st.vectors["u_prev"]) and not x.any()
        else:
            step = x - prev[0]
            plane = np.stack([prev[1], st.vectors["u_prev"]], axis=1)          # d̅ₖ₋₁, uₖ
            for vec in (step, d):
                coef = np.linalg.lstsq(plane, vec, rcond=None)[0]
                assert np.linalg.norm(vec - plane @ coef) <= 1e-12 * np.linalg.norm(vec)
            assert abs(float(step @ d)) <= 1e-10 * np.linalg.norm(step) * np.linalg.norm(d)
        prev = (x, d)


def test_callback_and_warm_start_of_the_restatement(oracle):
    S, b, c = case_system(oracle, "kron4_sinc")
    seen = []
    _, st = ul.usymlq(S, b, c, callback=lambda w: (seen.append(len(w.stats.residuals)), len(seen) == 3)[1])
    assert seen == [2, 3, 4] and st.niter == 3 and st.status == "user-requested exit"
    x, st = ul.usymlq(S, b, c, x0=np.linspace(-0.5, 0.5, S.shape[0]))
    assert st.solved and np.linalg.norm(b - S @ x) <= 1e-6 * np.linalg.norm(b)


# ---- injected faults the comparison rejects ---------------------------------------------------------------------------------------
# fault -> the c ≠ b system that shows it.  "one_guard" needs γ₂ = 0 ≠ β₂; "cg_no_guard" needs a pivot below eps that is not zero;
# "cg_old_dbar" changes x alone, on a `cg` ending, which is why the comparison includes x; it needs a system whose two points lie
# further apart than the budget (poisson8: the LQ point's residual is a hundred times the USYMCG point's; the slip does not
# depend on c, and poisson8 with c = sin is not admitted: its iteration counts differ between the dot modes).
FAULT_SYSTEMS = {"alpha_u": "kron4_sinc", "one_guard": "gamma2_zero", "zeta_shift": "kron4_sinc", "dbar_from_v": "kron4_sinc",
                 "cg_no_guard": "tiny_pivot", "cg_old_dbar": "poisson8"}


def _fault_system(oracle, where):
    if where in CASES:
        S, b, c = case_system(oracle, where)
        return S, b, c, budget(oracle, where)
    if where in BREAKDOWNS:
        return BREAKDOWNS[where], BREAKDOWN_B, BREAKDOWN_C, 1e-8
    return TINY_PIVOT + (1e-8,)


@pytest.mark.parametrize("fault", ul.FAULTS)
def test_comparison_rejects_injected_fault(oracle, fault):
    A, b, c, bud = _fault_system(oracle, FAULT_SYSTEMS[fault])
    assert fault == "cg_old_dbar" or not np.array_equal(b, c)
    x, st = ul.usymlq(A, b, c)
    xf, sf = ul.usymlq(A, b, c, fault=fault)
    assert mismatches(st, st, bud, x, x) == []
    bad = mismatches(sf, st, bud, xf, x)
    print(f"{fault} on {FAULT_SYSTEMS[fault]} (budget {bud:.1e}): {bad}")
    assert bad, f"the comparison does not see {fault}"


def test_alpha_fault_is_silent_with_c_equal_b_on_a_symmetric_operator(oracle):
    S, b, c = case_system(oracle, "poisson8")
    x, st = ul.usymlq(S, b, c)
    xf, sf = ul.usymlq(S, b, c, fault="alpha_u")
    assert mismatches(sf, st, budget(oracle, "poisson8"), xf, x) == []


# ---- the Python mirror's tables -----------------------------------------------------------------------------------------------------
USYMLQ_SYMBOLS = ("khip_usymlq_default_params", "khip_usymlq_workspace_create", "khip_usymlq_workspace_adopt",
                  "khip_usymlq_workspace_adopt_vector", "khip_usymlq_workspace_destroy", "khip_usymlq_warm_start", "khip_usymlq_solve",
                  "khip_usymlq_solution", "khip_usymlq_stats", "khip_usymlq_last_path", "khip_usymlq_vector",
                  "khip_usymlq_workspace_bytes")


def test_python_mirror_exports_usymlq():
    """The mirror has the whole USYMLQ surface (fails before the feature: K.usymlq did not exist)."""
    import krylov_jl_amd as K
    for name in ("usymlq", "usymlq_", "UsymlqWorkspace"):
        assert hasattr(K, name), name
    for sym in USYMLQ_SYMBOLS:
        assert sym in K.SIGNATURES, sym
        assert hasattr(K.lib(), sym), sym
    header = open(os.path.join(ROOT, "include", "krylov_hip.h")).read()
    assert sorted(set(re.findall(r"\b(khip_usymlq_[a-z_]+)\s*\(", header))) == sorted(USYMLQ_SYMBOLS)
    assert K._INPLACE[K.UsymlqWorkspace] == ("usymlq", K.usymlq_)
    assert "usymlq" not in K.WORKSPACE_KWARGS
    assert K.UsymlqWorkspace.VECTORS == ("u_prev", "u", "p", "x", "dbar", "v_prev", "v", "q")
    assert K.UsymlqWorkspace.ROW_SIDE == ("v_prev", "v", "q")
    assert len(K.SIGNATURES["khip_usymlq_workspace_adopt"][1]) == 3 + 8 + 1
    assert "runs the primitive sequence" in K.UsymlqWorkspace.__doc__ and "reports 0" in K.UsymlqWorkspace.__doc__
    assert K.lib().khip_usymlq_default_params().transfer_to_usymcg == 1
    assert K.Context.PROFILE_TAGS[14] == "usymlq_p3" and len(K.Context.PROFILE_TAGS) == 15


@ref_tree
def test_workspace_vectors_follow_the_reference_struct():
    ws_src = open(os.path.join(REFERENCE_SRC, "krylov_workspaces.jl")).read()
    struct = re.search(r"mutable struct UsymlqWorkspace\{T,FC,Sm,Sn\}.*?\nend", ws_src, flags=re.S).group(0)
    fields = re.findall(r"^\s+(\S+)\s+::\s+(Sm|Sn)\s*$", struct, flags=re.M)
    names = {"uₖ₋₁": "u_prev", "uₖ": "u", "p": "p", "Δx": "dx", "x": "x", "d̅": "dbar", "vₖ₋₁": "v_prev", "vₖ": "v", "q": "q"}
    import krylov_jl_amd as K
    assert tuple(names[f] for f, _ in fields if f != "Δx") == K.UsymlqWorkspace.VECTORS
    assert tuple(names[f] for f, side in fields if side == "Sm") == K.UsymlqWorkspace.ROW_SIDE


@ref_tree
def test_forwarded_defaults_equal_the_reference():
    """FORWARDED_DEFAULTS["usymlq"] = kwargs_usymlq / def_kwargs_usymlq of src/usymlq.jl, names in order, defaults as values."""
    import krylov_jl_amd as K
    src = open(os.path.join(REFERENCE_SRC, "usymlq.jl")).read()
    names = re.findall(r":(\w+)", re.search(r"^kwargs_usymlq = \((.*?)\)", src, flags=re.M).group(1))
    table = re.search(r"^def_kwargs_usymlq = \((.*?)\)\n\n", src, flags=re.M | re.S).group(1)
    defaults = {m.group(1): m.group(2) for m in
                re.finditer(r":\(;\s*(\w+)(?:::[^=]+?)?\s*=\s*(.*?)\s*\)\s*[,)]?\s*$", table, flags=re.M)}
    assert list(defaults) == names
    mine = K.FORWARDED_DEFAULTS["usymlq"]
    assert list(mine) == names
    sq = math.sqrt(np.finfo(np.float64).eps)
    value = {"false": False, "true": True, "√eps(T)": sq, "0": 0, "Inf": math.inf, "kstdout": None}
    for k, expr in defaults.items():
        if k == "callback":
            assert expr == "workspace -> false" and mine[k] is K.default_callback
        else:
            assert mine[k] == value[expr] and type(mine[k]) is type(value[expr]), (k, expr, mine[k])
    assert re.search(r"^args_usymlq = \(:A, :b, :c\)$", src, flags=re.M) and re.search(r"^optargs_usymlq = \(:x0,\)$", src, flags=re.M)


# ---- the Julia specialisation, as text ----------------------------------------------------------------------------------------------
def _julia_usymlq():
    glue = open(JULIA_SRC).read()
    m = re.search(r"function Krylov\.usymlq!\(ws::UsymlqWs, A::HIPCsr, b::HIPVector, c::HIPVector;(.*?)\)\n(.*?)\nend\n", glue, flags=re.S)
    assert m, "no specialised Krylov.usymlq!"
    return glue, m.group(1), m.group(2)


def test_julia_usymlq_specialisation_shape():
    """The Julia usymlq! (checked as text: Julia does not run here): the UsymlqWs alias, the eight adopted vectors in the order of
    khip_usymlq_workspace_adopt, the fallback gate, the default callback's recognition, LAST_PATH, A' taken once, the transfer
    flag passed in khip_usymlq_params, and test/usymlq.jl reached from runtests.jl."""
    glue, sig, body = _julia_usymlq()
    assert "const UsymlqWs = UsymlqWorkspace{Float64,Float64,HIPVector,HIPVector}" in glue
    adopt = re.search(r"ccall\(\(:khip_usymlq_workspace_adopt, lib\), Cint, \((.*?)\),\n\s+CTX\[\]\.h, ws\.m, ws\.n, (.*?), r\)\)", glue,
                      flags=re.S)
    assert adopt, "usymlq_handle does not adopt the workspace's vectors"
    assert adopt.group(1).count("Ptr{Cdouble}") == 8
    assert [a.strip() for a in adopt.group(2).split(",")] == [f"ws.{f}.ptr" for f in
                                                              ("uₖ₋₁", "uₖ", "p", "x", "d̅", "vₖ₋₁", "vₖ", "q")]
    assert "if !native_log(verbose, iostream)" in body
    assert "invoke(Krylov.usymlq!, Tuple{UsymlqWs,Any,AbstractVector{Float64},AbstractVector{Float64}}, ws, A, b, c;" in body
    assert "callback = callback === nothing ? (w -> false) : callback" in body
    assert "callback_args(user_callback(callback), ws, sp, history)" in body
    assert "NATIVE_SOLVES[] += 1" in body and "LAST_PATH[] = ccall((:khip_usymlq_last_path, lib)" in body
    assert "khip_usymlq_warm_start" in body and "ws.warm_start = false" in body
    assert "UsymlqParams(Cint(transfer_to_usymcg))" in body
    assert len(re.findall(r"(?<![\w])A'", body)) == 1, "A' is taken once per solve (and cached on the matrix by Base.adjoint)"
    assert "callback = nothing" in sig and "fused::Int = 2" in sig and "transfer_to_usymcg::Bool = true" in sig
    tests = os.path.join(ROOT, "julia", "KrylovHIP", "test")
    usymlq_jl = open(os.path.join(tests, "usymlq.jl")).read()
    for piece in ("UsymlqWorkspace(n, n, S, S)", "native(2) do; usymlq!(ws, A_gpu, b, c; history = true); end",
                  "generic(usymlq!, ws2, A_gpu, b, c;", "USYMLQ: system of $n equations in $n variables"):
        assert piece in usymlq_jl, piece
    assert 'include("usymlq.jl")' in open(os.path.join(tests, "runtests.jl")).read()


@ref_tree
def test_julia_usymlq_specialisation():
    """Against the reference tree: every keyword of kwargs_usymlq is in the signature, and the glue reads only fields of
    UsymlqWorkspace (src/krylov_workspaces.jl)."""
    glue, sig, body = _julia_usymlq()
    src = open(os.path.join(REFERENCE_SRC, "usymlq.jl")).read()
    names = re.findall(r":(\w+)", re.search(r"^kwargs_usymlq = \((.*?)\)", src, flags=re.M).group(1))
    for kw in names:
        assert re.search(r"(?<![\w])" + kw + r"(?![\w])", sig), f"usymlq!: keyword {kw} of the reference is missing"
    ws_src = open(os.path.join(REFERENCE_SRC, "krylov_workspaces.jl")).read()
    struct = re.search(r"mutable struct UsymlqWorkspace\{T,FC,Sm,Sn\}.*?\nend", ws_src, flags=re.S).group(0)
    fields = set(re.findall(r"^\s+(\S+)\s+::", struct, flags=re.M))
    used = set(re.findall(r"\bws\.([^\s.,;()\[\]]+)", body))
    handle = re.search(r"function usymlq_handle\(ws::UsymlqWs\)\n(.*?)\nend\n", glue, flags=re.S).group(1)
    used |= set(re.findall(r"\bws\.([^\s.,;()\[\]]+)", handle))
    assert used <= fields, used - fields
    assert {"uₖ₋₁", "uₖ", "p", "x", "d̅", "vₖ₋₁", "vₖ", "q", "Δx"} <= used
