"""tricg! without a GPU: the NumPy restatement (tests/tricg_reference.py) against independent answers (the Galerkin point on a
reorthogonalised basis of the process; the true residual ‖[b; c] − K [xₖ; yₖ]‖; the reference's own known systems); the conditions
that the GPU tests' case list has to meet; the injected faults that the GPU tests' comparison rejects; the Python mirror's tables
against src/tricg.jl; and the Julia specialisation's shape (as text: Julia does not run here)."""
import math
import os
import re
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tricg_reference as tc  # noqa: E402
import test_usymlq_host as lq_host  # noqa: E402
from process_checks import ssy_mo_breakdown, ssy_mo_breakdown2, ssy_mo_breakdown3  # noqa: E402
from test_bilq_host import other_c, rhs  # noqa: E402
from test_usymqr_host import (BREAKDOWN_B, BREAKDOWN_C, BREAKDOWNS, MEASURE_FLOOR, deviation, history_excess,  # noqa: E402,F401
                              nonsymmetric_definite)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_SRC = "/root/reference/src"
JULIA_SRC = os.path.join(ROOT, "julia", "KrylovHIP", "src", "KrylovHIP.jl")
ref_tree = pytest.mark.skipif(not os.path.isdir(REFERENCE_SRC), reason="the reference tree is only present in the build container")

TIRED, SOLVED, INCONSISTENT = tc.TIRED, tc.SOLVED, tc.INCONSISTENT
SQD, SPD = (1.0, -1.0), (1.0, 1.0)
PARAMS = (SQD, SPD)                                                  # the (τ, ν) every case of the list runs at


# ---- the GPU tests' case list (tests/test_gpu_tricg.py imports it) ----------------------------------------------------------------
# test_usymlq_host.CASES, every one of them with its iteration cap (the one it has with the transfer on), at (τ, ν) = (1, −1) and
# (1, 1).  kron4_sinc as a full solve deviates by 1.2e-4 between the dot modes (n = 64: the process has lost its orthogonality by
# then): it enters with itmax = 40.  name -> (case of test_usymlq_host.CASES, keywords)
CASES = {name: (name, dict(lq_host.CASES[name][4])) for name in lq_host.CASES}
CASES["kron4_sinc"] = ("kron4_sinc", dict(itmax=40))
# (niter, status) at (1, −1) and at (1, 1), pinned from the committed restatement
EXPECTED = {
    "kron4_sinc": ((40, TIRED), (40, TIRED)),
    "poisson8": ((27, SOLVED), (21, SOLVED)),
    "poisson16": ((38, SOLVED), (28, SOLVED)),
    "kron7_shift24_sinc": ((28, SOLVED), (28, SOLVED)),
    "kron8_shift24_sinc": ((28, SOLVED), (28, SOLVED)),
    "kron7_it60": ((60, TIRED), (60, TIRED)),
    "kron8_it60": ((60, TIRED), (60, TIRED)),
    "kron8_sinc_it60": ((60, TIRED), (60, TIRED)),
    "kron9_sinc_it60": ((60, TIRED), (60, TIRED)),
    "kron11_sinc_it60": ((60, TIRED), (60, TIRED)),
    "kron12_it60": ((60, TIRED), (60, TIRED)),
    "kron16_sinc_it30": ((30, TIRED), (30, TIRED)),
    "poisson16_sinc_it100": ((100, TIRED), (100, TIRED)),
}
SMALL_SIZES = (1, 2, 63, 64, 65)                                     # nonsymmetric_definite(n) with c = other_c(n), at (1, −1)
# _sign_matrix(m, n) with the right-hand sides of tests/test_gpu_trilqr.py: b = A (1 … n), c = Aᵀ (−m … −1); (65, 33) as a full solve is
# not admitted (1.5e-5) and is not here
RECT_SHAPES = ((12, 20), (20, 12), (33, 65))
RECT_EXPECTED = {(12, 20): 9, (20, 12): 9, (33, 65): 11}             # niter of the full solves at (1, −1)


def case_keywords(name, params=SQD):
    return dict(CASES[name][1], tau=params[0], nu=params[1])


def case_system(oracle, name):
    """(A as scipy CSR, b, c) of a case of the list."""
    return lq_host.case_system(oracle, CASES[name][0])


def _sign_matrix(rows, cols):
    i = np.arange(rows)[:, None]
    j = np.arange(cols)[None, :]
    return np.where(i == j, 10.0, np.where(i < j, 1.0, -1.0))


def rect_system(m, n):
    A = _sign_matrix(m, n)
    return A, A @ np.arange(1.0, n + 1), A.T @ np.arange(-float(m), 0.0)


def _vec_dev(a, ref):
    a, ref = np.asarray(a), np.asarray(ref)
    if not np.isfinite(ref).all():
        return 0.0 if np.array_equal(np.isnan(a), np.isnan(ref)) else math.inf
    if not np.isfinite(a).all():
        return math.inf
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), np.finfo(float).tiny)) if ref.size else 0.0


def mismatches(got, ref, budget, x=None, x_ref=None, y=None, y_ref=None):
    """What the GPU tests hold a solve to, as the list of what differs: niter, status, the two flags, the history within `budget` of
    each entry plus the absolute floor 1e-12 x the first entry and, where given, x and y within `budget` of max|x| and max|y|."""
    bad = []
    if got.niter != ref.niter:
        bad.append(f"niter {got.niter} != {ref.niter}")
    if got.status != ref.status:
        bad.append(f"status {got.status!r} != {ref.status!r}")
    flags = lambda s: (bool(s.solved), bool(s.inconsistent))  # noqa: E731
    if flags(got) != flags(ref):
        bad.append(f"flags {flags(got)} != {flags(ref)}")
    d = history_excess(got.residuals, ref.residuals, budget)
    if d > 0.0:
        bad.append(f"residuals deviate by {d:.2e} > {budget:.2e}")
    for name, a, r in (("x", x, x_ref), ("y", y, y_ref)):
        if a is not None:
            d = _vec_dev(a, r)
            if not d <= budget:
                bad.append(f"{name} deviates by {d:.2e} > {budget:.2e}")
    return bad


def own_deviation(pair):
    """A system's own np.dot-versus-exact deviation: on the history, an entry counting for no less than MEASURE_FLOOR x the first
    one, and on x and y relative to max|x| and max|y|."""
    (x1, y1, s1), (x2, y2, s2) = pair
    own = deviation(s1.residuals, s2.residuals, MEASURE_FLOOR)
    for a, r in ((x1, x2), (y1, y2)):
        if np.isfinite(a).all() and np.isfinite(r).all():
            own = max(own, _vec_dev(a, r))
    return own


def pair_budget(pair):
    """max(1e-8, 10 x own_deviation): the library's dots are as far from the exact ones as np.dot's are, in another order, and ten
    of those distances bound what the recurrences make of them (the rule of tests/test_trilqr_host.py)."""
    return max(1e-8, 10.0 * own_deviation(pair))


def admitted(pair):
    """The rule of the list: both dot modes agree on niter, status and the flags, and on the history to <= 1e-6 relative, an entry
    counting for no less than 1e-9 x the first one."""
    (x1, y1, s1), (x2, y2, s2) = pair
    return (summary(s1) == summary(s2) and (s1.solved, s1.inconsistent) == (s2.solved, s2.inconsistent)
            and deviation(s1.residuals, s2.residuals, MEASURE_FLOOR) <= 1e-6)


def dense_pair(A, b, c, **kw):
    A = np.asarray(A, dtype=np.float64)
    return tc.tricg(A, b, c, **kw), tc.tricg(A, b, c, dot=tc.fsum_dot, **kw)


_PAIRS = {}


def reference_pair(oracle, name, params=SQD, **extra):
    """(restatement with np.dot, restatement with exactly summed dots) of a case, as (x, y, stats) triples; computed once."""
    key = (name, params, tuple(sorted((k, repr(v)) for k, v in extra.items())))
    if key not in _PAIRS:
        S, b, c = case_system(oracle, name)
        St = S.T.tocsr()
        kw = dict(case_keywords(name, params), **extra)
        _PAIRS[key] = (tc.tricg(S, b, c, At=St, **kw), tc.tricg(S, b, c, At=St, dot=tc.fsum_dot, **kw))
    return _PAIRS[key]


def budget(oracle, name, params=SQD, **extra):
    """pair_budget of a case of the list."""
    return pair_budget(reference_pair(oracle, name, params, **extra))


def summary(st):
    return (st.niter, st.status)


@pytest.mark.parametrize("params", PARAMS)
@pytest.mark.parametrize("name", list(CASES))
def test_case_list_condition(oracle, name, params):
    """A case may be in the list only if the restatement with np.dot and with math.fsum dots agree on niter, status and the flags,
    and on the history to <= 1e-6 relative, an entry counting for no less than 1e-9 x the first one."""
    (x1, y1, s1), (x2, y2, s2) = pair = reference_pair(oracle, name, params)
    d = deviation(s1.residuals, s2.residuals, MEASURE_FLOOR)
    print(f"{name} (τ, ν) = {params}: {summary(s1)} / {summary(s2)}, deviation {d:.1e} (history) {own_deviation(pair):.1e} (with x, y), "
          f"budget {pair_budget(pair):.1e}")
    assert summary(s1) == summary(s2) == EXPECTED[name][PARAMS.index(params)]
    assert admitted(pair)
    limited = case_keywords(name, params).get("itmax") == s1.niter                    # ended by itmax
    assert limited == (not s1.solved) and (s1.status == TIRED) == limited and not s1.inconsistent


def test_case_list_has_every_ending(oracle):
    """What the GPU tests rely on the list for, checked and not assumed: a solved and a tired ending, both parities of niter (the
    parity is what fix_after_device_loop gets wrong if it is wrong), an odd n and n = 4096."""
    assert set(EXPECTED) == set(CASES) == set(lq_host.CASES)
    rows = [EXPECTED[name][i] for name in CASES for i in range(len(PARAMS))]
    assert any(r[1] == SOLVED for r in rows) and any(r[1] == TIRED for r in rows)
    assert {r[0] % 2 for r in rows if r[1] == SOLVED} == {0, 1} and {r[0] % 2 for r in rows} == {0, 1}
    sizes = {case_system(oracle, name)[0].shape[0] for name in CASES}
    assert any(n % 2 for n in sizes) and 4096 in sizes and max(sizes) <= 4096


def test_kron4_sinc_as_a_full_solve_is_not_admitted(oracle):
    S, b, c = lq_host.case_system(oracle, "kron4_sinc")
    pair = dense_pair(S.toarray(), b, c)
    print(f"kron4_sinc, full solve: {summary(pair[0][2])} / {summary(pair[1][2])}, own deviation {own_deviation(pair):.1e}")
    assert not admitted(pair)


@pytest.mark.parametrize("n", SMALL_SIZES)
def test_small_systems_are_admitted(n):
    M, b = nonsymmetric_definite(n)
    pair = dense_pair(M, b, other_c(n))
    assert admitted(pair) and pair[0][2].solved


def test_smallest_system_is_singular_at_tau_nu_one():
    """n = 1 at τ = ν = 1: K = [1 1; 1 1] is singular, d₂ = 0 and the history is NaN.  The GPU tests leave it out."""
    M, b = nonsymmetric_definite(1)
    x, y, st = tc.tricg(M, b, other_c(1), tau=1.0, nu=1.0)
    assert np.isnan(st.residuals[1:]).all() and not st.solved


@pytest.mark.parametrize("full", (False, True))
@pytest.mark.parametrize("shape", RECT_SHAPES)
def test_rectangular_systems_are_admitted(shape, full):
    A, b, c = rect_system(*shape)
    pair = dense_pair(A, b, c, **({} if full else dict(itmax=5)))
    st = pair[0][2]
    s2 = pair[1][2]
    print(f"{shape} full={full}: {summary(st)}, own deviation {own_deviation(pair):.1e}, budget {pair_budget(pair):.1e}")
    if (shape, full) == ((33, 65), True):
        # The one entry of this restatement that misses the list's 1e-6: the LAST entry of the full solve, 1.3e-8 of the first and
        # already below the solve's own ε = 1.5e-8 ‖r₀‖, deviates by 1.7e-6 between the dot modes (2e-14 of the first entry: ζ₂ₖ₋₁
        # cancels).  Every entry the stopping test did not accept agrees to 1e-6, and so do niter, status and the flags; the GPU
        # test's budget follows the measured deviation by the rule of pair_budget, 1.7e-5.
        assert summary(st) == summary(s2) and (st.solved, st.inconsistent) == (s2.solved, s2.inconsistent)
        assert deviation(st.residuals[:-1], s2.residuals[:-1], MEASURE_FLOOR) <= 1e-6
        assert st.residuals[-1] <= math.sqrt(np.finfo(float).eps) * (1.0 + st.residuals[0]) and pair_budget(pair) <= 1e-4
    else:
        assert admitted(pair)
    assert (st.niter, st.solved) == ((RECT_EXPECTED[shape], True) if full else (5, False))
    assert len(pair[0][0]) == shape[0] and len(pair[0][1]) == shape[1]


def test_65_by_33_as_a_full_solve_is_not_admitted():
    A, b, c = rect_system(65, 33)
    assert not admitted(dense_pair(A, b, c))


# ---- the restatement against independent answers ------------------------------------------------------------------------------------
def block_matrix(A, tau, nu):
    A = A.toarray() if sp.issparse(A) else np.asarray(A, dtype=np.float64)
    m, n = A.shape
    return np.block([[tau * np.eye(m), A], [A.T, nu * np.eye(n)]])


def ssy_basis(A, b, c, k):
    """V (m x k) and U (n x k) of the process started from b and c, each new vector orthogonalised TWICE against all the earlier
    ones: an orthonormal basis independent of the three-term recurrences."""
    A = A.toarray() if sp.issparse(A) else np.asarray(A, dtype=np.float64)
    V, U = [b / np.linalg.norm(b)], [c / np.linalg.norm(c)]
    for _ in range(k - 1):
        q, p = A @ U[-1], A.T @ V[-1]
        for _ in range(2):
            for v in V:
                q = q - (v @ q) * v
            for u in U:
                p = p - (u @ p) * u
        V.append(q / np.linalg.norm(q))
        U.append(p / np.linalg.norm(p))
    return np.array(V).T, np.array(U).T


GALERKIN_OPERATORS = ("poisson8", "kron7_shift24_sinc", "kron8_it60")
GALERKIN_PARAMS = (SQD, SPD, (12.0, -0.7))
_GALERKIN_K = (1, 2, 3, 4, 5, 8, 12, 15)


def _galerkin_system(oracle, name):
    S, b, _ = case_system(oracle, name)
    return S, b, other_c(S.shape[0])


@pytest.mark.parametrize("params", GALERKIN_PARAMS)
@pytest.mark.parametrize("name", GALERKIN_OPERATORS)
def test_iterate_is_the_galerkin_point(oracle, name, params):
    """[xₖ; yₖ] = W (WᵀKW)⁻¹ Wᵀ[b; c] with W = blkdiag(Vₖ, Uₖ) on a twice-reorthogonalised basis: 1e-10 of the largest entry."""
    S, b, c = _galerkin_system(oracle, name)
    m, n = S.shape
    Kmat = block_matrix(S, *params)
    V, U = ssy_basis(S, b, c, max(_GALERKIN_K))
    d = np.concatenate([b, c])
    worst = 0.0
    for k in _GALERKIN_K:
        x, y, st = tc.tricg(S, b, c, tau=params[0], nu=params[1], itmax=k, atol=0.0, rtol=0.0)
        assert st.niter == k
        W = np.block([[V[:, :k], np.zeros((m, k))], [np.zeros((n, k)), U[:, :k]]])
        z = W @ np.linalg.solve(W.T @ Kmat @ W, W.T @ d)
        worst = max(worst, float(np.abs(np.concatenate([x, y]) - z).max() / np.abs(z).max()))
    print(f"{name} (τ, ν) = {params}: {worst:.1e}")
    assert worst <= 1e-10


@pytest.mark.parametrize("name,params", [("kron4_sinc", SQD), ("poisson8", SPD), ("kron7_shift24_sinc", SQD), ("kron16_sinc_it30", SPD)])
def test_history_is_the_true_residual(oracle, name, params):
    """residuals[k] = ‖[b; c] − K [xₖ; yₖ]‖ over the first 19 iterations, from runs with itmax = k; 1e-10 of the first entry."""
    S, b, c = case_system(oracle, name)
    St = S.T.tocsr()
    worst = 0.0
    for k in range(1, 20):
        x, y, st = tc.tricg(S, b, c, At=St, tau=params[0], nu=params[1], itmax=k, atol=0.0, rtol=0.0)
        assert st.niter == k
        r = np.concatenate([b - params[0] * x - S @ y, c - St @ x - params[1] * y])
        worst = max(worst, abs(st.residuals[k] - np.linalg.norm(r)) / st.residuals[0])
    print(f"{name} (τ, ν) = {params}: {worst:.1e}")
    assert worst <= 1e-10


# test/test_utils.jl's systems that test/test_tricg.jl solves with M = N = I, restated as data
def sqd_matrix(n=5):
    """A of sqd(n) and of saddle_point(n): A[i, j] = 2^(i/j) j + (−1)^(i−j) n (i − 1), i, j = 1 … n; b = ones(n)."""
    i = np.arange(1.0, n + 1)[:, None]
    j = np.arange(1.0, n + 1)[None, :]
    return 2.0 ** (i / j) * j + (-1.0) ** (i - j) * n * (i - 1), np.ones(n)


def small_sqd(transpose):
    A = np.array([[1.0, 0.0], [0.0, -1.0], [3.0, 0.0]])
    A = A.T.copy() if transpose else A
    return A, np.ones(A.shape[0]), -np.ones(A.shape[1])


def rel_residual(A, b, c, x, y, tau, nu):
    r = np.concatenate([b - tau * x - A @ y, c - A.T @ x - nu * y])
    return float(np.linalg.norm(r) / np.linalg.norm(np.concatenate([b, c])))


KNOWN_PARAMS = ((1.0, -1.0), (1.0, 0.0), (-1.0, 1.0), (1.0, 1.0), (-1.0, -1.0), (12.0, -0.7), (-1e-6, 1e-8))


@pytest.mark.parametrize("params", KNOWN_PARAMS)
def test_known_sqd_and_saddle_point_systems(params):
    """sqd(5) and saddle_point(5) (the same A and b) with c = −b, test/test_tricg.jl at its tolerance 1e-6."""
    A, b = sqd_matrix()
    x, y, st = tc.tricg(A, b, -b, tau=params[0], nu=params[1])
    res = rel_residual(A, b, -b, x, y, *params)
    print(f"(τ, ν) = {params}: {summary(st)}, residual {res:.1e}")
    assert res <= 1e-6


def test_flags_equal_their_tau_and_nu():
    A, b = sqd_matrix()
    for flag, params in (("flip", (-1.0, 1.0)), ("spd", (1.0, 1.0)), ("snd", (-1.0, -1.0))):
        x, y, st = tc.tricg(A, b, -b, tau=3.0, nu=4.0, **{flag: True})
        x2, y2, st2 = tc.tricg(A, b, -b, tau=params[0], nu=params[1])
        assert np.array_equal(x, x2) and np.array_equal(y, y2) and np.array_equal(st.residuals, st2.residuals)
    for pair, msg in ((("spd", "flip"), "SPD and SQD"), (("snd", "flip"), "SND and SQD"), (("spd", "snd"), "SPD and SND")):
        with pytest.raises(ValueError, match="The matrix cannot be " + msg):
            tc.tricg(A, b, -b, **{k: True for k in pair})


def test_zero_right_hand_sides():
    """b = 0 and c = 0 are ordinary solves (v₁ = 0 or u₁ = 0 by a fill); c = 0 ends at itmax = m + n unsolved with a residual still
    below 1e-6; b = c = 0 starts solved."""
    A, b = sqd_matrix()
    x, y, st = tc.tricg(A, np.zeros(5), -b)
    assert rel_residual(A, np.zeros(5), -b, x, y, 1.0, -1.0) <= 1e-6 and np.isfinite(st.residuals).all()
    x, y, st = tc.tricg(A, b, np.zeros(5))
    print(f"c = 0: {summary(st)}, residual {rel_residual(A, b, np.zeros(5), x, y, 1.0, -1.0):.1e}")
    assert rel_residual(A, b, np.zeros(5), x, y, 1.0, -1.0) <= 1e-6
    assert summary(st) == (10, TIRED) and not st.solved
    x, y, st = tc.tricg(A, np.zeros(5), np.zeros(5))
    assert st.niter == 0 and st.solved and st.status == SOLVED and not x.any() and not y.any() and list(st.residuals) == [0.0]


@pytest.mark.parametrize("transpose", (False, True))
def test_small_sqd(transpose):
    A, b, c = small_sqd(transpose)
    x, y, st = tc.tricg(A, b, c)
    assert rel_residual(A, b, c, x, y, 1.0, -1.0) <= 1e-6 and len(x) == A.shape[0] and len(y) == A.shape[1]


def _breakdown(transpose):
    A, b, c = ssy_mo_breakdown()
    return (A.T.copy(), c, b) if transpose else (A, b, c)


@pytest.mark.parametrize("transpose", (False, True))
def test_breakdown_systems(transpose):
    """ssy_mo_breakdown, both orientations: solved at (1, −1); at τ = ν = 1 K is singular and the solve ends after two iterations
    with `inconsistent`."""
    A, b, c = _breakdown(transpose)
    x, y, st = tc.tricg(A, b, c)
    assert rel_residual(A, b, c, x, y, 1.0, -1.0) <= 1e-6
    assert np.linalg.matrix_rank(block_matrix(A, 1.0, 1.0)) < sum(A.shape)
    x, y, st = tc.tricg(A, b, c, tau=1.0, nu=1.0)
    assert st.inconsistent and not st.solved and summary(st) == (2, INCONSISTENT)


@pytest.mark.parametrize("system", (ssy_mo_breakdown2, ssy_mo_breakdown3))
def test_breakdown_systems_2_and_3(system):
    A, b, c = system()
    x, y, st = tc.tricg(A, b, c)
    assert rel_residual(A, b, c, x, y, 1.0, -1.0) <= 1e-6


def test_breakdown_on_one_side():
    """beta2_zero: β₂ = 0 exactly, the undivided zero q becomes v₂ and the solve ends solved after three iterations; gamma2_zero
    ends after one."""
    x, y, st = tc.tricg(BREAKDOWNS["beta2_zero"], BREAKDOWN_B, BREAKDOWN_C)
    assert summary(st) == (3, SOLVED) and rel_residual(BREAKDOWNS["beta2_zero"], BREAKDOWN_B, BREAKDOWN_C, x, y, 1.0, -1.0) <= 1e-6
    x, y, st = tc.tricg(BREAKDOWNS["gamma2_zero"], BREAKDOWN_B, BREAKDOWN_C)
    print(f"gamma2_zero: {summary(st)}")
    assert st.niter == 1


def test_roles_after_the_first_iteration(oracle):
    S, b, c = case_system(oracle, "kron7_it60")
    x, y, st = tc.tricg(S, b, c, itmax=1)
    v = st.vectors
    assert not v["gy_prev"].any() and np.array_equal(v["gx_prev"], v["v_prev"]) and np.array_equal(v["gy"], v["u_prev"])


def test_callback_and_warm_start_of_the_restatement(oracle):
    S, b, c = case_system(oracle, "kron4_sinc")
    seen = []
    _, _, st = tc.tricg(S, b, c, callback=lambda w: (seen.append(len(w.stats.residuals)), len(seen) == 3)[1])
    assert seen == [2, 3, 4] and st.niter == 3 and st.status == "user-requested exit"
    n = S.shape[0]
    x, y, st = tc.tricg(S, b, c, x0=np.linspace(-0.5, 0.5, n), y0=np.linspace(0.25, -0.25, n), tau=12.0, nu=-0.7)
    assert st.solved and rel_residual(S, b, c, x, y, 12.0, -0.7) <= 1e-6


# ---- injected faults the comparison rejects ---------------------------------------------------------------------------------------
# fault -> where it shows: "guard_ne_zero" needs a βₖ₊₁ or γₖ₊₁ that is tiny but not zero (ssy_mo_breakdown transposed, where the process
# breaks down on one side up to a rounding error and the solve ends after two iterations)
FAULT_SYSTEMS = {"g_rotation_swapped": "kron4_sinc", "guard_ne_zero": "breakdown_transposed", "sigma_for_eta": "kron4_sinc",
                 "no_delta_in_gy": "kron4_sinc", "pi_swapped": "kron4_sinc", "zeta_without_delta": "kron4_sinc"}


def _fault_run(oracle, where, fault):
    if where == "breakdown_transposed":
        A, b, c = _breakdown(True)
        pair = dense_pair(A, b, c)
        return pair[0], tc.tricg(A, b, c, fault=fault), pair_budget(pair)
    S, b, c = case_system(oracle, where)
    St = S.T.tocsr()
    return reference_pair(oracle, where)[0], tc.tricg(S, b, c, At=St, fault=fault, **case_keywords(where)), budget(oracle, where)


@pytest.mark.parametrize("fault", tc.FAULTS)
def test_comparison_rejects_injected_fault(oracle, fault):
    (x, y, st), (xf, yf, sf), bud = _fault_run(oracle, FAULT_SYSTEMS[fault], fault)
    assert mismatches(st, st, bud, x, x, y, y) == []
    bad = mismatches(sf, st, bud, xf, x, yf, y)
    print(f"{fault} on {FAULT_SYSTEMS[fault]} (budget {bud:.1e}): {bad}")
    assert bad, f"the comparison does not see {fault}"


# ---- the Python mirror's tables -----------------------------------------------------------------------------------------------------
TRICG_SYMBOLS = ("khip_tricg_default_params", "khip_tricg_workspace_create", "khip_tricg_workspace_adopt",
                 "khip_tricg_workspace_adopt_vector", "khip_tricg_workspace_destroy", "khip_tricg_warm_start", "khip_tricg_solve",
                 "khip_tricg_solution_x", "khip_tricg_solution_y", "khip_tricg_stats", "khip_tricg_last_path", "khip_tricg_vector",
                 "khip_tricg_workspace_bytes")


def test_python_mirror_exports_tricg():
    """The mirror has the whole TriCG surface (fails before the feature: K.tricg did not exist)."""
    import krylov_jl_amd as K
    for name in ("tricg", "tricg_", "TricgWorkspace", "CTricgParams"):
        assert hasattr(K, name), name
    for sym in TRICG_SYMBOLS:
        assert sym in K.SIGNATURES, sym
        assert hasattr(K.lib(), sym), sym
    header = open(os.path.join(ROOT, "include", "krylov_hip.h")).read()
    assert sorted(set(re.findall(r"\b(khip_tricg_[a-z_]+)\s*\(", header))) == sorted(TRICG_SYMBOLS)
    assert K._INPLACE[K.TricgWorkspace] == ("tricg", K.tricg_)
    assert "tricg" not in K.WORKSPACE_KWARGS
    assert K.TricgWorkspace.VECTORS == tc.VECTORS and K.TricgWorkspace.ROW_SIDE == tc.ROW_SIDE
    assert len(K.SIGNATURES["khip_tricg_workspace_adopt"][1]) == 3 + 12 + 1
    assert "runs the primitive sequence" in K.TricgWorkspace.__doc__ and "reports 0" in K.TricgWorkspace.__doc__
    prm = K.lib().khip_tricg_default_params()
    assert (prm.tau, prm.nu, prm.spd, prm.snd, prm.flip) == (1.0, -1.0, 0, 0, 0)
    assert [f[0] for f in K.CTricgParams._fields_] == ["tau", "nu", "spd", "snd", "flip"]
    assert K.Context.PROFILE_FAMILIES[16] == "tricg_p3" and K.Context.PROFILE_FAMILIES[:15] == K.Context.PROFILE_TAGS
    for piece in ("M and N other than I", "complex types", "fused kernels for m != n"):
        assert piece in header, piece


@ref_tree
def test_workspace_vectors_follow_the_reference_struct():
    ws_src = open(os.path.join(REFERENCE_SRC, "krylov_workspaces.jl")).read()
    struct = re.search(r"mutable struct TricgWorkspace\{T,FC,Sm,Sn\}.*?\nend", ws_src, flags=re.S).group(0)
    fields = re.findall(r"^\s+(\S+)\s+::\s+(Sm|Sn)\s*$", struct, flags=re.M)
    names = {"y": "y", "N⁻¹uₖ₋₁": "u_prev", "N⁻¹uₖ": "u", "p": "p", "gy₂ₖ₋₁": "gy_prev", "gy₂ₖ": "gy", "x": "x", "M⁻¹vₖ₋₁": "v_prev",
             "M⁻¹vₖ": "v", "q": "q", "gx₂ₖ₋₁": "gx_prev", "gx₂ₖ": "gx", "Δx": "dx", "Δy": "dy"}
    lazy = ("Δx", "Δy", "uₖ", "vₖ")                                       # uₖ and vₖ exist only with N and M
    import krylov_jl_amd as K
    assert tuple(names[f] for f, _ in fields if f not in lazy) == K.TricgWorkspace.VECTORS
    assert tuple(names[f] for f, side in fields if side == "Sm" and f not in lazy) + ("dx",) == K.TricgWorkspace.ROW_SIDE
    assert dict(fields)["Δx"] == "Sm" and dict(fields)["Δy"] == "Sn"


@ref_tree
def test_forwarded_defaults_equal_the_reference():
    """FORWARDED_DEFAULTS["tricg"] = kwargs_tricg / def_kwargs_tricg of src/tricg.jl, names in order, defaults as values."""
    import krylov_jl_amd as K
    src = open(os.path.join(REFERENCE_SRC, "tricg.jl")).read()
    names = re.findall(r":(\w+)", re.search(r"^kwargs_tricg = \((.*?)\)", src, flags=re.M).group(1))
    table = re.search(r"^def_kwargs_tricg = \((.*?)\)\n\n", src, flags=re.M | re.S).group(1)
    defaults = {m.group(1): m.group(2) for m in
                re.finditer(r":\(;\s*(\w+)(?:::[^=]+?)?\s*=\s*(.*?)\s*\)\s*[,)]?\s*$", table, flags=re.M)}
    assert list(defaults) == names
    mine = K.FORWARDED_DEFAULTS["tricg"]
    assert list(mine) == names
    sq = math.sqrt(np.finfo(np.float64).eps)
    value = {"false": False, "true": True, "√eps(T)": sq, "0": 0, "Inf": math.inf, "kstdout": None, "I": None, "one(T)": 1.0,
             "-one(T)": -1.0}
    for k, expr in defaults.items():
        if k == "callback":
            assert expr == "workspace -> false" and mine[k] is K.default_callback
        else:
            assert mine[k] == value[expr] and type(mine[k]) is type(value[expr]), (k, expr, mine[k])
    assert re.search(r"^args_tricg = \(:A, :b, :c\)$", src, flags=re.M) and re.search(r"^optargs_tricg = \(:x0, :y0\)$", src, flags=re.M)


# ---- the Julia specialisation, as text ----------------------------------------------------------------------------------------------
def _julia_tricg():
    glue = open(JULIA_SRC).read()
    m = re.search(r"function Krylov\.tricg!\(ws::TricgWs, A::HIPCsr, b::HIPVector, c::HIPVector;(.*?)\)\n(.*?)\nend\n", glue, flags=re.S)
    assert m, "no specialised Krylov.tricg!"
    return glue, m.group(1), m.group(2)


def test_julia_tricg_specialisation_shape():
    """The Julia tricg! (checked as text: Julia does not run here): the TricgWs alias, the twelve adopted vectors in the order of
    khip_tricg_workspace_adopt, the fallback gate (a log without a descriptor, M or N other than I), the default callback's
    recognition, LAST_PATH, A' taken once, τ, ν and the three flags passed in khip_tricg_params, and test/tricg.jl reached from
    runtests.jl."""
    glue, sig, body = _julia_tricg()
    assert "const TricgWs = TricgWorkspace{Float64,Float64,HIPVector,HIPVector}" in glue
    adopt = re.search(r"ccall\(\(:khip_tricg_workspace_adopt, lib\), Cint, \((.*?)\),\n\s+CTX\[\]\.h, ws\.m, ws\.n, (.*?), r\)\)", glue,
                      flags=re.S)
    assert adopt, "tricg_handle does not adopt the workspace's vectors"
    assert adopt.group(1).count("Ptr{Cdouble}") == 12
    assert [a.strip() for a in adopt.group(2).split(",")] == [f"ws.{f}.ptr" for f in
                                                              ("y", "N⁻¹uₖ₋₁", "N⁻¹uₖ", "p", "gy₂ₖ₋₁", "gy₂ₖ", "x", "M⁻¹vₖ₋₁", "M⁻¹vₖ", "q",
                                                               "gx₂ₖ₋₁", "gx₂ₖ")]
    assert "if !native_log(verbose, iostream) || !(M === I) || !(N === I)" in body
    assert "invoke(Krylov.tricg!, Tuple{TricgWs,Any,AbstractVector{Float64},AbstractVector{Float64}}, ws, A, b, c;" in body
    assert "callback = callback === nothing ? (w -> false) : callback" in body
    assert "NATIVE_SOLVES[] += 1" in body and "LAST_PATH[] = ccall((:khip_tricg_last_path, lib)" in body
    assert "khip_tricg_warm_start" in body and "ws.warm_start = false" in body
    assert "TricgParams(τ, ν, Cint(spd), Cint(snd), Cint(flip))" in body
    assert "st = fill_stats!(ws.stats, " in body
    assert len(re.findall(r"(?<![\w])A'", body)) == 1, "A' is taken once per solve (and cached on the matrix by Base.adjoint)"
    for piece in ("callback = nothing", "fused::Int = 2", "τ::Float64 = 1.0", "ν::Float64 = -1.0", "spd::Bool = false", "snd::Bool = false",
                  "flip::Bool = false", "M = I", "N = I", "ldiv::Bool = false"):
        assert piece in sig, piece
    tests = os.path.join(ROOT, "julia", "KrylovHIP", "test")
    tricg_jl = open(os.path.join(tests, "tricg.jl")).read()
    for piece in ("TricgWorkspace(n, n, S, S)", "native(2) do; tricg!(ws, A_gpu, b, c; history = true); end",
                  "generic(tricg!, ws2, A_gpu, b, c;", "TriCG: system of $(2n) equations in $(2n) variables"):
        assert piece in tricg_jl, piece
    assert 'include("tricg.jl")' in open(os.path.join(tests, "runtests.jl")).read()


@ref_tree
def test_julia_tricg_specialisation():
    """Against the reference tree: every keyword of kwargs_tricg is in the signature, and the glue reads only fields of
    TricgWorkspace (src/krylov_workspaces.jl)."""
    glue, sig, body = _julia_tricg()
    src = open(os.path.join(REFERENCE_SRC, "tricg.jl")).read()
    names = re.findall(r":(\w+)", re.search(r"^kwargs_tricg = \((.*?)\)", src, flags=re.M).group(1))
    for kw in names:
        assert re.search(r"(?<![\w])" + kw + r"(?![\w])", sig), f"tricg!: keyword {kw} of the reference is missing"
    ws_src = open(os.path.join(REFERENCE_SRC, "krylov_workspaces.jl")).read()
    struct = re.search(r"mutable struct TricgWorkspace\{T,FC,Sm,Sn\}.*?\nend", ws_src, flags=re.S).group(0)
    fields = set(re.findall(r"^\s+(\S+)\s+::", struct, flags=re.M))
    used = set(re.findall(r"\bws\.([^\s.,;()\[\]]+)", body))
    handle = re.search(r"function tricg_handle\(ws::TricgWs\)\n(.*?)\nend\n", glue, flags=re.S).group(1)
    used |= set(re.findall(r"\bws\.([^\s.,;()\[\]]+)", handle))
    assert used <= fields, used - fields
    assert {"y", "N⁻¹uₖ₋₁", "N⁻¹uₖ", "p", "gy₂ₖ₋₁", "gy₂ₖ", "x", "M⁻¹vₖ₋₁", "M⁻¹vₖ", "q", "gx₂ₖ₋₁", "gx₂ₖ", "Δx", "Δy"} <= used
