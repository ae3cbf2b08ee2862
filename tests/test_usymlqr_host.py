"""usymlqr! without a GPU: the NumPy restatement (tests/usymlqr_reference.py) against dense solves of [I A; Aᴴ 0] for the three
(ls, ln) settings; the conditions that the GPU tests' case list has to meet; the injected faults that the GPU tests' comparison
rejects; the reference behaviours that are kept (the 0 / 0 r coefficient, the `inconsistent` exit); the Python mirror's tables
against src/usymlqr.jl; and the Julia specialisation's shape (as text: Julia does not run here)."""
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import usymlqr_reference as ur  # noqa: E402
import test_tricg_host as cg_host  # noqa: E402
from test_bilq_host import other_c  # noqa: E402
from test_tricg_host import MEASURE_FLOOR, _vec_dev, deviation, history_excess, nonsymmetric_definite, rect_system, summary  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_SRC = "/root/reference/src"
JULIA_SRC = os.path.join(ROOT, "julia", "KrylovHIP", "src", "KrylovHIP.jl")
ref_tree = pytest.mark.skipif(not os.path.isdir(REFERENCE_SRC), reason="the reference tree is only present in the build container")

TIRED, SOLVED = ur.TIRED, ur.SOLVED
BOTH, LS_ONLY, LN_ONLY = (True, True), (True, False), (False, True)
FLAGS = (BOTH, LS_ONLY, LN_ONLY)                                      # the (ls, ln) every case of the list runs at


# ---- the GPU tests' case list (tests/test_gpu_usymlqr.py imports it) --------------------------------------------------------------
# test_tricg_host.CASES, every one of them with its iteration cap.  name -> (case of test_usymlq_host.CASES, keywords)
CASES = cg_host.CASES
# (niter, status) at (ls, ln) = (true, true), (true, false) and (false, true), pinned from the committed restatement
EXPECTED = {
    "kron4_sinc": ((40, TIRED),) * 3,
    "poisson8": ((36, SOLVED), (30, SOLVED), (36, SOLVED)),
    "poisson16": ((74, SOLVED), (62, SOLVED), (74, SOLVED)),
    "kron7_shift24_sinc": ((28, SOLVED), (28, SOLVED), (26, SOLVED)),
    "kron8_shift24_sinc": ((28, SOLVED),) * 3,
    "kron7_it60": ((60, TIRED),) * 3,
    "kron8_it60": ((60, TIRED),) * 3,
    "kron8_sinc_it60": ((60, TIRED),) * 3,
    "kron9_sinc_it60": ((60, TIRED),) * 3,
    "kron11_sinc_it60": ((60, TIRED),) * 3,
    "kron12_it60": ((60, TIRED),) * 3,
    "kron16_sinc_it30": ((30, TIRED),) * 3,
    "poisson16_sinc_it100": ((100, TIRED),) * 3,
}
# cases in which one side is solved several iterations before the other: name -> (last least-squares iteration, last least-norm one)
STAGGERED = {"poisson8": (30, 36), "poisson16": (62, 74), "kron7_shift24_sinc": (28, 26)}
# itmax of both parities on one case: the rotation of (wₖ₋₂, wₖ₋₁) after a device-resident loop depends on the parity of niter
PARITY_CASE, PARITY_ITMAX = "kron7_it60", (1, 2, 3, 4, 7, 8)
SMALL_SIZES = (1, 2, 3, 63, 64, 65)                                 # nonsymmetric_definite(n) with c = other_c(n)
# niter at the three settings, all solved: the solves end at k = 1, 2, 3 and later, in every stage of P3.  n = 1 with `ls` is the
# 0 / 0 case of test_beta_zero_makes_r_and_x_nan
SMALL_EXPECTED = {1: (2, 1, 2), 2: (2, 2, 2), 3: (4, 3, 4), 63: (10, 9, 10), 64: (10, 9, 10), 65: (10, 9, 10)}
# rect_system(m, n) of tests/test_tricg_host.py.  m < n: the least-squares side only.  m > n: itmax is capped at or below n.  (33, 65)
# and (65, 33) as full solves deviate by more than 1e-6 between the dot modes; they enter under the largest itmax at which the rule
# admits every setting they run at (test_rectangular_caps_are_the_largest_admitted)
RECT_CASES = {(12, 20): (dict(), (LS_ONLY,)), (33, 65): (dict(itmax=10), (LS_ONLY,)), (20, 12): (dict(itmax=12), FLAGS),
              (65, 33): (dict(itmax=11), FLAGS)}
RECT_EXPECTED = {((12, 20), LS_ONLY): (9, SOLVED), ((33, 65), LS_ONLY): (10, TIRED), ((20, 12), BOTH): (10, SOLVED),
                 ((20, 12), LS_ONLY): (9, SOLVED), ((20, 12), LN_ONLY): (10, SOLVED), ((65, 33), BOTH): (11, TIRED),
                 ((65, 33), LS_ONLY): (11, TIRED), ((65, 33), LN_ONLY): (11, TIRED)}


def case_keywords(name, flags=BOTH):
    return dict(CASES[name][1], ls=flags[0], ln=flags[1])


case_system = cg_host.case_system


def dense_pair(A, b, c, **kw):
    A = np.asarray(A, dtype=np.float64)
    return ur.usymlqr(A, b, c, **kw), ur.usymlqr(A, b, c, dot=ur.fsum_dot, **kw)


_PAIRS = {}


def reference_pair(oracle, name, flags=BOTH, **extra):
    """(restatement with np.dot, restatement with exactly summed dots) of a case, as (x, y, stats) triples; computed once."""
    key = (name, flags, tuple(sorted((k, repr(v)) for k, v in extra.items())))
    if key not in _PAIRS:
        S, b, c = case_system(oracle, name)
        St = S.T.tocsr()
        kw = dict(case_keywords(name, flags), **extra)
        _PAIRS[key] = (ur.usymlqr(S, b, c, At=St, **kw), ur.usymlqr(S, b, c, At=St, dot=ur.fsum_dot, **kw))
    return _PAIRS[key]


def _identical(pair):
    (x1, y1, s1), (x2, y2, s2) = pair
    return (summary(s1) == summary(s2) and np.array_equal(x1, x2, equal_nan=True) and np.array_equal(y1, y2, equal_nan=True)
            and np.array_equal(s1.residuals, s2.residuals, equal_nan=True) and np.array_equal(s1.Aresiduals, s2.Aresiduals, equal_nan=True))


def x_deviation(x, x_ref, floor):
    """max|x − x_ref| over max(max|x_ref|, floor).  x = (xᴸ) + r holds the least-squares residual b − A y, which vanishes on a
    consistent system: what is left of it is the rounding of terms of the size of b, so `floor` is max|b₀| (stats.x_floor)."""
    x, x_ref = np.asarray(x), np.asarray(x_ref)
    if not (np.isfinite(x).all() and np.isfinite(x_ref).all()):
        return _vec_dev(x, x_ref)
    return float(np.abs(x - x_ref).max() / max(np.abs(x_ref).max(), floor, np.finfo(float).tiny)) if x_ref.size else 0.0


def own_deviation(pair):
    """A system's own np.dot-versus-exact deviation (the measure of tests/test_tricg_host.py, with the Aresiduals history): on the
    two histories, an entry counting for no less than MEASURE_FLOOR x the first one, on y relative to max|y| and on x relative to
    max(max|x|, max|b₀|).  Two runs that agree in every bit deviate by 0 (n = 1: the history starts with a zero, which the relative
    measure cannot divide by)."""
    if _identical(pair):
        return 0.0
    (x1, y1, s1), (x2, y2, s2) = pair
    own = max(deviation(s1.residuals, s2.residuals, MEASURE_FLOOR), deviation(s1.Aresiduals, s2.Aresiduals, MEASURE_FLOOR))
    if np.isfinite(y1).all() and np.isfinite(y2).all():
        own = max(own, _vec_dev(y1, y2))
    if np.isfinite(x1).all() and np.isfinite(x2).all():
        own = max(own, x_deviation(x1, x2, s2.x_floor))
    return own


def pair_budget(pair):
    """max(1e-8, 10 x own_deviation), the rule of tests/test_tricg_host.py."""
    return max(1e-8, 10.0 * own_deviation(pair))


def admitted(pair):
    """The project's rule: both dot modes agree on niter, status and the flags, and on the histories to <= 1e-6 relative, an entry
    counting for no less than 1e-9 x the first one."""
    (x1, y1, s1), (x2, y2, s2) = pair
    if _identical(pair):
        return True
    return (cg_host.admitted(pair) and (s1.solved_ls, s1.solved_ln) == (s2.solved_ls, s2.solved_ln)
            and deviation(s1.Aresiduals, s2.Aresiduals, MEASURE_FLOOR) <= 1e-6)


def budget(oracle, name, flags=BOTH, **extra):
    return pair_budget(reference_pair(oracle, name, flags, **extra))


def mismatches(got, ref, budget, x=None, x_ref=None, y=None, y_ref=None):
    """What the GPU tests hold a solve to: tests/test_tricg_host.py's list (niter, status, the flags, the history, y), the Aresiduals
    history within `budget`, and x within `budget` of max(max|x|, max|b₀|) (x_deviation)."""
    bad = cg_host.mismatches(got, ref, budget, None, None, y, y_ref)
    d = history_excess(got.Aresiduals, ref.Aresiduals, budget)
    if d > 0.0:
        bad.append(f"Aresiduals deviate by {d:.2e} > {budget:.2e}")
    if x is not None:
        d = x_deviation(x, x_ref, ref.x_floor)
        if not d <= budget:
            bad.append(f"x deviates by {d:.2e} > {budget:.2e}")
    return bad


def role_deviation(got, want, name, floor=0.0):
    """max|got − want| of a named work vector over max|want| (non-finite vectors: equal or not); x and r, which hold the vanishing
    least-squares residual, over max(max|want|, floor) with floor = max|b₀|."""
    return x_deviation(got[name], want[name], floor) if name in ("x", "r") else _vec_dev(got[name], want[name])


def roles_budget(pair, names=ur.VECTORS):
    """The rule of pair_budget carried to the work vectors: max(pair_budget, 10 x the largest deviation of a named vector between the
    restatement's two dot modes)."""
    own = max(role_deviation(pair[0][2].vectors, pair[1][2].vectors, name, pair[1][2].x_floor) for name in names)
    return max(pair_budget(pair), 10.0 * own)


# ---- the case list and its admission rule ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("name", list(CASES))
def test_case_list_condition(oracle, name, flags):
    (x1, y1, s1), (x2, y2, s2) = pair = reference_pair(oracle, name, flags)
    print(f"{name} (ls, ln) = {flags}: {summary(s1)} / {summary(s2)}, own deviation {own_deviation(pair):.1e}, budget {pair_budget(pair):.1e}")
    assert summary(s1) == summary(s2) == EXPECTED[name][FLAGS.index(flags)]
    assert admitted(pair)
    limited = case_keywords(name, flags).get("itmax") == s1.niter                      # ended by itmax
    assert limited == (not s1.solved) and (s1.status == TIRED) == limited and not s1.inconsistent
    assert (len(s1.Aresiduals) > 0) == flags[0]                                        # ‖Aᴴrₖ₋₁‖ belongs to the least-squares side


def test_case_list_has_every_ending(oracle):
    """What the GPU tests rely on the list for, checked and not assumed: a solved and a tired ending, both parities of niter (the
    parity is what fix_after_device_loop gets wrong if it is wrong), an odd n and n = 4096, and the three settings."""
    assert set(EXPECTED) == set(CASES) and set(STAGGERED) <= set(CASES)
    rows = [EXPECTED[name][i] for name in CASES for i in range(len(FLAGS))]
    assert any(r[1] == SOLVED for r in rows) and any(r[1] == TIRED for r in rows)
    sizes = {case_system(oracle, name)[0].shape[0] for name in CASES}
    assert any(n % 2 for n in sizes) and 4096 in sizes and max(sizes) <= 4096
    # every niter of the list is even: the odd parity comes from the runs of PARITY_CASE under PARITY_ITMAX
    assert {r[0] % 2 for r in rows} == {0} and {k % 2 for k in PARITY_ITMAX} == {0, 1} and PARITY_CASE in CASES
    for k in PARITY_ITMAX:
        for flags in FLAGS:
            pair = reference_pair(oracle, PARITY_CASE, flags, itmax=k)
            assert admitted(pair) and summary(pair[0][2]) == (k, TIRED)


@pytest.mark.parametrize("name", list(STAGGERED))
def test_one_side_is_solved_several_iterations_before_the_other(oracle, name):
    """Each history is a prefix that ends with the iteration that solved its side; the interleaved history has one entry per active
    side and iteration, the least-squares entry first."""
    x, y, st = reference_pair(oracle, name, BOTH)[0]
    k_ls, k_ln = STAGGERED[name]
    assert abs(k_ls - k_ln) >= 2 and st.niter == max(k_ls, k_ln) and st.solved
    assert len(st.Aresiduals) == k_ls and len(st.residuals) == k_ls + k_ln
    ls_only = reference_pair(oracle, name, LS_ONLY)[0][2]
    ln_only = reference_pair(oracle, name, LN_ONLY)[0][2]
    both = min(k_ls, k_ln)
    assert np.array_equal(st.residuals[0:2 * both:2], ls_only.residuals[:both])       # the two sides do not see each other
    assert np.array_equal(st.residuals[1:2 * both:2], ln_only.residuals[:both])
    tail = st.residuals[2 * both:]
    assert np.array_equal(tail, (ls_only if k_ls > k_ln else ln_only).residuals[both:])
    assert np.array_equal(st.Aresiduals, ls_only.Aresiduals)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("n", SMALL_SIZES)
def test_small_systems_are_admitted(n, flags):
    M, b = nonsymmetric_definite(n)
    pair = dense_pair(M, b, other_c(n), ls=flags[0], ln=flags[1])
    st = pair[0][2]
    print(f"n = {n} (ls, ln) = {flags}: {summary(st)}, own deviation {own_deviation(pair):.1e}")
    assert admitted(pair) and st.solved and st.niter == SMALL_EXPECTED[n][FLAGS.index(flags)]


def test_small_systems_end_in_every_stage():
    ends = {SMALL_EXPECTED[n][i] for n in SMALL_SIZES for i in range(3)}
    assert {1, 2, 3} <= ends and max(ends) > 3


@pytest.mark.parametrize("shape", list(RECT_CASES))
def test_rectangular_systems_are_admitted(shape):
    A, b, c = rect_system(*shape)
    kw, settings = RECT_CASES[shape]
    assert shape[0] > shape[1] or settings == (LS_ONLY,)                                # m < n: ln = false only
    assert shape[0] < shape[1] or 0 < kw["itmax"] <= shape[1]                           # m > n: itmax capped at or below n
    for flags in settings:
        pair = dense_pair(A, b, c, ls=flags[0], ln=flags[1], **kw)
        st = pair[0][2]
        print(f"{shape} (ls, ln) = {flags}: {summary(st)}, own deviation {own_deviation(pair):.1e}, budget {pair_budget(pair):.1e}")
        assert admitted(pair) and summary(st) == RECT_EXPECTED[(shape, flags)]
        assert len(pair[0][0]) == shape[0] and len(pair[0][1]) == shape[1]


@pytest.mark.parametrize("shape", ((33, 65), (65, 33)))
def test_rectangular_caps_are_the_largest_admitted(shape):
    """(33, 65) and (65, 33): the full solves are not admitted; the cap of RECT_CASES is the largest itmax at which every setting the
    shape runs at is."""
    A, b, c = rect_system(*shape)
    kw, settings = RECT_CASES[shape]
    best = None
    for flags in settings:
        full = dense_pair(A, b, c, ls=flags[0], ln=flags[1])
        ok = [k for k in range(1, full[0][2].niter + 1) if admitted(dense_pair(A, b, c, ls=flags[0], ln=flags[1], itmax=k))]
        print(f"{shape} (ls, ln) = {flags}: full {summary(full[0][2])}, admitted up to itmax = {max(ok)}")
        assert ok == list(range(1, max(ok) + 1)) and max(ok) < full[0][2].niter
        best = max(ok) if best is None else min(best, max(ok))
    assert best == kw["itmax"]


# ---- the restatement against dense solves -----------------------------------------------------------------------------------------
def dense_answer(A, b, c, ls, ln):
    """[x; y] of [I A; Aᴴ 0] [x; y] = [b ls; c ln] by a dense factorisation (A of full column rank)."""
    A = np.asarray(A, dtype=np.float64)
    m, n = A.shape
    K = np.block([[np.eye(m), A], [A.T, np.zeros((n, n))]])
    s = np.linalg.solve(K, np.concatenate([b if ls else np.zeros(m), c if ln else np.zeros(n)]))
    return s[:m], s[m:]


def _known_systems():
    out = {}
    for n in (2, 3, 10, 65):
        M, b = nonsymmetric_definite(n)
        out[f"nsd{n}"] = (M, b, other_c(n))
    A, b, c = rect_system(20, 12)
    out["rect20x12"] = (A, b + np.cos(np.arange(20.0)), c)                              # b is not in the range of A: r ≠ 0
    A, b, c = rect_system(65, 33)
    out["rect65x33"] = (A, b + np.cos(np.arange(65.0)), c)
    return out


KNOWN = _known_systems()


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("name", list(KNOWN))
def test_known_answers(name, flags):
    """x and y against the dense solve, relative to the larger of max|x|, max|y|.  The square systems run at atol = rtol = 1e-13 with
    exactly summed dots and are held to 1e-8: what is left is the conditioning of K, below 1e4 here, times the rounding of the
    recurrences.  The rectangular systems have b outside the range of A, so ‖rₖ‖ of the least-squares side tends to ‖r*‖ > 0 and that
    side ends by the ‖Aᴴrₖ₋₁‖ test (the `inconsistent` exit) at the default tolerances √eps: they are held to 1e-6, the tolerance of
    the reference's own tests at those tolerances."""
    A, b, c = KNOWN[name]
    square = A.shape[0] == A.shape[1]
    kw = dict(atol=1e-13, rtol=1e-13) if square else {}
    x, y, st = ur.usymlqr(A, b, c, ls=flags[0], ln=flags[1], dot=ur.fsum_dot, **kw)
    xs, ys = dense_answer(A, b, c, *flags)
    scale = max(np.abs(xs).max(), np.abs(ys).max())
    ex, ey = np.abs(x - xs).max() / scale, np.abs(y - ys).max() / scale
    print(f"{name} (ls, ln) = {flags}: {summary(st)}, cond {np.linalg.cond(A):.1e}, errors {ex:.1e} {ey:.1e}")
    bound = 1e-8 if square else 1e-6
    assert ex <= bound and ey <= bound
    assert st.solved if (square or not flags[0]) else (st.inconsistent_exit and st.solved_ln and st.status == "unknown")
    assert len(x) == A.shape[0] and len(y) == A.shape[1]


def test_the_two_problems_add_up():
    """(ls, ln) = (true, true) is the sum of the two single problems, to rounding."""
    A, b, c = KNOWN["nsd10"]
    kw = dict(atol=1e-13, rtol=1e-13)
    x, y, _ = ur.usymlqr(A, b, c, **kw)
    x1, y1, _ = ur.usymlqr(A, b, c, ln=False, **kw)
    x2, y2, _ = ur.usymlqr(A, b, c, ls=False, **kw)
    assert np.abs(x - (x1 + x2)).max() <= 1e-10 * np.abs(x).max() and np.abs(y - (y1 + y2)).max() <= 1e-10 * np.abs(y).max()


def test_both_false_is_the_reference_error():
    A, b, c = KNOWN["nsd3"]
    with pytest.raises(ValueError, match=re.escape(ur.BOTH_FALSE)):
        ur.usymlqr(A, b, c, ls=False, ln=False)


@ref_tree
def test_messages_are_the_reference_strings():
    src = open(os.path.join(REFERENCE_SRC, "usymlqr.jl")).read()
    assert f'error("{ur.BOTH_FALSE}")' in src
    assert list(ur.STATUSES[1:]) == re.findall(r"&& \(status = \"([^\"]*)\"\)", src)
    assert "stats.inconsistent = false" in src                                         # always false


def test_callback_and_warm_start_of_the_restatement(oracle):
    S, b, c = case_system(oracle, "kron4_sinc")
    seen = []
    _, _, st = ur.usymlqr(S, b, c, callback=lambda w: (seen.append(len(w.stats.residuals)), len(seen) == 3)[1])
    assert seen == [2, 4, 6] and st.niter == 3 and st.status == "user-requested exit"     # nothing is pushed before iteration 1
    A, b, c = KNOWN["nsd10"]
    x, y, st = ur.usymlqr(A, b, c, x0=np.linspace(-0.5, 0.5, 10), y0=np.linspace(0.25, -0.25, 10), atol=1e-13, rtol=1e-13)
    xs, ys = dense_answer(A, b, c, True, True)
    assert st.solved and np.abs(x - xs).max() <= 1e-8 * np.abs(xs).max() and np.abs(y - ys).max() <= 1e-8 * np.abs(ys).max()


# ---- reference behaviours that are kept -------------------------------------------------------------------------------------------
NAN_SYSTEMS = {"1x1": (np.array([[3.0]]), np.array([2.0]), np.array([5.0])),
               "I3": (np.eye(3), np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0]))}


@pytest.mark.parametrize("name", list(NAN_SYSTEMS))
def test_beta_zero_makes_r_and_x_nan(name):
    """βₖ₊₁ = 0 exactly in an active least-squares step: the r coefficient -cₖ ϕbarₖ₊₁ / βₖ₊₁ is 0 / 0, r and then x are NaN, and the
    solve still ends `solved`; y, the histories and the least-norm side are finite.  With ls = false nothing is NaN."""
    A, b, c = NAN_SYSTEMS[name]
    x, y, st = ur.usymlqr(A, b, c)
    assert st.solved and st.status == SOLVED and not st.inconsistent
    assert np.isnan(st.vectors["r"]).all() and np.isnan(x).all()
    assert np.isfinite(y).all() and np.isfinite(st.residuals).all() and np.isfinite(st.Aresiduals).all()
    assert np.isfinite(st.vectors["z"]).all() and np.isfinite(st.vectors["dbar"]).all()
    x2, y2, st2 = ur.usymlqr(A, b, c, ls=False)
    assert st2.solved and np.isfinite(x2).all() and np.isfinite(y2).all()
    xs, ys = dense_answer(A, b, c, False, True)
    assert np.abs(x2 - xs).max() <= 1e-12 and np.abs(y2 - ys).max() <= 1e-12


def test_inconsistent_exit_leaves_the_status_unknown(oracle):
    """An exit by `inconsistent` (‖Aᴴrₖ₋₁‖ <= κ with the least-squares side unsolved) sets none of the conditions the status lines read:
    the status stays "unknown", solved is false and stats.inconsistent is false.  b ⟂ range(A) does it in one iteration."""
    A = np.array([[1.0, 0.0], [0.0, 1.0], [0.0, 0.0]])
    x, y, st = ur.usymlqr(A, np.array([0.0, 0.0, 1.0]), np.array([1.0, 2.0]))
    assert st.inconsistent_exit and st.status == "unknown" and not st.solved and st.inconsistent is False
    assert st.niter == 1 and not st.solved_ls


# ---- injected faults the comparison rejects ---------------------------------------------------------------------------------------
# every fault runs on poisson8 at (true, true), where the least-squares side is solved six iterations before the other;
# "r_coef_times_reciprocal" moves the last bit of r only: the budgets do not see it, the bitwise comparison of the named vectors
# (path 2 against path 1, and P3 against the NumPy expressions) does
FAULT_CASE = "poisson8"
BITWISE_ONLY = ("r_coef_times_reciprocal",)


@pytest.mark.parametrize("fault", [f for f in ur.FAULTS if f not in BITWISE_ONLY])
def test_comparison_rejects_injected_fault(oracle, fault):
    S, b, c = case_system(oracle, FAULT_CASE)
    St = S.T.tocsr()
    x, y, st = reference_pair(oracle, FAULT_CASE)[0]
    bud = budget(oracle, FAULT_CASE)
    xf, yf, sf = ur.usymlqr(S, b, c, At=St, fault=fault, **case_keywords(FAULT_CASE))
    assert mismatches(st, st, bud, x, x, y, y) == []
    bad = mismatches(sf, st, bud, xf, x, yf, y)
    print(f"{fault} on {FAULT_CASE} (budget {bud:.1e}): {bad}")
    assert bad, f"the comparison does not see {fault}"


@pytest.mark.parametrize("fault", BITWISE_ONLY)
def test_bitwise_comparison_rejects_injected_fault(oracle, fault):
    S, b, c = case_system(oracle, FAULT_CASE)
    St = S.T.tocsr()
    x, y, st = reference_pair(oracle, FAULT_CASE)[0]
    xf, yf, sf = ur.usymlqr(S, b, c, At=St, fault=fault, **case_keywords(FAULT_CASE))
    assert mismatches(sf, st, budget(oracle, FAULT_CASE), xf, x, yf, y) == []           # below every budget
    differ = [k for k in ur.VECTORS if not np.array_equal(st.vectors[k], sf.vectors[k])]
    print(f"{fault}: the named vectors that differ in a bit: {differ}")
    assert "r" in differ


def test_every_fault_is_covered():
    assert set(ur.FAULTS) == {"z_uses_new_w", "dbar_before_x", "frozen_ls_keeps_updating", "w_swap_at_k1", "arnorm_uses_ck",
                              "ln_before_ls_in_history", "r_coef_times_reciprocal"}


# ---- the Python mirror's tables -----------------------------------------------------------------------------------------------------
USYMLQR_SYMBOLS = ("khip_usymlqr_default_params", "khip_usymlqr_workspace_create", "khip_usymlqr_workspace_adopt",
                   "khip_usymlqr_workspace_adopt_vector", "khip_usymlqr_workspace_destroy", "khip_usymlqr_warm_start",
                   "khip_usymlqr_solve", "khip_usymlqr_solution_x", "khip_usymlqr_solution_y", "khip_usymlqr_stats",
                   "khip_usymlqr_aresiduals", "khip_usymlqr_last_path", "khip_usymlqr_vector", "khip_usymlqr_workspace_bytes")


def test_python_mirror_exports_usymlqr():
    """The mirror has the whole USYMLQR surface (fails before the feature: K.usymlqr did not exist)."""
    import krylov_jl_amd as K
    for name in ("usymlqr", "usymlqr_", "UsymlqrWorkspace", "CUsymlqrParams"):
        assert hasattr(K, name), name
    for sym in USYMLQR_SYMBOLS + ("khip_test_usymlqr_p3",):
        assert sym in K.SIGNATURES, sym
        assert hasattr(K.lib(), sym), sym
    header = open(os.path.join(ROOT, "include", "krylov_hip.h")).read()
    assert sorted(set(re.findall(r"\b(khip_usymlqr_[a-z_]+)\s*\(", header))) == sorted(USYMLQR_SYMBOLS)
    assert "khip_test_usymlqr" not in header
    assert "khip_test_usymlqr_p3(" in open(os.path.join(ROOT, "include", "krylov_hip_test.h")).read()
    assert K._INPLACE[K.UsymlqrWorkspace] == ("usymlqr", K.usymlqr_)
    assert "usymlqr" not in K.WORKSPACE_KWARGS
    assert K.UsymlqrWorkspace.VECTORS == ur.VECTORS and K.UsymlqrWorkspace.ROW_SIDE == ur.ROW_SIDE
    assert len(K.SIGNATURES["khip_usymlqr_workspace_adopt"][1]) == 3 + 13 + 1
    assert "runs the primitive sequence" in K.UsymlqrWorkspace.__doc__ and "reports 0" in K.UsymlqrWorkspace.__doc__
    prm = K.lib().khip_usymlqr_default_params()
    assert (prm.ls, prm.ln) == (1, 1)
    assert [f[0] for f in K.CUsymlqrParams._fields_] == ["ls", "ln"]
    assert K.Context.PROFILE_FAMILIES[18] == "usymlqr_p3" and K.Context.PROFILE_FAMILIES[:15] == K.Context.PROFILE_TAGS
    section = header[header.index("---- usymlqr!"):header.index("---- cgs!")]
    for piece in ("complex types", "fused kernels for m != n", "Float32", "6m + 7n doubles"):
        assert piece in section, piece


@ref_tree
def test_workspace_vectors_follow_the_reference_struct():
    ws_src = open(os.path.join(REFERENCE_SRC, "krylov_workspaces.jl")).read()
    struct = re.search(r"mutable struct UsymlqrWorkspace\{T,FC,Sm,Sn\}.*?\nend", ws_src, flags=re.S).group(0)
    fields = re.findall(r"^\s+(\S+)\s+::\s+(Sm|Sn)\s*$", struct, flags=re.M)
    names = {"r": "r", "x": "x", "y": "y", "z": "z", "vₖ₋₁": "v_prev", "vₖ": "v", "uₖ₋₁": "u_prev", "uₖ": "u", "p": "p", "q": "q", "d̅": "dbar",
             "wₖ₋₂": "w_m2", "wₖ₋₁": "w_m1", "Δx": "dx", "Δy": "dy"}
    lazy = ("Δx", "Δy")
    import krylov_jl_amd as K
    assert tuple(names[f] for f, _ in fields if f not in lazy) == K.UsymlqrWorkspace.VECTORS
    assert tuple(names[f] for f, side in fields if side == "Sm" and f not in lazy) + ("dx",) == K.UsymlqrWorkspace.ROW_SIDE
    assert dict(fields)["Δx"] == "Sm" and dict(fields)["Δy"] == "Sn"
    m_side = sum(1 for f, side in fields if side == "Sm" and f not in lazy)
    assert (m_side, len(fields) - 2 - m_side) == (6, 7)                                 # 6m + 7n doubles


@ref_tree
def test_forwarded_defaults_equal_the_reference():
    """FORWARDED_DEFAULTS["usymlqr"] = kwargs_usymlqr / def_kwargs_usymlqr of src/usymlqr.jl, names in order, defaults as values."""
    import krylov_jl_amd as K
    src = open(os.path.join(REFERENCE_SRC, "usymlqr.jl")).read()
    names = re.findall(r":(\w+)", re.search(r"^kwargs_usymlqr = \((.*?)\)", src, flags=re.M).group(1))
    table = re.search(r"^def_kwargs_usymlqr = \((.*?)\)\n\n", src, flags=re.M | re.S).group(1)
    defaults = {m.group(1): m.group(2) for m in
                re.finditer(r":\(;\s*(\w+)(?:::[^=]+?)?\s*=\s*(.*?)\s*\)\s*[,)]?\s*$", table, flags=re.M)}
    assert list(defaults) == names
    mine = K.FORWARDED_DEFAULTS["usymlqr"]
    assert list(mine) == names
    sq = math.sqrt(np.finfo(np.float64).eps)
    value = {"false": False, "true": True, "√eps(T)": sq, "0": 0, "Inf": math.inf, "kstdout": None}
    for k, expr in defaults.items():
        if k == "callback":
            assert expr == "workspace -> false" and mine[k] is K.default_callback
        else:
            assert mine[k] == value[expr] and type(mine[k]) is type(value[expr]), (k, expr, mine[k])
    assert re.search(r"^args_usymlqr = \(:A, :b, :c\)$", src, flags=re.M) and re.search(r"^optargs_usymlqr = \(:x0, :y0\)$", src, flags=re.M)


# ---- the Julia specialisation, as text ----------------------------------------------------------------------------------------------
JULIA_FIELDS = ("r", "x", "y", "z", "vₖ₋₁", "vₖ", "uₖ₋₁", "uₖ", "p", "q", "d̅", "wₖ₋₂", "wₖ₋₁")


def _julia_usymlqr():
    glue = open(JULIA_SRC).read()
    m = re.search(r"function Krylov\.usymlqr!\(ws::UsymlqrWs, A::HIPCsr, b::HIPVector, c::HIPVector;(.*?)\)\n(.*?)\nend\n", glue, flags=re.S)
    assert m, "no specialised Krylov.usymlqr!"
    return glue, m.group(1), m.group(2)


def test_julia_usymlqr_specialisation_shape():
    """The Julia usymlqr! (checked as text: Julia does not run here): the UsymlqrWs alias, the thirteen adopted vectors in the order
    of khip_usymlqr_workspace_adopt, the fallback gate (a log without a descriptor), the default callback's recognition, LAST_PATH,
    A' taken once, ls and ln passed in khip_usymlqr_params, the Aresiduals history, and test/usymlqr.jl, which does its own set-up
    (runtests.jl is not edited)."""
    glue, sig, body = _julia_usymlqr()
    assert "const UsymlqrWs = UsymlqrWorkspace{Float64,Float64,HIPVector,HIPVector}" in glue
    adopt = re.search(r"ccall\(\(:khip_usymlqr_workspace_adopt, lib\), Cint, \((.*?)\),\n\s+CTX\[\]\.h, ws\.m, ws\.n, (.*?), r\)\)", glue,
                      flags=re.S)
    assert adopt, "usymlqr_handle does not adopt the workspace's vectors"
    assert adopt.group(1).count("Ptr{Cdouble}") == 13
    assert [a.strip() for a in adopt.group(2).split(",")] == [f"ws.{f}.ptr" for f in JULIA_FIELDS]
    assert "if !native_log(verbose, iostream)\n" in body
    assert "invoke(Krylov.usymlqr!, Tuple{UsymlqrWs,Any,AbstractVector{Float64},AbstractVector{Float64}}, ws, A, b, c;" in body
    assert "callback = callback === nothing ? (w -> false) : callback" in body
    assert "NATIVE_SOLVES[] += 1" in body and "LAST_PATH[] = ccall((:khip_usymlqr_last_path, lib)" in body
    assert "khip_usymlqr_warm_start" in body and "ws.warm_start = false" in body
    assert "UsymlqrParams(Cint(ls), Cint(ln))" in body
    assert "st = fill_stats!(ws.stats, " in body and "khip_usymlqr_aresiduals" in body and "ws.stats.Aresiduals" in body
    assert ur.BOTH_FALSE in body
    assert len(re.findall(r"(?<![\w])A'", body)) == 1, "A' is taken once per solve (and cached on the matrix by Base.adjoint)"
    for piece in ("callback = nothing", "fused::Int = 2", "ls::Bool = true", "ln::Bool = true", "ldiv::Bool = false"):
        assert piece in sig, piece
    tests = os.path.join(ROOT, "julia", "KrylovHIP", "test")
    usymlqr_jl = open(os.path.join(tests, "usymlqr.jl")).read()
    for piece in ("UsymlqrWorkspace(n, n, S, S)", "native(2) do; usymlqr!(ws, A_gpu, b, c; history = true); end",
                  "generic(usymlqr!, ws2, A_gpu, b, c;", "USYMLQR: system of $(2n) equations in $(2n) variables", "ls = false", "ln = false"):
        assert piece in usymlqr_jl, piece
    assert "using Krylov, KrylovHIP" in usymlqr_jl and "CTX[] = Ctx(0)" in usymlqr_jl, "test/usymlqr.jl does its own set-up"
    assert "usymlqr" not in open(os.path.join(tests, "runtests.jl")).read()


@ref_tree
def test_julia_usymlqr_specialisation():
    """Against the reference tree: every keyword of kwargs_usymlqr is in the signature, and the glue reads only fields of
    UsymlqrWorkspace (src/krylov_workspaces.jl)."""
    glue, sig, body = _julia_usymlqr()
    src = open(os.path.join(REFERENCE_SRC, "usymlqr.jl")).read()
    names = re.findall(r":(\w+)", re.search(r"^kwargs_usymlqr = \((.*?)\)", src, flags=re.M).group(1))
    for kw in names:
        assert re.search(r"(?<![\w])" + kw + r"(?![\w])", sig), f"usymlqr!: keyword {kw} of the reference is missing"
    ws_src = open(os.path.join(REFERENCE_SRC, "krylov_workspaces.jl")).read()
    struct = re.search(r"mutable struct UsymlqrWorkspace\{T,FC,Sm,Sn\}.*?\nend", ws_src, flags=re.S).group(0)
    fields = set(re.findall(r"^\s+(\S+)\s+::", struct, flags=re.M))
    used = set(re.findall(r"\bws\.([^\s.,;()\[\]]+)", body))
    handle = re.search(r"function usymlqr_handle\(ws::UsymlqrWs\)\n(.*?)\nend\n", glue, flags=re.S).group(1)
    used |= set(re.findall(r"\bws\.([^\s.,;()\[\]]+)", handle))
    assert used <= fields, used - fields
    assert set(JULIA_FIELDS) | {"Δx", "Δy"} <= used
