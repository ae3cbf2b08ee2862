"""trimr! without a GPU: the NumPy restatement (tests/trimr_reference.py) against independent answers (the true residual
‖[b; c] − K [xₖ; yₖ]‖ at every k; a non-increasing history; tricg!'s true residual at the same k, which a minimal-residual iterate
cannot exceed; the reference's own known systems); the conditions that the GPU tests' case list has to meet; the injected faults
that the GPU tests' comparison rejects; the Python mirror's tables against src/trimr.jl; and the Julia specialisation's shape (as
text: Julia does not run here)."""
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trimr_reference as tm  # noqa: E402
import tricg_reference as tc  # noqa: E402
import test_tricg_host as cg_host  # noqa: E402
from process_checks import ssy_mo_breakdown2, ssy_mo_breakdown3  # noqa: E402
from test_bilq_host import other_c, rhs  # noqa: E402,F401
from test_tricg_host import (BREAKDOWN_B, BREAKDOWN_C, BREAKDOWNS, MEASURE_FLOOR, _breakdown, _vec_dev, admitted, block_matrix,  # noqa: E402,F401
                             deviation, history_excess, mismatches, nonsymmetric_definite, own_deviation, pair_budget, rect_system,
                             rel_residual, small_sqd, sqd_matrix, summary)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_SRC = "/root/reference/src"
JULIA_SRC = os.path.join(ROOT, "julia", "KrylovHIP", "src", "KrylovHIP.jl")
ref_tree = pytest.mark.skipif(not os.path.isdir(REFERENCE_SRC), reason="the reference tree is only present in the build container")

TIRED, SOLVED, INCONSISTENT = tm.TIRED, tm.SOLVED, tm.INCONSISTENT
SQD, SPD, SP, ADJ = (1.0, -1.0), (1.0, 1.0), (1.0, 0.0), (0.0, 0.0)
PARAMS = (SQD, SPD, SP, ADJ)                                         # the (τ, ν) every case of the list runs at; SP and ADJ are what
#                                                                      tricg! cannot take


# ---- the GPU tests' case list (tests/test_gpu_trimr.py imports it) ----------------------------------------------------------------
# test_tricg_host.CASES, every one of them with its iteration cap.  name -> (case of test_usymlq_host.CASES, keywords)
CASES = cg_host.CASES
# (niter, status) at (1, −1), (1, 1), (1, 0) and (0, 0), pinned from the committed restatement
EXPECTED = {
    "kron4_sinc": ((40, TIRED),) * 4,
    "poisson8": ((26, SOLVED), (21, SOLVED), (32, SOLVED), (30, SOLVED)),
    "poisson16": ((38, SOLVED), (27, SOLVED), (69, SOLVED), (62, SOLVED)),
    "kron7_shift24_sinc": ((28, SOLVED),) * 4,
    "kron8_shift24_sinc": ((28, SOLVED),) * 4,
    "kron7_it60": ((60, TIRED),) * 4,
    "kron8_it60": ((60, TIRED),) * 4,
    "kron8_sinc_it60": ((60, TIRED),) * 4,
    "kron9_sinc_it60": ((60, TIRED),) * 4,
    "kron11_sinc_it60": ((60, TIRED),) * 4,
    "kron12_it60": ((60, TIRED),) * 4,
    "kron16_sinc_it30": ((30, TIRED),) * 4,
    "poisson16_sinc_it100": ((100, TIRED),) * 4,
}
SMALL_SIZES = (1, 2, 3, 63, 64, 65)                                  # nonsymmetric_definite(n) with c = other_c(n), at (1, −1)
SMALL_EXPECTED = {1: 1, 2: 2, 3: 3, 63: 9, 64: 9, 65: 9}             # niter, all solved: n = 1, 2, 3 end in stage 1, 2 and 3 of P3
# rect_system(m, n) of tests/test_tricg_host.py.  (33, 65) as a full solve deviates by more than 1e-6 between the dot modes and enters
# under RECT_ITMAX_33_65, the largest itmax at which the rule admits it (test_rect_33_65_enters_under_its_largest_itmax); (65, 33)
# stays out
RECT_SHAPES = ((12, 20), (20, 12), (33, 65))
RECT_ITMAX_33_65 = 10
RECT_KEYWORDS = {(12, 20): {}, (20, 12): {}, (33, 65): dict(itmax=RECT_ITMAX_33_65)}
RECT_EXPECTED = {(12, 20): (9, SOLVED), (20, 12): (9, SOLVED), (33, 65): (RECT_ITMAX_33_65, TIRED)}


def case_keywords(name, params=SQD):
    return dict(CASES[name][1], tau=params[0], nu=params[1])


case_system = cg_host.case_system


def dense_pair(A, b, c, **kw):
    A = np.asarray(A, dtype=np.float64)
    return tm.trimr(A, b, c, **kw), tm.trimr(A, b, c, dot=tm.fsum_dot, **kw)


_PAIRS = {}


def reference_pair(oracle, name, params=SQD, **extra):
    """(restatement with np.dot, restatement with exactly summed dots) of a case, as (x, y, stats) triples; computed once."""
    key = (name, params, tuple(sorted((k, repr(v)) for k, v in extra.items())))
    if key not in _PAIRS:
        S, b, c = case_system(oracle, name)
        St = S.T.tocsr()
        kw = dict(case_keywords(name, params), **extra)
        _PAIRS[key] = (tm.trimr(S, b, c, At=St, **kw), tm.trimr(S, b, c, At=St, dot=tm.fsum_dot, **kw))
    return _PAIRS[key]


def budget(oracle, name, params=SQD, **extra):
    """pair_budget of a case of the list."""
    return pair_budget(reference_pair(oracle, name, params, **extra))


# ---- the work vectors by name -------------------------------------------------------------------------------------------------------
# A g vector is measured against the largest entry of the four g of its side, not against its own: at τ = −ν the odd-numbered gy
# and the even-numbered gx vanish in exact arithmetic (test_half_of_the_g_is_rounding_noise_when_tau_is_minus_nu) and hold rounding
# noise that no two summation orders share, while x and y take them with coefficients of the size of their neighbours'.
_GX, _GY = ("gx_m3", "gx_m2", "gx_m1", "gx"), ("gy_m3", "gy_m2", "gy_m1", "gy")
ROLE_FAMILY = {name: (_GX if name in _GX else _GY if name in _GY else (name,)) for name in tm.VECTORS}


def role_deviation(got, want, name):
    """max|got − want| of a named work vector over the largest entry of its family in `want`."""
    scale = max([float(np.abs(want[k]).max()) if len(want[k]) else 0.0 for k in ROLE_FAMILY[name]] + [np.finfo(float).tiny])
    a, w = np.asarray(got[name]), np.asarray(want[name])
    if not (np.isfinite(a).all() and np.isfinite(w).all()):
        return 0.0 if np.array_equal(a, w, equal_nan=True) else math.inf
    return float(np.abs(a - w).max() / scale) if w.size else 0.0


def roles_budget(pair, names=tm.VECTORS):
    """The rule of pair_budget carried to the work vectors: max(pair_budget, 10 x the largest deviation of a named vector between the
    restatement's two dot modes).  Near a breakdown vₖ₊₁ and uₖ₊₁ are quotients of rounding errors: their own deviation says so."""
    own = max(role_deviation(pair[0][2].vectors, pair[1][2].vectors, name) for name in names)
    return max(pair_budget(pair), 10.0 * own)


def test_half_of_the_g_is_rounding_noise_when_tau_is_minus_nu(oracle):
    """(1, −1) and (0, 0): gy₂ₖ₋₁ and gx₂ₖ are zero in exact arithmetic; what they hold is below 1e-12 of their side's largest g.  At
    (1, 0) and (1, 1) they are ordinary vectors."""
    S, b, c = case_system(oracle, "kron7_it60")
    for params in PARAMS:
        v = tm.trimr(S, b, c, itmax=6, tau=params[0], nu=params[1])[2].vectors
        noise = max(np.abs(v[k]).max() / max(np.abs(v[f]).max() for f in ROLE_FAMILY[k]) for k in ("gy_m3", "gy_m1", "gx_m2", "gx"))
        print(f"(τ, ν) = {params}: {noise:.1e}")
        assert (noise <= 1e-12) == (params[0] == -params[1])


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
    parity is what fix_after_device_loop gets wrong if it is wrong), an odd n and n = 4096; and the two saddle-point settings."""
    assert set(EXPECTED) == set(CASES)
    rows = [EXPECTED[name][i] for name in CASES for i in range(len(PARAMS))]
    assert any(r[1] == SOLVED for r in rows) and any(r[1] == TIRED for r in rows)
    assert {r[0] % 2 for r in rows if r[1] == SOLVED} == {0, 1} and {r[0] % 2 for r in rows} == {0, 1}
    sizes = {case_system(oracle, name)[0].shape[0] for name in CASES}
    assert any(n % 2 for n in sizes) and 4096 in sizes and max(sizes) <= 4096
    assert (1.0, 0.0) in PARAMS and (0.0, 0.0) in PARAMS
    for name in ("poisson8", "poisson16", "kron7_shift24_sinc", "kron8_shift24_sinc"):
        assert all(r[1] == SOLVED for r in EXPECTED[name]), name


@pytest.mark.parametrize("n", SMALL_SIZES)
def test_small_systems_are_admitted(n):
    M, b = nonsymmetric_definite(n)
    pair = dense_pair(M, b, other_c(n))
    assert admitted(pair) and pair[0][2].solved and pair[0][2].niter == SMALL_EXPECTED[n]


@pytest.mark.parametrize("shape", RECT_SHAPES)
def test_rectangular_systems_are_admitted(shape):
    A, b, c = rect_system(*shape)
    pair = dense_pair(A, b, c, **RECT_KEYWORDS[shape])
    st = pair[0][2]
    print(f"{shape}: {summary(st)}, own deviation {own_deviation(pair):.1e}, budget {pair_budget(pair):.1e}")
    assert admitted(pair) and summary(st) == RECT_EXPECTED[shape]
    assert len(pair[0][0]) == shape[0] and len(pair[0][1]) == shape[1]


def test_rect_33_65_enters_under_its_largest_itmax():
    """(33, 65): the full solve is not admitted; itmax = RECT_ITMAX_33_65 is the largest cap at which it is."""
    A, b, c = rect_system(33, 65)
    full = dense_pair(A, b, c)
    niter = full[0][2].niter
    print(f"(33, 65) full: {summary(full[0][2])}, history deviation {deviation(full[0][2].residuals, full[1][2].residuals, MEASURE_FLOOR):.1e}")
    assert not admitted(full)
    ok = [k for k in range(1, niter + 1) if admitted(dense_pair(A, b, c, itmax=k))]
    assert max(ok) == RECT_ITMAX_33_65 < niter


def test_65_by_33_as_a_full_solve_is_not_admitted():
    A, b, c = rect_system(65, 33)
    pair = dense_pair(A, b, c)
    print(f"(65, 33) full: history deviation {deviation(pair[0][2].residuals, pair[1][2].residuals, MEASURE_FLOOR):.1e}")
    assert not admitted(pair)


# ---- the restatement against independent answers ------------------------------------------------------------------------------------
def true_residual(S, St, b, c, x, y, tau, nu):
    return float(np.linalg.norm(np.concatenate([b - tau * x - S @ y, c - St @ x - nu * y])))


_K_MAX = 19


@pytest.mark.parametrize("params", PARAMS)
@pytest.mark.parametrize("name", list(CASES))
def test_history_is_the_true_residual_and_below_tricg(oracle, name, params):
    """residuals[k] = ‖[b; c] − K [xₖ; yₖ]‖ over the first 19 iterations, with xₖ, yₖ from runs with itmax = k: 1e-10 of the first
    entry.  The history does not increase (an entry may exceed its predecessor by rounding: 1e-12 of the first entry).  Where tricg!
    can run, (τ, ν) = (1, −1) and (1, 1), ‖rₖ‖ is no larger than the TRUE residual of tricg!'s iterate at the same k (both lie in the
    same space and trimr! minimises over it), with the 1e-10 of the first entry by which each side is known."""
    S, b, c = case_system(oracle, name)
    St = S.T.tocsr()
    cap = min(_K_MAX, case_keywords(name).get("itmax", _K_MAX))
    worst = worst_cg = 0.0
    for k in range(1, cap + 1):
        x, y, st = tm.trimr(S, b, c, At=St, tau=params[0], nu=params[1], itmax=k, atol=0.0, rtol=0.0)
        assert st.niter == k
        worst = max(worst, abs(st.residuals[k] - true_residual(S, St, b, c, x, y, *params)) / st.residuals[0])
        assert np.all(np.diff(st.residuals) <= 1e-12 * st.residuals[0])
        if params in (SQD, SPD):
            xc, yc, sc = tc.tricg(S, b, c, At=St, tau=params[0], nu=params[1], itmax=k, atol=0.0, rtol=0.0)
            excess = (st.residuals[k] - true_residual(S, St, b, c, xc, yc, *params)) / st.residuals[0]
            worst_cg = max(worst_cg, excess)
    print(f"{name} (τ, ν) = {params}: {worst:.1e}; above tricg! by {worst_cg:.1e}")
    assert worst <= 1e-10 and worst_cg <= 1e-10


@pytest.mark.parametrize("params", PARAMS)
@pytest.mark.parametrize("name", list(CASES))
def test_whole_history_is_non_increasing(oracle, name, params):
    st = reference_pair(oracle, name, params)[0][2]
    assert np.all(np.diff(st.residuals) <= 1e-12 * st.residuals[0])


KNOWN_PARAMS = ((1.0, -1.0), (1.0, 0.0), (0.0, 0.0), (-1.0, 1.0), (1.0, 1.0), (-1.0, -1.0), (12.0, -0.7), (-1e-6, 1e-8), (0.0, 1.0))


@pytest.mark.parametrize("params", KNOWN_PARAMS)
def test_known_sqd_and_saddle_point_systems(params):
    """sqd(5), saddle_point(5) and adjoint systems (the same A and b) with c = −b, test/test_trimr.jl at its tolerance 1e-6."""
    A, b = sqd_matrix()
    x, y, st = tm.trimr(A, b, -b, tau=params[0], nu=params[1])
    res = rel_residual(A, b, -b, x, y, *params)
    print(f"(τ, ν) = {params}: {summary(st)}, residual {res:.1e}")
    assert res <= 1e-6 and st.solved


def test_flags_equal_their_tau_and_nu():
    A, b = sqd_matrix()
    for flag, params in (("flip", (-1.0, 1.0)), ("spd", (1.0, 1.0)), ("snd", (-1.0, -1.0)), ("sp", (1.0, 0.0))):
        x, y, st = tm.trimr(A, b, -b, tau=3.0, nu=4.0, **{flag: True})
        x2, y2, st2 = tm.trimr(A, b, -b, tau=params[0], nu=params[1])
        assert np.array_equal(x, x2) and np.array_equal(y, y2) and np.array_equal(st.residuals, st2.residuals)
    assert len(tm.PAIR_ERRORS) == 6
    for pair, msg in tm.PAIR_ERRORS.items():
        with pytest.raises(ValueError, match=re.escape(msg)):
            tm.trimr(A, b, -b, **{k: True for k in pair})


@ref_tree
def test_pair_errors_are_the_reference_messages():
    src = open(os.path.join(REFERENCE_SRC, "trimr.jl")).read()
    found = re.findall(r"^\s+(\w+)\s+&&\s+(\w+)\s+&& error\(\"(The matrix cannot be [^\"]*)\"\)$", src, flags=re.M)
    assert {(a, b): msg for a, b, msg in found} == tm.PAIR_ERRORS
    assert [s for s in tm.STATUSES[1:]] == re.findall(r"&& \(status = \"([^\"]*)\"\)", src)


def test_zero_right_hand_sides():
    """b = 0 and c = 0 are ordinary solves (v₁ = 0 or u₁ = 0 by a fill); b = c = 0 starts solved."""
    A, b = sqd_matrix()
    z = np.zeros(5)
    for bb, cc in ((z, -b), (b, z)):
        x, y, st = tm.trimr(A, bb, cc)
        print(f"zero side: {summary(st)}, residual {rel_residual(A, bb, cc, x, y, 1.0, -1.0):.1e}")
        assert rel_residual(A, bb, cc, x, y, 1.0, -1.0) <= 1e-6 and np.isfinite(st.residuals).all()
    x, y, st = tm.trimr(A, z, z)
    assert st.niter == 0 and st.solved and st.status == SOLVED and not x.any() and not y.any() and list(st.residuals) == [0.0]


@pytest.mark.parametrize("transpose", (False, True))
def test_small_sqd(transpose):
    A, b, c = small_sqd(transpose)
    x, y, st = tm.trimr(A, b, c)
    assert rel_residual(A, b, c, x, y, 1.0, -1.0) <= 1e-6 and len(x) == A.shape[0] and len(y) == A.shape[1]


@pytest.mark.parametrize("transpose", (False, True))
def test_breakdown_systems(transpose):
    """ssy_mo_breakdown, both orientations: solved after two iterations at (1, −1); at τ = ν = 1 K is singular and the solve ends
    after two iterations with `inconsistent`, x and y finite."""
    A, b, c = _breakdown(transpose)
    x, y, st = tm.trimr(A, b, c)
    assert summary(st) == (2, SOLVED) and rel_residual(A, b, c, x, y, 1.0, -1.0) <= 1e-6
    assert np.linalg.matrix_rank(block_matrix(A, 1.0, 1.0)) < sum(A.shape)
    x, y, st = tm.trimr(A, b, c, tau=1.0, nu=1.0)
    assert st.inconsistent and not st.solved and summary(st) == (2, INCONSISTENT)
    assert np.isfinite(x).all() and np.isfinite(y).all()


@pytest.mark.parametrize("system", (ssy_mo_breakdown2, ssy_mo_breakdown3))
def test_breakdown_systems_2_and_3(system):
    A, b, c = system()
    x, y, st = tm.trimr(A, b, c)
    assert rel_residual(A, b, c, x, y, 1.0, -1.0) <= 1e-6


@pytest.mark.parametrize("transpose", (False, True))
@pytest.mark.parametrize("name", list(BREAKDOWNS))
def test_breakdown_on_one_side(name, transpose):
    """BREAKDOWNS, transposed or not: solved after one or three iterations."""
    M = BREAKDOWNS[name]
    A, b, c = (M.T.copy(), BREAKDOWN_C, BREAKDOWN_B) if transpose else (M, BREAKDOWN_B, BREAKDOWN_C)
    x, y, st = tm.trimr(A, b, c)
    print(f"{name} transpose={transpose}: {summary(st)}")
    assert st.solved and st.niter in (1, 3) and rel_residual(A, b, c, x, y, 1.0, -1.0) <= 1e-6


def test_roles_after_the_first_iterations(oracle):
    """k = 1: gy₁ and the older pairs keep the zeros of the set-up.  k = 2: the older pair holds (g₁, g₂) of k = 1."""
    S, b, c = case_system(oracle, "kron7_it60")
    v1 = tm.trimr(S, b, c, itmax=1)[2].vectors
    assert not v1["gy_m1"].any() and not any(v1[k].any() for k in ("gx_m3", "gx_m2", "gy_m3", "gy_m2"))
    assert v1["gx_m1"].any() and v1["gx"].any() and v1["gy"].any()
    v2 = tm.trimr(S, b, c, itmax=2)[2].vectors
    for old, new in (("gx_m1", "gx_m3"), ("gx", "gx_m2"), ("gy_m1", "gy_m3"), ("gy", "gy_m2")):
        assert np.array_equal(v1[old], v2[new])
    v3 = tm.trimr(S, b, c, itmax=3)[2].vectors
    for old, new in (("gx_m1", "gx_m3"), ("gx", "gx_m2"), ("gy_m1", "gy_m3"), ("gy", "gy_m2")):
        assert np.array_equal(v2[old], v3[new])


def test_callback_and_warm_start_of_the_restatement(oracle):
    S, b, c = case_system(oracle, "kron4_sinc")
    seen = []
    _, _, st = tm.trimr(S, b, c, callback=lambda w: (seen.append(len(w.stats.residuals)), len(seen) == 3)[1])
    assert seen == [2, 3, 4] and st.niter == 3 and st.status == "user-requested exit"
    n = S.shape[0]
    for params in ((12.0, -0.7), SP):
        x, y, st = tm.trimr(S, b, c, x0=np.linspace(-0.5, 0.5, n), y0=np.linspace(0.25, -0.25, n), tau=params[0], nu=params[1])
        assert st.solved and rel_residual(S, b, c, x, y, *params) <= 1e-6


# ---- injected faults the comparison rejects ---------------------------------------------------------------------------------------
# fault -> (where it shows, (τ, ν)): "guard_ne_zero" needs a βₖ₊₁ or γₖ₊₁ that is tiny but not zero (ssy_mo_breakdown transposed, where the
# process breaks down on one side up to a rounding error).  "g_last_term_old_buffer" cannot show at τ = −ν (the default (1, −1), and
# (0, 0)): there σ₂ₖ₋₁, the coefficient of that last term, is zero in every iteration (test_sigma_odd_vanishes_when_tau_is_minus_nu), so it
# runs at the saddle-point setting.  "mu_shift_at_k1" changes no bit anywhere: see test_mu_shift_at_k1_changes_no_bit.
FAULT_SYSTEMS = {"g_last_term_old_buffer": ("kron4_sinc", SP), "swap_after_update_k2": ("kron4_sinc", SQD),
                 "guard_ne_zero": ("breakdown_transposed", SPD), "pibar_swapped": ("kron4_sinc", SQD),
                 "mu_m4_takes_mu_m3": ("kron4_sinc", SQD), "c1_for_c3": ("kron4_sinc", SQD)}


def _fault_run(oracle, where, params, fault):
    if where == "breakdown_transposed":
        A, b, c = _breakdown(True)
        kw = dict(tau=params[0], nu=params[1])
        pair = dense_pair(A, b, c, **kw)
        return pair[0], tm.trimr(A, b, c, fault=fault, **kw), pair_budget(pair)
    S, b, c = case_system(oracle, where)
    St = S.T.tocsr()
    return (reference_pair(oracle, where, params)[0], tm.trimr(S, b, c, At=St, fault=fault, **case_keywords(where, params)),
            budget(oracle, where, params))


@pytest.mark.parametrize("fault", list(FAULT_SYSTEMS))
def test_comparison_rejects_injected_fault(oracle, fault):
    where, params = FAULT_SYSTEMS[fault]
    (x, y, st), (xf, yf, sf), bud = _fault_run(oracle, where, params, fault)
    assert mismatches(st, st, bud, x, x, y, y) == []
    bad = mismatches(sf, st, bud, xf, x, yf, y)
    print(f"{fault} on {where} at (τ, ν) = {params} (budget {bud:.1e}): {bad}")
    assert bad, f"the comparison does not see {fault}"


@pytest.mark.parametrize("params", (SQD, ADJ))
def test_sigma_odd_vanishes_when_tau_is_minus_nu(oracle, params):
    """At τ = −ν the fault "g_last_term_old_buffer" changes no bit of x and y: the term it corrupts is multiplied by σ₂ₖ₋₁ = 0."""
    S, b, c = case_system(oracle, "kron4_sinc")
    St = S.T.tocsr()
    x, y, st = reference_pair(oracle, "kron4_sinc", params)[0]
    xf, yf, sf = tm.trimr(S, b, c, At=St, fault="g_last_term_old_buffer", **case_keywords("kron4_sinc", params))
    assert np.array_equal(x, xf) and np.array_equal(y, yf)


def test_mu_shift_at_k1_changes_no_bit(oracle):
    """The guard `iter ≥ 2` of the μ / λ shift (:534-538) protects variables that are UNDEFINED at k = 1 in the reference; with them
    initialised (here: zeros) a shift at k = 1 copies zeros onto zeros, and nothing reads the targets before the shift of k = 2
    rewrites them.  The fault is not forced: it changes no bit of x, y, the history or any work vector."""
    assert set(tm.FAULTS) == set(FAULT_SYSTEMS) | {"mu_shift_at_k1"}
    for name in ("kron4_sinc", "poisson8"):
        S, b, c = case_system(oracle, name)
        St = S.T.tocsr()
        x, y, st = reference_pair(oracle, name)[0]
        xf, yf, sf = tm.trimr(S, b, c, At=St, fault="mu_shift_at_k1", **case_keywords(name))
        assert np.array_equal(x, xf) and np.array_equal(y, yf) and np.array_equal(st.residuals, sf.residuals)
        assert all(np.array_equal(st.vectors[k], sf.vectors[k]) for k in tm.VECTORS)


# ---- the Python mirror's tables -----------------------------------------------------------------------------------------------------
TRIMR_SYMBOLS = ("khip_trimr_default_params", "khip_trimr_workspace_create", "khip_trimr_workspace_adopt",
                 "khip_trimr_workspace_adopt_vector", "khip_trimr_workspace_destroy", "khip_trimr_warm_start", "khip_trimr_solve",
                 "khip_trimr_solution_x", "khip_trimr_solution_y", "khip_trimr_stats", "khip_trimr_last_path", "khip_trimr_vector",
                 "khip_trimr_workspace_bytes")


def test_python_mirror_exports_trimr():
    """The mirror has the whole TriMR surface (fails before the feature: K.trimr did not exist)."""
    import krylov_jl_amd as K
    for name in ("trimr", "trimr_", "TrimrWorkspace", "CTrimrParams"):
        assert hasattr(K, name), name
    for sym in TRIMR_SYMBOLS + ("khip_test_trimr_p3", "khip_test_trimr_g"):
        assert sym in K.SIGNATURES, sym
        assert hasattr(K.lib(), sym), sym
    header = open(os.path.join(ROOT, "include", "krylov_hip.h")).read()
    assert sorted(set(re.findall(r"\b(khip_trimr_[a-z_]+)\s*\(", header))) == sorted(TRIMR_SYMBOLS)
    assert "khip_test_trimr" not in header
    test_header = open(os.path.join(ROOT, "include", "krylov_hip_test.h")).read()
    assert "khip_test_trimr_p3(" in test_header and "khip_test_trimr_g(" in test_header
    assert K._INPLACE[K.TrimrWorkspace] == ("trimr", K.trimr_)
    assert "trimr" not in K.WORKSPACE_KWARGS
    assert K.TrimrWorkspace.VECTORS == tm.VECTORS and K.TrimrWorkspace.ROW_SIDE == tm.ROW_SIDE
    assert len(K.SIGNATURES["khip_trimr_workspace_adopt"][1]) == 3 + 16 + 1
    assert "runs the primitive sequence" in K.TrimrWorkspace.__doc__ and "reports 0" in K.TrimrWorkspace.__doc__
    prm = K.lib().khip_trimr_default_params()
    assert (prm.tau, prm.nu, prm.spd, prm.snd, prm.flip, prm.sp) == (1.0, -1.0, 0, 0, 0, 0)
    assert [f[0] for f in K.CTrimrParams._fields_] == ["tau", "nu", "spd", "snd", "flip", "sp"]
    assert K.Context.PROFILE_FAMILIES[17] == "trimr_p3" and K.Context.PROFILE_FAMILIES[:15] == K.Context.PROFILE_TAGS
    for piece in ("M and N other than I", "complex types", "fused kernels for m != n", "Float32"):
        assert piece in header[header.index("---- trimr!"):header.index("---- cgs!")], piece


def test_m_and_n_other_than_i_are_refused_with_error_5():
    import krylov_jl_amd as K
    ws = type("W", (), {"m": 2, "n": 2})()
    b = [0.0, 0.0]
    for kw in (dict(M=object()), dict(N=object())):
        with pytest.raises(K.KhipError) as e:
            K.trimr_(ws, None, b, b, **kw)
        assert "M and N other than I" in str(e.value) and ("-5" in str(e.value) or getattr(e.value, "code", None) == -5)


@ref_tree
def test_workspace_vectors_follow_the_reference_struct():
    ws_src = open(os.path.join(REFERENCE_SRC, "krylov_workspaces.jl")).read()
    struct = re.search(r"mutable struct TrimrWorkspace\{T,FC,Sm,Sn\}.*?\nend", ws_src, flags=re.S).group(0)
    fields = re.findall(r"^\s+(\S+)\s+::\s+(Sm|Sn)\s*$", struct, flags=re.M)
    names = {"y": "y", "N⁻¹uₖ₋₁": "u_prev", "N⁻¹uₖ": "u", "p": "p", "gy₂ₖ₋₃": "gy_m3", "gy₂ₖ₋₂": "gy_m2", "gy₂ₖ₋₁": "gy_m1", "gy₂ₖ": "gy", "x": "x",
             "M⁻¹vₖ₋₁": "v_prev", "M⁻¹vₖ": "v", "q": "q", "gx₂ₖ₋₃": "gx_m3", "gx₂ₖ₋₂": "gx_m2", "gx₂ₖ₋₁": "gx_m1", "gx₂ₖ": "gx", "Δx": "dx",
             "Δy": "dy"}
    lazy = ("Δx", "Δy", "uₖ", "vₖ")                                       # uₖ and vₖ exist only with N and M
    import krylov_jl_amd as K
    assert tuple(names[f] for f, _ in fields if f not in lazy) == K.TrimrWorkspace.VECTORS
    assert tuple(names[f] for f, side in fields if side == "Sm" and f not in lazy) + ("dx",) == K.TrimrWorkspace.ROW_SIDE
    assert dict(fields)["Δx"] == "Sm" and dict(fields)["Δy"] == "Sn"


@ref_tree
def test_forwarded_defaults_equal_the_reference():
    """FORWARDED_DEFAULTS["trimr"] = kwargs_trimr / def_kwargs_trimr of src/trimr.jl, names in order, defaults as values."""
    import krylov_jl_amd as K
    src = open(os.path.join(REFERENCE_SRC, "trimr.jl")).read()
    names = re.findall(r":(\w+)", re.search(r"^kwargs_trimr = \((.*?)\)", src, flags=re.M).group(1))
    table = re.search(r"^def_kwargs_trimr = \((.*?)\)\n\n", src, flags=re.M | re.S).group(1)
    defaults = {m.group(1): m.group(2) for m in
                re.finditer(r":\(;\s*(\w+)(?:::[^=]+?)?\s*=\s*(.*?)\s*\)\s*[,)]?\s*$", table, flags=re.M)}
    assert list(defaults) == names
    mine = K.FORWARDED_DEFAULTS["trimr"]
    assert list(mine) == names
    sq = math.sqrt(np.finfo(np.float64).eps)
    value = {"false": False, "true": True, "√eps(T)": sq, "0": 0, "Inf": math.inf, "kstdout": None, "I": None, "one(T)": 1.0,
             "-one(T)": -1.0}
    for k, expr in defaults.items():
        if k == "callback":
            assert expr == "workspace -> false" and mine[k] is K.default_callback
        else:
            assert mine[k] == value[expr] and type(mine[k]) is type(value[expr]), (k, expr, mine[k])
    assert re.search(r"^args_trimr = \(:A, :b, :c\)$", src, flags=re.M) and re.search(r"^optargs_trimr = \(:x0, :y0\)$", src, flags=re.M)


# ---- the Julia specialisation, as text ----------------------------------------------------------------------------------------------
JULIA_FIELDS = ("y", "N⁻¹uₖ₋₁", "N⁻¹uₖ", "p", "gy₂ₖ₋₃", "gy₂ₖ₋₂", "gy₂ₖ₋₁", "gy₂ₖ", "x", "M⁻¹vₖ₋₁", "M⁻¹vₖ", "q", "gx₂ₖ₋₃", "gx₂ₖ₋₂", "gx₂ₖ₋₁", "gx₂ₖ")


def _julia_trimr():
    glue = open(JULIA_SRC).read()
    m = re.search(r"function Krylov\.trimr!\(ws::TrimrWs, A::HIPCsr, b::HIPVector, c::HIPVector;(.*?)\)\n(.*?)\nend\n", glue, flags=re.S)
    assert m, "no specialised Krylov.trimr!"
    return glue, m.group(1), m.group(2)


def test_julia_trimr_specialisation_shape():
    """The Julia trimr! (checked as text: Julia does not run here): the TrimrWs alias, the sixteen adopted vectors in the order of
    khip_trimr_workspace_adopt, the fallback gate (a log without a descriptor, M or N other than I), the default callback's
    recognition, LAST_PATH, A' taken once, τ, ν and the four flags passed in khip_trimr_params, and test/trimr.jl, which does its own
    set-up (runtests.jl is not edited)."""
    glue, sig, body = _julia_trimr()
    assert "const TrimrWs = TrimrWorkspace{Float64,Float64,HIPVector,HIPVector}" in glue
    adopt = re.search(r"ccall\(\(:khip_trimr_workspace_adopt, lib\), Cint, \((.*?)\),\n\s+CTX\[\]\.h, ws\.m, ws\.n, (.*?), r\)\)", glue,
                      flags=re.S)
    assert adopt, "trimr_handle does not adopt the workspace's vectors"
    assert adopt.group(1).count("Ptr{Cdouble}") == 16
    assert [a.strip() for a in adopt.group(2).split(",")] == [f"ws.{f}.ptr" for f in JULIA_FIELDS]
    assert "if !native_log(verbose, iostream) || !(M === I) || !(N === I)" in body
    assert "invoke(Krylov.trimr!, Tuple{TrimrWs,Any,AbstractVector{Float64},AbstractVector{Float64}}, ws, A, b, c;" in body
    assert "callback = callback === nothing ? (w -> false) : callback" in body
    assert "NATIVE_SOLVES[] += 1" in body and "LAST_PATH[] = ccall((:khip_trimr_last_path, lib)" in body
    assert "khip_trimr_warm_start" in body and "ws.warm_start = false" in body
    assert "TrimrParams(τ, ν, Cint(spd), Cint(snd), Cint(flip), Cint(sp))" in body
    assert "st = fill_stats!(ws.stats, " in body
    assert not re.search(r"^\s*sp\s*=", body, flags=re.M), "`sp` is the saddle-point keyword: the stats pointer needs another name"
    assert len(re.findall(r"(?<![\w])A'", body)) == 1, "A' is taken once per solve (and cached on the matrix by Base.adjoint)"
    for piece in ("callback = nothing", "fused::Int = 2", "τ::Float64 = 1.0", "ν::Float64 = -1.0", "spd::Bool = false", "snd::Bool = false",
                  "flip::Bool = false", "sp::Bool = false", "M = I", "N = I", "ldiv::Bool = false"):
        assert piece in sig, piece
    tests = os.path.join(ROOT, "julia", "KrylovHIP", "test")
    trimr_jl = open(os.path.join(tests, "trimr.jl")).read()
    for piece in ("TrimrWorkspace(n, n, S, S)", "native(2) do; trimr!(ws, A_gpu, b, c; history = true); end",
                  "generic(trimr!, ws2, A_gpu, b, c;", "TriMR: system of $(2n) equations in $(2n) variables", "sp = true"):
        assert piece in trimr_jl, piece
    assert "using Krylov, KrylovHIP" in trimr_jl and "CTX[] = Ctx(0)" in trimr_jl, "test/trimr.jl does its own set-up"


@ref_tree
def test_julia_trimr_specialisation():
    """Against the reference tree: every keyword of kwargs_trimr is in the signature, and the glue reads only fields of
    TrimrWorkspace (src/krylov_workspaces.jl)."""
    glue, sig, body = _julia_trimr()
    src = open(os.path.join(REFERENCE_SRC, "trimr.jl")).read()
    names = re.findall(r":(\w+)", re.search(r"^kwargs_trimr = \((.*?)\)", src, flags=re.M).group(1))
    for kw in names:
        assert re.search(r"(?<![\w])" + kw + r"(?![\w])", sig), f"trimr!: keyword {kw} of the reference is missing"
    ws_src = open(os.path.join(REFERENCE_SRC, "krylov_workspaces.jl")).read()
    struct = re.search(r"mutable struct TrimrWorkspace\{T,FC,Sm,Sn\}.*?\nend", ws_src, flags=re.S).group(0)
    fields = set(re.findall(r"^\s+(\S+)\s+::", struct, flags=re.M))
    used = set(re.findall(r"\bws\.([^\s.,;()\[\]]+)", body))
    handle = re.search(r"function trimr_handle\(ws::TrimrWs\)\n(.*?)\nend\n", glue, flags=re.S).group(1)
    used |= set(re.findall(r"\bws\.([^\s.,;()\[\]]+)", handle))
    assert used <= fields, used - fields
    assert set(JULIA_FIELDS) | {"Δx", "Δy"} <= used
