"""trilqr! without a GPU: the NumPy restatement (tests/trilqr_reference.py) against independent answers (the restatement of usymlq!
on (A, b, c), entry for entry while the primal side is unsolved; the restatement of usymqr! on (Aᵀ, c, b); the true residuals
‖b − A xₖ‖ and ‖c − Aᵀ tₖ₋₁‖; the reference's own known adjoint systems); the conditions that the GPU tests' case list has to
meet; the injected faults that the GPU tests' comparison rejects; the Python mirror's tables against src/trilqr.jl; and the Julia
specialisation's shape (as text: Julia does not run here)."""
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trilqr_reference as tr  # noqa: E402
import usymlq_reference as ul  # noqa: E402
import usymqr_reference as uq  # noqa: E402
import test_usymlq_host as lq_host  # noqa: E402
from test_bilq_host import other_c  # noqa: E402
from test_usymqr_host import (BREAKDOWN_B, BREAKDOWN_C, BREAKDOWNS, MEASURE_FLOOR, deviation, history_excess,  # noqa: E402,F401
                              nonsymmetric_definite)
from test_usymlq_host import UNSYM_BREAKDOWN  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_SRC = "/root/reference/src"
JULIA_SRC = os.path.join(ROOT, "julia", "KrylovHIP", "src", "KrylovHIP.jl")
ref_tree = pytest.mark.skipif(not os.path.isdir(REFERENCE_SRC), reason="the reference tree is only present in the build container")

TIRED, BOTH_L, BOTH_C, ONLY_T = tr.TIRED, tr.BOTH_L, tr.BOTH_C, tr.ONLY_T


# ---- the GPU tests' case list (tests/test_gpu_trilqr.py imports it) ---------------------------------------------------------------
# test_usymlq_host.CASES, every one of them, and two more on its poisson operators with an itmax that ends the solve an EVEN
# number of iterations after the dual side did (transfer off: poisson8 ends its dual side at 31 and its primal side at 36,
# poisson16 at 63 and 74, both odd gaps).  name -> (case of test_usymlq_host.CASES, keywords added with the transfer on, ... off).
# kron4_sinc with the transfer on is a full solve of 54 iterations whose dual history deviates by 1.0e-4 between the dot modes
# (n = 64: the process has lost its orthogonality by then): it enters with the itmax = 40 it has with the transfer off.
CASES = {name: (name, {}, {}) for name in lq_host.CASES}
CASES["kron4_sinc"] = ("kron4_sinc", dict(itmax=40), {})
CASES["poisson8_it35"] = ("poisson8", dict(itmax=35), dict(itmax=35))
CASES["poisson16_it71"] = ("poisson16", dict(itmax=71), dict(itmax=71))
TRANSFERS = (True, False)
# (niter, status, nprimal, ndual) with the transfer on and off, pinned from the committed restatement; nprimal / ndual: the last
# iteration in which the primal / dual block ran (the histories have one entry more)
EXPECTED = {
    "kron4_sinc": ((40, TIRED, 40, 40), (40, TIRED, 40, 40)),
    "poisson8": ((31, BOTH_C, 30, 31), (36, BOTH_L, 36, 31)),
    "poisson16": ((63, BOTH_C, 63, 63), (74, BOTH_L, 74, 63)),
    "kron7_shift24_sinc": ((28, BOTH_C, 28, 27), (28, BOTH_L, 28, 27)),
    "kron8_shift24_sinc": ((30, BOTH_C, 30, 29), (30, BOTH_L, 30, 29)),
    "kron7_it60": ((60, TIRED, 60, 60), (60, TIRED, 60, 60)),
    "kron8_it60": ((60, TIRED, 60, 60), (60, TIRED, 60, 60)),
    "kron8_sinc_it60": ((60, TIRED, 60, 60), (60, TIRED, 60, 60)),
    "kron9_sinc_it60": ((60, TIRED, 60, 60), (60, TIRED, 60, 60)),
    "kron11_sinc_it60": ((60, TIRED, 60, 60), (60, TIRED, 60, 60)),
    "kron12_it60": ((60, TIRED, 60, 60), (60, TIRED, 60, 60)),
    "kron16_sinc_it30": ((30, TIRED, 30, 30), (30, TIRED, 30, 30)),
    "poisson16_sinc_it100": ((100, TIRED, 100, 100), (100, TIRED, 100, 100)),
    "poisson8_it35": ((31, BOTH_C, 30, 31), (35, ONLY_T, 35, 31)),
    "poisson16_it71": ((63, BOTH_C, 63, 63), (71, ONLY_T, 71, 63)),
}
SMALL_SIZES = (1, 2, 63, 64, 65)                                     # nonsymmetric_definite(n) with c = other_c(n)


def case_keywords(name, transfer):
    base, on, off = CASES[name]
    return dict(lq_host.case_keywords(base, transfer), **(on if transfer else off))


def case_system(oracle, name):
    """(A as scipy CSR, b, c) of a case of the list."""
    return lq_host.case_system(oracle, CASES[name][0])


def _vec_dev(a, ref):
    a, ref = np.asarray(a), np.asarray(ref)
    if not np.isfinite(ref).all():
        return 0.0 if np.array_equal(np.isnan(a), np.isnan(ref)) else math.inf
    if not np.isfinite(a).all():
        return math.inf
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), np.finfo(float).tiny)) if ref.size else 0.0


def mismatches(got, ref, budget, x=None, x_ref=None, t=None, t_ref=None):
    """What the GPU tests hold a solve to, as the list of what differs: niter, status, the three flags, both histories within
    `budget` of each entry plus the absolute floor 1e-12 x the first entry and, where given, x and t within `budget` of max|x| and
    max|t|."""
    bad = []
    if got.niter != ref.niter:
        bad.append(f"niter {got.niter} != {ref.niter}")
    if got.status != ref.status:
        bad.append(f"status {got.status!r} != {ref.status!r}")
    flags = lambda s: (bool(s.solved_primal), bool(s.solved_dual), bool(s.inconsistent))  # noqa: E731
    if flags(got) != flags(ref):
        bad.append(f"flags {flags(got)} != {flags(ref)}")
    for name in ("residuals_primal", "residuals_dual"):
        d = history_excess(getattr(got, name), getattr(ref, name), budget)
        if d > 0.0:
            bad.append(f"{name} deviate by {d:.2e} > {budget:.2e}")
    for name, a, r in (("x", x, x_ref), ("t", t, t_ref)):
        if a is not None:
            d = _vec_dev(a, r)
            if not d <= budget:
                bad.append(f"{name} deviates by {d:.2e} > {budget:.2e}")
    return bad


def own_deviation(pair):
    """A system's own np.dot-versus-exact deviation: on both histories, an entry counting for no less than MEASURE_FLOOR x the
    first one, and on x and t relative to max|x| and max|t|."""
    (x1, t1, s1), (x2, t2, s2) = pair
    own = max(deviation(s1.residuals_primal, s2.residuals_primal, MEASURE_FLOOR),
              deviation(s1.residuals_dual, s2.residuals_dual, MEASURE_FLOOR))
    for a, r in ((x1, x2), (t1, t2)):
        if np.isfinite(a).all() and np.isfinite(r).all():
            own = max(own, _vec_dev(a, r))
    return own


def pair_budget(pair):
    """max(1e-8, 10 x own_deviation): the library's dots are as far from the exact ones as np.dot's are, in another order, and ten
    of those distances bound what the recurrences make of them (the rule of tests/test_usymlq_host.py)."""
    return max(1e-8, 10.0 * own_deviation(pair))


def dense_pair(A, b, c, **kw):
    A = np.asarray(A, dtype=np.float64)
    return tr.trilqr(A, b, c, **kw), tr.trilqr(A, b, c, dot=tr.fsum_dot, **kw)


_PAIRS = {}


def reference_pair(oracle, name, transfer=True, **extra):
    """(restatement with np.dot, restatement with exactly summed dots) of a case, as (x, t, stats) triples; computed once."""
    key = (name, transfer, tuple(sorted((k, repr(v)) for k, v in extra.items())))
    if key not in _PAIRS:
        S, b, c = case_system(oracle, name)
        St = S.T.tocsr()
        kw = dict(case_keywords(name, transfer), **extra)
        _PAIRS[key] = (tr.trilqr(S, b, c, At=St, **kw), tr.trilqr(S, b, c, At=St, dot=tr.fsum_dot, **kw))
    return _PAIRS[key]


def budget(oracle, name, transfer=True, **extra):
    """pair_budget of a case of the list."""
    return pair_budget(reference_pair(oracle, name, transfer, **extra))


def summary(st):
    return (st.niter, st.status, len(st.residuals_primal) - 1, len(st.residuals_dual) - 1)


@pytest.mark.parametrize("transfer", TRANSFERS)
@pytest.mark.parametrize("name", list(CASES))
def test_case_list_condition(oracle, name, transfer):
    """A case may be in the list only if the restatement with np.dot and with math.fsum dots agree on niter, status, the flags and
    the lengths of both histories, and on both histories to <= 1e-6 relative, an entry counting for no less than 1e-9 x the first
    one."""
    (x1, t1, s1), (x2, t2, s2) = pair = reference_pair(oracle, name, transfer)
    dp = deviation(s1.residuals_primal, s2.residuals_primal, MEASURE_FLOOR)
    dd = deviation(s1.residuals_dual, s2.residuals_dual, MEASURE_FLOOR)
    print(f"{name} transfer={transfer}: {summary(s1)} / {summary(s2)}, deviation {dp:.1e} (primal) {dd:.1e} (dual) "
          f"{own_deviation(pair):.1e} (with x, t), budget {pair_budget(pair):.1e}")
    assert summary(s1) == summary(s2) == EXPECTED[name][0 if transfer else 1]
    assert (s1.solved_primal, s1.solved_dual, s1.inconsistent) == (s2.solved_primal, s2.solved_dual, s2.inconsistent)
    limited = case_keywords(name, transfer).get("itmax") == s1.niter                  # ended by itmax: not both sides solved
    assert limited == (not (s1.solved_primal and s1.solved_dual)) and (s1.status in (TIRED, ONLY_T)) == limited
    assert not (s1.solved_cg and not transfer)
    assert dp <= 1e-6 and dd <= 1e-6


def test_case_list_has_every_ending():
    """What the GPU tests rely on the list for, checked and not assumed: a primal side that ends first and a dual side that ends
    first; among the latter, gaps niter − ndual of both parities with ndual ≥ 3 (the parity is what fix_after_device_loop gets
    wrong if it is wrong); both sides ending in the same iteration; a tired case; the transfer off."""
    assert set(EXPECTED) == set(CASES) and set(lq_host.CASES) <= set(CASES)
    rows = [(name, tf) + EXPECTED[name][0 if tf else 1] for name in CASES for tf in TRANSFERS]
    primal_first = [r for r in rows if r[4] < r[5]]
    dual_first = [r for r in rows if r[5] < r[4]]
    assert primal_first and dual_first
    gaps = {(r[2] - r[5]) % 2 for r in dual_first if r[5] >= 3}
    assert gaps == {0, 1}, gaps
    assert any(r[4] == r[5] == r[2] and r[3] != TIRED for r in rows), "no case ends both sides in the same iteration"
    assert any(r[3] == TIRED for r in rows)
    assert any(r[3] == ONLY_T and r[5] < r[2] for r in rows), "no case ends at itmax with only the dual side solved"
    assert any(not r[1] and r[3] == BOTH_L for r in rows)


@pytest.mark.parametrize("transfer", TRANSFERS)
@pytest.mark.parametrize("n", SMALL_SIZES)
def test_small_systems_are_admitted(n, transfer):
    M, b = nonsymmetric_definite(n)
    (x1, t1, s1), (x2, t2, s2) = dense_pair(M, b, other_c(n), transfer_to_usymcg=transfer)
    assert summary(s1) == summary(s2) and s1.solved_primal and s1.solved_dual
    assert deviation(s1.residuals_primal, s2.residuals_primal, MEASURE_FLOOR) <= 1e-6
    assert deviation(s1.residuals_dual, s2.residuals_dual, MEASURE_FLOOR) <= 1e-6


# ---- the restatement against independent answers ------------------------------------------------------------------------------------
@pytest.mark.parametrize("transfer", TRANSFERS)
@pytest.mark.parametrize("name", list(CASES))
def test_primal_side_is_usymlq_entry_for_entry(oracle, name, transfer):
    """Until the primal side is solved, its history and x are usymlq!'s on (A, b, c): the same expressions, np.array_equal.  The
    restatement of usymlq! tests `rNorm ≤ ε` alone and trilqr! `rNorm + 1 ≤ 1` as well, which no case of the list reaches."""
    S, b, c = case_system(oracle, name)
    St = S.T.tocsr()
    kw = case_keywords(name, transfer)
    x, t, st = reference_pair(oracle, name, transfer)[0]
    nprimal = len(st.residuals_primal) - 1
    xl, sl = ul.usymlq(S, b, c, At=St, **dict(kw, itmax=nprimal))
    assert sl.niter == nprimal
    assert np.array_equal(sl.residuals, st.residuals_primal)
    assert np.array_equal(xl, x) and np.array_equal(sl.vectors["dbar"], st.vectors["dbar"])
    assert (sl.solved_lq, sl.solved_cg) == (st.solved_lq, st.solved_cg)


@pytest.mark.parametrize("name", list(CASES))
def test_dual_side_is_usymqr(oracle, name):
    """The dual history is usymqr!'s on (Aᵀ, c, b), one place later: iteration k of trilqr! pushes ‖sₖ₋₁‖ = |ψbarₖ| (:374), so its
    history is (‖s₀‖, ‖s₀‖, ‖s₁‖, …).  The two use different recurrences (the LQ factorisation of Tₖ here, the QR factorisation of
    its transpose there) that are equal in exact arithmetic: the budget is budget()'s rule, on the larger of the two solvers' own
    np.dot-against-exact deviations, and a case enters only if that is ≤ 1e-6."""
    S, b, c = case_system(oracle, name)
    St = S.T.tocsr()
    (x, t, st), (x2, t2, st2) = reference_pair(oracle, name, True)
    nd = len(st.residuals_dual) - 1
    (xq, sq), (xq2, sq2) = (uq.usymqr(St, c, b, At=S, itmax=nd - 1), uq.usymqr(St, c, b, At=S, itmax=nd - 1, dot=uq.fsum_dot))
    own = max(deviation(st.residuals_dual, st2.residuals_dual, MEASURE_FLOOR), deviation(sq.residuals, sq2.residuals, MEASURE_FLOOR))
    assert own <= 1e-6, f"{name}: own deviation {own:.1e} > 1e-6, the case should not be in the list"
    bud = max(1e-8, 10.0 * own)
    assert st.residuals_dual[1] == st.residuals_dual[0]
    k = min(len(sq.residuals), nd)
    d = history_excess(st.residuals_dual[1:1 + k], sq.residuals[:k], bud)
    print(f"{name}: {k} entries, own deviation {own:.1e}, budget {bud:.1e}, excess {d:.1e}")
    assert k >= nd - 1 and d == 0.0


@pytest.mark.parametrize("name", ["kron4_sinc", "poisson8", "kron7_shift24_sinc", "kron16_sinc_it30"])
def test_histories_are_the_true_residuals(oracle, name):
    """With the transfer off, residuals_primal[k] = ‖b − A xₖ‖ and residuals_dual[k] = ‖c − Aᵀ t‖ for the t that k iterations leave
    (tₖ₋₁), over the first 20 iterations, from runs with itmax = k; 1e-10 relative to each history's first entry."""
    S, b, c = case_system(oracle, name)
    St = S.T.tocsr()
    worst_p = worst_d = 0.0
    for k in range(1, 20):
        x, t, st = tr.trilqr(S, b, c, At=St, itmax=k, transfer_to_usymcg=False)
        assert st.niter == k
        worst_p = max(worst_p, abs(st.residuals_primal[k] - np.linalg.norm(b - S @ x)) / st.residuals_primal[0])
        worst_d = max(worst_d, abs(st.residuals_dual[k] - np.linalg.norm(c - St @ t)) / st.residuals_dual[0])
    print(f"{name}: primal {worst_p:.1e}, dual {worst_d:.1e}")
    assert worst_p <= 1e-10 and worst_d <= 1e-10


# test/test_utils.jl's adjoint systems, restated as data.  adjoint_ode and adjoint_pde are LEFT OUT: they discretise a
# differential operator with the reference's own finite-difference helpers, which are program text and not data.
def _sign_matrix(rows, cols):
    i = np.arange(rows)[:, None]
    j = np.arange(cols)[None, :]
    return np.where(i == j, 10.0, np.where(i < j, 1.0, -1.0))


def adjoint_system(name):
    if name == "square_adjoint":
        A = _sign_matrix(100, 100)
    elif name == "underdetermined_adjoint":
        A = _sign_matrix(100, 200)
    elif name == "overdetermined_adjoint":
        A = _sign_matrix(200, 100)
    elif name == "rectangular_adjoint":                 # A x = b underdetermined consistent, Aᴴ t = c overdetermined inconsistent
        A = np.ones((10, 25))
        c = np.arange(1.0, 26.0)
        c[0] = -1.0
        return A, A @ np.ones(25), c
    else:
        raise KeyError(name)
    m, n = A.shape
    return A, A @ np.arange(1.0, n + 1), A.T @ np.arange(-float(m), 0.0)


ADJOINT_SYSTEMS = ("square_adjoint", "underdetermined_adjoint", "overdetermined_adjoint", "rectangular_adjoint")


@pytest.mark.parametrize("name", ADJOINT_SYSTEMS)
def test_known_adjoint_systems(name):
    """test/test_trilqr.jl at its tolerance 1e-6: both relative residuals and both flags; on rectangular_adjoint the dual system
    is inconsistent and the test is ‖A s‖ / ‖A c‖ with s = c − Aᴴ t."""
    A, b, c = adjoint_system(name)
    x, t, st = tr.trilqr(A, b, c)
    assert np.linalg.norm(b - A @ x) <= 1e-6 * np.linalg.norm(b)
    assert st.solved_primal and st.solved_dual
    s = c - A.T @ t
    if name == "rectangular_adjoint":
        assert np.linalg.norm(A @ s) <= 1e-6 * np.linalg.norm(A @ c)
        assert st.inconsistent
    else:
        assert np.linalg.norm(s) <= 1e-6 * np.linalg.norm(c)
    print(f"{name}: {summary(st)}, inconsistent = {st.inconsistent}")


def test_unsymmetric_breakdown():
    A, b, c = UNSYM_BREAKDOWN
    x, t, st = tr.trilqr(A, b, c)
    assert np.isfinite(x).all() and np.isfinite(t).all() and st.solved_primal and st.solved_dual
    assert np.linalg.norm(b - A @ x) <= 1e-6 and np.linalg.norm(c - A.T @ t) <= 1e-6


def test_zero_right_hand_sides_do_not_return_early():
    """b = 0: the primal side starts solved and v₁ = 0 / 0; the loop still runs for the dual side (no early return, :190-202).
    b = c = 0: the loop never starts."""
    A = np.eye(4) * 2.0
    x, t, st = tr.trilqr(A, np.zeros(4), np.ones(4), itmax=3)
    assert st.niter == 3 and st.solved_primal and not x.any() and list(st.residuals_primal) == [0.0]
    assert np.isnan(st.vectors["v"]).all()
    x, t, st = tr.trilqr(A, np.ones(4), np.zeros(4), itmax=3)
    assert st.niter == 3 and st.solved_dual and not t.any() and list(st.residuals_dual) == [0.0]
    x, t, st = tr.trilqr(A, np.zeros(4), np.zeros(4))
    assert st.niter == 0 and st.solved_primal and st.solved_dual and st.status == "unknown"


def test_status_can_stay_unknown_when_the_dual_side_ends_by_inconsistent_alone():
    """rectangular_adjoint (A has rank 1): the primal side ends at k = 1 by the USYMCG point, whose residual estimate is below
    machine precision, the dual side at k = 2 by `inconsistent` alone.  The reference's strings read solved_qr_tol and
    solved_qr_mach, never `inconsistent`, and the primal-only strings require an UNSOLVED dual side: none applies, and the status
    stays "unknown" with both flags set (src/trilqr.jl:430-446)."""
    A, b, c = adjoint_system("rectangular_adjoint")
    x, t, st = tr.trilqr(A, b, c)
    assert st.inconsistent and st.solved_dual and st.solved_primal
    assert summary(st) == (2, "unknown", 1, 2)


def test_roles_after_the_first_iterations(oracle):
    """w_prev2 / w_prev3 after k iterations are wₖ₋₁ / wₖ₋₂, the last two columns of Wₖ₋₁ = Vₖ₋₁ Lₖ₋₁⁻ᵀ: t = Σ ψⱼ wⱼ solves the dual
    system in the least-squares sense over span(v₁ … vₖ₋₁)."""
    S, b, c = case_system(oracle, "kron4_sinc")
    prev_t = None
    for k in (1, 2, 3, 4, 5):
        x, t, st = tr.trilqr(S, b, c, itmax=k, transfer_to_usymcg=False)
        v = st.vectors
        if k == 1:
            assert not t.any() and not v["w_prev2"].any() and not v["w_prev3"].any()
            assert np.array_equal(v["dbar"], v["u_prev"])
        else:
            step = t - prev_t                                            # ψₖ₋₁ wₖ₋₁
            w = v["w_prev2"]
            coef = float(step @ w) / float(w @ w)
            assert np.linalg.norm(step - coef * w) <= 1e-12 * np.linalg.norm(step)
        prev_t = t


def test_callback_and_warm_start_of_the_restatement(oracle):
    S, b, c = case_system(oracle, "kron4_sinc")
    seen = []
    _, _, st = tr.trilqr(S, b, c, callback=lambda w: (seen.append((len(w.stats.residuals_primal), len(w.stats.residuals_dual))),
                                                       len(seen) == 3)[1])
    assert seen == [(2, 2), (3, 3), (4, 4)] and st.niter == 3 and st.status == "user-requested exit"
    n = S.shape[0]
    x, t, st = tr.trilqr(S, b, c, x0=np.linspace(-0.5, 0.5, n), y0=np.linspace(0.25, -0.25, n))
    assert st.solved_primal and st.solved_dual
    assert np.linalg.norm(b - S @ x) <= 1e-6 * np.linalg.norm(b) and np.linalg.norm(c - S.T @ t) <= 1e-6 * np.linalg.norm(c)


# ---- injected faults the comparison rejects ---------------------------------------------------------------------------------------
# fault -> (case, transfer): the w faults need a dual side that runs past k = 4 with c ≠ b; "dual_not_frozen" a dual side that ends
# first and "primal_not_frozen" a primal side that ends first
FAULT_SYSTEMS = {"lambda_sign": ("kron4_sinc", True), "stage4_as_3": ("kron4_sinc", True), "no_rotation": ("kron4_sinc", True),
                 "psi_after_shift": ("kron4_sinc", True), "dual_not_frozen": ("kron7_shift24_sinc", True),
                 "primal_not_frozen": ("poisson8", True), "v_prev_after_store": ("kron4_sinc", True)}
SILENT_FAULTS = ("stage3_as_4",)


def _fault_run(oracle, case, transfer, fault):
    S, b, c = case_system(oracle, case)
    St = S.T.tocsr()
    kw = case_keywords(case, transfer)
    return reference_pair(oracle, case, transfer)[0], tr.trilqr(S, b, c, At=St, fault=fault, **kw), budget(oracle, case, transfer)


@pytest.mark.parametrize("fault", [f for f in tr.FAULTS if f not in SILENT_FAULTS])
def test_comparison_rejects_injected_fault(oracle, fault):
    case, transfer = FAULT_SYSTEMS[fault]
    (x, t, st), (xf, tf, sf), bud = _fault_run(oracle, case, transfer, fault)
    assert mismatches(st, st, bud, x, x, t, t) == []
    bad = mismatches(sf, st, bud, xf, x, tf, t)
    print(f"{fault} on {case} (budget {bud:.1e}): {bad}")
    assert bad, f"the comparison does not see {fault}"


def test_scaling_at_stage_three_is_not_a_fault(oracle):
    """"Stage 3 treated as stage 4" (kscal!(-ϵₖ₋₃, wₖ₋₃) already at k = 3) changes no bit: ϵₖ₋₃ is still the 0 of the set-up at k = 3
    (:185, shifted at :400-402 only after the dual block) and wₖ₋₃ is the zero-filled buffer (:186), so -0 · 0 + v₂ = v₂.  The
    comparison cannot reject it because nothing differs; the opposite slip, stage 4 treated as stage 3, is in the list above."""
    (x, t, st), (xf, tf, sf), bud = _fault_run(oracle, "kron4_sinc", True, "stage3_as_4")
    assert np.array_equal(tf, t) and np.array_equal(xf, x)
    for name in tr.VECTORS:
        assert np.array_equal(sf.vectors[name], st.vectors[name]), name
    assert mismatches(sf, st, 0.0, xf, x, tf, t) == []


# ---- the Python mirror's tables -----------------------------------------------------------------------------------------------------
TRILQR_SYMBOLS = ("khip_trilqr_default_params", "khip_trilqr_workspace_create", "khip_trilqr_workspace_adopt",
                  "khip_trilqr_workspace_adopt_vector", "khip_trilqr_workspace_destroy", "khip_trilqr_warm_start", "khip_trilqr_solve",
                  "khip_trilqr_solution_x", "khip_trilqr_solution_y", "khip_trilqr_stats", "khip_trilqr_adjoint_stats",
                  "khip_trilqr_last_path", "khip_trilqr_vector", "khip_trilqr_workspace_bytes")


def test_python_mirror_exports_trilqr():
    """The mirror has the whole TRILQR surface (fails before the feature: K.trilqr did not exist)."""
    import krylov_jl_amd as K
    for name in ("trilqr", "trilqr_", "TrilqrWorkspace"):
        assert hasattr(K, name), name
    for sym in TRILQR_SYMBOLS:
        assert sym in K.SIGNATURES, sym
        assert hasattr(K.lib(), sym), sym
    header = open(os.path.join(ROOT, "include", "krylov_hip.h")).read()
    assert sorted(set(re.findall(r"\b(khip_trilqr_[a-z_]+)\s*\(", header))) == sorted(TRILQR_SYMBOLS)
    assert K._INPLACE[K.TrilqrWorkspace] == ("trilqr", K.trilqr_)
    assert "trilqr" not in K.WORKSPACE_KWARGS
    assert K.TrilqrWorkspace.VECTORS == tr.VECTORS
    assert K.TrilqrWorkspace.ROW_SIDE == ("v_prev", "v", "q", "y", "w_prev3", "w_prev2", "dy")
    assert len(K.SIGNATURES["khip_trilqr_workspace_adopt"][1]) == 3 + 11 + 1
    assert "runs the primitive sequence" in K.TrilqrWorkspace.__doc__ and "reports 0" in K.TrilqrWorkspace.__doc__
    assert K.lib().khip_trilqr_default_params().transfer_to_usymcg == 1
    assert K.Context.PROFILE_FAMILIES[15] == "trilqr_p3" and K.Context.PROFILE_FAMILIES[:15] == K.Context.PROFILE_TAGS


@ref_tree
def test_workspace_vectors_follow_the_reference_struct():
    ws_src = open(os.path.join(REFERENCE_SRC, "krylov_workspaces.jl")).read()
    struct = re.search(r"mutable struct TrilqrWorkspace\{T,FC,Sm,Sn\}.*?\nend", ws_src, flags=re.S).group(0)
    fields = re.findall(r"^\s+(\S+)\s+::\s+(Sm|Sn)\s*$", struct, flags=re.M)
    names = {"uₖ₋₁": "u_prev", "uₖ": "u", "p": "p", "d̅": "dbar", "Δx": "dx", "x": "x", "vₖ₋₁": "v_prev", "vₖ": "v", "q": "q",
             "Δy": "dy", "y": "y", "wₖ₋₃": "w_prev3", "wₖ₋₂": "w_prev2"}
    import krylov_jl_amd as K
    assert tuple(names[f] for f, _ in fields if f not in ("Δx", "Δy")) == K.TrilqrWorkspace.VECTORS
    assert tuple(names[f] for f, side in fields if side == "Sm" and f != "Δy") + ("dy",) == K.TrilqrWorkspace.ROW_SIDE
    assert dict(fields)["Δy"] == "Sm" and dict(fields)["Δx"] == "Sn"


@ref_tree
def test_forwarded_defaults_equal_the_reference():
    """FORWARDED_DEFAULTS["trilqr"] = kwargs_trilqr / def_kwargs_trilqr of src/trilqr.jl, names in order, defaults as values."""
    import krylov_jl_amd as K
    src = open(os.path.join(REFERENCE_SRC, "trilqr.jl")).read()
    names = re.findall(r":(\w+)", re.search(r"^kwargs_trilqr = \((.*?)\)", src, flags=re.M).group(1))
    table = re.search(r"^def_kwargs_trilqr = \((.*?)\)\n\n", src, flags=re.M | re.S).group(1)
    defaults = {m.group(1): m.group(2) for m in
                re.finditer(r":\(;\s*(\w+)(?:::[^=]+?)?\s*=\s*(.*?)\s*\)\s*[,)]?\s*$", table, flags=re.M)}
    assert list(defaults) == names
    mine = K.FORWARDED_DEFAULTS["trilqr"]
    assert list(mine) == names
    sq = math.sqrt(np.finfo(np.float64).eps)
    value = {"false": False, "true": True, "√eps(T)": sq, "0": 0, "Inf": math.inf, "kstdout": None}
    for k, expr in defaults.items():
        if k == "callback":
            assert expr == "workspace -> false" and mine[k] is K.default_callback
        else:
            assert mine[k] == value[expr] and type(mine[k]) is type(value[expr]), (k, expr, mine[k])
    assert re.search(r"^args_trilqr = \(:A, :b, :c\)$", src, flags=re.M) and re.search(r"^optargs_trilqr = \(:x0, :y0\)$", src, flags=re.M)


# ---- the Julia specialisation, as text ----------------------------------------------------------------------------------------------
def _julia_trilqr():
    glue = open(JULIA_SRC).read()
    m = re.search(r"function Krylov\.trilqr!\(ws::TrilqrWs, A::HIPCsr, b::HIPVector, c::HIPVector;(.*?)\)\n(.*?)\nend\n", glue, flags=re.S)
    assert m, "no specialised Krylov.trilqr!"
    return glue, m.group(1), m.group(2)


def test_julia_trilqr_specialisation_shape():
    """The Julia trilqr! (checked as text: Julia does not run here): the TrilqrWs alias, the eleven adopted vectors in the order of
    khip_trilqr_workspace_adopt, the fallback gate, the default callback's recognition, LAST_PATH, A' taken once, the transfer
    flag passed in khip_trilqr_params, both flags and both histories read back, and test/trilqr.jl reached from runtests.jl."""
    glue, sig, body = _julia_trilqr()
    assert "const TrilqrWs = TrilqrWorkspace{Float64,Float64,HIPVector,HIPVector}" in glue
    adopt = re.search(r"ccall\(\(:khip_trilqr_workspace_adopt, lib\), Cint, \((.*?)\),\n\s+CTX\[\]\.h, ws\.m, ws\.n, (.*?), r\)\)", glue,
                      flags=re.S)
    assert adopt, "trilqr_handle does not adopt the workspace's vectors"
    assert adopt.group(1).count("Ptr{Cdouble}") == 11
    assert [a.strip() for a in adopt.group(2).split(",")] == [f"ws.{f}.ptr" for f in
                                                              ("uₖ₋₁", "uₖ", "p", "d̅", "x", "vₖ₋₁", "vₖ", "q", "y", "wₖ₋₃", "wₖ₋₂")]
    assert "if !native_log(verbose, iostream)" in body
    assert "invoke(Krylov.trilqr!, Tuple{TrilqrWs,Any,AbstractVector{Float64},AbstractVector{Float64}}, ws, A, b, c;" in body
    assert "callback = callback === nothing ? (w -> false) : callback" in body
    assert "NATIVE_SOLVES[] += 1" in body and "LAST_PATH[] = ccall((:khip_trilqr_last_path, lib)" in body
    assert "khip_trilqr_warm_start" in body and "ws.warm_start = false" in body
    assert "TrilqrParams(Cint(transfer_to_usymcg))" in body
    assert "st = fill_trilqr_stats!(ws.stats, h, sp, history)" in body and "trilqr_callback(user_callback(callback), h, sp, history)" in body
    fill = re.search(r"function fill_trilqr_stats!\(.*?\nend\n", glue, flags=re.S).group(0)
    for piece in ("khip_trilqr_adjoint_stats", "stats.solved_primal = sprim[] != 0", "stats.solved_dual = sdual[] != 0",
                  "append!(stats.residuals_primal", "append!(stats.residuals_dual", "stats.status = unsafe_string"):
        assert piece in fill, piece
    assert len(re.findall(r"(?<![\w])A'", body)) == 1, "A' is taken once per solve (and cached on the matrix by Base.adjoint)"
    assert "callback = nothing" in sig and "fused::Int = 2" in sig and "transfer_to_usymcg::Bool = true" in sig
    tests = os.path.join(ROOT, "julia", "KrylovHIP", "test")
    trilqr_jl = open(os.path.join(tests, "trilqr.jl")).read()
    for piece in ("TrilqrWorkspace(n, n, S, S)", "native(2) do; trilqr!(ws, A_gpu, b, c; history = true); end",
                  "generic(trilqr!, ws2, A_gpu, b, c;", "TRILQR: primal system of $n equations in $n variables"):
        assert piece in trilqr_jl, piece
    assert 'include("trilqr.jl")' in open(os.path.join(tests, "runtests.jl")).read()


@ref_tree
def test_julia_trilqr_specialisation():
    """Against the reference tree: every keyword of kwargs_trilqr is in the signature, and the glue reads only fields of
    TrilqrWorkspace (src/krylov_workspaces.jl)."""
    glue, sig, body = _julia_trilqr()
    src = open(os.path.join(REFERENCE_SRC, "trilqr.jl")).read()
    names = re.findall(r":(\w+)", re.search(r"^kwargs_trilqr = \((.*?)\)", src, flags=re.M).group(1))
    for kw in names:
        assert re.search(r"(?<![\w])" + kw + r"(?![\w])", sig), f"trilqr!: keyword {kw} of the reference is missing"
    ws_src = open(os.path.join(REFERENCE_SRC, "krylov_workspaces.jl")).read()
    struct = re.search(r"mutable struct TrilqrWorkspace\{T,FC,Sm,Sn\}.*?\nend", ws_src, flags=re.S).group(0)
    fields = set(re.findall(r"^\s+(\S+)\s+::", struct, flags=re.M))
    used = set(re.findall(r"\bws\.([^\s.,;()\[\]]+)", body))
    handle = re.search(r"function trilqr_handle\(ws::TrilqrWs\)\n(.*?)\nend\n", glue, flags=re.S).group(1)
    used |= set(re.findall(r"\bws\.([^\s.,;()\[\]]+)", handle))
    assert used <= fields, used - fields
    assert {"uₖ₋₁", "uₖ", "p", "d̅", "x", "vₖ₋₁", "vₖ", "q", "y", "wₖ₋₃", "wₖ₋₂", "Δx", "Δy"} <= used
