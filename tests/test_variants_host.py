"""The restatements of the opt-in recurrences (tests/variants_reference.py) without a GPU: each against the oracle's cg! / gmres!
within the budgets the GPU tests of the variants already assert (tests/test_gpu_solvers.py), which pins the restatements before
anything is pinned to them; the condition that admits a case to the GPU tests' case list (tests/test_gpu_variants.py imports
it); and the ways a solve ends."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import variants_reference as vr  # noqa: E402

RESTATEMENT = {1: vr.cg_single_reduction, 2: vr.cg_pipelined}


def tridiagonal(n):
    """tridiag(-1, 2.5, -1): the operator of tests/test_gpu_vec_dispatch.py"""
    S = sp.diags([np.full(n - 1, -1.0), np.full(n, 2.5), np.full(n - 1, -1.0)], [-1, 0, 1], format="csr")
    S.sort_indices()
    return S


def case_matrix(oracle, kind, size):
    """the operator of a case as a SciPy CSR matrix"""
    if kind == "tridiagonal":
        return tridiagonal(size)
    S = {"poisson": oracle.poisson3d, "kron": oracle.kron_unsymmetric}[kind](size).to_scipy().tocsr()
    S.sort_indices()
    return S


def case_rhs(n, which):
    return np.ones(n) if which == "ones" else np.cos(0.37 * np.arange(n)) + 0.5


# ---- the GPU tests' case lists ------------------------------------------------------------------------------------------------------
# name -> (operator, size parameter, right-hand side, keywords)
# Tried and dropped by the admission rule (test_case_list_condition): poisson5_ones and poisson7_ones.  With b = ones on an odd grid the
# Krylov space ends exactly (7 and 16 steps) and the last residual is pure rounding: np.dot against fsum dots differ there by
# 3.7e-1 / 1.9e-1 (variant 1) and 2.9e-1 / 3.3e-1 (variant 2) relative.  Every other case measures <= 2.5e-8.
CG_CASES = {f"{kind}{size}_{which}": (kind, size, which, {})
            for kind, size in (("poisson", 5), ("poisson", 7), ("poisson", 8), ("tridiagonal", 511), ("tridiagonal", 513))
            for which in ("ones", "cos") if (kind, size, which) not in (("poisson", 5, "ones"), ("poisson", 7, "ones"))}
GMRES_CASES = {f"kron{size}_{which}_{tag}": ("kron", size, which, kw)
               for size in (7, 8) for which in ("ones", "cos")
               for tag, kw in (("mem10", dict(memory=10)), ("mem10_restart", dict(memory=10, restart=True)), ("mem4", dict(memory=4)))}

_PAIRS = {}


def reference_pair(oracle, solver, name, **extra):
    """(restatement with np.dot, restatement with exactly summed dots) of a case, as (x, stats) pairs; computed once.
    solver: 1 / 2 = the cg! variants, "gmres" = CGS2"""
    key = (solver, name, tuple(sorted((k, repr(v)) for k, v in extra.items())))
    if key not in _PAIRS:
        kind, size, which, kw = (GMRES_CASES if solver == "gmres" else CG_CASES)[name]
        S = case_matrix(oracle, kind, size)
        b = case_rhs(S.shape[0], which)
        fn = vr.gmres_cgs2 if solver == "gmres" else RESTATEMENT[solver]
        kw = dict(kw, **extra)
        _PAIRS[key] = (fn(S, b, **kw), fn(S, b, dot=vr.fsum_dot, **kw))
    return _PAIRS[key]


def _above(h, href, floor):
    k = min(len(h), len(href))
    big = href[:k] >= floor * href[0]
    return float(np.max(np.abs(h[:k] - href[:k])[big] / href[:k][big]))


@pytest.mark.parametrize("name", list(CG_CASES))
@pytest.mark.parametrize("variant", [1, 2])
def test_cg_restatements_against_the_oracle(oracle, variant, name):
    """the budgets of test_cg_single_reduction_variant_parity_budget / test_cg_pipelined_variant_parity_budget: same status,
    niter within 2 / 3, history within 1e-6 / 1e-5 relative while above 1e-6 / 1e-5 r_0"""
    kind, size, which, kw = CG_CASES[name]
    S = case_matrix(oracle, kind, size)
    b = case_rhs(S.shape[0], which)
    ref = oracle.cg(lambda v: S @ v, b, history=True)
    (x, st), _ = reference_pair(oracle, variant, name)
    slack, tol = {1: (2, 1e-6), 2: (3, 1e-5)}[variant]
    dev = _above(st.residuals, ref.residuals, tol)
    print(f"cg variant {variant} {name}: niter {st.niter} (oracle {ref.niter}), history {dev:.2e}")
    assert st.solved and st.status == ref.status == vr.SOLVED
    assert abs(st.niter - ref.niter) <= slack and len(st.residuals) == st.niter + 1
    assert dev <= tol
    assert np.allclose(x, ref.x, rtol=0, atol={1: 1e-7, 2: 1e-6}[variant] * np.abs(ref.x).max())


@pytest.mark.parametrize("name", list(GMRES_CASES))
def test_cgs2_restatement_against_the_oracle(oracle, name):
    """the budget of test_gmres_cgs2_variant_parity_budget: niter within 1, history within 1e-6 while above 1e-6 r_0"""
    kind, size, which, kw = GMRES_CASES[name]
    S = case_matrix(oracle, kind, size)
    b = case_rhs(S.shape[0], which)
    ref = oracle.gmres(lambda v: S @ v, b, history=True, **kw)
    (x, st), _ = reference_pair(oracle, "gmres", name)
    dev = _above(st.residuals, ref.residuals, 1e-6)
    print(f"gmres variant 1 {name}: niter {st.niter} (oracle {ref.niter}), history {dev:.2e}")
    assert st.solved and st.status == ref.status
    assert abs(st.niter - ref.niter) <= 1 and len(st.residuals) == st.niter + 1
    assert dev <= 1e-6
    assert np.linalg.norm(b - S @ x) / np.linalg.norm(b) <= 1e-6


@pytest.mark.parametrize("solver,name", [(v, n) for v in (1, 2) for n in CG_CASES] + [("gmres", n) for n in GMRES_CASES])
def test_case_list_condition(oracle, solver, name):
    """A case may be in a list only if the restatement with np.dot and with math.fsum dots agree on niter and status and their
    whole residual histories agree to <= 1e-6 relative (the admission rule of tests/test_qmr_host.py)."""
    (_, s1), (_, s2) = reference_pair(oracle, solver, name)
    dev = vr.history_deviation(s1.residuals, s2.residuals)
    print(f"{solver} {name}: niter = {s1.niter} / {s2.niter}, deviation {dev:.1e}")
    assert s1.niter == s2.niter and s1.status == s2.status and s1.solved
    assert dev <= 1e-6


# ---- the ways a solve ends ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [1, 2])
def test_cg_endings(variant):
    cg = RESTATEMENT[variant]
    A2, b2 = np.array([[4.0, 1.0], [1.0, 3.0]]), np.array([1.0, 2.0])
    x, st = cg(A2, b2)                                                       # exact after two steps in exact arithmetic
    assert st.solved and st.status == vr.SOLVED and st.niter <= 3 and np.allclose(A2 @ x, b2, atol=1e-12)
    x, st = cg(A2, b2, itmax=1)
    assert st.niter == 1 and not st.solved and st.status == vr.TIRED and len(st.residuals) == 2
    assert np.allclose(x, (b2 @ b2) / (b2 @ A2 @ b2) * b2)                   # the steepest-descent step
    x, st = cg(A2, np.zeros(2))
    assert st.niter == 0 and st.solved and st.status == vr.ZERO_RESIDUAL and not x.any() and list(st.residuals) == [0.0]
    x, st = cg(np.array([[2.0]]), np.array([3.0]))                           # n = 1
    assert st.niter == 1 and st.solved and x[0] == 1.5
    # indefinite diagonal operators: delta_0 = r.Ar <= 0 is refused before the loop ...
    x, st = cg(np.diag([1.0, -2.0]), np.array([1.0, 1.0]))
    assert st.error == vr.NOT_SPD and st.niter == 0 and not st.solved and not x.any()
    x, st = cg(np.array([[-1.0]]), np.array([1.0]))
    assert st.error == vr.NOT_SPD
    # ... and delta_0 > 0 with a negative direction later sets the breakdown flag in the epilogue
    x, st = cg(np.diag([1.0, -0.25]), np.array([1.0, 1.0]))
    assert st.error is None and st.breakdown and st.inconsistent and not st.solved and st.status == vr.ZERO_CURVATURE
    assert st.niter == 1


@pytest.mark.parametrize("variant", [1, 2])
def test_cg_warm_start(oracle, variant):
    S = case_matrix(oracle, "poisson", 5)
    b = case_rhs(S.shape[0], "cos")
    (x, st), _ = reference_pair(oracle, variant, "poisson5_cos")
    x0 = x * (1 + 1e-3 * np.cos(np.arange(x.size)))
    xw, sw = RESTATEMENT[variant](S, b, x0=x0)
    assert sw.solved and sw.niter < st.niter and np.allclose(xw, x, rtol=0, atol=1e-6 * np.abs(x).max())
    assert np.isclose(sw.residuals[0], np.linalg.norm(b - S @ x0))


def test_cgs2_basis_is_orthonormal_and_grows(oracle):
    S = case_matrix(oracle, "kron", 7)
    b = case_rhs(S.shape[0], "ones")
    x, st = vr.gmres_cgs2(S, b, memory=4)                                    # no restart: the basis grows past memory
    V = np.array(st.vectors["V"])
    assert st.solved and st.niter > 4 and V.shape[0] >= st.niter
    assert np.max(np.abs(V @ V.T - np.eye(V.shape[0]))) <= 1e-13
    x, st = vr.gmres_cgs2(S, b, memory=10, restart=True, itmax=13)
    assert st.niter == 13 and st.status == vr.TIRED and st.inner_iter == 3 and len(st.residuals) == 14
    x, st = vr.gmres_cgs2(S, np.zeros(S.shape[0]))
    assert st.niter == 0 and st.solved and st.status == vr.ZERO_RESIDUAL
