"""minres_qlp! without a GPU: the NumPy restatement (tests/minres_qlp_reference.py) against the reference's own test problems
(test/test_minres_qlp.jl), the case list of the GPU tests with the condition that admits a history of a case to their parity
list, three injected mistakes the parity comparison rejects, the Python mirror's tables and the header against
src/minres_qlp.jl, and the Julia specialisation's shape (as text: Julia does not run here)."""
import math
import os
import re
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import minres_qlp_reference as mr  # noqa: E402
from test_bilq_host import rhs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_SRC = "/root/reference/src"
JULIA_SRC = os.path.join(ROOT, "julia", "KrylovHIP", "src", "KrylovHIP.jl")
ref_tree = pytest.mark.skipif(not os.path.isdir(REFERENCE_SRC), reason="the reference tree is only present in the build container")


@pytest.fixture(autouse=True)
def _the_feature_is_there():
    """The restatement checks minres_qlp!: without the mirror's entry points there is nothing for it to check, and every test here
    fails."""
    import krylov_jl_amd as K
    assert hasattr(K, "minres_qlp") and hasattr(K, "minres_qlp_") and hasattr(K, "MinresQlpWorkspace")


# ---- operators -------------------------------------------------------------------------------------------------------------------
def tridiag(n, diag=2.0, off=-1.0):
    return sp.diags([np.full(max(n - 1, 0), off), np.full(n, diag), np.full(max(n - 1, 0), off)], [-1, 0, 1], format="csr")


def neumann(n):
    """The 1-D Laplacian with Neumann ends: singular, its null vector is the constant."""
    d = np.full(n, 2.0)
    d[0] = d[-1] = 1.0
    return sp.diags([np.full(n - 1, -1.0), d, np.full(n - 1, -1.0)], [-1, 0, 1], format="csr")


def smallest_eigenvalue(m):
    """Of get_div_grad(m, m, m): 6 - 6 cos(π / (m + 1)); its eigenvector is u ⊗ u ⊗ u with u_i = sin(π i / (m + 1))."""
    return 6.0 - 6.0 * math.cos(math.pi / (m + 1))


def null_vector(m):
    u = np.sin(np.pi * np.arange(1, m + 1) / (m + 1))
    return np.einsum("i,j,k->ijk", u, u, u).ravel()


_SP = {}


def case_matrix(oracle, kind, size):
    """The SciPy CSR operator of a case, built once."""
    if (kind, size) not in _SP:
        if kind == "poisson":                                         # get_div_grad(size, size, size)
            S = oracle.poisson3d(size).to_scipy()
        elif kind == "neumann":
            S = neumann(size)
        elif kind == "tridiag":
            S = tridiag(size)
        elif kind == "sym_indef":                                     # symmetric_indefinite (test/test_utils.jl:26-31)
            S = tridiag(size, 1.0, 1.0)
        elif kind == "square_inconsistent":                           # test/test_utils.jl:120-125: I with a zero at (1, 1), kept as an entry
            S = sp.diags([np.r_[0.0, np.ones(size - 1)]], [0], format="csr")
        elif kind == "symmetric_inconsistent":                        # test/test_utils.jl:128-132
            S = sp.csr_matrix(np.array([[3.0, 2.0, -1.0, 5.0], [2.0, -2.0, 4.0, 0.0], [-1.0, 4.0, 1.0, 3.0], [5.0, 0.0, 3.0, 5.0]]))
        else:                                                         # symmetric_breakdown (test/test_utils.jl:188-192)
            S = sp.csr_matrix(np.array([[0.0, 1.0], [1.0, 0.0]]))
        S = sp.csr_matrix(S)
        S.sort_indices()
        _SP[(kind, size)] = S
    return _SP[(kind, size)]


def case_rhs(S, which):
    n = S.shape[0]
    if which == "ones":
        return np.ones(n)
    if which == "sin":                                                # not orthogonal to the null vector: the system is inconsistent
        return np.sin(1.0 + 0.37 * np.arange(n))
    if which == "ramp":
        return np.arange(1.0, n + 1)
    if which == "ramp0":                                              # the ramp minus its mean: in the range of the Neumann operator
        b = np.arange(1.0, n + 1)
        return b - b.mean()
    if which == "A_ramp":                                             # b = A [1:n;]
        return S @ np.arange(1.0, n + 1)
    if which == "e1":
        return np.r_[1.0, np.zeros(n - 1)]
    if which == "zero":
        return np.zeros(n)
    if which == "sym_inc":
        return np.array([1.0, -8.0, 5.0, 2.0])
    return rhs(n)


# ---- the GPU tests' case list (tests/test_gpu_minres_qlp.py imports it) ----------------------------------------------------------
# name -> (operator, size parameter, right-hand side, keywords of minres_qlp).  λ = -0.5 lies inside the spectrum of get_div_grad(8³)
# (0.36 ... 11.6) and of get_div_grad(9³) (0.29 ... 11.7): A + λI is indefinite.  λ = -(smallest eigenvalue) makes it singular; the
# right-hand side sin(1 + 0.37 i) has a component along the null vector, so the system is inconsistent (b = ones ends "condition
# number seems too large" with ‖x‖ ≈ 1e17 on m = 8: the reference's behaviour, and no pin).
CASES = {
    "poisson8": ("poisson", 8, "ones", {}),                           # n = 512
    "poisson9": ("poisson", 9, "ones", {}),                           # n = 729: odd, the tail element
    "poisson8_lam": ("poisson", 8, "ones", dict(lam=-0.5)),
    "poisson9_lam": ("poisson", 9, "ones", dict(lam=-0.5)),
    "poisson8_tight": ("poisson", 8, "ones", dict(atol=0.0, rtol=1e-10)),
    "poisson8_itmax5": ("poisson", 8, "ones", dict(itmax=5)),
    "poisson8_singular": ("poisson", 8, "sin", dict(lam=-smallest_eigenvalue(8))),
    "poisson9_singular": ("poisson", 9, "sin", dict(lam=-smallest_eigenvalue(9))),
    "neumann63_inc": ("neumann", 63, "ramp", {}),
    "neumann64_inc": ("neumann", 64, "ramp", {}),
    "neumann65_inc": ("neumann", 65, "ramp", {}),
    "neumann63_cons": ("neumann", 63, "ramp0", {}),
    "neumann64_cons": ("neumann", 64, "ramp0", {}),
    "neumann65_cons": ("neumann", 65, "ramp0", {}),
    "tri1": ("tridiag", 1, "cos", {}),
    "tri2": ("tridiag", 2, "cos", {}),
    "tri3": ("tridiag", 3, "cos", {}),
    "tri63": ("tridiag", 63, "cos", {}),
    "tri64": ("tridiag", 64, "cos", {}),
    "tri65": ("tridiag", 65, "cos", {}),
    "sym_indef10": ("sym_indef", 10, "A_ramp", {}),
    "sym_indef10_lam2": ("sym_indef", 10, "A_ramp", dict(lam=2.0)),
    "square_inconsistent": ("square_inconsistent", 10, "ones", {}),
    "symmetric_inconsistent": ("symmetric_inconsistent", 4, "sym_inc", {}),
    "breakdown": ("breakdown", 2, "e1", {}),
    "zero_rhs": ("tridiag", 10, "zero", {}),
}
SINGULAR = ("poisson8_singular", "poisson9_singular")
INCONSISTENT = SINGULAR + ("neumann63_inc", "neumann64_inc", "neumann65_inc", "square_inconsistent", "symmetric_inconsistent")
# recorded from the restatement (np.dot and math.fsum dots agree on every one)
EXPECTED_NITER = {"poisson8": 18, "poisson9": 22, "poisson8_lam": 19, "poisson9_lam": 24, "poisson8_tight": 20, "poisson8_itmax5": 5,
                  "poisson8_singular": 42, "poisson9_singular": 49, "neumann63_inc": 32, "neumann64_inc": 33, "neumann65_inc": 33,
                  "neumann63_cons": 31, "neumann64_cons": 32, "neumann65_cons": 32, "tri1": 1, "tri2": 2, "tri3": 3, "tri63": 63,
                  "tri64": 64, "tri65": 65, "sym_indef10": 10, "sym_indef10_lam2": 10, "square_inconsistent": 2,
                  "symmetric_inconsistent": 4, "breakdown": 2, "zero_rhs": 0}
EXPECTED_STATUS = {name: (mr.INCONSISTENT if name in INCONSISTENT else mr.SOLVED) for name in CASES}
EXPECTED_STATUS.update(poisson8_itmax5=mr.TIRED, zero_rhs=mr.ZERO_RESIDUAL)
# The histories of a case that are compared entry by entry on the GPU: those whose own np.dot-against-fsum deviation is <= 1e-6
# (test_parity_list_condition).  The inconsistent endings by breakdown and the 2- and 4-iteration inconsistent cases carry rounding
# noise in the last entries of residuals and Acond (4e-4 ... 0.5); ‖Arₖ₋₁‖ of the singular Poisson cases converges to zero through
# cancellation (1e-2 and 2e-4).
PARITY_CAP = 1e-6
HIST_FLOOR = 1e-12                                                    # × the history's first entry: the floor of a comparison
MEASURE_FLOOR = 1e-9                                                  # × the history's first entry: the floor of the measurement
HISTORIES = ("residuals", "Aresiduals", "Acond")
_ALL = HISTORIES
_NO_R = ("Aresiduals", "Acond")       # the last entries of residuals, 1e-13 ‖r₀‖ and below, deviate by more than 1e-9 ‖r₀‖ × 1e-6
PARITY = {
    "poisson8": _ALL, "poisson9": _ALL, "poisson8_lam": _ALL, "poisson9_lam": _ALL, "poisson8_tight": _ALL, "poisson8_itmax5": _ALL,
    "poisson8_singular": ("residuals", "Acond"), "poisson9_singular": ("residuals", "Acond"),
    "neumann63_inc": (), "neumann64_inc": (), "neumann65_inc": (),
    "neumann63_cons": _NO_R, "neumann64_cons": _NO_R, "neumann65_cons": _ALL,
    "tri1": _ALL, "tri2": _ALL, "tri3": _ALL, "tri63": _NO_R, "tri64": _NO_R, "tri65": _NO_R,
    "sym_indef10": _NO_R, "sym_indef10_lam2": _ALL,
    "square_inconsistent": ("Aresiduals",), "symmetric_inconsistent": (),
    "breakdown": _ALL, "zero_rhs": _ALL,
}
PARITY_CASES = tuple(name for name in CASES if set(PARITY[name]) >= {"residuals", "Aresiduals"})


def history_floor(st, key, factor=HIST_FLOOR):
    """The absolute floor of a history: `factor` × its first entry (‖r₀‖ for residuals, the first ‖A r‖ for Aresiduals); none for
    Acond, which starts at 0 and never becomes small."""
    h = np.asarray(getattr(st, key))
    return 0.0 if key == "Acond" or len(h) == 0 else factor * abs(h[0])


def deviation(s1, s2, key):
    """Largest difference of two runs' history `key`, relative to its entries but to no less than 1e-9 × the first entry (an entry
    that far down is rounding noise of the recurrence); inf when the lengths or the places of NaN differ.  The floor of the
    measurement is a thousand times the floor of the comparison (HIST_FLOOR): a history is admitted on stricter terms than it
    is later compared on."""
    a, b = np.asarray(getattr(s1, key)), np.asarray(getattr(s2, key))
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return math.inf
    m = ~np.isnan(b)
    a, b = a[m], b[m]
    if len(b) == 0:
        return 0.0
    scale = np.maximum(np.maximum(np.abs(a), np.abs(b)), history_floor(s2, key, MEASURE_FLOOR))
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(a == b, 0.0, np.abs(a - b) / scale)
    return float(np.max(rel))


def x_deviation(x1, x2):
    return float(np.max(np.abs(x1 - x2)) / max(np.max(np.abs(x2)), np.finfo(np.float64).tiny)) if len(x2) else 0.0


_PAIRS = {}


def case_problem(oracle, name):
    kind, size, which, kw = CASES[name]
    S = case_matrix(oracle, kind, size)
    return S, case_rhs(S, which), dict(kw)


def reference_pair(oracle, name, **extra):
    """(restatement with np.dot, restatement with exactly summed dots) of a case, as (x, stats) pairs; computed once."""
    key = (name, tuple(sorted((k, id(v) if callable(v) else repr(v)) for k, v in extra.items())))
    if key not in _PAIRS:
        S, b, kw = case_problem(oracle, name)
        kw.update(extra)
        _PAIRS[key] = (mr.minres_qlp(S, b, **kw), mr.minres_qlp(S, b, dot=mr.fsum_dot, **kw))
    return _PAIRS[key]


def pair_budget(pair, keys=HISTORIES):
    """10 × the pair's own sensitivity to the rounding of its dots, over the histories `keys` and x; at least 1e-8."""
    (x1, s1), (x2, s2) = pair
    dev = max([deviation(s1, s2, k) for k in keys] + [x_deviation(x1, x2)])
    return max(1e-8, 10.0 * dev)


def case_budget(oracle, name):
    return pair_budget(reference_pair(oracle, name), PARITY[name])


@pytest.mark.parametrize("name", list(CASES))
def test_case_list(oracle, name):
    """Every case ends in the recorded number of iterations with the same status and flags whichever way the dots are rounded; its
    np.dot-against-fsum deviations are printed.  Acond has one entry more than Aresiduals."""
    (x1, s1), (x2, s2) = reference_pair(oracle, name)
    devs = {k: deviation(s1, s2, k) for k in HISTORIES}
    print(f"{name}: {s1.niter} iterations, {s1.status}; np.dot against fsum: " + ", ".join(f"{k} {v:.3e}" for k, v in devs.items()) +
          f", x {x_deviation(x1, x2):.3e}")
    assert s1.niter == s2.niter == EXPECTED_NITER[name], (s1.niter, s2.niter)
    assert s1.status == s2.status == EXPECTED_STATUS[name]
    assert s1.solved == s2.solved and s1.inconsistent == s2.inconsistent == (name in INCONSISTENT)
    assert len(s1.residuals) == len(s1.Acond) == s1.niter + 1 and len(s1.Aresiduals) == s1.niter
    assert x_deviation(x1, x2) <= 1e-9


def test_parity_list_condition(oracle):
    """A history of a case is compared on the GPU exactly when the restatement's own deviation between the two dot modes is
    <= 1e-6; at least 12 cases qualify with residuals and Aresiduals, and both singular Poisson cases qualify for residuals."""
    for name in CASES:
        (_, s1), (_, s2) = reference_pair(oracle, name)
        for k in HISTORIES:
            dev = deviation(s1, s2, k)
            assert (dev <= PARITY_CAP) == (k in PARITY[name]), (name, k, dev)
    assert len(PARITY_CASES) >= 12
    for name in SINGULAR:
        assert "residuals" in PARITY[name]


def test_outcomes_of_the_case_list(oracle):
    """What the endings mean, on the restatement: the shifted indefinite solves converge in the true residual of the SHIFTED system;
    the singular cases end with the minimum-length least-squares solution (‖(A + λI) r‖ small against ‖(A + λI) b‖, x orthogonal
    to the null vector); the Neumann cases end by breakdown, Σx ≈ 0."""
    for name in ("poisson8_lam", "poisson9_lam", "sym_indef10_lam2"):
        S, b, kw = case_problem(oracle, name)
        (x, st), _ = reference_pair(oracle, name)
        r = b - S @ x - kw["lam"] * x
        assert st.solved and abs(np.linalg.norm(r) - st.residuals[-1]) <= 1e-8 * np.linalg.norm(b)
    for name, m in zip(SINGULAR, (8, 9)):
        S, b, kw = case_problem(oracle, name)
        lo = spla.eigsh(S, k=1, which="SA", return_eigenvectors=False)[0]
        assert abs(lo + kw["lam"]) <= 1e-12
        (x, st), _ = reference_pair(oracle, name)
        r = b - S @ x - kw["lam"] * x
        Ar, Ab = S @ r + kw["lam"] * r, S @ b + kw["lam"] * b
        u = null_vector(m)
        print(f"{name}: ‖(A+λI)r‖ {np.linalg.norm(Ar):.3e}, x.u / (‖x‖‖u‖) {abs(x @ u) / np.linalg.norm(x) / np.linalg.norm(u):.3e}")
        assert st.inconsistent and not st.solved and np.linalg.norm(Ar) <= 1e-6 * np.linalg.norm(Ab)
        proj = abs(b @ u) / np.linalg.norm(u)                                       # b is not in the range: its part along u is
        assert proj > 1e-4 * np.linalg.norm(b)                                      # the least-squares residual
        assert abs(np.linalg.norm(r) - proj) <= 1e-8 * np.linalg.norm(b) and abs(st.residuals[-1] - proj) <= 1e-8 * np.linalg.norm(b)
        assert abs(x @ u) <= 1e-12 * np.linalg.norm(x) * np.linalg.norm(u)
    for n in (63, 64, 65):
        (x, st), _ = reference_pair(oracle, f"neumann{n}_inc")
        assert st.inconsistent and st.breakdown and abs(x.sum()) <= 1e-6 * np.abs(x).sum()
        (x, st), _ = reference_pair(oracle, f"neumann{n}_cons")
        assert st.solved and not st.inconsistent and abs(x.sum()) <= 1e-6 * np.abs(x).sum()


# ---- injected mistakes: the parity comparison of the GPU tests rejects each ------------------------------------------------------
def _parity_accepts(oracle, name, fault):
    """Whether a run with the injected mistake would pass the comparison the GPU tests make against the restatement: niter, status,
    flags, the qualifying histories and x within the case's budget."""
    S, b, kw = case_problem(oracle, name)
    (xr, sr_), _ = reference_pair(oracle, name)
    x, st = mr.minres_qlp(S, b, fault=fault, **kw)
    rtol = case_budget(oracle, name)
    if (st.niter, st.status, st.solved, st.inconsistent) != (sr_.niter, sr_.status, sr_.solved, sr_.inconsistent):
        return False
    for k in PARITY[name]:
        if deviation(st, sr_, k) > rtol:
            return False
    return x_deviation(x, xr) <= rtol


@pytest.mark.parametrize("fault", mr.FAULTS)
@pytest.mark.parametrize("name", ["poisson8_lam", "poisson9_lam", "poisson8_singular"])
def test_injected_mistakes_are_rejected(oracle, name, fault):
    """α taken as vₖᴴA vₖ, the dot a fused product delivers, instead of ⟨vₖ, A vₖ + λ vₖ − βₖ vₖ₋₁⟩; a dropped final
    kaxpy!(τₖ₋₁, wₖ₋₁, x); and cpₖ, spₖ of the iteration before in the x update: none passes; the unmodified run does."""
    assert _parity_accepts(oracle, name, None)
    assert not _parity_accepts(oracle, name, fault)


def test_where_alpha_as_vAv_cannot_be_seen(oracle):
    """With λ = 0 the two dots differ by βₖ ⟨vₖ, vₖ₋₁⟩ only, and consecutive Lanczos vectors are orthogonal to rounding: there the
    mistake is below every budget, which is why the cases above carry a shift."""
    assert _parity_accepts(oracle, "poisson8", "alpha_is_vAv")
    for fault in ("no_final_axpy", "stale_cp_sp"):
        assert not _parity_accepts(oracle, "poisson8", fault)


# ---- the reference's own test problems (test/test_minres_qlp.jl, test/test_utils.jl), Float64 -----------------------------------
def _reference_bound(A, b, x, lam=0.0, M=None):
    """resid ≤ minres_qlp_tol ‖A‖ ‖x‖ with resid = ‖b - (A + λI) x‖ / ‖b‖ (test/test_minres_qlp.jl:10-12, :65-67; with M the M-norm of
    r, :73-75); Julia's norm(A) of a matrix is the Frobenius norm."""
    fro = spla.norm(A) if sp.issparse(A) else np.linalg.norm(np.asarray(A))
    r = b - A @ x - lam * x
    resid = (np.linalg.norm(r) if M is None else math.sqrt(float(r @ (M @ r)))) / np.linalg.norm(b)
    print(f"resid {resid:.3e}, bound {1.0e-6 * fro * np.linalg.norm(x):.3e}")
    return resid <= 1.0e-6 * fro * np.linalg.norm(x)


def _aresid_bound(A, b, x):
    """‖A r‖ / ‖A b‖ ≤ minres_qlp_tol (test/test_minres_qlp.jl:48-50)."""
    r = b - A @ x
    return np.linalg.norm(A @ r) / np.linalg.norm(A @ b) <= 1.0e-6


def test_symmetric_definite():
    A = tridiag(10, 4.0, 1.0)
    b = A @ np.arange(1.0, 11.0)
    x, st = mr.minres_qlp(A, b)
    assert st.solved and _reference_bound(A, b, x)


@pytest.mark.parametrize("lam", [0.0, 2.0])
def test_symmetric_indefinite(lam):
    A = tridiag(10, 1.0, 1.0)
    b = A @ np.arange(1.0, 11.0)
    assert min(np.linalg.eigvalsh(A.toarray())) < 0
    x, st = mr.minres_qlp(A, b, lam=lam)
    assert st.solved and _reference_bound(A, b, x, lam=lam)


def test_sparse_laplacian(oracle):
    A = oracle.poisson3d(16).to_scipy()
    b = np.ones(16 ** 3)
    x, st = mr.minres_qlp(A, b)
    assert st.solved and _reference_bound(A, b, x)


def test_square_inconsistent():
    A = np.diag(np.r_[0.0, np.ones(9)])
    b = np.ones(10)
    x, st = mr.minres_qlp(A, b)
    assert st.inconsistent and _aresid_bound(A, b, x) and st.status == mr.INCONSISTENT


def test_symmetric_inconsistent():
    A = np.array([[3.0, 2.0, -1.0, 5.0], [2.0, -2.0, 4.0, 0.0], [-1.0, 4.0, 1.0, 3.0], [5.0, 0.0, 3.0, 5.0]])
    b = np.array([1.0, -8.0, 5.0, 2.0])
    x, st = mr.minres_qlp(A, b)
    assert st.inconsistent and _aresid_bound(A, b, x)


def test_zero_right_hand_side():
    x, st = mr.minres_qlp(np.random.default_rng(0).random((10, 10)), np.zeros(10))
    assert np.linalg.norm(x) == 0 and st.status == "x is a zero-residual solution" and st.niter == 0 and st.solved
    assert not st.inconsistent and list(st.residuals) == [0.0] and list(st.Acond) == [0.0] and len(st.Aresiduals) == 0


def test_square_preconditioned():
    n = 10
    A = np.ones((n, n)) + (n - 1) * np.eye(n)
    b = 10.0 * np.arange(1.0, n + 1)
    M = (1.0 / n) * np.eye(n)
    x, st = mr.minres_qlp(A, b, M=M)
    assert st.solved and _reference_bound(A, b, x, M=M) and "vk" in st.vectors


def test_warm_start_and_callback_of_the_restatement(oracle):
    S = case_matrix(oracle, "poisson", 8)
    b = rhs(512)
    x0 = np.linspace(-0.5, 0.5, 512)
    for lam in (0.0, -0.5):
        x, st = mr.minres_qlp(S, b, x0=x0, lam=lam)
        _, s0 = mr.minres_qlp(S, b - S @ x0 - lam * x0, lam=lam)
        assert st.niter == s0.niter and np.allclose(st.residuals, s0.residuals, rtol=1e-12, atol=0)
    seen = []
    x, st = mr.minres_qlp(S, b, callback=lambda w: (seen.append(len(w.stats.residuals)), len(seen) == 2)[1])
    assert seen == [2, 3] and st.niter == 2 and st.status == "user-requested exit"


# ---- the Python mirror's tables and the header -----------------------------------------------------------------------------------
MINRES_QLP_SYMBOLS = tuple("khip_minres_qlp_" + s for s in (
    "default_params", "workspace_create", "workspace_adopt", "workspace_adopt_vector", "workspace_destroy", "warm_start", "solve",
    "solution", "stats", "histories", "last_path", "fused_product", "vector", "workspace_bytes"))
CORE = ("x", "wkm1", "wk", "Mvkm1", "Mvk", "p")


def test_python_mirror_exports_minres_qlp():
    """The mirror has the whole MINRES-QLP surface (fails before the feature: K.minres_qlp did not exist)."""
    import krylov_jl_amd as K
    for name in ("minres_qlp", "minres_qlp_", "MinresQlpWorkspace"):
        assert hasattr(K, name), name
    for sym in MINRES_QLP_SYMBOLS:
        assert sym in K.SIGNATURES, sym
        assert hasattr(K.lib(), sym), sym
    assert K._INPLACE[K.MinresQlpWorkspace] == ("minres_qlp", K.minres_qlp_)
    assert "minres_qlp" not in K.WORKSPACE_KWARGS and K._workspace_kwargs("minres_qlp") == {}
    assert K.MinresQlpWorkspace.VECTORS == CORE
    assert len(K.SIGNATURES["khip_minres_qlp_workspace_adopt"][1]) == 3 + 6 + 1
    assert [f[0] for f in K.CMinresQlpParams._fields_] == ["lambda_", "Artol"]
    prm = K.lib().khip_minres_qlp_default_params()
    assert prm.lambda_ == 0.0 and math.isnan(prm.Artol)


def test_header_declares_the_minres_qlp_entries():
    """include/krylov_hip.h: every entry once, adopt with the six core vectors in the order of the workspace table, the parameter
    struct's fields in the mirror's order, the statuses, the ABI version untouched."""
    header = open(os.path.join(ROOT, "include", "krylov_hip.h"), encoding="utf-8").read()
    for sym in MINRES_QLP_SYMBOLS:
        assert len(re.findall(r"^[\w ]+\*?" + sym + r"\(", header, flags=re.M)) == 1, sym
    adopt = re.search(r"int khip_minres_qlp_workspace_adopt\(khip_ctx \*ctx, int64_t m, int64_t n, (.*?),\s*"
                      r"khip_minres_qlp_workspace \*\*out\);", header, flags=re.S)
    assert adopt and tuple(re.findall(r"double \*(\w+)", adopt.group(1))) == CORE
    struct = re.search(r"typedef struct \{([^{}]*?)\} khip_minres_qlp_params;", header, flags=re.S).group(1)
    struct = re.sub(r"/\*.*?\*/", "", struct, flags=re.S)
    assert re.findall(r"(double|int) (\w+);", struct) == [("double", "lambda"), ("double", "Artol")]
    solve = re.search(r"int khip_minres_qlp_solve\((.*?)\);", header, flags=re.S).group(1)
    assert re.findall(r"\*(\w+)(?:,|$)", solve) == ["ws", "A", "M", "b", "opts", "params"]
    assert '"x", "wkm1", "wk", "Mvkm1", "Mvk", "p", "dx", "vk"' in header
    assert "#define KHIP_VERSION_MINOR 4" in header
    for status in (mr.INCONSISTENT, mr.ZERO_RESID, mr.SOLVED):
        assert status in header
    source = open(os.path.join(ROOT, "krylov.jl_amd", "csrc", "minres_qlp.cpp"), encoding="utf-8").read()
    for status in (mr.ZERO_RESIDUAL, mr.TIRED, mr.ILL_COND_MACH, mr.INCONSISTENT, mr.ZERO_RESID, mr.SOLVED, mr.USER_EXIT, mr.OVERTIMED):
        assert f'"{status}"' in source, status
    table = re.search(r"constexpr WsVec<W> kVectors\[\] = \{(.*?)\};", source, flags=re.S).group(1)
    assert re.findall(r'\{"(\w+)", &W::\w+, (Core|Lazy)\}', table) == [(k, "Core") for k in CORE] + [("dx", "Lazy"), ("vk", "Lazy")]
    assert "minres_qlp.cpp" in open(os.path.join(ROOT, "krylov.jl_amd", "build.sh")).read()


@ref_tree
def test_forwarded_defaults_equal_the_reference():
    """FORWARDED_DEFAULTS["minres_qlp"] = kwargs_minres_qlp / def_kwargs_minres_qlp of src/minres_qlp.jl, names in order, defaults as
    values; the statuses of the restatement are the reference's."""
    import krylov_jl_amd as K
    src = open(os.path.join(REFERENCE_SRC, "minres_qlp.jl"), encoding="utf-8").read()
    names = re.findall(r":(\w+)", re.search(r"^kwargs_minres_qlp = \((.*?)\)", src, flags=re.M).group(1))
    table = re.search(r"^def_kwargs_minres_qlp = \((.*?)\)\n\n", src, flags=re.M | re.S).group(1)
    defaults = {m.group(1): m.group(2) for m in
                re.finditer(r":\(;\s*(\w+)(?:::[^=]+?)?\s*=\s*(.*?)\s*\)\s*[,)]?\s*$", table, flags=re.M)}
    assert list(defaults) == names
    mine = K.FORWARDED_DEFAULTS["minres_qlp"]
    assert list(mine) == names
    sq = math.sqrt(np.finfo(np.float64).eps)
    value = {"I": None, "false": False, "true": True, "zero(T)": 0.0, "√eps(T)": sq, "0": 0, "Inf": math.inf, "kstdout": None}
    for k, expr in defaults.items():
        if k == "callback":
            assert expr == "workspace -> false" and mine[k] is K.default_callback
        else:
            assert mine[k] == value[expr] and type(mine[k]) is type(value[expr]), (k, expr, mine[k])
    import inspect
    sig = inspect.signature(mr.minres_qlp).parameters
    for k, mk in (("lam", "λ"), ("atol", "atol"), ("rtol", "rtol"), ("Artol", "Artol"), ("itmax", "itmax"), ("timemax", "timemax")):
        assert sig[k].default == mine[mk], k
    for status in (mr.ZERO_RESIDUAL, mr.TIRED, mr.ILL_COND_MACH, mr.INCONSISTENT, mr.ZERO_RESID, mr.SOLVED, mr.USER_EXIT, mr.OVERTIMED):
        assert f'"{status}"' in src, status
    assert "btol = eps(T)^(3/4)" in src
    ws_src = open(os.path.join(REFERENCE_SRC, "krylov_workspaces.jl"), encoding="utf-8").read()
    struct = re.search(r"mutable struct MinresQlpWorkspace\{T,FC,S\}.*?\nend", ws_src, flags=re.S).group(0)
    assert re.findall(r"^\s+(\S+)\s+::\s+S$", struct, flags=re.M) == ["Δx", "wₖ₋₁", "wₖ", "M⁻¹vₖ₋₁", "M⁻¹vₖ", "npc_dir", "x", "p", "vₖ"]


# ---- the Julia glue, as text -----------------------------------------------------------------------------------------------------
def _julia_minres_qlp():
    glue = open(JULIA_SRC, encoding="utf-8").read()
    m = re.search(r"function Krylov\.minres_qlp!\(ws::MinresQlpWs, A::HIPCsr, b::HIPVector;(.*?)\)\n(.*?)\nend\n", glue, flags=re.S)
    assert m, "no specialised Krylov.minres_qlp!"
    return glue, m.group(1), m.group(2)


def test_julia_minres_qlp_specialisation_shape():
    """The Julia minres_qlp!: the MinresQlpWs alias, the six adopted vectors in the order of khip_minres_qlp_workspace_adopt, the
    lazy vectors handed over by name, the fallback gate (linesearch among it), the forwarded default callback, LAST_PATH, the
    parameter struct in the header's order, both extra histories, and test/minres_qlp.jl reached from runtests.jl."""
    glue, sig, body = _julia_minres_qlp()
    assert "const MinresQlpWs = MinresQlpWorkspace{Float64,Float64,HIPVector}" in glue
    adopt = re.search(r"ccall\(\(:khip_minres_qlp_workspace_adopt, lib\), Cint,\s*\((.*?)\),\n\s+CTX\[\]\.h, ws\.m, ws\.n, (.*?), r\)\)", glue,
                      flags=re.S)
    assert adopt, "minres_qlp_handle does not adopt the workspace's vectors"
    assert adopt.group(1).count("Ptr{Cdouble}") == 6
    assert [a.strip() for a in adopt.group(2).split(",")] == [f"ws.{f}.ptr" for f in ("x", "wₖ₋₁", "wₖ", "M⁻¹vₖ₋₁", "M⁻¹vₖ", "p")]
    assert re.search(r"struct MinresQlpParams[^\n]*\n\s+lambda::Cdouble; Artol::Cdouble\nend", glue)
    assert "MinresQlpParams(λ, Artol)" in body
    assert 'for (name, v) in (("vk", ws.vₖ), ("dx", ws.Δx))\n    minres_qlp_adopt(h, name, v)' in body
    assert "if ldiv || linesearch || !native_precond(M) || !native_log(verbose, iostream)" in body
    assert "invoke(Krylov.minres_qlp!, Tuple{MinresQlpWs,Any,AbstractVector{Float64}}, ws, A, b;" in body
    assert "callback = callback === nothing ? (w -> false) : callback" in body
    assert "callback_args(user_callback(callback), ws, sp, history)" in body
    assert "NATIVE_SOLVES[] += 1" in body and "LAST_PATH[] = ccall((:khip_minres_qlp_last_path, lib)" in body
    assert "khip_minres_qlp_warm_start" in body and "ws.warm_start = false" in body
    assert "khip_minres_qlp_histories" in body and "ws.stats.Aresiduals" in body and "ws.stats.Acond" in body
    assert "callback = nothing" in sig and "fused::Int = 2" in sig
    assert ("ccall((:khip_minres_qlp_solve, lib), Cint,\n" in body and
            "(Ptr{Cvoid}, Ref{Operator}, Ptr{Operator}, Ptr{Cdouble}, Ref{Options}, Ptr{Cvoid})" in body)
    tests = os.path.join(ROOT, "julia", "KrylovHIP", "test")
    qlp_jl = open(os.path.join(tests, "minres_qlp.jl"), encoding="utf-8").read()
    for piece in ("MinresQlpWorkspace(n, n, S)", "native(2) do; minres_qlp!(ws, A_gpu, b; history = true); end",
                  "generic_minres_qlp(ws2, A_gpu, b;", "MINRES-QLP: system of size $n", "stats.inconsistent", "Artol = "):
        assert piece in qlp_jl, piece
    runtests = open(os.path.join(tests, "runtests.jl"), encoding="utf-8").read()
    assert 'include("minres_qlp.jl")' in runtests


@ref_tree
def test_julia_minres_qlp_specialisation():
    """Against the reference tree: every keyword of kwargs_minres_qlp is in the signature and forwarded to the generic method, and
    the glue reads only fields of MinresQlpWorkspace (src/krylov_workspaces.jl:713-727), all eight vectors among them."""
    glue, sig, body = _julia_minres_qlp()
    src = open(os.path.join(REFERENCE_SRC, "minres_qlp.jl"), encoding="utf-8").read()
    names = re.findall(r":(\w+)", re.search(r"^kwargs_minres_qlp = \((.*?)\)", src, flags=re.M).group(1))
    fallback = re.search(r"invoke\(Krylov\.minres_qlp!, Tuple\{MinresQlpWs,Any,AbstractVector\{Float64\}\}, ws, A, b;(.*?)\)\n  end", body,
                         flags=re.S).group(1)
    for kw in names:
        assert re.search(r"(?<![\w])" + kw + r"(?![\w])", sig), f"minres_qlp!: keyword {kw} of the reference is missing"
        assert re.search(r"(?<![\w])" + kw + r"(?![\w])", fallback), f"minres_qlp!: keyword {kw} is not forwarded to the generic method"
    ws_src = open(os.path.join(REFERENCE_SRC, "krylov_workspaces.jl"), encoding="utf-8").read()
    struct = re.search(r"mutable struct MinresQlpWorkspace\{T,FC,S\}.*?\nend", ws_src, flags=re.S).group(0)
    fields = set(re.findall(r"^\s+(\S+)\s+::", struct, flags=re.M))
    used = set(re.findall(r"\bws\.([^\s.,;()\[\]]+)", body))
    handle = re.search(r"function minres_qlp_handle\(ws::MinresQlpWs\)\n(.*?)\nend\n", glue, flags=re.S).group(1)
    used |= set(re.findall(r"\bws\.([^\s.,;()\[\]]+)", handle))
    assert used <= fields, used - fields
    assert {"x", "wₖ₋₁", "wₖ", "M⁻¹vₖ₋₁", "M⁻¹vₖ", "p", "Δx", "vₖ"} <= used
