"""The case table of cg!, gmres! and bicgstab! at tiny shapes and on every ending, and the judge that compares two runs of a case.

Host only (NumPy): tests/test_first_solvers_cases_host.py pins the table on the CPU oracle, tests/test_gpu_first_solvers_cases.py
runs it on the three loops of the device.  The builders restate the reference's test/test_utils.jl (lines cited per builder) in
Float64; dense matrices become CSR with every entry stored, the banded ones keep their band (explicit zeros included).

A case is (operator kind, size, solver keywords, the ending it is named for, the loop `fused = 2` is expected to reach and why).
"""
import math

import numpy as np

EPS = float(np.finfo(float).eps)
# the project's tolerance for these three solvers (tests/test_gpu_solvers.py): |Δr_k| <= 1e-10 r_k + 100 eps r_0, x within 1e-9 max|x|
TOL = dict(rtol=1e-10, floor=100 * EPS, x=1e-9)
PARITY_CAP = 1e-6            # a case is in the history-parity list when the oracle's own two dot modes agree this well ...
PARITY_FLOOR = 1e-12         # ... on the entries above this fraction of the first one
PARITY_SHARE = 0.9           # at least this share of every solver's cases must qualify
RESID_TOL = 1e-6             # cg_tol = gmres_tol = bicgstab_tol of the reference's tests

SOLVED = "solution good enough given atol and rtol"
TIRED = "maximum number of iterations exceeded"
LSQ = "found approximate least-squares solution"
BREAKDOWN = "breakdown αₖ == 0"
BREAKDOWN_BC = "Breakdown bᴴc = 0"
ZERO_CURVATURE = "zero curvature detected"
NPC = "nonpositive curvature"
BOUNDARY = "on trust-region boundary"
SOLVERS = ("cg", "gmres", "bicgstab")


# ---- builders: (dense A, band or None, b, c or None); band = k keeps the entries with |i - j| <= k ------------------------------
def _tridiag(n, lo, di, up):
    return di * np.eye(n) + lo * np.eye(n, k=-1) + up * np.eye(n, k=1)


def _one_to(n):
    return np.arange(1.0, n + 1.0)


def symmetric_definite(n=10):
    """test/test_utils.jl:18-23: spdiagm(-1 => 1, 0 => 4, 1 => 1), b = A * [1:n;]."""
    A = _tridiag(n, 1.0, 4.0, 1.0)
    return A, 1, A @ _one_to(n), None


def symmetric_indefinite(n=10, shift=0):
    """test/test_utils.jl:26-31: spdiagm(-1 => 1, 0 => 1, 1 => 1) - shift * I, b = A * [1:n;]."""
    A = _tridiag(n, 1.0, 1.0, 1.0) - shift * np.eye(n)
    return A, 1, A @ _one_to(n), None


def nonsymmetric_definite(n=10):
    """test/test_utils.jl:72-80: n on the diagonal, 1 above it, -1 below it (dense), b = A * [1:n;]."""
    A = np.triu(np.ones((n, n)), 1) - np.tril(np.ones((n, n)), -1) + n * np.eye(n)
    return A, None, A @ _one_to(n), None


def nonsymmetric_indefinite(n=10):
    """test/test_utils.jl:83-91: as nonsymmetric_definite with the diagonal n * (-1)^(i * i), i = 1 ... n."""
    i = np.arange(1, n + 1)
    A = np.triu(np.ones((n, n)), 1) - np.tril(np.ones((n, n)), -1) + np.diag(n * (-1.0) ** (i * i))
    return A, None, A @ _one_to(n), None


def square_inconsistent(n=10):
    """test/test_utils.jl:120-125: Diagonal(ones(n)) with A[1, 1] = 0 (a stored zero), b = ones."""
    A = np.eye(n)
    A[0, 0] = 0.0
    return A, 0, np.ones(n), None


def symmetric_inconsistent():
    """test/test_utils.jl:128-132."""
    A = np.array([[3.0, 2.0, -1.0, 5.0], [2.0, -2.0, 4.0, 0.0], [-1.0, 4.0, 1.0, 3.0], [5.0, 0.0, 3.0, 5.0]])
    return A, None, np.array([1.0, -8.0, 5.0, 2.0]), None


def singular_consistent(n=10):
    """test/test_utils.jl:180-185: [i * j] + 5 I, then the first two rows and columns set to one; b = A * ones."""
    i = _one_to(n)
    A = np.outer(i, i) + 5.0 * np.eye(n)
    A[0, :] = 1.0
    A[1, :] = 1.0
    A[:, 1] = 1.0
    A[:, 0] = 1.0
    return A, None, A @ np.ones(n), None


def bc_breakdown():
    """test/test_utils.jl:204-209: bᴴc = 0."""
    return np.array([[1.0, 2.0], [3.0, 4.0]]), None, np.array([0.0, 1.0]), np.array([1.0, 0.0])


def identity(n=10):
    """A = I, b = 1:n: the Krylov space has dimension one."""
    return np.eye(n), 0, _one_to(n), None


def diag3(n):
    """Diagonal 1, 2, 3 repeating, b = ones: three distinct eigenvalues, so the Krylov space is exhausted at k = 3."""
    return np.diag(1.0 + np.arange(n) % 3), 0, np.ones(n), None


def rotation():
    """[[0, 1], [-1, 0]], b = e₁: c·v = 0 in bicgstab's first iteration (α = ∞ before it is NaN)."""
    return np.array([[0.0, 1.0], [-1.0, 0.0]]), None, np.array([1.0, 0.0]), None


def diag_pm():
    """diag(1, -1), b = (1, 1): pᵀAp = 0 at iteration 0."""
    return np.diag([1.0, -1.0]), 0, np.ones(2), None


def diag_21m():
    """diag(2, 1, -1), b = ones: negative curvature after one step."""
    return np.diag([2.0, 1.0, -1.0]), 0, np.ones(3), None


def diag_npc4(last=-1.0):
    """test/test_cg.jl:83-89 (last = -1, b[4] = 0.1) and :157-163 (last = 1, b = ones): diag(10, 8, 5, last)."""
    return np.diag([10.0, 8.0, 5.0, last]), 0, np.array([1.0, 1.0, 1.0, 0.1 if last < 0 else 1.0]), None


_BUILDERS = {"sd": symmetric_definite, "si": symmetric_indefinite, "nd": nonsymmetric_definite, "ni": nonsymmetric_indefinite,
             "sq_inc": square_inconsistent, "sym_inc": symmetric_inconsistent, "sing": singular_consistent, "bc": bc_breakdown,
             "eye": identity, "diag3": diag3, "rot": rotation, "diag_pm": diag_pm, "diag_21m": diag_21m, "npc4": diag_npc4}


class System:
    """One linear system: .A dense (for the checks made in NumPy), .rowptr / .col / .val its CSR form, .b, .c (or None)."""

    def __init__(self, A, rowptr, col, val, b, c):
        self.A, self.rowptr, self.col, self.val, self.b, self.c = A, rowptr, col, val, b, c
        self.n = len(b)
        self._csr = None

    def csr(self, oracle):
        if self._csr is None:
            self._csr = oracle.CsrMatrix.from_arrays(self.rowptr, self.col, self.val)
        return self._csr


_SYSTEMS = {}


def system(oracle, op):
    """op = (kind, *arguments), built once.  "poisson" and "kron" are the oracle's own generators (b = ones and A * ones)."""
    if op not in _SYSTEMS:
        kind, args = op[0], op[1:]
        if kind in ("poisson", "kron"):
            M = oracle.poisson3d(*args) if kind == "poisson" else oracle.kron_unsymmetric(*args)
            rowptr, col, val = M.rowptr.copy(), M.col.copy(), M.val.copy()
            A = M.to_scipy().toarray()
            b = np.ones(M.n) if kind == "poisson" else A @ np.ones(M.n)
            c = None
        else:
            A, band, b, c = _BUILDERS[kind](*args)
            n = len(b)
            i, j = np.indices((n, n))
            keep = np.ones((n, n), dtype=bool) if band is None else np.abs(i - j) <= band
            rowptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
            col = j[keep].astype(np.int32)                   # row-major order of the mask = CSR order
            val = A[keep].astype(np.float64)
        _SYSTEMS[op] = System(A, rowptr, col, val, np.asarray(b, dtype=np.float64), c)
    return _SYSTEMS[op]


# ---- the table ------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, op, kw=None, ending=SOLVED, path2=2, why="", boundary=False, c_ones=False):
        self.op, self.kw, self.ending = op, dict(kw or {}), ending
        self.c_ones = c_ones                       # bicgstab!: c = ones instead of c = b
        self.path2, self.why = path2, why          # the loop `fused = 2` reaches, and why when it is not 2
        self.boundary = boundary                   # the reference asserts |radius - ‖x‖| <= cg_tol radius (test/test_cg.jl:16-19)


SIZES = (1, 2, 3, 10, 63, 64, 65)
_GATE_CG = "cg!'s device loop has no trust region and no linesearch (the gate of csrc/solvers.cpp): the host-driven loop runs"
_GATE_REORTH = "gmres!'s look-ahead loop excludes reorthogonalization (the gate of csrc/solvers.cpp): the host-driven loop runs"
_GATE_BC = "bicgstab! returns on bᴴc = 0 before it chooses a loop (csrc/solvers.cpp): a fresh workspace keeps last_path = -1"


def _cg_cases():
    t = {f"sd{n}": Case(("sd", n)) for n in SIZES}
    t["poisson9"] = Case(("poisson", 9))
    t["sq_inc10"] = Case(("sq_inc", 10), ending=ZERO_CURVATURE)                                  # test/test_cg.jl:106-111
    t["sing10"] = Case(("sing", 10))                                                             # :98-104
    # niter = 0, yet the device-resident loop does launch: r₀ is not small, so its first pass forms pᵀAp and stops there.  (cg! sets
    # last_path before it tests `solved || tired`, csrc/solvers.cpp: only a solve that is over at r₀ would report 2 without a launch,
    # and the table has none.)
    t["diag_pm"] = Case(("diag_pm",), ending=ZERO_CURVATURE)
    t["diag_pm_radius2"] = Case(("diag_pm",), dict(radius=2.0), NPC, 1, _GATE_CG)
    t["diag_21m_linesearch"] = Case(("diag_21m",), dict(linesearch=True), NPC, 1, _GATE_CG)
    t["diag_21m_radius5"] = Case(("diag_21m",), dict(radius=5.0), NPC, 1, _GATE_CG)
    t["si10_shift5_radius1"] = Case(("si", 10, 5), dict(radius=1.0), NPC, 1, _GATE_CG)
    t["si10_shift5_radius100"] = Case(("si", 10, 5), dict(radius=100.0), NPC, 1, _GATE_CG)
    t["si10_shift5_linesearch"] = Case(("si", 10, 5), dict(linesearch=True), NPC, 1, _GATE_CG)
    t["si10_shift10_linesearch"] = Case(("si", 10, 10), dict(linesearch=True), NPC, 1, _GATE_CG)   # :51-62
    t["npc4_radius10"] = Case(("npc4",), dict(radius=10.0), NPC, 1, _GATE_CG)                     # :82-96
    t["npc4_linesearch"] = Case(("npc4",), dict(linesearch=True), NPC, 1, _GATE_CG)               # :136-153
    t["sd65_itmax3"] = Case(("sd", 65), dict(itmax=3), TIRED)
    t["sd10_radius"] = Case(("sd", 10), dict(radius=0.75 * math.sqrt(385.0), itmax=10), BOUNDARY, 1, _GATE_CG, boundary=True)   # :15-20
    return t


# gmres! with memory ∈ {1, 2, n, 20} x restart ∈ {false, true}, and the same again with reorthogonalization
GMRES_CROSS = (("nd", 3), ("nd", 9), ("nd", 65), ("diag3", 65), ("diag3", 729), ("sq_inc", 10))


def _gmres_cases():
    t = {}
    for fam in ("sd", "si", "nd", "ni"):
        for n in SIZES:
            t[f"{fam}{n}"] = Case((fam, n))
    t["poisson9"] = Case(("poisson", 9))
    t["kron7"] = Case(("kron", 7))
    t["eye10"] = Case(("eye", 10))                                           # breakdown Hbis <= btol at k = 1
    t["diag3_65"] = Case(("diag3", 65))                                      # breakdown at k = 3
    t["diag3_729"] = Case(("diag3", 729))
    t["diag3_65_m2_restart"] = Case(("diag3", 65), dict(memory=2, restart=True))     # the breakdown never falls inside a cycle of 2
    t["diag3_729_m2_restart"] = Case(("diag3", 729), dict(memory=2, restart=True))
    t["diag3_65_m5_restart"] = Case(("diag3", 65), dict(memory=5, restart=True))     # the breakdown inside a restart cycle
    t["sq_inc10"] = Case(("sq_inc", 10), ending=LSQ)                         # test/test_gmres.jl:47-53
    t["sq_inc10_m3_restart"] = Case(("sq_inc", 10), dict(memory=3, restart=True), LSQ)
    t["sym_inc"] = Case(("sym_inc",), ending=LSQ)
    t["nd5_m20"] = Case(("nd", 5), dict(memory=20))                          # n < memory
    t["nd9_m1"] = Case(("nd", 9), dict(memory=1))
    t["nd9_m1_restart"] = Case(("nd", 9), dict(memory=1, restart=True), TIRED)
    for kind, n in GMRES_CROSS:
        for mem in (1, 2, n, 20):
            for restart in (False, True):
                for reorth in (False, True):
                    name = f"x_{kind}{n}_m{mem}" + ("_restart" if restart else "") + ("_reorth" if reorth else "")
                    kw = dict(memory=mem, restart=restart)
                    if reorth:
                        kw["reorthogonalization"] = True
                    # the inconsistent operator ends in the least-squares status whatever the memory; the others end as the oracle says
                    t[name] = Case((kind, n), kw, LSQ if kind == "sq_inc" else None, 1 if reorth else 2, _GATE_REORTH if reorth else "")
    return t


def _bicgstab_cases():
    t = {}
    for fam in ("sd", "si", "nd", "ni"):
        for n in SIZES:
            t[f"{fam}{n}"] = Case((fam, n))
    for name in ("sd1", "si1", "nd1", "ni1", "si2"):                        # every n = 1 system and symmetric_indefinite(2)
        t[name].ending = BREAKDOWN
    t["poisson9"] = Case(("poisson", 9))
    t["kron7"] = Case(("kron", 7))
    t["eye10"] = Case(("eye", 10), ending=BREAKDOWN)
    t["sq_inc10"] = Case(("sq_inc", 10), ending=BREAKDOWN)
    t["rot"] = Case(("rot",), ending=BREAKDOWN)
    t["diag_pm"] = Case(("diag_pm",), ending=BREAKDOWN)
    t["bc"] = Case(("bc",), ending=BREAKDOWN_BC, path2=-1, why=_GATE_BC)
    # bicgstab!'s α and ω are ratios of cancelling dots: on symmetric_indefinite and nonsymmetric_indefinite at n = 63, 64, 65 the
    # oracle's own two dot modes end at different iterations (tests/test_first_solvers_cases_host.py), so those six serve the
    # loop-against-loop checks and the true residual only.  The further cases below keep the parity list at PARITY_SHARE of the
    # table with sizes and keywords the families above do not reach: n = 4, 5, 9, half a wave and its neighbours, c != b, a
    # tighter tolerance, itmax, an exhausted Krylov space and the singular systems.
    for fam, sizes in (("sd", (4, 5, 9, 31, 32, 33)), ("nd", (4, 5, 9, 31, 32, 33)), ("si", (4, 5, 9)), ("ni", (4, 5, 9))):
        for n in sizes:
            t[f"{fam}{n}"] = Case((fam, n))
    for fam, sizes in (("sd", (2, 3, 10, 65)), ("nd", (2, 3, 10, 65)), ("si", (2, 3)), ("ni", (2, 3, 10, 65))):
        for n in sizes:
            t[f"{fam}{n}_c_ones"] = Case((fam, n), c_ones=True)
    t["si2_c_ones"].ending = t["ni2_c_ones"].ending = BREAKDOWN
    for name, op in (("sd65", ("sd", 65)), ("nd65", ("nd", 65)), ("poisson9", ("poisson", 9)), ("kron7", ("kron", 7))):
        t[name + "_rtol12"] = Case(op, dict(atol=0.0, rtol=1e-12))
        t[name + "_itmax3"] = Case(op, dict(itmax=3), TIRED)
    t["diag3_65"] = Case(("diag3", 65))
    t["diag3_729"] = Case(("diag3", 729))
    t["sing10"] = Case(("sing", 10))
    t["sym_inc"] = Case(("sym_inc",), ending=TIRED)
    t["diag_21m"] = Case(("diag_21m",))
    t["npc4"] = Case(("npc4",))
    return t


CASES = {"cg": _cg_cases(), "gmres": _gmres_cases(), "bicgstab": _bicgstab_cases()}
# the cases named for an ending other than "solved": every test that runs a subset runs these
ENDING_CASES = {s: tuple(n for n, c in CASES[s].items() if c.ending not in (SOLVED, None)) + (("eye10", "diag3_65", "diag3_729",
                "diag3_65_m5_restart") if s == "gmres" else ()) for s in SOLVERS}


def case_ids(solver=None):
    return [(s, n) for s in (SOLVERS if solver is None else (solver,)) for n in CASES[s]]


def solver_kwargs(solver, name):
    """The keywords of a case as the oracle and the device entry points both take them (c is apart: case_c)."""
    kw = dict(CASES[solver][name].kw)
    if solver == "gmres":
        kw.setdefault("memory", 20)
    return kw


def case_c(S, case):
    """bicgstab!'s c of a case as a host vector, or None for c = b."""
    return np.ones(S.n) if case.c_ones else S.c


# ---- oracle runs ----------------------------------------------------------------------------------------------------------------
_RUNS = {}


def oracle_run(oracle, solver, name, dot_mode=0):
    """The oracle's result of a case (history on), computed once per dot mode: 0 = the documented sequential extended-precision
    dots, 1 = Dot2."""
    key = (solver, name, dot_mode)
    if key not in _RUNS:
        case = CASES[solver][name]
        S = system(oracle, case.op)
        kw = solver_kwargs(solver, name)
        if solver == "bicgstab" and case_c(S, case) is not None:
            kw["c"] = case_c(S, case)
        L = oracle.lib()
        L.ko_set_dot_mode(dot_mode)
        try:
            _RUNS[key] = getattr(oracle, solver)(S.csr(oracle), S.b, history=True, **kw)
        finally:
            L.ko_set_dot_mode(0)
    return _RUNS[key]


def flags(solver, r):
    """Everything but the numbers: niter, status and the flags (cg! also reports indefinite and npcCount)."""
    f = (r.niter, r.status, bool(r.solved), bool(r.inconsistent))
    return f + ((bool(r.indefinite), r.npcCount) if solver == "cg" else ())


def history_deviation(a, b):
    """Largest relative difference of two histories on the finite entries above PARITY_FLOOR of the first; inf when the lengths
    or the places of the non-finite entries differ."""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    if a.shape != b.shape or not np.array_equal(np.isfinite(a), np.isfinite(b)):
        return math.inf
    m = np.isfinite(b)
    if len(b) and math.isfinite(b[0]):
        m &= np.abs(b) > PARITY_FLOOR * abs(b[0])
    if not m.any():
        return 0.0
    return float(np.max(np.abs(a[m] - b[m]) / np.abs(b[m])))


def qualifies(oracle, solver, name):
    """(in the history-parity list?, the oracle's own deviation between its two dot modes).  The rule of
    tests/test_symmlq_host.py::test_parity_list_condition: the same niter, status and flags under both modes, histories within
    PARITY_CAP of each other."""
    r0, r1 = oracle_run(oracle, solver, name, 0), oracle_run(oracle, solver, name, 1)
    if flags(solver, r0) != flags(solver, r1):
        return False, math.inf
    dev = history_deviation(r1.residuals, r0.residuals)
    return dev <= PARITY_CAP, dev


# ---- the judge ------------------------------------------------------------------------------------------------------------------
class Mismatch(AssertionError):
    pass


def judge(got, want, tol=TOL, solver="cg", x=None, x_want=None):
    """`got` against `want` (objects with niter, status, solved, inconsistent, indefinite, npcCount, residuals), in this order:
    the shape of the history; niter, status and the flags; non-finite history entries exactly where `want` has them (the class
    is not compared: a compensated and a plain dot may give Inf against NaN after one overflow, tests/test_gpu_reduction_exact.py);
    the finite entries within |Δr_k| <= tol.rtol r_k + tol.floor r_0; and, when both are given, x within tol.x max|x_want| with
    non-finite entries in the same places.  Raises Mismatch; returns the largest deviation in units of the tolerance."""
    h, hw = np.asarray(got.residuals, dtype=float), np.asarray(want.residuals, dtype=float)
    if h.shape != hw.shape:
        raise Mismatch(f"history of {h.shape} entries, expected {hw.shape}")
    if flags(solver, got) != flags(solver, want):
        raise Mismatch(f"(niter, status, solved, inconsistent[, indefinite, npcCount]) = {flags(solver, got)}, expected {flags(solver, want)}")
    fin, finw = np.isfinite(h), np.isfinite(hw)
    if not np.array_equal(fin, finw):
        raise Mismatch(f"non-finite history entries at {np.flatnonzero(~fin).tolist()}, expected at {np.flatnonzero(~finw).tolist()}")
    units = 0.0
    if finw.any():
        r0 = abs(hw[0]) if math.isfinite(hw[0]) else 0.0
        bound = tol["rtol"] * np.abs(hw[finw]) + tol["floor"] * r0
        d = np.abs(h[finw] - hw[finw])
        bad = d > bound
        if bad.any():
            k = int(np.flatnonzero(finw)[np.argmax(bad)])
            raise Mismatch(f"history entry {k}: {h[k]!r} against {hw[k]!r}, allowed {tol['rtol']:.1e} r_k + {tol['floor']:.1e} r_0")
        with np.errstate(divide="ignore", invalid="ignore"):
            units = float(np.max(np.where(bound > 0, d / bound, 0.0)))
    if x is not None and x_want is not None:
        x, x_want = np.asarray(x, dtype=float), np.asarray(x_want, dtype=float)
        if x.shape != x_want.shape or not np.array_equal(np.isfinite(x), np.isfinite(x_want)):
            raise Mismatch("x: shape or the places of its non-finite entries differ")
        m = np.isfinite(x_want)
        if m.any():
            scale = float(np.abs(x_want[m]).max())
            d = float(np.abs(x[m] - x_want[m]).max())
            if d > tol["x"] * scale:
                raise Mismatch(f"x: largest deviation {d:.3e}, allowed {tol['x']:.1e} x {scale:.3e}")
            if scale > 0:
                units = max(units, d / (tol["x"] * scale))
    return units


def fsum_residual(S, x):
    """‖b - A x‖ with every row's sum formed exactly (math.fsum over the stored entries and b_i)."""
    r = [math.fsum([S.b[i]] + [-S.val[k] * x[S.col[k]] for k in range(S.rowptr[i], S.rowptr[i + 1])]) for i in range(S.n)]
    return math.sqrt(math.fsum(v * v for v in r))


class Record:
    """A run's flags, history and x as plain data (a copy: the judge's own tests perturb it)."""
    FIELDS = ("niter", "status", "solved", "inconsistent", "indefinite", "npcCount")

    def __init__(self, stats, x=None, **more):
        for k in self.FIELDS:
            setattr(self, k, getattr(stats, k))
        self.residuals = np.array(stats.residuals, dtype=float)
        x = getattr(stats, "x", None) if x is None else x
        self.x = None if x is None else np.array(x, dtype=float)
        self.__dict__.update(more)
