"""The case table of tests/first_solvers_cases.py without a GPU: every case reaches the ending it is named for on the CPU oracle;
the oracle itself is pinned on those endings by facts it does not compute (true residuals formed with math.fsum, the normal
equations and numpy.linalg.lstsq for the least-squares endings, the reference's own assertions of test/test_cg.jl and
test/test_gmres.jl for the curvature endings); the history-parity list and its 90 % condition hold; and the judge rejects what it
must."""
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import first_solvers_cases as fc  # noqa: E402
from first_solvers_cases import (BOUNDARY, BREAKDOWN, BREAKDOWN_BC, CASES, LSQ, NPC, SOLVED, SOLVERS, TIRED, TOL, ZERO_CURVATURE,  # noqa: E402
                                 Mismatch, Record, judge, oracle_run, qualifies, system)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORDED = json.load(open(os.path.join(ROOT, "tests", "golden", "first_solvers_cases_expected.json"), encoding="utf-8"))
SQRT_EPS = math.sqrt(fc.EPS)                     # the default atol and rtol of the three solvers

# The endings the table is named for, typed from the oracle's results as the table was drawn up: (niter, status, inconsistent).
EXPECTED = {
    "gmres": {
        "eye10": (1, SOLVED, False), "diag3_65": (3, SOLVED, False), "diag3_729": (3, SOLVED, False),
        "diag3_65_m2_restart": (18, SOLVED, False), "diag3_729_m2_restart": (18, SOLVED, False),
        "diag3_65_m5_restart": (3, SOLVED, False),
        "sq_inc10": (2, LSQ, True), "sq_inc10_m3_restart": (2, LSQ, True), "sym_inc": (4, LSQ, True),
        "nd5_m20": (5, SOLVED, False), "nd9_m1": (8, SOLVED, False), "nd9_m1_restart": (18, TIRED, False),
        "sd1": (1, SOLVED, False), "sd2": (2, SOLVED, False), "sd3": (3, SOLVED, False), "sd63": (12, SOLVED, False),
        "sd64": (12, SOLVED, False), "sd65": (12, SOLVED, False),
    },
    "bicgstab": {
        "eye10": (2, BREAKDOWN, False), "sd1": (2, BREAKDOWN, False), "si1": (2, BREAKDOWN, False), "nd1": (2, BREAKDOWN, False),
        "ni1": (2, BREAKDOWN, False), "si2": (2, BREAKDOWN, False), "sq_inc10": (3, BREAKDOWN, False), "rot": (2, BREAKDOWN, False),
        "bc": (0, BREAKDOWN_BC, False),
        "sd2": (2, SOLVED, False), "sd3": (3, SOLVED, False), "sd63": (8, SOLVED, False), "sd64": (8, SOLVED, False),
        "sd65": (8, SOLVED, False),
    },
    "cg": {
        "sq_inc10": (1, ZERO_CURVATURE, True), "sing10": (3, SOLVED, False), "diag_pm": (0, ZERO_CURVATURE, True),
        "diag_pm_radius2": (1, NPC, False), "diag_21m_linesearch": (1, NPC, False), "diag_21m_radius5": (2, NPC, False),
        "si10_shift5_radius1": (1, NPC, False), "si10_shift5_radius100": (1, NPC, False), "si10_shift5_linesearch": (0, NPC, False),
        "si10_shift10_linesearch": (0, NPC, False), "sd10_radius": (1, BOUNDARY, False),
        "sd1": (1, SOLVED, False), "sd2": (2, SOLVED, False), "sd3": (3, SOLVED, False), "sd63": (12, SOLVED, False),
        "sd64": (12, SOLVED, False), "sd65": (12, SOLVED, False),
    },
}
# the histories the table quotes
HISTORIES = {("gmres", "sq_inc10"): [3.1623, 1.0, 0.78209], ("bicgstab", "eye10"): [19.62, math.nan, math.nan],
             ("bicgstab", "sq_inc10"): [3.1623, 1.0, math.nan, math.nan]}
# bicgstab!'s α and ω are ratios of cancelling dots: on these the oracle's two dot modes already end at different iterations
CHAOTIC = {("bicgstab", f"{fam}{n}") for fam in ("si", "ni") for n in (63, 64, 65)}


# ---- 1. every case reaches its ending --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS)
def test_every_case_reaches_its_ending(oracle, solver):
    assert list(RECORDED[solver]) == list(CASES[solver]), "the recorded table and the case table list different cases"
    for name, case in CASES[solver].items():
        r = oracle_run(oracle, solver, name)
        niter, status = RECORDED[solver][name]
        print(f"{solver} {name}: niter {r.niter}, {r.status}, solved {r.solved}, inconsistent {r.inconsistent}")
        assert r.rc == 0 and r.status == status, (name, r.status)
        assert case.ending is None or r.status == case.ending, (name, r.status, case.ending)
        assert (niter is None) == ((solver, name) in CHAOTIC), name
        if niter is not None:
            assert r.niter == niter, (name, r.niter, niter)
        assert len(r.residuals) == r.niter + 1, name
        if name in EXPECTED[solver]:
            assert (r.niter, r.status, r.inconsistent) == EXPECTED[solver][name], name
    for name in EXPECTED[solver]:
        assert name in CASES[solver], name
    for (s, name), want in HISTORIES.items():
        if s == solver:
            h = oracle_run(oracle, s, name).residuals
            assert np.array_equal(np.isnan(h), np.isnan(want)) and np.allclose(h, want, rtol=1e-4, equal_nan=True), (name, h)


def test_gmres_cross_is_complete():
    """memory ∈ {1, 2, n, 20} x restart x reorthogonalization on the six operators of the subset: 96 cases, memory = n among them."""
    cross = [c for n, c in CASES["gmres"].items() if n.startswith("x_")]
    assert len(cross) == 6 * 4 * 2 * 2
    for kind, n in fc.GMRES_CROSS:
        seen = {(c.kw["memory"], c.kw["restart"], bool(c.kw.get("reorthogonalization"))) for c in cross if c.op == (kind, n)}
        assert seen == {(m, r, o) for m in (1, 2, n, 20) for r in (False, True) for o in (False, True)}
    assert all(c.path2 == (1 if c.kw.get("reorthogonalization") else 2) for c in cross)


def test_expected_path_is_explained():
    """Path 2 wherever the gate of csrc/solvers.cpp lets it run; every other expectation says why."""
    for s in SOLVERS:
        for name, c in CASES[s].items():
            gated = (s == "cg" and (c.kw.get("radius", 0.0) > 0 or c.kw.get("linesearch"))) or \
                    (s == "gmres" and c.kw.get("reorthogonalization"))
            if gated:
                assert c.path2 == 1 and c.why, (s, name)
            elif (s, name) == ("bicgstab", "bc"):
                assert c.path2 == -1 and c.why
            else:
                assert c.path2 == 2 and not c.why, (s, name)


# ---- 2. the oracle pinned by facts it does not compute itself ---------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS)
def test_solved_cases_meet_their_tolerance_in_exact_row_sums(oracle, solver):
    """status "solution good enough": ‖b - A x‖ <= atol + rtol ‖b‖ with every row of b - A x summed exactly, on every solved case,
    the six chaotic bicgstab! cases included (the stopping test is made on the recurrence's residual; the true one follows it)."""
    for name, case in CASES[solver].items():
        r = oracle_run(oracle, solver, name)
        if r.status != SOLVED:
            continue
        S = system(oracle, case.op)
        res = fc.fsum_residual(S, r.x)
        nb = float(np.linalg.norm(S.b))
        bound = case.kw.get("atol", SQRT_EPS) + case.kw.get("rtol", SQRT_EPS) * nb
        print(f"{solver} {name}: ||b - A x|| {res:.3e}, bound {bound:.3e}, recurrence {r.residuals[-1]:.3e}")
        assert r.solved
        assert res <= bound, (name, res, bound)


def test_gmres_least_squares_endings(oracle):
    """test/test_gmres.jl:47-53 on every case that ends "found approximate least-squares solution": ‖Aᵀ(b - A x)‖ <= 1e-6, and the
    part of x that A determines (its projection on the row space) is numpy.linalg.lstsq's minimum-norm solution."""
    n_seen = 0
    for name, case in CASES["gmres"].items():
        r = oracle_run(oracle, "gmres", name)
        if r.status != LSQ:
            continue
        n_seen += 1
        S = system(oracle, case.op)
        assert r.inconsistent
        normal = float(np.linalg.norm(S.A.T @ (S.b - S.A @ r.x)))
        xls = np.linalg.lstsq(S.A, S.b, rcond=None)[0]
        proj = np.linalg.pinv(S.A) @ (S.A @ r.x)
        print(f"gmres {name}: ||A'(b - A x)|| {normal:.3e}, row-space part of x against lstsq {np.abs(proj - xls).max():.3e}")
        assert normal <= 1e-6, name
        assert np.abs(proj - xls).max() <= 1e-6 * np.abs(xls).max(), name
        assert np.linalg.norm(S.b - S.A @ r.x) > 0.1                    # and the system is inconsistent indeed
    assert n_seen == 3 + 16


def _oracle_cg_with_npc_dir(oracle, S, **kw):
    """oracle.cg with the workspace kept long enough to read npc_dir."""
    L = oracle.lib()
    ws = L.ko_cg_workspace_create(S.n, S.n)
    o = oracle.make_options(**kw)
    A = S.csr(oracle)
    rc = L.ko_cg(ws, L.csr_matvec, oracle.NULL_MATVEC, A.ptr(), S.b.ctypes.data_as(oracle.c_double_p), C.byref(o))
    st = Record(oracle.Result(None, ws.contents.stats, rc))
    x = np.ctypeslib.as_array(ws.contents.x, shape=(S.n,)).copy()
    d = np.ctypeslib.as_array(ws.contents.npc_dir, shape=(S.n,)).copy()
    L.ko_cg_workspace_free(ws)
    return x, st, d


def test_cg_curvature_endings(oracle):
    """test/test_cg.jl:51-62 (linesearch on symmetric_indefinite(shift = 10)) and :82-96 (radius = 10 on diag(10, 8, 5, -1)) as
    written; the same facts on the table's other npc cases; :98-111 on the singular systems."""
    S = system(oracle, ("si", 10, 10))
    x, st, d = _oracle_cg_with_npc_dir(oracle, S, linesearch=True)
    assert st.status == NPC and not st.inconsistent and st.niter == 0 and st.indefinite and st.npcCount == 1
    assert d @ S.A @ d <= 0 and np.array_equal(d, S.b)
    S = system(oracle, ("npc4",))
    x, st, d = _oracle_cg_with_npc_dir(oracle, S, radius=10.0)
    assert st.npcCount == 1 and st.status == NPC and st.indefinite and d @ S.A @ d <= 0.01
    for name, case in CASES["cg"].items():
        if case.ending != NPC:
            continue
        S = system(oracle, case.op)
        x, st, d = _oracle_cg_with_npc_dir(oracle, S, **case.kw)
        r = oracle_run(oracle, "cg", name)
        assert (st.niter, st.status) == (r.niter, r.status) and np.array_equal(x, r.x)
        assert st.solved and st.indefinite and st.npcCount == 1 and not st.inconsistent, name
        assert d @ S.A @ d <= 0, name
        if "radius" in case.kw:                                        # the step ends on the boundary
            assert abs(np.linalg.norm(x) - case.kw["radius"]) <= 1e-6 * case.kw["radius"], name
    r = oracle_run(oracle, "cg", "sd10_radius")
    radius = CASES["cg"]["sd10_radius"].kw["radius"]
    assert r.solved and abs(radius - np.linalg.norm(r.x)) <= 1e-6 * radius            # :15-20
    r = oracle_run(oracle, "cg", "sing10")                                            # :98-104
    S = system(oracle, ("sing", 10))
    assert fc.fsum_residual(S, r.x) / np.linalg.norm(S.b) <= 1e-6 and not r.inconsistent
    assert np.linalg.matrix_rank(S.A) < 10
    for name in ("sq_inc10", "diag_pm"):                                              # :106-111
        r = oracle_run(oracle, "cg", name)
        assert r.inconsistent and not r.solved and r.status == ZERO_CURVATURE
    # the reset of indefinite / npcCount on a reused workspace (:136-170) is the oracle's reset of its stats at every solve
    L = oracle.lib()
    ws = L.ko_cg_workspace_create(4, 4)
    o = oracle.make_options(linesearch=True)
    for last, want in ((-1.0, (1, True, NPC)), (1.0, (0, False, SOLVED))):
        S = system(oracle, ("npc4", last))
        L.ko_cg(ws, L.csr_matvec, oracle.NULL_MATVEC, S.csr(oracle).ptr(), S.b.ctypes.data_as(oracle.c_double_p), C.byref(o))
        st = oracle.Result(None, ws.contents.stats, 0)
        assert (st.npcCount, st.indefinite, st.status) == want and st.solved
    L.ko_cg_workspace_free(ws)


def test_bicgstab_breakdowns_are_what_they_are_named_for(oracle):
    """α = ρ / (c·v): on the identity (and every n = 1 system) s = r - α v is exactly zero, so ω = 0 / 0 and the next α is NaN; on
    the rotation c·v = 0 and α = ∞ at once.  x before the breakdown of I₁₀ already is the solution."""
    for name in ("eye10", "sd1", "si1", "nd1", "ni1", "si2", "rot", "diag_pm"):
        r = oracle_run(oracle, "bicgstab", name)
        assert r.status == BREAKDOWN and not r.solved and r.niter == 2
        assert np.array_equal(np.isfinite(r.residuals), [True, False, False]), (name, r.residuals)
    r = oracle_run(oracle, "bicgstab", "sq_inc10")
    assert np.array_equal(np.isfinite(r.residuals), [True, True, False, False])
    r = oracle_run(oracle, "bicgstab", "bc")
    assert r.niter == 0 and not r.solved and not r.x.any() and len(r.residuals) == 1


# ---- 3. the history-parity list ---------------------------------------------------------------------------------------------------
def test_parity_list_condition(oracle):
    """A case is in the history-parity list when the oracle with its sequential extended-precision dots and with Dot2 gives the
    same niter, status and flags and histories within 1e-6; exactly the six chaotic bicgstab! cases are out, and at least 90 % of
    every solver's cases are in."""
    out = set()
    for s in SOLVERS:
        n_in = 0
        for name in CASES[s]:
            ok, dev = qualifies(oracle, s, name)
            r0, r1 = oracle_run(oracle, s, name, 0), oracle_run(oracle, s, name, 1)
            print(f"{s} {name}: niter {r0.niter} / {r1.niter}, deviation {dev:.2e}, {'in' if ok else 'OUT'}")
            n_in += ok
            if not ok:
                out.add((s, name))
            else:
                assert dev <= fc.PARITY_CAP
        print(f"{s}: {n_in} of {len(CASES[s])} cases qualify")
        assert n_in >= fc.PARITY_SHARE * len(CASES[s]), (s, n_in, len(CASES[s]))
    assert out == CHAOTIC
    assert fc.PARITY_CAP == 1e-6 and fc.PARITY_SHARE == 0.9 and fc.PARITY_FLOOR == 1e-12


# ---- 4. the judge -----------------------------------------------------------------------------------------------------------------
JUDGED = [("cg", "poisson9"), ("cg", "npc4_radius10"), ("gmres", "kron7"), ("gmres", "sq_inc10"), ("bicgstab", "kron7"),
          ("bicgstab", "sq_inc10"), ("bicgstab", "eye10")]


def _rec(oracle, solver, name):
    return Record(oracle_run(oracle, solver, name))


@pytest.mark.parametrize("solver,name", JUDGED)
def test_judge_accepts_the_unperturbed_result(oracle, solver, name):
    want = _rec(oracle, solver, name)
    assert judge(_rec(oracle, solver, name), want, TOL, solver, x=want.x, x_want=want.x) == 0.0
    # a history moved by half the tolerance and an x moved by half of its own still pass
    got = _rec(oracle, solver, name)
    fin = np.isfinite(got.residuals)
    got.residuals[fin] += 0.5 * (TOL["rtol"] * got.residuals[fin] + TOL["floor"] * got.residuals[0])
    units = judge(got, want, TOL, solver, x=want.x + 0.5 * TOL["x"] * np.abs(want.x).max(), x_want=want.x)
    assert 0.4 <= units <= 0.6


@pytest.mark.parametrize("solver,name", JUDGED)
def test_judge_rejects_what_it_must(oracle, solver, name):
    want = _rec(oracle, solver, name)
    fin = np.flatnonzero(np.isfinite(want.residuals))

    def rejected(change, what):
        got = _rec(oracle, solver, name)
        change(got)
        with pytest.raises(Mismatch, match=what):
            judge(got, want, TOL, solver, x=got.x, x_want=want.x)

    for k in {int(fin[0]), int(fin[-1])}:                                 # one history entry moved by 2 x the tolerance, either way
        for sign in (1.0, -1.0):
            def move(g, k=k, sign=sign):
                g.residuals[k] += sign * 2.0 * (TOL["rtol"] * abs(want.residuals[k]) + TOL["floor"] * want.residuals[0])
            rejected(move, f"history entry {k}")

    def one_more(g):
        g.niter += 1
    rejected(one_more, "niter, status")

    def one_less(g):
        g.niter -= 1
    rejected(one_less, "niter, status")

    def other_status(g):
        g.status = TIRED if g.status != TIRED else SOLVED
    rejected(other_status, "niter, status")

    def flip_inconsistent(g):
        g.inconsistent = not g.inconsistent
    rejected(flip_inconsistent, "niter, status")

    def flip_solved(g):
        g.solved = not g.solved
    rejected(flip_solved, "niter, status")
    if solver == "cg":
        def flip_indefinite(g):
            g.indefinite = not g.indefinite
        rejected(flip_indefinite, "niter, status")

        def npc_count(g):
            g.npcCount += 1
        rejected(npc_count, "niter, status")

    def longer(g):
        g.residuals = np.append(g.residuals, g.residuals[-1])
    rejected(longer, "history of")

    def x_off(g):
        g.x = g.x + 2.0 * TOL["x"] * np.abs(want.x).max() * (np.arange(len(g.x)) == len(g.x) - 1)
    if np.isfinite(want.x).all() and want.x.any():
        rejected(x_off, "x: largest deviation")

    def nan_entry(g):
        g.residuals[fin[-1]] = math.nan
    rejected(nan_entry, "non-finite history entries")
    nonfin = np.flatnonzero(~np.isfinite(want.residuals))
    if len(nonfin):
        k = int(nonfin[0])                                                # the first NaN, with a finite entry before it

        def nan_moved(g):
            g.residuals[k - 1], g.residuals[k] = g.residuals[k], g.residuals[k - 1]
        rejected(nan_moved, "non-finite history entries")

        def nan_replaced(g):
            g.residuals[k] = want.residuals[k - 1]
        rejected(nan_replaced, "non-finite history entries")

        def inf_for_nan(g):                                               # the class is not compared: Inf where NaN is expected passes
            g.residuals[k] = math.inf
        got = _rec(oracle, solver, name)
        inf_for_nan(got)
        judge(got, want, TOL, solver)
    else:
        assert name not in ("sq_inc10", "eye10") or solver != "bicgstab"


def test_judge_order_of_checks(oracle):
    """Shape first, then the flags, then the places of the non-finite entries, then the values."""
    want = _rec(oracle, "bicgstab", "sq_inc10")
    got = _rec(oracle, "bicgstab", "sq_inc10")
    got.residuals = np.append(got.residuals, 1.0)
    got.niter += 1
    with pytest.raises(Mismatch, match="history of"):
        judge(got, want, TOL, "bicgstab")
    got = _rec(oracle, "bicgstab", "sq_inc10")
    got.niter += 1
    got.residuals[2] = 1.0
    with pytest.raises(Mismatch, match="niter, status"):
        judge(got, want, TOL, "bicgstab")
    got = _rec(oracle, "bicgstab", "sq_inc10")
    got.residuals[2] = 1.0
    got.residuals[1] = 2.0
    with pytest.raises(Mismatch, match="non-finite history entries"):
        judge(got, want, TOL, "bicgstab")
