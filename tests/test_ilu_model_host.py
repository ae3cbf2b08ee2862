"""Host-only half of the exact ILU(0) tests (no device): the operator families of tests/ilu_model.py really have the properties
tests/test_gpu_ilu_exact.py relies on (through khip_test_ilu_paths_host, which runs the path decision of csrc/ilu.hip the launch
uses), the oracle's serial loops are pinned to exact rational arithmetic, and the bit-for-bit comparison rejects every fault
of ilu_model.FAULTS on the inputs the device test feeds."""
from fractions import Fraction

import numpy as np
import pytest

import ilu_model as M


@pytest.fixture(scope="module")
def refs(oracle):
    """name -> (oracle matrix, oracle factorisation), built once."""
    cache = {}

    def get(name, A=None):
        if name not in cache:
            A = M.family(name) if A is None else A
            OA = oracle.CsrMatrix.from_arrays(A.rowptr, A.col, A.val)
            cache[name] = (A, oracle.Ilu0(OA))
        return cache[name]
    return get


def _paths(K, A, ilu_blocks):
    return K.ilu_paths_host(A.rowptr, A.col, ilu_blocks)


# ---- what the families reach -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", M.FAMILIES)
def test_family_passes_the_create_gates(K, name):
    A = M.family(name)
    r = _paths(K, A, 1)
    nlo, nup = r["nlevels"]
    assert A.n >= 4096 and r["attempted"] == 1
    if name not in M.GRID_FAMILIES:                  # a recognised grid needs no rows-per-level ratio
        assert 2 * A.n // (nlo + nup) >= 32
    assert (2 * A.n // (nlo + nup) < 32) == (name in M.TOO_THIN_FOR_LEVEL_BLOCKS)
    assert (nlo, nup) == (len(M.level_widths(A)), len(M.level_widths(A, upper=True)))
    assert r["analysis"]["dims"] == (M.family_dims(name) if name != "too_big" else (0, 0, 0))
    assert _paths(K, A, 0)["attempted"] == 0 and _paths(K, A, 0)["blocks_in_use"] == 0


@pytest.mark.parametrize("name", list(M.LAYERED))
def test_layered_families_have_the_level_widths_they_were_given(name):
    A = M.family(name)
    assert M.level_widths(A) == M.LAYERED[name]["widths"]
    assert M.level_widths(A, upper=True) == M.LAYERED[name]["widths"]
    low = np.diff(A.rowptr) - 1                       # lower + upper entries; the two triangles mirror each other
    assert low.max() <= 2 * (M.LAYERED[name]["fan"] + M.LAYERED[name].get("far", 0))


@pytest.mark.parametrize("name", M.FAMILIES)
def test_family_reaches_the_path_it_exists_for(K, name):
    """The same expectations tests/test_gpu_ilu_exact.py asserts on the live operator (ilu_model.expect_paths)."""
    A = M.family(name)
    for ilu_blocks in sorted({b for b, _ in M.schedules(name)}):
        r = _paths(K, A, ilu_blocks)
        M.expect_paths(name, ilu_blocks, r)
        assert r["lower"]["workgroups"] == 0          # the host form knows no device


def test_edges_cuts_wide_levels_into_wave_blocks_with_remainders_1_and_63(K):
    """Levels of >= 64 rows are cut into 64-row blocks: 65 -> 64 + 1, 127 -> 64 + 63; [63], [1] and the merged [5, 5] stay whole."""
    widths = M.LAYERED["edges"]["widths"]
    want = 0
    merged = False
    for w in widths:
        if w >= 64:
            want += -(-w // 64); merged = False
        elif not merged:
            want += 1; merged = True
    r = _paths(K, M.family("edges"), 1)
    assert r["lower"]["blocks"] == r["upper"]["blocks"] == want == 72
    assert r["lower"]["rows_cap"] == 64 and r["lower"]["max_levels"] == 2 and r["lower"]["max_width"] == 64
    # level schedule: small-level runs of 7 and 3 are batched; the run of exactly one small level (256 between 300 and 257,
    # and the last 200) is a launch of its own, like the wide levels
    for kind in ("factor", "lower", "upper"):
        assert r["levels"][kind] == {"batched": 2, "single": 7}


def test_merge_caps(K):
    r = _paths(K, M.family("cap48"), 1)
    assert r["lower"]["max_levels"] == r["upper"]["max_levels"] == 48 and r["lower"]["rows_cap"] == 512      # closed by the 48 levels: 480 rows
    r = _paths(K, M.family("rows512"), 1)
    assert r["lower"]["max_levels"] == 8 and r["lower"]["rows_cap"] == 512 and r["lower"]["blocks"] == 12      # closed by the rows: 8 x 60 = 480, a ninth level would make 540


def test_too_big_falls_back_because_of_lds(K):
    for b in (1, 2):
        r = _paths(K, M.family("too_big"), b)
        assert r["attempted"] == 1 and r["blocks_in_use"] == 0 and r["fallback"] == 1
        assert r["lower"]["lds"] > 150 * 1024 and r["lower"]["blocks"] == 0
        assert r["levels"]["lower"] == {"batched": 0, "single": 12}          # 400 rows a level: none is small


# ---- same_bits itself ---------------------------------------------------------------------------------------------------------
def test_same_bits():
    a = np.array([1.0, -0.0, np.nan, np.inf, 5e-324])
    assert M.same_bits(a, a.copy())
    assert M.same_bits(a, np.array([1.0, -0.0, -np.nan, np.inf, 5e-324]))          # any NaN for a NaN
    assert not M.same_bits(a, np.array([1.0, 0.0, np.nan, np.inf, 5e-324]))        # the sign of zero counts
    assert not M.same_bits(a, np.array([1.0, -0.0, np.inf, np.inf, 5e-324]))       # NaN exactly where the reference has NaN
    assert not M.same_bits(a, np.array([1.0, -0.0, np.nan, np.nan, 5e-324]))
    assert not M.same_bits(a, np.array([1.0 + 2.0 ** -52, -0.0, np.nan, np.inf, 5e-324]))
    assert not M.same_bits(a, np.array([1.0, -0.0, np.nan, np.inf, 0.0]))
    assert not M.same_bits(a, a[:4])


# ---- the reference against exact arithmetic ----------------------------------------------------------------------------------
U_ROUND = Fraction(1, 2 ** 53)


def _gamma(r):
    return r * U_ROUND / (1 - r * U_ROUND)


@pytest.mark.parametrize("which", ["layered", "permuted"])
def test_oracle_against_exact_arithmetic(oracle, which):
    """The oracle's factors and solves satisfy the standard componentwise backward error bounds of LU and of substitution
    (Higham, Accuracy and Stability of Numerical Algorithms, Lemma 8.4 and Theorems 8.5 / 9.3) in exact rational arithmetic,
    with gamma_r = r u / (1 - r u), u = 2^-53, r = stored entries of the row -- no fitted constant:
      every pattern position   |A - L U| <= gamma_r (|L| |U|),
      lower solve              |x - L z| <= gamma_r |L| |z|,
      upper solve              |z - U y| <= gamma_r |U| |y|."""
    A = M.layered([10] * 30, fan=2, far=1, gap=3, seed=3) if which == "layered" else M.permuted("star", (7, 7, 6), seed=3)
    assert 290 <= A.n <= 300
    OA = oracle.CsrMatrix.from_arrays(A.rowptr, A.col, A.val)
    ref = oracle.Ilu0(OA)
    n, rp, col = A.n, A.rowptr.tolist(), A.col.tolist()
    dg = M.diag_positions(A).tolist()
    lu = [Fraction(v) for v in ref.lu.tolist()]
    a = [Fraction(v) for v in A.val.tolist()]
    pos = [{col[q]: q for q in range(rp[i], rp[i + 1])} for i in range(n)]
    worst = Fraction(0)
    for i in range(n):
        g = _gamma(rp[i + 1] - rp[i])
        for q in range(rp[i], rp[i + 1]):
            j = col[q]
            s = mag = Fraction(0)
            for qk in range(rp[i], dg[i]):                   # k < i with (i, k) stored
                k = col[qk]
                if k < j and j in pos[k]:                    # ... and (k, j) stored, k < min(i, j)
                    t = lu[qk] * lu[pos[k][j]]
                    s += t; mag += abs(t)
            last = lu[q] * lu[dg[j]] if j < i else lu[q]     # l_ij u_jj, or 1 * u_ij
            res, bound = abs(a[q] - s - last), g * (mag + abs(last))
            assert res <= bound, (i, j, float(res), float(bound))
            if bound:
                worst = max(worst, res / bound)
    assert worst > 0                                          # the check is not vacuous: some position rounds
    x = np.random.default_rng(8).standard_normal(n)
    y = ref.solve(x)
    # z = L \ x from the oracle's own loops: with U replaced by the identity the upper loop computes (z - 0.0 * y) / 1.0 = z
    unit = oracle.Ilu0(OA)
    rows = np.repeat(np.arange(n), np.diff(A.rowptr))
    unit.lu = np.where(A.col > rows, 0.0, np.where(A.col == rows, 1.0, ref.lu))
    z = unit.solve(x)
    xf, yf, zf = ([Fraction(v) for v in w.tolist()] for w in (x, y, z))
    for i in range(n):
        g = _gamma(rp[i + 1] - rp[i])
        s, mag = zf[i], abs(zf[i])
        for q in range(rp[i], dg[i]):
            t = lu[q] * zf[col[q]]
            s += t; mag += abs(t)
        assert abs(xf[i] - s) <= g * mag, ("lower", i)
        s = mag = Fraction(0)
        for q in range(dg[i], rp[i + 1]):
            t = lu[q] * yf[col[q]]
            s += t; mag += abs(t)
        assert abs(zf[i] - s) <= g * mag, ("upper", i)
    assert M.same_bits(M.serial_solve(A, ref.lu, x), y)


# ---- the model is the oracle; every fault is rejected -----------------------------------------------------------------------
@pytest.mark.parametrize("name", M.FAMILIES)
def test_inputs_and_model_against_the_oracle(refs, name):
    """serial_solve without a fault is the oracle bit for bit on every input of the device test, and the inputs are what the
    device test needs: the special rows leave at least half of the oracle's y finite wherever the operator allows it."""
    A, ref = refs(name)
    for kind, x in M.inputs(name).items():
        y = ref.solve(x)
        assert M.same_bits(M.serial_solve(A, ref.lu, x), y), kind
        if kind in ("normal", "negzero", "extremes"):
            assert np.isfinite(y).all(), kind
        if kind == "negzero":
            assert (y == 0.0).all() and np.signbit(y).any()
        if kind == "one_inf":
            assert np.isinf(y).any()
        if kind == "specials":
            assert np.isnan(y).any()
            if name in M.SPECIALS_STAY_NARROW:
                assert np.isfinite(y).mean() >= 0.5, np.isfinite(y).mean()
    if name not in M.SPECIALS_STAY_NARROW:
        # no placement can do better here: on these operators every row reaches, through the lower solve and then the upper
        # one, more than half of all rows (on a grid: all of them), so one non-finite entry of x makes most of y non-finite.
        # Their arithmetic is pinned by the finite inputs; `extremes` carries the signed zeros, subnormals and +-1e200.
        best = max(np.isfinite(ref.solve(M.specials(A.n, [r]))).mean() for r in range(0, A.n - 7, max(1, A.n // 60)))
        assert best < 0.5, best


@pytest.mark.parametrize("name", M.FAMILIES)
def test_the_comparison_rejects_every_fault(refs, name):
    """Each fault of ilu_model.FAULTS changes y on the input that can expose it (seeded normal x for the arithmetic ones; the
    specials / the all -0.0 x for those about absent entries, stored zeros and the sign of zero)."""
    A, ref = refs(name)
    xs = M.inputs(name)
    prev = ref.solve(np.random.default_rng(99).standard_normal(A.n))         # what an earlier application left in y
    widest_row = max((M.diag_positions(A) - A.rowptr[:-1]).max(), (A.rowptr[1:] - 1 - M.diag_positions(A)).max())
    widest_level = max(M.level_widths(A) + M.level_widths(A, upper=True))
    assert (widest_row < 2) == (name == "edges")
    for fault in M.FAULTS:
        if fault == "zero_absent":
            continue                                                            # needs stored zeros: next test
        if fault == "reverse" and widest_row < 2:
            continue                                                            # one entry per row and triangle: no order to reverse
        if fault == "skip_row64" and widest_level <= 64:
            continue                                                            # no level wider than the wave
        kinds = {"absent_inf": ("specials", "one_inf"), "drop_zero_sign": ("negzero",)}.get(fault, ("normal",))
        assert any(not M.same_bits(M.serial_solve(A, ref.lu, xs[k], fault=fault, y_prev=prev), ref.solve(xs[k])) for k in kinds), fault


@pytest.mark.parametrize("name", M.STORED_ZERO_FAMILIES)
def test_stored_zeros_are_not_absent(oracle, name):
    """A stored 0.0 times an Inf is NaN: the rows ilu_model.stored_zeros names come out NaN in the oracle, and treating a stored
    0.0 as absent is rejected."""
    A, nan_rows = M.stored_zeros(name)
    ref = oracle.Ilu0(oracle.CsrMatrix.from_arrays(A.rowptr, A.col, A.val))
    assert (ref.lu == 0.0).sum() == 3
    exposed = 0
    for kind, rows in nan_rows.items():
        x = M.inputs(name)[kind]
        y = ref.solve(x)
        assert np.isnan(y[rows]).all(), kind
        assert M.same_bits(M.serial_solve(A, ref.lu, x), y), kind
        exposed += not M.same_bits(M.serial_solve(A, ref.lu, x, fault="zero_absent"), y)
    assert exposed
