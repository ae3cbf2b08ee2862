"""tests/panel_model.py without a GPU: the geometry model against the C++ sources and hand-counted cases, the exact references
against rational arithmetic, the fault-free emulation of the kernels' partition inside the derived bounds on every real input
family (ratios printed), and every injected fault REJECTED by the comparisons tests/test_gpu_panel_exact.py applies to the
device -- on the integer family (equality) and the real families (bound) alike."""
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_reduction as er  # noqa: E402
import panel_model as pm  # noqa: E402


def test_model_constants_equal_the_sources():
    src = pm.constants_in_sources()
    assert src.pop("rows_per_wave_is_the_macro")
    assert src == {k: getattr(pm, k) for k in src}, src


def test_geometry_hand_counted():
    g = pm.tn_geometry(33333, 16)
    assert (g["n_pad"], g["waves"], g["workgroups"], g["reduce"], g["NT"]) == (33344, 131, 33, [33], 1)
    g = pm.tn_geometry(65537, 17)
    assert (g["n_pad"], g["waves"], g["workgroups"], g["reduce"], g["NT"]) == (65552, 257, 65, [65, 2], 2)
    assert pm.tn_geometry(0, 1) == {"n_pad": 0, "waves": 0, "workgroups": 1, "reduce": [1], "NT": 1}
    assert pm.tn_geometry(65536, 16)["reduce"] == [64] and pm.tn_geometry(4194304, 16)["reduce"] == [4096, 64]
    # roundings: one tile of 16 rows; a full wave; a full workgroup; two launches (63 + 1)
    assert pm.tn_roundings(1, 1) == 32 and pm.tn_roundings(256, 16) == 512
    assert pm.tn_roundings(1024, 16) == 515 and pm.tn_roundings(1025, 16) == 516
    assert pm.tn_roundings(65537, 16) == 512 + 3 + 63 + 1
    assert pm.tn_roundings(10_000_000, 16) == 512 + 3 + 63 + 63 + 2         # 9766 -> 153 -> 3 tiles
    # ... against the old per-entry tolerance 4 sqrt(n) eps = 8 sqrt(n) u at 10 M rows: about 35 times tighter
    assert 30 < 8 * math.sqrt(1e7) * er.U / er.gamma(pm.tn_roundings(10_000_000, 16) + 1) < 45


def test_geometry_of_the_chosen_sizes():
    """What each size of the GPU file is for."""
    geo = {n: pm.tn_geometry(n, 16) for n in pm.EDGE_SIZES + pm.MID_SIZES + (pm.THREE_LEVEL,)}
    for n in (1, 15, 16):                              # one tile, padding of 15 / 1 / 0 rows
        assert geo[n]["n_pad"] == 16 and geo[n]["waves"] == 1
    assert geo[17]["n_pad"] == 32                      # second tile, 15 padding rows
    assert [geo[n]["waves"] for n in (255, 256, 257, 272)] == [1, 1, 2, 2]
    assert geo[257]["n_pad"] == geo[272]["n_pad"] == 272          # the second wave holds 16 rows: less than one 32-row load step
    assert [geo[n]["workgroups"] for n in (1023, 1024, 1025, 1040)] == [1, 1, 2, 2]
    assert geo[1025]["waves"] == 5 and geo[1040]["n_pad"] == 1040
    assert geo[65536]["reduce"] == [64] and geo[65537]["reduce"] == [65, 2]
    assert geo[100 * 1024 + 1]["reduce"] == [101, 2]   # the second group of the first launch holds 37 tiles; both regions used
    assert geo[pm.THREE_LEVEL]["reduce"] == [4097, 65, 2] and geo[pm.THREE_LEVEL]["n_pad"] == pm.THREE_LEVEL + 15
    assert [geo[n]["workgroups"] for n in pm.MID_SIZES] == [2, 5] and all(geo[n]["n_pad"] % 256 for n in pm.MID_SIZES)
    assert all(n <= pm.ALL_ENTRIES_UP_TO for n in pm.EDGE_SIZES[:-1]) and pm.EDGE_SIZES[-1] > pm.ALL_ENTRIES_UP_TO
    # the non-finite rows: first, last real, and inside the last wave of the first 64-workgroup reduce group
    assert pm.NONFINITE_ROWS[1] == pm.NONFINITE_SIZE - 1 and pm.pad16(pm.NONFINITE_SIZE) > pm.NONFINITE_SIZE
    assert pm.NONFINITE_ROWS[2] // pm.ROWS_PER_WAVE == pm.FAN * pm.WAVES_PER_WG - 1
    # p = 17 is the first width of the NT = 2 instantiation
    assert pm.tn_geometry(100, 16)["NT"] == 1 and pm.tn_geometry(100, 17)["NT"] == 2
    # the three paths of khip_panel_multi_nn at the (p, k) the GPU file runs
    assert [pm.multi_path(*pk) for pk in ((16, 24), (32, 6))] == ["lds", "lds"]
    assert [pm.multi_path(*pk) for pk in ((16, 25), (32, 7), (17, 22))] == ["reread"] * 3
    assert pm.multi_path(16, 33) == "sequence" and pm.multi_path(16, 24, tiles=0) == "reread"


def test_integer_cases_stay_below_two_to_the_53():
    """Every integer case of the GPU file: V'Q sums, and the updates / product sequences built from the integer factors."""
    for n in pm.EDGE_SIZES + pm.MID_SIZES + (pm.THREE_LEVEL,):
        assert pm.int_condition(n)
        if n <= 2000:
            V, Q = pm.int_panels(n, 17)
            assert np.abs(V).max() <= 3 and np.abs(Q).max() <= 1000 and (V != 0).all() and (Q != 0).all()
            assert (np.abs(V).T @ np.abs(Q)).max() < 2.0 ** 53
    # update: |beta q| + |alpha| p |v| |psi| <= 4 * 1000 + 4 * 32 * 3 * 4; multi_nn with k <= 33 factors of magnitude <= 2
    assert 4 * 1000 + 4 * 32 * 3 * 4 < 2.0 ** 53 and 1000 + 33 * 32 * 3 * 2 < 2.0 ** 53
    V, Q = pm.int_panels(1025, 5)
    assert not np.array_equal(V.T @ Q, (V.T @ Q).T)
    assert np.array_equal(Q[:, 0], np.arange(1025) % 997 + 1)


def test_exact_update_equals_rational_arithmetic():
    rng = np.random.default_rng(5)
    for n, p, alpha, beta in ((3, 1, -1.0, 1.0), (7, 5, 0.3, -1.7), (4, 17, 2.0, 0.0)):
        V, Q, Psi = rng.standard_normal((n, p)), rng.standard_normal((n, p)), rng.standard_normal((p, p))
        hi, lo = pm.exact_update(alpha, V, Psi, beta, Q)
        for r in range(n):
            for c in range(p):
                F = Fraction(beta) * Fraction(Q[r, c]) + Fraction(alpha) * sum(Fraction(V[r, k]) * Fraction(Psi[k, c]) for k in range(p))
                mag = abs(beta * Q[r, c]) + abs(alpha) * float(np.abs(V[r]) @ np.abs(Psi[:, c]))
                assert abs(Fraction(hi[r, c]) + Fraction(lo[r, c]) - F) <= Fraction(mag) / 2 ** 80


HOST_CASES = [(17, 15), (272, 17), (1025, 16), (65537, 17), (100 * 1024 + 1, 5)]


@pytest.mark.parametrize("n,p", HOST_CASES)
def test_fault_free_emulation_meets_the_bounds(n, p):
    """The reference alone stays inside the bound: the NumPy restatement of the partition against exact_dot / the
    double-double update, on every real family."""
    entries = pm.all_entries(p) if n <= 2000 else pm.sample_entries(p)
    for fam in pm.families_for(n):
        V, Q = pm.real_panels(fam, n, p)
        r_tn = pm.tn_ratio(pm.emulate_tn(V, Q), V, Q, entries)
        Psi = pm.real_factor(p)
        r_nn = max(pm.nn_ratio(pm.emulate_nn(a, V, Psi, b, Q), a, V, Psi, b, Q) for a, b in ((-1.0, 1.0), (0.3, -1.7)))
        print(f"emulation n={n} p={p} {fam}: max|d|/bound  V'Q {r_tn:.3f} (m = {pm.tn_roundings(n, p) + 1})  update {r_nn:.3f}")
        assert r_tn <= 1.0 and r_nn <= 1.0
    V, Q = pm.int_panels(n, p)
    assert np.array_equal(pm.emulate_tn(V, Q), V.T @ Q)
    Psi = pm.int_factor(p)
    assert np.array_equal(pm.emulate_nn(-2.0, V, Psi, 3.0, Q), 3.0 * Q - 2.0 * (V @ Psi))


def _applies(fault, n, p):
    g = pm.tn_geometry(n, p)
    if fault == "fan63":
        return g["reduce"][0] >= pm.FAN
    if fault == "stale":
        return len(g["reduce"]) >= 2
    if fault == "colpred":
        return p % 16 != 0 and p > 1
    if fault == "transposed":
        return p > 1
    return True


@pytest.mark.parametrize("fault", pm.TN_FAULTS)
def test_every_injected_fault_of_the_product_is_rejected(fault):
    ran = 0
    for n, p in HOST_CASES:
        if not _applies(fault, n, p):
            continue
        ran += 1
        V, Q = pm.int_panels(n, p)
        assert not np.array_equal(pm.emulate_tn(V, Q, fault), V.T @ Q), (fault, n, p, "int")
        entries = pm.all_entries(p) if n <= 2000 else pm.sample_entries(p)
        for fam in pm.families_for(n):
            V, Q = pm.real_panels(fam, n, p)
            assert pm.tn_ratio(pm.emulate_tn(V, Q, fault), V, Q, entries) > 1.0, (fault, n, p, fam)
    assert ran >= 2, fault


@pytest.mark.parametrize("fault", pm.NN_FAULTS)
def test_every_injected_fault_of_the_update_is_rejected(fault):
    for n, p in HOST_CASES[:3] + [(1040, 31)]:
        if not _applies(fault, n, p):
            continue
        V, Q = pm.int_panels(n, p)
        Psi = pm.int_factor(p)
        assert not np.array_equal(pm.emulate_nn(-1.0, V, Psi, 1.0, Q, fault), Q - V @ Psi), (fault, n, p, "int")
        for fam in pm.families_for(n):
            V, Q = pm.real_panels(fam, n, p)
            Psi = pm.real_factor(p)
            assert pm.nn_ratio(pm.emulate_nn(-1.0, V, Psi, 1.0, Q, fault), -1.0, V, Psi, 1.0, Q) > 1.0, (fault, n, p, fam)


def test_the_old_whole_panel_tolerance_accepts_what_the_per_entry_bound_rejects():
    """Why the update gets a bound per entry: an entry that is small can be entirely wrong under one absolute tolerance for
    the whole panel (64 eps * max over all entries), and is rejected here."""
    rng = np.random.default_rng(3)
    n, p = 1000, 16
    V, Q, Psi = rng.standard_normal((n, p)), rng.standard_normal((n, p)), rng.standard_normal((p, p))
    V[:, :] *= np.exp2(-40.0 * (np.arange(n) % 2))[:, None]
    Q[:, :] *= np.exp2(-40.0 * (np.arange(n) % 2))[:, None]
    out = pm.emulate_nn(-1.0, V, Psi, 1.0, Q)
    out[1] *= 1.0 + 1e-6                                # a small row, wrong in the sixth digit
    ref = Q - V @ Psi
    assert np.allclose(out, ref, rtol=0, atol=64 * np.finfo(float).eps * (np.abs(Q) + np.abs(V) @ np.abs(Psi)).max())
    assert pm.nn_ratio(out, -1.0, V, Psi, 1.0, Q) > 1.0
