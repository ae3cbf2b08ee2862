"""The exact references of tests/exact_reduction.py against rational arithmetic, and the Dot2 bound against host restatements of
the compensated reductions: a NumPy restatement of the device's shape (lane-sequential acc_prod, then pairwise dd_merge) and the
oracle's Dot2 mode (ko_dot2, 1 / 3 / 8 threads) meet it up to condition 1e32; plain summation does not from 1e8 on.  Also the
non-finite results of the oracle's Dot2 mode (+-Inf stays +-Inf, Inf - Inf and NaN give NaN, as in the plain mode)."""
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_reduction as er  # noqa: E402

CONDS = [1.0, 1e4, 1e8, 1e16, 1e24, 1e32]
PLACES = ["waves", "blocks", "ends", "tail"]


def _frac_dot(x, y):
    return sum((Fraction(a) * Fraction(b) for a, b in zip(x.tolist(), y.tolist())), Fraction(0))


def _wide(rng, n, span):
    return rng.standard_normal(n) * np.exp2(rng.integers(-span, span + 1, n))


@pytest.mark.parametrize("n", [1, 2, 3, 17, 200, 1001])
def test_exact_dot_and_norm_equal_rational_arithmetic(n):
    rng = np.random.default_rng(n)
    cases = [(_wide(rng, n, 3), _wide(rng, n, 3)), (_wide(rng, n, 450), _wide(rng, n, 450))]
    if n >= 8:
        cases += [er.gen_dot(n, c, rng, "ends")[:2] for c in (1e8, 1e16, 1e32)]
    for x, y in cases:
        F = _frac_dot(x, y)
        assert er.exact_dot_fraction(x, y) == F
        assert er.exact_dot(x, y) == float(F)              # Fraction -> float rounds correctly
        # the norm: r is the double nearest to sqrt(S), S = sum x_i^2 exactly
        S = _frac_dot(x, x)
        r = er.exact_norm(x)
        lo, hi = Fraction(math.nextafter(r, 0.0)), Fraction(math.nextafter(r, math.inf))
        R = Fraction(r)
        assert ((lo + R) / 2) ** 2 <= S <= ((R + hi) / 2) ** 2, (n, r)
    assert er.exact_norm(np.zeros(3)) == 0.0 and er.exact_dot(np.zeros(2), np.ones(2)) == 0.0
    assert er.exact_norm(np.array([3.0, 4.0])) == 5.0


def test_exact_references_refuse_inputs_outside_the_window():
    for x, y in (([1e300], [1e300]), ([2.0 ** -500], [2.0 ** -500]), ([math.inf], [1.0]), ([math.nan], [1.0])):
        with pytest.raises(ValueError):
            er.exact_dot(np.array(x), np.array(y))
    # the edges themselves are inside
    assert er.exact_dot(np.array([2.0 ** 500]), np.array([2.0 ** 500])) == 2.0 ** 1000
    assert er.exact_dot(np.array([2.0 ** -484]), np.array([2.0 ** -485])) == 2.0 ** -969
    with pytest.raises(ValueError):
        er.exact_dot(np.array([2.0 ** -485]), np.array([2.0 ** -485]))


@pytest.mark.parametrize("place", PLACES)
def test_gen_dot_reaches_the_condition_it_was_asked_for(place):
    rng = np.random.default_rng(11)
    for cond in CONDS:
        x, y, got = er.gen_dot(4099, cond, rng, place)
        assert cond / 2 <= got <= cond * 2, (cond, got)
        assert math.isclose(got, er.absum(x, y) / abs(float(er.exact_dot_fraction(x, y))), rel_tol=1e-12)
    y = rng.standard_normal(3000)
    y[::3] = 0.0                                            # an SpMV product with zero rows: only x is generated
    x, y2, got = er.gen_dot(3000, 1e24, rng, "ends", y=y)
    assert np.array_equal(y2, y) and 5e23 <= got <= 2e24
    starts = [0, 1000, 2000, 3000]
    x, y, got = er.gen_dot(3000, 1e16, rng, "ranks", starts=starts)
    big = np.argsort(-np.abs(x * y))[:2]
    assert sorted(int(b) for b in big) == [999, 2000]


# ---------------------------------------------------------------------- host restatements of the reductions

def _two_sum(a, b):
    s = a + b
    z = s - a
    return s, (a - (s - z)) + (b - z)


def device_shape_dot(x, y, lanes=256):
    """csrc/device_reduce.hpp restated: element i goes to lane i % lanes, every lane runs acc_prod<true> over its elements in
    order (TwoProd, TwoSum into hi, errors into lo), then the lanes are folded pairwise with dd_merge; hi + lo at the end."""
    n = x.size
    hi, lo = np.zeros(lanes), np.zeros(lanes)
    p_all, e_all = er.two_product(x, y)
    for s in range(0, n, lanes):
        p, e = p_all[s:s + lanes], e_all[s:s + lanes]
        k = p.size
        h, err = _two_sum(hi[:k], p)
        hi[:k] = h
        lo[:k] += err + e
    while hi.size > 1:
        h, err = _two_sum(hi[0::2], hi[1::2])
        lo = (lo[0::2] + lo[1::2]) + err
        hi = h
    return float(hi[0] + lo[0])


def plain_lane_dot(x, y, lanes=256):
    """The same shape without compensation (compensated = 0)."""
    n = x.size
    hi = np.zeros(lanes)
    for s in range(0, n, lanes):
        p = x[s:s + lanes] * y[s:s + lanes]
        hi[:p.size] += p
    while hi.size > 1:
        hi = hi[0::2] + hi[1::2]
    return float(hi[0])


def _cases(n, seed):
    rng = np.random.default_rng(seed)
    for cond in CONDS:
        for place in PLACES:
            x, y, got = er.gen_dot(n, cond, rng, place)
            yield cond, place, x, y, got


@pytest.mark.parametrize("n", [1001, 100003])
def test_dot2_bound_holds_for_the_device_shape_and_fails_for_plain_summation(n):
    worst, violations = 0.0, {}
    for cond, place, x, y, got in _cases(n, n):
        s, a = er.exact_dot(x, y), er.absum(x, y)
        bound = er.dot2_bound(n, s, a)
        for lanes in (64, 256):
            d = device_shape_dot(x, y, lanes)
            assert abs(d - s) <= bound, (cond, place, lanes, d, s, bound)
            worst = max(worst, abs(d - s) / bound)
        plain = {"sequential": float(np.cumsum(x * y)[-1]), "lanes": plain_lane_dot(x, y)}
        for name, d in plain.items():
            if abs(d - s) > bound:
                violations.setdefault(name, []).append((cond, place))
    assert worst <= 1.0
    # teeth: plain summation is out of the bound in every case of condition 1e8 and 1e16, and in at least one placement at
    # every higher condition (there the bound reaches |s| or more: a plain sum that lost everything can land inside it)
    for name in ("sequential", "lanes"):
        got = violations[name]
        for cond in (1e8, 1e16):
            assert sum(c == cond for c, _ in got) == len(PLACES), (name, cond, got)
        for cond in (1e24, 1e32):
            assert any(c == cond for c, _ in got), (name, cond, got)


def test_dot2_bound_holds_for_the_oracle_dot2_mode(oracle):
    L = oracle.lib()
    n = 100003                                             # >= 2^16: ko_dot2 splits over the threads
    prev = L.ko_get_threads()
    try:
        L.ko_set_dot_mode(1)
        for cond, place, x, y, got in _cases(n, 5):
            s, a = er.exact_dot(x, y), er.absum(x, y)
            bound = er.dot2_bound(n, s, a)
            for th in (1, 3, 8):
                L.ko_set_threads(th)
                d = oracle.dot(x, y)
                assert abs(d - s) <= bound, (cond, place, th, d, s, bound)
    finally:
        L.ko_set_dot_mode(0)
        L.ko_set_threads(prev)


# Non-finite inputs.  Inputs whose plain result depends on the order in which partial sums overflow are out of scope: every
# case below has at most one overflowing product, or infinite inputs, so the plain result does not depend on the order (two
# overflowing products of opposite signs give NaN in Dot2 but +-Inf in an fma chain or in x87 extended precision).
NONFINITE = [
    ("overflow +", [1e300, 1.0, -2.0], [1e300, 3.0, 5.0], math.inf),
    ("overflow -", [-1e300, 1.0, -2.0], [1e300, 3.0, 5.0], -math.inf),
    ("inf input", [1.0, math.inf, 2.0], [1.0, 2.0, 3.0], math.inf),
    ("-inf input", [1.0, 2.0, 2.0], [1.0, -math.inf, 3.0], -math.inf),
    ("inf - inf", [math.inf, 1.0, -math.inf], [1.0, 1.0, 1.0], math.nan),
    ("nan", [1.0, math.nan, 2.0], [1.0, 1.0, 1.0], math.nan),
    ("inf * 0", [math.inf, 1.0], [0.0, 1.0], math.nan),
]


def _same_class(a, b):
    if math.isnan(b):
        return math.isnan(a)
    return a == b


@pytest.mark.parametrize("name,x,y,want", NONFINITE, ids=[c[0] for c in NONFINITE])
def test_nonfinite_results_of_the_oracle_dot2_mode(oracle, name, x, y, want):
    L = oracle.lib()
    prev = L.ko_get_threads()
    x, y = np.array(x), np.array(y)
    # also at a length where ko_dot2 splits over threads (the special value in the first thread's share, the rest zeros)
    xl, yl = np.zeros(1 << 17), np.zeros(1 << 17)
    xl[:x.size], yl[:y.size] = x, y
    try:
        for mode in (0, 1):
            L.ko_set_dot_mode(mode)
            for th in (1, 3):
                L.ko_set_threads(th)
                for a, b in ((x, y), (xl, yl), (xl[::-1].copy(), yl[::-1].copy())):
                    got = oracle.dot(a, b)
                    assert _same_class(got, want), (name, mode, th, got)
            if name.startswith("overflow"):
                # x holds 1e300: its square overflows in double (Dot2 mode) -> nrm2 = +Inf.  The default mode accumulates in x87
                # extended precision, where 1e300^2 is finite: there nrm2 stays finite (a documented difference, not tested).
                if mode == 1:
                    assert oracle.nrm2(x) == math.inf, (name, x)
            elif not math.isnan(want):
                v = x if np.isinf(x).any() else y          # the vector that holds the +-Inf input
                assert oracle.nrm2(v) == math.inf, (name, mode, v)
    finally:
        L.ko_set_dot_mode(0)
        L.ko_set_threads(prev)
