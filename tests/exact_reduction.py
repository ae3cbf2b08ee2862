"""Exact references for the compensated reductions (csrc/device_reduce.hpp, oracle/krylov_oracle.c ko_dot2).

exact_dot / exact_norm return the correctly rounded value of sum x_i y_i / sqrt(sum x_i^2); dot2_bound is the error bound a
Dot2-shaped reduction has to meet against it; gen_dot builds ill-conditioned pairs whose large cancelling partners sit where a
reduction tree is most likely to lose them; Tally logs and judges one result against them.  Imported by tests/test_exact_reduction_host.py,
tests/test_gpu_reduction_exact.py and tests/partition_model.py (the partitioned SpMV's fused scalars and row bounds).

Exactness window: every product x_i y_i is 0 or has a magnitude in [2^-969, 2^1000].  Above it the error-free products and
their sum could overflow; below it the error term of a product (down to 2^-106 of it) is no longer a double.  Inputs outside
the window, and non-finite inputs, raise ValueError.
"""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53                        # unit roundoff of binary64
WINDOW = (2.0 ** -969, 2.0 ** 1000)   # admitted magnitudes of a nonzero product
_SPLIT = 134217729.0                  # 2^27 + 1 (Veltkamp)


def two_product(x, y):
    """Error-free products of float64 arrays: p + e == x * y exactly (Dekker's TwoProduct with Veltkamp's split; Python 3.10
    has no math.fma).  The split runs on the frexp mantissas in [0.5, 1), so it cannot overflow, and the scale 2^(ex + ey)
    is applied last; inside WINDOW that scaling is exact for p and e alike.  Raises ValueError outside the window."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    if x.shape != y.shape:
        raise ValueError("length mismatch")
    if not (np.isfinite(x).all() and np.isfinite(y).all()):
        raise ValueError("non-finite input: outside the exact window")
    mx, ex = np.frexp(x)
    my, ey = np.frexp(y)
    p = mx * my
    c = _SPLIT * mx
    ah = c - (c - mx)
    al = mx - ah
    c = _SPLIT * my
    bh = c - (c - my)
    bl = my - bh
    e = al * bl - (((p - ah * bh) - al * bh) - ah * bl)
    k = ex.astype(np.int64) + ey.astype(np.int64)
    # |p + e| = |mx my| in [1/4, 1) and |x y| = |mx my| 2^k: decide 2^-969 <= |x y| <= 2^1000 exactly
    nz = p != 0
    if nz.any():
        kk, ap, ae = k[nz], np.abs(p[nz]), e[nz] * np.sign(p[nz])
        ok_lo = (kk >= -967) | ((kk == -968) & ((ap > 0.5) | ((ap == 0.5) & (ae >= 0))))
        ok_hi = (kk <= 1000) | ((kk == 1001) & ((ap < 0.5) | ((ap == 0.5) & (ae <= 0)))) | ((kk == 1002) & (ap == 0.25) & (ae == 0))
        if not (bool(ok_lo.all()) and bool(ok_hi.all())):
            raise ValueError("a product lies outside [2^-969, 2^1000]: outside the exact window")
    with np.errstate(over="ignore", under="ignore"):
        return np.ldexp(p, k), np.ldexp(e, k)


def exact_sum(terms):
    """The exact sum of float64 values as (N, E): the value is N * 2^E with N a Python int.  Vectorised: the 53-bit integer
    mantissas are cut into three 18-bit digits and binned by exponent with np.bincount (float64 bin sums of 18-bit integers
    stay exact below 2^35 terms); the <= 2100 bins are combined in Python integers."""
    t = np.ascontiguousarray(terms, dtype=np.float64).ravel()
    if not np.isfinite(t).all():
        raise ValueError("non-finite term")
    t = t[t != 0]
    if t.size == 0:
        return 0, 0
    if t.size >= 1 << 35:
        raise ValueError("too many terms for exact bin sums")
    m, e = np.frexp(t)
    M = (m * 2.0 ** 53).astype(np.int64)               # exact: |m| in [0.5, 1)
    e = e.astype(np.int64) - 53
    E0 = int(e.min())
    idx = e - E0
    neg = M < 0
    A = np.abs(M)
    N = 0
    for shift in (0, 18, 36):
        digit = ((A >> shift) & ((1 << 18) - 1)).astype(np.float64)
        digit[neg] = -digit[neg]
        bins = np.bincount(idx, weights=digit)
        for b in np.flatnonzero(bins).tolist():
            N += int(bins[b]) << (b + shift)
    return N, E0


def _as_fraction(N, E):
    return Fraction(N << E) if E >= 0 else Fraction(N, 1 << -E)


_CHUNK = 1 << 21


def _dot_sum(x, y):
    """sum x_i y_i exactly as (N, E), taken 2^21 elements at a time so that host memory stays bounded at any length."""
    x = np.ascontiguousarray(x, dtype=np.float64).ravel()
    y = np.ascontiguousarray(y, dtype=np.float64).ravel()
    if x.shape != y.shape:
        raise ValueError("length mismatch")
    N, E = 0, None
    for s in range(0, x.size, _CHUNK):
        p, e = two_product(x[s:s + _CHUNK], y[s:s + _CHUNK])
        n1, e1 = exact_sum(np.concatenate([p, e]))
        if n1 == 0:
            continue
        if E is None:
            N, E = n1, e1
        elif e1 < E:
            N, E = (N << (E - e1)) + n1, e1
        else:
            N += n1 << (e1 - E)
    return N, (0 if E is None else E)


def exact_dot_fraction(x, y) -> Fraction:
    """sum x_i y_i as an exact rational (inside the window)."""
    return _as_fraction(*_dot_sum(x, y))


def exact_dot(x, y) -> float:
    """The correctly rounded sum x_i y_i: error-free products (two_product), their exact integer sum, then one rounding --
    Python's int / int true division and int -> float conversion round correctly (to nearest, ties to even)."""
    N, E = _dot_sum(x, y)
    return float(N << E) if E >= 0 else N / (1 << -E)


def exact_norm(x) -> float:
    """The correctly rounded sqrt(sum x_i^2): the exact rational sum, then an integer square root with a sticky bit."""
    N, E = _dot_sum(x, x)
    if N == 0:
        return 0.0
    if E & 1:
        N, E = N << 1, E - 1
    j = max(0, (113 - N.bit_length()) // 2 + 1)         # N 4^j has >= 112 bits: the root >= 56 bits
    M = N << (2 * j)
    r = math.isqrt(M)
    r2 = 2 * r + (r * r != M)                           # 2 sqrt(M), its lowest bit sticky: rounds like the true root
    ex = E // 2 - j - 1
    return float(r2 << ex) if ex >= 0 else r2 / (1 << -ex)


def gamma(n: int) -> float:
    nu = n * U
    if nu >= 1.0:
        raise ValueError("n u >= 1")
    return nu / (1.0 - nu)


def dot2_bound(n: int, s: float, absum: float) -> float:
    """|res - s| <= u |s| + 2 gamma_n^2 sum|x_i y_i| (u = 2^-53, gamma_n = n u / (1 - n u)): the bound of Ogita, Rump & Oishi
    (SISC 26, 2005, Prop. 5.5) for Dot2, which has gamma_n^2 in place of 2 gamma_n^2.

    It holds for this code's summation shape too.  Every lane accumulates its elements sequentially (TwoProd, then TwoSum of the
    product into hi, both errors added into lo); dd_merge then applies TwoSum to the hi parts and adds the lo parts plainly,
    along a tree (DPP steps, workgroup, finish kernel, ranks) of depth <= n.  Every TwoProd and TwoSum error is captured
    exactly, so hi + (exact sum of all the errors) == s.  What matters is the TOTAL T of those errors: a TwoProd error is
    <= u |x_i y_i|, so they add up to <= u sum|x_i y_i|; a TwoSum error is <= u times the |hi| it produced, and a product
    enters at most depth <= n - 1 of those partial sums, so they add up to <= gamma_(n-1) sum|x_i y_i| (ORO's Sum2 lemma, for
    a tree as for a chain).  Hence T <= gamma_n sum|x_i y_i| to first order.  lo is a plain floating-point sum of at most 2n of
    these terms, so its own rounding costs <= gamma_(2n-1) T <= 2 gamma_n^2 sum|x_i y_i| (gamma_(2n-1) <= 2 gamma_n while
    2 n^2 u <= 1, i.e. n <= 6.7e7).  The final rounding of hi + lo adds u |s| (plus terms of order u^3).  A failure of this
    bound is a bug (a lost lo, a product not split, a fused or reassociated operation), not a tolerance that was too tight."""
    return U * abs(s) + 2.0 * gamma(max(int(n), 1)) ** 2 * absum


def absum(x, y) -> float:
    """sum |x_i y_i| (fsum per 2^21 elements, then fsum of those: within an ulp or two, which is all a bound needs)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return math.fsum(math.fsum(np.abs(x[s:s + _CHUNK] * y[s:s + _CHUNK]).tolist()) for s in range(0, x.size, _CHUNK))


def _positions(n, place, starts):
    """(i, j): where the largest cancelling pair goes."""
    if isinstance(place, tuple):
        return place
    if place == "waves":                  # 130 elements apart: another wave of the streaming kernels for VEC 1 / 2, U 1 / 4
        i = n // 3
        return i, min(n - 1, i + 130)
    if place == "blocks":                 # an eighth from either end: different finish-kernel blocks once G > 1
        return n // 8, n - 1 - n // 8
    if place == "ends":                   # the first and the last partial
        return 0, n - 1
    if place == "tail":                   # one partner is the odd tail element a VEC = 2 kernel handles separately
        return n // 2, n - 1
    if place == "ranks":                  # first rank's last row and last rank's first row of the row partition `starts`
        return starts[1] - 1, starts[-2]
    raise ValueError(place)


def gen_dot(n, cond, rng, place="waves", y=None, starts=None):
    """An ill-conditioned pair (x, y) with sum|x_i y_i| / |sum x_i y_i| close to `cond` (1 <= cond <= 1e32), in the spirit of
    Ogita, Rump & Oishi's GenDot: a base of positive products (condition 1), one large cancelling pair of products +-B placed
    by `place` ("waves", "blocks", "ends", "tail", "ranks" with `starts`, or an explicit (i, j)), a few smaller pairs with
    log-spread magnitudes at random positions, then corrections at random positions that cancel the pairs' residual (their
    product errors, ~u B) down to below the base's sum.  With `y` given (the product of an SpMV), only x is generated; zero
    entries of y are kept away from.  Returns (x, y, achieved condition); exact, so tests can assert their cases really are
    ill-conditioned."""
    if y is None:
        y = rng.standard_normal(n) * np.exp2(rng.integers(-8, 9, n))
    y = np.ascontiguousarray(y, dtype=np.float64)
    nzy = np.flatnonzero(y)
    if nzy.size == 0:
        raise ValueError("y == 0")
    # base: every product positive, magnitudes over 2^+-8
    x = np.zeros(n)
    x[nzy] = np.sign(y[nzy]) * np.abs(rng.standard_normal(nzy.size)) * np.exp2(rng.integers(-8, 9, nzy.size)) / np.abs(y[nzy])
    if cond > 1:
        if nzy.size < 8:
            raise ValueError("too few nonzero entries for an ill-conditioned pair")
        s0 = exact_dot_fraction(x, y)
        base_abs = float(s0)
        B = (cond - 1.0) * base_abs / 2.0

        def near_nz(k):                   # the nonzero entry of y closest to position k
            q = int(np.searchsorted(nzy, k))
            cands = [nzy[c] for c in (q - 1, q) if 0 <= c < nzy.size]
            return int(min(cands, key=lambda c: abs(c - k)))

        i, j = (near_nz(k) for k in _positions(n, place, starts))
        if i == j:
            raise ValueError("both partners on one element")
        used = {i, j}
        S = s0

        def put(k, v):
            nonlocal S
            S += Fraction(v) * Fraction(y[k]) - Fraction(x[k]) * Fraction(y[k])
            x[k] = v

        put(i, B / y[i])
        put(j, -B / y[j])
        free = np.setdiff1d(nzy, np.array(sorted(used)))
        rng.shuffle(free)
        fi = 0
        # smaller pairs, log-spread between the base and B / 16
        for t in range(4 if free.size >= 16 else 0):
            mag = base_abs * (B / 16.0 / base_abs) ** rng.uniform(0.2, 1.0) if B / 16.0 > base_abs else 0.0
            if mag == 0.0:
                break
            a, b = int(free[fi]), int(free[fi + 1])
            fi += 2
            put(a, mag * (1 + rng.uniform()) / y[a])
            put(b, -mag * (1 + rng.uniform()) / y[b])
        # corrections: cancel the residual down to below base_abs / 16 (each pass gains ~53 bits)
        target = s0
        while abs(S - target) > Fraction(base_abs) / 16:
            if fi >= free.size:
                raise ValueError("ran out of positions for the corrections")
            c = int(free[fi])
            fi += 1
            put(c, x[c] - float(S - target) / y[c])
        s = S
    else:
        s = exact_dot(x, y)
    achieved = math.inf if s == 0 else absum(x, y) / abs(float(s))
    return x, y, achieved


def ulp(v):
    return math.ulp(abs(v))


class Tally:
    """Per family: the largest |d - s| / bound, the share of results equal to the exactly rounded value, the conditions."""

    def __init__(self, log, family):
        self.log, self.family = log, family

    def dot(self, what, d, x, y, cond, n=None):
        n = x.size if n is None else n
        s, a = exact_dot(x, y), absum(x, y)
        bound = dot2_bound(n, s, a)
        self.log(test="exact_reduction", family=self.family, what=what, n=int(n), cond=float(cond),
                 ratio=abs(d - s) / bound if bound > 0 else (0.0 if d == s else math.inf), exact=bool(d == s))
        return abs(d - s) <= bound, (what, n, cond, d, s, bound)

    def sq(self, what, d, x):
        s = exact_dot(x, x)
        self.log(test="exact_reduction", family=self.family, what=what, n=int(x.size), cond=1.0,
                 ratio=abs(d - s) / ulp(s) if s else 0.0, exact=bool(d == s))
        return abs(d - s) <= ulp(s), (what, x.size, d, s)
