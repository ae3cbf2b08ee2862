"""Operator families and the comparison for the exact ILU(0) tests (tests/test_gpu_ilu_exact.py, tests/test_ilu_model_host.py).

Nothing here touches a device.  The families are built so that the block schedule of csrc/ilu.hip is driven down every one of
its row paths and block-forming rules (which path a family reaches is checked on the host by tests/test_ilu_model_host.py
through khip_test_ilu_paths_host and on the device through Ilu0.path_info()); `serial_solve` restates the two triangular loops
in plain Python floats, with switches for the faults the bit-for-bit comparison has to reject."""
from collections import namedtuple
from fractions import Fraction

import numpy as np
import scipy.sparse as sp

Csr = namedtuple("Csr", "n rowptr col val")          # int64 row pointers, int32 sorted columns, float64 values


def _finish(S, seed):
    """Pattern of S with seeded unsymmetric values in +-[0.25, 1] and a dominant diagonal of either sign (so that the zeros of
    a solve come in both signs)."""
    S = sp.csr_matrix(S); S.sort_indices()
    n = S.shape[0]
    rng = np.random.default_rng(seed)
    rowptr, col = S.indptr.astype(np.int64), S.indices.astype(np.int32)
    val = rng.uniform(0.25, 1.0, col.size) * rng.choice([-1.0, 1.0], col.size)
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    off = np.zeros(n)
    np.add.at(off, rows, np.abs(val))
    dg = rows == col
    assert dg.sum() == n
    val[dg] = (off - np.abs(val[dg]) + 1.0) * rng.uniform(1.0, 1.5, n) * rng.choice([-1.0, 1.0], n)
    return Csr(n, rowptr, col, val)


def layered(widths, fan, far=0, gap=0, seed=0):
    """Rows numbered level by level; a row of level k has `fan` distinct lower entries in level k - 1 (all of it where it is
    narrower) and `far` more among the rows at least `gap` levels back (they lengthen the face lists, not the levels).  The
    upper triangle is the lower pattern under i -> n - 1 - i, so the upper solve sees the same level widths."""
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(widths)]).astype(np.int64)
    n = int(off[-1])
    ri, ci = [], []
    for k in range(1, len(widths)):
        w, pw = int(widths[k]), int(widths[k - 1])
        f = min(fan, pw)
        pick = np.argsort(rng.random((w, pw)), axis=1)[:, :f] + off[k - 1]
        ri.append(np.repeat(np.arange(w) + off[k], f)); ci.append(pick.ravel())
        if far and k - gap >= 0 and off[k - gap + 1] >= far:
            pool = int(off[k - gap + 1])                                # rows of the levels 0 .. k - gap
            pick = np.argsort(rng.random((w, pool)), axis=1)[:, :far]
            ri.append(np.repeat(np.arange(w) + off[k], far)); ci.append(pick.ravel())
    ri, ci = np.concatenate(ri), np.concatenate(ci)
    L = sp.csr_matrix((np.ones(ri.size), (ri, ci)), shape=(n, n))
    L.data[:] = 1.0
    U = sp.csr_matrix((np.ones(ri.size), (n - 1 - ri, n - 1 - ci)), shape=(n, n))
    return _finish(L + U + sp.identity(n, format="csr"), seed + 1)


def _tri(n):
    return sp.diags([np.ones(n - 1), np.ones(n), np.ones(n - 1)], [-1, 0, 1], format="csr")


def star_pattern(n1, n2, n3):
    I = lambda n: sp.identity(n, format="csr")
    S = sp.kron(sp.kron(I(n3), I(n2)), _tri(n1)) + sp.kron(sp.kron(I(n3), _tri(n2)), I(n1))
    return (S + sp.kron(sp.kron(_tri(n3), I(n2)), I(n1))).tocsr()


def box_pattern(n1, n2, n3):
    return sp.kron(sp.kron(_tri(n3), _tri(n2)), _tri(n1)).tocsr()


def star(dims, seed=0):
    """5- / 7-point stencil on the grid dims in natural ordering."""
    return _finish(star_pattern(*dims), seed)


def box(dims, seed=0):
    """9- / 27-point stencil on the grid dims in natural ordering."""
    return _finish(box_pattern(*dims), seed)


def permuted(stencil, dims, seed=0):
    """A random symmetric permutation of the 7-point ("star") or 27-point ("box") stencil: no grid in natural ordering."""
    S = (star_pattern if stencil == "star" else box_pattern)(*dims)
    p = np.random.default_rng(seed).permutation(S.shape[0])
    return _finish(S[p][:, p], seed + 1)


def with_values(A, positions, value):
    """A copy of A whose stored entries at `positions` (indices into val) hold `value`."""
    val = A.val.copy()
    val[np.asarray(positions)] = value
    return Csr(A.n, A.rowptr, A.col, val)


def diag_positions(A):
    rows = np.repeat(np.arange(A.n), np.diff(A.rowptr))
    return np.flatnonzero(rows == A.col)


def levels(A, upper=False):
    """Level of every row in the lower (upper) solve: 1 + the largest level among the rows it reads."""
    lev = np.zeros(A.n, dtype=np.int64)
    rp, col = A.rowptr.tolist(), A.col.tolist()
    out = [0] * A.n
    for i in (range(A.n - 1, -1, -1) if upper else range(A.n)):
        lv = 0
        for q in range(rp[i], rp[i + 1]):
            j = col[q]
            if (j > i) if upper else (j < i):
                lv = max(lv, out[j] + 1)
        out[i] = lv
    lev[:] = out
    return lev


def level_widths(A, upper=False):
    return np.bincount(levels(A, upper)).tolist()


def same_bits(y, ref):
    """NaN exactly where the reference has NaN; everywhere else the same 64 bits (the sign of zero counts)."""
    y, ref = np.ascontiguousarray(y, dtype=np.float64), np.ascontiguousarray(ref, dtype=np.float64)
    if y.shape != ref.shape:
        return False
    ny, nr = np.isnan(y), np.isnan(ref)
    return bool(np.array_equal(ny, nr) and np.array_equal(y.view(np.uint64)[~nr], ref.view(np.uint64)[~nr]))


def specials(n, rows):
    """A right-hand side of ones with Inf, -Inf, NaN, -0.0, a subnormal and +-1e200 next to each other from each row in `rows`."""
    x = np.ones(n)
    pat = [np.inf, -np.inf, np.nan, -0.0, 5e-324, 1e200, -1e200]
    for r in rows:
        x[r:r + len(pat)] = pat[:max(0, min(len(pat), n - r))]
    return x


FAULTS = ("reverse", "fma", "absent_inf", "dump_row0", "pivot_neighbour", "divide_early", "skip_row64", "stale_face", "zero_absent",
          "drop_zero_sign")


def _fms(acc, v, y):
    """acc - v * y with ONE rounding (exact rational arithmetic, then the correctly rounded conversion)."""
    if not (np.isfinite(acc) and np.isfinite(v) and np.isfinite(y)):
        return acc - v * y
    r = Fraction(acc) - Fraction(v) * Fraction(y)
    if r == 0:
        return acc - v * y
    try:
        return float(r)
    except OverflowError:
        return acc - v * y


def serial_solve(A, lu, x, fault=None, y_prev=None):
    """y = U \\ (L \\ x) with the factors lu on A's pattern: the two serial loops, every entry of a row in stored order with one
    rounded multiply and one rounded subtract, the division last.  fault: one of FAULTS --
      reverse          the entries of a row are subtracted in reverse order;
      fma              multiply and subtract of a row's first entry fused into one rounding;
      absent_inf       a row of fewer than 16 entries (what a wide row record holds) also subtracts 0.0 * y[i - 2] (lower) /
                       0.0 * y[i + 2] (upper): an absent entry of a record pointing at a wrong slot instead of the constant 0.0;
      dump_row0        in every level whose width is no multiple of 64 the last row's result also lands in the level's first
                       row: what an idle lane computes written to a live slot instead of the dump slot;
      pivot_neighbour  the upper solve divides by the pivot of the next row;
      divide_early     the upper solve divides before its last subtraction;
      skip_row64       the 65th row of every level wider than 64 rows is not computed in the lower solve (its y stays 0.0);
      stale_face       the first entry of every 97th row of the lower solve reads y_prev (the previous application's result);
      zero_absent      a stored 0.0 is treated as absent;
      drop_zero_sign   -0.0 results are stored as +0.0."""
    assert fault is None or fault in FAULTS, fault
    n = A.n
    rp, col, lu, x = A.rowptr.tolist(), A.col.tolist(), np.asarray(lu, dtype=np.float64).tolist(), np.asarray(x, dtype=np.float64).tolist()
    dg = diag_positions(A).tolist()
    y = [0.0] * n
    yp = [0.0] * n if y_prev is None else np.asarray(y_prev, dtype=np.float64).tolist()
    skip, dump = set(), {}
    if fault in ("skip_row64", "dump_row0"):
        for upper in (False, True):
            lev = levels(A, upper)
            order = np.argsort(lev, kind="stable")
            ptr = np.concatenate([[0], np.cumsum(np.bincount(lev))])
            for l in range(len(ptr) - 1):
                rows = order[ptr[l]:ptr[l + 1]]
                if fault == "skip_row64" and not upper and len(rows) > 64:
                    skip.add(int(rows[64]))
                if fault == "dump_row0" and len(rows) % 64 and len(rows) > 1:
                    dump[(upper, int(rows[-1]))] = int(rows[0])
    for i in range(n):                                   # L z = x, unit lower; z overwrites y
        if i in skip:
            continue
        acc = x[i]
        qs = range(rp[i], dg[i])
        if fault == "reverse":
            qs = reversed(qs)
        first = True
        for q in qs:
            v = lu[q]
            if fault == "zero_absent" and v == 0.0:
                continue
            yy = y[col[q]]
            if first and fault == "stale_face" and i % 97 == 0:
                yy = yp[col[q]]
            if first and fault == "fma":
                acc = _fms(acc, v, yy)
            else:
                t = v * yy
                acc = acc - t
            first = False
        if fault == "absent_inf" and dg[i] - rp[i] < 16 and i >= 2:
            t = 0.0 * y[i - 2]
            acc = acc - t
        if fault == "drop_zero_sign" and acc == 0.0:
            acc = 0.0
        y[i] = acc
        if (False, i) in dump:
            y[dump[(False, i)]] = acc
    for i in range(n - 1, -1, -1):                       # U y = z
        acc = y[i]
        qs = list(range(dg[i] + 1, rp[i + 1]))
        if fault == "reverse":
            qs.reverse()
        piv = lu[dg[i + 1]] if fault == "pivot_neighbour" and i + 1 < n else lu[dg[i]]
        first = True
        for k, q in enumerate(qs):
            v = lu[q]
            if fault == "zero_absent" and v == 0.0:
                continue
            if fault == "divide_early" and k == len(qs) - 1:
                acc = acc / piv
            if first and fault == "fma":
                acc = _fms(acc, v, y[col[q]])
            else:
                t = v * y[col[q]]
                acc = acc - t
            first = False
        if fault == "absent_inf" and len(qs) < 16 and i + 2 < n:
            t = 0.0 * y[i + 2]
            acc = acc - t
        if not (fault == "divide_early" and qs):
            acc = acc / piv                              # no pivot is 0.0: the factorisation refuses those
        if fault == "drop_zero_sign" and acc == 0.0:
            acc = 0.0
        y[i] = acc
        if (True, i) in dump:
            y[dump[(True, i)]] = acc
    return np.array(y, dtype=np.float64)


# ---- the families (ISSUE: each >= 4096 rows and 2 n / (levels lower + upper) >= 32, which the create path requires) --------
LAYERED = {
    "edges": dict(widths=[63, 64, 65, 127, 128, 129, 1, 300, 256, 257, 255, 5, 5, 640, 1000, 700, 200], fan=1),
    "cap48": dict(widths=[10] * 100 + [1000] * 4, fan=2),
    "rows512": dict(widths=[60] * 90, fan=3),
    "faces_wide3": dict(widths=[60] * 90, fan=1, far=2, gap=9),
    "faces_1024": dict(widths=[60] * 90, fan=3, far=3, gap=9),
    "fan20": dict(widths=[200] * 30, fan=20),
    "too_big": dict(widths=[400] * 12, fan=300),
}
STAR_GRIDS = [(6, 6, 114), (683, 6, 1), (37, 37, 3), (64, 64, 1)]
BOX_GRIDS = [(30, 7, 20), (6, 6, 114)]
FAMILIES = list(LAYERED) + ["perm27"] + ["star%dx%dx%d" % d for d in STAR_GRIDS] + ["box%dx%dx%d" % d for d in BOX_GRIDS]
GRID_FAMILIES = [f for f in FAMILIES if f.startswith(("star", "box"))]

_cache = {}


def family(name):
    """The operator of a family (built once per session; treat it as read-only)."""
    if name not in _cache:
        if name in LAYERED:
            A = layered(seed=11, **LAYERED[name])
        elif name == "perm27":
            A = permuted("box", (17, 17, 17), seed=5)
        else:
            dims = tuple(int(d) for d in name[4 if name.startswith("star") else 3:].split("x"))
            A = (star if name.startswith("star") else box)(dims, seed=7)
        for a in (A.rowptr, A.col, A.val):
            a.setflags(write=False)
        _cache[name] = A
    return _cache[name]


def schedules(name):
    """The (ilu_blocks, ilu_grid) pairs a family is created under: default, packed lists only, level-sequence blocks on the grids,
    each block schedule also with 1 and 3 workgroups (every workgroup then takes many blocks in sequence), and level scheduling."""
    out = []
    for b in (1, 2) + ((3,) if name in GRID_FAMILIES else ()):
        out += [(b, 0), (b, 1), (b, 3)]
    return out + [(0, 0)]


def family_dims(name):
    """The grid a family is recognised as ((0, 0, 0): none)."""
    if name not in GRID_FAMILIES:
        return (0, 0, 0)
    return tuple(int(d) for d in name[4 if name.startswith("star") else 3:].split("x"))


# level-sequence blocks (ilu_blocks = 3) are not attempted on these grids: fewer than 32 rows per level
TOO_THIN_FOR_LEVEL_BLOCKS = ("star683x6x1", "box6x6x114")


def expect_paths(name, ilu_blocks, r):
    """Asserts on a path report (Ilu0.path_info() or ilu_paths_host) that the family runs the path it exists for."""
    lo, up = r["lower"], r["upper"]
    if name == "edges":
        # level schedule (in use with ilu_blocks = 0, and what the factorisation always runs): the runs of 7 and of 3 small levels
        # (<= 256 rows: 256 is small, 257 is not) are batched; the run of exactly one small level (256 between 300 and 257; the
        # last 200) is a launch of its own like every wide level
        assert r["levels"] == {k: {"batched": 2, "single": 7} for k in ("factor", "lower", "upper")}, r["levels"]
    if ilu_blocks == 0 or name == "too_big" or (ilu_blocks == 3 and name in TOO_THIN_FOR_LEVEL_BLOCKS):
        assert r["blocks_in_use"] == 0 and lo["blocks"] == up["blocks"] == 0, r
        assert r["attempted"] == (1 if name == "too_big" and ilu_blocks != 0 else 0), r
        assert r["fallback"] == (1 if name == "too_big" and ilu_blocks != 0 else 0), r          # 1: the LDS limit
        return
    assert r["blocks_in_use"] == 1 and r["fallback"] == 0, r
    for t in (lo, up):
        assert t["blocks"] > 0 and t["fast"] + t["wide"] + t["packed"] == t["blocks"], t
        assert t["lds"] <= 150 * 1024 and t["rows_cap"] % 64 == 0 and 64 <= t["rows_cap"] <= 512, t
        assert t["packed_pad0"] == 0, t           # no operator here has a block of 64 local levels or a local level wider than the wave
        long_rows = name in ("fan20", "perm27")
        assert (t["long_row_blocks"] > 0) == long_rows and (t["max_row"] > 16) == long_rows, t
        assert (t["long_face_blocks"] > 0) == (t["max_faces"] > 1024) == (name in ("faces_1024", "perm27")), t
        if ilu_blocks == 2 or long_rows:
            assert t["packed"] == t["blocks"], t
        elif name in ("edges", "cap48", "rows512") or name.startswith("star"):
            assert t["fast"] == t["blocks"] and t["max_row"] <= 3 and t["max_faces"] <= 254, t
        else:                                     # faces_wide3, faces_1024, the box grids
            assert t["wide"] == t["blocks"] and t["max_row"] <= 16, t
        if name == "faces_wide3":
            assert t["max_row"] <= 3 and t["max_faces"] > 254, t      # the wide path only because of the face list
        if name == "faces_1024":
            assert t["max_row"] == 6, t
        if name == "edges":
            assert t["rows_cap"] == 64 and t["max_levels"] == 2, t
        if name == "cap48":
            assert t["max_levels"] == 48, t
        if name == "rows512":
            assert t["rows_cap"] == 512 and t["max_levels"] == 8, t


# ---- the right-hand sides ---------------------------------------------------------------------------------------------------
# Rows where the specials start.  On SPECIALS_STAY_NARROW they were chosen on the CPU so that the oracle's y stays finite in at
# least half of its entries; on every other family no row can (tests/test_ilu_model_host.py shows it), there they are just fixed.
SPECIAL_ROWS = {"edges": [392, 3600], "cap48": [2230], "faces_wide3": [3530], "perm27": [4859]}
SPECIALS_STAY_NARROW = tuple(SPECIAL_ROWS)
STORED_ZERO_FAMILIES = ("edges", "star64x64x1")


def special_rows(name):
    n = family(name).n
    return SPECIAL_ROWS.get(name, [n // 3, n - 40])


def inputs(name):
    """The right-hand sides of a family: seeded normal, all -0.0, the specials, and finite extremes (signed zeros, subnormals,
    +-1e200, +-1e-200 on every 37th row), and ones with a single +Inf in the last row (it reaches the upper solve only)."""
    key = ("x", name)
    if key not in _cache:
        n = family(name).n
        ext = np.ones(n)
        pat = np.array([-0.0, 5e-324, 1e200, -1e200, 1e-200, -1e-300, 0.0])
        at = np.arange(3, n, 37)
        ext[at] = pat[np.arange(at.size) % pat.size]
        one = np.ones(n)
        one[n - 1] = np.inf
        _cache[key] = {"one_inf": one, "normal": np.random.default_rng(len(name) + n).standard_normal(n), "negzero": np.full(n, -0.0),
                       "specials": specials(n, special_rows(name)), "extremes": ext}
        for v in _cache[key].values():
            v.setflags(write=False)
    return _cache[key]


def stored_zeros(name):
    """(the family's operator with three stored 0.0 entries, {input: rows that must come out NaN}): the lower and the upper entry
    of two rows that read the row s where the specials have their first +Inf, and the upper entry of a row that reads the last
    row, where `one_inf` has its +Inf.  A stored 0.0 times an Inf is NaN."""
    A = family(name)
    rows = np.repeat(np.arange(A.n), np.diff(A.rowptr))
    s = special_rows(name)[0]
    hit = np.flatnonzero(A.col == s)
    lower, upper = hit[rows[hit] > s], hit[rows[hit] < s]
    last = np.flatnonzero((A.col == A.n - 1) & (rows < A.n - 1))
    assert lower.size and upper.size and last.size, (name, s)
    return (with_values(A, [lower[0], upper[-1], last[-1]], 0.0),
            {"specials": [int(rows[lower[0]]), int(rows[upper[-1]])], "one_inf": [int(rows[last[-1]])]})
