"""A host model of the row-partitioned SpMV (csrc/api.cpp spmv_any, csrc/spmv.hip spmv_plan / launch_spmv, csrc/comm.cpp).

Operator families with a row partition, the interior range of a slab (ghost_range_kernel), the launches a partitioned product is
made of, the form spmv_plan chooses for a slab under a set of options (with the builders' rules of colcode.hip / coldelta.hip),
a table of which (family, form) is expected to be available, exact references, a NumPy emulation of the partitioned product
that can carry injected faults, and the comparison functions (`judge`).  tests/test_partition_model_host.py shows that the
emulation passes `judge` and that every injected fault is rejected by it; tests/test_gpu_partitioned_spmv_exact.py hands the
device's results to the same `judge`.  Host only: NumPy, fractions (through exact_reduction) and the oracle's serial loop.

Values: the host-built families (grid7 / grid27 / banded / midrow) carry seeded normal values times 2^k, unsymmetric; a few rows
have no diagonal entry (the only rows on which a padding slot read as an entry, 0 * x[row], can show).  The families of the
device generators (poisson / kron_unsymmetric / stencil27) carry the generators' values: the row-template form needs rows that
repeat.

An empty slab (m = 0) is left out: include/krylov_hip.h states for khip_csr_create_dist that "this rank owns global rows
[row0, row0 + m)" and nothing about a rank that owns none; csr_create_common admits m = 0 but comm_build_plan sizes its
exchange buffers with max(..., 1) without saying that a rank without rows is part of the contract.
"""
import math
import os
import re
import sys
from dataclasses import dataclass, field

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
for _p in (_HERE, os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import exact_reduction as er  # noqa: E402

# ---------------------------------------------------------------------------------------------------- constants of the sources
HOLE_ALIGN = 256          # launch_spmv: one two-range launch only when (hole_lo - row_lo) & 255 == 0
BLOCKPTR_ALIGN = 256      # launch_spmv: a.blockptr only when (row_lo & 255) == 0
SLICE = 64                # sliced kernels: slice of a row = rowl >> 6
ROW_BLOCKS = (256, 128, 64, 32)
STAGE_WINDOW = 2048.0     # entries of the LDS window: rows * mean_row_nnz above it halves the row block
ONE_RANGE_OPTIONS = ("spmv_persist", "spmv_nt", "spmv_delta", "spmv_wide")      # spmv_plan p.one_range
STAGED_FAMILY = ("Staged", "Coded", "Sliced", "Sliced32")                        # SpmvPlan::staged_family
CODED_MAX_ROW = 64        # kCodedMaxRow
CODE_MAX = 2048           # kCodeMax: distinct diagonals at most
SELL_MAX_PAD = 1.20       # kSellMaxPad
SELL_SLACK = 65536.0
BIG_NNZ = 1 << 22
TMPL_MAX_LEN, TMPL_MAX, TMPL_LDS_MAX = 32, 1024, 60 * 1024      # template.hip: entries per row, distinct templates, table bytes


def source_constants(root=ROOT):
    """The same constants read out of the sources (tests/test_partition_model_host.py compares)."""
    src = os.path.join(root, "krylov.jl_amd", "csrc")
    spmv = open(os.path.join(src, "spmv.hip")).read()
    internal = open(os.path.join(src, "khip_internal.hpp")).read()
    colcode = open(os.path.join(src, "colcode.hip")).read()
    api = open(os.path.join(src, "api.cpp")).read()
    csr_aux = open(os.path.join(src, "csr_aux.hip")).read()
    out = {}
    m = re.search(r"takes_two_ranges\(\) && \(\(hole_lo - row_lo\) & (\d+)\) == 0", spmv)
    out["hole_align"] = int(m.group(1)) + 1 if m else None
    m = re.search(r"a\.blockptr = \(A->blockptr && \(row_lo & (\d+)\) == 0\)", spmv)
    out["blockptr_align"] = int(m.group(1)) + 1 if m else None
    out["slice"] = {1 << int(s) for s in re.findall(r"const int64_t sl = rowl >> (\d+);", spmv)}
    out["row_blocks"] = {tuple(int(v) for v in t) for t in
                         re.findall(r"if \(rows != (\d+) && rows != (\d+) && rows != (\d+) && rows != (\d+)\) rows = 256;", spmv)}
    out["stage_window"] = {float(v) for v in re.findall(r"rows \* A->mean_row_nnz > ([0-9.]+)\)", spmv)}
    m = re.search(r"p\.one_range = (.*?);", spmv)
    out["one_range"] = tuple(sorted(set(re.findall(r"spmv_\w+", m.group(1))) | ({"spmv_nt"} if re.search(r"\bnt\b", m.group(1)) else set()))) if m else None
    m = re.search(r"bool staged_family\(\) const \{ return (.*?); \}", internal)
    out["staged_family"] = tuple(re.findall(r"SpmvForm::(\w+)", m.group(1))) if m else None
    out["takes_two_ranges"] = "bool takes_two_ranges() const { return staged_family() && !one_range; }" in internal
    out["delta_guard"] = "const bool delta = plan.delta && row_lo % A->delta_rows == 0;" in spmv
    m = re.search(r"constexpr int kCodedMaxRow = (\d+);", spmv)
    out["coded_max_row"] = int(m.group(1)) if m else None
    m = re.search(r"constexpr int kCodeMax = (\d+);", colcode)
    out["code_max"] = int(m.group(1)) if m else None
    m = re.search(r"constexpr double kSellMaxPad = ([0-9.]+);", colcode)
    out["sell_max_pad"] = float(m.group(1)) if m else None
    out["sell_rule"] = "if (512.0 * (double)total > kSellMaxPad * ref_bytes + 65536.0) return KHIP_OK;" in colcode
    out["sell_limits"] = ("A->max_row_nnz > 64) return KHIP_OK;" in colcode and
                          "A->code_bits != 8 || A->code_T > 255)) return KHIP_OK;" in colcode)
    out["try32_rule"] = "const bool try32 = !coded && t.spmv_sell && !nt && rows == 256 && (t.spmv_codes == 2 || t.spmv_sell >= 3 || big);" in spmv
    tmpl = open(os.path.join(src, "template.hip")).read()
    m = re.search(r"constexpr int kTmplMaxLen = (\d+);.*?constexpr int kTmplMax = (\d+);.*?constexpr size_t kTmplLdsMax = (\d+) \* 1024;", tmpl, re.S)
    out["template"] = tuple(int(v) for v in m.groups()) if m else None
    out["template_rule"] = ("if (m == 0 || A->max_row_nnz > kTmplMaxLen || A->max_row_nnz < 1) return KHIP_OK;" in tmpl and
                            "if (T == 0 || T > kTmplMax || (size_t)T * K * 12 + (size_t)T * 4 > kTmplLdsMax) return KHIP_OK;" in tmpl)
    out["big"] = "const bool big = A->nnz >= ((int64_t)1 << 22);" in spmv
    # spmv_any: the interior launch first, then the boundary launch over [0, m) with the interior as its hole
    out["split_rule"] = "const bool split = ctx->tune.overlap_halo && A->interior_hi > A->interior_lo;" in api
    out["interior_launch"] = "launch_spmv(ctx, A, x, y, dot_slot, A->interior_lo, A->interior_hi, &cursor, false, dotw, dot_sq)" in api
    out["boundary_launch"] = "launch_spmv(ctx, A, x, y, dot_slot, 0, A->m, &cursor, true, dotw, dot_sq, A->interior_lo, A->interior_hi)" in api
    out["ghost_range"] = ("if (i < m / 2) atomicMax(&lo_hi[0], (unsigned long long)(i + 1));" in csr_aux and
                          "else atomicMin(&lo_hi[1], (unsigned long long)i);" in csr_aux and
                          "if (lo_hi_host[1] < lo_hi_host[0]) lo_hi_host[1] = lo_hi_host[0];" in csr_aux)
    return out


# ---------------------------------------------------------------------------------------------------- operators

def _values(rng, k):
    return rng.standard_normal(k) * np.exp2(rng.integers(-3, 4, k))


def grid_operator(n1, n2, n3, points, seed):
    """7- or 27-point operator on an n1 x n2 x n3 grid (row = i + n1 (j + n2 k)), columns increasing per row; rows with
    i = j = 0 and odd k have no diagonal entry."""
    n = n1 * n2 * n3
    r = np.arange(n)
    i, j, k = r % n1, (r // n1) % n2, r // (n1 * n2)
    rows, cols = [], []
    for dk in (-1, 0, 1):
        for dj in (-1, 0, 1):
            for di in (-1, 0, 1):
                if points == 7 and abs(di) + abs(dj) + abs(dk) > 1:
                    continue
                ok = (i + di >= 0) & (i + di < n1) & (j + dj >= 0) & (j + dj < n2) & (k + dk >= 0) & (k + dk < n3)
                if di == dj == dk == 0:
                    ok &= ~((i == 0) & (j == 0) & (k % 2 == 1))
                rows.append(r[ok])
                cols.append(r[ok] + di + n1 * (dj + n2 * dk))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    order = np.argsort(rows, kind="stable")           # offsets were visited in increasing column order
    rows, cols = rows[order], cols[order]
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=rowptr[1:])
    return rowptr, cols.astype(np.int32), _values(np.random.default_rng(seed), cols.size)


def banded_operator(starts, half_band, interiors, seed, keep=1.0, links=1):
    """Band of half width `half_band` (thinned to the share `keep`) plus `links` long-range entries into other ranks' columns in
    every row outside the chosen local interior [lo, hi) of its slab (interiors[rank]; None = links in every row).  Every
    seventeenth row has no diagonal entry."""
    n, world = starts[-1], len(starts) - 1
    rng = np.random.default_rng(seed)
    rowptr, cols = [0], []
    for rank in range(world):
        r0, r1 = starts[rank], starts[rank + 1]
        m = r1 - r0
        lohi = interiors[rank]
        for r in range(r0, r1):
            c = np.arange(max(0, r - half_band), min(n, r + half_band + 1))
            if keep < 1.0:
                c = c[(rng.random(c.size) < keep) | (c == r)]
            if r % 17 == 5:
                c = c[c != r]
            loc = r - r0
            if world > 1 and (lohi is None or loc < lohi[0] or loc >= lohi[1]):
                extra = []
                for t in range(links):
                    peer = (rank + 1 + (r + t) % (world - 1)) % world
                    size = starts[peer + 1] - starts[peer]
                    extra.append(starts[peer] + (r * 7919 + 17 + 31 * t) % size)
                c = np.union1d(c, np.array(extra, dtype=c.dtype))
            cols.append(c)
            rowptr.append(rowptr[-1] + c.size)
    cols = np.concatenate(cols)
    return np.array(rowptr, dtype=np.int64), cols.astype(np.int32), _values(rng, cols.size)


@dataclass
class Family:
    name: str
    kind: str                       # grid7 | grid27 | banded | midrow | gen
    stencil: bool
    align: str                      # a256 | a64 | a32 | odd | empty | shape
    sizes: tuple                    # rows per rank
    args: dict = field(default_factory=dict)
    gen: tuple = None               # (kind, n1, n2, n3) of the device generator
    unavailable: dict = field(default_factory=dict)      # form -> reason taken from the builder's rule

    @property
    def world(self):
        return len(self.sizes)

    @property
    def starts(self):
        return [0] + [int(v) for v in np.cumsum(self.sizes)]


def _planes(plane, counts):
    return tuple(plane * c for c in counts)


_NO_TEMPLATE = ("seeded values, every row is a template of its own: more than kTmplMax = 1024 of them, or a table of more than 60 KiB "
                "(12 B per entry of the longest row + 4 B, per template)")
_LONG_TEMPLATE = "max_row_nnz > kTmplMaxLen = 32: khip_csr_compress leaves the handle CSR"
_R_27 = "rows == 256 fails: 256 x mean row length > 2048 halves the row block of the staged family"
_R_16BIT = "more than 256 diagonals (code_bits == 16): csr_build_sell takes 8-bit codes only"
_R_NARROW = "narrow codes need <= 15 diagonals and rows of <= 8 entries: the plain sliced layout is built"


def _unav(*pairs, template=_NO_TEMPLATE):
    d = {"template": template} if template else {}
    for forms, reason in pairs:
        for f in forms:
            d[f] = reason
    return d


_SLICED_FORMS = ("sliced", "sliced_plain", "sliced_narrow", "sliced_tiles2", "sliced_tiles3")
_U_GRID7 = _unav()
_U_GRID27 = _unav((("sliced32", "sliced32_pair"), _R_27), (("sliced_narrow",), _R_NARROW))
_U_GEN7 = {}
_U_GEN27 = {"sliced32": _R_27, "sliced32_pair": _R_27, "sliced_narrow": _R_NARROW}
_U_BAND16 = _unav((_SLICED_FORMS, _R_16BIT), (("coded8",), _R_16BIT))
_U_BAND8 = _unav((("sliced_narrow",), _R_NARROW))
_R_CODEMAX = "more than kCodeMax = 2048 diagonals: csr_build_codes leaves the int32 columns"
_U_BAND_CODEMAX = _unav((_SLICED_FORMS + ("coded8", "coded16"), _R_CODEMAX))
_U_MID = _unav((_SLICED_FORMS + ("coded8",), _R_16BIT), (("sliced32", "sliced32_pair"), _R_27), template=_LONG_TEMPLATE)
_U_SHAPES = _unav((("sliced_narrow",), _R_NARROW), (("sliced32", "sliced32_pair"), _R_27), template=None)
_U_GRID7_SMALL = _unav(template=None)                 # slabs of a few hundred short rows: one template per row fits
_U_BAND16_SMALL = _unav((_SLICED_FORMS, _R_16BIT), (("coded8",), _R_16BIT), template=None)

FAMILIES = [
    # grids built on the host: a slab of whole planes has interior_lo = one plane
    Family("g7_256", "grid7", True, "a256", _planes(256, (4, 5, 4)), dict(dims=(16, 16)), unavailable=_U_GRID7),
    Family("g7_64", "grid7", True, "a64", _planes(192, (4, 4, 4, 4)), dict(dims=(8, 24)), unavailable=_U_GRID7),
    Family("g7_32", "grid7", True, "a32", _planes(96, (3,) * 8), dict(dims=(8, 12)), unavailable=_U_GRID7_SMALL),
    Family("g7_odd", "grid7", True, "odd", _planes(225, (4, 4, 5)), dict(dims=(15, 15)), unavailable=_U_GRID7),
    Family("g27_256", "grid27", True, "a256", _planes(256, (4, 4, 4)), dict(dims=(16, 16)), unavailable=_U_GRID27),
    Family("g27_64", "grid27", True, "a64", _planes(64, (5, 4, 6, 4)), dict(dims=(8, 8)), unavailable=_U_GRID27),
    Family("g27_32", "grid27", True, "a32", _planes(32, (6, 6, 6, 6)), dict(dims=(4, 8)), unavailable=_U_GRID27),
    Family("g27_odd", "grid27", True, "odd", _planes(63, (4, 5, 4)), dict(dims=(9, 7)), unavailable=_U_GRID27),
    # the device generators' operators (K.CsrMatrix.stencil(..., distributed=True)): the row-template form
    Family("dg_kron_256", "gen", True, "a256", _planes(256, (4, 4, 4, 4)), gen=("kron_unsymmetric", 16, 16, 16), unavailable=_U_GEN7),
    Family("dg_poisson_64", "gen", True, "a64", _planes(64, (4, 4, 4, 4)), gen=("poisson", 8, 8, 16), unavailable=_U_GEN7),
    Family("dg_poisson_32", "gen", True, "a32", _planes(96, (3, 3, 3, 3)), gen=("poisson", 8, 12, 12), unavailable=_U_GEN7),
    Family("dg_poisson_odd", "gen", True, "odd", _planes(225, (4, 4, 4)), gen=("poisson", 15, 15, 12), unavailable=_U_GEN7),
    Family("dg_s27_256", "gen", True, "a256", _planes(256, (4, 4, 4, 4)), gen=("stencil27", 16, 16, 16), unavailable=_U_GEN27),
    # band + long-range links outside a chosen interior
    Family("bd_256", "banded", False, "a256", (1024, 1024, 1024), dict(half_band=3, interiors=[(256, 768)] * 3), unavailable=_U_BAND16),
    Family("bd_64", "banded", False, "a64", (900, 1000, 900, 800), dict(half_band=3, interiors=[(192, 600)] * 4), unavailable=_U_BAND16),
    Family("bd_32", "banded", False, "a32", (640, 640, 640), dict(half_band=3, interiors=[(32, 608)] * 3), unavailable=_U_BAND8),
    Family("bd_odd", "banded", False, "odd", (700, 811, 650), dict(half_band=3, interiors=[(177, 501)] * 3), unavailable=_U_BAND16),
    # rows of 30-90 entries: spmv_kernel = 0 gives the stream kernel, the delta stream builds
    Family("mid_256", "midrow", False, "a256", (1024, 1024, 1024), dict(half_band=45, keep=0.72, interiors=[(256, 768)] * 3), unavailable=_U_MID),
    Family("mid_64", "midrow", False, "a64", (960, 960, 960), dict(half_band=45, keep=0.72, interiors=[(192, 832)] * 3), unavailable=_U_MID),
    # slabs of a few times 10^4 rows: thousands of reduction partials per launch (the finish kernel's multi-workgroup path),
    # boundary ranges of several 256-row blocks, sliced builds decided by kSellMaxPad and not by its 64 KiB of slack
    Family("g7_big_256", "grid7", True, "a256", _planes(4096, (8, 7, 8)), dict(dims=(64, 64)), unavailable=_U_GRID7),
    Family("g7_big_odd", "grid7", True, "odd", _planes(4095, (8, 8, 8)), dict(dims=(63, 65)), unavailable=_U_GRID7),
    Family("bd_big_256", "banded", False, "a256", (32768, 30000, 32768), dict(half_band=3, interiors=[(4096, 27000)] * 3), unavailable=_U_BAND_CODEMAX),
    Family("bd_big_odd", "banded", False, "odd", (30001, 32768, 31000), dict(half_band=3, interiors=[(1027, 29101), (1027, 31868), (1027, 30100)]), unavailable=_U_BAND16),
    # lopsided and degenerate slabs
    Family("g7_two", "grid7", True, "shape", _planes(256, (4, 4)), dict(dims=(16, 16)), unavailable=_U_GRID7),        # rank 0: lo = 0; rank 1: hi = m
    Family("g7_empty", "grid7", True, "empty", _planes(512, (1, 1, 1)), dict(dims=(16, 32)), unavailable=_U_GRID7_SMALL),   # every plane touches a neighbour
    Family("bd_empty", "banded", False, "empty", (500, 500, 500), dict(half_band=3, interiors=[None] * 3), unavailable=_U_BAND16_SMALL),
    Family("bd_shapes", "banded", False, "shape", (40, 1, 300, 130), dict(half_band=4, interiors=[(8, 30), None, (70, 200), (33, 100)]),
           unavailable=_U_SHAPES),                                                                                      # m < 64, one row, m % 64 != 0, unequal
    Family("g27_world8", "grid27", True, "a64", _planes(64, (4,) * 8), dict(dims=(8, 8)), unavailable=_U_GRID27),
]
FAMILY = {f.name: f for f in FAMILIES}


def align_class(lo):
    if lo % 256 == 0:
        return "a256"
    if lo % 64 == 0:
        return "a64"
    if lo % 32 == 0:
        return "a32"
    return "odd" if lo % 2 else "other"


# ---------------------------------------------------------------------------------------------------- forms and their options
# every form names ALL the options it depends on, on top of BASE (a test session runs with KHIP_SPMV_CODES = 2 and
# KHIP_SPMV_DELTA = 2 in the environment: spmv_delta != 0 alone makes every staged launch one range)
BASE = dict(spmv_kernel=0, spmv_codes=2, spmv_sell=2, spmv_sell_pair=1, spmv_sell_narrow=0, spmv_rows=256, spmv_vec=1, spmv_wide=0,
            spmv_delta=0, spmv_tiles=1, spmv_blk_pub=0, spmv_xcd=0, spmv_lanes=0, spmv_template=1, spmv_nt=0, spmv_persist=0,
            compensated=1)


def _f(want, **kw):
    return dict(want=want, opts=dict(BASE, **kw))


FORMS = {
    "staged": _f("Staged", spmv_kernel=4, spmv_codes=0, spmv_sell=0),
    "staged_tiles2": _f("Staged", spmv_kernel=4, spmv_codes=0, spmv_sell=0, spmv_tiles=2),
    "staged_tiles3_pub": _f("Staged", spmv_kernel=4, spmv_codes=0, spmv_sell=0, spmv_tiles=3, spmv_blk_pub=1),
    "staged_xcd": _f("Staged", spmv_kernel=4, spmv_codes=0, spmv_sell=0, spmv_xcd=2, spmv_tiles=2),
    "staged_one_range": _f("Staged", spmv_kernel=4, spmv_codes=0, spmv_sell=0, spmv_delta=2),
    "staged_plain_sum": _f("Staged", spmv_kernel=4, spmv_codes=0, spmv_sell=0, compensated=0),
    "coded8": _f("Coded8", spmv_kernel=4, spmv_sell=0),
    "coded16": _f("Coded16", spmv_kernel=4, spmv_sell=0, spmv_codes=16),
    "sliced": _f("Sliced", spmv_kernel=4),
    "sliced_plain": _f("Sliced", spmv_kernel=4, spmv_sell=1, spmv_sell_pair=0),
    "sliced_narrow": _f("SlicedNarrow", spmv_kernel=4, spmv_sell_narrow=1),
    "sliced_tiles2": _f("Sliced", spmv_kernel=4, spmv_tiles=2, spmv_blk_pub=1),
    "sliced_tiles3": _f("Sliced", spmv_kernel=4, spmv_tiles=3),
    "sliced32": _f("Sliced32", spmv_kernel=4, spmv_codes=0, spmv_sell=3),
    "sliced32_pair": _f("Sliced32", spmv_kernel=4, spmv_codes=0, spmv_sell=3, spmv_sell_pair=2, spmv_tiles=2),
    "stream256": _f("Stream", spmv_kernel=1, spmv_rows=256),
    "stream128_vec2": _f("Stream", spmv_kernel=1, spmv_rows=128, spmv_vec=2),
    "stream64": _f("Stream", spmv_kernel=1, spmv_rows=64),
    "stream32_vec2": _f("Stream", spmv_kernel=1, spmv_rows=32, spmv_vec=2),
    "wide": _f("StreamWide", spmv_kernel=1, spmv_wide=1),
    "delta8": _f("StreamDelta8", spmv_kernel=1, spmv_delta=8),
    "delta16": _f("StreamDelta16", spmv_kernel=1, spmv_delta=16, spmv_blk_pub=1),
    "wave": _f("Wave", spmv_kernel=6),
    "template": _f("Template", spmv_kernel=0),
    "ordered": _f("Ordered", spmv_kernel=3),
    "ordered_lanes8": _f("Ordered", spmv_kernel=3, spmv_lanes=8),
    "vector": _f("Vector", spmv_kernel=2),
}
TWO_REDUCTION_FORMS = ("Ordered", "Vector")          # spmv_any: spmv_dot2 as two reductions


def table():
    """(family, form) -> (available, reason)."""
    return {(f.name, form): ((form not in f.unavailable), f.unavailable.get(form, "")) for f in FAMILIES for form in FORMS}


# ---------------------------------------------------------------------------------------------------- the partitioned operator

def interior_range(rowptr, lcol, m):
    """ghost_range_kernel + launch_row_ghost_range: [lo, hi) references no ghost column."""
    touch = np.zeros(m, dtype=bool)
    rows = np.repeat(np.arange(m), np.diff(rowptr))
    touch[rows[lcol >= m]] = True
    t = np.flatnonzero(touch)
    low, high = t[t < m // 2], t[t >= m // 2]
    lo = int(low.max()) + 1 if low.size else 0
    hi = int(high.min()) if high.size else m
    return lo, max(hi, lo)


class Slab:
    def __init__(self, rank, r0, r1, rowptr, gcol, val, starts):
        self.rank, self.r0, self.r1, self.m = rank, r0, r1, r1 - r0
        self.rowptr, self.gcol, self.val, self.starts = rowptr, gcol, val, starts
        own = (gcol >= r0) & (gcol < r1)
        self.ghost_gid = np.unique(gcol[~own])                       # neighbour mode: sorted unique off-slab columns
        self.maxm = max(1, max(b - a for a, b in zip(starts[:-1], starts[1:])))
        self.world = len(starts) - 1
        self.lens = np.diff(rowptr)
        self.row_of = np.repeat(np.arange(self.m), self.lens)
        self._lcol = {}

    def lcol(self, mode):
        """Columns in [owned | ghost] numbering (col_remap_kernel / col_remap_gather_kernel)."""
        if mode not in self._lcol:
            g = self.gcol.astype(np.int64)
            own = (g >= self.r0) & (g < self.r1)
            if mode == "neighbour":
                out = np.where(own, g - self.r0, self.m + np.searchsorted(self.ghost_gid, g))
            else:
                st = np.asarray(self.starts[:-1])
                owner = np.searchsorted(st, g, side="right") - 1
                out = np.where(own, g - self.r0, self.m + owner * self.maxm + (g - st[owner]))
            self._lcol[mode] = out.astype(np.int64)
        return self._lcol[mode]

    def n_ghost(self, mode):
        return self.ghost_gid.size if mode == "neighbour" else self.world * self.maxm

    def ghost_buffer(self, mode, x):
        if mode == "neighbour":
            return x[self.ghost_gid].copy()
        buf = np.zeros(self.world * self.maxm)
        for r in range(self.world):
            a, b = self.starts[r], self.starts[r + 1]
            buf[r * self.maxm:r * self.maxm + (b - a)] = x[a:b]
        return buf

    def interior(self, mode):
        return interior_range(self.rowptr, self.lcol(mode), self.m)

    def templates(self, mode):
        """khip_csr_compress on this slab: the number of distinct (column - row, value) rows when the handle compresses, else 0."""
        K = int(self.lens.max()) if self.m else 0
        if self.m == 0 or K > TMPL_MAX_LEN or K < 1:
            return 0
        d = self.lcol(mode) - self.row_of
        rows = {(tuple(d[a:b]), self.val[a:b].tobytes()) for a, b in zip(self.rowptr[:-1], self.rowptr[1:])}
        T = len(rows)
        return T if (T <= TMPL_MAX and T * K * 12 + T * 4 <= TMPL_LDS_MAX) else 0

    def info(self, mode):
        nnz = int(self.rowptr[-1])
        d = np.unique(self.lcol(mode) - self.row_of) if nnz else np.zeros(0)
        return dict(m=self.m, nnz=nnz, max_row=int(self.lens.max()) if self.m else 0, mean_row=nnz / self.m if self.m else 0.0,
                    diagonals=int(d.size), lens=self.lens)


class Partitioned:
    def __init__(self, fam):
        self.fam = fam
        self.starts = fam.starts
        self.n = self.starts[-1]
        if fam.kind == "gen":
            import oracle as ok
            kind, n1, n2, n3 = fam.gen
            A = {"poisson": lambda: ok.poisson3d(n1, n2, n3), "kron_unsymmetric": lambda: ok.kron_unsymmetric(n1),
                 "stencil27": lambda: ok.stencil27_unsym(n1)}[kind]()
            assert A.n == self.n, (fam.name, A.n, self.n)
            self.rowptr, self.col, self.val = A.rowptr.astype(np.int64).copy(), A.col.copy(), A.val.copy()
        elif fam.kind in ("grid7", "grid27"):
            n1, n2 = fam.args["dims"]
            assert self.n % (n1 * n2) == 0
            self.rowptr, self.col, self.val = grid_operator(n1, n2, self.n // (n1 * n2), 7 if fam.kind == "grid7" else 27, _seed(fam.name))
        else:
            self.rowptr, self.col, self.val = banded_operator(self.starts, fam.args["half_band"], fam.args["interiors"], _seed(fam.name),
                                                              keep=fam.args.get("keep", 1.0))
        self.slabs = []
        for rank in range(fam.world):
            r0, r1 = self.starts[rank], self.starts[rank + 1]
            a, b = int(self.rowptr[r0]), int(self.rowptr[r1])
            self.slabs.append(Slab(rank, r0, r1, self.rowptr[r0:r1 + 1] - a, self.col[a:b], self.val[a:b], self.starts))

    def matvec(self, x):
        """The serial stored-order loop (one rounded multiply, one rounded add per entry): the oracle's ko_spmv."""
        import oracle as ok
        return ok.CsrMatrix.from_arrays(self.rowptr, self.col, self.val).matvec(x)

    def whole_info(self):
        """What predict() reads, for the operator as one whole handle."""
        lens = np.diff(self.rowptr)
        rows = np.repeat(np.arange(self.n), lens)
        return dict(m=self.n, nnz=int(self.rowptr[-1]), max_row=int(lens.max()), mean_row=float(self.rowptr[-1]) / self.n,
                    diagonals=int(np.unique(self.col.astype(np.int64) - rows).size), lens=lens)

    def whole_templates(self):
        whole = Slab(0, 0, self.n, self.rowptr, self.col, self.val, [0, self.n])
        return whole.templates("neighbour")

    def has_column(self, col):
        """Rows that reference `col`."""
        rows = np.repeat(np.arange(self.n), np.diff(self.rowptr))
        return np.unique(rows[self.col == col])


def _seed(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name)) % (1 << 31)


_CACHE = {}


def partitioned(name):
    if name not in _CACHE:
        _CACHE[name] = Partitioned(FAMILY[name])
    return _CACHE[name]


# ---------------------------------------------------------------------------------------------------- the plan

def _sell_units(L, mode):
    """sell_units_kernel."""
    if L <= 0:
        return 0
    Lp = L + (L & 1)
    h4 = (Lp // 2) + ((Lp // 2) & 1)
    h5 = ((L + 7) // 8) + (((L + 7) // 8) & 1)
    if mode == 5:
        return Lp + h5
    if mode == 4:
        return Lp + h4
    if mode == 3:
        return 2 * ((L + 2) // 2)
    return L + (0 if mode == 2 else ((L + 1) // 2 if mode == 1 else (L + 7) // 8))


def _sell_builds(info, o, cols32, code_T=0):
    """build_sell_form: (built, narrow)."""
    m, nnz = info["m"], info["nnz"]
    if m == 0 or nnz == 0 or info["max_row"] > 64:
        return False, False
    if not cols32 and code_T > 255:
        return False, False
    narrow = (not cols32) and bool(o["spmv_sell_narrow"]) and code_T <= 15 and info["max_row"] <= 8
    pair = (not narrow) and bool(o["spmv_sell_pair"])
    if cols32:
        mode = 4 if (pair and o["spmv_sell_pair"] >= 2) else 1
    else:
        mode = 2 if narrow else ((3 if info["max_row"] <= 8 else 5) if pair else 0)
    lens = info["lens"]
    total = 0
    for s in range(0, m, SLICE):
        total += _sell_units(int(lens[s:s + SLICE].max()), mode)
    ref = (12.0 if cols32 else 9.0) * nnz + 4.0 * m
    return 512.0 * total <= SELL_MAX_PAD * ref + SELL_SLACK, narrow


def predict(info, o, compressed=False):
    """spmv_kernel_choice + spmv_plan + the builders' rules on one slab: dict(kernel, form, rows, code_bits, delta_bits,
    delta_rows, one_range)."""
    nt = o["spmv_nt"] != 0
    big = info["nnz"] >= BIG_NNZ
    codes = o["spmv_codes"]
    try_codes = bool(codes) and (codes != 1 or big) and not nt
    tmpl = compressed and o["spmv_template"]
    code_bits = 32
    if try_codes and not tmpl and (o["spmv_kernel"] == 4 or (o["spmv_kernel"] == 0 and info["max_row"] <= CODED_MAX_ROW)):
        T = info["diagonals"]
        if info["m"] and info["nnz"] and 0 < T <= CODE_MAX:
            code_bits = 8 if (T <= 256 and codes != 16) else 16
    kernel = o["spmv_kernel"]
    if tmpl:
        kernel = 5
    elif kernel == 0:
        short = info["mean_row"] <= 12.0 and info["max_row"] <= CODED_MAX_ROW
        coded = code_bits != 32 and info["max_row"] <= CODED_MAX_ROW
        kernel = 4 if (short or coded) else (1 if info["mean_row"] <= 96.0 else 2)
    out = dict(kernel=kernel, code_bits=32, delta_bits=32, delta_rows=0, narrow=False,
               one_range=any(o[k] != 0 for k in ONE_RANGE_OPTIONS))
    rows = o["spmv_rows"]
    mean = info["mean_row"]
    if kernel == 5:
        out["form"] = "Template"
    elif kernel == 6:
        out["form"] = "Wave"
    elif kernel == 3:
        out["form"] = "Ordered"
    elif kernel == 2:
        out["form"] = "Vector"
    elif kernel == 1:
        if rows * mean > STAGE_WINDOW:
            rows = 256
            while rows > 32 and rows * mean > STAGE_WINDOW:
                rows >>= 1
        if rows not in ROW_BLOCKS:
            rows = 256
        dl = o["spmv_delta"]
        wide_ok = (not nt) and o["spmv_vec"] != 2 and o["spmv_persist"] == 0 and info["nnz"] > 0
        delta = False
        if wide_ok and dl and (dl != 1 or big) and info["m"] > 0:
            if dl in (8, 16):
                delta, out["delta_bits"] = True, dl            # a forced width always builds (blocks of <= 65535 entries)
                out["delta_rows"] = min(rows, 64) if dl == 8 else rows
            else:
                delta = None                                   # the cheaper width: not restated, no form relies on it
        out["form"] = "StreamDelta%d" % dl if delta else ("StreamWide" if (wide_ok and o["spmv_wide"]) else "Stream")
        assert delta is not None, "spmv_delta = 1 / 2 with the stream kernel is not modelled"
    else:
        if rows not in ROW_BLOCKS:
            rows = 256
        coded = try_codes and code_bits != 32
        out["code_bits"] = code_bits if coded else 32
        sliced = False
        if coded and o["spmv_sell"] and code_bits == 8:
            sliced, out["narrow"] = _sell_builds(info, o, False, info["diagonals"])
        if sliced:
            out["form"] = "SlicedNarrow" if out["narrow"] else "Sliced"
        else:
            out["narrow"] = False
            while rows > 32 and rows * mean > STAGE_WINDOW:
                rows >>= 1
            try32 = (not coded) and bool(o["spmv_sell"]) and not nt and rows == 256 and (codes == 2 or o["spmv_sell"] >= 3 or big)
            if coded:
                out["form"] = "Coded%d" % code_bits
            elif try32 and _sell_builds(info, o, True)[0]:
                out["form"] = "Sliced32"
            else:
                out["form"] = "Staged"
    out["rows"] = rows
    return out


def family_of(form):
    """The SpmvForm behind a form name of this file."""
    for f in ("Sliced32", "Sliced", "Coded", "Staged", "Stream", "Wave", "Template", "Ordered", "Vector"):
        if form.startswith(f):
            return f
    raise ValueError(form)


def launches(form, options, lo, hi, m, delta_rows=0):
    """spmv_any + launch_spmv: the kernel launches of one partitioned product, in order.  Each is a dict(ranges = [(a, b), ...]
    (two ranges = one launch with a hole), part = whole | interior | boundary, delta = the launch reads the delta stream,
    blockptr = it is given the handle's block pointers)."""
    fam = family_of(form)
    one_range = any(options[k] != 0 for k in ONE_RANGE_OPTIONS)
    is_delta = form.startswith("StreamDelta")

    def launch(part, *ranges):
        ranges = [(a, b) for a, b in ranges if b > a]
        if not ranges:
            return []
        a0 = ranges[0][0]
        return [dict(ranges=ranges, part=part, delta=is_delta and delta_rows > 0 and a0 % delta_rows == 0,
                     blockptr=a0 % BLOCKPTR_ALIGN == 0)]

    split = bool(options.get("overlap_halo", 1)) and hi > lo
    if not split:
        return launch("whole", (0, m))
    out = launch("interior", (lo, hi))
    if lo == 0 or hi == m:                                             # one of the ranges is empty: an ordinary launch
        return out + launch("boundary", (hi, m) if lo == 0 else (0, lo))
    if fam in STAGED_FAMILY and not one_range and lo % HOLE_ALIGN == 0:
        return out + launch("boundary", (0, lo), (hi, m))
    return out + launch("boundary", (0, lo)) + launch("boundary", (hi, m))


# ---------------------------------------------------------------------------------------------------- inputs and references

def _vec(rng, n):
    return rng.standard_normal(n) * np.exp2(rng.integers(-4, 5, n))


def special_columns(P):
    """((inf_owned, nan_owned), (inf_ghost, nan_ghost)): columns no other rank reads -- the first one, where there is one, the
    column of a row without a diagonal entry that is shorter than the longest row of its 64-row slice -- and columns that are
    ghosts on a neighbour; and whether columns that no other rank reads exist at all."""
    ghost = np.zeros(P.n, dtype=bool)
    for s in P.slabs:
        ghost[s.ghost_gid] = True
    rows = np.repeat(np.arange(P.n), np.diff(P.rowptr))
    has_diag = np.zeros(P.n, dtype=bool)
    has_diag[rows[P.col == rows]] = True
    lens = np.diff(P.rowptr)
    cand = []
    for s in P.slabs:
        for c in np.flatnonzero(~has_diag[s.r0:s.r1] & ~ghost[s.r0:s.r1]):
            sl = (c // SLICE) * SLICE
            if lens[s.r0 + c] < lens[s.r0 + sl:s.r0 + min(sl + SLICE, s.m)].max():
                cand.append(s.r0 + int(c))
    own = np.flatnonzero(~ghost)
    private = own.size >= 2
    if not private:                                   # every column is somebody's ghost (empty interiors): any two columns
        own = np.arange(P.n)
    inf_owned = cand[len(cand) // 2] if cand else int(own[own.size // 3])
    nan_owned = int(own[(2 * own.size) // 3])
    if nan_owned == inf_owned:
        nan_owned = int(own[-1])
    g = np.flatnonzero(ghost)
    return (inf_owned, nan_owned), (int(g[g.size // 3]), int(g[(2 * g.size) // 3])), private


def make_inputs(P, cond=1e10):
    """x_a, x_b, the two special vectors, a weight vector and an ill-conditioned weight vector whose cancelling partners lie
    on different ranks (gen_dot(..., place="ranks") on y = A x_a)."""
    rng = np.random.default_rng(_seed(P.fam.name) + 1)
    xa, xb, w = _vec(rng, P.n), _vec(rng, P.n), _vec(rng, P.n)
    sp = []
    for (ci, cn) in special_columns(P)[:2]:
        x = _vec(rng, P.n)
        x[ci], x[cn] = np.inf, np.nan
        sp.append(x)
    ya = P.matvec(xa)
    w_ill, _, achieved = er.gen_dot(P.n, cond, rng, place="ranks", y=ya, starts=P.starts)
    return dict(xs=[xa, xb] + sp, w=w, w_ill=w_ill, cond=achieved, y_ref=[P.matvec(x) for x in [xa, xb] + sp])


# ---------------------------------------------------------------------------------------------------- the emulation

FAULTS = ("hole_twice", "hole_never", "first_range_overrun", "second_range_at_hole_lo", "ghost_off_by_stride", "stale_ghost",
          "dropped_boundary_partial", "padding_as_entry", "delta_from_launch_row", "slice_by_tid")


def _rows_product(slab, lcol, xfull, target, source, pad_as_entry, rebase):
    """y of the rows `target`, read from the entries of the rows `source` (the same rows in a correct kernel), in stored order
    with one rounded multiply and one rounded add per entry.  pad_as_entry: the slots behind a row's last entry up to the
    longest row of its slice are entries (0.0, column = the row): the sentinel code 0xFF looks up diagonal 0.  rebase: (bits,
    R, launch row_lo) decodes the delta codes against the base of the block counted from the launch's first row."""
    acc = np.zeros(target.size)
    lens, ptr = slab.lens[source], slab.rowptr[source]
    ncol = xfull.size
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(int(lens.max()) if lens.size else 0):
            on = lens > k
            q = ptr[on] + k
            c = lcol[q]
            if rebase is not None:
                bits, R, row_lo = rebase
                H = max(((1 << bits) - 1 - R) // 2, 0)
                src = source[on]
                base = np.maximum((src // R) * R - H, 0)
                wrong = np.maximum(((src - row_lo) // R) * R - H, 0)
                esc = (c < base) | (c - base >= (1 << bits) - 1)
                c = np.where(esc, c, (wrong + (c - base)) % ncol)
            acc[on] = acc[on] + slab.val[q] * xfull[c]
        if pad_as_entry:
            sl = source // SLICE
            smax = np.array([slab.lens[s * SLICE:(s + 1) * SLICE].max() for s in sl]) if sl.size else np.zeros(0, dtype=int)
            padded = smax > lens
            acc[padded] = acc[padded] + 0.0 * xfull[source[padded]]
    return acc


def emulate_rank(slab, mode, x_global, pred, options, fault=None, ghost_prev=None):
    """One partitioned product on one rank: (y, covered rows with multiplicity, ghost buffer)."""
    m = slab.m
    lcol = slab.lcol(mode)
    ghost = slab.ghost_buffer(mode, x_global)
    if fault == "stale_ghost" and ghost_prev is not None:
        ghost = ghost_prev
    used = ghost
    if fault == "ghost_off_by_stride" and mode == "gather":
        used = np.roll(ghost, -slab.maxm)                               # index + one rank stride
    xfull = np.concatenate([x_global[slab.r0:slab.r1], used])
    lo, hi = slab.interior(mode)
    form = pred["form"]
    ls = launches(form, options, lo, hi, m, pred["delta_rows"])
    y = np.full(m, np.nan)
    covered = []
    sliced = family_of(form) in ("Sliced", "Sliced32")
    R = pred["rows"] if family_of(form) in STAGED_FAMILY or family_of(form) == "Stream" else 256
    for L in ls:
        ranges = list(L["ranges"])
        if fault == "hole_never" and L["part"] == "interior":
            continue
        if fault == "hole_twice" and L["part"] == "boundary" and hi > lo:
            ranges = [(ranges[0][0], max(hi, ranges[0][1]))] + ranges[1:] if ranges[0][0] == 0 else ranges
        if fault == "second_range_at_hole_lo" and len(ranges) == 2:
            ranges = [ranges[0], (lo, lo + (ranges[1][1] - ranges[1][0]))]
        if fault == "first_range_overrun" and L["part"] == "boundary" and ranges[0][0] == 0 and ranges[0][1] < m:
            ranges = [(0, min(m, -(-ranges[0][1] // R) * R))] + ranges[1:]
        row_lo = ranges[0][0]
        for (a, b) in ranges:
            target = np.arange(a, b)
            source = target
            if fault == "slice_by_tid" and sliced:
                source = np.minimum((a // SLICE) * SLICE + (target - a), m - 1)       # slice and lane counted from the range's first row
            rebase = None
            if fault == "delta_from_launch_row" and L["delta"]:
                rebase = (pred["delta_bits"], pred["delta_rows"], row_lo)
            y[target] = _rows_product(slab, lcol, xfull, target, source, fault == "padding_as_entry" and sliced, rebase)
            if not (fault == "dropped_boundary_partial" and L["part"] == "boundary"):
                covered.append(target)
    return y, (np.concatenate(covered) if covered else np.zeros(0, dtype=np.int64)), ghost


def emulate_case(P, inputs, form_name, mode, overlap, fault=None):
    """What the GPU file collects for one (form, halo mode, overlap) on every rank, from the emulation: a list over ranks of
    dict(form=..., y=[...], dot, dotw, dot2, dotw_ill, y_dot=[...])."""
    options = dict(FORMS[form_name]["opts"], overlap_halo=overlap)
    preds = [predict(s.info(mode), options, form_name == "template" and s.templates(mode) > 0) for s in P.slabs]
    ys, cov = [], []
    ghosts = [None] * len(P.slabs)
    for x in inputs["xs"] + [inputs["xs"][0]]:
        yk, ck = [], []
        for r, s in enumerate(P.slabs):
            y, c, ghosts[r] = emulate_rank(s, mode, x, preds[r], options, fault, ghosts[r])
            yk.append(y)
            ck.append(c)
        ys.append(yk)
        cov.append(ck)
    y_last, c_last = ys[-1], cov[-1]                                     # the product the fused dots ride on: x_a again

    def fused(w):
        wy = np.concatenate([w[s.r0:s.r1][c] for s, c in zip(P.slabs, c_last)])
        yy = np.concatenate([y[c] for y, c in zip(y_last, c_last)])
        try:
            return er.exact_dot(wy, yy), er.exact_dot(yy, yy)
        except ValueError:
            return math.nan, math.nan
    xa = inputs["xs"][0]
    d, sq = fused(xa)
    out = []
    for r, s in enumerate(P.slabs):
        out.append(dict(form=preds[r]["form"], y=[ys[k][r] for k in range(len(inputs["xs"]))], dot=d, dotw=fused(inputs["w"])[0],
                        dot2=(d, sq), dotw_ill=fused(inputs["w_ill"])[0], y_dot=[y_last[r]] * 4))
    return out


# ---------------------------------------------------------------------------------------------------- the comparisons

class Ratios:
    """The largest |d| / bound per check (written through parity_log by the GPU file)."""

    def __init__(self):
        self.worst = {}

    def add(self, what, ratio):
        self.worst[what] = max(self.worst.get(what, 0.0), float(ratio))


def vector_row_bound(P, x, y_dev, r0, r1, rows=None):
    """Rows of a product in ANY summation order, fused multiply-adds or not: |y_i - sum_j a_ij x_j| <= gamma(k_i) sum_j |a_ij x_j|
    with k_i the row length (Higham, Accuracy and Stability, sec. 3.1).  Returns the largest |d| / bound (0 / 0 = 0) over the
    local rows `rows` (default: all of [r0, r1)).  The row sums are first taken in double-double (error-free products, TwoSum,
    vectorised over the rows: off by at most 2 gamma(k)^2 sum|a x|, a 1e-14th of the bound); a row whose |d| comes out above 0.9
    of its bound is decided on the exact sum (math.fsum of the products, their errors and -y, rounded once)."""
    rows = np.arange(r1 - r0) if rows is None else np.asarray(rows)
    if rows.size == 0:
        return 0.0
    g = rows + r0
    ptr, lens = P.rowptr[g], np.diff(P.rowptr)[g]
    y = np.asarray(y_dev, dtype=np.float64)[rows]
    hi, lo, S = np.zeros(rows.size), np.zeros(rows.size), np.zeros(rows.size)
    for k in range(int(lens.max())):
        on = lens > k
        q = ptr[on] + k
        pk, ek = er.two_product(P.val[q], x[P.col[q]])
        h = hi[on]
        t = h + pk
        bp = t - h
        lo[on] += ((h - (t - bp)) + (pk - bp)) + ek
        hi[on] = t
        S[on] += np.abs(pk)
    d = np.abs((hi - y) + lo)
    bound = np.array([er.gamma(int(k)) if k else 0.0 for k in lens]) * S
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, d / bound, np.where(d == 0, 0.0, np.inf))
    for j in np.flatnonzero(ratio > 0.9):                                # decided exactly
        a, b = int(ptr[j]), int(ptr[j] + lens[j])
        if b == a:
            continue
        pj, ej = er.two_product(P.val[a:b], x[P.col[a:b]])
        dj = abs(math.fsum(list(pj) + list(ej) + [-float(y[j])]))
        bj = er.gamma(b - a) * math.fsum(np.abs(pj).tolist())
        ratio[j] = dj / bj if bj > 0 else (0.0 if dj == 0 else math.inf)
    return float(ratio.max())


def judge(P, inputs, outs, want_form, exact_y=True, compensated=True, ratios=None, two_reductions=False):
    """Every comparison of one (form, halo mode, overlap) case: returns the list of failures (empty = passes).  outs: per rank
    dict(form, y = [y(x_a), y(x_b), y(special owned), y(special ghost)], dot = x_a . y, dotw = w . y, dot2 = (x_a . y, y . y),
    dotw_ill, y_dot = [the y each of the four fused products left])."""
    ratios = ratios if ratios is not None else Ratios()
    fails = []
    starts = P.starts
    wants = want_form if isinstance(want_form, (list, tuple)) else [want_form] * len(outs)
    for r, o in enumerate(outs):
        if o["form"] != wants[r]:
            fails.append(f"rank {r}: ran {o['form']}, expected {wants[r]}")
    if fails:
        return fails                                                      # the form before any comparison
    nx = len(inputs["xs"])
    for k in range(nx):
        ref = inputs["y_ref"][k]
        special = k >= 2
        for r, o in enumerate(outs):
            r0, r1 = starts[r], starts[r + 1]
            y = o["y"][k]
            if exact_y:
                if not np.array_equal(y, ref[r0:r1], equal_nan=special):
                    bad = np.flatnonzero(~((y == ref[r0:r1]) | (np.isnan(y) & np.isnan(ref[r0:r1]) & special)))
                    fails.append(f"y[{k}] rank {r}: {bad.size} rows differ, first local row {int(bad[0])}")
            elif special:
                if not (np.array_equal(np.isnan(y), np.isnan(ref[r0:r1])) and np.array_equal(np.isinf(y), np.isinf(ref[r0:r1]))
                        and np.array_equal(np.sign(y[np.isinf(y)]), np.sign(ref[r0:r1][np.isinf(y)]))):
                    fails.append(f"y[{k}] rank {r}: non-finite rows differ from the serial loop's")
                    continue
                finite = np.flatnonzero(np.isfinite(ref[r0:r1]))               # the rows that reference neither special column
                xf = np.where(np.isfinite(inputs["xs"][k]), inputs["xs"][k], 0.0)      # those rows never read the two entries
                ratio = vector_row_bound(P, xf, y, r0, r1, finite)
                ratios.add("vector_rows", ratio)
                if ratio > 1.0:
                    fails.append(f"y[{k}] rank {r}: finite rows: |d| / (gamma(k) sum|a x|) = {ratio:.3g}")
            else:
                if not np.isfinite(y).all():
                    fails.append(f"y[{k}] rank {r}: non-finite rows")
                    continue
                ratio = vector_row_bound(P, inputs["xs"][k], y, r0, r1)
                ratios.add("vector_rows", ratio)
                if ratio > 1.0:
                    fails.append(f"y[{k}] rank {r}: |d| / (gamma(k) sum|a x|) = {ratio:.3g}")
    # the fused products: y unchanged by the fusion, scalars identical on the ranks and within the bound of the exact value
    for j, name in enumerate(("dot", "dotw", "dot2", "dotw_ill")):
        for r, o in enumerate(outs):
            if not np.array_equal(o["y_dot"][j], o["y"][0]):
                fails.append(f"{name} rank {r}: y of the fused product differs from the plain product's")
    y_all = np.concatenate([o["y"][0] for o in outs])
    if not np.isfinite(y_all).all():
        return fails + ["y is not finite: no exact value for the fused scalars"]
    n = P.n
    xa = inputs["xs"][0]

    tally = er.Tally(lambda **kw: ratios.add(kw["what"], kw["ratio"]), P.fam.name)

    def scalar(name, vals, u, v, sq=False):
        if any(not (a == vals[0]) for a in vals):
            fails.append(f"{name}: not the same bits on every rank: {vals}")
            return
        d = vals[0]
        if compensated:                                                   # Dot2 bound / one ulp of the exact sum of squares
            ok, detail = tally.sq(name, d, u) if sq else tally.dot(name, d, u, v, inputs["cond"] if name.endswith(".ill") else 1.0, n=n)
        else:                                                             # plain recursive summation, in any order
            s, bound = er.exact_dot(u, v), er.gamma(n) * er.absum(u, v)
            ratios.add(name + ".plain_sum", abs(d - s) / bound if bound > 0 else (0.0 if d == s else math.inf))
            ok, detail = abs(d - s) <= bound, (name, d, s, bound)
        if not ok:
            fails.append(f"{name}: outside its bound: {detail}")

    tag = ".two_reductions" if two_reductions else ""
    scalar("spmv_dot", [o["dot"] for o in outs], xa, y_all)
    scalar("spmv_dotw", [o["dotw"] for o in outs], inputs["w"], y_all)
    scalar("spmv_dot2.xy" + tag, [o["dot2"][0] for o in outs], xa, y_all)
    scalar("spmv_dot2.yy" + tag, [o["dot2"][1] for o in outs], y_all, y_all, sq=True)
    scalar("spmv_dotw.ill", [o["dotw_ill"] for o in outs], inputs["w_ill"], y_all)
    return fails
