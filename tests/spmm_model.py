"""Host model of the SpMM kernels' builders, launches and persistent loops (csrc/spmm_tile.hip, csrc/csr_aux.hip); numpy only.

Restated from the sources: the plane detection of csr_finalize, the group order of the tile records (tile_order_for,
tile_order_set_runs, tile_groups_for, tile_row_of), the distinct columns of a group with the long-row rule, spmm_tile_build's
decision, the window builder's refusal rule and flags, launch_spmm / launch_spmm_tile / launch_tile_L / launch_window for a
given option set (the grid only where an option forces it: the residency-derived default is not modelled), and the WALK: which
groups each workgroup of a kernel family visits, in order.  check_records reads the raw record bytes of a handle
(khip_test_csr_tile_records) and is semantic: it does not repeat the builder's slot policy, it checks what the kernels rely on.
reference_records is a plain host builder used only to give the checker's own CPU tests something to corrupt.

tests/test_spmm_model_host.py runs the model without a GPU; tests/test_gpu_spmm_exact.py holds the device to it.
"""
import os
import re
from collections import namedtuple

import numpy as np

# ---- constants copied from the sources (constants_in_sources re-derives them) -----------------------------------------------
kTileR = 32            # rows per group
kTileLen = 32          # entries per row on the register path
kTileCapMax = 256      # window slots (one-byte slot numbers)
kBlock = 256
REUSE_MIN = 1.5        # references per distinct column below which neither builder stages anything
FIT_PERCENT = 99       # the window takes this share of the groups
DBUF_BYTES = 26 * 1024
LDS_BYTES = 160 * 1024
KHIP_WIN_KB = 44
KHIP_WIN_WGS = 2
kTileDescBytes = kTileR * 16
kTileSlotBytes = kTileR * kTileLen

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "krylov.jl_amd", "csrc")


def constants_in_sources():
    tile = open(os.path.join(_CSRC, "spmm_tile.hip")).read()
    aux = open(os.path.join(_CSRC, "csr_aux.hip")).read()
    red = open(os.path.join(_CSRC, "device_reduce.hpp")).read()

    def one(pat, text):
        m = re.findall(pat, text)
        assert len(m) >= 1, pat
        assert len(set(m)) == 1, (pat, m)
        return m[0]

    out = {}
    out["kTileR"] = int(one(r"#define KHIP_TILE_ROWS (\d+)", tile))
    assert one(r"constexpr int kTileR = (\w+);", tile) == "KHIP_TILE_ROWS"
    out["kTileLen"] = int(one(r"constexpr int kTileLen = (\d+);", tile))
    out["kTileCapMax"] = int(one(r"constexpr int kTileCapMax = (\d+);", tile))
    out["kBlock"] = int(one(r"constexpr int kBlock = (\d+);", red))
    out["REUSE_MIN"] = float(one(r"if \(best_score < ([0-9.]+)\) return KHIP_OK;", tile))
    # ... and the window builder's form of the same threshold: 2 nnz < 3 sum  <=>  nnz / sum < 1.5
    assert one(r"(2 \* \(unsigned long long\)A->nnz < 3 \* st\[2\])", aux)
    a, b = one(r"if \((\d+) \* fit >= (\d+) \* \(unsigned long long\)groups\)", tile)
    assert int(a) == 100
    out["FIT_PERCENT"] = int(b)
    kib = one(r"\(size_t\)w\.cap \* 32 \* L \* 2 <= \(size_t\)(\d+) \* 1024", tile)
    out["DBUF_BYTES"] = int(kib) * 1024
    out["LDS_BYTES"] = int(one(r"\(size_t\)\((\d+) \* 1024\) / lds\)", tile)) * 1024
    out["KHIP_WIN_KB"] = int(one(r"#define KHIP_WIN_KB (\d+)", aux))
    out["KHIP_WIN_WGS"] = int(one(r"#define KHIP_WIN_WGS (\d+)", aux))
    out["kTileDescBytes"] = out["kTileR"] * int(one(r"constexpr int kTileDescBytes = kTileR \* (\d+);", tile))
    assert one(r"constexpr int kTileSlotBytes = (kTileR \* kTileLen);", tile)
    out["kTileSlotBytes"] = out["kTileR"] * out["kTileLen"]
    return out


# ---- operators ---------------------------------------------------------------------------------------------------------------
class Op:
    """A CSR operator on the host (int32 rowptr / col, float64 val) with its test inputs."""

    def __init__(self, name, m, n, rowptr, col, val):
        self.name, self.m, self.n = name, int(m), int(n)
        self.rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
        self.col = np.ascontiguousarray(col, dtype=np.int32)
        self.val = np.ascontiguousarray(val, dtype=np.float64)
        self.nnz = int(self.rowptr[-1])
        assert self.col.size == self.nnz == self.val.size and self.rowptr.size == self.m + 1
        self.lens = np.diff(self.rowptr).astype(np.int64)
        self._cache = {}

    @property
    def band(self):
        rows = np.repeat(np.arange(self.m, dtype=np.int64), self.lens)
        return int(np.max(np.abs(self.col.astype(np.int64) - rows))) if self.nnz else 0

    def planes(self):
        """(line_rows, plane_rows) as csr_finalize estimates them from one interior row."""
        if "planes" in self._cache:
            return self._cache["planes"]
        line = plane = 0
        max_row = int(self.lens.max()) if self.m else 0
        if self.m >= 128 and max_row >= 2:
            hist = np.bincount(np.minimum(self.lens, 256), minlength=257)
            mode = 2
            for l in range(2, 257):
                if hist[l] > hist[mode]:
                    mode = l
            if hist[mode] > 0:
                cand = np.nonzero(self.lens[self.m // 2:] == mode)[0]
                if cand.size:
                    row = self.m // 2 + int(cand[0])
                    cols = getattr(self, "plane_cols", self.col)[self.rowptr[row]:self.rowptr[row + 1]].astype(np.int64)
                    pos = np.sort(cols[cols > row] - row)
                    if pos.size:
                        start = second = second_end = 0
                        clusters = 1
                        for i in range(1, pos.size):
                            if pos[i] > 2 * pos[i - 1] + 2:
                                clusters += 1
                                if clusters == 2:
                                    second = i
                                if clusters == 3:
                                    second_end = i
                                start = i
                        plane = int((pos[start] + pos[-1]) // 2)
                        if clusters >= 2:
                            if clusters == 2:
                                second_end = pos.size
                            line = int((pos[second] + pos[second_end - 1]) // 2)
        self._cache["planes"] = (line, plane)
        return line, plane

    def with_values(self, val, name):
        o = Op(name, self.m, self.n, self.rowptr, self.col, val)
        for k in ("plane_cols", "ghosts", "global_cols", "r0", "n_global"):
            if hasattr(self, k):
                setattr(o, k, getattr(self, k))
        return o


def slab_op(op, r0, r1):
    """Rows [r0, r1) of op as a rank of a row partition holds them: own columns first (c - r0), then the ghost columns in ascending
    order (m + rank in the sorted list), as col_remap_kernel numbers them.  X of the slab: the rows r0..r1 of X, then the ghost
    rows (slab.ghosts).  csr_finalize looks at the slab BEFORE the renumbering, global columns against local rows, so its plane
    estimate comes from plane_cols (on every rank but the first the offsets all exceed r0 and form one cluster: no grid)."""
    m = r1 - r0
    rp = op.rowptr[r0:r1 + 1].astype(np.int64) - int(op.rowptr[r0])
    gcol = op.col[op.rowptr[r0]:op.rowptr[r1]].astype(np.int64)
    own = (gcol >= r0) & (gcol < r1)
    ghosts = np.unique(gcol[~own])
    col = np.where(own, gcol - r0, m + np.searchsorted(ghosts, gcol))
    s = Op("%s[%d:%d]" % (op.name, r0, r1), m, m + ghosts.size, rp, col, op.val[op.rowptr[r0]:op.rowptr[r1]])
    s.plane_cols, s.ghosts, s.global_cols, s.r0, s.n_global = gcol.astype(np.int32), ghosts, gcol.astype(np.int32), r0, op.n
    return s


def slab_x(slab, X):
    return np.concatenate([X[slab.r0:slab.r0 + slab.m], X[slab.ghosts]], axis=0)


def row_partition(n, world):
    return [g * n // world for g in range(world + 1)]


def _from_rows(name, m, n, rows, rng):
    """rows: list of column arrays (stored order as given)."""
    lens = np.array([len(r) for r in rows], dtype=np.int64)
    rowptr = np.concatenate([[0], np.cumsum(lens)])
    col = np.concatenate([np.asarray(r, dtype=np.int64) for r in rows]) if lens.sum() else np.zeros(0, dtype=np.int64)
    assert col.size == 0 or (col.min() >= 0 and col.max() < n)
    val = rng.standard_normal(col.size)
    val[val == 0.0] = 1.0
    return Op(name, m, n, rowptr, col, val)


def grid_op(n1, n2, n3, points=27, seed=0, extra=None, name=None):
    """7- or 27-point stencil pattern on an n1 x n2 x n3 grid (row = i + n1 j + n1 n2 k), columns ascending, random values.
    extra: {row: array of further columns} appended to the row (flagged groups)."""
    rng = np.random.default_rng(1000 + seed)
    rows = []
    for k in range(n3):
        for j in range(n2):
            for i in range(n1):
                cs = []
                for dk in (-1, 0, 1):
                    for dj in (-1, 0, 1):
                        for di in (-1, 0, 1):
                            if points == 7 and abs(di) + abs(dj) + abs(dk) > 1:
                                continue
                            a, b, c = i + di, j + dj, k + dk
                            if 0 <= a < n1 and 0 <= b < n2 and 0 <= c < n3:
                                cs.append(a + n1 * (b + n2 * c))
                rows.append(cs)
    m = n1 * n2 * n3
    if extra:
        for r, more in extra.items():
            have = set(rows[r])
            rows[r] = rows[r] + [int(c) for c in more if int(c) not in have]
    return _from_rows(name or "grid%d_%dx%dx%d" % (points, n1, n2, n3), m, m, rows, rng)


def band_op(m, h, s=1, seed=0, n=None, edit=None, name=None):
    """Row i holds the columns i + s k, k = -h..h, clipped to [0, n): 32 consecutive rows reach 32 + 2 h s distinct columns.
    edit(rows): changes the list of rows in place (long rows, empty rows, scattered rows)."""
    n = m if n is None else n
    rng = np.random.default_rng(2000 + seed)
    rows = []
    for i in range(m):
        cs = [i + s * k for k in range(-h, h + 1)]
        rows.append([c for c in cs if 0 <= c < n])
    if edit:
        edit(rows)
    return _from_rows(name or "band_m%d_h%d_s%d" % (m, h, s), m, n, rows, rng)


# ---- tile order ----------------------------------------------------------------------------------------------------------------
OPTION_DEFAULTS = dict(
    spmm_wide=1, spmm_window=1, spmm_window_grid=0, spmm_tile=1, spmm_tile_exp=0, spmm_tile_waves=0, spmm_tile_grid=0, spmm_tile_pair=1,
    spmm_tile_dbuf=-1, spmm_tile_xcd=-1, spmm_tile_ahead=0, spmm_tile_slide=-1, spmm_tile_pencil=0, spmm_tile_slices=0, spmm_tile_nt=0,
    spmm_tile_shape=0, spmm_sweep=0, spmm_win_sweep=0, spmm_sweep_s=0, spmm_sweep_w=64)
OPTION_KEYS = tuple(OPTION_DEFAULTS)


def options(**kw):
    o = dict(OPTION_DEFAULTS)
    for k, v in kw.items():
        assert k in o, k
        o[k] = v
    return o


class TileOrder:
    def __init__(self, m):
        self.m = m
        self.s1 = self.s2 = 0
        self.n1 = self.n2 = self.n3 = 0
        self.bi = self.bj = self.bk = 0
        self.gi = self.gj = self.gk = 0
        self.pj = 0
        self.run_pieces = 0
        self.run_len = 0

    @property
    def kind(self):
        return "identity" if self.s1 == 0 else ("runs" if self.run_len > 0 else "pencil")


_SHAPES = {1: (8, 2, 2), 2: (2, 4, 4), 3: (4, 2, 4), 4: (8, 4, 1), 5: (32, 1, 1)}


def tile_order_for(m, line_rows, plane_rows, opts, tiles):
    o = TileOrder(m)
    if not tiles:
        return o
    s1 = line_rows
    s2 = plane_rows if plane_rows > line_rows else m
    o.s1, o.s2 = s1, s2
    o.n1, o.n2, o.n3 = s1, (s2 + s1 - 1) // s1, (m + s2 - 1) // s2
    if o.n3 > 1:
        o.bi, o.bj, o.bk = _SHAPES.get(opts["spmm_tile_shape"], (4, 4, 2))
    else:
        o.bi, o.bj, o.bk = 8, kTileR // 8, 1
    o.gi = (o.n1 + o.bi - 1) // o.bi
    o.gj = (o.n2 + o.bj - 1) // o.bj
    o.gk = (o.n3 + o.bk - 1) // o.bk
    o.pj = opts["spmm_tile_pencil"] if opts["spmm_tile_pencil"] > 0 else 4
    if o.pj > o.gj:
        o.pj = o.gj
    return o


def tile_order_set_runs(o, opts):
    slide = opts["spmm_tile_slide"]
    o.run_len = 0
    if slide < 0:
        slide = 27 if o.s1 != 0 else 0
    if not slide:
        return
    if o.s1 == 0:
        o.run_len = slide if slide > 1 else 64
    else:
        full = o.gk if o.gk > 1 else o.gj
        o.run_len = full
        if 1 < slide < full:
            pieces = (full + slide - 1) // slide
            o.run_len = (full + pieces - 1) // pieces
        o.run_pieces = (full + o.run_len - 1) // o.run_len
    if o.run_len < 2:
        o.run_len = 0


def tile_runs_for(o):
    if o.run_len <= 0:
        return 0
    if o.s1 == 0:
        return ((o.m + kTileR - 1) // kTileR + o.run_len - 1) // o.run_len
    return (o.gi * o.gj if o.gk > 1 else o.gi) * o.run_pieces


def tile_groups_for(o):
    if o.run_len > 0:
        return tile_runs_for(o) * o.run_len
    if o.s1 == 0:
        return (o.m + kTileR - 1) // kTileR
    return o.gi * o.gj * o.gk


def tile_row_of(o, g, t):
    if o.s1 == 0:
        r = g * kTileR + t
        return r if r < o.m else -1
    if o.run_len > 0:
        rid0 = g // o.run_len
        nlines = o.gi * o.gj if o.gk > 1 else o.gi
        rid, pos = rid0 % nlines, (rid0 // nlines) * o.run_len + g % o.run_len
        if o.gk > 1:
            ti, tj, tk = rid % o.gi, rid // o.gi, pos
        else:
            ti, tj, tk = rid, pos, 0
        if ti >= o.gi or tj >= o.gj or tk >= o.gk:
            return -1
    else:
        per_pencil = o.gi * o.pj * o.gk
        pen = g // per_pencil
        wj = o.pj if (pen + 1) * o.pj <= o.gj else o.gj - pen * o.pj
        rem = g - pen * per_pencil
        ti, tjj, tk = rem % o.gi, (rem // o.gi) % wj, rem // (o.gi * wj)
        tj = pen * o.pj + tjj
        if tk >= o.gk:
            return -1
    di, dj, dk = t % o.bi, (t // o.bi) % o.bj, t // (o.bi * o.bj)
    i, j, k = ti * o.bi + di, tj * o.bj + dj, tk * o.bk + dk
    if i >= o.n1 or j >= o.n2 or k >= o.n3:
        return -1
    r = i + o.s1 * j + o.s2 * k
    return r if r < o.m else -1


def group_rows(o):
    """[groups, 32] rows of every group (-1: padding)."""
    G = tile_groups_for(o)
    out = np.empty((G, kTileR), dtype=np.int64)
    for g in range(G):
        for t in range(kTileR):
            out[g, t] = tile_row_of(o, g, t)
    return out


def group_columns(op, rows):
    """Per group: the ascending distinct columns, or None where a row has more than 32 entries."""
    out = []
    for g in range(rows.shape[0]):
        rr = rows[g][rows[g] >= 0]
        if rr.size and op.lens[rr].max() > kTileLen:
            out.append(None)
            continue
        cs = [op.col[op.rowptr[r]:op.rowptr[r + 1]] for r in rr]
        out.append(np.unique(np.concatenate(cs)) if cs else np.zeros(0, dtype=np.int32))
    return out


# ---- the build decision ------------------------------------------------------------------------------------------------------
def grid_ok_of(m, line_rows, plane_rows):
    return line_rows >= 4 and line_rows < m and (plane_rows <= line_rows or (plane_rows % line_rows == 0 and plane_rows // line_rows >= 4))


def tile_build(op, opts, planes=None):
    """What spmm_tile_build leaves on a fresh handle of op under opts: dict(state, cap, stride, groups, run_len, runs, ahead,
    grid_tiles, direct, reuse) plus the model's own order, rows, cols, counts (not compared with the device)."""
    key = ("build", tuple(opts[k] for k in ("spmm_tile_shape", "spmm_tile_pencil", "spmm_tile_slide", "spmm_tile_ahead", "spmm_tile_pair")), planes)
    if key in op._cache:
        return op._cache[key]
    line, plane = planes if planes is not None else op.planes()
    refused = dict(state=-1, cap=0, stride=0, groups=0, run_len=0, runs=0, ahead=0, grid_tiles=0, direct=0, reuse=0.0, why="")
    res = None
    if op.m <= 0 or op.nnz <= 0:
        res = dict(refused, why="empty")
    else:
        grid_ok = grid_ok_of(op.m, line, plane)
        best, best_score = None, -1.0
        scores = []
        for cand in range(2 if grid_ok else 1):
            o = tile_order_for(op.m, line, plane, opts, cand == 1)
            tile_order_set_runs(o, opts)
            groups = tile_groups_for(o)
            if groups <= 0 or groups > (1 << 30):
                continue
            rows = group_rows(o)
            cols = group_columns(op, rows)
            n_long = sum(1 for c in cols if c is None)
            total = sum(len(c) for c in cols if c is not None)
            score = float(op.nnz) / (float(total) + 32.0 * float(n_long)) if total > 0 else 0.0
            scores.append(score)
            if score > best_score:
                best_score, best = score, (o, rows, cols, n_long)
        if best_score < REUSE_MIN:
            res = dict(refused, why="reuse %.4f" % best_score, score=best_score, scores=scores, grid_ok=grid_ok)
        else:
            o, rows, cols, n_long = best
            groups = tile_groups_for(o)
            counts = np.array([-1 if c is None else len(c) for c in cols], dtype=np.int64)
            bins = np.bincount((counts[counts >= 0] + 7) // 8, minlength=kTileCapMax // 8 + 1 + 128)
            fit, cap = 0, -1
            for b in range(kTileCapMax // 8 + 1):
                fit += int(bins[b])
                if 100 * fit >= FIT_PERCENT * groups:
                    cap = 8 * b
                    break
            if cap < 0 and 2 * fit < groups:
                res = dict(refused, why="fewer than half of the groups fit %d slots" % kTileCapMax, score=best_score, scores=scores,
                           grid_ok=grid_ok, fit=fit, ngroups=groups)
            else:
                if cap < 0:
                    cap = kTileCapMax
                cap0 = cap = max(cap, 8)
                ahead = o.run_len > 0 and opts["spmm_tile_ahead"] != 0 and opts["spmm_tile_pair"] != 0 and cap + cap // 2 <= kTileCapMax
                if ahead:
                    cap = ((cap + cap // 2) + 7) & ~7
                direct = n_long + int(bins[cap // 8 + 1:].sum())
                res = dict(state=1, cap=cap, stride=kTileDescBytes + 4 * cap + kTileSlotBytes, groups=groups, run_len=o.run_len,
                           runs=tile_runs_for(o), ahead=1 if ahead else 0, grid_tiles=1 if o.s1 != 0 else 0, direct=direct,
                           reuse=best_score, why="", order=o, rows=rows, cols=cols, counts=counts, cap0=cap0, scores=scores,
                           grid_ok=grid_ok, fit=fit)
    res["line_rows"], res["plane_rows"] = line, plane
    op._cache[key] = res
    return res


BUILD_FIELDS = ("state", "cap", "stride", "groups", "run_len", "runs", "ahead", "grid_tiles", "direct", "line_rows", "plane_rows")


def build_failures(want, got):
    bad = ["%s: device %r, model %r" % (k, got[k], want[k]) for k in BUILD_FIELDS if got[k] != want[k]]
    if want["state"] == 1 and got["reuse"] != want["reuse"]:
        bad.append("reuse: device %r, model %r" % (got["reuse"], want["reuse"]))
    if want["state"] == 1 and got["state"] == 1:
        desc = got["meta"][:, :kTileDescBytes].copy().view(np.int32).reshape(-1, kTileR, 4)
        if desc.shape[0] != want["rows"].shape[0] or not np.array_equal(desc[:, :, 0], want["rows"]):
            bad.append("the rows of the records are not in the model's group order (%s)" % want["order"].kind)
    return bad


# ---- the window builder (csr_aux.hip) --------------------------------------------------------------------------------------
def win_shape(L):
    RPB = kBlock // L
    CAP = KHIP_WIN_KB * 1024 // (16 * L)
    STRIDE = (CAP + RPB - 1) // RPB * RPB
    ENTRIES = RPB * 32
    return dict(RPB=RPB, CAP=CAP, STRIDE=STRIDE, ENTRIES=ENTRIES, lds=STRIDE * L * 16 + (ENTRIES + 8) * 8 + (ENTRIES + 8) * 2)


def window_build(op, L):
    """dict(win_L, groups, flagged, flags, by_columns, by_entries, total): spmm_window_build for L lanes per row."""
    key = ("win", L)
    if key in op._cache:
        return op._cache[key]
    W = win_shape(L)
    groups = (op.m + W["RPB"] - 1) // W["RPB"]
    flags = np.zeros(groups, dtype=bool)
    by_cols = by_ent = total = 0
    for g in range(groups):
        r0, r1 = g * W["RPB"], min((g + 1) * W["RPB"], op.m)
        n_uniq = np.unique(op.col[op.rowptr[r0]:op.rowptr[r1]]).size
        over_c, over_e = n_uniq > W["CAP"], int(op.rowptr[r1] - op.rowptr[r0]) > W["ENTRIES"]
        flags[g] = over_c or over_e
        by_cols += over_c
        by_ent += over_e
        if not flags[g]:
            total += n_uniq
    nflag = int(flags.sum())
    refused = 2 * nflag > groups or total == 0 or 2 * op.nnz < 3 * total
    res = dict(win_L=-L if refused else L, groups=0 if refused else groups, flagged=0 if refused else nflag, flags=flags,
               by_columns=by_cols, by_entries=by_ent, total=total, all_groups=groups, all_flagged=nflag)
    op._cache[key] = res
    return res


# ---- the launch decision -----------------------------------------------------------------------------------------------------
LAUNCH_FIELDS = ("family", "L", "NL", "dbuf", "ahead", "run_len", "xcd", "launches", "direct", "sweep_S", "sweep_W", "sweep_K",
                 "sweep_cols", "nt", "dist", "p", "pow2", "block")


def _tile_launch(op, b, opts, L, dist, out):
    cap, run_len = b["cap"], b["run_len"]
    use_pair = bool(opts["spmm_tile_pair"]) and L >= 4 and not opts["spmm_tile_nt"]
    xo, exp = opts["spmm_tile_xcd"], opts["spmm_tile_exp"]
    if xo == 2:
        exp |= 128
    elif xo == 1 or (xo < 0 and b["grid_tiles"] == 0 and b["run_len"] == 0):
        exp |= 8
    ahead = 1 if (use_pair and b["ahead"] and run_len > 0 and opts["spmm_tile_ahead"] != 0) else 0
    dopt = opts["spmm_tile_dbuf"]
    dbuf = 1 if (not use_pair and (dopt > 0 or (dopt < 0 and cap * 32 * L * 2 <= DBUF_BYTES))) else 0
    if dbuf:
        run_len = 0
    NL = (cap + 63) // 64
    forced = opts["spmm_tile_grid"]
    grid = None
    if forced > 0:
        grid = forced
        if use_pair:
            if run_len > 0 and grid > b["runs"]:
                grid = b["runs"]
            if grid > b["groups"]:
                grid = b["groups"]
        else:
            if grid > b["groups"]:
                grid = b["groups"]
            if run_len > 0 and grid > b["runs"]:
                grid = b["runs"]
        if grid >= 64:
            grid &= ~7
    out.update(family="tile2" if use_pair else "tile1", L=L, NL=NL, dbuf=dbuf, ahead=ahead, run_len=run_len, grid=grid,
               xcd=exp & (8 | 128), launches=out["launches"] + 1, direct=b["direct"], nt=0 if use_pair else (1 if opts["spmm_tile_nt"] else 0),
               dist=1 if dist else 0, block=128 if use_pair else 64, lds=cap * 32 * L * (2 if dbuf else 1))


def launch(op, opts, p, dist=False, planes=None):
    """What khip_spmm launches for a fresh handle of op under opts (X and Y 16-byte aligned): the fields of
    khip_test_spmm_last_launch; "grid" is None where no option forces it; "error" names a refusal of the product itself."""
    out = dict(family="none", L=0, NL=0, dbuf=0, ahead=0, run_len=0, grid=None, xcd=0, launches=0, direct=0, sweep_S=0, sweep_W=0,
               sweep_K=0, sweep_cols=0, nt=0, dist=0, p=p, pow2=0, block=0, lds=0, error=None, tile_built=False, win_L=0)
    if p < 1 or p > 64:
        out["error"] = "1 <= p <= 64"
        return out
    P = 4
    while P < p:
        P <<= 1
    rpb = kBlock // P
    want = (op.m + rpb - 1) // rpb
    gcap = 1 << 22
    grid = max(1, min(want, gcap))
    band = op.band
    sw_s = sw_w = 0
    Wd = opts["spmm_sweep_w"] if opts["spmm_sweep_w"] > 0 else 64
    S = opts["spmm_sweep_s"] if opts["spmm_sweep_s"] > 0 else (band + rpb // 2) // rpb
    if opts["spmm_sweep"] != 0 and S >= 8 * Wd and (opts["spmm_sweep_s"] > 0 or band * 2 * p * 8 > (2 << 20)):
        Spad = (S + 8 * Wd - 1) // (8 * Wd) * (8 * Wd)
        Kk = (want + S - 1) // S
        if Kk * Spad <= gcap:
            sw_s, sw_w, grid = S, Wd, Kk * Spad
    if opts["spmm_wide"] and p % 2 == 0 and p >= 4:
        L = 2
        while 2 * L < p:
            L <<= 1
        rpb2 = kBlock // L
        want2 = (op.m + rpb2 - 1) // rpb2
        grid2 = min(max(want2, 1), gcap)
        sw_s = 0
        line, plane = planes if planes is not None else op.planes()
        if opts["spmm_sweep"] != 0 and not opts["spmm_window"]:
            W2 = opts["spmm_sweep_w"] if opts["spmm_sweep_w"] > 0 else 64
            pr = plane if plane > 0 else band
            S2 = opts["spmm_sweep_s"] if opts["spmm_sweep_s"] > 0 else (pr + rpb2 // 2) // rpb2
            if S2 >= 8 * W2:
                Spad = (S2 + 8 * W2 - 1) // (8 * W2) * (8 * W2)
                K2 = (want2 + S2 - 1) // S2
                if K2 * Spad <= gcap:
                    sw_s, sw_w, grid2 = S2, W2, K2 * Spad
        pow2 = p & (p - 1) == 0
        if opts["spmm_tile"] and pow2 and p >= 8 and op.m > 0 and op.nnz > 0:
            b = tile_build(op, opts, planes)
            out["tile_built"] = True
            long_rows = op.nnz >= 16 * op.m
            slices = p >= 32 and opts["spmm_tile_slices"] >= 0 and (p > 32 or opts["spmm_tile_slices"] > 0 or long_rows)
            fits = slices or b["cap"] * 8 * p <= LDS_BYTES
            wanted = p == 16 or p > 32 or opts["spmm_tile"] >= 2 or (p == 8 and b["grid_tiles"] == 1 and long_rows) or \
                (p == 32 and (long_rows if slices else b["grid_tiles"] == 1))
            if b["state"] == 1 and fits and wanted and (p <= 32 or slices):
                if slices and p % 16 == 0 and p > 16:
                    for _ in range(p // 16):
                        _tile_launch(op, b, opts, 4, dist, out)
                    return out
                if b["cap"] * 8 * p > LDS_BYTES:
                    out["error"] = "exceeds the LDS"
                    return out
                _tile_launch(op, b, opts, p // 4, dist, out)
                return out
        if opts["spmm_window"] and want2 <= gcap and op.m > 0:
            wb = window_build(op, L)
            out["win_L"] = wb["win_L"]
            if wb["win_L"] == L:
                W = win_shape(L)
                groups = wb["all_groups"]
                g = opts["spmm_window_grid"] if opts["spmm_window_grid"] > 0 else None
                if g is not None and g > groups:
                    g = groups
                out.update(family="window", L=L, launches=1, dist=1 if dist else 0, pow2=1 if p == 2 * L else 0, block=kBlock, lds=W["lds"])
                if opts["spmm_win_sweep"] != 0 and g is not None and g >= 64:
                    pr = plane if plane > 0 else band
                    S = opts["spmm_sweep_s"] if opts["spmm_sweep_s"] > 0 else (pr + W["RPB"] // 2) // W["RPB"]
                    Wc = opts["spmm_sweep_w"] if opts["spmm_sweep_w"] > 0 else 64
                    if S >= 8 * Wc and S < groups and (opts["spmm_sweep_s"] > 0 or pr * 2 * p * 8 > (2 << 20)):
                        g &= ~7
                        out.update(sweep_S=S, sweep_W=Wc, sweep_K=(groups + S - 1) // S, sweep_cols=(S + 8 * Wc - 1) // (8 * Wc))
                out["grid"] = g
                return out
        out.update(family="spmm2_kernel", L=L, grid=grid2, launches=1, sweep_S=sw_s, sweep_W=sw_w if sw_s else 0, dist=1 if dist else 0,
                   block=kBlock)
        return out
    out.update(family="spmm_kernel", L=P, grid=grid, launches=1, sweep_S=sw_s, sweep_W=sw_w if sw_s else 0, dist=1 if dist else 0, block=kBlock)
    return out


def launch_failures(want, got):
    bad = ["%s: device %r, model %r" % (k, got[k], want[k]) for k in LAUNCH_FIELDS if got[k] != want[k]]
    if want["grid"] is not None and got["grid"] != want["grid"]:
        bad.append("grid: device %r, model %r" % (got["grid"], want["grid"]))
    if got["family"] in ("tile1", "tile2", "window") and got["lds"] != want["lds"]:
        bad.append("lds: device %r, model %r" % (got["lds"], want["lds"]))
    return bad


# ---- the walk ------------------------------------------------------------------------------------------------------------------
def walk_tile(family, groups, runs, run_len, grid, xcd, dbuf=0):
    """Per workgroup, the groups it visits in order.  run_len is the one PASSED TO THE KERNEL (0 under dbuf)."""
    assert family in ("tile1", "tile2") and grid >= 1
    per_xcd, runs_per_xcd = (groups + 7) // 8, (runs + 7) // 8
    mult8 = grid % 8 == 0
    out = []
    for b in range(grid):
        x = b & 7
        if family == "tile1":
            eighths = not (xcd & 8) and mult8            # the one-wave kernel knows no chunked front: bit 128 leaves the eighths
            lin = b
            slide_eighths = mult8                        # ... and its runs go by eighths whenever the grid allows
        else:
            eighths = not (xcd & (8 | 128)) and mult8
            lin = (b & 7) * (grid >> 3) + (b >> 3) if ((xcd & 128) and mult8) else b
            slide_eighths = eighths
        seq = []
        if run_len > 0:
            G = grid >> 3 if slide_eighths else grid
            run = x * runs_per_xcd + (b >> 3) if slide_eighths else lin
            run_end = min((x + 1) * runs_per_xcd, runs) if slide_eighths else runs
            while run < run_end:
                seq.extend(range(run * run_len, (run + 1) * run_len))
                run += G
        else:
            if eighths:
                G, g, gend = grid >> 3, x * per_xcd + (b >> 3), min((x + 1) * per_xcd, groups)
            else:
                G, g, gend = grid, lin, groups
            seq = list(range(g, gend, G))
        out.append(seq)
    return out


def walk_window(groups, grid, S=0, W=0, K=0, cols=0):
    """Per workgroup of spmm_window_kernel: the virtual indices it takes, as group numbers (None: a padding slot of phys())."""
    out = []
    for b in range(grid):
        seq = []
        if S > 0:
            xcd, lstep, lend = b & 7, grid >> 3, cols * K * W
            l = b >> 3
            while l < lend:
                per = K * W
                tt, rem = divmod(l, per)
                k, ww = divmod(rem, W)
                pos = (tt * 8 + xcd) * W + ww
                g = k * S + pos
                seq.append(g if (pos < S and g < groups) else None)
                l += lstep
        else:
            seq = list(range(b, groups, grid))
        out.append(seq)
    return out


def walk_direct(ntiles, grid, S=0, W=0):
    """spmm_kernel / spmm2_kernel: the row tiles of every workgroup (plane sweep: one or none)."""
    out = []
    for b in range(grid):
        if S > 0:
            K = (ntiles + S - 1) // S
            l, per = b >> 3, K * W
            tt, rem = divmod(l, per)
            k, w = divmod(rem, W)
            ti = (tt * 8 + (b & 7)) * W + w
            t = k * S + ti
            out.append([t] if (ti < S and t < ntiles) else [])
        else:
            out.append(list(range(b, ntiles, grid)))
    return out


def walk_stats(walk, run_len=0):
    """dict(visits: sorted list of all real groups visited, max_groups, max_runs, empty_xcds, padding)"""
    flat = [g for seq in walk for g in seq if g is not None]
    per_x = [0] * 8
    for b, seq in enumerate(walk):
        per_x[b & 7] += sum(1 for g in seq if g is not None)
    return dict(visits=sorted(flat), max_groups=max((sum(1 for g in s if g is not None) for s in walk), default=0),
                max_runs=max((len(s) // run_len for s in walk), default=0) if run_len > 0 else 0,
                empty_xcds=[x for x in range(min(8, len(walk))) if per_x[x] == 0], padding=sum(1 for s in walk for g in s if g is None))


# ---- the records -------------------------------------------------------------------------------------------------------------
def split_records(meta, cap):
    """(desc int32 [G, 32, 4], list int32 [G, cap], slots uint8 [G, 32, 32]) views of the raw record bytes."""
    G = meta.shape[0]
    assert meta.dtype == np.uint8 and meta.shape[1] == kTileDescBytes + 4 * cap + kTileSlotBytes
    desc = np.ascontiguousarray(meta[:, :kTileDescBytes]).view(np.int32).reshape(G, kTileR, 4)
    lst = np.ascontiguousarray(meta[:, kTileDescBytes:kTileDescBytes + 4 * cap]).view(np.int32).reshape(G, cap)
    slots = np.ascontiguousarray(meta[:, kTileDescBytes + 4 * cap:]).reshape(G, kTileR, kTileLen)
    return desc, lst, slots


def check_records(op, meta, cap, run_len, direct_list, ncols=None, limit=12):
    """Failures (strings) of the raw records against what the kernels rely on; [] = sound.  ncols: valid list entries are
    < ncols (default op.n; a slab: m + n_ghost)."""
    ncols = op.n if ncols is None else ncols
    bad = []

    def fail(msg):
        if len(bad) < limit:
            bad.append(msg)

    desc, lst, slots = split_records(meta, cap)
    G = desc.shape[0]
    # every row in exactly one (group, slot), with its first entry and length; padding slots -1
    rows = desc[:, :, 0].astype(np.int64)
    if rows.min(initial=0) < -1 or rows.max(initial=-1) >= op.m:
        fail("a row slot names a row outside [-1, m)")
        return bad
    real = rows >= 0
    seen = np.bincount(rows[real], minlength=op.m)
    if np.any(seen != 1):
        r = int(np.nonzero(seen != 1)[0][0])
        fail("row %d is listed %d times" % (r, seen[r]))
    if not np.array_equal(desc[:, :, 1][real], op.rowptr[rows[real]]):
        fail("a row slot's first entry is not rowptr[row]")
    if not np.array_equal(desc[:, :, 2][real], op.lens[rows[real]]):
        fail("a row slot's length is not the row's")
    if lst.size and (lst.min() < 0 or lst.max() >= ncols):
        fail("a list entry is not a valid column (< %d)" % ncols)
    flagged = []
    window = None                                    # the column in every slot of the wave's window, -1 = unknown
    prev_used = None                                 # slots the predecessor of the chain reads
    for g in range(G):
        rr = rows[g][real[g]]
        lens = desc[g, :, 2].astype(np.int64) * real[g]
        longrow = bool(rr.size and op.lens[rr].max() > kTileLen)
        cols_g = np.unique(np.concatenate([op.col[op.rowptr[r]:op.rowptr[r + 1]] for r in rr])) if (rr.size and not longrow) else np.zeros(0, np.int32)
        n_uniq = 0 if longrow else cols_g.size
        aux = desc[g, :, 3]
        want_flag = 1 if (longrow or n_uniq > cap) else 0
        if aux[0] != n_uniq:
            fail("group %d: aux[0] = %d, %d distinct columns" % (g, aux[0], n_uniq))
        if aux[1] != want_flag:
            fail("group %d: flag %d, expected %d (long row %s, %d columns, window %d)" % (g, aux[1], want_flag, longrow, n_uniq, cap))
        at_run_start = run_len > 0 and g % run_len == 0
        if run_len <= 0 or at_run_start:
            window, prev_used = np.full(cap, -1, dtype=np.int64), None
        if aux[1] != 0:
            flagged.append(g)
            window, prev_used = np.full(cap, -1, dtype=np.int64), None       # the chain ends at a flagged group
            continue
        mask = int(aux[2]) & 0xffffffff
        look = int(aux[3])
        if run_len <= 0 and (mask != 0xffffffff or look != 0):
            fail("group %d: records without runs carry mask -1 and look 0 (mask %#x, look %d)" % (g, mask, look))
        if look not in (0, 1):
            fail("group %d: look = %d" % (g, look))
        octets = np.array([(mask >> (q >> 3)) & 1 for q in range(cap)], dtype=bool)
        chain_start = prev_used is None
        # the entries of the group: (slot byte, column)
        k = np.arange(kTileLen)
        ent = (k[None, :] < lens[:, None])
        sl = slots[g][ent].astype(np.int64)
        starts = desc[g, :, 1].astype(np.int64)
        cc = op.col[(starts[:, None] + k[None, :])[ent]].astype(np.int64) if ent.any() else np.zeros(0, np.int64)
        if sl.size and sl.max() >= cap:
            fail("group %d: a slot byte is outside the window (%d >= %d)" % (g, sl.max(), cap))
            window, prev_used = np.full(cap, -1, dtype=np.int64), None
            continue
        after = np.where(octets, lst[g].astype(np.int64), window)
        if run_len > 0 and np.any(after[sl] != cc):
            i = int(np.nonzero(after[sl] != cc)[0][0])
            fail("group %d: sliding window holds column %d in slot %d where an entry needs column %d" % (g, after[sl[i]], sl[i], cc[i]))
        if np.any(lst[g][sl] != cc):
            i = int(np.nonzero(lst[g][sl] != cc)[0][0])
            fail("group %d: the list names column %d in slot %d where an entry needs column %d" % (g, lst[g][sl[i]], sl[i], cc[i]))
        if run_len > 0 and chain_start and sl.size and not np.all(octets[sl]):
            fail("group %d starts a chain and its mask %#x misses an octet it reads" % (g, mask))
        if look == 1:
            if chain_start:
                fail("group %d: look-ahead flag at the start of a chain" % g)
            else:
                changed = octets & (after != window)
                if np.any(changed & prev_used):
                    q = int(np.nonzero(changed & prev_used)[0][0])
                    fail("group %d: look-ahead copy changes slot %d, which group %d still reads" % (g, q, g - 1))
        used = np.zeros(cap, dtype=bool)
        used[sl] = True
        window, prev_used = after, used
    dl = np.sort(np.asarray(direct_list, dtype=np.int64))
    if not np.array_equal(dl, np.array(flagged, dtype=np.int64)):
        fail("the direct list %s is not the set of flagged groups %s" % (dl.tolist()[:8], flagged[:8]))
    return bad


def reference_records(op, b, ahead=None):
    """Host-built records for the build outcome b (tile_build): a plain sliding-window policy of its own (kept columns stay, new
    columns take the lowest slots that are free) -- something sound for the checker's CPU tests to corrupt, not the device's bytes."""
    cap, run_len, rows, cols = b["cap"], b["run_len"], b["rows"], b["cols"]
    ahead = b["ahead"] if ahead is None else ahead
    G = rows.shape[0]
    meta = np.zeros((G, b["stride"]), dtype=np.uint8)
    direct = []
    slot_col, prev_used = None, None
    for g in range(G):
        desc = np.zeros((kTileR, 4), dtype=np.int32)
        lst = np.zeros(cap, dtype=np.int32)
        sl = np.zeros((kTileR, kTileLen), dtype=np.uint8)
        for t in range(kTileR):
            r = rows[g, t]
            desc[t, 0] = r
            if r >= 0:
                desc[t, 1], desc[t, 2] = op.rowptr[r], op.lens[r]
        c = cols[g]
        n_uniq = 0 if c is None else len(c)
        flag = c is None or n_uniq > cap
        desc[0, 3], desc[1, 3], desc[2, 3] = n_uniq, int(flag), -1
        if run_len > 0 and g % run_len == 0:
            slot_col, prev_used = None, None
        if flag:
            direct.append(g)
            slot_col, prev_used = None, None
        else:
            if run_len <= 0:
                where = {int(x): i for i, x in enumerate(c)}
                lst[:] = c[np.minimum(np.arange(cap), n_uniq - 1)] if n_uniq else 0
            else:
                chain = slot_col is not None
                if not chain:
                    slot_col, prev_used = np.full(cap, -1, dtype=np.int64), np.zeros(cap, dtype=bool)
                have = {int(x): q for q, x in enumerate(slot_col) if x >= 0}
                where = {int(x): have[int(x)] for x in c if int(x) in have}
                keep = np.zeros(cap, dtype=bool)
                keep[list(where.values())] = True
                new = [int(x) for x in c if int(x) not in where]
                free2 = [q for q in range(cap) if not keep[q] and not prev_used[q]]
                look = 1 if (ahead and chain and len(free2) >= len(new)) else 0
                free = free2 if look else [q for q in range(cap) if not keep[q]]
                mask = 0
                for x, q in zip(new, free):
                    where[x], slot_col[q] = q, x
                    mask |= 1 << (q >> 3)
                prev_used = np.zeros(cap, dtype=bool)
                prev_used[list(where.values())] = True
                lst[:] = np.where(slot_col >= 0, slot_col, c[-1] if n_uniq else 0)
                desc[2, 3], desc[3, 3] = np.int32(np.uint32(mask).view(np.int32)) if mask >= (1 << 31) else mask, look
            for t in range(kTileR):
                r = rows[g, t]
                if r >= 0:
                    for k in range(op.lens[r]):
                        sl[t, k] = where[int(op.col[op.rowptr[r] + k])]
        meta[g, :kTileDescBytes] = desc.view(np.uint8).ravel()
        meta[g, kTileDescBytes:kTileDescBytes + 4 * cap] = lst.view(np.uint8)
        meta[g, kTileDescBytes + 4 * cap:] = sl.ravel()
    return meta, np.array(direct, dtype=np.int32)


# ---- the judge -----------------------------------------------------------------------------------------------------------------
def serial_spmm(op, X, val=None):
    """Y = A X by the serial stored-order loop: per row and column a rounded multiply, then a rounded add, from +0.0."""
    val = op.val if val is None else val
    Y = np.zeros((op.m, X.shape[1]))
    with np.errstate(all="ignore"):
        for k in range(int(op.lens.max()) if op.m else 0):
            rr = np.nonzero(op.lens > k)[0]
            q = op.rowptr[rr].astype(np.int64) + k
            prod = val[q][:, None] * X[op.col[q]]
            Y[rr] = Y[rr] + prod
    return Y


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def inputs(op, p, seed=0):
    """X (n x p): finite, and special: +Inf, NaN, -0.0 and a subnormal in chosen rows (first, last, and spread)."""
    rng = np.random.default_rng(77 + seed + 13 * p)
    X = rng.standard_normal((op.n, p))
    Xs = X.copy()
    n = op.n
    Xs[n // 3, 0] = np.inf
    Xs[(2 * n) // 3, p - 1] = np.nan
    Xs[0, p // 2] = -0.0
    Xs[n - 1, 0] = 5e-324
    Xs[n // 2, :] = -0.0
    Xs[n // 5, 1 % p] = 2.0 ** -1060
    return X, Xs


def nonfinite_values(op):
    """The same structure with +Inf / -Inf / NaN VALUES where a masked or over-read entry would show: last entries of rows, the
    first entries of the row after a short row (what the 32-entry register path over-reads), entry 32 of a 32-entry row, the last
    entries of the matrix."""
    val = op.val.copy()
    specials = (np.inf, -np.inf, np.nan)
    pick = []
    nz = np.nonzero(op.lens > 0)[0]
    for i, r in enumerate(nz[::max(1, nz.size // 40)]):
        pick.append(int(op.rowptr[r + 1]) - 1)                                # last entry of a row
    short = np.nonzero((op.lens[:-1] < kTileLen) & (op.lens[1:] > 0))[0]
    for r in short[::max(1, short.size // 40)]:
        pick.extend(int(op.rowptr[r + 1]) + j for j in range(min(2, int(op.lens[r + 1]))))   # first entries of the next row
    for r in np.nonzero(op.lens == kTileLen)[0][:8]:
        pick.append(int(op.rowptr[r + 1]) - 1)                                # entry 32 of a 32-entry row
    pick.extend(range(max(0, op.nnz - 3), op.nnz))                            # last entries of the matrix
    for i, q in enumerate(sorted(set(pick))):
        val[q] = specials[i % 3]
    return op.with_values(val, op.name + "+nonfinite")


def panel_rows(n):
    return (n + 15) // 16 * 16


def x_buffer(X):
    """The raw row-major buffer of a panel of X: its padding rows hold NaN."""
    buf = np.full((panel_rows(X.shape[0]), X.shape[1]), np.nan)
    buf[:X.shape[0]] = X
    return buf


def y_prefill(m, p):
    buf = np.zeros((panel_rows(m), p))
    buf[:m] = np.nan
    return buf


def judge_y(op, X, ybuf, what, val=None):
    """Failures of the raw Y buffer (rows < m: the serial product bit for bit; padding rows: still +0.0)."""
    ref = serial_spmm(op, X, val)
    bad = []
    got = ybuf.reshape(-1, X.shape[1])
    if got.shape[0] != panel_rows(op.m):
        return ["%s: Y buffer of %d rows" % (what, got.shape[0])]
    if not same_bits(got[:op.m], ref):
        d = (got[:op.m].view(np.uint64) != ref.view(np.uint64)) & ~(np.isnan(got[:op.m]) & np.isnan(ref))
        i, j = [int(v[0]) for v in np.nonzero(d)]
        bad.append("%s: %d entries differ from the serial product, first Y[%d, %d] = %r, serial %r" % (what, int(d.sum()), i, j, got[i, j], ref[i, j]))
    pad = got[op.m:]
    if pad.size and np.any(pad.view(np.uint64) != 0):
        bad.append("%s: a padding row of Y is no longer +0.0" % what)
    return bad


# ---- the case table ----------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "group name op p options want")
# want: dict of expectations the CPU test asserts FROM THE MODEL'S OWN NUMBERS (the intended side of a rule), e.g. family, NL, cap,
# state, dbuf, ahead, order, min_groups (per workgroup), min_runs, empty_xcd, padded_runs, narrow_pencil, direct, flagged_mid ...

_OPS = {}


def _op(name, make):
    _OPS[name] = make


def get_op(name):
    f = _OPS[name]
    if callable(f):
        _OPS[name] = f = f()
        f.name = name
    return f


def _long(rows_at, n, extra=33):
    """edit: the rows in rows_at get `extra` entries (columns spread around the row)."""
    def edit(rows):
        for r in rows_at:
            rows[r] = sorted(set((r + 3 * k) % n for k in range(extra)))[:extra]
            assert len(rows[r]) == extra
    return edit


def _scatter(groups_at, n, per_row=12, stride=37):
    """edit: the 32 rows of each group in groups_at get per_row scattered columns: more distinct columns than a window of 256."""
    def edit(rows):
        for g in groups_at:
            for t in range(32):
                r = 32 * g + t
                if r < len(rows):
                    rows[r] = sorted(set((r * 11 + t * 101 + stride * k) % n for k in range(per_row)))
    return edit


def _wide(groups_at, n, ncols=300, per_row=24):
    """edit: the 32 rows of each group in groups_at take per_row columns each out of a pool of ncols consecutive ones: more distinct
    columns than a window of 256 holds, and still more than 1.5 references per column."""
    def edit(rows):
        for g in groups_at:
            for t in range(32):
                r = 32 * g + t
                if r < len(rows):
                    rows[r] = sorted(set((32 * g + (t * 9 + 13 * k) % ncols) % n for k in range(per_row)))
                    assert len(rows[r]) == per_row
    return edit


def _empty(rows_at):
    def edit(rows):
        for r in rows_at:
            rows[r] = []
    return edit


def _chain(*edits):
    def edit(rows):
        for e in edits:
            e(rows)
    return edit


_op("g27", lambda: grid_op(13, 10, 9, 27, seed=1))                     # partial tiles in i, j, k; gi, gj, gk = 4, 3, 5
_op("g27x", lambda: grid_op(17, 18, 13, 27, seed=41))                  # gi, gj, gk = 5, 5, 7: 175 groups, 75 runs of 3 (a forced grid of 67 stays above 64)
_op("g7", lambda: grid_op(11, 9, 7, 7, seed=2))
_op("plane", lambda: grid_op(19, 13, 1, 7, seed=3))                    # a single plane: 8 x 4 x 1 tiles, runs along j
_op("g27_pen", lambda: grid_op(12, 21, 6, 27, seed=4))                 # gj = 6: pencils of 4 leave a last pencil of 2
_op("band64", lambda: band_op(1000, 8, 2, seed=5))                     # 32 + 2 h s = 64 distinct columns: NL = 1
_op("band72", lambda: band_op(1000, 10, 2, seed=6))                    # 72: NL = 2
_op("band128", lambda: band_op(1000, 12, 4, seed=7))                   # 128: NL = 2
_op("band136", lambda: band_op(1000, 13, 4, seed=8))                   # 136: NL = 3
_op("band192", lambda: band_op(1000, 10, 8, seed=9))                   # 192: NL = 3
_op("band200", lambda: band_op(1000, 12, 7, seed=10))                  # 200: NL = 4
_op("band_small", lambda: band_op(1003, 3, 1, seed=12))                # 38 distinct columns: window 40, dbuf by rule at every L
# Flagged groups inside runs.  A flagged group is outside the 99 % the window is sized for, so a window small enough for the
# look-ahead (cap + cap / 2 <= 256) needs 100 groups per flagged one: the operators are long, and all but their first rows are empty.
# Identity order, runs of 4: a long row in group 4 (first of a run), 9 and a group of too many columns in 10 (middle, two in a row),
# a long row in 15 (last); group 17 holds empty rows only; the last row is empty; the groups are padded to whole runs.
CHAIN_M = 32 * 520 + 7
_op("band_chain", lambda: band_op(CHAIN_M, 6, 2, seed=13, edit=_chain(
    _empty(range(32 * 24, CHAIN_M - 40)), _empty([CHAIN_M - 1, 600, 601] + list(range(17 * 32, 18 * 32))),
    _long([4 * 32 + 5, 9 * 32 + 31, 15 * 32], CHAIN_M), _wide([10], CHAIN_M))))
# ... on a grid: 4 x 4 x 2 tiles of a 16 x 16 x 62 grid in runs of 8 along k (31 tiles per line: one padding group per line)
_op("g7_chain", lambda: _g7_chain())
# builder thresholds
_op("scatter_refuse", lambda: band_op(640, 0, 1, seed=14, edit=_scatter(range(20), 640, per_row=10, stride=61)))
_op("rows32", lambda: _rows32())
# long rows (33 entries, columns r .. r + 96) that reach across the slab boundaries of 2 and 3 ranks: ghost columns in flagged groups
_op("band_dist_long", lambda: band_op(1000, 6, 2, seed=44, edit=_long([498, 499, 331, 332, 664, 665], 1000)))
_op("band_m571", lambda: band_op(571, 4, 1, seed=43))
_op("band_m100", lambda: band_op(100, 4, 1, seed=15))                  # m < 128: no plane detection


CHAIN_GRID = (16, 16, 62)
CHAIN_TILES = ((0, 0, 0), (0, 0, 7), (2, 1, 10), (2, 1, 11))               # (ti, tj, tk): first and last of a run, two in a row in the middle


def _g7_chain():
    n1, n2, n3 = CHAIN_GRID
    m = n1 * n2 * n3
    extra = {}
    for (ti, tj, tk) in CHAIN_TILES:
        r = (4 * ti + 1) + n1 * ((4 * tj + 2) + n2 * (2 * tk + 1))
        extra[r] = [(r + 1000 + 7 * q) % m for q in range(27)]             # 7 + 27 = 34 entries
    return grid_op(n1, n2, n3, 7, seed=16, extra=extra)


def _win_scatter(groups_at, n, per_row):
    def edit(rows):
        for g in groups_at:
            for t in range(64):
                r = 64 * g + t
                rows[r] = sorted(set((t * per_row + k + 64 * g) % n for k in range(per_row)))      # 64 disjoint sets of per_row columns
    return edit


def _win_dense(groups_at, n, per_row):
    def edit(rows):
        for g in groups_at:
            for t in range(64):
                rows[64 * g + t] = [(64 * g + k) % n for k in range(per_row)]                       # the same per_row columns in every row
    return edit


def _reuse_tile_op(keep):
    """Every group of 32 rows: 96 entries over 64 distinct columns, a score of exactly 1.5 (keep), or one more column (below)."""
    m = 32 * 6
    rng = np.random.default_rng(40)
    rows = [[32 * g + t, 32 * g + (t + 1) % 32, m + 32 * g + t] for g in range(6) for t in range(32)]
    if not keep:
        rows[5] = [rows[5][0], rows[5][2], 2 * m]                          # column 6 stays (row 6 holds it): one more distinct column
    return _from_rows("reuse_tile", m, 2 * m + 1, rows, rng)


def _offsets_op(m, offs, seed):
    rng = np.random.default_rng(3000 + seed)
    rows = [sorted(c for c in [r] + [r + o for o in offs] + [r - o for o in offs] if 0 <= c < m) for r in range(m)]
    return _from_rows("offsets", m, m, rows, rng)


def _reuse_op(keep):
    """Every group of 64 rows: 2 nnz against 3 x distinct columns exactly on the threshold (keep) or one entry below it."""
    m = 64 * 6
    rng = np.random.default_rng(38)
    rows = []
    for g in range(6):
        # 64 rows x 3 entries = 192 entries over 128 distinct columns: 2 x 192 = 3 x 128
        for t in range(64):
            rows.append([64 * g + t, (64 * g + t + 1) % 64 + 64 * g, m + 64 * g + t])
    if not keep:
        rows[5] = [rows[5][0], rows[5][2], m + 64 * 6]                      # column 6 stays (row 6 holds it): 2 nnz < 3 total
    return _from_rows("reuse", m, m + 64 * 6 + 1, rows, rng)


# ---- operators of the threshold families
_op("band168", lambda: band_op(1000, 4, 17, seed=21))                     # 32 + 2 x 68 = 168: 168 + 84 <= 256, the widest window with look-ahead
_op("band176", lambda: band_op(1000, 9, 8, seed=22))                      # 176 + 88 > 256: no look-ahead records
_op("reuse_at", lambda: _reuse_tile_op(True))
_op("reuse_below", lambda: _reuse_tile_op(False))
_op("g_nomult", lambda: _offsets_op(900, (1, 8, 30), seed=39))            # line_rows 8, plane_rows 30: not a multiple
_op("band256", lambda: band_op(1000, 14, 8, seed=23))                     # 32 + 224 = 256 distinct columns: the ceiling itself
_op("band104", lambda: band_op(1000, 12, 3, seed=24))                     # 32 + 72 = 104
_op("band112", lambda: band_op(1000, 10, 4, seed=25))                     # 32 + 80 = 112
# more than 256 distinct columns in some groups (scattered rows of 12 entries: 384 columns), the others a narrow band
_op("band_over_fit", lambda: band_op(1024, 3, 1, seed=26, edit=_wide(list(range(0, 32, 2)), 1024)))               # 16 of 32 groups over: 16 fit (half)
_op("band_over_refuse", lambda: band_op(1024, 3, 1, seed=27, edit=_wide(list(range(0, 32, 2)) + [1], 1024)))      # 17 of 32 over: 15 fit (fewer than half)
_op("g_line5", lambda: grid_op(5, 9, 8, 7, seed=28))
_op("g_line4", lambda: grid_op(4, 9, 8, 7, seed=29))                      # lines of 4 rows merge into the first cluster of offsets
_op("g_planes3", lambda: grid_op(8, 3, 8, 7, seed=30))                    # plane_rows / line_rows = 3
_op("g_planes4", lambda: grid_op(8, 4, 9, 7, seed=31))
_op("plane_short", lambda: grid_op(40, 4, 1, 7, seed=32))                 # one plane, gj = 1: whole lines are runs of one group -> no runs
# window builder: L = 4 (p = 8): 64 rows per group, CAP = 704 columns, 2048 entries
_op("win_cols", lambda: band_op(64 * 12, 3, 1, seed=33, edit=_win_scatter([5], 64 * 12, 12)))          # group 5: 64 x 12 = 768 > 704 distinct columns
_op("win_entries", lambda: band_op(64 * 12, 3, 1, seed=34, edit=_win_dense([6], 64 * 12, 33)))         # group 6: 64 x 33 = 2112 > 2048 entries, few columns
_op("win_refuse_flag", lambda: band_op(64 * 12, 3, 1, seed=35, edit=_win_scatter(range(7), 64 * 12, 12)))   # 7 of 12 flagged: 2 x 7 > 12
_op("win_half_flag", lambda: band_op(64 * 12, 3, 1, seed=36, edit=_win_scatter(range(6), 64 * 12, 12)))     # 6 of 12: 2 x 6 = 12, kept
_op("win_refuse_reuse", lambda: _reuse_op(False))
_op("win_keep_reuse", lambda: _reuse_op(True))
_op("band_sweep", lambda: band_op(64 * 70 + 5, 5, 3, seed=37))             # L = 8: 141 groups of 32 rows; L = 4: 71 of 64
# The 99 % window.  200 groups of a narrow band (38 columns: 40 slots); some groups are widened to 72 columns (9 octets).  With
# 2 widened, 100 x 198 = 99 x 200: exactly on the rule's >=, the window stays at 40 and the two go down the direct path.  With 3,
# 100 x 197 < 99 x 200: the window grows to 72 and takes them.  73 columns in the widened groups: the next octet, 80 slots.
def _fit_op(widened, extra_col, seed):
    m = 32 * 200

    def edit(rows):
        for g in widened:
            for t in range(32):
                r = 32 * g + t
                rows[r] = [r + 2 * k for k in range(-10, 11)]            # 32 + 2 x 20 = 72 distinct columns in the group
            if extra_col:
                rows[32 * g + 31] = rows[32 * g + 31] + [32 * g + 31 + 23]   # odd offset past the group's span: a 73rd column
    return band_op(m, 3, 1, seed=seed, edit=edit)


_op("fit99_two", lambda: _fit_op([50, 120], False, 45))
_op("fit99_three", lambda: _fit_op([50, 120, 121], False, 46))
_op("fit99_three73", lambda: _fit_op([50, 120, 121], True, 47))


def _rows32():
    """Rows of 32, 5 and (one) 33 entries, columns wrapping around: every other row fills the register path to its last entry."""
    m = 400
    rng = np.random.default_rng(42)
    rows = [sorted((i + k) % m for k in range(32 if i % 2 == 0 else (33 if i == 201 else 5))) for i in range(m)]
    return _from_rows("rows32", m, m, rows, rng)


def _forms():
    """The six loop forms of the tile kernels as option sets."""
    return dict(
        one_plain=dict(spmm_tile_pair=0, spmm_tile_slide=0, spmm_tile_dbuf=0),
        one_dbuf=dict(spmm_tile_pair=0, spmm_tile_slide=0, spmm_tile_dbuf=1),
        one_slide=dict(spmm_tile_pair=0, spmm_tile_slide=3, spmm_tile_dbuf=0),
        two_plain=dict(spmm_tile_pair=1, spmm_tile_slide=0, spmm_tile_ahead=0),
        two_slide=dict(spmm_tile_pair=1, spmm_tile_slide=3, spmm_tile_ahead=0),
        two_ahead=dict(spmm_tile_pair=1, spmm_tile_slide=3, spmm_tile_ahead=1))


FORM_FAMILY = dict(one_plain=("tile1", 0, 0, False), one_dbuf=("tile1", 1, 0, False), one_slide=("tile1", 0, 0, True),
                   two_plain=("tile2", 0, 0, False), two_slide=("tile2", 0, 0, True), two_ahead=("tile2", 0, 1, True))
GRIDS = (1, 3, 8, 16, 67)


def _build_cases():
    cases = []

    def add(group, name, op, p, want=None, **kw):
        kw.setdefault("spmm_tile", 2)
        cases.append(Case(group, name, op, p, options(**kw), dict(want or {})))

    forms = _forms()
    # ---- tile_loops: form x forced grid on the 27-point grid with partial tiles
    for f, fo in forms.items():
        fam, dbuf, ahead, slide = FORM_FAMILY[f]
        for g in GRIDS:
            add("tile_loops", "g27x-%s-grid%d" % (f, g), "g27x", 16, dict(family=fam, dbuf=dbuf, ahead=ahead, slide=slide, state=1),
                spmm_tile_grid=g, **fo)
    # each other axis value with each form at least once
    nl_ops = (("band64", 1, 64), ("band72", 2, 72), ("band128", 2, 128), ("band136", 3, 136), ("band192", 3, 192), ("band200", 4, 200))
    others = []
    for i, (f, fo) in enumerate(forms.items()):
        fam, dbuf, ahead, slide = FORM_FAMILY[f]
        w = dict(family=fam, dbuf=dbuf, ahead=ahead, slide=slide, state=1)
        # NL: windows at 64 / 72, 128 / 136, 192 / 200 slots from identity-order bands (look-ahead enlarges by half: 96 ... 256 + refused)
        for (o, nl, cap) in nl_ops:
            if f == "two_ahead" and cap > 168:
                continue                                                   # cap + cap / 2 > 256: no look-ahead records (tile_build group)
            fo2 = dict(fo)
            if slide:
                fo2["spmm_tile_slide"] = 4                                 # identity order: runs of 4 consecutive groups
            w2 = dict(w)
            if f != "two_ahead":
                w2.update(NL=nl, cap=cap)
            others.append(("%s-%s" % (o, f), o, 16, w2, dict(fo2, spmm_tile_grid=(3, 8, 1, 16, 3, 8)[i])))
        # L: p = 8, 32 (p = 16 above); L = 2 exists on the one-wave kernel only
        for p in (8, 32):
            w2 = dict(w)
            if p == 8 and fam == "tile2":
                w2 = dict(state=1, family="tile1", ahead=0, L=2)           # p = 8 has no two-wave kernel: the launch rule falls to one wave
            others.append(("g27-%s-p%d" % (f, p), "g27", p, w2, dict(fo, spmm_tile_grid=(3, 8)[p == 32], spmm_tile_slices=-1)))
        # slices: p = 32 and 64 as 16-column launches
        for p in (32, 64):
            others.append(("g7-%s-slices-p%d" % (f, p), "g7", p, dict(w, launches=p // 16), dict(fo, spmm_tile_grid=3, spmm_tile_slices=1)))
        # the three XCD orders on a grid that is a multiple of 8, and on one that is not
        for xo in (0, 1, 2):
            others.append(("g7-%s-xcd%d" % (f, xo), "g7", 16, w, dict(fo, spmm_tile_grid=16, spmm_tile_xcd=xo)))
        # non-temporal instantiation (one-wave: the rule sends every form there)
        others.append(("plane-%s-nt" % f, "plane", 16, dict(state=1, family="tile1", ahead=0, nt=1), dict(fo, spmm_tile_grid=3, spmm_tile_nt=1)))
        # pencils of 4 with gj = 6 (the last pencil is narrower); pencil order only without runs
        others.append(("g27_pen-%s-pencil4" % f, "g27_pen", 16, dict(w, narrow_pencil=not slide), dict(fo, spmm_tile_grid=8, spmm_tile_pencil=4)))
        # run lengths: whole lines (1), 2, 3, 7 on grids and on the identity order; shapes 4 and 5
        for sl in (1, 2, 7):
            if slide:
                others.append(("g27-%s-slide%d" % (f, sl), "g27", 16, w, dict(fo, spmm_tile_slide=sl, spmm_tile_grid=3)))
                others.append(("band72-%s-slide%d" % (f, sl), "band72", 16, w, dict(fo, spmm_tile_slide=sl, spmm_tile_grid=1 if sl == 1 else 3)))
        # shape 4 (8 x 4 x 1 tiles) and 5 (32 x 1 x 1: whole pieces of lines -- their distinct columns add up to those of the identity
        # order, the score ties, and the builder keeps the identity order: the case holds the device to that)
        others.append(("g27-%s-shape4" % f, "g27", 16, dict(w, order="runs" if slide else "pencil"), dict(fo, spmm_tile_shape=4, spmm_tile_grid=8)))
        others.append(("g27-%s-shape5" % f, "g27", 16, dict(state=1, order="identity"), dict(fo, spmm_tile_shape=5, spmm_tile_grid=8)))
        others.append(("plane-%s" % f, "plane", 16, w, dict(fo, spmm_tile_grid=3)))
        fo2 = dict(fo, spmm_tile_grid=3)
        if slide:
            fo2["spmm_tile_slide"] = 4
        others.append(("band_small-%s" % f, "band_small", 16, dict(w, NL=1), fo2))       # 40 slots (60 -> 64 with look-ahead): NL = 1
        others.append(("g7-%s-grid1" % f, "g7", 16, w, dict(fo, spmm_tile_grid=1)))
        # 18 groups (9 runs of 2) over 8 workgroups by eighths: 3 groups (2 runs) per XCD leave XCDs without a group, without a run
        fo2 = dict(fo, spmm_tile_grid=8, spmm_tile_xcd=0)
        if slide:
            fo2["spmm_tile_slide"] = 2
        others.append(("band_m571-%s-grid8-eighths" % f, "band_m571", 16, w, fo2))
        # rows of exactly 32 entries next to short ones, and rows of 33 (flagged): the register path's last entry and what it over-reads
        fo2 = dict(fo, spmm_tile_grid=3)
        if slide:
            fo2["spmm_tile_slide"] = 4
        others.append(("rows32-%s" % f, "rows32", 16, dict(w, ahead=None), fo2))
    for name, o, p, w, kw in others:
        add("tile_loops", name, o, p, w, **kw)
    # spmm_tile_waves multiplies the residency-derived grid of the one-wave kernel: no forced grid, so the model predicts the form only
    add("tile_loops", "g27x-one_plain-waves2", "g27x", 16, dict(family="tile1", dbuf=0, state=1, no_grid=True), spmm_tile_waves=2, **forms["one_plain"])
    add("tile_loops", "g27x-one_slide-waves3", "g27x", 16, dict(family="tile1", slide=True, state=1, no_grid=True), spmm_tile_waves=3, **forms["one_slide"])
    # ---- tile_chain: flagged groups inside runs; sliding, look-ahead, and the same records under dbuf
    for o, sl in (("band_chain", 4), ("g7_chain", 8)):
        for tag, kw in (("slide", dict(spmm_tile_pair=1, spmm_tile_ahead=0)), ("ahead", dict(spmm_tile_pair=1, spmm_tile_ahead=1)),
                        ("slide1", dict(spmm_tile_pair=0, spmm_tile_dbuf=0, spmm_tile_ahead=1)), ("dbuf", dict(spmm_tile_pair=0, spmm_tile_dbuf=1))):
            for g in (1, 3):
                add("tile_chain", "%s-%s-grid%d" % (o, tag, g), o, 16,
                    dict(state=1, chain=True, form={"slide": "tile2-slide", "ahead": "tile2-ahead", "slide1": "tile1-slide", "dbuf": "tile1-dbuf"}[tag]),
                    spmm_tile_slide=sl, spmm_tile_grid=g, **kw)
    # ---- tile_build: either side of each builder rule
    add("tile_build", "reuse-below", "reuse_below", 16, dict(state=-1, family_not_tile=True))
    add("tile_build", "reuse-at-1.5", "reuse_at", 16, dict(state=1, reuse=1.5))
    add("tile_build", "reuse-scattered", "scatter_refuse", 16, dict(state=-1, family_not_tile=True))
    add("tile_build", "window99-on-the-rule", "fit99_two", 16, dict(state=1, cap=40, direct=2), spmm_tile_slide=0)
    add("tile_build", "window99-below-the-rule", "fit99_three", 16, dict(state=1, cap=72, direct=0), spmm_tile_slide=0)
    add("tile_build", "window99-next-octet", "fit99_three73", 16, dict(state=1, cap=80, direct=0), spmm_tile_slide=0)
    add("tile_build", "window99-on-the-rule-runs", "fit99_two", 16, dict(state=1, cap=40, direct=2), spmm_tile_slide=4, spmm_tile_grid=3)
    add("tile_build", "window-rounds-64", "band64", 16, dict(state=1, cap=64, NL=1), spmm_tile_slide=0)
    add("tile_build", "window-rounds-72", "band72", 16, dict(state=1, cap=72, NL=2), spmm_tile_slide=0)
    add("tile_build", "ahead-fits-168", "band168", 16, dict(state=1, cap0=168, cap=256, ahead=1, NL=4), spmm_tile_slide=4, spmm_tile_ahead=1)
    add("tile_build", "ahead-refused-176", "band176", 16, dict(state=1, cap=176, ahead=0, family="tile2"), spmm_tile_slide=4, spmm_tile_ahead=1)
    add("tile_build", "ahead-rounds-up-72", "band72", 16, dict(state=1, cap0=72, cap=112, ahead=1), spmm_tile_slide=4, spmm_tile_ahead=1)
    add("tile_build", "ceiling-256", "band256", 16, dict(state=1, cap=256, direct=0), spmm_tile_slide=0)
    add("tile_build", "ceiling-over-half-fit", "band_over_fit", 16, dict(state=1, cap=256, direct_min=1), spmm_tile_slide=0)
    add("tile_build", "ceiling-under-half-fit", "band_over_refuse", 16, dict(state=-1), spmm_tile_slide=0)
    add("tile_build", "dbuf-rule-fits-p16", "band_small", 16, dict(state=1, dbuf=1, family="tile1"), spmm_tile_pair=0)          # 2 x 40 x 128 B <= 26 KiB
    add("tile_build", "dbuf-rule-104-p16", "band104", 16, dict(state=1, cap=104, dbuf=1, family="tile1"), spmm_tile_pair=0)     # 2 x 104 x 128 = 26 KiB exactly
    add("tile_build", "dbuf-rule-112-p16", "band112", 16, dict(state=1, cap=112, dbuf=0, family="tile1"), spmm_tile_pair=0)
    # (line_rows 3 / 4: csr_finalize cannot report a line distance below 5 -- a cluster of offsets starts only past 2 x 1 + 2 -- so
    # that side of grid_ok is checked on the model's rule alone, tests/test_spmm_model_host.py; here the smallest it can report)
    add("tile_build", "grid-line5", "g_line5", 16, dict(line_rows=5, grid_ok=True))
    add("tile_build", "grid-line4-undetected", "g_line4", 16, dict(line_rows=36, plane_rows=36))
    add("tile_build", "grid-plane-no-multiple", "g_nomult", 16, dict(line_rows=8, plane_rows=30, grid_ok=False, order="identity"))
    add("tile_build", "grid-planes3", "g_planes3", 16, dict(line_rows=8, plane_rows=24, grid_ok=False, order="identity"))
    add("tile_build", "grid-planes4", "g_planes4", 16, dict(line_rows=8, plane_rows=32, grid_ok=True))
    add("tile_build", "no-detection-m100", "band_m100", 16, dict(line_rows=0, order="identity", state=1))
    add("tile_build", "runlen-falls-to-0", "plane_short", 16, dict(state=1, run_len=0), spmm_tile_slide=1)
    add("tile_build", "p64-without-slices", "g7", 64, dict(family_not_tile=True), spmm_tile_slices=-1)
    # ---- tile_dist: the DIST instantiations on in-process ranks (want["world"]); every slab has ghost panel rows
    fm = forms
    for name, o, p, world, kw in (
            ("g27-one_plain-grid1-w2", "g27", 16, 2, dict(fm["one_plain"], spmm_tile_grid=1)),
            ("g27-one_slide-grid8-w3", "g27", 16, 3, dict(fm["one_slide"], spmm_tile_grid=8)),
            ("g27-one_dbuf-grid8-w2", "g27", 16, 2, dict(fm["one_dbuf"], spmm_tile_grid=8)),
            ("g27-two_plain-grid8-w2", "g27", 16, 2, dict(fm["two_plain"], spmm_tile_grid=8)),
            ("g27-two_slide-grid1-w3", "g27", 16, 3, dict(fm["two_slide"], spmm_tile_grid=1)),
            ("g7-two_ahead-grid1-w2", "g7", 16, 2, dict(fm["two_ahead"], spmm_tile_grid=1)),
            ("g7-two_ahead-grid8-w3", "g7", 16, 3, dict(fm["two_ahead"], spmm_tile_grid=8)),
            ("band72-two_ahead-grid1-w3", "band72", 16, 3, dict(fm["two_ahead"], spmm_tile_grid=1, spmm_tile_slide=4)),
            ("g27-one_plain-p8-w3", "g27", 8, 3, dict(fm["one_plain"], spmm_tile_grid=8)),
            ("g27-two_plain-p32-w2", "g27", 32, 2, dict(fm["two_plain"], spmm_tile_grid=1, spmm_tile_slices=-1)),
            ("g7-two_slide-slices-p32-w2", "g7", 32, 2, dict(fm["two_slide"], spmm_tile_grid=8, spmm_tile_slices=1)),
            ("band_dist_long-two_slide-grid1-w2", "band_dist_long", 16, 2, dict(fm["two_slide"], spmm_tile_grid=1, spmm_tile_slide=4)),
            ("band_dist_long-one_plain-grid8-w3", "band_dist_long", 16, 3, dict(fm["one_plain"], spmm_tile_grid=8))):
        add("tile_dist", name, o, p, dict(world=world, long_ghost=o == "band_dist_long"), **kw)
    # the window kernel's DIST arm, both POW2 arms
    for name, p, world in (("g27-window-p16-w2", 16, 2), ("g27-window-p12-w3", 12, 3), ("g27-window-p8-w3", 8, 3)):
        add("tile_dist", name, "g27", p, dict(world=world, family="window"), spmm_tile=0, spmm_window_grid=3)
    # ---- window: spmm_window_kernel under a forced grid
    for g in (1, 3, 8, 64):
        add("window", "g27-p16-grid%d" % g, "g27", 16, dict(family="window"), spmm_tile=0, spmm_window_grid=g)
    for p in (2, 4, 6, 8, 12, 16, 24, 32):
        add("window", "band_small-p%d-grid3" % p, "band_small", p, dict(family="window" if p >= 4 else "spmm_kernel"), spmm_tile=0, spmm_window_grid=3)
    add("window", "flagged-by-columns-p8", "win_cols", 8, dict(family="window", by_columns=True), spmm_tile=0, spmm_window_grid=3)
    add("window", "flagged-by-entries-p8", "win_entries", 8, dict(family="window", by_entries=True), spmm_tile=0, spmm_window_grid=3)
    add("window", "refused-most-flagged-p8", "win_refuse_flag", 8, dict(family="spmm2_kernel", win_refused=True), spmm_tile=0, spmm_window_grid=3)
    add("window", "kept-half-flagged-p8", "win_half_flag", 8, dict(family="window"), spmm_tile=0, spmm_window_grid=3)
    add("window", "refused-no-reuse-p8", "win_refuse_reuse", 8, dict(family="spmm2_kernel", win_refused=True), spmm_tile=0, spmm_window_grid=3)
    add("window", "kept-reuse-1.5-p8", "win_keep_reuse", 8, dict(family="window"), spmm_tile=0, spmm_window_grid=3)
    add("window", "sweep-p16", "band_sweep", 16, dict(family="window", sweep=True, padding=True), spmm_tile=0, spmm_window_grid=64, spmm_win_sweep=1,
        spmm_sweep_s=24, spmm_sweep_w=2)
    add("window", "sweep-p8", "band_sweep", 8, dict(family="window", sweep=True, padding=True), spmm_tile=0, spmm_window_grid=67, spmm_win_sweep=1,
        spmm_sweep_s=20, spmm_sweep_w=1)
    add("window", "spmm2-sweep-p16", "band_sweep", 16, dict(family="spmm2_kernel", sweep=True), spmm_tile=0, spmm_window=0, spmm_sweep=1,
        spmm_sweep_s=20, spmm_sweep_w=2)
    add("window", "spmm-sweep-p5", "band_sweep", 5, dict(family="spmm_kernel", sweep=True), spmm_tile=0, spmm_sweep=1, spmm_sweep_s=20, spmm_sweep_w=2)
    return cases


CASES = None


def cases():
    global CASES
    if CASES is None:
        CASES = _build_cases()
        names = [c.name for c in CASES]
        assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return CASES


def cases_of(group):
    return [c for c in cases() if c.group == group]


def case_slabs(case):
    op = get_op(case.op)
    st = row_partition(op.m, case.want["world"])
    key = ("slabs", case.want["world"])
    if key not in op._cache:
        op._cache[key] = [slab_op(op, st[r], st[r + 1]) for r in range(case.want["world"])]
    return op._cache[key]


def case_walk(case, op=None):
    """(launch, walk, stats) of a case from the model alone; walk is None where no grid is forced or no loop exists.  op: a slab of
    the case's operator (tile_dist)."""
    dist = op is not None
    op = get_op(case.op) if op is None else op
    ln = launch(op, case.options, case.p, dist and op.n > op.m)
    if ln["grid"] is None or ln["error"]:
        return ln, None, None
    if ln["family"] in ("tile1", "tile2"):
        b = tile_build(op, case.options)
        w = walk_tile(ln["family"], b["groups"], b["runs"], ln["run_len"], ln["grid"], ln["xcd"], ln["dbuf"])
        return ln, w, walk_stats(w, ln["run_len"])
    if ln["family"] == "window":
        wb = window_build(op, ln["L"])
        w = walk_window(wb["all_groups"], ln["grid"], ln["sweep_S"], ln["sweep_W"], ln["sweep_K"], ln["sweep_cols"])
        return ln, w, walk_stats(w)
    rpb = kBlock // ln["L"]
    w = walk_direct((op.m + rpb - 1) // rpb, ln["grid"], ln["sweep_S"], ln["sweep_W"])
    return ln, w, walk_stats(w)


def form_name(ln):
    if ln["family"] == "tile1":
        return "tile1-" + ("dbuf" if ln["dbuf"] else ("slide" if ln["run_len"] else "plain"))
    if ln["family"] == "tile2":
        return "tile2-" + ("ahead" if ln["ahead"] else ("slide" if ln["run_len"] else "plain"))
    if ln["family"] == "window":
        return "window-sweep" if ln["sweep_S"] else "window"
    return ln["family"] + ("-sweep" if ln["sweep_S"] else "")
