"""A host model of the stored forms of a CSR handle and of their builders' thresholds.

A handle is never multiplied as it was given: on first use the library builds derived forms on the device -- dictionary codes
(csrc/colcode.hip csr_build_codes), the sliced copy in six layouts (build_sell_form, modes 0-5), the block-delta column stream
with escape lists (csrc/coldelta.hip), row templates (csrc/template.hip), the adjoint handle (csrc/csr_aux.hip csr_transpose)
-- and spmv_plan / spmv_kernel_choice (csrc/spmv.hip) decide which one a product reads.  This file restates every builder as
a NumPy ENCODER (the arrays the builder writes) and every kernel's read side as a DECODER (the columns, values and "no entry"
marks the kernel takes out of those arrays), multiplies in stored order with one rounded multiply and one rounded add per
entry (vectorised over the rows, entry position by entry position: the serial loop's rounding sequence), and holds

  * the builders' constants, pinned to the sources (`forms_source_constants`),
  * operator families that each sit on one edge of one builder, both sides of every edge (`OPS`),
  * the (family, option set) table `CASES`: every case states the form it is there for (`want`), `expected` derives every
    reported field (kernel number, code bits and T, sell state / units / total / narrow, sell32 state, delta bits / rows /
    escapes, templates, khip_spmv_bytes_stored) from the builders' rules, with partition_model.predict for the plan,
  * the coverage condition `coverage` (tests/test_operator_forms_host.py asserts it),
  * the emulation `emulate` (which can carry the injected faults `FAULTS`) and the comparison `judge` that the GPU file
    (tests/test_gpu_operator_forms_exact.py) hands the device's results to: the form first, then the numbers.

Values: partition_model._values; a few -0.0 / +0.0 / subnormal values are sprinkled over val, and +Inf / NaN / -0.0 / a
subnormal over the second input vector.  Every case runs on TWO handles: the finite one above, which also carries the fused
scalars (exact_reduction holds a scalar to an exact value, and a non-finite y has none), and `Op.nonfinite()`, the same structure
with +Inf / -Inf / NaN in val at the places where a kernel masks an entry by gathering x = 0.0 -- escape positions of both delta
widths, the first and last entries of rows at block boundaries, the last entry of rows shorter than their slice, the last entry
of all -- on which y alone is compared, bit for bit and NaN for NaN, on the finite rows too: a masked entry that is wrongly
accumulated adds 0 with a finite value and shows as NaN with these.  The families that
reach the vector kernel (mean row above 96: mean96, mean96_plus, the adjoints of tr_m1 / tr_n1) carry no subnormal: that kernel
is held to a RELATIVE row bound, gamma(k) sum|a x|, which a product that underflows does not obey in any summation order.

Fused scalars: spmv_dot / spmv_dot2 read x[row] for row < m, so they run where n >= m (x . y is then x[:m] . y); spmv_dotw
runs everywhere.  Host only: NumPy, exact_reduction and the oracle's serial loop.
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
import partition_model as pm  # noqa: E402
from partition_model import _sell_builds, _sell_units, _values, predict, source_constants, vector_row_bound  # noqa: E402,F401

# ---------------------------------------------------------------------------------------------------- constants of the sources
CODE_HASH, CODE_MAX, CODE_PAD = 4096, pm.CODE_MAX, 64             # colcode.hip kCodeHash / kCodeMax / kCodePad
SELL_MAX_PAD, SELL_UNIFORM_PAD, SELL_SLACK = pm.SELL_MAX_PAD, 1.02, pm.SELL_SLACK
CODED_MAX_ROW = pm.CODED_MAX_ROW                                  # spmv.hip kCodedMaxRow
MARK8, MARK4, MARK32 = 0xFF, 0xF, 0xFFFFFFFF                      # "no entry" in a code word / narrow code word / column word
SELL_MAX_T, NARROW_MAX_T, NARROW_MAX_ROW = 255, 15, 8             # build_sell_form: code_T > 255 refused; narrow: T <= 15, rows <= 8
SELL_MAX_ROW = 64
DELTA_PAD, DELTA_BLOCK_MAX = 64, 65535                            # coldelta.hip kDeltaPad; entries of a block (16-bit esc_pos)
TMPL_MAX_LEN, TMPL_MAX, TMPL_HASH, TMPL_LDS_MAX, TMPL_PROBES = pm.TMPL_MAX_LEN, pm.TMPL_MAX, 8192, pm.TMPL_LDS_MAX, 256
SCAN_TILE = 2048                                                  # csr_aux.hip kScanTile
PLAN_SHORT_MEAN, PLAN_STREAM_MEAN, PLAN_WINDOW = 12.0, 96.0, pm.STAGE_WINDOW
BIG_NNZ = pm.BIG_NNZ
SLICE = pm.SLICE


def forms_source_constants(root=ROOT):
    """The constants above read out of the sources (tests/test_operator_forms_host.py compares): a changed threshold fails a
    host test instead of being silently followed."""
    src = os.path.join(root, "krylov.jl_amd", "csrc")
    text = {f: open(os.path.join(src, f)).read() for f in ("colcode.hip", "coldelta.hip", "template.hip", "csr_aux.hip", "spmv.hip")}
    cc, cd, tp, ca, sp = (text[f] for f in ("colcode.hip", "coldelta.hip", "template.hip", "csr_aux.hip", "spmv.hip"))

    def num(pattern, s, conv=int):
        m = re.search(pattern, s)
        return conv(m.group(1)) if m else None
    out = dict(
        code_hash=num(r"constexpr int kCodeHash = (\d+);", cc), code_max=num(r"constexpr int kCodeMax = (\d+);", cc),
        code_pad=num(r"constexpr int kCodePad = (\d+);", cc), sell_max_pad=num(r"constexpr double kSellMaxPad = ([0-9.]+);", cc, float),
        sell_uniform_pad=num(r"constexpr double kSellUniformPad = ([0-9.]+);", cc, float),
        coded_max_row=num(r"constexpr int kCodedMaxRow = (\d+);", sp),
        code_bits_rule="const int bits = (T <= 256 && ctx->tune.spmv_codes != 16) ? 8 : 16;" in cc,
        code_count_rule="if (atomicAdd(&count_fail[0], 1) >= kCodeMax) atomicMax(&count_fail[1], 1);" in cc and "if (T == 0 || T > kCodeMax) return KHIP_OK;" in cc,
        mark8="const unsigned long long c = k < len ? (unsigned long long)code[q0 + k] : 0xFFull;" in cc and sp.count("c != 0xFF;") >= 3,
        mark4="word |= (u < len ? (uint32_t)code[q0 + u] : 0xFu) << (4 * u);" in cc and "on[u] = c != 0xF;" in sp,
        mark32=": 0xFFFFFFFFull;" in cc and "on[u] = cc[u] != -1;" in sp,
        sell_limits="A->max_row_nnz > 64) return KHIP_OK;" in cc and "A->code_bits != 8 || A->code_T > 255)) return KHIP_OK;" in cc,
        narrow_rule="ctx->tune.spmv_sell_narrow && A->code_T <= 15 && A->max_row_nnz <= 8;" in cc,
        mode_rule="const int mode = cols32 ? ((pair && ctx->tune.spmv_sell_pair >= 2) ? 4 : 1) : (narrow ? 2 : (pair ? (A->max_row_nnz <= 8 ? 3 : 5) : 0));" in cc,
        pad_rule="if (512.0 * (double)total > kSellMaxPad * ref_bytes + 65536.0) return KHIP_OK;" in cc,
        uniform_rule="const bool uniform = (double)umax * (double)slices <= kSellUniformPad * (double)total + 8.0;" in cc,
        head_words=("if (mode == 5) return T <= 18 ? 2 : (T <= 36 ? 4 : (T <= 54 ? 6 : 8));" in cc and "if (mode == 4) return 2 * ((T - 4) / 6) + 2;" in cc
                    and "return mode == 3 ? 1 : (mode == 2 ? 0 : (mode == 1 ? (T + 2) / 3 : (T + 8) / 9));" in cc),
        head_words_kernel="(PAIRG ? (COLS32 ? 2 * ((T - 4) / 6) + 2 : (T <= 18 ? 2 : (T <= 36 ? 4 : (T <= 54 ? 6 : 8))))" in sp
                          and ": (PAIR ? 1 : (C4 ? 0 : (COLS32 ? (T + 2) / 3 : (T + 8) / 9))));" in sp,
        delta_pad=num(r"constexpr int kDeltaPad = (\d+);", cd),
        delta_base=("const int64_t H = (((int64_t)1 << bits) - 1 - rows) / 2;" in cd and "const int64_t b = r0 - (H > 0 ? H : 0);" in cd
                    and "return (int32_t)(b > 0 ? b : 0);" in cd),
        delta_escape=("e8 += (c < b8 || c - b8 >= 255);" in cd and "e16 += (c < b16 || c - b16 >= 65535);" in cd
                      and "if (c < base || c - base >= ESC) {" in cd),
        delta_block_max=[int(v) for v in re.findall(r"if \(rowptr\[hi\] - rowptr\[row\] > (\d+)\) atomicMax\(too_long, 1\);", cd)],
        delta_rows8="const int rows16 = rows, rows8 = rows < 64 ? rows : 64;" in cd,
        delta_bytes=("const int64_t by8 = A->nnz + 6 * esc8, by16 = 2 * A->nnz + 6 * esc16, by32 = 4 * A->nnz;" in cd and "int bits = by8 <= by16 ? 8 : 16;" in cd
                     and "if (ctx->tune.spmv_delta < 2 && 6 * by > 5 * by32) return KHIP_OK;" in cd),
        delta_try="if (build && wide_ok && dl && (dl != 1 || big) && A->delta_state == 0) optional_build(csr_build_delta(ctx, Am, rows));" in sp,
        tmpl_max_len=num(r"constexpr int kTmplMaxLen = (\d+);", tp), tmpl_max=num(r"constexpr int kTmplMax = (\d+);", tp),
        tmpl_hash=num(r"constexpr int kTmplHash = (\d+);", tp), tmpl_lds_max=num(r"constexpr size_t kTmplLdsMax = (\d+) \* 1024;", tp),
        tmpl_probes={int(v) for v in re.findall(r"for \(int probe = 0; probe < (\d+); \+\+probe\)", tp)},
        tmpl_rule=("if (m == 0 || A->max_row_nnz > kTmplMaxLen || A->max_row_nnz < 1) return KHIP_OK;" in tp and
                   "if (T == 0 || T > kTmplMax || (size_t)T * K * 12 + (size_t)T * 4 > kTmplLdsMax) return KHIP_OK;" in tp),
        tmpl_by_bits="(__double_as_longlong(val[q]) == __double_as_longlong(t_val[(size_t)t * K + (q - s)]));" in tp,
        scan_tile=num(r"constexpr int kScanTile = (\d+);", ca),
        plan_short="const bool short_rows = A->mean_row_nnz <= 12.0 && A->max_row_nnz <= kCodedMaxRow;" in sp,
        plan_stream="kernel = (short_rows || coded) ? 4 : (A->mean_row_nnz <= 96.0 ? 1 : 2);" in sp,
        plan_window=sorted({float(v) for v in re.findall(r"rows \* A->mean_row_nnz > ([0-9.]+)\)", sp)}),
    )
    return out


EXPECTED_SOURCE_CONSTANTS = dict(
    code_hash=CODE_HASH, code_max=CODE_MAX, code_pad=CODE_PAD, sell_max_pad=SELL_MAX_PAD, sell_uniform_pad=SELL_UNIFORM_PAD,
    coded_max_row=CODED_MAX_ROW, code_bits_rule=True, code_count_rule=True, mark8=True, mark4=True, mark32=True, sell_limits=True,
    narrow_rule=True, mode_rule=True, pad_rule=True, uniform_rule=True, head_words=True, head_words_kernel=True, delta_pad=DELTA_PAD,
    delta_base=True, delta_escape=True, delta_block_max=[DELTA_BLOCK_MAX, DELTA_BLOCK_MAX], delta_rows8=True, delta_bytes=True,
    delta_try=True, tmpl_max_len=TMPL_MAX_LEN, tmpl_max=TMPL_MAX, tmpl_hash=TMPL_HASH, tmpl_lds_max=TMPL_LDS_MAX // 1024,
    tmpl_probes={TMPL_PROBES}, tmpl_rule=True, tmpl_by_bits=True, scan_tile=SCAN_TILE, plan_short=True, plan_stream=True,
    plan_window=[PLAN_WINDOW])


# ---------------------------------------------------------------------------------------------------- operators

def _seed(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name)) % (1 << 31)


class Op:
    """A CSR operator on the host: rowptr int64, col int32, val float64; rows may hold unsorted and repeated columns."""

    def __init__(self, name, m, n, rowptr, col, val, subnormal=True):
        self.name, self.m, self.n, self.subnormal = name, int(m), int(n), subnormal
        self.rowptr = np.ascontiguousarray(rowptr, dtype=np.int64)
        self.col = np.ascontiguousarray(col, dtype=np.int32)
        self.val = np.ascontiguousarray(val, dtype=np.float64)
        self.nnz = int(self.rowptr[-1])
        assert self.rowptr.size == self.m + 1 and self.col.size == self.nnz == self.val.size
        assert self.nnz == 0 or (0 <= int(self.col.min()) and int(self.col.max()) < self.n), name
        self.lens = np.diff(self.rowptr)
        self.row_of = np.repeat(np.arange(self.m, dtype=np.int64), self.lens)
        self._inputs, self._nf = None, None

    def info(self):
        """What partition_model.predict reads."""
        d = np.unique(self.col.astype(np.int64) - self.row_of) if self.nnz else np.zeros(0)
        return dict(m=self.m, nnz=self.nnz, max_row=int(self.lens.max()) if self.m else 0, mean_row=self.nnz / self.m if self.m else 0.0,
                    diagonals=int(d.size), lens=self.lens)

    def serial(self, x):
        """The plain serial product (the oracle's ko_spmv: acc = 0; acc = acc + val[q] * x[col[q]] in stored order); a
        rectangular operator is embedded in a square one (empty rows / zero entries of x behind its own)."""
        import oracle as ok
        N = max(self.m, self.n)
        rp = np.concatenate([self.rowptr, np.full(N - self.m, self.nnz, dtype=np.int64)])
        xx = np.concatenate([np.asarray(x, dtype=np.float64), np.zeros(N - self.n)])
        with np.errstate(all="ignore"):
            return ok.CsrMatrix.from_arrays(rp, self.col, self.val).matvec(xx)[:self.m].copy()

    def nonfinite(self):
        """The same operator with +Inf, -Inf and NaN in val where the kernels mask entries: escapes of the 8- and 16-bit delta
        stream (blocks of 32 / 64 / 256 rows), first and last entries of rows next to a 32-row boundary, last entries of rows
        shorter than the longest of their slice, the last entry of all.  At most 36 entries, in different rows where possible."""
        if self._nf is None:
            q = []
            if self.nnz:
                for bits, R in ((8, 32), (8, 64), (16, 32), (16, 256)):
                    esc = np.flatnonzero(_escapes(self, R, bits)[2])
                    q += esc[np.linspace(0, esc.size - 1, 3).astype(int)].tolist() if esc.size else []
                rows = np.flatnonzero(self.lens > 0)
                edge = rows[(rows % 32 == 31) | (rows % 32 == 0)]
                for r in edge[np.linspace(0, edge.size - 1, 8).astype(int)] if edge.size else []:
                    q.append(int(self.rowptr[r]) if r % 32 == 0 else int(self.rowptr[r + 1]) - 1)
                smax = np.repeat(np.maximum.reduceat(self.lens, np.arange(0, self.m, SLICE)), SLICE)[:self.m]
                short = np.flatnonzero((self.lens > 0) & (self.lens < smax))
                q += [int(self.rowptr[r + 1]) - 1 for r in (short[np.linspace(0, short.size - 1, 6).astype(int)] if short.size else [])]
                q += [0, self.nnz - 1]
            val = self.val.copy()
            seen = set()
            for i, k in enumerate(dict.fromkeys(q)):
                if self.row_of[k] in seen and k != self.nnz - 1:
                    continue
                seen.add(self.row_of[k])
                val[k] = (np.inf, np.nan, -np.inf)[i % 3]
            self._nf = Op(self.name, self.m, self.n, self.rowptr, self.col, val, self.subnormal)
            self._nf._nf = self._nf
        return self._nf

    def inputs(self):
        """x (finite), the special x (+Inf, NaN, -0.0 and a subnormal in four columns), a weight vector, and the serial
        products.  NaN sits, where there is one, in the column r of a row r that is shorter than the longest row of its 64-row
        slice and does not reference column r: the only place where a padding slot read as an entry (0.0 * x[row]) shows."""
        if self._inputs is None:
            rng = np.random.default_rng(_seed(self.name) + 1)
            x, w = pm._vec(rng, self.n), pm._vec(rng, self.m)
            xs = x.copy()
            cand = []
            if self.nnz:
                smax = np.repeat(np.maximum.reduceat(self.lens, np.arange(0, self.m, SLICE)), SLICE)[:self.m]
                diag = np.zeros(self.m, dtype=bool)
                diag[self.row_of[self.col == self.row_of]] = True
                cand = np.flatnonzero((self.lens < smax) & ~diag & (np.arange(self.m) < self.n)).tolist()
            cols = np.unique(self.col) if self.nnz else np.arange(min(self.n, 1))
            nan_c = cand[len(cand) // 2] if cand else int(cols[(2 * cols.size) // 3])
            rest = cols[cols != nan_c] if (cols != nan_c).any() else np.array([nan_c])
            inf_c, mz_c, sub_c = (int(rest[(f * rest.size) // 4]) for f in (1, 2, 3))
            xs[sub_c], xs[mz_c], xs[inf_c], xs[nan_c] = (3e-310 if self.subnormal else 0.0), -0.0, np.inf, np.nan
            self._inputs = dict(x=x, xs=xs, w=w, y=self.serial(x), ys=self.serial(xs))
        return self._inputs


def _sprinkle(rowptr, col, val, subnormal=True):
    """-0.0, +0.0 and two subnormals over val: in four different rows and four different columns that each hold another entry, so
    that no row of A or of A' sums to a number below the window in which exact_reduction's products are exact."""
    lens = np.diff(rowptr)
    row_of = np.repeat(np.arange(lens.size), lens)
    ok = np.flatnonzero((lens[row_of] >= 2) & (np.bincount(col, minlength=int(col.max()) + 1 if col.size else 1)[col] >= 2))
    rows, cols = set(), set()
    vals = [-0.0, 0.0] + ([4e-310, -2e-320] if subnormal else [])
    for q in ok[np.linspace(0, ok.size - 1, 64).astype(int)] if ok.size else []:
        if vals and row_of[q] not in rows and col[q] not in cols:
            rows.add(row_of[q]); cols.add(col[q])
            val[q] = vals.pop(0)
    return val


def _from_rows(name, n, rows, val=None, subnormal=True):
    """rows: a list of column arrays, stored order as given."""
    m = len(rows)
    rowptr = np.zeros(m + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=rowptr[1:])
    col = np.concatenate([np.asarray(r, dtype=np.int64) for r in rows]) if m and rowptr[-1] else np.zeros(0, dtype=np.int64)
    rng = np.random.default_rng(_seed(name))
    if val is None:
        val = _sprinkle(rowptr, col, _values(rng, col.size), subnormal)
    return Op(name, m, n, rowptr, col, val, subnormal)


def diag_op(name, T, kind="plain"):
    """Exactly T distinct offsets col - row.  plain: offsets 0 .. T - 1 on an m x (m + T) operator; last: the largest offset
    occurs only in the last row; neg: offsets -T .. -1 only (rows that cannot reach them are shorter or empty)."""
    Tc = T - 1 if kind == "last" else T
    k = min(3, Tc)
    m = max(197, -(-Tc // k) + 70) + (T if kind == "neg" else 0)
    rows = []
    for r in range(m):
        d = np.sort((r * k + np.arange(k)) % Tc)
        if kind == "neg":
            d = -(d + 1)
            d = np.sort(d[r + d >= 0])
        rows.append(r + d)
    if kind == "last":
        rows[-1] = np.array([m - 1 + T - 1])
    op = _from_rows(name, m if kind == "neg" else m + T, rows)
    assert op.info()["diagonals"] == T, (name, op.info()["diagonals"])
    return op


def sliced_op(name, slice_lens, T, tail=0, hole=None, lens_of=None, long_row=None):
    """Slices of 64 rows; slice s has longest row slice_lens[s]: 56 full rows, 4 of half the length, 4 empty (lens_of(s, i) gives
    other shapes); `tail` more rows of the last length; slice `hole` all empty; long_row = (row, length).  A row of length l
    holds l consecutive offsets out of 0 .. T - 1."""
    rows = []
    for s, L in enumerate(list(slice_lens) + ([slice_lens[-1]] if tail else [])):
        for i in range(64 if s < len(slice_lens) else tail):
            if lens_of is not None:
                l = lens_of(s, i)
            else:
                l = L if i % 16 not in (3, 11) else (L // 2 if i % 16 == 3 else 0)
            if hole is not None and s == hole:
                l = 0
            r = len(rows)
            if long_row is not None and r == long_row[0]:
                l = long_row[1]
            start = (r * 7) % (T - l + 1)
            rows.append(r + start + np.arange(l))
    return _from_rows(name, len(rows) + T, rows)


def _pad_ratio(op, mode, cols32):
    lay = sell_layout(op, mode)
    return 512.0 * lay["sum"] / ((12.0 if cols32 else 9.0) * op.nnz + 4.0 * op.m)


def sell32_heads_op(name):
    """Every head-word count of the int32 layouts (modes 1 and 4): 64 slices with one row of 1 .. 64 entries among rows of 4, and
    as many slices of full 8-entry rows as kSellMaxPad needs to admit the copy (ratio 1.19, so that the 64 KiB of slack do not
    decide) at a mean row length <= 8 (256-row blocks): the int32 copy is tried on no longer rows."""
    head = lambda s, i: (s + 1) if i == 5 else min(4, s + 1)                            # noqa: E731
    nnz_head = sum(head(s, i) for s in range(64) for i in range(64))
    filler = 0
    for mode in (1, 4):
        units = sum(_sell_units(s + 1, mode) for s in range(64))
        need = 512.0 * units - (SELL_MAX_PAD - 0.01) * (12.0 * nnz_head + 4.0 * 4096)
        gain = (SELL_MAX_PAD - 0.01) * (12.0 * 512 + 256) - 512.0 * _sell_units(8, mode)
        filler = max(filler, int(math.ceil(need / gain)))
    return sliced_op(name, list(range(1, 65)) + [8] * filler, 70, lens_of=lambda s, i: head(s, i) if s < 64 else 8)


def delta_edges_op(name, bits, rows):
    """The block-delta edges of one width: R rows per block; block 0 (base 0, clamped) holds columns 0, 2^bits - 2 (the last
    code) and 2^bits - 1 (the first escape); block B, the first whose base is >= 2, holds base - 1 (escape), base, base +
    2^bits - 2 and base + 2^bits - 1; block B + 1 has no escape; the last block is partial (R / 2 rows) with more than 256
    escapes.  Every row also holds its band entries r, r + 1."""
    R = min(rows, 64) if bits == 8 else rows
    ESC = (1 << bits) - 1
    H = (ESC - R) // 2
    B = -(-(H + 2) // R)
    m = (B + 2) * R + R // 2
    n = m + ESC + 300
    base = lambda r0: max(r0 - H, 0)                                                    # noqa: E731
    extra = {1: [ESC - 1, ESC], 2: [0]}
    b = base(B * R)
    assert b >= 2
    extra[B * R + 1] = [b - 1, b]
    extra[B * R + 2] = [b + ESC - 1, b + ESC]
    r0 = (B + 2) * R
    per = -(-257 // (R // 2)) + 1
    for r in range(r0, m):
        extra[r] = [base(r0) + ESC + 1 + j for j in range(per)]
    rows_ = [np.unique(np.array([r, r + 1] + extra.get(r, []))) for r in range(m)]
    return _from_rows(name, n, rows_)


def block_op(name, entries):
    """64 rows, row block 32 (mean row length far above 2048 / 64): block 0 has `entries` entries (rows of 2048 consecutive
    columns, the last row shorter), its LAST entry a far column (an escape at position entries - 1); block 1 rows of 4."""
    n = 66000
    rows, left = [], entries
    for r in range(32):
        l = min(2048, left - (31 - r))                 # at least one entry for every later row
        left -= l
        rows.append(r + np.arange(l))
    assert left == 0
    rows[31] = np.concatenate([rows[31][:-1], [n - 10]])
    rows += [r + np.arange(4) for r in range(32, 64)]
    return _from_rows(name, n, rows)


def by_rule_op(name, extra_escapes):
    """nnz = 2^22 + 2 = 9 k entries in rows of 4 (the last of 2), every entry outside the 8-bit window, `2 nnz / 9 + extra` of them
    outside the 16-bit window too: by16 = 2 nnz + 6 esc16 sits exactly on 6 by == 5 by32 (admitted) for extra = 0."""
    m = (1 << 20) + 1
    r = np.arange(m, dtype=np.int64)[:, None]
    up = r + 1900 < m
    c = np.where(up, r + 1000 + 300 * np.arange(4), r - 1000 - 300 * np.arange(4)[::-1])
    nnz = 4 * (m - 1) + 2
    far = 2 * nnz // 9 + extra_escapes
    rf = np.arange(far, dtype=np.int64)
    c[rf, 3] = np.where(rf + 100000 < m, rf + 100000, rf - 100000)
    c[rf] = np.sort(c[rf], axis=1)
    col = c.ravel()[:nnz]
    rowptr = np.minimum(4 * np.arange(m + 1, dtype=np.int64), nnz)
    rng = np.random.default_rng(_seed(name))
    return Op(name, m, m, rowptr, col, _sprinkle(rowptr, col, _values(rng, nnz)))


def template_op(name, m, n, K, T, long_row=None, empty_every=0):
    """Row r is template r % T: K entries at offsets 0 .. K - 1, first value 1 + t / 4096, the rest drawn once per template."""
    rng = np.random.default_rng(_seed(name))
    tv = _values(rng, T * K).reshape(T, K)
    tv[:, 0] = 1.0 + np.arange(T) / 4096.0
    rows, vals = [], []
    for r in range(m):
        if empty_every and r % empty_every == 0:
            rows.append(np.zeros(0, dtype=np.int64)); vals.append(np.zeros(0))
        elif long_row is not None and r == long_row[0]:
            rows.append(r + np.arange(long_row[1])); vals.append(np.full(long_row[1], 0.5))
        else:
            rows.append(r + np.arange(K)); vals.append(tv[r % T])
    return _from_rows(name, n, rows, val=np.concatenate(vals))


def template_bits_op(name, a, b):
    """Rows (1, a, 2) and (1, b, 2) alternating from row 64 on ((1, 3, 2) before): a and b differ only in bits."""
    m = 192
    rows = [r + np.arange(3) for r in range(m)]
    val = np.tile(np.array([1.0, 3.0, 2.0]), m).reshape(m, 3)
    val[64::2, 1], val[65::2, 1] = a, b
    return _from_rows(name, m + 3, rows, val=val.ravel())


def _nan(payload):
    return np.array([0x7FF8000000000000 | payload], dtype=np.uint64).view(np.float64)[0]


def transpose_op(name, m, n, long_col=None, per_row=5):
    """Random unsorted rows; columns 0 .. 9, the middle tenth and the last 10 are referenced by nobody."""
    rng = np.random.default_rng(_seed(name))
    ok = np.ones(n, dtype=bool)
    if n > 64:
        ok[:10] = ok[-10:] = False
        ok[n // 2 - n // 20:n // 2 + n // 20] = False
    allowed = np.flatnonzero(ok)
    rows = []
    for r in range(m):
        c = rng.choice(allowed, size=min(per_row, allowed.size), replace=False) if r % 9 else np.zeros(0, dtype=np.int64)
        if long_col is not None and r < long_col[1]:
            c = np.concatenate([c[c != long_col[0]][:2], [long_col[0]]])
        rows.append(c)
    return _from_rows(name, n, rows)


def repeats_op(name, m, n, subnormal=True):
    """Every row holds one column three times and another twice, interleaved with single ones, each with its own value."""
    rng = np.random.default_rng(_seed(name))
    rows = []
    for r in range(m):
        c = rng.choice(n, size=min(4, n), replace=False)
        rows.append(c[np.array([0, 1, 0, 2, 1, 0, 3]) % c.size] if r % 7 != 3 else c[:0])
    return _from_rows(name, n, rows, subnormal=subnormal)


def band_op(name, m, permute, split, longest=6):
    """Up to `longest` entries per row on the offsets {0, 1, 2, 3, 5, 8, 9} (longest = 12: on 14 offsets, rows beyond the 8 entries
    of the short sliced layouts); permute: every row's entries in a random order; split: every fifth entry stored twice (the
    same row and column, two values)."""
    rng = np.random.default_rng(_seed(name.split("_")[0]))              # the same operator under every variant
    offs = np.array([0, 1, 2, 3, 5, 8, 9] + ([11, 12, 14, 17, 18, 20, 21] if longest > 6 else []))
    rows = []
    for r in range(m):
        d = offs[np.sort(rng.choice(offs.size, size=int(rng.integers(0, longest + 1)), replace=False))]
        c = r + d
        if split:
            c = np.concatenate([c, c[::5][:max(longest + 2 - c.size, 0)]])
        if permute:
            c = c[np.random.default_rng(r + 1).permutation(c.size)]
        rows.append(c)
    return _from_rows(name, m + 22, rows)


def plan_op(name, m, length, one=None, T=None, subnormal=True):
    """m rows of `length` consecutive-offset entries; one = (row, length) replaces one row."""
    T = T or max(length, one[1] if one else 0) + 6
    rows = []
    for r in range(m):
        l = one[1] if (one and r == one[0]) else length
        rows.append(r + (r * 5) % (T - l + 1) + np.arange(l))
    return _from_rows(name, m + T, rows, subnormal=subnormal)


def _pad_op(name, admitted):
    """60 slices whose padding decides: one row of 16 among rows of 13 / 14 (ratio about 1.18 of kSellMaxPad = 1.20: admitted
    without the 64 KiB of slack), or one row of 32 among rows of 8 (ratio far above it: refused with the slack too)."""
    if admitted:
        return sliced_op(name, [16] * 60, 40, lens_of=lambda s, i: 16 if i == 0 else (14 if i <= 4 else 13))
    return sliced_op(name, [32] * 60, 40, lens_of=lambda s, i: 32 if i == 0 else 8)


OPS = {}
for _T in (1, 15, 16, 255, 256, 257, 2048, 2049):
    OPS["diag%d" % _T] = (lambda T=_T: diag_op("diag%d" % T, T))
OPS.update({
    "diag255_last": lambda: diag_op("diag255_last", 255, "last"), "diag256_last": lambda: diag_op("diag256_last", 256, "last"),
    "diag16_neg": lambda: diag_op("diag16_neg", 16, "neg"),
    "ragged64": lambda: sliced_op("ragged64", range(1, 65), 70),
    "ragged8": lambda: sliced_op("ragged8", list(range(1, 9)) * 2, 12, tail=1),
    "uniform9_hole": lambda: sliced_op("uniform9_hole", [9] * 39, 12, tail=63, hole=17, lens_of=lambda s, i: 9),
    "uniform7_hole": lambda: sliced_op("uniform7_hole", [7] * 39, 12, tail=63, hole=17, lens_of=lambda s, i: 7),
    "uniform7_m192": lambda: sliced_op("uniform7_m192", [7] * 3, 12, lens_of=lambda s, i: 7),
    "uniform7_m193": lambda: sliced_op("uniform7_m193", [7] * 3, 12, tail=1, lens_of=lambda s, i: 7),
    "uniform7_m40": lambda: _small_uniform(),
    "row64": lambda: sliced_op("row64", [7] * 4, 70, lens_of=lambda s, i: 7, long_row=(100, 64)),
    "row65": lambda: sliced_op("row65", [7] * 4, 70, lens_of=lambda s, i: 7, long_row=(100, 65)),
    "pad_admitted": lambda: _pad_op("pad_admitted", True), "pad_refused": lambda: _pad_op("pad_refused", False),
    "narrow8": lambda: sliced_op("narrow8", [8] * 3, 12, tail=1, lens_of=lambda s, i: 8),
    "narrow9": lambda: sliced_op("narrow9", [8] * 3, 12, tail=1, lens_of=lambda s, i: 8, long_row=(70, 9)),
    "sell32_heads": lambda: sell32_heads_op("sell32_heads"),
    "block65535": lambda: block_op("block65535", 65535), "block65536": lambda: block_op("block65536", 65536),
    "by_admit": lambda: by_rule_op("by_admit", 0), "by_refuse": lambda: by_rule_op("by_refuse", 1),
    "tmpl1024": lambda: template_op("tmpl1024", 2100, 2102, 2, 1024), "tmpl1025": lambda: template_op("tmpl1025", 2100, 2102, 2, 1025),
    "tmplK32": lambda: template_op("tmplK32", 100, 140, 5, 3, long_row=(50, 32)),
    "tmplK33": lambda: template_op("tmplK33", 100, 140, 5, 3, long_row=(50, 33)),
    "tmpl_bytes_at": lambda: template_op("tmpl_bytes_at", 2000, 2005, 5, 960),
    "tmpl_bytes_over": lambda: template_op("tmpl_bytes_over", 2000, 2005, 5, 961),
    "tmpl_zero_sign": lambda: template_bits_op("tmpl_zero_sign", 0.0, -0.0),
    "tmpl_nan_payload": lambda: template_bits_op("tmpl_nan_payload", _nan(1), _nan(2)),
    "tmpl_empty_rect": lambda: template_op("tmpl_empty_rect", 300, 700, 4, 2, empty_every=3),
    "tmpl_one_row": lambda: template_op("tmpl_one_row", 1, 5, 3, 1),
    "tr_long_col": lambda: transpose_op("tr_long_col", 2100, 4095, long_col=(77, 2000), per_row=3),
    "tr_repeats": lambda: repeats_op("tr_repeats", 200, 300),
    "tr_m1": lambda: repeats_op("tr_m1", 1, 50, subnormal=False), "tr_n1": lambda: repeats_op("tr_n1", 40, 1, subnormal=False),
    "band_perm": lambda: band_op("band_perm", 517, True, False), "band_split": lambda: band_op("band_split", 517, True, True),
    "band_perm12": lambda: band_op("band_perm12", 517, True, False, 12), "band_split12": lambda: band_op("band_split12", 517, True, True, 12),
    "mean12": lambda: plan_op("mean12", 256, 12), "mean12_plus": lambda: plan_op("mean12_plus", 256, 12, one=(9, 13)),
    "mean96": lambda: plan_op("mean96", 128, 96, subnormal=False), "mean96_plus": lambda: plan_op("mean96_plus", 128, 96, one=(9, 97), subnormal=False),
    "max64": lambda: plan_op("max64", 256, 4, one=(77, 64)), "max65": lambda: plan_op("max65", 256, 4, one=(77, 65)),
    "mean8": lambda: plan_op("mean8", 512, 8), "mean8_plus": lambda: plan_op("mean8_plus", 512, 8, one=(9, 9)),
})
for _n1 in (2047, 2048, 2049, 4096, 4097, 3 * 2048 + 1):
    OPS["tr_scan%d" % _n1] = (lambda n1=_n1: transpose_op("tr_scan%d" % n1, 300, n1 - 1))
for _bits in (8, 16):
    for _rows in (32, 64, 256):
        OPS["delta%d_r%d" % (_bits, _rows)] = (lambda b=_bits, r=_rows: delta_edges_op("delta%d_r%d" % (b, r), b, r))


def _small_uniform():
    rows = [r + (r * 7) % 6 + np.arange(7) for r in range(40)]
    return _from_rows("uniform7_m40", 40 + 12, rows)


_OP_CACHE = {}


def get_op(name):
    if name not in _OP_CACHE:
        _OP_CACHE[name] = OPS[name]()
    return _OP_CACHE[name]


# ---------------------------------------------------------------------------------------------------- stored-order arithmetic

def stored_sum(rowptr, prod):
    """acc = 0; acc = acc + prod[q] for the entries of a row in stored order, all rows at once."""
    lens = np.diff(rowptr)
    acc = np.zeros(lens.size)
    live = np.flatnonzero(lens > 0)
    with np.errstate(all="ignore"):
        for k in range(int(lens.max()) if lens.size else 0):
            live = live[lens[live] > k]
            acc[live] = acc[live] + prod[rowptr[live] + k]
    return acc


def stored_product(rowptr, col, val, x):
    with np.errstate(all="ignore"):
        return stored_sum(rowptr, val * x[col])


# ---------------------------------------------------------------------------------------------------- dictionary codes

def encode_codes(op, opts):
    """csr_build_codes: (table, codes, bits) or (None, reason)."""
    if op.m == 0 or op.nnz == 0:
        return None, "m == 0 || nnz == 0"
    d = op.col.astype(np.int64) - op.row_of
    tab = np.unique(d)
    if tab.size > CODE_MAX:
        return None, "h[0] > kCodeMax: too many diagonals, stays on the int32 stream"
    bits = 8 if (tab.size <= 256 and opts["spmv_codes"] != 16) else 16
    return dict(tab=tab, code=np.searchsorted(tab, d).astype(np.uint8 if bits == 8 else np.uint16), bits=bits, T=int(tab.size)), ""


def decode_codes(op, enc, x, fault=None):
    """spmv_code_kernel: col = row + tab[code]."""
    c = enc["code"].astype(np.int64)
    if fault == "code16_truncated_to_8" and enc["bits"] == 16:
        c = c & 0xFF
    col = op.row_of + enc["tab"][c]
    return stored_product(op.rowptr, np.clip(col, 0, op.n - 1), op.val, x)


# ---------------------------------------------------------------------------------------------------- the sliced copy

def head_words(T, mode):
    """sell_head_words, on an array of unit counts."""
    T = np.asarray(T, dtype=np.int64)
    if mode == 5:
        W = np.where(T <= 18, 2, np.where(T <= 36, 4, np.where(T <= 54, 6, 8)))
    elif mode == 4:
        W = 2 * ((T - 4) // 6) + 2
    elif mode == 3:
        W = np.ones_like(T)
    elif mode == 2:
        W = np.zeros_like(T)
    elif mode == 1:
        W = (T + 2) // 3
    else:
        W = (T + 8) // 9
    return np.where(T <= 0, 0, W)


def sell_mode(info, opts, cols32, code_T=0):
    """build_sell_form's mode and whether it is the narrow one."""
    narrow = (not cols32) and bool(opts["spmv_sell_narrow"]) and code_T <= NARROW_MAX_T and info["max_row"] <= NARROW_MAX_ROW
    pair = (not narrow) and bool(opts["spmv_sell_pair"])
    if cols32:
        return (4 if (pair and opts["spmv_sell_pair"] >= 2) else 1), False
    return (2 if narrow else ((3 if info["max_row"] <= 8 else 5) if pair else 0)), narrow


def sell_layout(op, mode):
    """Units per slice (sell_units_kernel through partition_model._sell_units), the uniform rule and the total."""
    S = (op.m + 63) // 64
    lens = np.zeros(S * 64, dtype=np.int64)
    lens[:op.m] = op.lens
    Ls = lens.reshape(S, 64).max(axis=1)
    units = np.array([_sell_units(int(L), mode) for L in Ls], dtype=np.int64)
    total, umax = int(units.sum()), int(units.max()) if S else 0
    uniform = umax * S <= SELL_UNIFORM_PAD * total + 8.0
    return dict(S=S, Ls=Ls, units=units, sum=total, umax=umax, uniform=bool(uniform), total=umax * S if uniform else total, mode=mode)


def encode_sell(op, lay, code=None):
    """sell_fill_kernel: the 64-bit words of the sliced copy (+ the narrow code words)."""
    mode, S = lay["mode"], lay["S"]
    cols32, pair = mode in (1, 4), mode >= 3
    rows = np.arange(S * 64, dtype=np.int64)
    s, lane = rows >> 6, rows & 63
    off = np.concatenate([[0], np.cumsum(lay["units"])])
    o0 = s * lay["umax"] if lay["uniform"] else off[s]
    T = np.full(rows.size, lay["umax"]) if lay["uniform"] else lay["units"][s]
    W = head_words(T, mode)
    L = T - W
    inside = rows < op.m
    q0 = np.where(inside, op.rowptr[np.minimum(rows, op.m - 1)], 0)
    ln = np.where(inside, op.lens[np.minimum(rows, op.m - 1)], 0)
    words = np.zeros(64 * (lay["total"] + 1), dtype=np.uint64)
    last = max(op.nnz - 1, 0)

    def slot(w):
        return o0 * 64 + (((w >> 1) * 64 + lane) * 2 + (w & 1) if pair else w * 64 + lane)
    for w in range(int(W.max()) if rows.size else 0):
        sel = W > w
        word = np.zeros(rows.size, dtype=np.uint64)
        if cols32:
            for h in (0, 1):
                k = 2 * w + h
                c = np.where(k < ln, op.col[np.minimum(q0 + k, last)].astype(np.int64) & MARK32, MARK32).astype(np.uint64)
                word |= c << np.uint64(32 * h)
        else:
            for u in range(8):
                k = 8 * w + u
                c = np.where(k < ln, code[np.minimum(q0 + k, last)].astype(np.int64), MARK8).astype(np.uint64)
                word |= c << np.uint64(8 * u)
        words[slot(np.full(rows.size, w))[sel]] = word[sel]
    vbits = op.val.view(np.uint64)
    for k in range(int(L.max()) if rows.size else 0):
        sel = L > k
        v = np.where(k < ln, vbits[np.minimum(q0 + k, last)], np.uint64(0))
        words[slot(W + k)[sel]] = v[sel]
    c4 = None
    if mode == 2:
        c4 = np.zeros(rows.size, dtype=np.uint32)
        for u in range(8):
            c = np.where(u < ln, code[np.minimum(q0 + u, last)].astype(np.int64), MARK4).astype(np.uint32)
            c4 |= c << np.uint32(4 * u)
    return dict(words=words, c4=c4, off=off, lay=lay)


def decode_sell(op, enc, x, tab=None, fault=None):
    """spmv_sell_kernel: lane l of slice s reads its head words (eight codes, or two columns, per word; the "no entry" marks
    switch an entry off), then its value words, in stored order."""
    lay = enc["lay"]
    mode = lay["mode"]
    cols32, pair = mode in (1, 4), mode >= 3
    rows = np.arange(op.m, dtype=np.int64)
    s, lane = rows >> 6, rows & 63
    uniform = lay["uniform"] or fault == "uniform_units_on_offset_layout"
    o0 = s * lay["umax"] if uniform else enc["off"][s]
    T = np.full(op.m, lay["umax"]) if uniform else lay["units"][s]
    W = head_words(T, mode)
    if fault == "mode5_head_words_off_in_one_range" and mode == 5:
        W = np.where(T <= 0, 0, np.where(T <= 18, 2, np.where(T <= 34, 4, np.where(T <= 54, 6, 8))))
    L = T - W
    words = enc["words"]
    stab = np.zeros(256, dtype=np.int64)
    if tab is not None:
        stab[:tab.size] = tab

    def load(w):
        idx = o0 * 64 + (((w >> 1) * 64 + lane) * 2 + (w & 1) if pair else w * 64 + lane)
        return words[np.clip(idx, 0, words.size - 1)]
    acc = np.zeros(op.m)
    steps = 8 if mode in (2, 3) else (int(L.max()) if op.m else 0)
    with np.errstate(all="ignore"):
        for k in range(steps):
            live = (T > 0) if mode in (2, 3) else (L > k)                 # modes 2 / 3: one step of eight entries for a row with units
            if mode == 2:
                c = (enc["c4"][:op.m].astype(np.int64) >> (4 * k)) & MARK4
                on = (c != MARK4) | (fault == "sentinel_f_read_as_entry")
                col = rows + stab[c]
            elif cols32:
                cw = load(np.full(op.m, k // 2))
                c = ((cw >> np.uint64(32 * (k & 1))) & np.uint64(MARK32)).astype(np.int64)
                on = c != MARK32
                col = c
            else:
                cw = load(np.full(op.m, 0 if mode == 3 else k // 8))
                c = ((cw >> np.uint64(8 * (k % 8))) & np.uint64(MARK8)).astype(np.int64)
                on = (c != MARK8) | (fault == "sentinel_ff_read_as_entry")
                col = rows + stab[c]
            wv = W + k
            if fault == "pair_value_word_swapped" and pair:
                wv = wv ^ 1
            v = load(wv).view(np.float64)
            if mode == 3:
                v = np.where(2 * ((1 + k) // 2) < T, v, 0.0)             # el[e] is loaded only for 2 e < T
            if mode == 2:
                v = np.where(k < L, v, 0.0)                              # vv[u] = (u < left) ? load : 0.0
            use = live & on
            acc[use] = acc[use] + v[use] * x[np.clip(col[use], 0, op.n - 1)]
    return acc


# ---------------------------------------------------------------------------------------------------- the block-delta stream

def delta_base(r0, rows, bits):
    H = ((1 << bits) - 1 - rows) // 2
    return np.maximum(r0 - max(H, 0), 0)


def stream_rows(info, opts):
    """The row block of the stream kernel (spmv_plan)."""
    rows = opts["spmv_rows"]
    if rows * info["mean_row"] > PLAN_WINDOW:
        rows = 256
        while rows > 32 and rows * info["mean_row"] > PLAN_WINDOW:
            rows >>= 1
    return rows if rows in pm.ROW_BLOCKS else 256


def _escapes(op, R, bits, fault=None):
    r0 = (op.row_of // R) * R
    base = delta_base(r0, R, bits)
    rel = op.col.astype(np.int64) - base
    ESC = (1 << bits) - 1
    below = rel < 0
    if fault == "delta_escape_bound_off_by_one":
        return base, rel, below | (rel > ESC)
    if fault == "delta_below_base_not_escaped":
        return base, rel, rel >= ESC
    return base, rel, below | (rel >= ESC)


def delta_model(op, opts, rows):
    """spmv_plan's gate and csr_build_delta's rules: dict(state, bits, rows, esc, reason); state 0 = not tried."""
    dl = opts["spmv_delta"]
    wide_ok = opts["spmv_nt"] == 0 and opts["spmv_vec"] != 2 and opts["spmv_persist"] == 0 and op.nnz > 0
    if not (wide_ok and dl and (dl != 1 or op.nnz >= BIG_NNZ)):
        return dict(state=0, bits=32, rows=0, esc=0, reason="not tried: spmv_delta = 0, or 1 on fewer than 2^22 entries")
    no = lambda why: dict(state=-1, bits=32, rows=0, esc=0, reason=why)                  # noqa: E731
    if op.m == 0 or op.nnz == 0 or rows < 32 or rows > 256:
        return no("m == 0 || nnz == 0 || rows < 32 || rows > 256")
    rows16, rows8 = rows, min(rows, 64)
    for R in (rows8, rows16):
        starts = np.arange(0, op.m, R)
        if int((op.rowptr[np.minimum(starts + R, op.m)] - op.rowptr[starts]).max()) > DELTA_BLOCK_MAX:
            return no("rowptr[hi] - rowptr[row] > 65535: a block's entries must be addressable by 16 bits (esc_pos)")
    esc8, esc16 = int(_escapes(op, rows8, 8)[2].sum()), int(_escapes(op, rows16, 16)[2].sum())
    by8, by16, by32 = op.nnz + 6 * esc8, 2 * op.nnz + 6 * esc16, 4 * op.nnz
    bits = 8 if by8 <= by16 else 16
    if dl in (8, 16):
        bits = dl
    by, esc = (by8, esc8) if bits == 8 else (by16, esc16)
    if dl < 2 and 6 * by > 5 * by32:
        return no("spmv_delta < 2 && 6 * by > 5 * by32: saves less than a sixth, stays on int32")
    return dict(state=1, bits=bits, rows=rows8 if bits == 8 else rows16, esc=esc, reason="", by=by, by32=by32)


def encode_delta(op, R, bits, fault=None):
    """delta_assign_kernel: codes, the base of every block, the escape lists (position in the block as 16 bits, column)."""
    base, rel, esc = _escapes(op, R, bits, fault)
    ESC = (1 << bits) - 1
    code = np.where(esc, ESC, rel & ESC)
    if fault == "delta_escape_bound_off_by_one":
        code = np.where(rel == ESC, ESC, code)                           # the column at base + 2^bits - 1 gets the all-ones code, and no list entry
    q = np.flatnonzero(esc)
    blk = op.row_of[q] // R
    pos = (q - op.rowptr[blk * R]) & 0xFFFF
    return dict(code=code, base=base, R=R, bits=bits, esc_blk=blk, esc_pos=pos, esc_col=op.col[q].astype(np.int64), esc=int(q.size))


def decode_delta(op, enc, x):
    """spmv_delta_kernel: col = base + code; an all-ones code contributes val * 0.0 until the block's list patches it."""
    ESC = (1 << enc["bits"]) - 1
    on = enc["code"] != ESC
    col = np.clip(enc["base"] + enc["code"], 0, op.n - 1)
    with np.errstate(all="ignore"):
        prod = op.val * np.where(on, x[col], 0.0)
        q = op.rowptr[enc["esc_blk"] * enc["R"]] + enc["esc_pos"]
        prod[q] = op.val[q] * x[enc["esc_col"]]
    return stored_sum(op.rowptr, prod)


# ---------------------------------------------------------------------------------------------------- row templates

def template_model(op, fault=None):
    """khip_csr_compress: rows are compared by the BITS of their values; ids in order of the first row of every template."""
    K = int(op.lens.max()) if op.m else 0
    if op.m == 0 or K > TMPL_MAX_LEN or K < 1:
        return dict(T=0, reason="m == 0 || max_row_nnz > kTmplMaxLen || max_row_nnz < 1")
    d = (op.col.astype(np.int64) - op.row_of).astype(np.int32)
    val = op.val
    if fault == "template_match_by_value":
        if np.isnan(val).any():
            return dict(T=0, reason="(fault) NaN != NaN: a row never matches its own template")
        val = np.where(val == 0.0, 0.0, val)
    ids, reps, seen = np.zeros(op.m, dtype=np.int64), [], {}
    for r in range(op.m):
        a, b = op.rowptr[r], op.rowptr[r + 1]
        key = (d[a:b].tobytes(), val[a:b].tobytes())
        if key not in seen:
            seen[key] = len(reps)
            reps.append(r)
        ids[r] = seen[key]
    T = len(reps)
    if T > TMPL_MAX:
        return dict(T=0, reason="T > kTmplMax")
    if T * K * 12 + T * 4 > TMPL_LDS_MAX:
        return dict(T=0, reason="T * K * 12 + T * 4 > kTmplLdsMax")
    t_off, t_val, t_cnt = np.zeros((T, K), dtype=np.int64), np.zeros((T, K)), np.zeros(T, dtype=np.int64)
    for t, r in enumerate(reps):
        a, b = op.rowptr[r], op.rowptr[r + 1]
        t_cnt[t] = b - a
        t_off[t, :b - a], t_val[t, :b - a] = d[a:b], op.val[a:b]
    return dict(T=T, K=K, ids=ids.astype(np.uint16), t_off=t_off, t_val=t_val, t_cnt=t_cnt, reason="")


def decode_template(op, tm, x, fault=None):
    """spmv_template_kernel: row r walks template ids[r]: col = r + t_off, in stored order."""
    ids = tm["ids"].astype(np.int64)
    if fault == "template_id_byte_truncated":
        ids = ids & 0xFF
    rows = np.arange(op.m)
    acc = np.zeros(op.m)
    with np.errstate(all="ignore"):
        for k in range(tm["K"]):
            on = tm["t_cnt"][ids] > k
            r = rows[on]
            acc[r] = acc[r] + tm["t_val"][ids[r], k] * x[np.clip(r + tm["t_off"][ids[r], k], 0, op.n - 1)]
    return acc


# ---------------------------------------------------------------------------------------------------- the adjoint handle

def scan_tiles(counts, fault=None):
    """exclusive_scan_i32: per-tile sums, the serial scan of the tile sums, the tile's offset added back."""
    cnt = counts.size
    ntiles = -(-cnt // SCAN_TILE)
    out = np.zeros(cnt, dtype=np.int64)
    run = 0
    for t in range(ntiles):
        tile = counts[t * SCAN_TILE:(t + 1) * SCAN_TILE]
        off = 0 if (fault == "scan_tile_offset_dropped" and t == 1) else run
        out[t * SCAN_TILE:t * SCAN_TILE + tile.size] = off + np.concatenate([[0], np.cumsum(tile)[:-1]])
        run += int(tile.sum())
    return out


def transpose_model(op, fault=None):
    """csr_transpose: column histogram, exclusive scan over n + 1 counts, scatter, stable sort of every row of A' by its column
    (= row of A): the stable column-major order of A.  Returns (rowptr, col, val) of A'."""
    counts = np.concatenate([np.bincount(op.col, minlength=op.n), [0]]).astype(np.int64)
    rowptr = scan_tiles(counts, fault)
    order = np.argsort(op.col, kind="stable")
    if fault == "transpose_unstable_among_repeats":
        key = op.col[order].astype(np.int64) * op.m + op.row_of[order]
        same = np.concatenate([[False], key[1:] == key[:-1]])
        first = np.flatnonzero(~same)
        for a, b in zip(first, np.concatenate([first[1:], [key.size]])):
            order[a:b] = order[a:b][::-1]
    return rowptr, op.row_of[order].astype(np.int32), op.val[order].copy()


def transpose_reference(op):
    """The rows of A' as the stable column-major order of A, by a lexicographic sort on (column, row, stored position)."""
    order = np.lexsort((np.arange(op.nnz), op.row_of, op.col))
    rowptr = np.zeros(op.n + 1, dtype=np.int64)
    np.cumsum(np.bincount(op.col, minlength=op.n), out=rowptr[1:])
    return rowptr, op.row_of[order].astype(np.int32), op.val[order].copy()


def transposed_op(op):
    rp, cl, vl = transpose_reference(op)
    return Op(op.name + "'", op.n, op.m, rp, cl, vl, op.subnormal)


# ---------------------------------------------------------------------------------------------------- the expected form

BASE = dict(pm.BASE)
OPTION_KEYS = tuple(BASE)
FIELDS = ("kernel", "form", "code", "sell", "narrow", "sell32", "delta", "templates", "bytes")


def form_name(f, opts):
    """The SpmvForm behind the fields a handle reports (tests/test_gpu_partitioned_spmv_exact.py ran_form)."""
    k = f["kernel"]
    if k in (5, 6, 3, 2):
        return {5: "Template", 6: "Wave", 3: "Ordered", 2: "Vector"}[k]
    if k == 1:
        if f["delta"][0] in (8, 16):
            return "StreamDelta%d" % f["delta"][0]
        return "StreamWide" if (opts["spmv_wide"] and opts["spmv_vec"] != 2) else "Stream"
    if f["code"][0] in (8, 16) and opts["spmv_codes"]:
        if opts["spmv_sell"] and f["sell"][0] == 1:
            return "SlicedNarrow" if f["narrow"] else "Sliced"
        return "Coded%d" % f["code"][0]
    return "Sliced32" if (opts["spmv_sell"] and f["sell32"][0] == 1) else "Staged"


def expected(op, opts, compress=False, fault=None):
    """Every field a handle reports after its first product under `opts` (after khip_csr_compress where compress), from the
    builders' rules; `why` holds the reason of every form that is not built, quoted from the builder."""
    info = op.info()
    why = {}
    tm = template_model(op, fault) if compress else dict(T=0, reason="khip_csr_compress not called")
    if compress and not tm["T"]:
        why["template"] = tm["reason"]
    tmpl = bool(tm["T"]) and bool(opts["spmv_template"])
    p = predict(info, dict(opts, spmv_delta=0), compressed=bool(tm["T"]))
    kernel = p["kernel"]
    nt = opts["spmv_nt"] != 0
    codes = opts["spmv_codes"]
    try_codes = bool(codes) and (codes != 1 or info["nnz"] >= BIG_NNZ) and not nt
    code = (32, 0)
    enc = None
    if try_codes and not tmpl and (opts["spmv_kernel"] == 4 or (opts["spmv_kernel"] == 0 and info["max_row"] <= CODED_MAX_ROW)):
        enc, reason = encode_codes(op, opts)
        if enc is None:
            why["codes"] = reason
        else:
            code = (enc["bits"], enc["T"])
    out = dict(kernel=kernel, code=code, sell=(0, 0, 0), narrow=False, sell32=(0, 0, 0), delta=(32, 0, 0), templates=tm["T"], why=why,
               codes_enc=enc, template=tm if tm["T"] else None, rows=p["rows"])
    m, n, nnz = op.m, op.n, op.nnz
    tail = 4 * (m + 1) + 8 * n + 8 * m
    by = 12 * nnz + tail
    if kernel == 5:
        by = 2 * m + 8 * n + 8 * m
    elif kernel == 1:
        rows = stream_rows(info, opts)
        dm = delta_model(op, opts, rows)
        out["rows"] = rows
        if dm["state"] == 1:
            out["delta"] = (dm["bits"], dm["rows"], dm["esc"])
            by = (8 + dm["bits"] // 8) * nnz + 6 * dm["esc"] + 8 * (-(-m // dm["rows"])) + tail
        elif opts["spmv_delta"]:
            why["delta"] = dm["reason"]
        out["delta_model"] = dm
    elif kernel == 4:
        coded = try_codes and enc is not None
        sliced = False
        if coded and opts["spmv_sell"] and enc["bits"] == 8:
            mode, narrow = sell_mode(info, opts, False, enc["T"])
            built = _sell_builds(info, opts, False, enc["T"])[0]
            if built:
                lay = sell_layout(op, mode)
                assert 512.0 * lay["sum"] <= SELL_MAX_PAD * (9.0 * nnz + 4.0 * m) + SELL_SLACK
                out["sell"], out["narrow"], out["sell_layout"], sliced = (1, lay["umax"] if lay["uniform"] else 0, lay["total"]), narrow, lay, True
                by = 512 * lay["total"] + (0 if lay["uniform"] else 4 * (lay["S"] + 1)) + (256 * lay["S"] if narrow else 0) + 8 * n + 8 * m
            else:
                out["sell"] = (-1, 0, 0)
                why["sell"] = ("max_row_nnz > 64" if info["max_row"] > SELL_MAX_ROW else
                               ("code_T > 255: 0xFF means no entry" if enc["T"] > SELL_MAX_T else "512 * total > kSellMaxPad * ref_bytes + 65536"))
        elif coded and opts["spmv_sell"]:
            why["sell"] = "code_bits != 8: csr_build_sell takes 8-bit codes only"
        if not sliced:
            rows = opts["spmv_rows"] if opts["spmv_rows"] in pm.ROW_BLOCKS else 256
            while rows > 32 and rows * info["mean_row"] > PLAN_WINDOW:
                rows >>= 1
            out["rows"] = rows
            try32 = (not coded) and bool(opts["spmv_sell"]) and not nt and rows == 256 and (codes == 2 or opts["spmv_sell"] >= 3 or info["nnz"] >= BIG_NNZ)
            if coded:
                by = (8 + enc["bits"] // 8) * nnz + tail
            elif try32:
                mode, _ = sell_mode(info, opts, True)
                if _sell_builds(info, opts, True)[0]:
                    lay = sell_layout(op, mode)
                    out["sell32"], out["sell32_layout"] = (1, lay["umax"] if lay["uniform"] else 0, lay["total"]), lay
                    by = 512 * lay["total"] + (0 if lay["uniform"] else 4 * (lay["S"] + 1)) + 8 * n + 8 * m
                else:
                    out["sell32"] = (-1, 0, 0)
                    why["sell32"] = "max_row_nnz > 64" if info["max_row"] > SELL_MAX_ROW else "512 * total > kSellMaxPad * ref_bytes + 65536"
            elif not coded and opts["spmv_sell"]:
                why["sell32"] = "rows == 256 fails, or neither spmv_codes == 2 nor spmv_sell >= 3 nor 2^22 entries: not tried"
    out["bytes"] = by
    out["form"] = form_name(out, opts)
    if kernel != 1:                       # partition_model.predict restates the same plan: the two must agree
        assert out["form"] == p["form"], (op.name, out["form"], p["form"])
    return out


# ---------------------------------------------------------------------------------------------------- the table

@dataclass
class Case:
    name: str
    group: str                      # codes | sliced | delta | template | transpose | unsorted | plan
    op: str
    opts: dict
    want: dict                      # the fields this case is there for (a subset of what `expected` derives)
    edge: str                       # the edge it sits on, and the side
    compress: bool = False
    transpose: bool = False
    want_t: str = ""                # transpose cases: the form A' is meant to run in ...
    want_tt: str = ""               # ... and (A')'
    unavailable: dict = field(default_factory=dict)      # form -> reason quoted from the builder's rule, where the purpose is a refusal

    @property
    def options(self):
        return dict(BASE, **self.opts)


_K4 = dict(spmv_kernel=4)
_CODED = dict(spmv_kernel=4, spmv_sell=0)
_PLAIN = dict(spmv_kernel=4, spmv_sell_pair=0)                                   # mode 0
_NARROW = dict(spmv_kernel=4, spmv_sell_narrow=1)                                # mode 2 where T <= 15 and rows <= 8
_S32 = dict(spmv_kernel=4, spmv_codes=0, spmv_sell=3)                            # mode 1
_S32P = dict(spmv_kernel=4, spmv_codes=0, spmv_sell=3, spmv_sell_pair=2)         # mode 4
_R_255 = "A->code_T > 255: 0xFF means no entry"
_R_16 = "code_bits != 8: csr_build_sell takes 8-bit codes only"
_R_MAX = "T > kCodeMax: stays on the int32 stream"
_R_64 = "A->max_row_nnz > 64"
_R_PAD = "512.0 * total > kSellMaxPad * ref_bytes + 65536.0"
_R_BLOCK = "rowptr[hi] - rowptr[row] > 65535: delta_state = -1"
_R_BY = "spmv_delta < 2 && 6 * by > 5 * by32"
_R_K = "max_row_nnz > kTmplMaxLen"
_R_T = "T > kTmplMax"
_R_LDS = "T * K * 12 + T * 4 > kTmplLdsMax"

CASES = []


def _c(*a, **kw):
    CASES.append(Case(*a, **kw))


# --- dictionary codes
for _T, _bits in ((1, 8), (15, 8), (16, 8), (255, 8)):
    _c("codes_T%d_sliced" % _T, "codes", "diag%d" % _T, _K4, dict(form="Sliced", code=(8, _T)), "T = %d: 8-bit codes, sliced" % _T)
    _c("codes_T%d_coded" % _T, "codes", "diag%d" % _T, _CODED, dict(form="Coded8", code=(8, _T)), "T = %d: 8-bit codes, CSR stream" % _T)
_c("codes_T15_narrow", "codes", "diag15", _NARROW, dict(form="SlicedNarrow", code=(8, 15), narrow=True), "T = 15 | 16: 0xF is free to mean no entry")
_c("codes_T16_narrow", "codes", "diag16", _NARROW, dict(form="Sliced", code=(8, 16), narrow=False), "T = 15 | 16: the 16th code would be 0xF")
_c("codes_T256", "codes", "diag256", _K4, dict(form="Coded8", code=(8, 256), sell=(-1, 0, 0)), "T = 255 | 256: the sliced form stops, 8-bit codes go on",
   unavailable={"sliced": _R_255})
_c("codes_T256_forced16", "codes", "diag256", dict(_K4, spmv_codes=16), dict(form="Coded16", code=(16, 256)), "spmv_codes = 16 at T = 256",
   unavailable={"sliced": _R_16})
_c("codes_T257", "codes", "diag257", _K4, dict(form="Coded16", code=(16, 257), sell=(0, 0, 0)), "T = 256 | 257: 16-bit codes", unavailable={"sliced": _R_16})
_c("codes_T2048", "codes", "diag2048", _K4, dict(form="Coded16", code=(16, 2048)), "T = 2048 | 2049: kCodeMax admits", unavailable={"sliced": _R_16})
_c("codes_T2049", "codes", "diag2049", _K4, dict(form="Sliced32", code=(32, 0)), "T = 2048 | 2049: kCodeMax refuses", unavailable={"coded": _R_MAX})
_c("codes_T2049_staged", "codes", "diag2049", dict(_K4, spmv_sell=0), dict(form="Staged", code=(32, 0)), "T = 2049 on the int32 CSR stream",
   unavailable={"coded": _R_MAX})
_c("codes_T255_last", "codes", "diag255_last", _K4, dict(form="Sliced", code=(8, 255)), "the largest code (254) only in the last row")
_c("codes_T256_last", "codes", "diag256_last", _K4, dict(form="Coded8", code=(8, 256)), "the largest code (255 = 0xFF) only in the last row",
   unavailable={"sliced": _R_255})
_c("codes_T256_last_kernel0", "codes", "diag256_last", {}, dict(form="Coded8", kernel=4, code=(8, 256)), "the same under spmv_kernel = 0",
   unavailable={"sliced": _R_255})
_c("codes_neg_sliced", "codes", "diag16_neg", _K4, dict(form="Sliced", code=(8, 16)), "negative offsets only")
_c("codes_neg_coded16", "codes", "diag16_neg", dict(_CODED, spmv_codes=16), dict(form="Coded16", code=(16, 16)), "negative offsets only, two-byte codes")
# --- sliced layouts
_c("sliced_ragged64_m0", "sliced", "ragged64", _PLAIN, dict(form="Sliced"), "L = 1 .. 64 per slice, mode 0, offsets")
_c("sliced_ragged64_m5", "sliced", "ragged64", _K4, dict(form="Sliced"), "L = 1 .. 64 per slice, mode 5, offsets")
_c("sliced_ragged8_m3", "sliced", "ragged8", _K4, dict(form="Sliced"), "L = 1 .. 8 per slice, mode 3, offsets, m % 64 = 1")
_c("sliced_ragged8_m0", "sliced", "ragged8", _PLAIN, dict(form="Sliced"), "L = 1 .. 8 per slice, mode 0")
_c("sliced_ragged8_m2", "sliced", "ragged8", _NARROW, dict(form="SlicedNarrow", narrow=True), "L = 1 .. 8 per slice, mode 2, offsets")
_c("sliced_ragged8_m1", "sliced", "ragged8", _S32, dict(form="Sliced32"), "L = 1 .. 8 per slice, mode 1, offsets")
_c("sliced_ragged8_m4", "sliced", "ragged8", _S32P, dict(form="Sliced32"), "L = 1 .. 8 per slice, mode 4, offsets")
_c("sliced_hole9_m0", "sliced", "uniform9_hole", _PLAIN, dict(form="Sliced"), "an all-empty slice inside a uniform layout, mode 0, m % 64 = 63")
_c("sliced_hole9_m5", "sliced", "uniform9_hole", _K4, dict(form="Sliced"), "an all-empty slice inside a uniform layout, mode 5")
_c("sliced_hole7_m3", "sliced", "uniform7_hole", _K4, dict(form="Sliced"), "an all-empty slice inside a uniform layout, mode 3")
_c("sliced_hole7_m2", "sliced", "uniform7_hole", _NARROW, dict(form="SlicedNarrow", narrow=True), "an all-empty slice inside a uniform layout, mode 2")
_c("sliced_hole7_m1", "sliced", "uniform7_hole", _S32, dict(form="Sliced32"), "an all-empty slice inside a uniform layout, mode 1")
_c("sliced_hole7_m4", "sliced", "uniform7_hole", _S32P, dict(form="Sliced32"), "an all-empty slice inside a uniform layout, mode 4")
for _m in (192, 193, 40):
    _c("sliced_m%d" % _m, "sliced", "uniform7_m%d" % _m, _K4, dict(form="Sliced"), "m = %d: m %% 64 = %d%s" % (_m, _m % 64, ", m < 64" if _m < 64 else ""))
_c("sliced_m40_m4", "sliced", "uniform7_m40", _S32P, dict(form="Sliced32"), "m < 64, mode 4")
_c("sliced_row64", "sliced", "row64", _K4, dict(form="Sliced", sell=None), "longest row 64 | 65: admitted")
_c("sliced_row65", "sliced", "row65", _K4, dict(form="Coded8", sell=(-1, 0, 0)), "longest row 64 | 65: refused", unavailable={"sliced": _R_64})
_c("sliced_row65_m1", "sliced", "row65", _S32, dict(form="Staged", sell32=(-1, 0, 0)), "longest row 65: the int32 copy refused too", unavailable={"sliced32": _R_64})
_c("sliced_pad_admitted", "sliced", "pad_admitted", _K4, dict(form="Sliced"), "kSellMaxPad just admits (ratio about 1.18, without the slack)")
_c("sliced_pad_refused", "sliced", "pad_refused", _K4, dict(form="Coded8", sell=(-1, 0, 0)), "kSellMaxPad refuses (with the slack too)", unavailable={"sliced": _R_PAD})
_c("sliced_narrow8", "sliced", "narrow8", _NARROW, dict(form="SlicedNarrow", narrow=True), "narrow codes at max_row_nnz 8 | 9: narrow")
_c("sliced_narrow9", "sliced", "narrow9", _NARROW, dict(form="Sliced", narrow=False), "narrow codes at max_row_nnz 8 | 9: byte codes, mode 5")
_c("sliced_heads_m1", "sliced", "sell32_heads", _S32, dict(form="Sliced32"), "every head-word count of mode 1")
_c("sliced_heads_m4", "sliced", "sell32_heads", _S32P, dict(form="Sliced32"), "every head-word count of mode 4")
# --- the delta stream
for _bits in (8, 16):
    for _rows in (32, 64, 256):
        _R = min(_rows, 64) if _bits == 8 else _rows
        _c("delta%d_rows%d" % (_bits, _rows), "delta", "delta%d_r%d" % (_bits, _rows), dict(spmv_kernel=1, spmv_delta=_bits, spmv_rows=_rows),
           dict(form="StreamDelta%d" % _bits, delta=(_bits, _R, None)), "base - 1 | base | base + 2^%d - 2 | base + 2^%d - 1 in blocks of %d rows" % (_bits, _bits, _R))
_c("delta_block65535_16", "delta", "block65535", dict(spmv_kernel=1, spmv_delta=16), dict(form="StreamDelta16", delta=(16, 32, 1)),
   "a 65535-entry block with an escape at position 65534")
_c("delta_block65535_8", "delta", "block65535", dict(spmv_kernel=1, spmv_delta=8), dict(form="StreamDelta8"), "the same block, 8 bits: 57 thousand escapes")
for _dl in (16, 8, 2):
    _c("delta_block65536_%d" % _dl, "delta", "block65536", dict(spmv_kernel=1, spmv_delta=_dl), dict(form="Stream", delta=(32, 0, 0)),
       "a 65536-entry block: delta_state = -1, y from the plain stream", unavailable={"delta": _R_BLOCK})
_c("delta_block65536_wide", "delta", "block65536", dict(spmv_kernel=1, spmv_delta=16, spmv_wide=1), dict(form="StreamWide", delta=(32, 0, 0)),
   "the same on the 16-byte-load form of the int32 columns", unavailable={"delta": _R_BLOCK})
_c("delta_by_admit_1", "delta", "by_admit", dict(spmv_kernel=1, spmv_delta=1), dict(form="StreamDelta16", delta=(16, 256, None)), "6 by == 5 by32 under spmv_delta = 1: built")
_c("delta_by_refuse_1", "delta", "by_refuse", dict(spmv_kernel=1, spmv_delta=1), dict(form="Stream", delta=(32, 0, 0)), "6 by > 5 by32 by one escape under spmv_delta = 1",
   unavailable={"delta": _R_BY})
_c("delta_by_admit_2", "delta", "by_admit", dict(spmv_kernel=1, spmv_delta=2), dict(form="StreamDelta16", delta=(16, 256, None)), "the same operator under spmv_delta = 2")
_c("delta_by_refuse_2", "delta", "by_refuse", dict(spmv_kernel=1, spmv_delta=2), dict(form="StreamDelta16", delta=(16, 256, None)), "spmv_delta = 2 takes the cheaper width whatever it saves")
# --- templates
_c("tmpl_1024", "template", "tmpl1024", {}, dict(form="Template", templates=1024), "kTmplMax 1024 | 1025: admitted", compress=True)
_c("tmpl_1025", "template", "tmpl1025", {}, dict(templates=0, kernel=4), "kTmplMax 1024 | 1025: refused", compress=True, unavailable={"template": _R_T})
_c("tmpl_K32", "template", "tmplK32", {}, dict(form="Template", templates=4), "kTmplMaxLen 32 | 33: admitted", compress=True)
_c("tmpl_K33", "template", "tmplK33", {}, dict(templates=0), "kTmplMaxLen 32 | 33: refused", compress=True, unavailable={"template": _R_K})
_c("tmpl_bytes_at", "template", "tmpl_bytes_at", {}, dict(form="Template", templates=960), "T * K * 12 + T * 4 = 61440: admitted", compress=True)
_c("tmpl_bytes_over", "template", "tmpl_bytes_over", {}, dict(templates=0), "T * K * 12 + T * 4 = 61504: refused", compress=True, unavailable={"template": _R_LDS})
_c("tmpl_zero_sign", "template", "tmpl_zero_sign", {}, dict(form="Template", templates=3), "rows that differ in the sign of a zero: two templates", compress=True)
_c("tmpl_nan_payload", "template", "tmpl_nan_payload", {}, dict(form="Template", templates=3), "rows that differ in a NaN payload: two templates", compress=True)
_c("tmpl_empty_rect", "template", "tmpl_empty_rect", {}, dict(form="Template", templates=3), "empty rows on a rectangular operator", compress=True)
_c("tmpl_one_row", "template", "tmpl_one_row", {}, dict(form="Template", templates=1), "a one-row operator", compress=True)
_c("tmpl_off", "template", "tmpl_empty_rect", dict(spmv_template=0), dict(templates=3, kernel=4), "compressed, spmv_template = 0: the CSR forms", compress=True)
# --- transpose
for _n1 in (2047, 2048, 2049, 4096, 4097, 3 * 2048 + 1):
    _c("tr_scan%d" % _n1, "transpose", "tr_scan%d" % _n1, {}, dict(form="Coded16"), "n + 1 = %d counts: %d scan tile(s)" % (_n1, -(-_n1 // SCAN_TILE)), transpose=True, want_t="Coded16", want_tt="Coded16")
_c("tr_long_col", "transpose", "tr_long_col", {}, dict(form="Sliced32"), "one column of 2000 entries (tr_sort_rows_kernel)", transpose=True,
   want_t="Stream", want_tt="Sliced32")
_c("tr_repeats", "transpose", "tr_repeats", {}, dict(form="Coded16"), "repeated (row, column) entries with different values", transpose=True,
   want_t="Coded16", want_tt="Coded16")
_c("tr_m1", "transpose", "tr_m1", {}, dict(form="Sliced"), "m = 1", transpose=True, want_t="Sliced", want_tt="Sliced")
_c("tr_n1", "transpose", "tr_n1", {}, dict(form="Sliced"), "n = 1: A' is one row of every entry, the vector kernel", transpose=True,
   want_t="Vector", want_tt="Sliced")
# --- unsorted and repeated columns through every form
for _op in ("band_perm", "band_split"):
    _c(_op + "_coded", "unsorted", _op, _CODED, dict(form="Coded8", code=(8, 7)), "unsorted rows: d == last in code_collect_kernel")
    _c(_op + "_m0", "unsorted", _op, _PLAIN, dict(form="Sliced"), "unsorted rows, mode 0")
    _c(_op + "_m3", "unsorted", _op, _K4, dict(form="Sliced"), "unsorted rows, mode 3")
    _c(_op + "_m2", "unsorted", _op, _NARROW, dict(form="SlicedNarrow"), "unsorted rows, mode 2")
    _c(_op + "_m1", "unsorted", _op, _S32, dict(form="Sliced32"), "unsorted rows, mode 1")
    _c(_op + "_m4", "unsorted", _op, _S32P, dict(form="Sliced32"), "unsorted rows, mode 4")
    _c(_op + "_d8", "unsorted", _op, dict(spmv_kernel=1, spmv_delta=8), dict(form="StreamDelta8"), "unsorted rows, 8-bit delta stream")
    _c(_op + "_d16", "unsorted", _op, dict(spmv_kernel=1, spmv_delta=16), dict(form="StreamDelta16"), "unsorted rows, 16-bit delta stream")
    _c(_op + "_tmpl", "unsorted", _op, {}, dict(form="Template"), "unsorted rows as templates", compress=True)
    _c(_op + "_tr", "unsorted", _op, {}, dict(form="Sliced"), "unsorted rows: the stable insertion sort of the transpose; band_kernel's extremes",
       transpose=True, want_t="Sliced", want_tt="Sliced")
    _c(_op + "_c16", "unsorted", _op, dict(_CODED, spmv_codes=16), dict(form="Coded16", code=(16, 7)), "unsorted rows, two-byte codes")
    _c(_op + "12_m5", "unsorted", _op + "12", _K4, dict(form="Sliced"), "unsorted rows of up to 12 entries, mode 5")
    _c(_op + "12_m0", "unsorted", _op + "12", _PLAIN, dict(form="Sliced"), "unsorted rows of up to 12 entries, mode 0")
    _c(_op + "12_c16", "unsorted", _op + "12", dict(_CODED, spmv_codes=16), dict(form="Coded16"), "unsorted rows of up to 12 entries, two-byte codes")
# --- plan thresholds
_NC = dict(spmv_codes=0)
_c("plan_mean12", "plan", "mean12", _NC, dict(kernel=4, form="Staged"), "mean row 12.0 | above: staged")
_c("plan_mean12_plus", "plan", "mean12_plus", _NC, dict(kernel=1, form="Stream"), "mean row 12.0 | above: stream")
_c("plan_mean96", "plan", "mean96", {}, dict(kernel=1, form="Stream"), "mean row 96.0 | above: stream")
_c("plan_mean96_plus", "plan", "mean96_plus", {}, dict(kernel=2, form="Vector"), "mean row 96.0 | above: vector (held to vector_row_bound)")
_c("plan_max64", "plan", "max64", _NC, dict(kernel=4, form="Staged"), "longest row 64 | 65 at mean <= 12: staged")
_c("plan_max65", "plan", "max65", _NC, dict(kernel=1, form="Stream"), "longest row 64 | 65 at mean <= 12: stream")
_c("plan_max64_codes", "plan", "max64", {}, dict(kernel=4, form="Sliced"), "longest row 64 with codes: kCodedMaxRow admits")
_c("plan_max65_codes", "plan", "max65", {}, dict(kernel=1, form="Stream", code=(32, 0)), "longest row 65: the codes are not tried")
_c("plan_mean8_delta", "plan", "mean8", dict(spmv_kernel=1, spmv_delta=16), dict(delta=(16, 256, None)), "256 * mean = 2048: 256-row blocks")
_c("plan_mean8_plus_delta", "plan", "mean8_plus", dict(spmv_kernel=1, spmv_delta=16), dict(delta=(16, 128, None)), "256 * mean > 2048: 128-row blocks")
_c("plan_mean8_s32", "plan", "mean8", _S32, dict(form="Sliced32"), "256 * mean = 2048: rows == 256, the int32 copy is tried")
_c("plan_mean8_plus_s32", "plan", "mean8_plus", _S32, dict(form="Staged", sell32=(0, 0, 0)), "256 * mean > 2048: rows == 128, not tried")

CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)
GROUPS = ("codes", "sliced", "delta", "template", "transpose", "unsorted", "plan")


def cases_of(group):
    return [c for c in CASES if c.group == group]


_EXP_CACHE = {}


def expected_of(case):
    if case.name not in _EXP_CACHE:
        _EXP_CACHE[case.name] = expected(get_op(case.op), case.options, case.compress)
    return _EXP_CACHE[case.name]


_EXP_NF_CACHE = {}


def expected_nf_of(case):
    """The fields of the handle with Inf / NaN values: the structure's, but for the templates, which are compared by value bits."""
    if case.name not in _EXP_NF_CACHE:
        _EXP_NF_CACHE[case.name] = expected(get_op(case.op).nonfinite(), case.options, case.compress)
    return _EXP_NF_CACHE[case.name]


def want_mismatches(case, exp=None):
    """Where the model's prediction differs from what the table states the case is there for: an error of the table."""
    exp = exp or expected_of(case)
    bad = []
    for k, v in case.want.items():
        if v is None:
            continue
        got = exp[k]
        if isinstance(v, tuple):
            if len(v) != len(got) or any(a is not None and a != b for a, b in zip(v, got)):
                bad.append((case.name, k, v, got))
        elif got != v:
            bad.append((case.name, k, v, got))
    if case.transpose:
        ref = transposed_op(get_op(case.op))
        for k, v, o in (("form of A'", case.want_t, ref), ("form of (A')'", case.want_tt, transposed_op(ref))):
            got = expected(o, case.options)["form"]
            if got != v:
                bad.append((case.name, k, v, got))
    return bad


# ---------------------------------------------------------------------------------------------------- the coverage condition

def coverage():
    """edge -> {side: [cases]}: every threshold of the builders and of the plan, hit from both sides; every sell_head_words value
    of modes 0, 1, 4, 5; uniform and offset layouts of every mode.  tests/test_operator_forms_host.py asserts that no list is
    empty."""
    cov = {}

    def hit(edge, side, case):
        cov.setdefault(edge, {}).setdefault(side, []).append(case.name)
    heads = {mode: set() for mode in range(6)}
    layouts = {mode: set() for mode in range(6)}
    for c in CASES:
        op, exp, o = get_op(c.op), expected_of(c), c.options
        info = op.info()
        T, L, mean = info["diagonals"], info["max_row"], info["mean_row"]
        if c.group == "codes":
            for lo in (15, 255, 256, 2048):
                if T in (lo, lo + 1):
                    if lo == 15 and not o["spmv_sell_narrow"]:
                        continue
                    hit("code_T %d | %d" % (lo, lo + 1), "at" if T == lo else "above", c)
        for key in ("sell_layout", "sell32_layout"):
            lay = exp.get(key)
            if lay:
                units = np.full(lay["S"], lay["umax"]) if lay["uniform"] else lay["units"]
                heads[lay["mode"]] |= set(int(w) for w in head_words(units, lay["mode"]) if w > 0)
                layouts[lay["mode"]].add("uniform" if lay["uniform"] else "offset")
                if lay["uniform"] and (lay["Ls"] == 0).any():
                    hit("all-empty slice in a uniform layout", "mode %d" % lay["mode"], c)
                hit("m % 64", str(op.m % 64) if op.m >= 64 else "m < 64", c)
        if c.group == "sliced":
            if L in (64, 65):
                hit("sell longest row 64 | 65", "at" if L == 64 else "above", c)
            if c.op.startswith("pad_"):
                ratio = _pad_ratio(op, sell_mode(info, o, False, T)[0], False)
                assert (ratio <= SELL_MAX_PAD) == (exp["sell"][0] == 1), "the 64 KiB of slack decides"
                hit("kSellMaxPad", "admitted" if exp["sell"][0] == 1 else "refused", c)
            if o["spmv_sell_narrow"] and L in (8, 9) and T <= 15:
                hit("narrow max_row_nnz 8 | 9", "at" if L == 8 else "above", c)
        dm = exp.get("delta_model")
        if dm and dm["state"] == 1:
            base, rel, esc = _escapes(op, dm["rows"], dm["bits"])
            ESC = (1 << dm["bits"]) - 1
            for name, sel in (("base - 1", rel == -1), ("base", rel == 0), ("base + 2^bits - 2", rel == ESC - 1), ("base + 2^bits - 1", rel == ESC)):
                if sel.any():
                    assert bool(esc[sel].all()) == (name in ("base - 1", "base + 2^bits - 1"))
                    hit("delta %d bits, %d rows" % (dm["bits"], dm["rows"]), name, c)
            if (base == 0).any() and (base > 0).any():
                hit("delta base", "clamped and free", c)
            per = np.bincount(op.row_of[esc] // dm["rows"], minlength=-(-op.m // dm["rows"]))
            if ((per[:-1] == 0) & (per[1:] > 256)).any():
                hit("delta escapes per block", "0 next to > 256", c)
            if op.m % dm["rows"]:
                hit("delta last block", "partial", c)
        if dm and c.op.startswith("block"):
            big = int(op.rowptr[32])
            hit("delta block entries 65535 | 65536", "at" if big == 65535 else "above", c)
            if dm["state"] == 1 and dm["bits"] == 16:
                e = encode_delta(op, dm["rows"], 16)
                assert 65534 in e["esc_pos"][e["esc_blk"] == 0]
                hit("delta esc_pos", "65534", c)
        if dm and o["spmv_delta"] in (1, 2) and c.op.startswith("by_"):
            hit("6 * by > 5 * by32 under spmv_delta = %d" % o["spmv_delta"], "6 by == 5 by32" if c.op == "by_admit" else "above", c)
        if c.group == "template":
            tm = template_model(op)
            n_t = len({(op.col[a:b].astype(np.int64) - r).tobytes() + op.val[a:b].tobytes() for r, (a, b) in enumerate(zip(op.rowptr[:-1], op.rowptr[1:]))})
            if n_t in (1024, 1025):
                hit("kTmplMax 1024 | 1025", "at" if n_t == 1024 else "above", c)
            if L in (32, 33):
                hit("kTmplMaxLen 32 | 33", "at" if L == 32 else "above", c)
            by = n_t * L * 12 + n_t * 4
            if L <= 32 and n_t <= 1024 and abs(by - TMPL_LDS_MAX) <= 64:
                hit("kTmplLdsMax 61440", "at" if by <= TMPL_LDS_MAX else "above", c)
            del tm
        if c.transpose:
            hit("scan tiles", "%d" % (-(-(op.n + 1) // SCAN_TILE)), c)
            if (op.n + 1) % SCAN_TILE in (0, 1, SCAN_TILE - 1):
                hit("scan n + 1 mod 2048", str((op.n + 1) % SCAN_TILE), c)
        if c.group == "plan":
            if o["spmv_kernel"] == 0 and o["spmv_codes"] == 0 and L <= 64 and abs(mean - 12.0) < 0.1:
                hit("plan mean 12.0", "at" if mean <= 12.0 else "above", c)
            if o["spmv_kernel"] == 0 and abs(mean - 96.0) < 0.1:
                hit("plan mean 96.0", "at" if mean <= 96.0 else "above", c)
            if o["spmv_kernel"] == 0 and mean <= 12.0 and L in (64, 65):
                hit("plan longest row 64 | 65 (spmv_codes = %d)" % o["spmv_codes"], "at" if L == 64 else "above", c)
            if abs(256 * mean - 2048.0) < 1.0:
                hit("plan 256 * mean 2048 (%s)" % ("stream" if exp["kernel"] == 1 else "staged"), "at" if 256 * mean <= 2048.0 else "above", c)
    for mode in range(6):
        for lay in ("uniform", "offset"):
            cov.setdefault("layout of mode %d" % mode, {})[lay] = [lay] if lay in layouts[mode] else []
    want_heads = {0: set(range(1, 9)), 1: set(range(1, 33)), 4: set(range(2, 33, 2)), 5: {2, 4, 6, 8}}
    for mode, want in want_heads.items():
        cov["sell_head_words of mode %d" % mode] = {str(w): ([w] if w in heads[mode] else []) for w in sorted(want)}
    return cov


_AT = ("at", "above")
_REL = ("base - 1", "base", "base + 2^bits - 2", "base + 2^bits - 1")
REQUIRED_SIDES = {
    "code_T 15 | 16": _AT, "code_T 255 | 256": _AT, "code_T 256 | 257": _AT, "code_T 2048 | 2049": _AT, "sell longest row 64 | 65": _AT,
    "kSellMaxPad": ("admitted", "refused"), "narrow max_row_nnz 8 | 9": _AT, "m % 64": ("0", "1", "63", "m < 64"),
    "all-empty slice in a uniform layout": tuple("mode %d" % k for k in range(6)),
    "delta 8 bits, 32 rows": _REL, "delta 8 bits, 64 rows": _REL, "delta 16 bits, 32 rows": _REL, "delta 16 bits, 64 rows": _REL,
    "delta 16 bits, 256 rows": _REL, "delta base": ("clamped and free",), "delta escapes per block": ("0 next to > 256",),
    "delta last block": ("partial",), "delta block entries 65535 | 65536": _AT, "delta esc_pos": ("65534",),
    "6 * by > 5 * by32 under spmv_delta = 1": ("6 by == 5 by32", "above"), "6 * by > 5 * by32 under spmv_delta = 2": ("6 by == 5 by32", "above"),
    "kTmplMax 1024 | 1025": _AT, "kTmplMaxLen 32 | 33": _AT, "kTmplLdsMax 61440": _AT, "scan tiles": ("1", "2", "3", "4"),
    "scan n + 1 mod 2048": ("2047", "0", "1"),
    "plan mean 12.0": _AT, "plan mean 96.0": _AT, "plan longest row 64 | 65 (spmv_codes = 0)": _AT, "plan longest row 64 | 65 (spmv_codes = 2)": _AT,
    "plan 256 * mean 2048 (stream)": _AT, "plan 256 * mean 2048 (staged)": _AT,
}


# ---------------------------------------------------------------------------------------------------- the emulation

FAULTS = ("delta_escape_bound_off_by_one", "delta_below_base_not_escaped", "sentinel_ff_read_as_entry", "sentinel_f_read_as_entry",
          "mode5_head_words_off_in_one_range", "uniform_units_on_offset_layout", "pair_value_word_swapped", "code16_truncated_to_8",
          "template_match_by_value", "template_id_byte_truncated", "transpose_unstable_among_repeats", "scan_tile_offset_dropped")


def product(op, exp, x, fault=None):
    """y = A x through the stored form `exp` describes: encode as the builder, decode as the kernel."""
    form = exp["form"]
    if form == "Template":
        return decode_template(op, exp["template"], x, fault)
    if form in ("Sliced", "SlicedNarrow"):
        enc = exp["codes_enc"]
        return decode_sell(op, encode_sell(op, exp["sell_layout"], enc["code"]), x, enc["tab"], fault)
    if form == "Sliced32":
        return decode_sell(op, encode_sell(op, exp["sell32_layout"]), x, None, fault)
    if form.startswith("Coded"):
        return decode_codes(op, exp["codes_enc"], x, fault)
    if form.startswith("StreamDelta"):
        bits, R, _ = exp["delta"]
        return decode_delta(op, encode_delta(op, R, bits, fault), x)
    return stored_product(op.rowptr, op.col, op.val, x)                   # the CSR kernels


def _scalars(op, x, w, y):
    """What spmv_dot / spmv_dotw / spmv_dot2 return, exactly rounded (NaN where y is not finite)."""
    if not np.isfinite(y).all():
        return dict(dot=math.nan, dotw=math.nan, dot2=(math.nan, math.nan))
    try:
        out = dict(dotw=er.exact_dot(w, y))
        if op.n >= op.m:
            out["dot"] = er.exact_dot(x[:op.m], y)
            out["dot2"] = (out["dot"], er.exact_dot(y, y))
    except ValueError:                                                   # a faulty emulation may leave the exact window
        out = dict(dot=math.nan, dotw=math.nan, dot2=(math.nan, math.nan))
    return out


def observe(op, exp, fault=None):
    """One handle's results, as the GPU file collects them: fields, y(x), y(special x), y of a second product, the fused ys
    and scalars."""
    inp = op.inputs()
    y0 = product(op, exp, inp["x"], fault)
    out = {k: exp[k] for k in FIELDS}
    out.update(y=[y0, product(op, exp, inp["xs"], fault), y0.copy()], y_dot=[y0.copy()] * 3, **_scalars(op, inp["x"], inp["w"], y0))
    return out


def emulate(case, fault=None):
    """The emulation of one case: dict(A = observation of the handle; for a transpose case also arrays = (rowptr, col, val) of
    A', At and Att = observations of A' and (A')')."""
    op = get_op(case.op)
    exp = expected(op, case.options, case.compress, fault) if fault in ("template_match_by_value",) else expected_of(case)
    out = dict(A=observe(op, exp, fault))
    nf = op.nonfinite()
    exp_nf = expected(nf, case.options, case.compress, fault if fault == "template_match_by_value" else None)
    out["N"] = dict({k: exp_nf[k] for k in FIELDS}, y=[product(nf, exp_nf, nf.inputs()[k], fault) for k in ("x", "xs")])
    if case.transpose:
        arrays = transpose_model(op, fault)
        out["arrays"] = arrays
        ref = transposed_op(op)
        ok = all(np.array_equal(a, b) for a, b in zip(arrays[:2], (ref.rowptr, ref.col)))
        opT = Op(ref.name, ref.m, ref.n, *arrays, ref.subnormal) if (fault and ok) else ref          # a broken structure is judged on the arrays alone
        out["At"] = observe(opT, expected(ref, case.options), None)
        opTT = transposed_op(opT)
        out["Att"] = observe(opTT, expected(transposed_op(ref), case.options), None)
    return out


# ---------------------------------------------------------------------------------------------------- the comparisons

def same_bits(a, b):
    """NaN for NaN, everything else bit for bit (the sign of a zero included)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    return bool(np.all((np.isnan(a) & np.isnan(b)) | (a.view(np.int64) == b.view(np.int64))))


def _first_diff(a, b):
    bad = np.flatnonzero(~((np.isnan(a) & np.isnan(b)) | (a.view(np.int64) == b.view(np.int64))))
    return "%d rows differ, first row %d: %r against %r" % (bad.size, int(bad[0]), float(a[bad[0]]), float(b[bad[0]]))


def form_failures(exp, obs, opts, what="A"):
    """The fields a handle reports against the model's: what the GPU file asserts before it looks at a number."""
    fails = ["%s: %s = %r, the model expects %r" % (what, k, obs[k], exp[k]) for k in FIELDS if k != "form" and obs[k] != exp[k]]
    name = form_name(obs, opts)
    if name != exp["form"]:
        fails.append("%s: ran %s, the model expects %s" % (what, name, exp["form"]))
    return fails


def judge_handle(op, exp, obs, opts, what, ratios=None, y_only=False):
    """One handle: the form BEFORE any number, then y against the serial product (the vector kernel: vector_row_bound), the fused
    products' y, and the fused scalars against exact_reduction's tally.  Returns the list of failures."""
    ratios = ratios if ratios is not None else pm.Ratios()
    fails = form_failures(exp, obs, opts, what)
    if fails:
        return fails
    inp = op.inputs()
    refs = [inp["y"], inp["ys"], inp["y"]][:len(obs["y"])]
    xs = [inp["x"], inp["xs"], inp["x"]]
    for k, (y, ref) in enumerate(zip(obs["y"], refs)):
        y = np.asarray(y, dtype=np.float64)
        if y.shape != ref.shape:
            fails.append("%s: y[%d] has %d rows, not %d" % (what, k, y.size, ref.size))
        elif exp["form"] != "Vector":
            if not same_bits(y, ref):
                fails.append("%s: y[%d]: %s" % (what, k, _first_diff(y, ref)))
        else:
            if not (np.array_equal(np.isnan(y), np.isnan(ref)) and np.array_equal(np.isinf(y), np.isinf(ref))
                    and np.array_equal(np.sign(y[np.isinf(y)]), np.sign(ref[np.isinf(y)]))):
                fails.append("%s: y[%d]: non-finite rows differ from the serial loop's" % (what, k))
                continue
            finite = np.flatnonzero(np.isfinite(ref))
            ratio = vector_row_bound(op, np.where(np.isfinite(xs[k]), xs[k], 0.0), y, 0, op.m, finite)
            ratios.add("vector_rows", ratio)
            if ratio > 1.0:
                fails.append("%s: y[%d]: |d| / (gamma(k) sum|a x|) = %.3g" % (what, k, ratio))
    if fails or y_only:
        return fails
    y0 = np.asarray(obs["y"][0], dtype=np.float64)
    for j, yd in enumerate(obs["y_dot"]):
        if yd is not None and not same_bits(np.asarray(yd, dtype=np.float64), y0):
            fails.append("%s: y of fused product %d differs from the plain product's" % (what, j))
    scal = [("spmv_dotw", obs["dotw"], inp["w"], False)]
    if op.n >= op.m:
        scal += [("spmv_dot", obs["dot"], inp["x"][:op.m], False), ("spmv_dot2.xy", obs["dot2"][0], inp["x"][:op.m], False),
                 ("spmv_dot2.yy", obs["dot2"][1], y0, True)]
    if not np.isfinite(y0).all():                                        # a NaN / Inf value in the operator: no exact value, IEEE says non-finite
        return fails + ["%s: %s = %r is finite although y is not" % (what, nm, d) for nm, d, _, _ in scal if math.isfinite(d)]
    tally = er.Tally(lambda **kw: ratios.add(kw["what"], kw["ratio"]), op.name)
    for nm, d, u, sq in scal:
        ok, detail = tally.sq(nm, d, y0) if sq else tally.dot(nm, d, u, y0, 1.0, n=op.m)
        if not ok:
            fails.append("%s: %s outside its bound: %r" % (what, nm, detail))
    return fails


def judge(case, obs, ratios=None):
    """Every comparison of one case; obs as `emulate` returns it.  Empty list = passes."""
    op = get_op(case.op)
    fails = ["table: %s %s = %r, the model predicts %r" % bad for bad in want_mismatches(case)]
    if fails:
        return fails
    opts = case.options
    fails = judge_handle(op, expected_of(case), obs["A"], opts, "A", ratios)
    if not fails:
        nf = op.nonfinite()
        fails = judge_handle(nf, expected_nf_of(case), obs["N"], opts, "A with Inf / NaN values", ratios, y_only=True)
    if not case.transpose or fails:
        return fails
    ref = transposed_op(op)
    for name, got, want in zip(("rowptr", "col", "val"), obs["arrays"], (ref.rowptr, ref.col, ref.val)):
        got = np.asarray(got)
        if got.shape != want.shape or not (same_bits(got, want) if name == "val" else np.array_equal(got, want)):
            fails.append("A': %s differs from the stable column-major order of A" % name)
    if fails:
        return fails
    fails += judge_handle(ref, expected(ref, opts), obs["At"], opts, "A'", ratios)
    refT = transposed_op(ref)
    return fails + judge_handle(refT, expected(refT, opts), obs["Att"], opts, "(A')'", ratios)
