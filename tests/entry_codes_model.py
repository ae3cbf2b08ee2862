"""Host model of the entry-coded sliced copy (krylov.jl_amd/csrc/colcode.hip csr_build_sell_entries, spmv_sell_kernel's ENT arm).

An ENTRY is the pair (column - row, bit pattern of the value).  A handle with 8-bit diagonal codes (at most 255 diagonals), rows of
at most 64 entries and at most 255 distinct entries keeps one byte per entry -- the rank of its pair in the dictionary, ascending by
(offset, value bits taken as unsigned), 0xFF = no entry -- in 64-row slices: lane l of slice s owns row 64 s + l.  A slice whose
longest row has L entries holds T = ent_units(L) words of eight codes per lane: T = 1 (L <= 8; word of lane l at o0 * 64 + l) or
ceil(L / 8) padded to an even count, in 16-byte pairs (word w of lane l at o0 * 64 + ((w / 2) * 64 + l) * 2 + (w & 1)).  Padding,
uniform and offset rules are build_sell_form's with this form's units, measured against the same CSR stream (9 nnz + 4 m bytes).

encode / decode / verify here are NumPy; the products follow the serial loop (stored order, one rounded multiply and one rounded
add per entry), so product(encode(op), x) must equal op.serial(x) bit for bit.  The operators come from operator_forms_model (their
structure) with values drawn from a small palette, so that they qualify.
"""
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)
import operator_forms_model as fm  # noqa: E402

ENT_MAX, MARK, SLICE = 255, 0xFF, 64
MAX_ROW, MAX_DIAGONALS = 64, 255
SELL_MAX_PAD, SELL_UNIFORM_PAD = fm.SELL_MAX_PAD, fm.SELL_UNIFORM_PAD
BIG_NNZ = fm.BIG_NNZ


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def nan_payload(p):
    return np.array([0x7FF8000000000000 | p], dtype=np.uint64).view(np.float64)[0]


# ---------------------------------------------------------------------------------------------------- operators

PALETTE = np.array([6.0, -1.0, 0.5, -0.0, 0.0, 3e-310, -2.75, 1.0 / 3.0])


def with_palette(op, name=None, k=2):
    """The structure of `op`, every value a function of (offset, row parity): at most k values per diagonal."""
    d = op.col.astype(np.int64) - op.row_of
    val = PALETTE[(3 * d + (op.row_of % k)) % PALETTE.size]
    return fm.Op(name or op.name + "_pal", op.m, op.n, op.rowptr, op.col, val, op.subnormal)


def stencil_op(kind, n1):
    """poisson / kron_unsymmetric / stencil27 as the library's generators store them (the oracle's arrays)."""
    import oracle as ok
    A = {"poisson": ok.poisson3d, "kron_unsymmetric": ok.kron_unsymmetric, "stencil27": ok.stencil27_unsym}[kind](n1)
    return fm.Op("%s%d" % (kind, n1), A.n, A.n, np.array(A.rowptr), np.array(A.col), np.array(A.val))      # copies: A owns its arrays


def pairs_op(name, P):
    """Exactly P distinct entries: row r holds (0, value number r % (P - 1)); the last row also holds (+1, 1.0) -- the largest
    pair, code P - 1, occurs in the last row alone."""
    m = P + 70
    vals = 1.0 + np.arange(P - 1) / 64.0
    rows = [np.array([r]) for r in range(m - 1)] + [np.array([m - 1, m])]
    val = np.concatenate([vals[np.arange(m) % (P - 1)], [1.0]])
    op = fm._from_rows(name, m + 1, rows, val=val)
    assert count_pairs(op) == P
    return op


def count_pairs(op):
    d = op.col.astype(np.int64) - op.row_of
    return np.unique(np.stack([d.view(np.uint64), bits(op.val)], axis=1), axis=0).shape[0]


# ---------------------------------------------------------------------------------------------------- dictionary and layout

def dictionary(op):
    """(offsets int32[P], value bits uint64[P]) ascending by (offset, bits as unsigned), or None above 255 pairs."""
    d = op.col.astype(np.int64) - op.row_of
    b = bits(op.val)
    order = np.lexsort((b, d))
    d, b = d[order], b[order]
    first = np.ones(d.size, dtype=bool)
    first[1:] = (d[1:] != d[:-1]) | (b[1:] != b[:-1])
    if int(first.sum()) > ENT_MAX:
        return None
    return d[first].astype(np.int32), b[first].copy()


def ent_units(L):
    return 0 if L <= 0 else (1 if L <= 8 else (L + 7) // 8 + (((L + 7) // 8) & 1))


def refusal(op):
    """Why csr_build_sell_entries refuses the handle, or None."""
    info = op.info()
    if op.m == 0 or op.nnz == 0:
        return "empty"
    if info["max_row"] > MAX_ROW:
        return "a row of more than 64 entries"
    if info["diagonals"] > MAX_DIAGONALS:
        return "more than 255 diagonals"
    if dictionary(op) is None:
        return "more than 255 pairs"
    lay = layout(op)
    if 512.0 * lay["sum"] > SELL_MAX_PAD * (9.0 * op.nnz + 4.0 * op.m) + 65536.0:
        return "too much padding"
    return None


def layout(op):
    slices = (op.m + SLICE - 1) // SLICE
    lens = np.concatenate([op.lens, np.zeros(slices * SLICE - op.m, dtype=op.lens.dtype)])
    units = np.array([ent_units(int(L)) for L in lens.reshape(slices, SLICE).max(axis=1)], dtype=np.int64)
    total, umax = int(units.sum()), int(units.max()) if slices else 0
    uniform = umax * slices <= SELL_UNIFORM_PAD * total + 8.0
    off = np.arange(slices + 1, dtype=np.int64) * umax if uniform else np.concatenate([[0], np.cumsum(units)])
    return dict(slices=slices, units=units, sum=total, uniform=uniform, umax=umax, total=umax * slices if uniform else total, off=off)


def sell_info(op):
    lay = layout(op)
    return (1, lay["umax"] if lay["uniform"] else 0, lay["total"])


def bytes_stored(op):
    """khip_spmv_bytes_stored of the entry-coded copy: 512 B per unit (+ 4 B per slice of offsets) + x + y; the table is ignored."""
    lay = layout(op)
    return 512 * lay["total"] + (0 if lay["uniform"] else 4 * (lay["slices"] + 1)) + 8 * op.n + 8 * op.m


def _slot(o0, T, w, lane):
    return o0 * 64 + (lane if T == 1 else ((w >> 1) * 64 + lane) * 2 + (w & 1))


def encode(op):
    """dict(off, vbits, words uint64[total * 64], lay) -- the dictionary and the slices as the fill pass writes them."""
    assert refusal(op) is None, refusal(op)
    tab_off, tab_bits = dictionary(op)
    lay = layout(op)
    d = op.col.astype(np.int64) - op.row_of
    b = bits(op.val)
    rank = {(int(o), int(v)): i for i, (o, v) in enumerate(zip(tab_off, tab_bits))}
    code = np.array([rank[(int(o), int(v))] for o, v in zip(d, b)], dtype=np.uint64)
    words = np.zeros(lay["total"] * 64, dtype=np.uint64)
    for row in range(lay["slices"] * SLICE):
        s, lane = row >> 6, row & 63
        o0 = int(lay["off"][s])
        T = lay["umax"] if lay["uniform"] else int(lay["units"][s])
        q0 = int(op.rowptr[row]) if row < op.m else 0
        ln = int(op.lens[row]) if row < op.m else 0
        for w in range(T):
            word = 0
            for u in range(8):
                k = 8 * w + u
                word |= (int(code[q0 + k]) if k < ln else MARK) << (8 * u)
            words[_slot(o0, T, w, lane)] = word
    return dict(off=tab_off, vbits=tab_bits, words=words, lay=lay, m=op.m)


def _row_codes(enc, row):
    lay = enc["lay"]
    s, lane = row >> 6, row & 63
    o0 = int(lay["off"][s])
    T = lay["umax"] if lay["uniform"] else int(lay["units"][s])
    out = []
    for w in range(T):
        word = int(enc["words"][_slot(o0, T, w, lane)])
        out += [(word >> (8 * u)) & 0xFF for u in range(8)]
    return out


def product(enc, x):
    """What the kernel's arm computes: every slot of the row's words in order, a slot other than 0xFF is an entry."""
    off = np.concatenate([enc["off"], np.zeros(256 - enc["off"].size, dtype=np.int32)])
    val = np.concatenate([enc["vbits"], np.zeros(256 - enc["vbits"].size, dtype=np.uint64)]).view(np.float64)
    y = np.zeros(enc["m"])
    with np.errstate(all="ignore"):
        for row in range(enc["m"]):
            acc = np.float64(0.0)
            for c in _row_codes(enc, row):
                if c != MARK:
                    acc = acc + val[c] * x[row + int(off[c])]
            y[row] = acc
    return y


def verify(enc, op):
    """The fill pass's check, read back: the dictionary ascends strictly, every entry's code names exactly its (offset, value
    bits), and every slot behind a row's last entry is 0xFF."""
    o, v = enc["off"].astype(np.int64), enc["vbits"]
    if o.size == 0 or o.size > ENT_MAX:
        return False
    if not all((o[i], int(v[i])) < (o[i + 1], int(v[i + 1])) for i in range(o.size - 1)):
        return False
    b = bits(op.val)
    for row in range(enc["lay"]["slices"] * SLICE):
        codes = _row_codes(enc, row)
        ln = int(op.lens[row]) if row < op.m else 0
        if ln > len(codes):
            return False
        for k, c in enumerate(codes):
            if k >= ln:
                if c != MARK:
                    return False
                continue
            q = int(op.rowptr[row]) + k
            if c >= o.size or int(o[c]) != int(op.col[q]) - row or int(v[c]) != int(b[q]):
                return False
    return True


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def same_bits_or_nan(a, b):
    """Bit views equal wherever either side is a number (zero signs, infinities); a NaN must face a NaN -- its sign and payload
    are the processor's choice (Inf - Inf is a negative NaN on x86 and a positive one on CDNA), so they are not compared."""
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])
