"""The entry-coded sliced copy on the host (tests/entry_codes_model.py): the emulated product against the serial product bit for
bit, the order of the dictionary, the rules that refuse the form, and injected faults."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import entry_codes_model as em  # noqa: E402
import operator_forms_model as fm  # noqa: E402

STRUCTURES = ("ragged8", "ragged64", "uniform9_hole", "uniform7_hole", "uniform7_m192", "uniform7_m193", "uniform7_m40", "row64")


def _ops():
    out = [em.stencil_op("poisson", 5), em.stencil_op("kron_unsymmetric", 5), em.stencil_op("stencil27", 5)]
    out += [em.with_palette(fm.get_op(name)) for name in STRUCTURES]
    out.append(em.pairs_op("pairs255", 255))
    return out


@pytest.mark.parametrize("op", _ops(), ids=lambda o: o.name)
def test_emulated_product_is_the_serial_product(op):
    assert em.refusal(op) is None
    enc = em.encode(op)
    assert em.verify(enc, op)
    inp = op.inputs()
    for x, y in ((inp["x"], inp["y"]), (inp["xs"], inp["ys"])):
        assert em.same_bits(em.product(enc, x), y)


def test_layout_units_and_bytes():
    assert [em.ent_units(L) for L in (0, 1, 8, 9, 16, 17, 27, 32, 33, 64)] == [0, 1, 1, 2, 2, 4, 4, 4, 6, 8]
    op = em.stencil_op("poisson", 8)                                    # 512 rows of at most 7 entries: one word per row
    assert em.sell_info(op) == (1, 1, 8) and em.bytes_stored(op) == 512 * 8 + 16 * 512
    n = 512 ** 3                                                        # the flagship operator: 24 B per row
    assert 512 * (n // 64) + 16 * n == 24 * n == 3221225472
    r8 = em.with_palette(fm.get_op("ragged8"))                          # L = 1 .. 8: every slice one unit, uniform
    assert em.layout(r8)["uniform"] and em.sell_info(r8)[1] == 1
    r64 = em.with_palette(fm.get_op("ragged64"))                        # L = 1 .. 64: per-slice offsets
    lay = em.layout(r64)
    assert not lay["uniform"] and lay["total"] == sum(em.ent_units(L) for L in range(1, 65))
    assert em.bytes_stored(r64) == 512 * lay["total"] + 4 * (lay["slices"] + 1) + 8 * r64.n + 8 * r64.m
    hole = em.layout(em.with_palette(fm.get_op("uniform9_hole")))       # an all-empty slice keeps its two units
    assert hole["uniform"] and hole["umax"] == 2 and hole["units"][17] == 0


def test_dictionary_order_is_deterministic():
    op = em.with_palette(fm.get_op("ragged64"))
    off, vb = em.dictionary(op)
    keys = list(zip(off.tolist(), vb.tolist()))
    assert keys == sorted(set(keys)) and len(keys) == em.count_pairs(op)
    # the same entries met in another order (rows reversed: another operator with the same pairs) give the same table
    rows = [op.col[op.rowptr[r]:op.rowptr[r + 1]] - r for r in range(op.m)][::-1]
    vals = [op.val[op.rowptr[r]:op.rowptr[r + 1]] for r in range(op.m)][::-1]
    shift = int(max(0, -min(int(d.min()) for d in rows if d.size)))
    rev = fm._from_rows("rev", op.n + op.m + shift, [d + r + shift for r, d in enumerate(rows)], val=np.concatenate(vals))
    off2, vb2 = em.dictionary(rev)
    assert np.array_equal(off2 - shift, off) and np.array_equal(vb2, vb)
    # values ascend by their bits taken as unsigned: +0.0 < positive < -0.0 < negative
    z = fm._from_rows("z", 4, [np.array([0]), np.array([1]), np.array([2]), np.array([3])], val=np.array([-1.0, -0.0, 1.0, 0.0]))
    assert em.dictionary(z)[1].view(np.float64).tolist() == [0.0, 1.0, -0.0, -1.0]
    assert np.signbit(em.dictionary(z)[1].view(np.float64)).tolist() == [False, False, True, True]


def test_pairs_by_bit_pattern():
    rows = [np.array([r]) for r in range(6)]
    zero = fm._from_rows("zero_sign", 6, rows, val=np.array([0.0, -0.0, 0.0, -0.0, 0.0, -0.0]))
    assert em.count_pairs(zero) == 2 and em.dictionary(zero)[0].tolist() == [0, 0]
    nans = fm._from_rows("nan_payload", 6, rows, val=np.array([em.nan_payload(1), em.nan_payload(2)] * 3))
    assert em.count_pairs(nans) == 2
    enc = em.encode(nans)
    assert em.verify(enc, nans) and enc["vbits"].tolist() == [0x7FF8000000000001, 0x7FF8000000000002]


def test_refusals():
    assert em.refusal(em.pairs_op("p255", 255)) is None
    assert em.refusal(em.pairs_op("p256", 256)) == "more than 255 pairs"
    p255 = em.pairs_op("p255", 255)
    enc = em.encode(p255)
    last = [c for c in em._row_codes(enc, p255.m - 1) if c != em.MARK]
    assert last[-1] == 254 and all(254 not in em._row_codes(enc, r) for r in range(p255.m - 1))
    assert em.refusal(em.with_palette(fm.get_op("row64"))) is None
    assert em.refusal(em.with_palette(fm.get_op("row65"))) == "a row of more than 64 entries"
    assert em.refusal(fm.get_op("ragged8")) == "more than 255 pairs"    # random values
    # one row of 32 among rows of 8 is too much padding for the copy with values, not for four code words per row ...
    assert em.refusal(em.with_palette(fm.get_op("pad_refused"))) is None
    # ... one row of 64 among rows of 1 is: 8 words per row against 9 * 127 + 256 bytes of CSR stream per slice
    skew = fm.sliced_op("pad_entries", [64] * 60, 70, lens_of=lambda s, i: 64 if i == 0 else 1)
    assert em.refusal(em.with_palette(skew)) == "too much padding"


@pytest.mark.parametrize("fault", ("wrong_code", "swapped_pair", "missing_mark"))
def test_injected_faults_are_rejected(fault):
    op = em.with_palette(fm.get_op("ragged8"))
    enc = em.encode(op)
    assert em.verify(enc, op)
    row = next(r for r in range(op.m) if 0 < op.lens[r] < 8)
    lay = enc["lay"]
    slot = em._slot(int(lay["off"][row >> 6]), 1, 0, row & 63)
    word = int(enc["words"][slot])
    if fault == "wrong_code":                                           # the first entry of the row names the neighbouring pair
        c = word & 0xFF
        enc["words"][slot] = np.uint64((word & ~0xFF) | (c + 1 if c + 1 < enc["off"].size else c - 1))
    elif fault == "swapped_pair":                                       # two pairs of the table change places
        enc["off"][[0, 1]], enc["vbits"][[0, 1]] = enc["off"][[1, 0]], enc["vbits"][[1, 0]]
    else:                                                               # the slot behind the row's last entry holds a code
        k = int(op.lens[row])
        enc["words"][slot] = np.uint64(word & ~(0xFF << (8 * k)))
    assert not em.verify(enc, op)
    if fault != "swapped_pair":
        assert not em.same_bits(em.product(enc, op.inputs()["x"]), op.inputs()["y"])
