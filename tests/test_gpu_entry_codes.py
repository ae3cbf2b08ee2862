"""The entry-coded sliced copy on the device (csrc/colcode.hip csr_build_sell_entries, spmv_sell_kernel's ENT arm) against
tests/entry_codes_model.py.

Every case runs on a fresh handle under spmv_codes = 2, spmv_kernel = 4, spmv_sell_entries = 2.  The form is asserted before any
number: sell_entries (the size of the dictionary), sell_info and spmv_bytes_stored against the model.  Then y, prefilled with NaN,
must be the serial stored-order product bit for bit (zero signs included; where values or x hold NaN, bit views everywhere but
at a NaN, which must face a NaN: entry_codes_model.same_bits_or_nan).  The
fused reductions, a short cg! and a short minres! must give the very bits of the same operator built with spmv_sell_entries = 0.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import entry_codes_model as em  # noqa: E402
import operator_forms_model as fm  # noqa: E402
from test_gpu_dist import _run_ranks  # noqa: E402  (the in-process rank harness)

pytestmark = pytest.mark.gpu

OPTS = dict(spmv_codes=2, spmv_kernel=4, spmv_sell_entries=2)
KEYS = tuple(OPTS) + ("spmv_tiles", "spmv_blk_pub", "overlap_halo")
STENCILS = (("poisson", 20), ("poisson", 37), ("kron_unsymmetric", 12), ("stencil27", 9))
STRUCTURES = ("ragged8", "ragged64", "uniform9_hole", "uniform7_hole", "uniform7_m192", "uniform7_m193", "uniform7_m40", "row64")


@pytest.fixture
def ent(ctx):
    saved = {k: ctx.get_option(k) for k in KEYS}
    for k, v in OPTS.items():
        ctx.set_option(k, v)
    yield ctx
    for k, v in saved.items():
        ctx.set_option(k, v)


def _nan(c, m):
    return c.array(np.full(m, np.nan))


def _handle(K, c, op):
    return K.CsrMatrix.from_host(c, op.rowptr, op.col, op.val, (op.m, op.n))


def _assert_form(A, op):
    """After the first product: the entry-coded copy, the size the model gives, the bytes the model gives."""
    assert A.sell_entries == em.count_pairs(op), (op.name, A.sell_entries, em.count_pairs(op))
    assert tuple(A.sell_info) == em.sell_info(op), (op.name, A.sell_info, em.sell_info(op))
    assert A.spmv_bytes_stored == em.bytes_stored(op), (op.name, A.spmv_bytes_stored, em.bytes_stored(op))
    assert not A.sell_narrow and A.code_info[0] == 8


def _check_products(c, A, op, form=_assert_form):
    inp = op.inputs()
    assert A.sell_entries == 0 and tuple(A.sell_info) == (0, 0, 0)          # nothing is built before the first product
    y = A.matvec(c.array(inp["x"]), _nan(c, op.m)).to_host()
    form(A, op)
    same = em.same_bits if np.isfinite(op.val).all() else em.same_bits_or_nan      # NaN values: a NaN faces a NaN, all else by bits
    assert same(y, inp["y"]), op.name
    ys = A.matvec(c.array(inp["xs"]), _nan(c, op.m)).to_host()             # +Inf, NaN, -0.0 and a subnormal in x
    assert em.same_bits_or_nan(ys, inp["ys"]), op.name
    assert same(A.matvec(c.array(inp["x"]), _nan(c, op.m)).to_host(), inp["y"])      # the cached copy
    form(A, op)


@pytest.mark.parametrize("kind,n1", STENCILS)
def test_stencils(K, ent, kind, n1):
    op = em.stencil_op(kind, n1)
    assert em.refusal(op) is None
    A = K.CsrMatrix.stencil(ent, kind, n1)
    assert (A.m, A.nnz) == (op.m, op.nnz)
    _check_products(ent, A, op)
    if kind == "stencil27":
        assert A.sell_info[1] == 4                                          # 27 entries per row: four words, two 16-byte pairs


@pytest.mark.parametrize("name", STRUCTURES)
def test_layouts(K, ent, name):
    """L = 1 .. 8 and 1 .. 64 per slice (offsets), the first two-word row (L = 9), an all-empty slice inside a uniform layout, empty
    rows, m = 40 / 192 / 193, a row of 64 entries."""
    op = em.with_palette(fm.get_op(name))
    assert em.refusal(op) is None
    _check_products(ent, _handle(K, ent, op), op)
    nf = em.with_palette(fm.get_op(name)).nonfinite()                       # +Inf / -Inf / NaN values: more pairs, y as bit views
    assert em.refusal(nf) is None and em.count_pairs(nf) > em.count_pairs(op)
    _check_products(ent, _handle(K, ent, nf), nf)


def _fallback_form(want_sell):
    def form(A, op):
        assert A.sell_entries == 0 and A.code_info[0] == 8
        assert (A.sell_info[0] == 1) == want_sell, A.sell_info
    return form


def test_dictionary_edges(K, ent):
    p255 = em.pairs_op("pairs255", 255)                                     # 255 pairs: admitted; code 254 in the last row alone
    _check_products(ent, _handle(K, ent, p255), p255)
    p256 = em.pairs_op("pairs256", 256)                                     # 256 pairs: refused, today's sliced copy, the same y
    assert em.refusal(p256) == "more than 255 pairs"
    _check_products(ent, _handle(K, ent, p256), p256, _fallback_form(True))
    r65 = em.with_palette(fm.get_op("row65"))                               # a row of 65 entries: no sliced copy at all
    assert em.refusal(r65) == "a row of more than 64 entries"
    _check_products(ent, _handle(K, ent, r65), r65, _fallback_form(False))
    rnd = fm.get_op("ragged8")                                              # random values: far more than 255 of them
    _check_products(ent, _handle(K, ent, rnd), rnd, _fallback_form(True))
    rows = [np.array([r, r + 1]) for r in range(70)]
    zero = fm._from_rows("zero_sign", 71, rows, val=np.tile([0.0, -0.0, -0.0, 0.0], 35))
    assert em.count_pairs(zero) == 4                                        # (0, +0), (0, -0), (1, +0), (1, -0)
    _check_products(ent, _handle(K, ent, zero), zero)
    nans = fm._from_rows("nan_payload", 71, rows, val=np.tile([em.nan_payload(1), 2.0, em.nan_payload(2), 2.0], 35))
    assert em.count_pairs(nans) == 3
    _check_products(ent, _handle(K, ent, nans), nans)
    ones = fm._from_rows("all_ones", 71, rows, val=np.tile(np.array([~np.uint64(0), 1], dtype=np.uint64).view(np.float64), 70))
    assert em.count_pairs(ones) == 2                                        # the pattern the value set uses for an empty slot
    _check_products(ent, _handle(K, ent, ones), ones)


@pytest.mark.parametrize("kind,n1", STENCILS)
def test_fused_reductions_and_solves_match_the_copy_with_values(K, ent, kind, n1):
    """1 / 2 / 3 row blocks per workgroup, both publish forms: spmv_dot and spmv_dot2, then cg! and minres!, bit for bit what the
    same operator gives with spmv_sell_entries = 0."""
    op = em.stencil_op(kind, n1)
    x = op.inputs()["x"]
    E = K.CsrMatrix.stencil(ent, kind, n1)
    E.matvec(ent.array(x), _nan(ent, op.m))
    _assert_form(E, op)
    ent.set_option("spmv_sell_entries", 0)
    V = K.CsrMatrix.stencil(ent, kind, n1)
    V.matvec(ent.array(x), _nan(ent, op.m))
    assert V.sell_entries == 0 and V.sell_info[0] == 1 and E.sell_entries == em.count_pairs(op)
    dx = ent.array(x)
    for tiles in (1, 2, 3):
        for blk in (0, 1):
            ent.set_option("spmv_tiles", tiles); ent.set_option("spmv_blk_pub", blk)
            got, want = [], []
            for A, out in ((E, got), (V, want)):
                y1, y2 = _nan(ent, op.m), _nan(ent, op.m)
                out += [K.spmv_dot(A, dx, y1), *K.spmv_dot2(A, dx, y2), y1.to_host(), y2.to_host()]
            assert np.array([got[:3]]).tobytes() == np.array([want[:3]]).tobytes(), (kind, n1, tiles, blk, got[:3], want[:3])
            assert em.same_bits(got[3], want[3]) and em.same_bits(got[4], want[4]) and em.same_bits(got[3], op.inputs()["y"])
            for solver in (K.cg, K.minres):
                res = []
                for A in (E, V):
                    b = ent.empty(op.m); K.kfill_(b, 1.0)
                    xs, st, _ = solver(A, b, atol=0.0, rtol=0.0, itmax=6, history=True)
                    res.append((xs.to_host(), np.asarray(st.residuals), st.niter))
                assert res[0][2] == res[1][2] and em.same_bits(res[0][1], res[1][1]) and em.same_bits(res[0][0], res[1][0]), \
                    (kind, n1, tiles, blk, solver.__name__)


@pytest.mark.parametrize("world", (2, 3))
def test_row_partitioned(K, world):
    """In-process ranks: the two-range launch of the boundary rows and the [owned | ghost] gather on entry-coded slabs."""
    n1 = 16
    op = em.stencil_op("poisson", n1)
    x = op.inputs()["x"]
    y_ref = op.inputs()["y"]
    starts = K.row_partition(op.m, world)

    def body(c, rank):
        r0, r1 = starts[rank], starts[rank + 1]
        out = {}
        for k, v in OPTS.items():
            c.set_option(k, v)
        for entries in (2, 0):
            c.set_option("spmv_sell_entries", entries)
            c.set_option("overlap_halo", 1)
            A = K.CsrMatrix.stencil(c, "poisson", n1, rows=(r0, r1), distributed=True)
            dx = c.array(x[r0:r1])
            res = []
            for overlap in (1, 0):
                c.set_option("overlap_halo", overlap)
                y = _nan(c, r1 - r0)
                A.matvec(dx, y)
                y2 = _nan(c, r1 - r0)
                res.append((y.to_host(), K.spmv_dot(A, dx, y2), y2.to_host()))
            out[entries] = dict(res=res, pairs=A.sell_entries, sell=tuple(A.sell_info))
        return out
    results = _run_ranks(K, world, 7900 + world, body)
    for rank, out in enumerate(results):
        r0, r1 = starts[rank], starts[rank + 1]
        assert out[2]["pairs"] >= 7 and out[2]["sell"][0] == 1 and out[0]["pairs"] == 0 and out[0]["sell"][0] == 1, (rank, out[2], out[0])
        for (y, d, y2), (yv, dv, y2v) in zip(out[2]["res"], out[0]["res"]):
            assert em.same_bits(y, y_ref[r0:r1]) and em.same_bits(y2, y_ref[r0:r1]) and em.same_bits(yv, y) and em.same_bits(y2v, y2)
            assert np.float64(d).tobytes() == np.float64(dv).tobytes(), (rank, d, dv)


@pytest.mark.parametrize("n1,want", ((84, False), (85, True)))
def test_default_size_rule(K, ent, oracle, n1, want):
    """spmv_sell_entries = 1: handles of at least 2^22 entries (7-point 85^3: 4,255,525; 84^3: 4,106,592 stays on the copy with values)."""
    ent.set_option("spmv_sell_entries", 1)
    ref = oracle.poisson3d(n1)
    assert (ref.nnz >= em.BIG_NNZ) == want
    A = K.CsrMatrix.stencil(ent, "poisson", n1)
    x = np.linspace(-1.0, 1.0, ref.n) ** 3 + 0.125
    y = A.matvec(ent.array(x), _nan(ent, ref.n)).to_host()
    assert A.sell_entries == (7 if want else 0) and A.sell_info[0] == 1
    if want:
        assert tuple(A.sell_info) == (1, 1, (ref.n + 63) // 64)
    assert em.same_bits(y, ref.matvec(x))
