"""The entry-coded row step with one wait per phase (csrc/spmv.hip ent_step, spmv_sell_persist_kernel's ONE arm).

The step looks all eight values of a code word up unconditionally (an absent entry, code 0xFF, reads slot 255 of the table, which is
zero) and skips an absent entry by a select; the ONE arm walks a row block outside its `row >= 0` guard (a lane without a row walks
eight absent entries) and loads the fused dot's weight beside the next block's code word.  What that can newly break, and nothing
else, is checked here, bit for bit:

* absent slots in every position, empty rows, and +Inf, -Inf, NaN and -0.0 in x at columns that some rows reference and others do
  not: an absent slot must contribute nothing (no 0 * Inf, no Inf - Inf), so a row that references no special column is finite and
  an empty row is +0.0;
* the ends of the walk: y does not depend on the dot's weight, the fused dots and minres!'s Lanczos epilogue do -- a weight of
  the wrong block or of a lane without a row (across virtual workgroups, behind the last block, in a partial block) shows only there;
* the two-range launch of a row-partitioned product: blocks on both sides of the hole.

References: the serial stored-order model of tests/entry_codes_model.py for y, the loop-free launch of the same handle
(spmv_sell_persist = 0) for everything.  Every case runs under spmv_codes = 2, spmv_kernel = 4, spmv_sell_entries = 2.
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
KEYS = tuple(OPTS) + ("spmv_tiles", "spmv_blk_pub", "spmv_sell_persist")


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


# ---------------------------------------------------------------------------------------------------- absent slots, special values

M_RAGGED, SHIFT = 193, 8
OFFSETS = np.array([2, -5, 7, 0, -8, 4, -1, -3])      # stored order, unsorted: the row's neighbourhood
VALUES = np.array([1.5, -2.0, 0.375])
SPECIAL = {30: -0.0, 60: np.inf, 100: -np.inf, 140: np.nan}


def _ragged():
    """193 rows, row i holds i mod 9 entries: every slot position is absent in some row, rows 0, 9, 18, ... are empty."""
    rows = [i + SHIFT + OFFSETS[:i % 9] for i in range(M_RAGGED)]
    val = np.concatenate([VALUES[(i + np.arange(i % 9)) % 3] for i in range(M_RAGGED)])
    return fm._from_rows("ragged_0to8_m193", M_RAGGED + 2 * SHIFT, rows, val=val)


def test_absent_slots_and_special_values(K, ent):
    op = _ragged()
    assert em.refusal(op) is None and sorted(set(op.lens.tolist())) == list(range(9))
    rng = np.random.default_rng(193)
    x = rng.uniform(-2.0, 2.0, op.n)
    for c, v in SPECIAL.items():
        x[c] = v
    touched = np.zeros(op.m, dtype=bool)          # rows that reference +-Inf or NaN
    for c, v in SPECIAL.items():
        refs = np.zeros(op.m, dtype=bool)
        refs[op.row_of[op.col == c]] = True
        assert refs.any() and not refs[op.lens > 0].all(), c      # some rows reference the column and others do not
        if not np.isfinite(v):
            touched |= refs
    enc = em.encode(op)
    assert em.verify(enc, op)
    y_model = em.product(enc, x)
    assert em.same_bits_or_nan(y_model, op.serial(x))
    assert touched.any() and np.isfinite(y_model[~touched]).all() and not np.isfinite(y_model[touched]).any()
    A = K.CsrMatrix.from_host(ent, op.rowptr, op.col, op.val, (op.m, op.n))
    dx = ent.array(x)
    ent.set_option("spmv_sell_persist", 0)
    y0 = _nan(ent, op.m)
    A.matvec(dx, y0)
    assert A.sell_entries == em.count_pairs(op) and tuple(A.sell_info) == em.sell_info(op)      # the entry-coded copy runs
    assert tuple(A.sell_info)[1] == 1                             # one code word per row: the persistent launch takes the ONE arm
    y_free = y0.to_host()
    # the model runs on the host: a NaN must face a NaN, its sign is the processor's choice (em.same_bits_or_nan)
    assert em.same_bits_or_nan(y_free, y_model)
    for grid in (2, 3):
        ent.set_option("spmv_sell_persist", grid)
        yd = _nan(ent, op.m)
        A.matvec(dx, yd)
        y = yd.to_host()
        assert em.same_bits_or_nan(y, y_model), grid
        assert em.same_bits(y, y_free), grid                      # the same processor: NaNs bit for bit too
        assert np.isfinite(y[~touched]).all(), (grid, np.flatnonzero(~np.isfinite(y) & ~touched))
        empty = np.flatnonzero(op.lens == 0)
        assert empty.size == 22 and not em.bits(y[empty]).any(), grid      # +0.0, not -0.0 and not what y held


# ---------------------------------------------------------------------------------------------------- ends of the walk

SIZES = (1, 63, 64, 65, 255, 256, 257, 513)
GRIDS = (2, 3, 7)
TILES = (1, 2, 3)
PUBS = (0, 1)
BAND = {0: 6.0, 1: -1.0, 2: 0.5, 3: -0.25}      # by |offset|: symmetric and diagonally dominant


def _uniform7(m):
    """m x m, every row holds seven entries, columns (row + d) mod m for d = -3 .. 3 (repeated columns where m < 7)."""
    d = np.arange(-3, 4)
    rows = [(r + d) % m for r in range(m)]
    val = np.tile(np.array([BAND[abs(int(k))] for k in d]), m)
    return fm._from_rows("uniform7_wrap_m%d" % m, m, rows, val=val)


def _measure(K, c, A, op, x):
    dx = c.array(x)
    y0, y1, y2 = _nan(c, op.m), _nan(c, op.m), _nan(c, op.m)
    A.matvec(dx, y0)
    out = dict(y=y0.to_host(), dot=np.float64(K.spmv_dot(A, dx, y1)), dot2=np.array(K.spmv_dot2(A, dx, y2), dtype=np.float64),
               y_dot=y1.to_host(), y_dot2=y2.to_host())
    b = c.array(1.0 + 0.5 * np.cos(np.arange(op.m)))
    xs, st, _ = K.minres(A, b, atol=0.0, rtol=0.0, itmax=6, history=True)
    out["minres"] = (xs.to_host(), np.asarray(st.residuals, dtype=np.float64), st.niter)
    return out


def _differs(got, want):
    for k in ("y", "y_dot", "y_dot2"):
        if not em.same_bits(got[k], want[k]):
            return k
    for k in ("dot", "dot2"):
        if got[k].tobytes() != want[k].tobytes():
            return k
    g, w = got["minres"], want["minres"]
    if g[2] != w[2] or not em.same_bits(g[1], w[1]) or not em.same_bits(g[0], w[0]):
        return "minres"
    return None


@pytest.mark.parametrize("m", SIZES)
def test_ends_of_the_walk(K, ent, m):
    op = _uniform7(m)
    assert em.refusal(op) is None and (op.lens == 7).all()
    x = np.random.default_rng(m).uniform(-2.0, 2.0, op.n)      # no two rows weigh alike: a weight of another block changes the dot
    y_model = em.product(em.encode(op), x)
    A = K.CsrMatrix.from_host(ent, op.rowptr, op.col, op.val, (op.m, op.n))
    ent.set_option("spmv_sell_persist", 0)
    A.matvec(ent.array(x), _nan(ent, op.m))
    assert A.sell_entries == em.count_pairs(op) and tuple(A.sell_info) == em.sell_info(op)      # the entry-coded copy, one word per row
    assert tuple(A.sell_info)[1] == 1
    for tiles in TILES:
        for pub in PUBS:
            ent.set_option("spmv_tiles", tiles)
            ent.set_option("spmv_blk_pub", pub)
            ent.set_option("spmv_sell_persist", 0)
            want = _measure(K, ent, A, op, x)
            assert em.same_bits(want["y"], y_model), (m, tiles, pub)
            for grid in GRIDS:
                ent.set_option("spmv_sell_persist", grid)
                got = _measure(K, ent, A, op, x)
                assert em.same_bits(got["y"], y_model), (m, tiles, pub, grid)
                bad = _differs(got, want)
                assert bad is None, (m, tiles, pub, grid, bad)


# ---------------------------------------------------------------------------------------------------- two-range launch

@pytest.mark.parametrize("world", (2, 3))
def test_two_range_launch_dots(K, world):
    """In-process ranks as tests/test_gpu_sell_persist.py test_row_partitioned sets them up: the boundary rows of a rank are one
    launch over two ranges, with blocks on both sides of the hole.  The dots, and not only y, against spmv_sell_persist = 0."""
    n1 = 16
    op = em.stencil_op("poisson", n1)
    x = np.random.default_rng(16).uniform(-2.0, 2.0, op.n)
    y_ref = op.serial(x)
    starts = K.row_partition(op.m, world)

    def body(c, rank):
        r0, r1 = starts[rank], starts[rank + 1]
        for k, v in OPTS.items():
            c.set_option(k, v)
        A = K.CsrMatrix.stencil(c, "poisson", n1, rows=(r0, r1), distributed=True)
        dx = c.array(x[r0:r1])
        out = {}
        for persist in (0, 2, 3):
            c.set_option("spmv_sell_persist", persist)
            res = []
            for overlap in (1, 0):
                c.set_option("overlap_halo", overlap)
                y, y1, y2 = _nan(c, r1 - r0), _nan(c, r1 - r0), _nan(c, r1 - r0)
                A.matvec(dx, y)
                d = np.float64(K.spmv_dot(A, dx, y1))
                d2 = np.array(K.spmv_dot2(A, dx, y2), dtype=np.float64)
                res.append((y.to_host(), y1.to_host(), y2.to_host(), d, d2))
            out[persist] = dict(res=res, pairs=A.sell_entries)
        return out
    results = _run_ranks(K, world, 7970 + world, body)
    for rank, out in enumerate(results):
        r0, r1 = starts[rank], starts[rank + 1]
        for persist in (2, 3):
            assert out[persist]["pairs"] >= 7, (rank, out[persist]["pairs"])
            for got, want in zip(out[persist]["res"], out[0]["res"]):
                for k in range(3):
                    assert em.same_bits(got[k], y_ref[r0:r1]) and em.same_bits(got[k], want[k]), (rank, persist, k)
                assert got[3].tobytes() == want[3].tobytes(), (rank, persist, got[3], want[3])
                assert got[4].tobytes() == want[4].tobytes(), (rank, persist, got[4], want[4])
