"""Long-lived workgroups of the entry-coded sliced product (csrc/spmv.hip spmv_sell_persist_kernel, option spmv_sell_persist)
against the loop-free launch of the same handle (spmv_sell_persist = 0).

spmv_sell_persist = G > 1 launches exactly min(G, nvirt) workgroups, where nvirt is the number of workgroups of the loop-free
launch; workgroup b walks the virtual workgroups b, b + G, ...  The rows, the lanes, the arithmetic and the slots of the
fused-dot partials are those of the loop-free launch, so everything compared here is compared bit for bit: y (prefilled with
NaN), spmv_dot, both outputs of spmv_dot2, and x, the residual history and niter of six iterations of cg! and of minres!
(the Lanczos epilogue rides on the product).  y is also the serial stored-order product of tests/entry_codes_model.py.

G = 2: one workgroup walks many virtual ones; 3 and 7: nvirt is no multiple of G; 1000: more workgroups asked for than there
are virtual ones.  1 / 2 / 3 row blocks per virtual workgroup and both publish forms (the block publish alternates two LDS
regions across the publishes of one workgroup).  Every case runs under spmv_codes = 2, spmv_kernel = 4, spmv_sell_entries = 2.
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
# 20^3: 8000 rows = 31 blocks + 64 rows; 37^3: an odd tail; 27 entries per row: four code words (the walk inside a block)
OPERATORS = (("poisson", 20), ("poisson", 37), ("kron_unsymmetric", 12), ("stencil27", 9),
             ("uniform7_m193", None), ("uniform7_hole", None), ("ragged8", None))
GRIDS = (2, 3, 7, 1000)
TILES = (1, 2, 3)
PUBS = (0, 1)
_REF = {}                                     # (operator, tiles, pub) -> what spmv_sell_persist = 0 gives; computed once, never changed


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


def _operator(K, c, kind, n1):
    if n1 is not None:
        return em.stencil_op(kind, n1), K.CsrMatrix.stencil(c, kind, n1)
    op = em.with_palette(fm.get_op(kind))
    return op, K.CsrMatrix.from_host(c, op.rowptr, op.col, op.val, (op.m, op.n))


def _measure(K, c, A, op, x):
    """Everything that is compared, as bytes-comparable pieces."""
    dx = c.array(x)
    y0, y1, y2 = _nan(c, op.m), _nan(c, op.m), _nan(c, op.m)
    A.matvec(dx, y0)
    out = dict(y=y0.to_host(), dot=np.float64(K.spmv_dot(A, dx, y1)), dot2=np.array(K.spmv_dot2(A, dx, y2), dtype=np.float64),
               y_dot=y1.to_host(), y_dot2=y2.to_host())
    if op.m == op.n:
        for solver in (K.cg, K.minres):
            b = c.empty(op.m)
            K.kfill_(b, 1.0)
            xs, st, _ = solver(A, b, atol=0.0, rtol=0.0, itmax=6, history=True)
            out[solver.__name__] = (xs.to_host(), np.asarray(st.residuals, dtype=np.float64), st.niter)
    return out


def _same(got, want):
    for k in ("y", "y_dot", "y_dot2"):
        if not em.same_bits(got[k], want[k]):
            return k
    if got["dot"].tobytes() != want["dot"].tobytes():
        return "dot"
    if got["dot2"].tobytes() != want["dot2"].tobytes():
        return "dot2"
    for k in ("cg", "minres"):
        if k in want:
            if got[k][2] != want[k][2] or not em.same_bits(got[k][1], want[k][1]) or not em.same_bits(got[k][0], want[k][0]):
                return k
    return None


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("kind,n1", OPERATORS)
def test_bits_of_the_loop_free_launch(K, ent, kind, n1, grid):
    op, A = _operator(K, ent, kind, n1)
    assert em.refusal(op) is None
    inp = op.inputs()
    x = inp["x"]
    ent.set_option("spmv_sell_persist", 0)
    A.matvec(ent.array(x), _nan(ent, op.m))
    assert A.sell_entries == em.count_pairs(op) and tuple(A.sell_info) == em.sell_info(op)      # the entry-coded copy runs
    for tiles in TILES:
        for pub in PUBS:
            ent.set_option("spmv_tiles", tiles)
            ent.set_option("spmv_blk_pub", pub)
            key = (kind, n1, tiles, pub)
            if key not in _REF:
                ent.set_option("spmv_sell_persist", 0)
                _REF[key] = _measure(K, ent, A, op, x)
                assert em.same_bits(_REF[key]["y"], inp["y"]), key
            ent.set_option("spmv_sell_persist", grid)
            got = _measure(K, ent, A, op, x)
            assert em.same_bits(got["y"], inp["y"]), (key, grid)                                # the model's serial product
            bad = _same(got, _REF[key])
            assert bad is None, (key, grid, bad)


@pytest.mark.parametrize("world", (2, 3))
def test_row_partitioned(K, world):
    """In-process ranks: the two-range launch of the boundary rows (virtual workgroups on both sides of the hole) and the
    [owned | ghost] gather, with and without the overlap of the halo exchange."""
    n1 = 16
    op = em.stencil_op("poisson", n1)
    x = op.inputs()["x"]
    y_ref = op.inputs()["y"]
    starts = K.row_partition(op.m, world)

    def body(c, rank):
        r0, r1 = starts[rank], starts[rank + 1]
        for k, v in OPTS.items():
            c.set_option(k, v)
        c.set_option("overlap_halo", 1)
        A = K.CsrMatrix.stencil(c, "poisson", n1, rows=(r0, r1), distributed=True)
        dx = c.array(x[r0:r1])
        out = {}
        for persist in (0, 3):
            c.set_option("spmv_sell_persist", persist)
            res = []
            for overlap in (1, 0):
                c.set_option("overlap_halo", overlap)
                y = _nan(c, r1 - r0)
                A.matvec(dx, y)
                y2 = _nan(c, r1 - r0)
                res.append((y.to_host(), K.spmv_dot(A, dx, y2), y2.to_host()))
            out[persist] = dict(res=res, pairs=A.sell_entries)
        return out
    results = _run_ranks(K, world, 7950 + world, body)
    for rank, out in enumerate(results):
        r0, r1 = starts[rank], starts[rank + 1]
        assert out[3]["pairs"] >= 7, (rank, out[3]["pairs"])
        for (y, d, y2), (yv, dv, y2v) in zip(out[3]["res"], out[0]["res"]):
            assert em.same_bits(y, y_ref[r0:r1]) and em.same_bits(y2, y_ref[r0:r1]) and em.same_bits(yv, y) and em.same_bits(y2v, y2)
            assert np.float64(d).tobytes() == np.float64(dv).tobytes(), (rank, d, dv)
