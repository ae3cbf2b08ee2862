"""The ILU(0) factorisation and solves of csrc/ilu.hip against the oracle's serial loops, bit for bit, on EVERY kernel path.

tests/test_gpu_ilu.py compares operator families; here each operator of tests/ilu_model.py exists for one path of the block
schedule -- the 48-byte records, the 176-byte records (because of the rows, or only because of the face list), the packed
lists with rows beyond 16 entries and face lists beyond 1024 rows, level-sequence blocks at their caps of 64 rows, 512 rows and
48 levels, partial and degenerate grid cubes, the fall-back to level scheduling when a block does not fit LDS, the batching
thresholds of the level schedule -- and Ilu0.path_info() asserts that the path really ran.  Option ilu_grid caps the
workgroups of the persistent launch at 1 and 3, so that a workgroup takes many blocks in sequence: LDS reuse, the constant
0.0 and dump slots written again, fast and packed blocks in turn, tickets drawn past the last block.
Right-hand sides: seeded normal, all -0.0, the specials (Inf, -Inf, NaN, -0.0, a subnormal, +-1e200 side by side), finite
extremes, and a single +Inf.  same_bits: NaN exactly where the oracle has NaN, the same 64 bits everywhere else.
tests/test_ilu_model_host.py pins the oracle to exact arithmetic and shows that this comparison rejects injected faults."""
import numpy as np
import pytest

import ilu_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def refs(oracle):
    """name -> (operator, oracle factors, {input: oracle y}); computed once, shared by every schedule, never written to."""
    cache = {}

    def get(name, A=None, kinds=None):
        if name not in cache:
            A = M.family(name) if A is None else A
            ref = oracle.Ilu0(oracle.CsrMatrix.from_arrays(A.rowptr, A.col, A.val))
            xs = M.inputs(name.split(":")[0])
            want = {k: ref.solve(x) for k, x in xs.items() if kinds is None or k in kinds}
            for v in want.values():
                v.setflags(write=False)
            cache[name] = (A, ref.lu, want)
        return cache[name]
    return get


def _create(K, ctx, A, ilu_blocks, ilu_grid):
    dA = K.CsrMatrix.from_host(ctx, A.rowptr, A.col, A.val, (A.n, A.n))
    ctx.set_option("ilu_blocks", ilu_blocks)
    ctx.set_option("ilu_grid", ilu_grid)
    try:
        return K.Ilu0(dA)
    finally:
        ctx.set_option("ilu_blocks", 1)
        ctx.set_option("ilu_grid", 0)


def _check_paths(K, name, A, P, ilu_blocks, ilu_grid):
    r = P.path_info()
    M.expect_paths(name, ilu_blocks, r)
    host = K.ilu_paths_host(A.rowptr, A.col, ilu_blocks)          # the device ran what the host analysis predicts
    for tri in ("lower", "upper"):
        assert {k: v for k, v in r[tri].items() if k != "workgroups"} == {k: v for k, v in host[tri].items() if k != "workgroups"}
    assert r["levels"] == host["levels"] and r["nlevels"] == host["nlevels"] == P.levels
    dims, nb, failed = P.block_info()
    assert failed == 0
    if r["blocks_in_use"]:
        assert nb == r["lower"]["blocks"] and dims == (M.family_dims(name) if ilu_blocks != 3 else (0, 0, 0))
        for tri in ("lower", "upper"):
            wg, blocks = r[tri]["workgroups"], r[tri]["blocks"]
            assert 1 <= wg <= blocks
            if ilu_grid:
                assert wg == min(ilu_grid, blocks) and blocks > wg          # every workgroup takes more than one block
    else:
        assert nb == 0 and dims == (0, 0, 0) and r["lower"]["workgroups"] == 0
    return r


def _check_solves(ctx, P, xs, want):
    n = next(iter(xs.values())).size
    dy = ctx.empty(n)
    for kind, y_ref in want.items():
        dx = ctx.array(xs[kind])
        for again in range(2):                     # twice: the epochs and the ticket base move on
            P(dx, dy)
            assert M.same_bits(dy.to_host(), y_ref), (kind, again)
    assert P.block_info()[2] == 0


CASES = [(name, b, g) for name in M.FAMILIES for b, g in M.schedules(name)]


@pytest.mark.parametrize("name,ilu_blocks,ilu_grid", CASES, ids=["%s-b%d-g%d" % c for c in CASES])
def test_family_bit_identical_on_its_path(K, ctx, refs, parity_log, name, ilu_blocks, ilu_grid):
    """Factors and solves equal the oracle's under same_bits, and path_info() shows the path the family exists for (ilu_model.
    expect_paths; tests/test_ilu_model_host.py checks the same expectations on the host analysis)."""
    A, lu, want = refs(name)
    P = _create(K, ctx, A, ilu_blocks, ilu_grid)
    r = _check_paths(K, name, A, P, ilu_blocks, ilu_grid)
    parity_log(test="ilu_exact_paths", family=name, ilu_blocks=ilu_blocks, ilu_grid=ilu_grid, lower=r["lower"], upper=r["upper"],
               levels=r["levels"], blocks_in_use=r["blocks_in_use"], fallback=r["fallback"])
    assert np.array_equal(P.values(), lu) and M.same_bits(P.values(), lu)
    assert np.isfinite(want["normal"]).all() and np.isnan(want["specials"]).any()
    if name in M.SPECIALS_STAY_NARROW:            # the specials hide no more than half of y
        assert np.isfinite(want["specials"]).mean() >= 0.5
    _check_solves(ctx, P, M.inputs(name), want)


STORED_ZERO_CASES = [(name, b, g) for name in M.STORED_ZERO_FAMILIES for b, g in M.schedules(name) if g in (0, 1)]


@pytest.mark.parametrize("name,ilu_blocks,ilu_grid", STORED_ZERO_CASES, ids=["%s-b%d-g%d" % c for c in STORED_ZERO_CASES])
def test_stored_zeros_times_inf_are_nan(K, ctx, refs, name, ilu_blocks, ilu_grid):
    """A stored 0.0 is an entry like any other: the rows that multiply it by an Inf come out NaN, as the oracle says (the record
    paths multiply absent entries by a constant 0.0 slot and must not confuse the two; the packed path selects)."""
    A0, nan_rows = M.stored_zeros(name)
    A, lu, want = refs(name + ":zeros", A0)
    assert (lu == 0.0).sum() == 3
    for kind, rows in nan_rows.items():
        assert np.isnan(want[kind][rows]).all()
    P = _create(K, ctx, A, ilu_blocks, ilu_grid)
    _check_paths(K, name, A, P, ilu_blocks, ilu_grid)
    assert M.same_bits(P.values(), lu)
    _check_solves(ctx, P, M.inputs(name), want)


@pytest.mark.parametrize("name", ["rows512", "box30x7x20"])
@pytest.mark.parametrize("ilu_blocks", [1, 0])
def test_nan_matrix_value_spreads_as_in_the_oracle(K, ctx, refs, name, ilu_blocks):
    """A NaN in one off-diagonal value: both implementations test `pivot == 0.0`, which a NaN passes, so the factorisation goes
    through and the factors equal the oracle's -- NaN in the same positions, the same bits elsewhere."""
    A = M.family(name)
    rows = np.repeat(np.arange(A.n), np.diff(A.rowptr))
    q = int(np.flatnonzero((rows == A.n // 2) & (A.col < rows))[0])
    A, lu, want = refs(name + ":nan", M.with_values(A, [q], np.nan), kinds=("normal",))
    assert 0 < np.isnan(lu).sum() < lu.size // 2
    P = _create(K, ctx, A, ilu_blocks, 0)
    assert M.same_bits(P.values(), lu)
    _check_solves(ctx, P, M.inputs(name), want)
