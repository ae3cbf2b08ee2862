"""The SpMM kernels' persistent loops and tile records against the serial product (tests/spmm_model.py).

One test id per case of the model's table.  Every case runs on a fresh handle under its own option set (restored in a finally)
and asserts khip_test_optional_build_failures == 0.  Order inside a case: the first product; the build outcome
(khip_test_csr_tile_records, khip_test_csr_window_info) equals the model's -- a predicted refusal is an asserted outcome and the
fallback kernel is then judged, never a skip; the record checker on the raw record bytes; what the product launched
(khip_test_spmm_last_launch) equals the model's launch decision, the forced grid included; only then the numbers.  The judge:
Y's whole buffer is written beforehand (NaN in the rows < m, +0.0 in the padding rows) and read back raw; rows < m equal the
serial stored-order product bit for bit (NaN for NaN, the sign of a zero included), the padding rows are still +0.0, the NaN in
X's own padding rows does not leak -- for a finite X, an X with +Inf / NaN / -0.0 / subnormals, a second product on the cached
records, and on a second handle of the same structure with +Inf / -Inf / NaN VALUES at the last entries of rows, after short
rows, at entry 32 of 32-entry rows and at the end of the matrix.  No bound is measured here; forms and seconds go to parity_log.
"""
import ctypes
import os
import sys
import threading
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spmm_model as sm  # noqa: E402

pytestmark = pytest.mark.gpu


def _product(K, ctx, A, op, X):
    """X: the rows of the panel this handle's context owns (all of them without a partition).  Returns Y's raw buffer."""
    dX = K.Panel.from_raw_buffer(ctx, X.shape[0], sm.x_buffer(X))
    dY = K.Panel.from_raw_buffer(ctx, op.m, sm.y_prefill(op.m, X.shape[1]))
    K.spmm_(A, dX, dY)
    return dY.buf.to_host()


def _observe(K, ctx, op, case, what, first_only=False):
    """First product -> build outcome -> records -> launch, asserted in that order; returns the raw Y buffers."""
    opts, p = case.options, case.p
    A = K.CsrMatrix.from_host(ctx, op.rowptr, op.col, op.val, (op.m, op.n))
    assert (A.m, A.n, A.nnz) == (op.m, op.n, op.nnz)
    assert A.tile_records()["state"] == 0 and A.window_info[0] == 0, "%s: built before the first product" % what
    X, Xs = sm.inputs(op, p)
    ys = [_product(K, ctx, A, op, X)]
    got = A.tile_records()
    planes = (got["line_rows"], got["plane_rows"])
    assert planes == op.planes(), "%s: csr_finalize reports planes %r, the model %r" % (what, planes, op.planes())
    want_ln = sm.launch(op, opts, p)
    assert want_ln["error"] is None
    if want_ln["tile_built"]:
        want_b = sm.tile_build(op, opts)
        bad = sm.build_failures(want_b, got)
        assert not bad, (what, bad)
        if want_b["state"] == 1:
            bad = sm.check_records(op, got["meta"], got["cap"], got["run_len"], got["direct_list"])
            assert not bad, (what, bad)
    else:
        assert got["state"] == 0, (what, "tile records were built for a product that does not ask for them")
    if want_ln["win_L"]:
        wb = sm.window_build(op, abs(want_ln["win_L"]))
        assert A.window_info == (wb["win_L"], wb["groups"], wb["flagged"]), (what, A.window_info, wb["win_L"], wb["groups"], wb["flagged"])
    else:
        assert A.window_info[0] == 0, (what, A.window_info)
    ln = ctx.spmm_last_launch()
    bad = sm.launch_failures(want_ln, ln)
    assert not bad, (what, bad)
    if not first_only:
        ys.append(_product(K, ctx, A, op, Xs))
        ys.append(_product(K, ctx, A, op, X))                            # a second product on the cached records
        again = ctx.spmm_last_launch()
        assert not sm.launch_failures(want_ln, again) and again["grid"] == ln["grid"], (what, again)
        after = A.tile_records()
        assert np.array_equal(after["meta"], got["meta"]) and after["state"] == got["state"], "%s: the records changed between products" % what
    return ln, (X, Xs), ys


def _run_case(K, ctx, case):
    op = sm.get_op(case.op)
    for k in sm.OPTION_KEYS:
        ctx.set_option(k, case.options[k])
    ln, (X, Xs), ys = _observe(K, ctx, op, case, "A")
    nf = sm.nonfinite_values(op)
    ln_nf, _, ys_nf = _observe(K, ctx, nf, case, "A with Inf / NaN values", first_only=True)
    assert sm.form_name(ln_nf) == sm.form_name(ln)
    fails = []
    fails += sm.judge_y(op, X, ys[0], "finite X")
    fails += sm.judge_y(op, Xs, ys[1], "X with Inf / NaN / -0.0 / subnormals")
    fails += sm.judge_y(op, X, ys[2], "second product")
    fails += sm.judge_y(nf, X, ys_nf[0], "Inf / NaN values")
    return ln, fails


def _check(K, ctx, parity_log, case):
    t0 = time.time()
    saved = {k: ctx.get_option(k) for k in sm.OPTION_KEYS}
    try:
        ln, fails = _run_case(K, ctx, case)
    finally:
        for k, v in saved.items():
            ctx.set_option(k, v)
    cnt = ctypes.c_int(-1)
    assert K.lib().khip_test_optional_build_failures(ctypes.byref(cnt)) == 0 and cnt.value == 0, cnt.value
    parity_log(test="spmm_exact", group=case.group, case=case.name, form=sm.form_name(ln), grid=ln["grid"], NL=ln["NL"], L=ln["L"],
               launches=ln["launches"], direct=ln["direct"], seconds=round(time.time() - t0, 3))
    assert not fails, fails


# ---- row slabs on in-process ranks (the DIST instantiations) ---------------------------------------------------------------
def _run_ranks(K, world, hub_id, body):
    results, errors = [None] * world, []

    def worker(rank):
        try:
            c = K.Context(0)
            c.comm_init_local(rank, world, hub_id)
            results[rank] = body(c, rank)
            c.barrier()
            c.close()
        except Exception as e:  # pragma: no cover
            import traceback
            errors.append(f"rank {rank}: {e}\n{traceback.format_exc()}")
    ts = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=120)
    assert not errors, errors
    assert all(not t.is_alive() for t in ts), "a rank is stuck (collective mismatch)"
    return results


def _check_dist(K, parity_log, case):
    """Every rank runs the same sequence of products (they are collectives) and only records; the order form -> records -> launch
    -> numbers is kept by the judge below, rank by rank."""
    t0 = time.time()
    world, p, opts = case.want["world"], case.p, case.options
    glob = sm.get_op(case.op)
    slabs = sm.case_slabs(case)
    X, Xs = sm.inputs(glob, p)

    def body(c, rank):
        for k in sm.OPTION_KEYS:
            c.set_option(k, opts[k])
        c.set_option("halo_mode", 1)                                     # neighbour exchange: ghost rows behind the owned ones
        out = {}
        for tag, slab in (("A", slabs[rank]), ("N", sm.nonfinite_values(slabs[rank]))):
            A = K.CsrMatrix.from_host(c, slab.rowptr, slab.global_cols, slab.val, (slab.m, slab.n_global),
                                      dist_rows=(slab.r0, slab.r0 + slab.m), n_global=slab.n_global)
            o = out[tag] = dict(cols=A.to_host_arrays()[1], before=(A.tile_records()["state"], A.window_info[0]), y=[])
            for i, xx in enumerate((X, Xs, X) if tag == "A" else (X,)):
                o["y"].append(_product(K, c, A, slab, xx[slab.r0:slab.r0 + slab.m]))
                if i == 0:
                    o["records"], o["window"], o["launch"] = A.tile_records(), A.window_info, c.spmm_last_launch()
            o["launch_last"], o["records_last"] = c.spmm_last_launch(), A.tile_records()
        return out

    res = _run_ranks(K, world, 616100 + sum(map(ord, case.name)), body)
    cnt = ctypes.c_int(-1)
    assert K.lib().khip_test_optional_build_failures(ctypes.byref(cnt)) == 0 and cnt.value == 0, cnt.value
    fails, forms = [], []
    for rank, out in enumerate(res):
        for tag, slab in (("A", slabs[rank]), ("N", sm.nonfinite_values(slabs[rank]))):
            o, what = out[tag], "rank %d %s" % (rank, tag)
            assert np.array_equal(o["cols"], slab.col), "%s: the handle's columns are not [owned | ghosts ascending]" % what
            assert o["before"] == (0, 0), "%s: built before the first product" % what
            got = o["records"]
            assert (got["line_rows"], got["plane_rows"]) == slab.planes(), (what, got["line_rows"], got["plane_rows"], slab.planes())
            assert got["n_ghost"] == slab.ghosts.size > 0
            want_ln = sm.launch(slab, opts, p, dist=True)
            assert want_ln["error"] is None and want_ln["grid"] is not None
            if want_ln["tile_built"]:
                want_b = sm.tile_build(slab, opts)
                bad = sm.build_failures(want_b, got)
                assert not bad, (what, bad)
                if want_b["state"] == 1:
                    bad = sm.check_records(slab, got["meta"], got["cap"], got["run_len"], got["direct_list"], ncols=slab.m + slab.ghosts.size)
                    assert not bad, (what, bad)
            else:
                assert got["state"] == 0
            if want_ln["win_L"]:
                wb = sm.window_build(slab, abs(want_ln["win_L"]))
                assert o["window"] == (wb["win_L"], wb["groups"], wb["flagged"]), (what, o["window"])
            for ln in (o["launch"], o["launch_last"]):
                bad = sm.launch_failures(want_ln, ln)
                assert not bad, (what, bad)
            assert np.array_equal(o["records_last"]["meta"], got["meta"])
            forms.append(sm.form_name(o["launch"]))
            for y, xx, name in zip(o["y"], (X, Xs, X), ("finite X", "X with Inf / NaN / -0.0 / subnormals", "second product")):
                fails += sm.judge_y(slab, sm.slab_x(slab, xx), y, what + ": " + name)
    parity_log(test="spmm_exact", group=case.group, case=case.name, form=sorted(set(forms)), world=world, seconds=round(time.time() - t0, 3))
    assert not fails, fails


def _cases(group):
    return pytest.mark.parametrize("case", sm.cases_of(group), ids=lambda c: c.name)


@_cases("tile_loops")
def test_tile_loops(K, ctx, parity_log, case):
    _check(K, ctx, parity_log, case)


@_cases("tile_chain")
def test_tile_chain(K, ctx, parity_log, case):
    _check(K, ctx, parity_log, case)


@_cases("tile_build")
def test_tile_build(K, ctx, parity_log, case):
    _check(K, ctx, parity_log, case)


@_cases("tile_dist")
def test_tile_dist(K, parity_log, case):
    _check_dist(K, parity_log, case)


@_cases("window")
def test_window(K, ctx, parity_log, case):
    _check(K, ctx, parity_log, case)
