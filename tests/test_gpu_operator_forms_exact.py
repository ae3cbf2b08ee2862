"""Every stored form of a CSR handle at its builder's thresholds, against the serial product (tests/operator_forms_model.py).

One parametrised test per group of the model's table (dictionary codes, sliced layouts, the block-delta stream, row templates,
the adjoint handle, unsorted and repeated columns, the plan's thresholds), one test id per (family, option set).  Every case runs
on a fresh handle under its own option set: nothing is built before the first product; after it the form that ran (khip_spmv_kernel_info, code_info, sell_info,
sell_narrow, sell32_info, delta_info, the return of khip_csr_compress, khip_spmv_bytes_stored against the model's byte formula)
is asserted against the model BEFORE any number is looked at -- where the builder refuses a form, the fallback the builder's rule
gives, never a skip.  Then operator_forms_model.judge: y prefilled with NaN comes back equal to the serial stored-order product
bit for bit (NaN for NaN, the sign of a zero included) for a finite x, for an x with +Inf / NaN / -0.0 / a subnormal, and for a
second product on the cached forms, and on a second handle of the same structure with +Inf / -Inf / NaN VALUES at escape positions,
block boundaries and last entries (y only: a masked entry that is wrongly accumulated shows as NaN there); the vector kernel (mean row above 96) is held to partition_model.vector_row_bound instead;
spmv_dot / spmv_dot2 / spmv_dotw leave the same y and meet exact_reduction's bounds (dot2_bound; y . y: one ulp).  For the
adjoint: the arrays of A' (test export khip_test_csr_arrays) are the stable column-major order of A, entry by entry, and A' x and
(A')' x equal the serial loops.  No bound is measured here: the ratios go to parity_log for the record.
"""
import ctypes
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import operator_forms_model as fm  # noqa: E402
import partition_model as pm  # noqa: E402

pytestmark = pytest.mark.gpu


def _nan(ctx, m):
    return ctx.array(np.full(m, np.nan))


def _fields(A, templates):
    return dict(kernel=A.spmv_kernel_choice, code=tuple(A.code_info), sell=tuple(A.sell_info), narrow=bool(A.sell_narrow),
                sell32=tuple(A.sell32_info), delta=tuple(A.delta_info), templates=templates, bytes=A.spmv_bytes_stored)


def _observe(K, ctx, A, op, exp, opts, what, compress=False):
    """What operator_forms_model.judge_handle reads of one handle; the form is asserted as soon as the first product has run."""
    assert (A.m, A.n, A.nnz) == (op.m, op.n, op.nnz)
    assert (A.code_info, A.sell_info, A.sell32_info, A.delta_info, A.sell_narrow) == ((32, 0), (0, 0, 0), (0, 0, 0), (32, 0, 0), False), \
        "%s: a form was built before the first product" % what
    templates = A.compress() if compress else 0
    inp = op.inputs()
    dx, dxs, dw = ctx.array(inp["x"]), ctx.array(inp["xs"]), ctx.array(inp["w"])
    dy = A.matvec(dx, _nan(ctx, op.m))
    out = _fields(A, templates)
    bad = fm.form_failures(exp, out, opts, what)
    assert not bad, bad                                                   # the form before any numeric comparison
    out["y"] = [dy.to_host(), A.matvec(dxs, _nan(ctx, op.m)).to_host(), A.matvec(dx, _nan(ctx, op.m)).to_host()]
    out["y_dot"] = [None, None, None]
    dy = _nan(ctx, op.m)
    out["dotw"] = K.spmv_dotw(A, dx, dy, dw)
    out["y_dot"][0] = dy.to_host()
    if op.n >= op.m:                                                      # the fused x . y reads x[row] for row < m
        dy = _nan(ctx, op.m)
        out["dot"] = K.spmv_dot(A, dx, dy)
        out["y_dot"][1] = dy.to_host()
        dy = _nan(ctx, op.m)
        out["dot2"] = K.spmv_dot2(A, dx, dy)
        out["y_dot"][2] = dy.to_host()
    again = _fields(A, templates)                                         # the cached forms were reused, none was rebuilt into another
    assert again == {k: out[k] for k in again}, (what, again)
    return out


def _run_case(K, ctx, case):
    op, opts = fm.get_op(case.op), case.options
    assert not fm.want_mismatches(case), fm.want_mismatches(case)
    for k in fm.OPTION_KEYS:
        ctx.set_option(k, opts[k])
    A = K.CsrMatrix.from_host(ctx, op.rowptr, op.col, op.val, (op.m, op.n))
    obs = dict(A=_observe(K, ctx, A, op, fm.expected_of(case), opts, "A", case.compress))
    # the same structure with +Inf / -Inf / NaN values where the kernels mask entries by x = 0.0: the form, then y alone
    nf = op.nonfinite()
    N = K.CsrMatrix.from_host(ctx, nf.rowptr, nf.col, nf.val, (nf.m, nf.n))
    templates = N.compress() if case.compress else 0
    y = N.matvec(ctx.array(nf.inputs()["x"]), _nan(ctx, nf.m))
    obs["N"] = _fields(N, templates)
    bad = fm.form_failures(fm.expected_nf_of(case), obs["N"], opts, "A with Inf / NaN values")
    assert not bad, bad
    obs["N"]["y"] = [y.to_host(), N.matvec(ctx.array(nf.inputs()["xs"]), _nan(ctx, nf.m)).to_host()]
    if case.transpose:
        At = A.transpose()
        ref = fm.transposed_op(op)
        assert At.shape == (op.n, op.m) and At.nnz == op.nnz
        obs["arrays"] = At.to_host_arrays()
        for name, got, want in zip(("rowptr", "col"), obs["arrays"], (ref.rowptr, ref.col)):      # the structure before the products
            assert np.array_equal(got, want), "A': %s differs from the stable column-major order of A" % name
        assert fm.same_bits(obs["arrays"][2], ref.val), "A': val differs from the stable column-major order of A"
        obs["At"] = _observe(K, ctx, At, ref, fm.expected(ref, opts), opts, "A'")
        Att = At.transpose()
        obs["Att"] = _observe(K, ctx, Att, fm.transposed_op(ref), fm.expected(fm.transposed_op(ref), opts), opts, "(A')'")
    return obs


def _check(K, ctx, parity_log, case):
    t0 = time.time()
    saved = {k: ctx.get_option(k) for k in fm.OPTION_KEYS}
    ratios = pm.Ratios()
    try:
        obs = _run_case(K, ctx, case)
    finally:
        for k, v in saved.items():
            ctx.set_option(k, v)
    cnt = ctypes.c_int(-1)
    assert K.lib().khip_test_optional_build_failures(ctypes.byref(cnt)) == 0 and cnt.value == 0, cnt.value
    fails = fm.judge(case, obs, ratios)
    ran = [fm.form_name(obs[h], case.options) for h in ("A", "N", "At", "Att") if h in obs]
    parity_log(test="operator_forms_exact", group=case.group, case=case.name, forms=ran, worst=ratios.worst, seconds=round(time.time() - t0, 3))
    assert not fails, fails


def _cases(group):
    return pytest.mark.parametrize("case", fm.cases_of(group), ids=lambda c: c.name)


@_cases("codes")
def test_dictionary_codes(K, ctx, parity_log, case):
    _check(K, ctx, parity_log, case)


@_cases("sliced")
def test_sliced_layouts(K, ctx, parity_log, case):
    _check(K, ctx, parity_log, case)


@_cases("delta")
def test_delta_stream(K, ctx, parity_log, case):
    _check(K, ctx, parity_log, case)


@_cases("template")
def test_row_templates(K, ctx, parity_log, case):
    _check(K, ctx, parity_log, case)


@_cases("transpose")
def test_adjoint_handle(K, ctx, parity_log, case):
    _check(K, ctx, parity_log, case)


@_cases("unsorted")
def test_unsorted_and_repeated_columns(K, ctx, parity_log, case):
    _check(K, ctx, parity_log, case)


@_cases("plan")
def test_plan_thresholds(K, ctx, parity_log, case):
    _check(K, ctx, parity_log, case)
