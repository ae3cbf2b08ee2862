"""The row-partitioned SpMV of every kernel form against exact references (tests/partition_model.py).

Every operator family of the model x {neighbour exchange, all-gather} x overlap_halo {1, 0} x every form of FORMS, on in-process
ranks (khip_comm_init_local, one host thread per rank, one process).  A case runs on a fresh handle, so its first product is
the split one with the lazy builds at plan time.  Before any comparison the form that ran (khip_spmv_kernel_info, code_info,
sell_info, sell32_info, delta_info) must be the one the model's table says: the wanted form where the table marks it
available, the fallback the builders' rules give where it does not -- never a skip.  Then `judge`: y prefilled with NaN comes
back array_equal to the serial stored-order loop on every rank for two successive products with different x (the vector form:
the row bound gamma(k) sum|a x| against the exact row sum), with +Inf / NaN once in an owned column and once in a column that
is a ghost on a neighbour; spmv_dot / spmv_dotw / spmv_dot2 have the same bits on every rank, meet dot2_bound against the
exact value (y . y: one ulp), leave y unchanged, one ill-conditioned dotw with its cancelling partners on different ranks;
compensated = 0: the plain recursive-sum bound.  No bound is measured: the ratios go to parity_log for the record.

The special values run on whole handles too (test_special_values_on_whole_handles).

What the library does not report: whether the stream kernel took its 16-byte-load path (ran_form takes StreamWide from the
options) and the row block of a launch.  The row block of the delta stream is reported (delta_info) and is asserted to be the one
the model derives the interior launch's delta read from.
"""
import ctypes
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import partition_model as pm  # noqa: E402
from test_gpu_dist import _run_ranks  # noqa: E402  (the in-process rank harness)

pytestmark = pytest.mark.gpu

HALO_MODE = {"neighbour": 1, "gather": 2}
OPTION_KEYS = tuple(k for k in pm.BASE)


def ran_form(A, opts):
    """The form the handle's last product ran, from what the library reports."""
    kernel = A.spmv_kernel_choice
    if kernel == 5:
        return "Template"
    if kernel == 6:
        return "Wave"
    if kernel == 3:
        return "Ordered"
    if kernel == 2:
        return "Vector"
    if kernel == 1:
        bits, rows, _ = A.delta_info
        if bits in (8, 16):
            return "StreamDelta%d" % bits
        return "StreamWide" if (opts["spmv_wide"] and opts["spmv_vec"] != 2) else "Stream"
    if kernel != 4:
        return "kernel %d" % kernel             # judged on the main thread: a rank must not leave its peers in a collective
    bits = A.code_info[0]
    if bits in (8, 16) and opts["spmv_codes"]:
        if opts["spmv_sell"] and A.sell_info[0] == 1:
            return "SlicedNarrow" if A.sell_narrow else "Sliced"
        return "Coded%d" % bits
    return "Sliced32" if (opts["spmv_sell"] and A.sell32_info[0] == 1) else "Staged"


def _make_handle(K, c, P, slab):
    fam = P.fam
    if fam.gen is not None:
        kind, n1, n2, n3 = fam.gen
        return K.CsrMatrix.stencil(c, kind, n1, n2, n3, rows=(slab.r0, slab.r1), distributed=True)
    return K.CsrMatrix.from_host(c, slab.rowptr.astype(np.int64), slab.gcol, slab.val, (slab.m, P.n), dist_rows=(slab.r0, slab.r1), n_global=P.n)


def _nan(c, m):
    return c.array(np.full(m, np.nan))


def _case(K, c, A, slab, inputs, opts):
    """One (form, halo mode, overlap) on one rank: what judge reads."""
    r0, r1, m = slab.r0, slab.r1, slab.m
    out = dict(y=[], y_dot=[])
    for x in inputs["xs"]:
        out["y"].append(A.matvec(c.array(x[r0:r1]), _nan(c, m)).to_host())
    out["form"] = ran_form(A, opts)
    out["delta_rows"] = A.delta_info[1]
    dx = c.array(inputs["xs"][0][r0:r1])
    dy = _nan(c, m)
    out["dot"] = K.spmv_dot(A, dx, dy)
    out["y_dot"].append(dy.to_host())
    dy = _nan(c, m)
    out["dotw"] = K.spmv_dotw(A, dx, dy, c.array(inputs["w"][r0:r1]))
    out["y_dot"].append(dy.to_host())
    dy = _nan(c, m)
    out["dot2"] = K.spmv_dot2(A, dx, dy)
    out["y_dot"].append(dy.to_host())
    dy = _nan(c, m)
    out["dotw_ill"] = K.spmv_dotw(A, dx, dy, c.array(inputs["w_ill"][r0:r1]))
    out["y_dot"].append(dy.to_host())
    return out


def _run_family(K, P, inputs, hub_id):
    """Every rank's results, results[rank][(form, mode, overlap)], and what the handles reported.  The ranks only collect:
    every assertion is made afterwards on the main thread, so no rank leaves a collective early."""
    def body(c, rank):
        slab, res = P.slabs[rank], {}
        for mode, hm in HALO_MODE.items():
            c.set_option("halo_mode", hm)
            for form, spec in pm.FORMS.items():
                opts = spec["opts"]
                for k in OPTION_KEYS:
                    c.set_option(k, opts[k])
                c.set_option("overlap_halo", 1)
                A = _make_handle(K, c, P, slab)                      # a fresh handle: its first product is the split one
                templates = A.compress() if form == "template" else 0
                gather, n_ghost, _ = A.halo_info
                for overlap in (1, 0):
                    c.set_option("overlap_halo", overlap)
                    out = _case(K, c, A, slab, inputs, opts)
                    out.update(gather=gather, n_ghost=n_ghost, templates=templates)
                    res[(form, mode, overlap)] = out
                del A
        return res
    return _run_ranks(K, P.fam.world, hub_id, body)


@pytest.mark.parametrize("fam", pm.FAMILIES, ids=lambda f: f.name)
def test_partitioned_product_of_every_form(K, parity_log, fam):
    t0 = time.time()
    P = pm.partitioned(fam.name)
    inputs = pm.make_inputs(P)
    results = _run_family(K, P, inputs, 7000 + pm.FAMILIES.index(fam))
    cnt = ctypes.c_int(-1)
    assert K.lib().khip_test_optional_build_failures(ctypes.byref(cnt)) == 0 and cnt.value == 0, cnt.value
    tab = pm.table()
    ratios = pm.Ratios()
    failures, ran = [], {}
    for mode in HALO_MODE:
        for r, s in enumerate(P.slabs):                                   # the halo mode asked for is the one the handle took
            got = results[r][("staged", mode, 1)]
            assert got["gather"] == (1 if mode == "gather" else 0), (fam.name, mode, r, got["gather"])
            assert got["n_ghost"] == s.n_ghost(mode), (fam.name, mode, r, got["n_ghost"], s.n_ghost(mode))
        for form, spec in pm.FORMS.items():
            available, _ = tab[(fam.name, form)]
            # the table's form, or the fallback the builders' rules give -- the same on every rank (tests/test_partition_model_host.py)
            templates = [s.templates(mode) if form == "template" else 0 for s in P.slabs]
            want = pm.predict(P.slabs[0].info(mode), spec["opts"], templates[0] > 0)["form"]
            assert (want == spec["want"]) == available
            got_t = [res[(form, mode, 1)]["templates"] for res in results]
            if got_t != templates:
                failures.append(f"{fam.name} {form} {mode}: khip_csr_compress gave {got_t} templates, the model {templates}")
                continue
            for overlap in (1, 0):
                outs = [res[(form, mode, overlap)] for res in results]
                ran[form] = outs[0]["form"]
                fam_ran = pm.family_of(want)
                for r, (o, sl) in enumerate(zip(outs, P.slabs)):          # the delta block the model's interior launch relies on
                    dr = pm.predict(sl.info(mode), spec["opts"], templates[r] > 0)["delta_rows"]
                    if o["delta_rows"] != dr:
                        failures.append(f"{fam.name} {form} {mode} rank {r}: delta_info rows {o['delta_rows']}, the model {dr}")
                fails = pm.judge(P, inputs, outs, want, exact_y=fam_ran != "Vector", compensated=bool(spec["opts"]["compensated"]),
                                 ratios=ratios, two_reductions=fam_ran in pm.TWO_REDUCTION_FORMS)
                failures += [f"{fam.name} {form} {mode} overlap={overlap}: {f}" for f in fails]
    parity_log(test="partitioned_spmv_exact", family=fam.name, world=fam.world, align=fam.align, forms=ran, ratios=ratios.worst,
               cases=4 * len(pm.FORMS), failures=len(failures), seconds=round(time.time() - t0, 2))
    assert not failures, "\n".join(failures[:40] + [f"... {len(failures)} in all"])


WHOLE = ("g7_odd", "g27_64", "dg_kron_256", "dg_s27_256", "bd_32", "bd_256", "mid_64")


@pytest.mark.parametrize("name", WHOLE)
def test_special_values_on_whole_handles(K, ctx, name):
    """+Inf and NaN in x on a whole handle, every form: y equals the serial loop's under array_equal(..., equal_nan=True) (the
    vector form: the same rows are +Inf / -Inf / NaN, the finite rows meet the row bound), the finite product is bit-identical."""
    P = pm.partitioned(name)
    fam = P.fam
    inputs = pm.make_inputs(P)
    info = P.whole_info()
    saved = {k: ctx.get_option(k) for k in OPTION_KEYS}
    failures = []
    try:
        for form, spec in pm.FORMS.items():
            opts = spec["opts"]
            for k in OPTION_KEYS:
                ctx.set_option(k, opts[k])
            if fam.gen is not None:
                A = K.CsrMatrix.stencil(ctx, *fam.gen)
            else:
                A = K.CsrMatrix.from_host(ctx, P.rowptr, P.col, P.val, (P.n, P.n))
            compressed = form == "template" and A.compress() > 0
            assert compressed == (form == "template" and P.whole_templates() > 0)
            want = pm.predict(info, opts, compressed)["form"]
            ys = [A.matvec(ctx.array(x), ctx.array(np.full(P.n, np.nan))).to_host() for x in inputs["xs"]]
            got = ran_form(A, opts)
            if got != want:
                failures.append(f"{name} {form}: ran {got}, expected {want}")
                continue
            for k, (y, ref) in enumerate(zip(ys, inputs["y_ref"])):
                if pm.family_of(want) == "Vector":
                    ok = (np.array_equal(np.isnan(y), np.isnan(ref)) and np.array_equal(np.isinf(y), np.isinf(ref)) and
                          np.array_equal(np.sign(y[np.isinf(y)]), np.sign(ref[np.isinf(ref)])))
                    if ok:                       # the finite rows (all of them for k < 2) meet the row bound
                        xf = np.where(np.isfinite(inputs["xs"][k]), inputs["xs"][k], 0.0)
                        ok = pm.vector_row_bound(P, xf, y, 0, P.n, np.flatnonzero(np.isfinite(ref))) <= 1.0
                else:
                    ok = np.array_equal(y, ref, equal_nan=k >= 2)
                if not ok:
                    failures.append(f"{name} {form}: y[{k}] differs from the serial loop's")
    finally:
        for k, v in saved.items():
            ctx.set_option(k, v)
    assert not failures, "\n".join(failures)
