"""Every device reduction the Python mirror reaches, against the exactly rounded value (tests/exact_reduction.py).

On ill-conditioned data (gen_dot, conditions 1 .. 1e24) a dot must meet the Dot2 bound |d - s| <= u|s| + 2 gamma_n^2 sum|x_i y_i|,
a squared norm must be within 1 ulp of the exact sum of squares, knorm within 1 ulp of the exact norm.  The exact reference is
always taken from the operands the reduction saw, read back from the device.  With compensated = 0 at least one case of every
family (BLAS-1, SpMV, ranks) must break the bound: the file tells the two modes apart.  Non-finite results: one overflowing
product or a +-Inf input gives +-Inf (knorm +Inf), Inf - Inf or a NaN gives NaN, in both modes.

The device-side cross-rank combine (combine_kernel in csrc/blas1.hip, behind comm_allreduce_dd_device) runs in the
device-resident solver loops of any RCCL communicator, one rank included; a one-rank RCCL worker process
(tests/rccl_combine_worker.py, as tests/self_halo_worker.py) pins it on cg! with fused = 2.
"""
import json
import math
import os
import subprocess
import sys
import tempfile
import threading
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_reduction as er  # noqa: E402
from exact_reduction import Tally, ulp  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 63, 64, 65, 255, 257, 1000, 4099, 100003, (1 << 20) + 1]     # those of test_gpu_primitives.py
CONDS = [1.0, 1e4, 1e8, 1e16, 1e24]
KBLOCK, PER_THREAD, FINISH_MAX = 256, 8, 256                                      # csrc/device_reduce.hpp, launch_finish


def finish_geometry(n, vec, u):
    """(partials P, finish grid G) of launch_reduce + launch_finish for n elements, VEC, U (csrc/blas1.hip)."""
    nvec = n // vec
    tiles = max(1, -(-nvec // (KBLOCK * u)))
    P = tiles * (KBLOCK // 64)
    G = min(FINISH_MAX, max(1, -(-P // (KBLOCK * PER_THREAD))))
    return P, G


# sizes from the geometry: G = 1 | 1 < G < 256 | G = 256 with more than 8 partials per thread (VEC = 1, U = 1: an odd offset)
N_G1, N_GMID, N_G256 = 100003, (1 << 20) + 1, (1 << 25) + (1 << 20) + 1


def _dev(ctx, a, misalign=False):
    if not misalign:
        return ctx.array(a)
    base = ctx.zeros(a.size + 1)
    v = base.slice(1, a.size + 1)
    v.copy_from_host(a)
    v._base = base
    return v


@pytest.fixture
def opts(ctx):
    saved = {}

    def set_(**kw):
        for k, v in kw.items():
            saved.setdefault(k, ctx.get_option(k))
            ctx.set_option(k, v)
    yield set_
    for k, v in saved.items():
        ctx.set_option(k, v)


# ------------------------------------------------------------------------------------------------------------ BLAS-1

def test_geometry_of_the_chosen_sizes():
    assert finish_geometry(N_G1, 2, 1)[1] == 1 and finish_geometry(N_G1, 1, 1)[1] == 1
    assert 1 < finish_geometry(N_GMID, 2, 1)[1] < 256 and 1 < finish_geometry(N_GMID, 1, 4)[1] < 256
    P, G = finish_geometry(N_G256, 1, 1)
    assert G == 256 and -(-P // G) > KBLOCK * PER_THREAD


def _blas1_case(K, ctx, tally, n, mis, cond, place, rng):
    x, y, got = er.gen_dot(n, cond, rng, place) if n >= 8 else (*er.gen_dot(n, 1.0, rng)[:2], 1.0)
    if cond > 1:
        assert got >= cond / 2, (n, cond, got)
    dx, dy = _dev(ctx, x, mis), _dev(ctx, y, mis)
    checks = [tally.dot("kdot", K.kdot(n, dx, dy), x, y, got)]
    a, b = K.dot2(n, dx, dy)
    checks += [tally.dot("dot2.xy", a, x, y, got), tally.sq("dot2.xx", b, x), tally.sq("kdot(x,x)", K.kdot(n, dx, dx), x)]
    nr = K.knorm(n, dx)
    en = er.exact_norm(x)
    tally.log(test="exact_reduction", family="blas1", what="knorm", n=n, cond=1.0, ratio=abs(nr - en) / ulp(en), exact=bool(nr == en))
    checks.append((abs(nr - en) <= ulp(en), ("knorm", n, nr, en)))
    assert K.kdot(n, dx, dy) == checks[0][1][3] and K.dot2(n, dx, dy) == (a, b)     # determinism
    return checks


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("mis", [False, True])
def test_blas1_dots_meet_the_dot2_bound(K, ctx, opts, parity_log, n, mis):
    tally = Tally(parity_log, "blas1")
    rng = np.random.default_rng(1000 * n + mis)
    for red_u in (1, 4):
        opts(red_u=red_u)
        for cond in (CONDS if n >= 8 else [1.0]):
            places = ("blocks",) if n > 200000 else ("blocks", "tail") if n > 5000 else ("waves", "blocks", "ends", "tail")
            for place in (places if n >= 1000 else ("ends",)):
                for ok, info in _blas1_case(K, ctx, tally, n, mis, cond, place, rng):
                    assert ok, (red_u, place, info)


@pytest.mark.parametrize("n,mis,red_u", [(N_GMID, True, 4), (N_G256, True, 1)])
def test_blas1_dots_at_the_finish_kernel_limits(K, ctx, opts, parity_log, n, mis, red_u):
    tally = Tally(parity_log, "blas1")
    rng = np.random.default_rng(n)
    opts(red_u=red_u)
    for cond, place in ((1e8, "blocks"), (1e16, "ends"))[: 1 if n > (1 << 24) else 2]:
        x, y, got = er.gen_dot(n, cond, rng, place)
        dx, dy = _dev(ctx, x, mis), _dev(ctx, y, mis)
        ok, info = tally.dot("kdot", K.kdot(n, dx, dy), x, y, got)
        assert ok, info
    nr, en = K.knorm(n, dx), er.exact_norm(x)
    assert abs(nr - en) <= ulp(en), (nr, en)


@pytest.mark.parametrize("n", [2, 1001, 100003, N_GMID])
def test_fused_blas1_reductions(K, ctx, parity_log, n):
    """axpy_sqnorm, axpy2_dot, cg_setup_: the squared norm of the vector each kernel wrote, read back, within 1 ulp."""
    tally = Tally(parity_log, "blas1")
    rng = np.random.default_rng(n + 3)
    p, q, x, r = (rng.standard_normal(n) * np.exp2(rng.integers(-20, 21, n)) for _ in range(4))
    dq, dr = ctx.array(q), ctx.array(r)
    ok, info = tally.sq("axpy_sqnorm", K.axpy_sqnorm(n, -0.3, dq, dr), dr.to_host())
    assert ok, info
    dp_, dq, dx, dr = (ctx.array(v) for v in (p, q, x, r))
    ok, info = tally.sq("axpy2_dot", K.axpy2_dot(n, 0.7, dp_, dq, dx, dr), dr.to_host())
    assert ok, info
    db = ctx.array(p)
    w1, w2, w3 = ctx.zeros(n), ctx.zeros(n), ctx.zeros(n)
    ok, info = tally.sq("cg_setup_", K.cg_setup_(n, db, w1, w2, w3), p)
    assert ok, info


def _mgs_data(n, k, cond, seed):
    rng = np.random.default_rng(seed)
    q0 = rng.standard_normal(n)
    V = [er.gen_dot(n, cond, rng, "blocks", y=q0)[0]]                                       # h_0 ill-conditioned
    for i in range(1, k):
        v = rng.standard_normal(n)
        V.append(v / np.linalg.norm(v))
    return q0, V


def _mgs_check(K, ctx, tally, n, q0, V, mis=False):
    """one mgs_ call on fresh device copies, replayed with kaxpy_: every coefficient within the Dot2 bound of the exact dot of
    the operands it saw, the replay's q equal to the kernel's q bit for bit, the norm within 1 ulp -> (h as returned, q)"""
    k = len(V)
    dV = [_dev(ctx, v, mis) for v in V]
    dq = _dev(ctx, q0, mis)
    h, nrm = K.mgs_(n, dV, dq)
    qf = dq.to_host()
    rq = _dev(ctx, q0, mis)
    for i in range(k):
        qi = rq.to_host()
        ok, info = tally.dot(f"mgs.h{i}", h[i], V[i], qi, er.absum(V[i], qi) / max(abs(er.exact_dot(V[i], qi)), 1e-300))
        assert ok, info
        K.kaxpy_(n, -h[i], dV[i], rq)
    assert np.array_equal(rq.to_host(), qf)
    en = er.exact_norm(qf)
    assert abs(nrm - en) <= ulp(en), (nrm, en)
    return h, nrm, qf


@pytest.mark.parametrize("n,k", [(1000, 1), (4099, 4), (100003, 5), (200001, 30)])
def test_mgs_coefficients_and_norm(K, ctx, parity_log, n, k):
    """mgs_ chains h_i = V_i . q_i with q_{i+1} = fma(-h_i, V_i, q_i) on the device; the q_i it saw are replayed with kaxpy_
    (the same fma) and the replay must end on the kernel's own q bit for bit, which pins the operands of every coefficient."""
    tally = Tally(parity_log, "blas1")
    q0, V = _mgs_data(n, k, {1: 1e16, 4: 1e8, 5: 1e4, 30: 1e16}[k], k)
    _mgs_check(K, ctx, tally, n, q0, V)


@pytest.mark.parametrize("n,k", [(1000, 1), (4099, 4), (513, 5)])
def test_mgs_on_misaligned_vectors(K, ctx, parity_log, n, k):
    """q and every V_i at 8 (mod 16): the 8-byte instantiation of reduce_kernel<RED_AXPYDEV>"""
    tally = Tally(parity_log, "blas1")
    q0, V = _mgs_data(n, k, {1: 1e16, 4: 1e8, 5: 1e4}[k], 50 + k)
    _mgs_check(K, ctx, tally, n, q0, V, mis=True)


@pytest.mark.parametrize("mgs_keep", [0, 1, 2])
@pytest.mark.parametrize("red_u", [1, 4])
@pytest.mark.parametrize("nt", ["default", 1])
@pytest.mark.parametrize("mis", [False, True])
def test_mgs_under_every_knob(K, ctx, opts, parity_log, mgs_keep, red_u, nt, mis):
    """the KEEP instantiation (mgs_keep = 1 with non-temporal accesses on aligned vectors), nothing streamed (2), four accesses
    per lane (red_u = 4): the same pins at n = 4099, k = 5"""
    tally = Tally(parity_log, "blas1")
    opts(mgs_keep=mgs_keep, red_u=red_u)
    if nt == 1:
        opts(nt_min_elems=1)
    q0, V = _mgs_data(4099, 5, 1e8, 77)
    _mgs_check(K, ctx, tally, 4099, q0, V, mis=mis)


def _quiet_tally():
    return Tally(lambda **kw: None, "blas1")


@pytest.mark.parametrize("k", [255, 256])
@pytest.mark.parametrize("mis", [False, True])
def test_mgs_at_the_ring_boundary(K, ctx, k, mis):
    """khip_mgs at n = 257: k + 1 == 256 slots fills the device scalar ring exactly (the cascade), k + 1 == 257 does not fit
    (the fallback sequence of khip_dot / khip_axpy)"""
    q0, V = _mgs_data(257, k, 1e8, 300 + k)
    _mgs_check(K, ctx, _quiet_tally(), 257, q0, V, mis=mis)


def test_mgs_wraps_the_ring_between_calls(K, ctx):
    """three consecutive calls of 101 slots each: wherever the ring stood, one of them starts over at slot 0"""
    for call in range(3):
        q0, V = _mgs_data(257, 100, 1e8, 400 + call)
        _mgs_check(K, ctx, _quiet_tally(), 257, q0, V)


def test_mgs_accumulates_into_the_callers_coefficients(K, ctx):
    """accumulate = 1 (reorthogonalisation) with the ring exactly full: h_out[i] = h_in[i] + h_i in one rounding, q as without"""
    n, k = 257, 255
    q0, V = _mgs_data(n, k, 1e8, 500)
    h, nrm, qf = _mgs_check(K, ctx, _quiet_tally(), n, q0, V)
    acc = np.random.default_rng(501).standard_normal(k).tolist()
    dV = [ctx.array(v) for v in V]
    dq = ctx.array(q0)
    h2, nrm2 = K.mgs_(n, dV, dq, accumulate_into=acc)
    assert h2 == [a + b for a, b in zip(acc, h)] and nrm2 == nrm
    assert np.array_equal(dq.to_host(), qf)


# --------------------------------------------------------------------------------------------------------------- SpMV

def _serial(S, x):
    y = np.zeros(S.shape[0])
    for i in range(S.shape[0]):
        acc = 0.0
        for q in range(S.indptr[i], S.indptr[i + 1]):
            acc = acc + S.data[q] * x[S.indices[q]]
        y[i] = acc
    return y


def _operators(K, oracle):
    """(name, scipy CSR, device constructor) -- Poisson, 27-point, kron_unsymmetric, banded + random, two fuzz shapes, and
    Poisson - 5.5 I (indefinite: x . Ax can be made ill-conditioned)."""
    import scipy.sparse as sp
    out = []
    for kind, n1, gen in (("poisson", 20, oracle.poisson3d), ("stencil27", 9, oracle.stencil27_unsym),
                          ("kron_unsymmetric", 12, oracle.kron_unsymmetric)):
        A = gen(n1)
        out.append((kind, A.to_scipy().tocsr(), lambda c, kind=kind, n1=n1: K.CsrMatrix.stencil(c, kind, n1)))
    B = oracle.banded_random(n=20000, seed=3, unsym=True)
    out.append(("banded_random", B.to_scipy().tocsr(), None))
    rng = np.random.default_rng(2024)
    for (m, mean, heavy) in ((1000, 3, 0), (900, 8, 3)):
        rows, cols, vals = [], [], []
        for i in range(m):
            k = int(rng.poisson(mean)) if rng.random() > 0.1 else 0
            if heavy and i % 97 == heavy:
                k = 300
            cs = np.sort(rng.choice(m, size=min(k, m), replace=False))
            rows += [i] * len(cs); cols += list(cs); vals += list(rng.standard_normal(len(cs)))
        S = sp.csr_matrix((vals, (rows, cols)), shape=(m, m)); S.sort_indices()
        out.append((f"fuzz{m}", S, None))
    P = oracle.poisson3d(16).to_scipy().tocsr()
    P = (P - 5.5 * sp.identity(P.shape[0], format="csr")).tocsr(); P.sort_indices()
    out.append(("poisson-5.5I", P, None))
    return out


def _upload(K, ctx, S, make):
    if make is not None:
        return make(ctx)
    return K.CsrMatrix.from_host(ctx, S.indptr.astype(np.int64), S.indices.astype(np.int32), S.data, S.shape)


# (name, options, bit-exact y, expected spmv_kernel_choice or None)
CONFIGS = [
    ("auto", dict(spmv_kernel=0), True, None),
    ("stream", dict(spmv_kernel=1, spmv_codes=0, spmv_delta=0, spmv_wide=0), True, 1),
    ("stream-wide", dict(spmv_kernel=1, spmv_codes=0, spmv_delta=0, spmv_wide=1), True, 1),
    ("stream-delta", dict(spmv_kernel=1, spmv_codes=0, spmv_delta=2), True, 1),
    ("vector-8", dict(spmv_kernel=2, spmv_lanes=8), False, 2),
    ("vector-32", dict(spmv_kernel=2, spmv_lanes=32), False, 2),
    ("ordered-16", dict(spmv_kernel=3, spmv_lanes=16), True, 3),
    ("staged", dict(spmv_kernel=4, spmv_codes=0, spmv_sell=0, spmv_blk_pub=0), True, 4),
    ("staged-pub", dict(spmv_kernel=4, spmv_codes=0, spmv_sell=0, spmv_blk_pub=1), True, 4),
    ("staged-early", dict(spmv_kernel=4, spmv_codes=0, spmv_sell=0, spmv_dot_early=1), True, 4),
    ("coded", dict(spmv_kernel=4, spmv_codes=2, spmv_sell=0, spmv_blk_pub=0), True, 4),
    ("coded-pub", dict(spmv_kernel=4, spmv_codes=2, spmv_sell=0, spmv_blk_pub=1), True, 4),
    ("sell8-pair1", dict(spmv_kernel=4, spmv_codes=2, spmv_sell=2, spmv_sell_pair=1), True, 4),
    ("sell8-pair0", dict(spmv_kernel=4, spmv_codes=2, spmv_sell=2, spmv_sell_pair=0), True, 4),
    ("sell8-narrow", dict(spmv_kernel=4, spmv_codes=2, spmv_sell=2, spmv_sell_narrow=1), True, 4),
    ("sell32", dict(spmv_kernel=4, spmv_codes=0, spmv_sell=3), True, 4),
    ("waves", dict(spmv_kernel=6), True, 6),
]
_ALL_KEYS = sorted({k for _, o, _, _ in CONFIGS for k in o})


@pytest.mark.parametrize("cfg", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_spmv_fused_dots_meet_the_dot2_bound(K, ctx, oracle, opts, parity_log, cfg):
    name, o, bit_exact, want_kernel = cfg
    tally = Tally(parity_log, "spmv:" + name)
    seed = zlib.crc32(name.encode())                                     # stable across processes (str hashes are salted)
    rng = np.random.default_rng(seed)
    opts(**{k: ctx.get_option(k) for k in _ALL_KEYS})                    # restore everything afterwards
    floor_hit = False
    for oname, S, make in _operators(K, oracle):
        opts(**o)
        m = S.shape[0]
        dA = _upload(K, ctx, S, make)
        x = rng.standard_normal(m) * np.exp2(rng.integers(-4, 5, m))
        dx = ctx.array(x)
        dy = ctx.zeros(m)
        dA.matvec(dx, dy)
        y = dy.to_host()
        if bit_exact:
            assert np.array_equal(y, _serial(S, x)), (name, oname)
        choice = dA.spmv_kernel_choice
        if want_kernel is not None:
            assert choice == want_kernel, (name, oname, choice)
        # the form a forced option asks for, on every operator it applies to (few diagonals: the stencils and Poisson - 5.5 I;
        # <= 8 entries per row for the int32 sliced form); the others are logged with the form they got
        few_diags = oname in ("poisson", "kron_unsymmetric", "stencil27", "poisson-5.5I")
        short_rows = few_diags and int(np.diff(S.indptr).max()) <= 8
        if name.startswith("sell8") and few_diags:
            assert dA.sell_info[0] == 1 and dA.code_info[0] == 8, (name, oname, dA.sell_info, dA.code_info)
        if name == "sell32" and short_rows:
            assert dA.sell32_info[0] == 1, (name, oname, dA.sell32_info)
        if name.startswith("coded") and few_diags:
            assert dA.code_info[0] == 8 and dA.sell_info[0] == 0, (name, oname, dA.code_info, dA.sell_info)
        if name in ("stream", "stream-wide", "staged", "staged-pub", "staged-early"):
            assert dA.code_info == (32, 0) and dA.sell_info[0] != 1 and dA.sell32_info[0] != 1, (name, oname)
        tally.log(test="exact_reduction", family="spmv-kernel", what=name, operator=oname, seed=seed, choice=choice,
                  code_info=list(dA.code_info), sell_info=list(dA.sell_info), sell32_info=list(dA.sell32_info),
                  delta_info=list(dA.delta_info))
        # spmv_dotw: w from gen_dot against this y
        for cond, place in ((1.0, "ends"), (1e8, "blocks"), (1e16, "ends"), (1e24, "waves")):
            w, _, got = er.gen_dot(m, cond, rng, place, y=y)
            assert got >= cond / 2
            dw, dy2 = ctx.array(w), ctx.zeros(m)
            d = K.spmv_dotw(dA, dx, dy2, dw)
            y2 = dy2.to_host()
            if bit_exact:
                assert np.array_equal(y2, y)
            ok, info = tally.dot("spmv_dotw", d, w, y2, got)
            assert ok, (name, oname, info)
            assert K.spmv_dotw(dA, dx, dy2, dw) == d                       # determinism
        # spmv_dot / spmv_dot2: x . Ax is what the operator makes of x; on Poisson - 5.5 I, x is mixed from two vectors so
        # that x . Ax nearly cancels
        xs = [x]
        if oname == "poisson-5.5I":
            u, v = rng.standard_normal(m), np.cos(np.arange(m) * 0.01)
            a, b, c = u @ (S @ u), u @ (S @ v) + v @ (S @ u), v @ (S @ v)
            if a * c < 0:
                t = (-b + math.sqrt(b * b - 4 * a * c)) / (2 * c)
                xs.append(u + t * v)
        for xv in xs:
            dxv, dy3 = ctx.array(xv), ctx.zeros(m)
            d = K.spmv_dot(dA, dxv, dy3)
            y3 = dy3.to_host()
            cnd = er.absum(xv, y3) / max(abs(er.exact_dot(xv, y3)), 1e-300)
            ok, info = tally.dot("spmv_dot", d, xv, y3, cnd)
            assert ok, (name, oname, info)
            d2 = K.spmv_dot2(dA, dxv, dy3)
            y4 = dy3.to_host()
            ok, info = tally.dot("spmv_dot2.xy", d2[0], xv, y4, cnd)
            assert ok, (name, oname, info)
            ok, info = tally.sq("spmv_dot2.yy", d2[1], y4)
            assert ok, (name, oname, info)
            if oname == "poisson-5.5I" and cnd >= 1e6:
                floor_hit = True
    assert floor_hit, name


def test_spmv_dot_of_a_compressed_template_handle(K, ctx, oracle, opts, parity_log):
    tally = Tally(parity_log, "spmv:template")
    A = oracle.poisson3d(24)
    dA = K.CsrMatrix.stencil(ctx, "poisson", 24)
    assert dA.compress() > 0
    assert dA.spmv_kernel_choice == 5
    rng = np.random.default_rng(5)
    x = rng.standard_normal(A.n)
    dx, dy = ctx.array(x), ctx.zeros(A.n)
    dA.matvec(dx, dy)
    y = dy.to_host()
    assert np.array_equal(y, A.matvec(x))
    for cond in CONDS:
        w, _, got = er.gen_dot(A.n, cond, rng, "blocks", y=y)
        dy2 = ctx.zeros(A.n)
        ok, info = tally.dot("spmv_dotw", K.spmv_dotw(dA, dx, dy2, ctx.array(w)), w, dy2.to_host(), got)
        assert ok, info
        d2 = K.spmv_dot2(dA, dx, dy2)
        ok, info = tally.dot("spmv_dot2.xy", d2[0], x, dy2.to_host(), 1.0)
        assert ok, info


def test_spmv_dotw_large_on_the_default_kernel(K, ctx, parity_log):
    """One large product (2^24 rows, the default sliced kernel) with the partners in different finish-kernel blocks."""
    tally = Tally(parity_log, "spmv:default-large")
    n1 = 256
    dA = K.CsrMatrix.stencil(ctx, "poisson", n1)
    n = n1 ** 3
    rng = np.random.default_rng(7)
    x = rng.standard_normal(n)
    dx, dy = ctx.array(x), ctx.zeros(n)
    dA.matvec(dx, dy)
    y = dy.to_host()
    for cond, place in ((1e8, "blocks"), (1e16, "ends")):
        w, _, got = er.gen_dot(n, cond, rng, place, y=y)
        dy2 = ctx.zeros(n)
        ok, info = tally.dot("spmv_dotw", K.spmv_dotw(dA, dx, dy2, ctx.array(w)), w, dy2.to_host(), got)
        assert ok, info


# -------------------------------------------------------------------------------------------------------------- ranks

def _run_ranks(K, world, hub_id, body):
    """In-process ranks on one device, one thread each (the pattern of tests/test_gpu_minres.py)."""
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
        t.join(timeout=300)
    assert not errors, errors
    assert all(not t.is_alive() for t in ts), "a rank is stuck (collective mismatch)"
    return results


def _rank_cases(K, oracle, world, comp, seed):
    """kdot, knorm and spmv_dotw / spmv_dot on a row partition with the cancelling partners on different ranks."""
    n1 = 24
    A = oracle.poisson3d(n1)
    n = A.n
    starts = K.row_partition(n, world)
    rng = np.random.default_rng(seed)
    x, y, got = er.gen_dot(n, 1e16, rng, "ranks", starts=starts)
    xv = rng.standard_normal(n)
    yA = A.matvec(xv)
    w, _, got_w = er.gen_dot(n, 1e16, rng, "ranks", y=yA, starts=starts)

    def body(c, rank):
        c.set_option("compensated", comp)
        r0, r1 = starts[rank], starts[rank + 1]
        nl = r1 - r0
        out = {"kdot": K.kdot(nl, c.array(x[r0:r1]), c.array(y[r0:r1])), "knorm": K.knorm(nl, c.array(x[r0:r1]))}
        dA = K.CsrMatrix.stencil(c, "poisson", n1, rows=(r0, r1), distributed=True)
        dy = c.zeros(nl)
        out["spmv_dotw"] = K.spmv_dotw(dA, c.array(xv[r0:r1]), dy, c.array(w[r0:r1]))
        out["y"] = dy.to_host()
        out["spmv_dot"] = K.spmv_dot(dA, c.array(xv[r0:r1]), dy)
        return out
    return body, (x, y, got, xv, yA, w, got_w)


@pytest.mark.parametrize("world", [2, 3])
def test_ranks_combine_meets_the_dot2_bound(K, oracle, parity_log, world):
    tally = Tally(parity_log, f"ranks{world}")
    body, (x, y, got, xv, yA, w, got_w) = _rank_cases(K, oracle, world, 1, world)
    res = _run_ranks(K, world, 900 + world, body)
    yd = np.concatenate([r["y"] for r in res])
    assert np.array_equal(yd, yA)
    for r in res:
        for key in ("kdot", "knorm", "spmv_dotw", "spmv_dot"):
            assert r[key] == res[0][key], key                       # the same bits on every rank
    assert got >= 5e15 and got_w >= 5e15
    for what, d, a, b, c in (("kdot", res[0]["kdot"], x, y, got), ("spmv_dotw", res[0]["spmv_dotw"], w, yA, got_w),
                             ("spmv_dot", res[0]["spmv_dot"], xv, yA, 1.0)):
        ok, info = tally.dot(what, d, a, b, c)
        assert ok, info
    en = er.exact_norm(x)
    assert abs(res[0]["knorm"] - en) <= ulp(en)


def test_device_combine_of_one_rccl_rank():
    """cg! (fused = 2) on a one-rank RCCL communicator: every p.Ap and r.r goes finish kernel -> ncclAllGather -> combine_kernel
    -> epilogue.  Finite: the history is bit-identical to the same solve on a context without a communicator.  A right-hand
    side whose first residual has r.r ~ 1e309 (finite squares, tests/rccl_combine_worker.py overflow_rhs): the combine must
    hand +Inf to the epilogue, so the history records ||r_1|| = +Inf (as without the communicator) before the NaN of the next
    iteration stops the solve; a NaN from the combine would stop it one iteration earlier with no second entry."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "r.json")
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
        try:
            p = subprocess.run([sys.executable, os.path.join(root, "tests", "rccl_combine_worker.py"), "30", out],
                               env=env, capture_output=True, text=True, timeout=240)
        except subprocess.TimeoutExpired:
            pytest.fail("the one-rank RCCL worker hangs")
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        with open(out) as f:
            r = json.load(f)
    assert r["rccl_ranks"] == 1
    assert r["probe"]["path"] == 2 and r["combine_launches"] >= 2 * r["probe"]["niter"] > 0, r["probe"]
    for fused in (2, 1):
        c, q = r[f"finite_comm_f{fused}"], r[f"finite_plain_f{fused}"]
        assert c["path"] == q["path"] == fused and not c["error"] and not q["error"]
        assert c["niter"] == q["niter"] and c["hist"] == q["hist"], fused         # the same bits
        c, q = r[f"overflow_comm_f{fused}"], r[f"overflow_plain_f{fused}"]
        assert np.array_equal(np.array(c["hist"]), np.array(q["hist"]), equal_nan=True) and c["error"] == q["error"], (fused, c, q)
    c = r["overflow_comm_f2"]
    assert len(c["hist"]) >= 2 and math.isfinite(c["hist"][0]) and c["hist"][1] == math.inf, c
    assert "positive definite" in c["error"], c


# -------------------------------------------------------------------------------------------------------------- teeth

def test_uncompensated_mode_breaks_the_bound_in_every_family(K, ctx, oracle, opts):
    """compensated = 0 (plain fma accumulation, same trees): the Dot2 bound must fail somewhere in each family, so this file can
    tell the two modes apart."""
    rng = np.random.default_rng(42)
    opts(compensated=0)
    broken = {"blas1": 0, "spmv": 0, "ranks": 0}
    n = 100003
    for cond, place in ((1e8, "waves"), (1e16, "blocks"), (1e8, "ends")):
        x, y, _ = er.gen_dot(n, cond, rng, place)
        s = er.exact_dot(x, y)
        broken["blas1"] += abs(K.kdot(n, ctx.array(x), ctx.array(y)) - s) > er.dot2_bound(n, s, er.absum(x, y))
    dA = K.CsrMatrix.stencil(ctx, "poisson", 20)
    m = 8000
    xv = rng.standard_normal(m)
    dx, dy = ctx.array(xv), ctx.zeros(m)
    dA.matvec(dx, dy)
    yv = dy.to_host()
    for cond, place in ((1e8, "blocks"), (1e16, "ends")):
        w, _, _ = er.gen_dot(m, cond, rng, place, y=yv)
        d = K.spmv_dotw(dA, dx, ctx.zeros(m), ctx.array(w))
        s = er.exact_dot(w, yv)
        broken["spmv"] += abs(d - s) > er.dot2_bound(m, s, er.absum(w, yv))
    body, (x, y, got, xv2, yA, w2, got_w) = _rank_cases(K, oracle, 2, 0, 77)
    res = _run_ranks(K, 2, 990, body)
    for d, a, b in ((res[0]["kdot"], x, y), (res[0]["spmv_dotw"], w2, yA)):
        s = er.exact_dot(a, b)
        broken["ranks"] += abs(d - s) > er.dot2_bound(a.size, s, er.absum(a, b))
    assert all(v > 0 for v in broken.values()), broken


# ------------------------------------------------------------------------------------------------------- non-finite

# Inputs whose plain result depends on the order in which partial sums overflow are out of scope: every case has at most one
# overflowing product, or infinite inputs (two overflowing products of opposite signs: NaN in Dot2, +-Inf in an fma chain).
NONFINITE = [
    ("overflow +", (0, 1e300, 1e300), math.inf),
    ("overflow -", (0, -1e300, 1e300), -math.inf),
    ("inf input", (1, math.inf, 2.0), math.inf),
    ("-inf input", (1, 2.0, -math.inf), -math.inf),
    ("inf - inf", (2, math.inf, -math.inf), math.nan),
    ("nan", (3, math.nan, 1.0), math.nan),
]


def _same(a, want):
    return math.isnan(a) if math.isnan(want) else a == want


@pytest.mark.parametrize("n,mis", [(5, False), (1001, True), (100003, False), (N_GMID, False)])
@pytest.mark.parametrize("case", NONFINITE, ids=[c[0] for c in NONFINITE])
def test_nonfinite_results(K, ctx, opts, n, mis, case):
    name, (kind, a, b), want = case
    rng = np.random.default_rng(n)
    x, y = rng.standard_normal(n), rng.standard_normal(n)
    i, j = n // 2, n - 1                                    # j: the odd tail element where n is odd
    if kind == 0:
        x[i], y[i] = a, b                                  # one overflowing product
    elif kind in (1, 3):
        x[i], x[j] = a, b                                  # +-Inf / NaN inputs in x (y finite)
        y[i], y[j] = 1.0, 1.0
    else:
        x[i], x[j], y[i], y[j] = a, b, 1.0, 1.0            # Inf and -Inf products
    for comp in (1, 0):
        opts(compensated=comp)
        dx, dy = _dev(ctx, x, mis), _dev(ctx, y, mis)
        got = {"kdot": K.kdot(n, dx, dy), "dot2.xy": K.dot2(n, dx, dy)[0]}
        for k, v in got.items():
            assert _same(v, want), (name, comp, k, v)
        # squared norms and knorm: +Inf for any infinite or overflowing x, NaN for NaN
        want_sq = math.nan if kind == 3 else math.inf
        xs = x.copy()
        if kind == 0:
            xs[i] = 1e300                                   # its square overflows
        dxs = _dev(ctx, xs, mis)
        sq = {"knorm": K.knorm(n, dxs), "kdot(x,x)": K.kdot(n, dxs, dxs), "dot2.xx": K.dot2(n, dxs, dy)[1],
              "cg_setup_": K.cg_setup_(n, dxs, ctx.zeros(n), ctx.zeros(n), ctx.zeros(n))}
        dz = _dev(ctx, xs, mis)
        sq["axpy_sqnorm"] = K.axpy_sqnorm(n, 0.0, _dev(ctx, np.zeros(n), mis), dz)
        for k, v in sq.items():
            assert _same(v, want_sq), (name, comp, k, v)


def test_nonfinite_spmv_dot_and_ranks(K, ctx, oracle, opts):
    A = oracle.poisson3d(12)
    n = A.n
    k = n // 2
    dA = K.CsrMatrix.stencil(ctx, "poisson", 12)
    for comp in (1, 0):
        opts(compensated=comp)
        xv = np.ones(n); xv[k] = 1e300                     # y stays finite; w_k y_k overflows, alone
        for wk, want in ((1e300, math.inf), (-1e300, -math.inf)):
            w = np.ones(n); w[k] = wk
            assert K.spmv_dotw(dA, ctx.array(xv), ctx.zeros(n), ctx.array(w)) == want, (comp, wk)
        xv = np.ones(n); xv[k] = math.nan
        assert math.isnan(K.spmv_dot(dA, ctx.array(xv), ctx.zeros(n))), comp
        xv = np.ones(n); xv[k] = math.inf                  # y_k = +Inf, its neighbours -Inf: Inf - Inf
        assert math.isnan(K.spmv_dot(dA, ctx.array(xv), ctx.zeros(n))), comp
    starts = K.row_partition(n, 2)

    def body(c, rank):
        r0, r1 = starts[rank], starts[rank + 1]
        out = {}
        for comp in (1, 0):
            c.set_option("compensated", comp)
            for name, xi, yi in (("inf", math.inf, 1.0), ("-inf", -math.inf, 1.0), ("overflow", 1e300, 1e300)):
                xv, yv = np.ones(n), np.ones(n)
                xv[r0], yv[r0] = xi, yi                     # one on each rank
                out[(comp, name)] = K.kdot(r1 - r0, c.array(xv[r0:r1]), c.array(yv[r0:r1]))
            xv = np.ones(n); xv[starts[0]] = math.inf; xv[starts[1]] = -math.inf
            out[(comp, "inf-inf")] = K.kdot(r1 - r0, c.array(xv[r0:r1]), c.array(np.ones(r1 - r0)))
        return out
    res = _run_ranks(K, 2, 995, body)
    for comp in (1, 0):
        for r in res:
            assert r[(comp, "inf")] == math.inf and r[(comp, "overflow")] == math.inf, r
            assert r[(comp, "-inf")] == -math.inf, r
            assert math.isnan(r[(comp, "inf-inf")]), r
