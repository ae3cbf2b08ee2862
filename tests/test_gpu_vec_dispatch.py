"""The instantiation a streaming vector kernel is launched with (csrc/vec_launch.hpp: vec_plan, vec_dispatch) against a property
that holds by construction: cache hints change no arithmetic, so every solver and every primitive must give the SAME BITS with
ctx option nt_min_elems = 1 (every launch takes its non-temporal instantiation where it has one) as with the default (none
does at these sizes).  A dispatcher that handed NT to a kernel's COMP slot, or the reverse, would change the accumulation of
the dots and fail here; so would one that mixed up VEC.

Sizes: n = 2 (below one workgroup on both paths), 511 (the odd tail element), 513 (the tail with a second workgroup on the
8-byte path); primitives also at n = 1.  Vectors are carved from one buffer at element offset 0 (16-byte path) and at offset
1 (8-byte path), the way tests/test_gpu_bilq.py does.  The offset-1 run is held to the offset-0 run by the tolerance of the
solver's own path tests, not to the bit: |dr_k| <= 1e-10 r_k + 100 eps r_0 for cg! and gmres! (tests/test_gpu_solvers.py),
9 d + 1e-13 with d the oracle's own distance from the exact history for bicgstab! (_bicgstab_rtol at its smallest case), and
1e-8 r_k + 1e-12 beta_1 for minres!, cg_lanczos_shift! and bilq! (the least value their budgets take); x within
1e-8 max|x|."""
import ctypes as C
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(float).eps
SIZES = (2, 511, 513)
SHIFTS = (0.5, 1.0, 2.0)
SOLVE = dict(itmax=6, atol=0.0, rtol=0.0, history=True)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def _carved(ctx, n, names, first):
    """len(names) vectors of n entries inside one buffer, at element offset `first` with an even stride: first = 1 puts every
    vector at 8 (mod 16), first = 0 keeps them 16-byte aligned"""
    stride = n + 2 - (n & 1) + 2
    buf = ctx.zeros(first + len(names) * stride)
    assert buf.ptr % 16 == 0
    vec = {k: buf.slice(first + i * stride, first + i * stride + n) for i, k in enumerate(names)}
    assert all(v.ptr % 16 == 8 * first for v in vec.values())
    return buf, vec


_OPS = {}


def _operator(K, ctx, n, skew=0.0):
    """tridiag(-1 - skew, 2.5, -1 + skew): the 1-D Laplacian shifted by 0.5, for bilq! with a skew part"""
    import scipy.sparse as sp
    if (n, skew) not in _OPS:
        S = sp.diags([np.full(n - 1, -1.0 - skew), np.full(n, 2.5), np.full(n - 1, -1.0 + skew)], [-1, 0, 1], format="csr")
        S.sort_indices()
        _OPS[(n, skew)] = K.CsrMatrix.from_host(ctx, S.indptr, S.indices, S.data, S.shape)
    return _OPS[(n, skew)]


def _rhs(n):
    return np.cos(0.37 * np.arange(n)) + 0.5


class _Options:
    """ctx options set for a block and put back after it"""

    def __init__(self, ctx, **opts):
        self.ctx, self.opts = ctx, opts

    def __enter__(self):
        self.prev = {k: self.ctx.get_option(k) for k in self.opts}
        for k, v in self.opts.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k, v in self.prev.items():
            self.ctx.set_option(k, v)


# ---- the solvers -------------------------------------------------------------------------------------------------------------------
VECTORS = {
    "cg": ("x", "r", "p", "Ap"),
    "bicgstab": ("x", "r", "p", "v", "s", "qd"),
    "gmres": ("x", "w") + tuple(f"V{i}" for i in range(8)),              # V5 .. V7: what the grow callback hands out
    "minres": ("x", "r1", "r2", "w1", "w2", "y"),
    "cg_lanczos_shift": ("Mv", "Mv_prev", "Mv_next") + tuple(f"x{i}" for i in range(3)) + tuple(f"p{i}" for i in range(3)),
}


def _workspace(K, ctx, solver, n, first):
    """the solver's workspace on caller-owned vectors carved at element offset `first`"""
    L = K.lib()
    if solver == "bilq":
        buf, v = _carved(ctx, n, K.BilqWorkspace.VECTORS, first)
        ws = K.BilqWorkspace(ctx, n, n, vectors=v)
        ws._buf = buf
        return ws
    cls = {"cg": K.CgWorkspace, "bicgstab": K.BicgstabWorkspace, "gmres": K.GmresWorkspace, "minres": K.MinresWorkspace,
           "cg_lanczos_shift": K.CgLanczosShiftWorkspace}[solver]
    buf, v = _carved(ctx, n, VECTORS[solver], first)
    ws = cls.__new__(cls)
    ws.ctx, ws.m, ws.n, ws.adopted, ws._alloc_s, ws._h, ws._buf = ctx, n, n, True, 0.0, C.c_void_p(), buf
    h = C.byref(ws._h)
    if solver == "cg":
        ws._vec = v
        rc = L.khip_cg_workspace_adopt(ctx._h, n, n, *[v[k].ptr for k in ("x", "r", "p", "Ap")], h)
    elif solver == "bicgstab":
        ws._vec = v
        rc = L.khip_bicgstab_workspace_adopt(ctx._h, n, n, *[v[k].ptr for k in VECTORS[solver]], h)
    elif solver == "minres":
        ws._vec, ws.window = v, 5
        rc = L.khip_minres_workspace_adopt(ctx._h, n, n, 5, *[v[k].ptr for k in VECTORS[solver]], h)
    elif solver == "gmres":
        mem = min(n, 5)
        ws._vec, ws.memory = {"x": v["x"], "w": v["w"]}, 5
        ws.V = [v[f"V{i}"] for i in range(mem)]
        spare = [v[f"V{i}"] for i in range(mem, 8)]
        ptrs = (C.c_void_p * mem)(*[u.ptr for u in ws.V])
        rc = L.khip_gmres_workspace_adopt(ctx._h, n, n, mem, v["x"].ptr, v["w"].ptr, ptrs, h)

        def grow(_ud):                                                  # push!(V, similar(x)): the next carved vector
            ws.V.append(spare.pop(0))
            return ws.V[-1].ptr
        ws._grow = K.GROW_FN(grow)
        assert rc == 0 and L.khip_gmres_workspace_set_grow(ws._h, ws._grow, None) == 0
    else:
        ws._vec, ws.nshifts = {k: v[k] for k in ("Mv", "Mv_prev", "Mv_next")}, 3
        ws._x, ws._pv = [v[f"x{i}"] for i in range(3)], [v[f"p{i}"] for i in range(3)]
        xs = (C.c_void_p * 3)(*[u.ptr for u in ws._x])
        ps = (C.c_void_p * 3)(*[u.ptr for u in ws._pv])
        rc = L.khip_cg_lanczos_shift_workspace_adopt(ctx._h, n, n, 3, v["Mv"].ptr, v["Mv_prev"].ptr, v["Mv_next"].ptr,
                                                     C.cast(xs, K.c_void_pp), C.cast(ps, K.c_void_pp), h)
    assert rc == 0, L.khip_last_error()
    return ws


def _solve(K, ctx, solver, n, first, fused, last_path=None, **kw):
    """one solve -> (x, history, niter, status); x and history as lists of arrays (one per shift for cg_lanczos_shift!).
    last_path: the loop the solve must report (default: the one `fused` asks for; the opt-in variants report 1)"""
    ws = _workspace(K, ctx, solver, n, first)
    b = ctx.array(_rhs(n))
    if solver == "bilq":
        K.bilq_(ws, _operator(K, ctx, n, 0.3), b, fused=fused, **SOLVE, **kw)
    elif solver == "cg_lanczos_shift":
        K.cg_lanczos_shift_(ws, _operator(K, ctx, n), b, SHIFTS, fused=fused, **SOLVE, **kw)
    else:
        {"cg": K.cg_, "bicgstab": K.bicgstab_, "gmres": K.gmres_, "minres": K.minres_}[solver](
            ws, _operator(K, ctx, n), b, fused=fused, **SOLVE, **kw)
    want = fused if last_path is None else last_path
    assert ws.last_path == want, (solver, n, first, fused, ws.last_path, want)
    st = ws.stats
    if solver == "cg_lanczos_shift":
        return [u.to_host() for u in ws.x], [np.array(h) for h in st.residuals], st.niter, st.status
    return [ws.x.to_host()], [np.array(st.residuals)], st.niter, st.status


def _bicgstab_rtol():
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "quad_histories.json")))
    d = min(c["oracle_double_max_rel_dev"] for c in g["cases"] if c["solver"] == "bicgstab")
    return 9.0 * d + 1e-13


def _tolerance(solver):
    """(rtol, floor in units of the first history entry) of the solver's own path tests"""
    if solver in ("cg", "gmres"):
        return 1e-10, 100 * EPS
    if solver == "bicgstab":
        return _bicgstab_rtol(), 100 * EPS
    return 1e-8, 1e-12


def _check_solver(K, ctx, solver, last_path=None, **kw):
    kw = dict(kw, last_path=last_path)
    default_nt = ctx.get_option("nt_min_elems")
    assert default_nt > max(SIZES)                     # the default launches nothing non-temporal at these sizes
    rtol, floor = _tolerance(solver)
    for n in SIZES:
        for fused in (2, 1):
            for comp in (1, 0):
                runs = {}
                for first in (0, 1):
                    with _Options(ctx, compensated=comp):
                        plain = _solve(K, ctx, solver, n, first, fused, **kw)
                        with _Options(ctx, nt_min_elems=1):
                            nt = _solve(K, ctx, solver, n, first, fused, **kw)
                    where = (solver, n, fused, comp, first)
                    assert plain[2:] == nt[2:], (where, plain[2:], nt[2:])
                    for a, b in zip(plain[0] + plain[1], nt[0] + nt[1]):
                        assert _bits(a) == _bits(b), where
                    runs[first] = plain
                # the 8-byte path against the 16-byte path: the same elementwise expressions, dots folded in another order
                (x0, h0, it0, st0), (x1, h1, it1, st1) = runs[0], runs[1]
                for a, b in zip(h1, h0):
                    k = min(len(a), len(b))
                    dev = float(np.max(np.abs(a[:k] - b[:k]) / (rtol * np.abs(b[:k]) + floor * b[0]))) if k else 0.0
                    print(f"{solver} n={n} fused={fused} compensated={comp}: offset 1 against offset 0, history {dev:.3e} of the tolerance")
                    assert len(a) == len(b) and dev <= 1.0, (solver, n, fused, comp, dev)
                for a, b in zip(x1, x0):
                    dx = float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
                    print(f"{solver} n={n} fused={fused} compensated={comp}: offset 1 against offset 0, x {dx:.3e} max|x|")
                    assert dx <= 1e-8, (solver, n, fused, comp, dx)
                assert (it0, st0) == (it1, st1), (solver, n, fused, comp, it0, st0, it1, st1)


@pytest.mark.parametrize("solver", ["cg", "bicgstab", "gmres", "minres", "cg_lanczos_shift", "bilq"])
def test_solver_bits_do_not_depend_on_cache_hints(K, ctx, solver):
    _check_solver(K, ctx, solver)


def test_cg_without_the_deferred_x_update(K, ctx):
    """cg_update_dev_kernel in place of the three modes of cg_defer_kernel"""
    with _Options(ctx, cg_defer_x=0):
        _check_solver(K, ctx, "cg")


def test_gmres_block_gram_schmidt(K, ctx):
    """variant = 1: multi_dot4_kernel on k = 5 basis vectors (a group of four and a group of one) and multi_axpy_dev_kernel"""
    for n in SIZES:
        for first in (0, 1):
            for comp in (1, 0):
                with _Options(ctx, compensated=comp):
                    ws = _workspace(K, ctx, "gmres", n, first)
                    K.gmres_(ws, _operator(K, ctx, n), ctx.array(_rhs(n)), variant=1, **SOLVE)
                    plain = (ws.x.to_host(), np.array(ws.stats.residuals), ws.stats.niter, ws.stats.status)
                    with _Options(ctx, nt_min_elems=1):
                        ws = _workspace(K, ctx, "gmres", n, first)
                        K.gmres_(ws, _operator(K, ctx, n), ctx.array(_rhs(n)), variant=1, **SOLVE)
                        nt = (ws.x.to_host(), np.array(ws.stats.residuals), ws.stats.niter, ws.stats.status)
                assert plain[2:] == nt[2:] and _bits(plain[0]) == _bits(nt[0]) and _bits(plain[1]) == _bits(nt[1]), (n, first, comp)
                assert n == 2 or plain[2] == 6                  # the sixth iteration orthogonalises against five vectors


# ---- the primitives ----------------------------------------------------------------------------------------------------------------
def _primitives(K, ctx, n, first):
    """every BLAS-1 primitive and fused pass of the mirror, each on fresh inputs -> {name: bits of what it wrote or returned}"""
    rng = np.random.default_rng(7 * n + first)
    host = {k: rng.standard_normal(n) for k in "abcdef"}
    host["d"] = np.abs(host["d"]) + 0.5                                 # a divisor
    basis_host = [rng.standard_normal(n) for _ in range(5)]
    buf, v = _carved(ctx, n, list("abcdef") + [f"V{i}" for i in range(5)], first)
    V = [v[f"V{i}"] for i in range(5)]
    out = {}

    def fresh():
        for k in "abcdef":
            v[k].copy_from_host(host[k])
        for u, hv in zip(V, basis_host):
            u.copy_from_host(hv)
        return v["a"], v["b"], v["c"], v["d"], v["e"], v["f"]

    def keep(name, *results):
        out[name] = b"".join(_bits(r.to_host() if isinstance(r, K.DeviceVector) else r) for r in results)

    a, b, c, d, e, f = fresh(); keep("copy", K.kcopy_(n, a, b))
    a, b, c, d, e, f = fresh(); keep("fill", K.kfill_(a, 1.25))
    a, b, c, d, e, f = fresh(); keep("scal", K.kscal_(n, 1.7, a))
    a, b, c, d, e, f = fresh(); keep("div", K.kdiv_(n, a, 1.7))
    a, b, c, d, e, f = fresh(); keep("scalcopy", K.kscalcopy_(n, a, 1.7, b))
    a, b, c, d, e, f = fresh(); keep("divcopy", K.kdivcopy_(n, a, b, 1.7))
    a, b, c, d, e, f = fresh(); keep("axpy", K.kaxpy_(n, 1.7, a, b))
    a, b, c, d, e, f = fresh(); keep("axpby", K.kaxpby_(n, 1.7, a, -0.3, b))
    a, b, c, d, e, f = fresh(); keep("ref", *K.kref_(n, a, b, 0.6, 0.8))
    a, b, c, d, e, f = fresh(); keep("vmul", K.kvmul_(n, c, a, b))
    a, b, c, d, e, f = fresh(); keep("vdiv", K.kvdiv_(n, c, a, d))
    a, b, c, d, e, f = fresh(); keep("waxpy", K.waxpy_(n, c, a, -0.3, b))
    a, b, c, d, e, f = fresh(); keep("cg_update", *K.cg_update_(n, 0.7, 0.2, a, b, c))
    a, b, c, d, e, f = fresh(); K.bicgstab_sx_(n, 0.7, a, b, c, e, f); keep("bicgstab_sx", e, f)
    a, b, c, d, e, f = fresh(); K.bicgstab_p_(n, 0.7, 0.2, a, b, c); keep("bicgstab_p", c)
    a, b, c, d, e, f = fresh(); keep("dot", [K.kdot(n, a, b)])
    a, b, c, d, e, f = fresh(); keep("dot_aliased", [K.kdot(n, a, a)])
    a, b, c, d, e, f = fresh(); keep("nrm2", [K.knorm(n, a)])
    a, b, c, d, e, f = fresh(); keep("dot2", list(K.dot2(n, a, b)))
    a, b, c, d, e, f = fresh(); keep("axpy2_dot", [K.axpy2_dot(n, 0.7, a, b, c, e)], c, e)
    a, b, c, d, e, f = fresh(); keep("axpy_sqnorm", [K.axpy_sqnorm(n, 0.7, a, b)], b)
    a, b, c, d, e, f = fresh(); keep("cg_setup", [K.cg_setup_(n, a, b, c, e)], b, c, e)
    a, b, c, d, e, f = fresh(); keep("bicgstab_xr", list(K.bicgstab_xr_(n, 0.7, a, b, c, d, e, f)), e, f)
    a, b, c, d, e, f = fresh(); keep("bicgstab_xr_z_is_s", list(K.bicgstab_xr_(n, 0.7, a, b, a, d, e, f)), e, f)
    a, b, c, d, e, f = fresh(); h, nrm = K.mgs_(n, V[:3], a); keep("mgs", h, [nrm], a)
    a, b, c, d, e, f = fresh(); keep("multi_axpy", K.multi_axpy_(n, [0.5, -0.25, 2.0, 1.5, -3.0], V, a))
    return out


@pytest.mark.parametrize("n", [1, 2, 511, 513])
@pytest.mark.parametrize("first", [0, 1])
def test_primitive_bits_do_not_depend_on_cache_hints(K, ctx, n, first):
    for comp in (1, 0):
        with _Options(ctx, compensated=comp):
            plain = _primitives(K, ctx, n, first)
            with _Options(ctx, nt_min_elems=1):
                nt = _primitives(K, ctx, n, first)
        assert len(plain) == 26 and list(plain) == list(nt)
        differ = [k for k in plain if plain[k] != nt[k]]
        assert not differ, (n, first, comp, differ)
