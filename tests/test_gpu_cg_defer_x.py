"""cg! with x updated every second iteration (ctx option cg_defer_x, csrc/solvers.cpp cg_device_loop) against the loop that
updates x every iteration (cg_defer_x = 0).  The deferred form evaluates the same expressions on the same operands in the
same order, so whatever ends the loop -- itmax after a light or a heavy iteration, convergence in either, the curvature test
with an x update pending -- x, r, p, Ap, the residual history, niter and the status must be EQUAL BIT FOR BIT.  Each case also
holds the history to the CPU oracle's within the tolerance of tests/test_gpu_solvers.py (|dr_k| <= 1e-10 r_k + 100 eps r_0)."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(float).eps
HIST_RTOL = 1e-10
HIST_FLOOR = 100 * EPS
SHAPES = (3, 11, 16)            # 27 rows (below one workgroup), 1331 (odd n: the tail element of the 16-byte path), 4096
# Poisson(n1) - s I with b = default_rng(100 + n1).standard_normal(n): p.Ap = 0 to within eps pNorm^2 after ONE completed
# iteration, i.e. with the x update of a light iteration pending.  Found with the oracle on the CPU (bisection on p_1' B p_1,
# then a scan of the neighbouring doubles for a shift at which ko_cg stops with "zero curvature detected" and niter = 1).
CURVATURE_SHIFTS = {3: 3.991510987997722, 11: 3.6207393632656744, 16: 3.626916713412626}


def _hist_dev(h_gpu, h_cpu):
    assert len(h_gpu) == len(h_cpu), (len(h_gpu), len(h_cpu))
    if not len(h_cpu):
        return 0.0
    return float(np.max(np.abs(h_gpu - h_cpu) / (HIST_RTOL * h_cpu + HIST_FLOOR * h_cpu[0])))


_CACHE = {}


def _problem(K, ctx, oracle, n1):
    """operator (oracle + device), right-hand side and a start vector of one shape: made once, shared, never changed"""
    if n1 not in _CACHE:
        A = oracle.poisson3d(n1)
        rng = np.random.default_rng(100 + n1)
        bh = rng.standard_normal(A.n)
        x0h = rng.standard_normal(A.n)
        dA = K.CsrMatrix.from_host(ctx, A.rowptr, A.col, A.val, (A.n, A.n))
        _CACHE[n1] = (A, dA, bh, ctx.array(bh), x0h, ctx.array(x0h))
    return _CACHE[n1]


def _workspace(K, ctx, n, kind):
    """library-owned; adopted (the caller's 16-byte aligned vectors); adopted with every vector offset by 8 bytes (the 8-byte path)"""
    if kind == "owned":
        return K.CgWorkspace(ctx, n, n, adopt=False)
    if kind == "adopted":
        return K.CgWorkspace(ctx, n, n, adopt=True)
    ws = K.CgWorkspace.__new__(K.CgWorkspace)
    ws.ctx, ws.m, ws.n, ws.adopted, ws._alloc_s = ctx, n, n, True, 0.0
    ws._h = C.c_void_p()
    ws._vec = {k: ctx.empty(n + 2).slice(1, n + 1) for k in ("x", "r", "p", "Ap")}
    v = ws._vec
    assert all(v[k].ptr % 16 == 8 for k in v)
    rc = K.lib().khip_cg_workspace_adopt(ctx._h, n, n, v["x"].ptr, v["r"].ptr, v["p"].ptr, v["Ap"].ptr, C.byref(ws._h))
    assert rc == 0
    return ws


def _state(ws):
    st = ws.stats
    return {"x": ws.vector("x").to_host(), "r": ws.vector("r").to_host(), "p": ws.vector("p").to_host(),
            "Ap": ws.vector("Ap").to_host(), "residuals": np.array(st.residuals), "niter": st.niter, "status": st.status,
            "solved": st.solved, "inconsistent": st.inconsistent}


def _solve(K, ctx, dA, b, defer, kind="owned", x0=None, ws=None, **kw):
    prev = ctx.get_option("cg_defer_x")
    ctx.set_option("cg_defer_x", defer)
    try:
        if ws is None:
            ws = _workspace(K, ctx, len(b), kind)
        if x0 is not None:
            ws.warm_start_(x0)
        K.cg_(ws, dA, b, fused=2, **kw)
    finally:
        ctx.set_option("cg_defer_x", prev)
    assert ws.last_path == 2                        # the device-resident loop ran
    return _state(ws), ws


def _assert_equal(s0, s1, what):
    for k in ("x", "r", "p", "Ap", "residuals"):
        assert np.array_equal(s0[k], s1[k]), (what, k)
    for k in ("niter", "status", "solved", "inconsistent"):
        assert s0[k] == s1[k], (what, k, s0[k], s1[k])


def _both(K, ctx, oracle, A, dA, bh, b, what, kind="owned", x0h=None, x0=None, **kw):
    s0, _ = _solve(K, ctx, dA, b, 0, kind, x0, **kw)
    s1, _ = _solve(K, ctx, dA, b, 1, kind, x0, **kw)
    _assert_equal(s0, s1, what)
    ref = oracle.cg(A, bh, x0=x0h, **kw)
    assert (s1["niter"], s1["status"]) == (ref.niter, ref.status), (what, s1["niter"], s1["status"], ref.niter, ref.status)
    if kw.get("history"):
        assert _hist_dev(s1["residuals"], ref.residuals) <= 1.0, what
    else:
        assert len(s1["residuals"]) == 0
    return s0, s1


def test_option_defaults_on(K, ctx):
    assert ctx.get_option("cg_defer_x") == 1


@pytest.mark.parametrize("n1", SHAPES)
@pytest.mark.parametrize("itmax", [1, 2, 3, 4, 5, 7, 8])
def test_itmax_either_parity_and_chunk_edges(K, ctx, oracle, n1, itmax):
    """both parities, the edges of the four-at-a-time enqueue, a flush after an odd count"""
    A, dA, bh, b, _, _ = _problem(K, ctx, oracle, n1)
    _, s1 = _both(K, ctx, oracle, A, dA, bh, b, ("itmax", n1, itmax), atol=0.0, rtol=0.0, itmax=itmax, history=True)
    # (the 27-row operator has seven distinct eigenvalues: there the seventh iteration, a light one, ends the solve as solved)
    assert s1["niter"] == itmax or (s1["solved"] and n1 == 3 and s1["niter"] == 7 <= itmax)


@pytest.mark.parametrize("n1", SHAPES)
def test_convergence_in_a_light_and_in_a_heavy_iteration(K, ctx, oracle, n1):
    """rtol from the cg_defer_x = 0 history: the solve converges at iteration k, once for an odd k (its last iteration is a light
    one: that kernel applies its own x update) and once for an even k (heavy: both updates, p_j copied back into p)"""
    A, dA, bh, b, _, _ = _problem(K, ctx, oracle, n1)
    h = _solve(K, ctx, dA, b, 0, atol=0.0, rtol=0.0, itmax=12, history=True)[0]["residuals"]
    seen = set()
    for k in range(1, len(h)):
        if k % 2 in seen or not h[k] < h[:k].min():
            continue
        seen.add(k % 2)
        rtol = 0.5 * (h[k] + h[:k].min()) / h[0]
        _, s1 = _both(K, ctx, oracle, A, dA, bh, b, ("rtol", n1, k), atol=0.0, rtol=rtol, history=True)
        assert s1["niter"] == k and s1["solved"]
    assert seen == {0, 1}


@pytest.mark.parametrize("n1", SHAPES)
@pytest.mark.parametrize("itmax", [3, 4])
def test_warm_start(K, ctx, oracle, n1, itmax):
    A, dA, bh, b, x0h, x0 = _problem(K, ctx, oracle, n1)
    _both(K, ctx, oracle, A, dA, bh, b, ("x0", n1, itmax), x0h=x0h, x0=x0, atol=0.0, rtol=0.0, itmax=itmax, history=True)


@pytest.mark.parametrize("n1", SHAPES)
@pytest.mark.parametrize("itmax", [5, 6])
def test_without_history(K, ctx, oracle, n1, itmax):
    A, dA, bh, b, _, _ = _problem(K, ctx, oracle, n1)
    _both(K, ctx, oracle, A, dA, bh, b, ("nohist", n1, itmax), atol=0.0, rtol=0.0, itmax=itmax, history=False)


@pytest.mark.parametrize("n1", SHAPES)
@pytest.mark.parametrize("kind", ["owned", "adopted", "adopted8"])
def test_workspace_kinds(K, ctx, oracle, n1, kind):
    """the second direction buffer is allocated on first use for adopted workspaces too; vectors at 8 (mod 16) take the 8-byte path"""
    A, dA, bh, b, _, _ = _problem(K, ctx, oracle, n1)
    for itmax in (3, 6):
        _both(K, ctx, oracle, A, dA, bh, b, ("ws", n1, kind, itmax), kind=kind, atol=0.0, rtol=0.0, itmax=itmax, history=True)


@pytest.mark.parametrize("n1", SHAPES)
def test_two_solves_on_one_workspace(K, ctx, oracle, n1):
    """the first solve ends with a flush; the second starts from scratch on the same buffers"""
    A, dA, bh, b, _, _ = _problem(K, ctx, oracle, n1)
    out = {}
    for defer in (0, 1):
        first, ws = _solve(K, ctx, dA, b, defer, atol=0.0, rtol=0.0, itmax=3, history=True)
        second, _ = _solve(K, ctx, dA, b, defer, ws=ws, atol=0.0, rtol=0.0, itmax=6, history=True)
        out[defer] = (first, second)
    _assert_equal(out[0][0], out[1][0], ("two solves, first", n1))
    _assert_equal(out[0][1], out[1][1], ("two solves, second", n1))
    ref = oracle.cg(A, bh, atol=0.0, rtol=0.0, itmax=6, history=True)
    assert out[1][1]["niter"] == ref.niter == 6 and _hist_dev(out[1][1]["residuals"], ref.residuals) <= 1.0


@pytest.mark.parametrize("n1", sorted(CURVATURE_SHIFTS))
def test_curvature_stop_with_an_update_pending(K, ctx, oracle, n1):
    """an indefinite operator whose p.Ap vanishes after an odd number of completed iterations: step 1 lowers stop_seq, the
    light iteration's x update is still pending and its alpha has not been overwritten"""
    A, _, bh, b, _, _ = _problem(K, ctx, oracle, n1)
    rows = np.repeat(np.arange(A.n), np.diff(A.rowptr))
    val = A.val.copy()
    val[A.col == rows] -= CURVATURE_SHIFTS[n1]
    B = oracle.CsrMatrix.from_arrays(A.rowptr.copy(), A.col.copy(), val)
    dB = K.CsrMatrix.from_host(ctx, B.rowptr, B.col, B.val, (A.n, A.n))
    _, s1 = _both(K, ctx, oracle, B, dB, bh, b, ("curvature", n1), atol=0.0, rtol=0.0, itmax=50, history=True)
    assert s1["status"] == "zero curvature detected" and s1["niter"] % 2 == 1 and s1["inconsistent"]


def test_row_partitioned_run_through_the_self_halo():
    """one RCCL rank exchanging its halo with itself (tests/cg_defer_x_halo_worker.py, own process as tests/test_gpu_self_halo.py):
    the halo exchange of a heavy iteration packs from the second direction buffer"""
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "r.json")
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
        try:
            p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cg_defer_x_halo_worker.py"), "16", "4", "12", out],
                               env=env, capture_output=True, text=True, timeout=240)
        except subprocess.TimeoutExpired:
            pytest.fail("the self Send/Recv hangs")
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        r = json.load(open(out))
    assert r["n_ghost"] == 2 * 16 * 16
    for itmax in ("3", "6", "0"):
        c = r["cases"][itmax]
        assert c["last_path"] == [2, 2] and c["niter"][0] == c["niter"][1] and c["status"][0] == c["status"][1], (itmax, c)
        assert all(c["equal"][k] for k in ("x", "r", "p", "Ap", "residuals")), (itmax, c)
        # against the same periodic slab as a plain operator: the dots go through one more (1-rank) combine step, <= 1 ulp per dot
        assert c["niter"][1] == c["plain_niter"] and c["max_rel_dev_plain"] <= 1e-12, (itmax, c)
    assert r["cases"]["3"]["niter"][0] == 3 and r["cases"]["6"]["niter"][0] == 6 and r["cases"]["0"]["niter"][0] > 8
