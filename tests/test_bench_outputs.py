"""bench.py --dump-outputs DIR: what the timed cg! returned after its last timed step, written as float64 .npy files so that two
builds of the project can be compared output for output; and --steps is the number of timed iterations behind ms_per_step."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_mod", BENCH)
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


class _HostVector:
    def __init__(self, a):
        self.a = a

    def to_host(self):
        return self.a.copy()


class _Stats:
    niter = 3
    residuals = np.array([4.0, 2.0, 1.0, 0.5])


class _Workspace:
    """What dump_outputs reads of a CgWorkspace: x (to_host) and stats."""

    def __init__(self, x):
        self.x, self.stats = _HostVector(x), _Stats()


def test_dump_outputs_samples_large_solutions_reproducibly(tmp_path):
    """Above DUMP_SAMPLE rows: a fixed, seeded sample of x in global row order, the same rows on every run, beside its row indices;
    every file float64 and the whole dump under 64 MB."""
    bench = _bench_module()
    n = bench.DUMP_SAMPLE * 3 + 17
    x = np.random.default_rng(1).standard_normal(n)
    dirs = [tmp_path / "a", tmp_path / "b"]
    for d in dirs:
        bench.dump_outputs(str(d), _Workspace(x), n, 0, n, 0, None)
    got = [{name: np.load(d / f"{name}.npy") for name in ("x", "x_index", "residuals", "niter")} for d in dirs]
    for name in got[0]:
        assert got[0][name].dtype == np.float64 and np.array_equal(got[0][name], got[1][name]), name
    idx = got[0]["x_index"].astype(np.int64)
    assert idx.size == bench.DUMP_SAMPLE and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < n
    assert np.array_equal(got[0]["x"], x[idx])
    assert np.array_equal(got[0]["residuals"], _Stats.residuals) and got[0]["niter"].tolist() == [3.0]
    assert sum(f.stat().st_size for f in dirs[0].iterdir()) <= 64 << 20


def test_dump_outputs_of_one_rank_of_several(tmp_path):
    """A row block of a partitioned run: the rank's own rows of the sample are picked from its local x (rank 0 of one writes all)."""
    bench = _bench_module()
    n = 1000
    x = np.arange(n, dtype=np.float64) * 0.5
    bench.dump_outputs(str(tmp_path), _Workspace(x[:n]), n, 0, n, 0, None)
    assert np.array_equal(np.load(tmp_path / "x.npy"), x) and np.array_equal(np.load(tmp_path / "x_index.npy"), np.arange(n))
    other = tmp_path / "rank1"
    bench.dump_outputs(str(other), _Workspace(x[400:]), n, 400, n, 1, None)     # not rank 0: nothing written
    assert not other.exists()


@pytest.mark.gpu
def test_bench_dumps_the_last_timed_step(tmp_path, oracle):
    """48^3, 7 timed steps: niter = 7, the residual history and the solution of those 7 iterations (all 110592 rows: below the
    sample size) agree with the oracle's cg! stopped after 7 iterations, and ms_per_step is the time of one of them."""
    n1, steps = 48, 7
    out_dir = tmp_path / "out"
    p = subprocess.run([sys.executable, BENCH, "--n1", str(n1), "--steps", str(steps), "--warmup", "2", "--no-cpu-baseline",
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["ms_per_step"] > 0
    assert d["ms_per_step"] == pytest.approx(1e3 / d["value"], rel=1e-9)
    got = {name: np.load(out_dir / f"{name}.npy") for name in ("x", "x_index", "residuals", "niter")}
    assert all(a.dtype == np.float64 for a in got.values())
    A = oracle.poisson3d(n1)
    ref = oracle.cg(A, np.ones(A.n), atol=0.0, rtol=0.0, itmax=steps, history=True)
    assert ref.niter == steps and got["niter"].tolist() == [float(steps)]
    assert np.array_equal(got["x_index"], np.arange(A.n, dtype=np.float64))
    assert got["residuals"].shape == ref.residuals.shape
    assert float(np.max(np.abs(got["residuals"] - ref.residuals) / ref.residuals)) <= 1e-9
    assert np.allclose(got["x"], ref.x, rtol=0, atol=1e-9 * np.abs(ref.x).max())


@pytest.mark.gpu
def test_plain_run_leaves_the_side_legs_to_full():
    """Without --full the line carries the headline and what the timed steps give, and none of the legs that take runs of
    their own: no parity or self-consistency leg, no CPU baseline, no int32-column roofline, no cfg 3 / cfg 5, no A/B."""
    p = subprocess.run([sys.executable, BENCH, "--n1", "48", "--steps", "5", "--warmup", "2"], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["metric"] == "cg_iters_per_sec_poisson3d_csr_512cubed" and d["unit"] == "iter/s" and d["dtype"] == "f64"
    assert d["higher_is_better"] is True and d["steps"] == 5 and d["ms_per_step"] == pytest.approx(1e3 / d["value"], rel=1e-9)
    assert d["full"] is False and "cpu_baseline" not in d
    for key in ("parity", "self_consistency", "roofline_int32_csr", "single_reduction_cg", "cfg3_gmres", "cfg5_block_gmres", "ab"):
        assert d[key] is None, key
    assert d["roofline"]["avg_ms"] > 0 and d["roofline"]["launches_per_iteration"] == 1.0     # from the timed steps' own brackets
