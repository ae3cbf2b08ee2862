"""Model of the MFMA panel kernels (csrc/panel.hip): launch geometry, rounding counts, exact references, input families that
are exact by construction, and a NumPy emulation of the summation partition with injectable faults.

Imported by tests/test_panel_model_host.py (no GPU: the model against the sources, the references against the emulation,
every injected fault rejected) and tests/test_gpu_panel_exact.py (the kernels against the same references).

Geometry (tn_plan / tn_reduce): a panel holds n_pad = n rounded up to PAD rows; a wave of the V'Q kernels folds ROWS_PER_WAVE
consecutive rows, a workgroup adds its WAVES_PER_WG waves (tn_publish) into ONE tile, panel_tn_reduce_kernel sums FAN
consecutive tiles per group and is launched until one tile is left, ping-ponging between two scratch regions.

Error bounds (derived from the code, not measured):
  V'Q     |Psi_dev[i,j] - exact| <= gamma(tn_roundings + 1) * sum_r |V[r,i]| |Q[r,j]|
  V Psi   |Q_dev[r,c]  - exact| <= gamma(2 p + 2) * (|alpha| sum_k |V[r,k]| |Psi[k,c]| + |beta Q[r,c]|)
with gamma(m) = m u / (1 - m u).  tn_roundings counts, on the longest path to one entry: 2 per product a wave folds (whether
v_mfma_f64_16x16x4_f64 rounds a product before adding it is not documented, so product and addition are counted), the
additions of tn_publish, the additions of every reduce launch; + 1 is the rounding of the correctly rounded reference.  The
update is p products and p - 1 effective additions (the first adds to zero), beta * q, and the final fma: 2 p + 1, + 1 for the
reference.  Additions of exact zeros (padding rows, zero-filled columns, waves past the panel) round nothing.
"""
import math
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import exact_reduction as er

PAD = 16               # pad16 (panel.hip)
ROWS_PER_WAVE = 256    # kRowsPerWaveTN (panel.hip, default of KHIP_ROWS_PER_WAVE_TN)
WAVES_PER_WG = 4       # kWavesPerBlock = kBlock / 64 (device_reduce.hpp)
FAN = 64               # kTnFan (panel.hip)
PSI_SLOTS = 64         # kPsiSlots (panel.hip): the fused sweep runs while k + 2 < PSI_SLOTS
MULTI_NN = 32          # kMultiNN (panel.hip)
LDS_FACTOR_BYTES = 48 * 1024

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "krylov.jl_amd", "csrc")


def constants_in_sources():
    """The constants above as the C++ sources state them (regular expressions over panel.hip / device_reduce.hpp)."""
    panel = open(os.path.join(_CSRC, "panel.hip")).read()
    red = open(os.path.join(_CSRC, "device_reduce.hpp")).read()

    def one(pattern, text):
        m = re.findall(pattern, text)
        assert len(m) == 1, (pattern, m)
        return m[0]

    # pad16: (n + 15) & ~15
    a, b = one(r"int64_t pad16\(int64_t n\) \{ return \(n \+ (\d+)\) & ~\(int64_t\)(\d+); \}", panel)
    assert a == b
    block = int(one(r"constexpr int kBlock = (\d+);", red))
    wave = int(one(r"constexpr int kWavesPerBlock = kBlock / (\d+);", red))
    return {
        "PAD": int(a) + 1,
        "ROWS_PER_WAVE": int(one(r"#define KHIP_ROWS_PER_WAVE_TN (\d+)", panel)),
        "rows_per_wave_is_the_macro": one(r"constexpr int kRowsPerWaveTN = (\w+);", panel) == "KHIP_ROWS_PER_WAVE_TN",
        "WAVES_PER_WG": block // wave,
        "FAN": int(one(r"constexpr int kTnFan = (\d+);", panel)),
        "PSI_SLOTS": int(one(r"constexpr int kPsiSlots = (\d+);", panel)),
        "MULTI_NN": int(one(r"constexpr int kMultiNN = (\d+);", panel)),
        "LDS_FACTOR_BYTES": int(one(r"T > 0 && lds <= (\d+) \* 1024", panel)) * 1024,
    }


def pad16(n):
    return (n + PAD - 1) // PAD * PAD


def tn_geometry(n, p):
    """Launch geometry of Psi = V'Q on an n x p panel: n_pad, waves that hold rows, workgroups (tn_plan launches one even for
    an empty panel), `reduce` = the tile count each panel_tn_reduce_kernel launch reads (the last launch writes Psi), NT."""
    n_pad = pad16(n)
    waves = -(-n_pad // ROWS_PER_WAVE)
    wgs = max(1, -(-waves // WAVES_PER_WG))
    reduce, count = [], wgs
    while True:
        reduce.append(count)
        groups = -(-count // FAN)
        if groups == 1:
            break
        count = groups
    return {"n_pad": n_pad, "waves": waves, "workgroups": wgs, "reduce": reduce, "NT": 1 if p <= 16 else 2}


def tn_roundings(n, p):
    """Rounding errors on the longest path to one entry of Psi = V'Q (see the module docstring)."""
    g = tn_geometry(n, p)
    m = 2 * min(g["n_pad"], ROWS_PER_WAVE)
    m += min(g["waves"], WAVES_PER_WG) - 1 if g["waves"] > 1 else 0
    m += sum(min(c, FAN) - 1 for c in g["reduce"])
    return m


def tn_bound(V, Q):
    """p x p per-entry bounds of V'Q.  The magnitude sums are a float64 product (relative error n u: nothing to a bound)."""
    n, p = V.shape
    return er.gamma(tn_roundings(n, p) + 1) * (np.abs(V).T @ np.abs(Q))


def nn_roundings(p):
    return 2 * p + 1


def multi_path(p, k, fuse=1, tiles=2):
    """Which of its three forms khip_panel_multi_nn takes: 'lds' (factors in LDS), 'reread', 'sequence' (k gemm_nn calls)."""
    if fuse == 0 or k < 1 or k > MULTI_NN or k + 1 >= PSI_SLOTS:
        return "sequence"
    return "lds" if tiles > 0 and k * p * p * 8 <= LDS_FACTOR_BYTES else "reread"


# ---------------------------------------------------------------------------------------------- references
_POOL = None


def _pool():
    global _POOL
    if _POOL is None:
        _POOL = ThreadPoolExecutor(max_workers=8)      # NumPy releases the GIL inside its loops
    return _POOL


def all_entries(p):
    return [(i, j) for i in range(p) for j in range(p)]


def sample_entries(p):
    """The fixed sample for panels above 70 000 rows: the diagonal, the four corners, one entry per 16 x 16 tile."""
    s = {(i, i) for i in range(p)} | {(0, 0), (0, p - 1), (p - 1, 0), (p - 1, p - 1)}
    for a in range(0, p, 16):
        for b in range(0, p, 16):
            s.add((min(a + 5, p - 1), min(b + 11, p - 1)))
    return sorted(s)


def exact_gram(V, Q, entries):
    """{(i, j): correctly rounded sum_r V[r,i] Q[r,j]} by exact_reduction.exact_dot."""
    Vc, Qc = np.asfortranarray(V), np.asfortranarray(Q)
    vals = _pool().map(lambda ij: er.exact_dot(Vc[:, ij[0]], Qc[:, ij[1]]), entries)
    return dict(zip(entries, vals))


def tn_ratio(Psi, V, Q, entries=None):
    """max over `entries` of |Psi[i,j] - exact| / bound (inf where the bound is zero and the entry is not exact)."""
    p = V.shape[1]
    entries = all_entries(p) if entries is None else entries
    if not np.isfinite(Psi).all():
        return math.inf
    ref, bound = exact_gram(V, Q, entries), tn_bound(V, Q)
    worst = 0.0
    for (i, j), r in ref.items():
        d = abs(float(Psi[i, j]) - r)
        worst = max(worst, (0.0 if d == 0.0 else math.inf) if bound[i, j] == 0.0 else d / bound[i, j])
    return worst


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _dd_add(hi, lo, a, b):
    """(hi, lo) + (a, b) in double-double: relative error of the order 2^-104 of the magnitudes."""
    s, e = _two_sum(hi, a)
    e = e + (lo + b)
    hi2 = s + e
    return hi2, e - (hi2 - s)


def exact_product(V, Psi):
    """V Psi per entry as a double-double (hi, lo): error-free products (two_product) of the p terms, accumulated with TwoSum.
    Good to about 2^-100 of sum_k |V[r,k]| |Psi[k,c]|."""
    n, p = V.shape
    hi, lo = np.zeros((n, p)), np.zeros((n, p))
    for k in range(p):
        a, b = er.two_product(np.broadcast_to(V[:, k:k + 1], (n, p)), np.broadcast_to(Psi[k:k + 1, :], (n, p)))
        hi, lo = _dd_add(hi, lo, a, b)
    return hi, lo


def exact_update(alpha, V, Psi, beta, Q, prod=None):
    """beta Q + alpha V Psi per entry as a double-double: exact_product (or `prod`, the same for another alpha / beta), then
    the two scalings with error-free products again."""
    n, p = V.shape
    hi, lo = exact_product(V, Psi) if prod is None else prod
    a, b = er.two_product(np.full((n, p), float(alpha)), hi)
    return _dd_add(a, b + alpha * lo, *er.two_product(np.full((n, p), float(beta)), Q))


def nn_bound(alpha, V, Psi, beta, Q):
    p = V.shape[1]
    return er.gamma(nn_roundings(p) + 1) * (abs(alpha) * (np.abs(V) @ np.abs(Psi)) + np.abs(beta * Q))


def nn_ratio(out, alpha, V, Psi, beta, Q, prod=None):
    """max |out - exact| / bound over all entries of the update (inf on a non-finite entry or a miss where the bound is zero)."""
    if not np.isfinite(out).all():
        return math.inf
    hi, lo = exact_update(alpha, V, Psi, beta, Q, prod)
    d = np.abs((out - hi) - lo)
    bound = nn_bound(alpha, V, Psi, beta, Q)
    zero = bound == 0.0
    if (d[zero] != 0.0).any():
        return math.inf
    return float((d[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0


# ---------------------------------------------------------------------------------------------- inputs
REAL_FAMILIES = ("normal", "scaled", "cancel")
CANCEL_MIN_ROWS = 64     # gen_dot needs room for its pairs and corrections; below it "cancel" is not defined


def families_for(n):
    return tuple(f for f in REAL_FAMILIES if f != "cancel" or n >= CANCEL_MIN_ROWS)


def _nonzero_ints(rng, hi, shape):
    return rng.integers(1, hi + 1, shape).astype(np.float64) * rng.choice([-1.0, 1.0], shape)


def int_panels(n, p, seed=0):
    """V in -3..3 and Q in -1000..1000 without zeros: every partial sum of V'Q in any order is an integer below 2^53
    (int_condition), so the device must return the integer result bit for bit.  Three columns of Q carry the row's identity
    (r mod 997, 31 r mod 991, r mod 16 -- the last one tells the rows of one tile apart), so that a row read from the wrong
    place changes the result."""
    rng = np.random.default_rng(1000003 * p + n + seed)
    V, Q = _nonzero_ints(rng, 3, (n, p)), _nonzero_ints(rng, 1000, (n, p))
    r = np.arange(n, dtype=np.int64)
    ident = ((r % 997) + 1, ((31 * r) % 991) + 1, (r % 16) + 1)
    for c, col in zip(sorted({0, p // 2, p - 1}), ident):
        Q[:, c] = col
    return V, Q


def int_factor(p, seed=0, lo=4):
    rng = np.random.default_rng(77 * p + seed)
    return _nonzero_ints(rng, lo, (p, p))


def int_condition(n, vmax=3.0, qmax=1000.0):
    """sum |v||q| < 2^53 for the integer panels of n rows."""
    return n * vmax * qmax < 2.0 ** 53


def real_panels(family, n, p, seed=0):
    """V != Q, both asymmetric.  normal: standard normal.  scaled: column c of V times 2^(300 (p - 1 - c) / p) and of Q times
    2^(-300 c / p): entries of V'Q between 2^-300 and 2^300, every product inside exact_reduction's window; the FIRST columns
    are the large ones, so that what a wrong predicate reads past a row's end (the next row's first entry) is not negligible.
    cancel: column c of Q is gen_dot's ill-conditioned partner (condition 1e8) of column c of V, the large cancelling pair in
    the first row of the last wave and in the LAST REAL ROW (next to the padding); off the diagonal the same huge entries meet
    unrelated ones, so only a bound in terms of sum |v||q| can hold."""
    rng = np.random.default_rng(7919 * p + n + 101 * REAL_FAMILIES.index(family) + seed)
    V, Q = rng.standard_normal((n, p)), rng.standard_normal((n, p))
    if family == "scaled":
        e = np.round(300.0 * np.arange(p) / p)
        V, Q = V * np.exp2(e[::-1]), Q * np.exp2(-e)
    elif family == "cancel":
        assert n >= CANCEL_MIN_ROWS
        first = (pad16(n) - 1) // ROWS_PER_WAVE * ROWS_PER_WAVE
        place = (first if first < n - 1 else 0, n - 1)
        for c in range(p):
            x, _, cond = er.gen_dot(n, 1e8, rng, place=place, y=V[:, c])
            assert cond >= 1e7, cond
            Q[:, c] = x
    return V, Q


def real_factor(p, seed=0):
    return np.random.default_rng(31 * p + seed).standard_normal((p, p))


# ---------------------------------------------------------------------------------------------- emulation
TN_FAULTS = ("tail16", "fan63", "stale", "colpred", "transposed")
NN_FAULTS = ("colpred", "transposed")


def emulate_tn(V, Q, fault=None):
    """Psi = V'Q with the kernel's partition in float64: per wave the rows in order, the workgroup's waves in wave order,
    FAN tiles per reduce group in tile order, launch after launch.  Faults (one at a time):
      tail16      the last 16-row tile of the panel is never folded
      fan63       a reduce group adds 63 of its 64 tiles (the launch still strides by 64)
      stale       no ping-pong swap: the second reduce launch reads the workgroup tiles again, not what the first wrote
      colpred     `col <= p` where the last tile is stored: the thread of row p, column c writes over Psi[0, c + 1]
                  (a wrong LOAD predicate alone is masked by the store's; the zero-filled column then holds the next row's first
                  entry, V[r + 1, 0])
      transposed  the A / B operands swapped: Psi'"""
    n, p = V.shape
    g = tn_geometry(n, p)
    wgs = g["workgroups"]
    rows = wgs * WAVES_PER_WG * ROWS_PER_WAVE
    Vp, Qp = np.zeros((rows, p)), np.zeros((rows, p))
    Vp[:n], Qp[:n] = V, Q
    if fault == "tail16":
        Vp[g["n_pad"] - PAD:g["n_pad"]] = 0.0
    Vw, Qw = Vp.reshape(-1, ROWS_PER_WAVE, p), Qp.reshape(-1, ROWS_PER_WAVE, p)
    acc = np.zeros((Vw.shape[0], p, p))
    for r in range(min(ROWS_PER_WAVE, g["n_pad"])):
        acc += Vw[:, r, :, None] * Qw[:, r, None, :]
    acc = acc.reshape(wgs, WAVES_PER_WG, p, p)
    tiles = acc[:, 0].copy()
    for w in range(1, WAVES_PER_WG):
        tiles += acc[:, w]
    first = tiles
    for launch, count in enumerate(g["reduce"]):
        src = first[:count] if (fault == "stale" and launch == 1) else tiles
        assert src.shape[0] == count
        groups = -(-count // FAN)
        out = np.zeros((groups, p, p))
        for gi in range(groups):
            hi = min(gi * FAN + (FAN - 1 if fault == "fan63" else FAN), count)
            for t in range(gi * FAN, hi):
                out[gi] += src[t]
        tiles = out
    Psi = tiles[0]
    if fault == "colpred" and p % 16 != 0:
        nxt = np.zeros(n)
        nxt[:-1] = V[1:, 0]
        Psi = Psi.copy()
        Psi[0, 1:] = (nxt @ Q)[:-1]
    if fault == "transposed":
        Psi = Psi.T.copy()
    return Psi


def emulate_nn(alpha, V, Psi, beta, Q, fault=None):
    """beta Q + alpha V Psi as the kernels order it: the p terms in column order, then alpha * acc + beta * q (two roundings
    where the device's fma has one: inside the count all the same, the first addition being exact).  Faults:
      colpred     `vcol <= p` and `prow <= p`: one term too many, V[r + 1, 0] * Psi[0, c + 1] in the device's memory order
      transposed  Psi read row-major"""
    n, p = V.shape
    if fault == "transposed":
        Psi = Psi.T
    acc = np.zeros((n, p))
    for k in range(p):
        acc += V[:, k:k + 1] * Psi[k:k + 1, :]
    if fault == "colpred" and p % 16 != 0:
        nxt = np.zeros((n, 1))
        nxt[:-1, 0] = V[1:, 0]
        extra = np.zeros((1, p))
        extra[0, :-1] = Psi[0, 1:]
        acc += nxt * extra
    return alpha * acc + beta * Q


# ---------------------------------------------------------------------------------------------- the sizes the GPU tests run
EDGE_WIDTHS = (1, 2, 15, 16, 17, 31, 32)
ROW_EDGES = (1, 15, 16, 17, 255, 256, 257, 272, 1023, 1024, 1025, 1040)     # one tile ... second workgroup
LEVEL_EDGES = (65536, 65537, 100 * 1024 + 1)                                 # one reduce launch / two / two with a partly filled group
EDGE_SIZES = ROW_EDGES + LEVEL_EDGES
THREE_LEVEL = 4194304 + 17                                                   # three reduce launches; widths 16 and 17, integers only
MID_SIZES = (1297, 4369)                                                     # every p in 1..32: two and five workgroups, partial last wave
ALL_ENTRIES_UP_TO = 70000                                                    # rows up to which every entry gets its exact dot
NONFINITE_SIZE = 65537
NONFINITE_ROWS = (0, NONFINITE_SIZE - 1, 65300)    # first row, last real row (next to the padding), last wave of the first reduce group
