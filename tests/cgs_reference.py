"""Test-side NumPy restatement of cgs! (src/cgs.jl:126-281, real Float64), line by line, with an injectable `dot` for kdot
(knorm(x) = sqrt(dot(x, x))).  A checker, not product code: tests/test_cgs_host.py and tests/test_gpu_cgs.py compare the
library's three loops with it.  The exactly summed dot is that of tests/bilq_reference.py."""
import math
import time
from types import SimpleNamespace

import numpy as np

from bilq_reference import EPS, _op, fsum_dot, history_deviation  # noqa: F401  (re-exported for the tests)

SOLVED = "solution good enough given atol and rtol"
TIRED = "maximum number of iterations exceeded"
BREAKDOWN = "breakdown αₖ == 0"
ZERO_RESIDUAL = "x is a zero-residual solution"
BC_BREAKDOWN = "Breakdown bᴴc = 0"


def cgs(A, b, x0=None, c=None, M=None, N=None, atol=math.sqrt(EPS), rtol=math.sqrt(EPS), itmax=0, timemax=math.inf,
        history=True, callback=None, dot=np.dot):
    """A, M, N: callables v -> op v or objects with `@`.  Returns (x, stats); stats.vectors holds u, p, q, r by the names of the
    reference's variables at the end of the loop."""
    start = time.perf_counter()
    mul = _op(A)
    Mop, Nop = _op(M), _op(N)
    norm = lambda v: math.sqrt(float(dot(v, v)))  # noqa: E731
    b = np.asarray(b, dtype=np.float64)
    c = b if c is None else np.asarray(c, dtype=np.float64)
    n = b.shape[0]
    st = SimpleNamespace(niter=0, solved=False, inconsistent=False, status="unknown", residuals=[], vectors={})

    def done(x):
        st.residuals = np.array(st.residuals)
        return x, st

    dx = None if x0 is None else np.asarray(x0, dtype=np.float64)
    r0 = b.copy() if dx is None else b - mul(dx)                             # :161-166
    x = np.zeros(n)                                                          # :168
    r = r0 if Mop is None else Mop(r0)                                       # :169
    rNorm = norm(r)                                                          # :172
    if history:
        st.residuals.append(rNorm)
    if rNorm == 0:                                                           # :174-182
        st.solved, st.status = True, ZERO_RESIDUAL
        return done(x if dx is None else x + dx)
    rho = float(dot(c, r))                                                   # :185
    if rho == 0:                                                             # :186-194
        st.status = BC_BREAKDOWN
        return done(x if dx is None else x + dx)
    it = 0                                                                   # :196-197
    if itmax == 0:
        itmax = 2 * n
    eps = atol + rtol * rNorm                                                # :199
    u = r.copy()                                                             # :203-205
    p = r.copy()
    q = np.zeros(n)
    solved = rNorm <= eps                                                    # :208-213
    tired = it >= itmax
    breakdown = user_exit = overtimed = False
    with np.errstate(all="ignore"):                       # the breakdown case divides by σ = 0 on purpose, as the reference does
        while not (solved or tired or breakdown or user_exit or overtimed):
            y = p if Nop is None else Nop(p)                                 # :217
            t = mul(y)                                                       # :218
            v = t if Mop is None else Mop(t)                                 # :219
            sigma = float(dot(c, v))                                         # :220
            alpha = np.float64(rho) / np.float64(sigma)                      # :221 (IEEE: x / 0 = Inf or NaN, no exception)
            alpha = float(alpha)
            q = u + (-alpha) * v                                             # :222-223
            u = u + 1.0 * q                                                  # :224
            z = u if Nop is None else Nop(u)                                 # :225
            x = x + alpha * z                                                # :226
            s = mul(z)                                                       # :227
            w = s if Mop is None else Mop(s)                                 # :228
            r = r + (-alpha) * w                                             # :229
            rho_next = float(dot(c, r))                                      # :230
            beta = float(np.float64(rho_next) / np.float64(rho))             # :231
            u = r + beta * q                                                 # :232-233
            p = 1.0 * q + beta * p                                           # :234
            p = 1.0 * u + beta * p                                           # :235
            rho = rho_next                                                   # :238
            it += 1                                                          # :241
            rNorm = norm(r)                                                  # :244
            if history:
                st.residuals.append(rNorm)
            resid_decrease_mach = rNorm + 1.0 <= 1.0                         # :249
            if callback is not None:                                         # :252
                st.niter = it
                user_exit = bool(callback(SimpleNamespace(x=x, stats=st)))
            resid_decrease_lim = rNorm <= eps                                # :253
            solved = resid_decrease_lim or resid_decrease_mach               # :254
            tired = it >= itmax                                              # :255
            breakdown = alpha == 0 or math.isnan(alpha)                      # :256
            overtimed = (time.perf_counter() - start) > timemax              # :257-258
    status = "unknown"                                                       # :264-268
    if tired:
        status = TIRED
    if breakdown:
        status = BREAKDOWN
    if solved:
        status = SOLVED
    if user_exit:
        status = "user-requested exit"
    if overtimed:
        status = "time limit exceeded"
    st.vectors = dict(u=u, p=p, q=q, r=r)
    if dx is not None:                                                       # :271
        x = x + dx
    st.niter, st.solved, st.status = it, bool(solved), status
    return done(x)
