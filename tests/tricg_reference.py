"""Test-side NumPy restatement of tricg! (src/tricg.jl:149-484, real Float64, M = N = I), line by line, with an injectable `dot`
for kdot and knorm (knorm(x) = sqrt(dot(x, x))).  A checker, not product code: tests/test_tricg_host.py and
tests/test_gpu_tricg.py compare the library's three loops with it.  The exactly summed dot is that of tests/bilq_reference.py.
Every scalar is an np.float64, so a zero divisor gives inf (or nan) as in the reference and raises nothing.

`fault` swaps ONE line for a plausible slip (tests/test_tricg_host.py shows that the comparison rejects each of them):
  "g_rotation_swapped"  after @kswap! the x and y updates take (g₂ₖ₋₁, g₂ₖ) the other way round
  "guard_ne_zero"       the guards of the shift are `≠ 0` in place of `> btol` (breakdown keeps its btol)
  "sigma_for_eta"       gₓ/gᵧ₂ₖ₋₁ = λₖ g₂ₖ₋₂ + σₖ g₂ₖ₋₃ in place of ηₖ g₂ₖ₋₃
  "no_delta_in_gy"      gy₂ₖ = uₖ − (…) without −δₖ gy₂ₖ₋₁
  "pi_swapped"          π₂ₖ₋₂ and π₂ₖ₋₃ change places in the shift
  "zeta_without_delta"  ζ₂ₖ₋₁ = π₂ₖ₋₁ without −δₖ π₂ₖ"""
import math
import time
from types import SimpleNamespace

import numpy as np

from bilq_reference import EPS, _op, fsum_dot  # noqa: F401  (re-exported for the tests)

TIRED = "maximum number of iterations exceeded"
SOLVED = "solution good enough given atol and rtol"
INCONSISTENT = "inconsistent linear system"
# every status string of src/tricg.jl:278, :466-470
STATUSES = ("unknown", TIRED, INCONSISTENT, SOLVED, "user-requested exit", "time limit exceeded")
FAULTS = ("g_rotation_swapped", "guard_ne_zero", "sigma_for_eta", "no_delta_in_gy", "pi_swapped", "zeta_without_delta")
# the work vectors by the names of khip_tricg_vector, in TricgWorkspace's order
VECTORS = ("y", "u_prev", "u", "p", "gy_prev", "gy", "x", "v_prev", "v", "q", "gx_prev", "gx")
ROW_SIDE = ("x", "v_prev", "v", "q", "gx_prev", "gx", "dx")
BTOL = EPS ** 0.75
F = np.float64


def tricg(A, b, c, x0=None, y0=None, At=None, tau=1.0, nu=-1.0, spd=False, snd=False, flip=False, atol=math.sqrt(EPS),
          rtol=math.sqrt(EPS), itmax=0, timemax=math.inf, history=True, callback=None, dot=np.dot, fault=None):
    """A, At: callables v -> op v or objects with `@` (At defaults to A.T); A has m rows and n columns, b has m entries, c has n.
    Returns (x, y, stats); stats.vectors holds the work vectors by the names of the reference's variables at the end of the solve."""
    assert fault is None or fault in FAULTS
    start = time.perf_counter()
    mul = _op(A)
    mult = _op(At) if At is not None else (lambda v: A.T @ v)
    norm = lambda v: F(math.sqrt(float(dot(v, v))))  # noqa: E731
    b = np.asarray(b, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    m, n = b.shape[0], c.shape[0]
    if spd and flip:                                                         # :162-164
        raise ValueError("The matrix cannot be SPD and SQD")
    if snd and flip:
        raise ValueError("The matrix cannot be SND and SQD")
    if spd and snd:
        raise ValueError("The matrix cannot be SPD and SND")
    if flip:                                                                 # :176-178
        tau, nu = -1.0, 1.0
    if spd:
        tau, nu = 1.0, 1.0
    if snd:
        tau, nu = -1.0, -1.0
    tau, nu = F(tau), F(nu)
    st = SimpleNamespace(niter=0, solved=False, inconsistent=False, status="unknown", residuals=[], vectors={})
    assert (x0 is None) == (y0 is None), "warm_start!(workspace, x0, y0) takes both"
    dx = None if x0 is None else np.asarray(x0, dtype=np.float64)
    dy = None if y0 is None else np.asarray(y0, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        x = np.zeros(m)                                                      # :205-206
        y = np.zeros(n)
        it = 0                                                               # :208-209
        if itmax == 0:
            itmax = m + n
        v_prev = np.zeros(m)                                                 # :212-213
        u_prev = np.zeros(n)
        b0, c0 = b, c
        if dx is not None:                                                   # :217-224
            b0 = mul(dy)
            if tau != 0:
                b0 = b0 + tau * dx
            b0 = b - b0
            c0 = mult(dx)
            if nu != 0:
                c0 = c0 + nu * dy
            c0 = c - c0
        v = b0.copy()                                                        # :227-237
        beta = norm(v)
        v = v * (F(1.0) / beta) if beta != 0 else np.zeros(m)
        u = c0.copy()                                                        # :240-250
        gamma = norm(u)
        u = u * (F(1.0) / gamma) if gamma != 0 else np.zeros(n)
        gx1, gy1, gx2, gy2 = np.zeros(m), np.zeros(n), np.zeros(m), np.zeros(n)   # gx₂ₖ₋₁, gy₂ₖ₋₁, gx₂ₖ, gy₂ₖ (:253-256)
        rNorm = F(math.sqrt(gamma * gamma + beta * beta))                    # :259-261
        if history:
            st.residuals.append(float(rNorm))
        eps = atol + rtol * rNorm
        d_m3 = d_m2 = F(0.0)                                                 # :267-269
        pi_m3 = pi_m2 = F(0.0)
        delta_prev = F(0.0)
        q = np.zeros(m)
        p = np.zeros(n)
        breakdown = False                                                    # :275-280
        solved = bool(rNorm <= eps)
        tired = it >= itmax
        user_exit = overtimed = False
        while not (solved or tired or breakdown or user_exit or overtimed):
            it += 1                                                          # :284
            q = mul(u)                                                       # :290-291
            p = mult(v)
            if it >= 2:                                                      # :293-296
                q = q - gamma * v_prev
                p = p - beta * u_prev
            alpha = F(dot(v, q))                                             # :298
            q = q - alpha * v                                                # :300-301
            p = p - alpha * u
            v_prev = v                                                       # :304-305
            u_prev = u
            if it == 1:                                                      # :330-341
                d1 = tau
                delta = alpha / d1
                d2 = nu - (delta * delta) * d1
            else:
                sigma = beta / d_m2
                eta = gamma / d_m3
                lam = -(eta * delta_prev * d_m3) / d_m2
                d1 = tau - (sigma * sigma) * d_m2
                delta = (alpha - lam * sigma * d_m2) / d1
                d2 = nu - (eta * eta) * d_m3 - (lam * lam) * d_m2 - (delta * delta) * d1
            if it == 1:                                                      # :355-361
                pi1 = beta / d1
                pi2 = (gamma - delta * beta) / d2
            else:
                pi1 = -(sigma * d_m2 * pi_m2) / d1
                pi2 = -(delta * d1 * pi1 + lam * d_m2 * pi_m2 + eta * d_m3 * pi_m3) / d2
            if it == 1:                                                      # :364-369
                gx1 = v.copy()
                gx2 = (-delta) * gx1
                gy2 = u.copy()
            else:                                                            # :384-396
                e = sigma if fault == "sigma_for_eta" else eta
                gx1 = lam * gx2 + e * gx1
                gy1 = lam * gy2 + e * gy1
                gx2 = 1.0 * v + (-sigma) * gx2
                gy2 = (-sigma) * gy2
                gx1 = (-delta) * gx2 + (-1.0) * gx1
                gy1 = 1.0 * u + (-1.0) * gy1
                if fault != "no_delta_in_gy":
                    gy1 = gy1 + (-delta) * gy2
                gx1, gx2 = gx2, gx1
                gy1, gy2 = gy2, gy1
            if fault == "g_rotation_swapped" and it >= 2:
                gx1, gx2 = gx2, gx1
                gy1, gy2 = gy2, gy1
            x = x + pi1 * gx1                                                # :400-405
            x = x + pi2 * gx2
            y = y + pi1 * gy1
            y = y + pi2 * gy2
            beta_next = norm(q)                                              # :411-412
            gamma_next = norm(p)
            if (beta_next != 0) if fault == "guard_ne_zero" else (beta_next > BTOL):     # :415-426
                q = q * (F(1.0) / beta_next)
            if (gamma_next != 0) if fault == "guard_ne_zero" else (gamma_next > BTOL):
                p = p * (F(1.0) / gamma_next)
            v = q.copy()                                                     # :431-432
            u = p.copy()
            zeta1 = pi1 if fault == "zeta_without_delta" else pi1 - delta * pi2           # :435-438
            zeta2 = pi2
            gz, bz = gamma_next * zeta1, beta_next * zeta2
            rNorm = F(math.sqrt(gz * gz + bz * bz)) if not math.isnan(gz * gz + bz * bz) else F(math.nan)
            if history:
                st.residuals.append(float(rNorm))
            beta, gamma = beta_next, gamma_next                              # :441-447
            pi_m3, pi_m2 = (pi2, pi1) if fault == "pi_swapped" else (pi1, pi2)
            d_m3, d_m2 = d1, d2
            delta_prev = delta
            mach = bool(rNorm + 1 <= 1)                                      # :451-460
            if callback is not None:
                st.niter = it
                user_exit = bool(callback(SimpleNamespace(x=x, y=y, stats=st)))
            lim = bool(rNorm <= eps)
            breakdown = bool(beta_next <= BTOL and gamma_next <= BTOL)
            solved = lim or mach
            tired = it >= itmax
            overtimed = (time.perf_counter() - start) > timemax
    status = "unknown"                                                       # :466-470
    for cond, text in ((tired, TIRED), (breakdown, INCONSISTENT), (solved, SOLVED), (user_exit, "user-requested exit"),
                       (overtimed, "time limit exceeded")):
        if cond:
            status = text
    if dx is not None:                                                       # :473-474
        x = x + dx
        y = y + dy
    st.vectors = dict(y=y, u_prev=u_prev, u=u, p=p, gy_prev=gy1, gy=gy2, x=x, v_prev=v_prev, v=v, q=q, gx_prev=gx1, gx=gx2)
    st.niter, st.solved, st.status = it, bool(solved), status
    st.inconsistent = bool(not solved and breakdown)
    st.breakdown = bool(breakdown)
    st.residuals = np.array(st.residuals)
    return x, y, st
