"""Test-side NumPy restatement of trimr! (src/trimr.jl:150-577, real Float64, M = N = I), line by line, with an injectable `dot`
for kdot and knorm (knorm(x) = sqrt(dot(x, x))).  A checker, not product code: tests/test_trimr_host.py and
tests/test_gpu_trimr.py compare the library's three loops with it.  The exactly summed dot is that of tests/bilq_reference.py.
Every scalar is an np.float64, so a zero divisor gives inf (or nan) as in the reference and raises nothing.

`fault` swaps ONE line for a plausible slip (tests/test_trimr_host.py shows which of them the comparison rejects):
  "g_last_term_old_buffer"  g₂ₖ's last term reads what the buffer of g₂ₖ₋₁ held BEFORE this iteration wrote it
  "swap_after_update_k2"    at k = 2 the three @kswap! come after the four updates, as they do from k = 3 on
  "guard_ne_zero"           the guards of the shift are `≠ 0` in place of `> btol` (breakdown keeps its btol)
  "pibar_swapped"           πbar₂ₖ₊₁ and πbar₂ₖ₊₂ change places in the shift
  "mu_m4_takes_mu_m3"       μ₂ₖ₋₄ = μ₂ₖ₋₃ in the shift, in place of μ₂ₖ₋₂
  "c1_for_c3"               πtmp₂ₖ = c₁ₖ πhat₂ₖ + s₃ₖ πbis₂ₖ₊₂
  "mu_shift_at_k1"          the shift of μ₂ₖ₋₅, μ₂ₖ₋₄ and λ₂ₖ₋₄ already runs at k = 1 (it changes no bit: at k = 1 the three sources are
                            the zeros they start as here -- the reference leaves them undefined -- and nothing reads the three
                            targets before the shift of k = 2 rewrites them)"""
import math
import time
from types import SimpleNamespace

import numpy as np

from bilq_reference import EPS, _op, fsum_dot, sym_givens as _sym_givens  # noqa: F401  (re-exported for the tests)

TIRED = "maximum number of iterations exceeded"
SOLVED = "solution good enough given atol and rtol"
INCONSISTENT = "inconsistent linear system"
# every status string of src/trimr.jl:290, :559-563
STATUSES = ("unknown", TIRED, INCONSISTENT, SOLVED, "user-requested exit", "time limit exceeded")
FAULTS = ("g_last_term_old_buffer", "swap_after_update_k2", "guard_ne_zero", "pibar_swapped", "mu_m4_takes_mu_m3", "c1_for_c3",
          "mu_shift_at_k1")
# the work vectors by the names of khip_trimr_vector, in TrimrWorkspace's order
VECTORS = ("y", "u_prev", "u", "p", "gy_m3", "gy_m2", "gy_m1", "gy", "x", "v_prev", "v", "q", "gx_m3", "gx_m2", "gx_m1", "gx")
ROW_SIDE = ("x", "v_prev", "v", "q", "gx_m3", "gx_m2", "gx_m1", "gx", "dx")
# the six pair errors of :163-168, (flag, flag) -> message
PAIR_ERRORS = {("spd", "flip"): "The matrix cannot be symmetric positive definite and symmetric quasi-definite !",
               ("spd", "snd"): "The matrix cannot be symmetric positive definite and symmetric negative definite !",
               ("spd", "sp"): "The matrix cannot be symmetric positive definite and a saddle-point !",
               ("snd", "flip"): "The matrix cannot be symmetric negative definite and symmetric quasi-definite !",
               ("snd", "sp"): "The matrix cannot be symmetric negative definite and a saddle-point !",
               ("sp", "flip"): "The matrix cannot be symmetric quasi-definite and a saddle-point !"}
BTOL = EPS ** 0.75
F = np.float64


def sym_givens(a, b):
    c, s, rho = _sym_givens(F(a), F(b))
    return F(c), F(s), F(rho)


def g_value(w, terms, delta):
    """One broadcast of :460-476 as it stands: (w .- c₀ .* a₀ .- c₁ .* a₁ …) ./ δ, or with .- c₀ .* a₀ in front when w is None.
    Separately rounded products, subtractions from left to right, one true division."""
    (c0, a0), rest = terms[0], terms[1:]
    t = w - c0 * a0 if w is not None else -(c0 * a0)
    for c, a in rest:
        t = t - c * a
    return t / delta


def trimr(A, b, c, x0=None, y0=None, At=None, tau=1.0, nu=-1.0, spd=False, snd=False, flip=False, sp=False, atol=math.sqrt(EPS),
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
    given = dict(spd=spd, snd=snd, flip=flip, sp=sp)
    for pair, msg in PAIR_ERRORS.items():                                    # :163-168
        if given[pair[0]] and given[pair[1]]:
            raise ValueError(msg)
    if flip:                                                                 # :180-183
        tau, nu = -1.0, 1.0
    if spd:
        tau, nu = 1.0, 1.0
    if snd:
        tau, nu = -1.0, -1.0
    if sp:
        tau, nu = 1.0, 0.0
    tau, nu = F(tau), F(nu)
    st = SimpleNamespace(niter=0, solved=False, inconsistent=False, status="unknown", residuals=[], vectors={})
    assert (x0 is None) == (y0 is None), "warm_start!(workspace, x0, y0) takes both"
    dx = None if x0 is None else np.asarray(x0, dtype=np.float64)
    dy = None if y0 is None else np.asarray(y0, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        x = np.zeros(m)                                                      # :211-212
        y = np.zeros(n)
        it = 0                                                               # :214-215
        if itmax == 0:
            itmax = m + n
        v_prev = np.zeros(m)                                                 # :218-219
        u_prev = np.zeros(n)
        b0, c0 = b, c
        if dx is not None:                                                   # :223-230
            b0 = mul(dy)
            if tau != 0:
                b0 = b0 + tau * dx
            b0 = b - b0
            c0 = mult(dx)
            if nu != 0:
                c0 = c0 + nu * dy
            c0 = c - c0
        v = b0.copy()                                                        # :233-243
        beta = norm(v)
        v = v * (F(1.0) / beta) if beta != 0 else np.zeros(m)
        u = c0.copy()                                                        # :246-256
        gamma = norm(u)
        u = u * (F(1.0) / gamma) if gamma != 0 else np.zeros(n)
        gx_m3, gy_m3, gx_m2, gy_m2 = np.zeros(m), np.zeros(n), np.zeros(m), np.zeros(n)   # :259-266
        gx_m1, gy_m1, gx_0, gy_0 = np.zeros(m), np.zeros(n), np.zeros(m), np.zeros(n)
        rNorm = F(np.sqrt(gamma * gamma + beta * beta))                      # :269-271
        if history:
            st.residuals.append(float(rNorm))
        eps = atol + rtol * rNorm
        old_c1 = old_c2 = old_c3 = old_c4 = F(0.0)                           # :277-281
        old_s1 = old_s2 = old_s3 = old_s4 = F(0.0)
        sigmabar_m2 = etabar_m3 = lambdabar_m3 = mu_m5 = lambda_m4 = mu_m4 = F(0.0)
        pibar1 = beta
        pibar2 = gamma
        mu_m3 = mu_m2 = lambda_m2 = F(0.0)                                   # (undefined in the reference until k = 2)
        q = np.zeros(m)
        p = np.zeros(n)
        breakdown = False                                                    # :287-292
        solved = bool(rNorm <= eps)
        tired = it >= itmax
        user_exit = overtimed = False
        while not (solved or tired or breakdown or user_exit or overtimed):
            it += 1                                                          # :298
            q = mul(u)                                                       # :304-305
            p = mult(v)
            if it >= 2:                                                      # :307-310
                q = q - gamma * v_prev
                p = p - beta * u_prev
            alpha = F(dot(v, q))                                             # :312
            q = q - alpha * v                                                # :314-315
            p = p - alpha * u
            beta_next = norm(q)                                              # :321-322
            gamma_next = norm(p)
            if (beta_next != 0) if fault == "guard_ne_zero" else (beta_next > BTOL):     # :325-336
                q = q * (F(1.0) / beta_next)
            if (gamma_next != 0) if fault == "guard_ne_zero" else (gamma_next > BTOL):
                p = p * (F(1.0) / gamma_next)
            if it == 1:                                                      # :353-360
                thetabar = alpha
                deltabar1 = tau
                deltabar2 = nu
                sigmabar1 = alpha
                sigmabar2 = beta_next
                lambdabar1 = gamma_next
                etabar1 = F(0.0)
            else:                                                            # :377-414
                sigmabis_m2 = old_c1 * sigmabar_m2 + old_s1 * alpha
                etabis_m2 = old_s1 * nu
                lambdabis_m2 = old_s1 * beta_next
                thetabis = old_s1 * sigmabar_m2 - old_c1 * alpha
                deltabis2 = -old_c1 * nu
                sigmabis2 = -old_c1 * beta_next
                eta_m3 = old_c2 * etabar_m3 + old_s2 * sigmabis_m2
                lambda_m3 = old_c2 * lambdabar_m3 + old_s2 * etabis_m2
                mu_m3 = old_s2 * lambdabis_m2
                sigmahat_m2 = old_s2 * etabar_m3 - old_c2 * sigmabis_m2
                etahat_m2 = old_s2 * lambdabar_m3 - old_c2 * etabis_m2
                lambdahat_m2 = -old_c2 * lambdabis_m2
                sigmatmp_m2 = old_c3 * sigmahat_m2 + old_s3 * thetabis
                etatmp_m2 = old_c3 * etahat_m2 + old_s3 * deltabis2
                lambdatmp_m2 = old_c3 * lambdahat_m2 + old_s3 * sigmabis2
                thetabar = old_s3 * sigmahat_m2 - old_c3 * thetabis
                deltabar2 = old_s3 * etahat_m2 - old_c3 * deltabis2
                sigmabar2 = old_s3 * lambdahat_m2 - old_c3 * sigmabis2
                sigma_m2 = old_c4 * sigmatmp_m2 + old_s4 * tau
                eta_m2 = old_c4 * etatmp_m2 + old_s4 * alpha
                lambda_m2 = old_c4 * lambdatmp_m2
                mu_m2 = old_s4 * gamma_next
                deltabar1 = old_s4 * sigmatmp_m2 - old_c4 * tau
                sigmabar1 = old_s4 * etatmp_m2 - old_c4 * alpha
                etabar1 = old_s4 * lambdatmp_m2
                lambdabar1 = -old_c4 * gamma_next
            c1, s1, theta = sym_givens(thetabar, gamma_next)                 # :421-423
            g = s1 * deltabar2
            deltabar2 = c1 * deltabar2
            c2, s2, delta_m1 = sym_givens(deltabar1, theta)                  # :429-431
            sigma_m1 = c2 * sigmabar1 + s2 * deltabar2
            deltabis2 = s2 * sigmabar1 - c2 * deltabar2
            c3, s3, deltahat2 = sym_givens(deltabis2, g)                     # :437
            c4, s4, delta_0 = sym_givens(deltahat2, beta_next)               # :443
            if it == 1:                                                      # :449-451
                gx_m1 = v / delta_m1
                gx_0 = (-sigma_m1 / delta_0) * gx_m1
                gy_0 = u / delta_0
            elif it == 2 and fault != "swap_after_update_k2":                # :457-463
                gx_m3, gx_m1 = gx_m1, gx_m3
                gx_m2, gx_0 = gx_0, gx_m2
                gy_m2, gy_0 = gy_0, gy_m2
                old = gx_m1
                gx_m1 = g_value(v, [(eta_m3, gx_m3), (sigma_m2, gx_m2)], delta_m1)
                last = old if fault == "g_last_term_old_buffer" else gx_m1
                gx_0 = g_value(None, [(lambda_m3, gx_m3), (eta_m2, gx_m2), (sigma_m1, last)], delta_0)
                old = gy_m1
                gy_m1 = g_value(None, [(eta_m3, gy_m3), (sigma_m2, gy_m2)], delta_m1)
                last = old if fault == "g_last_term_old_buffer" else gy_m1
                gy_0 = g_value(u, [(lambda_m3, gy_m3), (eta_m2, gy_m2), (sigma_m1, last)], delta_0)
            elif it == 2:                                                    # the fault: update in the names as they are, then swap
                gx_m1 = g_value(v, [(eta_m3, gx_m3), (sigma_m2, gx_m2)], delta_m1)
                gx_0 = g_value(None, [(lambda_m3, gx_m3), (eta_m2, gx_m2), (sigma_m1, gx_m1)], delta_0)
                gy_m1 = g_value(None, [(eta_m3, gy_m3), (sigma_m2, gy_m2)], delta_m1)
                gy_0 = g_value(u, [(lambda_m3, gy_m3), (eta_m2, gy_m2), (sigma_m1, gy_m1)], delta_0)
                gx_m3, gx_m1 = gx_m1, gx_m3
                gx_m2, gx_0 = gx_0, gx_m2
                gy_m2, gy_0 = gy_0, gy_m2
            else:                                                            # :467-478
                g_m5, g_m4, g_m3, g_m2 = gx_m3, gx_m2, gx_m1, gx_0
                g_m1 = g_value(v, [(mu_m5, g_m5), (lambda_m4, g_m4), (eta_m3, g_m3), (sigma_m2, g_m2)], delta_m1)
                last = g_m5 if fault == "g_last_term_old_buffer" else g_m1
                g_0 = g_value(None, [(mu_m4, g_m4), (lambda_m3, g_m3), (eta_m2, g_m2), (sigma_m1, last)], delta_0)
                gx_m3, gx_m2 = g_m1, g_0
                gx_m3, gx_m1 = gx_m1, gx_m3
                gx_m2, gx_0 = gx_0, gx_m2
                g_m5, g_m4, g_m3, g_m2 = gy_m3, gy_m2, gy_m1, gy_0
                g_m1 = g_value(None, [(mu_m5, g_m5), (lambda_m4, g_m4), (eta_m3, g_m3), (sigma_m2, g_m2)], delta_m1)
                last = g_m5 if fault == "g_last_term_old_buffer" else g_m1
                g_0 = g_value(u, [(mu_m4, g_m4), (lambda_m3, g_m3), (eta_m2, g_m2), (sigma_m1, last)], delta_0)
                gy_m3, gy_m2 = g_m1, g_0
                gy_m3, gy_m1 = gy_m1, gy_m3
                gy_m2, gy_0 = gy_0, gy_m2
            pibis2 = c1 * pibar2                                             # :482-492
            pibis4 = s1 * pibar2
            pi1 = c2 * pibar1 + s2 * pibis2
            pihat2 = s2 * pibar1 - c2 * pibis2
            pitmp2 = (c1 if fault == "c1_for_c3" else c3) * pihat2 + s3 * pibis4
            pibar4 = s3 * pihat2 - c3 * pibis4
            pi2 = c4 * pitmp2
            pibar3 = s4 * pitmp2
            x = x + pi1 * gx_m1                                              # :495-500
            x = x + pi2 * gx_0
            y = y + pi1 * gy_m1
            y = y + pi2 * gy_0
            rNorm = F(np.sqrt(pibar3 * pibar3 + pibar4 * pibar4))            # :503-504
            if history:
                st.residuals.append(float(rNorm))
            v_prev = v                                                       # :511-516
            u_prev = u
            v = q.copy()
            u = p.copy()
            old_s1, old_s2, old_s3, old_s4 = s1, s2, s3, s4                  # :519-526
            old_c1, old_c2, old_c3, old_c4 = c1, c2, c3, c4
            beta, gamma = beta_next, gamma_next                              # :529-540
            sigmabar_m2 = sigmabar2
            etabar_m3 = etabar1
            lambdabar_m3 = lambdabar1
            if it >= 2 or fault == "mu_shift_at_k1":
                mu_m5 = mu_m3
                mu_m4 = mu_m3 if fault == "mu_m4_takes_mu_m3" else mu_m2
                lambda_m4 = lambda_m2
            pibar1, pibar2 = (pibar4, pibar3) if fault == "pibar_swapped" else (pibar3, pibar4)
            mach = bool(rNorm + 1 <= 1)                                      # :544-553
            if callback is not None:
                st.niter = it
                user_exit = bool(callback(SimpleNamespace(x=x, y=y, stats=st)))
            lim = bool(rNorm <= eps)
            breakdown = bool(beta_next <= BTOL and gamma_next <= BTOL)
            solved = lim or mach
            tired = it >= itmax
            overtimed = (time.perf_counter() - start) > timemax
    status = "unknown"                                                       # :559-563
    for cond, text in ((tired, TIRED), (breakdown, INCONSISTENT), (solved, SOLVED), (user_exit, "user-requested exit"),
                       (overtimed, "time limit exceeded")):
        if cond:
            status = text
    if dx is not None:                                                       # :566-567
        x = x + dx
        y = y + dy
    st.vectors = dict(y=y, u_prev=u_prev, u=u, p=p, gy_m3=gy_m3, gy_m2=gy_m2, gy_m1=gy_m1, gy=gy_0, x=x, v_prev=v_prev, v=v, q=q,
                      gx_m3=gx_m3, gx_m2=gx_m2, gx_m1=gx_m1, gx=gx_0)
    st.niter, st.solved, st.status = it, bool(solved), status
    st.inconsistent = bool(not solved and breakdown)
    st.breakdown = bool(breakdown)
    st.residuals = np.array(st.residuals)
    return x, y, st
