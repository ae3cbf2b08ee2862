"""Test-side NumPy restatement of minres_qlp! (src/minres_qlp.jl:131-538, real Float64, linesearch = false), line by line, with an
injectable `dot` for kdotr / knorm.  A checker, not product code: tests/test_minres_qlp_host.py and tests/test_gpu_minres_qlp.py
compare the library's three loops with it.  The exactly summed dot is that of tests/bilq_reference.py.  `fault` injects one of
three mistakes a fused implementation can make, for the host tests that show the parity comparison rejects them."""
import math
import time
from types import SimpleNamespace

import numpy as np

from bilq_reference import EPS, _op, fsum_dot, history_deviation, sym_givens  # noqa: F401  (re-exported for the tests)

ZERO_RESIDUAL = "x is a zero-residual solution"
TIRED = "maximum number of iterations exceeded"
ILL_COND_MACH = "condition number seems too large for this machine"
INCONSISTENT = "found approximate minimum least-squares solution"
ZERO_RESID = "found approximate zero-residual solution"
SOLVED = "solution good enough given atol and rtol"
USER_EXIT = "user-requested exit"
OVERTIMED = "time limit exceeded"
FAULTS = ("alpha_is_vAv", "no_final_axpy", "stale_cp_sp")


def _div(a, b):
    """IEEE division: x / 0 is Inf or NaN, as in the reference, not an exception."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _jl_max(*v):
    return math.nan if any(math.isnan(e) for e in v) else max(v)


def _jl_min(*v):
    return math.nan if any(math.isnan(e) for e in v) else min(v)


def minres_qlp(A, b, x0=None, M=None, lam=0.0, atol=math.sqrt(EPS), rtol=math.sqrt(EPS), Artol=math.sqrt(EPS), itmax=0,
               timemax=math.inf, history=True, callback=None, dot=np.dot, fault=None):
    """A, M: callables v -> op v or objects with `@`.  Returns (x, stats); stats.vectors holds wkm1, wk, Mvkm1, Mvk, p (and vk with
    M) by the names of the reference's variables at the end of the solve."""
    assert fault is None or fault in FAULTS
    start = time.perf_counter()
    mul, Mop = _op(A), _op(M)
    MisI = Mop is None                                                       # :145
    b = np.asarray(b, dtype=np.float64)
    n = b.shape[0]
    st = SimpleNamespace(niter=0, solved=False, inconsistent=False, status="unknown", residuals=[], Aresiduals=[], Acond=[],
                         vectors={})

    def done(x):
        for k in ("residuals", "Aresiduals", "Acond"):
            setattr(st, k, np.array(getattr(st, k), dtype=np.float64))
        return x, st

    def norm_elliptic(x, y):                                                 # knorm_elliptic: knorm when x === y
        return math.sqrt(float(dot(x, y)))

    x = np.zeros(n)                                                          # :166
    dx = None if x0 is None else np.asarray(x0, dtype=np.float64)
    if dx is not None:                                                       # :168-172
        Mvk = mul(dx)
        if lam != 0:
            Mvk = Mvk + lam * dx
        Mvk = 1.0 * b + (-1.0) * Mvk
    else:
        Mvk = b.copy()                                                       # :173
    vk = Mvk if MisI else Mop(Mvk)                                           # :177
    beta = norm_elliptic(vk, Mvk)                                            # :178
    if beta != 0:                                                            # :180-183
        Mvk = (1.0 / beta) * Mvk
        vk = Mvk if MisI else (1.0 / beta) * vk
    rNorm = beta                                                             # :185-192
    ANorm2 = ANorm = mumin = mumax = Acond = 0.0
    if history:
        st.residuals.append(rNorm)
        st.Acond.append(Acond)
    if rNorm == 0:                                                           # :193-201
        st.niter, st.solved, st.inconsistent, st.status = 0, True, False, ZERO_RESIDUAL
        return done(x if dx is None else x + dx)
    it = 0                                                                   # :203-207
    if itmax == 0:
        itmax = 2 * n
    eps_tol = atol + rtol * rNorm
    kappa = 0.0
    Mvkm1 = np.zeros(n)                                                      # :212-221
    zbar = beta
    xi1 = 0.0
    tau2 = tau1 = tau = 0.0
    psibar2 = 0.0
    mubis2 = mubar1 = 0.0
    wkm1, wk = np.zeros(n), np.zeros(n)
    c2 = c1 = c = 1.0
    s2 = s1 = s = 0.0
    p = np.zeros(n)
    btol = EPS ** 0.75                                                       # :224
    breakdown = False                                                        # :227-236
    solved = zero_resid = rNorm <= eps_tol
    inconsistent = ill_cond_mach = False
    tired = it >= itmax
    user_exit = overtimed = False
    cp = sp = 0.0
    cp_before = sp_before = 0.0                                              # (for fault = "stale_cp_sp" only)

    with np.errstate(all="ignore"):
        while not (solved or tired or inconsistent or ill_cond_mach or breakdown or user_exit or overtimed):
            it += 1                                                          # :240
            p = mul(vk)                                                      # :246
            if fault == "alpha_is_vAv":                                      # the dot of a fused product: before λ vₖ and βₖ vₖ₋₁
                alpha_fault = float(dot(vk, p))
            if lam != 0:                                                     # :247-249
                p = p + lam * vk
            if it >= 2:                                                      # :251-253
                p = p + (-beta) * Mvkm1
            alpha = float(dot(vk, p))                                        # :255
            if fault == "alpha_is_vAv":
                alpha = alpha_fault
            p = p + (-alpha) * Mvk                                           # :257
            vnext = p if MisI else Mop(p)                                    # :259
            beta_next = norm_elliptic(vnext, p)                              # :261
            if beta_next > btol:                                             # :264-267
                vnext = (1.0 / beta_next) * vnext
                p = vnext if MisI else (1.0 / beta_next) * p
            ANorm2 = ANorm2 + alpha * alpha + beta * beta + beta_next * beta_next   # :269
            if it >= 3:                                                      # :288-293
                eps2 = s2 * beta
                gbar1 = -c2 * beta
            if it >= 2:                                                      # :295-301
                if it == 2:
                    gbar1 = beta
                gamma1 = c1 * gbar1 + s1 * alpha
                lambar = s1 * gbar1 - c1 * alpha
            if it == 1:                                                      # :302
                lambar = alpha
            c, s, lam_k = sym_givens(lambar, beta_next)                      # :333
            zeta = c * zbar                                                  # :340-341
            zbar_next = s * zbar
            cp_before, sp_before = cp, sp
            if it == 1:                                                      # :358-382
                mubar = lam_k
            elif it == 2:
                cp, sp, mubis1 = sym_givens(mubar1, gamma1)
                psibar1 = sp * lam_k
                mubar = -cp * lam_k
            else:
                cp, sp, mu2 = sym_givens(mubis2, eps2)
                psi2 = cp * psibar2 + sp * gamma1
                theta = sp * psibar2 - cp * gamma1
                rho2 = sp * lam_k
                eta = -cp * lam_k
                cd, sd, mubis1 = sym_givens(mubar1, theta)
                psibar1 = sd * eta
                mubar = -cd * eta
            if it == 1:                                                      # :392-405
                tau = _div(zeta, mubar)
            elif it == 2:
                tau1 = tau
                tau1 = _div(tau1 * mubar1, mubis1)
                xi = zeta
                tau = _div(xi - psibar1 * tau1, mubar)
            else:
                tau2 = tau1
                tau2 = _div(tau2 * mubis2, mu2)
                tau1 = _div(xi1 - psi2 * tau2, mubis1)
                xi = zeta - rho2 * tau2
                tau = _div(xi - psibar1 * tau1, mubar)
            if it == 1:                                                      # :408-435
                wk = vk.copy()
            elif it == 2:
                wkm1, wk = wk, wkm1
                wk = wkm1.copy()
                wk = (-cp) * vk + sp * wk
                wkm1 = sp * vk + cp * wkm1
            else:
                ucp, usp = (cp_before, sp_before) if fault == "stale_cp_sp" else (cp, sp)
                x = x + (ucp * tau2) * wkm1                                  # :427-428
                x = x + (usp * tau2) * vk
                wkm1 = (-ucp) * vk + usp * wkm1                              # :430
                wk, wkm1 = cd * wk + sd * wkm1, sd * wk - cd * wkm1          # kref!(w̄ₖ₋₁, wₐᵤₓ, cd, sd), :433
                wkm1, wk = wk, wkm1                                          # :434
            if not MisI:                                                     # :438-440
                vk = vnext
            Mvkm1 = Mvk
            Mvk = p
            if MisI:
                vk = Mvk
            rNorm = abs(zbar_next)                                           # :444-451
            if history:
                st.residuals.append(rNorm)
            ArNorm = abs(zbar) * math.sqrt(lambar * lambar + (c1 * beta_next) * (c1 * beta_next))
            if it == 1:
                kappa = atol + Artol * ArNorm
            if history:
                st.Aresiduals.append(ArNorm)
            ANorm = math.sqrt(ANorm2)                                        # :453-469
            abs_mubar = abs(mubar)
            if it == 1:
                mumin = mumax = abs_mubar
            elif it == 2:
                mumax = _jl_max(mumax, mubis1, abs_mubar)
                mumin = _jl_min(mumin, mubis1, abs_mubar)
            else:
                mumax = _jl_max(mumax, mu2, mubis1, abs_mubar)
                mumin = _jl_min(mumin, mu2, mubis1, abs_mubar)
            Acond = _div(mumax, mumin)
            if history:
                st.Acond.append(Acond)
            xNorm = math.sqrt(float(dot(x, x)))
            backward = _div(rNorm, ANorm * xNorm)
            ill_cond_mach = 1.0 + _div(1.0, Acond) <= 1.0                    # :474-482
            resid_decrease_mach = 1.0 + rNorm <= 1.0
            zero_resid_mach = 1.0 + backward <= 1.0
            tired = it >= itmax
            resid_decrease_lim = rNorm <= eps_tol
            zero_resid_lim = MisI and backward <= EPS
            breakdown = beta_next <= btol
            if callback is not None:                                         # :484
                st.niter = it
                st.vectors = dict(wkm1=wkm1, wk=wk, Mvkm1=Mvkm1, Mvk=Mvk, p=p)
                user_exit = bool(callback(SimpleNamespace(x=x, stats=st)))
            zero_resid = zero_resid_mach or zero_resid_lim                   # :485-490
            resid_decrease = resid_decrease_mach or resid_decrease_lim
            solved = resid_decrease or zero_resid
            inconsistent = (ArNorm <= kappa and abs(mubar) <= Artol) or (breakdown and not solved)
            overtimed = (time.perf_counter() - start) > timemax
            if it >= 2:                                                      # :493-504
                s2, c2, xi1, mubis2, psibar2 = s1, c1, xi, mubis1, psibar1
            s1, c1, mubar1, zbar, beta = s, c, mubar, zbar_next, beta_next

        st.xloop = x.copy()                                                  # (x before the two final updates, for the tests)
        if it >= 2 and fault != "no_final_axpy":                             # :510-515
            x = x + tau1 * wkm1
        if not inconsistent:
            x = x + tau * wk
    status = "unknown"                                                       # :518-524
    if tired:
        status = TIRED
    if ill_cond_mach:
        status = ILL_COND_MACH
    if inconsistent:
        status = INCONSISTENT
    if zero_resid:
        status = ZERO_RESID
    if solved:
        status = SOLVED
    if user_exit:
        status = USER_EXIT
    if overtimed:
        status = OVERTIMED
    st.vectors = dict(wkm1=wkm1, wk=wk, Mvkm1=Mvkm1, Mvk=Mvk, p=p)
    if not MisI:
        st.vectors["vk"] = vk
    if dx is not None:                                                       # :527
        x = x + dx
    st.niter, st.solved, st.inconsistent, st.status = it, bool(solved), bool(inconsistent), status
    st.beta, st.breakdown = beta, bool(breakdown)
    return done(x)
