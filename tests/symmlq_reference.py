"""Test-side NumPy restatement of symmlq! (src/symmlq.jl:132-464, real Float64), line by line, with an injectable `dot` for kdotr.
A checker, not product code: tests/test_symmlq_host.py and tests/test_gpu_symmlq.py compare the library's three loops with it.  The
exactly summed dot is that of tests/bilq_reference.py.  The reference's `missing` is NaN in every history."""
import math
import time
from types import SimpleNamespace

import numpy as np

from bilq_reference import EPS, _op, fsum_dot, history_deviation, sym_givens  # noqa: F401  (re-exported for the tests)

ZERO_RESIDUAL = "x is a zero-residual solution"
TIRED = "maximum number of iterations exceeded"
ILL_COND_MACH = "condition number seems too large for this machine"
ILL_COND_LIM = "condition number exceeds tolerance"
SOLVED = "found approximate solution"
SOLVED_LQ = "solution xᴸ good enough given atol and rtol"
SOLVED_CG = "solution xᶜ good enough given atol and rtol"
USER_EXIT = "user-requested exit"
OVERTIMED = "time limit exceeded"
NOT_PD = "Preconditioner is not positive definite"
MISSING = math.nan


def _div(a, b):
    """IEEE division: x / 0 is Inf or NaN, as in the reference, not an exception."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def symmlq(A, b, x0=None, M=None, window=5, transfer_to_cg=True, lam=0.0, lam_est=0.0, atol=math.sqrt(EPS), rtol=math.sqrt(EPS),
           etol=math.sqrt(EPS), conlim=1.0 / math.sqrt(EPS), itmax=0, timemax=math.inf, history=True, callback=None, dot=np.dot):
    """A, M: callables v -> op v or objects with `@`.  Returns (x, stats); stats.vectors holds Mvold, Mv, Mv_next, wbar (and v with
    M) by the names of the reference's variables at the end of the loop."""
    start = time.perf_counter()
    mul, Mop = _op(A), _op(M)
    MisI = Mop is None                                                       # :145
    b = np.asarray(b, dtype=np.float64)
    n = b.shape[0]
    st = SimpleNamespace(niter=0, solved=False, status="unknown", residuals=[], residualscg=[], errors=[], errorscg=[],
                         Anorm=math.nan, Acond=math.nan, vectors={})

    def done(x):
        for k in ("residuals", "residualscg", "errors", "errorscg"):
            setattr(st, k, np.array(getattr(st, k), dtype=np.float64))
        return x, st

    ctol = 1.0 / conlim if conlim > 0 else 0.0                               # :163
    x = np.zeros(n)                                                          # :166
    dx = None if x0 is None else np.asarray(x0, dtype=np.float64)
    if dx is not None:                                                       # :168-172
        Mvold = mul(dx)
        if lam != 0:
            Mvold = Mvold + lam * dx
        Mvold = 1.0 * b + (-1.0) * Mvold
    else:
        Mvold = b.copy()                                                     # :173
    vold = Mvold if MisI else Mop(Mvold)                                     # :178
    beta1 = float(dot(vold, Mvold))                                          # :179
    if beta1 == 0:                                                           # :180-192
        st.niter, st.solved, st.status = 0, True, ZERO_RESIDUAL
        if history:
            st.residuals.append(0.0)
            st.residualscg.append(0.0)
        return done(x if dx is None else x + dx)
    beta1 = math.sqrt(beta1)                                                 # :193
    beta = beta1
    with np.errstate(all="ignore"):                   # the Lanczos breakdown divides by β = 0 on purpose, as the reference does
        vold = (1.0 / beta) * vold                                           # :195
        if MisI:
            Mvold = vold
        else:
            Mvold = (1.0 / beta) * Mvold                                     # :196
        wbar = vold.copy()                                                   # :198
        Mv = mul(vold)                                                       # :200
        alpha = float(dot(vold, Mv)) + lam                                   # :201
        Mv = Mv + (-alpha) * Mvold                                           # :202
        v = Mv if MisI else Mop(Mv)                                          # :203
        beta = float(dot(v, Mv))                                             # :204
        if beta < 0:                                                         # :205
            raise ValueError(NOT_PD)
        beta = math.sqrt(beta)                                               # :206
        v = _div(1.0, beta) * v                                              # :207
        if MisI:
            Mv = v
        else:
            Mv = _div(1.0, beta) * Mv                                        # :208
        Mv_next = np.zeros(n)

        gbar, dbar = alpha, beta                                             # :211-219
        eps_old, c_old, s_old = 0.0, 1.0, 0.0  # noqa: F841
        eta_old, eta, zeta_old = 0.0, beta1, 0.0  # noqa: F841
        ANorm2 = alpha * alpha + beta * beta                                 # :221
        gmax, gmin = -math.inf, math.inf                                     # :223-226
        ANorm = Acond = 0.0
        xNorm = 0.0                                                          # :228
        rNorm = beta1
        if history:
            st.residuals.append(rNorm)
        zbar = rcgNorm = math.nan
        if gbar != 0:                                                        # :232-239
            zbar = _div(eta, gbar)
            xcgNorm = abs(zbar)  # noqa: F841
            rcgNorm = beta1 * abs(zbar)
            if history:
                st.residualscg.append(rcgNorm)
        elif history:
            st.residualscg.append(MISSING)
        err = errcg = math.inf                                               # :241-242
        clist, zlist, sprod = np.zeros(window), np.zeros(window), np.ones(window)   # :244-247
        if lam_est != 0:                                                     # :249-264
            rhobar = alpha - lam_est
            sigbar = beta
            rho = math.sqrt(rhobar * rhobar + beta * beta)
            cwold = -1.0
            cw = _div(rhobar, rho)
            sw = _div(beta, rho)
            if history:
                st.errors.append(abs(_div(beta1, lam_est)))
                if gbar != 0:
                    st.errorscg.append(math.sqrt(st.errors[0] * st.errors[0] - zbar * zbar))
                else:
                    st.errorscg.append(MISSING)
        it = 0                                                               # :266-267
        if itmax == 0:
            itmax = 2 * n
        tol = atol + rtol * beta1                                            # :272
        solved_lq = solved_mach = rNorm <= tol                               # :274-281
        solved_cg = (gbar != 0) and transfer_to_cg and rcgNorm <= tol
        tired = it >= itmax
        ill_cond = ill_cond_mach = ill_cond_lim = False
        solved = solved_lq or solved_cg
        user_exit = overtimed = False

        while not (solved or tired or ill_cond or user_exit or overtimed):
            it += 1                                                          # :284
            c, s, gamma = sym_givens(gbar, beta)                             # :287
            eta_old = eta                                                    # :290-291
            zeta = _div(eta_old, gamma)
            x = x + (c * zeta) * wbar                                        # :292
            x = x + (s * zeta) * v                                           # :293
            wbar = (-c) * v + s * wbar                                       # :295
            oldbeta = beta                                                   # :298
            Mv_next = mul(v)                                                 # :299
            alpha = float(dot(v, Mv_next)) + lam                             # :300
            Mv_next = Mv_next + (-oldbeta) * Mvold                           # :301
            Mvold = Mv                                                       # :302
            Mv_next = Mv_next + (-alpha) * Mv                                # :303
            Mv = Mv_next                                                     # :304
            v = Mv if MisI else Mop(Mv)                                      # :305
            beta = float(dot(v, Mv))                                         # :306
            if beta < 0:                                                     # :307
                raise ValueError(NOT_PD)
            beta = math.sqrt(beta)                                           # :308
            v = _div(1.0, beta) * v                                          # :309
            if MisI:
                Mv = v
            else:
                Mv = _div(1.0, beta) * Mv                                    # :310
            ANorm2 = ANorm2 + alpha * alpha + oldbeta * oldbeta + beta * beta   # :313
            if lam_est != 0:                                                 # :315-320
                eta = _div(-oldbeta * oldbeta * cwold, rhobar)
                omega = lam_est + eta
                psi = c * dbar + s * omega
                omegabar = s * dbar - c * omega
            delta = dbar * c + alpha * s                                     # :323-327
            gbar = dbar * s - alpha * c
            eps = beta * s
            dbar = -beta * c
            eta = -eps_old * zeta_old - delta * zeta
            rNorm = math.sqrt(gamma * gamma * zeta * zeta + eps_old * eps_old * zeta_old * zeta_old)   # :329
            xNorm = xNorm + zeta * zeta                                      # :330
            if history:
                st.residuals.append(rNorm)
            if gbar != 0:                                                    # :333-340
                zbar = _div(eta, gbar)
                rcgNorm = beta * abs(s * zeta - c * zbar)
                xcgNorm = xNorm + zbar * zbar  # noqa: F841
                if history:
                    st.residualscg.append(rcgNorm)
            elif history:
                st.residualscg.append(MISSING)
            if window > 0 and lam_est != 0:                                  # :342-374 (indices are the reference's, 1-based)
                if it < window and window > 1:
                    for i in range(it + 1, window + 1):
                        sprod[i - 1] = s * sprod[i - 1]
                ix = ((it - 1) % window) + 1
                clist[ix - 1] = c
                zlist[ix - 1] = zeta
                if it >= window:
                    jx = (it % window) + 1
                    zetabark = _div(zlist[jx - 1], clist[jx - 1])
                    if gbar != 0:
                        theta = 0.0
                        for i in range(1, window + 1):
                            theta += clist[i - 1] * sprod[i - 1] * zlist[i - 1]
                        theta = zetabark * abs(theta) + abs(zetabark * zbar * sprod[ix - 1] * s) - zetabark * zetabark
                        if history:
                            st.errorscg[it - window] = math.sqrt(abs(st.errorscg[it - window] * st.errorscg[it - window] - 2 * theta))
                    elif history:
                        st.errorscg[it - window] = MISSING
                ix = (it % window) + 1
                if it >= window and window > 1:
                    sprod *= _div(1.0, sprod[ix % window])
                    sprod[ix - 1] = sprod[(ix - 2) % window] * s
            if lam_est != 0:                                                 # :376-395
                err = abs(_div(eps_old * zeta_old + psi * zeta, omegabar))
                if history:
                    st.errors.append(err)
                if gbar != 0:
                    errcg = math.sqrt(abs(err * err - zbar * zbar))
                    if history:
                        st.errorscg.append(errcg)
                elif history:
                    st.errorscg.append(MISSING)
                rhobar = sw * sigbar - cw * (alpha - lam_est)
                sigbar = -cw * beta
                rho = math.sqrt(rhobar * rhobar + beta * beta)
                cwold = cw
                cw = _div(rhobar, rho)
                sw = _div(beta, rho)
            gmax = gamma if gamma > gmax or math.isnan(gamma) else gmax       # :398-399 (Julia's max / min: NaN wins)
            gmin = gamma if gamma < gmin or math.isnan(gamma) else gmin
            Acond = _div(gmax, gmin)                                         # :401-403
            ANorm = math.sqrt(ANorm2)
            test1 = _div(rNorm, ANorm * xNorm)
            eps_old, zeta_old, c_old = eps, zeta, c                          # :408-410
            resid_decrease_mach = 1.0 + rNorm <= 1.0                         # :414-416
            ill_cond_mach = 1.0 + _div(1.0, Acond) <= 1.0
            zero_resid_mach = 1.0 + test1 <= 1.0
            tired = it >= itmax                                              # :420-425
            ill_cond_lim = _div(1.0, Acond) <= ctol
            zero_resid_lim = test1 <= tol
            fwd_err = (err <= etol) or ((gbar != 0) and (errcg <= etol))
            solved_lq = rNorm <= tol
            solved_cg = transfer_to_cg and (gbar != 0) and rcgNorm <= tol
            if callback is not None:                                         # :427
                st.niter = it
                user_exit = bool(callback(SimpleNamespace(x=x, stats=st)))
            zero_resid = solved_lq or solved_cg                              # :428-432
            ill_cond = ill_cond_mach or ill_cond_lim
            solved = solved_mach or zero_resid or zero_resid_mach or zero_resid_lim or fwd_err or resid_decrease_mach
            overtimed = (time.perf_counter() - start) > timemax

        st.xlq = x.copy()                                                    # (xᴸ before the transfer, for the tests)
        if solved_cg:                                                        # :438-440
            x = x + zbar * wbar
    status = "unknown"                                                       # :443-450
    if tired:
        status = TIRED
    if ill_cond_mach:
        status = ILL_COND_MACH
    if ill_cond_lim:
        status = ILL_COND_LIM
    if solved:
        status = SOLVED
    if solved_lq:
        status = SOLVED_LQ
    if solved_cg:
        status = SOLVED_CG
    if user_exit:
        status = USER_EXIT
    if overtimed:
        status = OVERTIMED
    st.vectors = dict(Mvold=Mvold, Mv=Mv, Mv_next=Mv_next, wbar=wbar)
    if not MisI:
        st.vectors["v"] = v
    if dx is not None:                                                       # :453
        x = x + dx
    st.niter, st.solved, st.status, st.Anorm, st.Acond = it, bool(solved), status, ANorm, Acond
    st.solved_cg, st.solved_lq = bool(solved_cg), bool(solved_lq)
    st.beta = beta                                                           # the last β: Mv = Mv_next / β
    return done(x)
