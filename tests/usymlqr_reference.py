"""Test-side NumPy restatement of usymlqr! (src/usymlqr.jl:136-509, real Float64), line by line, with an injectable `dot` for kdot
and knorm (knorm(x) = sqrt(dot(x, x))).  A checker, not product code: tests/test_usymlqr_host.py and tests/test_gpu_usymlqr.py
compare the library's three loops with it.  The exactly summed dot is that of tests/bilq_reference.py.  Every scalar is an
np.float64, so a zero divisor gives inf (or nan) as in the reference and raises nothing.

`fault` swaps ONE line for a plausible slip (tests/test_usymlqr_host.py shows that the comparison rejects each of them):
  "z_uses_new_w"               z = z - ζₖ₋₁ wₖ, the vector this iteration has just written, in place of wₖ₋₁
  "dbar_before_x"              d̅ₖ is formed before x is updated, so x reads the new d̅
  "frozen_ls_keeps_updating"   the least-squares block goes on after solved_ls (the test is `ls` alone)
  "w_swap_at_k1"               wₖ₋₂ and wₖ₋₁ already change places at k = 1
  "arnorm_uses_ck"             ‖Aᴴrₖ₋₁‖ is formed with cₖ in place of cₖ₋₁
  "ln_before_ls_in_history"    the least-norm entry of an iteration is pushed before its least-squares entry
  "r_coef_times_reciprocal"    the r coefficient is -cₖ ϕbarₖ₊₁ (1 / βₖ₊₁) in place of -cₖ ϕbarₖ₊₁ / βₖ₊₁ (one rounding more: visible
                               in r's bits only)"""
import math
import time
from types import SimpleNamespace

import numpy as np

from bilq_reference import EPS, _op, fsum_dot, sym_givens as _sym_givens  # noqa: F401  (re-exported for the tests)

TIRED = "maximum number of iterations exceeded"
SOLVED = "solution good enough given atol and rtol"
# every status string of src/usymlqr.jl:234, :486-489
STATUSES = ("unknown", TIRED, SOLVED, "user-requested exit", "time limit exceeded")
BOTH_FALSE = "The keyword arguments `ls` and `ln` can't be both `false`."          # :145
FAULTS = ("z_uses_new_w", "dbar_before_x", "frozen_ls_keeps_updating", "w_swap_at_k1", "arnorm_uses_ck", "ln_before_ls_in_history",
          "r_coef_times_reciprocal")
# the work vectors by the names of khip_usymlqr_vector, in UsymlqrWorkspace's order
VECTORS = ("r", "x", "y", "z", "v_prev", "v", "u_prev", "u", "p", "q", "dbar", "w_m2", "w_m1")
ROW_SIDE = ("r", "x", "v_prev", "v", "q", "dbar", "dx")
F = np.float64


def sym_givens(a, b):
    c, s, rho = _sym_givens(F(a), F(b))
    return F(c), F(s), F(rho)


def usymlqr(A, b, c, x0=None, y0=None, At=None, ls=True, ln=True, atol=math.sqrt(EPS), rtol=math.sqrt(EPS), itmax=0,
            timemax=math.inf, history=True, callback=None, dot=np.dot, fault=None):
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
    if not (ls or ln):                                                       # :145
        raise ValueError(BOTH_FALSE)
    st = SimpleNamespace(niter=0, solved=False, inconsistent=False, status="unknown", residuals=[], Aresiduals=[], vectors={})
    assert (x0 is None) == (y0 is None), "warm_start!(workspace, x0, y0) takes both"
    dx = None if x0 is None else np.asarray(x0, dtype=np.float64)
    dy = None if y0 is None else np.asarray(y0, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        it = 0                                                               # :169-170
        if itmax == 0:
            itmax = n + m
        v_prev = np.zeros(m)                                                 # :173-174
        u_prev = np.zeros(n)
        b0, c0 = b, c
        if dx is not None:                                                   # :178-184
            b0 = mul(dy)
            b0 = b0 + dx
            b0 = b - b0
            c0 = mult(dx)
            c0 = c - c0
        r = b0.copy() if ls else np.zeros(m)                                 # :187-190
        x = np.zeros(m)
        y = np.zeros(n)
        z = np.zeros(n)
        v = b0.copy()                                                        # :193-200
        beta = norm(v)
        v = v * (F(1.0) / beta) if beta != 0 else np.zeros(m)
        u = c0.copy()                                                        # :203-210
        gamma = norm(u)
        u = u * (F(1.0) / gamma) if gamma != 0 else np.zeros(n)
        c_km2 = c_km1 = ck = F(-1.0)                                         # :212-213
        s_km2 = s_km1 = sk = F(0.0)
        w_m2 = np.zeros(n)                                                   # :214-216
        w_m1 = np.zeros(n)
        dbar = np.zeros(m)
        phibar = beta                                                        # :217-220
        zeta_m2 = zeta_m1 = F(0.0)
        eta_prev = F(0.0)
        delta_km1 = deltabar = F(0.0)
        eps_km2 = lam_km1 = lambar = F(0.0)                                  # (undefined in the reference until they are set)
        kappa = F(0.0)                                                       # :223-237
        ArNorm = F(np.inf)
        rNorm_ls = bNorm = beta  # noqa: F841
        rNorm_ln = cNorm = gamma
        eps_ls = atol + rtol * rNorm_ls
        eps_ln = atol + rtol * rNorm_ln
        solved_ls = bool(not ls or rNorm_ls <= eps_ls)
        solved_ln = bool(not ln or rNorm_ln <= eps_ln)
        solved = solved_ls and solved_ln
        inconsistent = False
        tired = it >= itmax
        user_exit = overtimed = False
        q = np.zeros(m)
        p = np.zeros(n)
        while not (solved or tired or inconsistent or user_exit or overtimed):
            it += 1                                                          # :246
            q = mul(u)                                                       # :252-253
            p = mult(v)
            if it >= 2:                                                      # :255-258
                q = q - gamma * v_prev
                p = p - beta * u_prev
            alpha = F(dot(v, q))                                             # :260
            q = q - alpha * v                                                # :262-263
            p = p - alpha * u
            v_prev = v                                                       # :266-267
            u_prev = u
            beta_next = norm(q)                                              # :270-271
            gamma_next = norm(p)
            if it >= 3:                                                      # :290-295
                eps_km2 = s_km2 * gamma
                lambar = -c_km2 * gamma
            if it >= 2:                                                      # :298-304
                if it == 2:
                    lambar = gamma
                lam_km1 = c_km1 * lambar + s_km1 * alpha
                deltabar = s_km1 * lambar - c_km1 * alpha
            if it == 1:                                                      # :307
                deltabar = alpha
            ck, sk, delta = sym_givens(deltabar, beta_next)                  # :310
            if it == 1:                                                      # :314-317
                w_m1 = u / delta
                w = w_m1
            if it == 2:                                                      # :319-324
                w_m2 = w_m2 + (-lam_km1) * w_m1
                w_m2 = w_m2 + u
                w_m2 = w_m2 * (F(1.0) / delta)
                w = w_m2
            if it >= 3:                                                      # :326-332
                w_m2 = (-eps_km2) * w_m2
                w_m2 = w_m2 + (-lam_km1) * w_m1
                w_m2 = w_m2 + u
                w_m2 = w_m2 * (F(1.0) / delta)
                w = w_m2
            entries = []                                                     # the pushes of this iteration, in order
            if ls and (not solved_ls or fault == "frozen_ls_keeps_updating"):                    # :334-367
                phi = ck * phibar
                phibar_next = sk * phibar
                y = y + phi * w                                              # :345
                if fault == "r_coef_times_reciprocal":
                    coef = -ck * phibar_next * (F(1.0) / beta_next)
                else:
                    coef = -ck * phibar_next / beta_next
                r = coef * q + (sk * sk) * r                                 # :350
                rNorm_ls = F(abs(phibar_next))                               # :353-354
                entries.append(float(rNorm_ls))
                cc = ck if fault == "arnorm_uses_ck" else c_km1
                cg = cc * gamma_next
                ArNorm = F(abs(phibar)) * F(np.sqrt(deltabar * deltabar + cg * cg))      # :357-358
                if history:
                    st.Aresiduals.append(float(ArNorm))
                phibar = phibar_next                                         # :361
                solved_ls = bool(rNorm_ls <= eps_ls)                         # :364-366
                if it == 1:
                    kappa = atol + rtol * ArNorm
                inconsistent = bool(not solved_ls and ArNorm <= kappa)
            if ln and not solved_ln:                                         # :369-438
                if it == 1:                                                  # :382-384
                    eta = gamma
                if it == 2:                                                  # :387-390
                    zeta_m1 = eta_prev / delta_km1
                    eta = -lam_km1 * zeta_m1
                if it >= 3:                                                  # :394-398
                    zeta_m2 = zeta_m1
                    zeta_m1 = eta_prev / delta_km1
                    eta = -eps_km2 * zeta_m2 - lam_km1 * zeta_m1
                if it == 1:                                                  # :404-406
                    dbar = v.copy()
                else:                                                        # :407-420
                    if fault == "dbar_before_x":
                        dbar = (-c_km1) * v + s_km1 * dbar
                    x = x + (zeta_m1 * c_km1) * dbar
                    x = x + (zeta_m1 * s_km1) * v
                    z = z + (-zeta_m1) * (w if fault == "z_uses_new_w" else w_m1)
                    if fault != "dbar_before_x":
                        dbar = (-c_km1) * v + s_km1 * dbar
                if it == 1:                                                  # :424-431
                    rNorm_ln = cNorm
                else:
                    mu = gamma * (s_km2 * zeta_m2 - c_km2 * c_km1 * zeta_m1) + alpha * s_km1 * zeta_m1
                    omega = gamma_next * s_km1 * zeta_m1
                    rNorm_ln = F(np.sqrt(mu * mu + omega * omega))
                if fault == "ln_before_ls_in_history":
                    entries.insert(0, float(rNorm_ln))
                else:
                    entries.append(float(rNorm_ln))
                eta_prev = eta                                               # :434
                solved_ln = bool(rNorm_ln <= eps_ln)                         # :437
            if history:
                st.residuals.extend(entries)
            v = q / beta_next if beta_next != 0 else np.zeros(m)             # :441-455
            u = p / gamma_next if gamma_next != 0 else np.zeros(n)
            if it >= 2 or fault == "w_swap_at_k1":                           # :458-460
                w_m2, w_m1 = w_m1, w_m2
            if it >= 2:                                                      # :463-471
                s_km2 = s_km1
                c_km2 = c_km1
            s_km1 = sk
            c_km1 = ck
            delta_km1 = delta
            gamma = gamma_next
            beta = beta_next
            if callback is not None:                                         # :474-478
                st.niter = it
                user_exit = bool(callback(SimpleNamespace(x=x, y=y, stats=st)))
            solved = solved_ls and solved_ln
            tired = it >= itmax
            overtimed = (time.perf_counter() - start) > timemax
        status = "unknown"                                                   # :486-489
        for cond, text in ((tired, TIRED), (solved, SOLVED), (user_exit, "user-requested exit"), (overtimed, "time limit exceeded")):
            if cond:
                status = text
        x = x + r                                                            # :494-495
        y = y + z
        if dx is not None:                                                   # :498-499
            x = x + dx
            y = y + dy
    st.vectors = dict(r=r, x=x, y=y, z=z, v_prev=v_prev, v=v, u_prev=u_prev, u=u, p=p, q=q, dbar=dbar, w_m2=w_m2, w_m1=w_m1)
    st.niter, st.solved, st.status = it, bool(solved), status
    st.inconsistent = False                                                  # :505
    st.solved_ls, st.solved_ln, st.inconsistent_exit = bool(solved_ls), bool(solved_ln), bool(inconsistent)
    st.x_floor = float(np.abs(b0).max()) if m else 0.0                     # the size of what r = b₀ − A y is formed from
    st.residuals = np.array(st.residuals)
    st.Aresiduals = np.array(st.Aresiduals)
    return x, y, st
