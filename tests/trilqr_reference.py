"""Test-side NumPy restatement of trilqr! (src/trilqr.jl:115-460, real Float64), line by line, with an injectable `dot` for kdot and
knorm (knorm(x) = sqrt(dot(x, x))).  A checker, not product code: tests/test_trilqr_host.py and tests/test_gpu_trilqr.py compare
the library's three loops with it.  sym_givens and the exactly summed dot are those of tests/bilq_reference.py, `_div` (Julia's
division by zero) that of tests/bilqr_reference.py.  The primal block uses the very expressions of tests/usymlq_reference.py, so
that the two agree entry for entry while the primal side is unsolved.

`fault` swaps ONE line for a plausible slip (tests/test_trilqr_host.py shows which of them the comparison rejects):
  "lambda_sign"         wₖ₋₁ takes +λₖ₋₂ wₖ₋₂
  "stage3_as_4"         kscal!(-ϵₖ₋₃, wₖ₋₃) already at k = 3 (silent: ϵₖ₋₃ = 0 and wₖ₋₃ = 0 there)
  "stage4_as_3"         no kscal!(-ϵₖ₋₃, wₖ₋₃) from k = 4 on
  "no_rotation"         @kswap!(wₖ₋₃, wₖ₋₂) skipped
  "psi_after_shift"     t takes cₖ ψbarₖ (ψbarₖ₋₁ after its shift) in place of ψₖ₋₁ = cₖ ψbarₖ₋₁
  "dual_not_frozen"     the dual block goes on after solved_dual
  "primal_not_frozen"   the primal block goes on after solved_primal
  "v_prev_after_store"  wₖ₋₁ is built from the buffer of vₖ₋₁ AFTER vₖ₊₁ was stored there"""
import math
import time
from types import SimpleNamespace

import numpy as np

from bilq_reference import EPS, _op, fsum_dot, history_deviation, sym_givens  # noqa: F401  (re-exported for the tests)
from bilqr_reference import _div

TIRED = "maximum number of iterations exceeded"
ONLY_L = "Only the primal solution xᴸ is good enough given atol and rtol"
ONLY_C = "Only the primal solution xᶜ is good enough given atol and rtol"
ONLY_T = "Only the dual solution t is good enough given atol and rtol"
BOTH_L = "Both primal and dual solutions (xᴸ, t) are good enough given atol and rtol"
BOTH_C = "Both primal and dual solutions (xᶜ, t) are good enough given atol and rtol"

# every status string of src/trilqr.jl:198, :430-446
STATUSES = (
    "unknown", TIRED, ONLY_L, ONLY_C, ONLY_T, BOTH_L, BOTH_C,
    "Only found approximate zero-residual primal solution xᴸ",
    "Only found approximate zero-residual primal solution xᶜ",
    "Only found approximate zero-residual dual solution t",
    "Found approximate zero-residual primal and dual solutions (xᴸ, t)",
    "Found approximate zero-residual primal and dual solutions (xᶜ, t)",
    "Found approximate zero-residual primal solutions xᴸ and a dual solution t good enough given atol and rtol",
    "Found approximate zero-residual primal solutions xᶜ and a dual solution t good enough given atol and rtol",
    "Found a primal solution xᴸ good enough given atol and rtol and an approximate zero-residual dual solutions t",
    "Found a primal solution xᶜ good enough given atol and rtol and an approximate zero-residual dual solutions t",
    "user-requested exit", "time limit exceeded",
)
FAULTS = ("lambda_sign", "stage3_as_4", "stage4_as_3", "no_rotation", "psi_after_shift", "dual_not_frozen", "primal_not_frozen",
          "v_prev_after_store")
# the work vectors by the names of khip_trilqr_vector, in TrilqrWorkspace's order
VECTORS = ("u_prev", "u", "p", "dbar", "x", "v_prev", "v", "q", "y", "w_prev3", "w_prev2")


def trilqr(A, b, c, x0=None, y0=None, At=None, transfer_to_usymcg=True, atol=math.sqrt(EPS), rtol=math.sqrt(EPS), itmax=0,
           timemax=math.inf, history=True, callback=None, dot=np.dot, fault=None):
    """A, At: callables v -> op v or objects with `@` (At defaults to A.T); A has m rows and n columns, b has m entries, c has n.
    Returns (x, t, stats); stats.vectors holds the work vectors by the names of the reference's variables at the end of the solve
    (x and y as returned; x_lq = the LQ point before the transfer)."""
    assert fault is None or fault in FAULTS
    start = time.perf_counter()
    mul = _op(A)
    mult = _op(At) if At is not None else (lambda v: A.T @ v)
    norm = lambda v: math.sqrt(float(dot(v, v)))  # noqa: E731
    b = np.asarray(b, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    m, n = b.shape[0], c.shape[0]
    st = SimpleNamespace(niter=0, solved_primal=False, solved_dual=False, inconsistent=False, status="unknown", residuals_primal=[],
                         residuals_dual=[], vectors={})
    assert (x0 is None) == (y0 is None), "warm_start!(workspace, x0, y0) takes both"
    dx = None if x0 is None else np.asarray(x0, dtype=np.float64)
    dy = None if y0 is None else np.asarray(y0, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        r0 = b if dx is None else b - mul(dx)                                # :142-150
        s0 = c if dy is None else c - mult(dy)
        x = np.zeros(n)                                                      # :153-158
        bNorm = norm(r0)
        t = np.zeros(m)
        cNorm = norm(s0)
        it = 0                                                               # :160-161
        if itmax == 0:
            itmax = m + n
        if history:                                                          # :163-164
            st.residuals_primal.append(bNorm)
            st.residuals_dual.append(cNorm)
        epsL = atol + rtol * bNorm                                           # :165-167
        epsQ = atol + rtol * cNorm
        xi = 0.0
        beta = norm(r0)                                                      # :172-177
        gamma = norm(s0)
        v_prev = np.zeros(m)
        u_prev = np.zeros(n)
        v = r0 / beta
        u = s0 / gamma
        c_km1 = ck = -1.0                                                    # :178-179
        s_km1 = sk = 0.0
        dbar_vec = np.zeros(n)                                               # :180
        zeta_km1 = zbar = 0.0                                                # :181-185
        zeta_km2 = eta = 0.0
        dbar_km1 = dbar = 0.0
        psibar_km1 = psi = 0.0
        eps_km3 = lam_km2 = 0.0
        w_km3 = np.zeros(m)                                                  # :186-187
        w_km2 = np.zeros(m)
        delta_km1 = lam_km1 = eps_km2 = 0.0
        rNorm_lq = rNorm_cg = sNorm = math.nan
        q = np.zeros(m)
        p = np.zeros(n)
        inconsistent = False                                                 # :190-200
        solved_lq = bNorm == 0
        solved_lq_tol = solved_lq_mach = False
        solved_cg = solved_cg_tol = solved_cg_mach = False
        solved_primal = solved_lq or solved_cg
        solved_qr_tol = solved_qr_mach = False
        solved_dual = cNorm == 0
        tired = it >= itmax
        user_exit = overtimed = False
        while not ((solved_primal and solved_dual) or tired or user_exit or overtimed):
            it += 1                                                          # :204
            q = mul(u)                                                       # :210-211
            p = mult(v)
            if it >= 2:                                                      # :213-216
                q = q - gamma * v_prev
                p = p - beta * u_prev
            alpha = float(dot(v, q))                                         # :218
            q = q - alpha * v                                                # :220-221
            p = p - alpha * u
            beta_next = norm(q)                                              # :223-224
            gamma_next = norm(p)
            if it == 1:                                                      # :235-255
                dbar = alpha
            elif it == 2:
                ck, sk, delta_km1 = sym_givens(dbar_km1, gamma)
                lam_km1 = ck * beta + sk * alpha
                dbar = sk * beta - ck * alpha
            else:
                ck, sk, delta_km1 = sym_givens(dbar_km1, gamma)
                eps_km2 = s_km1 * beta
                lam_km1 = -c_km1 * ck * beta + sk * alpha
                dbar = -c_km1 * sk * beta - ck * alpha
            v_next = q / beta_next if beta_next != 0 else v                  # what :392-394 will store over vₖ₋₁'s buffer
            if not solved_primal or (fault == "primal_not_frozen" and it >= 2):   # :257-324
                if it == 1:
                    eta = beta
                if it == 2:
                    eta_km1 = eta
                    zeta_km1 = _div(eta_km1, delta_km1)
                    eta = -lam_km1 * zeta_km1
                if it >= 3:
                    zeta_km2 = zeta_km1
                    eta_km1 = eta
                    zeta_km1 = _div(eta_km1, delta_km1)
                    eta = -eps_km2 * zeta_km2 - lam_km1 * zeta_km1
                if it == 1:                                                  # :283-295
                    dbar_vec = u.copy()
                else:
                    x = x + (zeta_km1 * ck) * dbar_vec
                    x = x + (zeta_km1 * sk) * u
                    dbar_vec = (-ck) * u + sk * dbar_vec
                if it == 1:                                                  # :299-306
                    rNorm_lq = bNorm
                else:
                    mu = beta * (s_km1 * zeta_km2 - c_km1 * ck * zeta_km1) + alpha * sk * zeta_km1
                    omega = beta_next * sk * zeta_km1
                    rNorm_lq = math.sqrt(mu * mu + omega * omega) if not math.isnan(mu * mu + omega * omega) else math.nan
                if history:
                    st.residuals_primal.append(rNorm_lq)
                cg_point = bool(transfer_to_usymcg and abs(dbar) > EPS)      # :310-314
                if cg_point:
                    zbar = float(np.float64(eta) / np.float64(dbar))
                    rho = beta_next * (sk * zeta_km1 - ck * zbar)
                    rNorm_cg = abs(rho)
                solved_lq_tol = rNorm_lq <= epsL                             # :317-323
                solved_lq_mach = rNorm_lq + 1 <= 1
                solved_lq = solved_lq_tol or solved_lq_mach
                solved_cg_tol = bool(cg_point and rNorm_cg <= epsL)
                solved_cg_mach = bool(cg_point and rNorm_cg + 1 <= 1)
                solved_cg = solved_cg_tol or solved_cg_mach
                solved_primal = solved_lq or solved_cg
            if not solved_dual or (fault == "dual_not_frozen" and it >= 2):  # :326-386
                if it == 1:
                    psibar = gamma
                else:
                    psi = ck * psibar_km1
                    psibar = sk * psibar_km1
                vp = v_next if fault == "v_prev_after_store" else v_prev
                if it == 2:                                                  # :339-342
                    w_km2 = vp / delta_km1
                    w_km1 = w_km2
                if it >= 3:                                                  # :344-357
                    scal = it >= 4 if fault != "stage3_as_4" else True
                    if fault == "stage4_as_3":
                        scal = False
                    w_km1 = (-eps_km3) * w_km3 if scal else w_km3
                    w_km1 = w_km1 + 1.0 * vp
                    w_km1 = w_km1 + (lam_km2 if fault == "lambda_sign" else -lam_km2) * w_km2
                    w_km1 = w_km1 * (1.0 / delta_km1)                        # kdiv! = kscal!(one(T) / δ), src/krylov_utils.jl
                    w_km3 = w_km1
                    if fault != "no_rotation":
                        w_km3, w_km2 = w_km2, w_km3                          # :359-362
                if it >= 2:                                                  # :364-368
                    t = t + (ck * psibar if fault == "psi_after_shift" else psi) * w_km1
                psibar_km1 = psibar                                          # :371
                sNorm = abs(psibar)                                          # :374-375
                if history:
                    st.residuals_dual.append(sNorm)
                AsNorm = abs(psibar) * math.sqrt(dbar * dbar + (ck * beta_next) ** 2)   # :378
                if it == 1:                                                  # :381-385
                    xi = atol + rtol * AsNorm
                solved_qr_tol = sNorm <= epsQ
                solved_qr_mach = sNorm + 1 <= 1
                inconsistent = AsNorm <= xi
                solved_dual = solved_qr_tol or solved_qr_mach or inconsistent
            v_prev = v                                                       # :389-397
            u_prev = u
            if beta_next != 0:
                v = q / beta_next
            if gamma_next != 0:
                u = p / gamma_next
            if it >= 3:                                                      # :400-410
                eps_km3 = eps_km2
            if it >= 2:
                lam_km2 = lam_km1
            dbar_km1, c_km1, s_km1 = dbar, ck, sk
            gamma, beta = gamma_next, beta_next
            if callback is not None:                                         # :412
                st.niter = it
                user_exit = bool(callback(SimpleNamespace(x=x, y=t, stats=st)))
            tired = it >= itmax                                              # :413-415
            overtimed = (time.perf_counter() - start) > timemax
        x_lq = x
        if solved_cg:                                                        # :425-427
            x = x + zbar * dbar_vec
    status = "unknown"                                                       # :430-446
    for cond, text in ((tired, TIRED),
                       (solved_lq_tol and not solved_dual, STATUSES[2]), (solved_cg_tol and not solved_dual, STATUSES[3]),
                       (not solved_primal and solved_qr_tol, STATUSES[4]), (solved_lq_tol and solved_qr_tol, STATUSES[5]),
                       (solved_cg_tol and solved_qr_tol, STATUSES[6]), (solved_lq_mach and not solved_dual, STATUSES[7]),
                       (solved_cg_mach and not solved_dual, STATUSES[8]), (not solved_primal and solved_qr_mach, STATUSES[9]),
                       (solved_lq_mach and solved_qr_mach, STATUSES[10]), (solved_cg_mach and solved_qr_mach, STATUSES[11]),
                       (solved_lq_mach and solved_qr_tol, STATUSES[12]), (solved_cg_mach and solved_qr_tol, STATUSES[13]),
                       (solved_lq_tol and solved_qr_mach, STATUSES[14]), (solved_cg_tol and solved_qr_mach, STATUSES[15]),
                       (user_exit, "user-requested exit"), (overtimed, "time limit exceeded")):
        if cond:
            status = text
    if dx is not None:                                                       # :449-450
        x = x + dx
        t = t + dy
    st.vectors = dict(u_prev=u_prev, u=u, p=p, dbar=dbar_vec, x=x, v_prev=v_prev, v=v, q=q, y=t, w_prev3=w_km3, w_prev2=w_km2, x_lq=x_lq)
    st.niter, st.solved_primal, st.solved_dual, st.status = it, bool(solved_primal), bool(solved_dual), status
    st.inconsistent = bool(inconsistent)
    st.solved_lq, st.solved_cg = bool(solved_lq), bool(solved_cg)
    st.solved = st.solved_primal and st.solved_dual
    st.residuals_primal = np.array(st.residuals_primal)
    st.residuals_dual = np.array(st.residuals_dual)
    st.residuals = st.residuals_primal
    return x, t, st
