"""Test-side NumPy restatement of bilqr! (src/bilqr.jl:116-484, real Float64), line by line, with an injectable `dot` for kdot and
kdotr (knorm(x) = sqrt(dot(x, x))).  A checker, not product code: tests/test_bilqr_host.py and tests/test_gpu_bilqr.py compare the
library's three loops with it.  sym_givens and the exactly summed dot are those of tests/bilq_reference.py.  Python floats raise on
a division by zero where Julia gives NaN or Inf: `_div` restates Julia's."""
import math
import time
from types import SimpleNamespace

import numpy as np

from bilq_reference import EPS, _op, fsum_dot, history_deviation, sym_givens  # noqa: F401  (re-exported for the tests)

TIRED = "maximum number of iterations exceeded"
BREAKDOWN = "Breakdown ⟨uₖ₊₁,vₖ₊₁⟩ = 0"
BC_BREAKDOWN = "Breakdown bᴴc = 0"
BOTH_C = "Both primal and dual solutions (xᶜ, t) are good enough given atol and rtol"
BOTH_L = "Both primal and dual solutions (xᴸ, t) are good enough given atol and rtol"

# every status string of src/bilqr.jl:179, :215, :452-469
STATUSES = (
    "unknown", BC_BREAKDOWN, TIRED, BREAKDOWN,
    "Only the primal solution xᴸ is good enough given atol and rtol",
    "Only the primal solution xᶜ is good enough given atol and rtol",
    "Only the dual solution t is good enough given atol and rtol",
    BOTH_L, BOTH_C,
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


def _div(a, b):
    """a / b of IEEE doubles: NaN for 0 / 0, a signed infinity for x / 0."""
    if b != 0:
        return a / b
    if a == 0 or a != a:
        return math.nan
    return math.copysign(math.inf, a) * math.copysign(1.0, b)


def _sqrt(a):
    return math.sqrt(a) if a >= 0 else math.nan          # (Julia throws on a negative argument; NaN stays NaN)


def bilqr(A, b, c, x0=None, y0=None, At=None, transfer_to_bicg=True, atol=math.sqrt(EPS), rtol=math.sqrt(EPS), itmax=0,
          timemax=math.inf, history=True, callback=None, dot=np.dot):
    """A, At: callables v -> op v or objects with `@` (At defaults to A.T).  Returns (x, y, stats); stats.vectors holds the work
    vectors by the names of the reference's variables at the end of the loop."""
    start = time.perf_counter()
    mul = _op(A)
    mult = _op(At) if At is not None else (lambda v: A.T @ v)
    norm = lambda v: math.sqrt(float(dot(v, v)))  # noqa: E731
    b = np.asarray(b, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    n = b.shape[0]
    st = SimpleNamespace(niter=0, solved_primal=False, solved_dual=False, status="unknown", residuals_primal=[], residuals_dual=[],
                         beta1=0.0, vectors={})

    def done(x, t):
        st.residuals_primal = np.array(st.residuals_primal)
        st.residuals_dual = np.array(st.residuals_dual)
        return x, t, st

    assert (x0 is None) == (y0 is None), "warm_start!(workspace, x0, y0) takes both"
    dx = None if x0 is None else np.asarray(x0, dtype=np.float64)
    dy = None if y0 is None else np.asarray(y0, dtype=np.float64)
    r0 = b if dx is None else b - mul(dx)                                    # :144-152
    s0 = c if dy is None else c - mult(dy)
    x = np.zeros(n)                                                          # :155-160
    bNorm = norm(r0)
    t = np.zeros(n)
    cNorm = norm(s0)
    it = 0                                                                   # :162-163
    if itmax == 0:
        itmax = 2 * n
    if history:                                                              # :165-166
        st.residuals_primal.append(bNorm)
        st.residuals_dual.append(cNorm)
    epsL = atol + rtol * bNorm                                               # :167-168
    epsQ = atol + rtol * cNorm
    cb = float(dot(s0, r0))                                                  # :173
    if cb == 0:                                                              # :174-184
        st.status = BC_BREAKDOWN
        return done(x if dx is None else x + dx, t if dy is None else t + dy)
    beta = math.sqrt(abs(cb))                                                # :187-188
    st.beta1 = beta
    gamma = cb / beta
    v_prev = np.zeros(n)                                                     # :189-192
    u_prev = np.zeros(n)
    v = r0 / beta
    u = s0 / gamma
    c_prev = ck = -1.0                                                       # :193-194
    s_prev = sk = 0.0
    dbar_vec = np.zeros(n)                                                   # :195
    zeta_m1 = zbar = 0.0                                                     # :196-199
    zeta_m2 = eta = 0.0
    dbar_prev = dbar = 0.0
    psibar_prev = psi = 0.0
    norm_v = bNorm / beta                                                    # :200
    eps_km3 = lam_km2 = 0.0                                                  # :201
    w_km3 = np.zeros(n)                                                      # :202-203
    w_km2 = np.zeros(n)
    tau = 0.0                                                                # :204
    delta = lam = eps_km2 = 0.0
    rNorm_lq = rNorm_cg = sNorm = math.nan
    q = np.zeros(n)
    p = np.zeros(n)
    solved_lq = bNorm == 0                                                   # :207-217
    solved_lq_tol = solved_lq_mach = False
    solved_cg = solved_cg_tol = solved_cg_mach = False
    solved_primal = solved_lq or solved_cg
    solved_qr_tol = solved_qr_mach = False
    solved_dual = cNorm == 0
    tired = it >= itmax
    breakdown = user_exit = overtimed = False
    while not ((solved_primal and solved_dual) or tired or breakdown or user_exit or overtimed):
        it += 1                                                              # :221
        q = mul(v)                                                           # :227-228
        p = mult(u)
        q = q - gamma * v_prev                                               # :230-231
        p = p - beta * u_prev
        alpha = float(dot(u, q))                                             # :233
        q = q - alpha * v                                                    # :235-236
        p = p - alpha * u
        pq = float(dot(p, q))                                                # :238-240
        beta_next = math.sqrt(abs(pq))
        gamma_next = _div(pq, beta_next)
        if it == 1:                                                          # :251-271
            dbar = alpha
        elif it == 2:
            ck, sk, delta = sym_givens(dbar_prev, gamma)
            lam = ck * beta + sk * alpha
            dbar = sk * beta - ck * alpha
        else:
            ck, sk, delta = sym_givens(dbar_prev, gamma)
            eps_km2 = s_prev * beta
            lam = -c_prev * ck * beta + sk * alpha
            dbar = -c_prev * sk * beta - ck * alpha
        if not solved_primal:                                                # :273-348
            if it == 1:
                eta = beta
            if it == 2:
                eta_prev = eta
                zeta_m1 = _div(eta_prev, delta)
                eta = -lam * zeta_m1
            if it >= 3:
                zeta_m2 = zeta_m1
                eta_prev = eta
                zeta_m1 = _div(eta_prev, delta)
                eta = -eps_km2 * zeta_m2 - lam * zeta_m1
            if it == 1:                                                      # :299-311
                dbar_vec = v.copy()
            else:
                x = x + (zeta_m1 * ck) * dbar_vec
                x = x + (zeta_m1 * sk) * v
                dbar_vec = (-ck) * v + sk * dbar_vec
            vv_next = _div(float(dot(v, q)), beta_next)                      # :314-315
            norm_next = _div(norm(q), beta_next)
            if it == 1:                                                      # :319-327
                rNorm_lq = bNorm
            else:
                mu = beta * (s_prev * zeta_m2 - c_prev * ck * zeta_m1) + alpha * sk * zeta_m1
                omega = beta_next * sk * zeta_m1
                theta = mu * omega * vv_next
                rNorm_lq = _sqrt(mu * mu * norm_v ** 2 + omega * omega * norm_next ** 2 + 2 * theta)
            if history:
                st.residuals_primal.append(rNorm_lq)
            norm_v = norm_next                                               # :330
            cg_point = transfer_to_bicg and abs(dbar) > EPS                  # :334-338
            if cg_point:
                zbar = eta / dbar
                rho = beta_next * (sk * zeta_m1 - ck * zbar)
                rNorm_cg = abs(rho) * norm_next
            solved_lq_tol = rNorm_lq <= epsL                                 # :341-347
            solved_lq_mach = rNorm_lq + 1 <= 1
            solved_lq = solved_lq_tol or solved_lq_mach
            solved_cg_tol = bool(cg_point and rNorm_cg <= epsL)
            solved_cg_mach = bool(cg_point and rNorm_cg + 1 <= 1)
            solved_cg = solved_cg_tol or solved_cg_mach
            solved_primal = solved_lq or solved_cg
        if not solved_dual:                                                  # :350-408
            if it == 1:
                psibar = gamma
            else:
                psi = ck * psibar_prev
                psibar = sk * psibar_prev
            if it == 2:                                                      # :363-366
                w_km2 = u_prev / delta
                w_km1 = w_km2
            if it >= 3:                                                      # :368-381
                w_km1 = (-eps_km3) * w_km3 if it >= 4 else w_km3
                w_km1 = w_km1 + 1.0 * u_prev
                w_km1 = w_km1 + (-lam_km2) * w_km2
                w_km1 = w_km1 * (1.0 / delta)                                # kdiv! = kscal!(one(T) / δ), src/krylov_utils.jl
                w_km3 = w_km1
                w_km3, w_km2 = w_km2, w_km3                                  # :383-386
            if it >= 2:                                                      # :388-392
                t = t + psi * w_km1
            psibar_prev = psibar                                             # :395
            tau = tau + float(dot(u, u))                                     # :398
            sNorm = abs(psibar) * math.sqrt(tau)                             # :401-402
            if history:
                st.residuals_dual.append(sNorm)
            solved_qr_tol = sNorm <= epsQ                                    # :405-407
            solved_qr_mach = sNorm + 1 <= 1
            solved_dual = solved_qr_tol or solved_qr_mach
        v_prev = v                                                           # :411-418
        u_prev = u
        if pq != 0:
            v = q / beta_next
            u = p / gamma_next
        if it >= 3:                                                          # :421-431
            eps_km3 = eps_km2
        if it >= 2:
            lam_km2 = lam
        dbar_prev, c_prev, s_prev = dbar, ck, sk
        gamma, beta = gamma_next, beta_next
        if callback is not None:                                             # :433
            st.niter = it
            user_exit = bool(callback(SimpleNamespace(x=x, y=t, stats=st)))
        tired = it >= itmax                                                  # :434-437
        breakdown = (not solved_lq) and (not solved_cg) and pq == 0
        overtimed = (time.perf_counter() - start) > timemax
    if solved_cg:                                                            # :447-449
        x = x + zbar * dbar_vec
    status = "unknown"                                                       # :452-469
    for cond, text in ((tired, TIRED), (breakdown, BREAKDOWN),
                       (solved_lq_tol and not solved_dual, STATUSES[4]), (solved_cg_tol and not solved_dual, STATUSES[5]),
                       (not solved_primal and solved_qr_tol, STATUSES[6]), (solved_lq_tol and solved_qr_tol, STATUSES[7]),
                       (solved_cg_tol and solved_qr_tol, STATUSES[8]), (solved_lq_mach and not solved_dual, STATUSES[9]),
                       (solved_cg_mach and not solved_dual, STATUSES[10]), (not solved_primal and solved_qr_mach, STATUSES[11]),
                       (solved_lq_mach and solved_qr_mach, STATUSES[12]), (solved_cg_mach and solved_qr_mach, STATUSES[13]),
                       (solved_lq_mach and solved_qr_tol, STATUSES[14]), (solved_cg_mach and solved_qr_tol, STATUSES[15]),
                       (solved_lq_tol and solved_qr_mach, STATUSES[16]), (solved_cg_tol and solved_qr_mach, STATUSES[17]),
                       (user_exit, "user-requested exit"), (overtimed, "time limit exceeded")):
        if cond:
            status = text
    st.vectors = dict(u_prev=u_prev, u=u, q=q, v_prev=v_prev, v=v, p=p, dbar=dbar_vec, w_prev3=w_km3, w_prev2=w_km2)
    if dx is not None:                                                       # :472-473
        x = x + dx
        t = t + dy
    st.niter, st.solved_primal, st.solved_dual, st.status = it, bool(solved_primal), bool(solved_dual), status
    return done(x, t)
