// solver_device.hpp -- device-resident scalar state of the solver loops ("fused = 2").
//
// The reference's cg! (src/cg.jl:195-268) computes its scalars (alpha, beta, pNorm^2, the stopping
// tests) on the host between kernels: two host round trips per iteration.  Here the same scalar
// recurrences run as an EPILOGUE of the reduction that produces their input (last thread of the finish
// kernel, or of the cross-rank combine kernel), in the same IEEE double operations and order as the
// host code, and the vector kernels read alpha / beta from this struct.  The host only enqueues
// iterations ahead and polls a snapshot; once a stopping test fires the epilogue lowers `stop_seq` and
// every later kernel of the queue (each carries its own sequence number) returns immediately, so the
// vectors end in exactly the state the reference's loop leaves them in.
#pragma once

#include <hip/hip_runtime.h>

namespace khip {

enum Epilogue { EPI_NONE = 0, EPI_CG_STEP1 = 1, EPI_CG_STEP2 = 2, EPI_BICG_A = 3, EPI_BICG_B = 4, EPI_BICG_C = 5, EPI_CGCG = 6,
               EPI_MINRES_A = 7, EPI_MINRES_B = 8, EPI_MINRES_C = 9, EPI_LZSHIFT_A = 10, EPI_LZSHIFT_B = 11,
               EPI_BILQ_A = 12, EPI_BILQ_B = 13, EPI_BILQ_C = 14, EPI_QMR_A = 15, EPI_QMR_B = 16, EPI_QMR_C = 17,
               EPI_BILQR_A = 18, EPI_BILQR_B = 19, EPI_BILQR_C = 20, EPI_CGS_A = 21, EPI_CGS_B = 22,
               EPI_SYMMLQ_A = 23, EPI_SYMMLQ_B = 24, EPI_MINRES_QLP_X = 25, EPI_MINRES_QLP_A = 26, EPI_MINRES_QLP_B = 27,
               EPI_USYMQR_A = 28, EPI_USYMQR_B = 29, EPI_USYMLQ_A = 30, EPI_USYMLQ_B = 31,
               EPI_TRILQR_A = 32, EPI_TRILQR_B = 33, EPI_TRICG_A = 34, EPI_TRICG_B = 35,
               EPI_TRIMR_A = 36, EPI_TRIMR_B = 37, EPI_USYMLQR_A = 38, EPI_USYMLQR_B = 39 };

struct CgDevState {
  double gamma;        // r.z of the current iterate              (src/cg.jl:162, 257)
  double pAp;          //                                          (:197)
  double alpha;        // gamma / pAp                              (:213)
  double alpha_prev;   // alpha of the iteration before: the x update a light iteration left pending (cg_defer_x, solvers.cpp)
  double beta;         // gamma_next / gamma                       (:256)
  double pNorm2;       //                                          (:257)
  double rNorm;        // sqrt(gamma_next)                         (:243)
  double eps_tol;      // atol + rtol * rNorm0                     (:186)
  double keps;         // eps(Float64) in the curvature test       (:198)
  long long stop_seq;  // kernels whose sequence number is >= stop_seq do nothing
  long long iter;      // completed iterations
  long long hist_base; // hist[k - 1 - hist_base] = rNorm after iteration k
  long long hist_cap;
  double *hist;        // device history window (null: no history)
  int solved, zero_curvature, inconsistent, not_spd;
};

// Single-reduction CG (Chronopoulos & Gear 1989): per iteration ONE reduction delivers
// gamma' = r.r and delta = (A r).r, from which beta = gamma'/gamma and alpha = gamma' / (delta - beta gamma'/alpha).
struct CgcgDevState {
  double gamma, alpha, beta, rNorm, eps_tol;
  long long stop_seq, iter, hist_base, hist_cap;
  double *hist;
  int solved, breakdown;      // breakdown: the alpha denominator is not positive (operator not SPD / loss of accuracy)
};

// bicgstab! (src/bicgstab.jl:213-253) with M = N = I: the scalars of one iteration
struct BicgDevState {
  double rho;          // c.r of the current iterate                 (:215)
  double alpha;        // rho / c.v                                   (:223)
  double omega;        // t.s / t.t                                   (:230)
  double beta;         // (next_rho / rho) (alpha / omega)            (:235)
  double rNorm;        // ||r||                                        (:240)
  double eps_tol;      // atol + rtol * rNorm0                        (:189)
  long long stop_seq;
  long long iter;
  long long hist_base;
  long long hist_cap;
  double *hist;
  int solved, breakdown;
};

constexpr long long kSeqNever = 0x7fffffffffffffffLL;

// minres! (src/minres.jl:164-484) with linesearch = false: the scalars of the Lanczos recurrence and of the Givens QR, the
// norm estimates and the stopping tests.  The same three steps run on the host (host-driven loop, fused = 1) and as the
// epilogues of the three reductions of an iteration (device-resident loop, fused = 2): one source, the same IEEE operations in
// the reference's order, so both loops produce the same bits.  Field names follow the reference.
constexpr int kMinresWindowMax = 64;     // err_vec entries the device state carries; larger windows run the host-driven loop

struct MinresDevState {
  // the Lanczos product's coefficients, contiguous: the sliced SpMV reads them as SpmvArgs::lz_coef[0..2]
  double lambda;       // λ                                            (:173)
  double inv_beta;     // one(T) / β: kdiv!(y, β) (:284) and the v / β term of w (:299)
  double c_r1;         // -β / oldβ                                    (:285)
  // constants of the solve
  double beta1;        // β₁                                           (:231)
  double eps_tol;      // ε = atol + rtol β₁                           (:274)
  double etol, ctol;   // etol, 1 / conlim                             (:202)
  long long itmax;
  int window, MisI;
  // recurrences (values of the current iteration)
  double beta, oldbeta, alpha, delta, dbar, epsln;   // β, oldβ, α, δ, δbar, ϵ
  double cs, sn, phibar, phi, gamma, gbar, root;     // cs, sn, ϕbar, ϕ, γ, γbar, root
  double gmin, gmax, ANorm2, xENorm2, rhs1, rhs2, err_lbnd;
  double rNorm, ArNorm, Acond, ANorm, xNorm, test1, test2;
  // coefficients the vector kernels read
  double c_r2;         // -α / β                                       (:288)
  double inv_gamma;    // one(T) / γ: kdiv!(w, γ)                      (:325)
  long long stop_seq, iter, hist_base, hist_cap;
  double *hist_r, *hist_ar, *hist_acond;   // device history windows (null: no history)
  int solved, zero_resid, ill_cond_mach, ill_cond_lim, fwd_err, lsq_exit, not_pd;
  double err_vec[kMinresWindowMax];
};

// Julia's max / min on Float64 (NaN wins)
__host__ __device__ inline double jl_max(double a, double b) { return (a != a || b != b) ? a + b : (a > b ? a : b); }
__host__ __device__ inline double jl_min(double a, double b) { return (a != a || b != b) ? a + b : (a < b ? a : b); }

// after the dot v.y of the Lanczos product (:287-288, :291)
__host__ __device__ inline void minres_step_a(MinresDevState &s, double vy) {
  s.alpha = vy / s.beta;
  s.c_r2 = -s.alpha / s.beta;
  s.delta = s.cs * s.dbar + s.sn * s.alpha;
}

// after beta^2 = r2.v of the next Lanczos vector (:305-336, :348-351); false when beta^2 < 0 (M not positive definite)
__host__ __device__ inline bool minres_step_b(MinresDevState &s, double beta2, long long k) {
  s.oldbeta = s.beta;
  if (beta2 < 0) { s.not_pd = 1; return false; }
  s.beta = sqrt(beta2);
  s.ANorm2 = s.ANorm2 + s.alpha * s.alpha + s.oldbeta * s.oldbeta + s.beta * s.beta;
  s.gbar = s.sn * s.dbar - s.cs * s.alpha;
  s.epsln = s.sn * s.beta;
  s.dbar = -s.cs * s.beta;
  s.root = sqrt(s.gbar * s.gbar + s.dbar * s.dbar);
  s.ArNorm = s.phibar * s.root;
  double g = sqrt(s.gbar * s.gbar + s.beta * s.beta);
  s.gamma = jl_max(g, 2.220446049250313e-16);
  s.inv_gamma = 1.0 / s.gamma;
  s.cs = s.gbar / s.gamma;
  s.sn = s.beta / s.gamma;
  s.phi = s.cs * s.phibar;
  s.phibar = s.sn * s.phibar;
  s.inv_beta = 1.0 / s.beta;       // for the next iteration's product and w update
  s.c_r1 = -s.beta / s.oldbeta;
  if (s.hist_ar) {
    const long long idx = k - 1 - s.hist_base;
    if (idx >= 0 && idx < s.hist_cap) s.hist_ar[idx] = s.ArNorm;
  }
  return true;
}

// after xNorm = knorm(n, x) of the updated iterate (:378, :385-451); k = iter.  err_vec: window entries.  True when the loop stops.
__host__ __device__ inline bool minres_step_c(MinresDevState &s, double xNorm, long long k, double *err_vec) {
  const double epsM = 2.220446049250313e-16;
  s.xENorm2 = s.xENorm2 + s.phi * s.phi;
  const int window = s.window;
  err_vec[k % window] = s.phi;
  if (k >= window) {                          // knorm(window, err_vec)
    double acc = 0.0;
    for (int i = 0; i < window; ++i) acc = acc + err_vec[i] * err_vec[i];
    s.err_lbnd = sqrt(acc);
  }
  s.gmax = jl_max(s.gmax, s.gamma);
  s.gmin = jl_min(s.gmin, s.gamma);
  const double zeta = s.rhs1 / s.gamma;
  s.rhs1 = s.rhs2 - s.delta * zeta;
  s.rhs2 = -s.epsln * zeta;
  s.ANorm = sqrt(s.ANorm2);
  s.xNorm = xNorm;
  s.rNorm = s.phibar;
  s.test1 = s.rNorm / (s.ANorm * s.xNorm);
  s.test2 = s.root / s.ANorm;
  s.Acond = s.gmax / s.gmin;
  if (s.hist_r) {
    const long long idx = k - 1 - s.hist_base;
    if (idx >= 0 && idx < s.hist_cap) { s.hist_r[idx] = s.rNorm; s.hist_acond[idx] = s.Acond; }
  }
  s.iter = k;
  if (k == 1 && s.beta / s.beta1 <= 10 * epsM) {   // A b = 0: x = 0 is a minimum least-squares solution (:410-419)
    s.lsq_exit = 1;
    s.solved = 1;
    return true;
  }
  const double inv_acond = 1.0 / s.Acond;
  s.ill_cond_mach = (1.0 + inv_acond <= 1.0);
  const bool solved_mach = (1.0 + s.test2 <= 1.0);
  const bool zero_resid_mach = (1.0 + s.test1 <= 1.0);
  const bool resid_decrease_mach = (s.rNorm + 1.0 <= 1.0);
  const bool tired = k >= s.itmax;
  s.ill_cond_lim = (inv_acond <= s.ctol);
  const bool solved_lim = (s.test2 <= s.eps_tol);
  const bool zero_resid_lim = s.MisI && (s.test1 <= epsM);
  const bool resid_decrease_lim = (s.rNorm <= s.eps_tol);
  if (k >= window) s.fwd_err = (s.err_lbnd <= s.etol * sqrt(s.xENorm2));
  s.zero_resid = zero_resid_mach || zero_resid_lim;
  const bool resid_decrease = resid_decrease_mach || resid_decrease_lim;
  const bool ill_cond = s.ill_cond_mach || s.ill_cond_lim;
  s.solved = solved_mach || solved_lim || s.zero_resid || s.fwd_err || resid_decrease;
  return s.solved || tired || ill_cond;
}

// cg_lanczos_shift! (src/cg_lanczos_shift.jl:107-284): the Lanczos scalars and the per-shift CG scalars of a family
// (A + s_i I) x_i = b.  The same code runs on the host (loops 0 and 1) and as the epilogue of the w.w reduction of an iteration
// (device-resident loop): one source, the reference's IEEE operations in its order, so loops 1 and 2 produce the same bits.
// The per-shift arrays sit in the state for the device-resident loop (p <= kShiftMax); the host loops keep their own.
constexpr int kShiftMax = 64;            // shifts the device state carries; more shifts run the host-driven loop

struct LanczosShiftDevState {
  double delta;        // δ = vᴴ A v of the current iteration                (:200)
  double beta;         // β: βₖ while the iteration runs, βₖ₊₁ after its step   (:187, :208)
  double inv_beta;     // one(T) / β: kdiv!(v, β)                             (:209)
  double rho;          // ‖v‖² (one(T) with M = I)                              (:214)
  double eps_tol;      // ε = atol + rtol β₁                                   (:238)
  long long stop_seq, iter, hist_base, hist_cap;
  double *hist;        // device history window: row k - 1 - hist_base holds iteration k's rNorms, one entry per shift
  int nshifts, check_curvature, solved, pad;
  // not_cv at the top of the update loop (:226-229) as the list P2 walks: act[0] = count, act[1 + j] = shift;
  // coef[3 j .. 3 j + 2] = (γ, σ, ω) of that shift, the coefficients of its kaxpy! and kaxpby!
  int act[kShiftMax + 1];
  int converged[kShiftMax], not_cv[kShiftMax], indefinite[kShiftMax];
  long long nhist[kShiftMax];        // entries pushed to each shift's history after β₁: the last iteration the shift was active
  double coef[3 * kShiftMax];
  double shifts[kShiftMax], sigma[kShiftMax], dhat[kShiftMax], omega[kShiftMax], gamma[kShiftMax], rNorms[kShiftMax];
};

// the per-shift arrays the scalar code works on: the device state's own, or the host loops' (any number of shifts)
struct LzShiftArrays {
  const double *shifts;
  double *sigma, *dhat, *omega, *gamma, *rNorms, *coef;
  int *converged, *not_cv, *indefinite, *act;
  long long *nhist;
};
__host__ __device__ inline LzShiftArrays lzshift_arrays(LanczosShiftDevState &s) {
  return LzShiftArrays{s.shifts, s.sigma, s.dhat, s.omega, s.gamma, s.rNorms, s.coef, s.converged, s.not_cv, s.indefinite, s.act,
                       s.nhist};
}

// β = knorm_elliptic(v, Mv) (:208): β² -> β, one(T) / β
__host__ __device__ inline void lzshift_beta(LanczosShiftDevState &s, double beta2) {
  s.beta = sqrt(beta2);
  s.inv_beta = 1.0 / s.beta;
}

// the per-shift loops of iteration k (:212-252) with s.delta, s.rho and the new s.beta; hist_row: where the pushed rNorms go
// (null: nowhere).  True when no shift is left (solved = !any(not_cv)).
__host__ __device__ inline bool lzshift_step(LanczosShiftDevState &s, const LzShiftArrays &a, long long k, double *hist_row) {
  const int p = s.nshifts;
  for (int i = 0; i < p; ++i) {
    a.dhat[i] = s.delta + s.rho * a.shifts[i];
    a.gamma[i] = 1.0 / (a.dhat[i] - a.omega[i] / a.gamma[i]);
  }
  for (int i = 0; i < p; ++i) a.indefinite[i] |= (a.gamma[i] <= 0) ? 1 : 0;
  int nact = 0;
  for (int i = 0; i < p; ++i) {
    a.not_cv[i] = s.check_curvature ? !(a.converged[i] || a.indefinite[i]) : !a.converged[i];
    if (a.not_cv[i]) {
      a.act[1 + nact] = i;
      a.coef[3 * nact] = a.gamma[i];
      a.omega[i] = s.beta * a.gamma[i];
      a.sigma[i] = a.sigma[i] * -a.omega[i];
      a.omega[i] = a.omega[i] * a.omega[i];
      a.coef[3 * nact + 1] = a.sigma[i];
      a.coef[3 * nact + 2] = a.omega[i];
      ++nact;
      a.rNorms[i] = fabs(a.sigma[i]);
      a.converged[i] = a.rNorms[i] <= s.eps_tol;
      if (hist_row) hist_row[i] = a.rNorms[i];       // the push uses this not_cv (:245-249)
      a.nhist[i] = k;
    }
  }
  a.act[0] = nact;
  bool any = false;
  for (int i = 0; i < p; ++i) {
    a.not_cv[i] = s.check_curvature ? !(a.converged[i] || a.indefinite[i]) : !a.converged[i];
    any = any || a.not_cv[i];
  }
  s.iter = k;
  s.solved = any ? 0 : 1;
  return !any;
}

// sym_givens(a, b) for reals, src/krylov_utils.jl:21-51: one source for the host code of gmres! and for the epilogues below
__host__ __device__ inline double sym_givens_sign(double v) { return v > 0 ? 1.0 : (v < 0 ? -1.0 : 0.0); }
__host__ __device__ inline void sym_givens(double a, double b, double &c, double &s, double &rho) {
  if (b == 0.0) {
    c = sym_givens_sign(a) + (a == 0.0 ? 1.0 : 0.0);
    s = 0.0;
    rho = fabs(a);
  } else if (a == 0.0) {
    c = 0.0;
    s = sym_givens_sign(b);
    rho = fabs(b);
  } else if (fabs(b) > fabs(a)) {
    const double t = a / b;
    s = sym_givens_sign(b) / sqrt(1.0 + t * t);
    c = s * t;
    rho = b / s;
  } else {
    const double t = b / a;
    c = sym_givens_sign(a) / sqrt(1.0 + t * t);
    s = c * t;
    rho = a / c;
  }
}

// bilq! (src/bilq.jl:118-407), real Float64: the scalars of the two-sided Lanczos process, of the LQ factorisation of Tₖ, the
// residual estimates of the LQ and CG points and the stopping tests.  The same three steps run on the host (loops 0 and 1) and as
// the epilogues of the three reductions of an iteration (device-resident loop): one source, the reference's IEEE operations in its
// order, so loops 1 and 2 produce the same bits.  Field names follow the reference.
// The coefficients of the two-sided Lanczos process that P1 and P2 (bilanczos_passes.hpp) read: the common leading part of the states
// of bilq! and qmr!, which run the same biorthogonalisation (src/bilq.jl:234-252 = src/qmr.jl:238-258).
struct BiLanczosCoef {
  double gamma, beta;            // γₖ, βₖ: P1                                   (src/bilq.jl:244-245, src/qmr.jl:248-249)
  double alpha;                  // αₖ: P2                                       (src/bilq.jl:247-250, src/qmr.jl:251-254)
};

struct BilqDevState : BiLanczosCoef {
  // coefficients the vector kernels read (γₖ, βₖ, αₖ: BiLanczosCoef)
  double beta_next, gamma_next;  // βₖ₊₁, γₖ₊₁: the divisors of P3               (:253-254, :329-330)
  double pq;                     // pᴴq                                          (:252)
  double zc, zs, neg_c, sn;      // ζₖ₋₁cₖ, ζₖ₋₁sₖ, -cₖ, sₖ: the x and d̅ updates (:316-321)
  // constants of the solve
  double bNorm, eps_tol;         // ‖r₀‖, ε = atol + rtol ‖r₀‖                   (:169, :199)
  // recurrences
  double cs, cs_prev, sn_prev;   // cₖ, cₖ₋₁, sₖ₋₁
  double delta, lambda, epsilon; // δₖ₋₁, λₖ₋₁, ϵₖ₋₂
  double dbar, dbar_prev;        // δbarₖ, δbarₖ₋₁
  double zeta_m1, zeta_m2, zbar; // ζₖ₋₁, ζₖ₋₂, ζbarₖ
  double eta, eta_prev;          // ηₖ, ηₖ₋₁
  double norm_v;                 // ‖vₖ‖
  double rNorm_lq, rNorm_cg;
  long long stop_seq, iter, hist_base, hist_cap;
  double *hist;                  // device history window (null: no history)
  int transfer_to_bicg, solved_lq, solved_cg, breakdown;
};

// after αₖ = ⟨uₖ, q⟩ (:247)
__host__ __device__ inline void bilq_step_a(BilqDevState &s, double uq) { s.alpha = uq; }

// after pᴴq = ⟨p, q⟩: βₖ₊₁, γₖ₊₁ and the LQ update (:252-305); k = iter
__host__ __device__ inline void bilq_step_b(BilqDevState &s, double pq, long long k) {
  s.pq = pq;
  s.beta_next = sqrt(fabs(pq));
  s.gamma_next = pq / s.beta_next;
  if (k == 1) {
    s.dbar = s.alpha;
  } else if (k == 2) {
    sym_givens(s.dbar_prev, s.gamma, s.cs, s.sn, s.delta);
    s.lambda = s.cs * s.beta + s.sn * s.alpha;
    s.dbar = s.sn * s.beta - s.cs * s.alpha;
  } else {
    sym_givens(s.dbar_prev, s.gamma, s.cs, s.sn, s.delta);
    s.epsilon = s.sn_prev * s.beta;
    s.lambda = -s.cs_prev * s.cs * s.beta + s.sn * s.alpha;
    s.dbar = -s.cs_prev * s.sn * s.beta - s.cs * s.alpha;
  }
  if (k == 1) s.eta = s.beta;
  if (k == 2) {
    s.zeta_m1 = s.eta_prev / s.delta;
    s.eta = -s.lambda * s.zeta_m1;
  }
  if (k >= 3) {
    s.zeta_m2 = s.zeta_m1;
    s.zeta_m1 = s.eta_prev / s.delta;
    s.eta = -s.epsilon * s.zeta_m2 - s.lambda * s.zeta_m1;
  }
  s.zc = s.zeta_m1 * s.cs;
  s.zs = s.zeta_m1 * s.sn;
  s.neg_c = -s.cs;
}

// after ⟨vₖ, vₖ₊₁⟩ and ‖vₖ₊₁‖ (:334-371): the residual estimates, the history entry, the shifts and the tests; true when the loop
// stops (tired / overtimed / the callback are the driver's)
__host__ __device__ inline bool bilq_step_c(BilqDevState &s, double vv_next, double norm_next, long long k) {
  if (k == 1) {
    s.rNorm_lq = s.bNorm;
  } else {
    const double mu = s.beta * (s.sn_prev * s.zeta_m2 - s.cs_prev * s.cs * s.zeta_m1) + s.alpha * s.sn * s.zeta_m1;
    const double omega = s.beta_next * s.sn * s.zeta_m1;
    const double theta = mu * omega * vv_next;
    s.rNorm_lq = sqrt(mu * mu * (s.norm_v * s.norm_v) + omega * omega * (norm_next * norm_next) + 2 * theta);
  }
  if (s.hist) {
    const long long idx = k - 1 - s.hist_base;
    if (idx >= 0 && idx < s.hist_cap) s.hist[idx] = s.rNorm_lq;
  }
  const bool cg_point = s.transfer_to_bicg && (fabs(s.dbar) > 2.220446049250313e-16);
  if (cg_point) {
    s.zbar = s.eta / s.dbar;
    const double rho = s.beta_next * (s.sn * s.zeta_m1 - s.cs * s.zbar);
    s.rNorm_cg = fabs(rho) * norm_next;
  }
  s.sn_prev = s.sn;
  s.cs_prev = s.cs;
  s.eta_prev = s.eta;
  s.gamma = s.gamma_next;
  s.beta = s.beta_next;
  s.dbar_prev = s.dbar;
  s.norm_v = norm_next;
  s.solved_lq = (s.rNorm_lq <= s.eps_tol) ? 1 : 0;
  s.solved_cg = (cg_point && s.rNorm_cg <= s.eps_tol) ? 1 : 0;
  s.breakdown = (!s.solved_lq && !s.solved_cg && s.pq == 0.0) ? 1 : 0;
  s.iter = k;
  return s.solved_lq || s.solved_cg || s.breakdown;
}

// qmr! (src/qmr.jl:124-406), real Float64: the scalars of the two-sided Lanczos process, of the QR factorisation of Tₖ₊₁.ₖ, the
// residual bound |ζbarₖ₊₁| √τₖ₊₁ and the stopping tests.  As for bilq!: the same three steps run on the host (loops 0 and 1) and as
// the epilogues of the three reductions of an iteration (device-resident loop), so loops 1 and 2 produce the same bits.
struct QmrDevState : BiLanczosCoef {
  // coefficients the vector kernels read (γₖ, βₖ, αₖ: BiLanczosCoef)
  double beta_next, gamma_next;  // βₖ₊₁, γₖ₊₁: the divisors of P3               (:257-258, :345-346)
  double pq;                     // pᴴq                                          (:256)
  double neg_eps, neg_lambda;    // -ϵₖ₋₂, -λₖ₋₁: kscal! and the first kaxpy! of wₖ (:329, :331)
  double delta, inv_delta;       // δₖ: kdivcopy!(w₁, v₁, δ₁) (:318); one(T) / δₖ: kdiv!(wₖ, δₖ) = kscal!(one(T) / δₖ) (:325, :333)
  double zeta;                   // ζₖ: x = x + ζₖ wₖ                             (:338)
  // constants of the solve
  double eps_tol;                // ε = atol + rtol ‖r₀‖                          (:205)
  // recurrences
  double c_km2, c_km1, s_km2, s_km1;   // cₖ₋₂, cₖ₋₁, sₖ₋₂, sₖ₋₁
  double epsilon, lambda;        // ϵₖ₋₂, λₖ₋₁
  double zbar, zbar_next;        // ζbarₖ, ζbarₖ₊₁
  double tau;                    // τₖ
  double rNorm;
  long long stop_seq, iter, hist_base, hist_cap;
  double *hist;                  // device history window (null: no history)
  int solved, breakdown;
};

// after αₖ = ⟨uₖ, q⟩ (:251)
__host__ __device__ inline void qmr_step_a(QmrDevState &s, double uq) { s.alpha = uq; }

// after pᴴq = ⟨p, q⟩: βₖ₊₁, γₖ₊₁, the two previous reflections, the new one, ζₖ and ζbarₖ₊₁ (:256-312); k = iter
__host__ __device__ inline void qmr_step_b(QmrDevState &s, double pq, long long k) {
  s.pq = pq;
  s.beta_next = sqrt(fabs(pq));
  s.gamma_next = pq / s.beta_next;
  double lbar = 0.0, dbar;       // λbarₖ₋₁, δbarₖ
  if (k >= 3) {
    s.epsilon = s.s_km2 * s.gamma;
    lbar = -s.c_km2 * s.gamma;
  }
  if (k >= 2) {
    if (k == 2) lbar = s.gamma;
    s.lambda = s.c_km1 * lbar + s.s_km1 * s.alpha;
    dbar = s.s_km1 * lbar - s.c_km1 * s.alpha;
    s.s_km2 = s.s_km1;
    s.c_km2 = s.c_km1;
  } else {
    dbar = s.alpha;
  }
  double c, sn;
  sym_givens(dbar, s.beta_next, c, sn, s.delta);
  s.zeta = c * s.zbar;
  s.zbar_next = sn * s.zbar;
  s.s_km1 = sn;
  s.c_km1 = c;
  s.neg_eps = -s.epsilon;
  s.neg_lambda = -s.lambda;
  s.inv_delta = 1.0 / s.delta;
}

// after ‖vₖ₊₁‖² = ⟨vₖ₊₁, vₖ₊₁⟩ (:350-376): τₖ₊₁, the residual bound, the history entry, the shifts and the tests; true when the
// loop stops (tired / overtimed / the callback are the driver's)
__host__ __device__ inline bool qmr_step_c(QmrDevState &s, double vv_next, long long k) {
  const double tau_next = s.tau + vv_next;
  s.rNorm = fabs(s.zbar_next) * sqrt(tau_next);
  if (s.hist) {
    const long long idx = k - 1 - s.hist_base;
    if (idx >= 0 && idx < s.hist_cap) s.hist[idx] = s.rNorm;
  }
  s.zbar = s.zbar_next;
  s.beta = s.beta_next;
  s.gamma = s.gamma_next;
  s.tau = tau_next;
  const bool resid_decrease_mach = (s.rNorm + 1.0 <= 1.0);
  const bool resid_decrease_lim = (s.rNorm <= s.eps_tol);
  s.solved = (resid_decrease_lim || resid_decrease_mach) ? 1 : 0;
  s.breakdown = (!s.solved && s.pq == 0.0) ? 1 : 0;
  s.iter = k;
  return s.solved || s.breakdown;
}

// bilqr! (src/bilqr.jl:116-484), real Float64: ONE two-sided Lanczos process that advances the BiLQ iterate of A x = b (with the
// BiCG transfer) and the QMR iterate of Aᴴ y = c.  As for bilq! and qmr!: the same three steps run on the host (loops 0 and 1) and as
// the epilogues of the three reductions of an iteration (device-resident loop), so loops 1 and 2 produce the same bits.  The primal
// block is frozen once solved_primal is set, the dual block once solved_dual is set; the LQ factorisation and the shifts go on.
struct BilqrDevState : BiLanczosCoef {
  // coefficients the vector kernels read (γₖ, βₖ, αₖ: BiLanczosCoef)
  double beta_next, gamma_next;  // βₖ₊₁, γₖ₊₁: the divisors of P3               (:239-240, :416-417)
  double pq;                     // pᴴq                                          (:238)
  double zc, zs, neg_c, sn;      // ζₖ₋₁cₖ, ζₖ₋₁sₖ, -cₖ, sₖ: the x and d̅ updates (:305-310)
  double neg_eps3, neg_lambda2;  // -ϵₖ₋₃, -λₖ₋₂: kscal! and the second kaxpy! of wₖ₋₁ (:371, :376, :379)
  double delta, inv_delta;       // δₖ₋₁: kdivcopy!(w₁, u₁, δ₁) (:365); one(T) / δₖ₋₁: kdiv! = kscal!(one(T) / δₖ₋₁) (:372, :380)
  double psi;                    // ψₖ₋₁: t = t + ψₖ₋₁ wₖ₋₁                       (:391)
  // constants of the solve
  double bNorm, eps_L, eps_Q;    // ‖r₀‖, εL = atol + rtol ‖r₀‖, εQ = atol + rtol ‖s₀‖ (:156, :167-168)
  // recurrences
  double cs, cs_prev, sn_prev;   // cₖ, cₖ₋₁, sₖ₋₁
  double lambda, epsilon;        // λₖ₋₁, ϵₖ₋₂
  double lambda2, eps3;          // λₖ₋₂, ϵₖ₋₃
  double dbar, dbar_prev;        // δbarₖ, δbarₖ₋₁
  double zeta_m1, zeta_m2, zbar; // ζₖ₋₁, ζₖ₋₂, ζbarₖ
  double eta;                    // ηₖ
  double norm_v;                 // ‖vₖ‖
  double psibar, psibar_prev;    // ψbarₖ, ψbarₖ₋₁
  double tau;                    // τₖ
  double uu;                     // ‖uₖ‖², carried from the previous iteration's P3 (‖u₁‖² from the set-up) to :398
  double rNorm_lq, rNorm_cg, sNorm;
  long long stop_seq, iter, hist_base, hist_cap;
  long long nhist_p, nhist_d;    // the last iteration that pushed to the primal / dual history: each side stops when it is solved
  double *hist_p, *hist_d;       // device history windows (null: no history)
  int transfer_to_bicg, breakdown;
  int solved_lq, solved_cg, solved_primal, solved_dual;
  int solved_lq_tol, solved_lq_mach, solved_cg_tol, solved_cg_mach, solved_qr_tol, solved_qr_mach;
};

// after αₖ = ⟨uₖ, q⟩ (:233)
__host__ __device__ inline void bilqr_step_a(BilqrDevState &s, double uq) { s.alpha = uq; }

// after pᴴq = ⟨p, q⟩: βₖ₊₁, γₖ₊₁, the LQ update, ζₖ₋₁ and ηₖ of an unsolved primal side, ψₖ₋₁ and ψbarₖ of an unsolved dual side
// (:238-294, :350-359) and the coefficients P3 reads; k = iter
__host__ __device__ inline void bilqr_step_b(BilqrDevState &s, double pq, long long k) {
  s.pq = pq;
  s.beta_next = sqrt(fabs(pq));
  s.gamma_next = pq / s.beta_next;
  if (k == 1) {
    s.dbar = s.alpha;
  } else if (k == 2) {
    sym_givens(s.dbar_prev, s.gamma, s.cs, s.sn, s.delta);
    s.lambda = s.cs * s.beta + s.sn * s.alpha;
    s.dbar = s.sn * s.beta - s.cs * s.alpha;
  } else {
    sym_givens(s.dbar_prev, s.gamma, s.cs, s.sn, s.delta);
    s.epsilon = s.sn_prev * s.beta;
    s.lambda = -s.cs_prev * s.cs * s.beta + s.sn * s.alpha;
    s.dbar = -s.cs_prev * s.sn * s.beta - s.cs * s.alpha;
  }
  if (!s.solved_primal) {
    if (k == 1) s.eta = s.beta;
    if (k == 2) {
      const double eta_prev = s.eta;
      s.zeta_m1 = eta_prev / s.delta;
      s.eta = -s.lambda * s.zeta_m1;
    }
    if (k >= 3) {
      s.zeta_m2 = s.zeta_m1;
      const double eta_prev = s.eta;
      s.zeta_m1 = eta_prev / s.delta;
      s.eta = -s.epsilon * s.zeta_m2 - s.lambda * s.zeta_m1;
    }
    s.zc = s.zeta_m1 * s.cs;
    s.zs = s.zeta_m1 * s.sn;
    s.neg_c = -s.cs;
  }
  if (!s.solved_dual) {
    if (k == 1) {
      s.psibar = s.gamma;
    } else {
      s.psi = s.cs * s.psibar_prev;
      s.psibar = s.sn * s.psibar_prev;
    }
    s.neg_eps3 = -s.eps3;
    s.neg_lambda2 = -s.lambda2;
    s.inv_delta = 1.0 / s.delta;
  }
}

// after ⟨vₖ, q⟩, ‖q‖ and ‖uₖ₊₁‖² (:313-347, :394-435): the residual estimates of the sides still unsolved, their history entries, the
// shifts and the tests; true when the loop stops (tired / overtimed / the callback are the driver's).  βₖ₊₁ = 0 divides as in the
// reference: the estimates become NaN and no test holds.
__host__ __device__ inline bool bilqr_step_c(BilqrDevState &s, double vq, double q_norm, double uu_next, long long k) {
  const double epsM = 2.220446049250313e-16;
  if (!s.solved_primal) {
    const double vv_next = vq / s.beta_next;
    const double norm_next = q_norm / s.beta_next;
    if (k == 1) {
      s.rNorm_lq = s.bNorm;
    } else {
      const double mu = s.beta * (s.sn_prev * s.zeta_m2 - s.cs_prev * s.cs * s.zeta_m1) + s.alpha * s.sn * s.zeta_m1;
      const double omega = s.beta_next * s.sn * s.zeta_m1;
      const double theta = mu * omega * vv_next;
      s.rNorm_lq = sqrt(mu * mu * (s.norm_v * s.norm_v) + omega * omega * (norm_next * norm_next) + 2 * theta);
    }
    if (s.hist_p) {
      const long long idx = k - 1 - s.hist_base;
      if (idx >= 0 && idx < s.hist_cap) s.hist_p[idx] = s.rNorm_lq;
    }
    s.nhist_p = k;
    s.norm_v = norm_next;
    const bool cg_point = s.transfer_to_bicg && (fabs(s.dbar) > epsM);
    if (cg_point) {
      s.zbar = s.eta / s.dbar;
      const double rho = s.beta_next * (s.sn * s.zeta_m1 - s.cs * s.zbar);
      s.rNorm_cg = fabs(rho) * norm_next;
    }
    s.solved_lq_tol = (s.rNorm_lq <= s.eps_L) ? 1 : 0;
    s.solved_lq_mach = (s.rNorm_lq + 1.0 <= 1.0) ? 1 : 0;
    s.solved_lq = (s.solved_lq_tol || s.solved_lq_mach) ? 1 : 0;
    s.solved_cg_tol = (cg_point && s.rNorm_cg <= s.eps_L) ? 1 : 0;
    s.solved_cg_mach = (cg_point && s.rNorm_cg + 1.0 <= 1.0) ? 1 : 0;
    s.solved_cg = (s.solved_cg_tol || s.solved_cg_mach) ? 1 : 0;
    s.solved_primal = (s.solved_lq || s.solved_cg) ? 1 : 0;
  }
  if (!s.solved_dual) {
    s.psibar_prev = s.psibar;
    s.tau = s.tau + s.uu;
    s.sNorm = fabs(s.psibar) * sqrt(s.tau);
    if (s.hist_d) {
      const long long idx = k - 1 - s.hist_base;
      if (idx >= 0 && idx < s.hist_cap) s.hist_d[idx] = s.sNorm;
    }
    s.nhist_d = k;
    s.solved_qr_tol = (s.sNorm <= s.eps_Q) ? 1 : 0;
    s.solved_qr_mach = (s.sNorm + 1.0 <= 1.0) ? 1 : 0;
    s.solved_dual = (s.solved_qr_tol || s.solved_qr_mach) ? 1 : 0;
  }
  s.uu = uu_next;
  if (k >= 3) s.eps3 = s.epsilon;
  if (k >= 2) s.lambda2 = s.lambda;
  s.dbar_prev = s.dbar;
  s.cs_prev = s.cs;
  s.sn_prev = s.sn;
  s.gamma = s.gamma_next;
  s.beta = s.beta_next;
  s.breakdown = (!s.solved_lq && !s.solved_cg && s.pq == 0.0) ? 1 : 0;
  s.iter = k;
  return (s.solved_primal && s.solved_dual) || s.breakdown;
}

// cgs! (src/cgs.jl:126-281), real Float64: the two scalars of the recurrence and the stopping tests.  As for qmr!: the same two steps
// run on the host (loops 0 and 1) and as the epilogues of the two reductions of an iteration (device-resident loop), so loops 1 and 2
// produce the same bits.
struct CgsDevState {
  double rho;          // ρₖ = ⟨r̅₀, rₖ⟩                                  (:185, :238)
  double alpha;        // αₖ = ρₖ / σₖ: P1 and P2                        (:221)
  double beta;         // βₖ = ρₖ₊₁ / ρₖ: P3                             (:231)
  double rNorm;        // ‖rₖ‖                                          (:244)
  double eps_tol;      // ε = atol + rtol ‖r₀‖                          (:199)
  long long stop_seq, iter, hist_base, hist_cap;
  double *hist;        // device history window (null: no history)
  int solved, breakdown;
};

// after σₖ = ⟨r̅₀, M⁻¹AN⁻¹pₖ⟩ (:220-221)
__host__ __device__ inline void cgs_step_a(CgsDevState &s, double sigma) { s.alpha = s.rho / sigma; }

// after ρₖ₊₁ = ⟨r̅₀, rₖ₊₁⟩ and ‖rₖ₊₁‖² (:230-231, :238-256): β, ρ, the history entry and the tests in the reference's order; true when
// the loop stops (tired / overtimed / the callback are the driver's).  The u and p updates of this iteration (:232-235) still run.
__host__ __device__ inline bool cgs_step_b(CgsDevState &s, double rho_next, double rr, long long k) {
  s.beta = rho_next / s.rho;
  s.rho = rho_next;
  s.rNorm = sqrt(rr);
  if (s.hist) {
    const long long idx = k - 1 - s.hist_base;
    if (idx >= 0 && idx < s.hist_cap) s.hist[idx] = s.rNorm;
  }
  const bool resid_decrease_mach = (s.rNorm + 1.0 <= 1.0);
  const bool resid_decrease_lim = (s.rNorm <= s.eps_tol);
  s.solved = (resid_decrease_lim || resid_decrease_mach) ? 1 : 0;
  s.breakdown = (s.alpha == 0.0 || s.alpha != s.alpha) ? 1 : 0;
  s.iter = k;
  return s.solved || s.breakdown;
}

// symmlq! (src/symmlq.jl:132-464), real Float64: the Lanczos scalars, the QR recurrences of Tₖ (and of Tₖ - λest I), the residual
// and error estimates of the LQ and CG points, the norm estimates and the stopping tests.  As for cgs!: the same steps run on the host
// (loops 0 and 1) and as the epilogues of the two reductions of an iteration (device-resident loop), so loops 1 and 2 produce the same
// bits.  Field names follow the reference; NaN stands for its `missing`.
struct SymmlqDevState {
  // coefficients the vector kernels read
  double inv_beta;               // one(T) / β: kdiv!(v, β) carried into the next P1                 (:309)
  double cz, sz, neg_c, sn;      // cζ, sζ, -c, s: the x and w̅ updates of P1                        (:292-295)
  double alpha, beta;            // α (λ included) and β: P2 reads -α and -oldβ = -β                 (:300-303)
  // constants of the solve
  double lambda, lambda_est;     // λ, λest
  double beta1, tol, etol, ctol; // β₁, atol + rtol β₁, etol, 1 / conlim                            (:163, :272)
  // the rotation of the iteration that runs (symmlq_rotation) and the recurrences
  double c, s, gamma, zeta;      // c, s, γ, ζ                                                       (:287-291)
  double gbar, dbar;             // γbar, δbar
  double eps_old, zeta_old, c_old;   // ϵold, ζold, cold
  double eta, zbar;              // η, ζbar
  double ANorm2, ANorm, Acond, gmax, gmin, xNorm, xcgNorm, rNorm, rcgNorm, test1;
  double err, errcg;             // Inf without λest
  double rhobar, sigbar, rho, cwold, cw, sw;   // the QR factorisation of Tₖ - λest I             (:251-256, :387-394)
  double hist_rcg, hist_errcg;   // what this iteration pushes to residualscg / errorscg: NaN where the reference pushes missing
  long long stop_seq, iter, hist_base, hist_cap;
  double *hist, *hist_cg;        // device history windows of residuals and residualscg (null: no history)
  int transfer_to_cg, window;
  int solved, solved_lq, solved_cg, solved_mach, fwd_err, ill_cond_mach, ill_cond_lim, not_pd;
};

// the host arrays of the window code (:342-374), which runs with λest ≠ 0 only: the workspace's clist, zlist and sprod, and
// stats.errorscg as it stands before this iteration's push (null without history).  The device-resident loop passes none.
struct SymmlqWindow {
  double *clist, *zlist, *sprod, *errorscg;
};

// (c, s, γ) = sym_givens(γbar, β) ; ηold = η ; ζ = ηold / γ (:287-291) and the coefficients of P1.  Runs on the host before
// iteration 1 and at the end of symmlq_step_b of an iteration that does not stop: the next P1 finds them in the state.
__host__ __device__ inline void symmlq_rotation(SymmlqDevState &s) {
  sym_givens(s.gbar, s.beta, s.c, s.s, s.gamma);
  s.zeta = s.eta / s.gamma;
  s.cz = s.c * s.zeta;
  s.sz = s.s * s.zeta;
  s.neg_c = -s.c;
  s.sn = s.s;
  s.inv_beta = 1.0 / s.beta;
}

// after vᴴ A v (:300)
__host__ __device__ inline void symmlq_step_a(SymmlqDevState &st, double vAv) { st.alpha = vAv + st.lambda; }

// after β² = ⟨v, Mv⟩ of the next Lanczos vector (:306-308, :313-430); k = iter.  True when the loop stops (tired / overtimed / the
// callback are the driver's); not_pd is set when β² < 0 (M not positive definite).
__host__ __device__ inline bool symmlq_step_b(SymmlqDevState &st, double beta2, long long k, const SymmlqWindow &win) {
  const double oldbeta = st.beta, alpha = st.alpha, c = st.c, s = st.s, gamma = st.gamma, zeta = st.zeta;
  const double lest = st.lambda_est;
  if (beta2 < 0) { st.not_pd = 1; return true; }
  const double beta = sqrt(beta2);
  st.beta = beta;
  st.ANorm2 = st.ANorm2 + alpha * alpha + oldbeta * oldbeta + beta * beta;
  double psi = 0.0, omegabar = 0.0;
  if (lest != 0) {
    const double eta_w = -oldbeta * oldbeta * st.cwold / st.rhobar;
    const double omega = lest + eta_w;
    psi = c * st.dbar + s * omega;
    omegabar = s * st.dbar - c * omega;
  }
  const double delta = st.dbar * c + alpha * s;
  st.gbar = st.dbar * s - alpha * c;
  const double eps = beta * s;
  st.dbar = -beta * c;
  st.eta = -st.eps_old * st.zeta_old - delta * zeta;
  st.rNorm = sqrt(gamma * gamma * zeta * zeta + st.eps_old * st.eps_old * st.zeta_old * st.zeta_old);
  st.xNorm = st.xNorm + zeta * zeta;
  const double nan = __builtin_nan("");                                                       // the reference's missing
  const bool cg_point = st.gbar != 0;
  if (cg_point) {
    st.zbar = st.eta / st.gbar;
    st.rcgNorm = beta * fabs(s * zeta - c * st.zbar);
    st.xcgNorm = st.xNorm + st.zbar * st.zbar;
  }
  st.hist_rcg = cg_point ? st.rcgNorm : nan;
  if (st.hist) {
    const long long idx = k - 1 - st.hist_base;
    if (idx >= 0 && idx < st.hist_cap) { st.hist[idx] = st.rNorm; st.hist_cg[idx] = st.hist_rcg; }
  }
  const int window = st.window;
  if (window > 0 && lest != 0) {                                                              // :342-374
    if (k < window && window > 1)
      for (long long i = k; i < window; ++i) win.sprod[i] = s * win.sprod[i];
    long long ix = (k - 1) % window;
    win.clist[ix] = c;
    win.zlist[ix] = zeta;
    if (k >= window) {
      const long long jx = k % window;
      const double zetabark = win.zlist[jx] / win.clist[jx];
      if (cg_point) {
        double theta = 0.0;
        for (int i = 0; i < window; ++i) theta = theta + win.clist[i] * win.sprod[i] * win.zlist[i];
        theta = zetabark * fabs(theta) + fabs(zetabark * st.zbar * win.sprod[ix] * s) - zetabark * zetabark;
        if (win.errorscg) {
          const double e = win.errorscg[k - window];
          win.errorscg[k - window] = sqrt(fabs(e * e - 2 * theta));
        }
      } else if (win.errorscg) {
        win.errorscg[k - window] = nan;
      }
    }
    ix = k % window;
    if (k >= window && window > 1) {
      const double f = 1.0 / win.sprod[(ix + 1) % window];                                    // kdiv! = kscal!(one(T) / s)
      for (int i = 0; i < window; ++i) win.sprod[i] = f * win.sprod[i];
      win.sprod[ix] = win.sprod[(ix - 1 + window) % window] * s;
    }
  }
  if (lest != 0) {                                                                            // :376-395
    st.err = fabs((st.eps_old * st.zeta_old + psi * zeta) / omegabar);
    if (cg_point) st.errcg = sqrt(fabs(st.err * st.err - st.zbar * st.zbar));
    st.hist_errcg = cg_point ? st.errcg : nan;
    st.rhobar = st.sw * st.sigbar - st.cw * (alpha - lest);
    st.sigbar = -st.cw * beta;
    st.rho = sqrt(st.rhobar * st.rhobar + beta * beta);
    st.cwold = st.cw;
    st.cw = st.rhobar / st.rho;
    st.sw = beta / st.rho;
  }
  st.gmax = jl_max(st.gmax, gamma);
  st.gmin = jl_min(st.gmin, gamma);
  st.Acond = st.gmax / st.gmin;
  st.ANorm = sqrt(st.ANorm2);
  st.test1 = st.rNorm / (st.ANorm * st.xNorm);
  st.eps_old = eps;
  st.zeta_old = zeta;
  st.c_old = c;
  const bool resid_decrease_mach = (1.0 + st.rNorm <= 1.0);                                   // :414-430
  st.ill_cond_mach = (1.0 + 1.0 / st.Acond <= 1.0) ? 1 : 0;
  const bool zero_resid_mach = (1.0 + st.test1 <= 1.0);
  st.ill_cond_lim = (1.0 / st.Acond <= st.ctol) ? 1 : 0;
  const bool zero_resid_lim = (st.test1 <= st.tol);
  st.fwd_err = ((st.err <= st.etol) || (cg_point && st.errcg <= st.etol)) ? 1 : 0;
  st.solved_lq = (st.rNorm <= st.tol) ? 1 : 0;
  st.solved_cg = (st.transfer_to_cg && cg_point && st.rcgNorm <= st.tol) ? 1 : 0;
  const bool zero_resid = st.solved_lq || st.solved_cg;
  const bool ill_cond = st.ill_cond_mach || st.ill_cond_lim;
  st.solved = (st.solved_mach || zero_resid || zero_resid_mach || zero_resid_lim || st.fwd_err || resid_decrease_mach) ? 1 : 0;
  st.iter = k;
  const bool stop = st.solved || ill_cond;
  if (!stop) symmlq_rotation(st);
  return stop;
}

// minres_qlp! (src/minres_qlp.jl:131-538), real Float64, linesearch = false: the Lanczos scalars, the QR factorisation of Tₖ₊₁.ₖ, the LQ
// factorisation of Rₖ, the solve with Lₖ, the norm estimates and the stopping tests.  As for symmlq!: the same steps run on the host
// (loops 0 and 1) and as the epilogues of the three reductions of an iteration (device-resident loop), so loops 1 and 2 produce the
// same bits.  Field names follow the reference; the suffixes 1 and 2 stand for its subscripts k-1 and k-2.
struct MinresQlpDevState {
  // the Lanczos product's coefficients, contiguous: the sliced SpMV reads them as SpmvArgs::lz_coef[0..2]
  double lambda;                 // λ                                                               (:248)
  double one;                    // 1.0: the product is not divided here (multiplication by 1.0 is exact)
  double neg_beta;               // -βₖ                                                             (:252)
  // coefficients the vector kernels read
  double inv_beta;               // one(T) / βₖ: kdiv!(vₖ₊₁, βₖ₊₁) carried into the next P1          (:265)
  double cpt, spt, neg_cp, sp;   // cpₖ τₖ₋₂, spₖ τₖ₋₂, -cpₖ, spₖ: x and wₐᵤₓ in P1 (k ≥ 3), the two outputs of P2 at k = 2 (:417-430)
  double cp;                     // cpₖ                                                             (:419)
  double neg_alpha, cd, sd;      // -αₖ, cdₖ, sdₖ: P2                                               (:257, :433)
  // constants of the solve
  double eps_tol, atol, Artol, btol, kappa;   // ε, atol, Artol, eps^(3/4), κ                     (:206, :224, :450)
  int MisI;
  // recurrences
  double alpha, beta;            // αₖ; βₖ, after step B βₖ₊₁
  double gbar1, gamma1, lambar, lam;   // γbarₖ₋₁, γₖ₋₁, λbarₖ, λₖ
  double c2, c1, c, s2, s1, s;   // cₖ₋₂, cₖ₋₁, cₖ, sₖ₋₂, sₖ₋₁, sₖ
  double zbar;                   // ζbarₖ
  double xi1;                    // ξₖ₋₁
  double tau2, tau1, tau;        // τₖ₋₂, τₖ₋₁, τₖ
  double psibar2, mubis2, mubar1;   // ψbarₖ₋₂, μbisₖ₋₂, μbarₖ₋₁
  double mu2, mubis1, psi2, theta, mubar;   // μₖ₋₂, μbisₖ₋₁, ψₖ₋₂, θₖ, μbarₖ (of the iteration that runs)
  double ANorm2, ANorm, Acond, mumin, mumax, xNorm, rNorm, ArNorm, backward;
  long long stop_seq, iter, hist_base, hist_cap;
  double *hist_r, *hist_ar, *hist_acond;   // device history windows (null: no history)
  int solved, zero_resid, inconsistent, ill_cond_mach, breakdown, not_pd;
};

// What iteration k = s.iter + 1 ≥ 3 knows before its product: ϵₖ₋₂, γbarₖ₋₁ (:291-292), (cpₖ, spₖ, μₖ₋₂) (:370) and τₖ₋₂ (:400-401) depend
// on βₖ and on earlier scalars only; for k = 2, γbarₖ₋₁ = βₖ (:296).  Runs at the end of minres_qlp_step_b of an iteration that does
// not stop: the next P1 and the next product find their coefficients in the state.
__host__ __device__ inline void minres_qlp_ahead(MinresQlpDevState &s, long long k) {
  if (k >= 3) {
    const double eps2 = s.s2 * s.beta;
    s.gbar1 = -s.c2 * s.beta;
    double cp, sp;
    sym_givens(s.mubis2, eps2, cp, sp, s.mu2);
    s.cp = cp;
    s.sp = sp;
    s.neg_cp = -cp;
    s.tau2 = s.tau1;
    s.tau2 = s.tau2 * s.mubis2 / s.mu2;
    s.cpt = cp * s.tau2;
    s.spt = sp * s.tau2;
  } else if (k == 2) {
    s.gbar1 = s.beta;
  }
  s.inv_beta = 1.0 / s.beta;
  s.neg_beta = -s.beta;
}

// after αₖ = ⟨vₖ, p⟩ (:255, :287-302, and what of :358-382 needs αₖ only); k = iter
__host__ __device__ inline void minres_qlp_step_a(MinresQlpDevState &s, double alpha, long long k) {
  s.alpha = alpha;
  s.neg_alpha = -alpha;
  if (k >= 2) {
    s.gamma1 = s.c1 * s.gbar1 + s.s1 * alpha;
    s.lambar = s.s1 * s.gbar1 - s.c1 * alpha;
  } else {
    s.lambar = alpha;
  }
  if (k == 2) {
    double cp, sp;
    sym_givens(s.mubar1, s.gamma1, cp, sp, s.mubis1);
    s.cp = cp;
    s.sp = sp;
    s.neg_cp = -cp;
  } else if (k >= 3) {
    s.psi2 = s.cp * s.psibar2 + s.sp * s.gamma1;
    s.theta = s.sp * s.psibar2 - s.cp * s.gamma1;
    sym_givens(s.mubar1, s.theta, s.cd, s.sd, s.mubis1);
  }
}

// after βₖ₊₁² = ⟨vₖ₊₁, p⟩ and xNorm = ‖x‖ (:261-269, :333-405 but for step A's part, :442-504); k = iter.  True when the loop stops
// (tired / overtimed / the callback are the driver's); not_pd is set when β² < 0 (M not positive definite).
__host__ __device__ inline bool minres_qlp_step_b(MinresQlpDevState &st, double beta2, double xNorm, long long k) {
  const double epsM = 2.220446049250313e-16;
  if (beta2 < 0) { st.not_pd = 1; return true; }
  const double beta = st.beta, alpha = st.alpha;
  const double beta_next = sqrt(beta2);
  st.ANorm2 = st.ANorm2 + alpha * alpha + beta * beta + beta_next * beta_next;                // :269
  sym_givens(st.lambar, beta_next, st.c, st.s, st.lam);                                       // :333
  const double zeta = st.c * st.zbar;                                                         // :340-341
  const double zbar_next = st.s * st.zbar;
  double psibar1 = 0.0, rho2 = 0.0;
  if (k == 1) {                                                                               // :358-382
    st.mubar = st.lam;
  } else if (k == 2) {
    psibar1 = st.sp * st.lam;
    st.mubar = -st.cp * st.lam;
  } else {
    rho2 = st.sp * st.lam;
    const double eta = -st.cp * st.lam;
    psibar1 = st.sd * eta;
    st.mubar = -st.cd * eta;
  }
  double xi = 0.0;
  if (k == 1) {                                                                               // :392-405
    st.tau = zeta / st.mubar;
  } else if (k == 2) {
    st.tau1 = st.tau;
    st.tau1 = st.tau1 * st.mubar1 / st.mubis1;
    xi = zeta;
    st.tau = (xi - psibar1 * st.tau1) / st.mubar;
  } else {
    st.tau1 = (st.xi1 - st.psi2 * st.tau2) / st.mubis1;
    xi = zeta - rho2 * st.tau2;
    st.tau = (xi - psibar1 * st.tau1) / st.mubar;
  }
  st.rNorm = fabs(zbar_next);                                                                 // :444
  const double cb = st.c1 * beta_next;
  st.ArNorm = fabs(st.zbar) * sqrt(st.lambar * st.lambar + cb * cb);                          // :449
  if (k == 1) st.kappa = st.atol + st.Artol * st.ArNorm;
  st.ANorm = sqrt(st.ANorm2);                                                                 // :453-466
  const double abs_mubar = fabs(st.mubar);
  if (k == 1) {
    st.mumin = abs_mubar;
    st.mumax = abs_mubar;
  } else if (k == 2) {
    st.mumax = jl_max(jl_max(st.mumax, st.mubis1), abs_mubar);
    st.mumin = jl_min(jl_min(st.mumin, st.mubis1), abs_mubar);
  } else {
    st.mumax = jl_max(jl_max(jl_max(st.mumax, st.mu2), st.mubis1), abs_mubar);
    st.mumin = jl_min(jl_min(jl_min(st.mumin, st.mu2), st.mubis1), abs_mubar);
  }
  st.Acond = st.mumax / st.mumin;
  st.xNorm = xNorm;                                                                           // :468-469
  st.backward = st.rNorm / (st.ANorm * xNorm);
  if (st.hist_r) {
    const long long idx = k - 1 - st.hist_base;
    if (idx >= 0 && idx < st.hist_cap) { st.hist_r[idx] = st.rNorm; st.hist_ar[idx] = st.ArNorm; st.hist_acond[idx] = st.Acond; }
  }
  st.ill_cond_mach = (1.0 + 1.0 / st.Acond <= 1.0) ? 1 : 0;                                   // :474-488
  const bool resid_decrease_mach = (1.0 + st.rNorm <= 1.0);
  const bool zero_resid_mach = (1.0 + st.backward <= 1.0);
  const bool resid_decrease_lim = (st.rNorm <= st.eps_tol);
  const bool zero_resid_lim = st.MisI && (st.backward <= epsM);
  st.breakdown = (beta_next <= st.btol) ? 1 : 0;
  st.zero_resid = (zero_resid_mach || zero_resid_lim) ? 1 : 0;
  const bool resid_decrease = resid_decrease_mach || resid_decrease_lim;
  st.solved = (resid_decrease || st.zero_resid) ? 1 : 0;
  st.inconsistent = ((st.ArNorm <= st.kappa && abs_mubar <= st.Artol) || (st.breakdown && !st.solved)) ? 1 : 0;
  if (k >= 2) {                                                                               // :493-504
    st.s2 = st.s1;
    st.c2 = st.c1;
    st.xi1 = xi;
    st.mubis2 = st.mubis1;
    st.psibar2 = psibar1;
  }
  st.s1 = st.s;
  st.c1 = st.c;
  st.mubar1 = st.mubar;
  st.zbar = zbar_next;
  st.beta = beta_next;
  st.iter = k;
  const bool stop = st.solved || st.inconsistent || st.ill_cond_mach || st.breakdown;
  if (!stop) minres_qlp_ahead(st, k + 1);
  return stop;
}

// usymqr! (src/usymqr.jl:130-365), real Float64: the scalars of the orthogonal tridiagonalisation of Saunders, Simon and Yip, of the
// QR factorisation of Tₖ₊₁.ₖ, the two residual norms and the stopping tests.  As for qmr!: the same two steps run on the host (loops 0
// and 1) and as the epilogues of the two reductions of an iteration (device-resident loop), so loops 1 and 2 produce the same bits.
// The coefficients of the process that P1 and P2 (ssy.hpp) read: the leading part of the state of every solver built on it.
struct SsyCoef {
  double gamma, beta;            // γₖ, βₖ: P1                                   (src/usymqr.jl:215-216)
  double alpha;                  // αₖ: P2                                       (:219-222)
};

struct UsymqrDevState : SsyCoef {
  // coefficients the vector kernels read (γₖ, βₖ, αₖ: SsyCoef)
  double beta_next, gamma_next;  // βₖ₊₁, γₖ₊₁: the divisors of P3               (:224-225, :312-317)
  double neg_eps, neg_lambda;    // -ϵₖ₋₂, -λₖ₋₁: kscal! and the first kaxpy! of wₖ (:283, :289, :291)
  double delta, inv_delta;       // δₖ: kdivcopy!(w₁, u₁, δ₁) (:278); one(T) / δₖ: kdiv!(wₖ, δₖ) = kscal!(one(T) / δₖ) (:285, :293)
  double zeta;                   // ζₖ: x = x + ζₖ wₖ                             (:298)
  // constants of the solve
  double eps_tol, kappa;         // ε = atol + rtol ‖r₀‖ (:178); κ = atol + rtol ‖Aᴴr₀‖, known after iteration 1 (:336)
  double atol, rtol;
  // recurrences
  double c_km2, c_km1, s_km2, s_km1;   // cₖ₋₂, cₖ₋₁, sₖ₋₂, sₖ₋₁
  double epsilon, lambda;        // ϵₖ₋₂, λₖ₋₁
  double dbar;                   // δbarₖ
  double zbar;                   // ζbarₖ
  double rNorm, ArNorm;          // ‖rₖ‖, ‖Aᴴrₖ₋₁‖
  long long stop_seq, iter, hist_base, hist_cap;
  double *hist_r, *hist_ar;      // device history windows of residuals and Aresiduals (null: no history)
  int solved, inconsistent;
};

// after αₖ = ⟨vₖ, q⟩ (:219)
__host__ __device__ inline void usymqr_step_a(UsymqrDevState &s, double vq) { s.alpha = vq; }

// after ‖q‖² and ‖p‖²: βₖ₊₁, γₖ₊₁, the two previous reflections, the new one, ζₖ and ζbarₖ₊₁, the two residual norms, their history
// entries, κ at k = 1, the shifts and the tests (:224-339); k = iter.  True when the loop stops (tired / overtimed / the callback are
// the driver's).  P3 of this iteration still runs: the reference updates x, vₖ₊₁ and uₖ₊₁ before it tests.
__host__ __device__ inline bool usymqr_step_b(UsymqrDevState &s, double qq, double pp, long long k) {
  s.beta_next = sqrt(qq);
  s.gamma_next = sqrt(pp);
  double lbar = 0.0;             // λbarₖ₋₁
  if (k >= 3) {
    s.epsilon = s.s_km2 * s.gamma;
    lbar = -s.c_km2 * s.gamma;
  }
  if (k >= 2) {
    if (k == 2) lbar = s.gamma;
    s.lambda = s.c_km1 * lbar + s.s_km1 * s.alpha;
    s.dbar = s.s_km1 * lbar - s.c_km1 * s.alpha;
  } else {
    s.dbar = s.alpha;
  }
  double c, sn;
  sym_givens(s.dbar, s.beta_next, c, sn, s.delta);
  s.zeta = c * s.zbar;
  const double zbar_next = sn * s.zbar;
  s.rNorm = fabs(zbar_next);
  const double cg = s.c_km1 * s.gamma_next;                  // cₖ₋₁ of before the shift, γₖ₊₁ of this iteration (:305)
  s.ArNorm = fabs(s.zbar) * sqrt(s.dbar * s.dbar + cg * cg);
  if (s.hist_r) {
    const long long idx = k - 1 - s.hist_base;
    if (idx >= 0 && idx < s.hist_cap) { s.hist_r[idx] = s.rNorm; s.hist_ar[idx] = s.ArNorm; }
  }
  if (k == 1) s.kappa = s.atol + s.rtol * s.ArNorm;
  s.neg_eps = -s.epsilon;
  s.neg_lambda = -s.lambda;
  s.inv_delta = 1.0 / s.delta;
  if (k >= 2) {
    s.s_km2 = s.s_km1;
    s.c_km2 = s.c_km1;
  }
  s.s_km1 = sn;
  s.c_km1 = c;
  s.zbar = zbar_next;
  s.gamma = s.gamma_next;        // P3 divides by gamma_next and beta_next; the next P1 reads gamma and beta
  s.beta = s.beta_next;
  s.solved = (s.rNorm <= s.eps_tol) ? 1 : 0;
  s.inconsistent = (!s.solved && s.ArNorm <= s.kappa) ? 1 : 0;
  s.iter = k;
  return s.solved || s.inconsistent;
}

// usymlq! (src/usymlq.jl:124-366), real Float64: the same process, the LQ factorisation of Tₖ, the residual norms of the LQ and the
// USYMCG points and the stopping tests.  As for usymqr!: the same two steps run on the host (loops 0 and 1) and as the epilogues of
// the two reductions of an iteration (device-resident loop), so loops 1 and 2 produce the same bits.
struct UsymlqDevState : SsyCoef {
  // coefficients the vector kernels read (γₖ, βₖ, αₖ: SsyCoef)
  double beta_next, gamma_next;  // βₖ₊₁, γₖ₊₁: the divisors of P3               (src/usymlq.jl:221-222, :297-302)
  double zc, zs, neg_c, sn;      // ζₖ₋₁cₖ, ζₖ₋₁sₖ, -cₖ, sₖ: the x and d̅ updates (:285-290)
  // constants of the solve
  double eps_tol;                // ε = atol + rtol ‖r₀‖                          (:175)
  // recurrences
  double bNorm;                  // ‖r₀‖: rNorm_lq of iteration 1                 (:307)
  double cs, cs_prev, sn_prev;   // cₖ, cₖ₋₁, sₖ₋₁
  double delta, lambda, epsilon; // δₖ₋₁, λₖ₋₁, ϵₖ₋₂
  double dbar, dbar_prev;        // δbarₖ, δbarₖ₋₁
  double eta, eta_prev;          // ηₖ, ηₖ₋₁
  double zeta_m2, zeta_m1, zbar; // ζₖ₋₂, ζₖ₋₁, ζbarₖ
  double rNorm_lq, rNorm_cg;
  long long stop_seq, iter, hist_base, hist_cap;
  double *hist_r;                // device history window (null: no history)
  int transfer, solved_lq, solved_cg;   // transfer: transfer_to_usymcg
};

// after αₖ = ⟨vₖ, q⟩ (:216)
__host__ __device__ inline void usymlq_step_a(UsymlqDevState &s, double vq) { s.alpha = vq; }

// after ‖q‖² and ‖p‖²: βₖ₊₁, γₖ₊₁, the LQ update (:234-254), ζ and η (:258-274), rNorm_lq (:306-312) and its history entry, the
// USYMCG residual (:317-321), the shifts (:324-329) and the two tests (:333-334); k = iter.  True when the loop stops (tired /
// overtimed / the callback are the driver's).  P3 of this iteration still runs: the reference updates x, d̅, vₖ₊₁ and uₖ₊₁ before
// it tests.
__host__ __device__ inline bool usymlq_step_b(UsymlqDevState &s, double qq, double pp, long long k) {
  s.beta_next = sqrt(qq);
  s.gamma_next = sqrt(pp);
  if (k == 1) {
    s.dbar = s.alpha;
  } else if (k == 2) {
    sym_givens(s.dbar_prev, s.gamma, s.cs, s.sn, s.delta);
    s.lambda = s.cs * s.beta + s.sn * s.alpha;
    s.dbar = s.sn * s.beta - s.cs * s.alpha;
  } else {
    sym_givens(s.dbar_prev, s.gamma, s.cs, s.sn, s.delta);
    s.epsilon = s.sn_prev * s.beta;
    s.lambda = -s.cs_prev * s.cs * s.beta + s.sn * s.alpha;
    s.dbar = -s.cs_prev * s.sn * s.beta - s.cs * s.alpha;
  }
  if (k == 1) s.eta = s.beta;
  if (k == 2) {
    s.zeta_m1 = s.eta_prev / s.delta;
    s.eta = -s.lambda * s.zeta_m1;
  }
  if (k >= 3) {
    s.zeta_m2 = s.zeta_m1;
    s.zeta_m1 = s.eta_prev / s.delta;
    s.eta = -s.epsilon * s.zeta_m2 - s.lambda * s.zeta_m1;
  }
  s.zc = s.zeta_m1 * s.cs;
  s.zs = s.zeta_m1 * s.sn;
  s.neg_c = -s.cs;
  if (k == 1) {
    s.rNorm_lq = s.bNorm;
  } else {
    const double mu = s.beta * (s.sn_prev * s.zeta_m2 - s.cs_prev * s.cs * s.zeta_m1) + s.alpha * s.sn * s.zeta_m1;
    const double omega = s.beta_next * s.sn * s.zeta_m1;
    s.rNorm_lq = sqrt(mu * mu + omega * omega);
  }
  if (s.hist_r) {
    const long long idx = k - 1 - s.hist_base;
    if (idx >= 0 && idx < s.hist_cap) s.hist_r[idx] = s.rNorm_lq;
  }
  const bool cg_point = s.transfer && (fabs(s.dbar) > 2.220446049250313e-16);
  if (cg_point) {
    s.zbar = s.eta / s.dbar;
    const double rho = s.beta_next * (s.sn * s.zeta_m1 - s.cs * s.zbar);
    s.rNorm_cg = fabs(rho);
  }
  s.sn_prev = s.sn;
  s.cs_prev = s.cs;
  s.eta_prev = s.eta;
  s.gamma = s.gamma_next;        // P3 divides by gamma_next and beta_next; the next P1 reads gamma and beta
  s.beta = s.beta_next;
  s.dbar_prev = s.dbar;
  s.solved_lq = (s.rNorm_lq <= s.eps_tol) ? 1 : 0;
  s.solved_cg = (cg_point && s.rNorm_cg <= s.eps_tol) ? 1 : 0;
  s.iter = k;
  return s.solved_lq || s.solved_cg;
}

// trilqr! (src/trilqr.jl:115-460), real Float64: ONE orthogonal tridiagonalisation that advances the USYMLQ iterate of A x = b (with
// the transfer to the USYMCG point) and the USYMQR iterate of Aᴴ t = c.  As for usymlq!: the same two steps run on the host (loops 0
// and 1) and as the epilogues of the two reductions of an iteration (device-resident loop), so loops 1 and 2 produce the same bits.
// The primal block is frozen once solved_primal is set, the dual block once solved_dual is set; the LQ factorisation and the
// shifts go on.  Both tests belong to P2's epilogue, which runs BEFORE P3: primal_on / dual_on keep for P3 which sides were
// unsolved when the iteration began.
struct TrilqrDevState : SsyCoef {
  // coefficients the vector kernels read (γₖ, βₖ, αₖ: SsyCoef)
  double beta_next, gamma_next;  // βₖ₊₁, γₖ₊₁: the divisors of P3               (src/trilqr.jl:223-224, :392-397)
  double zc, zs, neg_c, sn;      // ζₖ₋₁cₖ, ζₖ₋₁sₖ, -cₖ, sₖ: the x and d̅ updates (:289-294)
  double neg_eps3, neg_lambda2;  // -ϵₖ₋₃, -λₖ₋₂: kscal! and the second kaxpy! of wₖ₋₁ (:347, :352, :355)
  double delta, inv_delta;       // δₖ₋₁: kdivcopy!(w₁, v₁, δ₁) (:341); one(T) / δₖ₋₁: kdiv! = kscal!(one(T) / δₖ₋₁) (:348, :356)
  double psi;                    // ψₖ₋₁: t = t + ψₖ₋₁ wₖ₋₁                       (:367)
  // constants of the solve
  double bNorm, eps_L, eps_Q;    // ‖r₀‖, εL = atol + rtol ‖r₀‖, εQ = atol + rtol ‖s₀‖ (:154, :165-166)
  double atol, rtol, xi;         // ξ = atol + rtol ‖A s₀‖, known after iteration 1 of an unsolved dual side (:381)
  // recurrences
  double cs, cs_prev, sn_prev;   // cₖ, cₖ₋₁, sₖ₋₁
  double lambda, epsilon;        // λₖ₋₁, ϵₖ₋₂
  double lambda2, eps3;          // λₖ₋₂, ϵₖ₋₃
  double dbar, dbar_prev;        // δbarₖ, δbarₖ₋₁
  double zeta_m1, zeta_m2, zbar; // ζₖ₋₁, ζₖ₋₂, ζbarₖ
  double eta;                    // ηₖ
  double psibar, psibar_prev;    // ψbarₖ, ψbarₖ₋₁
  double rNorm_lq, rNorm_cg, sNorm, AsNorm;
  long long stop_seq, iter, hist_base, hist_cap;
  long long nhist_p, nhist_d;    // the last iteration that pushed to the primal / dual history: each side stops when it is solved
  double *hist_p, *hist_d;       // device history windows (null: no history)
  int transfer;                  // transfer_to_usymcg
  int primal_on, dual_on;        // the sides that were unsolved when this iteration began: what P3 updates
  int solved_lq, solved_cg, solved_primal, solved_dual, inconsistent;
  int solved_lq_tol, solved_lq_mach, solved_cg_tol, solved_cg_mach, solved_qr_tol, solved_qr_mach;
};

// after αₖ = ⟨vₖ, q⟩ (:218)
__host__ __device__ inline void trilqr_step_a(TrilqrDevState &s, double vq) { s.alpha = vq; }

// after ‖q‖² and ‖p‖²: βₖ₊₁, γₖ₊₁ and the LQ update always (:223-255); ζ, η, the two residual norms and the tests of a primal side
// still unsolved (:257-324); ψ, ‖sₖ₋₁‖, ‖A sₖ₋₁‖, ξ at k = 1 and the tests of a dual side still unsolved (:326-386); the shifts always
// (:399-410); k = iter.  True when the loop stops (tired / overtimed / the callback are the driver's).  P3 of this iteration
// still runs: the reference updates x, d̅, wₖ₋₁, t, vₖ₊₁ and uₖ₊₁ before it tests.
__host__ __device__ inline bool trilqr_step_b(TrilqrDevState &s, double qq, double pp, long long k) {
  const double epsM = 2.220446049250313e-16;
  s.beta_next = sqrt(qq);
  s.gamma_next = sqrt(pp);
  if (k == 1) {
    s.dbar = s.alpha;
  } else if (k == 2) {
    sym_givens(s.dbar_prev, s.gamma, s.cs, s.sn, s.delta);
    s.lambda = s.cs * s.beta + s.sn * s.alpha;
    s.dbar = s.sn * s.beta - s.cs * s.alpha;
  } else {
    sym_givens(s.dbar_prev, s.gamma, s.cs, s.sn, s.delta);
    s.epsilon = s.sn_prev * s.beta;
    s.lambda = -s.cs_prev * s.cs * s.beta + s.sn * s.alpha;
    s.dbar = -s.cs_prev * s.sn * s.beta - s.cs * s.alpha;
  }
  s.primal_on = s.solved_primal ? 0 : 1;
  s.dual_on = s.solved_dual ? 0 : 1;
  if (s.primal_on) {
    if (k == 1) s.eta = s.beta;
    if (k == 2) {
      const double eta_prev = s.eta;
      s.zeta_m1 = eta_prev / s.delta;
      s.eta = -s.lambda * s.zeta_m1;
    }
    if (k >= 3) {
      s.zeta_m2 = s.zeta_m1;
      const double eta_prev = s.eta;
      s.zeta_m1 = eta_prev / s.delta;
      s.eta = -s.epsilon * s.zeta_m2 - s.lambda * s.zeta_m1;
    }
    s.zc = s.zeta_m1 * s.cs;
    s.zs = s.zeta_m1 * s.sn;
    s.neg_c = -s.cs;
    if (k == 1) {
      s.rNorm_lq = s.bNorm;
    } else {
      const double mu = s.beta * (s.sn_prev * s.zeta_m2 - s.cs_prev * s.cs * s.zeta_m1) + s.alpha * s.sn * s.zeta_m1;
      const double omega = s.beta_next * s.sn * s.zeta_m1;
      s.rNorm_lq = sqrt(mu * mu + omega * omega);
    }
    if (s.hist_p) {
      const long long idx = k - 1 - s.hist_base;
      if (idx >= 0 && idx < s.hist_cap) s.hist_p[idx] = s.rNorm_lq;
    }
    s.nhist_p = k;
    const bool cg_point = s.transfer && (fabs(s.dbar) > epsM);
    if (cg_point) {
      s.zbar = s.eta / s.dbar;
      const double rho = s.beta_next * (s.sn * s.zeta_m1 - s.cs * s.zbar);
      s.rNorm_cg = fabs(rho);
    }
    s.solved_lq_tol = (s.rNorm_lq <= s.eps_L) ? 1 : 0;
    s.solved_lq_mach = (s.rNorm_lq + 1.0 <= 1.0) ? 1 : 0;
    s.solved_lq = (s.solved_lq_tol || s.solved_lq_mach) ? 1 : 0;
    s.solved_cg_tol = (cg_point && s.rNorm_cg <= s.eps_L) ? 1 : 0;
    s.solved_cg_mach = (cg_point && s.rNorm_cg + 1.0 <= 1.0) ? 1 : 0;
    s.solved_cg = (s.solved_cg_tol || s.solved_cg_mach) ? 1 : 0;
    s.solved_primal = (s.solved_lq || s.solved_cg) ? 1 : 0;
  }
  if (s.dual_on) {
    if (k == 1) {
      s.psibar = s.gamma;
    } else {
      s.psi = s.cs * s.psibar_prev;
      s.psibar = s.sn * s.psibar_prev;
    }
    s.neg_eps3 = -s.eps3;
    s.neg_lambda2 = -s.lambda2;
    s.inv_delta = 1.0 / s.delta;
    s.psibar_prev = s.psibar;
    s.sNorm = fabs(s.psibar);
    if (s.hist_d) {
      const long long idx = k - 1 - s.hist_base;
      if (idx >= 0 && idx < s.hist_cap) s.hist_d[idx] = s.sNorm;
    }
    s.nhist_d = k;
    const double cb = s.cs * s.beta_next;
    s.AsNorm = fabs(s.psibar) * sqrt(s.dbar * s.dbar + cb * cb);
    if (k == 1) s.xi = s.atol + s.rtol * s.AsNorm;
    s.solved_qr_tol = (s.sNorm <= s.eps_Q) ? 1 : 0;
    s.solved_qr_mach = (s.sNorm + 1.0 <= 1.0) ? 1 : 0;
    s.inconsistent = (s.AsNorm <= s.xi) ? 1 : 0;
    s.solved_dual = (s.solved_qr_tol || s.solved_qr_mach || s.inconsistent) ? 1 : 0;
  }
  if (k >= 3) s.eps3 = s.epsilon;
  if (k >= 2) s.lambda2 = s.lambda;
  s.dbar_prev = s.dbar;
  s.cs_prev = s.cs;
  s.sn_prev = s.sn;
  s.gamma = s.gamma_next;        // P3 divides by gamma_next and beta_next; the next P1 reads gamma and beta
  s.beta = s.beta_next;
  s.iter = k;
  return s.solved_primal && s.solved_dual;
}

// tricg! (src/tricg.jl:149-484), real Float64, M = N = I: the Galerkin iterate of [τI A; Aᴴ νI] [x; y] = [b; c] on the same
// orthogonal tridiagonalisation, by an LDLᴴ factorisation of the projected 2k × 2k matrix.  As for its siblings, the same two
// steps run on the host (loops 0 and 1) and as the epilogues of the two reductions of an iteration (device-resident loop).
// Step A needs αₖ only and does the whole LDLᴴ and π update; step B needs the two norms.  P3 of an iteration runs AFTER its
// step B and reads σₖ, ηₖ, λₖ, δₖ, π₂ₖ₋₁, π₂ₖ, βₖ₊₁ and γₖ₊₁: step B leaves them alone, the next step A (after that P3) rewrites them.
struct TricgDevState : SsyCoef {
  // coefficients the vector kernels read (γₖ, βₖ, αₖ: SsyCoef)
  double beta_next, gamma_next;  // βₖ₊₁, γₖ₊₁                                      (src/tricg.jl:411-412)
  double inv_beta_next, inv_gamma_next;   // kdiv! = kscal!(one(T) / ·)             (:416, :424)
  double sigma, eta, lambda, delta;       // σₖ, ηₖ, λₖ, δₖ                          (:332-339)
  double neg_sigma, neg_delta;            // the coefficients as the primitives get them (:368, :387-392)
  double pi1, pi2;               // π₂ₖ₋₁, π₂ₖ                                      (:356-360)
  // constants of the solve
  double tau, nu;                // τ, ν after flip / spd / snd                    (:176-178)
  double eps_tol, btol;          // ε = atol + rtol ‖r₀‖ (:261), eps^(3/4) (:272)
  // recurrences
  double d1, d2;                 // d₂ₖ₋₁, d₂ₖ
  double d_m3, d_m2;             // d₂ₖ₋₃, d₂ₖ₋₂
  double pi_m3, pi_m2;           // π₂ₖ₋₃, π₂ₖ₋₂
  double delta_prev;             // δₖ₋₁
  double rNorm;
  long long stop_seq, iter, hist_base, hist_cap;
  double *hist;                  // device history window (null: no history)
  int solved, breakdown;
};

// after αₖ = ⟨vₖ, q⟩ (:298): the LDLᴴ factorisation (:330-341) and π₂ₖ₋₁, π₂ₖ (:355-361); k = iter + 1.  τ = 0 or ν = 0 divides as
// the reference divides.
__host__ __device__ inline void tricg_step_a(TricgDevState &s, double vq) {
  s.alpha = vq;
  if (s.iter == 0) {
    s.d1 = s.tau;
    s.delta = s.alpha / s.d1;
    s.d2 = s.nu - (s.delta * s.delta) * s.d1;
    s.pi1 = s.beta / s.d1;
    s.pi2 = (s.gamma - s.delta * s.beta) / s.d2;
  } else {
    s.sigma = s.beta / s.d_m2;
    s.eta = s.gamma / s.d_m3;
    s.lambda = -(s.eta * s.delta_prev * s.d_m3) / s.d_m2;
    s.d1 = s.tau - (s.sigma * s.sigma) * s.d_m2;
    s.delta = (s.alpha - s.lambda * s.sigma * s.d_m2) / s.d1;
    s.d2 = s.nu - (s.eta * s.eta) * s.d_m3 - (s.lambda * s.lambda) * s.d_m2 - (s.delta * s.delta) * s.d1;
    s.pi1 = -(s.sigma * s.d_m2 * s.pi_m2) / s.d1;
    s.pi2 = -(s.delta * s.d1 * s.pi1 + s.lambda * s.d_m2 * s.pi_m2 + s.eta * s.d_m3 * s.pi_m3) / s.d2;
  }
  s.neg_sigma = -s.sigma;
  s.neg_delta = -s.delta;
}

// after ‖q‖² and ‖p‖²: βₖ₊₁, γₖ₊₁ (:411-412), ζ₂ₖ₋₁, ‖rₖ‖ (:435-438), the shift of the "previous" scalars (:441-447) and the tests
// (:451-457); k = iter.  True when the loop stops (tired / overtimed / the callback are the driver's).  P3 of this iteration
// still runs: the reference updates the g, x, y, vₖ₊₁ and uₖ₊₁ before it tests.
__host__ __device__ inline bool tricg_step_b(TricgDevState &s, double qq, double pp, long long k) {
  s.beta_next = sqrt(qq);
  s.gamma_next = sqrt(pp);
  s.inv_beta_next = 1.0 / s.beta_next;
  s.inv_gamma_next = 1.0 / s.gamma_next;
  const double zeta1 = s.pi1 - s.delta * s.pi2;
  const double gz = s.gamma_next * zeta1, bz = s.beta_next * s.pi2;
  s.rNorm = sqrt(gz * gz + bz * bz);
  if (s.hist) {
    const long long idx = k - 1 - s.hist_base;
    if (idx >= 0 && idx < s.hist_cap) s.hist[idx] = s.rNorm;
  }
  s.beta = s.beta_next;          // P3 reads beta_next and gamma_next; the next P1 reads beta and gamma
  s.gamma = s.gamma_next;
  s.pi_m3 = s.pi1;
  s.pi_m2 = s.pi2;
  s.d_m3 = s.d1;
  s.d_m2 = s.d2;
  s.delta_prev = s.delta;
  s.breakdown = (s.beta_next <= s.btol && s.gamma_next <= s.btol) ? 1 : 0;
  s.solved = (s.rNorm <= s.eps_tol || s.rNorm + 1.0 <= 1.0) ? 1 : 0;
  s.iter = k;
  return s.solved || s.breakdown;
}

// trimr! (src/trimr.jl:150-577), real Float64, M = N = I: the minimal-residual iterate of [τI A; Aᴴ νI] [x; y] = [b; c] on the same
// orthogonal tridiagonalisation, by a QR factorisation of the projected (2k + 2) × 2k matrix: four reflections per iteration.  τ and
// ν are never divided by, so ν = 0 (saddle-point systems) and τ = ν = 0 (adjoint systems) are ordinary solves.  As for its siblings,
// the same two steps run on the host (loops 0 and 1) and as the epilogues of the two reductions of an iteration.
// Step A only stores αₖ: the QR update needs βₖ₊₁ and γₖ₊₁, which exist after P2.  Step B does all the rest.  P3 of iteration k runs
// AFTER its step B and reads the twelve coefficients of the two rows of Rₖ that end in δ₂ₖ₋₁ and δ₂ₖ, π₂ₖ₋₁, π₂ₖ, βₖ₊₁ and γₖ₊₁ (at k = 1
// also −σ₁ / δ₂): step B publishes them in fields of their own (row1, row2, …), apart from the carries its shift has already moved
// on for k + 1; step B of k + 1 runs after P3 of k on the stream, so nothing overwrites them early.
struct TrimrRow {
  double mu, lambda, eta, sigma, delta;   // row one: μ₂ₖ₋₅, λ₂ₖ₋₄, η₂ₖ₋₃, σ₂ₖ₋₂, δ₂ₖ₋₁ ; row two: μ₂ₖ₋₄, λ₂ₖ₋₃, η₂ₖ₋₂, σ₂ₖ₋₁, δ₂ₖ
};
struct TrimrDevState : SsyCoef {
  // coefficients the vector kernels read (γₖ, βₖ, αₖ: SsyCoef)
  double beta_next, gamma_next;  // βₖ₊₁, γₖ₊₁                                      (src/trimr.jl:321-322)
  double inv_beta_next, inv_gamma_next;   // kdiv! = kscal!(one(T) / ·)             (:326, :334)
  TrimrRow row1, row2;           // what the g of iteration k are solved from       (:449-476)
  double first_scale;            // −σ₁ / δ₂, k = 1 only                            (:450)
  double pi1, pi2;               // π₂ₖ₋₁, π₂ₖ                                      (:485, :491)
  // constants of the solve
  double tau, nu;                // τ, ν after flip / spd / snd / sp               (:180-183)
  double eps_tol, btol;          // ε = atol + rtol ‖r₀‖ (:271), eps^(3/4) (:284)
  // carries
  double old_c1, old_c2, old_c3, old_c4, old_s1, old_s2, old_s3, old_s4;            // :519-526
  double sigmabar_m2, etabar_m3, lambdabar_m3;   // σbar₂ₖ₋₂, ηbar₂ₖ₋₃, λbar₂ₖ₋₃         (:531-533)
  double mu_m5, mu_m4, lambda_m4;         // μ₂ₖ₋₅, μ₂ₖ₋₄, λ₂ₖ₋₄ (shifted from k = 2 on)  (:534-538)
  double pibar1, pibar2;         // πbar₂ₖ₋₁, πbar₂ₖ                                 (:539-540)
  double rNorm;
  long long stop_seq, iter, hist_base, hist_cap;
  double *hist;                  // device history window (null: no history)
  int solved, breakdown;
};

// after αₖ = ⟨vₖ, q⟩ (:312): nothing else can be done before the norms
__host__ __device__ inline void trimr_step_a(TrimrDevState &s, double vq) { s.alpha = vq; }

// after ‖q‖² and ‖p‖²: βₖ₊₁, γₖ₊₁ (:321-322), the four previous reflections (:353-415), the four new ones (:421-443), the π update
// (:482-492), ‖rₖ‖ (:503), the shifts (:519-540) and the tests (:544-551); k = iter.  True when the loop stops (tired / overtimed / the
// callback are the driver's).  P3 of this iteration still runs: the reference updates the g, x, y, vₖ₊₁ and uₖ₊₁ before it tests.
// Every operation in the reference's order; the build has -ffp-contract=off.
__host__ __device__ inline bool trimr_step_b(TrimrDevState &s, double qq, double pp, long long k) {
  s.beta_next = sqrt(qq);
  s.gamma_next = sqrt(pp);
  s.inv_beta_next = 1.0 / s.beta_next;
  s.inv_gamma_next = 1.0 / s.gamma_next;
  const double alpha = s.alpha, beta_next = s.beta_next, gamma_next = s.gamma_next, tau = s.tau, nu = s.nu;
  double thetabar, deltabar1, deltabar2, sigmabar1, sigmabar2, lambdabar1, etabar1;
  double eta_m3 = 0.0, lambda_m3 = 0.0, mu_m3 = 0.0, sigma_m2 = 0.0, eta_m2 = 0.0, lambda_m2 = 0.0, mu_m2 = 0.0;
  if (k == 1) {
    thetabar = alpha;
    deltabar1 = tau;
    deltabar2 = nu;
    sigmabar1 = alpha;
    sigmabar2 = beta_next;
    lambdabar1 = gamma_next;
    etabar1 = 0.0;
  } else {
    const double sigmabis_m2 = s.old_c1 * s.sigmabar_m2 + s.old_s1 * alpha;
    const double etabis_m2 = s.old_s1 * nu;
    const double lambdabis_m2 = s.old_s1 * beta_next;
    const double thetabis = s.old_s1 * s.sigmabar_m2 - s.old_c1 * alpha;
    const double deltabis2 = -s.old_c1 * nu;
    const double sigmabis2 = -s.old_c1 * beta_next;
    eta_m3 = s.old_c2 * s.etabar_m3 + s.old_s2 * sigmabis_m2;
    lambda_m3 = s.old_c2 * s.lambdabar_m3 + s.old_s2 * etabis_m2;
    mu_m3 = s.old_s2 * lambdabis_m2;
    const double sigmahat_m2 = s.old_s2 * s.etabar_m3 - s.old_c2 * sigmabis_m2;
    const double etahat_m2 = s.old_s2 * s.lambdabar_m3 - s.old_c2 * etabis_m2;
    const double lambdahat_m2 = -s.old_c2 * lambdabis_m2;
    const double sigmatmp_m2 = s.old_c3 * sigmahat_m2 + s.old_s3 * thetabis;
    const double etatmp_m2 = s.old_c3 * etahat_m2 + s.old_s3 * deltabis2;
    const double lambdatmp_m2 = s.old_c3 * lambdahat_m2 + s.old_s3 * sigmabis2;
    thetabar = s.old_s3 * sigmahat_m2 - s.old_c3 * thetabis;
    deltabar2 = s.old_s3 * etahat_m2 - s.old_c3 * deltabis2;
    sigmabar2 = s.old_s3 * lambdahat_m2 - s.old_c3 * sigmabis2;
    sigma_m2 = s.old_c4 * sigmatmp_m2 + s.old_s4 * tau;
    eta_m2 = s.old_c4 * etatmp_m2 + s.old_s4 * alpha;
    lambda_m2 = s.old_c4 * lambdatmp_m2;
    mu_m2 = s.old_s4 * gamma_next;
    deltabar1 = s.old_s4 * sigmatmp_m2 - s.old_c4 * tau;
    sigmabar1 = s.old_s4 * etatmp_m2 - s.old_c4 * alpha;
    etabar1 = s.old_s4 * lambdatmp_m2;
    lambdabar1 = -s.old_c4 * gamma_next;
  }
  double c1, s1, theta, c2, s2, delta1, c3, s3, deltahat2, c4, s4, delta2;
  sym_givens(thetabar, gamma_next, c1, s1, theta);                      // :421-423
  const double g = s1 * deltabar2;
  deltabar2 = c1 * deltabar2;
  sym_givens(deltabar1, theta, c2, s2, delta1);                         // :429-431
  const double sigma1 = c2 * sigmabar1 + s2 * deltabar2;
  const double deltabis2 = s2 * sigmabar1 - c2 * deltabar2;
  sym_givens(deltabis2, g, c3, s3, deltahat2);                          // :437
  sym_givens(deltahat2, beta_next, c4, s4, delta2);                     // :443
  // what P3 of this iteration reads: the carries as they are BEFORE the shift below
  s.row1.mu = s.mu_m5;
  s.row1.lambda = s.lambda_m4;
  s.row1.eta = eta_m3;
  s.row1.sigma = sigma_m2;
  s.row1.delta = delta1;
  s.row2.mu = s.mu_m4;
  s.row2.lambda = lambda_m3;
  s.row2.eta = eta_m2;
  s.row2.sigma = sigma1;
  s.row2.delta = delta2;
  s.first_scale = -sigma1 / delta2;                                     // :450
  const double pibis2 = c1 * s.pibar2;                                  // :482-492
  const double pibis4 = s1 * s.pibar2;
  s.pi1 = c2 * s.pibar1 + s2 * pibis2;
  const double pihat2 = s2 * s.pibar1 - c2 * pibis2;
  const double pitmp2 = c3 * pihat2 + s3 * pibis4;
  const double pibar4 = s3 * pihat2 - c3 * pibis4;
  s.pi2 = c4 * pitmp2;
  const double pibar3 = s4 * pitmp2;
  s.rNorm = sqrt(pibar3 * pibar3 + pibar4 * pibar4);                    // :503
  if (s.hist) {
    const long long idx = k - 1 - s.hist_base;
    if (idx >= 0 && idx < s.hist_cap) s.hist[idx] = s.rNorm;
  }
  s.old_s1 = s1;                                                        // :519-526
  s.old_s2 = s2;
  s.old_s3 = s3;
  s.old_s4 = s4;
  s.old_c1 = c1;
  s.old_c2 = c2;
  s.old_c3 = c3;
  s.old_c4 = c4;
  s.beta = beta_next;            // P3 reads beta_next and gamma_next; the next P1 reads beta and gamma      (:529-530)
  s.gamma = gamma_next;
  s.sigmabar_m2 = sigmabar2;                                            // :531-533
  s.etabar_m3 = etabar1;
  s.lambdabar_m3 = lambdabar1;
  if (k >= 2) {                                                         // :534-538
    s.mu_m5 = mu_m3;
    s.mu_m4 = mu_m2;
    s.lambda_m4 = lambda_m2;
  }
  s.pibar1 = pibar3;                                                    // :539-540
  s.pibar2 = pibar4;
  s.breakdown = (beta_next <= s.btol && gamma_next <= s.btol) ? 1 : 0;  // :549
  s.solved = (s.rNorm <= s.eps_tol || s.rNorm + 1.0 <= 1.0) ? 1 : 0;    // :544-550
  s.iter = k;
  return s.solved || s.breakdown;
}

// usymlqr! (src/usymlqr.jl:136-509), real Float64: [I A; Aᴴ 0] [x; y] = [b; c] as the sum of the least-squares problem [b; 0]
// (USYMQR: y and the residual r) and the least-norm problem [0; c] (USYMLQ: x and z), both on ONE orthogonal tridiagonalisation and
// ONE QR factorisation of Tₖ₊₁.ₖ.  As for its siblings, the same two steps run on the host (loops 0 and 1) and as the epilogues of
// the two reductions of an iteration.  Each side is frozen once it is solved; the factorisation, wₖ and the shifts go on.  Both
// tests belong to P2's epilogue, which runs BEFORE P3: do_ls / do_ln keep for P3 which sides were active when the iteration began.
struct UsymlqrDevState : SsyCoef {
  // coefficients the vector kernels read (γₖ, βₖ, αₖ: SsyCoef)
  double beta_next, gamma_next;  // βₖ₊₁, γₖ₊₁: the divisors of P3               (src/usymlqr.jl:270-271, :441-455)
  double neg_eps, neg_lambda;    // -ϵₖ₋₂, -λₖ₋₁: kscal! and the first kaxpy! of wₖ (:321, :327, :329)
  double delta, inv_delta;       // δₖ: kdivcopy!(w₁, u₁, δ₁) (:316); one(T) / δₖ: kdiv!(wₖ, δₖ) = kscal!(one(T) / δₖ) (:323, :331)
  double phi;                    // ϕₖ: y = y + ϕₖ wₖ                             (:345)
  double r_coef, s2;             // -cₖ ϕbarₖ₊₁ / βₖ₊₁ and |sₖ|²: the kaxpby! of r   (:350)
  double zc, zs, neg_zeta;       // ζₖ₋₁cₖ₋₁, ζₖ₋₁sₖ₋₁, -ζₖ₋₁: the x and z updates   (:410-415)
  double neg_c, sn;              // -cₖ₋₁, sₖ₋₁: the kaxpby! of d̅                 (:419)
  // constants of the solve
  double eps_ls, eps_ln;         // ε_ls = atol + rtol β₁, ε_ln = atol + rtol γ₁ (:227-228)
  double kappa, atol, rtol;      // κ = atol + rtol ‖Aᴴr₀‖, known after iteration 1 of an active least-squares side (:365)
  double cNorm;                  // γ₁: rNorm_ln of iteration 1                  (:425)
  // recurrences
  double c_km2, c_km1, s_km2, s_km1;   // cₖ₋₂, cₖ₋₁, sₖ₋₂, sₖ₋₁
  double epsilon, lambda;        // ϵₖ₋₂, λₖ₋₁
  double dbar;                   // δbarₖ
  double delta_km1;              // δₖ₋₁
  double phibar;                 // ϕbarₖ
  double zeta_m2, zeta_m1;       // ζₖ₋₂, ζₖ₋₁
  double eta_prev;               // ηₖ₋₁
  double rNorm_ls, rNorm_ln, ArNorm;
  long long stop_seq, iter, hist_base, hist_cap;
  long long nhist_ls, nhist_ln;  // the last iteration that pushed to a side's history: each side stops when it is solved
  double *hist_ls, *hist_ln, *hist_ar;   // device history windows (null: no history); ‖Aᴴrₖ₋₁‖ follows the least-squares side
  int ls, ln;                    // the keyword arguments
  int do_ls, do_ln;              // the sides that were active when this iteration began: what P3 updates
  int solved_ls, solved_ln, inconsistent;
};

// after αₖ = ⟨vₖ, q⟩ (:260)
__host__ __device__ inline void usymlqr_step_a(UsymlqrDevState &s, double vq) { s.alpha = vq; }

// after ‖q‖² and ‖p‖²: βₖ₊₁, γₖ₊₁, the two previous reflections and the new one (:270-310) and the coefficients of wₖ always; ϕ, the
// r coefficient, the two norms, κ at k = 1 and the tests of an active least-squares side (:334-367); ζ, η, the residual norm and the
// test of an active least-norm side (:369-438); the shifts always (:462-471); k = iter.  True when the loop stops (tired /
// overtimed / the callback are the driver's).  P3 of this iteration still runs: the reference updates wₖ, y, r, x, z, d̅, vₖ₊₁ and
// uₖ₊₁ before it tests.  The r coefficient is formed as the reference writes it, (-cₖ ϕbarₖ₊₁) / βₖ₊₁: 0 / 0 when βₖ₊₁ = 0.
__host__ __device__ inline bool usymlqr_step_b(UsymlqrDevState &s, double qq, double pp, long long k) {
  s.beta_next = sqrt(qq);
  s.gamma_next = sqrt(pp);
  double lbar = 0.0;             // λbarₖ₋₁
  if (k >= 3) {
    s.epsilon = s.s_km2 * s.gamma;
    lbar = -s.c_km2 * s.gamma;
  }
  if (k >= 2) {
    if (k == 2) lbar = s.gamma;
    s.lambda = s.c_km1 * lbar + s.s_km1 * s.alpha;
    s.dbar = s.s_km1 * lbar - s.c_km1 * s.alpha;
  } else {
    s.dbar = s.alpha;
  }
  double c, sn;
  sym_givens(s.dbar, s.beta_next, c, sn, s.delta);
  s.neg_eps = -s.epsilon;
  s.neg_lambda = -s.lambda;
  s.inv_delta = 1.0 / s.delta;
  s.do_ls = (s.ls && !s.solved_ls) ? 1 : 0;
  s.do_ln = (s.ln && !s.solved_ln) ? 1 : 0;
  if (s.do_ls) {
    s.phi = c * s.phibar;
    const double phibar_next = sn * s.phibar;
    s.r_coef = -c * phibar_next / s.beta_next;
    s.s2 = sn * sn;
    s.rNorm_ls = fabs(phibar_next);
    const double cg = s.c_km1 * s.gamma_next;                  // cₖ₋₁ of before the shift, γₖ₊₁ of this iteration (:357)
    s.ArNorm = fabs(s.phibar) * sqrt(s.dbar * s.dbar + cg * cg);
    if (s.hist_ls) {
      const long long idx = k - 1 - s.hist_base;
      if (idx >= 0 && idx < s.hist_cap) { s.hist_ls[idx] = s.rNorm_ls; s.hist_ar[idx] = s.ArNorm; }
    }
    s.nhist_ls = k;
    s.phibar = phibar_next;
    s.solved_ls = (s.rNorm_ls <= s.eps_ls) ? 1 : 0;
    if (k == 1) s.kappa = s.atol + s.rtol * s.ArNorm;
    s.inconsistent = (!s.solved_ls && s.ArNorm <= s.kappa) ? 1 : 0;
  }
  if (s.do_ln) {
    double eta = 0.0;            // ηₖ
    if (k == 1) eta = s.gamma;
    if (k == 2) {
      s.zeta_m1 = s.eta_prev / s.delta_km1;
      eta = -s.lambda * s.zeta_m1;
    }
    if (k >= 3) {
      s.zeta_m2 = s.zeta_m1;
      s.zeta_m1 = s.eta_prev / s.delta_km1;
      eta = -s.epsilon * s.zeta_m2 - s.lambda * s.zeta_m1;
    }
    s.zc = s.zeta_m1 * s.c_km1;
    s.zs = s.zeta_m1 * s.s_km1;
    s.neg_zeta = -s.zeta_m1;
    s.neg_c = -s.c_km1;
    s.sn = s.s_km1;
    if (k == 1) {
      s.rNorm_ln = s.cNorm;
    } else {
      const double mu = s.gamma * (s.s_km2 * s.zeta_m2 - s.c_km2 * s.c_km1 * s.zeta_m1) + s.alpha * s.s_km1 * s.zeta_m1;
      const double omega = s.gamma_next * s.s_km1 * s.zeta_m1;
      s.rNorm_ln = sqrt(mu * mu + omega * omega);
    }
    if (s.hist_ln) {
      const long long idx = k - 1 - s.hist_base;
      if (idx >= 0 && idx < s.hist_cap) s.hist_ln[idx] = s.rNorm_ln;
    }
    s.nhist_ln = k;
    s.eta_prev = eta;
    s.solved_ln = (s.rNorm_ln <= s.eps_ln) ? 1 : 0;
  }
  if (k >= 2) {
    s.s_km2 = s.s_km1;
    s.c_km2 = s.c_km1;
  }
  s.s_km1 = sn;
  s.c_km1 = c;
  s.delta_km1 = s.delta;
  s.gamma = s.gamma_next;        // P3 divides by gamma_next and beta_next; the next P1 reads gamma and beta
  s.beta = s.beta_next;
  s.iter = k;
  return (s.solved_ls && s.solved_ln) || s.inconsistent;
}

__device__ __forceinline__ bool seq_skip(const long long *stop_seq, long long seq) {
  return stop_seq != nullptr && seq >= *stop_seq;
}

// v = the finished reduction result(s); seq = sequence number of the kernel that produced it
__device__ inline void solver_epilogue(int epi, void *state, const double *v, long long seq) {
  if (epi == EPI_CG_STEP1) {                       // v[0] = p.Ap          src/cg.jl:197-213
    CgDevState *st = static_cast<CgDevState *>(state);
    const double pAp = v[0];
    st->pAp = pAp;
    if (pAp <= st->keps * st->pNorm2) {            // radius == 0, linesearch == false in this mode
      if (fabs(pAp) <= st->keps * st->pNorm2) {
        st->zero_curvature = 1;
        st->inconsistent = 1;
        st->stop_seq = seq + 1;                    // the rest of this iteration and everything after: no-ops
        return;
      }
    }
    st->alpha_prev = st->alpha;
    st->alpha = st->gamma / pAp;
  } else if (epi == EPI_CG_STEP2) {                // v[0] = r.r after r -= alpha Ap     src/cg.jl:242-262
    CgDevState *st = static_cast<CgDevState *>(state);
    const double gamma_next = v[0];
    if (!(gamma_next >= 0)) {
      st->not_spd = 1;
      st->stop_seq = seq + 1;
      return;
    }
    const double rNorm = sqrt(gamma_next);
    st->rNorm = rNorm;
    const long long k = st->iter + 1;
    if (st->hist) {
      const long long idx = k - 1 - st->hist_base;
      if (idx >= 0 && idx < st->hist_cap) st->hist[idx] = rNorm;
    }
    const bool solved = (rNorm <= st->eps_tol) || (rNorm + 1.0 <= 1.0);
    if (!solved) {
      const double beta = gamma_next / st->gamma;
      st->beta = beta;
      st->pNorm2 = gamma_next + beta * beta * st->pNorm2;
      st->gamma = gamma_next;
    }
    st->solved = solved ? 1 : 0;
    st->iter = k;
    if (solved) st->stop_seq = seq + 2;            // the x update of this iteration (seq + 1) still runs
  } else if (epi == EPI_CGCG) {                    // v = (r.w, r.r) with w = A r
    CgcgDevState *st = static_cast<CgcgDevState *>(state);
    const double delta = v[0], gamma_next = v[1];
    const double rNorm = sqrt(gamma_next);
    st->rNorm = rNorm;
    const long long k = st->iter + 1;
    if (st->hist) {
      const long long idx = k - 1 - st->hist_base;
      if (idx >= 0 && idx < st->hist_cap) st->hist[idx] = rNorm;
    }
    const bool solved = (rNorm <= st->eps_tol) || (rNorm + 1.0 <= 1.0);
    const double beta = gamma_next / st->gamma;
    const double denom = delta - beta * gamma_next / st->alpha;
    const bool breakdown = !solved && !(denom > 0.0);
    st->solved = solved ? 1 : 0;
    st->breakdown = breakdown ? 1 : 0;
    st->iter = k;
    if (solved || breakdown) { st->stop_seq = seq + 1; return; }     // x, r already hold iterate k
    st->beta = beta;
    st->alpha = gamma_next / denom;
    st->gamma = gamma_next;
  } else if (epi == EPI_MINRES_A) {               // v[0] = v.y                 src/minres.jl:287-291
    minres_step_a(*static_cast<MinresDevState *>(state), v[0]);
  } else if (epi == EPI_MINRES_B) {                // v[0] = y.y = beta^2        :305-336
    MinresDevState *st = static_cast<MinresDevState *>(state);
    if (!minres_step_b(*st, v[0], st->iter + 1)) st->stop_seq = seq + 1;
  } else if (epi == EPI_MINRES_C) {                // v[0] = x.x                 :348-451
    MinresDevState *st = static_cast<MinresDevState *>(state);
    if (minres_step_c(*st, sqrt(v[0]), st->iter + 1, st->err_vec)) st->stop_seq = seq + 1;
  } else if (epi == EPI_LZSHIFT_A) {               // v[0] = v.(A v)             src/cg_lanczos_shift.jl:200
    static_cast<LanczosShiftDevState *>(state)->delta = v[0];
  } else if (epi == EPI_LZSHIFT_B) {               // v[0] = w.w = β²            :208-252
    LanczosShiftDevState *st = static_cast<LanczosShiftDevState *>(state);
    const long long k = st->iter + 1;
    lzshift_beta(*st, v[0]);
    double *row = nullptr;
    if (st->hist) {
      const long long idx = k - 1 - st->hist_base;
      if (idx >= 0 && idx < st->hist_cap) row = st->hist + idx * st->nshifts;
    }
    if (lzshift_step(*st, lzshift_arrays(*st), k, row)) st->stop_seq = seq + 2;   // this iteration's P2 (seq + 1) still runs
  } else if (epi == EPI_BILQ_A) {                  // v[0] = u.q                 src/bilq.jl:247
    bilq_step_a(*static_cast<BilqDevState *>(state), v[0]);
  } else if (epi == EPI_BILQ_B) {                  // v[0] = p.q                 :252-305
    BilqDevState *st = static_cast<BilqDevState *>(state);
    bilq_step_b(*st, v[0], st->iter + 1);
  } else if (epi == EPI_BILQ_C) {                  // v = (v_k.v_k+1, v_k+1.v_k+1)   :334-371
    BilqDevState *st = static_cast<BilqDevState *>(state);
    if (bilq_step_c(*st, v[0], sqrt(v[1]), st->iter + 1)) st->stop_seq = seq + 1;
  } else if (epi == EPI_QMR_A) {                   // v[0] = u.q                 src/qmr.jl:251
    qmr_step_a(*static_cast<QmrDevState *>(state), v[0]);
  } else if (epi == EPI_QMR_B) {                   // v[0] = p.q                 :256-312
    QmrDevState *st = static_cast<QmrDevState *>(state);
    qmr_step_b(*st, v[0], st->iter + 1);
  } else if (epi == EPI_QMR_C) {                   // v[0] = v_k+1.v_k+1         :350-376
    QmrDevState *st = static_cast<QmrDevState *>(state);
    if (qmr_step_c(*st, v[0], st->iter + 1)) st->stop_seq = seq + 1;
  } else if (epi == EPI_BILQR_A) {                 // v[0] = u.q                 src/bilqr.jl:233
    bilqr_step_a(*static_cast<BilqrDevState *>(state), v[0]);
  } else if (epi == EPI_BILQR_B) {                 // v[0] = p.q                 :238-294, :350-359
    BilqrDevState *st = static_cast<BilqrDevState *>(state);
    bilqr_step_b(*st, v[0], st->iter + 1);
  } else if (epi == EPI_BILQR_C) {                 // v = (v_k.q, q.q, u_k+1.u_k+1, 0)   :313-347, :394-435
    BilqrDevState *st = static_cast<BilqrDevState *>(state);
    if (bilqr_step_c(*st, v[0], sqrt(v[1]), v[2], st->iter + 1)) st->stop_seq = seq + 1;
  } else if (epi == EPI_BICG_A) {                  // v[0] = c.v                 src/bicgstab.jl:223
    BicgDevState *st = static_cast<BicgDevState *>(state);
    st->alpha = st->rho / v[0];
  } else if (epi == EPI_BICG_B) {                  // v = (t.s, t.t)             :230
    BicgDevState *st = static_cast<BicgDevState *>(state);
    st->omega = v[0] / v[1];
  } else if (epi == EPI_BICG_C) {                  // v = (c.r, r.r)             :234-252
    BicgDevState *st = static_cast<BicgDevState *>(state);
    const double next_rho = v[0];
    st->beta = (next_rho / st->rho) * (st->alpha / st->omega);
    const double rNorm = sqrt(v[1]);
    st->rNorm = rNorm;
    const long long k = st->iter + 1;
    if (st->hist) {
      const long long idx = k - 1 - st->hist_base;
      if (idx >= 0 && idx < st->hist_cap) st->hist[idx] = rNorm;
    }
    const bool solved = (rNorm <= st->eps_tol) || (rNorm + 1.0 <= 1.0);
    const bool breakdown = (st->alpha == 0.0) || (st->alpha != st->alpha);
    st->solved = solved ? 1 : 0;
    st->breakdown = breakdown ? 1 : 0;
    st->rho = next_rho;
    st->iter = k;
    if (solved || breakdown) st->stop_seq = seq + 2;   // the p update of this iteration (seq + 1) still runs (:236-237)
  } else if (epi == EPI_CGS_A) {                   // v[0] = c.ts                src/cgs.jl:220-221
    cgs_step_a(*static_cast<CgsDevState *>(state), v[0]);
  } else if (epi == EPI_CGS_B) {                   // v = (c.r, r.r)             :230-256
    CgsDevState *st = static_cast<CgsDevState *>(state);
    if (cgs_step_b(*st, v[0], v[1], st->iter + 1)) st->stop_seq = seq + 2;   // P3 of this iteration (seq + 1) still runs (:232-235)
  } else if (epi == EPI_SYMMLQ_A) {                // v[0] = v.(A v)             src/symmlq.jl:300
    symmlq_step_a(*static_cast<SymmlqDevState *>(state), v[0]);
  } else if (epi == EPI_SYMMLQ_B) {                // v[0] = Mv.Mv = β²          :306-430 (λest = 0 here: no window lists)
    SymmlqDevState *st = static_cast<SymmlqDevState *>(state);
    if (symmlq_step_b(*st, v[0], st->iter + 1, SymmlqWindow{nullptr, nullptr, nullptr, nullptr})) st->stop_seq = seq + 1;
  } else if (epi == EPI_MINRES_QLP_X) {            // v[0] = x.x                 src/minres_qlp.jl:468
    static_cast<MinresQlpDevState *>(state)->xNorm = sqrt(v[0]);
  } else if (epi == EPI_MINRES_QLP_A) {            // v[0] = ⟨vₖ, p⟩ = αₖ         :255, :287-302
    MinresQlpDevState *st = static_cast<MinresQlpDevState *>(state);
    minres_qlp_step_a(*st, v[0], st->iter + 1);
  } else if (epi == EPI_MINRES_QLP_B) {            // v[0] = p.p = βₖ₊₁²         :261-504
    MinresQlpDevState *st = static_cast<MinresQlpDevState *>(state);
    if (minres_qlp_step_b(*st, v[0], st->xNorm, st->iter + 1)) st->stop_seq = seq + 1;
  } else if (epi == EPI_USYMQR_A) {                // v[0] = v.q                 src/usymqr.jl:219
    usymqr_step_a(*static_cast<UsymqrDevState *>(state), v[0]);
  } else if (epi == EPI_USYMQR_B) {                // v = (q.q, p.p)             :224-339
    UsymqrDevState *st = static_cast<UsymqrDevState *>(state);
    if (usymqr_step_b(*st, v[0], v[1], st->iter + 1)) st->stop_seq = seq + 2;   // P3 of this iteration (seq + 1) still runs (:276-317)
  } else if (epi == EPI_USYMLQ_A) {                // v[0] = v.q                 src/usymlq.jl:216
    usymlq_step_a(*static_cast<UsymlqDevState *>(state), v[0]);
  } else if (epi == EPI_USYMLQ_B) {                // v = (q.q, p.p)             :221-334
    UsymlqDevState *st = static_cast<UsymlqDevState *>(state);
    if (usymlq_step_b(*st, v[0], v[1], st->iter + 1)) st->stop_seq = seq + 2;   // P3 of this iteration (seq + 1) still runs (:279-302)
  } else if (epi == EPI_TRILQR_A) {                // v[0] = v.q                 src/trilqr.jl:218
    trilqr_step_a(*static_cast<TrilqrDevState *>(state), v[0]);
  } else if (epi == EPI_TRILQR_B) {                // v = (q.q, p.p)             :223-410
    TrilqrDevState *st = static_cast<TrilqrDevState *>(state);
    if (trilqr_step_b(*st, v[0], v[1], st->iter + 1)) st->stop_seq = seq + 2;   // P3 of this iteration (seq + 1) still runs (:283-397)
  } else if (epi == EPI_TRICG_A) {                 // v[0] = v.q                 src/tricg.jl:298
    tricg_step_a(*static_cast<TricgDevState *>(state), v[0]);
  } else if (epi == EPI_TRICG_B) {                 // v = (q.q, p.p)             :411-457
    TricgDevState *st = static_cast<TricgDevState *>(state);
    if (tricg_step_b(*st, v[0], v[1], st->iter + 1)) st->stop_seq = seq + 2;    // P3 of this iteration (seq + 1) still runs (:364-432)
  } else if (epi == EPI_TRIMR_A) {                 // v[0] = v.q                 src/trimr.jl:312
    trimr_step_a(*static_cast<TrimrDevState *>(state), v[0]);
  } else if (epi == EPI_TRIMR_B) {                 // v = (q.q, p.p)             :321-551
    TrimrDevState *st = static_cast<TrimrDevState *>(state);
    if (trimr_step_b(*st, v[0], v[1], st->iter + 1)) st->stop_seq = seq + 2;    // P3 of this iteration (seq + 1) still runs (:446-516)
  } else if (epi == EPI_USYMLQR_A) {               // v[0] = v.q                 src/usymlqr.jl:260
    usymlqr_step_a(*static_cast<UsymlqrDevState *>(state), v[0]);
  } else if (epi == EPI_USYMLQR_B) {               // v = (q.q, p.p)             :270-471
    UsymlqrDevState *st = static_cast<UsymlqrDevState *>(state);
    if (usymlqr_step_b(*st, v[0], v[1], st->iter + 1)) st->stop_seq = seq + 2;  // P3 of this iteration (seq + 1) still runs (:312-455)
  }
}

}  // namespace khip
