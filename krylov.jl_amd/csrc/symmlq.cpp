// symmlq.cpp -- symmlq! (src/symmlq.jl:132-464) above the device primitives, with its fused gfx950 kernels.
//
// Real Float64.  Three loops, chosen as for cgs! (khip_symmlq_last_path):
//   0  options.fused = 0: the reference's primitive sequence, one launch per k* call, one host sync per kdotr;
//   1  the host-driven loop on the fused kernels (with M, a user operator, a callback, verbose > 0 or λest ≠ 0);
//   2  the device-resident loop (default; A a CSR handle, M = I, λest = 0): the Lanczos scalars, the QR recurrences and the stopping
//      tests run as the epilogues of the two reductions of an iteration (symmlq_step_a/b, solver_device.hpp), iterations are
//      enqueued ahead.
// λest ≠ 0 stays on loop 1: the window code (:342-374) rewrites errorscg[iter - window + 1] in retrospect, which does not fit device
// history windows that are emptied while the loop runs.  The window lists are never read with λest = 0, so no window size keeps a
// solve from loop 2.
// With M = I the reference aliases v = Mv and vold = Mvold.  One iteration on the fused paths:
//   P1   v = (1/β) v (off in iteration 1: the set-up normalised it, :207) ; x = fma(sζ, v, fma(cζ, w̅, x)) ;
//        w̅ = fma(-c, v, s w̅)                                                                  (:309, :292-295)      48n bytes
//   t = A v ; v.t                                the fused SpMV (spmv.hip)                     (:299-300)            -> α = v.t + λ
//   P2   t = fma(-α, v, fma(-oldβ, vold, t)) ; t.t                                             (:301-306)            32n bytes
// against 200n for the primitive sequence (10 BLAS-1 calls); kcopy!(Mvold, Mv) and kcopy!(Mv, Mv_next) become a rotation of the
// three buffers' roles, and kdiv!(v, β) is carried into the next P1: after the loop one kscal! brings Mv to the reference's state.
// Every elementwise value uses the expression of the primitive it replaces (fma(a, x, y) for kaxpy!, fma(a, x, b y) for kaxpby!,
// multiplication by one(T) / β for kdiv!): the fused loops agree with the primitive sequence bit for bit on elementwise values and
// to the reductions' one ulp otherwise; loops 1 and 2 run the same kernels and the same scalar code and produce the same bits.
#include "solver_host.hpp"
#include "vec_launch.hpp"

using namespace khip;

namespace khip {   // (named, not anonymous: stable kernel names in traces)

// ---------------------------------------------------------------------------------------------------------- kernels ----
// Each thread owns one VEC-vector of every stream; the odd tail element (VEC = 2, n odd) goes to thread 0 of block 0.
// Cache hints, the rule of qmr.cpp: a load is non-temporal when it is the LAST read of that data before it is overwritten; a store
// is non-temporal when nothing reads it before the next iteration's passes.  P1 reduces nothing: it has no COMP.

// P1: scale ? v = (1/β) v ; x = fma(sζ, v, fma(cζ, w̅, x)) ; w̅ = fma(-c, v, s w̅)          (:309 of the iteration before, :292-295)
//   v    load  cacheable: the product that follows and P2 read it.      store (scale) cacheable: the product reads it next.
//   x    load  NT: overwritten here.            store NT: next read by the next iteration's P1.
//   w̅    load  NT: overwritten here.            store NT: next read by the next iteration's P1.
template <int VEC, bool NT>
__global__ __launch_bounds__(kBlock) void symmlq_p1_kernel(int64_t n, const SymmlqDevState *st, const long long *stop_seq,
                                                          long long seq, double *v, double *x, double *wbar, int scale) {
  using T = typename VecT<VEC>::type;
  if (seq_skip(stop_seq, seq)) return;
  const double ib = st->inv_beta, cz = st->cz, sz = st->sz, nc = st->neg_c, sn = st->sn;
  const int64_t nvec = n / VEC;
  const int64_t i = lane_index();
  if (i < nvec) {
    const T vv = ldg<false>(reinterpret_cast<const T *>(v) + i);
    const T xv = ldg<NT>(reinterpret_cast<const T *>(x) + i);
    const T wv = ldg<NT>(reinterpret_cast<const T *>(wbar) + i);
    T vo, xo, wo;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const double vn = scale ? ib * vget(vv, e) : vget(vv, e);     // kdiv!(v, β) = kscal!(one(T) / β)
      const double we = vget(wv, e);
      vset(vo, e, vn);
      vset(xo, e, fma(sz, vn, fma(cz, we, vget(xv, e))));           // kaxpy!(c ζ, w̅, x) ; kaxpy!(s ζ, v, x)
      vset(wo, e, fma(nc, vn, sn * we));                            // kaxpby!(-c, v, s, w̅)
    }
    if (scale) stg<false>(vo, reinterpret_cast<T *>(v) + i);
    stg<NT>(xo, reinterpret_cast<T *>(x) + i);
    stg<NT>(wo, reinterpret_cast<T *>(wbar) + i);
  }
  if (VEC == 2 && owns_tail(n)) {
    const int64_t t = n - 1;
    const double vn = scale ? ib * v[t] : v[t];
    const double we = wbar[t];
    if (scale) v[t] = vn;
    x[t] = fma(sz, vn, fma(cz, we, x[t]));
    wbar[t] = fma(nc, vn, sn * we);
  }
}

// P2: t = fma(-α, v, fma(-oldβ, vold, t)) ; dot ? acc = t . t                                  (:301-306)
//   t    load  NT: overwritten here.            store cacheable: the next iteration's P1 reads it next (as v).
//   v    load  cacheable: the next iteration's P2 reads it again (as vold) before the product after it overwrites it.
//   vold load  NT: its last read; the next iteration's product overwrites it (as Mv_next).
template <int VEC, bool NT, bool COMP>
__global__ __launch_bounds__(kBlock) void symmlq_p2_kernel(int64_t n, const SymmlqDevState *st, const double *v, const double *vold,
                                                          double *t, int dot, RedArgs ra) {
  using T = typename VecT<VEC>::type;
  if (seq_skip(ra.stop_seq, ra.seq)) return;
  const double na = -st->alpha, nb = -st->beta;
  dd acc[1] = {dd{0.0, 0.0}};
  const int64_t nvec = n / VEC;
  const int64_t i = lane_index();
  if (i < nvec) {
    const T tv = ldg<NT>(reinterpret_cast<const T *>(t) + i);
    const T vv = ldg<false>(reinterpret_cast<const T *>(v) + i);
    const T ov = ldg<NT>(reinterpret_cast<const T *>(vold) + i);
    T to;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const double tn = fma(na, vget(vv, e), fma(nb, vget(ov, e), vget(tv, e)));   // kaxpy!(-oldβ, Mvold, t) ; kaxpy!(-α, Mv, t)
      vset(to, e, tn);
      if (dot) acc_prod<COMP>(acc[0], tn, tn);
    }
    stg<false>(to, reinterpret_cast<T *>(t) + i);
  }
  if (VEC == 2 && owns_tail(n)) {
    const int64_t k = n - 1;
    const double tn = fma(na, v[k], fma(nb, vold[k], t[k]));
    t[k] = tn;
    if (dot) acc_prod<COMP>(acc[0], tn, tn);
  }
  wave_publish<1>(acc, ra);
}

}  // namespace khip

namespace {

constexpr ScalarPathNT kScalarNT = ScalarPathNT::never;

// P1 takes its sequence number from ctx->ctl, as the reductions do (all zero on the host-driven loop)
int launch_p1(khip_ctx *ctx, int64_t n, const SymmlqDevState *st, double *v, double *x, double *wbar, bool scale) {
  VecPlan L;
  KHIP_TRY(vec_plan(ctx, n, {v, x, wbar}, &L));
  const SeqCtl ctl = ctx->ctl;
  vec_dispatch_vn<kScalarNT>(L, [&](auto V, auto N) {
    hipLaunchKernelGGL((symmlq_p1_kernel<V, N>), L.grid(), dim3(kBlock), 0, ctx->stream, n, st, ctl.stop_seq, ctl.seq, v, x, wbar,
                       scale ? 1 : 0); });
  KHIP_CHECK_HIP(hipGetLastError());
  return KHIP_OK;
}

int launch_p2(khip_ctx *ctx, int64_t n, const SymmlqDevState *st, const double *v, const double *vold, double *t, bool dot,
              int slot) {
  VecPlan L;
  KHIP_TRY(vec_plan(ctx, n, {v, vold, t}, &L, 1));
  RedArgs ra = make_red_args(ctx, slot);
  vec_dispatch<kScalarNT>(L, [&](auto V, auto N, auto C) {
    hipLaunchKernelGGL((symmlq_p2_kernel<V, N, C>), L.grid(), dim3(kBlock), 0, ctx->stream, n, st, v, vold, t, dot ? 1 : 0, ra); });
  KHIP_CHECK_HIP(hipGetLastError());
  if (!dot) return KHIP_OK;        // the partials are not folded: nothing reads them
  return launch_finish(ctx, L.waves(), 1, slot);
}

}  // namespace

struct khip_symmlq_workspace {
  khip_ctx *ctx;
  int64_t m, n;
  int window;
  double *x = nullptr, *Mvold = nullptr, *Mv = nullptr, *Mv_next = nullptr, *wbar = nullptr, *dx = nullptr, *v = nullptr;
  Borrowed borrowed;                        // the caller's vectors (khip_symmlq_workspace_adopt*): never freed here
  std::vector<double> clist, zlist, sprod;  // the window lists (:244-247)
  bool warm_start = false;
  StatsBox box;
  std::vector<double> residualscg, errors, errorscg;   // the histories next to box.residuals; NaN = missing
  double Anorm = NAN, Acond = NAN;
  DeviceLoop<SymmlqDevState, 3> loop;       // fused loops: device copy of the scalar state, pinned snapshots + staging, histories
};

namespace {

// x, Mvold, Mv, Mv_next, w̅ come with the workspace; Δx and v stay empty until needed (src/krylov_workspaces.jl:461-476)
using W = khip_symmlq_workspace;
constexpr WsVec<W> kVectors[] = {{"x", &W::x, Core},         {"Mvold", &W::Mvold, Core}, {"Mv", &W::Mv, Core}, {"Mv_next", &W::Mv_next, Core},
                                 {"wbar", &W::wbar, Core},   {"dx", &W::dx, Lazy},       {"v", &W::v, Lazy}};

// the three Lanczos buffers by their CURRENT role: the fused loops rotate them where the reference copies (:302, :304)
struct Roles {
  double *Mvold, *Mv, *Mv_next;
  void rotate() { double *old = Mvold; Mvold = Mv; Mv = Mv_next; Mv_next = old; }
};

void verbose_row(const khip_options &o, long long iter, const SymmlqDevState &s, double c, double sn, double t0, bool first_row) {
  if (first_row)                                                                                          // :270
    klogf(o.log_fd, "%5lld  %7.1e  %7.1e  %8.1e  %8.1e  %7.1e  %7.1e  %7s  %.2fs\n", iter, s.rNorm, s.beta, c, sn, s.ANorm, s.Acond,
          "\xe2\x9c\x97 \xe2\x9c\x97 \xe2\x9c\x97 \xe2\x9c\x97", now_s() - t0);
  else                                                                                                    // :405
    klogf(o.log_fd, "%5lld  %7.1e  %7.1e  %8.1e  %8.1e  %7.1e  %7.1e  %7.1e  %.2fs\n", iter, s.rNorm, s.beta, c, sn, s.ANorm, s.Acond,
          s.test1, now_s() - t0);
}

int new_workspace(khip_ctx *ctx, int64_t m, int64_t n, int window, W **out) {
  W *ws = new W();
  ws->ctx = ctx; ws->m = m; ws->n = n; ws->window = window;
  ws->clist.assign((size_t)window, 0.0);
  ws->zlist.assign((size_t)window, 0.0);
  ws->sprod.assign((size_t)window, 1.0);
  *out = ws;
  return KHIP_OK;
}

}  // namespace

extern "C" {

khip_symmlq_params khip_symmlq_default_params(void) {
  khip_symmlq_params p;
  memset(&p, 0, sizeof(p));
  p.lambda = 0.0;
  p.lambda_est = 0.0;
  p.etol = NAN;
  p.conlim = NAN;
  p.transfer_to_cg = 1;
  return p;
}

int khip_symmlq_workspace_create(khip_ctx *ctx, int64_t m, int64_t n, int window, khip_symmlq_workspace **out) {
  KHIP_REQUIRE(ctx && out && m >= 0 && n >= 0, "symmlq_workspace_create: bad argument");
  KHIP_REQUIRE(window >= 0, "symmlq_workspace_create: window must not be negative");
  khip_symmlq_workspace *ws = nullptr;
  KHIP_TRY(new_workspace(ctx, m, n, window, &ws));
  const int rc = ws_create_core(ws, kVectors);
  if (rc) { khip_symmlq_workspace_destroy(ws); return rc; }
  *out = ws;
  return KHIP_OK;
}

int khip_symmlq_workspace_adopt(khip_ctx *ctx, int64_t m, int64_t n, int window, double *x, double *Mvold, double *Mv,
                                double *Mv_next, double *wbar, khip_symmlq_workspace **out) {
  KHIP_REQUIRE(ctx && out && m >= 0 && n >= 0, "symmlq_workspace_adopt: bad argument");
  KHIP_REQUIRE(window >= 0, "symmlq_workspace_adopt: window must not be negative");
  khip_symmlq_workspace *ws = nullptr;
  KHIP_TRY(new_workspace(ctx, m, n, window, &ws));
  const int rc = ws_adopt_core(ws, kVectors, "symmlq_workspace_adopt", {x, Mvold, Mv, Mv_next, wbar});
  if (rc) { delete ws; return rc; }
  *out = ws;
  return KHIP_OK;
}

int khip_symmlq_workspace_adopt_vector(khip_symmlq_workspace *ws, const char *name, double *ptr) {
  return ws_adopt_vector(ws, kVectors, "symmlq_workspace_adopt_vector", name, ptr);
}

int khip_symmlq_workspace_destroy(khip_symmlq_workspace *ws) {
  if (!ws) return KHIP_OK;
  ws_free_vectors(ws, kVectors);
  ws->loop.release();
  delete ws;
  return KHIP_OK;
}

int khip_symmlq_warm_start(khip_symmlq_workspace *ws, const double *x0) { return ws_warm_start(ws, kVectors, x0, "symmlq_warm_start"); }
double *khip_symmlq_solution(khip_symmlq_workspace *ws) { return ws ? ws->x : nullptr; }
const khip_stats *khip_symmlq_stats(khip_symmlq_workspace *ws) { return ws ? &ws->box.st : nullptr; }
int khip_symmlq_last_path(khip_symmlq_workspace *ws) { return ws ? ws->box.path : -1; }
double *khip_symmlq_vector(khip_symmlq_workspace *ws, const char *name) { return ws_vector(ws, kVectors, name); }
size_t khip_symmlq_workspace_bytes(khip_symmlq_workspace *ws) { return ws_bytes(ws, kVectors); }

int khip_symmlq_histories(khip_symmlq_workspace *ws, const double **residualscg, int *nresidualscg, const double **errors,
                          int *nerrors, const double **errorscg, int *nerrorscg) {
  KHIP_REQUIRE(ws && residualscg && nresidualscg && errors && nerrors && errorscg && nerrorscg, "symmlq_histories: null argument");
  *residualscg = ws->residualscg.empty() ? nullptr : ws->residualscg.data();
  *nresidualscg = (int)ws->residualscg.size();
  *errors = ws->errors.empty() ? nullptr : ws->errors.data();
  *nerrors = (int)ws->errors.size();
  *errorscg = ws->errorscg.empty() ? nullptr : ws->errorscg.data();
  *nerrorscg = (int)ws->errorscg.size();
  return KHIP_OK;
}

int khip_symmlq_norms(khip_symmlq_workspace *ws, double *Anorm, double *Acond) {
  KHIP_REQUIRE(ws && Anorm && Acond, "symmlq_norms: null argument");
  *Anorm = ws->Anorm;
  *Acond = ws->Acond;
  return KHIP_OK;
}

int khip_symmlq_solve(khip_symmlq_workspace *ws, const khip_operator *A, const khip_operator *M, const double *b,
                      const khip_options *opts_in, const khip_symmlq_params *params_in) {
  KHIP_REQUIRE(ws && A && b, "symmlq_solve: null argument");
  khip_ctx *ctx = ws->ctx;
  const khip_options o = opts_in ? *opts_in : khip_default_options();
  const khip_symmlq_params prm = params_in ? *params_in : khip_symmlq_default_params();
  const double t0 = now_s();
  const double timemax = timemax_of(o);
  const int64_t n = ws->n;
  const double atol = tol_or_default(o.atol), rtol = tol_or_default(o.rtol), etol = tol_or_default(prm.etol);
  const double conlim = std::isnan(prm.conlim) ? 1.0 / std::sqrt(kEps) : prm.conlim;
  const double lambda = prm.lambda, lest = prm.lambda_est;
  const bool history = o.history != 0;
  const int window = ws->window;
  (void)take_alloc_seconds();

  if (int rc = check_shape(ws, {A})) return rc;                                                            // :138-139
  if (ws->m != ws->n) return ws->box.fail(KHIP_ERR_INVALID, "System must be square");
  if (o.variant != 0) return ws->box.fail(KHIP_ERR_INVALID, "symmlq: options.variant must be 0 (there is no other recurrence)");
  if (o.verbose > 0) klogf(o.log_fd, "SYMMLQ: system of size %lld\n", (long long)n);                      // :142

  const bool MisI = (M == nullptr);
  if (!MisI && !ws->v) K(alloc_vec(ctx, n, &ws->v));                                                       // :152
  const bool warm_start = ws->warm_start;
  ws->box.reset(); ws->residualscg.clear(); ws->errors.clear(); ws->errorscg.clear();                    // reset!(stats)
  ws->Anorm = NAN; ws->Acond = NAN;
  Roles B{ws->Mvold, ws->Mv, ws->Mv_next};
  double *x = ws->x, *wbar = ws->wbar;
  double *vM = ws->v;                                                     // v and vold with M (:159-160); with M = I they are Mv, Mvold
  const double ctol = conlim > 0 ? 1.0 / conlim : 0.0;                                                     // :163
  ws->box.path = o.fused ? 1 : 0;

  // set-up, the same primitives on every path (:166-264)
  K(khip_fill(ctx, n, x, 0.0));
  K(residual0(ws, A, lambda, b, warm_start, B.Mvold));
  double *vold = MisI ? B.Mvold : vM;
  if (!MisI) K(apply_op(ctx, M, B.Mvold, vold));                                                           // :178
  double beta1;
  K(khip_dot(ctx, n, vold, B.Mvold, &beta1));
  if (beta1 == 0) {                                                                                        // :180-192
    if (history) { ws->box.push(0.0); ws->residualscg.push_back(0.0); }
    return ws_end(ws, {0, 1, 0, "x is a zero-residual solution", warm_start, t0, true});   // Anorm, Acond stay NaN
  }
  // ⟨b, M b⟩ < 0: the reference takes the square root (:193, a DomainError); the message of its later check (:205) says why
  if (beta1 < 0) return ws->box.fail(KHIP_ERR_INVALID, "Preconditioner is not positive definite");
  beta1 = std::sqrt(beta1);
  SymmlqDevState s;
  memset(&s, 0, sizeof(s));
  s.beta = beta1;
  K(khip_div(ctx, n, vold, s.beta));                                                                       // :195-196
  if (!MisI) K(khip_div(ctx, n, B.Mvold, s.beta));
  K(khip_copy(ctx, n, wbar, vold));                                                                        // :198
  K(apply_op(ctx, A, vold, B.Mv));                                                                         // :200
  double vAv;
  K(khip_dot(ctx, n, vold, B.Mv, &vAv));
  s.lambda = lambda;
  symmlq_step_a(s, vAv);                                                                                   // :201
  K(khip_axpy(ctx, n, -s.alpha, B.Mvold, B.Mv));                                                           // :202
  double *v = MisI ? B.Mv : vM;
  if (!MisI) K(apply_op(ctx, M, B.Mv, v));                                                                 // :203
  double beta2;
  K(khip_dot(ctx, n, v, B.Mv, &beta2));
  if (beta2 < 0) return ws->box.fail(KHIP_ERR_INVALID, "Preconditioner is not positive definite");         // :205
  s.beta = std::sqrt(beta2);
  K(khip_div(ctx, n, v, s.beta));                                                                          // :207-208
  if (!MisI) K(khip_div(ctx, n, B.Mv, s.beta));

  s.lambda_est = lest; s.beta1 = beta1; s.etol = etol; s.ctol = ctol;
  s.transfer_to_cg = prm.transfer_to_cg ? 1 : 0;
  s.window = window;
  s.gbar = s.alpha;                                                                                        // :211-221
  s.dbar = s.beta;
  s.eps_old = 0.0; s.c_old = 1.0;
  s.eta = beta1; s.zeta_old = 0.0;
  s.ANorm2 = s.alpha * s.alpha + s.beta * s.beta;
  s.gmax = -std::numeric_limits<double>::infinity();                                                       // :223-229
  s.gmin = std::numeric_limits<double>::infinity();
  s.ANorm = 0.0; s.Acond = 0.0; s.xNorm = 0.0;
  s.rNorm = beta1;
  if (history) ws->box.push(s.rNorm);
  const bool cg_point0 = s.gbar != 0;
  if (cg_point0) {                                                                                         // :232-239
    s.zbar = s.eta / s.gbar;
    s.xcgNorm = std::fabs(s.zbar);
    s.rcgNorm = beta1 * std::fabs(s.zbar);
  }
  if (history) ws->residualscg.push_back(cg_point0 ? s.rcgNorm : NAN);
  s.err = std::numeric_limits<double>::infinity();                                                         // :241-242
  s.errcg = std::numeric_limits<double>::infinity();
  std::fill(ws->clist.begin(), ws->clist.end(), 0.0);                                                      // :245-247
  std::fill(ws->zlist.begin(), ws->zlist.end(), 0.0);
  std::fill(ws->sprod.begin(), ws->sprod.end(), 1.0);
  if (lest != 0) {                                                                                         // :249-264
    s.rhobar = s.alpha - lest;
    s.sigbar = s.beta;
    s.rho = std::sqrt(s.rhobar * s.rhobar + s.beta * s.beta);
    s.cwold = -1.0;
    s.cw = s.rhobar / s.rho;
    s.sw = s.beta / s.rho;
    if (history) {
      ws->errors.push_back(std::fabs(beta1 / lest));
      ws->errorscg.push_back(cg_point0 ? std::sqrt(ws->errors[0] * ws->errors[0] - s.zbar * s.zbar) : NAN);
    }
  }

  int64_t iter = 0;
  const int64_t itmax = o.itmax == 0 ? 2 * global_rows(ctx, A, n) : o.itmax;      // 2n of the GLOBAL system on every rank (:267)
  if (o.verbose > 0)                                                                                       // :269-270
    klogf(o.log_fd, "%5s  %s  %s  %8s  %8s  %s  %s  %7s  %5s\n", "k", "    \xe2\x80\x96r\xe2\x80\x96", "      \xce\xb2", "cos", "sin",
          "    \xe2\x80\x96" "A\xe2\x80\x96", "   \xce\xba(A)", "test1", "timer");    // %7s of the UTF-8 labels, padded by hand
  if (kdisplay(iter, o.verbose)) verbose_row(o, iter, s, s.c_old, 0.0, t0, true);

  s.tol = atol + rtol * beta1;                                                                             // :272-281
  s.stop_seq = kSeqNever;
  s.solved_lq = s.solved_mach = (s.rNorm <= s.tol) ? 1 : 0;
  s.solved_cg = (cg_point0 && s.transfer_to_cg && s.rcgNorm <= s.tol) ? 1 : 0;
  s.solved = (s.solved_lq || s.solved_cg) ? 1 : 0;
  bool tired = iter >= itmax, user_exit = false, overtimed = false;
  auto running = [&] { return !(s.solved || tired || s.ill_cond_mach || s.ill_cond_lim || user_exit || overtimed); };
  if (running()) symmlq_rotation(s);                                                                       // :287-291 of iteration 1

  SymmlqWindow win{ws->clist.data(), ws->zlist.data(), ws->sprod.data(), nullptr};
  // the end of an iteration on the host-driven loops (:306-308, :313-432): c and s of the iteration for its log row
  auto host_tail = [&](int64_t k, double b2) -> int {
    const double c_k = s.c, s_k = s.s;
    win.errorscg = (history && !ws->errorscg.empty()) ? ws->errorscg.data() : nullptr;
    symmlq_step_b(s, b2, k, win);
    if (s.not_pd) return KHIP_ERR_INVALID;
    if (history) {
      ws->box.push(s.rNorm);
      ws->residualscg.push_back(s.hist_rcg);
      if (lest != 0) { ws->errors.push_back(s.err); ws->errorscg.push_back(s.hist_errcg); }
    }
    if (kdisplay(k, o.verbose)) verbose_row(o, k, s, c_k, s_k, t0, false);
    tired = k >= itmax;
    host_exit(ws, o, t0, timemax, &user_exit, &overtimed);
    return KHIP_OK;
  };
  const char *not_pd_msg = "Preconditioner is not positive definite";                                      // :307

  const bool fastA = A->csr && !A->apply;
  const bool device_loop = o.fused >= 2 && fastA && MisI && lest == 0 && !o.callback && o.verbose <= 0;
  ws->box.path = (device_loop && running()) ? 2 : (o.fused ? 1 : 0);   // a loop that never starts reports 1, as the early returns do
  if (ws->box.path == 0) {
    // -------------------------------------------------------------- the reference's primitive sequence ------------------
    while (running()) {
      const int64_t k = ++iter;
      K(khip_axpy(ctx, n, s.c * s.zeta, wbar, x));                                                        // :292
      K(khip_axpy(ctx, n, s.s * s.zeta, v, x));                                                           // :293
      K(khip_axpby(ctx, n, -s.c, v, s.s, wbar));                                                          // :295
      K(apply_op(ctx, A, v, B.Mv_next));                                                                  // :299
      K(khip_dot(ctx, n, v, B.Mv_next, &vAv));
      symmlq_step_a(s, vAv);                                                                              // :300
      K(khip_axpy(ctx, n, -s.beta, B.Mvold, B.Mv_next));                                                  // :301
      K(khip_copy(ctx, n, B.Mvold, B.Mv));                                                                // :302
      K(khip_axpy(ctx, n, -s.alpha, B.Mv, B.Mv_next));                                                    // :303
      K(khip_copy(ctx, n, B.Mv, B.Mv_next));                                                              // :304
      if (!MisI) K(apply_op(ctx, M, B.Mv, v));                                                            // :305
      K(khip_dot(ctx, n, v, B.Mv, &beta2));                                                               // :306
      if (host_tail(k, beta2) != KHIP_OK) return ws->box.fail(KHIP_ERR_INVALID, not_pd_msg);
      K(khip_div(ctx, n, v, s.beta));                                                                     // :309-310
      if (!MisI) K(khip_div(ctx, n, B.Mv, s.beta));
    }
  } else if (ws->box.path == 1) {
    // -------------------------------------------------------------- host-driven loop on the fused kernels ---------------
    K(ws->loop.alloc());
    const SymmlqDevState *dev = ws->loop.dev;
    while (running()) {
      const int64_t k = ++iter;
      K(ws->loop.upload(ctx, s));
      K(launch_p1(ctx, n, dev, v, x, wbar, MisI && k >= 2));                                              // :292-295 (and :309 of k - 1)
      if (fastA && MisI) {
        const int slot = take_slots(ctx, 1);
        K(spmv_any(ctx, A->csr, v, B.Mv_next, slot));                                                     // :299-300  t = A v ; v.t
        K(fetch_results(ctx, slot, 1, &vAv));
      } else {
        K(apply_op(ctx, A, v, B.Mv_next));
        K(khip_dot(ctx, n, v, B.Mv_next, &vAv));
      }
      symmlq_step_a(s, vAv);
      K(ws->loop.upload(ctx, s));
      const int slot = take_slots(ctx, 1);
      K(launch_p2(ctx, n, dev, B.Mv, B.Mvold, B.Mv_next, MisI, slot));                                    // :301-306
      B.rotate();                                                                                         // :302, :304
      if (MisI) {
        v = B.Mv;
        K(fetch_results(ctx, slot, 1, &beta2));
      } else {
        K(apply_op(ctx, M, B.Mv, v));                                                                     // :305
        K(khip_dot(ctx, n, v, B.Mv, &beta2));
      }
      if (host_tail(k, beta2) != KHIP_OK) return ws->box.fail(KHIP_ERR_INVALID, not_pd_msg);
      if (!MisI) {
        K(khip_div(ctx, n, v, s.beta));                                                                   // :309-310
        K(khip_div(ctx, n, B.Mv, s.beta));
      }
    }
    if (MisI && iter > 0) K(khip_scal(ctx, n, 1.0 / s.beta, B.Mv));                                       // :309 of the last iteration
  } else {
    // -------------------------------------------------------------- device-resident loop ------------------------------
    const Roles first = B;
    const khip_csr *Ac = A->csr;
    auto step = [&](SymmlqDevState *dev, long long j) {
      KHIP_TRY(dev_pass(ctx, &dev->stop_seq, 3 * j, EPI_NONE, nullptr, [&] {
        return launch_p1(ctx, n, dev, B.Mv, x, wbar, j >= 1); }));                                        // :292-295 (and :309 of k - 1)
      KHIP_TRY(dev_stage(ctx, dev, 3 * j + 1, EPI_SYMMLQ_A, 1, [&](int slot) {
        return spmv_any(ctx, Ac, B.Mv, B.Mv_next, slot); }));                                             // :299-300  v.t -> α
      KHIP_TRY(dev_stage(ctx, dev, 3 * j + 2, EPI_SYMMLQ_B, 1, [&](int slot) {
        return launch_p2(ctx, n, dev, B.Mv, B.Mvold, B.Mv_next, true, slot); }));                         // :301-306  t.t -> β, the tests
      B.rotate();
      return (int)KHIP_OK;
    };
    K(ws->loop.run(ctx, s, device_loop_args(itmax, t0, timemax, history, {&ws->box.residuals, &ws->residualscg}), step, &s, &overtimed));
    iter = s.iter;
    tired = iter >= itmax;
    B = replay(first, iter, 3, [](Roles &r) { r.rotate(); });
    if (iter > 0) K(khip_scal(ctx, n, 1.0 / s.beta, B.Mv));                                               // :309 of the last iteration
  }
  ws->Mvold = B.Mvold; ws->Mv = B.Mv; ws->Mv_next = B.Mv_next;
  if (o.verbose > 0) { klogf(o.log_fd, "\n"); klog_flush(o.log_fd); }                                      // :434

  if (s.solved_cg) K(khip_axpy(ctx, n, s.zbar, wbar, x));                                                  // :438-440

  const char *status = "unknown";                                                                         // :443-450
  if (tired) status = "maximum number of iterations exceeded";
  if (s.ill_cond_mach) status = "condition number seems too large for this machine";
  if (s.ill_cond_lim) status = "condition number exceeds tolerance";
  if (s.solved) status = "found approximate solution";
  if (s.solved_lq) status = "solution x\xe1\xb4\xb8 good enough given atol and rtol";
  if (s.solved_cg) status = "solution x\xe1\xb6\x9c good enough given atol and rtol";
  if (user_exit) status = "user-requested exit";
  if (overtimed) status = "time limit exceeded";
  ws->Anorm = s.ANorm;
  ws->Acond = s.Acond;
  return ws_end(ws, {iter, s.solved ? 1 : 0, 0, status, warm_start, t0, true});                           // :453-463
}

}  // extern "C"
