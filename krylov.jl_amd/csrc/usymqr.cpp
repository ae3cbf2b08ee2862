// usymqr.cpp -- usymqr! (src/usymqr.jl:130-365) above the device primitives, with its fused gfx950 kernels.
//
// Real Float64, A of m rows and n columns, no M and N.  Three loops, chosen as for qmr! (khip_usymqr_last_path):
//   0  options.fused = 0, and every m ≠ n system: the reference's primitive sequence, one launch per k* call, one host sync per
//      kdot / knorm;
//   1  the host-driven loop on the fused kernels (a user operator, a callback or verbose > 0);
//   2  the device-resident loop (default; A and Aᴴ both CSR handles): the scalar recurrences and stopping tests run as the
//      epilogues of the two reductions of an iteration (usymqr_step_a/b, solver_device.hpp), iterations are enqueued ahead.
// One iteration on the fused paths (m = n), after q = A uₖ and p = Aᴴ vₖ:
//   P1   k ≥ 2: q = fma(-γₖ, vₖ₋₁, q) ; p = fma(-βₖ, uₖ₋₁, p) ; vₖ.q                    (ssy.hpp)                   56n bytes
//   P2   q = fma(-αₖ, vₖ, q) ; p = fma(-αₖ, uₖ, p) ; (q.q, p.p)                        (ssy.hpp)                   48n bytes
//   P3   wₖ = (uₖ - λₖ₋₁ wₖ₋₁ - ϵₖ₋₂ wₖ₋₂) / δₖ ; x = fma(ζₖ, wₖ, x) ; βₖ₊₁ ≠ 0 ? vₖ₊₁ = q / βₖ₊₁ ; γₖ₊₁ ≠ 0 ? uₖ₊₁ = p / γₖ₊₁     80n bytes
// against 296n for the primitive sequence; kcopy!(vₖ₋₁, vₖ), kcopy!(uₖ₋₁, uₖ) and @kswap!(wₖ₋₂, wₖ₋₁) become rotations of the
// buffers' roles (vₖ₊₁ is written where vₖ₋₁ was, wₖ where wₖ₋₂ was).  Every elementwise value uses the expression of the primitive
// it replaces (fma for kaxpy!, a x for kscal!, x (1 / a) for kdiv!, which the reference defines as kscal!(1 / a), / for kdivcopy!):
// the fused loops agree with the primitive sequence bit for bit on elementwise values and to the reductions' one ulp otherwise;
// loops 1 and 2 run the same kernels and the same scalar code and produce the same bits.
// P3 has no reduction; the stopping tests belong to P2's epilogue, and P3 of the iteration that stops still runs, because the
// reference updates x, vₖ₊₁ and uₖ₊₁ before it tests.
// This file owns P3, the set-up scalars, the QR part of a primitive iteration and the status strings; the loops are ssy.hpp's.
#include "ssy.hpp"   // P1, P2 and the driver of the three loops

using namespace khip;

namespace khip {   // (named, not anonymous: stable kernel names in traces)

// ---------------------------------------------------------------------------------------------------------- kernels ----
// Each thread owns one VEC-vector of every stream; the odd tail element (VEC = 2, n odd) goes to thread 0 of block 0.
// Cache hints, the rule of bilanczos.hpp: a load is non-temporal when it is the LAST read of that data (wₖ₋₂, x, q, p: overwritten
// here or by the next products); wₖ₋₁ is read again by the next P3 (as wₖ₋₂) and uₖ by the next P1 (as uₖ₋₁): they stay cacheable.  A
// store is non-temporal when nothing reads it before the next iteration's P3 (x, wₖ); vₖ₊₁ and uₖ₊₁ are read by the next products.

// wₖ of one element (:276-294), qmr_w (qmr.cpp) with uₖ.  stage 1: kdivcopy!(w, u, δ).  stage 2: kaxpy!(-λ, w₁, w₂) ;
// kaxpy!(1, u, w₂) ; kdiv!(w₂, δ).  stage >= 3: kscal!(-ϵ, w₂) first.
__device__ __forceinline__ double usymqr_w(int stage, double u, double w1, double w2, double ne, double nl, double dl, double idl) {
  if (stage == 1) return u / dl;
  double t = stage >= 3 ? ne * w2 : w2;
  t = fma(nl, w1, t);
  t = fma(1.0, u, t);
  return t * idl;
}

// P3: w_out = wₖ (usymqr_w) ; x = fma(ζₖ, wₖ, x) ; v_next = βₖ₊₁ ≠ 0 ? q / βₖ₊₁ : v ; u_next = γₖ₊₁ ≠ 0 ? p / γₖ₊₁ : u    (:276-317)
// The two guards are independent.  w_out is w2 from stage 2 on (wₖ over wₖ₋₂) and the buffer of the role wₖ₋₁ at stage 1, where
// neither w1 nor w2 is read.  No reduction: the sequence number comes as an argument.
template <int VEC, bool NT>
__global__ __launch_bounds__(kBlock) void usymqr_p3_kernel(int64_t n, const UsymqrDevState *st, const long long *stop_seq, long long seq,
                                                          double *x, const double *w2, const double *w1, double *w_out,
                                                          const double *v, const double *u, const double *q, const double *p,
                                                          double *v_next, double *u_next, int stage) {
  using T = typename VecT<VEC>::type;
  if (seq_skip(stop_seq, seq)) return;
  const double ne = st->neg_eps, nl = st->neg_lambda, dl = st->delta, idl = st->inv_delta, zt = st->zeta;
  const double bn = st->beta_next, gn = st->gamma_next;
  const bool div_v = bn != 0.0, div_u = gn != 0.0;
  const int64_t nvec = n / VEC;
  const int64_t i = lane_index();
  if (i < nvec) {
    const T uv = ldg<false>(reinterpret_cast<const T *>(u) + i);       // u is the next iteration's u_prev
    const T xv = ldg<NT>(reinterpret_cast<const T *>(x) + i);
    T w2v = {}, w1v = {};
    if (stage >= 2) {
      w2v = ldg<NT>(reinterpret_cast<const T *>(w2) + i);
      w1v = ldg<false>(reinterpret_cast<const T *>(w1) + i);           // wₖ₋₁ is the next iteration's wₖ₋₂
    }
    T vo = div_v ? ldg<NT>(reinterpret_cast<const T *>(q) + i) : ldg<false>(reinterpret_cast<const T *>(v) + i);
    T uo = uv;
    if (div_u) uo = ldg<NT>(reinterpret_cast<const T *>(p) + i);
    T wo, xo;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const double w = usymqr_w(stage, vget(uv, e), vget(w1v, e), vget(w2v, e), ne, nl, dl, idl);
      vset(wo, e, w);
      vset(xo, e, fma(zt, w, vget(xv, e)));
      if (div_v) vset(vo, e, vget(vo, e) / bn);
      if (div_u) vset(uo, e, vget(uo, e) / gn);
    }
    stg<NT>(xo, reinterpret_cast<T *>(x) + i);
    stg<NT>(wo, reinterpret_cast<T *>(w_out) + i);
    stg<false>(vo, reinterpret_cast<T *>(v_next) + i);                  // read by the next products
    stg<false>(uo, reinterpret_cast<T *>(u_next) + i);
  }
  if (VEC == 2 && owns_tail(n)) {
    const int64_t t = n - 1;
    const double ue = u[t];
    const double w = usymqr_w(stage, ue, stage >= 2 ? w1[t] : 0.0, stage >= 2 ? w2[t] : 0.0, ne, nl, dl, idl);
    x[t] = fma(zt, w, x[t]);
    w_out[t] = w;
    v_next[t] = div_v ? q[t] / bn : v[t];
    u_next[t] = div_u ? p[t] / gn : ue;
  }
}

}  // namespace khip

namespace {

// P3 takes its sequence number from ctx->ctl, as the reductions do (all zero on the host-driven loop)
int launch_p3(khip_ctx *ctx, int64_t n, const UsymqrDevState *st, double *x, const double *w2, const double *w1, double *w_out,
              const double *v, const double *u, const double *q, const double *p, double *v_next, double *u_next, int stage) {
  VecPlan L;
  KHIP_TRY(vec_plan(ctx, n, {x, w2, w1, w_out, v, u, q, p, v_next, u_next}, &L));
  const SeqCtl ctl = ctx->ctl;
  ProfScope prof_scope(ctx, kProfUsymqrP3);
  vec_dispatch_vn<ScalarPathNT::never>(L, [&](auto V, auto N) {
    hipLaunchKernelGGL((usymqr_p3_kernel<V, N>), L.grid(), dim3(kBlock), 0, ctx->stream, n, st, ctl.stop_seq, ctl.seq, x, w2, w1, w_out,
                       v, u, q, p, v_next, u_next, stage); });
  KHIP_CHECK_HIP(hipGetLastError());
  return KHIP_OK;
}

}  // namespace

struct khip_usymqr_workspace {
  khip_ctx *ctx;
  int64_t m, n;
  // by their CURRENT role: the fused loops rotate (v_prev, v), (u_prev, u) and (w_prev2, w_prev).  v_prev, v, q have m entries,
  // the others n
  double *v_prev = nullptr, *v = nullptr, *q = nullptr, *x = nullptr, *w_prev2 = nullptr, *w_prev = nullptr, *u_prev = nullptr,
         *u = nullptr, *p = nullptr, *dx = nullptr;
  Borrowed borrowed;                        // the caller's vectors (khip_usymqr_workspace_adopt*): never freed here
  bool warm_start = false;
  StatsBox box;
  std::vector<double> aresiduals;           // the Aresiduals history next to box.residuals
  DeviceLoop<UsymqrDevState, 3> loop;       // fused loops: device copy of the scalar state, pinned snapshots + staging, histories
};

namespace {

// vₖ₋₁, vₖ, q, x, wₖ₋₂, wₖ₋₁, uₖ₋₁, uₖ, p come with the workspace; Δx stays empty until a warm start (src/krylov_workspaces.jl,
// UsymqrWorkspace: the table keeps its order)
using W = khip_usymqr_workspace;
constexpr WsVec<W> kVectors[] = {{"v_prev", &W::v_prev, Core, RowSide}, {"v", &W::v, Core, RowSide},   {"q", &W::q, Core, RowSide},
                                 {"x", &W::x, Core},                    {"w_prev2", &W::w_prev2, Core}, {"w_prev", &W::w_prev, Core},
                                 {"u_prev", &W::u_prev, Core},          {"u", &W::u, Core},             {"p", &W::p, Core},
                                 {"dx", &W::dx, Lazy}};

// what usymqr! adds to the driver of the process (ssy.hpp)
struct Usymqr : SsyPolicy<UsymqrDevState, W> {
  static constexpr Epilogue kEpiA = EPI_USYMQR_A, kEpiB = EPI_USYMQR_B;
  double *x, *w2, *w1;                                                                 // wₖ₋₂, wₖ₋₁ by their current role
  static void step_a(State &s, double vq) { usymqr_step_a(s, vq); }
  static void step_b(State &s, double qq, double pp, int64_t k) { (void)usymqr_step_b(s, qq, pp, k); }
  static bool stopped(const State &s) { return s.solved || s.inconsistent; }
  int p3(khip_ctx *ctx, int64_t n, const State *dev, const SsyRoles &r, int64_t k) const {
    return launch_p3(ctx, n, dev, x, w2, w1, k == 1 ? w1 : w2, r.v, r.u, r.q, r.p, r.v_prev, r.u_prev, k < 3 ? (int)k : 3);
  }
  void rotate(int64_t k) { if (k >= 2) std::swap(w2, w1); }                            // wₖ was written over wₖ₋₂ (src/usymqr.jl:320-322)
  void fix_after_device_loop(const State &s) { if (s.iter >= 2 && !(s.iter & 1)) std::swap(w2, w1); }
  void store(W *ws) const { ws->w_prev = w1; ws->w_prev2 = w2; }
  void push_history(W *ws, const State &s) const { ws->box.push(s.rNorm); ws->aresiduals.push_back(s.ArNorm); }
  static std::vector<double> *dual_history(W *ws) { return &ws->aresiduals; }
  void verbose_row(const khip_options &o, long long k, const State &s, double t0) const {                // src/usymqr.jl:343
    klogf(o.log_fd, "%5lld  %7.1e  %8.1e  %.2fs\n", k, s.rNorm, s.ArNorm, now_s() - t0);
  }
  // wₖ and x, then the shift of v and u (src/usymqr.jl:276-322)
  int primitive_tail(Ssy<Usymqr> &L, int64_t k) {
    W *ws = L.ws;
    khip_ctx *ctx = L.ctx;
    const int64_t n = L.n;
    State &s = L.s;
    double *w = w2;
    if (k == 1) {
      w = w1;
      K(khip_divcopy(ctx, n, w, L.r.u, s.delta));
    } else {
      if (k >= 3) K(khip_scal(ctx, n, s.neg_eps, w));
      K(khip_axpy(ctx, n, s.neg_lambda, w1, w));
      K(khip_axpy(ctx, n, 1.0, L.r.u, w));
      K(khip_div(ctx, n, w, s.delta));
    }
    K(khip_axpy(ctx, n, s.zeta, w, x));
    K(L.shift());
    rotate(k);                                                                         // @kswap!(wₖ₋₂, wₖ₋₁)
    return KHIP_OK;
  }
};

}  // namespace

extern "C" {

int khip_usymqr_workspace_create(khip_ctx *ctx, int64_t m, int64_t n, khip_usymqr_workspace **out) {
  return ws_create(ctx, m, n, kVectors, "usymqr_workspace_create", khip_usymqr_workspace_destroy, out);
}

int khip_usymqr_workspace_adopt(khip_ctx *ctx, int64_t m, int64_t n, double *v_prev, double *v, double *q, double *x, double *w_prev2,
                                double *w_prev, double *u_prev, double *u, double *p, khip_usymqr_workspace **out) {
  return ws_adopt(ctx, m, n, kVectors, "usymqr_workspace_adopt", {v_prev, v, q, x, w_prev2, w_prev, u_prev, u, p}, out);
}

int khip_usymqr_workspace_adopt_vector(khip_usymqr_workspace *ws, const char *name, double *ptr) {
  return ws_adopt_vector(ws, kVectors, "usymqr_workspace_adopt_vector", name, ptr);
}

int khip_usymqr_workspace_destroy(khip_usymqr_workspace *ws) {
  if (!ws) return KHIP_OK;
  ws_free_vectors(ws, kVectors);
  ws->loop.release();
  delete ws;
  return KHIP_OK;
}

int khip_usymqr_warm_start(khip_usymqr_workspace *ws, const double *x0) { return ws_warm_start(ws, kVectors, x0, "usymqr_warm_start"); }
double *khip_usymqr_solution(khip_usymqr_workspace *ws) { return ws ? ws->x : nullptr; }
const khip_stats *khip_usymqr_stats(khip_usymqr_workspace *ws) { return ws ? &ws->box.st : nullptr; }
int khip_usymqr_last_path(khip_usymqr_workspace *ws) { return ws ? ws->box.path : -1; }
double *khip_usymqr_vector(khip_usymqr_workspace *ws, const char *name) { return ws_vector(ws, kVectors, name); }
size_t khip_usymqr_workspace_bytes(khip_usymqr_workspace *ws) { return ws_bytes(ws, kVectors); }

int khip_usymqr_aresiduals(khip_usymqr_workspace *ws, const double **aresiduals, int *naresiduals) {
  KHIP_REQUIRE(ws && aresiduals && naresiduals, "usymqr_aresiduals: null argument");
  *aresiduals = ws->aresiduals.empty() ? nullptr : ws->aresiduals.data();
  *naresiduals = (int)ws->aresiduals.size();
  return KHIP_OK;
}

int khip_usymqr_solve(khip_usymqr_workspace *ws, const khip_operator *A, const khip_operator *At, const double *b, const double *c,
                      const khip_options *opts_in) {
  KHIP_REQUIRE(ws && A && b, "usymqr_solve: null argument");
  Ssy<Usymqr> L(ws, A, At, opts_in);
  khip_ctx *ctx = L.ctx;
  const khip_options &o = L.o;
  const int64_t m = L.m, n = L.n;
  UsymqrDevState &s = L.s;
  const double atol = tol_or_default(o.atol), rtol = tol_or_default(o.rtol);

  if (int rc = L.check("usymqr", c)) return rc;                                                           // :133-136
  if (o.verbose > 0) klogf(o.log_fd, "USYMQR: system of %lld equations in %lld variables\n", (long long)m, (long long)n);   // :137
  const bool warm_start = ws->warm_start;
  ws->box.reset(); ws->aresiduals.clear();                                                               // reset!(stats)
  double *x = L.pol.x = ws->x;
  L.pol.w1 = ws->w_prev;
  L.pol.w2 = ws->w_prev2;

  // set-up, the same primitives on every path (:153-201)
  const double *r0;
  K(L.residual(b, warm_start, &r0));
  K(khip_fill(ctx, n, x, 0.0));
  double rNorm0;
  K(khip_nrm2(ctx, m, r0, &rNorm0));
  if (L.history) ws->box.push(rNorm0);
  ws->box.path = (o.fused && L.square()) ? 1 : 0;
  if (rNorm0 == 0) return L.end(1, 0, "x is a zero-residual solution", warm_start);                      // :164-173
  L.itmax = o.itmax == 0 ? global_rows(ctx, A, m) + global_rows(ctx, At, n) : o.itmax;                   // m + n of the global system (:176)
  s.eps_tol = atol + rtol * rNorm0;                                                                      // :178
  s.atol = atol; s.rtol = rtol; s.kappa = 0.0;
  if (o.verbose > 0) {                                                                                    // :180-181 (labels padded by hand)
    klogf(o.log_fd, "%5s  %s  %s  %5s\n", "k", "   ‖rₖ‖", "‖Aᴴrₖ₋₁‖", "timer");
    if (kdisplay(0, o.verbose)) klogf(o.log_fd, "%5d  %7.1e  %s  %.2fs\n", 0, rNorm0, " ✗ ✗ ✗ ✗", now_s() - L.t0);
  }
  double gamma1;
  K(khip_nrm2(ctx, n, c, &gamma1));                                                                      // :184
  K(L.start(rNorm0, gamma1, r0, c));                                                                     // :183-188
  s.c_km2 = s.c_km1 = 1.0;                                                                               // :189-190
  K(khip_fill(ctx, n, L.pol.w2, 0.0));                                                                   // :191-192
  K(khip_fill(ctx, n, L.pol.w1, 0.0));
  s.zbar = s.beta;                                                                                        // :193
  s.rNorm = rNorm0;
  s.stop_seq = kSeqNever;
  s.solved = (rNorm0 <= s.eps_tol) ? 1 : 0;                                                              // :196-197

  K(L.iterate());                                                                                         // :203-345

  const char *status = "unknown";                                                                         // :348-351
  if (L.tired) status = "maximum number of iterations exceeded";
  if (s.solved) status = "solution good enough given atol and rtol";
  if (L.user_exit) status = "user-requested exit";
  if (L.overtimed) status = "time limit exceeded";
  return L.end(s.solved ? 1 : 0, s.inconsistent ? 1 : 0, status, warm_start);                           // :354-363
}

}  // extern "C"
