// qmr.cpp -- qmr! (src/qmr.jl:124-406) above the device primitives, with its fused gfx950 kernels.
//
// Real Float64.  Three loops, chosen as for bilq! (khip_qmr_last_path):
//   0  options.fused = 0: the reference's primitive sequence, one launch per k* call, one host sync per kdot / kdotr;
//   1  the host-driven loop on the fused kernels (with M or N, a user operator, a callback or verbose > 0);
//   2  the device-resident loop (default; A and A' both CSR handles): the scalar recurrences and stopping tests run as the
//      epilogues of the three reductions of an iteration (qmr_step_a/b/c, solver_device.hpp), iterations are enqueued ahead.
// One iteration with M = N = I on the fused paths, after q = A vₖ and p = A' uₖ:
//   P1   q = fma(-γₖ, vₖ₋₁, q) ; p = fma(-βₖ, uₖ₋₁, p) ; uₖ.q                          (bilanczos.hpp)             56n bytes
//   P2   q = fma(-αₖ, vₖ, q) ; p = fma(-αₖ, uₖ, p) ; p.q                               (bilanczos.hpp)             48n bytes
//   P3   wₖ = (vₖ - λₖ₋₁ wₖ₋₁ - ϵₖ₋₂ wₖ₋₂) / δₖ ; x = fma(ζₖ, wₖ, x) ; vₖ₊₁ = q / βₖ₊₁ ; uₖ₊₁ = p / γₖ₊₁ ; vₖ₊₁.vₖ₊₁        80n bytes
// against 304n for the primitive sequence; kcopy!(vₖ₋₁, vₖ), kcopy!(uₖ₋₁, uₖ) and @kswap!(wₖ₋₂, wₖ₋₁) become rotations of the
// buffers' roles (vₖ₊₁ is written where vₖ₋₁ was, wₖ where wₖ₋₂ was).  Every elementwise value uses the expression of the primitive
// it replaces (fma for kaxpy!, a x for kscal!, x (1 / a) for kdiv!, which the reference defines as kscal!(1 / a), / for kdivcopy!):
// the fused loops agree with the primitive sequence bit for bit on elementwise values and to the reductions' one ulp otherwise;
// loops 1 and 2 run the same kernels and the same scalar code and produce the same bits.
// This file owns P3, the set-up scalars, the QR part of a primitive iteration and the status strings; the loops are bilanczos.hpp's.
#include "bilanczos.hpp"   // P1, P2 and the driver of the three loops, shared with bilq.cpp and bilqr.cpp

using namespace khip;

namespace khip {   // (named, not anonymous: stable kernel names in traces)

// ---------------------------------------------------------------------------------------------------------- kernels ----
// Each thread owns one VEC-vector of every stream; the odd tail element (VEC = 2, n odd) goes to thread 0 of block 0.
// Cache hints, the rule of bilq.cpp: a load is non-temporal when it is the LAST read of that data (wₖ₋₂, x, q, p: overwritten here or
// by the next products); wₖ₋₁ is read again by the next P3 (as wₖ₋₂) and vₖ by the next P1 (as vₖ₋₁): they stay cacheable.  A store
// is non-temporal when nothing reads it before the next iteration's P3 (x, wₖ); vₖ₊₁ and uₖ₊₁ are read by the next products.

// wₖ of one element (:316-334).  stage 1: kdivcopy!(w, v, δ).  stage 2: kaxpy!(-λ, w₁, w₂) ; kaxpy!(1, v, w₂) ; kdiv!(w₂, δ).
// stage >= 3: kscal!(-ϵ, w₂) first.  The general form with λ = ϵ = 0 differs from the special ones in the sign of zeros.
__device__ __forceinline__ double qmr_w(int stage, double v, double w1, double w2, double ne, double nl, double dl, double idl) {
  if (stage == 1) return v / dl;
  double t = stage >= 3 ? ne * w2 : w2;
  t = fma(nl, w1, t);
  t = fma(1.0, v, t);
  return t * idl;
}

// P3: w_out = wₖ (qmr_w) ; x = fma(ζₖ, wₖ, x) ; pᴴq ≠ 0 ? (v_next = q / βₖ₊₁ ; u_next = p / γₖ₊₁) : (v_next = v ; u_next = u) ;
// acc = v_next . v_next                                                                (:316-350)
// w_out is w2 from stage 2 on (wₖ over wₖ₋₂) and the buffer of the role wₖ₋₁ at stage 1, where neither w1 nor w2 is read.
template <int VEC, bool NT, bool COMP>
__global__ __launch_bounds__(kBlock) void qmr_p3_kernel(int64_t n, const QmrDevState *st, double *x, const double *w2, const double *w1,
                                                       double *w_out, const double *v, const double *u, const double *q,
                                                       const double *p, double *v_next, double *u_next, int stage, RedArgs ra) {
  using T = typename VecT<VEC>::type;
  if (seq_skip(ra.stop_seq, ra.seq)) return;
  const double ne = st->neg_eps, nl = st->neg_lambda, dl = st->delta, idl = st->inv_delta, zt = st->zeta;
  const double bn = st->beta_next, gn = st->gamma_next;
  const bool divide = st->pq != 0.0;
  dd acc[1] = {dd{0.0, 0.0}};
  const int64_t nvec = n / VEC;
  const int64_t i = lane_index();
  if (i < nvec) {
    const T vv = ldg<false>(reinterpret_cast<const T *>(v) + i);       // v is the next iteration's v_prev
    const T xv = ldg<NT>(reinterpret_cast<const T *>(x) + i);
    T w2v = {}, w1v = {};
    if (stage >= 2) {
      w2v = ldg<NT>(reinterpret_cast<const T *>(w2) + i);
      w1v = ldg<false>(reinterpret_cast<const T *>(w1) + i);           // wₖ₋₁ is the next iteration's wₖ₋₂
    }
    T qv = {}, pv = {};
    if (divide) {
      qv = ldg<NT>(reinterpret_cast<const T *>(q) + i);
      pv = ldg<NT>(reinterpret_cast<const T *>(p) + i);
    }
    T wo, xo;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const double w = qmr_w(stage, vget(vv, e), vget(w1v, e), vget(w2v, e), ne, nl, dl, idl);
      vset(wo, e, w);
      vset(xo, e, fma(zt, w, vget(xv, e)));
    }
    stg<NT>(xo, reinterpret_cast<T *>(x) + i);
    stg<NT>(wo, reinterpret_cast<T *>(w_out) + i);
    T vo, uo;
    if (divide) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        vset(vo, e, vget(qv, e) / bn);
        vset(uo, e, vget(pv, e) / gn);
      }
    } else {
      vo = vv;
      uo = ldg<false>(reinterpret_cast<const T *>(u) + i);
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc_prod<COMP>(acc[0], vget(vo, e), vget(vo, e));
    stg<false>(vo, reinterpret_cast<T *>(v_next) + i);                  // read by the next products
    stg<false>(uo, reinterpret_cast<T *>(u_next) + i);
  }
  if (VEC == 2 && owns_tail(n)) {
    const int64_t t = n - 1;
    const double ve = v[t];
    const double w = qmr_w(stage, ve, stage >= 2 ? w1[t] : 0.0, stage >= 2 ? w2[t] : 0.0, ne, nl, dl, idl);
    x[t] = fma(zt, w, x[t]);
    w_out[t] = w;
    const double vo = divide ? q[t] / bn : ve;
    const double uo = divide ? p[t] / gn : u[t];
    v_next[t] = vo;
    u_next[t] = uo;
    acc_prod<COMP>(acc[0], vo, vo);
  }
  wave_publish<1>(acc, ra);
}

}  // namespace khip

namespace {

constexpr ScalarPathNT kScalarNT = ScalarPathNT::never;

int launch_p3(khip_ctx *ctx, int64_t n, const QmrDevState *st, double *x, const double *w2, const double *w1, double *w_out,
              const double *v, const double *u, const double *q, const double *p, double *v_next, double *u_next, int stage, int slot) {
  VecPlan L;
  KHIP_TRY(vec_plan(ctx, n, {x, w2, w1, w_out, v, u, q, p, v_next, u_next}, &L, 1));
  RedArgs ra = make_red_args(ctx, slot);
  vec_dispatch<kScalarNT>(L, [&](auto V, auto N, auto C) {
    hipLaunchKernelGGL((qmr_p3_kernel<V, N, C>), L.grid(), dim3(kBlock), 0, ctx->stream, n, st, x, w2, w1, w_out, v, u, q, p, v_next,
                       u_next, stage, ra); });
  KHIP_CHECK_HIP(hipGetLastError());
  return launch_finish(ctx, L.waves(), 1, slot);
}

}  // namespace

struct khip_qmr_workspace {
  khip_ctx *ctx;
  int64_t m, n;
  // by their CURRENT role: the fused loops rotate (v_prev, v), (u_prev, u) and (w_prev2, w_prev)
  double *u_prev = nullptr, *u = nullptr, *q = nullptr, *v_prev = nullptr, *v = nullptr, *p = nullptr, *x = nullptr,
         *w_prev2 = nullptr, *w_prev = nullptr, *dx = nullptr, *t = nullptr, *s = nullptr;
  Borrowed borrowed;                        // the caller's vectors (khip_qmr_workspace_adopt*): never freed here
  bool warm_start = false;
  StatsBox box;
  DeviceLoop<QmrDevState, 3> loop;          // fused loops: device copy of the scalar state, pinned snapshots + staging, history
};

namespace {

// uₖ₋₁, uₖ, q, vₖ₋₁, vₖ, p, x, wₖ₋₂, wₖ₋₁ come with the workspace; Δx, t, s stay empty until needed (src/krylov_workspaces.jl, QmrWorkspace)
using W = khip_qmr_workspace;
constexpr WsVec<W> kVectors[] = {{"u_prev", &W::u_prev, Core}, {"u", &W::u, Core}, {"q", &W::q, Core}, {"v_prev", &W::v_prev, Core},
                                 {"v", &W::v, Core},           {"p", &W::p, Core}, {"x", &W::x, Core}, {"w_prev2", &W::w_prev2, Core},
                                 {"w_prev", &W::w_prev, Core}, {"dx", &W::dx, Lazy}, {"t", &W::t, Lazy}, {"s", &W::s, Lazy}};

// what qmr! adds to the two-sided Lanczos driver (bilanczos.hpp)
struct Qmr : BiLanczosPolicy<QmrDevState, W> {
  static constexpr Epilogue kEpiA = EPI_QMR_A, kEpiB = EPI_QMR_B, kEpiC = EPI_QMR_C;
  static constexpr int kP3Sums = 1;                                                    // vₖ₊₁.vₖ₊₁
  double *x, *w2, *w1;                                                                 // wₖ₋₂, wₖ₋₁ by their current role
  static void step_a(State &s, double uq) { qmr_step_a(s, uq); }
  static void step_b(State &s, double pq, int64_t k) { qmr_step_b(s, pq, k); }
  static void step_c(State &s, const double *sums, int64_t k) { qmr_step_c(s, sums[0], k); }
  static bool stopped(const State &s) { return s.solved || s.breakdown; }
  int p3(khip_ctx *ctx, int64_t n, const State *dev, const BiLanczosRoles &r, int64_t k, int slot) const {
    return launch_p3(ctx, n, dev, x, w2, w1, k == 1 ? w1 : w2, r.v, r.u, r.q, r.p, r.v_prev, r.u_prev, k < 3 ? (int)k : 3, slot);
  }
  void rotate(int64_t k, bool) { if (k >= 2) std::swap(w2, w1); }                     // wₖ was written over wₖ₋₂ (src/qmr.jl:357-359)
  void fix_after_device_loop(const State &s) { if (s.iter >= 2 && !(s.iter & 1)) std::swap(w2, w1); }
  void store(W *ws) const { ws->w_prev = w1; ws->w_prev2 = w2; }
  void push_history(W *ws, const State &s) const { ws->box.push(s.rNorm); }
  static void row(const khip_options &o, long long iter, double alpha, double rNorm, double t0) {   // src/qmr.jl:207, :379
    klogf(o.log_fd, "%5lld  %8.1e  %7.1e  %.2fs\n", iter, alpha, rNorm, now_s() - t0);
  }
  void verbose_row(const khip_options &o, long long k, const State &s, double t0) const { row(o, k, s.alpha, s.rNorm, t0); }
  // wₖ and x, the shift, then ‖vₖ₊₁‖² on the shifted vector (src/qmr.jl:316-359)
  int primitive_tail(BiLanczos<Qmr> &L, int64_t k, double pq) {
    W *ws = L.ws;
    khip_ctx *ctx = L.ctx;
    const int64_t n = L.n;
    State &s = L.s;
    double *w = w2;
    if (k == 1) {
      w = w1;
      K(khip_divcopy(ctx, n, w, L.r.v, s.delta));
    } else {
      if (k >= 3) K(khip_scal(ctx, n, s.neg_eps, w));
      K(khip_axpy(ctx, n, s.neg_lambda, w1, w));
      K(khip_axpy(ctx, n, 1.0, L.r.v, w));
      K(khip_div(ctx, n, w, s.delta));
    }
    K(khip_axpy(ctx, n, s.zeta, w, x));
    K(L.shift(pq));
    double vv;
    K(khip_dot(ctx, n, L.r.v, L.r.v, &vv));
    rotate(k, true);                                                                   // @kswap!(wₖ₋₂, wₖ₋₁)
    qmr_step_c(s, vv, k);
    return KHIP_OK;
  }
};

}  // namespace

extern "C" {

khip_qmr_params khip_qmr_default_params(void) {
  khip_qmr_params p;
  p.Mt = nullptr;
  p.Nt = nullptr;
  return p;
}

int khip_qmr_workspace_create(khip_ctx *ctx, int64_t m, int64_t n, khip_qmr_workspace **out) {
  KHIP_REQUIRE(ctx && out && m >= 0 && n >= 0, "qmr_workspace_create: bad argument");
  KHIP_REQUIRE(m == n, "System must be square");
  khip_qmr_workspace *ws = new khip_qmr_workspace();
  ws->ctx = ctx; ws->m = m; ws->n = n;
  const int rc = ws_create_core(ws, kVectors);
  if (rc) { khip_qmr_workspace_destroy(ws); return rc; }
  *out = ws;
  return KHIP_OK;
}

int khip_qmr_workspace_adopt(khip_ctx *ctx, int64_t m, int64_t n, double *u_prev, double *u, double *q, double *v_prev, double *v,
                             double *p, double *x, double *w_prev2, double *w_prev, khip_qmr_workspace **out) {
  KHIP_REQUIRE(ctx && out && m >= 0 && n >= 0, "qmr_workspace_adopt: bad argument");
  KHIP_REQUIRE(m == n, "System must be square");
  khip_qmr_workspace *ws = new khip_qmr_workspace();
  ws->ctx = ctx; ws->m = m; ws->n = n;
  const int rc = ws_adopt_core(ws, kVectors, "qmr_workspace_adopt", {u_prev, u, q, v_prev, v, p, x, w_prev2, w_prev});
  if (rc) { delete ws; return rc; }
  *out = ws;
  return KHIP_OK;
}

int khip_qmr_workspace_adopt_vector(khip_qmr_workspace *ws, const char *name, double *ptr) {
  return ws_adopt_vector(ws, kVectors, "qmr_workspace_adopt_vector", name, ptr);
}

int khip_qmr_workspace_destroy(khip_qmr_workspace *ws) {
  if (!ws) return KHIP_OK;
  ws_free_vectors(ws, kVectors);
  ws->loop.release();
  delete ws;
  return KHIP_OK;
}

int khip_qmr_warm_start(khip_qmr_workspace *ws, const double *x0) { return ws_warm_start(ws, kVectors, x0, "qmr_warm_start"); }
double *khip_qmr_solution(khip_qmr_workspace *ws) { return ws ? ws->x : nullptr; }
const khip_stats *khip_qmr_stats(khip_qmr_workspace *ws) { return ws ? &ws->box.st : nullptr; }
int khip_qmr_last_path(khip_qmr_workspace *ws) { return ws ? ws->box.path : -1; }
double *khip_qmr_vector(khip_qmr_workspace *ws, const char *name) { return ws_vector(ws, kVectors, name); }
size_t khip_qmr_workspace_bytes(khip_qmr_workspace *ws) { return ws_bytes(ws, kVectors); }

int khip_qmr_solve(khip_qmr_workspace *ws, const khip_operator *A, const khip_operator *At, const khip_operator *M,
                   const khip_operator *N, const double *b, const double *c, const khip_options *opts_in,
                   const khip_qmr_params *params_in) {
  KHIP_REQUIRE(ws && A && b, "qmr_solve: null argument");
  const khip_qmr_params prm = params_in ? *params_in : khip_qmr_default_params();
  BiLanczos<Qmr> L(ws, A, At, M, N, prm.Mt, prm.Nt, opts_in);
  khip_ctx *ctx = L.ctx;
  const khip_options &o = L.o;
  const int64_t n = L.n;
  QmrDevState &s = L.s;
  const double atol = tol_or_default(o.atol), rtol = tol_or_default(o.rtol);

  if (int rc = L.check("qmr", "System must be square")) return rc;                                         // :130-132
  if (o.verbose > 0) klogf(o.log_fd, "QMR: system of size %lld\n", (long long)n);                        // :134
  K(L.allocate_ts());                                                                                     // :151-152
  if (!c) c = b;
  const bool warm_start = ws->warm_start;
  ws->box.reset();
  double *x = L.pol.x = ws->x;
  L.pol.w1 = ws->w_prev;
  L.pol.w2 = ws->w_prev2;

  // set-up, the same primitives on every path (:164-228)
  const double *r0;
  K(L.residual(b, warm_start, &r0));
  K(khip_fill(ctx, n, x, 0.0));
  double rNorm0;
  K(khip_nrm2(ctx, n, r0, &rNorm0));
  if (L.history) ws->box.push(rNorm0);
  ws->box.path = o.fused ? 1 : 0;
  if (rNorm0 == 0) return L.end(1, "x is a zero-residual solution", warm_start, true);                   // :178-187
  L.itmax = o.itmax == 0 ? 2 * global_rows(ctx, A, n) : o.itmax;
  double cb;
  K(khip_dot(ctx, n, c, r0, &cb));
  if (cb == 0) return L.end(0, "Breakdown b\xe1\xb4\xb4" "c = 0", warm_start, true);                     // :194-203
  s.eps_tol = atol + rtol * rNorm0;
  if (o.verbose > 0) {
    klogf(o.log_fd, "%5s        %s     %s  %5s\n", "k", "\xce\xb1\xe2\x82\x96", "\xe2\x80\x96r\xe2\x82\x96\xe2\x80\x96", "timer");
    if (kdisplay(0, o.verbose)) Qmr::row(o, 0, cb, rNorm0, L.t0);
  }
  K(L.start(cb, r0, c));
  K(khip_fill(ctx, n, L.pol.w2, 0.0));
  K(khip_fill(ctx, n, L.pol.w1, 0.0));
  s.zbar = s.beta;
  K(khip_dot(ctx, n, L.r.v, L.r.v, &s.tau));                                                              // kdotr(n, vₖ, vₖ), :220
  s.rNorm = rNorm0;
  s.stop_seq = kSeqNever;
  s.solved = (rNorm0 <= s.eps_tol) ? 1 : 0;

  K(L.iterate());                                                                                         // :230-380

  const char *status = "unknown";                                                                         // :384-388
  if (L.tired) status = "maximum number of iterations exceeded";
  if (s.breakdown) status = "Breakdown \xe2\x9f\xa8u\xe2\x82\x96\xe2\x82\x8a\xe2\x82\x81,v\xe2\x82\x96\xe2\x82\x8a\xe2\x82\x81\xe2\x9f\xa9 = 0";
  if (s.solved) status = "solution good enough given atol and rtol";
  if (L.user_exit) status = "user-requested exit";
  if (L.overtimed) status = "time limit exceeded";
  return L.end(s.solved ? 1 : 0, status, warm_start);                                                     // :391-394
}

}  // extern "C"
