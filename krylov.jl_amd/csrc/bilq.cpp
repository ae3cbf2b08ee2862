// bilq.cpp -- bilq! (src/bilq.jl:118-407) above the device primitives, with its fused gfx950 kernels.
//
// Real Float64.  Three loops, chosen as for minres! (khip_bilq_last_path):
//   0  options.fused = 0: the reference's primitive sequence, one launch per k* call, one host sync per kdot / knorm;
//   1  the host-driven loop on the fused kernels below (with M or N, a user operator, a callback or verbose > 0);
//   2  the device-resident loop (default; A and A' both CSR handles): the scalar recurrences and stopping tests run as the
//      epilogues of the three reductions of an iteration (bilq_step_a/b/c, solver_device.hpp), iterations are enqueued ahead.
// One iteration with M = N = I on the fused paths, after q = A vₖ and p = A' uₖ:
//   P1   q = fma(-γₖ, vₖ₋₁, q) ; p = fma(-βₖ, uₖ₋₁, p) ; uₖ.q                                         56n bytes
//   P2   q = fma(-αₖ, vₖ, q) ; p = fma(-αₖ, uₖ, p) ; p.q                                              48n bytes
//   P3   x = fma(ζₖ₋₁sₖ, vₖ, fma(ζₖ₋₁cₖ, d̅, x)) ; d̅ = fma(-cₖ, vₖ, sₖ d̅) ; vₖ₊₁ = q / βₖ₊₁ ; uₖ₊₁ = p / γₖ₊₁ ;
//        vₖ.vₖ₊₁ ; vₖ₊₁.vₖ₊₁                                                                           72n bytes
// against 288n for the primitive sequence; kcopy!(vₖ₋₁, vₖ) and kcopy!(uₖ₋₁, uₖ) become a rotation of the buffers' roles (vₖ₊₁ is
// written where vₖ₋₁ was).  Every elementwise value uses the expression of the primitive it replaces (fma for kaxpy!, fma(a, x, b y)
// for kaxpby!, / for kdivcopy!): the fused loops agree with the primitive sequence bit for bit on elementwise values and to the
// reductions' one ulp otherwise; loops 1 and 2 run the same kernels and the same scalar code and produce the same bits.
// This file owns P3, the set-up scalars, the LQ part of a primitive iteration and the status strings; the loops are bilanczos.hpp's.
#include "bilanczos.hpp"   // P1, P2 and the driver of the three loops, shared with qmr.cpp and bilqr.cpp

using namespace khip;

namespace khip {   // (named, not anonymous: stable kernel names in traces)

// ---------------------------------------------------------------------------------------------------------- kernels ----
// (P1 and P2: bilanczos.hpp.)
// Each thread owns one VEC-vector of every stream; the odd tail element (VEC = 2, n odd) goes to thread 0 of block 0.
// Cache hints, one rule: a load is non-temporal when it is the LAST read of that data (the vector is dead or overwritten
// afterwards: v_prev, u_prev, q, p, x, d̅); vₖ and uₖ are read again up to the next iteration's P1 (as vₖ₋₁, uₖ₋₁) and stay
// cacheable.  A store is non-temporal when nothing reads it before the next iteration's P3 (x, d̅).

// P3: first ? d̅ = v : (x = fma(ζs, v, fma(ζc, d̅, x)) ; d̅ = fma(-c, v, s d̅)) ; pᴴq ≠ 0 ? (v_next = q / βₖ₊₁ ; u_next = p / γₖ₊₁)
// : (v_next = v ; u_next = u) ; acc = (v . v_next, v_next . v_next)                    (:310-335)
template <int VEC, bool NT, bool COMP>
__global__ __launch_bounds__(kBlock) void bilq_p3_kernel(int64_t n, const BilqDevState *st, double *x, double *dbar, const double *v,
                                                        const double *u, const double *q, const double *p, double *v_next,
                                                        double *u_next, int first, RedArgs ra) {
  using T = typename VecT<VEC>::type;
  if (seq_skip(ra.stop_seq, ra.seq)) return;
  const double zc = st->zc, zs = st->zs, nc = st->neg_c, sn = st->sn, bn = st->beta_next, gn = st->gamma_next;
  const bool divide = st->pq != 0.0;
  dd acc[2] = {dd{0.0, 0.0}, dd{0.0, 0.0}};
  const int64_t nvec = n / VEC;
  const int64_t i = lane_index();
  if (i < nvec) {
    const T vv = ldg<false>(reinterpret_cast<const T *>(v) + i);       // v is the next iteration's v_prev
    T xo = {}, dv;
    if (first) {
      dv = vv;
    } else {
      const T xv = ldg<NT>(reinterpret_cast<const T *>(x) + i);
      const T dd_ = ldg<NT>(reinterpret_cast<const T *>(dbar) + i);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        vset(xo, e, fma(zs, vget(vv, e), fma(zc, vget(dd_, e), vget(xv, e))));
        vset(dv, e, fma(nc, vget(vv, e), sn * vget(dd_, e)));
      }
      stg<NT>(xo, reinterpret_cast<T *>(x) + i);
    }
    stg<NT>(dv, reinterpret_cast<T *>(dbar) + i);
    T vo, uo;
    if (divide) {
      const T qv = ldg<NT>(reinterpret_cast<const T *>(q) + i);
      const T pv = ldg<NT>(reinterpret_cast<const T *>(p) + i);
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
    for (int e = 0; e < VEC; ++e) {
      acc_prod<COMP>(acc[0], vget(vv, e), vget(vo, e));
      acc_prod<COMP>(acc[1], vget(vo, e), vget(vo, e));
    }
    stg<false>(vo, reinterpret_cast<T *>(v_next) + i);                  // read by the next products
    stg<false>(uo, reinterpret_cast<T *>(u_next) + i);
  }
  if (VEC == 2 && owns_tail(n)) {
    const int64_t t = n - 1;
    const double ve = v[t];
    if (first) {
      dbar[t] = ve;
    } else {
      const double de = dbar[t];
      x[t] = fma(zs, ve, fma(zc, de, x[t]));
      dbar[t] = fma(nc, ve, sn * de);
    }
    const double vo = divide ? q[t] / bn : ve;
    const double uo = divide ? p[t] / gn : u[t];
    v_next[t] = vo;
    u_next[t] = uo;
    acc_prod<COMP>(acc[0], ve, vo);
    acc_prod<COMP>(acc[1], vo, vo);
  }
  wave_publish<2>(acc, ra);
}

}  // namespace khip

namespace {

constexpr ScalarPathNT kScalarNT = ScalarPathNT::never;

int launch_p3(khip_ctx *ctx, int64_t n, const BilqDevState *st, double *x, double *dbar, const double *v, const double *u,
              const double *q, const double *p, double *v_next, double *u_next, bool first, int slot) {
  VecPlan L;
  KHIP_TRY(vec_plan(ctx, n, {x, dbar, v, u, q, p, v_next, u_next}, &L, 2));
  RedArgs ra = make_red_args(ctx, slot);
  vec_dispatch<kScalarNT>(L, [&](auto V, auto N, auto C) {
    hipLaunchKernelGGL((bilq_p3_kernel<V, N, C>), L.grid(), dim3(kBlock), 0, ctx->stream, n, st, x, dbar, v, u, q, p, v_next, u_next,
                       first ? 1 : 0, ra); });
  KHIP_CHECK_HIP(hipGetLastError());
  return launch_finish(ctx, L.waves(), 2, slot);
}

}  // namespace

struct khip_bilq_workspace {
  khip_ctx *ctx;
  int64_t m, n;
  // by their CURRENT role: the fused loops rotate (v_prev, v) and (u_prev, u)
  double *u_prev = nullptr, *u = nullptr, *q = nullptr, *v_prev = nullptr, *v = nullptr, *p = nullptr, *x = nullptr, *dbar = nullptr,
         *dx = nullptr, *t = nullptr, *s = nullptr;
  Borrowed borrowed;                        // the caller's vectors (khip_bilq_workspace_adopt*): never freed here
  bool warm_start = false;
  StatsBox box;
  DeviceLoop<BilqDevState, 3> loop;         // fused loops: device copy of the scalar state, pinned snapshots + staging, history
};

namespace {

// uₖ₋₁, uₖ, q, vₖ₋₁, vₖ, p, x, d̅ come with the workspace; Δx, t, s stay empty until needed (src/krylov_workspaces.jl, BilqWorkspace)
using W = khip_bilq_workspace;
constexpr WsVec<W> kVectors[] = {{"u_prev", &W::u_prev, Core}, {"u", &W::u, Core}, {"q", &W::q, Core}, {"v_prev", &W::v_prev, Core},
                                 {"v", &W::v, Core},           {"p", &W::p, Core}, {"x", &W::x, Core}, {"dbar", &W::dbar, Core},
                                 {"dx", &W::dx, Lazy},         {"t", &W::t, Lazy}, {"s", &W::s, Lazy}};

// what bilq! adds to the two-sided Lanczos driver (bilanczos.hpp)
struct Bilq : BiLanczosPolicy<BilqDevState, W> {
  static constexpr Epilogue kEpiA = EPI_BILQ_A, kEpiB = EPI_BILQ_B, kEpiC = EPI_BILQ_C;
  static constexpr int kP3Sums = 2;                                                    // vₖ.vₖ₊₁, vₖ₊₁.vₖ₊₁
  double *x, *dbar;
  static void step_a(State &s, double uq) { bilq_step_a(s, uq); }
  static void step_b(State &s, double pq, int64_t k) { bilq_step_b(s, pq, k); }
  static void step_c(State &s, const double *sums, int64_t k) { bilq_step_c(s, sums[0], std::sqrt(sums[1]), k); }
  static bool stopped(const State &s) { return s.solved_lq || s.solved_cg || s.breakdown; }
  int p3(khip_ctx *ctx, int64_t n, const State *dev, const BiLanczosRoles &r, int64_t k, int slot) const {
    return launch_p3(ctx, n, dev, x, dbar, r.v, r.u, r.q, r.p, r.v_prev, r.u_prev, k == 1, slot);
  }
  void push_history(W *ws, const State &s) const { ws->box.push(s.rNorm_lq); }
  static void row(const khip_options &o, long long iter, double alpha, double rNorm, double t0) {   // src/bilq.jl:201, :374
    klogf(o.log_fd, "%5lld  %8.1e  %7.1e  %.2fs\n", iter, alpha, rNorm, now_s() - t0);
  }
  void verbose_row(const khip_options &o, long long k, const State &s, double t0) const { row(o, k, s.alpha, s.rNorm_lq, t0); }
  // the LQ update, the shift, then vₖ.vₖ₊₁ and ‖vₖ₊₁‖ on the shifted vectors (src/bilq.jl:310-345)
  int primitive_tail(BiLanczos<Bilq> &L, int64_t k, double pq) const {
    W *ws = L.ws;
    khip_ctx *ctx = L.ctx;
    const int64_t n = L.n;
    State &s = L.s;
    if (k == 1) {
      K(khip_copy(ctx, n, dbar, L.r.v));
    } else {
      K(khip_axpy(ctx, n, s.zc, dbar, x));
      K(khip_axpy(ctx, n, s.zs, L.r.v, x));
      K(khip_axpby(ctx, n, s.neg_c, L.r.v, s.sn, dbar));
    }
    K(L.shift(pq));
    double vv, norm_next;
    K(khip_dot(ctx, n, L.r.v_prev, L.r.v, &vv));
    K(khip_nrm2(ctx, n, L.r.v, &norm_next));
    bilq_step_c(s, vv, norm_next, k);
    return KHIP_OK;
  }
};

}  // namespace

extern "C" {

khip_bilq_params khip_bilq_default_params(void) {
  khip_bilq_params p;
  p.transfer_to_bicg = 1;
  p.Mt = nullptr;
  p.Nt = nullptr;
  return p;
}

int khip_bilq_workspace_create(khip_ctx *ctx, int64_t m, int64_t n, khip_bilq_workspace **out) {
  KHIP_REQUIRE(ctx && out && m >= 0 && n >= 0, "bilq_workspace_create: bad argument");
  KHIP_REQUIRE(m == n, "System must be square");
  khip_bilq_workspace *ws = new khip_bilq_workspace();
  ws->ctx = ctx; ws->m = m; ws->n = n;
  const int rc = ws_create_core(ws, kVectors);
  if (rc) { khip_bilq_workspace_destroy(ws); return rc; }
  *out = ws;
  return KHIP_OK;
}

int khip_bilq_workspace_adopt(khip_ctx *ctx, int64_t m, int64_t n, double *u_prev, double *u, double *q, double *v_prev, double *v,
                              double *p, double *x, double *dbar, khip_bilq_workspace **out) {
  KHIP_REQUIRE(ctx && out && m >= 0 && n >= 0, "bilq_workspace_adopt: bad argument");
  KHIP_REQUIRE(m == n, "System must be square");
  khip_bilq_workspace *ws = new khip_bilq_workspace();
  ws->ctx = ctx; ws->m = m; ws->n = n;
  const int rc = ws_adopt_core(ws, kVectors, "bilq_workspace_adopt", {u_prev, u, q, v_prev, v, p, x, dbar});
  if (rc) { delete ws; return rc; }
  *out = ws;
  return KHIP_OK;
}

int khip_bilq_workspace_adopt_vector(khip_bilq_workspace *ws, const char *name, double *ptr) {
  return ws_adopt_vector(ws, kVectors, "bilq_workspace_adopt_vector", name, ptr);
}

int khip_bilq_workspace_destroy(khip_bilq_workspace *ws) {
  if (!ws) return KHIP_OK;
  ws_free_vectors(ws, kVectors);
  ws->loop.release();
  delete ws;
  return KHIP_OK;
}

int khip_bilq_warm_start(khip_bilq_workspace *ws, const double *x0) { return ws_warm_start(ws, kVectors, x0, "bilq_warm_start"); }
double *khip_bilq_solution(khip_bilq_workspace *ws) { return ws ? ws->x : nullptr; }
const khip_stats *khip_bilq_stats(khip_bilq_workspace *ws) { return ws ? &ws->box.st : nullptr; }
int khip_bilq_last_path(khip_bilq_workspace *ws) { return ws ? ws->box.path : -1; }
double *khip_bilq_vector(khip_bilq_workspace *ws, const char *name) { return ws_vector(ws, kVectors, name); }
size_t khip_bilq_workspace_bytes(khip_bilq_workspace *ws) { return ws_bytes(ws, kVectors); }

int khip_bilq_solve(khip_bilq_workspace *ws, const khip_operator *A, const khip_operator *At, const khip_operator *M,
                    const khip_operator *N, const double *b, const double *c, const khip_options *opts_in,
                    const khip_bilq_params *params_in) {
  KHIP_REQUIRE(ws && A && b, "bilq_solve: null argument");
  const khip_bilq_params prm = params_in ? *params_in : khip_bilq_default_params();
  BiLanczos<Bilq> L(ws, A, At, M, N, prm.Mt, prm.Nt, opts_in);
  khip_ctx *ctx = L.ctx;
  const khip_options &o = L.o;
  const int64_t n = L.n;
  BilqDevState &s = L.s;
  const double atol = tol_or_default(o.atol), rtol = tol_or_default(o.rtol);

  if (int rc = L.check("bilq", "System must be square")) return rc;                                        // :124-126
  if (o.verbose > 0) klogf(o.log_fd, "BILQ: system of size %lld\n", (long long)n);                       // :128
  K(L.allocate_ts());                                                                                     // :145-146
  if (!c) c = b;
  const bool warm_start = ws->warm_start;
  ws->box.reset();
  double *x = L.pol.x = ws->x, *dbar = L.pol.dbar = ws->dbar;

  // set-up, the same primitives on every path (:158-215)
  const double *r0;
  K(L.residual(b, warm_start, &r0));
  K(khip_fill(ctx, n, x, 0.0));
  double bNorm;
  K(khip_nrm2(ctx, n, r0, &bNorm));
  if (L.history) ws->box.push(bNorm);
  ws->box.path = o.fused ? 1 : 0;
  if (bNorm == 0) return L.end(1, "x is a zero-residual solution", warm_start, true);                    // :172-181
  L.itmax = o.itmax == 0 ? 2 * global_rows(ctx, A, n) : o.itmax;
  double cb;
  K(khip_dot(ctx, n, c, r0, &cb));
  if (cb == 0) return L.end(0, "Breakdown b\xe1\xb4\xb4" "c = 0", warm_start, true);                     // :188-197
  s.bNorm = bNorm;
  s.eps_tol = atol + rtol * bNorm;
  if (o.verbose > 0) {
    klogf(o.log_fd, "%5s        %s     %s  %5s\n", "k", "\xce\xb1\xe2\x82\x96", "\xe2\x80\x96r\xe2\x82\x96\xe2\x80\x96", "timer");
    if (kdisplay(0, o.verbose)) Bilq::row(o, 0, cb, bNorm, L.t0);
  }
  K(L.start(cb, r0, c));
  s.cs = s.cs_prev = -1.0;
  K(khip_fill(ctx, n, dbar, 0.0));
  s.norm_v = bNorm / s.beta;
  s.transfer_to_bicg = prm.transfer_to_bicg ? 1 : 0;
  s.stop_seq = kSeqNever;
  s.solved_lq = (bNorm <= s.eps_tol) ? 1 : 0;

  K(L.iterate());                                                                                         // :226-375

  if (s.solved_cg) K(khip_axpy(ctx, n, s.zbar, dbar, x));                                                // :380-382
  const char *status = "unknown";                                                                         // :385-390
  if (L.tired) status = "maximum number of iterations exceeded";
  if (s.breakdown) status = "Breakdown \xe2\x9f\xa8u\xe2\x82\x96\xe2\x82\x8a\xe2\x82\x81,v\xe2\x82\x96\xe2\x82\x8a\xe2\x82\x81\xe2\x9f\xa9 = 0";
  if (s.solved_lq) status = "solution x\xe1\xb4\xb8 good enough given atol and rtol";
  if (s.solved_cg) status = "solution x\xe1\xb6\x9c good enough given atol and rtol";
  if (L.user_exit) status = "user-requested exit";
  if (L.overtimed) status = "time limit exceeded";
  return L.end((s.solved_lq || s.solved_cg) ? 1 : 0, status, warm_start);                                // :393-396
}

}  // extern "C"
