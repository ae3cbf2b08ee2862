// bilqr.cpp -- bilqr! (src/bilqr.jl:116-484) above the device primitives, with its fused gfx950 kernels.
//
// Real Float64.  ONE two-sided Lanczos process advances the BiLQ iterate of A x = b (with the BiCG transfer) and the QMR iterate of
// Aᴴ y = c.  Three loops, chosen as for bilq! and qmr! (khip_bilqr_last_path):
//   0  options.fused = 0: the reference's primitive sequence, one launch per k* call, one host sync per kdot / knorm / kdotr;
//   1  the host-driven loop on the fused kernels (a user operator, a callback or verbose > 0);
//   2  the device-resident loop (default; A and A' both CSR handles): the scalar recurrences and stopping tests run as the
//      epilogues of the three reductions of an iteration (bilqr_step_a/b/c, solver_device.hpp), iterations are enqueued ahead.
// One iteration on the fused paths, after q = A vₖ and p = A' uₖ, with both sides unsolved:
//   P1   q = fma(-γₖ, vₖ₋₁, q) ; p = fma(-βₖ, uₖ₋₁, p) ; uₖ.q                          (bilanczos.hpp)             56n bytes
//   P2   q = fma(-αₖ, vₖ, q) ; p = fma(-αₖ, uₖ, p) ; p.q                               (bilanczos.hpp)             48n bytes
//   P3   x = fma(ζₖ₋₁sₖ, vₖ, fma(ζₖ₋₁cₖ, d̅, x)) ; d̅ = fma(-cₖ, vₖ, sₖ d̅) ;
//        wₖ₋₁ = (uₖ₋₁ - λₖ₋₂ wₖ₋₂ - ϵₖ₋₃ wₖ₋₃) / δₖ₋₁ ; y = fma(ψₖ₋₁, wₖ₋₁, y) ;
//        vₖ₊₁ = q / βₖ₊₁ ; uₖ₊₁ = p / γₖ₊₁ ; vₖ.q ; q.q ; uₖ₊₁.uₖ₊₁                                                 120n bytes
//        reads  x, d̅, vₖ, q, p, uₖ₋₁, wₖ₋₃, wₖ₋₂, y (9) ; writes x, d̅, vₖ₊₁, uₖ₊₁, wₖ₋₁, y (6)
// 224n against 400n for the primitive sequence; a side that is solved drops its streams (primal: x, d̅ read and written, 32n; dual:
// uₖ₋₁, wₖ₋₃, wₖ₋₂, y read, wₖ₋₁, y written, 48n).  kcopy!(vₖ₋₁, vₖ), kcopy!(uₖ₋₁, uₖ) and @kswap!(wₖ₋₃, wₖ₋₂) become rotations of the
// buffers' roles (vₖ₊₁ and uₖ₊₁ are written where vₖ₋₁ and uₖ₋₁ were, wₖ₋₁ where wₖ₋₃ was).  Every elementwise value uses the
// expression of the primitive it replaces (fma for kaxpy!, fma(a, x, b y) for kaxpby!, a x for kscal!, x (1 / a) for kdiv!, / for
// kdivcopy!): the fused loops agree with the primitive sequence bit for bit on elementwise values and to the reductions' one ulp
// otherwise; loops 1 and 2 run the same kernels and the same scalar code and produce the same bits.
// The primal estimates need ⟨vₖ, q⟩ / βₖ₊₁ and ‖q‖ / βₖ₊₁ (:314-315, unlike bilq!, which reads vₖ₊₁): P3 sums vₖ.q and q.q and the
// scalar step divides, so that βₖ₊₁ = 0 gives the reference's NaN.  ‖uₖ₊₁‖² is the third sum: the scalar step keeps it and adds it to
// τ in the NEXT iteration (:398), as qmr! carries ‖vₖ₊₁‖²; ‖u₁‖² comes from one dot at set-up.  The finish kernel exists for 1, 2 and
// 4 sums: a fourth, zero, is published beside the three.
// This file owns P3, the set-up of both systems, the LQ and QR parts of a primitive iteration and the status strings; the loops are
// bilanczos.hpp's.
#include <string>

#include "bilanczos.hpp"   // P1, P2 and the driver of the three loops, shared with bilq.cpp and qmr.cpp

using namespace khip;

namespace khip {   // (named, not anonymous: stable kernel names in traces)

// ---------------------------------------------------------------------------------------------------------- kernels ----
// Each thread owns one VEC-vector of every stream; the odd tail element (VEC = 2, n odd) goes to thread 0 of block 0.
// Cache hints, the rule of bilq.cpp: a load is non-temporal when it is the LAST read of that data (x, d̅, y, wₖ₋₃, uₖ₋₁, q, p:
// overwritten here or by the next products); vₖ is read again by the next P1 (as vₖ₋₁) and wₖ₋₂ by the next P3 (as wₖ₋₃): they stay
// cacheable.  A store is non-temporal when nothing reads it before the next iteration's P3 (x, d̅, y, wₖ₋₁); vₖ₊₁ and uₖ₊₁ are read
// by the next products.

// wₖ₋₁ of one element (:363-381).  stage 2: kdivcopy!(w, u₁, δ₁).  stage 3: kaxpy!(1, uₖ₋₁, w₃) ; kaxpy!(-λ, w₂, w₃) ; kdiv!(w₃, δ).
// stage >= 4: kscal!(-ϵ, w₃) first.  (The +uₖ₋₁ axpy comes BEFORE the -λ axpy here, the other way round from qmr!.)
__device__ __forceinline__ double bilqr_w(int stage, double up, double w2, double w3, double ne, double nl, double dl, double idl) {
  if (stage == 2) return up / dl;
  double t = stage >= 4 ? ne * w3 : w3;
  t = fma(1.0, up, t);
  t = fma(nl, w2, t);
  return t * idl;
}

// P3 (:296-311, :361-392, :410-418).  primal (the primal system was unsolved when the iteration began): stage == 1 ? d̅ = v :
// (x = fma(ζs, v, fma(ζc, d̅, x)) ; d̅ = fma(-c, v, s d̅)) ; acc0 = v . q ; acc1 = q . q.  dual, from stage 2 on: w_out = wₖ₋₁
// (bilqr_w) ; y = fma(ψ, wₖ₋₁, y).  Always: pᴴq ≠ 0 ? (v_next = q / βₖ₊₁ ; u_next = p / γₖ₊₁) : (v_next = v ; u_next = u) ;
// acc2 = u_next . u_next.  The branches are uniform (device state and a kernel argument); a side that is off loads and stores
// nothing of its streams.  w_out is w2 at stage 2 and w3 afterwards.  u_next MAY BE u_prev's buffer (it is, in the loops below):
// every thread reads its elements of u_prev before it writes u_next.
template <int VEC, bool NT, bool COMP>
__global__ __launch_bounds__(kBlock) void bilqr_p3_kernel(int64_t n, const BilqrDevState *st, double *x, double *dbar, double *y,
                                                         const double *w3, const double *w2, double *w_out, const double *v,
                                                         const double *u, const double *u_prev, const double *q, const double *p,
                                                         double *v_next, double *u_next, int stage, RedArgs ra) {
  using T = typename VecT<VEC>::type;
  if (seq_skip(ra.stop_seq, ra.seq)) return;
  const double zc = st->zc, zs = st->zs, nc = st->neg_c, sn = st->sn, bn = st->beta_next, gn = st->gamma_next;
  const double ne = st->neg_eps3, nl = st->neg_lambda2, dl = st->delta, idl = st->inv_delta, psi = st->psi;
  const bool divide = st->pq != 0.0;
  const bool primal = !st->solved_primal;
  const bool dual = !st->solved_dual && stage >= 2;
  dd acc[4] = {dd{0.0, 0.0}, dd{0.0, 0.0}, dd{0.0, 0.0}, dd{0.0, 0.0}};
  const int64_t nvec = n / VEC;
  const int64_t i = lane_index();
  if (i < nvec) {
    T vv = {}, qv = {};
    if (primal || !divide) vv = ldg<false>(reinterpret_cast<const T *>(v) + i);       // v is the next iteration's v_prev
    if (primal || divide) qv = ldg<NT>(reinterpret_cast<const T *>(q) + i);
    if (primal) {
      T dv;
      if (stage == 1) {
        dv = vv;
      } else {
        const T xv = ldg<NT>(reinterpret_cast<const T *>(x) + i);
        const T dd_ = ldg<NT>(reinterpret_cast<const T *>(dbar) + i);
        T xo;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          vset(xo, e, fma(zs, vget(vv, e), fma(zc, vget(dd_, e), vget(xv, e))));
          vset(dv, e, fma(nc, vget(vv, e), sn * vget(dd_, e)));
        }
        stg<NT>(xo, reinterpret_cast<T *>(x) + i);
      }
      stg<NT>(dv, reinterpret_cast<T *>(dbar) + i);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        acc_prod<COMP>(acc[0], vget(vv, e), vget(qv, e));
        acc_prod<COMP>(acc[1], vget(qv, e), vget(qv, e));
      }
    }
    if (dual) {
      const T upv = ldg<NT>(reinterpret_cast<const T *>(u_prev) + i);   // overwritten below (u_next)
      const T yv = ldg<NT>(reinterpret_cast<const T *>(y) + i);
      T w3v = {}, w2v = {};
      if (stage >= 3) {
        w3v = ldg<NT>(reinterpret_cast<const T *>(w3) + i);
        w2v = ldg<false>(reinterpret_cast<const T *>(w2) + i);         // wₖ₋₂ is the next iteration's wₖ₋₃
      }
      T wo, yo;
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const double w = bilqr_w(stage, vget(upv, e), vget(w2v, e), vget(w3v, e), ne, nl, dl, idl);
        vset(wo, e, w);
        vset(yo, e, fma(psi, w, vget(yv, e)));
      }
      stg<NT>(wo, reinterpret_cast<T *>(w_out) + i);
      stg<NT>(yo, reinterpret_cast<T *>(y) + i);
    }
    T vo, uo;
    if (divide) {
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
    for (int e = 0; e < VEC; ++e) acc_prod<COMP>(acc[2], vget(uo, e), vget(uo, e));
    stg<false>(vo, reinterpret_cast<T *>(v_next) + i);                  // read by the next products
    stg<false>(uo, reinterpret_cast<T *>(u_next) + i);
  }
  if (VEC == 2 && owns_tail(n)) {
    const int64_t t = n - 1;
    const double ve = v[t], qe = q[t];
    if (primal) {
      if (stage == 1) {
        dbar[t] = ve;
      } else {
        const double de = dbar[t];
        x[t] = fma(zs, ve, fma(zc, de, x[t]));
        dbar[t] = fma(nc, ve, sn * de);
      }
      acc_prod<COMP>(acc[0], ve, qe);
      acc_prod<COMP>(acc[1], qe, qe);
    }
    if (dual) {
      const double w = bilqr_w(stage, u_prev[t], stage >= 3 ? w2[t] : 0.0, stage >= 3 ? w3[t] : 0.0, ne, nl, dl, idl);
      w_out[t] = w;
      y[t] = fma(psi, w, y[t]);
    }
    const double vo = divide ? qe / bn : ve;
    const double uo = divide ? p[t] / gn : u[t];
    v_next[t] = vo;
    u_next[t] = uo;
    acc_prod<COMP>(acc[2], uo, uo);
  }
  wave_publish<4>(acc, ra);
}

}  // namespace khip

namespace {

constexpr ScalarPathNT kScalarNT = ScalarPathNT::never;
constexpr int kP3Sums = 4;         // vₖ.q, q.q, uₖ₊₁.uₖ₊₁ and a zero: the finish kernel has no three-sum form

int launch_p3(khip_ctx *ctx, int64_t n, const BilqrDevState *st, double *x, double *dbar, double *y, const double *w3, const double *w2,
              double *w_out, const double *v, const double *u, const double *u_prev, const double *q, const double *p, double *v_next,
              double *u_next, int stage, int slot) {
  VecPlan L;
  KHIP_TRY(vec_plan(ctx, n, {x, dbar, y, w3, w2, w_out, v, u, u_prev, q, p, v_next, u_next}, &L, kP3Sums));
  RedArgs ra = make_red_args(ctx, slot);
  vec_dispatch<kScalarNT>(L, [&](auto V, auto N, auto C) {
    hipLaunchKernelGGL((bilqr_p3_kernel<V, N, C>), L.grid(), dim3(kBlock), 0, ctx->stream, n, st, x, dbar, y, w3, w2, w_out, v, u,
                       u_prev, q, p, v_next, u_next, stage, ra); });
  KHIP_CHECK_HIP(hipGetLastError());
  return launch_finish(ctx, L.waves(), kP3Sums, slot);
}

}  // namespace

struct khip_bilqr_workspace {
  khip_ctx *ctx;
  int64_t m, n;
  // by their CURRENT role: the fused loops rotate (v_prev, v), (u_prev, u) and (w_prev3, w_prev2)
  double *u_prev = nullptr, *u = nullptr, *q = nullptr, *v_prev = nullptr, *v = nullptr, *p = nullptr, *x = nullptr, *y = nullptr,
         *dbar = nullptr, *w_prev3 = nullptr, *w_prev2 = nullptr, *dx = nullptr, *dy = nullptr;
  Borrowed borrowed;                        // the caller's vectors (khip_bilqr_workspace_adopt*): never freed here
  bool warm_start = false;
  StatsBox box;                             // box.residuals: the primal history
  std::vector<double> residuals_dual;
  std::string status;                       // the full status: four of the reference's strings do not fit khip_stats.status
  int solved_primal = 0, solved_dual = 0;
  DeviceLoop<BilqrDevState, 3> loop;        // fused loops: device copy of the scalar state, pinned snapshots + staging, histories
};

namespace {

// uₖ₋₁, uₖ, q, vₖ₋₁, vₖ, p, x, y, d̅, wₖ₋₃, wₖ₋₂ come with the workspace; Δx, Δy stay empty until a warm start
// (src/krylov_workspaces.jl, BilqrWorkspace)
using W = khip_bilqr_workspace;
constexpr WsVec<W> kVectors[] = {{"u_prev", &W::u_prev, Core},   {"u", &W::u, Core},   {"q", &W::q, Core}, {"v_prev", &W::v_prev, Core},
                                 {"v", &W::v, Core},             {"p", &W::p, Core},   {"x", &W::x, Core}, {"y", &W::y, Core},
                                 {"dbar", &W::dbar, Core},       {"w_prev3", &W::w_prev3, Core},
                                 {"w_prev2", &W::w_prev2, Core}, {"dx", &W::dx, Lazy}, {"dy", &W::dy, Lazy}};

// "%7s" of the reference pads characters; ✗ ✗ ✗ ✗ is seven of them                                        (src/bilqr.jl:439-441)
const char *const kCrosses = "\xe2\x9c\x97 \xe2\x9c\x97 \xe2\x9c\x97 \xe2\x9c\x97";

// what bilqr! adds to the two-sided Lanczos driver (bilanczos.hpp)
struct Bilqr : BiLanczosPolicy<BilqrDevState, W> {
  static constexpr Epilogue kEpiA = EPI_BILQR_A, kEpiB = EPI_BILQR_B, kEpiC = EPI_BILQR_C;
  static constexpr int kP3Sums = ::kP3Sums;
  double *x, *dbar, *y, *w3, *w2;                                                      // wₖ₋₃, wₖ₋₂ by their current role
  bool primal = true, dual = true;                  // host-driven loops: the sides that were unsolved when the iteration began
  static void step_a(State &s, double uq) { bilqr_step_a(s, uq); }
  static void step_b(State &s, double pq, int64_t k) { bilqr_step_b(s, pq, k); }
  static void step_c(State &s, const double *sums, int64_t k) { bilqr_step_c(s, sums[0], std::sqrt(sums[1]), sums[2], k); }
  static bool stopped(const State &s) { return (s.solved_primal && s.solved_dual) || s.breakdown; }
  void begin_iteration(const State &s) { primal = !s.solved_primal; dual = !s.solved_dual; }
  int fused_start(khip_ctx *ctx, int64_t n, const BiLanczosRoles &r, State &s) { return khip_dot(ctx, n, r.u, r.u, &s.uu); }   // ‖u₁‖²
  // u_prev twice: read as uₖ₋₁ and written as uₖ₊₁
  int p3(khip_ctx *ctx, int64_t n, const State *dev, const BiLanczosRoles &r, int64_t k, int slot) const {
    return launch_p3(ctx, n, dev, x, dbar, y, w3, w2, k == 2 ? w2 : w3, r.v, r.u, r.u_prev, r.q, r.p, r.v_prev, r.u_prev,
                     k < 4 ? (int)k : 4, slot);
  }
  // wₖ₋₁ was written over wₖ₋₃ (src/bilqr.jl:383-386); enqueued ahead, a dual side that is solved no longer touches either buffer
  void rotate(int64_t k, bool host_driven) { if (k >= 3 && (dual || !host_driven)) std::swap(w3, w2); }
  void fix_after_device_loop(const State &s) { if (s.nhist_d >= 3 && (s.nhist_d & 1)) std::swap(w3, w2); }   // the dual block ran nhist_d times
  void store(W *ws) const { ws->w_prev3 = w3; ws->w_prev2 = w2; }
  static std::vector<double> *dual_history(W *ws) { return &ws->residuals_dual; }
  void push_history(W *ws, const State &s) const {                                     // :327, :402
    if (primal) ws->box.push(s.rNorm_lq);
    if (dual) ws->residuals_dual.push_back(s.sNorm);
  }
  void verbose_row(const khip_options &o, long long iter, const State &s, double t0) const {
    if (s.solved_primal && !s.solved_dual) klogf(o.log_fd, "%5lld  %s  %7.1e  %.2fs\n", iter, kCrosses, s.sNorm, now_s() - t0);
    if (!s.solved_primal && s.solved_dual) klogf(o.log_fd, "%5lld  %7.1e  %s  %.2fs\n", iter, s.rNorm_lq, kCrosses, now_s() - t0);
    if (!s.solved_primal && !s.solved_dual) klogf(o.log_fd, "%5lld  %7.1e  %7.1e  %.2fs\n", iter, s.rNorm_lq, s.sNorm, now_s() - t0);
  }
  // the LQ update with vₖ.q and ‖q‖, the QR update with ‖uₖ‖², both BEFORE the shift (src/bilqr.jl:296-418)
  int primitive_tail(BiLanczos<Bilqr> &L, int64_t k, double pq) {
    W *ws = L.ws;
    khip_ctx *ctx = L.ctx;
    const int64_t n = L.n;
    State &s = L.s;
    const BiLanczosRoles &r = L.r;
    double vq = 0.0, q_norm = 0.0;
    if (primal) {                                                                                         // :296-315
      if (k == 1) {
        K(khip_copy(ctx, n, dbar, r.v));
      } else {
        K(khip_axpy(ctx, n, s.zc, dbar, x));
        K(khip_axpy(ctx, n, s.zs, r.v, x));
        K(khip_axpby(ctx, n, s.neg_c, r.v, s.sn, dbar));
      }
      K(khip_dot(ctx, n, r.v, r.q, &vq));
      K(khip_nrm2(ctx, n, r.q, &q_norm));
    }
    if (dual) {                                                                                           // :361-398
      double *w = nullptr;
      if (k == 2) {
        w = w2;
        K(khip_divcopy(ctx, n, w, r.u_prev, s.delta));
      }
      if (k >= 3) {
        w = w3;
        if (k >= 4) K(khip_scal(ctx, n, s.neg_eps3, w));
        K(khip_axpy(ctx, n, 1.0, r.u_prev, w));
        K(khip_axpy(ctx, n, s.neg_lambda2, w2, w));
        K(khip_div(ctx, n, w, s.delta));
        rotate(k, true);                                                                                  // @kswap!(wₖ₋₃, wₖ₋₂)
      }
      if (k >= 2) K(khip_axpy(ctx, n, s.psi, w, y));
      K(khip_dot(ctx, n, r.u, r.u, &s.uu));                                                               // kdotr(n, uₖ, uₖ), :398
    }
    K(L.shift(pq));                                                                                       // :410-418
    bilqr_step_c(s, vq, q_norm, 0.0, k);            // ‖uₖ₊₁‖² is not carried here: the next iteration takes its own kdotr
    return KHIP_OK;
  }
};

// the first bytes of `full` that fit `cap` (with the terminator), cut at a UTF-8 character boundary
void copy_status(char *dst, size_t cap, const std::string &full) {
  size_t len = std::min(full.size(), cap - 1);
  while (len > 0 && len < full.size() && (static_cast<unsigned char>(full[len]) & 0xC0) == 0x80) --len;
  memcpy(dst, full.data(), len);
  dst[len] = 0;
}

// the termination status (:451-469); XL / XC: "xᴸ" / "xᶜ"
#define XL "x\xe1\xb4\xb8"
#define XC "x\xe1\xb6\x9c"
const char *status_of(const BilqrDevState &s, bool tired, bool user_exit, bool overtimed) {
  const char *status = "unknown";
  if (tired) status = "maximum number of iterations exceeded";
  if (s.breakdown) status = "Breakdown \xe2\x9f\xa8u\xe2\x82\x96\xe2\x82\x8a\xe2\x82\x81,v\xe2\x82\x96\xe2\x82\x8a\xe2\x82\x81\xe2\x9f\xa9 = 0";
  if (s.solved_lq_tol && !s.solved_dual) status = "Only the primal solution " XL " is good enough given atol and rtol";
  if (s.solved_cg_tol && !s.solved_dual) status = "Only the primal solution " XC " is good enough given atol and rtol";
  if (!s.solved_primal && s.solved_qr_tol) status = "Only the dual solution t is good enough given atol and rtol";
  if (s.solved_lq_tol && s.solved_qr_tol) status = "Both primal and dual solutions (" XL ", t) are good enough given atol and rtol";
  if (s.solved_cg_tol && s.solved_qr_tol) status = "Both primal and dual solutions (" XC ", t) are good enough given atol and rtol";
  if (s.solved_lq_mach && !s.solved_dual) status = "Only found approximate zero-residual primal solution " XL;
  if (s.solved_cg_mach && !s.solved_dual) status = "Only found approximate zero-residual primal solution " XC;
  if (!s.solved_primal && s.solved_qr_mach) status = "Only found approximate zero-residual dual solution t";
  if (s.solved_lq_mach && s.solved_qr_mach) status = "Found approximate zero-residual primal and dual solutions (" XL ", t)";
  if (s.solved_cg_mach && s.solved_qr_mach) status = "Found approximate zero-residual primal and dual solutions (" XC ", t)";
  if (s.solved_lq_mach && s.solved_qr_tol)
    status = "Found approximate zero-residual primal solutions " XL " and a dual solution t good enough given atol and rtol";
  if (s.solved_cg_mach && s.solved_qr_tol)
    status = "Found approximate zero-residual primal solutions " XC " and a dual solution t good enough given atol and rtol";
  if (s.solved_lq_tol && s.solved_qr_mach)
    status = "Found a primal solution " XL " good enough given atol and rtol and an approximate zero-residual dual solutions t";
  if (s.solved_cg_tol && s.solved_qr_mach)
    status = "Found a primal solution " XC " good enough given atol and rtol and an approximate zero-residual dual solutions t";
  if (user_exit) status = "user-requested exit";
  if (overtimed) status = "time limit exceeded";
  return status;
}
#undef XL
#undef XC

}  // namespace

extern "C" {

khip_bilqr_params khip_bilqr_default_params(void) {
  khip_bilqr_params p;
  p.transfer_to_bicg = 1;
  return p;
}

int khip_bilqr_workspace_create(khip_ctx *ctx, int64_t m, int64_t n, khip_bilqr_workspace **out) {
  KHIP_REQUIRE(ctx && out && m >= 0 && n >= 0, "bilqr_workspace_create: bad argument");
  KHIP_REQUIRE(m == n, "Systems must be square");
  khip_bilqr_workspace *ws = new khip_bilqr_workspace();
  ws->ctx = ctx; ws->m = m; ws->n = n;
  const int rc = ws_create_core(ws, kVectors);
  if (rc) { khip_bilqr_workspace_destroy(ws); return rc; }
  *out = ws;
  return KHIP_OK;
}

int khip_bilqr_workspace_adopt(khip_ctx *ctx, int64_t m, int64_t n, double *u_prev, double *u, double *q, double *v_prev, double *v,
                               double *p, double *x, double *y, double *dbar, double *w_prev3, double *w_prev2,
                               khip_bilqr_workspace **out) {
  KHIP_REQUIRE(ctx && out && m >= 0 && n >= 0, "bilqr_workspace_adopt: bad argument");
  KHIP_REQUIRE(m == n, "Systems must be square");
  khip_bilqr_workspace *ws = new khip_bilqr_workspace();
  ws->ctx = ctx; ws->m = m; ws->n = n;
  const int rc = ws_adopt_core(ws, kVectors, "bilqr_workspace_adopt", {u_prev, u, q, v_prev, v, p, x, y, dbar, w_prev3, w_prev2});
  if (rc) { delete ws; return rc; }
  *out = ws;
  return KHIP_OK;
}

int khip_bilqr_workspace_adopt_vector(khip_bilqr_workspace *ws, const char *name, double *ptr) {
  return ws_adopt_vector(ws, kVectors, "bilqr_workspace_adopt_vector", name, ptr);
}

int khip_bilqr_workspace_destroy(khip_bilqr_workspace *ws) {
  if (!ws) return KHIP_OK;
  ws_free_vectors(ws, kVectors);
  ws->loop.release();
  delete ws;
  return KHIP_OK;
}

int khip_bilqr_warm_start(khip_bilqr_workspace *ws, const double *x0, const double *y0) {
  KHIP_REQUIRE(ws && x0 && y0, "bilqr_warm_start: x0 and y0 are both required");
  if (!ws->dx) KHIP_TRY(alloc_vec(ws->ctx, ws->n, &ws->dx));
  if (!ws->dy) KHIP_TRY(alloc_vec(ws->ctx, ws->n, &ws->dy));
  if (x0 != ws->dx) KHIP_TRY(khip_copy(ws->ctx, ws->n, ws->dx, x0));
  if (y0 != ws->dy) KHIP_TRY(khip_copy(ws->ctx, ws->n, ws->dy, y0));
  ws->warm_start = true;
  return KHIP_OK;
}

double *khip_bilqr_solution_x(khip_bilqr_workspace *ws) { return ws ? ws->x : nullptr; }
double *khip_bilqr_solution_y(khip_bilqr_workspace *ws) { return ws ? ws->y : nullptr; }
const khip_stats *khip_bilqr_stats(khip_bilqr_workspace *ws) { return ws ? &ws->box.st : nullptr; }
int khip_bilqr_adjoint_stats(khip_bilqr_workspace *ws, int *solved_primal, int *solved_dual, const double **residuals_primal,
                             int *nprimal, const double **residuals_dual, int *ndual, const char **status) {
  KHIP_REQUIRE(ws, "bilqr_adjoint_stats: null workspace");
  if (solved_primal) *solved_primal = ws->solved_primal;
  if (solved_dual) *solved_dual = ws->solved_dual;
  if (residuals_primal) *residuals_primal = ws->box.residuals.empty() ? nullptr : ws->box.residuals.data();
  if (nprimal) *nprimal = (int)ws->box.residuals.size();
  if (residuals_dual) *residuals_dual = ws->residuals_dual.empty() ? nullptr : ws->residuals_dual.data();
  if (ndual) *ndual = (int)ws->residuals_dual.size();
  if (status) *status = ws->status.c_str();
  return KHIP_OK;
}
// test-only export (include/krylov_hip_test.h): the status the flags of `mask` end in, whole (*full, a literal) and as
// khip_stats.status holds it (cut96).  Bits: 0 lq_tol, 1 lq_mach, 2 cg_tol, 3 cg_mach, 4 qr_tol, 5 qr_mach, 6 tired, 7 breakdown,
// 8 user exit, 9 overtimed.  Host only.
int khip_test_bilqr_status(int mask, char *cut96, const char **full) {
  KHIP_REQUIRE(cut96 && full, "test_bilqr_status: null argument");
  BilqrDevState s;
  memset(&s, 0, sizeof(s));
  s.solved_lq_tol = mask & 1; s.solved_lq_mach = (mask >> 1) & 1; s.solved_cg_tol = (mask >> 2) & 1; s.solved_cg_mach = (mask >> 3) & 1;
  s.solved_qr_tol = (mask >> 4) & 1; s.solved_qr_mach = (mask >> 5) & 1; s.breakdown = (mask >> 7) & 1;
  s.solved_lq = s.solved_lq_tol || s.solved_lq_mach;
  s.solved_cg = s.solved_cg_tol || s.solved_cg_mach;
  s.solved_primal = s.solved_lq || s.solved_cg;
  s.solved_dual = s.solved_qr_tol || s.solved_qr_mach;
  *full = status_of(s, (mask >> 6) & 1, (mask >> 8) & 1, (mask >> 9) & 1);
  copy_status(cut96, 96, *full);
  return KHIP_OK;
}
int khip_bilqr_last_path(khip_bilqr_workspace *ws) { return ws ? ws->box.path : -1; }
double *khip_bilqr_vector(khip_bilqr_workspace *ws, const char *name) { return ws_vector(ws, kVectors, name); }
size_t khip_bilqr_workspace_bytes(khip_bilqr_workspace *ws) { return ws_bytes(ws, kVectors); }

int khip_bilqr_solve(khip_bilqr_workspace *ws, const khip_operator *A, const khip_operator *At, const double *b, const double *c,
                     const khip_options *opts_in, const khip_bilqr_params *params_in) {
  KHIP_REQUIRE(ws && A && b, "bilqr_solve: null argument");
  const khip_bilqr_params prm = params_in ? *params_in : khip_bilqr_default_params();
  BiLanczos<Bilqr> L(ws, A, At, nullptr, nullptr, nullptr, nullptr, opts_in);          // no M, no N
  khip_ctx *ctx = L.ctx;
  const khip_options &o = L.o;
  const int64_t n = L.n;
  BilqrDevState &s = L.s;
  khip_stats *st = &ws->box.st;
  const double atol = tol_or_default(o.atol), rtol = tol_or_default(o.rtol);

  if (int rc = L.check("bilqr", "Systems must be square",                                                  // :122-123
                       c ? nullptr : "bilqr_solve: c (the right-hand side of the dual system) is required"))
    return rc;
  if (o.verbose > 0) klogf(o.log_fd, "BILQR: systems of size %lld\n", (long long)n);                     // :127
  const bool warm_start = ws->warm_start;
  ws->box.reset();
  ws->residuals_dual.clear();
  ws->status = "unknown";
  ws->solved_primal = ws->solved_dual = 0;
  double *x = L.pol.x = ws->x, *y = L.pol.y = ws->y, *dbar = L.pol.dbar = ws->dbar;
  L.pol.w3 = ws->w_prev3;
  L.pol.w2 = ws->w_prev2;
  auto finish = [&](const char *status, int solved_primal, int solved_dual) {
    ws->status = status;
    ws->solved_primal = solved_primal;
    ws->solved_dual = solved_dual;
    st->solved = (solved_primal && solved_dual) ? 1 : 0;
    st->inconsistent = 0;
    copy_status(st->status, sizeof(st->status), ws->status);
    L.finish();
  };

  // set-up, the same primitives on every path (:144-217)
  const double *r0 = b, *s0 = c;
  if (warm_start) {
    K(apply_op(ctx, A, ws->dx, L.r.q));
    K(khip_axpby(ctx, n, 1.0, b, -1.0, L.r.q));
    K(apply_op(ctx, At, ws->dy, L.r.p));
    K(khip_axpby(ctx, n, 1.0, c, -1.0, L.r.p));
    r0 = L.r.q;
    s0 = L.r.p;
  }
  K(khip_fill(ctx, n, x, 0.0));
  double bNorm, cNorm;
  K(khip_nrm2(ctx, n, r0, &bNorm));
  K(khip_fill(ctx, n, y, 0.0));
  K(khip_nrm2(ctx, n, s0, &cNorm));
  L.itmax = o.itmax == 0 ? 2 * global_rows(ctx, A, n) : o.itmax;
  if (L.history) {
    ws->box.push(bNorm);
    ws->residuals_dual.push_back(cNorm);
  }
  s.bNorm = bNorm;
  s.eps_L = atol + rtol * bNorm;
  s.eps_Q = atol + rtol * cNorm;
  s.sNorm = cNorm;
  s.rNorm_lq = bNorm;
  ws->box.path = o.fused ? 1 : 0;
  if (o.verbose > 0) {
    klogf(o.log_fd, "%5s  %s  %s  %5s\n", "k", "   \xe2\x80\x96r\xe2\x82\x96\xe2\x80\x96", "   \xe2\x80\x96s\xe2\x82\x96\xe2\x80\x96", "timer");
    if (kdisplay(0, o.verbose)) klogf(o.log_fd, "%5d  %7.1e  %7.1e  %.2fs\n", 0, bNorm, cNorm, now_s() - L.t0);
  }
  double cb;
  K(khip_dot(ctx, n, s0, r0, &cb));
  if (cb == 0) {                                                                                         // :174-184
    st->niter = 0;
    if (warm_start) {
      K(khip_axpy(ctx, n, 1.0, ws->dx, x));
      K(khip_axpy(ctx, n, 1.0, ws->dy, y));
    }
    finish("Breakdown b\xe1\xb4\xb4" "c = 0", 0, 0);
    return KHIP_OK;
  }
  K(L.start(cb, r0, s0));
  s.cs = s.cs_prev = -1.0;
  K(khip_fill(ctx, n, dbar, 0.0));
  s.norm_v = bNorm / s.beta;
  K(khip_fill(ctx, n, L.pol.w3, 0.0));
  K(khip_fill(ctx, n, L.pol.w2, 0.0));
  s.transfer_to_bicg = prm.transfer_to_bicg ? 1 : 0;
  s.stop_seq = kSeqNever;
  s.solved_lq = (bNorm == 0) ? 1 : 0;                                                                    // :207-212
  s.solved_primal = s.solved_lq;
  s.solved_dual = (cNorm == 0) ? 1 : 0;

  K(L.iterate());                                                                                         // :219-442

  if (s.solved_cg) K(khip_axpy(ctx, n, s.zbar, dbar, x));                                                // :447-449
  const char *status = status_of(s, L.tired, L.user_exit, L.overtimed);
  if (warm_start) {                                                                                       // :472-473
    K(khip_axpy(ctx, n, 1.0, ws->dx, x));
    K(khip_axpy(ctx, n, 1.0, ws->dy, y));
  }
  st->niter = (int)L.iter;
  finish(status, s.solved_primal ? 1 : 0, s.solved_dual ? 1 : 0);
  return KHIP_OK;
}

}  // extern "C"
