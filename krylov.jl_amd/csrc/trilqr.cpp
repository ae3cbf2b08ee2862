// trilqr.cpp -- trilqr! (src/trilqr.jl:115-460) above the device primitives, with its fused gfx950 kernel.
//
// Real Float64, A of m rows and n columns, no M and N.  ONE orthogonal tridiagonalisation of Saunders, Simon and Yip advances the
// USYMLQ iterate of A x = b (with the transfer to the USYMCG point) and the USYMQR iterate of Aᴴ t = c: two products per iteration
// where usymlq! followed by usymqr! takes four.  Three loops, chosen as for its siblings (khip_trilqr_last_path):
//   0  options.fused = 0, and every m ≠ n system: the reference's primitive sequence, one launch per k* call, one host sync per
//      kdot / knorm;
//   1  the host-driven loop on the fused kernels (a user operator, a callback or verbose > 0);
//   2  the device-resident loop (default; A and Aᴴ both CSR handles): the scalar recurrences and stopping tests run as the
//      epilogues of the two reductions of an iteration (trilqr_step_a/b, solver_device.hpp), iterations are enqueued ahead.
// One iteration on the fused paths (m = n), after q = A uₖ and p = Aᴴ vₖ, with both sides unsolved:
//   P1   k ≥ 2: q = fma(-γₖ, vₖ₋₁, q) ; p = fma(-βₖ, uₖ₋₁, p) ; vₖ.q                    (ssy.hpp)                   56n bytes
//   P2   q = fma(-αₖ, vₖ, q) ; p = fma(-αₖ, uₖ, p) ; (q.q, p.p)                        (ssy.hpp)                   48n bytes
//   P3   k = 1: d̅ = uₖ ; else x = fma(ζₖ₋₁sₖ, uₖ, fma(ζₖ₋₁cₖ, d̅, x)) ; d̅ = fma(-cₖ, uₖ, sₖ d̅) ;
//        k ≥ 2: wₖ₋₁ = (vₖ₋₁ - λₖ₋₂ wₖ₋₂ - ϵₖ₋₃ wₖ₋₃) / δₖ₋₁ ; t = fma(ψₖ₋₁, wₖ₋₁, t) ;
//        βₖ₊₁ ≠ 0 ? vₖ₊₁ = q / βₖ₊₁ ; γₖ₊₁ ≠ 0 ? uₖ₊₁ = p / γₖ₊₁                                                    120n bytes
//        reads  uₖ, x, d̅, q, p, vₖ₋₁, wₖ₋₃, wₖ₋₂, t (9) ; writes x, d̅, vₖ₊₁, uₖ₊₁, wₖ₋₁, t (6)
// That is 224n beside the two products, against 368n for the primitive sequence: two kaxpy! of P1 (48n), kdot (16n), two kaxpy!
// of P2 (48n), two knorm (16n), two kaxpy! into x (48n), kaxpby! (24n), kscal! (16n), two kaxpy! into wₖ₋₁ (48n), kdiv! (16n),
// kaxpy! into t (24n), two kcopy! (32n), two kdivcopy! (32n).  A side that is solved drops its streams: the primal side x and d̅,
// read and written, and uₖ, which only the primal block and the γₖ₊₁ = 0 fallback read (40n), P3 = 80n; the dual side vₖ₋₁, wₖ₋₃,
// wₖ₋₂, t read and wₖ₋₁, t written (48n), P3 = 72n, usymlq!'s.  Smaller still at the first iterations: 48n at k = 1 (x and d̅ are
// not read, x is not written, the dual block does not run), 104n at k = 2 (wₖ₋₃ and wₖ₋₂ are not read).
// kcopy!(vₖ₋₁, vₖ), kcopy!(uₖ₋₁, uₖ) and @kswap!(wₖ₋₃, wₖ₋₂) become rotations of the buffers' roles (vₖ₊₁ and uₖ₊₁ are written where
// vₖ₋₁ and uₖ₋₁ were, wₖ₋₁ where wₖ₋₃ was).  Every elementwise value uses the expression of the primitive it replaces (fma for
// kaxpy!, fma(a, x, b y) for kaxpby!, a x for kscal!, x (1 / a) for kdiv!, / for kdivcopy!): the fused loops agree with the
// primitive sequence bit for bit on elementwise values and to the reductions' one ulp otherwise; loops 1 and 2 run the same
// kernels and the same scalar code and produce the same bits.
// P3 has no reduction; both sides' stopping tests belong to P2's epilogue, and P3 of the iteration that stops still runs,
// because the reference updates x, d̅, wₖ₋₁, t, vₖ₊₁ and uₖ₊₁ before it tests.  The epilogue therefore runs BEFORE P3 and leaves it
// which sides were unsolved when the iteration began (primal_on, dual_on).
// This file owns P3, the set-up of both systems, the LQ and QR parts of a primitive iteration and the status strings; the loops
// are ssy.hpp's.
#include <string>

#include "ssy.hpp"   // P1, P2 and the driver of the three loops
#include "usymlq_xd.hpp"

using namespace khip;

namespace khip {   // (named, not anonymous: stable kernel names in traces)

// ---------------------------------------------------------------------------------------------------------- kernels ----
// Each thread owns one VEC-vector of every stream; the odd tail element (VEC = 2, n odd) goes to thread 0 of block 0.
// Cache hints, the rule of ssy.hpp: a load is non-temporal when it is the LAST read of that data (x, d̅, t, wₖ₋₃, vₖ₋₁, q, p:
// overwritten here or by the next products); uₖ is read again by the next P1 (as uₖ₋₁), vₖ (read only when βₖ₊₁ = 0) likewise and
// wₖ₋₂ by the next P3 (as wₖ₋₃): they stay cacheable.  A store is non-temporal when nothing reads it before the next iteration's
// P3 (x, d̅, t, wₖ₋₁); vₖ₊₁ and uₖ₊₁ are read by the next products.

// wₖ₋₁ of one element (:339-357).  stage 2: kdivcopy!(w, v₁, δ₁).  stage 3: kaxpy!(1, vₖ₋₁, w₃) ; kaxpy!(-λ, w₂, w₃) ; kdiv!(w₃, δ).
// stage >= 4: kscal!(-ϵ, w₃) first.
__device__ __forceinline__ double trilqr_w(int stage, double vp, double w2, double w3, double ne, double nl, double dl, double idl) {
  if (stage == 2) return vp / dl;
  double t = stage >= 4 ? ne * w3 : w3;
  t = fma(1.0, vp, t);
  t = fma(nl, w2, t);
  return t * idl;
}

// P3 (:283-295, :339-368, :389-397).  primal (the primal system was unsolved when the iteration began): stage == 1 ? d̅ = u :
// usymlq_xd.  dual, from stage 2 on: w_out = wₖ₋₁ (trilqr_w) ; t = fma(ψ, wₖ₋₁, t).  Always: v_next = βₖ₊₁ ≠ 0 ? q / βₖ₊₁ : v ;
// u_next = γₖ₊₁ ≠ 0 ? p / γₖ₊₁ : u, two independent guards.  The branches are uniform (device state and a kernel argument); a
// side that is off loads and stores nothing of its streams.  w_out is w2 at stage 2 and w3 afterwards.  v_next MAY BE v_prev's
// buffer (it is, in the loops below): every thread reads its elements of v_prev before it writes v_next, the tail included.
// No reduction: the sequence number comes as an argument.
template <int VEC, bool NT>
__global__ __launch_bounds__(kBlock) void trilqr_p3_kernel(int64_t n, const TrilqrDevState *st, const long long *stop_seq, long long seq,
                                                          double *x, double *dbar, double *t, const double *w3, const double *w2,
                                                          double *w_out, const double *v, const double *u, const double *v_prev,
                                                          const double *q, const double *p, double *v_next, double *u_next,
                                                          int stage) {
  using T = typename VecT<VEC>::type;
  if (seq_skip(stop_seq, seq)) return;
  const double zc = st->zc, zs = st->zs, nc = st->neg_c, sn = st->sn, bn = st->beta_next, gn = st->gamma_next;
  const double ne = st->neg_eps3, nl = st->neg_lambda2, dl = st->delta, idl = st->inv_delta, psi = st->psi;
  const bool div_v = bn != 0.0, div_u = gn != 0.0;
  const bool primal = st->primal_on != 0;
  const bool dual = st->dual_on != 0 && stage >= 2;
  const int64_t nvec = n / VEC;
  const int64_t i = lane_index();
  if (i < nvec) {
    if (dual) {
      const T vpv = ldg<NT>(reinterpret_cast<const T *>(v_prev) + i);  // overwritten below (v_next): read first
      const T tv = ldg<NT>(reinterpret_cast<const T *>(t) + i);
      T w3v = {}, w2v = {};
      if (stage >= 3) {
        w3v = ldg<NT>(reinterpret_cast<const T *>(w3) + i);
        w2v = ldg<false>(reinterpret_cast<const T *>(w2) + i);         // wₖ₋₂ is the next iteration's wₖ₋₃
      }
      T wo, to;
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const double w = trilqr_w(stage, vget(vpv, e), vget(w2v, e), vget(w3v, e), ne, nl, dl, idl);
        vset(wo, e, w);
        vset(to, e, fma(psi, w, vget(tv, e)));
      }
      stg<NT>(wo, reinterpret_cast<T *>(w_out) + i);
      stg<NT>(to, reinterpret_cast<T *>(t) + i);
    }
    T uv = {};
    if (primal || !div_u) uv = ldg<false>(reinterpret_cast<const T *>(u) + i);        // u is the next iteration's u_prev
    if (primal) {
      T dv = uv;
      if (stage != 1) {
        T xv = ldg<NT>(reinterpret_cast<const T *>(x) + i);
        dv = ldg<NT>(reinterpret_cast<const T *>(dbar) + i);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          double xe = vget(xv, e), de = vget(dv, e);
          usymlq_xd(vget(uv, e), xe, de, zc, zs, nc, sn);
          vset(xv, e, xe);
          vset(dv, e, de);
        }
        stg<NT>(xv, reinterpret_cast<T *>(x) + i);
      }
      stg<NT>(dv, reinterpret_cast<T *>(dbar) + i);
    }
    T vo = div_v ? ldg<NT>(reinterpret_cast<const T *>(q) + i) : ldg<false>(reinterpret_cast<const T *>(v) + i);
    T uo = uv;
    if (div_u) uo = ldg<NT>(reinterpret_cast<const T *>(p) + i);
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      if (div_v) vset(vo, e, vget(vo, e) / bn);
      if (div_u) vset(uo, e, vget(uo, e) / gn);
    }
    stg<false>(vo, reinterpret_cast<T *>(v_next) + i);                  // read by the next products
    stg<false>(uo, reinterpret_cast<T *>(u_next) + i);
  }
  if (VEC == 2 && owns_tail(n)) {
    const int64_t e = n - 1;
    if (dual) {
      const double w = trilqr_w(stage, v_prev[e], stage >= 3 ? w2[e] : 0.0, stage >= 3 ? w3[e] : 0.0, ne, nl, dl, idl);
      w_out[e] = w;
      t[e] = fma(psi, w, t[e]);
    }
    const double ue = u[e];
    if (primal) {
      if (stage == 1) {
        dbar[e] = ue;
      } else {
        double xe = x[e], de = dbar[e];
        usymlq_xd(ue, xe, de, zc, zs, nc, sn);
        x[e] = xe;
        dbar[e] = de;
      }
    }
    v_next[e] = div_v ? q[e] / bn : v[e];
    u_next[e] = div_u ? p[e] / gn : ue;
  }
}

}  // namespace khip

namespace {

// P3 takes its sequence number from ctx->ctl, as the reductions do (all zero on the host-driven loop)
int launch_p3(khip_ctx *ctx, int64_t n, const TrilqrDevState *st, double *x, double *dbar, double *t, const double *w3, const double *w2,
              double *w_out, const double *v, const double *u, const double *v_prev, const double *q, const double *p, double *v_next,
              double *u_next, int stage) {
  VecPlan L;
  KHIP_TRY(vec_plan(ctx, n, {x, dbar, t, w3, w2, w_out, v, u, v_prev, q, p, v_next, u_next}, &L));
  const SeqCtl ctl = ctx->ctl;
  ProfScope prof_scope(ctx, kProfTrilqrP3);
  vec_dispatch_vn<ScalarPathNT::never>(L, [&](auto V, auto N) {
    hipLaunchKernelGGL((trilqr_p3_kernel<V, N>), L.grid(), dim3(kBlock), 0, ctx->stream, n, st, ctl.stop_seq, ctl.seq, x, dbar, t, w3,
                       w2, w_out, v, u, v_prev, q, p, v_next, u_next, stage); });
  KHIP_CHECK_HIP(hipGetLastError());
  return KHIP_OK;
}

}  // namespace

struct khip_trilqr_workspace {
  khip_ctx *ctx;
  int64_t m, n;
  // by their CURRENT role: the fused loops rotate (v_prev, v), (u_prev, u) and (w_prev3, w_prev2).  u_prev, u, p, dbar, x have n
  // entries, the others m
  double *u_prev = nullptr, *u = nullptr, *p = nullptr, *dbar = nullptr, *x = nullptr, *v_prev = nullptr, *v = nullptr, *q = nullptr,
         *y = nullptr, *w_prev3 = nullptr, *w_prev2 = nullptr, *dx = nullptr, *dy = nullptr;
  Borrowed borrowed;                        // the caller's vectors (khip_trilqr_workspace_adopt*): never freed here
  bool warm_start = false;
  StatsBox box;                             // box.residuals: the primal history
  std::vector<double> residuals_dual;
  std::string status;                       // the full status: four of the reference's strings do not fit khip_stats.status
  int solved_primal = 0, solved_dual = 0;
  DeviceLoop<TrilqrDevState, 3> loop;       // fused loops: device copy of the scalar state, pinned snapshots + staging, histories
};

namespace {

// uₖ₋₁, uₖ, p, d̅, x, vₖ₋₁, vₖ, q, t ("y"), wₖ₋₃, wₖ₋₂ come with the workspace; Δx, Δy stay empty until a warm start
// (src/krylov_workspaces.jl, TrilqrWorkspace: the table keeps its order)
using W = khip_trilqr_workspace;
constexpr WsVec<W> kVectors[] = {{"u_prev", &W::u_prev, Core},            {"u", &W::u, Core},          {"p", &W::p, Core},
                                 {"dbar", &W::dbar, Core},                {"x", &W::x, Core},          {"v_prev", &W::v_prev, Core, RowSide},
                                 {"v", &W::v, Core, RowSide},             {"q", &W::q, Core, RowSide}, {"y", &W::y, Core, RowSide},
                                 {"w_prev3", &W::w_prev3, Core, RowSide}, {"w_prev2", &W::w_prev2, Core, RowSide},
                                 {"dx", &W::dx, Lazy},                    {"dy", &W::dy, Lazy, RowSide}};

// "%7s" of the reference pads characters; ✗ ✗ ✗ ✗ is seven of them                                      (src/trilqr.jl:417-418)
const char *const kCrosses = "\xe2\x9c\x97 \xe2\x9c\x97 \xe2\x9c\x97 \xe2\x9c\x97";

// what trilqr! adds to the driver of the process (ssy.hpp)
struct Trilqr : SsyPolicy<TrilqrDevState, W> {
  static constexpr Epilogue kEpiA = EPI_TRILQR_A, kEpiB = EPI_TRILQR_B;
  double *x, *dbar, *t, *w3, *w2;                                                      // wₖ₋₃, wₖ₋₂ by their current role
  // host-driven loops: the sides that were unsolved when the iteration began.  The device-resident loop never calls
  // begin_iteration: enqueued ahead, its copy of the policy rotates (w₃, w₂) at every k ≥ 3 and fix_after_device_loop puts right
  // what the dual block did not do
  bool primal = true, dual = true;
  static void step_a(State &s, double vq) { trilqr_step_a(s, vq); }
  static void step_b(State &s, double qq, double pp, int64_t k) { (void)trilqr_step_b(s, qq, pp, k); }
  static bool stopped(const State &s) { return s.solved_primal && s.solved_dual; }
  void begin_iteration(const State &s) { primal = !s.solved_primal; dual = !s.solved_dual; }
  // v_prev twice: read as vₖ₋₁ and written as vₖ₊₁
  int p3(khip_ctx *ctx, int64_t n, const State *dev, const SsyRoles &r, int64_t k) const {
    return launch_p3(ctx, n, dev, x, dbar, t, w3, w2, k == 2 ? w2 : w3, r.v, r.u, r.v_prev, r.q, r.p, r.v_prev, r.u_prev,
                     k < 4 ? (int)k : 4);
  }
  // wₖ₋₁ was written over wₖ₋₃ (:359-362); a dual side that is solved no longer touches either buffer
  void rotate(int64_t k) { if (k >= 3 && dual) std::swap(w3, w2); }
  void fix_after_device_loop(const State &s) { if (s.nhist_d >= 3 && (s.nhist_d & 1)) std::swap(w3, w2); }   // the dual block ran nhist_d times
  void store(W *ws) const { ws->w_prev3 = w3; ws->w_prev2 = w2; }
  static std::vector<double> *dual_history(W *ws) { return &ws->residuals_dual; }
  void push_history(W *ws, const State &s) const {                                     // :306, :375
    if (primal) ws->box.push(s.rNorm_lq);
    if (dual) ws->residuals_dual.push_back(s.sNorm);
  }
  void verbose_row(const khip_options &o, long long iter, const State &s, double t0) const {             // :417-419
    if (s.solved_primal && !s.solved_dual) klogf(o.log_fd, "%5lld  %s  %7.1e  %.2fs\n", iter, kCrosses, s.sNorm, now_s() - t0);
    if (!s.solved_primal && s.solved_dual) klogf(o.log_fd, "%5lld  %7.1e  %s  %.2fs\n", iter, s.rNorm_lq, kCrosses, now_s() - t0);
    if (!s.solved_primal && !s.solved_dual) klogf(o.log_fd, "%5lld  %7.1e  %7.1e  %.2fs\n", iter, s.rNorm_lq, s.sNorm, now_s() - t0);
  }
  // the LQ part (d̅ and x), the QR part (wₖ₋₁ and t), then the shift of v and u, in the reference's order (:283-397)
  int primitive_tail(Ssy<Trilqr> &L, int64_t k) {
    W *ws = L.ws;
    khip_ctx *ctx = L.ctx;
    const int64_t m = L.m, n = L.n;
    State &s = L.s;
    if (primal) {                                                                                         // :283-295
      if (k == 1) {
        K(khip_copy(ctx, n, dbar, L.r.u));
      } else {
        K(khip_axpy(ctx, n, s.zc, dbar, x));
        K(khip_axpy(ctx, n, s.zs, L.r.u, x));
        K(khip_axpby(ctx, n, s.neg_c, L.r.u, s.sn, dbar));
      }
    }
    if (dual) {                                                                                           // :339-368
      double *w = nullptr;
      if (k == 2) {
        w = w2;
        K(khip_divcopy(ctx, m, w, L.r.v_prev, s.delta));
      }
      if (k >= 3) {
        w = w3;
        if (k >= 4) K(khip_scal(ctx, m, s.neg_eps3, w));
        K(khip_axpy(ctx, m, 1.0, L.r.v_prev, w));
        K(khip_axpy(ctx, m, s.neg_lambda2, w2, w));
        K(khip_div(ctx, m, w, s.delta));
        rotate(k);                                                                                        // @kswap!(wₖ₋₃, wₖ₋₂)
      }
      if (k >= 2) K(khip_axpy(ctx, m, s.psi, w, t));
    }
    K(L.shift());                                                                                         // :389-397
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

// the termination status (:430-446); XL / XC: "xᴸ" / "xᶜ".  A dual side that ended only by `inconsistent` sets none of the flags
// these lines read, so the status can stay "unknown", as in the reference.
#define XL "x\xe1\xb4\xb8"
#define XC "x\xe1\xb6\x9c"
const char *status_of(const TrilqrDevState &s, bool tired, bool user_exit, bool overtimed) {
  const char *status = "unknown";
  if (tired) status = "maximum number of iterations exceeded";
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

khip_trilqr_params khip_trilqr_default_params(void) {
  khip_trilqr_params p;
  p.transfer_to_usymcg = 1;
  return p;
}

int khip_trilqr_workspace_create(khip_ctx *ctx, int64_t m, int64_t n, khip_trilqr_workspace **out) {
  return ws_create(ctx, m, n, kVectors, "trilqr_workspace_create", khip_trilqr_workspace_destroy, out);
}

int khip_trilqr_workspace_adopt(khip_ctx *ctx, int64_t m, int64_t n, double *u_prev, double *u, double *p, double *dbar, double *x,
                                double *v_prev, double *v, double *q, double *y, double *w_prev3, double *w_prev2,
                                khip_trilqr_workspace **out) {
  return ws_adopt(ctx, m, n, kVectors, "trilqr_workspace_adopt", {u_prev, u, p, dbar, x, v_prev, v, q, y, w_prev3, w_prev2}, out);
}

int khip_trilqr_workspace_adopt_vector(khip_trilqr_workspace *ws, const char *name, double *ptr) {
  return ws_adopt_vector(ws, kVectors, "trilqr_workspace_adopt_vector", name, ptr);
}

int khip_trilqr_workspace_destroy(khip_trilqr_workspace *ws) {
  if (!ws) return KHIP_OK;
  ws_free_vectors(ws, kVectors);
  ws->loop.release();
  delete ws;
  return KHIP_OK;
}

int khip_trilqr_warm_start(khip_trilqr_workspace *ws, const double *x0, const double *y0) {   // Δx of n entries, Δy of m
  return ws_warm_start2(ws, kVectors, x0, y0, "trilqr_warm_start");
}

double *khip_trilqr_solution_x(khip_trilqr_workspace *ws) { return ws ? ws->x : nullptr; }
double *khip_trilqr_solution_y(khip_trilqr_workspace *ws) { return ws ? ws->y : nullptr; }
const khip_stats *khip_trilqr_stats(khip_trilqr_workspace *ws) { return ws ? &ws->box.st : nullptr; }
int khip_trilqr_adjoint_stats(khip_trilqr_workspace *ws, int *solved_primal, int *solved_dual, const double **residuals_primal,
                              int *nprimal, const double **residuals_dual, int *ndual, const char **status) {
  KHIP_REQUIRE(ws, "trilqr_adjoint_stats: null workspace");
  if (solved_primal) *solved_primal = ws->solved_primal;
  if (solved_dual) *solved_dual = ws->solved_dual;
  if (residuals_primal) *residuals_primal = ws->box.residuals.empty() ? nullptr : ws->box.residuals.data();
  if (nprimal) *nprimal = (int)ws->box.residuals.size();
  if (residuals_dual) *residuals_dual = ws->residuals_dual.empty() ? nullptr : ws->residuals_dual.data();
  if (ndual) *ndual = (int)ws->residuals_dual.size();
  if (status) *status = ws->status.c_str();
  return KHIP_OK;
}
int khip_trilqr_last_path(khip_trilqr_workspace *ws) { return ws ? ws->box.path : -1; }
double *khip_trilqr_vector(khip_trilqr_workspace *ws, const char *name) { return ws_vector(ws, kVectors, name); }
size_t khip_trilqr_workspace_bytes(khip_trilqr_workspace *ws) { return ws_bytes(ws, kVectors); }

int khip_trilqr_solve(khip_trilqr_workspace *ws, const khip_operator *A, const khip_operator *At, const double *b, const double *c,
                      const khip_options *opts_in, const khip_trilqr_params *params_in) {
  KHIP_REQUIRE(ws && A && b, "trilqr_solve: null argument");
  const khip_trilqr_params prm = params_in ? *params_in : khip_trilqr_default_params();
  Ssy<Trilqr> L(ws, A, At, opts_in);
  khip_ctx *ctx = L.ctx;
  const khip_options &o = L.o;
  const int64_t m = L.m, n = L.n;
  TrilqrDevState &s = L.s;
  const double atol = tol_or_default(o.atol), rtol = tol_or_default(o.rtol);

  if (int rc = L.check("trilqr", c)) return rc;                                                           // :121-124
  if (o.verbose > 0) {                                                                                    // :125-126
    klogf(o.log_fd, "TRILQR: primal system of %lld equations in %lld variables\n", (long long)m, (long long)n);
    klogf(o.log_fd, "TRILQR: dual system of %lld equations in %lld variables\n", (long long)n, (long long)m);
  }
  const bool warm_start = ws->warm_start;
  ws->box.reset();                                                                                        // reset!(stats)
  ws->residuals_dual.clear();
  ws->status = "unknown";
  ws->solved_primal = ws->solved_dual = 0;
  double *x = L.pol.x = ws->x, *t = L.pol.t = ws->y, *dbar = L.pol.dbar = ws->dbar;
  L.pol.w3 = ws->w_prev3;
  L.pol.w2 = ws->w_prev2;

  // set-up, the same primitives on every path (:142-200).  No early return for b = 0 or c = 0: a side whose right-hand side is
  // zero starts solved and the process goes on from 0 / 0, as in the reference
  const double *r0, *s0 = c;
  K(L.residual(b, warm_start, &r0));                                                                      // :145-147 (m, not n)
  if (warm_start) {                                                                                       // :148-149
    K(apply_op(ctx, At, ws->dy, L.r.p));
    K(khip_axpby(ctx, n, 1.0, c, -1.0, L.r.p));
    s0 = L.r.p;
  }
  K(khip_fill(ctx, n, x, 0.0));
  double bNorm, cNorm;
  K(khip_nrm2(ctx, m, r0, &bNorm));
  K(khip_fill(ctx, m, t, 0.0));
  K(khip_nrm2(ctx, n, s0, &cNorm));
  L.itmax = o.itmax == 0 ? global_rows(ctx, A, m) + global_rows(ctx, At, n) : o.itmax;                   // m + n of the global system (:161)
  if (L.history) {
    ws->box.push(bNorm);
    ws->residuals_dual.push_back(cNorm);
  }
  s.bNorm = bNorm;
  s.eps_L = atol + rtol * bNorm;                                                                         // :165-166
  s.eps_Q = atol + rtol * cNorm;
  s.atol = atol;
  s.rtol = rtol;
  s.rNorm_lq = bNorm;
  s.sNorm = cNorm;
  ws->box.path = (o.fused && L.square()) ? 1 : 0;
  if (o.verbose > 0) {                                                                                    // :168-169 (labels padded by hand)
    klogf(o.log_fd, "%5s  %s  %s  %5s\n", "k", "   \xe2\x80\x96r\xe2\x82\x96\xe2\x80\x96", "   \xe2\x80\x96s\xe2\x82\x96\xe2\x80\x96", "timer");
    if (kdisplay(0, o.verbose)) klogf(o.log_fd, "%5d  %7.1e  %7.1e  %.2fs\n", 0, bNorm, cNorm, now_s() - L.t0);
  }
  K(L.start(bNorm, cNorm, r0, s0));                                                                      // :172-177
  s.cs = s.cs_prev = -1.0;                                                                               // :178-179
  K(khip_fill(ctx, n, dbar, 0.0));                                                                       // :180
  K(khip_fill(ctx, m, L.pol.w3, 0.0));                                                                   // :186-187
  K(khip_fill(ctx, m, L.pol.w2, 0.0));
  s.transfer = prm.transfer_to_usymcg ? 1 : 0;
  s.stop_seq = kSeqNever;
  s.solved_lq = (bNorm == 0) ? 1 : 0;                                                                    // :190-196
  s.solved_primal = s.solved_lq;
  s.solved_dual = (cNorm == 0) ? 1 : 0;

  K(L.iterate());                                                                                         // :202-420

  if (s.solved_cg) K(khip_axpy(ctx, n, s.zbar, dbar, x));                                                // :425-427, d̅ₖ as P3 left it
  const char *status = status_of(s, L.tired, L.user_exit, L.overtimed);                                  // :430-446
  if (warm_start) K(khip_axpy(ctx, m, 1.0, ws->dy, t));                                                  // :450 (x + Δx: L.end)
  const int rc = L.end((s.solved_primal && s.solved_dual) ? 1 : 0, s.inconsistent ? 1 : 0, status, warm_start);
  if (rc != KHIP_OK) return rc;
  ws->status = status;
  ws->solved_primal = s.solved_primal ? 1 : 0;
  ws->solved_dual = s.solved_dual ? 1 : 0;
  copy_status(ws->box.st.status, sizeof(ws->box.st.status), ws->status);
  return KHIP_OK;
}

}  // extern "C"
