// usymlqr.cpp -- usymlqr! (src/usymlqr.jl:136-509) above the device primitives, with its fused gfx950 kernel.
//
// Real Float64, A of m rows and n columns, no preconditioners.  ONE orthogonal tridiagonalisation of Saunders, Simon and Yip and ONE
// QR factorisation of Tₖ₊₁.ₖ solve
//   [ I   A ] [x]   [b]
//   [ Aᴴ  0 ] [y] = [c]          x, b of m entries ; y, c of n entries
// as the sum of the least-squares problem [b; 0] (USYMQR: y and its residual r, when `ls`) and the least-norm problem [0; c]
// (USYMLQ: x and z, when `ln`); after the loop x += r and y += z.  Each side is frozen once its own test is met; wₖ, the
// factorisation and the shifts go on.  Three loops, chosen as for its siblings (khip_usymlqr_last_path):
//   0  options.fused = 0, and every m ≠ n system: the reference's primitive sequence, one launch per k* call, one host sync per
//      kdot / knorm;
//   1  the host-driven loop on the fused kernels (a user operator, a callback or verbose > 0);
//   2  the device-resident loop (default; A and Aᴴ both CSR handles): the scalar recurrences and stopping tests run as the
//      epilogues of the two reductions of an iteration (usymlqr_step_a/b, solver_device.hpp), iterations are enqueued ahead.
// One iteration on the fused paths (m = n), after q = A uₖ and p = Aᴴ vₖ:
//   P1   k ≥ 2: q = fma(-γₖ, vₖ₋₁, q) ; p = fma(-βₖ, uₖ₋₁, p) ; vₖ.q                    (ssy.hpp)                   56n bytes
//   P2   q = fma(-αₖ, vₖ, q) ; p = fma(-αₖ, uₖ, p) ; (q.q, p.p)                        (ssy.hpp)                   48n bytes
//        epilogue B: the reflections, do_ls / do_ln, every coefficient below, the three norms, the tests
//   P3   always: wₖ = (uₖ - λₖ₋₁ wₖ₋₁ - ϵₖ₋₂ wₖ₋₂) / δₖ ; vₖ₊₁ = βₖ₊₁ ≠ 0 ? q / βₖ₊₁ : 0 ; uₖ₊₁ = γₖ₊₁ ≠ 0 ? p / γₖ₊₁ : 0
//        do_ls:  y = fma(ϕₖ, wₖ, y) ; r = fma(-cₖϕbarₖ₊₁/βₖ₊₁, q, |sₖ|² r)
//        do_ln:  k = 1: d̅ = vₖ ; else x = fma(ζₖ₋₁sₖ₋₁, vₖ, fma(ζₖ₋₁cₖ₋₁, d̅, x)) ; z = fma(-ζₖ₋₁, wₖ₋₁, z) ; d̅ = fma(-cₖ₋₁, vₖ, sₖ₋₁ d̅)
//        k ≥ 3, both sides: reads uₖ, wₖ₋₁, wₖ₋₂, y, q, r, vₖ, x, d̅, z, p (11) ; writes wₖ, y, r, x, d̅, z, vₖ₊₁, uₖ₊₁ (8)      152n bytes
//        least squares only: reads uₖ, wₖ₋₁, wₖ₋₂, y, q, r, p (7) ; writes wₖ, y, r, vₖ₊₁, uₖ₊₁ (5)                            96n bytes
//        least norm only:    reads uₖ, wₖ₋₁, wₖ₋₂, vₖ, x, d̅, z, q, p (9) ; writes wₖ, x, d̅, z, vₖ₊₁, uₖ₊₁ (6)                   120n bytes
//        k = 1, both sides: reads uₖ, y, q, r, vₖ, p (6) ; writes wₖ, y, r, d̅, vₖ₊₁, uₖ₊₁ (6): 96n ; k = 2 as k ≥ 3 (wₖ₋₂ is read unscaled)
// That is 256n beside the two products with both sides active, against 416n for the primitive sequence: two kaxpy! of P1 (48n),
// kdot (16n), two kaxpy! of P2 (48n), two knorm (16n): 128n; then the tail, 288n: kscal!, two kaxpy! and kdiv! of wₖ (80n), kaxpy!
// into y and kaxpby! into r (48n), two kaxpy! into x, kaxpy! into z and kaxpby! into d̅ (96n), two kcopy! and two kdivcopy! (64n).
// With the two products of the 512³ 7-point operator at the handle's spmv_bytes (208n for both) this predicts 464n / 624n = 0.7435
// for path 2 over path 0; measured 0.711 (7.580 against 10.663 ms per iteration; DESIGN.md says why it is lower).
// kcopy!(vₖ₋₁, vₖ), kcopy!(uₖ₋₁, uₖ) and @kswap!(wₖ₋₂, wₖ₋₁) become rotations of the buffers' roles (vₖ₊₁ and uₖ₊₁ are written where vₖ₋₁ and
// uₖ₋₁ were, wₖ where wₖ₋₂ was; at k = 1 wₖ goes to the buffer of the role wₖ₋₁ and nothing is swapped).  Every elementwise value uses
// the expression of the primitive it replaces (fma for kaxpy!, fma(a, x, b y) for kaxpby!, a x for kscal!, x (1 / a) for kdiv!,
// which the reference defines as kscal!(1 / a), / for kdivcopy!): given the same scalars the three loops agree bit for bit on
// every vector; they differ through the reductions' one ulp.  Loops 1 and 2 run the same kernels and the same scalar code and
// produce the same bits.
// A side that is not active loads and stores none of its streams: a frozen y, r, x, z or d̅ keeps its bits whatever the other side
// holds.  z is updated with the OLD wₖ₋₁ (the kernel keeps it in registers and never writes its buffer).
// Where usymlqr! leaves the driver, as tricg! does: x has m entries and y has n, so the warm start's Δx and Δy are added here and
// Ssy::end gets warm_start = false; the start gives v₁ = 0 by a fill when β₁ = 0 (likewise u₁), and so does the shift (:441-455).
// Out of scope: complex types, fused kernels for m ≠ n, Float32; `ldiv` has no meaning without preconditioners.
// This file owns P3, the set-up, the tail of a primitive iteration, the histories' interleaving and the status strings; the loops
// are ssy.hpp's.
#include "ssy.hpp"   // P1, P2 and the driver of the three loops
#include "usymlq_xd.hpp"

using namespace khip;

namespace khip {   // (named, not anonymous: stable kernel names in traces)

// ---------------------------------------------------------------------------------------------------------- kernels ----
// Each thread owns one VEC-vector of every stream; the odd tail element (VEC = 2, n odd) goes to thread 0 of block 0.
// Cache hints, the rule of ssy.hpp and trimr.cpp: a load is non-temporal when it is the LAST read of that data before it is
// overwritten or dead (wₖ₋₂, y, r, x, d̅, z: overwritten here and read by nothing else before the next P3; q, p: overwritten by the
// next products); wₖ₋₁ is read again by the next P3 (as wₖ₋₂), uₖ and vₖ by the next P1 (as uₖ₋₁, vₖ₋₁): they stay cacheable.  A store
// is non-temporal when nothing reads it before the next iteration's P3 (wₖ, y, r, x, d̅, z); vₖ₊₁ and uₖ₊₁ are read by the next
// products.

// wₖ of one element (:312-332), usymqr!'s.  stage 1: kdivcopy!(w, u, δ).  stage 2: kaxpy!(-λ, w₁, w₂) ; kaxpy!(1, u, w₂) ;
// kdiv!(w₂, δ).  stage 3: kscal!(-ϵ, w₂) first.
__device__ __forceinline__ double usymlqr_w(int stage, double u, double w1, double w2, double ne, double nl, double dl, double idl) {
  if (stage == 1) return u / dl;
  double t = stage >= 3 ? ne * w2 : w2;
  t = fma(nl, w1, t);
  t = fma(1.0, u, t);
  return t * idl;
}

// P3 (:312-455).  stage: min(k, 3).  w_out is w2 from stage 2 on (wₖ over wₖ₋₂) and the buffer of the role wₖ₋₁ at stage 1, where
// neither w1 nor w2 is read.  v_next / u_next: the buffers of vₖ₋₁ / uₖ₋₁, which nothing here reads.  do_ls / do_ln come from the
// device state; the branches are uniform (device state and a kernel argument).  No reduction: the sequence number comes as an
// argument.
template <int VEC, bool NT>
__global__ __launch_bounds__(kBlock) void usymlqr_p3_kernel(int64_t n, const UsymlqrDevState *st, const long long *stop_seq, long long seq,
                                                           double *x, double *r, double *dbar, double *y, double *z, const double *w2,
                                                           const double *w1, double *w_out, const double *v, const double *u,
                                                           const double *q, const double *p, double *v_next, double *u_next,
                                                           int stage) {
  using T = typename VecT<VEC>::type;
  if (seq_skip(stop_seq, seq)) return;
  const bool ls = st->do_ls != 0, ln = st->do_ln != 0;
  const double ne = st->neg_eps, nl = st->neg_lambda, dl = st->delta, idl = st->inv_delta;
  const double phi = st->phi, rc = st->r_coef, s2 = st->s2;
  const double zc = st->zc, zs = st->zs, nz = st->neg_zeta, nc = st->neg_c, sn = st->sn;
  const double bn = st->beta_next, gn = st->gamma_next;
  const bool div_v = bn != 0.0, div_u = gn != 0.0;
  const int64_t nvec = n / VEC;
  const int64_t i = lane_index();
  if (i < nvec) {
    // wₖ: always
    const T uv = ldg<false>(reinterpret_cast<const T *>(u) + i);       // u is the next iteration's u_prev
    T w2v = {}, w1v = {};
    if (stage >= 2) {
      w2v = ldg<NT>(reinterpret_cast<const T *>(w2) + i);
      w1v = ldg<false>(reinterpret_cast<const T *>(w1) + i);           // wₖ₋₁ is the next iteration's wₖ₋₂
    }
    T wo;
#pragma unroll
    for (int e = 0; e < VEC; ++e) vset(wo, e, usymlqr_w(stage, vget(uv, e), vget(w1v, e), vget(w2v, e), ne, nl, dl, idl));
    stg<NT>(wo, reinterpret_cast<T *>(w_out) + i);
    T qv = {};
    if (ls || div_v) qv = ldg<NT>(reinterpret_cast<const T *>(q) + i);
    if (ls) {                                                           // :345, :350
      T yv = ldg<NT>(reinterpret_cast<const T *>(y) + i);
      T rv = ldg<NT>(reinterpret_cast<const T *>(r) + i);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        vset(yv, e, fma(phi, vget(wo, e), vget(yv, e)));
        vset(rv, e, fma(rc, vget(qv, e), s2 * vget(rv, e)));
      }
      stg<NT>(yv, reinterpret_cast<T *>(y) + i);
      stg<NT>(rv, reinterpret_cast<T *>(r) + i);
    }
    if (ln) {                                                           // :404-420
      const T vv = ldg<false>(reinterpret_cast<const T *>(v) + i);     // v is the next iteration's v_prev
      if (stage == 1) {
        stg<NT>(vv, reinterpret_cast<T *>(dbar) + i);
      } else {
        T xv = ldg<NT>(reinterpret_cast<const T *>(x) + i);
        T dv = ldg<NT>(reinterpret_cast<const T *>(dbar) + i);
        T zv = ldg<NT>(reinterpret_cast<const T *>(z) + i);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          double xe = vget(xv, e), de = vget(dv, e);
          usymlq_xd(vget(vv, e), xe, de, zc, zs, nc, sn);
          vset(xv, e, xe);
          vset(dv, e, de);
          vset(zv, e, fma(nz, vget(w1v, e), vget(zv, e)));              // the OLD wₖ₋₁
        }
        stg<NT>(xv, reinterpret_cast<T *>(x) + i);
        stg<NT>(dv, reinterpret_cast<T *>(dbar) + i);
        stg<NT>(zv, reinterpret_cast<T *>(z) + i);
      }
    }
    T vo = {}, uo = {};                                                 // βₖ₊₁ = 0: vₖ₊₁ = 0 (:446) ; γₖ₊₁ = 0: uₖ₊₁ = 0 (:454)
    if (div_v) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) vset(vo, e, vget(qv, e) / bn);
    }
    if (div_u) {
      const T pv = ldg<NT>(reinterpret_cast<const T *>(p) + i);
#pragma unroll
      for (int e = 0; e < VEC; ++e) vset(uo, e, vget(pv, e) / gn);
    }
    stg<false>(vo, reinterpret_cast<T *>(v_next) + i);                  // read by the next products
    stg<false>(uo, reinterpret_cast<T *>(u_next) + i);
  }
  if (VEC == 2 && owns_tail(n)) {
    const int64_t t = n - 1;
    const double w1e = stage >= 2 ? w1[t] : 0.0;
    const double w = usymlqr_w(stage, u[t], w1e, stage >= 2 ? w2[t] : 0.0, ne, nl, dl, idl);
    w_out[t] = w;
    if (ls) {
      y[t] = fma(phi, w, y[t]);
      r[t] = fma(rc, q[t], s2 * r[t]);
    }
    if (ln) {
      if (stage == 1) {
        dbar[t] = v[t];
      } else {
        double xe = x[t], de = dbar[t];
        usymlq_xd(v[t], xe, de, zc, zs, nc, sn);
        x[t] = xe;
        dbar[t] = de;
        z[t] = fma(nz, w1e, z[t]);
      }
    }
    v_next[t] = div_v ? q[t] / bn : 0.0;
    u_next[t] = div_u ? p[t] / gn : 0.0;
  }
}

}  // namespace khip

namespace {

// P3 takes its sequence number from ctx->ctl, as the reductions do (all zero on the host-driven loop)
int launch_p3(khip_ctx *ctx, int64_t n, const UsymlqrDevState *st, double *x, double *r, double *dbar, double *y, double *z,
              const double *w2, const double *w1, double *w_out, const double *v, const double *u, const double *q, const double *p,
              double *v_next, double *u_next, int stage) {
  VecPlan L;
  KHIP_TRY(vec_plan(ctx, n, {x, r, dbar, y, z, w2, w1, w_out, v, u, q, p, v_next, u_next}, &L));
  const SeqCtl ctl = ctx->ctl;
  ProfScope prof_scope(ctx, kProfUsymlqrP3);
  vec_dispatch_vn<ScalarPathNT::never>(L, [&](auto V, auto N) {
    hipLaunchKernelGGL((usymlqr_p3_kernel<V, N>), L.grid(), dim3(kBlock), 0, ctx->stream, n, st, ctl.stop_seq, ctl.seq, x, r, dbar, y, z,
                       w2, w1, w_out, v, u, q, p, v_next, u_next, stage); });
  KHIP_CHECK_HIP(hipGetLastError());
  return KHIP_OK;
}

}  // namespace

struct khip_usymlqr_workspace {
  khip_ctx *ctx;
  int64_t m, n;
  // by their CURRENT role: the fused loops rotate (v_prev, v), (u_prev, u) and (w_m2, w_m1).  r, x, v_prev, v, q, dbar and Δx have m
  // entries, the others n
  double *r = nullptr, *x = nullptr, *y = nullptr, *z = nullptr, *v_prev = nullptr, *v = nullptr, *u_prev = nullptr, *u = nullptr,
         *p = nullptr, *q = nullptr, *dbar = nullptr, *w_m2 = nullptr, *w_m1 = nullptr, *dx = nullptr, *dy = nullptr;
  Borrowed borrowed;                        // the caller's vectors (khip_usymlqr_workspace_adopt*): never freed here
  bool warm_start = false;
  StatsBox box;                             // box.residuals: ‖rₖ‖_LS and ‖rₖ‖_LN in the reference's push order
  std::vector<double> residuals_ln;         // the device-resident loop's least-norm stream, until it is interleaved
  std::vector<double> aresiduals;           // the Aresiduals history
  DeviceLoop<UsymlqrDevState, 3> loop;      // fused loops: device copy of the scalar state, pinned snapshots + staging, histories
};

namespace {

// r, x, y, z, vₖ₋₁, vₖ, uₖ₋₁, uₖ, p, q, d̅, wₖ₋₂, wₖ₋₁ come with the workspace; Δx, Δy stay empty until a warm start
// (src/krylov_workspaces.jl, UsymlqrWorkspace: the table keeps its order)
using W = khip_usymlqr_workspace;
constexpr WsVec<W> kVectors[] = {{"r", &W::r, Core, RowSide},           {"x", &W::x, Core, RowSide}, {"y", &W::y, Core},
                                 {"z", &W::z, Core},                    {"v_prev", &W::v_prev, Core, RowSide},
                                 {"v", &W::v, Core, RowSide},           {"u_prev", &W::u_prev, Core}, {"u", &W::u, Core},
                                 {"p", &W::p, Core},                    {"q", &W::q, Core, RowSide},
                                 {"dbar", &W::dbar, Core, RowSide},     {"w_m2", &W::w_m2, Core},    {"w_m1", &W::w_m1, Core},
                                 {"dx", &W::dx, Lazy, RowSide},         {"dy", &W::dy, Lazy}};

// "%7s" of the reference pads characters; ✗ ✗ ✗ ✗ is seven of them                                      (src/usymlqr.jl:240-241)
const char *const kCrosses = "\xe2\x9c\x97 \xe2\x9c\x97 \xe2\x9c\x97 \xe2\x9c\x97";

// what usymlqr! adds to the driver of the process (ssy.hpp)
struct Usymlqr : SsyPolicy<UsymlqrDevState, W> {
  static constexpr Epilogue kEpiA = EPI_USYMLQR_A, kEpiB = EPI_USYMLQR_B;
  double *x, *r, *dbar, *y, *z, *w2, *w1;                                              // wₖ₋₂, wₖ₋₁ by their current role
  static void step_a(State &s, double vq) { usymlqr_step_a(s, vq); }
  static void step_b(State &s, double qq, double pp, int64_t k) { (void)usymlqr_step_b(s, qq, pp, k); }
  static bool stopped(const State &s) { return (s.solved_ls && s.solved_ln) || s.inconsistent; }
  // vₖ₊₁ and uₖ₊₁ go where vₖ₋₁ and uₖ₋₁ were
  int p3(khip_ctx *ctx, int64_t n, const State *dev, const SsyRoles &R, int64_t k) const {
    return launch_p3(ctx, n, dev, x, r, dbar, y, z, w2, w1, k == 1 ? w1 : w2, R.v, R.u, R.q, R.p, R.v_prev, R.u_prev, k < 3 ? (int)k : 3);
  }
  void rotate(int64_t k) { if (k >= 2) std::swap(w2, w1); }                            // wₖ was written over wₖ₋₂ (:457-460)
  void fix_after_device_loop(const State &s) { if (s.iter >= 2 && !(s.iter & 1)) std::swap(w2, w1); }   // iter - 1 swaps ran
  void store(W *ws) const { ws->w_m1 = w1; ws->w_m2 = w2; }
  static std::vector<double> *dual_history(W *ws) { return &ws->residuals_ln; }
  void push_history(W *ws, const State &s) const {                                     // :354, :358, :431
    if (s.do_ls) { ws->box.push(s.rNorm_ls); ws->aresiduals.push_back(s.ArNorm); }
    if (s.do_ln) ws->box.push(s.rNorm_ln);
  }
  void verbose_row(const khip_options &o, long long k, const State &s, double t0) const {                // :479-481
    if (!s.ls && s.ln)
      klogf(o.log_fd, "%5lld  %7.1e  %7.1e  %s  %7.1e  %.2fs\n", k, s.beta_next, s.gamma_next, kCrosses, s.rNorm_ln, now_s() - t0);
    if (s.ls && !s.ln)
      klogf(o.log_fd, "%5lld  %7.1e  %7.1e  %7.1e  %s  %.2fs\n", k, s.beta_next, s.gamma_next, s.rNorm_ls, kCrosses, now_s() - t0);
    if (s.ls && s.ln)
      klogf(o.log_fd, "%5lld  %7.1e  %7.1e  %7.1e  %7.1e  %.2fs\n", k, s.beta_next, s.gamma_next, s.rNorm_ls, s.rNorm_ln, now_s() - t0);
  }
  // wₖ (:312-332), the least-squares part (:345-350), the least-norm part (:404-420), then the shift of v and u (:266-267, :441-455)
  // and the swap (:457-460), on the primitives in the reference's order.  The two norms come earlier here (the head).
  int primitive_tail(Ssy<Usymlqr> &L, int64_t k) {
    W *ws = L.ws;
    khip_ctx *ctx = L.ctx;
    const int64_t m = L.m, n = L.n;
    const State &s = L.s;
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
    if (s.do_ls) {
      K(khip_axpy(ctx, n, s.phi, w, y));
      K(khip_axpby(ctx, m, s.r_coef, L.r.q, s.s2, r));
    }
    if (s.do_ln) {
      if (k == 1) {
        K(khip_copy(ctx, m, dbar, L.r.v));
      } else {
        K(khip_axpy(ctx, m, s.zc, dbar, x));
        K(khip_axpy(ctx, m, s.zs, L.r.v, x));
        K(khip_axpy(ctx, n, s.neg_zeta, w1, z));
        K(khip_axpby(ctx, m, s.neg_c, L.r.v, s.sn, dbar));
      }
    }
    K(khip_copy(ctx, m, L.r.v_prev, L.r.v));
    K(khip_copy(ctx, n, L.r.u_prev, L.r.u));
    if (s.beta_next != 0) K(khip_divcopy(ctx, m, L.r.v, L.r.q, s.beta_next));
    else K(khip_fill(ctx, m, L.r.v, 0.0));
    if (s.gamma_next != 0) K(khip_divcopy(ctx, n, L.r.u, L.r.p, s.gamma_next));
    else K(khip_fill(ctx, n, L.r.u, 0.0));
    rotate(k);                                                                         // @kswap!(wₖ₋₂, wₖ₋₁)
    return KHIP_OK;
  }
};

}  // namespace

extern "C" {

khip_usymlqr_params khip_usymlqr_default_params(void) {
  khip_usymlqr_params p;
  p.ls = 1;
  p.ln = 1;
  return p;
}

int khip_usymlqr_workspace_create(khip_ctx *ctx, int64_t m, int64_t n, khip_usymlqr_workspace **out) {
  return ws_create(ctx, m, n, kVectors, "usymlqr_workspace_create", khip_usymlqr_workspace_destroy, out);
}

int khip_usymlqr_workspace_adopt(khip_ctx *ctx, int64_t m, int64_t n, double *r, double *x, double *y, double *z, double *v_prev, double *v,
                                 double *u_prev, double *u, double *p, double *q, double *dbar, double *w_m2, double *w_m1,
                                 khip_usymlqr_workspace **out) {
  return ws_adopt(ctx, m, n, kVectors, "usymlqr_workspace_adopt", {r, x, y, z, v_prev, v, u_prev, u, p, q, dbar, w_m2, w_m1}, out);
}

int khip_usymlqr_workspace_adopt_vector(khip_usymlqr_workspace *ws, const char *name, double *ptr) {
  return ws_adopt_vector(ws, kVectors, "usymlqr_workspace_adopt_vector", name, ptr);
}

int khip_usymlqr_workspace_destroy(khip_usymlqr_workspace *ws) {
  if (!ws) return KHIP_OK;
  ws_free_vectors(ws, kVectors);
  ws->loop.release();
  delete ws;
  return KHIP_OK;
}

int khip_usymlqr_warm_start(khip_usymlqr_workspace *ws, const double *x0, const double *y0) {   // Δx of m entries, Δy of n
  return ws_warm_start2(ws, kVectors, x0, y0, "usymlqr_warm_start");
}

double *khip_usymlqr_solution_x(khip_usymlqr_workspace *ws) { return ws ? ws->x : nullptr; }
double *khip_usymlqr_solution_y(khip_usymlqr_workspace *ws) { return ws ? ws->y : nullptr; }
const khip_stats *khip_usymlqr_stats(khip_usymlqr_workspace *ws) { return ws ? &ws->box.st : nullptr; }
int khip_usymlqr_last_path(khip_usymlqr_workspace *ws) { return ws ? ws->box.path : -1; }
double *khip_usymlqr_vector(khip_usymlqr_workspace *ws, const char *name) { return ws_vector(ws, kVectors, name); }
size_t khip_usymlqr_workspace_bytes(khip_usymlqr_workspace *ws) { return ws_bytes(ws, kVectors); }

int khip_usymlqr_aresiduals(khip_usymlqr_workspace *ws, const double **aresiduals, int *naresiduals) {
  KHIP_REQUIRE(ws && aresiduals && naresiduals, "usymlqr_aresiduals: null argument");
  *aresiduals = ws->aresiduals.empty() ? nullptr : ws->aresiduals.data();
  *naresiduals = (int)ws->aresiduals.size();
  return KHIP_OK;
}

int khip_usymlqr_solve(khip_usymlqr_workspace *ws, const khip_operator *A, const khip_operator *At, const double *b, const double *c,
                       const khip_options *opts_in, const khip_usymlqr_params *params_in) {
  KHIP_REQUIRE(ws && A && b, "usymlqr_solve: null argument");
  const khip_usymlqr_params prm = params_in ? *params_in : khip_usymlqr_default_params();
  Ssy<Usymlqr> L(ws, A, At, opts_in);
  khip_ctx *ctx = L.ctx;
  const khip_options &o = L.o;
  const int64_t m = L.m, n = L.n;
  UsymlqrDevState &s = L.s;
  const double atol = tol_or_default(o.atol), rtol = tol_or_default(o.rtol);
  const bool ls = prm.ls != 0, ln = prm.ln != 0;

  if (int rc = L.check("usymlqr", c)) return rc;                                                          // :141-144
  if (!ls && !ln) return ws->box.fail(KHIP_ERR_INVALID, "The keyword arguments `ls` and `ln` can't be both `false`.");   // :145
  if (o.verbose > 0)                                                                                      // :146
    klogf(o.log_fd, "USYMLQR: system of %lld equations in %lld variables\n", (long long)(m + n), (long long)(m + n));
  const bool warm_start = ws->warm_start;
  ws->box.reset(); ws->residuals_ln.clear(); ws->aresiduals.clear();                                      // reset!(stats)
  Usymlqr &P = L.pol;
  P.x = ws->x; P.r = ws->r; P.dbar = ws->dbar; P.y = ws->y; P.z = ws->z; P.w2 = ws->w_m2; P.w1 = ws->w_m1;
  L.itmax = o.itmax == 0 ? global_rows(ctx, A, m) + global_rows(ctx, At, n) : o.itmax;                    // m + n of the global system (:170)

  // set-up, the same primitives on every path (:173-237)
  K(khip_fill(ctx, m, L.r.v_prev, 0.0));
  K(khip_fill(ctx, n, L.r.u_prev, 0.0));
  const double *b0 = b, *c0 = c;
  if (warm_start) {                                                                                       // :178-184
    K(apply_op(ctx, A, ws->dy, L.r.q));
    K(khip_axpy(ctx, m, 1.0, ws->dx, L.r.q));
    K(khip_axpby(ctx, m, 1.0, b, -1.0, L.r.q));
    K(apply_op(ctx, At, ws->dx, L.r.p));
    K(khip_axpby(ctx, n, 1.0, c, -1.0, L.r.p));
    b0 = L.r.q;
    c0 = L.r.p;
  }
  if (ls) K(khip_copy(ctx, m, P.r, b0));                                                                  // :187-190
  else K(khip_fill(ctx, m, P.r, 0.0));
  K(khip_fill(ctx, m, P.x, 0.0));
  K(khip_fill(ctx, n, P.y, 0.0));
  K(khip_fill(ctx, n, P.z, 0.0));
  double beta1, gamma1;
  K(khip_copy(ctx, m, L.r.v, b0));                                                                        // :193-200
  K(khip_nrm2(ctx, m, L.r.v, &beta1));
  if (beta1 != 0) K(khip_div(ctx, m, L.r.v, beta1));
  else K(khip_fill(ctx, m, L.r.v, 0.0));
  K(khip_copy(ctx, n, L.r.u, c0));                                                                        // :203-210
  K(khip_nrm2(ctx, n, L.r.u, &gamma1));
  if (gamma1 != 0) K(khip_div(ctx, n, L.r.u, gamma1));
  else K(khip_fill(ctx, n, L.r.u, 0.0));
  K(khip_fill(ctx, n, P.w2, 0.0));                                                                        // :214-216
  K(khip_fill(ctx, n, P.w1, 0.0));
  K(khip_fill(ctx, m, P.dbar, 0.0));
  s.beta = s.beta_next = beta1;
  s.gamma = s.gamma_next = gamma1;
  s.c_km2 = s.c_km1 = -1.0;                                                                               // :212-213
  s.phibar = beta1;                                                                                       // :217
  s.atol = atol; s.rtol = rtol; s.kappa = 0.0;                                                            // :223
  s.ArNorm = std::numeric_limits<double>::infinity();                                                     // :224
  s.rNorm_ls = beta1;                                                                                     // :225-228
  s.rNorm_ln = s.cNorm = gamma1;
  s.eps_ls = atol + rtol * beta1;
  s.eps_ln = atol + rtol * gamma1;
  s.ls = ls ? 1 : 0;
  s.ln = ln ? 1 : 0;
  s.solved_ls = (!ls || s.rNorm_ls <= s.eps_ls) ? 1 : 0;                                                  // :229-230
  s.solved_ln = (!ln || s.rNorm_ln <= s.eps_ln) ? 1 : 0;
  s.stop_seq = kSeqNever;
  ws->box.path = (o.fused && L.square()) ? 1 : 0;
  ws->loop.third_stream = &ws->aresiduals;
  if (o.verbose > 0) {                                                                                    // :239-242 (labels padded by hand)
    klogf(o.log_fd, "%5s  %s  %s  %s  %s  %5s\n", "k", "   \xce\xb2\xe2\x82\x96\xe2\x82\x8a\xe2\x82\x81", "   \xce\xb3\xe2\x82\x96\xe2\x82\x8a\xe2\x82\x81",
          "\xe2\x80\x96r\xe2\x82\x96\xe2\x80\x96_LS", "\xe2\x80\x96r\xe2\x82\x96\xe2\x80\x96_LN", "timer");
    if (kdisplay(0, o.verbose)) {
      if (!ls && ln) klogf(o.log_fd, "%5d  %7.1e  %7.1e  %s  %7.1e  %.2fs\n", 0, beta1, gamma1, kCrosses, s.rNorm_ln, now_s() - L.t0);
      if (ls && !ln) klogf(o.log_fd, "%5d  %7.1e  %7.1e  %7.1e  %s  %.2fs\n", 0, beta1, gamma1, s.rNorm_ls, kCrosses, now_s() - L.t0);
      if (ls && ln) klogf(o.log_fd, "%5d  %7.1e  %7.1e  %7.1e  %7.1e  %.2fs\n", 0, beta1, gamma1, s.rNorm_ls, s.rNorm_ln, now_s() - L.t0);
    }
  }

  K(L.iterate());                                                                                         // :244-482

  // the device-resident loop kept one stream per side, each a prefix that ends with the iteration that solved its side; the
  // reference pushes, per iteration, the least-squares entry and then the least-norm entry (:354, :431)
  if (ws->box.path == 2 && L.history) {
    const std::vector<double> rls = ws->box.residuals;
    std::vector<double> &out = ws->box.residuals;
    out.clear();
    for (size_t k = 0; k < (size_t)L.iter; ++k) {
      if (k < rls.size()) out.push_back(rls[k]);
      if (k < ws->residuals_ln.size()) out.push_back(ws->residuals_ln[k]);
    }
  }
  ws->residuals_ln.clear();

  const bool solved = s.solved_ls && s.solved_ln;
  const char *status = "unknown";                                                                         // :486-489
  if (L.tired) status = "maximum number of iterations exceeded";
  if (solved) status = "solution good enough given atol and rtol";
  if (L.user_exit) status = "user-requested exit";
  if (L.overtimed) status = "time limit exceeded";
  K(khip_axpy(ctx, m, 1.0, ws->r, ws->x));                                                                // :494-495
  K(khip_axpy(ctx, n, 1.0, ws->z, ws->y));
  if (warm_start) {                                                                                       // :498-499: Δx has m entries, Δy has n
    K(khip_axpy(ctx, m, 1.0, ws->dx, ws->x));
    K(khip_axpy(ctx, n, 1.0, ws->dy, ws->y));
  }
  return L.end(solved ? 1 : 0, 0, status, false);                                                         // :500-507: inconsistent is always false
}

// ---- test-only exports (include/krylov_hip_test.h) --------------------------------------------------------------------------
// P3 at a given stage and pair of activity flags with the caller's coefficients: coef14 = -ϵₖ₋₂, -λₖ₋₁, δₖ, ϕₖ, the r coefficient, |sₖ|²,
// ζₖ₋₁cₖ₋₁, ζₖ₋₁sₖ₋₁, -ζₖ₋₁, -cₖ₋₁, sₖ₋₁, βₖ₊₁, γₖ₊₁, 1 / δₖ.
int khip_test_usymlqr_p3(khip_ctx *ctx, int64_t n, int stage, int do_ls, int do_ln, const double *coef14, double *x, double *r, double *dbar,
                         double *y, double *z, double *w_m2, double *w_m1, const double *v, const double *u, const double *q,
                         const double *p, double *v_next, double *u_next) {
  KHIP_REQUIRE(ctx && n >= 0 && stage >= 1 && stage <= 3 && coef14 && x && r && dbar && y && z && w_m2 && w_m1 && v && u && q && p &&
                   v_next && u_next,
               "test_usymlqr_p3: bad argument");
  UsymlqrDevState h;
  memset(&h, 0, sizeof(h));
  h.neg_eps = coef14[0];
  h.neg_lambda = coef14[1];
  h.delta = coef14[2];
  h.phi = coef14[3];
  h.r_coef = coef14[4];
  h.s2 = coef14[5];
  h.zc = coef14[6];
  h.zs = coef14[7];
  h.neg_zeta = coef14[8];
  h.neg_c = coef14[9];
  h.sn = coef14[10];
  h.beta_next = coef14[11];
  h.gamma_next = coef14[12];
  h.inv_delta = coef14[13];
  h.do_ls = do_ls ? 1 : 0;
  h.do_ln = do_ln ? 1 : 0;
  h.stop_seq = kSeqNever;
  UsymlqrDevState *dev = nullptr;
  KHIP_CHECK_HIP(hipMalloc(&dev, sizeof(h)));
  int rc = KHIP_OK;
  if (hipMemcpy(dev, &h, sizeof(h), hipMemcpyHostToDevice) != hipSuccess) rc = KHIP_ERR_HIP;
  const SeqCtl keep = ctx->ctl;
  ctx->ctl = SeqCtl{};
  if (rc == KHIP_OK && n > 0)
    rc = launch_p3(ctx, n, dev, x, r, dbar, y, z, w_m2, w_m1, stage == 1 ? w_m1 : w_m2, v, u, q, p, v_next, u_next, stage);
  ctx->ctl = keep;
  if (hipStreamSynchronize(ctx->stream) != hipSuccess && rc == KHIP_OK) rc = KHIP_ERR_HIP;
  (void)hipFree(dev);
  return rc;
}

}  // extern "C"
