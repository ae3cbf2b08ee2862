// trimr.cpp -- trimr! (src/trimr.jl:150-577) above the device primitives, with its fused gfx950 kernel.
//
// Real Float64, A of m rows and n columns, M = N = I.  The orthogonal tridiagonalisation of Saunders, Simon and Yip, started from
// b and c, gives the minimal-residual iterate of the 2 × 2 block system
//   [ τI   A ] [x]   [b]
//   [ Aᴴ  νI ] [y] = [c]          x, b of m entries ; y, c of n entries
// through a QR factorisation in scalars (four reflections per iteration).  Unlike tricg! it never divides by τ or ν: saddle-point
// systems (ν = 0, the `sp` flag) and adjoint systems (τ = ν = 0) are ordinary solves, and ‖rₖ‖ is non-increasing.  Three loops, chosen
// as for its siblings (khip_trimr_last_path):
//   0  options.fused = 0, and every m ≠ n system: the reference's primitive sequence, one launch per k* call, one host sync per
//      kdot / knorm;
//   1  the host-driven loop on the fused kernels (a user operator, a callback or verbose > 0);
//   2  the device-resident loop (default; A and Aᴴ both CSR handles): the scalar recurrences and stopping tests run as the
//      epilogues of the two reductions of an iteration (trimr_step_a/b, solver_device.hpp), iterations are enqueued ahead.
// One iteration on the fused paths (m = n), after q = A uₖ and p = Aᴴ vₖ:
//   P1   k ≥ 2: q = fma(-γₖ, vₖ₋₁, q) ; p = fma(-βₖ, uₖ₋₁, p) ; vₖ.q                    (ssy.hpp)                   56n bytes
//        epilogue A: stores αₖ (the QR update needs βₖ₊₁ and γₖ₊₁)
//   P2   q = fma(-αₖ, vₖ, q) ; p = fma(-αₖ, uₖ, p) ; (q.q, p.p)                        (ssy.hpp)                   48n bytes
//        epilogue B: βₖ₊₁, γₖ₊₁, the four previous and the four new reflections, π₂ₖ₋₁, π₂ₖ, ‖rₖ‖, the shifts, breakdown and solved
//   P3   k = 1: gx₁ = v₁ / δ₁ ; gx₂ = (-σ₁ / δ₂) gx₁ ; gy₂ = u₁ / δ₂ (gy₁ keeps the zeros of the set-up)             88n bytes
//        k = 2: the four broadcasts of :460-463, (g₁, g₂) -> (g₃, g₄) into the other pair's buffers                  144n bytes
//        k ≥ 3: the four broadcasts of :468-476, (g₂ₖ₋₁, g₂ₖ) written over (g₂ₖ₋₅, g₂ₖ₋₄)                              176n bytes
//        every k: x = fma(π₂ₖ, gx₂ₖ, fma(π₂ₖ₋₁, gx₂ₖ₋₁, x)), y likewise ; vₖ₊₁ = βₖ₊₁ > btol ? q (1 / βₖ₊₁) : q ; uₖ₊₁ likewise
//        k ≥ 3 reads  vₖ, uₖ, eight g, x, y, q, p (14) ; writes four g, x, y, vₖ₊₁, uₖ₊₁ (8)
//        k = 2 reads  vₖ, uₖ, four g, x, y, q, p (10) ; writes four g, x, y, vₖ₊₁, uₖ₊₁ (8)
//        k = 1 reads  vₖ, uₖ, q, p (4) ; writes gx₁, gx₂, gy₂, x, y, vₖ₊₁, uₖ₊₁ (7)
// That is 280n beside the two products, against 496n for the primitive sequence: P1 (two kaxpy! 48n), kdot (16n), P2 (two
// kaxpy! 48n), two knorm (16n), two kdiv! (32n): 160n; the four broadcasts (reads 5 + 4 + 4 + 5, one write each: 22 streams)
// 176n; four kaxpy! into x and y 96n; four kcopy! 64n.
// Every g value is the reference's broadcast expression as it stands: separately rounded products, subtractions from left to
// right, a leading -(c g) where the expression starts with `.-`, then ONE true division by δ (not a product with a reciprocal).
// The fused P3 and the elementwise kernel of the primitive sequence (trimr_g_kernel, one output vector per launch) are built from
// the same per-element function trimr_g, so given the same scalars all three loops agree bit for bit on every g; they differ
// through the reductions' one ulp.  Loops 1 and 2 run the same kernels and the same scalar code and produce the same bits.
// The reference's @kswap!s (:457-459, :470-471, :477-478) become ONE rotation of the policy's roles: from k = 2 on the older pair
// (g₂ₖ₋₃, g₂ₖ₋₂ by name as the iteration begins) and the newer pair (g₂ₖ₋₁, g₂ₖ) of each side change places once per iteration --
// before the update at k = 2, after it from k = 3 on, which for a P3 that writes into the older pair's buffers and then swaps
// is the same thing.  (At k = 2 the reference does not swap gy₂ₖ₋₃ with gy₂ₖ₋₁: both are zero.)  kcopy!(vₖ₋₁, vₖ), kcopy!(uₖ₋₁, uₖ)
// are the rotation of ssy.hpp.  g₂ₖ's last term uses the NEW g₂ₖ₋₁ from registers, never the buffer it overwrote.
// P3 does NOT write q / βₖ₊₁ back into q (nor p): on the fused paths "q" and "p" hold the undivided vectors after an iteration,
// on path 0 the divided ones, as in the reference.  No other name differs.
// Where trimr! leaves the driver, as tricg! does: x has m entries and y has n, so the warm start's Δx and Δy are added here and
// Ssy::end gets warm_start = false; the start gives v₁ = 0 by a fill when β₁ = 0 (likewise u₁); the shift's guards are > btol, and
// a vector that is not divided is still taken over.
// Out of scope: M and N other than I, complex types, fused kernels for m ≠ n, Float32.
// This file owns P3, the g kernel of path 0, the set-up, the g, x and y part of a primitive iteration and the status strings;
// the loops are ssy.hpp's.
#include "ssy.hpp"   // P1, P2 and the driver of the three loops

using namespace khip;

namespace khip {   // (named, not anonymous: stable kernel names in traces)

// ---------------------------------------------------------------------------------------------------------- kernels ----
// One g value (:460-476): (w - c0 a0 - c1 a1 [- c2 a2 [- c3 a3]]) / δ, or with -(c0 a0) in front where the row has no right-hand
// side.  nterm and has_w are compile-time constants at every call in P3 and uniform in trimr_g_kernel.
__device__ __forceinline__ double trimr_g(bool has_w, int nterm, double w, double c0, double a0, double c1, double a1, double c2,
                                          double a2, double c3, double a3, double delta) {
  double t = has_w ? w - c0 * a0 : -(c0 * a0);
  t = t - c1 * a1;
  if (nterm > 2) t = t - c2 * a2;
  if (nterm > 3) t = t - c3 * a3;
  return t / delta;
}

struct TrimrCoef {
  TrimrRow r1, r2;
  double first_scale, pi1, pi2;
};
// k = 1 (:449-451, :495-500): x and y are zero and are not read; gy₁ is zero and is neither read nor written
__device__ __forceinline__ void trimr_first(const TrimrCoef &c, double v, double u, double &gx1, double &gx2, double &gy2, double &x,
                                            double &y) {
  gx1 = v / c.r1.delta;
  gx2 = c.first_scale * gx1;
  gy2 = u / c.r2.delta;
  x = fma(c.pi2, gx2, fma(c.pi1, gx1, 0.0));
  y = fma(c.pi2, gy2, fma(c.pi1, 0.0, 0.0));
}
// k = 2 (:460-463): n1, n2 hold (g₁, g₂) of a side; o1, o2 take (g₃, g₄).  has_w: w = vₖ stands in row one (x side); else w = uₖ
// stands in row two (y side)
__device__ __forceinline__ void trimr_second(const TrimrCoef &c, bool x_side, double w, double n1, double n2, double &o1, double &o2) {
  o1 = trimr_g(x_side, 2, w, c.r1.eta, n1, c.r1.sigma, n2, 0.0, 0.0, 0.0, 0.0, c.r1.delta);
  o2 = trimr_g(!x_side, 3, w, c.r2.lambda, n1, c.r2.eta, n2, c.r2.sigma, o1, 0.0, 0.0, c.r2.delta);
}
// k ≥ 3 (:467-476): o1, o2 hold (g₂ₖ₋₅, g₂ₖ₋₄) and take (g₂ₖ₋₁, g₂ₖ); n1, n2 hold (g₂ₖ₋₃, g₂ₖ₋₂)
__device__ __forceinline__ void trimr_later(const TrimrCoef &c, bool x_side, double w, double n1, double n2, double &o1, double &o2) {
  const double g1 = trimr_g(x_side, 4, w, c.r1.mu, o1, c.r1.lambda, o2, c.r1.eta, n1, c.r1.sigma, n2, c.r1.delta);
  o2 = trimr_g(!x_side, 4, w, c.r2.mu, o2, c.r2.lambda, n1, c.r2.eta, n2, c.r2.sigma, g1, c.r2.delta);
  o1 = g1;
}

// Each thread owns one VEC-vector of every stream; the odd tail element (VEC = 2, n odd) goes to thread 0 of block 0.
// Cache hints, the rule of ssy.hpp: a load is non-temporal when it is the LAST read of that data before it is overwritten or
// dead (the g, x, y: the older pair is overwritten here, the newer pair by the next P3 after one more read -- both are read
// by nothing else in between and a P3's streams exceed the caches; q, p: overwritten by the next products); vₖ and uₖ are read
// again by the next P1 (as vₖ₋₁, uₖ₋₁) and stay cacheable.  A store is non-temporal when nothing reads it before the next
// iteration's P3 (the g, x, y); vₖ₊₁ and uₖ₊₁ are read by the next products.

// P3 (:446-516).  stage: min(k, 3).  gxo1, gxo2 / gyo1, gyo2: the buffers of the roles (g₂ₖ₋₃, g₂ₖ₋₂) as the iteration begins (the older
// pair); gxn1, gxn2 / gyn1, gyn2: those of (g₂ₖ₋₁, g₂ₖ) (the newer pair).  Stage 1 writes the newer pair (the roles are the final ones,
// no swap); from stage 2 on the older pair's buffers take (g₂ₖ₋₁, g₂ₖ) and the driver swaps the pairs' roles.  v_next / u_next: the
// buffers of vₖ₋₁ / uₖ₋₁, which nothing here reads.  The branches are uniform (device state and a kernel argument).  No reduction:
// the sequence number comes as an argument.
template <int VEC, bool NT>
__global__ __launch_bounds__(kBlock) void trimr_p3_kernel(int64_t n, const TrimrDevState *st, const long long *stop_seq, long long seq,
                                                         double *x, double *y, double *gxo1, double *gxo2, double *gxn1, double *gxn2,
                                                         double *gyo1, double *gyo2, double *gyn1, double *gyn2, const double *v,
                                                         const double *u, const double *q, const double *p, double *v_next,
                                                         double *u_next, int stage) {
  using T = typename VecT<VEC>::type;
  if (seq_skip(stop_seq, seq)) return;
  const TrimrCoef c = {st->row1, st->row2, st->first_scale, st->pi1, st->pi2};
  const double btol = st->btol;
  const bool div_v = st->beta_next > btol, div_u = st->gamma_next > btol;
  const double ib = st->inv_beta_next, ig = st->inv_gamma_next;
  const int64_t nvec = n / VEC;
  const int64_t i = lane_index();
  if (i < nvec) {
    const T vv = ldg<false>(reinterpret_cast<const T *>(v) + i);       // v and u are the next iteration's v_prev and u_prev
    const T uv = ldg<false>(reinterpret_cast<const T *>(u) + i);
    if (stage == 1) {
      T x1, x2, y2, xv, yv;
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        double g1, g2, h2, xe, ye;
        trimr_first(c, vget(vv, e), vget(uv, e), g1, g2, h2, xe, ye);
        vset(x1, e, g1);
        vset(x2, e, g2);
        vset(y2, e, h2);
        vset(xv, e, xe);
        vset(yv, e, ye);
      }
      stg<NT>(x1, reinterpret_cast<T *>(gxn1) + i);
      stg<NT>(x2, reinterpret_cast<T *>(gxn2) + i);
      stg<NT>(y2, reinterpret_cast<T *>(gyn2) + i);
      stg<NT>(xv, reinterpret_cast<T *>(x) + i);
      stg<NT>(yv, reinterpret_cast<T *>(y) + i);
    } else {
      // the x side, then the y side: eight g streams are not all live at once
      {
        const T n1 = ldg<NT>(reinterpret_cast<const T *>(gxn1) + i);
        const T n2 = ldg<NT>(reinterpret_cast<const T *>(gxn2) + i);
        T xv = ldg<NT>(reinterpret_cast<const T *>(x) + i);
        T o1, o2;
        if (stage == 2) {
#pragma unroll
          for (int e = 0; e < VEC; ++e) {
            double a, b;
            trimr_second(c, true, vget(vv, e), vget(n1, e), vget(n2, e), a, b);
            vset(o1, e, a);
            vset(o2, e, b);
          }
        } else {
          o1 = ldg<NT>(reinterpret_cast<const T *>(gxo1) + i);
          o2 = ldg<NT>(reinterpret_cast<const T *>(gxo2) + i);
#pragma unroll
          for (int e = 0; e < VEC; ++e) {
            double a = vget(o1, e), b = vget(o2, e);
            trimr_later(c, true, vget(vv, e), vget(n1, e), vget(n2, e), a, b);
            vset(o1, e, a);
            vset(o2, e, b);
          }
        }
#pragma unroll
        for (int e = 0; e < VEC; ++e) vset(xv, e, fma(c.pi2, vget(o2, e), fma(c.pi1, vget(o1, e), vget(xv, e))));
        stg<NT>(o1, reinterpret_cast<T *>(gxo1) + i);
        stg<NT>(o2, reinterpret_cast<T *>(gxo2) + i);
        stg<NT>(xv, reinterpret_cast<T *>(x) + i);
      }
      {
        const T n1 = ldg<NT>(reinterpret_cast<const T *>(gyn1) + i);   // (zero at k = 2: read all the same)
        const T n2 = ldg<NT>(reinterpret_cast<const T *>(gyn2) + i);
        T yv = ldg<NT>(reinterpret_cast<const T *>(y) + i);
        T o1, o2;
        if (stage == 2) {
#pragma unroll
          for (int e = 0; e < VEC; ++e) {
            double a, b;
            trimr_second(c, false, vget(uv, e), vget(n1, e), vget(n2, e), a, b);
            vset(o1, e, a);
            vset(o2, e, b);
          }
        } else {
          o1 = ldg<NT>(reinterpret_cast<const T *>(gyo1) + i);
          o2 = ldg<NT>(reinterpret_cast<const T *>(gyo2) + i);
#pragma unroll
          for (int e = 0; e < VEC; ++e) {
            double a = vget(o1, e), b = vget(o2, e);
            trimr_later(c, false, vget(uv, e), vget(n1, e), vget(n2, e), a, b);
            vset(o1, e, a);
            vset(o2, e, b);
          }
        }
#pragma unroll
        for (int e = 0; e < VEC; ++e) vset(yv, e, fma(c.pi2, vget(o2, e), fma(c.pi1, vget(o1, e), vget(yv, e))));
        stg<NT>(o1, reinterpret_cast<T *>(gyo1) + i);
        stg<NT>(o2, reinterpret_cast<T *>(gyo2) + i);
        stg<NT>(yv, reinterpret_cast<T *>(y) + i);
      }
    }
    T vo = ldg<NT>(reinterpret_cast<const T *>(q) + i);
    T uo = ldg<NT>(reinterpret_cast<const T *>(p) + i);
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      if (div_v) vset(vo, e, vget(vo, e) * ib);
      if (div_u) vset(uo, e, vget(uo, e) * ig);
    }
    stg<false>(vo, reinterpret_cast<T *>(v_next) + i);                  // read by the next products
    stg<false>(uo, reinterpret_cast<T *>(u_next) + i);
  }
  if (VEC == 2 && owns_tail(n)) {
    const int64_t e = n - 1;
    if (stage == 1) {
      double g1, g2, h2, xe, ye;
      trimr_first(c, v[e], u[e], g1, g2, h2, xe, ye);
      gxn1[e] = g1;
      gxn2[e] = g2;
      gyn2[e] = h2;
      x[e] = xe;
      y[e] = ye;
    } else {
      double a = 0.0, b = 0.0;
      if (stage == 2) {
        trimr_second(c, true, v[e], gxn1[e], gxn2[e], a, b);
      } else {
        a = gxo1[e];
        b = gxo2[e];
        trimr_later(c, true, v[e], gxn1[e], gxn2[e], a, b);
      }
      gxo1[e] = a;
      gxo2[e] = b;
      x[e] = fma(c.pi2, b, fma(c.pi1, a, x[e]));
      if (stage == 2) {
        trimr_second(c, false, u[e], gyn1[e], gyn2[e], a, b);
      } else {
        a = gyo1[e];
        b = gyo2[e];
        trimr_later(c, false, u[e], gyn1[e], gyn2[e], a, b);
      }
      gyo1[e] = a;
      gyo2[e] = b;
      y[e] = fma(c.pi2, b, fma(c.pi1, a, y[e]));
    }
    v_next[e] = div_v ? q[e] * ib : q[e];
    u_next[e] = div_u ? p[e] * ig : p[e];
  }
}

// One broadcast of the primitive sequence (:460-476): out = trimr_g(…) per element, any length, one element per thread.  `out`
// may be one of the a (each element is read before it is written, by its own thread); absent vectors are never read.
__global__ __launch_bounds__(kBlock) void trimr_g_kernel(int64_t n, double *out, const double *w, int nterm, double c0, const double *a0,
                                                        double c1, const double *a1, double c2, const double *a2, double c3,
                                                        const double *a3, double delta) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const double t2 = nterm > 2 ? a2[i] : 0.0, t3 = nterm > 3 ? a3[i] : 0.0;
  out[i] = trimr_g(w != nullptr, nterm, w ? w[i] : 0.0, c0, a0[i], c1, a1[i], c2, t2, c3, t3, delta);
}

}  // namespace khip

namespace {

// P3 takes its sequence number from ctx->ctl, as the reductions do (all zero on the host-driven loop)
struct TrimrG {                              // the eight g of the policy by their current role
  double *gx_m3, *gx_m2, *gx_m1, *gx, *gy_m3, *gy_m2, *gy_m1, *gy;
};
int launch_p3(khip_ctx *ctx, int64_t n, const TrimrDevState *st, double *x, double *y, const TrimrG &g, const double *v, const double *u,
              const double *q, const double *p, double *v_next, double *u_next, int stage) {
  VecPlan L;
  KHIP_TRY(vec_plan(ctx, n, {x, y, g.gx_m3, g.gx_m2, g.gx_m1, g.gx, g.gy_m3, g.gy_m2, g.gy_m1, g.gy, v, u, q, p, v_next, u_next}, &L));
  const SeqCtl ctl = ctx->ctl;
  ProfScope prof_scope(ctx, kProfTrimrP3);
  vec_dispatch_vn<ScalarPathNT::never>(L, [&](auto V, auto N) {
    hipLaunchKernelGGL((trimr_p3_kernel<V, N>), L.grid(), dim3(kBlock), 0, ctx->stream, n, st, ctl.stop_seq, ctl.seq, x, y, g.gx_m3,
                       g.gx_m2, g.gx_m1, g.gx, g.gy_m3, g.gy_m2, g.gy_m1, g.gy, v, u, q, p, v_next, u_next, stage); });
  KHIP_CHECK_HIP(hipGetLastError());
  return KHIP_OK;
}

// one broadcast of path 0; w = nullptr: the row has no right-hand side
int launch_g(khip_ctx *ctx, int64_t n, double *out, const double *w, int nterm, double c0, const double *a0, double c1, const double *a1,
             double c2, const double *a2, double c3, const double *a3, double delta) {
  if (n <= 0) return KHIP_OK;
  KHIP_REQUIRE(nterm >= 2 && nterm <= 4 && out && a0 && a1 && (nterm < 3 || a2) && (nterm < 4 || a3), "trimr: bad g broadcast");
  const int64_t blocks = (n + kBlock - 1) / kBlock;
  KHIP_REQUIRE(blocks <= 0x7fffffffLL, "vector too long for one launch");
  hipLaunchKernelGGL(trimr_g_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, ctx->stream, n, out, w, nterm, c0, a0, c1, a1, c2, a2, c3,
                     a3, delta);
  KHIP_CHECK_HIP(hipGetLastError());
  return KHIP_OK;
}

// the four broadcasts of an iteration k ≥ 2 on one side: (o1, o2) are the older pair's buffers and take (g₂ₖ₋₁, g₂ₖ)
int launch_g_side(khip_ctx *ctx, int64_t n, const TrimrDevState &s, bool x_side, const double *w, double *o1, double *o2, const double *n1,
                  const double *n2, int64_t k) {
  const TrimrRow &a = s.row1, &b = s.row2;
  const double *w1 = x_side ? w : nullptr, *w2 = x_side ? nullptr : w;
  if (k == 2) {
    KHIP_TRY(launch_g(ctx, n, o1, w1, 2, a.eta, n1, a.sigma, n2, 0.0, nullptr, 0.0, nullptr, a.delta));
    KHIP_TRY(launch_g(ctx, n, o2, w2, 3, b.lambda, n1, b.eta, n2, b.sigma, o1, 0.0, nullptr, b.delta));
  } else {
    KHIP_TRY(launch_g(ctx, n, o1, w1, 4, a.mu, o1, a.lambda, o2, a.eta, n1, a.sigma, n2, a.delta));
    KHIP_TRY(launch_g(ctx, n, o2, w2, 4, b.mu, o2, b.lambda, n1, b.eta, n2, b.sigma, o1, b.delta));
  }
  return KHIP_OK;
}

}  // namespace

struct khip_trimr_workspace {
  khip_ctx *ctx;
  int64_t m, n;
  // by their CURRENT role: the fused loops rotate (v_prev, v), (u_prev, u) and the two pairs of g of each side.  y, u_prev, u, p,
  // the four gy and Δy have n entries, the others m
  double *y = nullptr, *u_prev = nullptr, *u = nullptr, *p = nullptr, *gy_m3 = nullptr, *gy_m2 = nullptr, *gy_m1 = nullptr, *gy = nullptr,
         *x = nullptr, *v_prev = nullptr, *v = nullptr, *q = nullptr, *gx_m3 = nullptr, *gx_m2 = nullptr, *gx_m1 = nullptr, *gx = nullptr,
         *dx = nullptr, *dy = nullptr;
  Borrowed borrowed;                        // the caller's vectors (khip_trimr_workspace_adopt*): never freed here
  bool warm_start = false;
  StatsBox box;
  DeviceLoop<TrimrDevState, 3> loop;        // fused loops: device copy of the scalar state, pinned snapshots + staging, history
};

namespace {

// y, N⁻¹uₖ₋₁, N⁻¹uₖ, p, gy₂ₖ₋₃, gy₂ₖ₋₂, gy₂ₖ₋₁, gy₂ₖ, x, M⁻¹vₖ₋₁, M⁻¹vₖ, q, gx₂ₖ₋₃, gx₂ₖ₋₂, gx₂ₖ₋₁, gx₂ₖ come with the workspace; Δx, Δy stay empty
// until a warm start (src/krylov_workspaces.jl, TrimrWorkspace: the table keeps its order; with M = N = I its uₖ and vₖ never exist)
using W = khip_trimr_workspace;
constexpr WsVec<W> kVectors[] = {{"y", &W::y, Core},         {"u_prev", &W::u_prev, Core}, {"u", &W::u, Core},         {"p", &W::p, Core},
                                 {"gy_m3", &W::gy_m3, Core}, {"gy_m2", &W::gy_m2, Core},   {"gy_m1", &W::gy_m1, Core}, {"gy", &W::gy, Core},
                                 {"x", &W::x, Core, RowSide},         {"v_prev", &W::v_prev, Core, RowSide}, {"v", &W::v, Core, RowSide},
                                 {"q", &W::q, Core, RowSide},         {"gx_m3", &W::gx_m3, Core, RowSide},   {"gx_m2", &W::gx_m2, Core, RowSide},
                                 {"gx_m1", &W::gx_m1, Core, RowSide}, {"gx", &W::gx, Core, RowSide},
                                 {"dx", &W::dx, Lazy, RowSide},       {"dy", &W::dy, Lazy}};

// what trimr! adds to the driver of the process (ssy.hpp)
struct Trimr : SsyPolicy<TrimrDevState, W> {
  static constexpr Epilogue kEpiA = EPI_TRIMR_A, kEpiB = EPI_TRIMR_B;
  double *x, *y;
  TrimrG g;                                                                            // the g by their current role
  static void step_a(State &s, double vq) { trimr_step_a(s, vq); }
  static void step_b(State &s, double qq, double pp, int64_t k) { (void)trimr_step_b(s, qq, pp, k); }
  static bool stopped(const State &s) { return s.solved || s.breakdown; }
  // vₖ₊₁ and uₖ₊₁ go where vₖ₋₁ and uₖ₋₁ were
  int p3(khip_ctx *ctx, int64_t n, const State *dev, const SsyRoles &r, int64_t k) const {
    return launch_p3(ctx, n, dev, x, y, g, r.v, r.u, r.q, r.p, r.v_prev, r.u_prev, k < 3 ? (int)k : 3);
  }
  // the @kswap! of :457-459, :470-471 and :477-478: the older and the newer pair of each side change places
  void rotate(int64_t k) {
    if (k >= 2) { std::swap(g.gx_m3, g.gx_m1); std::swap(g.gx_m2, g.gx); std::swap(g.gy_m3, g.gy_m1); std::swap(g.gy_m2, g.gy); }
  }
  void fix_after_device_loop(const State &s) { if (s.iter >= 2 && !(s.iter & 1)) rotate(2); }   // iter - 1 swaps ran
  void store(W *ws) const {
    ws->gx_m3 = g.gx_m3; ws->gx_m2 = g.gx_m2; ws->gx_m1 = g.gx_m1; ws->gx = g.gx;
    ws->gy_m3 = g.gy_m3; ws->gy_m2 = g.gy_m2; ws->gy_m1 = g.gy_m1; ws->gy = g.gy;
  }
  void push_history(W *ws, const State &s) const { ws->box.push(s.rNorm); }                            // :504
  void verbose_row(const khip_options &o, long long iter, const State &s, double t0) const {            // :554
    klogf(o.log_fd, "%5lld  %7.1e  %7.1e  %7.1e  %.2fs\n", iter, s.rNorm, s.beta_next, s.gamma_next, now_s() - t0);
  }
  // the g (:446-479), x and y (:495-500), then the shift of v and u (:326, :334, :511-516), on the primitives in the reference's
  // order.  The two norms come earlier here (the head); kdiv!(q) and kdiv!(p) come after the g, which read neither.
  int primitive_tail(Ssy<Trimr> &L, int64_t k) {
    W *ws = L.ws;
    khip_ctx *ctx = L.ctx;
    const int64_t m = L.m, n = L.n;
    const State &s = L.s;
    if (k == 1) {
      K(khip_divcopy(ctx, m, g.gx_m1, L.r.v, s.row1.delta));
      K(khip_scalcopy(ctx, m, g.gx, s.first_scale, g.gx_m1));
      K(khip_divcopy(ctx, n, g.gy, L.r.u, s.row2.delta));
    } else {
      K(launch_g_side(ctx, m, s, true, L.r.v, g.gx_m3, g.gx_m2, g.gx_m1, g.gx, k));
      K(launch_g_side(ctx, n, s, false, L.r.u, g.gy_m3, g.gy_m2, g.gy_m1, g.gy, k));
      rotate(k);
    }
    K(khip_axpy(ctx, m, s.pi1, g.gx_m1, x));
    K(khip_axpy(ctx, m, s.pi2, g.gx, x));
    K(khip_axpy(ctx, n, s.pi1, g.gy_m1, y));
    K(khip_axpy(ctx, n, s.pi2, g.gy, y));
    if (s.beta_next > s.btol) K(khip_div(ctx, m, L.r.q, s.beta_next));
    if (s.gamma_next > s.btol) K(khip_div(ctx, n, L.r.p, s.gamma_next));
    K(khip_copy(ctx, m, L.r.v_prev, L.r.v));
    K(khip_copy(ctx, n, L.r.u_prev, L.r.u));
    K(khip_copy(ctx, m, L.r.v, L.r.q));
    K(khip_copy(ctx, n, L.r.u, L.r.p));
    return KHIP_OK;
  }
};

}  // namespace

extern "C" {

khip_trimr_params khip_trimr_default_params(void) {
  khip_trimr_params p;
  p.tau = 1.0;
  p.nu = -1.0;
  p.spd = p.snd = p.flip = p.sp = 0;
  return p;
}

int khip_trimr_workspace_create(khip_ctx *ctx, int64_t m, int64_t n, khip_trimr_workspace **out) {
  return ws_create(ctx, m, n, kVectors, "trimr_workspace_create", khip_trimr_workspace_destroy, out);
}

int khip_trimr_workspace_adopt(khip_ctx *ctx, int64_t m, int64_t n, double *y, double *u_prev, double *u, double *p, double *gy_m3,
                               double *gy_m2, double *gy_m1, double *gy, double *x, double *v_prev, double *v, double *q, double *gx_m3,
                               double *gx_m2, double *gx_m1, double *gx, khip_trimr_workspace **out) {
  return ws_adopt(ctx, m, n, kVectors, "trimr_workspace_adopt",
                  {y, u_prev, u, p, gy_m3, gy_m2, gy_m1, gy, x, v_prev, v, q, gx_m3, gx_m2, gx_m1, gx}, out);
}

int khip_trimr_workspace_adopt_vector(khip_trimr_workspace *ws, const char *name, double *ptr) {
  return ws_adopt_vector(ws, kVectors, "trimr_workspace_adopt_vector", name, ptr);
}

int khip_trimr_workspace_destroy(khip_trimr_workspace *ws) {
  if (!ws) return KHIP_OK;
  ws_free_vectors(ws, kVectors);
  ws->loop.release();
  delete ws;
  return KHIP_OK;
}

int khip_trimr_warm_start(khip_trimr_workspace *ws, const double *x0, const double *y0) {   // Δx of m entries, Δy of n
  return ws_warm_start2(ws, kVectors, x0, y0, "trimr_warm_start");
}

double *khip_trimr_solution_x(khip_trimr_workspace *ws) { return ws ? ws->x : nullptr; }
double *khip_trimr_solution_y(khip_trimr_workspace *ws) { return ws ? ws->y : nullptr; }
const khip_stats *khip_trimr_stats(khip_trimr_workspace *ws) { return ws ? &ws->box.st : nullptr; }
int khip_trimr_last_path(khip_trimr_workspace *ws) { return ws ? ws->box.path : -1; }
double *khip_trimr_vector(khip_trimr_workspace *ws, const char *name) { return ws_vector(ws, kVectors, name); }
size_t khip_trimr_workspace_bytes(khip_trimr_workspace *ws) { return ws_bytes(ws, kVectors); }

int khip_trimr_solve(khip_trimr_workspace *ws, const khip_operator *A, const khip_operator *At, const double *b, const double *c,
                     const khip_options *opts_in, const khip_trimr_params *params_in) {
  KHIP_REQUIRE(ws && A && b, "trimr_solve: null argument");
  khip_trimr_params prm = params_in ? *params_in : khip_trimr_default_params();
  Ssy<Trimr> L(ws, A, At, opts_in);
  khip_ctx *ctx = L.ctx;
  const khip_options &o = L.o;
  const int64_t m = L.m, n = L.n;
  TrimrDevState &s = L.s;
  const double atol = tol_or_default(o.atol), rtol = tol_or_default(o.rtol);

  if (int rc = L.check("trimr", c)) return rc;                                                            // :156-159
  if (o.verbose > 0)                                                                                      // :160
    klogf(o.log_fd, "TriMR: system of %lld equations in %lld variables\n", (long long)(m + n), (long long)(m + n));
  if (prm.spd && prm.flip)                                                                                // :163-168
    return ws->box.fail(KHIP_ERR_INVALID, "The matrix cannot be symmetric positive definite and symmetric quasi-definite !");
  if (prm.spd && prm.snd)
    return ws->box.fail(KHIP_ERR_INVALID, "The matrix cannot be symmetric positive definite and symmetric negative definite !");
  if (prm.spd && prm.sp) return ws->box.fail(KHIP_ERR_INVALID, "The matrix cannot be symmetric positive definite and a saddle-point !");
  if (prm.snd && prm.flip)
    return ws->box.fail(KHIP_ERR_INVALID, "The matrix cannot be symmetric negative definite and symmetric quasi-definite !");
  if (prm.snd && prm.sp) return ws->box.fail(KHIP_ERR_INVALID, "The matrix cannot be symmetric negative definite and a saddle-point !");
  if (prm.sp && prm.flip) return ws->box.fail(KHIP_ERR_INVALID, "The matrix cannot be symmetric quasi-definite and a saddle-point !");
  if (prm.flip) { prm.tau = -1.0; prm.nu = 1.0; }                                                         // :180-183
  if (prm.spd) { prm.tau = 1.0; prm.nu = 1.0; }
  if (prm.snd) { prm.tau = -1.0; prm.nu = -1.0; }
  if (prm.sp) { prm.tau = 1.0; prm.nu = 0.0; }
  const double tau = prm.tau, nu = prm.nu;
  const bool warm_start = ws->warm_start;
  ws->box.reset();                                                                                        // reset!(stats)
  double *x = L.pol.x = ws->x, *y = L.pol.y = ws->y;
  TrimrG &g = L.pol.g;
  g = TrimrG{ws->gx_m3, ws->gx_m2, ws->gx_m1, ws->gx, ws->gy_m3, ws->gy_m2, ws->gy_m1, ws->gy};

  // set-up, the same primitives on every path (:211-294)
  K(khip_fill(ctx, m, x, 0.0));
  K(khip_fill(ctx, n, y, 0.0));
  L.itmax = o.itmax == 0 ? global_rows(ctx, A, m) + global_rows(ctx, At, n) : o.itmax;                    // m + n of the global system (:215)
  K(khip_fill(ctx, m, L.r.v_prev, 0.0));
  K(khip_fill(ctx, n, L.r.u_prev, 0.0));
  const double *b0 = b, *c0 = c;
  if (warm_start) {                                                                                       // :223-230
    K(apply_op(ctx, A, ws->dy, L.r.q));
    if (tau != 0) K(khip_axpy(ctx, m, tau, ws->dx, L.r.q));
    K(khip_axpby(ctx, m, 1.0, b, -1.0, L.r.q));
    K(apply_op(ctx, At, ws->dx, L.r.p));
    if (nu != 0) K(khip_axpy(ctx, n, nu, ws->dy, L.r.p));
    K(khip_axpby(ctx, n, 1.0, c, -1.0, L.r.p));
    b0 = L.r.q;
    c0 = L.r.p;
  }
  double beta1, gamma1;
  K(khip_copy(ctx, m, L.r.v, b0));                                                                        // :233-243
  K(khip_nrm2(ctx, m, L.r.v, &beta1));
  if (beta1 != 0) K(khip_div(ctx, m, L.r.v, beta1));
  else K(khip_fill(ctx, m, L.r.v, 0.0));
  K(khip_copy(ctx, n, L.r.u, c0));                                                                        // :246-256
  K(khip_nrm2(ctx, n, L.r.u, &gamma1));
  if (gamma1 != 0) K(khip_div(ctx, n, L.r.u, gamma1));
  else K(khip_fill(ctx, n, L.r.u, 0.0));
  K(khip_fill(ctx, m, g.gx_m3, 0.0));                                                                     // :259-266
  K(khip_fill(ctx, n, g.gy_m3, 0.0));
  K(khip_fill(ctx, m, g.gx_m2, 0.0));
  K(khip_fill(ctx, n, g.gy_m2, 0.0));
  K(khip_fill(ctx, m, g.gx_m1, 0.0));
  K(khip_fill(ctx, n, g.gy_m1, 0.0));
  K(khip_fill(ctx, m, g.gx, 0.0));
  K(khip_fill(ctx, n, g.gy, 0.0));
  const double rNorm = std::sqrt(gamma1 * gamma1 + beta1 * beta1);                                        // :269-271
  if (L.history) ws->box.push(rNorm);
  s.beta = beta1;
  s.gamma = gamma1;
  s.beta_next = beta1;
  s.gamma_next = gamma1;
  s.tau = tau;
  s.nu = nu;
  s.eps_tol = atol + rtol * rNorm;
  s.pibar1 = beta1;                                                                                       // :280-281
  s.pibar2 = gamma1;
  s.btol = 0x1p-39;                                                                                       // eps(Float64)^(3/4) (:284)
  s.rNorm = rNorm;
  s.stop_seq = kSeqNever;
  s.solved = (rNorm <= s.eps_tol) ? 1 : 0;                                                                // :288
  ws->box.path = (o.fused && L.square()) ? 1 : 0;
  if (o.verbose > 0) {                                                                                    // :273-274 (labels padded by hand)
    klogf(o.log_fd, "%5s  %s  %s  %s  %5s\n", "k", "   \xe2\x80\x96r\xe2\x82\x96\xe2\x80\x96", "   \xce\xb2\xe2\x82\x96\xe2\x82\x8a\xe2\x82\x81",
          "   \xce\xb3\xe2\x82\x96\xe2\x82\x8a\xe2\x82\x81", "timer");
    if (kdisplay(0, o.verbose)) klogf(o.log_fd, "%5d  %7.1e  %7.1e  %7.1e  %.2fs\n", 0, rNorm, beta1, gamma1, now_s() - L.t0);
  }

  K(L.iterate());                                                                                         // :296-555

  const char *status = "unknown";                                                                         // :559-563
  if (L.tired) status = "maximum number of iterations exceeded";
  if (s.breakdown) status = "inconsistent linear system";
  if (s.solved) status = "solution good enough given atol and rtol";
  if (L.user_exit) status = "user-requested exit";
  if (L.overtimed) status = "time limit exceeded";
  if (warm_start) {                                                                                       // :566-567: Δx has m entries, Δy has n
    K(khip_axpy(ctx, m, 1.0, ws->dx, ws->x));
    K(khip_axpy(ctx, n, 1.0, ws->dy, ws->y));
  }
  return L.end(s.solved ? 1 : 0, (!s.solved && s.breakdown) ? 1 : 0, status, false);                      // :568-575
}

// ---- test-only exports (include/krylov_hip_test.h) --------------------------------------------------------------------------
// P3 at a given stage with the caller's coefficients: coef16 = row one (μ, λ, η, σ, δ), row two (μ, λ, η, σ, δ), −σ₁ / δ₂, π₂ₖ₋₁, π₂ₖ, βₖ₊₁,
// γₖ₊₁, btol; g8 = gx₂ₖ₋₃, gx₂ₖ₋₂, gx₂ₖ₋₁, gx₂ₖ, gy₂ₖ₋₃, gy₂ₖ₋₂, gy₂ₖ₋₁, gy₂ₖ by their role as the iteration begins.
int khip_test_trimr_p3(khip_ctx *ctx, int64_t n, int stage, const double *coef16, double *x, double *y, double *const *g8, const double *v,
                       const double *u, const double *q, const double *p, double *v_next, double *u_next) {
  KHIP_REQUIRE(ctx && n >= 0 && stage >= 1 && stage <= 3 && coef16 && x && y && g8 && v && u && q && p && v_next && u_next,
               "test_trimr_p3: bad argument");
  for (int i = 0; i < 8; ++i) KHIP_REQUIRE(g8[i] != nullptr, "test_trimr_p3: bad argument");
  TrimrDevState h;
  memset(&h, 0, sizeof(h));
  h.row1 = TrimrRow{coef16[0], coef16[1], coef16[2], coef16[3], coef16[4]};
  h.row2 = TrimrRow{coef16[5], coef16[6], coef16[7], coef16[8], coef16[9]};
  h.first_scale = coef16[10];
  h.pi1 = coef16[11];
  h.pi2 = coef16[12];
  h.beta_next = coef16[13];
  h.gamma_next = coef16[14];
  h.btol = coef16[15];
  h.inv_beta_next = 1.0 / h.beta_next;
  h.inv_gamma_next = 1.0 / h.gamma_next;
  h.stop_seq = kSeqNever;
  TrimrDevState *dev = nullptr;
  KHIP_CHECK_HIP(hipMalloc(&dev, sizeof(h)));
  int rc = KHIP_OK;
  if (hipMemcpy(dev, &h, sizeof(h), hipMemcpyHostToDevice) != hipSuccess) rc = KHIP_ERR_HIP;
  const SeqCtl keep = ctx->ctl;
  ctx->ctl = SeqCtl{};
  if (rc == KHIP_OK && n > 0)
    rc = launch_p3(ctx, n, dev, x, y, TrimrG{g8[0], g8[1], g8[2], g8[3], g8[4], g8[5], g8[6], g8[7]}, v, u, q, p, v_next, u_next, stage);
  ctx->ctl = keep;
  if (hipStreamSynchronize(ctx->stream) != hipSuccess && rc == KHIP_OK) rc = KHIP_ERR_HIP;
  (void)hipFree(dev);
  return rc;
}

// one broadcast of path 0: out = (w − c[0] a0 − c[1] a1 [− c[2] a2 [− c[3] a3]]) / delta, w = NULL: −(c[0] a0) in front
int khip_test_trimr_g(khip_ctx *ctx, int64_t n, double *out, const double *w, int nterm, const double *coef4, const double *a0,
                      const double *a1, const double *a2, const double *a3, double delta) {
  KHIP_REQUIRE(ctx && n >= 0 && coef4, "test_trimr_g: bad argument");
  KHIP_TRY(launch_g(ctx, n, out, w, nterm, coef4[0], a0, coef4[1], a1, coef4[2], a2, coef4[3], a3, delta));
  KHIP_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  return KHIP_OK;
}

}  // extern "C"
