// tricg.cpp -- tricg! (src/tricg.jl:149-484) above the device primitives, with its fused gfx950 kernel.
//
// Real Float64, A of m rows and n columns, M = N = I.  The orthogonal tridiagonalisation of Saunders, Simon and Yip, started from
// b and c, gives the Galerkin iterate of the 2 × 2 block system
//   [ τI   A ] [x]   [b]
//   [ Aᴴ  νI ] [y] = [c]          x, b of m entries ; y, c of n entries
// (symmetric quasi-definite, saddle-point, regularised least-squares and least-norm systems) through an LDLᴴ factorisation in
// scalars.  Three loops, chosen as for its siblings (khip_tricg_last_path):
//   0  options.fused = 0, and every m ≠ n system: the reference's primitive sequence, one launch per k* call, one host sync per
//      kdot / knorm;
//   1  the host-driven loop on the fused kernels (a user operator, a callback or verbose > 0);
//   2  the device-resident loop (default; A and Aᴴ both CSR handles): the scalar recurrences and stopping tests run as the
//      epilogues of the two reductions of an iteration (tricg_step_a/b, solver_device.hpp), iterations are enqueued ahead.
// One iteration on the fused paths (m = n), after q = A uₖ and p = Aᴴ vₖ:
//   P1   k ≥ 2: q = fma(-γₖ, vₖ₋₁, q) ; p = fma(-βₖ, uₖ₋₁, p) ; vₖ.q                    (ssy.hpp)                   56n bytes
//        epilogue A: the whole LDLᴴ update (d₂ₖ₋₁, δₖ, d₂ₖ, from k = 2 on σₖ, ηₖ, λₖ) and π₂ₖ₋₁, π₂ₖ: none of it needs the norms
//   P2   q = fma(-αₖ, vₖ, q) ; p = fma(-αₖ, uₖ, p) ; (q.q, p.p)                        (ssy.hpp)                   48n bytes
//        epilogue B: βₖ₊₁, γₖ₊₁, ζ₂ₖ₋₁, ‖rₖ‖, the shift of the "previous" scalars, breakdown and solved
//   P3   k = 1: gx₁ = v₁ ; gx₂ = -δ₁ gx₁ ; gy₂ = u₁ (gy₁ keeps the zeros of the set-up)                              88n bytes
//        k ≥ 2: the seven primitives of :384-392 per element, (g₂ₖ₋₃, g₂ₖ₋₂) -> (g₂ₖ, g₂ₖ₋₁) in place                  144n bytes
//        every k: x = fma(π₂ₖ, gx₂ₖ, fma(π₂ₖ₋₁, gx₂ₖ₋₁, x)), y likewise ; vₖ₊₁ = βₖ₊₁ > btol ? q (1 / βₖ₊₁) : q ; uₖ₊₁ likewise
//        k ≥ 2 reads  vₖ, uₖ, four g, x, y, q, p (10) ; writes four g, x, y, vₖ₊₁, uₖ₊₁ (8)
//        k = 1 reads  vₖ, uₖ, q, p (4) ; writes gx₁, gx₂, gy₂, x, y, vₖ₊₁, uₖ₊₁ (7)
// That is 248n beside the two products, against 480n for the primitive sequence: two kaxpy! of P1 (48n), kdot (16n), two kaxpy!
// of P2 (48n), two kcopy! (32n), two kaxpby! (48n), kaxpby! and kscal! (40n), kaxpby! (24n), kaxpby! and kaxpy! (48n), four
// kaxpy! into x and y (96n), two knorm (16n), two kdiv! (32n), two kcopy! (32n).
// kcopy!(vₖ₋₁, vₖ), kcopy!(uₖ₋₁, uₖ) and the two @kswap! become rotations of the buffers' roles (vₖ₊₁ and uₖ₊₁ are written where vₖ₋₁
// and uₖ₋₁ were; the buffer of g₂ₖ₋₃ takes g₂ₖ and the buffer of g₂ₖ₋₂ takes g₂ₖ₋₁).  Every elementwise value uses the expression of the
// primitive it replaces (fma for kaxpy!, fma(a, x, b y) for kaxpby!, a x for kscal! and kscalcopy!, x (1 / a) for kdiv!): the
// fused loops agree with the primitive sequence bit for bit on elementwise values and to the reductions' one ulp otherwise;
// loops 1 and 2 run the same kernels and the same scalar code and produce the same bits.
// P3 does NOT write q / βₖ₊₁ back into q (nor p): on the fused paths "q" and "p" hold the undivided vectors after an iteration,
// on path 0 the divided ones, as in the reference.  No other name differs.
// Where tricg! leaves the driver: x has m entries and y has n (the siblings have x on the n side), so the warm start's Δx and Δy
// are added here and Ssy::end gets warm_start = false; the start gives v₁ = 0 by a fill when β₁ = 0 (likewise u₁), so b = 0 or
// c = 0 is an ordinary solve; the shift's guards are > btol, and a vector that is not divided is still taken over.
// Out of scope: M and N other than I, complex types, fused kernels for m ≠ n, a P2 that carries P3's work.
// This file owns P3, the set-up, the g, x and y part of a primitive iteration and the status strings; the loops are ssy.hpp's.
#include "ssy.hpp"   // P1, P2 and the driver of the three loops

using namespace khip;

namespace khip {   // (named, not anonymous: stable kernel names in traces)

// ---------------------------------------------------------------------------------------------------------- kernels ----
// Each thread owns one VEC-vector of every stream; the odd tail element (VEC = 2, n odd) goes to thread 0 of block 0.
// Cache hints, the rule of ssy.hpp: a load is non-temporal when it is the LAST read of that data (the four g, x, y: overwritten
// here; q, p: overwritten by the next products); vₖ and uₖ are read again by the next P1 (as vₖ₋₁, uₖ₋₁) and stay cacheable.  A
// store is non-temporal when nothing reads it before the next iteration's P3 (the four g, x, y); vₖ₊₁ and uₖ₊₁ are read by the
// next products.

// the g, x and y of one element.  ga / gb: the buffers whose roles are (g₂ₖ₋₁, g₂ₖ) when the iteration begins, that is, they hold
// (g₂ₖ₋₃, g₂ₖ₋₂); on return ga holds g₂ₖ and gb holds g₂ₖ₋₁ (the driver swaps the roles).  w: vₖ for the x side, uₖ for the y side.
//   x side (:384, :387, :390): ga = fma(λ, gb, η ga) ; gb = fma(1, v, -σ gb) ; ga = fma(-δ, gb, -1 ga)
//   y side (:385, :388, :391-392): ga = fma(λ, gb, η ga) ; gb = -σ gb ; ga = fma(1, u, -1 ga) ; ga = fma(-δ, gb, ga)
struct TricgCoef {
  double eta, lambda, neg_sigma, neg_delta, pi1, pi2;
};
__device__ __forceinline__ void tricg_gx(const TricgCoef &c, double v, double &ga, double &gb, double &x) {
  ga = fma(c.lambda, gb, c.eta * ga);
  gb = fma(1.0, v, c.neg_sigma * gb);
  ga = fma(c.neg_delta, gb, -1.0 * ga);
  x = fma(c.pi2, ga, fma(c.pi1, gb, x));
}
__device__ __forceinline__ void tricg_gy(const TricgCoef &c, double u, double &ga, double &gb, double &y) {
  ga = fma(c.lambda, gb, c.eta * ga);
  gb = c.neg_sigma * gb;
  ga = fma(1.0, u, -1.0 * ga);
  ga = fma(c.neg_delta, gb, ga);
  y = fma(c.pi2, ga, fma(c.pi1, gb, y));
}
// k = 1 (:367-369, :400-405): x and y are zero and are not read; gy₁ is zero and is neither read nor written
__device__ __forceinline__ void tricg_first(const TricgCoef &c, double v, double u, double &gx1, double &gx2, double &gy2, double &x,
                                            double &y) {
  gx1 = v;
  gx2 = c.neg_delta * gx1;
  gy2 = u;
  x = fma(c.pi2, gx2, fma(c.pi1, gx1, 0.0));
  y = fma(c.pi2, gy2, fma(c.pi1, 0.0, 0.0));
}

// P3 (:364-432).  first: iteration 1.  gxa, gya: the buffers of the roles (gx₂ₖ₋₁, gy₂ₖ₋₁) as the iteration begins; gxb, gyb: those of
// (gx₂ₖ, gy₂ₖ).  At k = 1 the roles are the final ones (no swap), from k = 2 on a holds g₂ₖ and b holds g₂ₖ₋₁ on return.
// v_next / u_next: the buffers of vₖ₋₁ / uₖ₋₁, which nothing here reads.  The branches are uniform (device state and a kernel
// argument).  No reduction: the sequence number comes as an argument.
template <int VEC, bool NT>
__global__ __launch_bounds__(kBlock) void tricg_p3_kernel(int64_t n, const TricgDevState *st, const long long *stop_seq, long long seq,
                                                         double *x, double *y, double *gxa, double *gxb, double *gya, double *gyb,
                                                         const double *v, const double *u, const double *q, const double *p,
                                                         double *v_next, double *u_next, int first) {
  using T = typename VecT<VEC>::type;
  if (seq_skip(stop_seq, seq)) return;
  const TricgCoef c = {st->eta, st->lambda, st->neg_sigma, st->neg_delta, st->pi1, st->pi2};
  const double btol = st->btol;
  const bool div_v = st->beta_next > btol, div_u = st->gamma_next > btol;
  const double ib = st->inv_beta_next, ig = st->inv_gamma_next;
  const int64_t nvec = n / VEC;
  const int64_t i = lane_index();
  if (i < nvec) {
    const T vv = ldg<false>(reinterpret_cast<const T *>(v) + i);       // v and u are the next iteration's v_prev and u_prev
    const T uv = ldg<false>(reinterpret_cast<const T *>(u) + i);
    T xa, xb, ya, yb, xv, yv;
    if (first) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        double g1, g2, h2, xe, ye;
        tricg_first(c, vget(vv, e), vget(uv, e), g1, g2, h2, xe, ye);
        vset(xa, e, g1);
        vset(xb, e, g2);
        vset(yb, e, h2);
        vset(xv, e, xe);
        vset(yv, e, ye);
      }
    } else {
      xa = ldg<NT>(reinterpret_cast<const T *>(gxa) + i);
      xb = ldg<NT>(reinterpret_cast<const T *>(gxb) + i);
      ya = ldg<NT>(reinterpret_cast<const T *>(gya) + i);
      yb = ldg<NT>(reinterpret_cast<const T *>(gyb) + i);
      xv = ldg<NT>(reinterpret_cast<const T *>(x) + i);
      yv = ldg<NT>(reinterpret_cast<const T *>(y) + i);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        double a = vget(xa, e), b = vget(xb, e), xe = vget(xv, e);
        tricg_gx(c, vget(vv, e), a, b, xe);
        vset(xa, e, a);
        vset(xb, e, b);
        vset(xv, e, xe);
        double ay = vget(ya, e), by = vget(yb, e), ye = vget(yv, e);
        tricg_gy(c, vget(uv, e), ay, by, ye);
        vset(ya, e, ay);
        vset(yb, e, by);
        vset(yv, e, ye);
      }
      stg<NT>(ya, reinterpret_cast<T *>(gya) + i);
    }
    stg<NT>(xa, reinterpret_cast<T *>(gxa) + i);
    stg<NT>(xb, reinterpret_cast<T *>(gxb) + i);
    stg<NT>(yb, reinterpret_cast<T *>(gyb) + i);
    stg<NT>(xv, reinterpret_cast<T *>(x) + i);
    stg<NT>(yv, reinterpret_cast<T *>(y) + i);
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
    if (first) {
      double g1, g2, h2, xe, ye;
      tricg_first(c, v[e], u[e], g1, g2, h2, xe, ye);
      gxa[e] = g1;
      gxb[e] = g2;
      gyb[e] = h2;
      x[e] = xe;
      y[e] = ye;
    } else {
      double a = gxa[e], b = gxb[e], xe = x[e];
      tricg_gx(c, v[e], a, b, xe);
      gxa[e] = a;
      gxb[e] = b;
      x[e] = xe;
      double ay = gya[e], by = gyb[e], ye = y[e];
      tricg_gy(c, u[e], ay, by, ye);
      gya[e] = ay;
      gyb[e] = by;
      y[e] = ye;
    }
    v_next[e] = div_v ? q[e] * ib : q[e];
    u_next[e] = div_u ? p[e] * ig : p[e];
  }
}

}  // namespace khip

namespace {

// P3 takes its sequence number from ctx->ctl, as the reductions do (all zero on the host-driven loop)
int launch_p3(khip_ctx *ctx, int64_t n, const TricgDevState *st, double *x, double *y, double *gxa, double *gxb, double *gya, double *gyb,
              const double *v, const double *u, const double *q, const double *p, double *v_next, double *u_next, bool first) {
  VecPlan L;
  KHIP_TRY(vec_plan(ctx, n, {x, y, gxa, gxb, gya, gyb, v, u, q, p, v_next, u_next}, &L));
  const SeqCtl ctl = ctx->ctl;
  ProfScope prof_scope(ctx, kProfTricgP3);
  vec_dispatch_vn<ScalarPathNT::never>(L, [&](auto V, auto N) {
    hipLaunchKernelGGL((tricg_p3_kernel<V, N>), L.grid(), dim3(kBlock), 0, ctx->stream, n, st, ctl.stop_seq, ctl.seq, x, y, gxa, gxb,
                       gya, gyb, v, u, q, p, v_next, u_next, first ? 1 : 0); });
  KHIP_CHECK_HIP(hipGetLastError());
  return KHIP_OK;
}

}  // namespace

struct khip_tricg_workspace {
  khip_ctx *ctx;
  int64_t m, n;
  // by their CURRENT role: the fused loops rotate (v_prev, v), (u_prev, u), (gx_prev, gx) and (gy_prev, gy).  y, u_prev, u, p,
  // gy_prev, gy and Δy have n entries, the others m
  double *y = nullptr, *u_prev = nullptr, *u = nullptr, *p = nullptr, *gy_prev = nullptr, *gy = nullptr, *x = nullptr, *v_prev = nullptr,
         *v = nullptr, *q = nullptr, *gx_prev = nullptr, *gx = nullptr, *dx = nullptr, *dy = nullptr;
  Borrowed borrowed;                        // the caller's vectors (khip_tricg_workspace_adopt*): never freed here
  bool warm_start = false;
  StatsBox box;
  DeviceLoop<TricgDevState, 3> loop;        // fused loops: device copy of the scalar state, pinned snapshots + staging, history
};

namespace {

// y, N⁻¹uₖ₋₁, N⁻¹uₖ, p, gy₂ₖ₋₁, gy₂ₖ, x, M⁻¹vₖ₋₁, M⁻¹vₖ, q, gx₂ₖ₋₁, gx₂ₖ come with the workspace; Δx, Δy stay empty until a warm start
// (src/krylov_workspaces.jl, TricgWorkspace: the table keeps its order; with M = N = I its uₖ and vₖ never exist)
using W = khip_tricg_workspace;
constexpr WsVec<W> kVectors[] = {{"y", &W::y, Core},             {"u_prev", &W::u_prev, Core},            {"u", &W::u, Core},
                                 {"p", &W::p, Core},             {"gy_prev", &W::gy_prev, Core},          {"gy", &W::gy, Core},
                                 {"x", &W::x, Core, RowSide},    {"v_prev", &W::v_prev, Core, RowSide},   {"v", &W::v, Core, RowSide},
                                 {"q", &W::q, Core, RowSide},    {"gx_prev", &W::gx_prev, Core, RowSide}, {"gx", &W::gx, Core, RowSide},
                                 {"dx", &W::dx, Lazy, RowSide},  {"dy", &W::dy, Lazy}};

// what tricg! adds to the driver of the process (ssy.hpp)
struct Tricg : SsyPolicy<TricgDevState, W> {
  static constexpr Epilogue kEpiA = EPI_TRICG_A, kEpiB = EPI_TRICG_B;
  double *x, *y, *gx_prev, *gx, *gy_prev, *gy;                                         // the g by their current role
  static void step_a(State &s, double vq) { tricg_step_a(s, vq); }
  static void step_b(State &s, double qq, double pp, int64_t k) { (void)tricg_step_b(s, qq, pp, k); }
  static bool stopped(const State &s) { return s.solved || s.breakdown; }
  // vₖ₊₁ and uₖ₊₁ go where vₖ₋₁ and uₖ₋₁ were
  int p3(khip_ctx *ctx, int64_t n, const State *dev, const SsyRoles &r, int64_t k) const {
    return launch_p3(ctx, n, dev, x, y, gx_prev, gx, gy_prev, gy, r.v, r.u, r.q, r.p, r.v_prev, r.u_prev, k == 1);
  }
  // @kswap!(gx₂ₖ₋₁, gx₂ₖ) ; @kswap!(gy₂ₖ₋₁, gy₂ₖ) (:395-396)
  void rotate(int64_t k) { if (k >= 2) { std::swap(gx_prev, gx); std::swap(gy_prev, gy); } }
  void fix_after_device_loop(const State &s) { if (s.iter >= 2 && !(s.iter & 1)) rotate(2); }   // iter - 1 swaps ran
  void store(W *ws) const { ws->gx_prev = gx_prev; ws->gx = gx; ws->gy_prev = gy_prev; ws->gy = gy; }
  void push_history(W *ws, const State &s) const { ws->box.push(s.rNorm); }                            // :438
  void verbose_row(const khip_options &o, long long iter, const State &s, double t0) const {            // :461
    klogf(o.log_fd, "%5lld  %7.1e  %7.1e  %7.1e  %.2fs\n", iter, s.rNorm, s.beta_next, s.gamma_next, now_s() - t0);
  }
  // the g (:364-397), x and y (:400-405), then the shift of v and u (:304-305, :415-432), on the primitives in the reference's
  // order.  The two norms come earlier here (the head): nothing between reads or writes what they depend on.
  int primitive_tail(Ssy<Tricg> &L, int64_t k) {
    W *ws = L.ws;
    khip_ctx *ctx = L.ctx;
    const int64_t m = L.m, n = L.n;
    const State &s = L.s;
    if (k == 1) {
      K(khip_copy(ctx, m, gx_prev, L.r.v));
      K(khip_scalcopy(ctx, m, gx, s.neg_delta, gx_prev));
      K(khip_copy(ctx, n, gy, L.r.u));
    } else {
      K(khip_axpby(ctx, m, s.lambda, gx, s.eta, gx_prev));
      K(khip_axpby(ctx, n, s.lambda, gy, s.eta, gy_prev));
      K(khip_axpby(ctx, m, 1.0, L.r.v, s.neg_sigma, gx));
      K(khip_scal(ctx, n, s.neg_sigma, gy));
      K(khip_axpby(ctx, m, s.neg_delta, gx, -1.0, gx_prev));
      K(khip_axpby(ctx, n, 1.0, L.r.u, -1.0, gy_prev));
      K(khip_axpy(ctx, n, s.neg_delta, gy, gy_prev));
      rotate(k);
    }
    K(khip_axpy(ctx, m, s.pi1, gx_prev, x));
    K(khip_axpy(ctx, m, s.pi2, gx, x));
    K(khip_axpy(ctx, n, s.pi1, gy_prev, y));
    K(khip_axpy(ctx, n, s.pi2, gy, y));
    K(khip_copy(ctx, m, L.r.v_prev, L.r.v));
    K(khip_copy(ctx, n, L.r.u_prev, L.r.u));
    if (s.beta_next > s.btol) K(khip_div(ctx, m, L.r.q, s.beta_next));
    if (s.gamma_next > s.btol) K(khip_div(ctx, n, L.r.p, s.gamma_next));
    K(khip_copy(ctx, m, L.r.v, L.r.q));
    K(khip_copy(ctx, n, L.r.u, L.r.p));
    return KHIP_OK;
  }
};

}  // namespace

extern "C" {

khip_tricg_params khip_tricg_default_params(void) {
  khip_tricg_params p;
  p.tau = 1.0;
  p.nu = -1.0;
  p.spd = p.snd = p.flip = 0;
  return p;
}

int khip_tricg_workspace_create(khip_ctx *ctx, int64_t m, int64_t n, khip_tricg_workspace **out) {
  return ws_create(ctx, m, n, kVectors, "tricg_workspace_create", khip_tricg_workspace_destroy, out);
}

int khip_tricg_workspace_adopt(khip_ctx *ctx, int64_t m, int64_t n, double *y, double *u_prev, double *u, double *p, double *gy_prev,
                               double *gy, double *x, double *v_prev, double *v, double *q, double *gx_prev, double *gx,
                               khip_tricg_workspace **out) {
  return ws_adopt(ctx, m, n, kVectors, "tricg_workspace_adopt", {y, u_prev, u, p, gy_prev, gy, x, v_prev, v, q, gx_prev, gx}, out);
}

int khip_tricg_workspace_adopt_vector(khip_tricg_workspace *ws, const char *name, double *ptr) {
  return ws_adopt_vector(ws, kVectors, "tricg_workspace_adopt_vector", name, ptr);
}

int khip_tricg_workspace_destroy(khip_tricg_workspace *ws) {
  if (!ws) return KHIP_OK;
  ws_free_vectors(ws, kVectors);
  ws->loop.release();
  delete ws;
  return KHIP_OK;
}

int khip_tricg_warm_start(khip_tricg_workspace *ws, const double *x0, const double *y0) {   // Δx of m entries, Δy of n
  return ws_warm_start2(ws, kVectors, x0, y0, "tricg_warm_start");
}

double *khip_tricg_solution_x(khip_tricg_workspace *ws) { return ws ? ws->x : nullptr; }
double *khip_tricg_solution_y(khip_tricg_workspace *ws) { return ws ? ws->y : nullptr; }
const khip_stats *khip_tricg_stats(khip_tricg_workspace *ws) { return ws ? &ws->box.st : nullptr; }
int khip_tricg_last_path(khip_tricg_workspace *ws) { return ws ? ws->box.path : -1; }
double *khip_tricg_vector(khip_tricg_workspace *ws, const char *name) { return ws_vector(ws, kVectors, name); }
size_t khip_tricg_workspace_bytes(khip_tricg_workspace *ws) { return ws_bytes(ws, kVectors); }

int khip_tricg_solve(khip_tricg_workspace *ws, const khip_operator *A, const khip_operator *At, const double *b, const double *c,
                     const khip_options *opts_in, const khip_tricg_params *params_in) {
  KHIP_REQUIRE(ws && A && b, "tricg_solve: null argument");
  khip_tricg_params prm = params_in ? *params_in : khip_tricg_default_params();
  Ssy<Tricg> L(ws, A, At, opts_in);
  khip_ctx *ctx = L.ctx;
  const khip_options &o = L.o;
  const int64_t m = L.m, n = L.n;
  TricgDevState &s = L.s;
  const double atol = tol_or_default(o.atol), rtol = tol_or_default(o.rtol);

  if (int rc = L.check("tricg", c)) return rc;                                                            // :155-158
  if (o.verbose > 0)                                                                                      // :159
    klogf(o.log_fd, "TriCG: system of %lld equations in %lld variables\n", (long long)(m + n), (long long)(m + n));
  if (prm.spd && prm.flip) return ws->box.fail(KHIP_ERR_INVALID, "The matrix cannot be SPD and SQD");     // :162-164
  if (prm.snd && prm.flip) return ws->box.fail(KHIP_ERR_INVALID, "The matrix cannot be SND and SQD");
  if (prm.spd && prm.snd) return ws->box.fail(KHIP_ERR_INVALID, "The matrix cannot be SPD and SND");
  if (prm.flip) { prm.tau = -1.0; prm.nu = 1.0; }                                                         // :176-178
  if (prm.spd) { prm.tau = 1.0; prm.nu = 1.0; }
  if (prm.snd) { prm.tau = -1.0; prm.nu = -1.0; }
  const double tau = prm.tau, nu = prm.nu;
  const bool warm_start = ws->warm_start;
  ws->box.reset();                                                                                        // reset!(stats)
  double *x = L.pol.x = ws->x, *y = L.pol.y = ws->y;
  L.pol.gx_prev = ws->gx_prev;
  L.pol.gx = ws->gx;
  L.pol.gy_prev = ws->gy_prev;
  L.pol.gy = ws->gy;

  // set-up, the same primitives on every path (:205-280)
  K(khip_fill(ctx, m, x, 0.0));
  K(khip_fill(ctx, n, y, 0.0));
  L.itmax = o.itmax == 0 ? global_rows(ctx, A, m) + global_rows(ctx, At, n) : o.itmax;                    // m + n of the global system (:209)
  K(khip_fill(ctx, m, L.r.v_prev, 0.0));
  K(khip_fill(ctx, n, L.r.u_prev, 0.0));
  const double *b0 = b, *c0 = c;
  if (warm_start) {                                                                                       // :217-224
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
  K(khip_copy(ctx, m, L.r.v, b0));                                                                        // :227-237
  K(khip_nrm2(ctx, m, L.r.v, &beta1));
  if (beta1 != 0) K(khip_div(ctx, m, L.r.v, beta1));
  else K(khip_fill(ctx, m, L.r.v, 0.0));
  K(khip_copy(ctx, n, L.r.u, c0));                                                                        // :240-250
  K(khip_nrm2(ctx, n, L.r.u, &gamma1));
  if (gamma1 != 0) K(khip_div(ctx, n, L.r.u, gamma1));
  else K(khip_fill(ctx, n, L.r.u, 0.0));
  K(khip_fill(ctx, m, L.pol.gx_prev, 0.0));                                                               // :253-256
  K(khip_fill(ctx, n, L.pol.gy_prev, 0.0));
  K(khip_fill(ctx, m, L.pol.gx, 0.0));
  K(khip_fill(ctx, n, L.pol.gy, 0.0));
  const double rNorm = std::sqrt(gamma1 * gamma1 + beta1 * beta1);                                        // :259-261
  if (L.history) ws->box.push(rNorm);
  s.beta = beta1;
  s.gamma = gamma1;
  s.beta_next = beta1;
  s.gamma_next = gamma1;
  s.tau = tau;
  s.nu = nu;
  s.eps_tol = atol + rtol * rNorm;
  s.btol = 0x1p-39;                                                                                       // eps(Float64)^(3/4) (:272)
  s.rNorm = rNorm;
  s.stop_seq = kSeqNever;
  s.solved = (rNorm <= s.eps_tol) ? 1 : 0;                                                                // :276
  ws->box.path = (o.fused && L.square()) ? 1 : 0;
  if (o.verbose > 0) {                                                                                    // :263-264 (labels padded by hand)
    klogf(o.log_fd, "%5s  %s  %s  %s  %5s\n", "k", "   \xe2\x80\x96r\xe2\x82\x96\xe2\x80\x96", "   \xce\xb2\xe2\x82\x96\xe2\x82\x8a\xe2\x82\x81",
          "   \xce\xb3\xe2\x82\x96\xe2\x82\x8a\xe2\x82\x81", "timer");
    if (kdisplay(0, o.verbose)) klogf(o.log_fd, "%5d  %7.1e  %7.1e  %7.1e  %.2fs\n", 0, rNorm, beta1, gamma1, now_s() - L.t0);
  }

  K(L.iterate());                                                                                         // :282-462

  const char *status = "unknown";                                                                         // :466-470
  if (L.tired) status = "maximum number of iterations exceeded";
  if (s.breakdown) status = "inconsistent linear system";
  if (s.solved) status = "solution good enough given atol and rtol";
  if (L.user_exit) status = "user-requested exit";
  if (L.overtimed) status = "time limit exceeded";
  if (warm_start) {                                                                                       // :473-474: Δx has m entries, Δy has n
    K(khip_axpy(ctx, m, 1.0, ws->dx, ws->x));
    K(khip_axpy(ctx, n, 1.0, ws->dy, ws->y));
  }
  return L.end(s.solved ? 1 : 0, (!s.solved && s.breakdown) ? 1 : 0, status, false);                      // :475-482
}

}  // extern "C"
