// minres_qlp.cpp -- minres_qlp! (src/minres_qlp.jl:131-538) above the device primitives, with its fused gfx950 kernels.
//
// Real Float64, linesearch = false.  Three loops, chosen as for symmlq! (khip_minres_qlp_last_path):
//   0  options.fused = 0: the reference's primitive sequence, one launch per k* call, one host sync per kdotr / knorm;
//   1  the host-driven loop on the fused kernels (with M, a user operator, a callback or verbose > 0);
//   2  the device-resident loop (default; A a CSR handle, M = I): the Lanczos scalars, the QR and LQ recurrences and the stopping
//      tests run as the epilogues of the three reductions of an iteration (minres_qlp_step_a/b, solver_device.hpp), iterations are
//      enqueued ahead.
// With M = I the reference aliases vₖ = M⁻¹vₖ and vₖ₊₁ = p.  Iteration k on the fused paths:
//   P1   k ≥ 2: vₖ = (1/βₖ) vₖ (:265 of the iteration before) ; k ≥ 3: x = fma(spₖτₖ₋₂, vₖ, fma(cpₖτₖ₋₂, ẘₖ₋₂, x)) ;
//        wₐᵤₓ = fma(-cpₖ, vₖ, spₖ ẘₖ₋₂) ; x.x                                                   (:427-430, :468)      48n bytes
//   p = fma(-βₖ, M⁻¹vₖ₋₁, fma(λ, vₖ, A vₖ)) ; vₖ.p       the sliced SpMV with its Lanczos epilogue, coefficients (λ, 1, -βₖ)
//                                                        (+ 8n for M⁻¹vₖ₋₁); other products: p = A vₖ, then
//                                                        minres_qlp_lz_kernel (32n)              (:246-255)            -> αₖ
//   P2   p = fma(-αₖ, vₖ, p) ; p.p ; k = 1: wₖ = vₖ ; k = 2: the two outputs of :414-419 ; k ≥ 3: kref!(w̄ₖ₋₁, wₐᵤₓ, cdₖ, sdₖ)
//                                                                                               (:257-261, :408-435)  56n bytes
// against 232n for the primitive sequence (12 BLAS-1 calls with k ≥ 3 and λ = 0); the two kcopy! of :439-440 become a rotation of
// the three Lanczos buffers' roles, the two @kswap! a swap of the roles of wₖ₋₁ and wₖ, and kdiv!(vₖ₊₁, βₖ₊₁) is carried into the
// next P1: after the loop one kscal! brings M⁻¹vₖ to the reference's state.  cpₖ, spₖ, μₖ₋₂ and τₖ₋₂ need βₖ and earlier scalars
// only, so they are formed at the end of iteration k - 1 (minres_qlp_ahead).  αₖ is the dot taken AFTER βₖ M⁻¹vₖ₋₁ has been
// subtracted (:252-255): this is not symmlq!'s vᴴAv.  minres_qlp_lz_kernel is a sibling of minres_p1_kernel, which stays as it is.
// Every elementwise value uses the expression of the primitive it replaces (fma(a, x, y) for kaxpy!, fma(a, x, b y) for kaxpby!,
// khip_ref's c x + s y and s x - c y for kref!, multiplication by one(T) / β for kdiv!): the fused loops agree with the primitive
// sequence bit for bit on elementwise values and to the reductions' one ulp otherwise; loops 1 and 2 run the same kernels and
// the same scalar code and produce the same bits.
#include "solver_host.hpp"
#include "vec_launch.hpp"

using namespace khip;

namespace khip {   // (named, not anonymous: stable kernel names in traces)

// ---------------------------------------------------------------------------------------------------------- kernels ----
// Each thread owns one VEC-vector of every stream; the odd tail element (VEC = 2, n odd) goes to thread 0 of block 0.
// Cache hints, the rule of qmr.cpp: a load is non-temporal when it is the LAST read of that data before it is overwritten; a store
// is non-temporal when nothing reads it before the next iteration's passes.

// P1: scale ? v = (1/β) v ; upd ? x = fma(spτ, v, fma(cpτ, ẘ, x)) ; ẘ = fma(-cp, v, sp ẘ) ; acc = x . x   (:265 before, :427-430, :468)
//   v    load  cacheable: the product that follows and P2 read it.      store (scale) cacheable: the product reads it next.
//   x    load  NT: overwritten here.            store NT: next read by the next iteration's P1.
//   ẘ    load  NT: overwritten here.            store cacheable: P2 of this iteration reads it (as wₐᵤₓ).
template <int VEC, bool NT, bool COMP>
__global__ __launch_bounds__(kBlock) void minres_qlp_p1_kernel(int64_t n, const MinresQlpDevState *st, double *v, double *x,
                                                              double *wkm1, int scale, int upd, RedArgs ra) {
  using T = typename VecT<VEC>::type;
  if (seq_skip(ra.stop_seq, ra.seq)) return;
  const double ib = st->inv_beta, cpt = st->cpt, spt = st->spt, ncp = st->neg_cp, sp = st->sp;
  dd acc[1] = {dd{0.0, 0.0}};
  const int64_t nvec = n / VEC;
  const int64_t i = lane_index();
  if (i < nvec) {
    const T vv = ldg<false>(reinterpret_cast<const T *>(v) + i);
    T xv = {}, wv = {};
    if (upd) {
      xv = ldg<NT>(reinterpret_cast<const T *>(x) + i);
      wv = ldg<NT>(reinterpret_cast<const T *>(wkm1) + i);
    }
    T vo, xo, wo;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const double vn = scale ? ib * vget(vv, e) : vget(vv, e);     // kdiv!(vₖ₊₁, βₖ₊₁) = kscal!(one(T) / β)
      const double we = vget(wv, e);
      const double xn = fma(spt, vn, fma(cpt, we, vget(xv, e)));    // kaxpy!(cp τ, ẘ, x) ; kaxpy!(sp τ, v, x)
      vset(vo, e, vn);
      vset(xo, e, xn);
      vset(wo, e, fma(ncp, vn, sp * we));                           // kaxpby!(-cp, v, sp, ẘ)
      if (upd) acc_prod<COMP>(acc[0], xn, xn);
    }
    if (scale) stg<false>(vo, reinterpret_cast<T *>(v) + i);
    if (upd) {
      stg<NT>(xo, reinterpret_cast<T *>(x) + i);
      stg<false>(wo, reinterpret_cast<T *>(wkm1) + i);
    }
  }
  if (VEC == 2 && owns_tail(n)) {
    const int64_t t = n - 1;
    const double vn = scale ? ib * v[t] : v[t];
    if (scale) v[t] = vn;
    if (upd) {
      const double we = wkm1[t];
      const double xn = fma(spt, vn, fma(cpt, we, x[t]));
      x[t] = xn;
      wkm1[t] = fma(ncp, vn, sp * we);
      acc_prod<COMP>(acc[0], xn, xn);
    }
  }
  wave_publish<1>(acc, ra);
}

// The Lanczos step after a product that does not carry it: p = fma(-β, r1, fma(λ, v, p)) ; acc = v . p      (:247-255)
// lanczos_row's expression (spmv_common.hpp) with the coefficients (λ, 1, -β): the multiplication by 1 is exact and left out.
//   p    load  NT: overwritten here.            store cacheable: P2 reads it.
//   v    load  cacheable: P2 reads it.
//   r1   load  NT: its last read; the next iteration's product overwrites it (as p).
template <int VEC, bool NT, bool COMP>
__global__ __launch_bounds__(kBlock) void minres_qlp_lz_kernel(int64_t n, const MinresQlpDevState *st, const double *v,
                                                              const double *r1, double *p, int sub_r1, RedArgs ra) {
  using T = typename VecT<VEC>::type;
  if (seq_skip(ra.stop_seq, ra.seq)) return;
  const double lam = st->lambda, nb = st->neg_beta;
  const bool use_lam = lam != 0.0;
  dd acc[1] = {dd{0.0, 0.0}};
  const int64_t nvec = n / VEC;
  const int64_t i = lane_index();
  auto one = [&](double pe, double ve, double re) {
    double t = pe;
    if (use_lam) t = fma(lam, ve, t);                               // kaxpy!(λ, vₖ, p)
    if (sub_r1) t = fma(nb, re, t);                                 // kaxpy!(-βₖ, M⁻¹vₖ₋₁, p)
    acc_prod<COMP>(acc[0], ve, t);
    return t;
  };
  if (i < nvec) {
    const T pv = ldg<NT>(reinterpret_cast<const T *>(p) + i);
    const T vv = ldg<false>(reinterpret_cast<const T *>(v) + i);
    T rv = {};
    if (sub_r1) rv = ldg<NT>(reinterpret_cast<const T *>(r1) + i);
    T po;
#pragma unroll
    for (int e = 0; e < VEC; ++e) vset(po, e, one(vget(pv, e), vget(vv, e), vget(rv, e)));
    stg<false>(po, reinterpret_cast<T *>(p) + i);
  }
  if (VEC == 2 && owns_tail(n)) {
    const int64_t t = n - 1;
    p[t] = one(p[t], v[t], sub_r1 ? r1[t] : 0.0);
  }
  wave_publish<1>(acc, ra);
}

// P2: p = fma(-α, mv, p) ; dot ? acc = p . p ; the directions by `form` (the iteration number, 3 for k ≥ 3)   (:257-261, :408-435)
//   form 1: wk = v                                                                 (kcopy!, :410)
//   form 2: a = wk ; wkm1 = fma(-cp, v, sp a) ; wk = fma(sp, v, cp a)                (:414-419; the caller swaps the roles after)
//   form 3: a = wk, u = wkm1 ; wk = cd a + sd u ; wkm1 = sd a - cd u                 (kref!, :433; the caller swaps the roles after)
// mv = M⁻¹vₖ and v = vₖ are the same vector when M = I.
//   p    load  NT: overwritten here.            store cacheable: the next iteration's P1 reads it next (as vₖ).
//   mv   load  cacheable: the next iteration's product reads it again (as M⁻¹vₖ₋₁).
//   wk, wkm1   load NT: overwritten here.       store NT: next read by the next iteration's passes.
template <int VEC, bool NT, bool COMP>
__global__ __launch_bounds__(kBlock) void minres_qlp_p2_kernel(int64_t n, const MinresQlpDevState *st, const double *mv,
                                                              const double *v, double *p, double *wk, double *wkm1, int form,
                                                              int dot, RedArgs ra) {
  using T = typename VecT<VEC>::type;
  if (seq_skip(ra.stop_seq, ra.seq)) return;
  const double na = st->neg_alpha, cp = st->cp, sp = st->sp, ncp = st->neg_cp, cd = st->cd, sd = st->sd;
  const bool same = (mv == v);
  dd acc[1] = {dd{0.0, 0.0}};
  const int64_t nvec = n / VEC;
  const int64_t i = lane_index();
  auto one = [&](double pe, double me, double ve, double a, double u, double &wko, double &wk1o) {
    const double pn = fma(na, me, pe);                              // kaxpy!(-αₖ, M⁻¹vₖ, p)
    if (form == 1) {
      wko = ve;
      wk1o = 0.0;
    } else if (form == 2) {
      wk1o = fma(ncp, ve, sp * a);                                  // kaxpby!(-cp, vₖ, sp, wₖ) on the copy of w̅ₖ₋₁
      wko = fma(sp, ve, cp * a);                                    // kaxpby!(sp, vₖ, cp, wₖ₋₁)
    } else {
      wko = cd * a + sd * u;                                        // kref!(w̄ₖ₋₁, wₐᵤₓ, cd, sd)
      wk1o = sd * a - cd * u;
    }
    if (dot) acc_prod<COMP>(acc[0], pn, pn);
    return pn;
  };
  if (i < nvec) {
    const T pv = ldg<NT>(reinterpret_cast<const T *>(p) + i);
    const T mvv = ldg<false>(reinterpret_cast<const T *>(mv) + i);
    const T vv = same ? mvv : ldg<false>(reinterpret_cast<const T *>(v) + i);
    T av = {}, uv = {};
    if (form >= 2) av = ldg<NT>(reinterpret_cast<const T *>(wk) + i);
    if (form >= 3) uv = ldg<NT>(reinterpret_cast<const T *>(wkm1) + i);
    T po, wko, wk1o;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      double w0, w1;
      vset(po, e, one(vget(pv, e), vget(mvv, e), vget(vv, e), vget(av, e), vget(uv, e), w0, w1));
      vset(wko, e, w0);
      vset(wk1o, e, w1);
    }
    stg<false>(po, reinterpret_cast<T *>(p) + i);
    stg<NT>(wko, reinterpret_cast<T *>(wk) + i);
    if (form >= 2) stg<NT>(wk1o, reinterpret_cast<T *>(wkm1) + i);
  }
  if (VEC == 2 && owns_tail(n)) {
    const int64_t t = n - 1;
    double w0, w1;
    p[t] = one(p[t], mv[t], v[t], form >= 2 ? wk[t] : 0.0, form >= 3 ? wkm1[t] : 0.0, w0, w1);
    wk[t] = w0;
    if (form >= 2) wkm1[t] = w1;
  }
  wave_publish<1>(acc, ra);
}

}  // namespace khip

namespace {

constexpr ScalarPathNT kScalarNT = ScalarPathNT::never;

int launch_p1(khip_ctx *ctx, int64_t n, const MinresQlpDevState *st, double *v, double *x, double *wkm1, bool scale, bool upd,
              int slot) {
  VecPlan L;
  KHIP_TRY(vec_plan(ctx, n, {v, upd ? x : nullptr, upd ? wkm1 : nullptr}, &L, 1));
  RedArgs ra = make_red_args(ctx, slot);
  vec_dispatch<kScalarNT>(L, [&](auto V, auto N, auto C) {
    hipLaunchKernelGGL((minres_qlp_p1_kernel<V, N, C>), L.grid(), dim3(kBlock), 0, ctx->stream, n, st, v, x, wkm1, scale ? 1 : 0,
                       upd ? 1 : 0, ra); });
  KHIP_CHECK_HIP(hipGetLastError());
  if (!upd) return KHIP_OK;        // no reduction before iteration 3: xNorm = 0
  return launch_finish(ctx, L.waves(), 1, slot);
}

int launch_lz(khip_ctx *ctx, int64_t n, const MinresQlpDevState *st, const double *v, const double *r1, double *p, bool sub_r1,
              int slot) {
  VecPlan L;
  KHIP_TRY(vec_plan(ctx, n, {v, sub_r1 ? r1 : nullptr, p}, &L, 1));
  RedArgs ra = make_red_args(ctx, slot);
  vec_dispatch<kScalarNT>(L, [&](auto V, auto N, auto C) {
    hipLaunchKernelGGL((minres_qlp_lz_kernel<V, N, C>), L.grid(), dim3(kBlock), 0, ctx->stream, n, st, v, r1, p, sub_r1 ? 1 : 0, ra); });
  KHIP_CHECK_HIP(hipGetLastError());
  return launch_finish(ctx, L.waves(), 1, slot);
}

int launch_p2(khip_ctx *ctx, int64_t n, const MinresQlpDevState *st, const double *mv, const double *v, double *p, double *wk,
              double *wkm1, int64_t k, bool dot, int slot) {
  VecPlan L;
  KHIP_TRY(vec_plan(ctx, n, {mv, v, p, wk, wkm1}, &L, 1));
  RedArgs ra = make_red_args(ctx, slot);
  const int form = (int)std::min<int64_t>(k, 3);
  vec_dispatch<kScalarNT>(L, [&](auto V, auto N, auto C) {
    hipLaunchKernelGGL((minres_qlp_p2_kernel<V, N, C>), L.grid(), dim3(kBlock), 0, ctx->stream, n, st, mv, v, p, wk, wkm1, form,
                       dot ? 1 : 0, ra); });
  KHIP_CHECK_HIP(hipGetLastError());
  if (!dot) return KHIP_OK;        // the partials are not folded: nothing reads them
  return launch_finish(ctx, L.waves(), 1, slot);
}

// p = A v followed by the Lanczos step, reduction v.p into results[slot].  fuse (SpmvPlan::carries_lanczos): ONE launch -- the
// sliced SpMV applies the epilogue with (λ, 1, -βₖ) to each row's product and forms v.p in its fused dot; otherwise the plain
// product, then minres_qlp_lz_kernel.  Same elementwise expressions either way.
int lanczos_product(khip_ctx *ctx, const khip_operator *A, bool fuse, int64_t n, const MinresQlpDevState *st, const double *v,
                    const double *r1, double *p, bool sub_r1, int slot) {
  if (fuse) {
    ctx->lz = LanczosEpi{&st->lambda, r1, sub_r1 ? 1 : 0};
    const int rc = spmv_any(ctx, A->csr, v, p, slot);
    ctx->lz = LanczosEpi{};
    return rc;
  }
  KHIP_TRY(apply_op_no_epilogue(ctx, A, v, p));
  return launch_lz(ctx, n, st, v, r1, p, sub_r1, slot);
}

}  // namespace

struct khip_minres_qlp_workspace {
  khip_ctx *ctx;
  int64_t m, n;
  double *x = nullptr, *wkm1 = nullptr, *wk = nullptr, *Mvkm1 = nullptr, *Mvk = nullptr, *p = nullptr, *dx = nullptr, *vk = nullptr;
  Borrowed borrowed;                        // the caller's vectors (khip_minres_qlp_workspace_adopt*): never freed here
  bool warm_start = false;
  StatsBox box;
  std::vector<double> aresiduals, aconds;   // the Aresiduals / Acond histories next to box.residuals
  bool fused_product = false;               // the last solve's Lanczos step ran inside the sliced SpMV
  DeviceLoop<MinresQlpDevState, 3> loop;    // fused loops: device copy of the scalar state, pinned snapshots + staging, histories
};

namespace {

// x, wₖ₋₁, wₖ, M⁻¹vₖ₋₁, M⁻¹vₖ, p come with the workspace; Δx and vₖ stay empty until needed (src/krylov_workspaces.jl:713-768)
using W = khip_minres_qlp_workspace;
constexpr WsVec<W> kVectors[] = {{"x", &W::x, Core},         {"wkm1", &W::wkm1, Core}, {"wk", &W::wk, Core}, {"Mvkm1", &W::Mvkm1, Core},
                                 {"Mvk", &W::Mvk, Core},     {"p", &W::p, Core},       {"dx", &W::dx, Lazy}, {"vk", &W::vk, Lazy}};

// the buffers by their CURRENT role: the fused loops rotate the Lanczos three where the reference copies (:439-440) and swap the
// two directions where it swaps (:414, :434)
struct Roles {
  double *Mvkm1, *Mvk, *p, *wkm1, *wk;
  void rotate() { double *old = Mvkm1; Mvkm1 = Mvk; Mvk = p; p = old; }
  void swap_w() { std::swap(wkm1, wk); }
};

void verbose_row(const khip_options &o, long long iter, const MinresQlpDevState &s, double t0, bool first_row) {
  if (first_row)                                                                                          // :209
    klogf(o.log_fd, "%5lld  %7.1e  %7s  %7.1e  %7s  %8s  %7.1e  %7.1e  %8s  %.2fs\n", iter, s.rNorm, "✗ ✗ ✗ ✗", s.beta, "✗ ✗ ✗ ✗",
          " ✗ ✗ ✗ ✗", s.ANorm, s.Acond, " ✗ ✗ ✗ ✗", now_s() - t0);
  else                                                                                                    // :505
    klogf(o.log_fd, "%5lld  %7.1e  %7.1e  %7.1e  %7.1e  %8.1e  %7.1e  %7.1e  %8.1e  %.2fs\n", iter, s.rNorm, s.ArNorm, s.beta, s.lam,
          s.mubar, s.ANorm, s.Acond, s.backward, now_s() - t0);
}

}  // namespace

extern "C" {

khip_minres_qlp_params khip_minres_qlp_default_params(void) {
  khip_minres_qlp_params p;
  memset(&p, 0, sizeof(p));
  p.lambda = 0.0;
  p.Artol = NAN;
  return p;
}

int khip_minres_qlp_workspace_create(khip_ctx *ctx, int64_t m, int64_t n, khip_minres_qlp_workspace **out) {
  KHIP_REQUIRE(ctx && out && m >= 0 && n >= 0, "minres_qlp_workspace_create: bad argument");
  khip_minres_qlp_workspace *ws = new khip_minres_qlp_workspace();
  ws->ctx = ctx; ws->m = m; ws->n = n;
  const int rc = ws_create_core(ws, kVectors);
  if (rc) { khip_minres_qlp_workspace_destroy(ws); return rc; }
  *out = ws;
  return KHIP_OK;
}

int khip_minres_qlp_workspace_adopt(khip_ctx *ctx, int64_t m, int64_t n, double *x, double *wkm1, double *wk, double *Mvkm1,
                                    double *Mvk, double *p, khip_minres_qlp_workspace **out) {
  KHIP_REQUIRE(ctx && out && m >= 0 && n >= 0, "minres_qlp_workspace_adopt: bad argument");
  khip_minres_qlp_workspace *ws = new khip_minres_qlp_workspace();
  ws->ctx = ctx; ws->m = m; ws->n = n;
  const int rc = ws_adopt_core(ws, kVectors, "minres_qlp_workspace_adopt", {x, wkm1, wk, Mvkm1, Mvk, p});
  if (rc) { delete ws; return rc; }
  *out = ws;
  return KHIP_OK;
}

int khip_minres_qlp_workspace_adopt_vector(khip_minres_qlp_workspace *ws, const char *name, double *ptr) {
  return ws_adopt_vector(ws, kVectors, "minres_qlp_workspace_adopt_vector", name, ptr);
}

int khip_minres_qlp_workspace_destroy(khip_minres_qlp_workspace *ws) {
  if (!ws) return KHIP_OK;
  ws_free_vectors(ws, kVectors);
  ws->loop.release();
  delete ws;
  return KHIP_OK;
}

int khip_minres_qlp_warm_start(khip_minres_qlp_workspace *ws, const double *x0) { return ws_warm_start(ws, kVectors, x0, "minres_qlp_warm_start"); }
double *khip_minres_qlp_solution(khip_minres_qlp_workspace *ws) { return ws ? ws->x : nullptr; }
const khip_stats *khip_minres_qlp_stats(khip_minres_qlp_workspace *ws) { return ws ? &ws->box.st : nullptr; }
int khip_minres_qlp_last_path(khip_minres_qlp_workspace *ws) { return ws ? ws->box.path : -1; }
int khip_minres_qlp_fused_product(khip_minres_qlp_workspace *ws) { return ws ? (ws->fused_product ? 1 : 0) : -1; }
double *khip_minres_qlp_vector(khip_minres_qlp_workspace *ws, const char *name) { return ws_vector(ws, kVectors, name); }
size_t khip_minres_qlp_workspace_bytes(khip_minres_qlp_workspace *ws) { return ws_bytes(ws, kVectors); }

int khip_minres_qlp_histories(khip_minres_qlp_workspace *ws, const double **aresiduals, int *naresiduals, const double **acond,
                              int *nacond) {
  KHIP_REQUIRE(ws && aresiduals && naresiduals && acond && nacond, "minres_qlp_histories: null argument");
  *aresiduals = ws->aresiduals.empty() ? nullptr : ws->aresiduals.data();
  *naresiduals = (int)ws->aresiduals.size();
  *acond = ws->aconds.empty() ? nullptr : ws->aconds.data();
  *nacond = (int)ws->aconds.size();
  return KHIP_OK;
}

int khip_minres_qlp_solve(khip_minres_qlp_workspace *ws, const khip_operator *A, const khip_operator *M, const double *b,
                          const khip_options *opts_in, const khip_minres_qlp_params *params_in) {
  KHIP_REQUIRE(ws && A && b, "minres_qlp_solve: null argument");
  khip_ctx *ctx = ws->ctx;
  const khip_options o = opts_in ? *opts_in : khip_default_options();
  const khip_minres_qlp_params prm = params_in ? *params_in : khip_minres_qlp_default_params();
  const double t0 = now_s();
  const double timemax = timemax_of(o);
  const int64_t n = ws->n;
  const double atol = tol_or_default(o.atol), rtol = tol_or_default(o.rtol), Artol = tol_or_default(prm.Artol);
  const double lambda = prm.lambda;
  const bool history = o.history != 0;
  (void)take_alloc_seconds();

  if (int rc = check_shape(ws, {A})) return rc;                                                            // :137-138
  if (ws->m != ws->n) return ws->box.fail(KHIP_ERR_INVALID, "System must be square");                     // :139
  if (o.variant != 0) return ws->box.fail(KHIP_ERR_INVALID, "minres_qlp: options.variant must be 0 (there is no other recurrence)");
  if (o.verbose > 0) klogf(o.log_fd, "MINRES-QLP: system of size %lld\n", (long long)n);                  // :141
  if (o.linesearch)
    return ws->box.fail(KHIP_ERR_UNSUPPORTED, "minres_qlp: linesearch = true (nonpositive-curvature detection) is not supported");

  const bool MisI = (M == nullptr);
  if (!MisI && !ws->vk) K(alloc_vec(ctx, n, &ws->vk));                                                     // :152
  const bool warm_start = ws->warm_start;
  ws->box.reset(); ws->aresiduals.clear(); ws->aconds.clear();                                           // reset!(stats)
  ws->fused_product = false;
  Roles B{ws->Mvkm1, ws->Mvk, ws->p, ws->wkm1, ws->wk};
  double *x = ws->x;
  double *vM = ws->vk;                                                    // vₖ with M (:162); with M = I it is M⁻¹vₖ
  ws->box.path = o.fused ? 1 : 0;

  // set-up, the same primitives on every path (:166-236)
  K(khip_fill(ctx, n, x, 0.0));
  K(residual0(ws, A, lambda, b, warm_start, B.Mvk));
  double *v = MisI ? B.Mvk : vM;
  if (!MisI) K(apply_op(ctx, M, B.Mvk, v));                                                                // :177
  double beta1;
  if (MisI) {                                                                                              // :178 (knorm_elliptic)
    K(khip_nrm2(ctx, n, v, &beta1));
  } else {
    K(khip_dot(ctx, n, v, B.Mvk, &beta1));
    if (beta1 < 0) return ws->box.fail(KHIP_ERR_NUMERIC, "Preconditioner is not positive definite");
    beta1 = std::sqrt(beta1);
  }
  if (beta1 != 0) {                                                                                        // :180-183
    K(khip_div(ctx, n, B.Mvk, beta1));
    if (!MisI) K(khip_div(ctx, n, v, beta1));
  }
  MinresQlpDevState s;
  memset(&s, 0, sizeof(s));
  s.lambda = lambda; s.one = 1.0;
  s.beta = beta1; s.rNorm = beta1;                                                                         // :185-192
  s.atol = atol; s.Artol = Artol; s.MisI = MisI ? 1 : 0;
  if (history) { ws->box.push(s.rNorm); ws->aconds.push_back(0.0); }
  if (s.rNorm == 0) return ws_end(ws, {0, 1, 0, "x is a zero-residual solution", warm_start, t0, true});   // :193-201

  int64_t iter = 0;
  const int64_t itmax = o.itmax == 0 ? 2 * global_rows(ctx, A, n) : o.itmax;      // 2n of the GLOBAL system on every rank (:204)
  s.eps_tol = atol + rtol * s.rNorm;                                                                       // :206
  if (o.verbose > 0)                                                                                       // :208-209
    klogf(o.log_fd, "%5s  %s  %s  %s  %s  %s  %s  %s  %8s  %5s\n", "k", "   ‖rₖ‖", "‖Arₖ₋₁‖", "   βₖ₊₁", "   Rₖ.ₖ", "    Lₖ.ₖ", "    ‖A‖",
          "   κ(A)", "backward", "timer");                          // %7s / %8s of the UTF-8 labels, padded by hand
  if (kdisplay(iter, o.verbose)) verbose_row(o, iter, s, t0, true);

  K(khip_fill(ctx, n, B.Mvkm1, 0.0));                                                                      // :212-221
  s.zbar = s.beta;
  K(khip_fill(ctx, n, B.wkm1, 0.0));
  K(khip_fill(ctx, n, B.wk, 0.0));
  s.c2 = s.c1 = s.c = 1.0;
  s.btol = std::pow(kEps, 0.75);                                                                           // :224
  s.stop_seq = kSeqNever;
  s.solved = s.zero_resid = (s.rNorm <= s.eps_tol) ? 1 : 0;                                               // :227-236
  bool tired = iter >= itmax, user_exit = false, overtimed = false;
  auto running = [&] {
    return !(s.solved || tired || s.inconsistent || s.ill_cond_mach || s.breakdown || user_exit || overtimed);
  };

  // the end of an iteration on the host-driven loops (:261-269, :333-505); false when β² < 0
  auto host_tail = [&](int64_t k, double b2, double xNorm) -> bool {
    (void)minres_qlp_step_b(s, b2, xNorm, k);
    if (s.not_pd) return false;
    if (history) { ws->box.push(s.rNorm); ws->aresiduals.push_back(s.ArNorm); ws->aconds.push_back(s.Acond); }
    tired = k >= itmax;
    return true;
  };
  // :484-490, :505 (after the vectors of the iteration are in place)
  auto iteration_end = [&](int64_t k) {
    if (o.callback) { ws->Mvkm1 = B.Mvkm1; ws->Mvk = B.Mvk; ws->p = B.p; ws->wkm1 = B.wkm1; ws->wk = B.wk; }   // the names follow the roles
    host_exit(ws, o, t0, timemax, &user_exit, &overtimed);
    if (kdisplay(k, o.verbose)) verbose_row(o, k, s, t0, false);
  };
  const char *not_pd_msg = "Preconditioner is not positive definite";

  const bool fastA = A->csr && !A->apply;
  const bool device_loop = o.fused >= 2 && fastA && MisI && !o.callback && o.verbose <= 0;
  ws->box.path = (device_loop && running()) ? 2 : (o.fused ? 1 : 0);   // a loop that never starts reports 1, as the early returns do
  // the Lanczos step inside the product: fused loops with M = I on a CSR handle whose product runs the sliced kernel (both fused
  // loops decide alike, so they keep producing the same bits)
  const bool fuse = ws->box.path >= 1 && fastA && MisI && spmv_plan(ctx, A->csr, true).carries_lanczos();
  ws->fused_product = fuse;
  double alpha, beta2, xNorm;

  if (ws->box.path == 0) {
    // -------------------------------------------------------------- the reference's primitive sequence ------------------
    double *vnext = MisI ? B.p : B.Mvkm1;                                                                 // :163
    while (running()) {
      const int64_t k = ++iter;
      K(apply_op(ctx, A, v, B.p));                                                                        // :246
      if (lambda != 0) K(khip_axpy(ctx, n, lambda, v, B.p));                                              // :248
      if (k >= 2) K(khip_axpy(ctx, n, -s.beta, B.Mvkm1, B.p));                                            // :252
      K(khip_dot(ctx, n, v, B.p, &alpha));                                                                // :255
      minres_qlp_step_a(s, alpha, k);
      K(khip_axpy(ctx, n, -alpha, B.Mvk, B.p));                                                           // :257
      if (!MisI) K(apply_op(ctx, M, B.p, vnext));                                                         // :259
      K(khip_dot(ctx, n, vnext, B.p, &beta2));                       // :261; M = I: knorm is the square root of this sum (khip_nrm2)
      // cpₖ, spₖ, τₖ₋₂, cdₖ, sdₖ of THIS iteration: step B below forms the next iteration's (minres_qlp_ahead)
      const double cp = s.cp, sp = s.sp, tau2 = s.tau2, cd = s.cd, sd = s.sd;
      const double beta_next = std::sqrt(beta2);                     // NaN when β² < 0: no division, host_tail reports it
      if (beta_next > s.btol) {                                                                           // :264-267
        K(khip_div(ctx, n, vnext, beta_next));
        if (!MisI) K(khip_div(ctx, n, B.p, beta_next));
      }
      if (k == 1) {                                                                                       // :408-435
        K(khip_copy(ctx, n, B.wk, v));
      } else if (k == 2) {
        B.swap_w();
        K(khip_copy(ctx, n, B.wk, B.wkm1));
        K(khip_axpby(ctx, n, -cp, v, sp, B.wk));
        K(khip_axpby(ctx, n, sp, v, cp, B.wkm1));
      } else {
        K(khip_axpy(ctx, n, cp * tau2, B.wkm1, x));
        K(khip_axpy(ctx, n, sp * tau2, v, x));
        K(khip_axpby(ctx, n, -cp, v, sp, B.wkm1));
        K(khip_ref(ctx, n, B.wk, B.wkm1, cd, sd));
        B.swap_w();
      }
      if (!MisI) K(khip_copy(ctx, n, v, vnext));                                                          // :438-440
      K(khip_copy(ctx, n, B.Mvkm1, B.Mvk));
      K(khip_copy(ctx, n, B.Mvk, B.p));
      K(khip_nrm2(ctx, n, x, &xNorm));                                                                    // :468
      if (!host_tail(k, beta2, xNorm)) return ws->box.fail(KHIP_ERR_NUMERIC, not_pd_msg);
      iteration_end(k);
    }
  } else if (ws->box.path == 1) {
    // -------------------------------------------------------------- host-driven loop on the fused kernels ---------------
    K(ws->loop.alloc());
    const MinresQlpDevState *dev = ws->loop.dev;
    // with a callback the kdiv! is not carried: the named vectors hold the reference's state when the callback runs
    const bool carry = MisI && !o.callback;
    while (running()) {
      const int64_t k = ++iter;
      K(ws->loop.upload(ctx, s));
      const bool scale = carry && k >= 2, upd = k >= 3;
      if (scale || upd) {
        const int slot = take_slots(ctx, 1);
        K(launch_p1(ctx, n, dev, v, x, B.wkm1, scale, upd, slot));                                        // :427-430, :468 (and :265 of k - 1)
        if (upd) {
          double xx;
          K(fetch_results(ctx, slot, 1, &xx));
          s.xNorm = std::sqrt(xx);
        }
      }
      int slot = take_slots(ctx, 1);
      K(lanczos_product(ctx, A, fuse, n, dev, v, B.Mvkm1, B.p, k >= 2, slot));                            // :246-255
      K(fetch_results(ctx, slot, 1, &alpha));
      minres_qlp_step_a(s, alpha, k);
      K(ws->loop.upload(ctx, s));
      slot = take_slots(ctx, 1);
      K(launch_p2(ctx, n, dev, B.Mvk, v, B.p, B.wk, B.wkm1, k, MisI, slot));                              // :257-261, :408-435
      if (k >= 2) B.swap_w();
      if (MisI) {
        K(fetch_results(ctx, slot, 1, &beta2));
        B.rotate();                                                                                       // :439-440
        v = B.Mvk;
        if (!host_tail(k, beta2, s.xNorm)) return ws->box.fail(KHIP_ERR_NUMERIC, not_pd_msg);
        if (!carry && s.beta > s.btol) K(khip_scal(ctx, n, 1.0 / s.beta, B.Mvk));                         // :265
      } else {
        double *vnext = B.Mvkm1;
        K(apply_op(ctx, M, B.p, vnext));                                                                  // :259
        K(khip_dot(ctx, n, vnext, B.p, &beta2));                                                          // :261
        if (!host_tail(k, beta2, s.xNorm)) return ws->box.fail(KHIP_ERR_NUMERIC, not_pd_msg);
        if (s.beta > s.btol) {                                                                            // :264-267
          K(khip_div(ctx, n, vnext, s.beta));
          K(khip_div(ctx, n, B.p, s.beta));
        }
        K(khip_copy(ctx, n, v, vnext));                                                                   // :438-440
        K(khip_copy(ctx, n, B.Mvkm1, B.Mvk));
        K(khip_copy(ctx, n, B.Mvk, B.p));
      }
      iteration_end(k);
    }
    if (carry && iter > 0 && s.beta > s.btol) K(khip_scal(ctx, n, 1.0 / s.beta, B.Mvk));                  // :265 of the last iteration
  } else {
    // -------------------------------------------------------------- device-resident loop ------------------------------
    const Roles first = B;
    auto step = [&](MinresQlpDevState *dev, long long j) {
      const int64_t k = j + 1;
      // P1 (:427-430, :468 and :265 of k - 1): from iteration 3 on it updates x and x.x -> xNorm; at k = 2 it only scales vₖ
      auto p1 = [&](int slot) { return launch_p1(ctx, n, dev, B.Mvk, x, B.wkm1, true, k >= 3, slot); };
      if (k >= 3) KHIP_TRY(dev_stage(ctx, dev, 3 * j, EPI_MINRES_QLP_X, 1, p1));
      else if (k == 2) KHIP_TRY(dev_pass(ctx, &dev->stop_seq, 3 * j, EPI_NONE, nullptr, [&] { return p1(take_slots(ctx, 1)); }));
      KHIP_TRY(dev_stage(ctx, dev, 3 * j + 1, EPI_MINRES_QLP_A, 1, [&](int slot) {
        return lanczos_product(ctx, A, fuse, n, dev, B.Mvk, B.Mvkm1, B.p, k >= 2, slot); }));             // :246-255  v.p -> αₖ
      KHIP_TRY(dev_stage(ctx, dev, 3 * j + 2, EPI_MINRES_QLP_B, 1, [&](int slot) {
        return launch_p2(ctx, n, dev, B.Mvk, B.Mvk, B.p, B.wk, B.wkm1, k, true, slot); }));               // :257-261  p.p -> βₖ₊₁, the tests
      if (k >= 2) B.swap_w();
      B.rotate();
      return (int)KHIP_OK;
    };
    K(ws->loop.run(ctx, s, device_loop_args(itmax, t0, timemax, history, {&ws->box.residuals, &ws->aresiduals, &ws->aconds}), step,
                   &s, &overtimed));
    iter = s.iter;
    tired = iter >= itmax;
    B = replay(first, iter, 3, [](Roles &r) { r.rotate(); });
    if (iter >= 2 && (iter - 1) % 2) B.swap_w();
    if (iter > 0 && s.beta > s.btol) K(khip_scal(ctx, n, 1.0 / s.beta, B.Mvk));                           // :265 of the last iteration
  }
  ws->Mvkm1 = B.Mvkm1; ws->Mvk = B.Mvk; ws->p = B.p; ws->wkm1 = B.wkm1; ws->wk = B.wk;
  if (o.verbose > 0) { klogf(o.log_fd, "\n"); klog_flush(o.log_fd); }                                      // :507

  if (iter >= 2) K(khip_axpy(ctx, n, s.tau1, B.wkm1, x));                                                  // :510-515
  if (!s.inconsistent) K(khip_axpy(ctx, n, s.tau, B.wk, x));

  const char *status = "unknown";                                                                         // :518-524
  if (tired) status = "maximum number of iterations exceeded";
  if (s.ill_cond_mach) status = "condition number seems too large for this machine";
  if (s.inconsistent) status = "found approximate minimum least-squares solution";
  if (s.zero_resid) status = "found approximate zero-residual solution";
  if (s.solved) status = "solution good enough given atol and rtol";
  if (user_exit) status = "user-requested exit";
  if (overtimed) status = "time limit exceeded";
  return ws_end(ws, {iter, s.solved ? 1 : 0, s.inconsistent ? 1 : 0, status, warm_start, t0, true});     // :527-536
}

}  // extern "C"
