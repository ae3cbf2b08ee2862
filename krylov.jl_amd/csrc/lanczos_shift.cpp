// lanczos_shift.cpp -- cg_lanczos_shift! (src/cg_lanczos_shift.jl:107-284) above the device primitives, with its gfx950 kernels.
//
// Real Float64: one Lanczos basis for the family (A + s_i I) x_i = b, i = 1 .. p.  Three loops, chosen as for minres!
// (khip_cg_lanczos_shift_last_path):
//   0  options.fused = 0: the reference's primitive sequence, one launch per k* call, one host sync per kdotr / knorm;
//   1  the host-driven loop on the kernels below (with M, a user operator, a callback, verbose > 0 or p > kShiftMax);
//   2  the device-resident loop (default): the Lanczos and per-shift scalars run as the epilogues of the two reductions of an
//      iteration (lzshift_step, solver_device.hpp), iterations are enqueued ahead.
// One iteration with M = I on the fused paths:
//   P0  y = A v ; δ = v.y                                   the fused SpMV with its dot (spmv_any, as cg! forms p.Ap)
//   P1  w = fma(-β, v_prev, fma(-δ, v, y)) ; w.w -> β        32n bytes (iteration 1: no v_prev term)
//   P2  v = (1/β) w, stored once ; for every active shift:   16n + 32n per active shift
//       x_i = fma(γ_i, p_i, x_i) ; p_i = fma(σ_i, v, ω_i p_i)
// and kcopy!(Mv_prev, Mv), kcopy!(Mv, Mv_next) become a rotation of the three buffers' roles.  Every elementwise value uses the
// expression of the primitive it replaces (fma for kaxpy!, fma(s, x, t y) for kaxpby!, kscal! by one(T)/β for kdiv!): the fused
// loops agree with the primitive sequence bit for bit on elementwise values and to the reductions' one ulp otherwise; loops 1
// and 2 run the same kernels and the same scalar code and produce the same bits.
#include <chrono>
#include <string>
#include <utility>

#include "solver_host.hpp"
#include "vec_launch.hpp"

using namespace khip;

namespace khip {   // (named, not anonymous: stable kernel names in traces)

// ---------------------------------------------------------------------------------------------------------- kernels ----
// Each thread owns one VEC-vector of every stream; the odd tail element (VEC = 2, n odd) goes to thread 0 of block 0.

// P1: w = fma(-β, prev, fma(-δ, cur, y)) in place of y ; acc = w . w          (src/cg_lanczos_shift.jl:201-208)
template <int VEC, bool NT, bool COMP>
__global__ __launch_bounds__(kBlock) void lzshift_p1_kernel(int64_t n, const LanczosShiftDevState *st, const double *prev,
                                                           const double *cur, double *y, int sub_prev, int dot, RedArgs ra) {
  using T = typename VecT<VEC>::type;
  if (seq_skip(ra.stop_seq, ra.seq)) return;
  const double nd = -st->delta, nb = -st->beta;
  dd acc[1] = {dd{0.0, 0.0}};
  const int64_t nvec = n / VEC;
  const int64_t i = lane_index();
  auto one = [&](double ye, double ce, double pe) {
    double w = fma(nd, ce, ye);
    if (sub_prev) w = fma(nb, pe, w);
    if (dot) acc_prod<COMP>(acc[0], w, w);
    return w;
  };
  if (i < nvec) {
    const T yv = ldg<NT>(reinterpret_cast<const T *>(y) + i);
    const T cv = ldg<NT>(reinterpret_cast<const T *>(cur) + i);
    T pv = {};
    if (sub_prev) pv = ldg<NT>(reinterpret_cast<const T *>(prev) + i);
    T wo;
#pragma unroll
    for (int e = 0; e < VEC; ++e) vset(wo, e, one(vget(yv, e), vget(cv, e), vget(pv, e)));
    stg<false>(wo, reinterpret_cast<T *>(y) + i);                      // w is read again by P2
  }
  if (VEC == 2 && owns_tail(n)) {
    const int64_t t = n - 1;
    y[t] = one(y[t], cur[t], sub_prev ? prev[t] : 0.0);
  }
  if (dot) wave_publish<1>(acc, ra);
}

// With M: v = (1/β) v ; Mv = (1/β) Mv ; acc = v . v                            (:209-210, :214)
template <int VEC, bool NT, bool COMP>
__global__ __launch_bounds__(kBlock) void lzshift_scale_kernel(int64_t n, const LanczosShiftDevState *st, double *v, double *Mv,
                                                              RedArgs ra) {
  using T = typename VecT<VEC>::type;
  if (seq_skip(ra.stop_seq, ra.seq)) return;
  const double ib = st->inv_beta;
  dd acc[1] = {dd{0.0, 0.0}};
  const int64_t nvec = n / VEC;
  const int64_t i = lane_index();
  if (i < nvec) {
    const T vv = ldg<NT>(reinterpret_cast<const T *>(v) + i);
    const T mv = ldg<NT>(reinterpret_cast<const T *>(Mv) + i);
    T vo, mo;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const double a = ib * vget(vv, e);
      vset(vo, e, a);
      vset(mo, e, ib * vget(mv, e));
      acc_prod<COMP>(acc[0], a, a);
    }
    stg<false>(vo, reinterpret_cast<T *>(v) + i);
    stg<false>(mo, reinterpret_cast<T *>(Mv) + i);
  }
  if (VEC == 2 && owns_tail(n)) {
    const int64_t t = n - 1;
    const double a = ib * v[t];
    v[t] = a;
    Mv[t] = ib * Mv[t];
    acc_prod<COMP>(acc[0], a, a);
  }
  wave_publish<1>(acc, ra);
}

// P2, the multi-shift update (:222-234): SCALE: v = (1/β) w stored in place of w (M = I), else v is read as it is.  Then for
// every active shift j (act[0] of them, act[1 + j] = shift, coef[3 j ..] = (γ, σ, ω)):
//   x_i = fma(γ, p_i, x_i) ; p_i = fma(σ, v, ω p_i)
// tab[2 i], tab[2 i + 1] = x_i, p_i.  The list, the coefficients and the table are uniform across the grid (scalar loads); the
// loads of shift j + 1 are issued before the stores of shift j, so two shifts' streams are in flight per thread.
template <int VEC, bool NT, bool SCALE>
__global__ __launch_bounds__(kBlock) void lzshift_p2_kernel(int64_t n, const double *__restrict__ inv_beta,
                                                           const int *__restrict__ act, const double *__restrict__ coef,
                                                           double *const *__restrict__ tab, double *w, const long long *stop_seq,
                                                           long long seq) {
  using T = typename VecT<VEC>::type;
  if (seq_skip(stop_seq, seq)) return;
  const double ib = *inv_beta;
  const int na = act[0];
  const int64_t nvec = n / VEC;
  const int64_t i = lane_index();
  if (i < nvec) {
    const T wv = ldg<NT>(reinterpret_cast<const T *>(w) + i);
    T vv;
    if (SCALE) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) vset(vv, e, ib * vget(wv, e));
      stg<NT>(vv, reinterpret_cast<T *>(w) + i);
    } else {
      vv = wv;
    }
    if (na > 0) {
      int s = act[1];
      T *xp = reinterpret_cast<T *>(tab[2 * s]), *pp = reinterpret_cast<T *>(tab[2 * s + 1]);
      T xa = ldg<NT>(xp + i), pa = ldg<NT>(pp + i);
      for (int j = 0; j < na; ++j) {
        T xb = {}, pb = {};
        T *xq = nullptr, *pq = nullptr;
        if (j + 1 < na) {                              // next shift's loads ahead of this shift's stores
          const int s2 = act[j + 2];
          xq = reinterpret_cast<T *>(tab[2 * s2]);
          pq = reinterpret_cast<T *>(tab[2 * s2 + 1]);
          xb = ldg<NT>(xq + i);
          pb = ldg<NT>(pq + i);
        }
        const double g = coef[3 * j], sg = coef[3 * j + 1], om = coef[3 * j + 2];
        T xo, po;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          vset(xo, e, fma(g, vget(pa, e), vget(xa, e)));
          vset(po, e, fma(sg, vget(vv, e), om * vget(pa, e)));
        }
        stg<NT>(xo, xp + i);
        stg<NT>(po, pp + i);
        xa = xb; pa = pb; xp = xq; pp = pq;
      }
    }
  }
  if (VEC == 2 && owns_tail(n)) {
    const int64_t t = n - 1;
    double v = w[t];
    if (SCALE) { v = ib * v; w[t] = v; }
    for (int j = 0; j < na; ++j) {
      const int s = act[1 + j];
      double *x = tab[2 * s], *p = tab[2 * s + 1];
      const double pe = p[t];
      x[t] = fma(coef[3 * j], pe, x[t]);
      p[t] = fma(coef[3 * j + 1], v, coef[3 * j + 2] * pe);
    }
  }
}

// x_i = 0 for every shift and, with copy_p, p_i = src (the initial pᵢ ← v of :187-196 in one pass)
template <int VEC, bool NT>
__global__ __launch_bounds__(kBlock) void lzshift_init_kernel(int64_t n, int p, double *const *__restrict__ tab,
                                                             const double *src, int copy_p) {
  using T = typename VecT<VEC>::type;
  const int64_t nvec = n / VEC;
  const int64_t i = lane_index();
  if (i < nvec) {
    T sv = {};
    if (copy_p) sv = ldg<NT>(reinterpret_cast<const T *>(src) + i);
    const T z = {};
    for (int s = 0; s < p; ++s) {
      stg<NT>(z, reinterpret_cast<T *>(tab[2 * s]) + i);
      if (copy_p) stg<NT>(sv, reinterpret_cast<T *>(tab[2 * s + 1]) + i);
    }
  }
  if (VEC == 2 && owns_tail(n)) {
    const int64_t t = n - 1;
    for (int s = 0; s < p; ++s) {
      tab[2 * s][t] = 0.0;
      if (copy_p) tab[2 * s + 1][t] = src[t];
    }
  }
}

}  // namespace khip

namespace {

constexpr ScalarPathNT kScalarNT = ScalarPathNT::never;

int launch_p1(khip_ctx *ctx, int64_t n, const LanczosShiftDevState *st, const double *prev, const double *cur, double *y,
              bool sub_prev, bool dot, int slot) {
  VecPlan L;
  KHIP_TRY(vec_plan(ctx, n, {sub_prev ? prev : nullptr, cur, y}, &L, dot ? 1 : 0));
  RedArgs ra = make_red_args(ctx, slot);
  vec_dispatch<kScalarNT>(L, [&](auto V, auto N, auto C) {
    hipLaunchKernelGGL((lzshift_p1_kernel<V, N, C>), L.grid(), dim3(kBlock), 0, ctx->stream, n, st, prev, cur, y, sub_prev ? 1 : 0,
                       dot ? 1 : 0, ra); });
  KHIP_CHECK_HIP(hipGetLastError());
  if (!dot) return KHIP_OK;        // nothing reads the partials
  return launch_finish(ctx, L.waves(), 1, slot);
}
int launch_scale(khip_ctx *ctx, int64_t n, const LanczosShiftDevState *st, double *v, double *Mv, int slot) {
  VecPlan L;
  KHIP_TRY(vec_plan(ctx, n, {v, Mv}, &L, 1));
  RedArgs ra = make_red_args(ctx, slot);
  vec_dispatch<kScalarNT>(L, [&](auto V, auto N, auto C) {
    hipLaunchKernelGGL((lzshift_scale_kernel<V, N, C>), L.grid(), dim3(kBlock), 0, ctx->stream, n, st, v, Mv, ra); });
  KHIP_CHECK_HIP(hipGetLastError());
  return launch_finish(ctx, L.waves(), 1, slot);
}

// tab_aligned: every x_i / p_i of the table is 16-byte aligned (checked when the table is built)
int launch_p2(khip_ctx *ctx, int64_t n, const double *inv_beta, const int *act, const double *coef, double *const *tab,
              bool tab_aligned, double *w, bool scale) {
  VecPlan L;
  KHIP_TRY(vec_plan(ctx, n, {w}, &L, 0, tab_aligned));
  const long long *stop = ctx->ctl.stop_seq;
  const long long seq = ctx->ctl.seq;
  vec_dispatch_vn<kScalarNT>(L, [&](auto V, auto N) {
    if (scale) hipLaunchKernelGGL((lzshift_p2_kernel<V, N, true>), L.grid(), dim3(kBlock), 0, ctx->stream, n, inv_beta, act, coef, tab, w, stop, seq);
    else hipLaunchKernelGGL((lzshift_p2_kernel<V, N, false>), L.grid(), dim3(kBlock), 0, ctx->stream, n, inv_beta, act, coef, tab, w, stop, seq); });
  KHIP_CHECK_HIP(hipGetLastError());
  return KHIP_OK;
}
int launch_init(khip_ctx *ctx, int64_t n, int p, double *const *tab, bool tab_aligned, const double *src, bool copy_p) {
  if (n <= 0 || p <= 0) return KHIP_OK;
  VecPlan L;
  KHIP_TRY(vec_plan(ctx, n, {copy_p ? src : nullptr}, &L, 0, tab_aligned));
  vec_dispatch_vn<kScalarNT>(L, [&](auto V, auto N) {
    hipLaunchKernelGGL((lzshift_init_kernel<V, N>), L.grid(), dim3(kBlock), 0, ctx->stream, n, p, tab, src, copy_p ? 1 : 0); });
  KHIP_CHECK_HIP(hipGetLastError());
  return KHIP_OK;
}

}  // namespace

struct khip_cg_lanczos_shift_workspace {
  khip_ctx *ctx;
  int64_t m, n;
  int nshifts;
  double *Mv = nullptr, *Mv_prev = nullptr, *Mv_next = nullptr, *v = nullptr;
  std::vector<double *> x, p;
  Borrowed borrowed;                        // the caller's vectors (khip_cg_lanczos_shift_workspace_adopt*): never freed here
  StatsBox box;
  std::vector<std::vector<double>> hist;    // stats.residuals[i]
  std::vector<double> sigma, dhat, omega, gamma, rNorms, coef;
  std::vector<int> converged, not_cv, indefinite, act;
  std::vector<long long> nhist;
  double **tab = nullptr;                   // device pointer table (x_1, p_1, x_2, p_2, ...), rebuilt at every solve
  std::vector<double *> tab_host;
  int *act_dev = nullptr;                   // host-driven loop: act and coef of the iteration, uploaded
  double *coef_dev = nullptr;
  DeviceLoop<LanczosShiftDevState, 3> loop; // fused loops: device copy of the scalar state, pinned snapshots + staging, history
};

namespace {

void init_arrays(khip_cg_lanczos_shift_workspace *ws) {
  const size_t p = (size_t)ws->nshifts;
  for (auto *a : {&ws->sigma, &ws->dhat, &ws->omega, &ws->gamma, &ws->rNorms}) a->assign(p, 0.0);
  for (auto *a : {&ws->converged, &ws->not_cv, &ws->indefinite}) a->assign(p, 0);
  ws->act.assign(p + 1, 0);
  ws->coef.assign(3 * p, 0.0);
  ws->nhist.assign(p, 0);
  ws->hist.assign(p, std::vector<double>());
}

LzShiftArrays host_arrays(khip_cg_lanczos_shift_workspace *ws, const double *shifts) {
  return LzShiftArrays{shifts, ws->sigma.data(), ws->dhat.data(), ws->omega.data(), ws->gamma.data(), ws->rNorms.data(),
                       ws->coef.data(), ws->converged.data(), ws->not_cv.data(), ws->indefinite.data(), ws->act.data(),
                       ws->nhist.data()};
}

// the host copy of the fused loops' pointer table (x_i, p_i); false when one of the vectors is not 16-byte aligned
bool fill_table(khip_cg_lanczos_shift_workspace *ws) {
  bool aligned = true;
  ws->tab_host.resize(2 * (size_t)ws->nshifts);
  for (size_t i = 0; i < (size_t)ws->nshifts; ++i) {
    ws->tab_host[2 * i] = ws->x[i];
    ws->tab_host[2 * i + 1] = ws->p[i];
    aligned = aligned && aligned16(ws->x[i]) && aligned16(ws->p[i]);
  }
  return aligned;
}

// act / coef of the host-driven loop's iteration (from pageable host memory: waited for)
int upload_coefs(khip_cg_lanczos_shift_workspace *ws) {
  const int na = ws->act[0];
  KHIP_CHECK_HIP(hipMemcpyAsync(ws->act_dev, ws->act.data(), sizeof(int) * (size_t)(1 + na), hipMemcpyHostToDevice, ws->ctx->stream));
  if (na > 0)
    KHIP_CHECK_HIP(hipMemcpyAsync(ws->coef_dev, ws->coef.data(), sizeof(double) * 3 * (size_t)na, hipMemcpyHostToDevice,
                                  ws->ctx->stream));
  KHIP_CHECK_HIP(hipStreamSynchronize(ws->ctx->stream));
  return KHIP_OK;
}

void verbose_row(const khip_options &o, long long iter, const std::vector<double> &rNorms, double t0) {
  std::string line;
  char buf[64];
  snprintf(buf, sizeof(buf), "%5lld", iter);
  line += buf;
  for (double r : rNorms) { snprintf(buf, sizeof(buf), "  %8.1e", r); line += buf; }
  snprintf(buf, sizeof(buf), "  %.2fs\n", now_s() - t0);
  line += buf;
  klogf(o.log_fd, "%s", line.c_str());
}

int distinct_vectors(const std::vector<const double *> &all, const char *fn) {
  for (size_t i = 0; i < all.size(); ++i)
    for (size_t j = i + 1; j < all.size(); ++j)
      KHIP_REQUIRE(all[i] != all[j], "%s: Mv, Mv_prev, Mv_next and every x[i], p[i] must be distinct", fn);
  return KHIP_OK;
}

}  // namespace

extern "C" {

khip_cg_lanczos_shift_params khip_cg_lanczos_shift_default_params(void) {
  khip_cg_lanczos_shift_params p;
  p.shifts = nullptr;
  p.nshifts = 0;
  p.check_curvature = 0;
  return p;
}

int khip_cg_lanczos_shift_workspace_create(khip_ctx *ctx, int64_t m, int64_t n, int nshifts, khip_cg_lanczos_shift_workspace **out) {
  KHIP_REQUIRE(ctx && out && m >= 0 && n >= 0, "cg_lanczos_shift_workspace_create: bad argument");
  KHIP_REQUIRE(nshifts >= 1, "cg_lanczos_shift_workspace_create: nshifts must be positive");
  khip_cg_lanczos_shift_workspace *ws = new khip_cg_lanczos_shift_workspace();
  ws->ctx = ctx; ws->m = m; ws->n = n; ws->nshifts = nshifts;
  init_arrays(ws);
  (void)take_alloc_seconds();
  // Mv, Mv_prev, Mv_next, x[i], p[i] allocated; v stays empty until M needs it (src/krylov_workspaces.jl:636-660)
  ws->x.assign((size_t)nshifts, nullptr);
  ws->p.assign((size_t)nshifts, nullptr);
  int rc = KHIP_OK;
  for (double **slot : {&ws->Mv, &ws->Mv_prev, &ws->Mv_next})
    if (!rc) rc = alloc_vec(ctx, n, slot);
  for (int i = 0; i < nshifts && !rc; ++i) rc = alloc_vec(ctx, n, &ws->x[(size_t)i]);
  for (int i = 0; i < nshifts && !rc; ++i) rc = alloc_vec(ctx, n, &ws->p[(size_t)i]);
  if (rc) { khip_cg_lanczos_shift_workspace_destroy(ws); return rc; }
  ws->box.st.allocation_timer = take_alloc_seconds();
  *out = ws;
  return KHIP_OK;
}

int khip_cg_lanczos_shift_workspace_adopt(khip_ctx *ctx, int64_t m, int64_t n, int nshifts, double *Mv, double *Mv_prev,
                                          double *Mv_next, double *const *x, double *const *p, khip_cg_lanczos_shift_workspace **out) {
  KHIP_REQUIRE(ctx && out && m >= 0 && n >= 0, "cg_lanczos_shift_workspace_adopt: bad argument");
  KHIP_REQUIRE(nshifts >= 1, "cg_lanczos_shift_workspace_adopt: nshifts must be positive");
  KHIP_REQUIRE(x && p, "cg_lanczos_shift_workspace_adopt: x and p must be arrays of nshifts device vectors");
  std::vector<const double *> all = {Mv, Mv_prev, Mv_next};
  for (int i = 0; i < nshifts; ++i) { all.push_back(x[i]); all.push_back(p[i]); }
  for (const double *q : all)
    KHIP_REQUIRE(n == 0 || q, "cg_lanczos_shift_workspace_adopt: Mv, Mv_prev, Mv_next, x[i], p[i] must be device vectors of n entries");
  if (n > 0) KHIP_TRY(distinct_vectors(all, "cg_lanczos_shift_workspace_adopt"));
  khip_cg_lanczos_shift_workspace *ws = new khip_cg_lanczos_shift_workspace();
  ws->ctx = ctx; ws->m = m; ws->n = n; ws->nshifts = nshifts;
  init_arrays(ws);
  ws->Mv = Mv; ws->Mv_prev = Mv_prev; ws->Mv_next = Mv_next;
  ws->x.assign(x, x + nshifts);
  ws->p.assign(p, p + nshifts);
  for (const double *q : all) ws->borrowed.add(q);
  *out = ws;
  return KHIP_OK;
}

int khip_cg_lanczos_shift_workspace_adopt_vector(khip_cg_lanczos_shift_workspace *ws, const char *name, double *ptr) {
  KHIP_REQUIRE(ws && name, "cg_lanczos_shift_workspace_adopt_vector: null argument");
  for (int i = 0; ptr && i < ws->nshifts; ++i)     // adopt_named's rule, extended to the x / p lists
    KHIP_REQUIRE(ptr != ws->x[(size_t)i] && ptr != ws->p[(size_t)i],
                 "cg_lanczos_shift_workspace_adopt_vector: the pointer for '%s' already is the workspace's '%s[%d]' (every vector needs "
                 "its own storage)", name, ptr == ws->x[(size_t)i] ? "x" : "p", i + 1);
  using S = NamedSlot;
  return adopt_named(ws->ctx, ws->borrowed, {{"Mv", &ws->Mv, S::Fixed}, {"Mv_prev", &ws->Mv_prev, S::Fixed},
                     {"Mv_next", &ws->Mv_next, S::Fixed}, {"v", &ws->v, S::Optional}},
                     "cg_lanczos_shift_workspace_adopt_vector", "vector", name, ptr);
}

int khip_cg_lanczos_shift_workspace_destroy(khip_cg_lanczos_shift_workspace *ws) {
  if (!ws) return KHIP_OK;
  for (double *q : {ws->Mv, ws->Mv_prev, ws->Mv_next, ws->v}) free_unless_borrowed(ws->ctx, ws->borrowed, q);
  for (double *q : ws->x) free_unless_borrowed(ws->ctx, ws->borrowed, q);
  for (double *q : ws->p) free_unless_borrowed(ws->ctx, ws->borrowed, q);
  if (ws->tab) (void)hipFree(ws->tab);
  if (ws->act_dev) (void)hipFree(ws->act_dev);
  if (ws->coef_dev) (void)hipFree(ws->coef_dev);
  ws->loop.release();
  delete ws;
  return KHIP_OK;
}

double *khip_cg_lanczos_shift_solution(khip_cg_lanczos_shift_workspace *ws, int i) {
  return (ws && i >= 0 && i < ws->nshifts) ? ws->x[(size_t)i] : nullptr;
}
const khip_stats *khip_cg_lanczos_shift_stats(khip_cg_lanczos_shift_workspace *ws) { return ws ? &ws->box.st : nullptr; }
int khip_cg_lanczos_shift_last_path(khip_cg_lanczos_shift_workspace *ws) { return ws ? ws->box.path : -1; }
int khip_cg_lanczos_shift_residuals(khip_cg_lanczos_shift_workspace *ws, int i, const double **residuals, int *nres) {
  KHIP_REQUIRE(ws && residuals && nres, "cg_lanczos_shift_residuals: null argument");
  KHIP_REQUIRE(i >= 0 && i < ws->nshifts, "cg_lanczos_shift_residuals: shift index %d out of range", i);
  const std::vector<double> &h = ws->hist[(size_t)i];
  *residuals = h.empty() ? nullptr : h.data();
  *nres = (int)h.size();
  return KHIP_OK;
}
int khip_cg_lanczos_shift_arrays(khip_cg_lanczos_shift_workspace *ws, double *out) {
  KHIP_REQUIRE(ws && out, "cg_lanczos_shift_arrays: null argument");
  const size_t p = (size_t)ws->nshifts;
  const std::vector<double> *dbl[5] = {&ws->rNorms, &ws->sigma, &ws->dhat, &ws->omega, &ws->gamma};
  for (int a = 0; a < 5; ++a) for (size_t i = 0; i < p; ++i) out[a * p + i] = (*dbl[a])[i];
  const std::vector<int> *flg[3] = {&ws->converged, &ws->not_cv, &ws->indefinite};
  for (int a = 0; a < 3; ++a) for (size_t i = 0; i < p; ++i) out[(5 + a) * p + i] = (*flg[a])[i] ? 1.0 : 0.0;
  return KHIP_OK;
}
double *khip_cg_lanczos_shift_vector(khip_cg_lanczos_shift_workspace *ws, const char *name) {
  if (!ws || !name) return nullptr;
  struct { const char *k; double *p; } tab[] = {{"Mv", ws->Mv}, {"Mv_prev", ws->Mv_prev}, {"Mv_next", ws->Mv_next}, {"v", ws->v}};
  for (auto &e : tab) if (strcmp(e.k, name) == 0) return e.p;
  if ((name[0] == 'x' || name[0] == 'p') && name[1]) {             // "x1" .. "xp", "p1" .. "pp"
    char *end = nullptr;
    const long i = strtol(name + 1, &end, 10);
    if (*end == 0 && i >= 1 && i <= ws->nshifts) return (name[0] == 'x' ? ws->x : ws->p)[(size_t)(i - 1)];
  }
  return nullptr;
}
size_t khip_cg_lanczos_shift_workspace_bytes(khip_cg_lanczos_shift_workspace *ws) {
  if (!ws) return 0;
  size_t cnt = 0;
  for (double *q : {ws->Mv, ws->Mv_prev, ws->Mv_next, ws->v}) cnt += q ? 1 : 0;
  for (double *q : ws->x) cnt += q ? 1 : 0;
  for (double *q : ws->p) cnt += q ? 1 : 0;
  return cnt * sizeof(double) * (size_t)ws->n;
}

int khip_cg_lanczos_shift_solve(khip_cg_lanczos_shift_workspace *ws, const khip_operator *A, const khip_operator *M, const double *b,
                                const khip_options *opts_in, const khip_cg_lanczos_shift_params *params) {
  KHIP_REQUIRE(ws && A && b && params, "cg_lanczos_shift_solve: null argument");
  khip_ctx *ctx = ws->ctx;
  const khip_options o = opts_in ? *opts_in : khip_default_options();
  const double t0 = now_s();
  const double timemax = timemax_of(o);
  const int64_t n = ws->n;
  const int p = ws->nshifts;
  khip_stats *st = &ws->box.st;
  const double atol = tol_or_default(o.atol), rtol = tol_or_default(o.rtol);
  const int verbose = o.verbose;
  const bool history = o.history != 0;
  (void)take_alloc_seconds();

  if (int rc = check_shape(ws, {A})) return rc;                                                           // :115-118
  if (ws->m != ws->n) return ws->box.fail(KHIP_ERR_INVALID, "System must be square");
  if (params->nshifts != p) {                                                                             // :121-122
    char msg[160];
    snprintf(msg, sizeof(msg), "workspace.nshifts = %d is inconsistent with length(shifts) = %d", p, params->nshifts);
    return ws->box.fail(KHIP_ERR_INVALID, msg);
  }
  if (p > 0 && !params->shifts) return ws->box.fail(KHIP_ERR_INVALID, "cg_lanczos_shift_solve: shifts is null");
  if (verbose > 0)
    klogf(o.log_fd, "CG-LANCZOS-SHIFT: system of %lld equations in %lld variables with %d shifts\n", (long long)n, (long long)n, p);
  const bool MisI = (M == nullptr);
  if (!MisI && !ws->v) K(alloc_vec(ctx, n, &ws->v));                                                    // :133
  const std::vector<double> shifts(params->shifts, params->shifts + p);
  // reset!(stats)
  ws->box.reset();
  for (auto &h : ws->hist) h.clear();
  std::fill(ws->nhist.begin(), ws->nhist.end(), 0LL);
  double *Mv = ws->Mv, *Mv_prev = ws->Mv_prev, *Mv_next = ws->Mv_next;
  double *v = MisI ? Mv : ws->v;
  auto finish = [&](void) {                                  // there is no Δx here: the stats of the moment, no ws_end
    int any = 0;
    for (int i = 0; i < p; ++i) any |= ws->indefinite[(size_t)i];
    st->indefinite = any;
    ws_finish(ws, t0);
  };
  // the device pointer table of the fused loops: the vectors may have been re-adopted since the last solve
  bool tab_aligned = true;
  if (o.fused) {
    tab_aligned = fill_table(ws);
    if (!ws->tab) K(khip_malloc(ctx, sizeof(double *) * 2 * (size_t)p, reinterpret_cast<void **>(&ws->tab)));
    KHIP_CHECK_HIP(hipMemcpyAsync(ws->tab, ws->tab_host.data(), sizeof(double *) * 2 * (size_t)p, hipMemcpyHostToDevice, ctx->stream));
    KHIP_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  }

  // initial state, the same on every path (:140-172)
  if (o.fused) K(launch_init(ctx, n, p, ws->tab, tab_aligned, nullptr, false));
  else for (int i = 0; i < p; ++i) K(khip_fill(ctx, n, ws->x[(size_t)i], 0.0));
  K(khip_copy(ctx, n, Mv, b));
  if (!MisI) K(apply_op(ctx, M, Mv, v));
  double beta;
  if (MisI) {
    K(khip_nrm2(ctx, n, v, &beta));                          // knorm_elliptic(n, v, Mv) with v === Mv: knorm
  } else {
    double vm;
    K(khip_dot(ctx, n, v, Mv, &vm));
    beta = std::sqrt(vm);
  }
  std::fill(ws->rNorms.begin(), ws->rNorms.end(), beta);
  if (history) for (int i = 0; i < p; ++i) ws->hist[(size_t)i].push_back(beta);
  std::fill(ws->indefinite.begin(), ws->indefinite.end(), 0);
  if (beta == 0) {                                                                                        // :163-169
    st->niter = 0; st->solved = 1; st->inconsistent = 0;
    snprintf(st->status, sizeof(st->status), "x is a zero-residual solution");
    ws->box.path = o.fused ? 1 : 0;
    finish();
    return KHIP_OK;
  }
  if (o.fused) K(launch_init(ctx, n, p, ws->tab, tab_aligned, v, true));                                 // pᵢ ← v (:172-174)
  else for (int i = 0; i < p; ++i) K(khip_copy(ctx, n, ws->p[(size_t)i], v));
  LanczosShiftDevState s;
  memset(&s, 0, sizeof(s));
  s.beta = beta;
  s.inv_beta = 1.0 / beta;
  s.rho = 1.0;                                                                                            // :183
  s.eps_tol = atol + rtol * beta;                                                                         // :190
  s.nshifts = p;
  s.check_curvature = params->check_curvature ? 1 : 0;
  s.stop_seq = kSeqNever;
  std::fill(ws->sigma.begin(), ws->sigma.end(), beta);
  std::fill(ws->dhat.begin(), ws->dhat.end(), 0.0);
  std::fill(ws->omega.begin(), ws->omega.end(), 0.0);
  std::fill(ws->gamma.begin(), ws->gamma.end(), 1.0);
  bool any = false;
  for (int i = 0; i < p; ++i) {                                                                           // :193-196
    ws->converged[(size_t)i] = ws->rNorms[(size_t)i] <= s.eps_tol;
    ws->not_cv[(size_t)i] = !ws->converged[(size_t)i];
    any = any || ws->not_cv[(size_t)i];
  }
  const int64_t itmax = o.itmax == 0 ? 2 * global_rows(ctx, A, n) : o.itmax;
  if (kdisplay(0, verbose)) verbose_row(o, 0, ws->rNorms, t0);
  bool solved = !any, tired = 0 >= itmax, user_exit = false, overtimed = false;
  int64_t iter = 0;
  const LzShiftArrays ha = host_arrays(ws, shifts.data());

  const bool device_loop = o.fused >= 2 && A->csr && !A->apply && MisI && !o.callback && verbose <= 0 && p <= kShiftMax;
  ws->box.path = device_loop ? 2 : (o.fused ? 1 : 0);

  if (ws->box.path == 0) {
    // ---------------------------------------------------------------- the reference's primitive sequence (:205-267) ----
    K(khip_div(ctx, n, v, beta));                                                                         // :177-179
    if (!MisI) K(khip_div(ctx, n, Mv, beta));
    K(khip_copy(ctx, n, Mv_prev, Mv));
    while (!(solved || tired || user_exit || overtimed)) {
      K(apply_op(ctx, A, v, Mv_next));
      K(khip_dot(ctx, n, v, Mv_next, &s.delta));
      K(khip_axpy(ctx, n, -s.delta, Mv, Mv_next));
      if (iter > 0) {
        K(khip_axpy(ctx, n, -s.beta, Mv_prev, Mv_next));
        K(khip_copy(ctx, n, Mv_prev, Mv));
      }
      K(khip_copy(ctx, n, Mv, Mv_next));
      if (!MisI) K(apply_op(ctx, M, Mv, v));
      if (MisI) {
        K(khip_nrm2(ctx, n, v, &s.beta));                   // knorm_elliptic(n, v, Mv) with v === Mv: knorm
        s.inv_beta = 1.0 / s.beta;
      } else {
        double b2;
        K(khip_dot(ctx, n, v, Mv, &b2));
        lzshift_beta(s, b2);
      }
      K(khip_div(ctx, n, v, s.beta));
      if (!MisI) K(khip_div(ctx, n, Mv, s.beta));
      if (!MisI) K(khip_dot(ctx, n, v, v, &s.rho));
      std::vector<double> row((size_t)p, 0.0);
      solved = lzshift_step(s, ha, iter + 1, row.data());
      for (int j = 0; j < ws->act[0]; ++j) {
        const size_t i = (size_t)ws->act[1 + (size_t)j];
        K(khip_axpy(ctx, n, ws->gamma[i], ws->p[i], ws->x[i]));
        K(khip_axpby(ctx, n, ws->sigma[i], v, ws->omega[i], ws->p[i]));
        if (history) ws->hist[i].push_back(row[i]);
      }
      iter = iter + 1;
      if (kdisplay(iter, verbose)) verbose_row(o, iter, ws->rNorms, t0);
      if (o.callback) {
        KHIP_CHECK_HIP(hipStreamSynchronize(ctx->stream));
        finish();                                 // the callback sees the timers and the indefinite flag of the moment
      }
      tired = iter >= itmax;
      host_exit(ws, o, t0, timemax, &user_exit, &overtimed);
    }
  } else if (ws->box.path == 1) {
    // ---------------------------------------------------------------- host-driven loop on the fused kernels ----------
    K(ws->loop.alloc());
    if (!ws->act_dev) K(khip_malloc(ctx, sizeof(int) * (size_t)(p + 1), reinterpret_cast<void **>(&ws->act_dev)));
    if (!ws->coef_dev) K(khip_malloc(ctx, sizeof(double) * 3 * (size_t)p, reinterpret_cast<void **>(&ws->coef_dev)));
    K(khip_div(ctx, n, v, beta));                                                                         // :177-178
    if (!MisI) K(khip_div(ctx, n, Mv, beta));
    double *cur = Mv, *prev = Mv_prev, *nxt = Mv_next;      // Mv_prev ← Mv (:179) is not needed: iteration 1 does not read it
    std::vector<double> row((size_t)p, 0.0);
    while (!(solved || tired || user_exit || overtimed)) {
      const int64_t k = iter + 1;
      const double *vin = MisI ? cur : v;
      int slot = take_slots(ctx, 1);
      if (A->csr && !A->apply) {
        K(spmv_any(ctx, A->csr, vin, nxt, slot));                                        // y = A v ; v.y
      } else {
        K(apply_op(ctx, A, vin, nxt));
        K(launch_dot(ctx, n, vin, nxt, slot));
      }
      K(fetch_results(ctx, slot, 1, &s.delta));
      K(ws->loop.upload(ctx, s));
      slot = take_slots(ctx, 1);
      K(launch_p1(ctx, n, ws->loop.dev, prev, cur, nxt, k >= 2, MisI, slot));           // w ; w.w
      double b2;
      if (MisI) {
        K(fetch_results(ctx, slot, 1, &b2));
      } else {
        K(apply_op(ctx, M, nxt, v));
        K(khip_dot(ctx, n, v, nxt, &b2));
      }
      lzshift_beta(s, b2);
      if (!MisI) {
        K(ws->loop.upload(ctx, s));
        slot = take_slots(ctx, 1);
        K(launch_scale(ctx, n, ws->loop.dev, v, nxt, slot));                             // v, Mv /= β ; ρ = v.v
        K(fetch_results(ctx, slot, 1, &s.rho));
      }
      solved = lzshift_step(s, ha, k, row.data());
      K(ws->loop.upload(ctx, s));
      K(upload_coefs(ws));
      K(launch_p2(ctx, n, &ws->loop.dev->inv_beta, ws->act_dev, ws->coef_dev, ws->tab, tab_aligned, MisI ? nxt : v, MisI));
      double *old_prev = prev;                                                            // Mv_prev <- Mv ; Mv <- Mv_next
      prev = cur; cur = nxt; nxt = old_prev;
      if (history) for (int j = 0; j < ws->act[0]; ++j) ws->hist[(size_t)ws->act[1 + (size_t)j]].push_back(row[(size_t)ws->act[1 + (size_t)j]]);
      iter = k;
      if (kdisplay(iter, verbose)) verbose_row(o, iter, ws->rNorms, t0);
      if (o.callback) {
        KHIP_CHECK_HIP(hipStreamSynchronize(ctx->stream));
        finish();                                 // the callback sees the timers and the indefinite flag of the moment
      }
      tired = iter >= itmax;
      host_exit(ws, o, t0, timemax, &user_exit, &overtimed);
    }
    ws->Mv = cur; ws->Mv_prev = prev; ws->Mv_next = nxt;
  } else if (!(solved || tired)) {
    // ---------------------------------------------------------------- device-resident loop -----------------------------
    for (int i = 0; i < p; ++i) {
      s.shifts[i] = shifts[(size_t)i];
      s.sigma[i] = ws->sigma[(size_t)i]; s.dhat[i] = ws->dhat[(size_t)i]; s.omega[i] = ws->omega[(size_t)i];
      s.gamma[i] = ws->gamma[(size_t)i]; s.rNorms[i] = ws->rNorms[(size_t)i];
      s.converged[i] = ws->converged[(size_t)i]; s.not_cv[i] = ws->not_cv[(size_t)i]; s.indefinite[i] = 0;
    }
    K(khip_div(ctx, n, v, beta));                                                                         // v₁ = Mv₁ / β₁
    struct Roles {                                            // Mv_prev <- Mv ; Mv <- Mv_next as a rotation of the roles
      double *cur, *prev, *nxt;
      void rotate() { double *old_prev = prev; prev = cur; cur = nxt; nxt = old_prev; }
    };
    const Roles first{Mv, Mv_prev, Mv_next};
    Roles B = first;
    auto step = [&](LanczosShiftDevState *dev, long long j) {
      const int64_t k = j + 1;
      KHIP_TRY(dev_stage(ctx, dev, 3 * j + 1, EPI_LZSHIFT_A, 1, [&](int slot) {
        return spmv_any(ctx, A->csr, B.cur, B.nxt, slot); }));                           // P0: y = A v ; v.y -> δ
      KHIP_TRY(dev_stage(ctx, dev, 3 * j + 2, EPI_LZSHIFT_B, 1, [&](int slot) {
        return launch_p1(ctx, n, dev, B.prev, B.cur, B.nxt, k >= 2, true, slot); }));   // P1: w ; w.w -> β, the shifts' step
      KHIP_TRY(dev_pass(ctx, &dev->stop_seq, 3 * j + 3, EPI_NONE, dev, [&] {
        return launch_p2(ctx, n, &dev->inv_beta, dev->act, dev->coef, ws->tab, tab_aligned, B.nxt, true); }));   // P2: v ; x_i, p_i
      B.rotate();
      return (int)KHIP_OK;
    };
    DeviceLoopArgs loop_args = device_loop_args(itmax, t0, timemax, history, {});
    loop_args.width = p;
    loop_args.columns = ws->hist.data();
    K(ws->loop.run(ctx, s, loop_args, step, &s, &overtimed));
    iter = s.iter;
    tired = iter >= itmax;
    solved = s.solved != 0;
    for (int i = 0; i < p; ++i) {
      ws->sigma[(size_t)i] = s.sigma[i]; ws->dhat[(size_t)i] = s.dhat[i]; ws->omega[(size_t)i] = s.omega[i];
      ws->gamma[(size_t)i] = s.gamma[i]; ws->rNorms[(size_t)i] = s.rNorms[i];
      ws->converged[(size_t)i] = s.converged[i]; ws->not_cv[(size_t)i] = s.not_cv[i]; ws->indefinite[(size_t)i] = s.indefinite[i];
      ws->nhist[(size_t)i] = s.nhist[i];
    }
    B = replay(first, iter, 3, [](Roles &r) { r.rotate(); });
    ws->Mv = B.cur; ws->Mv_prev = B.prev; ws->Mv_next = B.nxt;
  }
  if (verbose > 0) klogf(o.log_fd, "\n");
  const char *status = "unknown";                                                                         // :269-273
  if (tired) status = "maximum number of iterations exceeded";
  if (solved) status = "solution good enough given atol and rtol";
  if (user_exit) status = "user-requested exit";
  if (overtimed) status = "time limit exceeded";
  st->niter = (int)iter;
  st->solved = solved ? 1 : 0;
  st->inconsistent = 0;
  snprintf(st->status, sizeof(st->status), "%s", status);
  finish();
  return KHIP_OK;
}

}  // extern "C"
