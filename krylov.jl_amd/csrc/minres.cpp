// minres.cpp -- minres! (src/minres.jl:164-484) above the device primitives, with its fused gfx950 kernels.
//
// Real Float64, linesearch = false.  Three loops, chosen as for cg! (khip_minres_last_path):
//   0  options.fused = 0: the reference's primitive sequence, one launch per k* call, one host sync per kdotr / knorm;
//   1  the host-driven loop on the fused kernels below (with M, a user operator, a callback or verbose > 0);
//   2  the device-resident loop (default): the scalar recurrences and stopping tests run as the epilogues of the three
//      reductions of an iteration (minres_step_a/b/c, solver_device.hpp), iterations are enqueued ahead.
// One iteration with M = I on the fused paths:
//   SpMV+P1  y = ((A v + lambda v) / beta) - (beta / oldbeta) r1 ; v.y               the sliced SpMV with its Lanczos epilogue
//                                                                                    (+ 8n for r1); other products: y = A v, then
//                                                                                    minres_p1_kernel (32n)
//   P2       y -= (alpha / beta) v ; w <- -eps w1 - delta w2 + v / beta ; y.y        48n bytes
//   P3       w /= gamma ; x += phi w ; x.x                                           32n bytes
// and kcopy!(r1, r2), kcopy!(r2, y), @kswap!(w1, w2) become a rotation of the buffers' roles.  Every elementwise value uses the
// expression of the primitive it replaces (fma for kaxpy!, kscal! by one(T)/s for kdiv!, / for kdivcopy!, a * y for kscal!):
// the fused loops agree with the primitive sequence bit for bit on elementwise values and to the reductions' one ulp otherwise;
// loops 1 and 2 run the same kernels and the same scalar code and produce the same bits.
#include <chrono>
#include <utility>

#include "solver_host.hpp"
#include "vec_launch.hpp"

using namespace khip;

namespace khip {   // (named, not anonymous: stable kernel names in traces)

// ---------------------------------------------------------------------------------------------------------- kernels ----
// Each thread owns one VEC-vector of every stream; the odd tail element (VEC = 2, n odd) goes to thread 0 of block 0.

// P1: y = ((y + lambda v) * (1 / beta)) + c_r1 r1 ; acc = v . y          (src/minres.jl:283-287)
template <int VEC, bool NT, bool COMP>
__global__ __launch_bounds__(kBlock) void minres_p1_kernel(int64_t n, const MinresDevState *st, const double *v, const double *r1,
                                                          double *y, int sub_r1, RedArgs ra) {
  using T = typename VecT<VEC>::type;
  if (seq_skip(ra.stop_seq, ra.seq)) return;
  const double lam = st->lambda, ib = st->inv_beta, c1 = st->c_r1;
  const bool use_lam = lam != 0.0;
  dd acc[1] = {dd{0.0, 0.0}};
  const int64_t nvec = n / VEC;
  const int64_t i = lane_index();
  auto one = [&](double ye, double ve, double re) {
    double t = ye;
    if (use_lam) t = fma(lam, ve, t);
    t = ib * t;
    if (sub_r1) t = fma(c1, re, t);
    acc_prod<COMP>(acc[0], ve, t);
    return t;
  };
  if (i < nvec) {
    const T yv = ldg<NT>(reinterpret_cast<const T *>(y) + i);
    const T vv = ldg<false>(reinterpret_cast<const T *>(v) + i);      // v is read again by P2
    T rv = {};
    if (sub_r1) rv = ldg<NT>(reinterpret_cast<const T *>(r1) + i);
    T yo;
#pragma unroll
    for (int e = 0; e < VEC; ++e) vset(yo, e, one(vget(yv, e), vget(vv, e), vget(rv, e)));
    stg<false>(yo, reinterpret_cast<T *>(y) + i);                      // y is read again by P2
  }
  if (VEC == 2 && owns_tail(n)) {
    const int64_t t = n - 1;
    y[t] = one(y[t], v[t], sub_r1 ? r1[t] : 0.0);
  }
  wave_publish<1>(acc, ra);
}

// P2: y = fma(c_r2, r2, y) ; w = first ? v / beta : fma(1/beta, v, fma(-delta, w2, scal ? (-eps) w1 : w1)) ; acc = y . y
// (src/minres.jl:288-302).  w is written to w2 in iteration 1 and to w1 after; with M = I, r2 === v.
template <int VEC, bool NT, bool COMP>
__global__ __launch_bounds__(kBlock) void minres_p2_kernel(int64_t n, const MinresDevState *st, const double *r2, const double *v,
                                                          double *y, double *w1, double *w2, int first, int scal, int dot,
                                                          RedArgs ra) {
  using T = typename VecT<VEC>::type;
  if (seq_skip(ra.stop_seq, ra.seq)) return;
  const double c2 = st->c_r2, beta = st->beta, ib = st->inv_beta, nd = -st->delta, ne = -st->epsln;
  const bool same = (r2 == v);
  dd acc[1] = {dd{0.0, 0.0}};
  const int64_t nvec = n / VEC;
  const int64_t i = lane_index();
  auto one = [&](double ye, double re, double ve, double w1e, double w2e, double &wo) {
    const double yn = fma(c2, re, ye);
    if (first) {
      wo = ve / beta;
    } else {
      double w = w1e;
      if (scal) w = ne * w;
      w = fma(nd, w2e, w);
      wo = fma(ib, ve, w);
    }
    if (dot) acc_prod<COMP>(acc[0], yn, yn);
    return yn;
  };
  if (i < nvec) {
    const T yv = ldg<NT>(reinterpret_cast<const T *>(y) + i);
    const T rv = ldg<NT>(reinterpret_cast<const T *>(r2) + i);
    const T vv = same ? rv : ldg<NT>(reinterpret_cast<const T *>(v) + i);
    T w1v = {}, w2v = {};
    if (!first) {
      w1v = ldg<NT>(reinterpret_cast<const T *>(w1) + i);
      w2v = ldg<NT>(reinterpret_cast<const T *>(w2) + i);
    }
    T yo, wo;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      double we;
      vset(yo, e, one(vget(yv, e), vget(rv, e), vget(vv, e), vget(w1v, e), vget(w2v, e), we));
      vset(wo, e, we);
    }
    stg<NT>(yo, reinterpret_cast<T *>(y) + i);
    stg<false>(wo, reinterpret_cast<T *>(first ? w2 : w1) + i);       // w is read again by P3
  }
  if (VEC == 2 && owns_tail(n)) {
    const int64_t t = n - 1;
    double we;
    y[t] = one(y[t], r2[t], v[t], first ? 0.0 : w1[t], first ? 0.0 : w2[t], we);
    (first ? w2 : w1)[t] = we;
  }
  wave_publish<1>(acc, ra);
}

// P3: w = (1 / gamma) w ; x = fma(phi, w, x) ; acc = x . x                 (src/minres.jl:325, :376, :386)
template <int VEC, bool NT, bool COMP>
__global__ __launch_bounds__(kBlock) void minres_p3_kernel(int64_t n, const MinresDevState *st, double *w, double *x, RedArgs ra) {
  using T = typename VecT<VEC>::type;
  if (seq_skip(ra.stop_seq, ra.seq)) return;
  const double ig = st->inv_gamma, phi = st->phi;
  dd acc[1] = {dd{0.0, 0.0}};
  const int64_t nvec = n / VEC;
  const int64_t i = lane_index();
  if (i < nvec) {
    const T wv = ldg<false>(reinterpret_cast<const T *>(w) + i);
    const T xv = ldg<NT>(reinterpret_cast<const T *>(x) + i);
    T wo, xo;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const double wn = ig * vget(wv, e);
      const double xn = fma(phi, wn, vget(xv, e));
      vset(wo, e, wn);
      vset(xo, e, xn);
      acc_prod<COMP>(acc[0], xn, xn);
    }
    stg<NT>(wo, reinterpret_cast<T *>(w) + i);
    stg<NT>(xo, reinterpret_cast<T *>(x) + i);
  }
  if (VEC == 2 && owns_tail(n)) {
    const int64_t t = n - 1;
    const double wn = ig * w[t];
    const double xn = fma(phi, wn, x[t]);
    w[t] = wn;
    x[t] = xn;
    acc_prod<COMP>(acc[0], xn, xn);
  }
  wave_publish<1>(acc, ra);
}

}  // namespace khip

namespace {

constexpr ScalarPathNT kScalarNT = ScalarPathNT::never;

int launch_p1(khip_ctx *ctx, int64_t n, const MinresDevState *st, const double *v, const double *r1, double *y, bool sub_r1,
              int slot) {
  VecPlan L;
  KHIP_TRY(vec_plan(ctx, n, {v, sub_r1 ? r1 : nullptr, y}, &L, 1));
  RedArgs ra = make_red_args(ctx, slot);
  vec_dispatch<kScalarNT>(L, [&](auto V, auto N, auto C) {
    hipLaunchKernelGGL((minres_p1_kernel<V, N, C>), L.grid(), dim3(kBlock), 0, ctx->stream, n, st, v, r1, y, sub_r1 ? 1 : 0, ra); });
  KHIP_CHECK_HIP(hipGetLastError());
  return launch_finish(ctx, L.waves(), 1, slot);
}
int launch_p2(khip_ctx *ctx, int64_t n, const MinresDevState *st, const double *r2, const double *v, double *y, double *w1,
              double *w2, int k, bool dot, int slot) {
  VecPlan L;
  KHIP_TRY(vec_plan(ctx, n, {r2, v, y, w1, w2}, &L, 1));
  RedArgs ra = make_red_args(ctx, slot);
  vec_dispatch<kScalarNT>(L, [&](auto V, auto N, auto C) {
    hipLaunchKernelGGL((minres_p2_kernel<V, N, C>), L.grid(), dim3(kBlock), 0, ctx->stream, n, st, r2, v, y, w1, w2, k == 1 ? 1 : 0,
                       k >= 3 ? 1 : 0, dot ? 1 : 0, ra); });
  KHIP_CHECK_HIP(hipGetLastError());
  if (!dot) return KHIP_OK;        // the partials are not folded: nothing reads them
  return launch_finish(ctx, L.waves(), 1, slot);
}
int launch_p3(khip_ctx *ctx, int64_t n, const MinresDevState *st, double *w, double *x, int slot) {
  VecPlan L;
  KHIP_TRY(vec_plan(ctx, n, {w, x}, &L, 1));
  RedArgs ra = make_red_args(ctx, slot);
  vec_dispatch<kScalarNT>(L, [&](auto V, auto N, auto C) {
    hipLaunchKernelGGL((minres_p3_kernel<V, N, C>), L.grid(), dim3(kBlock), 0, ctx->stream, n, st, w, x, ra); });
  KHIP_CHECK_HIP(hipGetLastError());
  return launch_finish(ctx, L.waves(), 1, slot);
}

// y = A v followed by P1, reduction v.y into results[slot].  fuse (SpmvPlan::carries_lanczos): ONE launch -- the sliced SpMV applies the
// Lanczos epilogue to each row's product and forms v.y in its fused dot; otherwise the plain product, then P1.  Same elementwise
// expressions either way; under ctx->ctl the epilogue of the reduction runs in its finish kernel.
int lanczos_product(khip_ctx *ctx, const khip_operator *A, bool fuse, int64_t n, const MinresDevState *st, const double *v,
                    const double *r1, double *y, bool sub_r1, int slot) {
  if (fuse) {
    ctx->lz = LanczosEpi{&st->lambda, r1, sub_r1 ? 1 : 0};
    const int rc = spmv_any(ctx, A->csr, v, y, slot);
    ctx->lz = LanczosEpi{};
    return rc;
  }
  KHIP_TRY(apply_op_no_epilogue(ctx, A, v, y));
  return launch_p1(ctx, n, st, v, r1, y, sub_r1, slot);
}

}  // namespace

struct khip_minres_workspace {
  khip_ctx *ctx;
  int64_t m, n;
  int window;
  double *dx = nullptr, *x = nullptr, *r1 = nullptr, *r2 = nullptr, *npc_dir = nullptr, *w1 = nullptr, *w2 = nullptr,
         *y = nullptr, *v = nullptr;
  Borrowed borrowed;                        // the caller's vectors (khip_minres_workspace_adopt*): never freed here
  std::vector<double> err_vec;
  bool warm_start = false;
  StatsBox box;
  std::vector<double> aresiduals, aconds;   // the Aresiduals / Acond histories next to box.residuals
  bool fused_product = false;               // the last solve's Lanczos epilogue ran inside the sliced SpMV
  DeviceLoop<MinresDevState, 3> loop;       // fused loops: device copy of the scalar state, pinned snapshots + staging, histories
};

namespace {

// x, r1, r2, w1, w2, y come with the workspace; dx, v, npc_dir stay empty until needed (src/krylov_workspaces.jl:94-112)
using W = khip_minres_workspace;
constexpr WsVec<W> kVectors[] = {{"x", &W::x, Core},   {"r1", &W::r1, Core}, {"r2", &W::r2, Core},
                                 {"w1", &W::w1, Core}, {"w2", &W::w2, Core}, {"y", &W::y, Core},
                                 {"dx", &W::dx, Lazy}, {"v", &W::v, Lazy},   {"npc_dir", &W::npc_dir, Lazy}};

struct Bufs {
  double *x, *r1, *r2, *y, *v, *w1, *w2;   // v == r2 when M = I
};

void verbose_row(const khip_options &o, long long iter, const MinresDevState &s, double t0, bool first_row) {
  if (first_row)
    klogf(o.log_fd, "%5lld  %7.1e  %7.1e  %7.1e  %8.1e  %8.1e  %7.1e  %7.1e  %7s  %7s  %.2fs\n", iter, s.rNorm, s.ArNorm, s.beta,
          s.cs, s.sn, s.ANorm, s.Acond, "\xe2\x9c\x97 \xe2\x9c\x97 \xe2\x9c\x97 \xe2\x9c\x97",
          "\xe2\x9c\x97 \xe2\x9c\x97 \xe2\x9c\x97 \xe2\x9c\x97", now_s() - t0);
  else
    klogf(o.log_fd, "%5lld  %7.1e  %7.1e  %7.1e  %8.1e  %8.1e  %7.1e  %7.1e  %7.1e  %7.1e  %.2fs\n", iter, s.rNorm, s.ArNorm, s.beta,
          s.cs, s.sn, s.ANorm, s.Acond, s.test1, s.test2, now_s() - t0);
}

}  // namespace

extern "C" {

khip_minres_params khip_minres_default_params(void) {
  khip_minres_params p;
  p.lambda = 0.0;
  p.etol = NAN;
  p.conlim = NAN;
  return p;
}

int khip_minres_workspace_create(khip_ctx *ctx, int64_t m, int64_t n, int window, khip_minres_workspace **out) {
  KHIP_REQUIRE(ctx && out && m >= 0 && n >= 0, "minres_workspace_create: bad argument");
  KHIP_REQUIRE(window >= 1, "minres_workspace_create: window must be positive");
  khip_minres_workspace *ws = new khip_minres_workspace();
  ws->ctx = ctx; ws->m = m; ws->n = n; ws->window = window;
  ws->err_vec.assign((size_t)window, 0.0);
  const int rc = ws_create_core(ws, kVectors);
  if (rc) { khip_minres_workspace_destroy(ws); return rc; }
  *out = ws;
  return KHIP_OK;
}

int khip_minres_workspace_adopt(khip_ctx *ctx, int64_t m, int64_t n, int window, double *x, double *r1, double *r2, double *w1,
                                double *w2, double *y, khip_minres_workspace **out) {
  KHIP_REQUIRE(ctx && out && m >= 0 && n >= 0, "minres_workspace_adopt: bad argument");
  KHIP_REQUIRE(window >= 1, "minres_workspace_adopt: window must be positive");
  khip_minres_workspace *ws = new khip_minres_workspace();
  ws->ctx = ctx; ws->m = m; ws->n = n; ws->window = window;
  ws->err_vec.assign((size_t)window, 0.0);
  const int rc = ws_adopt_core(ws, kVectors, "minres_workspace_adopt", {x, r1, r2, w1, w2, y});
  if (rc) { delete ws; return rc; }
  *out = ws;
  return KHIP_OK;
}

int khip_minres_workspace_adopt_vector(khip_minres_workspace *ws, const char *name, double *ptr) {
  return ws_adopt_vector(ws, kVectors, "minres_workspace_adopt_vector", name, ptr);
}

int khip_minres_workspace_destroy(khip_minres_workspace *ws) {
  if (!ws) return KHIP_OK;
  ws_free_vectors(ws, kVectors);
  ws->loop.release();
  delete ws;
  return KHIP_OK;
}

int khip_minres_warm_start(khip_minres_workspace *ws, const double *x0) { return ws_warm_start(ws, kVectors, x0, "minres_warm_start"); }

double *khip_minres_solution(khip_minres_workspace *ws) { return ws ? ws->x : nullptr; }
const khip_stats *khip_minres_stats(khip_minres_workspace *ws) { return ws ? &ws->box.st : nullptr; }
int khip_minres_last_path(khip_minres_workspace *ws) { return ws ? ws->box.path : -1; }
int khip_minres_fused_product(khip_minres_workspace *ws) { return ws ? (ws->fused_product ? 1 : 0) : -1; }
int khip_minres_histories(khip_minres_workspace *ws, const double **aresiduals, int *naresiduals, const double **acond,
                          int *nacond) {
  KHIP_REQUIRE(ws && aresiduals && naresiduals && acond && nacond, "minres_histories: null argument");
  *aresiduals = ws->aresiduals.empty() ? nullptr : ws->aresiduals.data();
  *naresiduals = (int)ws->aresiduals.size();
  *acond = ws->aconds.empty() ? nullptr : ws->aconds.data();
  *nacond = (int)ws->aconds.size();
  return KHIP_OK;
}
double *khip_minres_vector(khip_minres_workspace *ws, const char *name) { return ws_vector(ws, kVectors, name); }
size_t khip_minres_workspace_bytes(khip_minres_workspace *ws) { return ws_bytes(ws, kVectors); }

int khip_minres_solve(khip_minres_workspace *ws, const khip_operator *A, const khip_operator *M, const double *b,
                      const khip_options *opts_in, const khip_minres_params *params_in) {
  KHIP_REQUIRE(ws && A && b, "minres_solve: null argument");
  khip_ctx *ctx = ws->ctx;
  const khip_options o = opts_in ? *opts_in : khip_default_options();
  const khip_minres_params prm = params_in ? *params_in : khip_minres_default_params();
  const double t0 = now_s();
  const double timemax = timemax_of(o);
  const int64_t n = ws->n;
  const double atol = tol_or_default(o.atol), rtol = tol_or_default(o.rtol), etol = tol_or_default(prm.etol);
  const double conlim = std::isnan(prm.conlim) ? 1.0 / std::sqrt(kEps) : prm.conlim;
  const double lambda = prm.lambda;
  const int verbose = o.verbose;
  (void)take_alloc_seconds();

  if (A->csr && !A->apply) {
    int64_t am, an;
    khip_csr_shape(A->csr, &am, &an, nullptr);
    if (am != ws->m) return ws->box.fail(KHIP_ERR_INVALID, "(workspace.m, workspace.n) is inconsistent with size(A)");
  }
  if (ws->m != ws->n) return ws->box.fail(KHIP_ERR_INVALID, "System must be square");
  if (verbose > 0) klogf(o.log_fd, "MINRES: system of size %lld\n", (long long)n);                       // src/minres.jl:180
  if (o.linesearch)
    return ws->box.fail(KHIP_ERR_UNSUPPORTED, "minres: linesearch = true (nonpositive-curvature detection) is not supported");
  const bool MisI = (M == nullptr);
  if (!MisI && !ws->v) K(alloc_vec(ctx, n, &ws->v));                                                     // :192
  const bool warm_start = ws->warm_start;
  // reset!(stats)
  ws->box.reset(); ws->aresiduals.clear(); ws->aconds.clear();
  ws->fused_product = false;
  Bufs B{ws->x, ws->r1, ws->r2, ws->y, MisI ? ws->r2 : ws->v, ws->w1, ws->w2};
  const double ctol = conlim > 0 ? 1.0 / conlim : 0.0;
  const bool history = o.history != 0;

  // set-up, the same primitives on every path (:208-231)
  K(khip_fill(ctx, n, B.x, 0.0));
  K(residual0(ws, A, lambda, b, warm_start, B.r1));
  K(khip_copy(ctx, n, B.r2, B.r1));
  if (!MisI) K(apply_op(ctx, M, B.r1, B.v));
  double beta1;
  K(khip_dot(ctx, n, B.r1, B.v, &beta1));
  if (beta1 < 0) return ws->box.fail(KHIP_ERR_NUMERIC, "Preconditioner is not positive definite");
  if (beta1 == 0) {                                                                                       // :233-244
    if (history) { ws->box.residuals.push_back(beta1); ws->aresiduals.push_back(0.0); ws->aconds.push_back(0.0); }
    ws->box.path = o.fused ? 1 : 0;
    return ws_end(ws, {1, 1, 0, "x is a zero-residual solution", warm_start, t0, false});   // niter = 1, as the least-squares exit
  }
  beta1 = std::sqrt(beta1);
  MinresDevState s;
  memset(&s, 0, sizeof(s));
  s.lambda = lambda; s.beta1 = beta1; s.beta = beta1; s.oldbeta = 0.0; s.dbar = 0.0; s.epsln = 0.0;
  s.rNorm = beta1; s.phibar = beta1; s.rhs1 = beta1; s.rhs2 = 0.0; s.gmax = 0.0;
  s.gmin = std::numeric_limits<double>::infinity(); s.cs = -1.0; s.sn = 0.0;
  s.ANorm2 = 0.0; s.ANorm = 0.0; s.Acond = 0.0; s.ArNorm = 0.0; s.xNorm = 0.0; s.xENorm2 = 0.0; s.err_lbnd = 0.0;
  s.eps_tol = atol + rtol * beta1; s.etol = etol; s.ctol = ctol;
  s.window = ws->window; s.MisI = MisI ? 1 : 0;
  s.inv_beta = 1.0 / beta1;
  s.stop_seq = kSeqNever;
  if (history) { ws->box.residuals.push_back(beta1); ws->aconds.push_back(0.0); ws->aresiduals.push_back(0.0); }
  K(khip_fill(ctx, n, B.w1, 0.0));
  K(khip_fill(ctx, n, B.w2, 0.0));
  std::fill(ws->err_vec.begin(), ws->err_vec.end(), 0.0);
  const int64_t itmax = o.itmax == 0 ? 2 * global_rows(ctx, A, n) : o.itmax;
  s.itmax = itmax;
  if (verbose > 0) {
    klogf(o.log_fd, "%5s  %7s  %7s  %7s  %8s  %8s  %7s  %7s  %7s  %7s  %5s\n", "k", "\xe2\x80\x96r\xe2\x80\x96",
          "\xe2\x80\x96" "A\xe1\xb4\xb4" "r\xe2\x80\x96", "\xce\xb2", "cos", "sin", "\xe2\x80\x96" "A\xe2\x80\x96", "\xce\xba(A)", "test1",
          "test2", "timer");
    verbose_row(o, 0, s, t0, true);
  }
  s.zero_resid = (s.rNorm <= s.eps_tol) ? 1 : 0;
  bool tired = 0 >= itmax, user_exit = false, overtimed = false, stop = tired;
  int64_t iter = 0;

  const bool device_loop = o.fused >= 2 && A->csr && !A->apply && MisI && !o.callback && verbose <= 0 &&
                           ws->window <= kMinresWindowMax;
  ws->box.path = device_loop ? 2 : (o.fused ? 1 : 0);
  // the Lanczos epilogue inside the product: fused loops on a CSR handle whose product runs the sliced kernel (both fused loops decide
  // alike, so they keep producing the same bits)
  const bool fuse = ws->box.path >= 1 && A->csr && !A->apply && spmv_plan(ctx, A->csr, true).carries_lanczos();
  ws->fused_product = fuse;

  if (ws->box.path == 0) {
    // ---------------------------------------------------------------- the reference's primitive sequence (:283-451) ----
    double *w = nullptr;
    while (!stop) {
      const int64_t k = ++iter;
      K(apply_op(ctx, A, B.v, B.y));
      if (lambda != 0) K(khip_axpy(ctx, n, lambda, B.v, B.y));
      K(khip_div(ctx, n, B.y, s.beta));
      if (k >= 2) K(khip_axpy(ctx, n, -s.beta / s.oldbeta, B.r1, B.y));
      double vy;
      K(khip_dot(ctx, n, B.v, B.y, &vy));
      minres_step_a(s, vy);
      K(khip_axpy(ctx, n, -s.alpha / s.beta, B.r2, B.y));
      if (k == 1) {
        w = B.w2;
        K(khip_divcopy(ctx, n, w, B.v, s.beta));
      } else {
        w = B.w1;
        if (k >= 3) K(khip_scal(ctx, n, -s.epsln, w));
        K(khip_axpy(ctx, n, -s.delta, B.w2, w));
        K(khip_axpy(ctx, n, 1.0 / s.beta, B.v, w));
      }
      K(khip_copy(ctx, n, B.r1, B.r2));
      K(khip_copy(ctx, n, B.r2, B.y));
      if (!MisI) K(apply_op(ctx, M, B.r2, B.v));
      double b2;
      K(khip_dot(ctx, n, B.r2, B.v, &b2));
      if (!minres_step_b(s, b2, k)) return ws->box.fail(KHIP_ERR_NUMERIC, "Preconditioner is not positive definite");
      if (history) ws->aresiduals.push_back(s.ArNorm);
      K(khip_div(ctx, n, w, s.gamma));
      K(khip_axpy(ctx, n, s.phi, w, B.x));
      if (k >= 2) std::swap(B.w1, B.w2);
      double xNorm;
      K(khip_nrm2(ctx, n, B.x, &xNorm));
      stop = minres_step_c(s, xNorm, k, ws->err_vec.data());
      if (history) { ws->box.residuals.push_back(s.rNorm); ws->aconds.push_back(s.Acond); }
      if (kdisplay(k, verbose)) verbose_row(o, k, s, t0, false);
      if (s.lsq_exit) break;
      tired = k >= itmax;
      host_exit(ws, o, t0, timemax, &user_exit, &overtimed);
      stop = stop || user_exit || overtimed;
    }
  } else if (ws->box.path == 1) {
    // ---------------------------------------------------------------- host-driven loop on the fused kernels ----------
    K(ws->loop.alloc());
    s.hist_r = s.hist_ar = s.hist_acond = nullptr;
    while (!stop) {
      const int64_t k = ++iter;
      K(ws->loop.upload(ctx, s));
      int slot = take_slots(ctx, 1);
      K(lanczos_product(ctx, A, fuse, n, ws->loop.dev, B.v, B.r1, B.y, k >= 2, slot));
      double vy;
      K(fetch_results(ctx, slot, 1, &vy));
      minres_step_a(s, vy);
      K(ws->loop.upload(ctx, s));
      slot = take_slots(ctx, 1);
      K(launch_p2(ctx, n, ws->loop.dev, B.r2, B.v, B.y, B.w1, B.w2, (int)std::min<int64_t>(k, 3), MisI, slot));
      double *w = k == 1 ? B.w2 : B.w1;
      double *old_r1 = B.r1;                       // r1 <- r2 ; r2 <- y (:303-304) as a rotation of the roles
      B.r1 = B.r2; B.r2 = B.y; B.y = old_r1;
      double b2;
      if (MisI) {
        B.v = B.r2;
        K(fetch_results(ctx, slot, 1, &b2));
      } else {
        K(apply_op(ctx, M, B.r2, B.v));
        K(khip_dot(ctx, n, B.r2, B.v, &b2));
      }
      if (!minres_step_b(s, b2, k)) return ws->box.fail(KHIP_ERR_NUMERIC, "Preconditioner is not positive definite");
      if (history) ws->aresiduals.push_back(s.ArNorm);
      K(ws->loop.upload(ctx, s));
      slot = take_slots(ctx, 1);
      K(launch_p3(ctx, n, ws->loop.dev, w, B.x, slot));
      double xx;
      K(fetch_results(ctx, slot, 1, &xx));
      if (k >= 2) std::swap(B.w1, B.w2);
      stop = minres_step_c(s, std::sqrt(xx), k, ws->err_vec.data());
      if (history) { ws->box.residuals.push_back(s.rNorm); ws->aconds.push_back(s.Acond); }
      if (kdisplay(k, verbose)) verbose_row(o, k, s, t0, false);
      if (s.lsq_exit) break;
      tired = k >= itmax;
      host_exit(ws, o, t0, timemax, &user_exit, &overtimed);
      stop = stop || user_exit || overtimed;
    }
  } else if (!stop) {
    // ---------------------------------------------------------------- device-resident loop -----------------------------
    for (int i = 0; i < ws->window; ++i) s.err_vec[i] = 0.0;
    auto step = [&](MinresDevState *dev, long long j) {
      const int64_t k = j + 1;
      KHIP_TRY(dev_stage(ctx, dev, 4 * j + 1, EPI_MINRES_A, 1, [&](int slot) {
        return lanczos_product(ctx, A, fuse, n, dev, B.v, B.r1, B.y, k >= 2, slot); }));   // y = A v + P1 ; v.y -> alpha, delta
      KHIP_TRY(dev_stage(ctx, dev, 4 * j + 2, EPI_MINRES_B, 1, [&](int slot) {
        return launch_p2(ctx, n, dev, B.r2, B.v, B.y, B.w1, B.w2, (int)std::min<int64_t>(k, 3), true, slot); }));   // P2 ; y.y -> rotation
      double *w = k == 1 ? B.w2 : B.w1;
      double *old_r1 = B.r1;
      B.r1 = B.r2; B.r2 = B.y; B.y = old_r1; B.v = B.r2;
      KHIP_TRY(dev_stage(ctx, dev, 4 * j + 3, EPI_MINRES_C, 1, [&](int slot) {
        return launch_p3(ctx, n, dev, w, B.x, slot); }));                                // P3 ; x.x -> tests
      if (k >= 2) std::swap(B.w1, B.w2);
      return (int)KHIP_OK;
    };
    K(ws->loop.run(ctx, s, device_loop_args(itmax, t0, timemax, history, {&ws->box.residuals, &ws->aresiduals, &ws->aconds}), step,
                   &s, &overtimed));
    iter = s.iter;
    tired = iter >= itmax;
  }
  if (verbose > 0) klogf(o.log_fd, "\n");
  if (s.lsq_exit)                                                                                         // :410-419
    return ws_end(ws, {1, 1, 1, "x is a minimum least-squares solution", warm_start, t0, false});
  const char *status = "unknown";
  if (tired) status = "maximum number of iterations exceeded";
  if (s.ill_cond_mach) status = "condition number seems too large for this machine";
  if (s.ill_cond_lim) status = "condition number exceeds tolerance";
  if (s.solved) status = "found approximate minimum least-squares solution";
  if (s.zero_resid) status = "found approximate zero-residual solution";
  if (s.fwd_err) status = "truncated forward error small enough";
  if (user_exit) status = "user-requested exit";
  if (overtimed) status = "time limit exceeded";
  return ws_end(ws, {iter, s.solved, !s.zero_resid, status, warm_start, t0, false});
}

}  // extern "C"
