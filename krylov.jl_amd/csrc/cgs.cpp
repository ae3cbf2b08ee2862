// cgs.cpp -- cgs! (src/cgs.jl:126-281) above the device primitives, with its fused gfx950 kernels.
//
// Real Float64.  Three loops, chosen as for bicgstab! (khip_cgs_last_path):
//   0  options.fused = 0: the reference's primitive sequence, one launch per k* call, one host sync per kdot / knorm;
//   1  the host-driven loop on the fused kernels (with M or N, a user operator, a callback or verbose > 0);
//   2  the device-resident loop (default; A a CSR handle, M = N = I): the two scalars and the stopping tests run as the epilogues
//      of the two reductions of an iteration (cgs_step_a/b, solver_device.hpp), iterations are enqueued ahead.
// With M = N = I the reference aliases t = s = v = w = ts, y = p and z = u.  One iteration on the fused paths:
//   ts = A p ; σ = c.ts                        the fused SpMV (spmv.hip)                                           -> α = ρ / σ
//   P1   q = fma(-α, ts, u) ; u = fma(1, q, u) ; x = fma(α, u, x)                                   (:222-226)     48n bytes
//   ts = A u
//   P2   r = fma(-α, ts, r) ; c.r ; r.r                                                             (:229-230, :244)  32n bytes
//   P3   u = fma(β, q, r) ; p_aux = fma(1, q, β p) ; p = fma(1, u, β p_aux)                         (:232-235)     40n bytes
// against 240n for the primitive sequence (11 BLAS-1 calls).  Every elementwise value uses the expression of the primitive it
// replaces (fma(a, x, y) for kaxpy!, fma(a, x, b y) for kaxpby!, with a = 1 and b = β as they stand; kcopy! + kaxpy! is one fma):
// the fused loops agree with the primitive sequence bit for bit on elementwise values and to the reductions' one ulp otherwise;
// loops 1 and 2 run the same kernels and the same scalar code and produce the same bits.
// The reference updates u and p BEFORE its tests (:232-235 against :249-256): P3 of the last iteration still runs.
#include "solver_host.hpp"
#include "vec_launch.hpp"

using namespace khip;

namespace khip {   // (named, not anonymous: stable kernel names in traces)

// ---------------------------------------------------------------------------------------------------------- kernels ----
// Each thread owns one VEC-vector of every stream; the odd tail element (VEC = 2, n odd) goes to thread 0 of block 0.
// Cache hints, the rule of qmr.cpp: a load is non-temporal when it is the LAST read of that data before it is overwritten; a store
// is non-temporal when nothing reads it before the next iteration's passes.  P1 and P3 reduce nothing: they have no COMP.

// P1: q = fma(-α, v, u) ; u = fma(1, q, u) ; update_x ? x = fma(α, u, x)                 (:222-226)
//   u    load  NT: overwritten here.            store cacheable: the product that follows reads it.
//   v    load  NT: ts (or vw under M) is overwritten by that product (by M's solve after it).
//   x    load  NT: overwritten here.            store NT: next read by the next iteration's P1.
//   q    (not read)                             store cacheable: P3 of this iteration reads it.
template <int VEC, bool NT>
__global__ __launch_bounds__(kBlock) void cgs_p1_kernel(int64_t n, const CgsDevState *st, const long long *stop_seq, long long seq,
                                                       const double *v, double *u, double *q, double *x, int update_x) {
  using T = typename VecT<VEC>::type;
  if (seq_skip(stop_seq, seq)) return;
  const double a = st->alpha, na = -a;
  const int64_t nvec = n / VEC;
  const int64_t i = lane_index();
  if (i < nvec) {
    const T uv = ldg<NT>(reinterpret_cast<const T *>(u) + i);
    const T vv = ldg<NT>(reinterpret_cast<const T *>(v) + i);
    T xv = {};
    if (update_x) xv = ldg<NT>(reinterpret_cast<const T *>(x) + i);
    T qo, uo, xo;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const double qn = fma(na, vget(vv, e), vget(uv, e));          // kcopy!(q, u) ; kaxpy!(-α, v, q)
      const double un = fma(1.0, qn, vget(uv, e));                  // kaxpy!(1, q, u)
      vset(qo, e, qn);
      vset(uo, e, un);
      vset(xo, e, fma(a, un, vget(xv, e)));                         // kaxpy!(α, u, x)
    }
    stg<false>(qo, reinterpret_cast<T *>(q) + i);
    stg<false>(uo, reinterpret_cast<T *>(u) + i);
    if (update_x) stg<NT>(xo, reinterpret_cast<T *>(x) + i);
  }
  if (VEC == 2 && owns_tail(n)) {
    const int64_t t = n - 1;
    const double ut = u[t];
    const double qn = fma(na, v[t], ut);
    const double un = fma(1.0, qn, ut);
    q[t] = qn;
    u[t] = un;
    if (update_x) x[t] = fma(a, un, x[t]);
  }
}

// P2: r = fma(-α, w, r) ; acc = (c . r, r . r)                                          (:229-230, :244)
//   r    load  NT: overwritten here.            store cacheable: P3 reads it next.
//   w    load  NT: ts (or vw) is next overwritten by the next iteration's first product.
//   c    load  cacheable: read by every iteration, never overwritten.
template <int VEC, bool NT, bool COMP>
__global__ __launch_bounds__(kBlock) void cgs_p2_kernel(int64_t n, const CgsDevState *st, const double *w, const double *c, double *r,
                                                       RedArgs ra) {
  using T = typename VecT<VEC>::type;
  if (seq_skip(ra.stop_seq, ra.seq)) return;
  const double na = -st->alpha;
  dd acc[2] = {dd{0.0, 0.0}, dd{0.0, 0.0}};
  const int64_t nvec = n / VEC;
  const int64_t i = lane_index();
  if (i < nvec) {
    const T rv = ldg<NT>(reinterpret_cast<const T *>(r) + i);
    const T wv = ldg<NT>(reinterpret_cast<const T *>(w) + i);
    const T cv = ldg<false>(reinterpret_cast<const T *>(c) + i);
    T ro;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const double rn = fma(na, vget(wv, e), vget(rv, e));          // kaxpy!(-α, w, r)
      vset(ro, e, rn);
      acc_prod<COMP>(acc[0], vget(cv, e), rn);
      acc_prod<COMP>(acc[1], rn, rn);
    }
    stg<false>(ro, reinterpret_cast<T *>(r) + i);
  }
  if (VEC == 2 && owns_tail(n)) {
    const int64_t t = n - 1;
    const double rn = fma(na, w[t], r[t]);
    r[t] = rn;
    acc_prod<COMP>(acc[0], c[t], rn);
    acc_prod<COMP>(acc[1], rn, rn);
  }
  wave_publish<2>(acc, ra);
}

// P3: u = fma(β, q, r) ; p_aux = fma(1, q, β p) ; p = fma(1, u, β p_aux)                 (:232-235)
//   r    load  cacheable: the next iteration's P2 reads it again before it overwrites it.
//   q    load  NT: the next P1 overwrites it without reading.
//   p    load  NT: overwritten here.            store cacheable: the product that follows reads it.
//   u    (not read)                             store NT: next read by the next iteration's P1, a whole product later.
template <int VEC, bool NT>
__global__ __launch_bounds__(kBlock) void cgs_p3_kernel(int64_t n, const CgsDevState *st, const long long *stop_seq, long long seq,
                                                       const double *r, const double *q, double *u, double *p) {
  using T = typename VecT<VEC>::type;
  if (seq_skip(stop_seq, seq)) return;
  const double b = st->beta;
  const int64_t nvec = n / VEC;
  const int64_t i = lane_index();
  if (i < nvec) {
    const T rv = ldg<false>(reinterpret_cast<const T *>(r) + i);
    const T qv = ldg<NT>(reinterpret_cast<const T *>(q) + i);
    const T pv = ldg<NT>(reinterpret_cast<const T *>(p) + i);
    T uo, po;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const double un = fma(b, vget(qv, e), vget(rv, e));           // kcopy!(u, r) ; kaxpy!(β, q, u)
      const double pa = fma(1.0, vget(qv, e), b * vget(pv, e));     // kaxpby!(1, q, β, p)
      vset(uo, e, un);
      vset(po, e, fma(1.0, un, b * pa));                            // kaxpby!(1, u, β, p)
    }
    stg<NT>(uo, reinterpret_cast<T *>(u) + i);
    stg<false>(po, reinterpret_cast<T *>(p) + i);
  }
  if (VEC == 2 && owns_tail(n)) {
    const int64_t t = n - 1;
    const double qt = q[t];
    const double un = fma(b, qt, r[t]);
    const double pa = fma(1.0, qt, b * p[t]);
    u[t] = un;
    p[t] = fma(1.0, un, b * pa);
  }
}

}  // namespace khip

namespace {

constexpr ScalarPathNT kScalarNT = ScalarPathNT::never;

// P1 and P3 take their sequence number from ctx->ctl, as the reductions do (all zero on the host-driven loop)
int launch_p1(khip_ctx *ctx, int64_t n, const CgsDevState *st, const double *v, double *u, double *q, double *x, bool update_x) {
  VecPlan L;
  KHIP_TRY(vec_plan(ctx, n, {v, u, q, x}, &L));
  const SeqCtl ctl = ctx->ctl;
  vec_dispatch_vn<kScalarNT>(L, [&](auto V, auto N) {
    hipLaunchKernelGGL((cgs_p1_kernel<V, N>), L.grid(), dim3(kBlock), 0, ctx->stream, n, st, ctl.stop_seq, ctl.seq, v, u, q, x,
                       update_x ? 1 : 0); });
  KHIP_CHECK_HIP(hipGetLastError());
  return KHIP_OK;
}

int launch_p2(khip_ctx *ctx, int64_t n, const CgsDevState *st, const double *w, const double *c, double *r, int slot) {
  VecPlan L;
  KHIP_TRY(vec_plan(ctx, n, {w, c, r}, &L, 2));
  RedArgs ra = make_red_args(ctx, slot);
  vec_dispatch<kScalarNT>(L, [&](auto V, auto N, auto C) {
    hipLaunchKernelGGL((cgs_p2_kernel<V, N, C>), L.grid(), dim3(kBlock), 0, ctx->stream, n, st, w, c, r, ra); });
  KHIP_CHECK_HIP(hipGetLastError());
  return launch_finish(ctx, L.waves(), 2, slot);
}

int launch_p3(khip_ctx *ctx, int64_t n, const CgsDevState *st, const double *r, const double *q, double *u, double *p) {
  VecPlan L;
  KHIP_TRY(vec_plan(ctx, n, {r, q, u, p}, &L));
  const SeqCtl ctl = ctx->ctl;
  vec_dispatch_vn<kScalarNT>(L, [&](auto V, auto N) {
    hipLaunchKernelGGL((cgs_p3_kernel<V, N>), L.grid(), dim3(kBlock), 0, ctx->stream, n, st, ctl.stop_seq, ctl.seq, r, q, u, p); });
  KHIP_CHECK_HIP(hipGetLastError());
  return KHIP_OK;
}

}  // namespace

struct khip_cgs_workspace {
  khip_ctx *ctx;
  int64_t m, n;
  double *x = nullptr, *r = nullptr, *u = nullptr, *p = nullptr, *q = nullptr, *ts = nullptr, *dx = nullptr, *yz = nullptr,
         *vw = nullptr;
  Borrowed borrowed;                        // the caller's vectors (khip_cgs_workspace_adopt*): never freed here
  bool warm_start = false;
  StatsBox box;
  DeviceLoop<CgsDevState, 3> loop;          // fused loops: device copy of the scalar state, pinned snapshots + staging, history
};

namespace {

// x, r, u, p, q, ts come with the workspace; Δx, yz, vw stay empty until needed (src/krylov_workspaces.jl, CgsWorkspace)
using W = khip_cgs_workspace;
constexpr WsVec<W> kVectors[] = {{"x", &W::x, Core},   {"r", &W::r, Core},   {"u", &W::u, Core},   {"p", &W::p, Core}, {"q", &W::q, Core},
                                 {"ts", &W::ts, Core}, {"dx", &W::dx, Lazy}, {"yz", &W::yz, Lazy}, {"vw", &W::vw, Lazy}};

void verbose_row(const khip_options &o, long long iter, double rNorm, double t0) {                        // :201, :259
  klogf(o.log_fd, "%5lld  %7.1e  %.2fs\n", iter, rNorm, now_s() - t0);
}

// The loop of :215-260 with M = N = I on a CSR handle and ρ, α, β and the tests on the device: five launches per iteration, each
// carrying its sequence number.  P3 is the last: a stop found by P2's epilogue leaves it running (stop_seq = its number + 1).
int cgs_device_loop(W *ws, const khip_csr *A, const double *c, const CgsDevState &h, const DeviceLoopArgs &a, CgsDevState *out,
                    bool *overtimed) {
  khip_ctx *ctx = ws->ctx;
  const int64_t n = ws->n;
  double *x = ws->x, *r = ws->r, *u = ws->u, *p = ws->p, *q = ws->q, *ts = ws->ts;
  auto step = [&](CgsDevState *dev, long long j) {
    const long long *stop = &dev->stop_seq;
    KHIP_TRY(dev_stage(ctx, dev, 5 * j, EPI_CGS_A, 1, [&](int slot) { return spmv_any(ctx, A, p, ts, slot, c, 0); }));   // :218-221  ts = A p ; c.ts -> α
    KHIP_TRY(dev_pass(ctx, stop, 5 * j + 1, EPI_NONE, nullptr, [&] { return launch_p1(ctx, n, dev, ts, u, q, x, true); }));   // :222-226
    KHIP_TRY(dev_pass(ctx, stop, 5 * j + 2, EPI_NONE, nullptr, [&] { return spmv_any(ctx, A, u, ts, -1); }));   // :227      ts = A u
    KHIP_TRY(dev_stage(ctx, dev, 5 * j + 3, EPI_CGS_B, 2, [&](int slot) { return launch_p2(ctx, n, dev, ts, c, r, slot); }));   // :229-230, :244 -> β, ρ, the tests
    return dev_pass(ctx, stop, 5 * j + 4, EPI_NONE, nullptr, [&] { return launch_p3(ctx, n, dev, r, q, u, p); });   // :232-235
  };
  return ws->loop.run(ctx, h, a, step, out, overtimed);
}

}  // namespace

extern "C" {

int khip_cgs_workspace_create(khip_ctx *ctx, int64_t m, int64_t n, khip_cgs_workspace **out) {
  KHIP_REQUIRE(ctx && out && m >= 0 && n >= 0, "cgs_workspace_create: bad argument");
  khip_cgs_workspace *ws = new khip_cgs_workspace();
  ws->ctx = ctx; ws->m = m; ws->n = n;
  const int rc = ws_create_core(ws, kVectors);
  if (rc) { khip_cgs_workspace_destroy(ws); return rc; }
  *out = ws;
  return KHIP_OK;
}

int khip_cgs_workspace_adopt(khip_ctx *ctx, int64_t m, int64_t n, double *x, double *r, double *u, double *p, double *q, double *ts,
                             khip_cgs_workspace **out) {
  KHIP_REQUIRE(ctx && out && m >= 0 && n >= 0, "cgs_workspace_adopt: bad argument");
  khip_cgs_workspace *ws = new khip_cgs_workspace();
  ws->ctx = ctx; ws->m = m; ws->n = n;
  const int rc = ws_adopt_core(ws, kVectors, "cgs_workspace_adopt", {x, r, u, p, q, ts});
  if (rc) { delete ws; return rc; }
  *out = ws;
  return KHIP_OK;
}

int khip_cgs_workspace_adopt_vector(khip_cgs_workspace *ws, const char *name, double *ptr) {
  return ws_adopt_vector(ws, kVectors, "cgs_workspace_adopt_vector", name, ptr);
}

int khip_cgs_workspace_destroy(khip_cgs_workspace *ws) {
  if (!ws) return KHIP_OK;
  ws_free_vectors(ws, kVectors);
  ws->loop.release();
  delete ws;
  return KHIP_OK;
}

int khip_cgs_warm_start(khip_cgs_workspace *ws, const double *x0) { return ws_warm_start(ws, kVectors, x0, "cgs_warm_start"); }
double *khip_cgs_solution(khip_cgs_workspace *ws) { return ws ? ws->x : nullptr; }
const khip_stats *khip_cgs_stats(khip_cgs_workspace *ws) { return ws ? &ws->box.st : nullptr; }
int khip_cgs_last_path(khip_cgs_workspace *ws) { return ws ? ws->box.path : -1; }
double *khip_cgs_vector(khip_cgs_workspace *ws, const char *name) { return ws_vector(ws, kVectors, name); }
size_t khip_cgs_workspace_bytes(khip_cgs_workspace *ws) { return ws_bytes(ws, kVectors); }

int khip_cgs_solve(khip_cgs_workspace *ws, const khip_operator *A, const khip_operator *M, const khip_operator *N, const double *b,
                   const double *c, const khip_options *opts_in) {
  KHIP_REQUIRE(ws && A && b, "cgs_solve: null argument");
  khip_ctx *ctx = ws->ctx;
  const khip_options o = opts_in ? *opts_in : khip_default_options();
  const double t0 = now_s();
  const double timemax = timemax_of(o);
  const int64_t n = ws->n;
  const double atol = tol_or_default(o.atol), rtol = tol_or_default(o.rtol);
  const bool history = o.history != 0;
  (void)take_alloc_seconds();

  if (int rc = check_shape(ws, {A})) return rc;                                                            // :132-134
  if (ws->m != ws->n) return ws->box.fail(KHIP_ERR_INVALID, "System must be square");
  if (o.variant != 0) return ws->box.fail(KHIP_ERR_INVALID, "cgs: options.variant must be 0 (there is no other recurrence)");
  if (o.verbose > 0) klogf(o.log_fd, "CGS: system of size %lld\n", (long long)n);                         // :136
  if (!c) c = b;                                                                                           // :106

  const bool MisI = (M == nullptr), NisI = (N == nullptr);
  if (!MisI && !ws->vw) K(alloc_vec(ctx, n, &ws->vw));                                                     // :148-149
  if (!NisI && !ws->yz) K(alloc_vec(ctx, n, &ws->yz));
  double *x = ws->x, *r = ws->r, *u = ws->u, *p = ws->p, *q = ws->q, *ts = ws->ts;
  const bool warm_start = ws->warm_start;
  ws->box.reset();
  double *v = MisI ? ts : ws->vw;                                                                          // t = s = ts; v = w (:154-159)
  double *y = NisI ? p : ws->yz;
  double *z = NisI ? u : ws->yz;
  double *r0 = MisI ? r : ts;

  // set-up, the same primitives on every path (:161-213)
  K(residual0(ws, A, 0.0, b, warm_start, r0));
  K(khip_fill(ctx, n, x, 0.0));
  if (!MisI) K(apply_op(ctx, M, r0, r));
  CgsDevState s;
  memset(&s, 0, sizeof(s));
  K(khip_nrm2(ctx, n, r, &s.rNorm));
  if (history) ws->box.push(s.rNorm);
  ws->box.path = o.fused ? 1 : 0;
  if (s.rNorm == 0) return ws_end(ws, {0, 1, 0, "x is a zero-residual solution", warm_start, t0, true});
  K(khip_dot(ctx, n, c, r, &s.rho));
  if (s.rho == 0) return ws_end(ws, {0, 0, 0, "Breakdown b\xe1\xb4\xb4" "c = 0", warm_start, t0, true});

  int64_t iter = 0;
  const int64_t itmax = o.itmax == 0 ? 2 * global_rows(ctx, A, n) : o.itmax;      // 2n of the GLOBAL system on every rank
  s.eps_tol = atol + rtol * s.rNorm;
  if (o.verbose > 0) klogf(o.log_fd, "    k     \xe2\x80\x96r\xe2\x82\x96\xe2\x80\x96  timer\n");          // :200  k  ‖rₖ‖  timer
  if (kdisplay(iter, o.verbose)) verbose_row(o, iter, s.rNorm, t0);

  K(khip_copy(ctx, n, u, r));
  K(khip_copy(ctx, n, p, r));
  K(khip_fill(ctx, n, q, 0.0));

  s.stop_seq = kSeqNever;
  s.solved = (s.rNorm <= s.eps_tol) ? 1 : 0;
  bool tired = iter >= itmax, user_exit = false, overtimed = false;
  auto running = [&] { return !(s.solved || tired || s.breakdown || user_exit || overtimed); };
  // the end of an iteration on the host-driven loops (:244-259)
  auto host_tail = [&](int64_t k) {
    if (history) ws->box.push(s.rNorm);
    tired = k >= itmax;
    host_exit(ws, o, t0, timemax, &user_exit, &overtimed);
    if (kdisplay(k, o.verbose)) verbose_row(o, k, s.rNorm, t0);
  };

  const bool fastA = A->csr && !A->apply;
  const bool device_loop = o.fused >= 2 && fastA && MisI && NisI && !o.callback && o.verbose <= 0;
  ws->box.path = (device_loop && running()) ? 2 : (o.fused ? 1 : 0);   // a loop that never starts reports 1, as the early returns do
  if (ws->box.path == 0) {
    // -------------------------------------------------------------- the reference's primitive sequence ------------------
    while (running()) {
      const int64_t k = ++iter;
      if (!NisI) K(apply_op(ctx, N, p, y));                                                               // :217
      K(apply_op(ctx, A, y, ts));                                                                         // :218
      if (!MisI) K(apply_op(ctx, M, ts, v));                                                              // :219
      double sigma;
      K(khip_dot(ctx, n, c, v, &sigma));                                                                  // :220
      cgs_step_a(s, sigma);                                                                               // :221
      K(khip_copy(ctx, n, q, u));                                                                         // :222
      K(khip_axpy(ctx, n, -s.alpha, v, q));                                                               // :223
      K(khip_axpy(ctx, n, 1.0, q, u));                                                                    // :224
      if (!NisI) K(apply_op(ctx, N, u, z));                                                               // :225
      K(khip_axpy(ctx, n, s.alpha, z, x));                                                                // :226
      K(apply_op(ctx, A, z, ts));                                                                         // :227
      if (!MisI) K(apply_op(ctx, M, ts, v));                                                              // :228
      K(khip_axpy(ctx, n, -s.alpha, v, r));                                                               // :229
      double rho_next;
      K(khip_dot(ctx, n, c, r, &rho_next));                                                               // :230
      const double beta = rho_next / s.rho;                                                               // :231
      K(khip_copy(ctx, n, u, r));                                                                         // :232
      K(khip_axpy(ctx, n, beta, q, u));                                                                   // :233
      K(khip_axpby(ctx, n, 1.0, q, beta, p));                                                             // :234
      K(khip_axpby(ctx, n, 1.0, u, beta, p));                                                             // :235
      K(khip_nrm2(ctx, n, r, &s.rNorm));                                                                  // :244
      s.beta = beta;
      s.rho = rho_next;                                                                                   // :238
      s.solved = (s.rNorm <= s.eps_tol || s.rNorm + 1.0 <= 1.0) ? 1 : 0;                                  // :249-254
      s.breakdown = (s.alpha == 0 || std::isnan(s.alpha)) ? 1 : 0;                                        // :256
      s.iter = k;
      host_tail(k);
    }
  } else if (ws->box.path == 1) {
    // -------------------------------------------------------------- host-driven loop on the fused kernels ---------------
    K(ws->loop.alloc());
    const CgsDevState *dev = ws->loop.dev;
    while (running()) {
      const int64_t k = ++iter;
      double sigma;
      if (!NisI) K(apply_op(ctx, N, p, y));                                                               // :217
      if (fastA && MisI) {
        const int slot = take_slots(ctx, 1);
        K(spmv_any(ctx, A->csr, y, ts, slot, c, 0));                                                      // :218-220  ts = A y ; c.ts
        K(fetch_results(ctx, slot, 1, &sigma));
      } else {
        K(apply_op(ctx, A, y, ts));
        if (!MisI) K(apply_op(ctx, M, ts, v));                                                            // :219
        K(khip_dot(ctx, n, c, v, &sigma));
      }
      cgs_step_a(s, sigma);                                                                               // :221
      K(ws->loop.upload(ctx, s));
      K(launch_p1(ctx, n, dev, v, u, q, x, NisI));                                                        // :222-226
      if (!NisI) {
        K(apply_op(ctx, N, u, z));                                                                        // :225
        K(khip_axpy(ctx, n, s.alpha, z, x));                                                              // :226
      }
      K(apply_op(ctx, A, z, ts));                                                                         // :227
      if (!MisI) K(apply_op(ctx, M, ts, v));                                                              // :228
      const int slot = take_slots(ctx, 2);
      K(launch_p2(ctx, n, dev, v, c, r, slot));                                                           // :229-230, :244
      double two[2];
      K(fetch_results(ctx, slot, 2, two));
      cgs_step_b(s, two[0], two[1], k);
      K(ws->loop.upload(ctx, s));
      K(launch_p3(ctx, n, dev, r, q, u, p));                                                              // :232-235
      host_tail(k);
    }
  } else {
    // -------------------------------------------------------------- device-resident loop ------------------------------
    K(cgs_device_loop(ws, A->csr, c, s, device_loop_args(itmax, t0, timemax, history, {&ws->box.residuals}), &s, &overtimed));
    iter = s.iter;
    tired = iter >= itmax;
  }
  if (o.verbose > 0) { klogf(o.log_fd, "\n"); klog_flush(o.log_fd); }                                      // :261

  const char *status = "unknown";                                                                         // :264-268
  if (tired) status = "maximum number of iterations exceeded";
  if (s.breakdown) status = "breakdown \xce\xb1\xe2\x82\x96 == 0";
  if (s.solved) status = "solution good enough given atol and rtol";
  if (user_exit) status = "user-requested exit";
  if (overtimed) status = "time limit exceeded";
  return ws_end(ws, {iter, s.solved ? 1 : 0, 0, status, warm_start, t0, true});                         // :271-280
}

}  // extern "C"
