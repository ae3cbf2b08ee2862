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
#include <chrono>
#include <utility>

#include "bilanczos_passes.hpp"   // P1, P2 and their launchers, shared with qmr.cpp

using namespace khip;

namespace khip {   // (named, not anonymous: stable kernel names in traces)

// ---------------------------------------------------------------------------------------------------------- kernels ----
// (P1 and P2: bilanczos_passes.hpp.)
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

void verbose_row(const khip_options &o, long long iter, double alpha, double rNorm, double t0) {     // src/bilq.jl:201, :374
  klogf(o.log_fd, "%5lld  %8.1e  %7.1e  %.2fs\n", iter, alpha, rNorm, now_s() - t0);
}

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
  (void)take_alloc_seconds();
  // uₖ₋₁, uₖ, q, vₖ₋₁, vₖ, p, x, d̅ allocated; Δx, t, s stay empty until needed (src/krylov_workspaces.jl, BilqWorkspace)
  int rc = KHIP_OK;
  for (double **slot : {&ws->u_prev, &ws->u, &ws->q, &ws->v_prev, &ws->v, &ws->p, &ws->x, &ws->dbar})
    if (!rc) rc = alloc_vec(ctx, n, slot);
  if (rc) { khip_bilq_workspace_destroy(ws); return rc; }
  ws->box.st.allocation_timer = take_alloc_seconds();
  *out = ws;
  return KHIP_OK;
}

int khip_bilq_workspace_adopt(khip_ctx *ctx, int64_t m, int64_t n, double *u_prev, double *u, double *q, double *v_prev, double *v,
                              double *p, double *x, double *dbar, khip_bilq_workspace **out) {
  KHIP_REQUIRE(ctx && out && m >= 0 && n >= 0, "bilq_workspace_adopt: bad argument");
  KHIP_REQUIRE(m == n, "System must be square");
  KHIP_REQUIRE(n == 0 || (u_prev && u && q && v_prev && v && p && x && dbar),
               "bilq_workspace_adopt: u_prev, u, q, v_prev, v, p, x, dbar must be device vectors of n entries");
  const double *all[8] = {u_prev, u, q, v_prev, v, p, x, dbar};
  for (int i = 0; i < 8; ++i)
    for (int j = i + 1; j < 8; ++j)
      KHIP_REQUIRE(n == 0 || all[i] != all[j], "bilq_workspace_adopt: u_prev, u, q, v_prev, v, p, x, dbar must be distinct");
  khip_bilq_workspace *ws = new khip_bilq_workspace();
  ws->ctx = ctx; ws->m = m; ws->n = n;
  ws->u_prev = u_prev; ws->u = u; ws->q = q; ws->v_prev = v_prev; ws->v = v; ws->p = p; ws->x = x; ws->dbar = dbar;
  for (const double *ptr : all) ws->borrowed.add(ptr);
  *out = ws;
  return KHIP_OK;
}

int khip_bilq_workspace_adopt_vector(khip_bilq_workspace *ws, const char *name, double *ptr) {
  KHIP_REQUIRE(ws && name, "bilq_workspace_adopt_vector: null argument");
  using S = NamedSlot;
  return adopt_named(ws->ctx, ws->borrowed, {{"u_prev", &ws->u_prev, S::Fixed}, {"u", &ws->u, S::Fixed}, {"q", &ws->q, S::Fixed},
                     {"v_prev", &ws->v_prev, S::Fixed}, {"v", &ws->v, S::Fixed}, {"p", &ws->p, S::Fixed}, {"x", &ws->x, S::Fixed},
                     {"dbar", &ws->dbar, S::Fixed}, {"dx", &ws->dx, S::Optional}, {"t", &ws->t, S::Optional},
                     {"s", &ws->s, S::Optional}},
                     "bilq_workspace_adopt_vector", "vector", name, ptr);
}

int khip_bilq_workspace_destroy(khip_bilq_workspace *ws) {
  if (!ws) return KHIP_OK;
  for (double *ptr : {ws->u_prev, ws->u, ws->q, ws->v_prev, ws->v, ws->p, ws->x, ws->dbar, ws->dx, ws->t, ws->s})
    free_unless_borrowed(ws->ctx, ws->borrowed, ptr);
  ws->loop.release();
  delete ws;
  return KHIP_OK;
}

int khip_bilq_warm_start(khip_bilq_workspace *ws, const double *x0) {
  KHIP_REQUIRE(ws && x0, "bilq_warm_start: null argument");
  if (!ws->dx) KHIP_TRY(alloc_vec(ws->ctx, ws->n, &ws->dx));
  if (x0 != ws->dx) KHIP_TRY(khip_copy(ws->ctx, ws->n, ws->dx, x0));
  ws->warm_start = true;
  return KHIP_OK;
}

double *khip_bilq_solution(khip_bilq_workspace *ws) { return ws ? ws->x : nullptr; }
const khip_stats *khip_bilq_stats(khip_bilq_workspace *ws) { return ws ? &ws->box.st : nullptr; }
int khip_bilq_last_path(khip_bilq_workspace *ws) { return ws ? ws->box.path : -1; }
double *khip_bilq_vector(khip_bilq_workspace *ws, const char *name) {
  if (!ws || !name) return nullptr;
  struct { const char *k; double *p; } tab[] = {{"u_prev", ws->u_prev}, {"u", ws->u}, {"q", ws->q}, {"v_prev", ws->v_prev},
                                                {"v", ws->v}, {"p", ws->p}, {"x", ws->x}, {"dbar", ws->dbar}, {"dx", ws->dx},
                                                {"t", ws->t}, {"s", ws->s}};
  for (auto &e : tab) if (strcmp(e.k, name) == 0) return e.p;
  return nullptr;
}
size_t khip_bilq_workspace_bytes(khip_bilq_workspace *ws) {
  if (!ws) return 0;
  size_t cnt = 0;
  for (double *ptr : {ws->u_prev, ws->u, ws->q, ws->v_prev, ws->v, ws->p, ws->x, ws->dbar, ws->dx, ws->t, ws->s}) cnt += ptr ? 1 : 0;
  return cnt * sizeof(double) * (size_t)ws->n;
}

int khip_bilq_solve(khip_bilq_workspace *ws, const khip_operator *A, const khip_operator *At, const khip_operator *M,
                    const khip_operator *N, const double *b, const double *c, const khip_options *opts_in,
                    const khip_bilq_params *params_in) {
  KHIP_REQUIRE(ws && A && b, "bilq_solve: null argument");
  khip_ctx *ctx = ws->ctx;
  const khip_options o = opts_in ? *opts_in : khip_default_options();
  const khip_bilq_params prm = params_in ? *params_in : khip_bilq_default_params();
  const double t0 = now_s();
  const double timemax = timemax_of(o);
  const int64_t n = ws->n;
  khip_stats *st = &ws->box.st;
  const double atol = tol_or_default(o.atol), rtol = tol_or_default(o.rtol);
  const int verbose = o.verbose;
  const bool history = o.history != 0;
  (void)take_alloc_seconds();

  if (!At) return ws->box.fail(KHIP_ERR_INVALID, "bilq_solve: At (the adjoint of A) is required");
  for (const khip_operator *op : {A, At}) {                                                              // :124-126
    if (!(op->csr && !op->apply)) continue;
    int64_t am, an;
    khip_csr_shape(op->csr, &am, &an, nullptr);
    if (am != ws->m || (an != ws->n && !op->csr->dist)) {             // a row-partitioned handle counts global columns
      char msg[160];
      snprintf(msg, sizeof(msg), "(workspace.m, workspace.n) = (%lld, %lld) is inconsistent with size(A) = (%lld, %lld)",
               (long long)ws->m, (long long)ws->n, (long long)am, (long long)an);
      return ws->box.fail(KHIP_ERR_INVALID, msg);
    }
  }
  if (ws->m != ws->n) return ws->box.fail(KHIP_ERR_INVALID, "System must be square");
  if (verbose > 0) klogf(o.log_fd, "BILQ: system of size %lld\n", (long long)n);                         // :128
  const bool MisI = (M == nullptr), NisI = (N == nullptr);
  const khip_operator *Mt = prm.Mt ? prm.Mt : M, *Nt = prm.Nt ? prm.Nt : N;
  if (!MisI && !ws->t) K(alloc_vec(ctx, n, &ws->t));                                                     // :145-146
  if (!NisI && !ws->s) K(alloc_vec(ctx, n, &ws->s));
  if (!c) c = b;
  const bool warm_start = ws->warm_start;
  ws->box.reset();
  double *x = ws->x, *dbar = ws->dbar, *q = ws->q, *p = ws->p;
  double *v = ws->v, *v_prev = ws->v_prev, *u = ws->u, *u_prev = ws->u_prev;
  auto finish = [&](void) {
    st->timer = now_s() - t0;
    ws->warm_start = false;
    st->allocation_timer += take_alloc_seconds();
    ws->box.publish();
  };

  // set-up, the same primitives on every path (:158-215)
  const double *r0 = b;
  if (warm_start) {
    K(apply_op(ctx, A, ws->dx, q));
    K(khip_axpby(ctx, n, 1.0, b, -1.0, q));
    r0 = q;
  }
  if (!MisI) {
    K(apply_op(ctx, M, r0, ws->t));
    r0 = ws->t;
  }
  K(khip_fill(ctx, n, x, 0.0));
  double bNorm;
  K(khip_nrm2(ctx, n, r0, &bNorm));
  if (history) ws->box.push(bNorm);
  ws->box.path = o.fused ? 1 : 0;
  auto early = [&](int solved, const char *status) {
    st->niter = 0; st->solved = solved; st->inconsistent = 0;
    snprintf(st->status, sizeof(st->status), "%s", status);
    if (warm_start) K(khip_axpy(ctx, n, 1.0, ws->dx, x));
    finish();
    return (int)KHIP_OK;
  };
  if (bNorm == 0) return early(1, "x is a zero-residual solution");                                      // :172-181
  const int64_t itmax = o.itmax == 0 ? 2 * global_rows(ctx, A, n) : o.itmax;
  double cb;
  K(khip_dot(ctx, n, c, r0, &cb));
  if (cb == 0) return early(0, "Breakdown b\xe1\xb4\xb4" "c = 0");                                       // :188-197
  BilqDevState s;
  memset(&s, 0, sizeof(s));
  s.bNorm = bNorm;
  s.eps_tol = atol + rtol * bNorm;
  if (verbose > 0) {
    klogf(o.log_fd, "%5s        %s     %s  %5s\n", "k", "\xce\xb1\xe2\x82\x96", "\xe2\x80\x96r\xe2\x82\x96\xe2\x80\x96", "timer");
    if (kdisplay(0, verbose)) verbose_row(o, 0, cb, bNorm, t0);
  }
  s.beta = std::sqrt(std::fabs(cb));
  s.gamma = cb / s.beta;
  K(khip_fill(ctx, n, v_prev, 0.0));
  K(khip_fill(ctx, n, u_prev, 0.0));
  K(khip_divcopy(ctx, n, v, r0, s.beta));
  K(khip_divcopy(ctx, n, u, c, s.gamma));
  s.cs = s.cs_prev = -1.0;
  K(khip_fill(ctx, n, dbar, 0.0));
  s.norm_v = bNorm / s.beta;
  s.transfer_to_bicg = prm.transfer_to_bicg ? 1 : 0;
  s.stop_seq = kSeqNever;
  s.solved_lq = (bNorm <= s.eps_tol) ? 1 : 0;
  bool tired = 0 >= itmax, user_exit = false, overtimed = false;
  int64_t iter = 0;
  auto running = [&] { return !(s.solved_lq || s.solved_cg || tired || s.breakdown || user_exit || overtimed); };
  // q <- M A N v and p <- N' A' M' u (:234-242)
  auto products = [&](const double *vk, const double *uk, double *qk, double *pk) -> int {
    if (!NisI) KHIP_TRY(apply_op_no_epilogue(ctx, N, vk, ws->s));
    KHIP_TRY(apply_op_no_epilogue(ctx, A, NisI ? vk : ws->s, MisI ? qk : ws->t));
    if (!MisI) KHIP_TRY(apply_op_no_epilogue(ctx, M, ws->t, qk));
    if (!MisI) KHIP_TRY(apply_op_no_epilogue(ctx, Mt, uk, ws->t));
    KHIP_TRY(apply_op_no_epilogue(ctx, At, MisI ? uk : ws->t, NisI ? pk : ws->s));
    if (!NisI) KHIP_TRY(apply_op_no_epilogue(ctx, Nt, ws->s, pk));
    return KHIP_OK;
  };
  // the end of an iteration on the host-driven loops (:347, :367-374)
  auto host_tail = [&](int64_t k) {
    if (history) ws->box.push(s.rNorm_lq);
    if (o.callback) {
      ws->box.publish();                          // the callback reads stats.residuals
      user_exit = o.callback(ws, o.callback_data) != 0;
    }
    tired = k >= itmax;
    overtimed = time_limit_reached(ctx, now_s() - t0, timemax);
    if (kdisplay(k, verbose)) verbose_row(o, k, s.alpha, s.rNorm_lq, t0);
  };

  const bool csr_pair = A->csr && !A->apply && At->csr && !At->apply;
  const bool device_loop = o.fused >= 2 && csr_pair && MisI && NisI && !o.callback && verbose <= 0;
  ws->box.path = (device_loop && running()) ? 2 : (o.fused ? 1 : 0);   // a loop that never starts reports 1, as the early returns do

  if (ws->box.path == 0) {
    // ---------------------------------------------------------------- the reference's primitive sequence (:226-375) ----
    while (running()) {
      const int64_t k = ++iter;
      K(products(v, u, q, p));
      K(khip_axpy(ctx, n, -s.gamma, v_prev, q));
      K(khip_axpy(ctx, n, -s.beta, u_prev, p));
      double uq;
      K(khip_dot(ctx, n, u, q, &uq));
      bilq_step_a(s, uq);
      K(khip_axpy(ctx, n, -s.alpha, v, q));
      K(khip_axpy(ctx, n, -s.alpha, u, p));
      double pq;
      K(khip_dot(ctx, n, p, q, &pq));
      bilq_step_b(s, pq, k);
      if (k == 1) {
        K(khip_copy(ctx, n, dbar, v));
      } else {
        K(khip_axpy(ctx, n, s.zc, dbar, x));
        K(khip_axpy(ctx, n, s.zs, v, x));
        K(khip_axpby(ctx, n, s.neg_c, v, s.sn, dbar));
      }
      K(khip_copy(ctx, n, v_prev, v));
      K(khip_copy(ctx, n, u_prev, u));
      if (pq != 0) {
        K(khip_divcopy(ctx, n, v, q, s.beta_next));
        K(khip_divcopy(ctx, n, u, p, s.gamma_next));
      }
      double vv, norm_next;
      K(khip_dot(ctx, n, v_prev, v, &vv));
      K(khip_nrm2(ctx, n, v, &norm_next));
      bilq_step_c(s, vv, norm_next, k);
      host_tail(k);
    }
  } else if (ws->box.path == 1) {
    // ---------------------------------------------------------------- host-driven loop on the fused kernels ----------
    K(ws->loop.alloc());
    s.hist = nullptr;
    while (running()) {
      const int64_t k = ++iter;
      K(products(v, u, q, p));
      K(ws->loop.upload(ctx, s));
      int slot = take_slots(ctx, 1);
      K(launch_p1(ctx, n, ws->loop.dev, v_prev, u_prev, u, q, p, slot));
      double uq;
      K(fetch_results(ctx, slot, 1, &uq));
      bilq_step_a(s, uq);
      K(ws->loop.upload(ctx, s));
      slot = take_slots(ctx, 1);
      K(launch_p2(ctx, n, ws->loop.dev, v, u, q, p, slot));
      double pq;
      K(fetch_results(ctx, slot, 1, &pq));
      bilq_step_b(s, pq, k);
      K(ws->loop.upload(ctx, s));
      slot = take_slots(ctx, 2);
      K(launch_p3(ctx, n, ws->loop.dev, x, dbar, v, u, q, p, v_prev, u_prev, k == 1, slot));
      double r[2];
      K(fetch_results(ctx, slot, 2, r));
      std::swap(v, v_prev);                        // vₖ₋₁ <- vₖ ; vₖ <- vₖ₊₁ (:325-330) as a rotation of the roles
      std::swap(u, u_prev);
      bilq_step_c(s, r[0], std::sqrt(r[1]), k);
      host_tail(k);
    }
  } else {
    // ---------------------------------------------------------------- device-resident loop -----------------------------
    double *vc = v, *vp = v_prev, *uc = u, *up = u_prev;
    auto step = [&](BilqDevState *dev, long long j) {
      const int64_t k = j + 1;
      ctx->ctl = SeqCtl{&dev->stop_seq, 4 * j + 1, EPI_NONE, nullptr};
      int rc = spmv_any(ctx, A->csr, vc, q, -1);                                          // q = A vₖ
      if (rc == KHIP_OK) rc = spmv_any(ctx, At->csr, uc, p, -1);                          // p = A' uₖ
      if (rc != KHIP_OK) return rc;
      ctx->ctl = SeqCtl{&dev->stop_seq, 4 * j + 2, EPI_BILQ_A, dev};
      int slot = take_slots(ctx, 1);
      rc = launch_p1(ctx, n, dev, vp, up, uc, q, p, slot);                               // P1 ; u.q -> α
      if (rc == KHIP_OK && ctx->comm) rc = comm_allreduce_dd_device(ctx, slot, 1);
      if (rc != KHIP_OK) return rc;
      ctx->ctl = SeqCtl{&dev->stop_seq, 4 * j + 3, EPI_BILQ_B, dev};
      slot = take_slots(ctx, 1);
      rc = launch_p2(ctx, n, dev, vc, uc, q, p, slot);                                   // P2 ; p.q -> the LQ update
      if (rc == KHIP_OK && ctx->comm) rc = comm_allreduce_dd_device(ctx, slot, 1);
      if (rc != KHIP_OK) return rc;
      ctx->ctl = SeqCtl{&dev->stop_seq, 4 * j + 4, EPI_BILQ_C, dev};
      slot = take_slots(ctx, 2);
      rc = launch_p3(ctx, n, dev, x, dbar, vc, uc, q, p, vp, up, k == 1, slot);          // P3 ; the two dots -> tests
      if (rc == KHIP_OK && ctx->comm) rc = comm_allreduce_dd_device(ctx, slot, 2);
      ctx->ctl = SeqCtl{};
      if (rc != KHIP_OK) return rc;
      std::swap(vc, vp);
      std::swap(uc, up);
      return KHIP_OK;
    };
    // a finite timemax: the first chunk is ONE iteration, so that a limit already used up stops after iteration 1 as the
    // host-driven loop does
    const DeviceLoopArgs loop_args{itmax, t0, timemax, history, {&ws->box.residuals, nullptr, nullptr},
                                   timemax < 1e300 ? 1 : kDevChunk};
    K(ws->loop.run(ctx, s, loop_args, step, &s, &overtimed));
    iter = s.iter;
    tired = iter >= itmax;
    // the host rotated the roles for every iteration it enqueued; the device ran s.iter of them
    if (iter & 1) { std::swap(v, v_prev); std::swap(u, u_prev); }
  }
  ws->v = v; ws->v_prev = v_prev; ws->u = u; ws->u_prev = u_prev;
  if (verbose > 0) klogf(o.log_fd, "\n");
  if (s.solved_cg) K(khip_axpy(ctx, n, s.zbar, dbar, x));                                                // :380-382
  const char *status = "unknown";                                                                         // :385-390
  if (tired) status = "maximum number of iterations exceeded";
  if (s.breakdown) status = "Breakdown \xe2\x9f\xa8u\xe2\x82\x96\xe2\x82\x8a\xe2\x82\x81,v\xe2\x82\x96\xe2\x82\x8a\xe2\x82\x81\xe2\x9f\xa9 = 0";
  if (s.solved_lq) status = "solution x\xe1\xb4\xb8 good enough given atol and rtol";
  if (s.solved_cg) status = "solution x\xe1\xb6\x9c good enough given atol and rtol";
  if (user_exit) status = "user-requested exit";
  if (overtimed) status = "time limit exceeded";
  if (!NisI) {                                                                                            // :393-396
    K(khip_copy(ctx, n, ws->s, x));
    K(apply_op(ctx, N, ws->s, x));
  }
  if (warm_start) K(khip_axpy(ctx, n, 1.0, ws->dx, x));
  st->niter = (int)iter;
  st->solved = (s.solved_lq || s.solved_cg) ? 1 : 0;
  st->inconsistent = 0;
  snprintf(st->status, sizeof(st->status), "%s", status);
  finish();
  return KHIP_OK;
}

}  // extern "C"
