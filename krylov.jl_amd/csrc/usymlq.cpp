// usymlq.cpp -- usymlq! (src/usymlq.jl:124-366) above the device primitives, with its fused gfx950 kernel.
//
// Real Float64, A of m rows and n columns, no M and N.  The minimum-error counterpart of usymqr! on the same process, with the
// transfer to the USYMCG point.  Three loops, chosen as for usymqr! (khip_usymlq_last_path):
//   0  options.fused = 0, and every m ≠ n system: the reference's primitive sequence, one launch per k* call, one host sync per
//      kdot / knorm;
//   1  the host-driven loop on the fused kernels (a user operator, a callback or verbose > 0);
//   2  the device-resident loop (default; A and Aᴴ both CSR handles): the scalar recurrences and stopping tests run as the
//      epilogues of the two reductions of an iteration (usymlq_step_a/b, solver_device.hpp), iterations are enqueued ahead.
// One iteration on the fused paths (m = n), after q = A uₖ and p = Aᴴ vₖ:
//   P1   k ≥ 2: q = fma(-γₖ, vₖ₋₁, q) ; p = fma(-βₖ, uₖ₋₁, p) ; vₖ.q                    (ssy.hpp)                   56n bytes
//   P2   q = fma(-αₖ, vₖ, q) ; p = fma(-αₖ, uₖ, p) ; (q.q, p.p)                        (ssy.hpp)                   48n bytes
//   P3   k = 1: d̅ = uₖ ; else x = fma(ζₖ₋₁sₖ, uₖ, fma(ζₖ₋₁cₖ, d̅, x)) ; d̅ = fma(-cₖ, uₖ, sₖ d̅) ;
//        βₖ₊₁ ≠ 0 ? vₖ₊₁ = q / βₖ₊₁ ; γₖ₊₁ ≠ 0 ? uₖ₊₁ = p / γₖ₊₁                                                     72n bytes
// (P3 reads uₖ, x, d̅, q, p and writes x, d̅, vₖ₊₁, uₖ₊₁; 48n at k = 1, where x and d̅ are not read and x is not written.)  That
// is 176n beside the two products, against 264n for the primitive sequence: two kaxpy! of P1 (48n), kdot (16n), two kaxpy! of
// P2 (48n), two knorm (16n), two kaxpy! into x (48n), kaxpby! (24n), two kcopy! (32n), two kdivcopy! (32n).  kcopy!(vₖ₋₁, vₖ)
// and kcopy!(uₖ₋₁, uₖ) become rotations of the buffers' roles (vₖ₊₁ is written where vₖ₋₁ was).  Every elementwise value uses
// the expression of the primitive it replaces (fma for kaxpy!, fma(a, x, b y) for kaxpby!, / for kdivcopy!): the fused loops
// agree with the primitive sequence bit for bit on elementwise values and to the reductions' one ulp otherwise; loops 1 and 2
// run the same kernels and the same scalar code and produce the same bits.
// P3 has no reduction; the stopping tests belong to P2's epilogue, and P3 of the iteration that stops still runs, because the
// reference updates x, d̅, vₖ₊₁ and uₖ₊₁ before it tests.
// This file owns P3, the set-up scalars, the LQ part of a primitive iteration, the USYMCG point and the status strings; the loops
// are ssy.hpp's.
#include "ssy.hpp"   // P1, P2 and the driver of the three loops
#include "usymlq_xd.hpp"

using namespace khip;

namespace khip {   // (named, not anonymous: stable kernel names in traces)

// ---------------------------------------------------------------------------------------------------------- kernels ----
// Each thread owns one VEC-vector of every stream; the odd tail element (VEC = 2, n odd) goes to thread 0 of block 0.
// Cache hints, the rule of ssy.hpp: a load is non-temporal when it is the LAST read of that data (x, d̅, q, p: overwritten here
// or by the next products); uₖ is read again by the next P1 (as uₖ₋₁) and vₖ (read only when βₖ₊₁ = 0) likewise: they stay
// cacheable.  A store is non-temporal when nothing reads it before the next iteration's P3 (x, d̅); vₖ₊₁ and uₖ₊₁ are read by
// the next products.

// x and d̅ of one element from iteration 2 on (:285-290): usymlq_xd (usymlq_xd.hpp, shared with trilqr.cpp)

// P3: first ? d̅ = u : usymlq_xd ; v_next = βₖ₊₁ ≠ 0 ? q / βₖ₊₁ : v ; u_next = γₖ₊₁ ≠ 0 ? p / γₖ₊₁ : u                (:279-302)
// The two guards are independent.  No reduction: the sequence number comes as an argument.
template <int VEC, bool NT>
__global__ __launch_bounds__(kBlock) void usymlq_p3_kernel(int64_t n, const UsymlqDevState *st, const long long *stop_seq, long long seq,
                                                          double *x, double *dbar, const double *v, const double *u, const double *q,
                                                          const double *p, double *v_next, double *u_next, int first) {
  using T = typename VecT<VEC>::type;
  if (seq_skip(stop_seq, seq)) return;
  const double zc = st->zc, zs = st->zs, nc = st->neg_c, sn = st->sn;
  const double bn = st->beta_next, gn = st->gamma_next;
  const bool div_v = bn != 0.0, div_u = gn != 0.0;
  const int64_t nvec = n / VEC;
  const int64_t i = lane_index();
  if (i < nvec) {
    const T uv = ldg<false>(reinterpret_cast<const T *>(u) + i);       // u is the next iteration's u_prev
    T dv = uv;
    if (!first) {
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
    const int64_t t = n - 1;
    const double ue = u[t];
    if (first) {
      dbar[t] = ue;
    } else {
      double xe = x[t], de = dbar[t];
      usymlq_xd(ue, xe, de, zc, zs, nc, sn);
      x[t] = xe;
      dbar[t] = de;
    }
    v_next[t] = div_v ? q[t] / bn : v[t];
    u_next[t] = div_u ? p[t] / gn : ue;
  }
}

}  // namespace khip

namespace {

// P3 takes its sequence number from ctx->ctl, as the reductions do (all zero on the host-driven loop)
int launch_p3(khip_ctx *ctx, int64_t n, const UsymlqDevState *st, double *x, double *dbar, const double *v, const double *u,
              const double *q, const double *p, double *v_next, double *u_next, bool first) {
  VecPlan L;
  KHIP_TRY(vec_plan(ctx, n, {x, dbar, v, u, q, p, v_next, u_next}, &L));
  const SeqCtl ctl = ctx->ctl;
  ProfScope prof_scope(ctx, kProfUsymlqP3);
  vec_dispatch_vn<ScalarPathNT::never>(L, [&](auto V, auto N) {
    hipLaunchKernelGGL((usymlq_p3_kernel<V, N>), L.grid(), dim3(kBlock), 0, ctx->stream, n, st, ctl.stop_seq, ctl.seq, x, dbar, v, u,
                       q, p, v_next, u_next, first ? 1 : 0); });
  KHIP_CHECK_HIP(hipGetLastError());
  return KHIP_OK;
}

}  // namespace

struct khip_usymlq_workspace {
  khip_ctx *ctx;
  int64_t m, n;
  // by their CURRENT role: the fused loops rotate (v_prev, v) and (u_prev, u).  v_prev, v, q have m entries, the others n
  double *u_prev = nullptr, *u = nullptr, *p = nullptr, *x = nullptr, *dbar = nullptr, *v_prev = nullptr, *v = nullptr, *q = nullptr,
         *dx = nullptr;
  Borrowed borrowed;                        // the caller's vectors (khip_usymlq_workspace_adopt*): never freed here
  bool warm_start = false;
  StatsBox box;
  DeviceLoop<UsymlqDevState, 3> loop;       // fused loops: device copy of the scalar state, pinned snapshots + staging, history
};

namespace {

// uₖ₋₁, uₖ, p, x, d̅, vₖ₋₁, vₖ, q come with the workspace; Δx stays empty until a warm start (src/krylov_workspaces.jl,
// UsymlqWorkspace: the table keeps its order)
using W = khip_usymlq_workspace;
constexpr WsVec<W> kVectors[] = {{"u_prev", &W::u_prev, Core}, {"u", &W::u, Core},       {"p", &W::p, Core},
                                 {"x", &W::x, Core},           {"dbar", &W::dbar, Core}, {"v_prev", &W::v_prev, Core, RowSide},
                                 {"v", &W::v, Core, RowSide},  {"q", &W::q, Core, RowSide}, {"dx", &W::dx, Lazy}};

// what usymlq! adds to the driver of the process (ssy.hpp)
struct Usymlq : SsyPolicy<UsymlqDevState, W> {
  static constexpr Epilogue kEpiA = EPI_USYMLQ_A, kEpiB = EPI_USYMLQ_B;
  double *x, *dbar;
  static void step_a(State &s, double vq) { usymlq_step_a(s, vq); }
  static void step_b(State &s, double qq, double pp, int64_t k) { (void)usymlq_step_b(s, qq, pp, k); }
  static bool stopped(const State &s) { return s.solved_lq || s.solved_cg; }
  int p3(khip_ctx *ctx, int64_t n, const State *dev, const SsyRoles &r, int64_t k) const {
    return launch_p3(ctx, n, dev, x, dbar, r.v, r.u, r.q, r.p, r.v_prev, r.u_prev, k == 1);
  }
  void push_history(W *ws, const State &s) const { ws->box.push(s.rNorm_lq); }
  void verbose_row(const khip_options &o, long long k, const State &s, double t0) const {                // src/usymlq.jl:338
    klogf(o.log_fd, "%5lld  %7.1e  %.2fs\n", k, s.rNorm_lq, now_s() - t0);
  }
  // d̅ and x, then the shift of v and u (src/usymlq.jl:279-302)
  int primitive_tail(Ssy<Usymlq> &L, int64_t k) {
    W *ws = L.ws;
    khip_ctx *ctx = L.ctx;
    const int64_t n = L.n;
    State &s = L.s;
    if (k == 1) {
      K(khip_copy(ctx, n, dbar, L.r.u));
    } else {
      K(khip_axpy(ctx, n, s.zc, dbar, x));
      K(khip_axpy(ctx, n, s.zs, L.r.u, x));
      K(khip_axpby(ctx, n, s.neg_c, L.r.u, s.sn, dbar));
    }
    K(L.shift());
    return KHIP_OK;
  }
};

}  // namespace

extern "C" {

khip_usymlq_params khip_usymlq_default_params(void) {
  khip_usymlq_params p;
  p.transfer_to_usymcg = 1;
  return p;
}

int khip_usymlq_workspace_create(khip_ctx *ctx, int64_t m, int64_t n, khip_usymlq_workspace **out) {
  return ws_create(ctx, m, n, kVectors, "usymlq_workspace_create", khip_usymlq_workspace_destroy, out);
}

int khip_usymlq_workspace_adopt(khip_ctx *ctx, int64_t m, int64_t n, double *u_prev, double *u, double *p, double *x, double *dbar,
                                double *v_prev, double *v, double *q, khip_usymlq_workspace **out) {
  return ws_adopt(ctx, m, n, kVectors, "usymlq_workspace_adopt", {u_prev, u, p, x, dbar, v_prev, v, q}, out);
}

int khip_usymlq_workspace_adopt_vector(khip_usymlq_workspace *ws, const char *name, double *ptr) {
  return ws_adopt_vector(ws, kVectors, "usymlq_workspace_adopt_vector", name, ptr);
}

int khip_usymlq_workspace_destroy(khip_usymlq_workspace *ws) {
  if (!ws) return KHIP_OK;
  ws_free_vectors(ws, kVectors);
  ws->loop.release();
  delete ws;
  return KHIP_OK;
}

int khip_usymlq_warm_start(khip_usymlq_workspace *ws, const double *x0) { return ws_warm_start(ws, kVectors, x0, "usymlq_warm_start"); }
double *khip_usymlq_solution(khip_usymlq_workspace *ws) { return ws ? ws->x : nullptr; }
const khip_stats *khip_usymlq_stats(khip_usymlq_workspace *ws) { return ws ? &ws->box.st : nullptr; }
int khip_usymlq_last_path(khip_usymlq_workspace *ws) { return ws ? ws->box.path : -1; }
double *khip_usymlq_vector(khip_usymlq_workspace *ws, const char *name) { return ws_vector(ws, kVectors, name); }
size_t khip_usymlq_workspace_bytes(khip_usymlq_workspace *ws) { return ws_bytes(ws, kVectors); }

int khip_usymlq_solve(khip_usymlq_workspace *ws, const khip_operator *A, const khip_operator *At, const double *b, const double *c,
                      const khip_options *opts_in, const khip_usymlq_params *params_in) {
  KHIP_REQUIRE(ws && A && b, "usymlq_solve: null argument");
  const khip_usymlq_params prm = params_in ? *params_in : khip_usymlq_default_params();
  Ssy<Usymlq> L(ws, A, At, opts_in);
  khip_ctx *ctx = L.ctx;
  const khip_options &o = L.o;
  const int64_t m = L.m, n = L.n;
  UsymlqDevState &s = L.s;
  const double atol = tol_or_default(o.atol), rtol = tol_or_default(o.rtol);

  if (int rc = L.check("usymlq", c)) return rc;                                                           // :130-133
  if (o.verbose > 0) klogf(o.log_fd, "USYMLQ: system of %lld equations in %lld variables\n", (long long)m, (long long)n);   // :134
  const bool warm_start = ws->warm_start;
  ws->box.reset();                                                                                        // reset!(stats)
  double *x = L.pol.x = ws->x, *dbar = L.pol.dbar = ws->dbar;

  // set-up, the same primitives on every path (:150-198)
  const double *r0;
  K(L.residual(b, warm_start, &r0));
  K(khip_fill(ctx, n, x, 0.0));
  double bNorm;
  K(khip_nrm2(ctx, m, r0, &bNorm));
  if (L.history) ws->box.push(bNorm);
  ws->box.path = (o.fused && L.square()) ? 1 : 0;
  if (bNorm == 0) return L.end(1, 0, "x is a zero-residual solution", warm_start);                       // :161-170
  L.itmax = o.itmax == 0 ? global_rows(ctx, A, m) + global_rows(ctx, At, n) : o.itmax;                   // m + n of the global system (:173)
  s.bNorm = bNorm;
  s.eps_tol = atol + rtol * bNorm;                                                                       // :175
  if (o.verbose > 0) {                                                                                    // :176-177 (label padded by hand)
    klogf(o.log_fd, "%5s  %s  %5s\n", "k", "   \xe2\x80\x96r\xe2\x82\x96\xe2\x80\x96", "timer");
    if (kdisplay(0, o.verbose)) klogf(o.log_fd, "%5d  %7.1e  %.2fs\n", 0, bNorm, now_s() - L.t0);
  }
  double gamma1;
  K(khip_nrm2(ctx, n, c, &gamma1));                                                                      // :180
  K(L.start(bNorm, gamma1, r0, c));                                                                      // :179-184
  s.cs = s.cs_prev = -1.0;                                                                               // :185-186
  K(khip_fill(ctx, n, dbar, 0.0));                                                                       // :187
  s.transfer = prm.transfer_to_usymcg ? 1 : 0;
  s.stop_seq = kSeqNever;
  s.solved_lq = (bNorm <= s.eps_tol) ? 1 : 0;                                                            // :193-194

  K(L.iterate());                                                                                         // :200-339

  if (s.solved_cg) K(khip_axpy(ctx, n, s.zbar, dbar, x));                                                // :344-346, d̅ₖ as P3 left it
  const char *status = "unknown";                                                                         // :349-353
  if (L.tired) status = "maximum number of iterations exceeded";
  if (s.solved_lq) status = "solution x\xe1\xb4\xb8 good enough given atol and rtol";
  if (s.solved_cg) status = "solution x\xe1\xb6\x9c good enough given atol and rtol";
  if (L.user_exit) status = "user-requested exit";
  if (L.overtimed) status = "time limit exceeded";
  return L.end((s.solved_lq || s.solved_cg) ? 1 : 0, 0, status, warm_start);                             // :356-365
}

}  // extern "C"
