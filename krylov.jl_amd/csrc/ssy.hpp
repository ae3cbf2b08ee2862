// ssy.hpp -- the orthogonal tridiagonalisation of Saunders, Simon and Yip as usymqr! (usymqr.cpp) runs it, written so that the
// other solvers on the same process (usymlq!, trilqr!) can follow on it: its two fused passes and the three loops around them.
//
// The process is the same in all of them, line for line (src/usymqr.jl:211-225): after q = A uₖ and p = Aᴴ vₖ,
//   P1   k ≥ 2: q = fma(-γₖ, vₖ₋₁, q) ; p = fma(-βₖ, uₖ₋₁, p) ; every k: vₖ.q                                      56n bytes
//   P2   q = fma(-αₖ, vₖ, q) ; p = fma(-αₖ, uₖ, p) ; (q.q, p.p)                                                   48n bytes
// The kernels read γₖ, βₖ and αₖ from the common leading part of a solver's device state (SsyCoef, solver_device.hpp).  At k = 1
// the reference skips the two kaxpy! of P1 (v₀ = u₀ = 0, :214-217); P1 skips them as well (`first`: neither vₖ₋₁ nor uₖ₋₁ is
// read and q, p are not written, 8n bytes), so no signed zero can differ from the primitive sequence.
//
// Ssy<P> is the driver, a sibling of BiLanczos<P> (bilanczos.hpp): the argument and shape checks, the products, the path
// decision, the primitive sequence's head and shift (path 0, with one length per side: m ≠ n runs there), the host-driven loop
// on the fused kernels (path 1), the device-resident loop (path 2) and the end of a host-driven iteration.  A solver is a
// policy P (SsyPolicy names what it may leave out): its device state and epilogue ids, its scalar steps, its P3 launch, the
// rotation of its own buffers, and its part of a primitive iteration.  The process has two reductions, so an iteration of the
// device-resident loop has four numbers: the products, P1, P2 and the solver's P3, which has no reduction and still runs in the
// iteration that stops the loop (the epilogue of P2 sets stop_seq = seq + 2).  One template, resolved at compile time.
#pragma once

#include <utility>

#include "solver_host.hpp"
#include "vec_launch.hpp"

namespace khip {   // (named, not anonymous: stable kernel names in traces)

// Each thread owns one VEC-vector of every stream; the odd tail element (VEC = 2, n odd) goes to thread 0 of block 0.
// Cache hints, the rule of bilanczos.hpp: a load is non-temporal when it is the LAST read of that data (the vector is dead or
// overwritten afterwards); vₖ and uₖ are read again up to the next iteration's P1 (as vₖ₋₁, uₖ₋₁) and stay cacheable.  A store is
// non-temporal when nothing reads it before the next iteration's P3.

// P1: !first ? (q = fma(-γ, v_prev, q) ; p = fma(-β, u_prev, p)) ; acc = v . q                        (src/usymqr.jl:214-219)
// The dot partner is v, not u: that is the difference from bilq_p1_kernel.
template <int VEC, bool NT, bool COMP>
__global__ __launch_bounds__(kBlock) void ssy_p1_kernel(int64_t n, const SsyCoef *st, const double *v_prev, const double *u_prev,
                                                       const double *v, double *q, double *p, int first, RedArgs ra) {
  using T = typename VecT<VEC>::type;
  if (seq_skip(ra.stop_seq, ra.seq)) return;
  const double ng = -st->gamma, nb = -st->beta;
  dd acc[1] = {dd{0.0, 0.0}};
  const int64_t nvec = n / VEC;
  const int64_t i = lane_index();
  if (i < nvec) {
    const T vv = ldg<false>(reinterpret_cast<const T *>(v) + i);       // v is read again by P2
    if (first) {
      const T qv = ldg<false>(reinterpret_cast<const T *>(q) + i);     // q is read again by P2
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc_prod<COMP>(acc[0], vget(vv, e), vget(qv, e));
    } else {
      const T qv = ldg<NT>(reinterpret_cast<const T *>(q) + i);
      const T pv = ldg<NT>(reinterpret_cast<const T *>(p) + i);
      const T vp = ldg<NT>(reinterpret_cast<const T *>(v_prev) + i);
      const T up = ldg<NT>(reinterpret_cast<const T *>(u_prev) + i);
      T qo, po;
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const double qn = fma(ng, vget(vp, e), vget(qv, e));
        vset(qo, e, qn);
        vset(po, e, fma(nb, vget(up, e), vget(pv, e)));
        acc_prod<COMP>(acc[0], vget(vv, e), qn);
      }
      stg<false>(qo, reinterpret_cast<T *>(q) + i);                     // q, p are read again by P2
      stg<false>(po, reinterpret_cast<T *>(p) + i);
    }
  }
  if (VEC == 2 && owns_tail(n)) {
    const int64_t t = n - 1;
    double qn = q[t];
    if (!first) {
      qn = fma(ng, v_prev[t], qn);
      q[t] = qn;
      p[t] = fma(nb, u_prev[t], p[t]);
    }
    acc_prod<COMP>(acc[0], v[t], qn);
  }
  wave_publish<1>(acc, ra);
}

// P2: q = fma(-α, v, q) ; p = fma(-α, u, p) ; acc = (q . q, p . p)                                     (src/usymqr.jl:221-225)
template <int VEC, bool NT, bool COMP>
__global__ __launch_bounds__(kBlock) void ssy_p2_kernel(int64_t n, const SsyCoef *st, const double *v, const double *u, double *q,
                                                       double *p, RedArgs ra) {
  using T = typename VecT<VEC>::type;
  if (seq_skip(ra.stop_seq, ra.seq)) return;
  const double na = -st->alpha;
  dd acc[2] = {dd{0.0, 0.0}, dd{0.0, 0.0}};
  const int64_t nvec = n / VEC;
  const int64_t i = lane_index();
  if (i < nvec) {
    const T qv = ldg<NT>(reinterpret_cast<const T *>(q) + i);
    const T pv = ldg<NT>(reinterpret_cast<const T *>(p) + i);
    const T vv = ldg<false>(reinterpret_cast<const T *>(v) + i);       // v is the next iteration's v_prev
    const T uv = ldg<false>(reinterpret_cast<const T *>(u) + i);       // u is read again by P3 and the next P1
    T qo, po;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const double qn = fma(na, vget(vv, e), vget(qv, e));
      const double pn = fma(na, vget(uv, e), vget(pv, e));
      vset(qo, e, qn);
      vset(po, e, pn);
      acc_prod<COMP>(acc[0], qn, qn);
      acc_prod<COMP>(acc[1], pn, pn);
    }
    stg<false>(qo, reinterpret_cast<T *>(q) + i);                       // q, p are read again by P3
    stg<false>(po, reinterpret_cast<T *>(p) + i);
  }
  if (VEC == 2 && owns_tail(n)) {
    const int64_t t = n - 1;
    const double qn = fma(na, v[t], q[t]);
    const double pn = fma(na, u[t], p[t]);
    q[t] = qn;
    p[t] = pn;
    acc_prod<COMP>(acc[0], qn, qn);
    acc_prod<COMP>(acc[1], pn, pn);
  }
  wave_publish<2>(acc, ra);
}

namespace {   // each solver file gets its own copy of the launchers, as of everything in solver_host.hpp

int launch_ssy_p1(khip_ctx *ctx, int64_t n, const SsyCoef *st, const double *v_prev, const double *u_prev, const double *v, double *q,
                  double *p, bool first, int slot) {
  VecPlan L;
  KHIP_TRY(vec_plan(ctx, n, {v_prev, u_prev, v, q, p}, &L, 1));
  RedArgs ra = make_red_args(ctx, slot);
  { ProfScope prof_scope(ctx, kProfSsyP1);
    vec_dispatch<ScalarPathNT::never>(L, [&](auto V, auto N, auto C) {
      hipLaunchKernelGGL((ssy_p1_kernel<V, N, C>), L.grid(), dim3(kBlock), 0, ctx->stream, n, st, v_prev, u_prev, v, q, p, first ? 1 : 0,
                         ra); });
  }
  KHIP_CHECK_HIP(hipGetLastError());
  return launch_finish(ctx, L.waves(), 1, slot);
}
int launch_ssy_p2(khip_ctx *ctx, int64_t n, const SsyCoef *st, const double *v, const double *u, double *q, double *p, int slot) {
  VecPlan L;
  KHIP_TRY(vec_plan(ctx, n, {v, u, q, p}, &L, 2));
  RedArgs ra = make_red_args(ctx, slot);
  { ProfScope prof_scope(ctx, kProfSsyP2);
    vec_dispatch<ScalarPathNT::never>(L, [&](auto V, auto N, auto C) {
      hipLaunchKernelGGL((ssy_p2_kernel<V, N, C>), L.grid(), dim3(kBlock), 0, ctx->stream, n, st, v, u, q, p, ra); });
  }
  KHIP_CHECK_HIP(hipGetLastError());
  return launch_finish(ctx, L.waves(), 2, slot);
}

// the six vectors of the process by their CURRENT role: the fused loops rotate (v_prev, v) and (u_prev, u) where the reference
// copies (vₖ₊₁ and uₖ₊₁ are written where vₖ₋₁ and uₖ₋₁ were).  v, v_prev and q have m entries; u, u_prev and p have n.
struct SsyRoles {
  double *v, *v_prev, *u, *u_prev, *q, *p;
  void rotate() { std::swap(v, v_prev); std::swap(u, u_prev); }
};

// What a policy may leave out.  It must supply: State (an SsyCoef with beta_next, gamma_next, iter and the DeviceLoop fields),
// Workspace, kEpiA / kEpiB, step_a(s, vq), step_b(s, qq, pp, k) (the fetched sums as they are: the policy takes the square
// roots), stopped(s), p3(ctx, n, dev, roles, k) (it takes its sequence number from ctx->ctl), push_history(ws, s),
// verbose_row(o, k, s, t0) and primitive_tail(driver, k): what the reference does between its two norms and the end of the
// iteration, on the primitives, with driver.shift() where the reference has its kcopy! / kdivcopy! of v and u.
template <class S, class W>
struct SsyPolicy {
  using State = S;
  using Workspace = W;
  void begin_iteration(const S &) {}                       // host-driven loops: before the products of an iteration
  void rotate(int64_t /*k*/) {}                            // the policy's own buffers, after P3 of iteration k
  void fix_after_device_loop(const S &) {}                 // ... which the host rotated once per ENQUEUED iteration
  void store(W *) const {}                                 // the roles of its own buffers back into the workspace
  static std::vector<double> *dual_history(W *) { return nullptr; }   // a second history stream of the device loop
};

template <class P>
struct Ssy {
  using State = typename P::State;
  using W = typename P::Workspace;
  W *const ws;
  khip_ctx *const ctx;
  const khip_operator *const A, *const At;
  const khip_options o;
  const double t0 = now_s(), timemax;
  const int64_t m, n;                                       // A is m × n: v, v_prev, q have m entries; u, u_prev, p, x, w have n
  const bool history;
  int64_t itmax = 0, iter = 0;
  bool tired = false, user_exit = false, overtimed = false;
  SsyRoles r;
  State s;
  P pol;

  Ssy(W *ws_, const khip_operator *A_, const khip_operator *At_, const khip_options *opts)
      : ws(ws_), ctx(ws_->ctx), A(A_), At(At_), o(opts ? *opts : khip_default_options()), timemax(timemax_of(o)), m(ws_->m),
        n(ws_->n), history(o.history != 0), r{ws_->v, ws_->v_prev, ws_->u, ws_->u_prev, ws_->q, ws_->p} {
    memset(&s, 0, sizeof(s));
    (void)take_alloc_seconds();
  }

  bool square() const { return m == n; }

  // At, c and the shapes (src/usymqr.jl:133-136): A is m × n and At is n × m.  A row-partitioned handle counts global columns,
  // so its side lengths cannot be told apart from here: it is taken when the local block is square and refused otherwise.
  int check(const char *solver, const double *c) {
    char msg[200];
    snprintf(msg, sizeof(msg), "%s_solve: At (the adjoint of A) is required", solver);
    if (!At) return ws->box.fail(KHIP_ERR_INVALID, msg);
    snprintf(msg, sizeof(msg), "%s_solve: c is required", solver);
    if (!c) return ws->box.fail(KHIP_ERR_INVALID, msg);
    const bool dist = (A->csr && !A->apply && A->csr->dist) || (At->csr && !At->apply && At->csr->dist);
    if (dist && !square()) {
      snprintf(msg, sizeof(msg), "%s_solve: a row-partitioned rectangular system (m != n) is not supported", solver);
      return ws->box.fail(KHIP_ERR_UNSUPPORTED, msg);
    }
    if (int rc = check_shape(ws, {A})) return rc;
    if (At->csr && !At->apply) {
      int64_t am, an;
      khip_csr_shape(At->csr, &am, &an, nullptr);
      if (am != n || (an != m && !At->csr->dist)) {
        snprintf(msg, sizeof(msg), "(workspace.n, workspace.m) = (%lld, %lld) is inconsistent with size(At) = (%lld, %lld)",
                 (long long)n, (long long)m, (long long)am, (long long)an);
        return ws->box.fail(KHIP_ERR_INVALID, msg);
      }
    }
    return KHIP_OK;
  }

  // r₀ = b - A Δx after a warm start (held in q, m entries), b itself otherwise (src/usymqr.jl:153-158, with m where the reference
  // passes n to its kaxpby!: its slip for m ≠ n)
  int residual(const double *b, bool warm_start, const double **r0) {
    *r0 = b;
    if (!warm_start) return KHIP_OK;
    K(apply_op(ctx, A, ws->dx, r.q));
    K(khip_axpby(ctx, m, 1.0, b, -1.0, r.q));
    *r0 = r.q;
    return KHIP_OK;
  }

  // every return of a solve past the checks (ws_end speaks of ws->n, which is x's length)
  int end(int solved, int inconsistent, const char *status, bool warm_start) {
    return ws_end(ws, {iter, solved, inconsistent, status, warm_start, t0, true});
  }

  // β₁ v₁ = r₀, γ₁ u₁ = c (src/usymqr.jl:183-188)
  int start(double beta1, double gamma1, const double *r0, const double *c) {
    s.beta = beta1;
    s.gamma = gamma1;
    K(khip_fill(ctx, m, r.v_prev, 0.0));
    K(khip_fill(ctx, n, r.u_prev, 0.0));
    K(khip_divcopy(ctx, m, r.v, r0, s.beta));
    K(khip_divcopy(ctx, n, r.u, c, s.gamma));
    return KHIP_OK;
  }

  bool running() const { return !(P::stopped(s) || tired || user_exit || overtimed); }

  // q <- A uₖ and p <- Aᴴ vₖ (src/usymqr.jl:211-212)
  int products(const double *vk, const double *uk, double *qk, double *pk) {
    KHIP_TRY(apply_op_no_epilogue(ctx, A, uk, qk));
    KHIP_TRY(apply_op_no_epilogue(ctx, At, vk, pk));
    return KHIP_OK;
  }

  // path 0, the head of an iteration: the products and the step of the process up to the two norms (src/usymqr.jl:211-225)
  int primitive_head(int64_t k) {
    K(products(r.v, r.u, r.q, r.p));
    if (k >= 2) {
      K(khip_axpy(ctx, m, -s.gamma, r.v_prev, r.q));
      K(khip_axpy(ctx, n, -s.beta, r.u_prev, r.p));
    }
    double vq;
    K(khip_dot(ctx, m, r.v, r.q, &vq));
    P::step_a(s, vq);
    K(khip_axpy(ctx, m, -s.alpha, r.v, r.q));
    K(khip_axpy(ctx, n, -s.alpha, r.u, r.p));
    double qq, pp;
    K(khip_dot(ctx, m, r.q, r.q, &qq));                     // knorm is the square root of this sum
    K(khip_dot(ctx, n, r.p, r.p, &pp));
    P::step_b(s, qq, pp, k);
    return KHIP_OK;
  }
  // path 0: vₖ₋₁ <- vₖ ; uₖ₋₁ <- uₖ ; βₖ₊₁ ≠ 0 ? vₖ₊₁ = q / βₖ₊₁ ; γₖ₊₁ ≠ 0 ? uₖ₊₁ = p / γₖ₊₁ (src/usymqr.jl:309-317): two guards
  int shift() {
    K(khip_copy(ctx, m, r.v_prev, r.v));
    K(khip_copy(ctx, n, r.u_prev, r.u));
    if (s.beta_next != 0) K(khip_divcopy(ctx, m, r.v, r.q, s.beta_next));
    if (s.gamma_next != 0) K(khip_divcopy(ctx, n, r.u, r.p, s.gamma_next));
    return KHIP_OK;
  }

  void store_roles() {
    ws->v = r.v; ws->v_prev = r.v_prev; ws->u = r.u; ws->u_prev = r.u_prev;
    pol.store(ws);
  }

  // the end of an iteration on the host-driven loops (src/usymqr.jl:302-306, :337-343); the names follow the roles when the
  // callback runs
  void host_tail(int64_t k) {
    if (history) pol.push_history(ws, s);
    tired = k >= itmax;
    if (o.callback) store_roles();
    host_exit(ws, o, t0, timemax, &user_exit, &overtimed);
    if (kdisplay(k, o.verbose)) pol.verbose_row(o, k, s, t0);
  }

  // One of the three loops, from the state the set-up left in s, until the solver's tests, itmax, the callback or the time
  // limit end it (ws->box.path says which loop ran).  On return the roles are back in the workspace.
  int iterate() {
    tired = 0 >= itmax;
    const bool csr_pair = A->csr && !A->apply && At->csr && !At->apply;
    const int fused = square() ? o.fused : 0;              // m ≠ n: the primitive sequence, whatever options.fused says
    const bool device_loop = fused >= 2 && csr_pair && !o.callback && o.verbose <= 0;
    ws->box.path = (device_loop && running()) ? 2 : (fused ? 1 : 0);   // a loop that never starts reports 1, as the early returns do
    if (ws->box.path == 0) {
      // -------------------------------------------------------------- the reference's primitive sequence --------------
      while (running()) {
        const int64_t k = ++iter;
        pol.begin_iteration(s);
        K(primitive_head(k));
        K(pol.primitive_tail(*this, k));
        host_tail(k);
      }
    } else if (ws->box.path == 1) {
      // -------------------------------------------------------------- host-driven loop on the fused kernels -----------
      // The state goes up before iteration 1 and after each scalar step; P3 has no reduction, and nothing changes the state
      // between it and the next P1, so the staging copy is never rewritten while an upload may still read it.
      K(ws->loop.alloc());
      set_history(s, nullptr);
      if (running()) K(ws->loop.upload(ctx, s));
      while (running()) {
        const int64_t k = ++iter;
        pol.begin_iteration(s);
        K(products(r.v, r.u, r.q, r.p));
        int slot = take_slots(ctx, 1);
        K(launch_ssy_p1(ctx, n, ws->loop.dev, r.v_prev, r.u_prev, r.v, r.q, r.p, k == 1, slot));
        double vq;
        K(fetch_results(ctx, slot, 1, &vq));
        P::step_a(s, vq);
        K(ws->loop.upload(ctx, s));
        slot = take_slots(ctx, 2);
        K(launch_ssy_p2(ctx, n, ws->loop.dev, r.v, r.u, r.q, r.p, slot));
        double two[2];
        K(fetch_results(ctx, slot, 2, two));
        P::step_b(s, two[0], two[1], k);
        K(ws->loop.upload(ctx, s));
        K(pol.p3(ctx, n, ws->loop.dev, r, k));
        r.rotate();                                // vₖ₋₁ <- vₖ ; vₖ <- vₖ₊₁ as a rotation of the roles
        pol.rotate(k);
        host_tail(k);
      }
    } else {
      // -------------------------------------------------------------- device-resident loop ----------------------------
      SsyRoles d = r;                              // the roles as the host enqueues; r and pol stay where the loop began
      P dpol = pol;
      auto step = [&](State *dev, long long j) {
        const int64_t k = j + 1;
        KHIP_TRY(dev_pass(ctx, &dev->stop_seq, 4 * j + 1, EPI_NONE, nullptr, [&] {       // both products under one number
          const int rc = spmv_any(ctx, A->csr, d.u, d.q, -1);                            // q = A uₖ
          return rc != KHIP_OK ? rc : spmv_any(ctx, At->csr, d.v, d.p, -1); }));         // p = Aᴴ vₖ
        KHIP_TRY(dev_stage(ctx, dev, 4 * j + 2, P::kEpiA, 1, [&](int slot) {
          return launch_ssy_p1(ctx, n, dev, d.v_prev, d.u_prev, d.v, d.q, d.p, k == 1, slot); }));   // P1 ; v.q -> α
        KHIP_TRY(dev_stage(ctx, dev, 4 * j + 3, P::kEpiB, 2, [&](int slot) {
          return launch_ssy_p2(ctx, n, dev, d.v, d.u, d.q, d.p, slot); }));              // P2 ; (q.q, p.p) -> the solver's update and tests
        KHIP_TRY(dev_pass(ctx, &dev->stop_seq, 4 * j + 4, EPI_NONE, nullptr, [&] {
          return dpol.p3(ctx, n, dev, d, k); }));                                        // P3: also in the iteration that stops
        d.rotate();
        dpol.rotate(k);
        return (int)KHIP_OK;
      };
      K(ws->loop.run(ctx, s, device_loop_args(itmax, t0, timemax, history, {&ws->box.residuals, P::dual_history(ws)}), step, &s,
                     &overtimed));
      iter = s.iter;
      tired = iter >= itmax;
      r = replay(r, iter, 2, [](SsyRoles &b) { b.rotate(); });   // r stayed where the loop began
      pol.fix_after_device_loop(s);
    }
    store_roles();
    if (o.verbose > 0) { klogf(o.log_fd, "\n"); klog_flush(o.log_fd); }
    return KHIP_OK;
  }
};

}  // namespace
}  // namespace khip
