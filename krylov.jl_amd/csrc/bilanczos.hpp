// bilanczos.hpp -- what bilq! (bilq.cpp), qmr! (qmr.cpp) and bilqr! (bilqr.cpp) share: the two-sided Lanczos process and the
// three loops around it.
//
// The biorthogonalisation is the same in all three, line for line (src/bilq.jl:234-252 = src/qmr.jl:238-258 = src/bilqr.jl:227-238):
// P1 and P2 below.  The kernels read γₖ, βₖ and αₖ from the common leading part of a solver's device state (BiLanczosCoef,
// solver_device.hpp); they keep the names they have had in traces since bilq! (bilq_p1_kernel, bilq_p2_kernel).
//
// BiLanczos<P> is the driver: the argument and shape checks, the products, the path decision, the primitive sequence's head
// and shift (path 0), the host-driven loop on the fused kernels (path 1), the device-resident loop (path 2) and the end of a
// host-driven iteration.  A solver is a policy P (BiLanczosPolicy names what it may leave out): its device state and epilogue
// ids, its scalar steps, its P3 launch, the rotation of its own buffers, and its part of a primitive iteration.  Set-up and
// the termination status stay in the solver's file.  One template, resolved at compile time: nothing on the per-iteration
// path goes through a pointer to a function.
#pragma once

#include <utility>

#include "solver_host.hpp"
#include "vec_launch.hpp"

namespace khip {   // (named, not anonymous: stable kernel names in traces)

// Each thread owns one VEC-vector of every stream; the odd tail element (VEC = 2, n odd) goes to thread 0 of block 0.
// Cache hints, one rule: a load is non-temporal when it is the LAST read of that data (the vector is dead or overwritten
// afterwards); vₖ and uₖ are read again up to the next iteration's P1 (as vₖ₋₁, uₖ₋₁) and stay cacheable.  A store is non-temporal
// when nothing reads it before the next iteration's P3.

// P1: q = fma(-γ, v_prev, q) ; p = fma(-β, u_prev, p) ; acc = u . q                    (src/bilq.jl:244-247, src/qmr.jl:248-251)
template <int VEC, bool NT, bool COMP>
__global__ __launch_bounds__(kBlock) void bilq_p1_kernel(int64_t n, const BiLanczosCoef *st, const double *v_prev, const double *u_prev,
                                                        const double *u, double *q, double *p, RedArgs ra) {
  using T = typename VecT<VEC>::type;
  if (seq_skip(ra.stop_seq, ra.seq)) return;
  const double ng = -st->gamma, nb = -st->beta;
  dd acc[1] = {dd{0.0, 0.0}};
  const int64_t nvec = n / VEC;
  const int64_t i = lane_index();
  if (i < nvec) {
    const T qv = ldg<NT>(reinterpret_cast<const T *>(q) + i);
    const T pv = ldg<NT>(reinterpret_cast<const T *>(p) + i);
    const T vp = ldg<NT>(reinterpret_cast<const T *>(v_prev) + i);
    const T up = ldg<NT>(reinterpret_cast<const T *>(u_prev) + i);
    const T uv = ldg<false>(reinterpret_cast<const T *>(u) + i);       // u is read again by P2
    T qo, po;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const double qn = fma(ng, vget(vp, e), vget(qv, e));
      vset(qo, e, qn);
      vset(po, e, fma(nb, vget(up, e), vget(pv, e)));
      acc_prod<COMP>(acc[0], vget(uv, e), qn);
    }
    stg<false>(qo, reinterpret_cast<T *>(q) + i);                       // q, p are read again by P2
    stg<false>(po, reinterpret_cast<T *>(p) + i);
  }
  if (VEC == 2 && owns_tail(n)) {
    const int64_t t = n - 1;
    const double qn = fma(ng, v_prev[t], q[t]);
    q[t] = qn;
    p[t] = fma(nb, u_prev[t], p[t]);
    acc_prod<COMP>(acc[0], u[t], qn);
  }
  wave_publish<1>(acc, ra);
}

// P2: q = fma(-α, v, q) ; p = fma(-α, u, p) ; acc = p . q                              (src/bilq.jl:249-252, src/qmr.jl:253-256)
template <int VEC, bool NT, bool COMP>
__global__ __launch_bounds__(kBlock) void bilq_p2_kernel(int64_t n, const BiLanczosCoef *st, const double *v, const double *u, double *q,
                                                        double *p, RedArgs ra) {
  using T = typename VecT<VEC>::type;
  if (seq_skip(ra.stop_seq, ra.seq)) return;
  const double na = -st->alpha;
  dd acc[1] = {dd{0.0, 0.0}};
  const int64_t nvec = n / VEC;
  const int64_t i = lane_index();
  if (i < nvec) {
    const T qv = ldg<NT>(reinterpret_cast<const T *>(q) + i);
    const T pv = ldg<NT>(reinterpret_cast<const T *>(p) + i);
    const T vv = ldg<false>(reinterpret_cast<const T *>(v) + i);       // v is read again by P3 and the next P1
    const T uv = ldg<false>(reinterpret_cast<const T *>(u) + i);       // u is the next iteration's u_prev
    T qo, po;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const double qn = fma(na, vget(vv, e), vget(qv, e));
      const double pn = fma(na, vget(uv, e), vget(pv, e));
      vset(qo, e, qn);
      vset(po, e, pn);
      acc_prod<COMP>(acc[0], pn, qn);
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
    acc_prod<COMP>(acc[0], pn, qn);
  }
  wave_publish<1>(acc, ra);
}

namespace {   // each solver file gets its own copy of the launchers, as of everything in solver_host.hpp

int launch_p1(khip_ctx *ctx, int64_t n, const BiLanczosCoef *st, const double *v_prev, const double *u_prev, const double *u, double *q,
              double *p, int slot) {
  VecPlan L;
  KHIP_TRY(vec_plan(ctx, n, {v_prev, u_prev, u, q, p}, &L, 1));
  RedArgs ra = make_red_args(ctx, slot);
  vec_dispatch<ScalarPathNT::never>(L, [&](auto V, auto N, auto C) {
    hipLaunchKernelGGL((bilq_p1_kernel<V, N, C>), L.grid(), dim3(kBlock), 0, ctx->stream, n, st, v_prev, u_prev, u, q, p, ra); });
  KHIP_CHECK_HIP(hipGetLastError());
  return launch_finish(ctx, L.waves(), 1, slot);
}
int launch_p2(khip_ctx *ctx, int64_t n, const BiLanczosCoef *st, const double *v, const double *u, double *q, double *p, int slot) {
  VecPlan L;
  KHIP_TRY(vec_plan(ctx, n, {v, u, q, p}, &L, 1));
  RedArgs ra = make_red_args(ctx, slot);
  vec_dispatch<ScalarPathNT::never>(L, [&](auto V, auto N, auto C) {
    hipLaunchKernelGGL((bilq_p2_kernel<V, N, C>), L.grid(), dim3(kBlock), 0, ctx->stream, n, st, v, u, q, p, ra); });
  KHIP_CHECK_HIP(hipGetLastError());
  return launch_finish(ctx, L.waves(), 1, slot);
}

// the six vectors of the process by their CURRENT role: the fused loops rotate (v_prev, v) and (u_prev, u) where the reference
// copies (vₖ₊₁ and uₖ₊₁ are written where vₖ₋₁ and uₖ₋₁ were)
struct BiLanczosRoles {
  double *v, *v_prev, *u, *u_prev, *q, *p;
  void rotate() { std::swap(v, v_prev); std::swap(u, u_prev); }
};

// What a policy may leave out.  It must supply: State (a BiLanczosCoef with beta_next, gamma_next, iter and the DeviceLoop
// fields), Workspace, kEpiA / kEpiB / kEpiC, kP3Sums, step_a(s, uq), step_b(s, pq, k), step_c(s, sums, k) (the fetched sums as
// they are: the policy takes the square roots), stopped(s), p3(ctx, n, dev, roles, k, slot), push_history(ws, s),
// verbose_row(o, k, s, t0) and primitive_tail(driver, k, pq): what the reference does between its p.q and the end of the
// iteration, on the primitives, with driver.shift(pq) where the reference has its kcopy! / kdivcopy! of v and u.
template <class S, class W>
struct BiLanczosPolicy {
  using State = S;
  using Workspace = W;
  void begin_iteration(const S &) {}                       // host-driven loops: before the products of an iteration
  int fused_start(khip_ctx *, int64_t, const BiLanczosRoles &, S &) { return KHIP_OK; }   // before a fused loop that will run
  void rotate(int64_t /*k*/, bool /*host_driven*/) {}     // the policy's own buffers, after P3 of iteration k
  void fix_after_device_loop(const S &) {}                 // ... which the host rotated once per ENQUEUED iteration
  void store(W *) const {}                                 // the roles of its own buffers back into the workspace
  static std::vector<double> *dual_history(W *) { return nullptr; }   // a second history stream of the device loop
};

template <class P>
struct BiLanczos {
  using State = typename P::State;
  using W = typename P::Workspace;
  W *const ws;
  khip_ctx *const ctx;
  const khip_operator *const A, *const At, *const M, *const N, *const Mt, *const Nt;
  const khip_options o;
  const double t0 = now_s(), timemax;
  const int64_t n;
  const bool history;
  double *t = nullptr, *s_tmp = nullptr;                    // products with M / N pass through them (the workspace's t and s)
  int64_t itmax = 0, iter = 0;
  bool tired = false, user_exit = false, overtimed = false;
  BiLanczosRoles r;
  State s;
  P pol;

  BiLanczos(W *ws_, const khip_operator *A_, const khip_operator *At_, const khip_operator *M_, const khip_operator *N_,
            const khip_operator *Mt_, const khip_operator *Nt_, const khip_options *opts)
      : ws(ws_), ctx(ws_->ctx), A(A_), At(At_), M(M_), N(N_), Mt(Mt_ ? Mt_ : M_), Nt(Nt_ ? Nt_ : N_),
        o(opts ? *opts : khip_default_options()), timemax(timemax_of(o)), n(ws_->n), history(o.history != 0),
        r{ws_->v, ws_->v_prev, ws_->u, ws_->u_prev, ws_->q, ws_->p} {
    memset(&s, 0, sizeof(s));
    (void)take_alloc_seconds();
  }

  // At, a solver's own required argument (`missing`: its message, or null) and the shapes (src/bilq.jl:124-126)
  int check(const char *solver, const char *square, const char *missing = nullptr) {
    char msg[160];
    snprintf(msg, sizeof(msg), "%s_solve: At (the adjoint of A) is required", solver);
    if (!At) return ws->box.fail(KHIP_ERR_INVALID, msg);
    if (missing) return ws->box.fail(KHIP_ERR_INVALID, missing);
    if (int rc = check_shape(ws, {A, At})) return rc;
    if (ws->m != ws->n) return ws->box.fail(KHIP_ERR_INVALID, square);
    return KHIP_OK;
  }

  // bilq!, qmr!: t and s, which M and N need, allocated on first need (src/bilq.jl:145-146)
  int allocate_ts() {
    if (M && !ws->t) K(alloc_vec(ctx, n, &ws->t));
    if (N && !ws->s) K(alloc_vec(ctx, n, &ws->s));
    t = ws->t;
    s_tmp = ws->s;
    return KHIP_OK;
  }
  // bilq!, qmr!: *r0 = M (b - A Δx), held in t or q where it is not b itself (src/bilq.jl:158-169)
  int residual(const double *b, bool warm_start, const double **r0) {
    *r0 = b;
    if (warm_start) {
      K(residual0(ws, A, 0.0, b, true, r.q));
      *r0 = r.q;
    }
    if (M) {
      K(apply_op(ctx, M, *r0, t));
      *r0 = t;
    }
    return KHIP_OK;
  }
  // bilq!, qmr!: x <- N x + Δx and the stats (src/bilq.jl:393-406); `early`: a return before the loops, which leaves N alone
  int end(int solved, const char *status, bool warm_start, bool early = false) {
    if (N && !early) {
      K(khip_copy(ctx, n, s_tmp, ws->x));
      K(apply_op(ctx, N, s_tmp, ws->x));
    }
    return ws_end(ws, {iter, solved, 0, status, warm_start, t0, false});
  }

  // βₖ, γₖ from cᴴr₀ and the first Lanczos vectors (src/bilq.jl:204-209)
  int start(double cb, const double *r0, const double *c0) {
    s.beta = std::sqrt(std::fabs(cb));
    s.gamma = cb / s.beta;
    K(khip_fill(ctx, n, r.v_prev, 0.0));
    K(khip_fill(ctx, n, r.u_prev, 0.0));
    K(khip_divcopy(ctx, n, r.v, r0, s.beta));
    K(khip_divcopy(ctx, n, r.u, c0, s.gamma));
    return KHIP_OK;
  }

  bool running() const { return !(P::stopped(s) || tired || user_exit || overtimed); }

  // q <- M A N v and p <- N' A' M' u (src/bilq.jl:234-242)
  int products(const double *vk, const double *uk, double *qk, double *pk) {
    if (N) KHIP_TRY(apply_op_no_epilogue(ctx, N, vk, s_tmp));
    KHIP_TRY(apply_op_no_epilogue(ctx, A, N ? s_tmp : vk, M ? t : qk));
    if (M) KHIP_TRY(apply_op_no_epilogue(ctx, M, t, qk));
    if (M) KHIP_TRY(apply_op_no_epilogue(ctx, Mt, uk, t));
    KHIP_TRY(apply_op_no_epilogue(ctx, At, M ? t : uk, N ? s_tmp : pk));
    if (N) KHIP_TRY(apply_op_no_epilogue(ctx, Nt, s_tmp, pk));
    return KHIP_OK;
  }

  // path 0, the head of an iteration: the products and the two-sided Lanczos step up to pᴴq (src/bilq.jl:234-252)
  int primitive_head(int64_t k, double *pq) {
    K(products(r.v, r.u, r.q, r.p));
    K(khip_axpy(ctx, n, -s.gamma, r.v_prev, r.q));
    K(khip_axpy(ctx, n, -s.beta, r.u_prev, r.p));
    double uq;
    K(khip_dot(ctx, n, r.u, r.q, &uq));
    P::step_a(s, uq);
    K(khip_axpy(ctx, n, -s.alpha, r.v, r.q));
    K(khip_axpy(ctx, n, -s.alpha, r.u, r.p));
    K(khip_dot(ctx, n, r.p, r.q, pq));
    P::step_b(s, *pq, k);
    return KHIP_OK;
  }
  // path 0: vₖ₋₁ <- vₖ ; uₖ₋₁ <- uₖ ; pᴴq ≠ 0 ? (vₖ₊₁ = q / βₖ₊₁ ; uₖ₊₁ = p / γₖ₊₁) (src/bilq.jl:325-333).  The references take their
  // reductions at different places around it, so primitive_tail calls it.
  int shift(double pq) {
    K(khip_copy(ctx, n, r.v_prev, r.v));
    K(khip_copy(ctx, n, r.u_prev, r.u));
    if (pq != 0) {
      K(khip_divcopy(ctx, n, r.v, r.q, s.beta_next));
      K(khip_divcopy(ctx, n, r.u, r.p, s.gamma_next));
    }
    return KHIP_OK;
  }

  // the end of an iteration on the host-driven loops (src/bilq.jl:347, :367-374)
  void host_tail(int64_t k) {
    if (history) pol.push_history(ws, s);
    tired = k >= itmax;
    host_exit(ws, o, t0, timemax, &user_exit, &overtimed);
    if (kdisplay(k, o.verbose)) pol.verbose_row(o, k, s, t0);
  }

  // One of the three loops, from the state the set-up left in s, until the solver's tests, itmax, the callback or the time
  // limit end it (ws->box.path says which loop ran).  On return the roles are back in the workspace.
  int iterate() {
    tired = 0 >= itmax;
    const bool csr_pair = A->csr && !A->apply && At->csr && !At->apply;
    const bool device_loop = o.fused >= 2 && csr_pair && !M && !N && !o.callback && o.verbose <= 0;
    ws->box.path = (device_loop && running()) ? 2 : (o.fused ? 1 : 0);   // a loop that never starts reports 1, as the early returns do
    if (ws->box.path == 0) {
      // -------------------------------------------------------------- the reference's primitive sequence --------------
      while (running()) {
        const int64_t k = ++iter;
        pol.begin_iteration(s);
        double pq;
        K(primitive_head(k, &pq));
        K(pol.primitive_tail(*this, k, pq));
        host_tail(k);
      }
    } else if (ws->box.path == 1) {
      // -------------------------------------------------------------- host-driven loop on the fused kernels -----------
      K(ws->loop.alloc());
      set_history(s, nullptr);
      if (running()) K(pol.fused_start(ctx, n, r, s));
      while (running()) {
        const int64_t k = ++iter;
        pol.begin_iteration(s);
        K(products(r.v, r.u, r.q, r.p));
        K(ws->loop.upload(ctx, s));
        int slot = take_slots(ctx, 1);
        K(launch_p1(ctx, n, ws->loop.dev, r.v_prev, r.u_prev, r.u, r.q, r.p, slot));
        double uq;
        K(fetch_results(ctx, slot, 1, &uq));
        P::step_a(s, uq);
        K(ws->loop.upload(ctx, s));
        slot = take_slots(ctx, 1);
        K(launch_p2(ctx, n, ws->loop.dev, r.v, r.u, r.q, r.p, slot));
        double pq;
        K(fetch_results(ctx, slot, 1, &pq));
        P::step_b(s, pq, k);
        K(ws->loop.upload(ctx, s));
        slot = take_slots(ctx, P::kP3Sums);
        K(pol.p3(ctx, n, ws->loop.dev, r, k, slot));
        double sums[P::kP3Sums];
        K(fetch_results(ctx, slot, P::kP3Sums, sums));
        r.rotate();                                // vₖ₋₁ <- vₖ ; vₖ <- vₖ₊₁ as a rotation of the roles
        pol.rotate(k, true);
        P::step_c(s, sums, k);
        host_tail(k);
      }
    } else {
      // -------------------------------------------------------------- device-resident loop ----------------------------
      K(pol.fused_start(ctx, n, r, s));
      BiLanczosRoles d = r;                        // the roles as the host enqueues; r and pol stay where the loop began
      P dpol = pol;
      auto step = [&](State *dev, long long j) {
        const int64_t k = j + 1;
        KHIP_TRY(dev_pass(ctx, &dev->stop_seq, 4 * j + 1, EPI_NONE, nullptr, [&] {       // both products under one number
          const int rc = spmv_any(ctx, A->csr, d.v, d.q, -1);                            // q = A vₖ
          return rc != KHIP_OK ? rc : spmv_any(ctx, At->csr, d.u, d.p, -1); }));         // p = A' uₖ
        KHIP_TRY(dev_stage(ctx, dev, 4 * j + 2, P::kEpiA, 1, [&](int slot) {
          return launch_p1(ctx, n, dev, d.v_prev, d.u_prev, d.u, d.q, d.p, slot); }));   // P1 ; u.q -> α
        KHIP_TRY(dev_stage(ctx, dev, 4 * j + 3, P::kEpiB, 1, [&](int slot) {
          return launch_p2(ctx, n, dev, d.v, d.u, d.q, d.p, slot); }));                  // P2 ; p.q -> the solver's update
        KHIP_TRY(dev_stage(ctx, dev, 4 * j + 4, P::kEpiC, P::kP3Sums, [&](int slot) {
          return dpol.p3(ctx, n, dev, d, k, slot); }));                                  // P3 ; its sums -> the tests
        d.rotate();
        dpol.rotate(k, false);
        return (int)KHIP_OK;
      };
      K(ws->loop.run(ctx, s, device_loop_args(itmax, t0, timemax, history, {&ws->box.residuals, P::dual_history(ws)}), step, &s,
                     &overtimed));
      iter = s.iter;
      tired = iter >= itmax;
      r = replay(r, iter, 2, [](BiLanczosRoles &b) { b.rotate(); });   // r stayed where the loop began
      pol.fix_after_device_loop(s);
    }
    ws->v = r.v; ws->v_prev = r.v_prev; ws->u = r.u; ws->u_prev = r.u_prev;
    pol.store(ws);
    if (o.verbose > 0) klogf(o.log_fd, "\n");
    return KHIP_OK;
  }

  // the end of every solve that got past the checks
  void finish() {
    ws->warm_start = false;
    ws_finish(ws, t0);
  }
};

}  // namespace
}  // namespace khip
