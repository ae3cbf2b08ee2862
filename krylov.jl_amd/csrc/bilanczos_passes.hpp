// bilanczos_passes.hpp -- the two passes of the two-sided Lanczos process that bilq! (bilq.cpp) and qmr! (qmr.cpp) share: the
// biorthogonalisation is the same in both, line for line (src/bilq.jl:234-252 = src/qmr.jl:238-258).  The kernels read γₖ, βₖ and αₖ
// from the common leading part of either solver's device state (BiLanczosCoef, solver_device.hpp); they keep the names they have
// had in traces since bilq! (bilq_p1_kernel, bilq_p2_kernel).
#pragma once

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

}  // namespace
}  // namespace khip
