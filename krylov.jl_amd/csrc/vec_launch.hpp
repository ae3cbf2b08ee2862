// vec_launch.hpp -- how a streaming vector kernel (blas1.hip and the solvers' fused passes) is launched, decided once.
//
// A kernel template<VEC, NT[, COMP]> moves 16 bytes per access when every vector is 16-byte aligned (VEC = 2; the odd tail
// element goes to one lane, owns_tail) and 8 otherwise, streams past the caches from tune.nt_min_elems on (NT), accumulates
// its dots compensated or plain (COMP), and runs LOOP-FREE on one workgroup per 256 * U accesses.  vec_plan takes that
// decision from the pointers and the two tune values alone -- it needs no device -- and vec_dispatch turns it into the
// kernel's instantiation.
#pragma once

#include <initializer_list>
#include <type_traits>

#include "device_reduce.hpp"

namespace khip {

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }   // (null counts as aligned)

inline bool use_nt(int64_t n, int nt_min_elems) { return n >= (int64_t)nt_min_elems; }

inline int64_t tiles_for(int64_t nvec, int u) {
  int64_t t = (nvec + (int64_t)kBlock * u - 1) / ((int64_t)kBlock * u);
  return t < 1 ? 1 : t;
}

// 16-byte accesses: at least one pair, every pointer aligned; extra_aligned speaks for pointers that are not in the list
// (a device table of vectors, checked where the table is built)
inline bool vec_pairs(int64_t n, std::initializer_list<const void *> ptrs, bool extra_aligned = true) {
  bool al = n >= 2 && extra_aligned;
  for (const void *p : ptrs) if (!aligned16(p)) al = false;
  return al;
}

struct VecPlan {
  int64_t g;            // workgroups of kBlock lanes; a reduction publishes g * kWavesPerBlock partials
  bool v2, nt, comp;
  dim3 grid() const { return dim3((unsigned)g); }
  int64_t waves() const { return g * kWavesPerBlock; }
};

// u: accesses per lane (4 for the long read-only reductions, else 1)
inline int vec_plan(int64_t n, std::initializer_list<const void *> ptrs, bool extra_aligned, int u, int nt_min_elems,
                    int compensated, VecPlan *L) {
  L->v2 = vec_pairs(n, ptrs, extra_aligned);
  L->nt = use_nt(n, nt_min_elems);
  L->comp = compensated != 0;
  L->g = tiles_for(L->v2 ? n / 2 : n, u);
  if (L->g > 0x7fffffffLL) { set_error("vector too long for one launch"); return KHIP_ERR_INVALID; }
  return KHIP_OK;
}
// ... from a context's tune values; a reduction of nout sums also gets its scratch for L->waves() partials
inline int vec_plan(khip_ctx *ctx, int64_t n, std::initializer_list<const void *> ptrs, VecPlan *L, int nout = 0,
                    bool extra_aligned = true, int u = 1) {
  KHIP_TRY(vec_plan(n, ptrs, extra_aligned, u, ctx->tune.nt_min_elems, ctx->tune.compensated, L));
  return nout > 0 ? ensure_reduction_scratch(ctx, L->waves(), nout) : KHIP_OK;
}

// Whether the 8-byte path has non-temporal instantiations.  blas1.hip has them and follows the plan; the solvers' fused passes
// (minres.cpp, lanczos_shift.cpp, bilq.cpp) never had.  Which is right for unaligned vectors of 4 M elements and more has
// not been measured, so both stay as they were, by name.
enum class ScalarPathNT { never, follow };

// The plan as integral constants, for hipLaunchKernelGGL((kernel<V, N, C>), ...): vec_dispatch_vn calls f(V, N) for a kernel
// without COMP, vec_dispatch f(V, N, C).  A kernel whose COMP comes first (blas1.hip's reductions) nests the two halves the
// other way round, vec_dispatch_comp outside, so that its instantiations stay in the order they have always had in the code
// object.  Only what a policy can reach is instantiated.
template <ScalarPathNT POLICY, class F>
inline void vec_dispatch_vn(const VecPlan &L, F &&f) {
  using V1 = std::integral_constant<int, 1>;
  using V2 = std::integral_constant<int, 2>;
  if (L.v2) {
    if (L.nt) f(V2{}, std::true_type{}); else f(V2{}, std::false_type{});
    return;
  }
  if constexpr (POLICY == ScalarPathNT::follow) {
    if (L.nt) { f(V1{}, std::true_type{}); return; }
  }
  f(V1{}, std::false_type{});
}
template <class F>
inline void vec_dispatch_comp(const VecPlan &L, F &&f) {
  if (L.comp) f(std::true_type{}); else f(std::false_type{});
}
template <ScalarPathNT POLICY, class F>
inline void vec_dispatch(const VecPlan &L, F &&f) {
  vec_dispatch_vn<POLICY>(L, [&](auto V, auto N) { vec_dispatch_comp(L, [&](auto C) { f(V, N, C); }); });
}

}  // namespace khip
