// bilqr.cpp -- bilqr! (src/bilqr.jl:116-484) above the device primitives, with its fused gfx950 kernels.
//
// Real Float64.  ONE two-sided Lanczos process advances the BiLQ iterate of A x = b (with the BiCG transfer) and the QMR iterate of
// Aᴴ y = c.  Three loops, chosen as for bilq! and qmr! (khip_bilqr_last_path):
//   0  options.fused = 0: the reference's primitive sequence, one launch per k* call, one host sync per kdot / knorm / kdotr;
//   1  the host-driven loop on the fused kernels (a user operator, a callback or verbose > 0);
//   2  the device-resident loop (default; A and A' both CSR handles): the scalar recurrences and stopping tests run as the
//      epilogues of the three reductions of an iteration (bilqr_step_a/b/c, solver_device.hpp), iterations are enqueued ahead.
// One iteration on the fused paths, after q = A vₖ and p = A' uₖ, with both sides unsolved:
//   P1   q = fma(-γₖ, vₖ₋₁, q) ; p = fma(-βₖ, uₖ₋₁, p) ; uₖ.q                          (bilanczos_passes.hpp)      56n bytes
//   P2   q = fma(-αₖ, vₖ, q) ; p = fma(-αₖ, uₖ, p) ; p.q                               (bilanczos_passes.hpp)      48n bytes
//   P3   x = fma(ζₖ₋₁sₖ, vₖ, fma(ζₖ₋₁cₖ, d̅, x)) ; d̅ = fma(-cₖ, vₖ, sₖ d̅) ;
//        wₖ₋₁ = (uₖ₋₁ - λₖ₋₂ wₖ₋₂ - ϵₖ₋₃ wₖ₋₃) / δₖ₋₁ ; y = fma(ψₖ₋₁, wₖ₋₁, y) ;
//        vₖ₊₁ = q / βₖ₊₁ ; uₖ₊₁ = p / γₖ₊₁ ; vₖ.q ; q.q ; uₖ₊₁.uₖ₊₁                                                 120n bytes
//        reads  x, d̅, vₖ, q, p, uₖ₋₁, wₖ₋₃, wₖ₋₂, y (9) ; writes x, d̅, vₖ₊₁, uₖ₊₁, wₖ₋₁, y (6)
// 224n against 400n for the primitive sequence; a side that is solved drops its streams (primal: x, d̅ read and written, 32n; dual:
// uₖ₋₁, wₖ₋₃, wₖ₋₂, y read, wₖ₋₁, y written, 48n).  kcopy!(vₖ₋₁, vₖ), kcopy!(uₖ₋₁, uₖ) and @kswap!(wₖ₋₃, wₖ₋₂) become rotations of the
// buffers' roles (vₖ₊₁ and uₖ₊₁ are written where vₖ₋₁ and uₖ₋₁ were, wₖ₋₁ where wₖ₋₃ was).  Every elementwise value uses the
// expression of the primitive it replaces (fma for kaxpy!, fma(a, x, b y) for kaxpby!, a x for kscal!, x (1 / a) for kdiv!, / for
// kdivcopy!): the fused loops agree with the primitive sequence bit for bit on elementwise values and to the reductions' one ulp
// otherwise; loops 1 and 2 run the same kernels and the same scalar code and produce the same bits.
// The primal estimates need ⟨vₖ, q⟩ / βₖ₊₁ and ‖q‖ / βₖ₊₁ (:314-315, unlike bilq!, which reads vₖ₊₁): P3 sums vₖ.q and q.q and the
// scalar step divides, so that βₖ₊₁ = 0 gives the reference's NaN.  ‖uₖ₊₁‖² is the third sum: the scalar step keeps it and adds it to
// τ in the NEXT iteration (:398), as qmr! carries ‖vₖ₊₁‖²; ‖u₁‖² comes from one dot at set-up.  The finish kernel exists for 1, 2 and
// 4 sums: a fourth, zero, is published beside the three.
#include <chrono>
#include <string>
#include <utility>

#include "bilanczos_passes.hpp"   // P1, P2 and their launchers, shared with bilq.cpp and qmr.cpp

using namespace khip;

namespace khip {   // (named, not anonymous: stable kernel names in traces)

// ---------------------------------------------------------------------------------------------------------- kernels ----
// Each thread owns one VEC-vector of every stream; the odd tail element (VEC = 2, n odd) goes to thread 0 of block 0.
// Cache hints, the rule of bilq.cpp: a load is non-temporal when it is the LAST read of that data (x, d̅, y, wₖ₋₃, uₖ₋₁, q, p:
// overwritten here or by the next products); vₖ is read again by the next P1 (as vₖ₋₁) and wₖ₋₂ by the next P3 (as wₖ₋₃): they stay
// cacheable.  A store is non-temporal when nothing reads it before the next iteration's P3 (x, d̅, y, wₖ₋₁); vₖ₊₁ and uₖ₊₁ are read
// by the next products.

// wₖ₋₁ of one element (:363-381).  stage 2: kdivcopy!(w, u₁, δ₁).  stage 3: kaxpy!(1, uₖ₋₁, w₃) ; kaxpy!(-λ, w₂, w₃) ; kdiv!(w₃, δ).
// stage >= 4: kscal!(-ϵ, w₃) first.  (The +uₖ₋₁ axpy comes BEFORE the -λ axpy here, the other way round from qmr!.)
__device__ __forceinline__ double bilqr_w(int stage, double up, double w2, double w3, double ne, double nl, double dl, double idl) {
  if (stage == 2) return up / dl;
  double t = stage >= 4 ? ne * w3 : w3;
  t = fma(1.0, up, t);
  t = fma(nl, w2, t);
  return t * idl;
}

// P3 (:296-311, :361-392, :410-418).  primal (the primal system was unsolved when the iteration began): stage == 1 ? d̅ = v :
// (x = fma(ζs, v, fma(ζc, d̅, x)) ; d̅ = fma(-c, v, s d̅)) ; acc0 = v . q ; acc1 = q . q.  dual, from stage 2 on: w_out = wₖ₋₁
// (bilqr_w) ; y = fma(ψ, wₖ₋₁, y).  Always: pᴴq ≠ 0 ? (v_next = q / βₖ₊₁ ; u_next = p / γₖ₊₁) : (v_next = v ; u_next = u) ;
// acc2 = u_next . u_next.  The branches are uniform (device state and a kernel argument); a side that is off loads and stores
// nothing of its streams.  w_out is w2 at stage 2 and w3 afterwards.  u_next MAY BE u_prev's buffer (it is, in the loops below):
// every thread reads its elements of u_prev before it writes u_next.
template <int VEC, bool NT, bool COMP>
__global__ __launch_bounds__(kBlock) void bilqr_p3_kernel(int64_t n, const BilqrDevState *st, double *x, double *dbar, double *y,
                                                         const double *w3, const double *w2, double *w_out, const double *v,
                                                         const double *u, const double *u_prev, const double *q, const double *p,
                                                         double *v_next, double *u_next, int stage, RedArgs ra) {
  using T = typename VecT<VEC>::type;
  if (seq_skip(ra.stop_seq, ra.seq)) return;
  const double zc = st->zc, zs = st->zs, nc = st->neg_c, sn = st->sn, bn = st->beta_next, gn = st->gamma_next;
  const double ne = st->neg_eps3, nl = st->neg_lambda2, dl = st->delta, idl = st->inv_delta, psi = st->psi;
  const bool divide = st->pq != 0.0;
  const bool primal = !st->solved_primal;
  const bool dual = !st->solved_dual && stage >= 2;
  dd acc[4] = {dd{0.0, 0.0}, dd{0.0, 0.0}, dd{0.0, 0.0}, dd{0.0, 0.0}};
  const int64_t nvec = n / VEC;
  const int64_t i = lane_index();
  if (i < nvec) {
    T vv = {}, qv = {};
    if (primal || !divide) vv = ldg<false>(reinterpret_cast<const T *>(v) + i);       // v is the next iteration's v_prev
    if (primal || divide) qv = ldg<NT>(reinterpret_cast<const T *>(q) + i);
    if (primal) {
      T dv;
      if (stage == 1) {
        dv = vv;
      } else {
        const T xv = ldg<NT>(reinterpret_cast<const T *>(x) + i);
        const T dd_ = ldg<NT>(reinterpret_cast<const T *>(dbar) + i);
        T xo;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          vset(xo, e, fma(zs, vget(vv, e), fma(zc, vget(dd_, e), vget(xv, e))));
          vset(dv, e, fma(nc, vget(vv, e), sn * vget(dd_, e)));
        }
        stg<NT>(xo, reinterpret_cast<T *>(x) + i);
      }
      stg<NT>(dv, reinterpret_cast<T *>(dbar) + i);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        acc_prod<COMP>(acc[0], vget(vv, e), vget(qv, e));
        acc_prod<COMP>(acc[1], vget(qv, e), vget(qv, e));
      }
    }
    if (dual) {
      const T upv = ldg<NT>(reinterpret_cast<const T *>(u_prev) + i);   // overwritten below (u_next)
      const T yv = ldg<NT>(reinterpret_cast<const T *>(y) + i);
      T w3v = {}, w2v = {};
      if (stage >= 3) {
        w3v = ldg<NT>(reinterpret_cast<const T *>(w3) + i);
        w2v = ldg<false>(reinterpret_cast<const T *>(w2) + i);         // wₖ₋₂ is the next iteration's wₖ₋₃
      }
      T wo, yo;
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const double w = bilqr_w(stage, vget(upv, e), vget(w2v, e), vget(w3v, e), ne, nl, dl, idl);
        vset(wo, e, w);
        vset(yo, e, fma(psi, w, vget(yv, e)));
      }
      stg<NT>(wo, reinterpret_cast<T *>(w_out) + i);
      stg<NT>(yo, reinterpret_cast<T *>(y) + i);
    }
    T vo, uo;
    if (divide) {
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
    for (int e = 0; e < VEC; ++e) acc_prod<COMP>(acc[2], vget(uo, e), vget(uo, e));
    stg<false>(vo, reinterpret_cast<T *>(v_next) + i);                  // read by the next products
    stg<false>(uo, reinterpret_cast<T *>(u_next) + i);
  }
  if (VEC == 2 && owns_tail(n)) {
    const int64_t t = n - 1;
    const double ve = v[t], qe = q[t];
    if (primal) {
      if (stage == 1) {
        dbar[t] = ve;
      } else {
        const double de = dbar[t];
        x[t] = fma(zs, ve, fma(zc, de, x[t]));
        dbar[t] = fma(nc, ve, sn * de);
      }
      acc_prod<COMP>(acc[0], ve, qe);
      acc_prod<COMP>(acc[1], qe, qe);
    }
    if (dual) {
      const double w = bilqr_w(stage, u_prev[t], stage >= 3 ? w2[t] : 0.0, stage >= 3 ? w3[t] : 0.0, ne, nl, dl, idl);
      w_out[t] = w;
      y[t] = fma(psi, w, y[t]);
    }
    const double vo = divide ? qe / bn : ve;
    const double uo = divide ? p[t] / gn : u[t];
    v_next[t] = vo;
    u_next[t] = uo;
    acc_prod<COMP>(acc[2], uo, uo);
  }
  wave_publish<4>(acc, ra);
}

}  // namespace khip

namespace {

constexpr ScalarPathNT kScalarNT = ScalarPathNT::never;
constexpr int kP3Sums = 4;         // vₖ.q, q.q, uₖ₊₁.uₖ₊₁ and a zero: the finish kernel has no three-sum form

int launch_p3(khip_ctx *ctx, int64_t n, const BilqrDevState *st, double *x, double *dbar, double *y, const double *w3, const double *w2,
              double *w_out, const double *v, const double *u, const double *u_prev, const double *q, const double *p, double *v_next,
              double *u_next, int stage, int slot) {
  VecPlan L;
  KHIP_TRY(vec_plan(ctx, n, {x, dbar, y, w3, w2, w_out, v, u, u_prev, q, p, v_next, u_next}, &L, kP3Sums));
  RedArgs ra = make_red_args(ctx, slot);
  vec_dispatch<kScalarNT>(L, [&](auto V, auto N, auto C) {
    hipLaunchKernelGGL((bilqr_p3_kernel<V, N, C>), L.grid(), dim3(kBlock), 0, ctx->stream, n, st, x, dbar, y, w3, w2, w_out, v, u,
                       u_prev, q, p, v_next, u_next, stage, ra); });
  KHIP_CHECK_HIP(hipGetLastError());
  return launch_finish(ctx, L.waves(), kP3Sums, slot);
}

}  // namespace

struct khip_bilqr_workspace {
  khip_ctx *ctx;
  int64_t m, n;
  // by their CURRENT role: the fused loops rotate (v_prev, v), (u_prev, u) and (w_prev3, w_prev2)
  double *u_prev = nullptr, *u = nullptr, *q = nullptr, *v_prev = nullptr, *v = nullptr, *p = nullptr, *x = nullptr, *y = nullptr,
         *dbar = nullptr, *w_prev3 = nullptr, *w_prev2 = nullptr, *dx = nullptr, *dy = nullptr;
  Borrowed borrowed;                        // the caller's vectors (khip_bilqr_workspace_adopt*): never freed here
  bool warm_start = false;
  StatsBox box;                             // box.residuals: the primal history
  std::vector<double> residuals_dual;
  std::string status;                       // the full status: four of the reference's strings do not fit khip_stats.status
  int solved_primal = 0, solved_dual = 0;
  DeviceLoop<BilqrDevState, 3> loop;        // fused loops: device copy of the scalar state, pinned snapshots + staging, histories
};

namespace {

// "%7s" of the reference pads characters; ✗ ✗ ✗ ✗ is seven of them                                        (src/bilqr.jl:439-441)
const char *const kCrosses = "\xe2\x9c\x97 \xe2\x9c\x97 \xe2\x9c\x97 \xe2\x9c\x97";

void verbose_row(const khip_options &o, long long iter, const BilqrDevState &s, double t0) {
  if (s.solved_primal && !s.solved_dual) klogf(o.log_fd, "%5lld  %s  %7.1e  %.2fs\n", iter, kCrosses, s.sNorm, now_s() - t0);
  if (!s.solved_primal && s.solved_dual) klogf(o.log_fd, "%5lld  %7.1e  %s  %.2fs\n", iter, s.rNorm_lq, kCrosses, now_s() - t0);
  if (!s.solved_primal && !s.solved_dual) klogf(o.log_fd, "%5lld  %7.1e  %7.1e  %.2fs\n", iter, s.rNorm_lq, s.sNorm, now_s() - t0);
}

// the first bytes of `full` that fit `cap` (with the terminator), cut at a UTF-8 character boundary
void copy_status(char *dst, size_t cap, const std::string &full) {
  size_t len = std::min(full.size(), cap - 1);
  while (len > 0 && len < full.size() && (static_cast<unsigned char>(full[len]) & 0xC0) == 0x80) --len;
  memcpy(dst, full.data(), len);
  dst[len] = 0;
}

// the termination status (:451-469); XL / XC: "xᴸ" / "xᶜ"
#define XL "x\xe1\xb4\xb8"
#define XC "x\xe1\xb6\x9c"
const char *status_of(const BilqrDevState &s, bool tired, bool user_exit, bool overtimed) {
  const char *status = "unknown";
  if (tired) status = "maximum number of iterations exceeded";
  if (s.breakdown) status = "Breakdown \xe2\x9f\xa8u\xe2\x82\x96\xe2\x82\x8a\xe2\x82\x81,v\xe2\x82\x96\xe2\x82\x8a\xe2\x82\x81\xe2\x9f\xa9 = 0";
  if (s.solved_lq_tol && !s.solved_dual) status = "Only the primal solution " XL " is good enough given atol and rtol";
  if (s.solved_cg_tol && !s.solved_dual) status = "Only the primal solution " XC " is good enough given atol and rtol";
  if (!s.solved_primal && s.solved_qr_tol) status = "Only the dual solution t is good enough given atol and rtol";
  if (s.solved_lq_tol && s.solved_qr_tol) status = "Both primal and dual solutions (" XL ", t) are good enough given atol and rtol";
  if (s.solved_cg_tol && s.solved_qr_tol) status = "Both primal and dual solutions (" XC ", t) are good enough given atol and rtol";
  if (s.solved_lq_mach && !s.solved_dual) status = "Only found approximate zero-residual primal solution " XL;
  if (s.solved_cg_mach && !s.solved_dual) status = "Only found approximate zero-residual primal solution " XC;
  if (!s.solved_primal && s.solved_qr_mach) status = "Only found approximate zero-residual dual solution t";
  if (s.solved_lq_mach && s.solved_qr_mach) status = "Found approximate zero-residual primal and dual solutions (" XL ", t)";
  if (s.solved_cg_mach && s.solved_qr_mach) status = "Found approximate zero-residual primal and dual solutions (" XC ", t)";
  if (s.solved_lq_mach && s.solved_qr_tol)
    status = "Found approximate zero-residual primal solutions " XL " and a dual solution t good enough given atol and rtol";
  if (s.solved_cg_mach && s.solved_qr_tol)
    status = "Found approximate zero-residual primal solutions " XC " and a dual solution t good enough given atol and rtol";
  if (s.solved_lq_tol && s.solved_qr_mach)
    status = "Found a primal solution " XL " good enough given atol and rtol and an approximate zero-residual dual solutions t";
  if (s.solved_cg_tol && s.solved_qr_mach)
    status = "Found a primal solution " XC " good enough given atol and rtol and an approximate zero-residual dual solutions t";
  if (user_exit) status = "user-requested exit";
  if (overtimed) status = "time limit exceeded";
  return status;
}
#undef XL
#undef XC

}  // namespace

extern "C" {

khip_bilqr_params khip_bilqr_default_params(void) {
  khip_bilqr_params p;
  p.transfer_to_bicg = 1;
  return p;
}

int khip_bilqr_workspace_create(khip_ctx *ctx, int64_t m, int64_t n, khip_bilqr_workspace **out) {
  KHIP_REQUIRE(ctx && out && m >= 0 && n >= 0, "bilqr_workspace_create: bad argument");
  KHIP_REQUIRE(m == n, "Systems must be square");
  khip_bilqr_workspace *ws = new khip_bilqr_workspace();
  ws->ctx = ctx; ws->m = m; ws->n = n;
  (void)take_alloc_seconds();
  // uₖ₋₁, uₖ, q, vₖ₋₁, vₖ, p, x, y, d̅, wₖ₋₃, wₖ₋₂ allocated; Δx, Δy stay empty until a warm start (src/krylov_workspaces.jl, BilqrWorkspace)
  int rc = KHIP_OK;
  for (double **slot : {&ws->u_prev, &ws->u, &ws->q, &ws->v_prev, &ws->v, &ws->p, &ws->x, &ws->y, &ws->dbar, &ws->w_prev3,
                        &ws->w_prev2})
    if (!rc) rc = alloc_vec(ctx, n, slot);
  if (rc) { khip_bilqr_workspace_destroy(ws); return rc; }
  ws->box.st.allocation_timer = take_alloc_seconds();
  *out = ws;
  return KHIP_OK;
}

int khip_bilqr_workspace_adopt(khip_ctx *ctx, int64_t m, int64_t n, double *u_prev, double *u, double *q, double *v_prev, double *v,
                               double *p, double *x, double *y, double *dbar, double *w_prev3, double *w_prev2,
                               khip_bilqr_workspace **out) {
  KHIP_REQUIRE(ctx && out && m >= 0 && n >= 0, "bilqr_workspace_adopt: bad argument");
  KHIP_REQUIRE(m == n, "Systems must be square");
  KHIP_REQUIRE(n == 0 || (u_prev && u && q && v_prev && v && p && x && y && dbar && w_prev3 && w_prev2),
               "bilqr_workspace_adopt: u_prev, u, q, v_prev, v, p, x, y, dbar, w_prev3, w_prev2 must be device vectors of n entries");
  const double *all[11] = {u_prev, u, q, v_prev, v, p, x, y, dbar, w_prev3, w_prev2};
  for (int i = 0; i < 11; ++i)
    for (int j = i + 1; j < 11; ++j)
      KHIP_REQUIRE(n == 0 || all[i] != all[j],
                   "bilqr_workspace_adopt: u_prev, u, q, v_prev, v, p, x, y, dbar, w_prev3, w_prev2 must be distinct");
  khip_bilqr_workspace *ws = new khip_bilqr_workspace();
  ws->ctx = ctx; ws->m = m; ws->n = n;
  ws->u_prev = u_prev; ws->u = u; ws->q = q; ws->v_prev = v_prev; ws->v = v; ws->p = p; ws->x = x; ws->y = y; ws->dbar = dbar;
  ws->w_prev3 = w_prev3; ws->w_prev2 = w_prev2;
  for (const double *ptr : all) ws->borrowed.add(ptr);
  *out = ws;
  return KHIP_OK;
}

int khip_bilqr_workspace_adopt_vector(khip_bilqr_workspace *ws, const char *name, double *ptr) {
  KHIP_REQUIRE(ws && name, "bilqr_workspace_adopt_vector: null argument");
  using S = NamedSlot;
  return adopt_named(ws->ctx, ws->borrowed, {{"u_prev", &ws->u_prev, S::Fixed}, {"u", &ws->u, S::Fixed}, {"q", &ws->q, S::Fixed},
                     {"v_prev", &ws->v_prev, S::Fixed}, {"v", &ws->v, S::Fixed}, {"p", &ws->p, S::Fixed}, {"x", &ws->x, S::Fixed},
                     {"y", &ws->y, S::Fixed}, {"dbar", &ws->dbar, S::Fixed}, {"w_prev3", &ws->w_prev3, S::Fixed},
                     {"w_prev2", &ws->w_prev2, S::Fixed}, {"dx", &ws->dx, S::Optional}, {"dy", &ws->dy, S::Optional}},
                     "bilqr_workspace_adopt_vector", "vector", name, ptr);
}

int khip_bilqr_workspace_destroy(khip_bilqr_workspace *ws) {
  if (!ws) return KHIP_OK;
  for (double *ptr : {ws->u_prev, ws->u, ws->q, ws->v_prev, ws->v, ws->p, ws->x, ws->y, ws->dbar, ws->w_prev3, ws->w_prev2, ws->dx,
                      ws->dy})
    free_unless_borrowed(ws->ctx, ws->borrowed, ptr);
  ws->loop.release();
  delete ws;
  return KHIP_OK;
}

int khip_bilqr_warm_start(khip_bilqr_workspace *ws, const double *x0, const double *y0) {
  KHIP_REQUIRE(ws && x0 && y0, "bilqr_warm_start: x0 and y0 are both required");
  if (!ws->dx) KHIP_TRY(alloc_vec(ws->ctx, ws->n, &ws->dx));
  if (!ws->dy) KHIP_TRY(alloc_vec(ws->ctx, ws->n, &ws->dy));
  if (x0 != ws->dx) KHIP_TRY(khip_copy(ws->ctx, ws->n, ws->dx, x0));
  if (y0 != ws->dy) KHIP_TRY(khip_copy(ws->ctx, ws->n, ws->dy, y0));
  ws->warm_start = true;
  return KHIP_OK;
}

double *khip_bilqr_solution_x(khip_bilqr_workspace *ws) { return ws ? ws->x : nullptr; }
double *khip_bilqr_solution_y(khip_bilqr_workspace *ws) { return ws ? ws->y : nullptr; }
const khip_stats *khip_bilqr_stats(khip_bilqr_workspace *ws) { return ws ? &ws->box.st : nullptr; }
int khip_bilqr_adjoint_stats(khip_bilqr_workspace *ws, int *solved_primal, int *solved_dual, const double **residuals_primal,
                             int *nprimal, const double **residuals_dual, int *ndual, const char **status) {
  KHIP_REQUIRE(ws, "bilqr_adjoint_stats: null workspace");
  if (solved_primal) *solved_primal = ws->solved_primal;
  if (solved_dual) *solved_dual = ws->solved_dual;
  if (residuals_primal) *residuals_primal = ws->box.residuals.empty() ? nullptr : ws->box.residuals.data();
  if (nprimal) *nprimal = (int)ws->box.residuals.size();
  if (residuals_dual) *residuals_dual = ws->residuals_dual.empty() ? nullptr : ws->residuals_dual.data();
  if (ndual) *ndual = (int)ws->residuals_dual.size();
  if (status) *status = ws->status.c_str();
  return KHIP_OK;
}
// test-only export (include/krylov_hip_test.h): the status the flags of `mask` end in, whole (*full, a literal) and as
// khip_stats.status holds it (cut96).  Bits: 0 lq_tol, 1 lq_mach, 2 cg_tol, 3 cg_mach, 4 qr_tol, 5 qr_mach, 6 tired, 7 breakdown,
// 8 user exit, 9 overtimed.  Host only.
int khip_test_bilqr_status(int mask, char *cut96, const char **full) {
  KHIP_REQUIRE(cut96 && full, "test_bilqr_status: null argument");
  BilqrDevState s;
  memset(&s, 0, sizeof(s));
  s.solved_lq_tol = mask & 1; s.solved_lq_mach = (mask >> 1) & 1; s.solved_cg_tol = (mask >> 2) & 1; s.solved_cg_mach = (mask >> 3) & 1;
  s.solved_qr_tol = (mask >> 4) & 1; s.solved_qr_mach = (mask >> 5) & 1; s.breakdown = (mask >> 7) & 1;
  s.solved_lq = s.solved_lq_tol || s.solved_lq_mach;
  s.solved_cg = s.solved_cg_tol || s.solved_cg_mach;
  s.solved_primal = s.solved_lq || s.solved_cg;
  s.solved_dual = s.solved_qr_tol || s.solved_qr_mach;
  *full = status_of(s, (mask >> 6) & 1, (mask >> 8) & 1, (mask >> 9) & 1);
  copy_status(cut96, 96, *full);
  return KHIP_OK;
}
int khip_bilqr_last_path(khip_bilqr_workspace *ws) { return ws ? ws->box.path : -1; }
double *khip_bilqr_vector(khip_bilqr_workspace *ws, const char *name) {
  if (!ws || !name) return nullptr;
  struct { const char *k; double *p; } tab[] = {{"u_prev", ws->u_prev}, {"u", ws->u}, {"q", ws->q}, {"v_prev", ws->v_prev},
                                                {"v", ws->v}, {"p", ws->p}, {"x", ws->x}, {"y", ws->y}, {"dbar", ws->dbar},
                                                {"w_prev3", ws->w_prev3}, {"w_prev2", ws->w_prev2}, {"dx", ws->dx}, {"dy", ws->dy}};
  for (auto &e : tab) if (strcmp(e.k, name) == 0) return e.p;
  return nullptr;
}
size_t khip_bilqr_workspace_bytes(khip_bilqr_workspace *ws) {
  if (!ws) return 0;
  size_t cnt = 0;
  for (double *ptr : {ws->u_prev, ws->u, ws->q, ws->v_prev, ws->v, ws->p, ws->x, ws->y, ws->dbar, ws->w_prev3, ws->w_prev2, ws->dx,
                      ws->dy})
    cnt += ptr ? 1 : 0;
  return cnt * sizeof(double) * (size_t)ws->n;
}

int khip_bilqr_solve(khip_bilqr_workspace *ws, const khip_operator *A, const khip_operator *At, const double *b, const double *c,
                     const khip_options *opts_in, const khip_bilqr_params *params_in) {
  KHIP_REQUIRE(ws && A && b, "bilqr_solve: null argument");
  khip_ctx *ctx = ws->ctx;
  const khip_options o = opts_in ? *opts_in : khip_default_options();
  const khip_bilqr_params prm = params_in ? *params_in : khip_bilqr_default_params();
  const double t0 = now_s();
  const double timemax = timemax_of(o);
  const int64_t n = ws->n;
  khip_stats *st = &ws->box.st;
  const double atol = tol_or_default(o.atol), rtol = tol_or_default(o.rtol);
  const int verbose = o.verbose;
  const bool history = o.history != 0;
  (void)take_alloc_seconds();

  if (!At) return ws->box.fail(KHIP_ERR_INVALID, "bilqr_solve: At (the adjoint of A) is required");
  if (!c) return ws->box.fail(KHIP_ERR_INVALID, "bilqr_solve: c (the right-hand side of the dual system) is required");
  for (const khip_operator *op : {A, At}) {                                                              // :122-123
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
  if (ws->m != ws->n) return ws->box.fail(KHIP_ERR_INVALID, "Systems must be square");
  if (verbose > 0) klogf(o.log_fd, "BILQR: systems of size %lld\n", (long long)n);                       // :127
  const bool warm_start = ws->warm_start;
  ws->box.reset();
  ws->residuals_dual.clear();
  ws->status = "unknown";
  ws->solved_primal = ws->solved_dual = 0;
  double *x = ws->x, *y = ws->y, *dbar = ws->dbar, *q = ws->q, *p = ws->p;
  double *v = ws->v, *v_prev = ws->v_prev, *u = ws->u, *u_prev = ws->u_prev, *w3 = ws->w_prev3, *w2 = ws->w_prev2;
  auto finish = [&](const char *status, int solved_primal, int solved_dual) {
    ws->status = status;
    ws->solved_primal = solved_primal;
    ws->solved_dual = solved_dual;
    st->solved = (solved_primal && solved_dual) ? 1 : 0;
    st->inconsistent = 0;
    copy_status(st->status, sizeof(st->status), ws->status);
    st->timer = now_s() - t0;
    ws->warm_start = false;
    st->allocation_timer += take_alloc_seconds();
    ws->box.publish();
  };

  // set-up, the same primitives on every path (:144-217)
  const double *r0 = b, *s0 = c;
  if (warm_start) {
    K(apply_op(ctx, A, ws->dx, q));
    K(khip_axpby(ctx, n, 1.0, b, -1.0, q));
    K(apply_op(ctx, At, ws->dy, p));
    K(khip_axpby(ctx, n, 1.0, c, -1.0, p));
    r0 = q;
    s0 = p;
  }
  K(khip_fill(ctx, n, x, 0.0));
  double bNorm, cNorm;
  K(khip_nrm2(ctx, n, r0, &bNorm));
  K(khip_fill(ctx, n, y, 0.0));
  K(khip_nrm2(ctx, n, s0, &cNorm));
  const int64_t itmax = o.itmax == 0 ? 2 * global_rows(ctx, A, n) : o.itmax;
  if (history) {
    ws->box.push(bNorm);
    ws->residuals_dual.push_back(cNorm);
  }
  BilqrDevState s;
  memset(&s, 0, sizeof(s));
  s.bNorm = bNorm;
  s.eps_L = atol + rtol * bNorm;
  s.eps_Q = atol + rtol * cNorm;
  s.sNorm = cNorm;
  s.rNorm_lq = bNorm;
  ws->box.path = o.fused ? 1 : 0;
  if (verbose > 0) {
    klogf(o.log_fd, "%5s  %s  %s  %5s\n", "k", "   \xe2\x80\x96r\xe2\x82\x96\xe2\x80\x96", "   \xe2\x80\x96s\xe2\x82\x96\xe2\x80\x96", "timer");
    if (kdisplay(0, verbose)) klogf(o.log_fd, "%5d  %7.1e  %7.1e  %.2fs\n", 0, bNorm, cNorm, now_s() - t0);
  }
  double cb;
  K(khip_dot(ctx, n, s0, r0, &cb));
  if (cb == 0) {                                                                                         // :174-184
    st->niter = 0;
    if (warm_start) {
      K(khip_axpy(ctx, n, 1.0, ws->dx, x));
      K(khip_axpy(ctx, n, 1.0, ws->dy, y));
    }
    finish("Breakdown b\xe1\xb4\xb4" "c = 0", 0, 0);
    return KHIP_OK;
  }
  s.beta = std::sqrt(std::fabs(cb));
  s.gamma = cb / s.beta;
  K(khip_fill(ctx, n, v_prev, 0.0));
  K(khip_fill(ctx, n, u_prev, 0.0));
  K(khip_divcopy(ctx, n, v, r0, s.beta));
  K(khip_divcopy(ctx, n, u, s0, s.gamma));
  s.cs = s.cs_prev = -1.0;
  K(khip_fill(ctx, n, dbar, 0.0));
  s.norm_v = bNorm / s.beta;
  K(khip_fill(ctx, n, w3, 0.0));
  K(khip_fill(ctx, n, w2, 0.0));
  s.transfer_to_bicg = prm.transfer_to_bicg ? 1 : 0;
  s.stop_seq = kSeqNever;
  s.solved_lq = (bNorm == 0) ? 1 : 0;                                                                    // :207-212
  s.solved_primal = s.solved_lq;
  s.solved_dual = (cNorm == 0) ? 1 : 0;
  bool tired = 0 >= itmax, user_exit = false, overtimed = false;
  int64_t iter = 0;
  auto running = [&] { return !((s.solved_primal && s.solved_dual) || tired || s.breakdown || user_exit || overtimed); };
  auto products = [&](const double *vk, const double *uk, double *qk, double *pk) -> int {              // :227-228
    KHIP_TRY(apply_op_no_epilogue(ctx, A, vk, qk));
    KHIP_TRY(apply_op_no_epilogue(ctx, At, uk, pk));
    return KHIP_OK;
  };
  // the end of an iteration on the host-driven loops (:327, :402, :433-441); the flags are those before the iteration's tests
  auto host_tail = [&](int64_t k, bool primal_ran, bool dual_ran) {
    if (history && primal_ran) ws->box.push(s.rNorm_lq);
    if (history && dual_ran) ws->residuals_dual.push_back(s.sNorm);
    if (o.callback) {
      ws->box.publish();                          // the callback reads both histories
      user_exit = o.callback(ws, o.callback_data) != 0;
    }
    tired = k >= itmax;
    overtimed = time_limit_reached(ctx, now_s() - t0, timemax);
    if (kdisplay(k, verbose)) verbose_row(o, k, s, t0);
  };

  const bool csr_pair = A->csr && !A->apply && At->csr && !At->apply;
  const bool device_loop = o.fused >= 2 && csr_pair && !o.callback && verbose <= 0;
  ws->box.path = (device_loop && running()) ? 2 : (o.fused ? 1 : 0);   // a loop that never starts reports 1, as the early return does

  if (ws->box.path == 0) {
    // ---------------------------------------------------------------- the reference's primitive sequence (:219-442) ----
    while (running()) {
      const int64_t k = ++iter;
      const bool primal = !s.solved_primal, dual = !s.solved_dual;
      K(products(v, u, q, p));
      K(khip_axpy(ctx, n, -s.gamma, v_prev, q));
      K(khip_axpy(ctx, n, -s.beta, u_prev, p));
      double uq;
      K(khip_dot(ctx, n, u, q, &uq));
      bilqr_step_a(s, uq);
      K(khip_axpy(ctx, n, -s.alpha, v, q));
      K(khip_axpy(ctx, n, -s.alpha, u, p));
      double pq;
      K(khip_dot(ctx, n, p, q, &pq));
      bilqr_step_b(s, pq, k);
      double vq = 0.0, q_norm = 0.0;
      if (primal) {                                                                                       // :296-315
        if (k == 1) {
          K(khip_copy(ctx, n, dbar, v));
        } else {
          K(khip_axpy(ctx, n, s.zc, dbar, x));
          K(khip_axpy(ctx, n, s.zs, v, x));
          K(khip_axpby(ctx, n, s.neg_c, v, s.sn, dbar));
        }
        K(khip_dot(ctx, n, v, q, &vq));
        K(khip_nrm2(ctx, n, q, &q_norm));
      }
      if (dual) {                                                                                         // :361-398
        double *w = nullptr;
        if (k == 2) {
          w = w2;
          K(khip_divcopy(ctx, n, w, u_prev, s.delta));
        }
        if (k >= 3) {
          w = w3;
          if (k >= 4) K(khip_scal(ctx, n, s.neg_eps3, w));
          K(khip_axpy(ctx, n, 1.0, u_prev, w));
          K(khip_axpy(ctx, n, s.neg_lambda2, w2, w));
          K(khip_div(ctx, n, w, s.delta));
          std::swap(w3, w2);                                                                              // @kswap!(wₖ₋₃, wₖ₋₂)
        }
        if (k >= 2) K(khip_axpy(ctx, n, s.psi, w, y));
        K(khip_dot(ctx, n, u, u, &s.uu));                                                                 // kdotr(n, uₖ, uₖ), :398
      }
      K(khip_copy(ctx, n, v_prev, v));
      K(khip_copy(ctx, n, u_prev, u));
      if (pq != 0) {
        K(khip_divcopy(ctx, n, v, q, s.beta_next));
        K(khip_divcopy(ctx, n, u, p, s.gamma_next));
      }
      bilqr_step_c(s, vq, q_norm, 0.0, k);          // ‖uₖ₊₁‖² is not carried here: the next iteration takes its own kdotr
      host_tail(k, primal, dual);
    }
  } else if (ws->box.path == 1) {
    // ---------------------------------------------------------------- host-driven loop on the fused kernels ----------
    K(ws->loop.alloc());
    s.hist_p = s.hist_d = nullptr;
    if (running()) K(khip_dot(ctx, n, u, u, &s.uu));                                                      // ‖u₁‖²
    while (running()) {
      const int64_t k = ++iter;
      const bool primal = !s.solved_primal, dual = !s.solved_dual;
      K(products(v, u, q, p));
      K(ws->loop.upload(ctx, s));
      int slot = take_slots(ctx, 1);
      K(launch_p1(ctx, n, ws->loop.dev, v_prev, u_prev, u, q, p, slot));
      double uq;
      K(fetch_results(ctx, slot, 1, &uq));
      bilqr_step_a(s, uq);
      K(ws->loop.upload(ctx, s));
      slot = take_slots(ctx, 1);
      K(launch_p2(ctx, n, ws->loop.dev, v, u, q, p, slot));
      double pq;
      K(fetch_results(ctx, slot, 1, &pq));
      bilqr_step_b(s, pq, k);
      K(ws->loop.upload(ctx, s));
      slot = take_slots(ctx, kP3Sums);
      K(launch_p3(ctx, n, ws->loop.dev, x, dbar, y, w3, w2, k == 2 ? w2 : w3, v, u, u_prev, q, p, v_prev, u_prev,
                  k < 4 ? (int)k : 4, slot));
      double r[kP3Sums];
      K(fetch_results(ctx, slot, kP3Sums, r));
      std::swap(v, v_prev);                        // vₖ₋₁ <- vₖ ; vₖ <- vₖ₊₁ (:411-418) as a rotation of the roles
      std::swap(u, u_prev);
      if (dual && k >= 3) std::swap(w3, w2);       // wₖ₋₁ was written over wₖ₋₃ (:383-386)
      bilqr_step_c(s, r[0], std::sqrt(r[1]), r[2], k);
      host_tail(k, primal, dual);
    }
  } else {
    // ---------------------------------------------------------------- device-resident loop -----------------------------
    K(khip_dot(ctx, n, u, u, &s.uu));                                                                     // ‖u₁‖²
    double *vc = v, *vp = v_prev, *uc = u, *up = u_prev, *wc3 = w3, *wc2 = w2;
    auto step = [&](BilqrDevState *dev, long long j) {
      const int64_t k = j + 1;
      ctx->ctl = SeqCtl{&dev->stop_seq, 4 * j + 1, EPI_NONE, nullptr};
      int rc = spmv_any(ctx, A->csr, vc, q, -1);                                          // q = A vₖ
      if (rc == KHIP_OK) rc = spmv_any(ctx, At->csr, uc, p, -1);                          // p = A' uₖ
      if (rc != KHIP_OK) return rc;
      ctx->ctl = SeqCtl{&dev->stop_seq, 4 * j + 2, EPI_BILQR_A, dev};
      int slot = take_slots(ctx, 1);
      rc = launch_p1(ctx, n, dev, vp, up, uc, q, p, slot);                               // P1 ; u.q -> α
      if (rc == KHIP_OK && ctx->comm) rc = comm_allreduce_dd_device(ctx, slot, 1);
      if (rc != KHIP_OK) return rc;
      ctx->ctl = SeqCtl{&dev->stop_seq, 4 * j + 3, EPI_BILQR_B, dev};
      slot = take_slots(ctx, 1);
      rc = launch_p2(ctx, n, dev, vc, uc, q, p, slot);                                   // P2 ; p.q -> the LQ update
      if (rc == KHIP_OK && ctx->comm) rc = comm_allreduce_dd_device(ctx, slot, 1);
      if (rc != KHIP_OK) return rc;
      ctx->ctl = SeqCtl{&dev->stop_seq, 4 * j + 4, EPI_BILQR_C, dev};
      slot = take_slots(ctx, kP3Sums);
      rc = launch_p3(ctx, n, dev, x, dbar, y, wc3, wc2, k == 2 ? wc2 : wc3, vc, uc, up, q, p, vp, up, k < 4 ? (int)k : 4,
                     slot);                                                               // P3 ; the three sums -> tests
      if (rc == KHIP_OK && ctx->comm) rc = comm_allreduce_dd_device(ctx, slot, kP3Sums);
      ctx->ctl = SeqCtl{};
      if (rc != KHIP_OK) return rc;
      std::swap(vc, vp);
      std::swap(uc, up);
      if (k >= 3) std::swap(wc3, wc2);             // a dual side that is solved no longer touches either buffer
      return KHIP_OK;
    };
    // a finite timemax: the first chunk is ONE iteration, so that a limit already used up stops after iteration 1 as the
    // host-driven loop does
    const DeviceLoopArgs loop_args{itmax, t0, timemax, history, {&ws->box.residuals, &ws->residuals_dual, nullptr},
                                   timemax < 1e300 ? 1 : kDevChunk};
    K(ws->loop.run(ctx, s, loop_args, step, &s, &overtimed));
    iter = s.iter;
    tired = iter >= itmax;
    // the host rotated the roles for every iteration it enqueued; the device ran s.iter of them, and its dual block s.nhist_d
    if (iter & 1) { std::swap(v, v_prev); std::swap(u, u_prev); }
    if (s.nhist_d >= 3 && (s.nhist_d & 1)) std::swap(w3, w2);
  }
  ws->v = v; ws->v_prev = v_prev; ws->u = u; ws->u_prev = u_prev; ws->w_prev3 = w3; ws->w_prev2 = w2;
  if (verbose > 0) klogf(o.log_fd, "\n");
  if (s.solved_cg) K(khip_axpy(ctx, n, s.zbar, dbar, x));                                                // :447-449
  const char *status = status_of(s, tired, user_exit, overtimed);
  if (warm_start) {                                                                                       // :472-473
    K(khip_axpy(ctx, n, 1.0, ws->dx, x));
    K(khip_axpy(ctx, n, 1.0, ws->dy, y));
  }
  st->niter = (int)iter;
  finish(status, s.solved_primal ? 1 : 0, s.solved_dual ? 1 : 0);
  return KHIP_OK;
}

}  // extern "C"
