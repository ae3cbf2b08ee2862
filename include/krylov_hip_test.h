/*
 * krylov_hip_test.h -- TEST-ONLY exports of libkrylov_hip.so.
 *
 * Not part of the drop-in boundary (include/krylov_hip.h): nothing in the Julia glue of INTEGRATION.md, the reference's
 * C / Fortran interface (libkrylov_hip_capi.so) or the examples calls these.  They let tests/ check host-side pieces of the
 * product against the reference's exact known answers (test/test_aux.jl:3-117) and against LAPACK without a device
 * (tests/test_abi.py, tests/test_panel_qr_host.py, tests/test_ilu_blocks_host.py) and may change or disappear at any time.
 */
#ifndef KRYLOV_HIP_TEST_H
#define KRYLOV_HIP_TEST_H

#include "krylov_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Test-only exports of the scalar helpers of the solver loops, so that the reference's exact known answers
 * (test/test_aux.jl:3-117) are checked against the copies the product runs: sym_givens (src/krylov_utils.jl:21-51),
 * roots_quadratic (:110-152), to_boundary with M = I (:375-402; x, d device vectors, the dots run on the device). */
int khip_test_sym_givens(double a, double b, double *c, double *s, double *rho);
/* bilqr!'s termination status (src/bilqr.jl:451-469) for the flags of `mask` -- bits: 0 solved_lq_tol, 1 solved_lq_mach, 2 solved_cg_tol,
 * 3 solved_cg_mach, 4 solved_qr_tol, 5 solved_qr_mach, 6 tired, 7 breakdown, 8 user-requested exit, 9 overtimed -- whole (*full) and as
 * khip_stats.status holds it (cut96: char[96], cut at a UTF-8 character boundary).  Host only. */
int khip_test_bilqr_status(int mask, char *cut96, const char **full);
int khip_test_roots_quadratic(double q2, double q1, double q0, int nitref, double *root1, double *root2);
int khip_test_to_boundary(khip_ctx *ctx, int64_t n, const double *x, const double *d, double radius, int flip,
                          double *sigma1, double *sigma2);

/* test-only measurement hook (tools/slab_iteration.py, tests/test_gpu_self_halo.py): a ONE-rank RCCL communicator whose slab's
 * off-slab columns wrap onto its own rows and travel through the real exchange plan (pack kernel, grouped ncclSend / ncclRecv to
 * itself on the halo stream, interior / boundary split, 16-byte all-gather + combine).  Set before khip_comm_init / the handle's
 * creation.  Not an option of khip_ctx_set_option: it changes the operator (periodic slab). */
int khip_test_set_halo_self(khip_ctx *ctx, int enable);

/* test-only, host-only: the analysis behind the block schedule on a CSR pattern in host memory (no device; checks that
 * every row lands in exactly one block and no block depends on a later one).  mode 1 = as khip_ilu0_create, 3 = level
 * sequence.  out10 = grid dims[3], skewed basis, blocks lower / upper, largest face list, 48-byte records possible,
 * largest row, rows of the largest block rounded up to the wave. */
int khip_test_ilu_blocks_host(int64_t n, const int64_t *rowptr, const int32_t *col, int mode, int64_t *out10);
/* test-only: which row path the blocks of the triangular solves take, from the one decision the launch uses.  paths48:
 * [0..15] lower and [16..31] upper triangle: blocks on the 48-byte records, the 176-byte records, the packed lists; packed
 * blocks inside a handle that has records (64 local levels or more, or a level wider than the wave); blocks with a row of
 * more than 16 entries; blocks with more than 1024 face rows; largest face list; largest row; most local levels; widest
 * local level; rows_cap; dynamic LDS bytes; workgroups launched (0 in the host-only form); blocks.  [32..37] batched
 * small-level launches and single-level launches of the factorisation, the lower and the upper level solve.  [38] 1 = block
 * schedule in use, [39] why an attempted one is not (1: LDS, 2: 16-bit slot range), [40] 1 = the create path attempts one
 * (option, grid or rows-per-level gate), [41] [42] levels of the lower / upper triangle.
 * khip_test_ilu0_paths: a live operator.  khip_test_ilu_paths_host: host-only, the arguments of khip_test_ilu_blocks_host
 * plus the value of option ilu_blocks the operator would be created under (3 implies mode 3). */
int khip_test_ilu0_paths(const khip_operator *op, int64_t *paths48);
int khip_test_ilu_paths_host(int64_t n, const int64_t *rowptr, const int32_t *col, int mode, int ilu_blocks, int64_t *out10,
                             int64_t *paths48);

/* test-only, host-only: the rows [row0, row0 + m) of khip_gen_banded_random into host arrays (no device): rowptr_out has m + 1
 * entries; col_out / val_out may be null on a first call that only asks for the row pointers and *nnz_out. */
int khip_test_gen_banded_random_host(int64_t n, int half_band, int links, uint64_t seed, int flags, int dense_rows, int64_t row0,
                                     int64_t m, int32_t *rowptr_out, int32_t *col_out, double *val_out, int64_t *nnz_out);
/* test-only, host-only: the p x p host steps of khip_panel_qr (no device).  deflating_chol: G = Gram matrix (column-major); detect
 * != 0: columns whose Cholesky pivot is <= tol^2 max_j G_jj are left out of the factor and returned as a bit mask, else the
 * columns `preset` are; Rhat (column-major, upper) = the factor of the other columns with R_jj = 1 and a zero row for those left
 * out; *ok = 0 when a column that is not left out has a vanishing pivot.  householder_r: R (row-major, upper) of a rows x p
 * row-major matrix by unblocked Householder QR (the last TSQR level across ranks); A is overwritten.
 * householder_signs: LAPACK's column signs S and tau of the Householder QR of an n x p panel with orthonormal columns from its
 * top p x p block Q1 (row-major; overwritten). */
int khip_test_deflating_chol(int p, const double *G, double tol, int detect, unsigned preset, double *Rhat, int *ok, unsigned *mask);
int khip_test_householder_r(int rows, int p, double *A, double *R);
int khip_test_householder_signs(int p, int64_t n, double *Q1, double *S, double *tau);
/* ... and the small dense routines block_gmres! runs on the host for its 2p x p blocks (column-major, LAPACK semantics): which = 0
 * DGEQR2 (A m x n in place, tau), 1 DORG2R (first n columns of Q in place of DGEQR2's output), 2 DORM2R('L', 'T') on C (m x nc),
 * 3 the inverse of an upper triangular n x n matrix into C. */
int khip_test_small_dense(int which, int m, int n, int nc, double *A, double *tau, double *Cmat);

/* test-only: how many lazily built accelerators (coded / delta column streams, SpMM tile records) failed to build for a reason
 * OTHER than an out-of-memory device since the library was loaded -- such a failure degrades to the plain kernels (results stay
 * right) and is a defect of the builder; the GPU test session asserts 0 (tests/conftest.py). */
int khip_test_optional_build_failures(int *count);

/* test-only: the CSR arrays a handle holds (for a transposed handle: what khip_csr_transpose built), copied to the host:
 * rowptr_out has m + 1 entries, col_out / val_out nnz (tests/test_gpu_operator_forms_exact.py compares the rows of A' with the
 * stable column-major order of A, entry by entry). */
int khip_test_csr_arrays(const khip_csr *A, int32_t *rowptr_out, int32_t *col_out, double *val_out);

/* test-only: the SpMM pin (tests/spmm_model.py, tests/test_gpu_spmm_exact.py).
 * khip_test_csr_tile_records: what spmm_tile_build left on the handle.  out16 = state (0 not tried, 1 built, -1 refused), window
 * slots (cap), bytes per record, groups, run_len, runs, look-ahead flag, 1 = grid tiles, groups on the direct path (all 0 unless
 * state == 1), then line_rows, plane_rows, m, n, nnz, n_ghost, band of the handle.  *reuse = the builder's score (references per
 * distinct column).  meta_out (groups x stride bytes) / direct_out (direct-path groups) may be null: a first call reads the sizes.
 * A record: int32 {row, first entry, length, aux}[32] | int32 list[cap] | uint8 slot[32][32]; aux of row slot 0 = distinct
 * columns, 1 = direct-path flag, 2 = octets of window slots to copy, 3 = look-ahead flag.
 * khip_test_csr_window_info: *win_L = lanes per row the window metadata was built for (-L: refused for L, 0: not tried), its row
 * groups and how many of them are flagged for the direct path.
 * khip_test_spmm_last_launch: what the last khip_spmm on ctx launched, written from the variables of the launch itself where it is
 * decided (it changes no decision).  out24 = family (0 none yet, 1 spmm_kernel, 2 spmm2_kernel, 3 spmm_window_kernel, 4 spmm_tile_kernel,
 * 5 spmm_tile2_kernel), L (spmm_kernel: P), NL, dbuf, ahead, run_len passed to the kernel, workgroups, XCD-order bits (8 round-robin,
 * 128 chunked front, 0 eighths), tile launches (column slices), workgroups of the direct-path kernel, sweep S, W, K, columns per
 * XCD, non-temporal instantiation, DIST instantiation, p, POW2 arm of the window kernel, threads per workgroup, dynamic LDS bytes,
 * CUs of the device; the rest 0. */
int khip_test_csr_tile_records(const khip_csr *A, int64_t *out16, double *reuse, char *meta_out, int64_t meta_bytes,
                               int32_t *direct_out, int64_t direct_cap);
int khip_test_csr_window_info(const khip_csr *A, int *win_L, int64_t *groups, int64_t *flagged);
int khip_test_spmm_last_launch(const khip_ctx *ctx, int64_t *out24);

/* test-only, host-only: the launch plan of the streaming vector kernels and the instantiation their dispatcher picks for it
 * (csrc/vec_launch.hpp: vec_plan, vec_dispatch -- the two functions every launcher calls; no device, nothing is allocated).
 * ptrs: up to 8 vector addresses as integers, 0 = absent; extra_aligned: what a launcher says of the vectors of a device table;
 * u: accesses per lane; scalar_path_nt: 0 = the 8-byte path has no non-temporal instantiation (the solvers' fused passes),
 * 1 = it follows the plan (blas1.hip).  out7 = workgroups g, v2, nt, comp of the plan, then the (VEC, NT, COMP) the dispatcher
 * hands to its callable.  KHIP_ERR_INVALID with "vector too long for one launch" when g does not fit a launch. */
int khip_test_vec_plan(int64_t n, const uint64_t *ptrs, int nptrs, int extra_aligned, int u, int nt_min_elems, int compensated,
                       int scalar_path_nt, int64_t *out7);

/* test-only: the three kernels only gmres! reaches (variant = 1 / 2 and the look-ahead), launched the way the solver launches them
 * (tests/test_gpu_gram_schmidt_exact.py).  V_host: k device pointers in host memory.
 * khip_test_multi_dot: out_host[i] = V_i . q for i < k, through (k + 3) & ~3 slots of the device scalar ring (multi_dot4_kernel,
 * four outputs per launch); q may be one of the V_i.
 * khip_test_multi_axpy_dev: x <- x - sum_j coef[j] V_j in the order j = 0 .. k - 1 (multi_axpy_dev_kernel); the coefficients are
 * copied into ring slots on the context's stream and the kernel reads them there.  k <= 256.
 * khip_test_divcopy_dev: y = x / sqrt(sumsq) (divcopy_dev_kernel), sumsq read from a ring slot. */
int khip_test_multi_dot(khip_ctx *ctx, int64_t n, int k, const double *const *V_host, const double *q, double *out_host);
int khip_test_multi_axpy_dev(khip_ctx *ctx, int64_t n, int k, const double *coef_host, const double *const *V_host, double *x);
int khip_test_divcopy_dev(khip_ctx *ctx, int64_t n, double sumsq, const double *x, double *y);

/* test-only: the two vector kernels of trimr! (csrc/trimr.cpp) with the caller's coefficients and device vectors
 * (tests/test_gpu_trimr.py compares every output with the NumPy expression, bit for bit).
 * khip_test_trimr_p3: the fused third pass at stage 1, 2 or 3 (= min(k, 3)).  coef16 (host) = row one (μ₂ₖ₋₅, λ₂ₖ₋₄, η₂ₖ₋₃, σ₂ₖ₋₂, δ₂ₖ₋₁), row
 * two (μ₂ₖ₋₄, λ₂ₖ₋₃, η₂ₖ₋₂, σ₂ₖ₋₁, δ₂ₖ), -σ₁ / δ₂, π₂ₖ₋₁, π₂ₖ, βₖ₊₁, γₖ₊₁, btol.  g8 (host array of device pointers) = gx₂ₖ₋₃, gx₂ₖ₋₂, gx₂ₖ₋₁, gx₂ₖ,
 * gy₂ₖ₋₃, gy₂ₖ₋₂, gy₂ₖ₋₁, gy₂ₖ by their role as the iteration begins: stage 1 writes gx₂ₖ₋₁, gx₂ₖ and gy₂ₖ; stages 2 and 3 write the new
 * (g₂ₖ₋₁, g₂ₖ) into the buffers of (g₂ₖ₋₃, g₂ₖ₋₂).  v_next / u_next take vₖ₊₁ / uₖ₊₁.  All vectors have n entries.
 * khip_test_trimr_g: one broadcast of the primitive sequence, out = (w - c[0] a0 - c[1] a1 [- c[2] a2 [- c[3] a3]]) / delta with
 * nterm = 2, 3 or 4 terms; w = NULL puts -(c[0] a0) in front.  out may be one of the a. */
int khip_test_trimr_p3(khip_ctx *ctx, int64_t n, int stage, const double *coef16, double *x, double *y, double *const *g8, const double *v,
                       const double *u, const double *q, const double *p, double *v_next, double *u_next);
int khip_test_trimr_g(khip_ctx *ctx, int64_t n, double *out, const double *w, int nterm, const double *coef4, const double *a0,
                      const double *a1, const double *a2, const double *a3, double delta);

/* test-only: the fused third pass of usymlqr! (csrc/usymlqr.cpp) at stage 1, 2 or 3 (= min(k, 3)) with the caller's activity flags,
 * coefficients and device vectors (tests/test_gpu_usymlqr.py compares every output with the NumPy expression, bit for bit).
 * coef14 (host) = -ϵₖ₋₂, -λₖ₋₁, δₖ, ϕₖ, the r coefficient -cₖϕbarₖ₊₁/βₖ₊₁, |sₖ|², ζₖ₋₁cₖ₋₁, ζₖ₋₁sₖ₋₁, -ζₖ₋₁, -cₖ₋₁, sₖ₋₁, βₖ₊₁, γₖ₊₁, 1 / δₖ.  w_m2 / w_m1: the
 * buffers of the roles wₖ₋₂ / wₖ₋₁ as the iteration begins: stage 1 writes wₖ into w_m1, stages 2 and 3 into w_m2.  v_next / u_next
 * take vₖ₊₁ / uₖ₊₁.  All vectors have n entries. */
int khip_test_usymlqr_p3(khip_ctx *ctx, int64_t n, int stage, int do_ls, int do_ln, const double *coef14, double *x, double *r, double *dbar,
                         double *y, double *z, double *w_m2, double *w_m1, const double *v, const double *u, const double *q,
                         const double *p, double *v_next, double *u_next);

#ifdef __cplusplus
}
#endif
#endif /* KRYLOV_HIP_TEST_H */
