/*
 * krylov_hip.h -- C ABI of the MI355X-native Krylov inner-loop engine (libkrylov_hip.so).
 *
 * This is the drop-in boundary behind Krylov.jl's own extension contract
 * (docs/src/custom_workspaces.md:107-300): a Julia device
 * vector type forwards each `Krylov.k*` method to one entry point below with a
 * `ccall`; INTEGRATION.md shows that glue.  Plain pointers and sizes only: every
 * `double*` argument is a DEVICE pointer (gfx950 HBM) unless the name ends in
 * `_host`.  Element type: Float64 real (T = FC = Float64), int32 column indices.
 *
 * Conventions (mirror docs/src/interfaces/reference.md:144-165): every function
 * returns an int, 0 = success, < 0 = error; nothing is thrown across the ABI;
 * khip_last_error() holds the message of the last failure on this thread.
 * All calls on one khip_ctx must come from one host thread (the reference's C
 * library has the same rule, reference.md:172).  Kernels run on the context's HIP
 * stream; only the entry points that return a host scalar synchronise.
 *
 * "ref:" comments cite the reference interface each entry point replaces
 * (paths relative to the Krylov.jl v0.10.8 tree).
 */
#ifndef KRYLOV_HIP_H
#define KRYLOV_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KHIP_OK               0
#define KHIP_ERR_INVALID     -1   /* bad argument / inconsistent sizes (Julia error(...)) */
#define KHIP_ERR_HIP         -2   /* a HIP runtime call failed */
#define KHIP_ERR_UNSUPPORTED -3
#define KHIP_ERR_COMM        -4   /* RCCL failure */
#define KHIP_ERR_NUMERIC     -5   /* e.g. operator not SPD (src/cg.jl:163,243) */

#define KHIP_VERSION_MAJOR 0
#define KHIP_VERSION_MINOR 4   /* 2: khip_options gained log_fd (round 4); 3: khip_*_workspace_adopt & co. (round 5); 4: khip_*_last_path,
                                * history published before every callback (round 6).  Clients check
                                * khip_version() against the header they were built with */

typedef struct khip_ctx khip_ctx;   /* device + stream + scratch + (optional) communicator */
typedef struct khip_csr khip_csr;   /* CSR operator resident in HBM */

const char *khip_last_error(void);
void        khip_version(int *major, int *minor);

/* ---------------------------------------------------------------- context ---- */
/* stream: a hipStream_t to borrow (e.g. the caller's current stream) or NULL to create one. */
int   khip_device_count(int *count);            /* HIP devices visible to this process (0 without a GPU; never fails) */
int   khip_device_pci_id(int device, char *buf, size_t cap);   /* "0000:05:00.0": the physical GPU behind a device index (cap >= 16) */
int   khip_ctx_create(int device, void *stream, khip_ctx **out);
int   khip_ctx_destroy(khip_ctx *ctx);
int   khip_ctx_sync(khip_ctx *ctx);
void *khip_ctx_stream(khip_ctx *ctx);
/* tuning / behaviour knobs, see DESIGN.md ("spmv_rows", "spmv_vec", "spmv_nt", "spmv_xcd",
 * "compensated", "blas1_blocks", ...).  Unknown key -> KHIP_ERR_INVALID.
 * "cg_defer_x" (default 1): the device-resident loop of khip_cg_solve (fused = 2, variant 0) updates x every second
 * iteration through a second direction buffer of n doubles that the workspace allocates on first use (adopted workspaces
 * too; it is not one of the workspace's named vectors and khip_cg_workspace_bytes does not count it) -- 4n fewer bytes
 * per iteration, every vector, the history and the stats bit-identical.  0: x every iteration, no extra buffer.  When the
 * buffer cannot be allocated the solve runs as with 0. */
int   khip_ctx_set_option(khip_ctx *ctx, const char *key, int value);
int   khip_ctx_get_option(khip_ctx *ctx, const char *key, int *value);

/* ------------------------------------------------ device buffers ------------- */
/* ref: S(undef, n) / similar(x) in every workspace constructor
 *      (src/krylov_workspaces.jl:269-285,1605-1623,2898-2918; allocate_if src/krylov_utils.jl:281-299) */
int khip_malloc(khip_ctx *ctx, size_t bytes, void **dptr);
int khip_free(khip_ctx *ctx, void *dptr);
int khip_memcpy_h2d(khip_ctx *ctx, void *dst, const void *src_host, size_t bytes);
int khip_memcpy_d2h(khip_ctx *ctx, void *dst_host, const void *src, size_t bytes);
int khip_memcpy_d2d(khip_ctx *ctx, void *dst, const void *src, size_t bytes);
int khip_mem_info(khip_ctx *ctx, size_t *free_bytes, size_t *total_bytes);

/* ------------------------------------------------ CSR operator --------------- */
/* ref: the sparse matrix handed to kmul!(y, A, x) = mul!(y, A, x) (src/krylov_utils.jl:305);
 *      on the existing GPU path a ROCSparseMatrixCSR (docs/src/gpu.md:165-225).
 * rowptr has m+1 entries of `rowptr_bits` (32 or 64) bits, col/val have nnz entries;
 * index_base is 0 or 1 (Julia arrays are 1-based).  The arrays are COPIED (from host when
 * on_device == 0, from device otherwise); the handle owns its HBM copy.  nnz of one handle
 * must be < 2^31 (one GPU's shard; SURVEY.md section 7 "int32 limits"). */
int khip_csr_create(khip_ctx *ctx, int64_t m, int64_t n, int64_t nnz, const void *rowptr,
                    int rowptr_bits, const int32_t *col, const double *val, int index_base,
                    int on_device, khip_csr **out);
/* Distributed form (ref recipe docs/src/custom_workspaces.md:477-586):
 * this rank owns global rows [row0, row0+m) of an n_global-square operator; col[] holds
 * GLOBAL indices.  Requires khip_comm_init on ctx.  Builds the halo plan (needed remote
 * columns, send lists) and remaps columns to [owned | ghost] numbering.
 * A product on such a handle gives, whatever kernel form, halo mode and "overlap_halo" setting, the y of the serial stored-order
 * loop bit for bit on every rank (the vector kernel, "spmv_kernel" = 2: every row within gamma(row length) sum|a_ij x_j|), and
 * its fused scalars (khip_spmv_dot / _dotw / _dot2) come back with identical bits on all ranks. */
int khip_csr_create_dist(khip_ctx *ctx, int64_t n_global, int64_t row0, int64_t m, int64_t nnz,
                         const void *rowptr, int rowptr_bits, const int32_t *col,
                         const double *val, int index_base, int on_device, khip_csr **out);
/* The adjoint operator A' as its own handle (built on the device; entries of a row of A' in increasing column
 * order = the order of a column of A).  khip_spmv(At, x, y) is then `mul!(y, A', x)` (docs/src/matrix_free.md:36-42),
 * what MINRES-QLP / LSQR / LSMR / BiLQ / QMR ... ask of an operator besides `mul!(y, A, x)`.
 * A row-partitioned handle (khip_csr_create_dist) gives a row-partitioned A' with the SAME partition: every rank's entries
 * travel to the owners of their columns (one all-to-all at set-up, collective: call it on every rank), and y = A' x is
 * bit-identical to the single-GPU product.  ref: the two-sided processes and solvers, src/krylov_processes.jl:133-222. */
int khip_csr_transpose(khip_ctx *ctx, const khip_csr *A, khip_csr **At_out);
int khip_csr_destroy(khip_csr *A);
/* Optional internal re-encoding of a handle whose rows repeat few (column - row, value) sequences (stencils):
 * one 16-bit row-template id per row instead of 12 bytes per nonzero (csrc/template.hip).  *templates = number
 * of distinct templates, 0 when the operator is not compressible (it then stays plain CSR).  Results of
 * khip_spmv & co. are bit-identical either way; ctx option "spmv_template" = 0 ignores the compressed form. */
int khip_csr_compress(khip_ctx *ctx, khip_csr *A, int *templates);
/* bytes one SpMV of this handle moves in its CURRENT representation (khip_spmv_bytes: always the CSR formula) */
int khip_spmv_bytes_stored(const khip_csr *A, int64_t *bytes);
int khip_csr_shape(const khip_csr *A, int64_t *m, int64_t *n, int64_t *nnz);
/* How the staged SpMV reads the column indices of this handle (csrc/colcode.hip): *bits = 32 (the int32 CSR columns),
 * or 8 / 16 when the operator's entries lie on at most 256 / 2048 distinct diagonals (column - row) and the handle keeps,
 * next to its CSR arrays, one / two bytes per entry (the rank of the entry's diagonal in a sorted table; col = row +
 * table[code], exact).  The coded stream is built by the first khip_spmv that can use it; *diagonals = table size
 * (0 before that, or when the operator has too many).  y is bit-identical either way; ctx option "spmv_codes": 1 (default)
 * codes operators of at least 4 M entries (smaller ones are latency bound and keep the int32 stream), 2 codes whatever the
 * size, 16 forces two-byte codes, 0 keeps the int32 stream (environment variable KHIP_SPMV_CODES sets the initial value).  ref: the product is kmul!(y, A, x), src/krylov_utils.jl:305. */
int khip_csr_code_info(const khip_csr *A, int *bits, int *diagonals);
/* The SLICED form of a handle with 8-bit codes (csrc/colcode.hip csr_build_sell, read by spmv_sell_kernel): the entries of every 64
 * consecutive rows stored a second time transposed -- per slice, per lane, W = ceil(L / 8) words of eight codes then L values
 * (L = longest row of the slice; a unit = 64 words = 512 bytes) -- so that every lane loads the entries of its own row with
 * coalesced 8-byte loads: no LDS window and no barrier in the row walk.  Built by the first khip_spmv that can use it when the
 * padding costs at most 12 % (ctx option "spmv_sell": 2 default = non-temporal loads of the matrix words, 1 = default policy,
 * 0 = off: the coded CSR stream).  *state = 1 built, 0 not tried, -1 not usable; *units_per_slice > 0: every slice is padded to
 * that many units (no offset array), 0: per-slice offsets; *total_units: units stored.  y and the fused dots are bit-identical to
 * the coded CSR kernel's.  khip_spmv_bytes_stored counts 512 B per unit (+ 4 B per slice of offsets) while the form is in use. */
int khip_csr_sell_info(const khip_csr *A, int *state, int *units_per_slice, int64_t *total_units);
/* *narrow = 1 when the sliced form keeps 4-bit codes: operators with at most 15 diagonals and at most 8 entries per row store ONE
 * 32-bit word of eight codes per row (indexed by the row) and the slices hold values only -- 60 instead of 64 B per 7-point row
 * (ctx option "spmv_sell_narrow" = 1; default 0: it measured 8-10 % slower than the byte-coded words at 512^3, whose slices are 4 KB blocks). */
int khip_csr_sell_narrow(const khip_csr *A, int *narrow);
/* *pairs = size of the entry dictionary when the sliced copy is ENTRY-CODED, 0 when it is not: a handle with 8-bit diagonal codes,
 * rows of at most 64 entries and at most 255 distinct entries -- pairs (column - row, bit pattern of the value) -- keeps one byte
 * per entry (the rank of its pair, ascending (offset, value bits as unsigned); 0xFF = no entry) and no values in its slices:
 * 8 B per row of at most 8 entries, ceil(L / 8) words padded to an even count beyond.  khip_csr_sell_info reports this copy.
 * ctx option "spmv_sell_entries": 1 (default) = handles of at least 2^22 entries, 2 = whenever the handle qualifies, 0 = never.
 * ctx option "spmv_sell_persist": how the entry-coded product is launched.  1 (default) = on handles of one code word per row, where
 * the loop-free launch would have more workgroups than eight rounds of what the device holds at once, that many long-lived workgroups
 * walk the loop-free launch's workgroups, strided (same rows, same reduction partials: every result keeps its bits); 0 = the loop-free
 * launch always; G > 1 = exactly min(G, workgroups of the loop-free launch) long-lived workgroups on every entry-coded handle. */
int khip_csr_sell_entries(const khip_csr *A, int *pairs);
/* The same for the int32 column stream -- operators that are not coded (more than 2048 diagonals, fewer than 4 M entries under
 * "spmv_codes" = 1, or "spmv_codes" = 0) with short rows (the staged kernel's operators: at most 12 entries per row on average):
 * per slice, per lane, ceil(L / 2) words of two int32 columns (-1 = no entry) then L values; same padding rule, same size rule as
 * the codes (at least 4 M entries unless "spmv_codes" = 2 or "spmv_sell" >= 3), same option.  y and the fused dots are
 * bit-identical to the staged CSR kernel's. */
int khip_csr_sell32_info(const khip_csr *A, int *state, int *units_per_slice, int64_t *total_units);
/* Block-delta column stream of the stream SpMV (operators that are not stencils: more than 2048 diagonals; built at the first
 * product that can use it, ctx option "spmv_delta"): bits = 8 / 16 (32: not in use), rows = rows per block, escapes = entries
 * that stay int32 (6 B each).  khip_spmv_bytes_stored counts what that kernel streams. */
int khip_csr_delta_info(const khip_csr *A, int *bits, int *rows, int64_t *escapes);
/* Which SpMV kernel khip_spmv takes for this handle under the context's options: 1 = stream (products in nnz order through
 * LDS), 2 = strided vector (very long rows), 3 = ordered sub-wave, 4 = staged rows (one lane per row; also the one that streams
 * the dictionary codes), 5 = row templates (khip_csr_compress), 6 = wave-private windows (LDS-DMA). */
int khip_spmv_kernel_info(khip_ctx *ctx, const khip_csr *A, int *kernel);
/* Which SpMM kernel a product with 16 right-hand sides runs on this handle (csrc/spmm_tile.hip): *state = 1 when the handle
 * keeps group records for the wave-private-window kernel (built by the first khip_spmm with p = 16; 0 before that, -1 when
 * the operator lacks the locality and the other SpMM kernels are used); *window = distinct panel rows a group's LDS window
 * holds; *grid_tiles = 1 when the 32-row groups are 4 x 4 x 2 tiles of a structured grid recognised from the pattern, 0 when
 * they are 32 consecutive rows; *direct_groups of *groups go down the direct-gather path (a row longer than 32 entries, or
 * more distinct columns than the window takes); *reuse = entries per distinct column of a group.  Y is bit-identical in
 * every case; ctx option "spmm_tile" = 0 switches the kernel off.  ref: mul!(W, A, P), src/block_gmres.jl:242. */
int khip_csr_tile_info(const khip_csr *A, int *state, int *window, int *grid_tiles, int64_t *groups, int64_t *direct_groups,
                       double *reuse);
/* How a distributed handle fetches the remote part of x before a product (csrc/comm.cpp; the reference's MPI recipe,
 * docs/src/custom_workspaces.md:517-521 and :583-586): *gather_mode = 0: only the entries this rank's columns reference
 * travel (grouped Send/Recv with the owning ranks; *n_ghost entries received, *n_send sent per product); 1: every rank's
 * slice is all-gathered (*n_ghost = ranks x largest slice, *n_send = own slice).  Chosen at khip_csr_create_dist by the
 * ctx options "halo_mode" (0 = per operator: gather when some rank would fetch more than "halo_gather_pct" % of its own
 * row count, 1 = always the neighbour exchange, 2 = always the all-gather).  y is bit-identical in both modes. */
int khip_csr_halo_info(const khip_csr *A, int *gather_mode, int64_t *n_ghost, int64_t *n_send);
/* device-side generators of the benchmark operators (rows [row0, row0+m) of the global matrix,
 * global columns; ref: test/get_div_grad.jl:8-25, test/test_utils.jl:160-169).
 * kind: 0 = get_div_grad(n1,n2,n3) 7-pt Poisson, 1 = kron_unsymmetric(n1), 2 = 27-pt cfg-5 operator.
 * Outputs are device arrays owned by the caller (khip_free): rowptr int32[m+1] (local, 0-based),
 * col int32[nnz] (global, 0-based), val double[nnz]. */
int khip_gen_stencil(khip_ctx *ctx, int kind, int n1, int n2, int n3, int64_t row0, int64_t m,
                     int32_t **rowptr_dev, int32_t **col_dev, double **val_dev, int64_t *nnz);
/* Generator of the "banded + random, fixed seed" benchmark operator (csrc/gen_irregular.cpp; the stand-in for the
 * SuiteSparse matrices of the reference's benchmarks, benchmark/cg_bmark.jl:29-54, benchmark/gpu.jl:15-47, which cannot be
 * fetched offline): a symmetric band of half width half_band with 1 entry in 8 left out, `links` long-range partners per row
 * from seeded involutions of blocks of 2^20 rows (far more than 2048 distinct diagonals), off-diagonal entries in (-2, -1],
 * diagonal = 1/16 + the row's absolute sum (strictly diagonally dominant; SPD when symmetric).  flags bit 0: nonsymmetric values
 * (entries above the diagonal halved); dense_rows > 0 (nonsymmetric only): that many rows with 3000 further entries each.
 * Built on the host, rows [row0, row0 + m) of the global operator; outputs as khip_gen_stencil.  The definition is restated in
 * the file's header and, independently, by the oracle (ko_csr_banded_random). */
int khip_gen_banded_random(khip_ctx *ctx, int64_t n, int half_band, int links, uint64_t seed, int flags, int dense_rows,
                           int64_t row0, int64_t m, int32_t **rowptr_dev, int32_t **col_dev, double **val_dev, int64_t *nnz);

/* y <- A x.  ref: kmul!(y, A, x) src/krylov_utils.jl:305; sites src/cg.jl:155,196,
 * src/gmres.jl:159,222,257, src/bicgstab.jl:160,221,228.  For a distributed handle x and y are
 * the owned slices; the halo exchange happens inside. */
int khip_spmv(khip_ctx *ctx, const khip_csr *A, const double *x, double *y);
/* Y <- A X for row-major n-by-p panels (ld = p).  ref: mul!(W, A, P) src/block_gmres.jl:242.
 * The first product with an even p on an operator whose neighbouring rows share columns (banded / stencil) builds,
 * once per handle and range of p, a list of the distinct columns of every group of 256 / ceil_pow2(p / 2) rows and a
 * 16-bit slot per nonzero (~2 B per nonzero + 4 B per list entry of device memory, about the time of five products);
 * later products copy each distinct panel row once into LDS instead of gathering it per nonzero.  Y is bit-identical
 * either way (ctx option "spmm_window" = 0 keeps the direct gathers).  Like every call on a handle, this is confined
 * to the context's thread. */
int khip_spmm(khip_ctx *ctx, const khip_csr *A, const double *X, double *Y, int p);
/* algorithmic HBM bytes of one khip_spmv on this handle: 12 nnz + 4 (m+1) + 8 n + 8 m */
int khip_spmv_bytes(const khip_csr *A, int64_t *bytes);

/* Profiling hook used by bench.py's roofline leg: with khip_ctx_set_option(ctx, "profile_spmv", 1)
 * every SpMV kernel launch is bracketed by HIP events on the context's stream; this call
 * synchronises, returns the number of launches recorded since the last call and their summed
 * duration, and resets the counters. */
int khip_profile_spmv(khip_ctx *ctx, int64_t *launches, double *total_ms);
/* The same brackets by kernel family (what bench.py's cfg-3 / cfg-5 legs report): launches[t] and total_ms[t] for t < ntags of
 * 0 = SpMV, 1 = SpMM (khip_spmm: the main kernel of a launch), 2 = panel_gemm_tn (V' Q), 3 = panel_nn_tn (the fused block
 * Gram-Schmidt step Q -= V Psi ; Psi' = V' Q), 4 = panel_multi_nn (X += sum V_i Y_i), 5 = panel_gemm_nn, 6 = the panel QR's passes
 * (scale + Gram), 7 = halo pack kernel, 8 = halo transfer (grouped ncclSend / ncclRecv or the all-gather of x, bracketed on the
 * stream it runs on), 9 = a dot's 16-byte all-gather + combine kernel, 10 = the boundary rows' SpMV launch of a row-partitioned
 * product (tag 0 then is the interior launch), 11 / 12 / 13 = the fused passes P1, P2 and P3 of usymqr! (the pass's own kernel, without
 * the reduction's finish kernel), 14 = P3 of usymlq! (its P1 and P2 are 11 and 12), 15 = P3 of trilqr! (likewise), 16 = P3 of tricg! (likewise), 17 = P3 of trimr! (likewise), 18 = P3 of usymlqr! (likewise); at most 19 families.  Synchronises the context's streams and resets every counter. */
int khip_profile_kernels(khip_ctx *ctx, int ntags, int64_t *launches, double *total_ms);

/* ------------------------------------------------ BLAS-1 shim ---------------- */
/* ref: src/krylov_utils.jl:309-349.  x and y may alias exactly (BLAS semantics). */
int khip_dot(khip_ctx *ctx, int64_t n, const double *x, const double *y, double *result_host);      /* kdot  :309-311 (kdotr :313-314) */
int khip_nrm2(khip_ctx *ctx, int64_t n, const double *x, double *result_host);                      /* knorm :316-317 */
int khip_scal(khip_ctx *ctx, int64_t n, double s, double *x);                                       /* kscal! :321-323 */
int khip_div(khip_ctx *ctx, int64_t n, double *x, double s);                                        /* kdiv!  :325-326 (= scal by 1/s) */
int khip_copy(khip_ctx *ctx, int64_t n, double *y, const double *x);                                /* kcopy! :328-329, (dest, src) */
int khip_scalcopy(khip_ctx *ctx, int64_t n, double *y, double s, const double *x);                  /* kscalcopy! :331-332 */
int khip_divcopy(khip_ctx *ctx, int64_t n, double *y, const double *x, double s);                   /* kdivcopy!  :334-335 */
int khip_axpy(khip_ctx *ctx, int64_t n, double s, const double *x, double *y);                      /* kaxpy!  :337-339 */
int khip_axpby(khip_ctx *ctx, int64_t n, double s, const double *x, double t, double *y);           /* kaxpby! :341-345 */
int khip_fill(khip_ctx *ctx, int64_t n, double *x, double val);                                     /* kfill!  :347 */
int khip_ref(khip_ctx *ctx, int64_t n, double *x, double *y, double c, double s);                   /* kref!   :349 */

/* elementwise products for diagonal operators / Jacobi preconditioning (SURVEY.md section 8f N1;
 * ref: M = Diagonal(1 ./ diag(A)) applied through mulorldiv!, src/cg.jl:160,241, test/test_gmres.jl:105-128) */
int khip_vmul(khip_ctx *ctx, int64_t n, double *w, const double *x, const double *y);   /* w = x .* y */
int khip_vdiv(khip_ctx *ctx, int64_t n, double *w, const double *x, const double *y);   /* w = x ./ y */
int khip_csr_diagonal(khip_ctx *ctx, const khip_csr *A, double *diag);                  /* diag[i] = A[i,i] */

/* ------------------------------------------------ fused accelerators --------- */
/* Each equals its unfused sequence on the device up to the last bit of the reduction
 * (elementwise results are bit-identical; reductions agree to <= 1 ulp). */
/* y <- A x ; *result_host = x . y           (src/cg.jl:196-197) */
int khip_spmv_dot(khip_ctx *ctx, const khip_csr *A, const double *x, double *y, double *result_host);
/* x <- x + a p ; r <- r - a q ; *result_host = r . r     (src/cg.jl:239-242 with M = I) */
int khip_axpy2_dot(khip_ctx *ctx, int64_t n, double a, const double *p, const double *q,
                   double *x, double *r, double *result_host);
/* y <- y + a x ; *result_host = y . y                      (src/cg.jl:240,242 with M = I: r <- r - alpha Ap ; r.r) */
int khip_axpy_sqnorm(khip_ctx *ctx, int64_t n, double a, const double *x, double *y, double *result_host);
/* The set-up of cg! with M = I and no warm start (src/cg.jl:153,158,161,162: kfill!(x, 0); kcopy!(r, b); kcopy!(p, r); gamma =
 * kdotr(r, r)) in ONE pass: 8n bytes read, 24n written instead of 48n; x, r, p and gamma hold what the four primitives leave (the
 * all-reduce of gamma included on row-partitioned vectors).  The four vectors must be distinct. */
int khip_cg_setup(khip_ctx *ctx, int64_t n, const double *b, double *x, double *r, double *p, double *result_host);
/* x <- x + a p ; p <- r + b p in one pass over p          (src/cg.jl:239 and :259 = kaxpy!(n, a, p, x) ; kaxpby!(n, 1, r, b, p)).
 * Legal because x is not read between the two reference lines; 40n bytes instead of 48n. */
int khip_cg_update(khip_ctx *ctx, int64_t n, double a, double b, const double *r, double *p, double *x);
/* y <- A x ; *result_host = w . y               (src/bicgstab.jl:221-223: v = A p ; c . v in one pass) */
int khip_spmv_dotw(khip_ctx *ctx, const khip_csr *A, const double *x, double *y, const double *w, double *result_host);
/* y <- A x ; result_host[0] = x . y ; result_host[1] = y . y        (src/bicgstab.jl:228-230: t = A s ; t.s ; t.t) */
int khip_spmv_dot2(khip_ctx *ctx, const khip_csr *A, const double *x, double *y, double *result_host);
/* s <- r - alpha v ; x <- x + alpha y                                (src/bicgstab.jl:224-226) */
int khip_bicgstab_sx(khip_ctx *ctx, int64_t n, double alpha, const double *r, const double *v, const double *y,
                     double *s, double *x);
/* x <- x + omega z ; r <- s - omega t ; result_host = {c . r, r . r}  (src/bicgstab.jl:231-234,240; z may alias s) */
int khip_bicgstab_xr(khip_ctx *ctx, int64_t n, double omega, const double *s, const double *t, const double *z,
                     const double *c, double *x, double *r, double *result_host);
/* p <- r + beta (p - omega v)                                         (src/bicgstab.jl:236-237) */
int khip_bicgstab_p(khip_ctx *ctx, int64_t n, double omega, double beta, const double *v, const double *r, double *p);
/* w <- x + b y  written to w (w may alias x or y): copy + axpy in one pass (src/bicgstab.jl:224-225,232-233) */
int khip_waxpy(khip_ctx *ctx, int64_t n, double *w, const double *x, double b, const double *y);
/* result_host[0] = x . y ; result_host[1] = x . x      (src/bicgstab.jl:230) */
int khip_dot2(khip_ctx *ctx, int64_t n, const double *x, const double *y, double *result_host);
/* Modified Gram-Schmidt cascade against k basis vectors V[0..k) (device pointers in a HOST array),
 * in the reference's order (src/gmres.jl:259-262): for i: h_i = V_i . q ; q <- q - h_i V_i.
 * Runs k+1 dependent kernels with device-resident scalars and ONE host sync; h_host gets the k
 * coefficients, *nrm_host = ||q|| afterwards (src/gmres.jl:274) when nrm_host != NULL.
 * accumulate != 0 adds the coefficients into h_host instead (reorthogonalisation pass :265-271). */
int khip_mgs(khip_ctx *ctx, int64_t n, int k, const double *const *V_host, double *q,
             double *h_host, double *nrm_host, int accumulate);
/* x <- x + sum_i y_i V_i, applied per element in the order i = 0..k-1 (bit-identical to k
 * kaxpy! calls, src/gmres.jl:348-350) */
int khip_multi_axpy(khip_ctx *ctx, int64_t n, int k, const double *y_host,
                    const double *const *V_host, double *x);

/* ------------------------------------------------ panel (block-GMRES) -------- */
/* Panels are n-by-p ROW-MAJOR in HBM (p contiguous; DESIGN.md "panel layout").
 * ref: mul!(R, V', Q) / mul!(Q, V, R, -1, 1) src/block_gmres.jl:244-247, householder!
 * src/block_krylov_utils.jl:201-208, X += V*Y src/block_gmres.jl:324-326. */
/* a panel holds n_pad = n rounded up to 16 rows; the padding rows must be (and stay) zero: khip_panel_gemm_tn and
 * khip_panel_norm read them.  khip_panel_from_colmajor zeroes them itself (P may have held anything); every other entry
 * expects them zero and leaves them zero FOR FINITE FACTORS -- the kernels compute the padding rows like any other row
 * (0 * psi = 0) and do not mask rows >= n, so a factor block with an Inf or NaN turns them into NaN (0 * Inf); the same
 * column of every real row is non-finite then as well.  n = 0: khip_panel_gemm_tn returns Psi = 0, the updates do
 * nothing.  (tests/test_gpu_panel_exact.py) */
int khip_panel_rows(int64_t n, int64_t *n_pad);
int khip_panel_from_colmajor(khip_ctx *ctx, int64_t n, int p, const double *X_colmajor, double *P);
int khip_panel_to_colmajor(khip_ctx *ctx, int64_t n, int p, const double *P, double *X_colmajor);
/* Psi_host (p-by-p, column-major, HOST) <- V^T Q */
int khip_panel_gemm_tn(khip_ctx *ctx, int64_t n, int p, const double *V, const double *Q, double *Psi_host);
/* Q <- beta*Q + alpha * V * Psi  (Psi p-by-p column-major HOST).  beta == 0: the old Q is not read (it may hold NaN), and V
 * may then be Q itself (in-place Q <- Q Psi, same bits as out of place) */
int khip_panel_gemm_nn(khip_ctx *ctx, int64_t n, int p, double alpha, const double *V,
                       const double *Psi_host, double beta, double *Q);
/* Block Gram-Schmidt sweep of Q against the k panels V[0..k) (device pointers in a HOST array) in the reference's
 * order (src/block_gmres.jl:244-247): for i: Psi_i = V_i^T Q ; Q <- Q - V_i Psi_i.  Psi_host receives the k blocks
 * (p x p column-major each, block i at Psi_host + i p p); accumulate != 0 adds them instead (the reorthogonalisation
 * pass :250-256).  On one GPU Psi_{i+1} is formed by the kernel that applies Psi_i (four panel passes per step
 * instead of five, one host synchronisation per sweep); same bits as the khip_panel_gemm_tn / _nn sequence. */
int khip_panel_mgs(khip_ctx *ctx, int64_t n, int p, int k, const double *const *V_host, double *Q, double *Psi_host,
                   int accumulate);
/* X <- beta X + sum_{i < k} V_i Y_i, the products applied in the order i = 0 .. k-1: the k calls mul!(Xr, V[i], Y[i], 1, 1) of
 * the solution update src/block_gmres.jl:324-326 in one pass over X (k + 2 panel passes instead of 3 k).  V_host: k device
 * panel pointers in a HOST array; Y_host: k blocks of p x p, column-major, HOST.  Bit-identical to the k khip_panel_gemm_nn
 * calls.  ctx option "panel_multi_tiles" (default 2; 0 = one tile per wave, factors re-read per tile). */
int khip_panel_multi_nn(khip_ctx *ctx, int64_t n, int p, int k, const double *const *V_host, const double *Y_host, double beta,
                        double *X);
/* Reduced QR of the panel as householder!(Q, R, tau) = kgeqrf! + korgqr! leaves it (src/block_krylov_utils.jl:201-208,
 * :230-236, :254-262): Q overwritten by the orthonormal factor, R_host (p-by-p column-major, upper triangular) and
 * tau_host (p, may be null) with LAPACK's sign convention (R_jj = -sign(alpha_j) |x_j|, tau_j in [1, 2]).  Computed on the
 * device by CholeskyQR2 (shifted CholeskyQR3 for ill-conditioned blocks); the signs and tau come from the top p-by-p block
 * of Q (csrc/block.cpp).  ctx option "panel_signs" = 0 leaves the positive diagonal of the Cholesky factor.  A block without
 * full column rank (equal, dependent or zero columns) is factored as LAPACK factors it: A = Q R with orthonormal Q, zeros on
 * R's diagonal where a column lies in the span of the columns before it and an arbitrary unit vector in Q there; only a
 * block that is zero or not finite altogether is KHIP_ERR_NUMERIC. */
int khip_panel_qr(khip_ctx *ctx, int64_t n, int p, double *Q, double *R_host);
int khip_panel_qr_tau(khip_ctx *ctx, int64_t n, int p, double *Q, double *R_host, double *tau_host);
int khip_panel_norm(khip_ctx *ctx, int64_t n, int p, const double *Q, double *result_host);

/* ------------------------------------------------ multi-GPU ------------------- */
/* One process per GPU.  unique_id is the 128-byte ncclUniqueId created by
 * khip_comm_unique_id on rank 0 and broadcast by the launcher (torch.distributed / MPI). */
int khip_comm_unique_id(void *id128_host);
int khip_comm_init(khip_ctx *ctx, int rank, int nranks, const void *id128_host);
/* In-process backend: all `nranks` ranks are contexts of THIS process (one host thread each; any mix of
 * devices, including several ranks on one GPU), exchanging by device-to-device copies.  Same semantics as
 * the RCCL backend for everything built on top; used to test the distributed path on a single GPU. */
int khip_comm_init_local(khip_ctx *ctx, int rank, int nranks, int hub_id);
int khip_comm_rank(khip_ctx *ctx, int *rank, int *nranks);
/* What the communicator attached to ctx looks like: *rccl_ranks = ncclCommCount of the RCCL communicator (0 for the
 * in-process backend or without a communicator), *local_backend = 1 for khip_comm_init_local, *halo_comm_separate = 1
 * when the halo exchange runs on its own communicator split off the first (csrc/comm.cpp: dot all-gathers on the
 * context's stream and communicator, halo Send/Recv on the second stream and communicator).  Any pointer may be null.
 * ref: the reference's MPI recipe docs/src/custom_workspaces.md:477-586. */
int khip_comm_info(khip_ctx *ctx, int *rank, int *nranks, int *rccl_ranks, int *local_backend, int *halo_comm_separate);
int khip_comm_barrier(khip_ctx *ctx);

/* Host-only helpers of the partition / halo logic (no GPU needed; used by khip_csr_create_dist and
 * by the world_size-2 gloo tests).  ghost_columns: sorted unique columns of rows [row0, row0+m)
 * that fall outside [row0, row0+m) (rowptr is int64, local, 0-based; col global).  halo_plan: given
 * EVERY rank's sorted ghost list (concatenated, offsets ghost_off[nranks+1]) and the partition
 * row_starts[nranks+1], derive for `rank` the per-peer receive segments of its own ghost list
 * (recv_off) and the owned indices it must pack for each peer (send_idx, segments send_off). */
int khip_ghost_columns_host(const int64_t *rowptr, const int32_t *col, int64_t m, int64_t row0,
                            int32_t *out, int64_t cap, int64_t *count);
int khip_halo_plan_host(int rank, int nranks, const int64_t *row_starts, const int32_t *ghost_all,
                        const int64_t *ghost_off, int64_t *recv_off, int64_t *send_off,
                        int32_t *send_idx, int64_t send_cap);

/* ------------------------------------------------ solvers --------------------- */
/* Host control flow of the reference's in-place methods, restated in C++ above the primitives
 * (Julia is absent in this build environment; with Julia the unmodified src/cg.jl etc. drive the
 * same primitives through the k* methods).  Operators: a khip_csr, or a user callback on device
 * pointers (the mul!-based operator contract, docs/src/matrix_free.md:32-34). */
typedef int (*khip_apply_fn)(void *self, const double *x, double *y);   /* y <- Op x, 0 on success */
typedef struct {
  const khip_csr *csr;       /* used when apply == NULL */
  khip_apply_fn   apply;     /* user operator on device pointers */
  void           *self;
} khip_operator;

/* built-in Jacobi preconditioner z <- r ./ diag(A) as an operator for the M / N arguments of the solvers */
int khip_jacobi_create(khip_ctx *ctx, const khip_csr *A, khip_operator *op_out);
int khip_jacobi_destroy(khip_operator *op);

/* ILU(0) of A on its own pattern as an operator y <- U^{-1} L^{-1} x for the M / N arguments; for SPD A this is
 * the IC(0) preconditioner (U = D L^T).  Replaces the vendor ic02 / ilu02 + triangular ldiv! of the
 * reference's GPU recipes (docs/src/gpu.md:74-163, test/gpu/nvidia.jl:37-100).  A must outlive the operator,
 * its column indices must be sorted within rows, every row needs a diagonal entry (KHIP_ERR_NUMERIC
 * otherwise, as for a zero pivot).  Distributed handle: block-Jacobi ILU(0) of the owned diagonal block. */
int khip_ilu0_create(khip_ctx *ctx, const khip_csr *A, khip_operator *op_out);
int khip_ilu0_destroy(khip_operator *op);
/* introspection: number of level-scheduling levels of the two triangular solves; device pointer to the
 * factor values (strict lower part = L without its unit diagonal, upper part incl. diagonal = U) on A's pattern */
int khip_ilu0_info(const khip_operator *op, int64_t *levels_lower, int64_t *levels_upper, const double **lu_dev);
/* replay the 2 x levels launches of one application from a cached hipGraph (default 1) or enqueue them one by one (0) */
int khip_ilu0_set_graph(khip_operator *op, int enable);
/* How the triangular solves are scheduled: dims3 = the grid n1 x n2 x n3 the pattern was recognised as (natural ordering,
 * dependencies towards smaller coordinates; the solves then run block by block, one persistent launch per triangle) or
 * 0, 0, 0 (level scheduling, one launch per level); blocks per triangle; failed = 1 if a bounded wait of the block schedule
 * ever gave up (never expected).  Synchronises the context's stream.  Option "ilu_blocks" = 0 at create keeps level scheduling,
 * = 2 runs the block schedule on packed entry lists only (no row records; for tests), = 3 takes the blocks from the level-sorted
 * row sequence even where a grid is recognised (what patterns without a grid get: dims3 = 0, 0, 0 but blocks > 0). */
int khip_ilu0_block_info(const khip_operator *op, int64_t *dims3, int64_t *blocks, int *failed);
typedef int (*khip_callback_fn)(void *workspace, void *userdata);       /* callback(workspace)::Bool */

typedef struct {
  double atol, rtol;          /* NaN -> sqrt(eps)                 (src/cg.jl:104-105) */
  int    itmax;               /* 0 -> 2n (2*div(n,p) for block)   (src/cg.jl:177) */
  double timemax;             /* NaN or <= 0 -> Inf */
  int    history;             /* push residual norms             (src/cg.jl:165,245) */
  double radius;              /* cg: trust-region radius          (src/cg.jl:215-237) */
  int    linesearch;          /* cg                               (src/cg.jl:198-211) */
  int    restart;             /* gmres / block_gmres              (src/gmres.jl:219-226) */
  int    reorthogonalization; /* gmres / block_gmres              (src/gmres.jl:265-271) */
  int    fused;               /* 0 = issue primitives exactly as the reference does; 1 = fused kernels;
                               * 2 = fused kernels + scalar recurrences and stopping tests on the device (cg, bicgstab: no
                               * host round trip inside the loop; gmres: one-step look-ahead behind the single sync per inner
                               * iteration); bit-identical to 1; falls back to 1 where it does not apply */
  khip_callback_fn callback; void *callback_data;
  int    variant;             /* 0 = the reference's recurrences.  cg: 1 = single-reduction CG (Chronopoulos & Gear 1989): the two
                               * dots of an iteration are computed by ONE reduction (one all-reduce per iteration on N GPUs,
                               * 2 passes per iteration).  Different rounding: same solution to the requested tolerance, iteration
                               * counts within a few of the reference recurrence -- opt-in, own parity budget.
                               * Needs M = I, a CSR operator, no trust region / linesearch / callback (else KHIP_ERR_UNSUPPORTED).
                               * cg: 2 = pipelined CG (Ghysels & Vanroose 2014): r, w = A r and their images are recurred, the one
                               * reduction (r.w, r.r) of an iteration does not feed the product q = A w that runs beside it; on N GPUs
                               * its all-gather, the cross-rank combine and the scalar update run on the communication stream while the
                               * product runs (needs a second communicator, else in order).  104n + SpMV bytes per iteration and two more
                               * work vectors.  Opt-in, own parity budget; same requirements as variant 1.
                               * gmres: 1 = CGS2, classical Gram-Schmidt applied twice instead of the modified Gram-Schmidt cascade of
                               * src/gmres.jl:259-271: h = V_k' q as one reduction per four basis vectors, q -= V_k h in one pass, twice:
                               * three all-reduces per inner iteration on N GPUs instead of k + 1.  Opt-in, own parity budget.
                               * gmres: 2 = s-step GMRES (monomial basis, s = ctx option "gmres_sstep", 1..8, default 4): s products, one batched
                               * CGS2 against the basis and a CholeskyQR2 of the block per s inner iterations -- four reductions per s
                               * iterations; Hessenberg columns, Givens rotations and the stopping test on the host, column by column.
                               * Needs restart = true, a CSR operator, M = N = I, memory x s <= 256.  Opt-in, own parity budget. */
  int    verbose;             /* > 0: the reference's log on stdout, one row every `verbose` iterations (src/cg.jl:132,182-183,224,
                               * 267-269; src/gmres.jl:131,191-192,315,364; src/bicgstab.jl:135,193-194,255-257;
                               * src/block_gmres.jl:120,181-182,297,340; kdisplay: src/krylov_utils.jl:301).  The rows need the scalars
                               * on the host, so a verbose solve runs the host-driven loop (as fused <= 1, and with the reference's
                               * recurrence: variant != 0 has no such rows and is refused with verbose > 0); results are the same bits */
  int    log_fd;              /* where the verbose log goes -- the reference's `iostream` keyword (src/cg.jl:24,182-183; default
                               * stdout): 0 = stdout, otherwise an open file descriptor of the caller (Julia: `fd(io)`), written with
                               * dprintf, never closed by the library */
} khip_options;

typedef struct {              /* SimpleStats, src/krylov_stats.jl:24-44 */
  int    niter, solved, inconsistent, indefinite, npcCount;
  double timer;
  char   status[96];
  const double *residuals; int nres;
  char   error[160];
  double allocation_timer;    /* seconds spent allocating the workspace's vectors: at its creation plus the lazy allocations of
                               * later solves (allocate_if, src/krylov_utils.jl:281-288; stats.allocation_timer, src/krylov_stats.jl) */
} khip_stats;

khip_options khip_default_options(void);

typedef struct khip_cg_workspace          khip_cg_workspace;           /* CgWorkspace       src/krylov_workspaces.jl:236-291 */
typedef struct khip_gmres_workspace       khip_gmres_workspace;        /* GmresWorkspace    :2857-2924 */
typedef struct khip_bicgstab_workspace    khip_bicgstab_workspace;     /* BicgstabWorkspace :1568-1629 */
typedef struct khip_block_gmres_workspace khip_block_gmres_workspace;  /* BlockGmresWorkspace src/block_krylov_workspaces.jl:115-171 */

/* ---- workspaces on CALLER-OWNED vectors ("adopt") -------------------------------------------------------------------
 * The reference's workspaces own their vectors on the Julia side (`x, r, p, Ap :: S`, src/krylov_workspaces.jl:236-291) and
 * `solution(ws) === ws.x` (test/test_interface.jl:260).  A binding that specialises `cg!(ws::CgWorkspace{..,HIPVector}, A, b)`
 * therefore hands the device pointers of THOSE vectors to khip_*_workspace_adopt once, and then runs khip_*_solve -- the fused,
 * device-resident loops -- directly on them: the solution lands in the caller's x, nothing is copied, nothing the caller
 * owns is ever freed or replaced by the library.  Vectors the reference allocates lazily (z, Δx, npc_dir, p, q, yz, t;
 * allocate_if, src/krylov_utils.jl:281-299) are handed over with khip_*_workspace_adopt_vector once the caller has
 * allocated them (ptr == NULL empties the slot again); a solve that needs one the caller never handed over allocates and
 * owns it.  Histories and stats are the same bits as on a khip_*_workspace_create workspace.  After a solve only x and the
 * stats are defined: the other work vectors hold scratch (the reference promises nothing about them either), and the
 * restart-time zero fill of the basis (src/gmres.jl:211-213, src/block_gmres.jl:195-197) is not performed.
 * khip_grow_fn: restart = false lets the basis outgrow `memory`; the library then asks the caller for one more vector
 * (`push!(V, similar(x))`, src/gmres.jl:319-324; a ZEROED panel for block-GMRES, src/block_gmres.jl:300-305) -- return its
 * device pointer, or NULL to fail the solve.  Without a grow callback the library allocates (and owns) the extra vectors. */
typedef double *(*khip_grow_fn)(void *userdata);

int khip_cg_workspace_create(khip_ctx *ctx, int64_t m, int64_t n, khip_cg_workspace **out);
/* CgWorkspace on the caller's x, r, p, Ap (distinct device vectors of n doubles); adopt_vector names: "x", "r", "p", "Ap",
 * "z", "dx" (the reference's Δx: hand it over, then khip_cg_warm_start(ws, dx) only sets the flag), "npc_dir" */
int khip_cg_workspace_adopt(khip_ctx *ctx, int64_t m, int64_t n, double *x, double *r, double *p, double *Ap,
                            khip_cg_workspace **out);
int khip_cg_workspace_adopt_vector(khip_cg_workspace *ws, const char *name, double *ptr);
int khip_cg_workspace_destroy(khip_cg_workspace *ws);
int khip_cg_warm_start(khip_cg_workspace *ws, const double *x0);                   /* warm_start! src/workspace_accessors.jl:193-200 */
/* cg!(ws, A, b; M, ...)  src/cg.jl:120-291.  M == NULL means M = I; otherwise z <- M r. */
int khip_cg_solve(khip_cg_workspace *ws, const khip_operator *A, const khip_operator *M,
                  const double *b, const khip_options *opts);
double           *khip_cg_solution(khip_cg_workspace *ws);                         /* solution(ws) === ws.x */
const khip_stats *khip_cg_stats(khip_cg_workspace *ws);
/* Which loop the workspace's last solve ran: 2 = the device-resident loop (cg!, bicgstab!) / the look-ahead loop (gmres!) --
 * what the default keywords of the reference's entry points get (src/interface.jl:146-154 forwards M = I, ldiv = false,
 * callback = workspace -> false, verbose = 0: the binding maps that default callback to NULL); 1 = the host-driven loop on the
 * fused kernels (a callback, verbose > 0, a preconditioner, a user operator; same bits); 0 = one launch per primitive
 * (options.fused = 0); -1 = no solve yet.  block_gmres!: 1 (it has one loop).  A binding's test asserts on this that an entry
 * point reached the loop it was meant to reach. */
int khip_cg_last_path(khip_cg_workspace *ws);
/* named work vectors for callbacks: "x","r","p","Ap","z","dx","npc_dir" */
double           *khip_cg_vector(khip_cg_workspace *ws, const char *name);
size_t            khip_cg_workspace_bytes(khip_cg_workspace *ws);                  /* storage test, test/test_allocations.jl:41-57 */

/* ---- minres! (src/minres.jl:164-484), real Float64.  MinresWorkspace (src/krylov_workspaces.jl:77-114): window = length of the
 * forward-error window err_vec (the reference's workspace keyword, default 5).  The MINRES-only scalars travel in their own struct;
 * khip_options / khip_stats keep their layout.  NaN in etol / conlim -> the reference's defaults sqrt(eps) / 1 / sqrt(eps). */
typedef struct khip_minres_workspace khip_minres_workspace;
typedef struct {
  double lambda;              /* λ: solve (A + λ I) x = b                     (src/minres.jl:141, 283-285) */
  double etol;                /* forward-error tolerance over the window      (:146, :443) */
  double conlim;              /* condition-number limit                       (:147, :437) */
} khip_minres_params;
khip_minres_params khip_minres_default_params(void);   /* lambda = 0, etol = conlim = NaN */
int khip_minres_workspace_create(khip_ctx *ctx, int64_t m, int64_t n, int window, khip_minres_workspace **out);
/* MinresWorkspace on the caller's x, r1, r2, w1, w2, y (distinct device vectors of n doubles); adopt_vector names: "dx" (Δx: hand
 * it over, then khip_minres_warm_start(ws, dx) only sets the flag), "v" (the preconditioned vector, needed with M), "npc_dir" */
int khip_minres_workspace_adopt(khip_ctx *ctx, int64_t m, int64_t n, int window, double *x, double *r1, double *r2, double *w1,
                                double *w2, double *y, khip_minres_workspace **out);
int khip_minres_workspace_adopt_vector(khip_minres_workspace *ws, const char *name, double *ptr);
int khip_minres_workspace_destroy(khip_minres_workspace *ws);
int khip_minres_warm_start(khip_minres_workspace *ws, const double *x0);
/* minres!(ws, A, b; M, λ, atol, rtol, etol, conlim, itmax, timemax, verbose, history, callback).  M == NULL means M = I, otherwise
 * v <- M r (M must be symmetric positive definite).  options.linesearch != 0 (nonpositive-curvature detection) returns
 * KHIP_ERR_UNSUPPORTED; options.radius / restart / reorthogonalization / variant are ignored.  params == NULL: the defaults.
 * Loops (khip_minres_last_path): 2 = device-resident (CSR operator, M = I, no callback, verbose = 0, window <= 64), 1 = host-driven
 * on the fused kernels (same bits as 2), 0 = one launch per primitive (options.fused = 0). */
int khip_minres_solve(khip_minres_workspace *ws, const khip_operator *A, const khip_operator *M, const double *b,
                      const khip_options *opts, const khip_minres_params *params);
double           *khip_minres_solution(khip_minres_workspace *ws);
const khip_stats *khip_minres_stats(khip_minres_workspace *ws);      /* residuals = the reference's stats.residuals */
/* stats.Aresiduals and stats.Acond of the last solve (history = true), owned by the workspace until its next solve */
int khip_minres_histories(khip_minres_workspace *ws, const double **aresiduals, int *naresiduals, const double **acond,
                          int *nacond);
int khip_minres_last_path(khip_minres_workspace *ws);
/* 1 when the last solve's Lanczos step (y = ((A v + λ v) / β) - (β / oldβ) r1 and v.y) ran inside the CSR handle's product -- the
 * sliced SpMV kernel (khip_spmv_kernel_info 4 on a coded or int32 sliced copy) carries it as an epilogue; 0 when the product and the
 * step were separate passes (other kernels, user operators, options.fused = 0); -1 without a workspace */
int khip_minres_fused_product(khip_minres_workspace *ws);
/* named work vectors: "x", "r1", "r2", "w1", "w2", "y", "v", "dx", "npc_dir" */
double           *khip_minres_vector(khip_minres_workspace *ws, const char *name);
size_t            khip_minres_workspace_bytes(khip_minres_workspace *ws);   /* 6n doubles without M and without warm start */

/* ---- cg_lanczos_shift! (src/cg_lanczos_shift.jl:107-284), real Float64: the family (A + s_i I) x_i = b, i = 1 .. nshifts, from one
 * Lanczos basis.  CgLanczosShiftWorkspace (src/krylov_workspaces.jl:616-660).  The shifts travel in their own struct; khip_options /
 * khip_stats keep their layout (stats.residuals stays empty: each shift's history comes from khip_cg_lanczos_shift_residuals;
 * stats.indefinite = any shift indefinite).  Device footprint: 2 nshifts + 3 vectors of n doubles (x_i, p_i, Mv, Mv_prev, Mv_next),
 * + 1 (v) with M. */
typedef struct khip_cg_lanczos_shift_workspace khip_cg_lanczos_shift_workspace;
typedef struct {
  const double *shifts;       /* host array of nshifts shifts s_i                         (src/cg_lanczos_shift.jl:95) */
  int nshifts;                /* must equal the workspace's                               (:121-122) */
  int check_curvature;        /* freeze the shifts whose (A + s_i I) shows curvature <= 0 (:98, :226-229) */
} khip_cg_lanczos_shift_params;
khip_cg_lanczos_shift_params khip_cg_lanczos_shift_default_params(void);   /* shifts = NULL, nshifts = 0, check_curvature = 0 */
int khip_cg_lanczos_shift_workspace_create(khip_ctx *ctx, int64_t m, int64_t n, int nshifts, khip_cg_lanczos_shift_workspace **out);
/* CgLanczosShiftWorkspace on the caller's Mv, Mv_prev, Mv_next and x[0 .. nshifts), p[0 .. nshifts) (device pointers in HOST arrays);
 * every pointer must be distinct.  adopt_vector names: "v" (the preconditioned vector, needed with M); a pointer that already is
 * another vector of the workspace, x_i and p_i included, is refused. */
int khip_cg_lanczos_shift_workspace_adopt(khip_ctx *ctx, int64_t m, int64_t n, int nshifts, double *Mv, double *Mv_prev,
                                          double *Mv_next, double *const *x, double *const *p, khip_cg_lanczos_shift_workspace **out);
int khip_cg_lanczos_shift_workspace_adopt_vector(khip_cg_lanczos_shift_workspace *ws, const char *name, double *ptr);
int khip_cg_lanczos_shift_workspace_destroy(khip_cg_lanczos_shift_workspace *ws);
/* cg_lanczos_shift!(ws, A, b, shifts; M, check_curvature, atol, rtol, itmax, timemax, verbose, history, callback).  M == NULL means
 * M = I, otherwise v <- M Mv (symmetric positive definite).  No warm start (the reference has none).  Loops
 * (khip_cg_lanczos_shift_last_path): 2 = device-resident (CSR operator, M = I, no callback, verbose = 0, nshifts <= 64), 1 = host-driven
 * on the same kernels (same bits as 2), 0 = one launch per primitive (options.fused = 0). */
int khip_cg_lanczos_shift_solve(khip_cg_lanczos_shift_workspace *ws, const khip_operator *A, const khip_operator *M, const double *b,
                                const khip_options *opts, const khip_cg_lanczos_shift_params *params);
double           *khip_cg_lanczos_shift_solution(khip_cg_lanczos_shift_workspace *ws, int i);   /* x_i, i = 0 .. nshifts - 1 */
const khip_stats *khip_cg_lanczos_shift_stats(khip_cg_lanczos_shift_workspace *ws);
/* stats.residuals[i] of the last solve (history = true), owned by the workspace until its next solve */
int khip_cg_lanczos_shift_residuals(khip_cg_lanczos_shift_workspace *ws, int i, const double **residuals, int *nres);
/* the workspace's per-shift arrays after the last solve, 8 x nshifts doubles in this order: rNorms, σ, δhat, ω, γ, converged, not_cv,
 * stats.indefinite (the last three as 0 / 1) */
int khip_cg_lanczos_shift_arrays(khip_cg_lanczos_shift_workspace *ws, double *out);
int khip_cg_lanczos_shift_last_path(khip_cg_lanczos_shift_workspace *ws);
/* named work vectors: "Mv", "Mv_prev", "Mv_next", "v", "x1" .. "x<nshifts>", "p1" .. "p<nshifts>" */
double           *khip_cg_lanczos_shift_vector(khip_cg_lanczos_shift_workspace *ws, const char *name);
size_t            khip_cg_lanczos_shift_workspace_bytes(khip_cg_lanczos_shift_workspace *ws);   /* (2 nshifts + 3) n doubles without M */

/* ---- bilq! (src/bilq.jl:118-407), real Float64: square nonsymmetric systems by the two-sided Lanczos process on A and A', with the
 * transfer to the BiCG point.  BilqWorkspace (src/krylov_workspaces.jl): uₖ₋₁, uₖ, q, vₖ₋₁, vₖ, p, x, d̅ (8 vectors of n doubles), + Δx
 * with a warm start, + t with M, + s with N (allocated lazily, counted by stats.allocation_timer).  The adjoint travels as its own
 * operator: khip_csr_transpose builds it for a CSR handle (row-partitioned handles included).  options.radius, linesearch, restart,
 * reorthogonalization and variant are ignored.  After a solve only x and the stats are defined: the fused loops rotate the roles of
 * (vₖ₋₁, vₖ) and (uₖ₋₁, uₖ) instead of copying, and khip_bilq_vector returns a name's pointer by its current role. */
typedef struct khip_bilq_workspace khip_bilq_workspace;
typedef struct {
  int transfer_to_bicg;        /* also test and return the BiCG point xᶜ; default 1        (src/bilq.jl:98) */
  const khip_operator *Mt, *Nt; /* adjoints of M, N; NULL = the operator is applied as its own adjoint: right for a diagonal (Jacobi) one only, the caller's duty otherwise */
} khip_bilq_params;
khip_bilq_params khip_bilq_default_params(void);   /* transfer_to_bicg = 1, Mt = Nt = NULL */
int khip_bilq_workspace_create(khip_ctx *ctx, int64_t m, int64_t n, khip_bilq_workspace **out);   /* m != n: KHIP_ERR_INVALID "System must be square" */
/* BilqWorkspace on the caller's eight vectors; every pointer must be distinct.  adopt_vector names: "dx" (Δx: warm_start! fills it on
 * the caller's side and hands it over, then khip_bilq_warm_start(ws, dx) only sets the flag), "t" (needed with M), "s" (needed with N) */
int khip_bilq_workspace_adopt(khip_ctx *ctx, int64_t m, int64_t n, double *u_prev, double *u, double *q, double *v_prev, double *v,
                              double *p, double *x, double *dbar, khip_bilq_workspace **out);
int khip_bilq_workspace_adopt_vector(khip_bilq_workspace *ws, const char *name, double *ptr);
int khip_bilq_workspace_destroy(khip_bilq_workspace *ws);
int khip_bilq_warm_start(khip_bilq_workspace *ws, const double *x0);
/* bilq!(ws, A, b; c, transfer_to_bicg, M, N, atol, rtol, itmax, timemax, verbose, history, callback).  At = A' is required (NULL:
 * KHIP_ERR_INVALID); c == NULL means c = b; M / N == NULL mean the identity, otherwise q <- M A N v and p <- Nt At Mt u.
 * Loops (khip_bilq_last_path): 2 = device-resident (A and At CSR handles, M = N = I, no callback, verbose = 0), 1 = host-driven on the
 * same kernels (same bits as 2), 0 = one launch per primitive (options.fused = 0). */
int khip_bilq_solve(khip_bilq_workspace *ws, const khip_operator *A, const khip_operator *At, const khip_operator *M,
                    const khip_operator *N, const double *b, const double *c, const khip_options *opts, const khip_bilq_params *params);
double           *khip_bilq_solution(khip_bilq_workspace *ws);
const khip_stats *khip_bilq_stats(khip_bilq_workspace *ws);
int khip_bilq_last_path(khip_bilq_workspace *ws);
/* named work vectors: "u_prev", "u", "q", "v_prev", "v", "p", "x", "dbar", "dx", "t", "s" (NULL while not allocated) */
double           *khip_bilq_vector(khip_bilq_workspace *ws, const char *name);
size_t            khip_bilq_workspace_bytes(khip_bilq_workspace *ws);   /* 8n doubles without M, N and warm start */

/* ---- qmr! (src/qmr.jl:124-406), real Float64: square nonsymmetric systems by the same two-sided Lanczos process as bilq!, with the
 * quasi-minimal residual iterate and the residual bound |ζbarₖ₊₁| √τₖ₊₁.  QmrWorkspace (src/krylov_workspaces.jl): uₖ₋₁, uₖ, q, vₖ₋₁,
 * vₖ, p, x, wₖ₋₂, wₖ₋₁ (9 vectors of n doubles), + Δx with a warm start, + t with M, + s with N (allocated lazily, counted by
 * stats.allocation_timer).  The adjoint travels as its own operator, as for bilq!.  options.radius, linesearch, restart,
 * reorthogonalization and variant are ignored.  The fused loops rotate the roles of (vₖ₋₁, vₖ), (uₖ₋₁, uₖ) and (wₖ₋₂, wₖ₋₁) instead
 * of copying or swapping, and khip_qmr_vector returns a name's pointer by its current role: after k iterations every name holds what
 * the reference's variable of that name holds ("w_prev" = wₖ, "w_prev2" = wₖ₋₁), in whichever buffer. */
typedef struct khip_qmr_workspace khip_qmr_workspace;
typedef struct {
  const khip_operator *Mt, *Nt; /* adjoints of M, N; NULL = the operator is applied as its own adjoint: right for a diagonal (Jacobi) one only, the caller's duty otherwise */
} khip_qmr_params;
khip_qmr_params khip_qmr_default_params(void);   /* Mt = Nt = NULL */
int khip_qmr_workspace_create(khip_ctx *ctx, int64_t m, int64_t n, khip_qmr_workspace **out);   /* m != n: KHIP_ERR_INVALID "System must be square" */
/* QmrWorkspace on the caller's nine vectors; every pointer must be distinct.  adopt_vector names: "dx" (Δx: warm_start! fills it on
 * the caller's side and hands it over, then khip_qmr_warm_start(ws, dx) only sets the flag), "t" (needed with M), "s" (needed with N) */
int khip_qmr_workspace_adopt(khip_ctx *ctx, int64_t m, int64_t n, double *u_prev, double *u, double *q, double *v_prev, double *v,
                             double *p, double *x, double *w_prev2, double *w_prev, khip_qmr_workspace **out);
int khip_qmr_workspace_adopt_vector(khip_qmr_workspace *ws, const char *name, double *ptr);
int khip_qmr_workspace_destroy(khip_qmr_workspace *ws);
int khip_qmr_warm_start(khip_qmr_workspace *ws, const double *x0);
/* qmr!(ws, A, b; c, M, N, atol, rtol, itmax, timemax, verbose, history, callback).  At = A' is required (NULL: KHIP_ERR_INVALID);
 * c == NULL means c = b; M / N == NULL mean the identity, otherwise q <- M A N v and p <- Nt At Mt u.
 * Loops (khip_qmr_last_path): 2 = device-resident (A and At CSR handles, M = N = I, no callback, verbose = 0), 1 = host-driven on the
 * same kernels (same bits as 2), 0 = one launch per primitive (options.fused = 0). */
int khip_qmr_solve(khip_qmr_workspace *ws, const khip_operator *A, const khip_operator *At, const khip_operator *M,
                   const khip_operator *N, const double *b, const double *c, const khip_options *opts, const khip_qmr_params *params);
double           *khip_qmr_solution(khip_qmr_workspace *ws);
const khip_stats *khip_qmr_stats(khip_qmr_workspace *ws);
int khip_qmr_last_path(khip_qmr_workspace *ws);
/* named work vectors: "u_prev", "u", "q", "v_prev", "v", "p", "x", "w_prev2", "w_prev", "dx", "t", "s" (NULL while not allocated) */
double           *khip_qmr_vector(khip_qmr_workspace *ws, const char *name);
size_t            khip_qmr_workspace_bytes(khip_qmr_workspace *ws);   /* 9n doubles without M, N and warm start */

/* ---- bilqr! (src/bilqr.jl:116-484), real Float64: the adjoint pair A x = b and Aᴴ y = c from ONE two-sided Lanczos process, the
 * BiLQ iterate (with the BiCG transfer) for the primal system and the QMR iterate for the dual one.  There is no M or N.
 * BilqrWorkspace (src/krylov_workspaces.jl): uₖ₋₁, uₖ, q, vₖ₋₁, vₖ, p, x, y, d̅, wₖ₋₃, wₖ₋₂ ("u_prev", "u", "q", "v_prev", "v", "p", "x",
 * "y", "dbar", "w_prev3", "w_prev2"); Δx and Δy ("dx", "dy") stay empty until a warm start.  The fused loops rotate the roles of
 * (vₖ₋₁, vₖ), (uₖ₋₁, uₖ) and (wₖ₋₃, wₖ₋₂) instead of copying or swapping, and khip_bilqr_vector returns a name's pointer by its current
 * role: after k iterations every name holds what the reference's variable of that name holds, in whichever buffer. */
typedef struct khip_bilqr_workspace khip_bilqr_workspace;
typedef struct {
  int transfer_to_bicg;         /* transfer from the BiLQ point to the BiCG point when it exists (default 1) */
} khip_bilqr_params;
khip_bilqr_params khip_bilqr_default_params(void);   /* transfer_to_bicg = 1 */
int khip_bilqr_workspace_create(khip_ctx *ctx, int64_t m, int64_t n, khip_bilqr_workspace **out);   /* m != n: KHIP_ERR_INVALID "Systems must be square" */
/* BilqrWorkspace on the caller's eleven vectors; every pointer must be distinct.  adopt_vector names: "dx" and "dy" (Δx, Δy:
 * warm_start! fills them on the caller's side and hands them over, then khip_bilqr_warm_start(ws, dx, dy) only sets the flag) */
int khip_bilqr_workspace_adopt(khip_ctx *ctx, int64_t m, int64_t n, double *u_prev, double *u, double *q, double *v_prev, double *v,
                               double *p, double *x, double *y, double *dbar, double *w_prev3, double *w_prev2,
                               khip_bilqr_workspace **out);
int khip_bilqr_workspace_adopt_vector(khip_bilqr_workspace *ws, const char *name, double *ptr);
int khip_bilqr_workspace_destroy(khip_bilqr_workspace *ws);
int khip_bilqr_warm_start(khip_bilqr_workspace *ws, const double *x0, const double *y0);   /* both are required */
/* bilqr!(ws, A, b, c; transfer_to_bicg, atol, rtol, itmax, timemax, verbose, history, callback).  At = A' and c are required (NULL:
 * KHIP_ERR_INVALID).  Loops (khip_bilqr_last_path): 2 = device-resident (A and At CSR handles, no callback, verbose = 0), 1 =
 * host-driven on the same kernels (same bits as 2), 0 = one launch per primitive (options.fused = 0). */
int khip_bilqr_solve(khip_bilqr_workspace *ws, const khip_operator *A, const khip_operator *At, const double *b, const double *c,
                     const khip_options *opts, const khip_bilqr_params *params);
double           *khip_bilqr_solution_x(khip_bilqr_workspace *ws);
double           *khip_bilqr_solution_y(khip_bilqr_workspace *ws);
/* AdjointStats does not fit khip_stats: there solved = solved_primal && solved_dual, residuals = the primal history and status = the
 * first bytes of the full status, cut at a UTF-8 character boundary (four of the reference's strings are longer than status[96]) */
const khip_stats *khip_bilqr_stats(khip_bilqr_workspace *ws);
/* the whole AdjointStats; the arrays and the string belong to the workspace until its next solve; any out pointer may be NULL */
int khip_bilqr_adjoint_stats(khip_bilqr_workspace *ws, int *solved_primal, int *solved_dual, const double **residuals_primal,
                             int *nprimal, const double **residuals_dual, int *ndual, const char **status);
int khip_bilqr_last_path(khip_bilqr_workspace *ws);
/* named work vectors: "u_prev", "u", "q", "v_prev", "v", "p", "x", "y", "dbar", "w_prev3", "w_prev2", "dx", "dy" (NULL while not allocated) */
double           *khip_bilqr_vector(khip_bilqr_workspace *ws, const char *name);
size_t            khip_bilqr_workspace_bytes(khip_bilqr_workspace *ws);   /* 11n doubles without warm start */

/* ---- usymqr! (src/usymqr.jl:130-365), real Float64: A x = b with A of m rows and n columns by the orthogonal tridiagonalisation of
 * Saunders, Simon and Yip, started from b and c; the minimum-residual iterate, with ‖rₖ‖ and ‖Aᴴrₖ₋₁‖ both tested (stats.solved,
 * stats.inconsistent).  There is no M or N.  UsymqrWorkspace (src/krylov_workspaces.jl): vₖ₋₁, vₖ, q (m doubles each), x, wₖ₋₂, wₖ₋₁,
 * uₖ₋₁, uₖ, p (n doubles each); Δx ("dx", n doubles) stays empty until a warm start.  The adjoint travels as its own operator, as for
 * qmr!.  options.radius, linesearch, restart, reorthogonalization and variant are ignored.  The fused loops rotate the roles of
 * (vₖ₋₁, vₖ), (uₖ₋₁, uₖ) and (wₖ₋₂, wₖ₋₁) instead of copying or swapping, and khip_usymqr_vector returns a name's pointer by its current
 * role: after k iterations every name holds what the reference's variable of that name holds ("w_prev" = wₖ, "w_prev2" = wₖ₋₁), in
 * whichever buffer. */
typedef struct khip_usymqr_workspace khip_usymqr_workspace;
int khip_usymqr_workspace_create(khip_ctx *ctx, int64_t m, int64_t n, khip_usymqr_workspace **out);   /* m != n is allowed */
/* UsymqrWorkspace on the caller's nine vectors, in the reference's order; every pointer must be distinct.  adopt_vector names: "dx"
 * (Δx: warm_start! fills it on the caller's side and hands it over, then khip_usymqr_warm_start(ws, dx) only sets the flag) */
int khip_usymqr_workspace_adopt(khip_ctx *ctx, int64_t m, int64_t n, double *v_prev, double *v, double *q, double *x, double *w_prev2,
                                double *w_prev, double *u_prev, double *u, double *p, khip_usymqr_workspace **out);
int khip_usymqr_workspace_adopt_vector(khip_usymqr_workspace *ws, const char *name, double *ptr);
int khip_usymqr_workspace_destroy(khip_usymqr_workspace *ws);
int khip_usymqr_warm_start(khip_usymqr_workspace *ws, const double *x0);
/* usymqr!(ws, A, b, c; atol, rtol, itmax, timemax, verbose, history, callback).  At = A' (n rows, m columns) and c (n doubles) are
 * required (NULL: KHIP_ERR_INVALID); itmax = 0 means m + n of the global system.
 * Loops (khip_usymqr_last_path): 2 = device-resident (m = n, A and At CSR handles, no callback, verbose = 0), 1 = host-driven on the
 * same kernels (same bits as 2), 0 = one launch per primitive (options.fused = 0).  A rectangular system (m != n) runs loop 0
 * whatever options.fused says, and last_path reports 0; a row-partitioned rectangular handle is KHIP_ERR_UNSUPPORTED. */
int khip_usymqr_solve(khip_usymqr_workspace *ws, const khip_operator *A, const khip_operator *At, const double *b, const double *c,
                      const khip_options *opts);
double           *khip_usymqr_solution(khip_usymqr_workspace *ws);
const khip_stats *khip_usymqr_stats(khip_usymqr_workspace *ws);           /* residuals = the reference's stats.residuals */
/* stats.Aresiduals of the last solve (history = true), owned by the workspace until its next solve */
int khip_usymqr_aresiduals(khip_usymqr_workspace *ws, const double **aresiduals, int *naresiduals);
int khip_usymqr_last_path(khip_usymqr_workspace *ws);
/* named work vectors: "v_prev", "v", "q", "x", "w_prev2", "w_prev", "u_prev", "u", "p", "dx" (NULL while not allocated) */
double           *khip_usymqr_vector(khip_usymqr_workspace *ws, const char *name);
size_t            khip_usymqr_workspace_bytes(khip_usymqr_workspace *ws);   /* 3m + 6n doubles without warm start */

/* ---- usymlq! (src/usymlq.jl:124-366), real Float64: the minimum-error counterpart of usymqr! on the same process, A of m rows and
 * n columns, started from b and c; with transfer_to_usymcg the USYMCG point xᶜ is tested as well and returned when it is the one that
 * meets the tolerance.  There is no M or N.  UsymlqWorkspace (src/krylov_workspaces.jl): uₖ₋₁, uₖ, p, x, d̅ (n doubles each), vₖ₋₁, vₖ,
 * q (m doubles each); Δx ("dx", n doubles) stays empty until a warm start.  The adjoint travels as its own operator.
 * options.radius, linesearch, restart, reorthogonalization and variant are ignored.  The fused loops rotate the roles of (vₖ₋₁, vₖ)
 * and (uₖ₋₁, uₖ) instead of copying, and khip_usymlq_vector returns a name's pointer by its current role: after k iterations every
 * name holds what the reference's variable of that name holds ("dbar" = d̅ₖ), in whichever buffer. */
typedef struct khip_usymlq_workspace khip_usymlq_workspace;
typedef struct khip_usymlq_params {
  int transfer_to_usymcg;      /* also test and return the USYMCG point xᶜ; default 1      (src/usymlq.jl:107) */
} khip_usymlq_params;
khip_usymlq_params khip_usymlq_default_params(void);   /* transfer_to_usymcg = 1 */
int khip_usymlq_workspace_create(khip_ctx *ctx, int64_t m, int64_t n, khip_usymlq_workspace **out);   /* m != n is allowed */
/* UsymlqWorkspace on the caller's eight vectors, in the reference's order; every pointer must be distinct.  adopt_vector names: "dx"
 * (Δx: warm_start! fills it on the caller's side and hands it over, then khip_usymlq_warm_start(ws, dx) only sets the flag) */
int khip_usymlq_workspace_adopt(khip_ctx *ctx, int64_t m, int64_t n, double *u_prev, double *u, double *p, double *x, double *dbar,
                                double *v_prev, double *v, double *q, khip_usymlq_workspace **out);
int khip_usymlq_workspace_adopt_vector(khip_usymlq_workspace *ws, const char *name, double *ptr);
int khip_usymlq_workspace_destroy(khip_usymlq_workspace *ws);
int khip_usymlq_warm_start(khip_usymlq_workspace *ws, const double *x0);
/* usymlq!(ws, A, b, c; transfer_to_usymcg, atol, rtol, itmax, timemax, verbose, history, callback).  At = A' (n rows, m columns) and
 * c (n doubles) are required (NULL: KHIP_ERR_INVALID); itmax = 0 means m + n of the global system; params = NULL means the defaults.
 * stats.inconsistent is always 0.
 * Loops (khip_usymlq_last_path): 2 = device-resident (m = n, A and At CSR handles, no callback, verbose = 0), 1 = host-driven on the
 * same kernels (same bits as 2), 0 = one launch per primitive (options.fused = 0).  A rectangular system (m != n) runs loop 0
 * whatever options.fused says, and last_path reports 0; a row-partitioned rectangular handle is KHIP_ERR_UNSUPPORTED. */
int khip_usymlq_solve(khip_usymlq_workspace *ws, const khip_operator *A, const khip_operator *At, const double *b, const double *c,
                      const khip_options *opts, const khip_usymlq_params *params);
double           *khip_usymlq_solution(khip_usymlq_workspace *ws);
const khip_stats *khip_usymlq_stats(khip_usymlq_workspace *ws);           /* residuals = the reference's stats.residuals */
int khip_usymlq_last_path(khip_usymlq_workspace *ws);
/* named work vectors: "u_prev", "u", "p", "x", "dbar", "v_prev", "v", "q", "dx" (NULL while not allocated) */
double           *khip_usymlq_vector(khip_usymlq_workspace *ws, const char *name);
size_t            khip_usymlq_workspace_bytes(khip_usymlq_workspace *ws);   /* 5n + 3m doubles without warm start */

/* ---- trilqr! (src/trilqr.jl:115-460), real Float64: the adjoint pair A x = b and Aᴴ t = c, A of m rows and n columns, from ONE
 * orthogonal tridiagonalisation: x by USYMLQ (with transfer_to_usymcg the USYMCG point xᶜ is tested as well and returned when it is the
 * one that meets the tolerance), t by USYMQR.  Two products per iteration where usymlq! followed by usymqr! takes four.  There is no
 * M or N.  TrilqrWorkspace (src/krylov_workspaces.jl): uₖ₋₁, uₖ, p, d̅, x (n doubles each), vₖ₋₁, vₖ, q, t, wₖ₋₃, wₖ₋₂ (m doubles each)
 * ("u_prev", "u", "p", "dbar", "x", "v_prev", "v", "q", "y", "w_prev3", "w_prev2"); Δx ("dx", n doubles) and Δy ("dy", m doubles)
 * stay empty until a warm start.  The adjoint travels as its own operator.  options.radius, linesearch, restart,
 * reorthogonalization and variant are ignored.  A side that is solved is frozen; the solve ends when both are.  There is no early
 * return for b = 0 or c = 0, as in the reference: that side starts solved and the process goes on from 0 / 0.  The fused loops rotate
 * the roles of (vₖ₋₁, vₖ), (uₖ₋₁, uₖ) and (wₖ₋₃, wₖ₋₂) instead of copying or swapping, and khip_trilqr_vector returns a name's pointer
 * by its current role: after k iterations every name holds what the reference's variable of that name holds, in whichever buffer. */
typedef struct khip_trilqr_workspace khip_trilqr_workspace;
typedef struct khip_trilqr_params {
  int transfer_to_usymcg;      /* also test and return the USYMCG point xᶜ; default 1      (src/trilqr.jl:99) */
} khip_trilqr_params;
khip_trilqr_params khip_trilqr_default_params(void);   /* transfer_to_usymcg = 1 */
int khip_trilqr_workspace_create(khip_ctx *ctx, int64_t m, int64_t n, khip_trilqr_workspace **out);   /* m != n is allowed */
/* TrilqrWorkspace on the caller's eleven vectors, in the reference's order; every pointer must be distinct.  adopt_vector names:
 * "dx" and "dy" (Δx, Δy: warm_start! fills them on the caller's side and hands them over, then khip_trilqr_warm_start(ws, dx, dy)
 * only sets the flag) */
int khip_trilqr_workspace_adopt(khip_ctx *ctx, int64_t m, int64_t n, double *u_prev, double *u, double *p, double *dbar, double *x,
                                double *v_prev, double *v, double *q, double *y, double *w_prev3, double *w_prev2,
                                khip_trilqr_workspace **out);
int khip_trilqr_workspace_adopt_vector(khip_trilqr_workspace *ws, const char *name, double *ptr);
int khip_trilqr_workspace_destroy(khip_trilqr_workspace *ws);
int khip_trilqr_warm_start(khip_trilqr_workspace *ws, const double *x0, const double *y0);   /* both are required: n and m doubles */
/* trilqr!(ws, A, b, c; transfer_to_usymcg, atol, rtol, itmax, timemax, verbose, history, callback).  At = A' (n rows, m columns) and
 * c (n doubles) are required (NULL: KHIP_ERR_INVALID); itmax = 0 means m + n of the global system; params = NULL means the defaults.
 * Loops (khip_trilqr_last_path): 2 = device-resident (m = n, A and At CSR handles, no callback, verbose = 0), 1 = host-driven on the
 * same kernels (same bits as 2), 0 = one launch per primitive (options.fused = 0).  A rectangular system (m != n) runs loop 0
 * whatever options.fused says, and last_path reports 0; a row-partitioned rectangular handle is KHIP_ERR_UNSUPPORTED. */
int khip_trilqr_solve(khip_trilqr_workspace *ws, const khip_operator *A, const khip_operator *At, const double *b, const double *c,
                      const khip_options *opts, const khip_trilqr_params *params);
double           *khip_trilqr_solution_x(khip_trilqr_workspace *ws);
double           *khip_trilqr_solution_y(khip_trilqr_workspace *ws);      /* t, m doubles */
/* AdjointStats does not fit khip_stats: there solved = solved_primal && solved_dual, residuals = the primal history and status = the
 * first bytes of the full status, cut at a UTF-8 character boundary (four of the reference's strings are longer than status[96]).
 * stats.inconsistent carries the dual side's `inconsistent` flag (‖A sₖ₋₁‖ <= ξ), which the reference counts into solved_dual and
 * does not report: an addition to its AdjointStats.  The status can stay "unknown" when the dual side ends by that flag alone. */
const khip_stats *khip_trilqr_stats(khip_trilqr_workspace *ws);
/* the whole AdjointStats; the arrays and the string belong to the workspace until its next solve; any out pointer may be NULL */
int khip_trilqr_adjoint_stats(khip_trilqr_workspace *ws, int *solved_primal, int *solved_dual, const double **residuals_primal,
                              int *nprimal, const double **residuals_dual, int *ndual, const char **status);
int khip_trilqr_last_path(khip_trilqr_workspace *ws);
/* named work vectors: "u_prev", "u", "p", "dbar", "x", "v_prev", "v", "q", "y", "w_prev3", "w_prev2", "dx", "dy" (NULL while not allocated) */
double           *khip_trilqr_vector(khip_trilqr_workspace *ws, const char *name);
size_t            khip_trilqr_workspace_bytes(khip_trilqr_workspace *ws);   /* 5n + 6m doubles without warm start */

/* ---- tricg! (src/tricg.jl:149-484), real Float64, M = N = I: the 2 x 2 block system [τI A; Aᴴ νI] [x; y] = [b; c] for A of m rows and
 * n columns (symmetric quasi-definite, saddle-point, regularised least-squares and least-norm systems), by the Galerkin iterate on
 * the orthogonal tridiagonalisation started from b and c.  x and b have m entries, y and c have n: x is on the ROW side, unlike in
 * usymqr!, usymlq! and trilqr!.  TricgWorkspace (src/krylov_workspaces.jl): y, uₖ₋₁, uₖ, p, gy₂ₖ₋₁, gy₂ₖ (n doubles each), x, vₖ₋₁, vₖ, q,
 * gx₂ₖ₋₁, gx₂ₖ (m doubles each) ("y", "u_prev", "u", "p", "gy_prev", "gy", "x", "v_prev", "v", "q", "gx_prev", "gx"); Δx ("dx", m
 * doubles) and Δy ("dy", n doubles) stay empty until a warm start.  The adjoint travels as its own operator.  options.radius,
 * linesearch, restart, reorthogonalization and variant are ignored.  β₁ = 0 gives v₁ = 0 by a fill (likewise γ₁ and u₁), so b = 0 or
 * c = 0 is an ordinary solve, and b = c = 0 starts solved.  τ = 0 or ν = 0 divides as the reference divides.  The fused loops rotate
 * the roles of (vₖ₋₁, vₖ), (uₖ₋₁, uₖ), (gx₂ₖ₋₁, gx₂ₖ) and (gy₂ₖ₋₁, gy₂ₖ) instead of copying or swapping, and khip_tricg_vector returns a
 * name's pointer by its current role: after k iterations every name holds what the reference's variable of that name holds, in
 * whichever buffer -- EXCEPT "q" and "p": the reference divides them in place by βₖ₊₁ and γₖ₊₁ before it copies them into vₖ₊₁ and
 * uₖ₊₁, loop 0 does the same, and the fused loops write the quotient into vₖ₊₁ and uₖ₊₁ only and leave q and p undivided.
 * Out of scope: M and N other than I, complex types, fused kernels for m != n, a second fused pass that carries the third's work. */
typedef struct khip_tricg_workspace khip_tricg_workspace;
typedef struct khip_tricg_params {
  double tau, nu;              /* τ, ν; defaults 1 and -1                                  (src/tricg.jl:131-132) */
  int spd, snd, flip;          /* spd: τ = ν = 1; snd: τ = ν = -1; flip: τ = -1, ν = 1; at most one (:162-164, :176-178) */
} khip_tricg_params;
khip_tricg_params khip_tricg_default_params(void);   /* τ = 1, ν = -1, no flag */
int khip_tricg_workspace_create(khip_ctx *ctx, int64_t m, int64_t n, khip_tricg_workspace **out);   /* m != n is allowed */
/* TricgWorkspace on the caller's twelve vectors, in the reference's order; every pointer must be distinct.  adopt_vector names:
 * "dx" and "dy" (Δx, Δy: warm_start! fills them on the caller's side and hands them over, then khip_tricg_warm_start(ws, dx, dy)
 * only sets the flag) */
int khip_tricg_workspace_adopt(khip_ctx *ctx, int64_t m, int64_t n, double *y, double *u_prev, double *u, double *p, double *gy_prev,
                               double *gy, double *x, double *v_prev, double *v, double *q, double *gx_prev, double *gx,
                               khip_tricg_workspace **out);
int khip_tricg_workspace_adopt_vector(khip_tricg_workspace *ws, const char *name, double *ptr);
int khip_tricg_workspace_destroy(khip_tricg_workspace *ws);
int khip_tricg_warm_start(khip_tricg_workspace *ws, const double *x0, const double *y0);   /* both are required: m and n doubles */
/* tricg!(ws, A, b, c; spd, snd, flip, τ, ν, atol, rtol, itmax, timemax, verbose, history, callback).  At = A' (n rows, m columns) and
 * c (n doubles) are required (NULL: KHIP_ERR_INVALID); two of spd, snd, flip together are KHIP_ERR_INVALID with the reference's
 * message; itmax = 0 means m + n of the global system; params = NULL means the defaults.  After a warm start the right-hand sides
 * are b - τΔx - AΔy and c - AᴴΔx - νΔy (the τ and ν terms only when the coefficient is not zero).
 * Loops (khip_tricg_last_path): 2 = device-resident (m = n, A and At CSR handles, no callback, verbose = 0), 1 = host-driven on the
 * same kernels (same bits as 2), 0 = one launch per primitive (options.fused = 0).  A rectangular system (m != n) runs loop 0
 * whatever options.fused says, and last_path reports 0; a row-partitioned rectangular handle is KHIP_ERR_UNSUPPORTED.
 * stats: residuals holds ‖r₀‖ and one entry per iteration; inconsistent = !solved && breakdown (βₖ₊₁ and γₖ₊₁ both <= eps^(3/4)). */
int khip_tricg_solve(khip_tricg_workspace *ws, const khip_operator *A, const khip_operator *At, const double *b, const double *c,
                     const khip_options *opts, const khip_tricg_params *params);
double           *khip_tricg_solution_x(khip_tricg_workspace *ws);        /* m doubles */
double           *khip_tricg_solution_y(khip_tricg_workspace *ws);        /* n doubles */
const khip_stats *khip_tricg_stats(khip_tricg_workspace *ws);
int khip_tricg_last_path(khip_tricg_workspace *ws);
/* named work vectors: "y", "u_prev", "u", "p", "gy_prev", "gy", "x", "v_prev", "v", "q", "gx_prev", "gx", "dx", "dy" (NULL while not
 * allocated) */
double           *khip_tricg_vector(khip_tricg_workspace *ws, const char *name);
size_t            khip_tricg_workspace_bytes(khip_tricg_workspace *ws);   /* 6n + 6m doubles without warm start */

/* ---- trimr! (src/trimr.jl:150-577), real Float64, M = N = I: the same 2 x 2 block system [τI A; Aᴴ νI] [x; y] = [b; c] as tricg!, by
 * the minimal-residual iterate on the orthogonal tridiagonalisation started from b and c (a QR factorisation in scalars).  It never
 * divides by τ or ν: saddle-point systems (ν = 0, the sp flag) and adjoint systems (τ = ν = 0) are ordinary solves, and the residual
 * history is non-increasing.  x and b have m entries, y and c have n: x is on the ROW side, as in tricg!.  TrimrWorkspace
 * (src/krylov_workspaces.jl): y, uₖ₋₁, uₖ, p, gy₂ₖ₋₃, gy₂ₖ₋₂, gy₂ₖ₋₁, gy₂ₖ (n doubles each), x, vₖ₋₁, vₖ, q, gx₂ₖ₋₃, gx₂ₖ₋₂, gx₂ₖ₋₁, gx₂ₖ (m doubles each)
 * ("y", "u_prev", "u", "p", "gy_m3", "gy_m2", "gy_m1", "gy", "x", "v_prev", "v", "q", "gx_m3", "gx_m2", "gx_m1", "gx"); Δx ("dx", m
 * doubles) and Δy ("dy", n doubles) stay empty until a warm start.  The adjoint travels as its own operator.  options.radius,
 * linesearch, restart, reorthogonalization and variant are ignored.  β₁ = 0 gives v₁ = 0 by a fill (likewise γ₁ and u₁), so b = 0 or
 * c = 0 is an ordinary solve, and b = c = 0 starts solved.  The fused loops rotate the roles of (vₖ₋₁, vₖ), (uₖ₋₁, uₖ) and of the older
 * and the newer pair of g of each side, (g₂ₖ₋₃, g₂ₖ₋₂) and (g₂ₖ₋₁, g₂ₖ), instead of copying or swapping, and khip_trimr_vector returns a
 * name's pointer by its current role: after k iterations every name holds what the reference's variable of that name holds, in
 * whichever buffer -- EXCEPT "q" and "p": the reference divides them in place by βₖ₊₁ and γₖ₊₁ before it copies them into vₖ₊₁ and
 * uₖ₊₁, loop 0 does the same, and the fused loops write the quotient into vₖ₊₁ and uₖ₊₁ only and leave q and p undivided.
 * Out of scope: M and N other than I, complex types, fused kernels for m != n, Float32. */
typedef struct khip_trimr_workspace khip_trimr_workspace;
typedef struct khip_trimr_params {
  double tau, nu;              /* τ, ν; defaults 1 and -1                                  (src/trimr.jl:132-133) */
  int spd, snd, flip, sp;      /* spd: τ = ν = 1; snd: τ = ν = -1; flip: τ = -1, ν = 1; sp: τ = 1, ν = 0; at most one (:163-168, :180-183) */
} khip_trimr_params;
khip_trimr_params khip_trimr_default_params(void);   /* τ = 1, ν = -1, no flag */
int khip_trimr_workspace_create(khip_ctx *ctx, int64_t m, int64_t n, khip_trimr_workspace **out);   /* m != n is allowed */
/* TrimrWorkspace on the caller's sixteen vectors, in the reference's order; every pointer must be distinct.  adopt_vector names:
 * "dx" and "dy" (Δx, Δy: warm_start! fills them on the caller's side and hands them over, then khip_trimr_warm_start(ws, dx, dy)
 * only sets the flag) */
int khip_trimr_workspace_adopt(khip_ctx *ctx, int64_t m, int64_t n, double *y, double *u_prev, double *u, double *p, double *gy_m3,
                               double *gy_m2, double *gy_m1, double *gy, double *x, double *v_prev, double *v, double *q, double *gx_m3,
                               double *gx_m2, double *gx_m1, double *gx, khip_trimr_workspace **out);
int khip_trimr_workspace_adopt_vector(khip_trimr_workspace *ws, const char *name, double *ptr);
int khip_trimr_workspace_destroy(khip_trimr_workspace *ws);
int khip_trimr_warm_start(khip_trimr_workspace *ws, const double *x0, const double *y0);   /* both are required: m and n doubles */
/* trimr!(ws, A, b, c; spd, snd, flip, sp, τ, ν, atol, rtol, itmax, timemax, verbose, history, callback).  At = A' (n rows, m columns)
 * and c (n doubles) are required (NULL: KHIP_ERR_INVALID); two of spd, snd, flip, sp together are KHIP_ERR_INVALID with the
 * reference's message; itmax = 0 means m + n of the global system; params = NULL means the defaults.  After a warm start the
 * right-hand sides are b - τΔx - AΔy and c - AᴴΔx - νΔy (the τ and ν terms only when the coefficient is not zero).
 * Loops (khip_trimr_last_path): 2 = device-resident (m = n, A and At CSR handles, no callback, verbose = 0), 1 = host-driven on the
 * same kernels (same bits as 2), 0 = one launch per primitive (options.fused = 0).  A rectangular system (m != n) runs loop 0
 * whatever options.fused says, and last_path reports 0; a row-partitioned rectangular handle is KHIP_ERR_UNSUPPORTED.
 * stats: residuals holds ‖r₀‖ and one entry per iteration; inconsistent = !solved && breakdown (βₖ₊₁ and γₖ₊₁ both <= eps^(3/4)). */
int khip_trimr_solve(khip_trimr_workspace *ws, const khip_operator *A, const khip_operator *At, const double *b, const double *c,
                     const khip_options *opts, const khip_trimr_params *params);
double           *khip_trimr_solution_x(khip_trimr_workspace *ws);        /* m doubles */
double           *khip_trimr_solution_y(khip_trimr_workspace *ws);        /* n doubles */
const khip_stats *khip_trimr_stats(khip_trimr_workspace *ws);
int khip_trimr_last_path(khip_trimr_workspace *ws);
/* named work vectors: "y", "u_prev", "u", "p", "gy_m3", "gy_m2", "gy_m1", "gy", "x", "v_prev", "v", "q", "gx_m3", "gx_m2", "gx_m1", "gx",
 * "dx", "dy" (NULL while not allocated) */
double           *khip_trimr_vector(khip_trimr_workspace *ws, const char *name);
size_t            khip_trimr_workspace_bytes(khip_trimr_workspace *ws);   /* 8n + 8m doubles without warm start */

/* ---- usymlqr! (src/usymlqr.jl:136-509), real Float64, no preconditioners: [I A; Aᴴ 0] [x; y] = [b; c] as the sum of the least-squares
 * problem [b; 0] (USYMQR, when ls) and the least-norm problem [0; c] (USYMLQ, when ln) on ONE orthogonal tridiagonalisation and one
 * QR factorisation; each side is frozen once its own test is met.  x and b have m entries, y and c have n: x is on the ROW side, as
 * in tricg!.  UsymlqrWorkspace (src/krylov_workspaces.jl): r, x (m), y, z (n), vₖ₋₁, vₖ (m), uₖ₋₁, uₖ, p (n), q, d̅ (m), wₖ₋₂, wₖ₋₁ (n)
 * ("r", "x", "y", "z", "v_prev", "v", "u_prev", "u", "p", "q", "dbar", "w_m2", "w_m1"); Δx ("dx", m doubles) and Δy ("dy", n doubles)
 * stay empty until a warm start.  The adjoint travels as its own operator.  options.radius, linesearch, restart,
 * reorthogonalization and variant are ignored; the reference's `ldiv` has no meaning without preconditioners.  β₁ = 0 gives v₁ = 0
 * by a fill (likewise γ₁ and u₁), and so do βₖ₊₁ = 0 and γₖ₊₁ = 0 in the loop.  The fused loops rotate the roles of (vₖ₋₁, vₖ), (uₖ₋₁, uₖ) and
 * (wₖ₋₂, wₖ₋₁) instead of copying or swapping, and khip_usymlqr_vector returns a name's pointer by its current role: after k
 * iterations every name holds what the reference's variable of that name holds, in whichever buffer ("q" and "p" too: nothing
 * divides them in place here).  As in the reference: stats.inconsistent is always 0, an `inconsistent` exit leaves the status
 * "unknown", and βₖ₊₁ = 0 in an active least-squares step makes the r coefficient 0 / 0 (r, then x, become NaN).
 * Out of scope: complex types, fused kernels for m != n, Float32. */
typedef struct khip_usymlqr_workspace khip_usymlqr_workspace;
typedef struct khip_usymlqr_params {
  int ls, ln;                  /* solve the least-squares / the least-norm problem; defaults 1 and 1 (src/usymlqr.jl:117-118) */
} khip_usymlqr_params;
khip_usymlqr_params khip_usymlqr_default_params(void);   /* ls = ln = 1 */
int khip_usymlqr_workspace_create(khip_ctx *ctx, int64_t m, int64_t n, khip_usymlqr_workspace **out);   /* m != n is allowed */
/* UsymlqrWorkspace on the caller's thirteen vectors, in the reference's order; every pointer must be distinct.  adopt_vector names:
 * "dx" and "dy" (Δx, Δy: warm_start! fills them on the caller's side and hands them over, then khip_usymlqr_warm_start(ws, dx, dy)
 * only sets the flag) */
int khip_usymlqr_workspace_adopt(khip_ctx *ctx, int64_t m, int64_t n, double *r, double *x, double *y, double *z, double *v_prev, double *v,
                                 double *u_prev, double *u, double *p, double *q, double *dbar, double *w_m2, double *w_m1,
                                 khip_usymlqr_workspace **out);
int khip_usymlqr_workspace_adopt_vector(khip_usymlqr_workspace *ws, const char *name, double *ptr);
int khip_usymlqr_workspace_destroy(khip_usymlqr_workspace *ws);
int khip_usymlqr_warm_start(khip_usymlqr_workspace *ws, const double *x0, const double *y0);   /* both are required: m and n doubles */
/* usymlqr!(ws, A, b, c; ls, ln, atol, rtol, itmax, timemax, verbose, history, callback).  At = A' (n rows, m columns) and c (n
 * doubles) are required (NULL: KHIP_ERR_INVALID); ls = ln = 0 is KHIP_ERR_INVALID with the reference's message; itmax = 0 means
 * m + n of the global system; params = NULL means the defaults.  After a warm start the right-hand sides are b - Δx - AΔy and
 * c - AᴴΔx.
 * Loops (khip_usymlqr_last_path): 2 = device-resident (m = n, A and At CSR handles, no callback, verbose = 0), 1 = host-driven on
 * the same kernels (same bits as 2), 0 = one launch per primitive (options.fused = 0).  A rectangular system (m != n) runs loop 0
 * whatever options.fused says, and last_path reports 0; a row-partitioned rectangular handle is KHIP_ERR_UNSUPPORTED.
 * stats: residuals holds, per iteration, ‖rₖ‖ of the least-squares side and then ‖rₖ‖ of the least-norm side, each while its side is
 * active, and nothing for iteration 0; khip_usymlqr_aresiduals is ‖Aᴴrₖ₋₁‖ of the least-squares side. */
int khip_usymlqr_solve(khip_usymlqr_workspace *ws, const khip_operator *A, const khip_operator *At, const double *b, const double *c,
                       const khip_options *opts, const khip_usymlqr_params *params);
double           *khip_usymlqr_solution_x(khip_usymlqr_workspace *ws);      /* m doubles */
double           *khip_usymlqr_solution_y(khip_usymlqr_workspace *ws);      /* n doubles */
const khip_stats *khip_usymlqr_stats(khip_usymlqr_workspace *ws);
/* the Aresiduals history (valid until the next solve or destroy) */
int khip_usymlqr_aresiduals(khip_usymlqr_workspace *ws, const double **aresiduals, int *naresiduals);
int khip_usymlqr_last_path(khip_usymlqr_workspace *ws);
/* named work vectors: "r", "x", "y", "z", "v_prev", "v", "u_prev", "u", "p", "q", "dbar", "w_m2", "w_m1", "dx", "dy" (NULL while not
 * allocated) */
double           *khip_usymlqr_vector(khip_usymlqr_workspace *ws, const char *name);
size_t            khip_usymlqr_workspace_bytes(khip_usymlqr_workspace *ws);   /* 6m + 7n doubles without warm start */

/* ---- cgs! (src/cgs.jl:126-281), real Float64: square nonsymmetric systems by the conjugate gradient squared recurrence; transpose-
 * free (no A'), two products with A per iteration.  CgsWorkspace (src/krylov_workspaces.jl): x, r, u, p, q, ts; Δx, yz and vw ("dx",
 * "yz", "vw") stay empty until a warm start, N or M needs them.  options.variant != 0 is refused (there is no other recurrence);
 * window, reorthogonalization and restart are ignored. */
typedef struct khip_cgs_workspace khip_cgs_workspace;
int khip_cgs_workspace_create(khip_ctx *ctx, int64_t m, int64_t n, khip_cgs_workspace **out);
/* CgsWorkspace on the caller's six vectors; every pointer must be distinct.  adopt_vector names: "dx" (Δx: warm_start! fills it on the
 * caller's side and hands it over, then khip_cgs_warm_start(ws, dx) only sets the flag), "yz" (needed with N), "vw" (needed with M) */
int khip_cgs_workspace_adopt(khip_ctx *ctx, int64_t m, int64_t n, double *x, double *r, double *u, double *p, double *q, double *ts,
                             khip_cgs_workspace **out);
int khip_cgs_workspace_adopt_vector(khip_cgs_workspace *ws, const char *name, double *ptr);
int khip_cgs_workspace_destroy(khip_cgs_workspace *ws);
int khip_cgs_warm_start(khip_cgs_workspace *ws, const double *x0);
/* cgs!(ws, A, b; c, M, N, atol, rtol, itmax, timemax, verbose, history, callback).  c == NULL means c = b; M / N == NULL mean the
 * identity.  m != n: KHIP_ERR_INVALID "System must be square".  Loops (khip_cgs_last_path): 2 = device-resident (A a CSR handle,
 * M = N = I, no callback, verbose = 0), 1 = host-driven on the same kernels (same bits as 2), 0 = one launch per primitive
 * (options.fused = 0). */
int khip_cgs_solve(khip_cgs_workspace *ws, const khip_operator *A, const khip_operator *M, const khip_operator *N, const double *b,
                   const double *c, const khip_options *opts);
double           *khip_cgs_solution(khip_cgs_workspace *ws);
const khip_stats *khip_cgs_stats(khip_cgs_workspace *ws);
int khip_cgs_last_path(khip_cgs_workspace *ws);
/* named work vectors: "x", "r", "u", "p", "q", "ts", "dx", "yz", "vw" (NULL while not allocated) */
double           *khip_cgs_vector(khip_cgs_workspace *ws, const char *name);
size_t            khip_cgs_workspace_bytes(khip_cgs_workspace *ws);   /* 6n doubles without M, N and warm start */

/* ---- symmlq! (src/symmlq.jl:132-464), real Float64: (A + λI) x = b with A symmetric, possibly indefinite; the iterate xᴸ minimises
 * the error, and the CG point xᶜ is handed back when it is good enough (transfer_to_cg).  SymmlqWorkspace
 * (src/krylov_workspaces.jl:461-476): x, Mvold, Mv, Mv_next, w̅ ("wbar"); Δx and v ("dx", "v") stay empty until a warm start or M
 * needs them; clist, zlist and sprod (window entries each) live in the library.  options.variant != 0 is refused (there is no other
 * recurrence); radius, linesearch, reorthogonalization and restart are ignored. */
typedef struct khip_symmlq_workspace khip_symmlq_workspace;
typedef struct {
  double lambda;       /* λ */
  double lambda_est;   /* λest: 0 = no error estimates */
  double etol;         /* NaN: the reference's default, √eps */
  double conlim;       /* NaN: the reference's default, 1 / √eps */
  int transfer_to_cg;  /* default 1 */
} khip_symmlq_params;
khip_symmlq_params khip_symmlq_default_params(void);   /* lambda = lambda_est = 0, etol = conlim = NaN, transfer_to_cg = 1 */
int khip_symmlq_workspace_create(khip_ctx *ctx, int64_t m, int64_t n, int window, khip_symmlq_workspace **out);
/* SymmlqWorkspace on the caller's five vectors; every pointer must be distinct.  adopt_vector names: "dx" (Δx: warm_start! fills it
 * on the caller's side and hands it over, then khip_symmlq_warm_start(ws, dx) only sets the flag), "v" (needed with M).  The fused
 * loops rotate the roles of (Mvold, Mv, Mv_next) where the reference copies: khip_symmlq_vector returns a name's pointer by its
 * current role, so after a solve every name holds what the reference's variable of that name holds. */
int khip_symmlq_workspace_adopt(khip_ctx *ctx, int64_t m, int64_t n, int window, double *x, double *Mvold, double *Mv,
                                double *Mv_next, double *wbar, khip_symmlq_workspace **out);
int khip_symmlq_workspace_adopt_vector(khip_symmlq_workspace *ws, const char *name, double *ptr);
int khip_symmlq_workspace_destroy(khip_symmlq_workspace *ws);
int khip_symmlq_warm_start(khip_symmlq_workspace *ws, const double *x0);
/* symmlq!(ws, A, b; M, transfer_to_cg, λ, λest, atol, rtol, etol, conlim, itmax, timemax, verbose, history, callback).  M == NULL
 * means the identity; params == NULL: the defaults.  m != n: KHIP_ERR_INVALID "System must be square"; ⟨v, Mv⟩ < 0:
 * KHIP_ERR_INVALID "Preconditioner is not positive definite" (also where the reference takes the square root of ⟨b, M b⟩ < 0).  The
 * status strings are the reference's, in UTF-8:
 *   "solution xᴸ good enough given atol and rtol", "solution xᶜ good enough given atol and rtol", "found approximate solution", ...
 * Loops (khip_symmlq_last_path): 2 = device-resident (A a CSR handle, M = I, λest = 0, no callback, verbose = 0), 1 = host-driven on
 * the same kernels (same bits as 2), 0 = one launch per primitive (options.fused = 0). */
int khip_symmlq_solve(khip_symmlq_workspace *ws, const khip_operator *A, const khip_operator *M, const double *b,
                      const khip_options *opts, const khip_symmlq_params *params);
double           *khip_symmlq_solution(khip_symmlq_workspace *ws);
const khip_stats *khip_symmlq_stats(khip_symmlq_workspace *ws);      /* residuals = the reference's stats.residuals */
/* stats.residualscg, stats.errors and stats.errorscg of the last solve (history = true), owned by the workspace until its next
 * solve.  Where the reference stores `missing` (no CG point: γbar = 0) the entry is NaN.  errors and errorscg are empty unless
 * λest != 0. */
int khip_symmlq_histories(khip_symmlq_workspace *ws, const double **residualscg, int *nresidualscg, const double **errors,
                          int *nerrors, const double **errorscg, int *nerrorscg);
/* stats.Anorm and stats.Acond of the last solve (NaN after "x is a zero-residual solution", as in the reference) */
int khip_symmlq_norms(khip_symmlq_workspace *ws, double *Anorm, double *Acond);
int khip_symmlq_last_path(khip_symmlq_workspace *ws);
/* named work vectors: "x", "Mvold", "Mv", "Mv_next", "wbar", "dx", "v" (NULL while not allocated) */
double           *khip_symmlq_vector(khip_symmlq_workspace *ws, const char *name);
size_t            khip_symmlq_workspace_bytes(khip_symmlq_workspace *ws);   /* 5n doubles without M and warm start */

/* ---- minres_qlp! (src/minres_qlp.jl:131-538), real Float64: (A + λI) x = b with A symmetric, possibly indefinite or SINGULAR; on a
 * singular inconsistent system the iterate is the minimum-length least-squares solution.  MinresQlpWorkspace
 * (src/krylov_workspaces.jl:713-768): x, wₖ₋₁, wₖ, M⁻¹vₖ₋₁, M⁻¹vₖ, p ("x", "wkm1", "wk", "Mvkm1", "Mvk", "p"); Δx and vₖ ("dx", "vk")
 * stay empty until a warm start or M needs them.  options.linesearch: KHIP_ERR_UNSUPPORTED; options.variant != 0 is refused (there
 * is no other recurrence); radius, reorthogonalization and restart are ignored. */
typedef struct khip_minres_qlp_workspace khip_minres_qlp_workspace;
typedef struct {
  double lambda;       /* λ */
  double Artol;        /* NaN: the reference's default, √eps */
} khip_minres_qlp_params;
khip_minres_qlp_params khip_minres_qlp_default_params(void);   /* lambda = 0, Artol = NaN */
int khip_minres_qlp_workspace_create(khip_ctx *ctx, int64_t m, int64_t n, khip_minres_qlp_workspace **out);
/* MinresQlpWorkspace on the caller's six vectors; every pointer must be distinct.  adopt_vector names: "dx" (Δx: warm_start! fills
 * it on the caller's side and hands it over, then khip_minres_qlp_warm_start(ws, dx) only sets the flag), "vk" (needed with M).
 * The fused loops rotate the roles of (Mvkm1, Mvk, p) where the reference copies and swap those of (wkm1, wk) where it swaps:
 * khip_minres_qlp_vector returns a name's pointer by its current role, so after a solve every name holds what the reference's
 * variable of that name holds (p is scratch there: the fused loops leave M⁻¹vₖ₋₂ in it). */
int khip_minres_qlp_workspace_adopt(khip_ctx *ctx, int64_t m, int64_t n, double *x, double *wkm1, double *wk, double *Mvkm1,
                                    double *Mvk, double *p, khip_minres_qlp_workspace **out);
int khip_minres_qlp_workspace_adopt_vector(khip_minres_qlp_workspace *ws, const char *name, double *ptr);
int khip_minres_qlp_workspace_destroy(khip_minres_qlp_workspace *ws);
int khip_minres_qlp_warm_start(khip_minres_qlp_workspace *ws, const double *x0);
/* minres_qlp!(ws, A, b; M, λ, atol, rtol, Artol, itmax, timemax, verbose, history, callback).  M == NULL means the identity;
 * params == NULL: the defaults.  m != n: KHIP_ERR_INVALID "System must be square"; ⟨v, Mv⟩ < 0: KHIP_ERR_NUMERIC "Preconditioner is
 * not positive definite".  stats.inconsistent is the reference's flag; the status strings are the reference's:
 *   "found approximate minimum least-squares solution", "found approximate zero-residual solution",
 *   "solution good enough given atol and rtol", ...
 * Loops (khip_minres_qlp_last_path): 2 = device-resident (A a CSR handle, M = I, no callback, verbose = 0), 1 = host-driven on the
 * same kernels (same bits as 2), 0 = one launch per primitive (options.fused = 0).  A callback on loop 1 finds every named vector
 * in the reference's state of that point (the division of vₖ₊₁ by βₖ₊₁ is not carried forward then). */
int khip_minres_qlp_solve(khip_minres_qlp_workspace *ws, const khip_operator *A, const khip_operator *M, const double *b,
                          const khip_options *opts, const khip_minres_qlp_params *params);
double           *khip_minres_qlp_solution(khip_minres_qlp_workspace *ws);
const khip_stats *khip_minres_qlp_stats(khip_minres_qlp_workspace *ws);      /* residuals = the reference's stats.residuals */
/* stats.Aresiduals and stats.Acond of the last solve (history = true), owned by the workspace until its next solve; Acond has one
 * entry more than Aresiduals (the reference pushes it before the loop as well) */
int khip_minres_qlp_histories(khip_minres_qlp_workspace *ws, const double **aresiduals, int *naresiduals, const double **acond,
                              int *nacond);
int khip_minres_qlp_last_path(khip_minres_qlp_workspace *ws);
/* 1 when the last solve's Lanczos step (p = A vₖ + λ vₖ - βₖ M⁻¹vₖ₋₁ and αₖ = vₖ.p) ran inside the CSR handle's product, as for
 * khip_minres_fused_product; 0 when the product and the step were separate passes; -1 without a workspace */
int khip_minres_qlp_fused_product(khip_minres_qlp_workspace *ws);
/* named work vectors: "x", "wkm1", "wk", "Mvkm1", "Mvk", "p", "dx", "vk" (NULL while not allocated) */
double           *khip_minres_qlp_vector(khip_minres_qlp_workspace *ws, const char *name);
size_t            khip_minres_qlp_workspace_bytes(khip_minres_qlp_workspace *ws);   /* 6n doubles without M and warm start */

int khip_gmres_workspace_create(khip_ctx *ctx, int64_t m, int64_t n, int memory, khip_gmres_workspace **out);
/* GmresWorkspace on the caller's x, w and basis V_host[0 .. memory) (device pointers in a HOST array; `V::Vector{S}`,
 * src/krylov_workspaces.jl:2857-2873).  adopt_vector names: "x", "w", "p", "q", "dx".  adopt_basis replaces the whole list
 * (k >= memory: the caller's V after restart = false grew it).  khip_gmres_host_state copies c, s, z (cap entries each at
 * most) and the packed R (cap (cap + 1) / 2) of the last solve out, *len = their current length, *inner_iter as the
 * reference's field; any output may be NULL. */
int khip_gmres_workspace_adopt(khip_ctx *ctx, int64_t m, int64_t n, int memory, double *x, double *w,
                               double *const *V_host, khip_gmres_workspace **out);
int khip_gmres_workspace_adopt_vector(khip_gmres_workspace *ws, const char *name, double *ptr);
int khip_gmres_workspace_adopt_basis(khip_gmres_workspace *ws, int k, double *const *V_host);
int khip_gmres_workspace_set_grow(khip_gmres_workspace *ws, khip_grow_fn grow, void *userdata);
int khip_gmres_host_state(khip_gmres_workspace *ws, int cap, double *c_host, double *s_host, double *z_host, double *R_host,
                          int *len, int *inner_iter);
int khip_gmres_workspace_destroy(khip_gmres_workspace *ws);
int khip_gmres_warm_start(khip_gmres_workspace *ws, const double *x0);
/* gmres!(ws, A, b; M, N, restart, reorthogonalization, ...)  src/gmres.jl:121-384 */
int khip_gmres_solve(khip_gmres_workspace *ws, const khip_operator *A, const khip_operator *M,
                     const khip_operator *N, const double *b, const khip_options *opts);
double           *khip_gmres_solution(khip_gmres_workspace *ws);
const khip_stats *khip_gmres_stats(khip_gmres_workspace *ws);
int khip_gmres_last_path(khip_gmres_workspace *ws);
size_t            khip_gmres_workspace_bytes(khip_gmres_workspace *ws);

int khip_bicgstab_workspace_create(khip_ctx *ctx, int64_t m, int64_t n, khip_bicgstab_workspace **out);
/* BicgstabWorkspace on the caller's x, r, p, v, s, qd (src/krylov_workspaces.jl:1568-1582); adopt_vector names: those six and
 * "yz", "t", "dx" */
int khip_bicgstab_workspace_adopt(khip_ctx *ctx, int64_t m, int64_t n, double *x, double *r, double *p, double *v, double *s,
                                  double *qd, khip_bicgstab_workspace **out);
int khip_bicgstab_workspace_adopt_vector(khip_bicgstab_workspace *ws, const char *name, double *ptr);
int khip_bicgstab_workspace_destroy(khip_bicgstab_workspace *ws);
int khip_bicgstab_warm_start(khip_bicgstab_workspace *ws, const double *x0);
/* bicgstab!(ws, A, b; c, M, N, ...)  src/bicgstab.jl:125-277 ; c == NULL -> c = b */
int khip_bicgstab_solve(khip_bicgstab_workspace *ws, const khip_operator *A, const khip_operator *M,
                        const khip_operator *N, const double *b, const double *c,
                        const khip_options *opts);
double           *khip_bicgstab_solution(khip_bicgstab_workspace *ws);
const khip_stats *khip_bicgstab_stats(khip_bicgstab_workspace *ws);
int khip_bicgstab_last_path(khip_bicgstab_workspace *ws);
size_t            khip_bicgstab_workspace_bytes(khip_bicgstab_workspace *ws);

int khip_block_gmres_workspace_create(khip_ctx *ctx, int64_t m, int64_t n, int p, int memory,
                                      khip_block_gmres_workspace **out);
/* BlockGmresWorkspace on the caller's panels X, W, V_host[0 .. memory): row-major panels of khip_panel_rows(n) x p doubles
 * with zero padding rows (the tall blocks of a BlockGmresWorkspace{..,HIPMatrix}, src/block_krylov_workspaces.jl:115-163;
 * the small blocks stay inside the library).  adopt_panel names: "X", "W", "P", "Q", "dX". */
int khip_block_gmres_workspace_adopt(khip_ctx *ctx, int64_t m, int64_t n, int p, int memory, double *X, double *W,
                                     double *const *V_host, khip_block_gmres_workspace **out);
int khip_block_gmres_workspace_adopt_panel(khip_block_gmres_workspace *ws, const char *name, double *ptr);
int khip_block_gmres_workspace_adopt_basis(khip_block_gmres_workspace *ws, int k, double *const *V_host);
int khip_block_gmres_workspace_set_grow(khip_block_gmres_workspace *ws, khip_grow_fn grow, void *userdata);
int khip_block_gmres_workspace_destroy(khip_block_gmres_workspace *ws);
int khip_block_gmres_warm_start(khip_block_gmres_workspace *ws, const double *X0_colmajor);
int khip_block_gmres_warm_start_panel(khip_block_gmres_workspace *ws, const double *X0_panel);   /* X0 already a row-major panel */
/* block_gmres!(ws, A, B; restart, reorthogonalization, ...) src/block_gmres.jl:110-358.
 * B and the solution are n-by-p COLUMN-MAJOR device arrays (the reference layout); the
 * workspace converts to row-major panels internally.  A: CSR handle (SpMM kernel) or an apply
 * callback; M / N: NULL (= I) or apply callbacks.  Callbacks of the block solver receive ROW-MAJOR
 * device panels of khip_panel_rows(n) x p doubles (padding rows zero, and they must stay zero). */
int khip_block_gmres_solve(khip_block_gmres_workspace *ws, const khip_operator *A, const khip_operator *M,
                           const khip_operator *N, const double *B_colmajor, const khip_options *opts);
/* the same with B a row-major panel (khip_panel_rows(n) x p, zero padding rows) read in place; the solution is the X panel */
int khip_block_gmres_solve_panel(khip_block_gmres_workspace *ws, const khip_operator *A, const khip_operator *M,
                                 const khip_operator *N, const double *B_panel, const khip_options *opts);
int khip_block_gmres_get_X(khip_block_gmres_workspace *ws, double *X_colmajor);
const khip_stats *khip_block_gmres_stats(khip_block_gmres_workspace *ws);
int khip_block_gmres_last_path(khip_block_gmres_workspace *ws);
/* storage test (test/test_allocations.jl:734-761): bytes of the workspace with n x p blocks at their logical size;
 * *extra_bytes (may be null) = what this implementation holds beyond the reference's formula (the row-major panel copy
 * of B and the p x p staging blocks of the fused sweeps) */
size_t            khip_block_gmres_workspace_bytes(khip_block_gmres_workspace *ws, size_t *extra_bytes);

/* ---- Krylov processes (src/krylov_processes.jl) --------------------------------------------------------------
 * The bases are dense COLUMN-MAJOR device arrays as in the reference (`M(undef, n, k+1)`): column j starts at
 * V + j*ldv, ldv >= n and even, V 16-byte aligned.  The small matrices come back on the HOST in the reference's
 * own storage.  An exact breakdown returns KHIP_ERR_NUMERIC with the reference's message in khip_last_error()
 * unless allow_breakdown != 0 (the new basis vector is then zero-filled, as the reference does).
 * Row-partitioned operators: n (and m) are the local row counts; dots and norms are all-reduced inside. */
/* V, beta1, T = hermitian_lanczos(A, b, k; allow_breakdown, reorthogonalization)     src/krylov_processes.jl:28-102
 * T_nzval_host[3k-1] = nzval of the (k+1) x k tridiagonal SparseMatrixCSC of :35-48: column 1 holds (T11, T21),
 * column i >= 2 holds (T[i-1,i], T[i,i], T[i+1,i]). */
int khip_hermitian_lanczos(khip_ctx *ctx, const khip_operator *A, int64_t n, const double *b, int k,
                           int allow_breakdown, int reorthogonalization, double *V, int64_t ldv,
                           double *beta1_host, double *T_nzval_host);
/* V, beta, H = arnoldi(A, b, k; allow_breakdown, reorthogonalization)                 src/krylov_processes.jl:250-296
 * H_host = dense (k+1) x k upper Hessenberg, column-major with leading dimension k+1. */
int khip_arnoldi(khip_ctx *ctx, const khip_operator *A, int64_t n, const double *b, int k, int allow_breakdown,
                 int reorthogonalization, double *V, int64_t ldv, double *beta_host, double *H_host);
/* V, U, beta1, L = golub_kahan(A, b, k; allow_breakdown)                              src/krylov_processes.jl:323-398
 * A is m x n, At its adjoint (khip_csr_transpose or a callback); V is n x (k+1), U is m x (k+1);
 * L_nzval_host[2k+1] = nzval of the (k+1) x (k+1) lower bidiagonal SparseMatrixCSC of :331-347:
 * (L11, L21, L22, L32, ..., L[k+1,k], L[k+1,k+1]). */
int khip_golub_kahan(khip_ctx *ctx, const khip_operator *A, const khip_operator *At, int64_t m, int64_t n,
                     const double *b, int k, int allow_breakdown, double *V, int64_t ldv, double *U, int64_t ldu,
                     double *beta1_host, double *L_nzval_host);
/* V, beta1, T, U, gamma1, Tt = nonhermitian_lanczos(A, b, c, k; allow_breakdown)   src/krylov_processes.jl:133-222
 * A square, At its adjoint; V, U are n x (k+1); T_nzval_host / Tt_nzval_host [3k-1] = nzval of T and of T^H in the
 * tridiagonal pattern above (column i: T[i-1,i] = gamma_i, T[i,i] = alpha_i, T[i+1,i] = beta_{i+1}). */
int khip_nonhermitian_lanczos(khip_ctx *ctx, const khip_operator *A, const khip_operator *At, int64_t n, const double *b,
                              const double *c, int k, int allow_breakdown, double *V, int64_t ldv, double *U, int64_t ldu,
                              double *beta1_host, double *gamma1_host, double *T_nzval_host, double *Tt_nzval_host);
/* V, beta1, T, U, gamma1, Tt = saunders_simon_yip(A, b, c, k; allow_breakdown)      src/krylov_processes.jl:431-524
 * A is m x n; V is m x (k+1), U is n x (k+1); same storage of T and T^H as above. */
int khip_saunders_simon_yip(khip_ctx *ctx, const khip_operator *A, const khip_operator *At, int64_t m, int64_t n,
                            const double *b, const double *c, int k, int allow_breakdown, double *V, int64_t ldv,
                            double *U, int64_t ldu, double *beta1_host, double *gamma1_host, double *T_nzval_host,
                            double *Tt_nzval_host);
/* V, beta, H, U, gamma, F = montoison_orban(A, B, b, c, k; allow_breakdown, reorthogonalization)
 *                                                                                   src/krylov_processes.jl:553-632
 * A is m x n, B is n x m; V is m x (k+1), U is n x (k+1); H_host, F_host dense (k+1) x k column-major. */
int khip_montoison_orban(khip_ctx *ctx, const khip_operator *A, const khip_operator *B, int64_t m, int64_t n,
                         const double *b, const double *c, int k, int allow_breakdown, int reorthogonalization,
                         double *V, int64_t ldv, double *U, int64_t ldu, double *beta_host, double *gamma_host,
                         double *H_host, double *F_host);

#ifdef __cplusplus
}
#endif
#endif /* KRYLOV_HIP_H */
