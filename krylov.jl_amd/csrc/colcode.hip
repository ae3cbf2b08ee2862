// colcode.hip -- dictionary-coded column indices for the staged SpMV (spmv_code_kernel, spmv.hip).
//
// A banded / stencil operator touches few distinct DIAGONALS d = column - row: get_div_grad(n1,n2,n3)
// (test/get_div_grad.jl:8-25) has 7 whatever the grid size, the kron-unsymmetric operator 7, the 27-point operator 27,
// and a rank's renumbered [owned | ghost] slab two more (every ghost plane sits at one constant offset from the rows
// that reference it).  When all entries of a handle lie on at most 256 diagonals the handle keeps, NEXT TO its CSR
// arrays, one byte per entry: the rank of d in the ascending table of distinct diagonals (two bytes up to 2048
// diagonals).  The staged SpMV then streams 8 + 1 bytes per entry instead of 8 + 4 and rebuilds col = row + tab[code]
// with exact integer arithmetic, so nothing about the product changes -- not the order of the entries, not a bit of y.
// The boundary (khip_csr_create, src/krylov_utils.jl:305 kmul!) still takes and keeps plain CSR; every other kernel
// (SpMM, transpose, ILU, halo plan) reads the int32 columns.  Operators with more diagonals simply stay on the int32 stream.
//
// Construction, on the device, at the first product that can use it: every row inserts its offsets into a 4096-slot
// open-addressing table (read first, atomicCAS only on an empty slot -> after the first few workgroups the pass is a
// read-only stream of col), the host sorts the <= 2048 keys (deterministic), a second pass writes rank(d) per entry.
#include <algorithm>
#include <cstring>

#include "spmv_common.hpp"

namespace khip {

constexpr int kCodeHash = 4096;            // slots (power of two)
constexpr int kCodeMax = 2048;             // distinct diagonals at most (8 KB of LDS per workgroup)
constexpr int32_t kCodeEmpty = INT32_MIN;  // never a valid offset (|col - row| < 2^31 - 1)
constexpr int kCodePad = 64;               // zeroed codes behind the last entry (lane loads may overrun)

__device__ __forceinline__ unsigned code_hash(int32_t d) { return ((unsigned)d * 2654435761u) >> 20; }   // 12 bits

__global__ __launch_bounds__(kBlock) void code_collect_kernel(const int32_t *rowptr, const int32_t *col, int64_t m,
                                                              int32_t *keys, int *count_fail) {
  const int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (row >= m) return;
  if (__atomic_load_n(&count_fail[1], __ATOMIC_RELAXED)) return;
  int32_t last = kCodeEmpty;
  for (int32_t q = rowptr[row]; q < rowptr[row + 1]; ++q) {
    const int32_t d = col[q] - (int32_t)row;
    if (d == last) continue;
    last = d;
    unsigned slot = code_hash(d) & (kCodeHash - 1);
    bool done = false;
    for (int probe = 0; probe < kCodeHash && !done; ++probe) {
      int32_t cur = __atomic_load_n(&keys[slot], __ATOMIC_RELAXED);
      if (cur == kCodeEmpty) {
        cur = atomicCAS(&keys[slot], kCodeEmpty, d);
        if (cur == kCodeEmpty) {
          if (atomicAdd(&count_fail[0], 1) >= kCodeMax) atomicMax(&count_fail[1], 1);
          cur = d;
        }
      }
      if (cur == d) done = true;
      else slot = (slot + 1) & (kCodeHash - 1);
    }
    if (!done) { atomicMax(&count_fail[1], 1); return; }
  }
}

template <typename CODE>
__global__ __launch_bounds__(kBlock) void code_assign_kernel(const int32_t *rowptr, const int32_t *col, int64_t m,
                                                             const int32_t *tab, int T, CODE *code, int *fail) {
  extern __shared__ int32_t s_tab[];
  for (int i = threadIdx.x; i < T; i += kBlock) s_tab[i] = tab[i];
  __syncthreads();
  const int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (row >= m) return;
  for (int32_t q = rowptr[row]; q < rowptr[row + 1]; ++q) {
    const int32_t d = col[q] - (int32_t)row;
    int lo = 0, hi = T - 1;
    while (lo < hi) {                      // first entry >= d
      const int mid = (lo + hi) >> 1;
      if (s_tab[mid] < d) lo = mid + 1; else hi = mid;
    }
    if (s_tab[lo] != d) { atomicMax(fail, 1); return; }
    code[q] = (CODE)lo;
  }
}

// ---------------------------------------------------------------- sliced form (spmv_sell_kernel) ----
// The coded kernel reads the CSR value / code streams of a row block coalesced, parks them in LDS and lets lane i walk row i out of
// LDS: rowptr -> window loads -> barrier -> LDS reads -> gathers is one dependent chain per workgroup.  Here the SAME entries, in the
// SAME order per row, are stored a second time transposed per 64-row slice, so that lane l reads entry k of its own row with a
// coalesced 8-byte load (512 contiguous bytes per wave instruction): slice s starts at unit off[s] (a unit = 64 words of 8 bytes);
// its first W = ceil(L / 8) units hold, per lane, eight 1-byte codes per word (0xFF = the row has no such entry), the next L units
// the values (L = longest row of the slice).  64 B per row for the 7-point operator (7 values + one code word) where CSR + codes
// + row pointer is 67.  y is bit-identical (stored order, one rounded multiply and one rounded add per entry).
constexpr double kSellMaxPad = 1.20;       // bytes of the sliced copy / bytes of the CSR stream it replaces above which it is not built
constexpr double kSellUniformPad = 1.02;   // padding every slice to the longest one may cost this much (then there is no offset array)

__global__ __launch_bounds__(kBlock) void sell_units_kernel(const int32_t *rowptr, int64_t m, int64_t slices, int32_t *units, int mode) {
  const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (s >= slices) return;
  int L = 0;
  const int64_t r0 = s * 64, r1 = (r0 + 64 < m) ? r0 + 64 : m;
  int32_t prev = rowptr[r0];
  for (int64_t r = r0; r < r1; ++r) {
    const int32_t nxt = rowptr[r + 1];
    L = (nxt - prev > L) ? nxt - prev : L;
    prev = nxt;
  }
  const int Lp = L + (L & 1);                // pair layouts: an even number of value words ...
  const int h4 = (Lp / 2) + ((Lp / 2) & 1), h5 = ((L + 7) / 8) + (((L + 7) / 8) & 1);      // ... behind an even number of column / code words
  units[s] = L > 0 ? (mode == 5 ? Lp + h5 : (mode == 4 ? Lp + h4 : (mode == 3 ? 2 * ((L + 2) / 2) : L + (mode == 2 ? 0 : (mode == 1 ? (L + 1) / 2 : (L + 7) / 8))))) : 0;      // mode 0: 8-bit code words, 1: int32 column words, 2: values only (narrow codes live in their own array), 3: one code word + values, an even number of words (16-byte pairs; L <= 8), 4 / 5: int32 column words / code words padded to an even count, then the values padded to an even count (16-byte pairs, any L)
}

// words per row ahead of the values for T units of a slice: code words (T = L + ceil(L / 8)) or column words (T = L + ceil(L / 2))
__host__ __device__ __forceinline__ int sell_head_words(int T, int mode) {
  if (T <= 0) return 0;
  if (mode == 5) return T <= 18 ? 2 : (T <= 36 ? 4 : (T <= 54 ? 6 : 8));       // T = Lp + even(ceil(Lp / 8)), Lp even <= 64: disjoint ranges
  if (mode == 4) return 2 * ((T - 4) / 6) + 2;                                 // T = Lp + even(Lp / 2)
  return mode == 3 ? 1 : (mode == 2 ? 0 : (mode == 1 ? (T + 2) / 3 : (T + 8) / 9));
}

__global__ __launch_bounds__(kBlock) void sell_fill_kernel(const int32_t *rowptr, const double *val, const uint8_t *code, const int32_t *col, int64_t m,
                                                           int64_t slices, const uint32_t *off, int uniform_units,
                                                           unsigned long long *sell, uint32_t *c4, int mode) {
  const int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x;      // rows of the last slice beyond m are written too (no entry)
  if (row >= slices * 64) return;
  const int64_t s = row >> 6;
  const int lane = (int)(row & 63);
  const int64_t o0 = uniform_units ? s * uniform_units : (int64_t)off[s];
  const int T = uniform_units ? uniform_units : (int)(off[s + 1] - off[s]);
  const int cols32 = col != nullptr;
  const bool pair = mode >= 3;
  const int32_t q0 = row < m ? rowptr[row] : 0;
  const int len = row < m ? rowptr[row + 1] - q0 : 0;
  if (c4) {                                   // eight 4-bit codes, 0xF = no entry
    uint32_t word = 0;
    for (int u = 0; u < 8; ++u) word |= (u < len ? (uint32_t)code[q0 + u] : 0xFu) << (4 * u);
    c4[row] = word;
  }
  if (T == 0) return;
  const int W = sell_head_words(T, mode), L = T - W;
  unsigned long long *base = sell + (size_t)o0 * 64 + lane;
  // word w of this lane: plain layout (w * 64 + lane); pair layout ((w / 2) * 64 + lane) * 2 + (w & 1)
  auto slot = [&](int w) -> unsigned long long & { return pair ? sell[(size_t)o0 * 64 + ((size_t)(w >> 1) * 64 + lane) * 2 + (w & 1)] : base[(size_t)w * 64]; };
  for (int w = 0; w < W; ++w) {
    unsigned long long word = 0;
    if (cols32) {
      const unsigned long long c0 = 2 * w < len ? (unsigned long long)(uint32_t)col[q0 + 2 * w] : 0xFFFFFFFFull;
      const unsigned long long c1 = 2 * w + 1 < len ? (unsigned long long)(uint32_t)col[q0 + 2 * w + 1] : 0xFFFFFFFFull;
      word = c0 | (c1 << 32);
    } else {
      for (int u = 0; u < 8; ++u) {
        const int k = 8 * w + u;
        const unsigned long long c = k < len ? (unsigned long long)code[q0 + k] : 0xFFull;
        word |= c << (8 * u);
      }
    }
    slot(w) = word;
  }
  for (int k = 0; k < L; ++k) slot(W + k) = k < len ? (unsigned long long)__double_as_longlong(val[q0 + k]) : 0ull;
}

// ---------------------------------------------------------------- entry-coded sliced form (spmv_sell_kernel, ENT) ----
// A stencil operator repeats not only its diagonals but its ENTRIES: the pair (column - row, value) takes 7 distinct values on the
// 7-point operator with constant coefficients, 27 on the 27-point one.  A handle with 8-bit diagonal codes, rows of at most 64
// entries and at most 255 distinct pairs -- values compared as 64-bit patterns: +0.0 and -0.0 are two, NaNs with different payloads
// are two -- keeps in its sliced fields code words ONLY: one byte per entry = the rank of its pair in the handle's entry dictionary
// (ascending by offset, then by the value's bits taken as unsigned; 0xFF = no entry), the SAME 64-row slices and the same per-lane
// word order as the code words above, without the values.  A slice whose longest row has L entries holds, per lane, one word
// (L <= 8: 512 B per slice, 8 B per row) or ceil(L / 8) words padded to an even count and stored in 16-byte pairs as in mode 5.  The
// kernel rebuilds col = row + off[code] and val[code] from a 256-slot table in LDS: stored order, the same bits, the same y.
// Construction on the device, verified entry by entry: a CAS set of the value patterns, a presence map over (diagonal code, value id),
// the host sorts / compacts the at most 255 pairs, the fill pass checks every entry it codes against the table and refuses the
// form on any mismatch.
constexpr int kEntMax = 255;               // pairs at most (0xFF = no entry)
constexpr int kEntHash = 1024;             // slots of the value set (power of two)
constexpr unsigned long long kEntEmpty = ~0ull;   // empty slot; a value with this very pattern (a NaN) is flagged apart

__device__ __forceinline__ unsigned ent_hash(unsigned long long b) { return (unsigned)((b * 0x9E3779B97F4A7C15ull) >> 54); }   // 10 bits

// flags: [0] distinct values so far, [1] failure, [2] the all-ones pattern occurs
__global__ __launch_bounds__(kBlock) void ent_values_kernel(const int32_t *rowptr, const double *val, int64_t m, unsigned long long *keys, int *flags) {
  const int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (row >= m) return;
  if (__atomic_load_n(&flags[1], __ATOMIC_RELAXED)) return;
  unsigned long long last = 0;
  bool have = false;
  for (int32_t q = rowptr[row]; q < rowptr[row + 1]; ++q) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(val[q]);
    if (have && b == last) continue;
    last = b; have = true;
    if (b == kEntEmpty) { if (!__atomic_load_n(&flags[2], __ATOMIC_RELAXED)) atomicOr(&flags[2], 1); continue; }
    unsigned slot = ent_hash(b) & (kEntHash - 1);
    bool done = false;
    for (int probe = 0; probe < kEntHash && !done; ++probe) {
      unsigned long long cur = __atomic_load_n(&keys[slot], __ATOMIC_RELAXED);
      if (cur == kEntEmpty) {
        cur = atomicCAS(&keys[slot], kEntEmpty, b);
        if (cur == kEntEmpty) {
          if (atomicAdd(&flags[0], 1) >= kEntMax) atomicMax(&flags[1], 1);
          cur = b;
        }
      }
      if (cur == b) done = true;
      else slot = (slot + 1) & (kEntHash - 1);
    }
    if (!done) { atomicMax(&flags[1], 1); return; }
  }
}

// rank of the pattern b in the ascending table vals[0, V), or -1
__device__ __forceinline__ int ent_value_id(const unsigned long long *vals, int V, unsigned long long b) {
  int lo = 0, hi = V - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (vals[mid] < b) lo = mid + 1; else hi = mid;
  }
  return (V > 0 && vals[lo] == b) ? lo : -1;
}

// presence map over (diagonal code, value id): bit (code * 256 + id) of 65,536
__global__ __launch_bounds__(kBlock) void ent_presence_kernel(const int32_t *rowptr, const double *val, const uint8_t *code, int64_t m,
                                                              const unsigned long long *vals, int V, unsigned *present, int *flags) {
  __shared__ unsigned long long s_vals[256];
  for (int i = threadIdx.x; i < 256; i += kBlock) s_vals[i] = i < V ? vals[i] : kEntEmpty;
  __syncthreads();
  const int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (row >= m) return;
  for (int32_t q = rowptr[row]; q < rowptr[row + 1]; ++q) {
    const int id = ent_value_id(s_vals, V, (unsigned long long)__double_as_longlong(val[q]));
    if (id < 0) { atomicMax(&flags[1], 1); return; }
    const unsigned bit = (unsigned)code[q] * 256u + (unsigned)id;
    if (!((__atomic_load_n(&present[bit >> 5], __ATOMIC_RELAXED) >> (bit & 31)) & 1u)) atomicOr(&present[bit >> 5], 1u << (bit & 31));
  }
}

// units of a slice: one word of eight entry codes up to 8 entries per row, else ceil(L / 8) words padded to an even count (16-byte pairs)
__host__ __device__ __forceinline__ int ent_units(int L) { return L <= 0 ? 0 : (L <= 8 ? 1 : ((L + 7) / 8) + (((L + 7) / 8) & 1)); }

__global__ __launch_bounds__(kBlock) void ent_units_kernel(const int32_t *rowptr, int64_t m, int64_t slices, int32_t *units) {
  const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (s >= slices) return;
  int L = 0;
  const int64_t r0 = s * 64, r1 = (r0 + 64 < m) ? r0 + 64 : m;
  int32_t prev = rowptr[r0];
  for (int64_t r = r0; r < r1; ++r) {
    const int32_t nxt = rowptr[r + 1];
    L = (nxt - prev > L) ? nxt - prev : L;
    prev = nxt;
  }
  units[s] = ent_units(L);
}

// pairmap[code * 256 + id] = rank of the pair (0xFF: absent); tab_off / tab_val = the dictionary (256 slots each).  Every entry is
// checked against the table it is coded with: offset and value bits, exactly.
__global__ __launch_bounds__(kBlock) void ent_fill_kernel(const int32_t *rowptr, const int32_t *col, const double *val, const uint8_t *code, int64_t m,
                                                          int64_t slices, const uint32_t *off, int uniform_units, const unsigned long long *vals, int V,
                                                          const uint8_t *pairmap, const int32_t *tab_off, const double *tab_val,
                                                          unsigned long long *sell, int *flags) {
  __shared__ unsigned long long s_vals[256];
  for (int i = threadIdx.x; i < 256; i += kBlock) s_vals[i] = i < V ? vals[i] : kEntEmpty;
  __syncthreads();
  const int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x;      // rows of the last slice beyond m are written too (no entry)
  if (row >= slices * 64) return;
  const int64_t s = row >> 6;
  const int lane = (int)(row & 63);
  const int64_t o0 = uniform_units ? s * uniform_units : (int64_t)off[s];
  const int T = uniform_units ? uniform_units : (int)(off[s + 1] - off[s]);
  const int32_t q0 = row < m ? rowptr[row] : 0;
  const int len = row < m ? rowptr[row + 1] - q0 : 0;
  if (len > 8 * T) { atomicMax(&flags[1], 1); return; }
  for (int w = 0; w < T; ++w) {
    unsigned long long word = 0;
    for (int u = 0; u < 8; ++u) {
      const int k = 8 * w + u;
      unsigned long long e = 0xFFull;
      if (k < len) {
        const unsigned long long b = (unsigned long long)__double_as_longlong(val[q0 + k]);
        const int id = ent_value_id(s_vals, V, b);
        e = id >= 0 ? (unsigned long long)pairmap[(size_t)code[q0 + k] * 256 + (size_t)id] : 0xFFull;
        if (e == 0xFFull || tab_off[e] != col[q0 + k] - (int32_t)row || (unsigned long long)__double_as_longlong(tab_val[e]) != b) { atomicMax(&flags[1], 1); return; }
      }
      word |= e << (8 * u);
    }
    // word w of this lane: one word per lane (T == 1), else pairs ((w / 2) * 64 + lane) * 2 + (w & 1)
    sell[(size_t)o0 * 64 + (T == 1 ? (size_t)lane : ((size_t)(w >> 1) * 64 + lane) * 2 + (w & 1))] = word;
  }
}

void csr_free_sell(khip_csr *A) {
  (void)hipFree(A->sell); (void)hipFree(A->sell_off); (void)hipFree(A->sell_c4); (void)hipFree(A->sell_ent_tab);
  A->sell = nullptr; A->sell_off = nullptr; A->sell_c4 = nullptr; A->sell_pair = 0; A->sell_ent_tab = nullptr;
  A->sell_units = 0; A->sell_total_units = 0; A->sell_state = 0; A->sell_entries = 0; A->sell_ent_state = 0;
}

void csr_free_sell32(khip_csr *A) {
  (void)hipFree(A->sell32); (void)hipFree(A->sell32_off);
  A->sell32 = nullptr; A->sell32_off = nullptr;
  A->sell32_units = 0; A->sell32_total_units = 0; A->sell32_state = 0; A->sell32_pair = 0;
}

// cols32 = false: code words (needs the 8-bit codes); true: int32 column words
static int build_sell_form(khip_ctx *ctx, khip_csr *A, bool cols32) {
  const bool ent_refused = !cols32 && A->sell_ent_state == -1;       // the entry-coded build was tried on this handle: stays tried
  if (cols32) csr_free_sell32(A); else csr_free_sell(A);
  if (ent_refused) A->sell_ent_state = -1;
  int &state = cols32 ? A->sell32_state : A->sell_state;
  unsigned long long *&words = cols32 ? A->sell32 : A->sell;
  uint32_t *&offs = cols32 ? A->sell32_off : A->sell_off;
  state = -1;
  const int64_t m = A->m;
  if (m == 0 || A->nnz == 0 || A->max_row_nnz > 64) return KHIP_OK;
  if (!cols32 && (A->code_state != 1 || A->code_bits != 8 || A->code_T > 255)) return KHIP_OK;
  const bool narrow = !cols32 && ctx->tune.spmv_sell_narrow && A->code_T <= 15 && A->max_row_nnz <= 8;
  const bool pair = !narrow && ctx->tune.spmv_sell_pair;
  // int32 columns: the pair layout costs 96 instead of 88 B per 7-point row and measured no faster (plain 2.36 against 2.27 ms, fused 2.44
  // against 2.41 at 512^3, profiles/r06aw): only with spmv_sell_pair = 2
  const int mode = cols32 ? ((pair && ctx->tune.spmv_sell_pair >= 2) ? 4 : 1) : (narrow ? 2 : (pair ? (A->max_row_nnz <= 8 ? 3 : 5) : 0));
  const int64_t slices = (m + 63) / 64;
  int32_t *units_d = nullptr;
  KHIP_CHECK_HIP(hipMalloc(&units_d, sizeof(int32_t) * (size_t)slices));
  struct Scratch { int32_t *&p; ~Scratch() { (void)hipFree(p); } } scratch{units_d};
  hipLaunchKernelGGL(sell_units_kernel, dim3((unsigned)((slices + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream, A->rowptr, m, slices, units_d, mode);
  KHIP_CHECK_HIP(hipGetLastError());
  std::vector<int32_t> units((size_t)slices);
  KHIP_CHECK_HIP(hipMemcpyAsync(units.data(), units_d, sizeof(int32_t) * (size_t)slices, hipMemcpyDeviceToHost, ctx->stream));
  KHIP_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  int64_t total = 0, slots = 0;
  int umax = 0;
  for (int32_t u : units) { total += u; const int W = sell_head_words(u, mode); slots += (int64_t)(u - W) * 64; umax = u > umax ? u : umax; }
  (void)slots;
  const double ref_bytes = (cols32 ? 12.0 : 9.0) * (double)A->nnz + 4.0 * (double)m;    // the CSR stream this copy replaces
  if (512.0 * (double)total > kSellMaxPad * ref_bytes + 65536.0) return KHIP_OK;       // too much padding: stays on the CSR stream
  const bool uniform = (double)umax * (double)slices <= kSellUniformPad * (double)total + 8.0;
  if (uniform) total = (int64_t)umax * slices;
  if (total >= ((int64_t)1 << 32)) return KHIP_OK;
  bool keep = false;
  struct Guard { khip_csr *A; bool cols32; int &state; bool &keep;
                 ~Guard() { if (!keep) { if (cols32) csr_free_sell32(A); else csr_free_sell(A); state = -1; } } } guard{A, cols32, state, keep};
  if (!uniform) {
    std::vector<uint32_t> off((size_t)slices + 1);
    uint32_t run = 0;
    for (int64_t s = 0; s < slices; ++s) { off[(size_t)s] = run; run += (uint32_t)units[(size_t)s]; }
    off[(size_t)slices] = run;
    KHIP_CHECK_HIP(hipMalloc(&offs, sizeof(uint32_t) * ((size_t)slices + 1)));
    KHIP_CHECK_HIP(hipMemcpyAsync(offs, off.data(), sizeof(uint32_t) * ((size_t)slices + 1), hipMemcpyHostToDevice, ctx->stream));
    KHIP_CHECK_HIP(hipStreamSynchronize(ctx->stream));                                  // `off` dies with this scope
  }
  KHIP_CHECK_HIP(hipMalloc(&words, sizeof(unsigned long long) * 64 * (size_t)(total + 1)));
  if (narrow) KHIP_CHECK_HIP(hipMalloc(&A->sell_c4, sizeof(uint32_t) * 64 * (size_t)slices));
  hipLaunchKernelGGL(sell_fill_kernel, dim3((unsigned)((slices * 64 + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream, A->rowptr, A->val,
                     (const uint8_t *)A->code, cols32 ? A->col : (const int32_t *)nullptr, m, slices, offs, uniform ? umax : 0, words, narrow ? A->sell_c4 : (uint32_t *)nullptr, mode);
  KHIP_CHECK_HIP(hipGetLastError());
  KHIP_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  keep = true;
  (cols32 ? A->sell32_units : A->sell_units) = uniform ? umax : 0;
  (cols32 ? A->sell32_total_units : A->sell_total_units) = total;
  if (cols32) A->sell32_pair = mode == 4 ? 2 : 0; else A->sell_pair = mode == 3 ? 1 : (mode == 5 ? 2 : 0);
  state = 1;
  return KHIP_OK;
}

// The entry-coded copy in the handle's sliced fields.  Success: sell_state = sell_ent_state = 1.  Refusal (more than 255 pairs, a row
// of more than 64 entries, too much padding, a mismatch found by the fill pass): sell_ent_state = -1 and sell_state stays 0 -- the
// caller builds the copy with values.
int csr_build_sell_entries(khip_ctx *ctx, khip_csr *A) {
  csr_free_sell(A);
  A->sell_ent_state = -1;
  const int64_t m = A->m;
  if (m == 0 || A->nnz == 0 || A->max_row_nnz > 64) return KHIP_OK;
  if (A->code_state != 1 || A->code_bits != 8 || A->code_T > 255) return KHIP_OK;
  const int64_t slices = (m + 63) / 64;
  struct Dev { void *p = nullptr; ~Dev() { (void)hipFree(p); } };
  Dev keys_d, flags_d, vals_d, present_d, map_d, units_d;
  KHIP_CHECK_HIP(hipMalloc(&keys_d.p, sizeof(unsigned long long) * kEntHash));
  KHIP_CHECK_HIP(hipMalloc(&flags_d.p, sizeof(int) * 4));
  KHIP_CHECK_HIP(hipMemsetAsync(keys_d.p, 0xFF, sizeof(unsigned long long) * kEntHash, ctx->stream));
  KHIP_CHECK_HIP(hipMemsetAsync(flags_d.p, 0, sizeof(int) * 4, ctx->stream));
  int *flags = (int *)flags_d.p;
  const unsigned grid = (unsigned)((m + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(ent_values_kernel, dim3(grid), dim3(kBlock), 0, ctx->stream, A->rowptr, A->val, m, (unsigned long long *)keys_d.p, flags);
  KHIP_CHECK_HIP(hipGetLastError());
  int h[4] = {0, 0, 0, 0};
  std::vector<unsigned long long> hk(kEntHash);
  KHIP_CHECK_HIP(hipMemcpyAsync(h, flags, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
  KHIP_CHECK_HIP(hipMemcpyAsync(hk.data(), keys_d.p, sizeof(unsigned long long) * kEntHash, hipMemcpyDeviceToHost, ctx->stream));
  KHIP_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  if (h[1]) return KHIP_OK;                                           // more than 255 values: more than 255 pairs
  std::vector<unsigned long long> vals;
  for (unsigned long long k : hk) if (k != kEntEmpty) vals.push_back(k);
  if (h[2]) vals.push_back(kEntEmpty);
  std::sort(vals.begin(), vals.end());
  const int V = (int)vals.size();
  if (V == 0 || V > kEntMax) return KHIP_OK;
  KHIP_CHECK_HIP(hipMalloc(&vals_d.p, sizeof(unsigned long long) * 256));
  KHIP_CHECK_HIP(hipMalloc(&present_d.p, 65536 / 8));
  KHIP_CHECK_HIP(hipMemcpyAsync(vals_d.p, vals.data(), sizeof(unsigned long long) * (size_t)V, hipMemcpyHostToDevice, ctx->stream));
  KHIP_CHECK_HIP(hipMemsetAsync(present_d.p, 0, 65536 / 8, ctx->stream));
  hipLaunchKernelGGL(ent_presence_kernel, dim3(grid), dim3(kBlock), 0, ctx->stream, A->rowptr, A->val, (const uint8_t *)A->code, m,
                     (const unsigned long long *)vals_d.p, V, (unsigned *)present_d.p, flags);
  KHIP_CHECK_HIP(hipGetLastError());
  std::vector<unsigned> present(65536 / 32);
  std::vector<int32_t> diag((size_t)A->code_T);
  KHIP_CHECK_HIP(hipMemcpyAsync(h, flags, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
  KHIP_CHECK_HIP(hipMemcpyAsync(present.data(), present_d.p, 65536 / 8, hipMemcpyDeviceToHost, ctx->stream));
  KHIP_CHECK_HIP(hipMemcpyAsync(diag.data(), A->code_tab, sizeof(int32_t) * (size_t)A->code_T, hipMemcpyDeviceToHost, ctx->stream));
  KHIP_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  if (h[1]) return KHIP_OK;
  // the dictionary: diagonal codes ascend with the offset, value ids with the bits, so walking the map in order IS the sorted order
  struct Table { int32_t off[256]; double val[256]; } tab;
  memset(&tab, 0, sizeof(tab));
  std::vector<uint8_t> pairmap(65536, 0xFF);
  int P = 0;
  for (int c = 0; c < A->code_T; ++c)
    for (int id = 0; id < V; ++id) {
      const unsigned bit = (unsigned)c * 256u + (unsigned)id;
      if (!((present[bit >> 5] >> (bit & 31)) & 1u)) continue;
      if (P >= kEntMax) return KHIP_OK;                               // 256 pairs or more: refused
      tab.off[P] = diag[(size_t)c];
      memcpy(&tab.val[P], &vals[(size_t)id], sizeof(double));
      pairmap[bit] = (uint8_t)P++;
    }
  if (P == 0) return KHIP_OK;
  // slices: the rules of build_sell_form with this form's units
  KHIP_CHECK_HIP(hipMalloc(&units_d.p, sizeof(int32_t) * (size_t)slices));
  hipLaunchKernelGGL(ent_units_kernel, dim3((unsigned)((slices + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream, A->rowptr, m, slices, (int32_t *)units_d.p);
  KHIP_CHECK_HIP(hipGetLastError());
  std::vector<int32_t> units((size_t)slices);
  KHIP_CHECK_HIP(hipMemcpyAsync(units.data(), units_d.p, sizeof(int32_t) * (size_t)slices, hipMemcpyDeviceToHost, ctx->stream));
  KHIP_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  int64_t total = 0;
  int umax = 0;
  for (int32_t u : units) { total += u; umax = u > umax ? u : umax; }
  const double ref_bytes = 9.0 * (double)A->nnz + 4.0 * (double)m;    // the CSR stream this copy replaces (the one build_sell_form compares with)
  if (512.0 * (double)total > kSellMaxPad * ref_bytes + 65536.0) return KHIP_OK;
  const bool uniform = (double)umax * (double)slices <= kSellUniformPad * (double)total + 8.0;
  if (uniform) total = (int64_t)umax * slices;
  if (total >= ((int64_t)1 << 32)) return KHIP_OK;
  bool keep = false;
  struct Guard { khip_csr *A; bool &keep; ~Guard() { if (!keep) { csr_free_sell(A); A->sell_ent_state = -1; } } } guard{A, keep};
  if (!uniform) {
    std::vector<uint32_t> off((size_t)slices + 1);
    uint32_t run = 0;
    for (int64_t s = 0; s < slices; ++s) { off[(size_t)s] = run; run += (uint32_t)units[(size_t)s]; }
    off[(size_t)slices] = run;
    KHIP_CHECK_HIP(hipMalloc(&A->sell_off, sizeof(uint32_t) * ((size_t)slices + 1)));
    KHIP_CHECK_HIP(hipMemcpyAsync(A->sell_off, off.data(), sizeof(uint32_t) * ((size_t)slices + 1), hipMemcpyHostToDevice, ctx->stream));
    KHIP_CHECK_HIP(hipStreamSynchronize(ctx->stream));                                  // `off` dies with this scope
  }
  KHIP_CHECK_HIP(hipMalloc(&A->sell, sizeof(unsigned long long) * 64 * (size_t)(total + 1)));
  KHIP_CHECK_HIP(hipMalloc(&A->sell_ent_tab, sizeof(tab)));
  KHIP_CHECK_HIP(hipMalloc(&map_d.p, 65536));
  KHIP_CHECK_HIP(hipMemcpyAsync(A->sell_ent_tab, &tab, sizeof(tab), hipMemcpyHostToDevice, ctx->stream));
  KHIP_CHECK_HIP(hipMemcpyAsync(map_d.p, pairmap.data(), 65536, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(ent_fill_kernel, dim3((unsigned)((slices * 64 + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream, A->rowptr, A->col, A->val,
                     (const uint8_t *)A->code, m, slices, A->sell_off, uniform ? umax : 0, (const unsigned long long *)vals_d.p, V,
                     (const uint8_t *)map_d.p, (const int32_t *)A->sell_ent_tab, (const double *)((const int32_t *)A->sell_ent_tab + 256),
                     A->sell, flags);
  KHIP_CHECK_HIP(hipGetLastError());
  KHIP_CHECK_HIP(hipMemcpyAsync(h, flags, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
  KHIP_CHECK_HIP(hipStreamSynchronize(ctx->stream));                  // also keeps `tab` / `pairmap` alive until the uploads are done
  if (h[1]) return KHIP_OK;                                           // an entry did not match the table it was coded with
  keep = true;
  A->sell_units = uniform ? umax : 0;
  A->sell_total_units = total;
  A->sell_pair = 0;
  A->sell_entries = P;
  A->sell_ent_state = 1;
  A->sell_state = 1;
  return KHIP_OK;
}

int csr_build_sell(khip_ctx *ctx, khip_csr *A) { return build_sell_form(ctx, A, false); }
int csr_build_sell32(khip_ctx *ctx, khip_csr *A) { return build_sell_form(ctx, A, true); }

void csr_free_codes(khip_csr *A) {
  csr_free_sell(A);                          // the sliced form carries the codes
  csr_free_sell32(A);                        // ... and its int32 twin the columns (called wherever the columns change, and by destroy)
  (void)hipFree(A->code); (void)hipFree(A->code_tab);
  A->code = nullptr; A->code_tab = nullptr;
  A->code_T = 0; A->code_bits = 0; A->code_state = 0;
}

int csr_build_codes(khip_ctx *ctx, khip_csr *A) {
  csr_free_codes(A);
  A->code_state = -1;
  const int64_t m = A->m;
  if (m == 0 || A->nnz == 0) return KHIP_OK;
  int32_t *keys = nullptr;
  int *cf = nullptr;
  KHIP_CHECK_HIP(hipMalloc(&keys, sizeof(int32_t) * kCodeHash));
  KHIP_CHECK_HIP(hipMalloc(&cf, sizeof(int) * 2));
  bool keep = false;
  struct Scratch {
    int32_t *&keys; int *&cf; khip_csr *A; bool &keep;
    ~Scratch() {
      (void)hipFree(keys); (void)hipFree(cf);
      if (!keep) { csr_free_codes(A); A->code_state = -1; }
    }
  } scratch{keys, cf, A, keep};
  std::vector<int32_t> init(kCodeHash, kCodeEmpty);
  KHIP_CHECK_HIP(hipMemcpyAsync(keys, init.data(), sizeof(int32_t) * kCodeHash, hipMemcpyHostToDevice, ctx->stream));
  KHIP_CHECK_HIP(hipMemsetAsync(cf, 0, sizeof(int) * 2, ctx->stream));
  const unsigned grid = (unsigned)((m + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(code_collect_kernel, dim3(grid), dim3(kBlock), 0, ctx->stream, A->rowptr, A->col, m, keys, cf);
  KHIP_CHECK_HIP(hipGetLastError());
  int h[2] = {0, 0};
  std::vector<int32_t> hk(kCodeHash);
  KHIP_CHECK_HIP(hipMemcpyAsync(h, cf, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
  KHIP_CHECK_HIP(hipMemcpyAsync(hk.data(), keys, sizeof(int32_t) * kCodeHash, hipMemcpyDeviceToHost, ctx->stream));
  KHIP_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  if (h[1] || h[0] > kCodeMax) return KHIP_OK;                       // too many diagonals: stays on the int32 stream
  std::vector<int32_t> tab;
  for (int32_t k : hk) if (k != kCodeEmpty) tab.push_back(k);
  std::sort(tab.begin(), tab.end());
  const int T = (int)tab.size();
  if (T == 0 || T > kCodeMax) return KHIP_OK;
  const int bits = (T <= 256 && ctx->tune.spmv_codes != 16) ? 8 : 16;
  KHIP_CHECK_HIP(hipMalloc(&A->code_tab, sizeof(int32_t) * (size_t)T));
  KHIP_CHECK_HIP(hipMemcpyAsync(A->code_tab, tab.data(), sizeof(int32_t) * (size_t)T, hipMemcpyHostToDevice, ctx->stream));
  const size_t bytes = (size_t)(A->nnz + kCodePad) * (size_t)(bits / 8);
  KHIP_CHECK_HIP(hipMalloc(&A->code, bytes));
  KHIP_CHECK_HIP(hipMemsetAsync((char *)A->code + (size_t)A->nnz * (size_t)(bits / 8), 0, (size_t)kCodePad * (size_t)(bits / 8),
                                ctx->stream));
  KHIP_CHECK_HIP(hipMemsetAsync(cf, 0, sizeof(int) * 2, ctx->stream));
  if (bits == 8)
    hipLaunchKernelGGL(code_assign_kernel<uint8_t>, dim3(grid), dim3(kBlock), sizeof(int32_t) * (size_t)T, ctx->stream, A->rowptr,
                       A->col, m, A->code_tab, T, (uint8_t *)A->code, cf + 1);
  else
    hipLaunchKernelGGL(code_assign_kernel<uint16_t>, dim3(grid), dim3(kBlock), sizeof(int32_t) * (size_t)T, ctx->stream,
                       A->rowptr, A->col, m, A->code_tab, T, (uint16_t *)A->code, cf + 1);
  KHIP_CHECK_HIP(hipGetLastError());
  KHIP_CHECK_HIP(hipMemcpyAsync(h, cf, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
  KHIP_CHECK_HIP(hipStreamSynchronize(ctx->stream));      // also keeps `tab` alive until the upload is done
  if (h[1]) return KHIP_OK;
  keep = true;
  A->code_T = T;
  A->code_bits = bits;
  A->code_state = 1;
  return KHIP_OK;
}

}  // namespace khip
