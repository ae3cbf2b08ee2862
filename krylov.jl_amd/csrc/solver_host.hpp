// solver_host.hpp -- host-side pieces every solver shares: the workspace core (stats box, caller-owned vectors,
// allocation timer, option defaults) and the driver of the device-resident loops ("fused = 2", solver_device.hpp).
#pragma once

#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <limits>
#include <vector>

#include "khip_internal.hpp"
#include "solver_device.hpp"

namespace khip {
namespace {   // each solver file gets its own copy, as before: nothing here is exported from the library

constexpr double kEps = std::numeric_limits<double>::epsilon();

double tol_or_default(double t) { return std::isnan(t) ? std::sqrt(kEps) : t; }
double timemax_of(const khip_options &o) {
  return (std::isnan(o.timemax) || o.timemax <= 0) ? std::numeric_limits<double>::infinity() : o.timemax;
}
int64_t padded(int64_t n) { return (n + 31) & ~(int64_t)31; }   // 256-byte multiples keep every slice 16-B aligned

// ---- options.verbose: the reference's per-iteration log (kdisplay, src/krylov_utils.jl:301) on stdout.  Column headers are
// padded by hand: the labels are UTF-8 and printf pads bytes, Julia pads characters.
bool kdisplay(int64_t iter, int verbose) { return verbose > 0 && iter % verbose == 0; }

// workspace.stats and the residual history behind it
struct StatsBox {
  khip_stats st;
  std::vector<double> residuals;
  int path = -1;       // which loop the last solve ran (khip_*_last_path): 2 device-resident / look-ahead, 1 host-driven fused, 0 primitive sequence
  StatsBox() {
    memset(&st, 0, sizeof(st));
    snprintf(st.status, sizeof(st.status), "unknown");
  }
  void reset() {   // reset!(stats), src/krylov_stats.jl:38-44
    residuals.clear();
    st.residuals = nullptr;
    st.nres = 0;
    st.indefinite = 0;
    st.npcCount = 0;
    st.error[0] = 0;
  }
  void push(double v) { residuals.push_back(v); }
  void publish() {
    st.residuals = residuals.empty() ? nullptr : residuals.data();
    st.nres = (int)residuals.size();
  }
  int fail(int code, const char *msg) {
    snprintf(st.error, sizeof(st.error), "%s", msg);
    set_error("%s", msg);
    publish();
    return code;
  }
  int fail_rc(int rc) {   // a primitive failed: message already in khip_last_error()
    snprintf(st.error, sizeof(st.error), "%s", khip_last_error());
    publish();
    return rc;
  }
};

// a failed primitive ends the solve with its message in ws->box
#define K(expr)                                    \
  do {                                             \
    int rc_k = (expr);                             \
    if (rc_k != KHIP_OK) return ws->box.fail_rc(rc_k); \
  } while (0)

// stats.allocation_timer (src/krylov_utils.jl:281-288, allocate_if): every vector allocation of a workspace -- at its
// creation and the lazy ones inside later solves -- adds its wall time to this accumulator; the creation / solve entry
// points move it into the workspace's stats (take_alloc_seconds).
thread_local double g_alloc_seconds = 0.0;
int alloc_vec(khip_ctx *ctx, int64_t n, double **out) {
  const double t = now_s();
  const int rc = khip_malloc(ctx, sizeof(double) * (size_t)padded(n > 0 ? n : 1), reinterpret_cast<void **>(out));
  g_alloc_seconds += now_s() - t;
  return rc;
}
double take_alloc_seconds() { const double v = g_alloc_seconds; g_alloc_seconds = 0.0; return v; }

// Caller-owned work vectors (khip_*_workspace_adopt, khip_*_workspace_adopt_vector): the workspace of the reference owns
// its vectors on the Julia side (src/krylov_workspaces.jl:236-291), so a binding hands their device pointers over and the
// library must neither free nor replace them.  One list per workspace; everything not in it was allocated here.
struct Borrowed {
  std::vector<const double *> v;
  bool has(const double *p) const {
    for (const double *q : v) if (q == p) return true;
    return false;
  }
  void add(const double *p) { if (p && !has(p)) v.push_back(p); }
  void drop(const double *p) {
    for (size_t i = 0; i < v.size(); ++i) if (v[i] == p) { v.erase(v.begin() + (long)i); return; }
  }
};
void free_unless_borrowed(khip_ctx *ctx, const Borrowed &b, double *p) {
  if (p && !b.has(p)) khip_free(ctx, p);
}

// One named vector of a workspace for khip_*_workspace_adopt_vector / adopt_panel.  Required slots cannot be emptied; fixed
// slots are only checked against (their vectors come with khip_*_workspace_adopt).
struct NamedSlot {
  enum Use { Optional, Required, Fixed };
  const char *k;
  double **slot;
  Use use;
};
struct NamedSlots {   // a braced list at the call, or the array ws_adopt_vector fills from a workspace's vector table
  const NamedSlot *b, *e;
  NamedSlots(std::initializer_list<NamedSlot> l) : b(l.begin()), e(l.end()) {}
  NamedSlots(const NamedSlot *tab, size_t n) : b(tab), e(tab + n) {}
  const NamedSlot *begin() const { return b; }
  const NamedSlot *end() const { return e; }
};
// name's slot <- ptr as a caller-owned vector (ptr == nullptr empties the slot); what the library had allocated there is
// freed.  `Borrowed` is a set of pointers, so a pointer may sit in ONE slot only: a pointer that already is
// another vector of the workspace (or of `basis`, named "V") is refused; handing a slot the pointer it already holds changes
// nothing, in particular not who owns it.  fn / what: the entry point and "vector" / "panel", for the messages.
int adopt_named(khip_ctx *ctx, Borrowed &b, NamedSlots tab, const char *fn, const char *what,
                const char *name, double *ptr, const std::vector<double *> *basis = nullptr) {
  std::string names, required;
  for (const NamedSlot &e : tab) {
    if (e.use == NamedSlot::Fixed) continue;
    names += (names.empty() ? "" : ", ") + std::string(e.k);
    if (e.use == NamedSlot::Required) required += (required.empty() ? "" : ", ") + std::string(e.k);
  }
  for (const NamedSlot &e : tab) {
    if (e.use == NamedSlot::Fixed || strcmp(e.k, name) != 0) continue;
    KHIP_REQUIRE(ptr || e.use != NamedSlot::Required, "%s: %s cannot be emptied", fn, required.c_str());
    const char *other = nullptr;
    for (const NamedSlot &o : tab) if (ptr && o.slot != e.slot && *o.slot == ptr) other = o.k;
    if (ptr && basis) for (const double *v : *basis) if (v == ptr) other = "V";
    KHIP_REQUIRE(!other, "%s: the pointer for '%s' already is the workspace's '%s' (every %s needs its own storage)", fn, name,
                 other, what);
    if (*e.slot == ptr) return KHIP_OK;
    if (*e.slot) { if (b.has(*e.slot)) b.drop(*e.slot); else khip_free(ctx, *e.slot); }
    *e.slot = ptr;
    b.add(ptr);
    return KHIP_OK;
  }
  set_error("%s: unknown %s '%s' (%s)", fn, what, name, names.c_str());
  return KHIP_ERR_INVALID;
}

// ---- one vector table per workspace type: the only place a workspace lists its vectors and says how long each one is -----------
// Core vectors are allocated by khip_*_workspace_create, handed over in the table's order by khip_*_workspace_adopt and fixed
// for khip_*_workspace_adopt_vector; they come first.  Lazy vectors stay empty until a solve, a warm start or adopt_vector
// fills them.  A vector has n entries unless its entry says RowSide (m entries: the solvers on an m x n operator).  A workspace W
// has ctx, m, n, borrowed and box beside its vectors; `fn` is the entry point, for the messages.
enum WsVecKind { Core, Lazy };
enum WsVecSide { ColSide, RowSide };   // n entries (what an entry without a fourth member means) / m entries
template <class W>
struct WsVec {
  const char *k;
  double *W::*slot;
  WsVecKind kind;
  WsVecSide side;
};
template <class W> int64_t ws_len(const W *ws, const WsVec<W> &e) { return e.side == RowSide ? ws->m : ws->n; }
template <class W, size_t N> const WsVec<W> *ws_entry(const WsVec<W> (&tab)[N], double *W::*slot) {
  for (const WsVec<W> &e : tab) if (e.slot == slot) return &e;
  return nullptr;
}
template <class W, size_t N> std::string ws_core_names(const WsVec<W> (&tab)[N]) {
  std::string names;
  for (const WsVec<W> &e : tab) if (e.kind == Core) names += (names.empty() ? "" : ", ") + std::string(e.k);
  return names;
}
// stops at the first allocation that fails; what was allocated before it stays in its slot for khip_*_workspace_destroy
template <class W, size_t N> int ws_create_core(W *ws, const WsVec<W> (&tab)[N]) {
  (void)take_alloc_seconds();
  int rc = KHIP_OK;
  for (const WsVec<W> &e : tab) if (e.kind == Core && rc == KHIP_OK) rc = alloc_vec(ws->ctx, ws_len(ws, e), &(ws->*e.slot));
  ws->box.st.allocation_timer = take_alloc_seconds();
  return rc;
}
template <class W, size_t N>
int ws_adopt_core(W *ws, const WsVec<W> (&tab)[N], const char *fn, std::initializer_list<double *> ptrs) {
  const std::string names = ws_core_names(tab);
  bool all = true;
  for (const double *p : ptrs) all = all && p;
  // the message says "n entries" for every table (its wording since the square solvers); a RowSide vector has m
  KHIP_REQUIRE(ws->n == 0 || all, "%s: %s must be device vectors of n entries", fn, names.c_str());
  for (const double *const *i = ptrs.begin(); i != ptrs.end(); ++i)
    for (const double *const *j = i + 1; j != ptrs.end(); ++j)
      KHIP_REQUIRE(ws->n == 0 || *i != *j, "%s: %s must be distinct", fn, names.c_str());
  double *const *next = ptrs.begin();
  for (const WsVec<W> &e : tab) {
    if (e.kind != Core) continue;
    KHIP_REQUIRE(next != ptrs.end(), "%s: fewer pointers than core vectors", fn);
    ws->*e.slot = *next;
    ws->borrowed.add(*next++);
  }
  return KHIP_OK;
}
// khip_*_workspace_create / _adopt of the solvers on an m x n operator: a fresh workspace with its core vectors allocated
// here / taken from the caller in the table's order.  `destroy` is the solver's khip_*_workspace_destroy.
template <class W, size_t N>
int ws_create(khip_ctx *ctx, int64_t m, int64_t n, const WsVec<W> (&tab)[N], const char *fn, int (*destroy)(W *), W **out) {
  KHIP_REQUIRE(ctx && out && m >= 0 && n >= 0, "%s: bad argument", fn);
  W *ws = new W();
  ws->ctx = ctx; ws->m = m; ws->n = n;
  const int rc = ws_create_core(ws, tab);
  if (rc) { (void)destroy(ws); return rc; }
  *out = ws;
  return KHIP_OK;
}
template <class W, size_t N>
int ws_adopt(khip_ctx *ctx, int64_t m, int64_t n, const WsVec<W> (&tab)[N], const char *fn, std::initializer_list<double *> ptrs,
             W **out) {
  KHIP_REQUIRE(ctx && out && m >= 0 && n >= 0, "%s: bad argument", fn);
  W *ws = new W();
  ws->ctx = ctx; ws->m = m; ws->n = n;
  const int rc = ws_adopt_core(ws, tab, fn, ptrs);
  if (rc) { delete ws; return rc; }
  *out = ws;
  return KHIP_OK;
}
template <class W, size_t N>
int ws_adopt_vector(W *ws, const WsVec<W> (&tab)[N], const char *fn, const char *name, double *ptr) {
  KHIP_REQUIRE(ws && name, "%s: null argument", fn);
  NamedSlot slots[N];
  for (size_t i = 0; i < N; ++i)
    slots[i] = NamedSlot{tab[i].k, &(ws->*tab[i].slot), tab[i].kind == Core ? NamedSlot::Fixed : NamedSlot::Optional};
  return adopt_named(ws->ctx, ws->borrowed, NamedSlots(slots, N), fn, "vector", name, ptr);
}
template <class W, size_t N> void ws_free_vectors(W *ws, const WsVec<W> (&tab)[N]) {
  for (const WsVec<W> &e : tab) free_unless_borrowed(ws->ctx, ws->borrowed, ws->*e.slot);
}
template <class W, size_t N> double *ws_vector(W *ws, const WsVec<W> (&tab)[N], const char *name) {
  if (!ws || !name) return nullptr;
  for (const WsVec<W> &e : tab) if (strcmp(e.k, name) == 0) return ws->*e.slot;
  return nullptr;
}
template <class W, size_t N> size_t ws_bytes(W *ws, const WsVec<W> (&tab)[N]) {
  if (!ws) return 0;
  size_t cnt = 0;
  for (const WsVec<W> &e : tab) if (ws->*e.slot) cnt += (size_t)ws_len(ws, e);
  return cnt * sizeof(double);
}
// khip_*_warm_start of the workspaces with one Δx: x0 == ws->dx only sets the flag
template <class W, size_t N> int ws_warm_start(W *ws, const WsVec<W> (&tab)[N], const double *x0, const char *fn) {
  KHIP_REQUIRE(ws && x0, "%s: null argument", fn);
  const int64_t len = ws_len(ws, *ws_entry(tab, &W::dx));
  if (!ws->dx) KHIP_TRY(alloc_vec(ws->ctx, len, &ws->dx));
  if (x0 != ws->dx) KHIP_TRY(khip_copy(ws->ctx, len, ws->dx, x0));
  ws->warm_start = true;
  return KHIP_OK;
}
// khip_*_warm_start of the workspaces with Δx and Δy, each at its own length: x0 == ws->dx / y0 == ws->dy only sets the flag
template <class W, size_t N> int ws_warm_start2(W *ws, const WsVec<W> (&tab)[N], const double *x0, const double *y0, const char *fn) {
  KHIP_REQUIRE(ws && x0 && y0, "%s: x0 and y0 are both required", fn);
  const int64_t nx = ws_len(ws, *ws_entry(tab, &W::dx)), ny = ws_len(ws, *ws_entry(tab, &W::dy));
  if (!ws->dx) KHIP_TRY(alloc_vec(ws->ctx, nx, &ws->dx));
  if (!ws->dy) KHIP_TRY(alloc_vec(ws->ctx, ny, &ws->dy));
  if (x0 != ws->dx) KHIP_TRY(khip_copy(ws->ctx, nx, ws->dx, x0));
  if (y0 != ws->dy) KHIP_TRY(khip_copy(ws->ctx, ny, ws->dy, y0));
  ws->warm_start = true;
  return KHIP_OK;
}

// y = op x inside a sequence whose reductions carry epilogues: the product keeps the sequence number (it is skipped once the
// loop has stopped) and runs no epilogue of its own
int apply_op_no_epilogue(khip_ctx *ctx, const khip_operator *op, const double *x, double *y) {
  const SeqCtl keep = ctx->ctl;
  ctx->ctl.epi = EPI_NONE;
  ctx->ctl.epi_state = nullptr;
  const int rc = apply_op(ctx, op, x, y);
  ctx->ctl = keep;
  return rc;
}

// ---- the device-resident loops ---------------------------------------------------------------------------------------------
constexpr int kDevChunk = 4;             // iterations enqueued between two snapshots of the device state

// the device history windows a state writes (null: no history); minres! keeps three streams, one window each
template <class S> void set_history(S &s, double *w) { s.hist = w; }
void set_history(MinresDevState &s, double *w) {
  s.hist_r = w;
  s.hist_ar = w ? w + kHistWindowMax : nullptr;
  s.hist_acond = w ? w + 2 * kHistWindowMax : nullptr;
}
void set_history(MinresQlpDevState &s, double *w) {
  s.hist_r = w;
  s.hist_ar = w ? w + kHistWindowMax : nullptr;
  s.hist_acond = w ? w + 2 * kHistWindowMax : nullptr;
}
void set_history(SymmlqDevState &s, double *w) {
  s.hist = w;
  s.hist_cg = w ? w + kHistWindowMax : nullptr;
}
void set_history(UsymqrDevState &s, double *w) {
  s.hist_r = w;
  s.hist_ar = w ? w + kHistWindowMax : nullptr;
}
void set_history(UsymlqDevState &s, double *w) { s.hist_r = w; }
void set_history(BilqrDevState &s, double *w) {
  s.hist_p = w;
  s.hist_d = w ? w + kHistWindowMax : nullptr;
}
void set_history(TrilqrDevState &s, double *w) {
  s.hist_p = w;
  s.hist_d = w ? w + kHistWindowMax : nullptr;
}
void set_history(UsymlqrDevState &s, double *w) {
  s.hist_ls = w;
  s.hist_ln = w ? w + kHistWindowMax : nullptr;
  s.hist_ar = w ? w + 2 * kHistWindowMax : nullptr;
}

// entries of column c of a history row (cg_lanczos_shift!: each shift's history is a prefix) or of stream c (bilqr!, trilqr!: each side's
// history ends with the iteration that solved it) that belong to a state's history
template <class S> long long hist_rows(const S &, int) { return std::numeric_limits<long long>::max(); }
long long hist_rows(const LanczosShiftDevState &s, int c) { return s.nhist[c]; }
long long hist_rows(const BilqrDevState &s, int c) { return c == 0 ? s.nhist_p : s.nhist_d; }
long long hist_rows(const TrilqrDevState &s, int c) { return c == 0 ? s.nhist_p : s.nhist_d; }
long long hist_rows(const UsymlqrDevState &s, int c) { return c == 1 ? s.nhist_ln : s.nhist_ls; }   // ‖Aᴴrₖ₋₁‖ (2) ends with ‖rₖ‖_LS (0)

struct DeviceLoopArgs {
  int64_t itmax;
  double t0, timemax;
  bool history;
  std::vector<double> *drain_to[3];      // history stream h -> its host vector (unused streams: null)
  int first_chunk = kDevChunk;           // iterations of the first chunk
  int width = 1;                         // columns != null: ONE stream of rows of `width` entries per iteration,
  std::vector<double> *columns = nullptr; // column c -> columns[c], drained up to hist_rows(state, c)
};

// The driver of a loop whose scalar state S lives on the device (solver_device.hpp) and stops itself: iterations are
// enqueued kDevChunk at a time, each kernel carrying its sequence number; after each chunk the state is snapshot into one of
// two pinned slots and the host waits only for the PREVIOUS chunk's snapshot, so the queue never runs dry.  The history lives
// in device windows of hist_window entries per stream, emptied into the caller's vectors when full and at the end.  What
// the device state, pinned slots and events hold is allocated on first use and kept with the workspace.
template <class S, int kPinned = 2>     // kPinned = 3: pinned[2] stages the uploads of a host-driven loop (minres!)
struct DeviceLoop {
  S *dev = nullptr;
  S *pinned = nullptr;
  double *hist = nullptr;                // history windows, kHistWindowMax entries per stream (allocated with history only)
  std::vector<double> *third_stream = nullptr;   // a third history stream of a solver whose driver names two (usymlqr! on Ssy<P>)
  hipEvent_t snap_ev[2] = {nullptr, nullptr};

  void release() {                       // khip_*_workspace_destroy
    if (dev) (void)hipFree(dev);
    if (pinned) (void)hipHostFree(pinned);
    if (hist) (void)hipFree(hist);
    for (auto e : snap_ev) if (e) (void)hipEventDestroy(e);
  }

  int alloc() {
    if (!dev) KHIP_CHECK_HIP(hipMalloc(&dev, sizeof(S)));
    if (!pinned) KHIP_CHECK_HIP(hipHostMalloc(reinterpret_cast<void **>(&pinned), kPinned * sizeof(S), hipHostMallocDefault));
    for (auto &e : snap_ev) if (!e) KHIP_CHECK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return KHIP_OK;
  }

  // the host-driven loop on the same kernels: its state of the moment, staged in pinned[2], becomes the device copy
  int upload(khip_ctx *ctx, const S &s) {
    static_assert(kPinned == 3, "DeviceLoop::upload stages in pinned[2]");
    pinned[2] = s;
    KHIP_CHECK_HIP(hipMemcpyAsync(dev, &pinned[2], sizeof(S), hipMemcpyHostToDevice, ctx->stream));
    return KHIP_OK;
  }

  // Runs the loop from the initial state h until the device state stops it, itmax iterations are enqueued or the time limit
  // (*overtimed) is reached.  step(dev, j) enqueues iteration j (0-based); before_snapshot() runs after the last step of each
  // chunk.  On return the final state is in *out and its history in the caller's vectors.
  template <class Step, class Hook>
  int run(khip_ctx *ctx, S h, const DeviceLoopArgs &args, Step &&step, Hook &&before_snapshot, S *out, bool *overtimed) {
    KHIP_TRY(alloc());
    DeviceLoopArgs a = args;
    if (third_stream && !a.columns && a.drain_to[1] && !a.drain_to[2]) a.drain_to[2] = third_stream;
    int streams = 0;
    while (streams < 3 && a.drain_to[streams]) ++streams;
    if (a.columns) streams = 1;
    const size_t width = a.columns ? (size_t)a.width : 1;
    if (a.history && !hist)
      KHIP_TRY(khip_malloc(ctx, sizeof(double) * (size_t)streams * kHistWindowMax * width, reinterpret_cast<void **>(&hist)));
    const long long window = std::min<long long>(std::max<long long>(ctx->tune.hist_window, kDevChunk), kHistWindowMax);
    h.stop_seq = kSeqNever;
    h.hist_base = 0;
    h.hist_cap = window;
    set_history(h, a.history ? hist : nullptr);
    KHIP_CHECK_HIP(hipMemcpyAsync(dev, &h, sizeof(S), hipMemcpyHostToDevice, ctx->stream));
    KHIP_CHECK_HIP(hipStreamSynchronize(ctx->stream));          // h is a stack object

    int64_t enq = 0;            // iterations enqueued
    long long hist_base = 0;
    std::vector<double> win;
    auto drain = [&](long long upto_iter, const S &st) -> int {   // entries for iterations (hist_base, upto_iter]
      const long long cnt = upto_iter - hist_base;
      if (!a.history || cnt <= 0) return KHIP_OK;
      win.resize((size_t)cnt * width);
      for (int s = 0; s < streams; ++s) {
        KHIP_CHECK_HIP(hipMemcpy(win.data(), hist + (size_t)s * kHistWindowMax * width, sizeof(double) * (size_t)cnt * width,
                                 hipMemcpyDeviceToHost));
        if (!a.columns) {                                         // stream s up to its own last entry (all of cnt but for bilqr!)
          const long long rows = std::max<long long>(0, std::min<long long>(cnt, hist_rows(st, s) - hist_base));
          a.drain_to[s]->insert(a.drain_to[s]->end(), win.begin(), win.begin() + rows);
          continue;
        }
        for (size_t c = 0; c < width; ++c) {
          const long long rows = std::min<long long>(cnt, hist_rows(st, (int)c) - hist_base);
          for (long long r = 0; r < rows; ++r) a.columns[c].push_back(win[(size_t)r * width + c]);
        }
      }
      return KHIP_OK;
    };
    int rc = KHIP_OK;
    bool stopped = false;
    for (int chunk = 0; !stopped; ++chunk) {
      const int64_t c = std::min<int64_t>(chunk == 0 ? a.first_chunk : kDevChunk, a.itmax - enq);
      if (a.history && enq + c - hist_base > window) {         // window full: empty it (rare: every 16384 iterations)
        KHIP_CHECK_HIP(hipStreamSynchronize(ctx->stream));
        S cur;
        KHIP_CHECK_HIP(hipMemcpy(&cur, dev, sizeof(cur), hipMemcpyDeviceToHost));
        if (cur.stop_seq != kSeqNever) break;
        if ((rc = drain(cur.iter, cur)) != KHIP_OK) break;
        hist_base = cur.iter;
        KHIP_CHECK_HIP(hipMemcpy(&dev->hist_base, &hist_base, sizeof(hist_base), hipMemcpyHostToDevice));
      }
      for (int64_t i = 0; i < c && rc == KHIP_OK; ++i) rc = step(dev, (long long)(enq + i));
      if (rc == KHIP_OK) rc = before_snapshot();
      ctx->ctl = SeqCtl{};
      if (rc != KHIP_OK) break;
      enq += c;
      const int b = chunk & 1;
      KHIP_CHECK_HIP(hipMemcpyAsync(&pinned[b], dev, sizeof(S), hipMemcpyDeviceToHost, ctx->stream));
      KHIP_CHECK_HIP(hipEventRecord(snap_ev[b], ctx->stream));
      if (chunk >= 1) {                                        // look at the PREVIOUS chunk: the queue never runs dry
        KHIP_CHECK_HIP(hipEventSynchronize(snap_ev[b ^ 1]));
        if (pinned[b ^ 1].stop_seq != kSeqNever) stopped = true;
      }
      if (enq >= a.itmax) stopped = true;
      if (!stopped && time_limit_reached(ctx, now_s() - a.t0, a.timemax)) { *overtimed = true; stopped = true; }
    }
    ctx->ctl = SeqCtl{};
    KHIP_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    if (rc != KHIP_OK) return rc;
    KHIP_CHECK_HIP(hipMemcpy(out, dev, sizeof(S), hipMemcpyDeviceToHost));
    return drain(out->iter, *out);
  }
  template <class Step>
  int run(khip_ctx *ctx, const S &h, const DeviceLoopArgs &a, Step &&step, S *out, bool *overtimed) {
    return run(ctx, h, a, step, [] { return KHIP_OK; }, out, overtimed);
  }
};

}  // namespace
}  // namespace khip

#include "solve_frame.hpp"   // the frame around a solver's iterations, on top of the pieces above
