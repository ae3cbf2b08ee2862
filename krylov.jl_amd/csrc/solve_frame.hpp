// solve_frame.hpp -- what surrounds the iterations of a single-vector solver, written once: the shape check, the warm-start
// residual, the end of a solve, the tail of a host-driven iteration, one stage of a device-resident iteration, the arguments of
// the device loop and the replay of the role rotations after it.  Included by solver_host.hpp (it needs StatsBox, DeviceLoopArgs
// and the K macro's workspace conventions): a workspace W has ctx, m, n, box and, where it can be warm-started, x, dx, warm_start.
#pragma once

namespace khip {
namespace {   // one copy per solver file, like everything in solver_host.hpp

// the stored shape of every CSR handle among `ops` against the workspace's (user operators have none to check)
template <class W> int check_shape(W *ws, std::initializer_list<const khip_operator *> ops) {
  for (const khip_operator *op : ops) {
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
  return KHIP_OK;
}

// dst = b - (A + λI) Δx after a warm start, dst = b otherwise
template <class W>
int residual0(W *ws, const khip_operator *A, double lambda, const double *b, bool warm_start, double *dst) {
  khip_ctx *ctx = ws->ctx;
  if (!warm_start) return khip_copy(ctx, ws->n, dst, b);
  KHIP_TRY(apply_op(ctx, A, ws->dx, dst));
  if (lambda != 0) KHIP_TRY(khip_axpy(ctx, ws->n, lambda, ws->dx, dst));
  return khip_axpby(ctx, ws->n, 1.0, b, -1.0, dst);
}

// the tail of every return past the checks: the timers and the history behind stats.residuals
template <class W> void ws_finish(W *ws, double t0) {
  ws->box.st.timer = now_s() - t0;
  ws->box.st.allocation_timer += take_alloc_seconds();          // lazy allocations of this solve (allocate_if)
  ws->box.publish();
}

struct EndArgs {
  int64_t iter;
  int solved, inconsistent;
  const char *status;
  bool warm_start;
  double t0;
  bool sync;                 // khip_ctx_sync before the stats are written
};
// every return of a solve past the checks: x <- x + Δx, the warm start is used up, the stats
template <class W> int ws_end(W *ws, const EndArgs &e) {
  if (e.warm_start) K(khip_axpy(ws->ctx, ws->n, 1.0, ws->dx, ws->x));
  ws->warm_start = false;
  if (e.sync) K(khip_ctx_sync(ws->ctx));
  khip_stats *st = &ws->box.st;
  st->niter = (int)e.iter;
  st->solved = e.solved;
  st->inconsistent = e.inconsistent;
  snprintf(st->status, sizeof(st->status), "%s", e.status);
  ws_finish(ws, e.t0);
  return KHIP_OK;
}

// the end of an iteration on the host-driven loops: the callback, which reads stats.residuals, and the time limit
template <class W>
void host_exit(W *ws, const khip_options &o, double t0, double timemax, bool *user_exit, bool *overtimed) {
  if (o.callback) {
    ws->box.publish();
    *user_exit = o.callback(ws, o.callback_data) != 0;
  }
  *overtimed = time_limit_reached(ws->ctx, now_s() - t0, timemax);
}

// One stage of a device-resident iteration whose launch ends in a reduction of nsums sums: the launch carries the sequence
// number and the epilogue that consumes the sums, which are combined across ranks where there are several.  launch(slot)
// returns an rc; it is a [&] lambda at every call, inlined like DeviceLoop::run's step.
template <class S, class Launch> int dev_stage(khip_ctx *ctx, S *dev, long long seq, int epi, int nsums, Launch &&launch) {
  ctx->ctl = SeqCtl{&dev->stop_seq, seq, epi, dev};
  const int slot = take_slots(ctx, nsums);
  int rc = launch(slot);
  if (rc == KHIP_OK && ctx->comm) rc = comm_allreduce_dd_device(ctx, slot, nsums);
  return rc;
}
// ... and a stage without a reduction
template <class Launch>
int dev_pass(khip_ctx *ctx, const long long *stop_seq, long long seq, int epi, void *state, Launch &&launch) {
  ctx->ctl = SeqCtl{stop_seq, seq, epi, state};
  return launch();
}

// The arguments of DeviceLoop::run with one host vector per history stream.  A finite timemax: the first chunk is ONE
// iteration, so that a limit already used up stops after iteration 1 as the host-driven loop does.
DeviceLoopArgs device_loop_args(int64_t itmax, double t0, double timemax, bool history,
                                std::initializer_list<std::vector<double> *> streams) {
  DeviceLoopArgs a{itmax, t0, timemax, history, {nullptr, nullptr, nullptr}, timemax < 1e300 ? 1 : kDevChunk};
  int h = 0;
  for (std::vector<double> *s : streams) a.drain_to[h++] = s;
  return a;
}

// The roles after a device loop: the host rotated them once per iteration it ENQUEUED, the device ran `iter` of them, and
// `period` rotations bring the roles back to where they began.
template <class R, class Rotate> R replay(R first, int64_t iter, int period, Rotate &&rotate) {
  for (int64_t j = 0; j < iter % period; ++j) rotate(first);
  return first;
}

}  // namespace
}  // namespace khip
