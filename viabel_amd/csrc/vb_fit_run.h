// FitRun: the part of a device-resident fit that does not depend on the family.  It owns the optimiser step's arguments
// (FitStep), lays out ctx->fit_work -- the only code that does --
//   [theta (front: the families whose parameter lives here) | out (1 + p) | s1 (p) | s2 (p) | values (n_iters)
//    | iterates (hist_len x p) | directions (n_iters x p) | gradients (n_iters x p)]          (each rounded up to 16 doubles)
// and moves the state in and the results out.  vb_fit (vb_fit.hip) and vb_flow_fit (vb_flow.hip) add their checks, their
// parameter upload and the loop body; vb_fit_history_mean reads the kept iterates back through ctx->fit_hist_*.
// While an iterate chain is open (vb_chain_open, vb_chain.hip) the step's history store points at the chain's tail instead:
// iterate k lands in row chain_rows + k, nothing of length p is logged for the history, finish() adds n_iters to chain_rows.
//
// The rows a fit logs per iteration (iterate, descent direction, gradient: optimization.py:83-127 returns every iterate,
// :541 FASO's gradient history) used to leave in one pageable copy after the last step: at p = 525 312 (D = 1024 dense)
// 4.2 MB per row at ~13 GB/s, as long again as the iteration that produced it.  With long rows each iteration's rows go,
// behind an event, through a copy stream into a ring of pinned slots while the following iterations run; the enqueuing
// thread, which is R iterations ahead of the GPU at most, moves a slot to the caller's arrays before it reuses it.
#pragma once

#include "vb_common.h"

#include <cstdlib>
#include <cstring>

namespace vb {

struct FitRun {
  vb_ctx* ctx;
  FitStep step;                 // the caller sets step.theta
  double* front = nullptr;      // the first `front_doubles` doubles of the workspace (vb_fit's parameter)
  double* out = nullptr;        // [value | grad (p)]: where the objective of an iteration leaves its result
  int64_t n_iters = 0, hist_len = 0, o_out = 0, o_hist = 0;
  int has_state = 0;
  double *h_hist = nullptr, *h_dirs = nullptr, *h_grads = nullptr;      // caller's arrays
  bool streamed = false;        // the logged rows leave through the pinned ring
  bool chained = false;         // the iterates go to the open chain's tail (no history of their own)
  int64_t drained = 0;          // iterations whose rows have reached the caller

  explicit FitRun(vb_ctx* c) : ctx(c) {}

  // the checks every device fit shares; `sizes` names what `sizes_positive` covers besides n_iters
  static int check(vb_ctx* ctx, const char* sizes, bool sizes_positive, int64_t n, int64_t n_total, int64_t n_iters,
                   int opt_kind, int64_t hist_len, const double* history, int has_state, const double* state) {
    if (ctx->model.id < 0) return fail(ctx, VB_ERR_STATE, "no model bound (vb_set_model)");
    if (!sizes_positive || n_iters <= 0) return fail(ctx, VB_ERR_INVALID, "%s and n_iters must be positive", sizes);
    if (n_total < n) return fail(ctx, VB_ERR_INVALID, "n_total must be >= n");
    if (opt_kind < VB_OPT_SGD || opt_kind > VB_OPT_ADAGRAD)
      return fail(ctx, VB_ERR_INVALID, "unknown optimiser kind %d", opt_kind);
    if (hist_len < 0 || hist_len > n_iters || (hist_len > 0 && !history))
      return fail(ctx, VB_ERR_INVALID, "hist_len must be in [0, n_iters] with a history buffer");
    if (has_state && !state) return fail(ctx, VB_ERR_INVALID, "has_state set without a state buffer");
    return VB_OK;
  }

  // Workspace, optimiser state (uploaded, or zeroed) and row stream.  The uploads are enqueued only: the caller adds its
  // own and synchronises once (the caller's buffers are pageable: the copies are staged).
  int begin(int64_t p, int64_t front_doubles, int64_t iters, int opt_kind, const double hyper[4], const double* state,
            int with_state, double* history, int64_t hist, double* directions, double* gradients) {
    n_iters = iters, hist_len = hist, has_state = with_state;
    chained = ctx->chain_open;
    if (chained) {      // (before anything is allocated or launched)
      if (hist > 0)
        return fail(ctx, VB_ERR_INVALID, "an iterate chain is open: the iterates stay on the device, pass hist_len = 0");
      if (p != ctx->chain_p)
        return fail(ctx, VB_ERR_INVALID, "the open iterate chain holds rows of %lld doubles, this fit's parameter has %lld",
                    (long long)ctx->chain_p, (long long)p);
      if (iters > ctx->chain_cap - ctx->chain_rows)
        return fail(ctx, VB_ERR_INVALID, "the open iterate chain has room for %lld more rows, this fit appends %lld",
                    (long long)(ctx->chain_cap - ctx->chain_rows), (long long)iters);
    }
    int64_t off = 0;
    auto carve = [&off](int64_t doubles) {
      const int64_t o = off;
      off += round_up(doubles, 16);
      return o;
    };
    carve(front_doubles);
    o_out = carve(1 + p);
    const int64_t o_s1 = carve(p), o_s2 = carve(p), o_val = carve(n_iters);
    o_hist = carve(hist_len * p);
    const int64_t o_dirs = carve(directions ? n_iters * p : 0), o_grads = carve(gradients ? n_iters * p : 0);
    ctx->fit_hist_len = 0;      // (the kept iterates of an earlier fit are about to be overwritten)
    VB_TRY(ensure(ctx, ctx->fit_work, (size_t)off * sizeof(double)));
    double* base = (double*)ctx->fit_work.ptr;
    front = base;
    out = base + o_out;
    if (has_state) {
      VB_HIP(ctx, hipMemcpyAsync(base + o_s1, state, (size_t)p * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
      VB_HIP(ctx, hipMemcpyAsync(base + o_s2, state + p, (size_t)p * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    } else {   // the part of the state an optimiser does not use is returned as zeros, not as stale workspace
      VB_HIP(ctx, hipMemsetAsync(base + o_s1, 0, (size_t)(o_val - o_s1) * sizeof(double), ctx->stream));
    }
    step.kind = opt_kind;
    step.p = p;
    step.lr = hyper[0];
    step.beta1 = hyper[1];
    step.one_minus_beta1 = 1.0 - hyper[1];
    step.beta2 = hyper[2];
    step.one_minus_beta2 = 1.0 - hyper[2];
    step.jitter = hyper[3];
    step.out = out;
    step.s1 = base + o_s1;
    step.s2 = base + o_s2;
    step.values = base + o_val;
    step.hist = hist_len > 0 ? base + o_hist : nullptr;
    step.hist_first = n_iters - hist_len;
    if (chained) {
      step.hist = (double*)ctx->chain.ptr + ctx->chain_rows * p;
      step.hist_first = 0;
    }
    step.dirs = directions ? base + o_dirs : nullptr;
    step.grads = gradients ? base + o_grads : nullptr;
    h_hist = hist_len > 0 ? history : nullptr, h_dirs = directions, h_grads = gradients;
    return ring_begin();
  }

  void iteration(int64_t k) {
    step.k = k;
    step.first = (k == 0 && !has_state) ? 1 : 0;
  }

  int after_step(int64_t k) {      // iteration k's kernels (its step included) are enqueued on the main stream
    if (ctx->model.id == VB_MODEL_MINIBATCH_GLM) ++ctx->mb_batch;      // the next iteration's batch, as the host loop counts
    if (!streamed) return VB_OK;
    if (k >= vb_ctx::kFitRing) VB_TRY(drain_one());      // the slot's previous tenant: iteration k - R
    const int slot = (int)(k % vb_ctx::kFitRing);
    const int64_t p = step.p;
    hipStream_t cs = ctx->fit_copy_st;
    VB_HIP(ctx, hipEventRecord(ctx->fit_ev_step[slot], ctx->stream));
    VB_HIP(ctx, hipStreamWaitEvent(cs, ctx->fit_ev_step[slot], 0));
    double* dst = ctx->fit_ring.host_as<double>() + (size_t)slot * ctx->fit_ring_doubles;
    const size_t row = (size_t)p * sizeof(double);
    if (h_hist && k >= step.hist_first)
      VB_HIP(ctx, hipMemcpyAsync(dst, step.hist + (k - step.hist_first) * p, row, hipMemcpyDeviceToHost, cs));
    if (h_dirs) VB_HIP(ctx, hipMemcpyAsync(dst + p, step.dirs + k * p, row, hipMemcpyDeviceToHost, cs));
    if (h_grads) VB_HIP(ctx, hipMemcpyAsync(dst + 2 * p, step.grads + k * p, row, hipMemcpyDeviceToHost, cs));
    VB_HIP(ctx, hipEventRecord(ctx->fit_ev_copy[slot], cs));
    return VB_OK;
  }

  // results to the caller's arrays (`state` may be NULL), the one wait, the record vb_fit_history_mean reads
  int finish(double* theta, double* values, double* state) {
    const int64_t p = step.p;
    hipStream_t st = ctx->stream;
    auto fetch = [&](double* dst, const double* src, int64_t doubles) {
      return hipMemcpyAsync(dst, src, (size_t)doubles * sizeof(double), hipMemcpyDeviceToHost, st);
    };
    VB_HIP(ctx, fetch(theta, step.theta, p));
    VB_HIP(ctx, fetch(values, step.values, n_iters));
    if (state) {
      VB_HIP(ctx, fetch(state, step.s1, p));
      VB_HIP(ctx, fetch(state + p, step.s2, p));
    }
    if (!streamed) {
      if (h_hist) VB_HIP(ctx, fetch(h_hist, step.hist, hist_len * p));
      if (h_dirs) VB_HIP(ctx, fetch(h_dirs, step.dirs, n_iters * p));
      if (h_grads) VB_HIP(ctx, fetch(h_grads, step.grads, n_iters * p));
    } else {
      while (drained < n_iters) VB_TRY(drain_one());
    }
    VB_HIP(ctx, hipStreamSynchronize(st));
    ctx->fit_hist_off = o_hist, ctx->fit_hist_len = hist_len, ctx->fit_hist_p = p, ctx->fit_out_off = o_out;
    if (chained) ctx->chain_rows += n_iters;
    return comm_check(ctx);
  }

 private:
  int ring_begin() {
    const int64_t p = step.p;
    const char* e = getenv("VB_FIT_STREAM_ROWS");
    const char* m = getenv("VB_FIT_STREAM_MIN_BYTES");
    streamed = (h_hist || h_dirs || h_grads) && !(e && atoi(e) == 0) &&
               (size_t)p * sizeof(double) >= (m ? (size_t)atoll(m) : (size_t)1 << 18);
    if (!streamed) return VB_OK;
    VB_HIP(ctx, ctx->fit_copy_st.create(hipStreamNonBlocking));
    const size_t slot = (size_t)round_up(3 * p, 16);
    if (ctx->fit_ring_doubles < slot) {
      VB_HIP(ctx, hipStreamSynchronize(ctx->fit_copy_st));
      ctx->fit_ring_doubles = 0;
      VB_TRY(ensure_pinned(ctx, ctx->fit_ring, vb_ctx::kFitRing * slot * sizeof(double), false));
      ctx->fit_ring_doubles = slot;
    }
    for (int i = 0; i < vb_ctx::kFitRing; ++i) {
      VB_HIP(ctx, ctx->fit_ev_step[i].create(hipEventDisableTiming));
      VB_HIP(ctx, ctx->fit_ev_copy[i].create(hipEventDisableTiming));
    }
    return VB_OK;
  }
  int drain_one() {           // iteration `drained`: wait for its copies, hand the rows over
    const int64_t k = drained, p = step.p;
    const int slot = (int)(k % vb_ctx::kFitRing);
    VB_HIP(ctx, hipEventSynchronize(ctx->fit_ev_copy[slot]));
    const double* src = ctx->fit_ring.host_as<double>() + (size_t)slot * ctx->fit_ring_doubles;
    const size_t row = (size_t)p * sizeof(double);
    if (h_hist && k >= step.hist_first) memcpy(h_hist + (k - step.hist_first) * p, src, row);
    if (h_dirs) memcpy(h_dirs + k * p, src + p, row);
    if (h_grads) memcpy(h_grads + k * p, src + 2 * p, row);
    ++drained;
    return VB_OK;
  }
};

}  // namespace vb
