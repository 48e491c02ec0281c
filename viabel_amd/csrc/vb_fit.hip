// Device-resident stochastic-gradient step: the descent directions of the reference's optimisers
// (optimization.py: StochasticGradientOptimizer :51-145, RMSProp :147-197, Adam :260-326, Adagrad :398-433)
// applied to the parameter where the objective kernels left (value, grad) -- so a whole fit is a chain of
// {Philox noise -> objective -> step} launches on one stream with no host round trip (vb_fit below; what it shares
// with vb_flow_fit is FitRun, vb_fit_run.h).
//
// The arithmetic is written operation by operation in numpy's order and compiled without floating-point
// contraction, so that a device fit reproduces the host loop (numpy update on the same gradients) bit for
// bit: IEEE fp64 multiply / add / divide / sqrt are correctly rounded on both sides.
#include "vb_common.h"
#include "vb_fit.h"
#include "vb_fit_run.h"

namespace vb {

namespace {

#pragma clang fp contract(off)

__global__ void __launch_bounds__(256) fit_step_kernel(FitStep a) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i == 0) a.values[a.k] = a.out[0];
  if (i >= a.p) return;
  fit_step_apply(a, i, a.out[1 + i]);
}

}  // namespace

int fit_step_enqueue(vb_ctx* ctx, const FitStep& a) {
  hipLaunchKernelGGL(fit_step_kernel, dim3((unsigned)((a.p + 255) / 256)), dim3(256), 0, ctx->stream, a);
  VB_HIP(ctx, hipGetLastError());
  return VB_OK;
}

}  // namespace vb

using namespace vb;

extern "C" {

// ---- device-resident fit (optimization.py:83-127) ----------------------------------------------------
int vb_fit(vb_ctx* ctx, int slot, int slot_aux, int64_t n, int64_t d, int64_t n_total, int64_t row_offset, int family,
           double df, unsigned flags, int cv_mode, int noise_kind, double noise_df, uint64_t seed,
           uint64_t first_stream, int opt_kind, const double hyper[4], int64_t n_iters, double* theta, int64_t p,
           double* state, int has_state, double* values, double* history, int64_t hist_len, double* directions,
           double* gradients) {
  if (!ctx || !hyper || !theta || !values) return fail(ctx, VB_ERR_INVALID, "NULL argument");
  VB_TRY(FitRun::check(ctx, "n, d", n > 0 && d > 0, n, n_total, n_iters, opt_kind, hist_len, history, has_state,
                       state));
  const bool meanfield = family == VB_FAMILY_MF_GAUSSIAN || family == VB_FAMILY_MF_STUDENT_T;
  const bool fullrank = family == VB_FAMILY_FULLRANK_GAUSSIAN;
  const bool lowrank = family == VB_FAMILY_LOWRANK_GAUSSIAN;
  if (!meanfield && !fullrank && !lowrank)
    return fail(ctx, VB_ERR_UNSUPPORTED, "device-resident fit: family %d is not supported", family);
  const int64_t lr_k = lowrank ? (p - 2 * d) / d : 0;
  if (lowrank) {
    if (lr_k < 1 || lr_k > 16 || p != 2 * d + d * lr_k)
      return fail(ctx, VB_ERR_INVALID, "low-rank family: parameter length %lld is not 2 d + d k with 1 <= k <= 16",
                  (long long)p);
    if (cv_mode != VB_CV_NONE || (flags & VB_FLAG_PATH_DERIV))
      return fail(ctx, VB_ERR_UNSUPPORTED, "low-rank family: entropy-form estimator only");
    if (slot_aux == slot) return fail(ctx, VB_ERR_INVALID, "the two noise blocks need different slots");
  } else if (p != (meanfield ? 2 * d : d + d * (d + 1) / 2)) {
    return fail(ctx, VB_ERR_INVALID, "parameter length %lld does not match the family", (long long)p);
  }
  if (fullrank && cv_mode != VB_CV_NONE)
    return fail(ctx, VB_ERR_UNSUPPORTED, "full-rank family: the RGE control variates do not apply");
  VB_HIP(ctx, hipSetDevice(ctx->device));
  VB_TRY(main_stream_write(ctx));
  VB_TRY(noise_slot_alloc(ctx, slot, n, d));
  NoiseSlot& ns = ctx->noise[slot];
  if (lowrank) VB_TRY(noise_slot_alloc(ctx, slot_aux, n, lr_k));

  FitRun run(ctx);      // (the parameter lives at the front of the fit's workspace)
  VB_TRY(run.begin(p, p, n_iters, opt_kind, hyper, state, has_state, history, hist_len, directions, gradients));
  FitStep& step = run.step;
  double* theta_dev = step.theta = run.front;
  double* out_dev = run.out;
  hipStream_t st = ctx->stream;
  VB_HIP(ctx, hipMemcpyAsync(theta_dev, theta, (size_t)p * sizeof(double), hipMemcpyHostToDevice, st));
  VB_HIP(ctx, hipStreamSynchronize(st));   // the caller's buffers are pageable: copies above are staged

  MfCall c;
  if (meanfield) {
    c.count = 1;
    c.noise[0] = &ns;
    c.theta_src[0] = theta_dev;
    c.theta_on_device = true;
    c.out[0] = out_dev;
    c.n = n;
    c.d = d;
    c.n_total = n_total;
    c.family = family;
    c.df = df;
    c.flags = flags;
    c.cv_mode = cv_mode;
  }
  const bool gen_in_kernel =
      (ctx->model.id == VB_MODEL_GAUSS_DIAG || ctx->model.id == VB_MODEL_FUNNEL) &&
      ((family == VB_FAMILY_MF_GAUSSIAN && noise_kind == VB_NOISE_NORMAL) ||
       (family == VB_FAMILY_MF_STUDENT_T && noise_kind == VB_NOISE_STUDENT_T && noise_df == df));
  bool step_done = false, prep_done = false;
  // the dense family's fused step leaves mu / L' of the FIT's iterate in fr_lt (fr_step_unpack_enqueue): on every way out
  // of this function -- error returns included -- the copy is declared stale for the resident parameter too, or a later
  // set_theta-once / enqueue-many caller with the same d would be evaluated at the fit's parameter
  struct LtReset {
    vb_ctx* c;
    bool on;
    ~LtReset() {
      if (on) {
        c->fr_lt_owner = nullptr;
        c->fr_lt_d = 0;
      }
    }
  } lt_reset{ctx, fullrank};
  if (meanfield) {
    c.step = &step;
    c.step_done = &step_done;
    c.prep_done = &prep_done;
  }
  for (int64_t k = 0; k < n_iters; ++k) {
    run.iteration(k);
    step_done = false;
    if (lowrank) {
      NoiseSlot& nz = ctx->noise[slot_aux];
      const uint64_t s2 = 2 * (first_stream + (uint64_t)k);
      VB_TRY(rng_fill(ctx, (double*)ns.buf.ptr, ns.ld, VB_NOISE_NORMAL, 0.0, seed, s2, row_offset, n, d));
      VB_TRY(rng_fill(ctx, (double*)nz.buf.ptr, nz.ld, VB_NOISE_NORMAL, 0.0, seed, s2 + 1, row_offset, n, lr_k));
      VB_TRY(lr_elbo_grad_enqueue(ctx, ns, nz, n, d, lr_k, n_total, theta_dev, out_dev));
    } else if (gen_in_kernel) {
      // single-use Gaussian noise never touches HBM: the streaming kernel generates it in registers
      c.skip_prep = prep_done;                 // done by the previous iteration's finalize kernel
      c.prep_next = k + 1 < n_iters;
      prep_done = false;
      c.gen = 1;
      c.gen_seed = seed;
      c.gen_stream = first_stream + (uint64_t)k;
      c.gen_row_offset = row_offset;
      VB_TRY(mf_enqueue(ctx, c));
    } else {
      VB_TRY(rng_fill(ctx, (double*)ns.buf.ptr, ns.ld, noise_kind, noise_df, seed, first_stream + (uint64_t)k,
                      row_offset, n, d));
      if (meanfield)
        VB_TRY(mf_enqueue(ctx, c));
      else
        VB_TRY(fr_elbo_grad_enqueue(ctx, ns, n, d, n_total, theta_dev, out_dev, flags));
    }
    if (fullrank && ctx->pipe.post_pending) {   // sharded full-rank evaluations finish on the communication stream
      VB_HIP(ctx, hipStreamWaitEvent(st, ctx->pipe.ev_fin[ctx->pipe.last_set], 0));
      ctx->pipe.post_pending = false;
    }
    if (fullrank && !ctx->comm) {
      // dense family: the step writes mu and L' of the stepped parameter itself, the next evaluation skips its unpack
      VB_TRY(fr_step_unpack_enqueue(ctx, step, d));
      step_done = true;
    }
    if (!step_done) VB_TRY(fit_step_enqueue(ctx, step));
    VB_TRY(run.after_step(k));
  }
  return run.finish(theta, values, state);
}

namespace {
// out[j] = (h[0][j] + h[1][j] + ... in row order) / rows: numpy's add.reduce over the leading axis followed by true_divide
__global__ void __launch_bounds__(256) fit_history_mean_kernel(const double* __restrict__ h, int64_t rows, int64_t p,
                                                               double* __restrict__ out) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= p) return;
  double s = h[j];
  for (int64_t r0 = 1; r0 < rows; r0 += 8) {      // eight rows' loads in flight, added in row order
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = h[(r0 + u < rows ? r0 + u : rows - 1) * p + j];
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (r0 + u < rows) s += v[u];
  }
  out[j] = s / (double)rows;
}
}  // namespace

}  // extern "C"

namespace vb {
int history_mean_enqueue(vb_ctx* ctx, const double* h, int64_t rows, int64_t p, double* out) {
  hipLaunchKernelGGL(fit_history_mean_kernel, dim3((unsigned)((p + 255) / 256)), dim3(256), 0, ctx->stream, h, rows, p, out);
  VB_HIP(ctx, hipGetLastError());
  return VB_OK;
}
}  // namespace vb

extern "C" {

int vb_fit_history_mean(vb_ctx* ctx, int64_t rows, int64_t p, double* mean) {
  if (!ctx || !mean || rows <= 0 || p <= 0) return fail(ctx, VB_ERR_INVALID, "bad argument");
  if (!ctx->fit_work.ptr || ctx->fit_hist_len < rows || ctx->fit_hist_p != p)
    return fail(ctx, VB_ERR_STATE, "no resident iterate history of %lld rows x %lld (the last fit kept %lld x %lld)", (long long)rows,
                (long long)p, (long long)ctx->fit_hist_len, (long long)ctx->fit_hist_p);
  VB_HIP(ctx, hipSetDevice(ctx->device));
  VB_TRY(main_stream_write(ctx));
  const double* h = (const double*)ctx->fit_work.ptr + ctx->fit_hist_off + (ctx->fit_hist_len - rows) * p;
  double* out = (double*)ctx->fit_work.ptr + ctx->fit_out_off;      // (the fit's own [value | gradient] area: free once it has returned)
  hipStream_t st = ctx->stream;
  VB_TRY(history_mean_enqueue(ctx, h, rows, p, out));
  const FetchSeg seg[1] = {{out, (size_t)p * sizeof(double), mean}};
  return fetch_blocking(ctx, st, seg, 1);
}

}  // extern "C"
