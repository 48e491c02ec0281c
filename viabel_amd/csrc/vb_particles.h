// What the particle entries share (vb_hmc.hip, vb_smc.hip, vb_svgd.hip, vb_ksd.hip): the 256-thread sum, the 64 x 64 pair
// tile's constants and draw order, the constants of an HMC transition's Metropolis decision; on the host the refusals of a
// model that cannot serve rows on the device, the positive-and-finite check, the padded row copies and the guard that drains
// the stream on every way out.  (wave_sum, wave_max and Carver are vb_rows_target.h's.)  Not part of the C ABI.
#pragma once

#include "vb_rows_target.h"

#include <cmath>

namespace vb {

// 256 threads, a fixed tree: the wave by shuffles, the four waves as (w0 + w1) + (w2 + w3); every thread gets the sum.  sh: 4
// doubles of LDS, free again after the call's first barrier, so two calls in a row may share it.
__device__ __forceinline__ double block_sum(double x, double* sh) {
  x = wave_sum(x);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = x;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

constexpr int kPairTile = 64;               // rows per row block and per column tile
constexpr int kPairK = 16;                  // coordinates per LDS step
constexpr int kPairLdsRow = kPairTile + 2;  // doubles per coordinate in LDS: the two more keep the staging stores (four
                                            // coordinates 2 q apart per 16 lanes) on distinct banks; reads have one coordinate
                                            // per instruction and do not care
// the thread's four rows of a 64-row tile: two adjacent pairs 32 apart, so that the 16 lanes of one ds_read_b128 group read
// 256 contiguous bytes (threads along the tile) or two adjacent 16-byte pieces (threads across it, broadcast)
__device__ __forceinline__ int pair_draw(int t, int q) { return (q >> 1) * 32 + t * 2 + (q & 1); }

constexpr uint32_t kUniformCol = 0xFFFFFFFEu;      // pseudo column of the accept, jitter and stage uniforms
constexpr double kDivergence = 1000.0;             // an energy error above this is a divergence

// `entry` needs a bound model of dimension d, the width of its argument `arg`.  `hint` continues the advice in a message's
// closing parenthesis (ksd: ", or pass scores")
inline int model_bound_refuse(vb_ctx* ctx, const char* entry, const char* arg, int64_t d, const char* hint = "") {
  const ModelDev& m = ctx->model;
  if (m.id < 0) return fail(ctx, VB_ERR_STATE, "%s: no model bound (vb_set_model%s)", entry, hint);
  if (d != m.dim)
    return fail(ctx, VB_ERR_INVALID, "%s: %s has %lld columns, model dimension is %d", entry, arg, (long long)d, m.dim);
  return VB_OK;
}
// the bound model serves rows on the device: no host callback; whole_target: no minibatch target; one_process: no
// communicator attached
inline int model_device_refuse(vb_ctx* ctx, const char* entry, bool whole_target, bool one_process, const char* hint = "") {
  const ModelDev& m = ctx->model;
  if (m.id == VB_MODEL_SOURCE && ctx->user_host_fn)
    return fail(ctx, VB_ERR_UNSUPPORTED, "%s evaluates the model's rows on the device without host synchronisation: a "
                                         "host-callback model cannot supply them (write the density as a source model%s)",
                entry, hint);
  if (whole_target && m.id == VB_MODEL_MINIBATCH_GLM)
    return fail(ctx, VB_ERR_UNSUPPORTED, "%s needs the scores of the whole target: the minibatch target's change from batch "
                                         "to batch (bind the full-data model%s)", entry, hint);
  if (one_process && ctx->comm)
    return fail(ctx, VB_ERR_UNSUPPORTED, "%s runs on one process's engine: detach the communicator", entry);
  return VB_OK;
}

// entries [0, n) of `what` must be positive and finite
inline int positive_finite(vb_ctx* ctx, const char* entry, const char* what, const double* v, int64_t n) {
  for (int64_t j = 0; j < n; ++j)
    if (!(v[j] > 0.0) || !std::isfinite(v[j]))
      return fail(ctx, VB_ERR_INVALID, "%s: %s[%lld] must be positive and finite", entry, what, (long long)j);
  return VB_OK;
}

// n host rows of d doubles into device rows of ld doubles at dst, enqueued on ctx->stream; the pad columns are zeroed
// first unless the caller has zeroed them already or a kernel writes them before anything reads them
inline int upload_rows(vb_ctx* ctx, double* dst, const double* src, int64_t n, int64_t d, int64_t ld, bool zero_pads = true) {
  const size_t row_bytes = (size_t)d * sizeof(double), ld_bytes = (size_t)ld * sizeof(double);
  if (zero_pads && ld != d) VB_HIP(ctx, hipMemsetAsync(dst, 0, (size_t)n * ld_bytes, ctx->stream));
  VB_HIP(ctx, hipMemcpy2DAsync(dst, ld_bytes, src, row_bytes, row_bytes, (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  return VB_OK;
}
// the way back: n device rows of ld doubles into host rows of d
inline hipError_t download_rows(vb_ctx* ctx, double* dst, const double* src, int64_t n, int64_t d, int64_t ld) {
  const size_t row_bytes = (size_t)d * sizeof(double);
  return hipMemcpy2DAsync(dst, row_bytes, src, (size_t)ld * sizeof(double), row_bytes, (size_t)n, hipMemcpyDeviceToHost,
                          ctx->stream);
}

// Declared before an entry's first enqueue: the stream is drained on every way out, so the host memory its asynchronous
// uploads read (the caller's arrays, the entry's own staging) outlives them also where a later step fails.
struct StreamDrain {
  hipStream_t st;
  ~StreamDrain() { (void)hipStreamSynchronize(st); }
};

}  // namespace vb
