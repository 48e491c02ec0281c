// What the rows targets share (vb_softmax.hip, vb_multilevel.hip, vb_locscale.hip, vb_sparse.hip, vb_neuralnet.hip) and,
// through vb_particles.h, the particle entries: the plain-store GEMM epilogue, the wave and workgroup sums in their fixed
// order, the per-observation constant of a GLM likelihood, and the host pieces of a layout, of the argument checks and of
// vb_set_model.  Not part of the C ABI.
#pragma once

#include "vb_common.h"
#include "vb_gemm_f64.h"

namespace vb {

constexpr double kLog2Pi = 1.8378770664093454835606594728112;
constexpr double kHalfLog2Pi = 0.91893853320467274178;

struct EpiStorePlain {       // Y = acc
  double* Y;
  int64_t ldy;
  __device__ void operator()(int, int row, int col, double acc) const { Y[(int64_t)row * ldy + col] = acc; }
  __device__ d2v pair(int, int row, int col, double a0, double a1) const {
    const d2v v = (d2v){a0, a1};
    *reinterpret_cast<d2v*>(Y + (int64_t)row * ldy + col) = v;
    return v;
  }
};

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
  return x;
}
__device__ __forceinline__ double wave_max(double x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x = fmax(x, __shfl_down(x, off, 64));
  return x;
}

// The tail of a 256-thread (row, strip) workgroup: NP = 1 or 2 sums over its lanes to part[NP blockIdx.x (+ 1)] -- the wave
// by shuffles, the four waves as (w0 + w1) + (w2 + w3).  Every thread of the workgroup must call it.
template <int NP>
__device__ __forceinline__ void strip_partials_store(double a, double b, double* __restrict__ part) {
  __shared__ double wsum[8];
  a = wave_sum(a);
  if (NP == 2) b = wave_sum(b);
  if ((threadIdx.x & 63) == 0) {
    wsum[threadIdx.x >> 6] = a;
    if (NP == 2) wsum[4 + (threadIdx.x >> 6)] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[NP * (int64_t)blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
    if (NP == 2) part[2 * (int64_t)blockIdx.x + 1] = (wsum[4] + wsum[5]) + (wsum[6] + wsum[7]);
  }
}

// what glm_term leaves out of log p(y | eta): the constant of one observation
__host__ __device__ __forceinline__ double glm_obs_const(int link, double aux, double y) {
  if (link == VB_GLM_POISSON) return -lgamma(y + 1.0);
  if (link == VB_GLM_GAUSSIAN) return -log(aux) - kHalfLog2Pi;
  return 0.0;
}

// c0 / f0 of vb_set_model continued with that constant over the n observations y: the Poisson terms one by one in index
// order, the Gaussian ones as one product
inline double glm_const_continue(double acc, int link, double aux, const double* y, int64_t n) {
  if (link == VB_GLM_POISSON)
    for (int64_t i = 0; i < n; ++i) acc += glm_obs_const(link, aux, y[i]);
  else if (link == VB_GLM_GAUSSIAN)
    acc -= (double)n * (log(aux) + 0.5 * kLog2Pi);
  return acc;
}

// offsets into a workspace in multiples of 32 doubles: every piece starts 256-B aligned
struct Carver {
  int64_t off = 0;
  int64_t operator()(int64_t doubles) {
    const int64_t o = off;
    off += round_up(doubles, 32);
    return o;
  }
};

// rows per chunk: what the budget holds, at least 8, at most the n rows there are
inline int64_t rows_chunk(int64_t budget_doubles, int64_t doubles_per_row, int64_t n) {
  int64_t chunk = budget_doubles / doubles_per_row;
  chunk = chunk < 8 ? 8 : chunk;
  return chunk > n ? n : chunk;
}

// the GEMM-fed targets: the GEMMs move 16-byte pairs of Z and G, and the gradient's epilogue addresses both with one stride
inline int rows_operands_check(vb_ctx* ctx, const char* name, const double* Z, int64_t ldz, int d, const double* G,
                               int64_t ldg) {
  if (((uintptr_t)Z & 15) || (ldz & 1) || ldz < d)
    return fail(ctx, VB_ERR_INVALID, "%s rows: the samples must be 16-byte aligned with an even row stride >= %d", name, d);
  if (G && (((uintptr_t)G & 15) || ldg != ldz))
    return fail(ctx, VB_ERR_INVALID, "%s rows: the gradient must be 16-byte aligned and share the samples' row stride "
                                     "(%lld, not %lld)", name, (long long)ldz, (long long)ldg);
  return VB_OK;
}

// the dense design in both forms, [X (n_data x ldp) | X' (p x ldq)] at dev[at], from the row-major src (n_data x p); dev is
// sized and zero already, so the pad columns stay zero
inline void pack_design(std::vector<double>& dev, size_t at, const double* src, int64_t n_data, int64_t p, int64_t ldp,
                        int64_t ldq) {
  for (int64_t i = 0; i < n_data; ++i)
    for (int64_t j = 0; j < p; ++j) {
      const double v = src[i * p + j];
      dev[at + (size_t)i * ldp + j] = v;
      dev[at + (size_t)n_data * ldp + (size_t)j * ldq + i] = v;
    }
}

}  // namespace vb
