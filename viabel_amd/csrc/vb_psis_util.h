// Helpers shared by the Pareto-smoothing kernels (vb_psis.hip: one long vector; vb_psis_batch.hip: many short ones):
// wave reductions, the order-preserving key of the radix select and the (value, index) order of the tail sort.
#pragma once

#include "vb_common.h"

namespace vb {

__device__ __forceinline__ double ps_wave_sum(double x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
  return x;
}
__device__ __forceinline__ double ps_wave_max(double x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x = fmax(x, __shfl_down(x, off, 64));
  return x;
}

__device__ __forceinline__ unsigned long long ps_key(double v) {   // ascending order-preserving key
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double ps_unkey(unsigned long long k) {
  const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)u);
}

// (value, index) lexicographic "a after b"
__device__ __forceinline__ bool ps_after(double av, int ai, double bv, int bi) {
  return (av > bv) | ((av == bv) & (ai > bi));      // no short circuit: a branch per comparison cost 25 us per call
}

}  // namespace vb
