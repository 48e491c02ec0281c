// The steps of Pareto smoothing (viabel/_psis.py:113-209 psislw, :212-332 gpdfitnew), once, for the three kernels that run
// them: psis_kernel and psis_grid_kernel (vb_psis.hip: one long vector on one or on up to 64 workgroups of 1024 threads) and
// psis_batch_kernel (vb_psis_batch.hip: many short vectors, one 256-thread workgroup each).  In the order of the smoothing:
//   ps_wave_sum / ps_wave_max, ps_block_sum / ps_block_max      reductions in a fixed order
//   ps_key / ps_unkey, ps_hist_add, ps_wave_prefix, ps_pick_bin,
//   ps_scan_hist256, ps_bin_put, ps_rank_among                   exact radix select of the cut-off's key
//   ps_cutoff, ps_tail_put                                       the cut-off and the values above it
//   ps_after                                                     order of the tail by (value, index): the comparison
//   ps_tail_exp, ps_quad_points, ps_quad_ks, ps_gpd_fit          the Zhang-Stephens fit of the generalised Pareto tail
//   ps_quantile                                                  the fitted order statistic that replaces a tail value
// THREADS is the workgroup's size, CAP a capacity of the caller's LDS arrays; the arrays themselves are the kernels' and come
// in as pointers.  A function with a __syncthreads() inside says so: every thread of the workgroup must call it.  The order of
// every floating-point sum is fixed and part of the contract: the kernels agree on k-hat bit for bit.
// Two things stay in the kernels.  The loops over a thread's own weights (the select's passes, the two gathers) call the
// per-value functions here: a helper that took the loop as a callable gave psis_kernel<true>, which spills, more scratch.
// The rank sort of the tail is spelled out in psis_kernel and psis_batch_kernel: as one function here it spilled scalar
// registers in both.
#pragma once

#include "vb_common.h"

#include <cfloat>
#include <cmath>

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

// workgroup-wide sum / max over WAVES waves; every thread gets the result (sh: WAVES doubles; barriers inside).  Four waves
// add as (w0 + w1) + (w2 + w3), more add one after the other: the two orders give different last bits and both stay.
template <int WAVES>
__device__ __forceinline__ double ps_block_sum(double x, double* sh) {
  x = ps_wave_sum(x);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = x;
  __syncthreads();
  if constexpr (WAVES == 4) {
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
  } else {
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) t += sh[w];
    return t;
  }
}
template <int WAVES>
__device__ __forceinline__ double ps_block_max(double x, double* sh) {
  x = ps_wave_max(x);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = x;
  __syncthreads();
  if constexpr (WAVES == 4) {
    return fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
  } else {
    double t = sh[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) t = fmax(t, sh[w]);
    return t;
  }
}

__device__ __forceinline__ unsigned long long ps_key(double v) {   // ascending order-preserving key
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double ps_unkey(unsigned long long k) {
  const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)u);
}

// ---- radix select ---------------------------------------------------------------------------------------------------
// One key of every lane of a wave into an LDS histogram (act: this lane has one).  The top bytes of log weights are sign and
// exponent: a wave's 64 keys fall into one or two bins, and 64 LDS atomics on one address are served one after the other.
// Two rounds of "the first lane's bin: everybody in it is counted by one add"; what is left (the low bytes' spread-out bins)
// goes lane by lane.  Every lane of the wave must call it.
__device__ __forceinline__ void ps_hist_add(int* hist, int bin, bool act) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int round = 0; round < 2; ++round) {
    const unsigned long long todo = __ballot(act);
    if (!todo) break;
    const int leader = __builtin_ctzll(todo);
    const int b = __shfl(bin, leader, 64);
    const bool same = act && bin == b;
    const unsigned long long m = __ballot(same);
    if (lane == leader) atomicAdd(&hist[b], __builtin_popcountll(m));
    act = act && !same;
  }
  if (act) atomicAdd(&hist[bin], 1);
}

__device__ __forceinline__ long long ps_wave_prefix(long long x) {      // inclusive prefix sum over the lanes of a wave
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const long long up = __shfl_up(x, off, 64);
    if (lane >= off) x += up;
  }
  return x;
}

// A thread holds the counts c0 .. c3 of the four consecutive bins from bin0 and the number of keys before them (excl) and
// up to their end (incl).  Exactly one thread has excl <= want < incl (the total is > want); the last thread (`last`) also
// takes a rank beyond the total's reach.  That thread walks to the bin of rank `want` (bins end at last_bin) and records it:
// the key prefix with the bin at `shift`, the rank within the bin and the bin's count.
__device__ __forceinline__ void ps_pick_bin(long long want, long long excl, long long incl, bool last, int c0, int c1, int c2,
                                            int c3, int bin0, int last_bin, unsigned long long prefix, int shift,
                                            unsigned long long* sel_prefix, long long* sel_rank, int* sel_bin_count) {
  const bool mine = (excl <= want && want < incl) || (last && want >= incl);
  if (mine) {
    long long rr = want - excl;
    int bin = bin0, cb = c0;
    if (rr >= c0 && bin < last_bin) { rr -= c0; ++bin; cb = c1;
      if (rr >= c1 && bin < last_bin) { rr -= c1; ++bin; cb = c2;
        if (rr >= c2 && bin < last_bin) { rr -= c2; ++bin; cb = c3; } } }
    *sel_rank = rr;
    *sel_prefix = prefix | ((unsigned long long)bin << shift);
    *sel_bin_count = cb;
  }
}

// The bin of a 256-bin LDS histogram that holds rank *sel_rank, by ONE wave (all its lanes call): four consecutive bins per
// lane (a serial walk by one thread was 3.5 us of every pass)
__device__ __forceinline__ void ps_scan_hist256(const int* hist, unsigned long long prefix, int shift,
                                                unsigned long long* sel_prefix, long long* sel_rank, int* sel_bin_count) {
  const int lane = threadIdx.x & 63;
  const long long want = *sel_rank;
  const int c0 = hist[4 * lane], c1 = hist[4 * lane + 1], c2 = hist[4 * lane + 2], c3 = hist[4 * lane + 3];
  const long long mine4 = (long long)c0 + c1 + c2 + c3;
  const long long incl = ps_wave_prefix(mine4);
  ps_pick_bin(want, incl - mine4, incl, lane == 63, c0, c1, c2, c3, 4 * lane, 255, prefix, shift, sel_prefix, sel_rank,
              sel_bin_count);
}

// The nb keys bk[] of the selected bin, one per thread, counted against each other: the key of rank *sel_rank among them is
// the wanted one (every thread that holds it writes the same value).  No barrier inside: one before (bk, *sel_rank) and one
// after (*sel_prefix) are the caller's.
__device__ __forceinline__ void ps_rank_among(const unsigned long long* bk, int nb, unsigned long long* sel_prefix,
                                              const long long* sel_rank) {
  const int t = threadIdx.x;
  const long long want = *sel_rank;
  if (t < nb) {
    const unsigned long long mk = bk[t];
    int lt = 0, le = 0;
    for (int j = 0; j < nb; ++j) {
      const unsigned long long o = bk[j];
      lt += o < mk ? 1 : 0;
      le += o <= mk ? 1 : 0;
    }
    if (lt <= want && want < le) *sel_prefix = mk;
  }
}

// one value on the way to ps_rank_among: a key that agrees with prefix under mask takes the next place of bk (*count counts
// them all, CAP are kept)
template <int CAP>
__device__ __forceinline__ void ps_bin_put(double v, unsigned long long prefix, unsigned long long mask, unsigned long long* bk,
                                           int* count) {
  const unsigned long long k = ps_key(v);
  if ((k & mask) == prefix) {
    const int p = atomicAdd(count, 1);
    if (p < CAP) bk[p] = k;
  }
}

// ---- the tail -------------------------------------------------------------------------------------------------------
// the cut-off of the selected key, not below log(DBL_MIN) (:159); *expxc = exp(cut-off)
__device__ __forceinline__ double ps_cutoff(unsigned long long key, double* expxc) {
  const double cutoffmin = log(DBL_MIN);
  const double xcutoff = fmax(ps_unkey(key), cutoffmin);
  *expxc = exp(xcutoff);
  return xcutoff;
}

// right tail (:175-177), one value: above the cut-off it takes the next place of tv / ti with its index, in the order the
// atomics fall (*count counts them all, CAP are kept)
template <int CAP>
__device__ __forceinline__ void ps_tail_put(int i, double v, double xcutoff, double* tv, int* ti, int* count) {
  if (v > xcutoff) {
    const int p = atomicAdd(count, 1);
    if (p < CAP) {
      tv[p] = v;
      ti[p] = i;
    }
  }
}

// (value, index) lexicographic "a after b"
__device__ __forceinline__ bool ps_after(double av, int ai, double bv, int bi) {
  return (av > bv) | ((av == bv) & (ai > bi));      // no short circuit: a branch per comparison cost 25 us per call
}

// ---- gpdfitnew (:266-325) -------------------------------------------------------------------------------------------
// x2 = exp(x2) - exp(xcutoff)   (:185-186).  Barrier inside.
template <int THREADS>
__device__ __forceinline__ void ps_tail_exp(double* tv, int n2, double expxc) {
  for (int i = threadIdx.x; i < n2; i += THREADS) tv[i] = exp(tv[i]) - expxc;
  __syncthreads();
}

// the m = 30 + int(sqrt(n2)) quadrature points q_bs of the sorted, shifted tail tv (PRIOR = 3); returns m.  Barrier inside.
__device__ __forceinline__ int ps_quad_points(const double* tv, int n2, double* q_bs) {
  const int t = threadIdx.x;
  const int m = 30 + (int)sqrt((double)n2);
  const double xq = tv[(int)(n2 / 4.0 + 0.5) - 1], xl = tv[n2 - 1];
  if (t < m) q_bs[t] = (1.0 - sqrt((double)m / ((double)(t + 1) - 0.5))) / (3.0 * xq) + 1.0 / xl;
  __syncthreads();
  return m;
}

// q_L[j] = n2 (log(-bs_j / ks_j) - ks_j - 1) with ks_j = mean log1p(-bs_j x).  Sixteen lanes per quadrature point
// (THREADS / 16 points at a time), each a fixed stride of the tail, combined by a fixed butterfly -- the m n2 logarithms
// spread over the whole workgroup instead of one wave per point.  Barrier inside.
template <int THREADS>
__device__ __forceinline__ void ps_quad_ks(const double* tv, int n2, int m, const double* q_bs, double* q_L) {
  const int grp = threadIdx.x >> 4, gl = threadIdx.x & 15;
  for (int j = grp; j < m; j += THREADS / 16) {
    const double nb = -q_bs[j];
    double s = 0.0;
    // log(1 + y) for log1p(y): the ABSOLUTE error of a term is what the mean sees, and that is one rounding of 1 + y
    // (<= 1.1e-16) either way; log costs half of what log1p does, and these m n2 evaluations are the phase's time
    // four logarithms in flight per lane (independent chains: the evaluation is latency-bound), added in the same order
    int i = gl;
    for (; i + 48 < n2; i += 64) {
      const double l0 = log(fma(nb, tv[i], 1.0)), l1 = log(fma(nb, tv[i + 16], 1.0)), l2 = log(fma(nb, tv[i + 32], 1.0)),
                   l3 = log(fma(nb, tv[i + 48], 1.0));
      s += l0;
      s += l1;
      s += l2;
      s += l3;
    }
    for (; i < n2; i += 16) s += log(fma(nb, tv[i], 1.0));
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (gl == 0) {
      const double ks = s / n2;
      q_L[j] = n2 * (log(-(q_bs[j] / ks)) - ks - 1.0);
    }
  }
  __syncthreads();
}

// From the m profile log-likelihoods q_L (visible to the workgroup: a barrier before is the caller's): the posterior weights
// q_w, the posterior mean of b (thread 0, serially, through bc[0]), k = mean log1p(-b x) with the weakly informative prior
// a = 10, *sigma = -k / b before the prior.  Returns k.  sh: ps_block_sum's.  Barriers inside.
template <int THREADS>
__device__ __forceinline__ double ps_gpd_fit(const double* tv, int n2, int m, const double* q_bs, const double* q_L,
                                             double* q_w, double* bc, double* sh, double* sigma) {
  const int t = threadIdx.x, grp = t >> 4, gl = t & 15;
  for (int j = grp; j < m; j += THREADS / 16) {
    const double lj = q_L[j];
    double s = 0.0;
    for (int i = gl; i < m; i += 16) s += exp(q_L[i] - lj);
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (gl == 0) {
      const double w = 1.0 / s;
      q_w[j] = w >= 10.0 * DBL_EPSILON ? w : 0.0;              // remove negligible weights
    }
  }
  __syncthreads();
  if (t == 0) {
    double ws = 0.0, bsum = 0.0;
    for (int i = 0; i < m; ++i) ws += q_w[i];
    for (int i = 0; i < m; ++i) bsum += q_bs[i] * (q_w[i] / ws);
    bc[0] = bsum;                                              // posterior mean of b
  }
  __syncthreads();
  const double b = bc[0];
  double s = 0.0;
  for (int i = t; i < n2; i += THREADS) s += log1p(-b * tv[i]);
  s = ps_block_sum<THREADS / 64>(s, sh);
  const double k = s / n2;
  *sigma = -k / b;
  return k * n2 / (n2 + 10.0) + 10.0 * 0.5 / (n2 + 10.0);      // weakly informative prior, a = 10
}

// smoothed tail (:188-199): the order statistic i of n2 of the fitted GPD (NaN for sigma <= 0) above the cut-off, as a log
// weight truncated at the largest raw weight (0 after the shift)
__device__ __forceinline__ double ps_quantile(int i, int n2, double k, double sigma, double expxc) {
  const double p = ((double)i + 0.5) / n2;
  double qq = NAN;
  if (sigma > 0.0) {
    const double l = log1p(-p);
    qq = (fabs(k) < DBL_EPSILON ? -l : expm1(-k * l) / k) * sigma;
  }
  double v = log(qq + expxc);
  if (v > 0.0) v = 0.0;
  return v;
}

}  // namespace vb
