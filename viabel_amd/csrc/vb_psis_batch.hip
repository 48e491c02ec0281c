// Batched Pareto smoothing and PSIS leave-one-out on the device.
// Reference: viabel/_psis.py:69-110 (psisloo), :113-209 (psislw with a 2-D argument: one weight vector per column).
//
// psis_batch_kernel smooths m independent vectors of S log weights in ONE launch, one 256-thread workgroup per vector
// (vb_psis.hip's kernels are sized for one long vector: 1024 threads, ~115 KB of LDS, one launch per vector).  Per vector
// it does what psis_kernel does, in the same order: max shift, exact selection of the cut-off (the (M+1)-th largest,
// M = ceil(min(0.2 S, 3 sqrt(S / Reff)))) by a byte-wise radix select on order-preserving keys, tail gathered and ordered
// by (value, index), Zhang-Stephens fit with 30 + floor(sqrt(n_tail)) points, quantile replacement when k >= 1/3,
// truncation at 0, log-sum-exp normalisation; k = inf when the tail has at most 4 values.  The steps themselves are
// vb_psis_util.h's, the ones vb_psis.hip's kernels run; this file holds the kernel's register passes and its closing sums.
//   * capacity: S <= 16 384 (VPT = 4, 16 or 64 values per thread, held in registers from the load to the end: the
//     loads of a vector are contiguous and all issued before the first use) and a tail of at most 1024 values
//     (384 at S = 16 384, Reff = 1; 62 quadrature points at most).  Longer vectors / tails keep the column loop.
//   * the smoothed tail is NOT scattered back into the registers: it stays in LDS in sorted order with its element
//     indices, and the closing sums take the untouched elements from registers and the tail from that list.
//   * integer atomics on LDS only (histogram, gather counter); ties are ordered by index, every floating-point sum has a
//     fixed order: results are bit-reproducible run to run and do not depend on the gather order.
//   * mode "smooth": the vector is A[j], smoothed in place.  Mode "loo": the vector is log_ratios - A[j] (- A[j]
//     without ratios), nothing is written back; loo[j] = logsumexp_s(smoothed_s + A[j][s]) and, with the full-data
//     weights log_w, lpd[j] = logsumexp_s(log_w[s] + A[j][s]) leave instead: three doubles per vector.
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; scratch 0 in all three variants;
// LDS 14 920 B per workgroup: ten workgroups' worth in a CU's 160 KiB, so LDS never bounds the occupancy):
//     VPT  4 (S <= 1024):    90 VGPRs -> 5 workgroups per CU
//     VPT 16 (S <= 4096):   117 VGPRs -> 4 workgroups per CU
//     VPT 64 (S <= 16 384): 256 VGPRs + 88 AGPRs -> 1 workgroup per CU (the vector alone is 128 registers; a fully
//                           unrolled pass over it, its exponentials inlined, keeps the rest busy)
//   Registers bound the occupancy everywhere.
//
// Pointwise log-likelihoods of the regression targets: LL[i][s] = log p(y_i | x_i' theta_s) as a normalised density is
// one fp64 MFMA product X (n_data x D) times the TRANSPOSED draws (D x S) with a per-element epilogue (EpiPointwise).
// That orientation -- not Z X' written transposed from the epilogue -- because the result must be observation-major
// (n_data rows of S contiguous doubles: the smoothing kernel reads one observation's S values as a unit) and the GEMM's
// result lanes hold adjacent COLUMNS: with draws as columns a lane pair stores 16 contiguous bytes and a quad 64,
// whereas the transposed store would put every lane of a row on its own line, S doubles apart.  The transpose of the
// draws is S x D doubles, negligible next to the n_data x S result.
//
// Posterior prediction (vb_glm_predict): the same product with a plain store (EpiStorePlain), against the bound design or an
// uploaded one (chunks of observations, padded like the bound X), followed by glm_predict_kernel: one 256-thread workgroup
// per observation streams its S linear predictors twice -- weighted means and the log-sum-exp of the predictive density,
// then the weighted squared deviations from those means -- and writes five doubles.  The weights are normalised once per
// call on the host (S values); the m x S matrix is written once and read twice on the device and nothing of that order
// crosses the bus.  No sort, so no cap on S.  Resources (as above; scratch 0 in all three; LDS 32 B per workgroup):
//     Bernoulli-logit: 105 VGPRs -> 4 workgroups per CU
//     Poisson:          82 VGPRs -> 5 workgroups per CU
//     Gaussian:         74 VGPRs -> 6 workgroups per CU
#include "vb_rows_target.h"
#include "vb_psis_util.h"

#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <vector>

namespace vb {

constexpr int kPbThreads = 256;
constexpr int kPbWaves = kPbThreads / 64;
constexpr int kPbTailCap = 1024;       // tail values sorted in LDS
constexpr int kPbQuadCap = 64;         // 30 + sqrt(1024) = 62 quadrature points at most
constexpr int kPbMaxVpt = 64;
constexpr int64_t kPbMaxN = (int64_t)kPbMaxVpt * kPbThreads;      // 16 384
// device memory a call may hold for the n_data x S likelihood matrix (or the vectors of vb_psis_smooth_batch): larger
// problems go through in chunks of observations
constexpr size_t kLooBudgetBytes = (size_t)1 << 30;
constexpr int64_t kLooBudgetDoubles = (int64_t)(kLooBudgetBytes / sizeof(double));

struct PsisBatchArgs {
  double* A;                  // m vectors of n doubles, vector j at A + j * ld
  int64_t ld;
  int n, m_tail;
  int loo;                    // 0: smooth A[j] in place; 1: smooth log_ratios - A[j], write loo / lpd
  const double* log_ratios;   // [n] or nullptr (loo)
  const double* log_w;        // [n] or nullptr (loo): full-data smoothed log weights
  double* khat;               // [m]
  double* loo_out;            // [m] (loo)
  double* lpd_out;            // [m] (loo, with log_w)
};

// running log-sum-exp of one thread: sum = s * exp(m)
struct PbLse {
  double m = -INFINITY, s = 0.0;
  template <int C>
  __device__ __forceinline__ void add(const double (&t)[C]) {      // C terms at the cost of C + 1 exponentials
    double cm = t[0];
#pragma unroll
    for (int q = 1; q < C; ++q) cm = fmax(cm, t[q]);
    const double mn = fmax(m, cm);
    s *= (m == mn) ? 1.0 : exp(m - mn);
#pragma unroll
    for (int q = 0; q < C; ++q) s += (t[q] == -INFINITY) ? 0.0 : exp(t[q] - mn);      // (a term of -inf adds nothing)
    m = mn;
  }
  __device__ __forceinline__ double total(double* sh) const {      // over the workgroup, in a fixed order
    const double M = ps_block_max<kPbWaves>(m, sh);
    const double part = (m == -INFINITY) ? 0.0 : s * exp(m - M);
    return log(ps_block_sum<kPbWaves>(part, sh)) + M;
  }
};

template <int VPT>
__global__ void __launch_bounds__(kPbThreads) psis_batch_kernel(const PsisBatchArgs a) {
  __shared__ double sh[kPbWaves];
  __shared__ int hist[256];
  __shared__ unsigned long long sel_prefix;
  __shared__ long long sel_rank;
  __shared__ int sel_bin_count;
  __shared__ int tail_count;
  __shared__ double tv[kPbTailCap];
  __shared__ int ti[kPbTailCap];
  __shared__ double q_bs[kPbQuadCap], q_L[kPbQuadCap], q_w[kPbQuadCap];
  __shared__ double bc[2];
  const int t = threadIdx.x, wave = t >> 6;
  const int n = a.n;
  double* __restrict__ row = a.A + (int64_t)blockIdx.x * a.ld;

  // the vector: element t + 256 u in r[u] (coalesced; up to sixteen loads per thread -- and as many of the ratios -- are
  // issued before the first value is used).  The slots beyond n hold -inf: the smallest key, never above a cut-off, zero in
  // every sum of exponentials -- the passes over the registers need no bounds predicate (64 of them held in scalar
  // registers cost the VPT = 64 variant its second workgroup per CU); the wanted rank counts them in.
  double r[VPT];
  constexpr int LB = VPT < 16 ? VPT : 16;
#pragma unroll
  for (int u0 = 0; u0 < VPT; u0 += LB) {
    double lr[LB];
#pragma unroll
    for (int q = 0; q < LB; ++q) {
      const int i = t + (u0 + q) * kPbThreads;
      r[u0 + q] = row[i < n ? i : n - 1];      // (clamped, not branched over: the slot is overwritten below)
    }
    if (a.loo) {
#pragma unroll
      for (int q = 0; q < LB; ++q) {
        const int i = t + (u0 + q) * kPbThreads;
        lr[q] = a.log_ratios ? a.log_ratios[i < n ? i : n - 1] : 0.0;
      }
#pragma unroll
      for (int q = 0; q < LB; ++q) r[u0 + q] = a.log_ratios ? lr[q] - r[u0 + q] : -r[u0 + q];
    }
#pragma unroll
    for (int q = 0; q < LB; ++q)
      if (t + (u0 + q) * kPbThreads >= n) r[u0 + q] = -INFINITY;
  }
  // (every pass over the registers forms its element indices from an opaque copy of the thread index: left to itself the
  // compiler keeps the VPT indices and byte offsets of the first pass alive to the last -- 150 registers at VPT = 64)
  auto each = [&](auto&& f) __attribute__((always_inline)) {
    int tt = t;
    asm volatile("" : "+v"(tt));
#pragma unroll
    for (int u = 0; u < VPT; ++u) {
      f(tt + u * kPbThreads, r[u]);
    }
  };

  // 1. improve numerical accuracy: x -= max(x)   (_psis.py:166)
  double mx = -INFINITY;
  each([&](int, double v) { mx = fmax(mx, v); });
  mx = ps_block_max<kPbWaves>(mx, sh);
#pragma unroll
  for (int u = 0; u < VPT; ++u) r[u] -= mx;

  // 2. x_sorted[n - m_tail - 1] by radix select (8 bits per pass, most significant first)   (:170-173)
  if (t == 0) {
    sel_prefix = 0ull;
    sel_rank = (long long)VPT * kPbThreads - a.m_tail - 1;     // 0-based ascending rank, the -inf pads included
  }
  int pass_done = -1;
  for (int pass = 7; pass >= 0; --pass) {
    hist[t] = 0;
    __syncthreads();
    const unsigned long long prefix = sel_prefix;
    const unsigned long long mask = pass == 7 ? 0ull : (~0ull << (8 * (pass + 1)));
#pragma unroll
    for (int u = 0; u < VPT; ++u) {
      const unsigned long long k = ps_key(r[u]);
      ps_hist_add(hist, (int)((k >> (8 * pass)) & 255ull), (k & mask) == prefix);
    }
    __syncthreads();
    if (wave == 0) ps_scan_hist256(hist, prefix, 8 * pass, &sel_prefix, &sel_rank, &sel_bin_count);
    __syncthreads();
    pass_done = pass;
    if (pass > 0 && sel_bin_count <= kPbThreads) break;      // (uniform: a shared value read behind the barrier)
  }
  if (pass_done > 0) {
    // the members of the selected bin, one per thread, counted against each other
    unsigned long long* bk = reinterpret_cast<unsigned long long*>(tv);
    if (t == 0) tail_count = 0;
    __syncthreads();
    const unsigned long long prefix = sel_prefix, mask = ~0ull << (8 * pass_done);
    each([&](int, double v) { ps_bin_put<kPbThreads>(v, prefix, mask, bk, &tail_count); });
    __syncthreads();
    ps_rank_among(bk, tail_count < kPbThreads ? tail_count : kPbThreads, &sel_prefix, &sel_rank);
    __syncthreads();
  }
  double expxc;
  const double xcutoff = ps_cutoff(sel_prefix, &expxc);

  // 3. right tail: x > xcutoff   (:175-177)
  __syncthreads();
  if (t == 0) tail_count = 0;
  __syncthreads();
  each([&](int i, double v) { ps_tail_put<kPbTailCap>(i, v, xcutoff, tv, ti, &tail_count); });
  __syncthreads();
  const int n2 = tail_count < kPbTailCap ? tail_count : kPbTailCap;
  double k = INFINITY, sigma = NAN;
  bool replaced = false;
  if (n2 > 4) {                                                 // :178-180
    // 4. order of the tail by (value, index): every element counts the elements before it and moves to that position
    // (psis_kernel's generic branch, spelled out in both: see there)
    constexpr int kPer = kPbTailCap / kPbThreads;
    double my_v[kPer];
    int my_i[kPer], my_r[kPer];
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int e = t + u * kPbThreads;
      my_v[u] = e < n2 ? tv[e] : INFINITY;
      my_i[u] = e < n2 ? ti[e] : 0x7fffffff;
      my_r[u] = 0;
    }
    for (int j0 = 0; j0 < n2; j0 += 8) {      // eight comparands read before the first comparison; beyond n2 a sentinel
      double v8[8];
      int i8[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int jx = j0 + q;
        const int jc = jx < n2 ? jx : n2 - 1;
        const double vv = tv[jc];
        const int ii = ti[jc];
        v8[q] = jx < n2 ? vv : INFINITY;
        i8[q] = jx < n2 ? ii : 0x7fffffff;
      }
#pragma unroll
      for (int q = 0; q < 8; ++q)
#pragma unroll
        for (int u = 0; u < kPer; ++u)
          if (u * kPbThreads < n2) my_r[u] += ps_after(my_v[u], my_i[u], v8[q], i8[q]) ? 1 : 0;     // (uniform condition)
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      if (t + u * kPbThreads < n2) {
        tv[my_r[u]] = my_v[u];
        ti[my_r[u]] = my_i[u];
      }
    }
    __syncthreads();
    ps_tail_exp<kPbThreads>(tv, n2, expxc);      // x2 = exp(x2) - exp(xcutoff)   (:185-186)

    // 5. gpdfitnew (:266-325), in psis_kernel's order of additions
    const int m = ps_quad_points(tv, n2, q_bs);
    ps_quad_ks<kPbThreads>(tv, n2, m, q_bs, q_L);
    k = ps_gpd_fit<kPbThreads>(tv, n2, m, q_bs, q_L, q_w, bc, sh, &sigma);

    // 6. smoothed tail (:188-199): order statistics of the fitted GPD, truncated at the largest raw weight; left in
    // tv (sorted order) beside the element indices ti
    replaced = k >= 1.0 / 3.0 && !isinf(k);
    if (replaced) {
      __syncthreads();
      for (int i = t; i < n2; i += kPbThreads) tv[i] = ps_quantile(i, n2, k, sigma, expxc);
    }
  }
  __syncthreads();

  // 7. renormalise: x -= sumlogs(x)   (:201, :380-396); the replaced elements (x > xcutoff) come from the list
  double m2 = -INFINITY;
  each([&](int, double v) {
    if (!(replaced && v > xcutoff)) m2 = fmax(m2, v);
  });
  if (replaced)
    for (int i = t; i < n2; i += kPbThreads) m2 = fmax(m2, tv[i]);
  m2 = ps_block_max<kPbWaves>(m2, sh);
  double se = 0.0;
  each([&](int, double v) {
    if (!(replaced && v > xcutoff)) se += exp(v - m2);
  });
  if (replaced)
    for (int i = t; i < n2; i += kPbThreads) se += exp(tv[i] - m2);
  se = ps_block_sum<kPbWaves>(se, sh);
  const double lse = log(se) + m2;
  if (t == 0) a.khat[blockIdx.x] = k;

  if (!a.loo) {
    each([&](int i, double v) {
      if (i < n && !(replaced && v > xcutoff)) row[i] = v - lse;
    });
    if (replaced)
      for (int i = t; i < n2; i += kPbThreads) row[ti[i]] = tv[i] - lse;
    return;
  }

  // 8. loo[j] = logsumexp_s(smoothed_s + A[j][s]), lpd[j] = logsumexp_s(log_w[s] + A[j][s]): the vector is read once
  // more (a workgroup's own 8 S bytes, just read), a chunk of loads before its first use
  constexpr int CH = 4;      // (eight: 12 more registers, and the VPT = 16 variant loses its fourth workgroup per CU)
  int tq = t;
  asm volatile("" : "+v"(tq));
  PbLse acc_loo, acc_lpd;
  const bool want_lpd = a.log_w != nullptr;
#pragma unroll
  for (int u0 = 0; u0 < VPT; u0 += CH) {
    double av[CH], wv[CH];
#pragma unroll
    for (int q = 0; q < CH; ++q) {
      const int i = tq + (u0 + q) * kPbThreads;
      av[q] = i < n ? row[i] : -INFINITY;      // (beyond n: both terms -inf)
      wv[q] = (want_lpd && i < n) ? a.log_w[i] : 0.0;
    }
    double tl[CH], tp[CH];
#pragma unroll
    for (int q = 0; q < CH; ++q) {
      const double v = r[u0 + q];
      tl[q] = !(replaced && v > xcutoff) ? (v - lse) + av[q] : -INFINITY;
      tp[q] = wv[q] + av[q];
    }
    acc_loo.add(tl);
    if (want_lpd) acc_lpd.add(tp);
  }
  if (replaced)
    for (int i = t; i < n2; i += kPbThreads) {
      const double tl[1] = {(tv[i] - lse) + row[ti[i]]};
      acc_loo.add(tl);
    }
  const double loo = acc_loo.total(sh);
  if (t == 0) a.loo_out[blockIdx.x] = loo;
  if (want_lpd) {
    const double lpd = acc_lpd.total(sh);
    if (t == 0) a.lpd_out[blockIdx.x] = lpd;
  }
}

static bool psis_batch_fits(int64_t n, double reff) {
  return n >= 2 && n <= kPbMaxN && reff > 0.0 && psis_tail_size(n, reff) <= kPbTailCap;
}

static int psis_batch_enqueue(vb_ctx* ctx, hipStream_t st, PsisBatchArgs a, int64_t m) {
  const dim3 grid((unsigned)m), block(kPbThreads);
  if (a.n <= 4 * kPbThreads) hipLaunchKernelGGL(psis_batch_kernel<4>, grid, block, 0, st, a);
  else if (a.n <= 16 * kPbThreads) hipLaunchKernelGGL(psis_batch_kernel<16>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(psis_batch_kernel<64>, grid, block, 0, st, a);
  VB_HIP(ctx, hipGetLastError());
  return VB_OK;
}

// ---- pointwise log-likelihoods of the regression targets -----------------------------------------------------------
// what glm_term leaves out of log p(y_i | eta): Bernoulli-logit nothing, Poisson -log(y_i !), Gaussian -log(s) - log(2 pi) / 2
__global__ void __launch_bounds__(256) glm_const_kernel(const double* __restrict__ y, int64_t n, int link, double aux,
                                                        double* __restrict__ cst) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  cst[i] = glm_obs_const(link, aux, y[i]);
}

struct EpiPointwise {        // LL[observation][draw] = log p(y_obs | eta): row = observation, col = draw
  double* LL;
  int64_t ld;
  const double* y;
  const double* cst;
  int link;
  double aux;
  __device__ __forceinline__ double term(int row, double eta) const {
    double dl;
    return glm_term(link, aux, y[row], eta, &dl) + cst[row];
  }
  __device__ void operator()(int, int row, int col, double eta) const { LL[(int64_t)row * ld + col] = term(row, eta); }
  __device__ d2v pair(int, int row, int col, double e0, double e1) const {
    const d2v v = (d2v){term(row, e0), term(row, e1)};
    *reinterpret_cast<d2v*>(LL + (int64_t)row * ld + col) = v;
    return v;
  }
};

// dst[c][r] = src[r][c] through a 32 x 33 LDS tile (both sides coalesced)
__global__ void __launch_bounds__(256) pb_transpose_kernel(const double* __restrict__ src, int64_t lds, int64_t rows,
                                                           int64_t cols, double* __restrict__ dst, int64_t ldd) {
  __shared__ double tile[32][33];
  const int64_t tiles_c = (cols + 31) / 32;
  const int64_t c0 = (blockIdx.x % tiles_c) * 32, r0 = (blockIdx.x / tiles_c) * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int64_t rr = r0 + ty + 8 * q, cc = c0 + tx;
    if (rr < rows && cc < cols) tile[ty + 8 * q][tx] = src[rr * lds + cc];
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int64_t cc = c0 + ty + 8 * q, rr = r0 + tx;
    if (rr < rows && cc < cols) dst[cc * ldd + rr] = tile[tx][ty + 8 * q];
  }
}

static int pb_transpose(vb_ctx* ctx, hipStream_t st, const double* src, int64_t lds, int64_t rows, int64_t cols, double* dst,
                        int64_t ldd) {
  const int64_t tiles = ((cols + 31) / 32) * ((rows + 31) / 32);
  if (tiles > 0x7fffffffll) return fail(ctx, VB_ERR_UNSUPPORTED, "matrix of %lld x %lld is too large to transpose in one launch",
                                        (long long)rows, (long long)cols);
  hipLaunchKernelGGL(pb_transpose_kernel, dim3((unsigned)tiles), dim3(256), 0, st, src, lds, rows, cols, dst, ldd);
  VB_HIP(ctx, hipGetLastError());
  return VB_OK;
}

static int glm_check(vb_ctx* ctx, int64_t s, int64_t d) {
  if (ctx->model.id < 0) return fail(ctx, VB_ERR_STATE, "no model bound (vb_set_model)");
  if (ctx->model.id != VB_MODEL_LOGISTIC)
    return fail(ctx, VB_ERR_UNSUPPORTED, "pointwise log-likelihoods exist for the regression targets only (model id %d has no "
                                         "per-observation structure)", ctx->model.id);
  if (d != ctx->model.dim)
    return fail(ctx, VB_ERR_INVALID, "x has %lld columns, model dimension is %d", (long long)d, ctx->model.dim);
  if (s <= 0 || s > 0x7fffffffll) return fail(ctx, VB_ERR_INVALID, "the number of draws must be positive");
  return VB_OK;
}

// Where the pieces of a pointwise / LOO call live in ctx->loo_work (doubles from the base)
struct GlmLayout {
  int64_t lds, ldx, ndp;                   // row strides: draws-as-columns (round_up(S, 16)), draws-as-rows, round_up(n_data, 16)
  int64_t o_x, o_xt, o_c, o_vec, o_res, o_ll, o_t, total;
  int64_t chunk;                           // observations per pass
};
static GlmLayout glm_layout(const ModelDev& m, int64_t s, int64_t d, bool with_transposed_out) {
  GlmLayout L;
  L.lds = round_up(s, 16), L.ldx = round_up(d, 16), L.ndp = round_up(m.n_data, 16);
  const int64_t budget = kLooBudgetDoubles / (with_transposed_out ? 2 : 1);
  int64_t chunk = budget / L.lds;
  chunk = chunk < 1 ? 1 : (chunk > m.n_data ? m.n_data : chunk);
  L.chunk = chunk;
  int64_t off = 0;
  auto carve = [&off](int64_t doubles) {
    const int64_t o = off;
    off += round_up(doubles, 16);
    return o;
  };
  L.o_x = carve(s * L.ldx), L.o_xt = carve(d * L.lds), L.o_c = carve(L.ndp), L.o_vec = carve(2 * L.lds),
  L.o_res = carve(3 * L.ndp), L.o_ll = carve(chunk * L.lds), L.o_t = carve(with_transposed_out ? s * chunk : 0);
  L.total = off;
  return L;
}

// draws up and transposed; the per-observation constants
// the draws (S x D, host) into X (row stride ldx) and transposed into Xt (D x lds, the padding zeroed)
static int glm_stage_draws(vb_ctx* ctx, hipStream_t st, double* X, int64_t ldx, double* Xt, int64_t lds, const double* x_host,
                           int64_t s, int64_t d) {
  VB_HIP(ctx, hipMemsetAsync(Xt, 0, (size_t)d * lds * sizeof(double), st));
  VB_HIP(ctx, hipMemcpy2DAsync(X, (size_t)ldx * sizeof(double), x_host, (size_t)d * sizeof(double), (size_t)d * sizeof(double),
                               (size_t)s, hipMemcpyHostToDevice, st));
  return pb_transpose(ctx, st, X, ldx, s, d, Xt, lds);
}

static int glm_stage(vb_ctx* ctx, hipStream_t st, const GlmLayout& L, const double* x_host, int64_t s, int64_t d) {
  const ModelDev& m = ctx->model;
  VB_TRY(ensure(ctx, ctx->loo_work, (size_t)L.total * sizeof(double)));
  double* base = (double*)ctx->loo_work.ptr;
  VB_TRY(glm_stage_draws(ctx, st, base + L.o_x, L.ldx, base + L.o_xt, L.lds, x_host, s, d));
  hipLaunchKernelGGL(glm_const_kernel, dim3((unsigned)((m.n_data + 255) / 256)), dim3(256), 0, st, m.p2, m.n_data, m.link, m.aux,
                     base + L.o_c);
  VB_HIP(ctx, hipGetLastError());
  return VB_OK;
}

// LL[0 .. rows) = pointwise log-likelihoods of the observations [r0, r0 + rows) at the staged draws
static int glm_pointwise_enqueue(vb_ctx* ctx, hipStream_t st, const GlmLayout& L, int64_t r0, int64_t rows, int64_t s, int64_t d) {
  const ModelDev& m = ctx->model;
  double* base = (double*)ctx->loo_work.ptr;
  GemmArgs g;                        // LL = X theta'   [rows x S x D]
  g.A = m.p0 + r0 * m.ldp, g.lda = m.ldp;
  g.B = base + L.o_xt, g.ldb = L.lds;
  g.M = (int)rows, g.N = (int)s, g.K = (int)d, g.tri_mode = 0;
  gemm_f64_launch<true>(st, g, 1, ctx->prop.multiProcessorCount,
                        EpiPointwise{base + L.o_ll, L.lds, m.p2 + r0, base + L.o_c + r0, m.link, m.aux});
  VB_HIP(ctx, hipGetLastError());
  return VB_OK;
}


// ---- posterior prediction of the regression targets (vb_glm_predict) ------------------------------------------------
// ETA[observation][draw] = x_obs' theta_draw: the product of glm_pointwise_enqueue with a plain store, against the bound
// design or a chunk of an uploaded one (EpiStorePlain)
// (PredictArgs: vb_common.h)

// One 256-thread workgroup per observation, two passes over its n linear predictors (8 n bytes the workgroup has just
// read: the second pass comes from the cache).  Pass 1: the weighted sums of eta, mu(eta), V(eta) and the running
// log-sum-exp of log w + log p(y | eta) (glm_predict_term: one exponential per element for all three).  Pass 2: the
// weighted squared deviations of eta and mu from those means -- never E[x^2] - E[x]^2.  Thread t takes the elements
// t + 256 k in order, the workgroup's sums are ps_block_sum's fixed tree: bit-reproducible.  An element of weight 0 adds
// nothing, whatever its value (the guard keeps 0 * inf out of the sums).
template <int LINK>
__global__ void __launch_bounds__(kPbThreads) glm_predict_kernel(const PredictArgs a) {
  __shared__ double sh[kPbWaves];
  constexpr int CH = 4;
  const int t = threadIdx.x;
  const int64_t n = a.n;
  const double* __restrict__ row = a.eta + (int64_t)blockIdx.x * a.ld;
  const bool has_y = a.y != nullptr;
  const double y = has_y ? a.y[blockIdx.x] : 0.0;

  double s_eta = 0.0, s_mu = 0.0, s_v = 0.0;
  PbLse lse;
  for (int64_t i0 = t; i0 < n; i0 += CH * kPbThreads) {
    double e[CH], w[CH], lw[CH], tl[CH];
#pragma unroll
    for (int q = 0; q < CH; ++q) {      // (clamped, not branched over: the loads of a round are issued together)
      const int64_t i = i0 + q * kPbThreads, ic = i < n ? i : n - 1;
      e[q] = row[ic];
      w[q] = a.w[ic];
      lw[q] = a.log_w[ic];
    }
#pragma unroll
    for (int q = 0; q < CH; ++q) {
      const bool live = i0 + q * kPbThreads < n && w[q] > 0.0;
      double mu, v;
      const double ll = glm_predict_term(LINK, a.aux, y, e[q], &mu, &v);
      s_eta += live ? w[q] * e[q] : 0.0;
      s_mu += live ? w[q] * mu : 0.0;
      s_v += live ? w[q] * v : 0.0;
      tl[q] = i0 + q * kPbThreads < n ? lw[q] + ll : -INFINITY;
    }
    if (has_y) lse.add(tl);
  }
  const double eta_mean = ps_block_sum<kPbWaves>(s_eta, sh);
  const double mean = ps_block_sum<kPbWaves>(s_mu, sh);
  const double within = ps_block_sum<kPbWaves>(s_v, sh);

  double d_eta = 0.0, d_mu = 0.0;
  for (int64_t i0 = t; i0 < n; i0 += CH * kPbThreads) {
    double e[CH], w[CH];
#pragma unroll
    for (int q = 0; q < CH; ++q) {
      const int64_t i = i0 + q * kPbThreads, ic = i < n ? i : n - 1;
      e[q] = row[ic];
      w[q] = a.w[ic];
    }
#pragma unroll
    for (int q = 0; q < CH; ++q) {
      const bool live = i0 + q * kPbThreads < n && w[q] > 0.0;
      double mu, v;
      glm_predict_term(LINK, a.aux, 0.0, e[q], &mu, &v);
      const double de = e[q] - eta_mean, dm = mu - mean;
      d_eta += live ? w[q] * (de * de) : 0.0;
      d_mu += live ? w[q] * (dm * dm) : 0.0;
    }
  }
  const double eta_var = ps_block_sum<kPbWaves>(d_eta, sh);
  const double between = ps_block_sum<kPbWaves>(d_mu, sh);
  if (t == 0) {
    a.eta_mean[blockIdx.x] = eta_mean;
    a.eta_var[blockIdx.x] = eta_var;
    a.mean[blockIdx.x] = mean;
    a.var[blockIdx.x] = within + between;
  }
  if (has_y) {      // what glm_term leaves out of log p(y | eta) does not depend on the draw: added to the log-sum-exp
    const double total = lse.total(sh);
    if (t == 0) {
      double c = 0.0;
      if (LINK == VB_GLM_POISSON) c = -lgamma(y + 1.0);
      else if (LINK == VB_GLM_GAUSSIAN) c = -log(a.aux) - 0.91893853320467274178;
      a.lpd[blockIdx.x] = total + c;
    }
  }
}

int glm_predict_enqueue(vb_ctx* ctx, hipStream_t st, int link, const PredictArgs& a, int64_t rows) {
  const dim3 grid((unsigned)rows), block(kPbThreads);
  if (link == VB_GLM_POISSON) hipLaunchKernelGGL(glm_predict_kernel<VB_GLM_POISSON>, grid, block, 0, st, a);
  else if (link == VB_GLM_GAUSSIAN) hipLaunchKernelGGL(glm_predict_kernel<VB_GLM_GAUSSIAN>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(glm_predict_kernel<VB_GLM_BERNOULLI_LOGIT>, grid, block, 0, st, a);
  VB_HIP(ctx, hipGetLastError());
  return VB_OK;
}

// Where the pieces of a prediction live in ctx->loo_work (doubles from the base); the chunk of observations is the one of
// the LOO layout: what fits kLooBudgetBytes at round_up(S, 16) doubles per observation
struct PredictLayout {
  int64_t lds, ldx, mp;                    // row strides: draws-as-columns, draws-as-rows / design rows; round_up(m, 16)
  int64_t o_x, o_xt, o_w, o_xn, o_y, o_res, o_eta, total;
  int64_t chunk;
};
static PredictLayout predict_layout(int64_t s, int64_t d, int64_t m, bool own_design) {
  PredictLayout L;
  L.lds = round_up(s, 16), L.ldx = round_up(d, 16), L.mp = round_up(m, 16);
  int64_t chunk = kLooBudgetDoubles / L.lds;
  chunk = chunk < 1 ? 1 : (chunk > m ? m : chunk);
  L.chunk = chunk;
  int64_t off = 0;
  auto carve = [&off](int64_t doubles) {
    const int64_t o = off;
    off += round_up(doubles, 16);
    return o;
  };
  L.o_x = carve(s * L.ldx), L.o_xt = carve(d * L.lds), L.o_w = carve(2 * L.lds), L.o_xn = carve(own_design ? chunk * L.ldx : 0),
  L.o_y = carve(L.mp), L.o_res = carve(5 * L.mp), L.o_eta = carve(chunk * L.lds);
  L.total = off;
  return L;
}

// (contract: vb_common.h)
bool predict_weights(const double* log_w, int64_t s, std::vector<double>& out) {
  out.resize((size_t)(2 * s));
  double *w = out.data(), *lw = w + s;
  if (!log_w) {
    const double u = 1.0 / (double)s, lu = -log((double)s);
    for (int64_t i = 0; i < s; ++i) w[i] = u, lw[i] = lu;
    return true;
  }
  double mx = -INFINITY, sum = 0.0;
  for (int64_t i = 0; i < s; ++i) mx = log_w[i] > mx ? log_w[i] : mx;
  if (!std::isfinite(mx)) return false;
  for (int64_t i = 0; i < s; ++i) sum += exp(log_w[i] - mx);
  const double lse = mx + log(sum);
  if (!std::isfinite(lse)) return false;
  for (int64_t i = 0; i < s; ++i) {
    lw[i] = log_w[i] - lse;
    w[i] = exp(lw[i]);
  }
  return true;
}

}  // namespace vb

using namespace vb;

extern "C" {

int vb_psis_smooth_batch(vb_ctx* ctx, const double* lw, int64_t n, int64_t m, int64_t ld, double reff, double* out,
                         double* khat) {
  if (!ctx || !lw || !out || !khat) return fail(ctx, VB_ERR_INVALID, "NULL argument");
  if (n <= 1) return fail(ctx, VB_ERR_INVALID, "More than one log-weight needed.");
  if (m <= 0 || m > 0x7fffffffll) return fail(ctx, VB_ERR_INVALID, "the number of weight vectors must be positive");
  if (ld < n) return fail(ctx, VB_ERR_INVALID, "stride %lld is shorter than the vectors (%lld)", (long long)ld, (long long)n);
  if (!(reff > 0.0)) return fail(ctx, VB_ERR_INVALID, "Reff must be positive");
  if (!psis_batch_fits(n, reff))
    return fail(ctx, VB_ERR_UNSUPPORTED, "batched PSIS takes vectors of at most %lld weights with a tail of at most %d values (got "
                                         "%lld weights): smooth them one by one (vb_psis_smooth)",
                (long long)kPbMaxN, kPbTailCap, (long long)n);
  VB_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int64_t ldd = round_up(n, 16);
  int64_t chunk = kLooBudgetDoubles / ldd;
  chunk = chunk < 1 ? 1 : (chunk > m ? m : chunk);
  VB_TRY(ensure(ctx, ctx->loo_work, (size_t)(chunk * ldd + round_up(chunk, 16)) * sizeof(double)));
  double* A = (double*)ctx->loo_work.ptr;
  double* kd = A + chunk * ldd;
  for (int64_t j0 = 0; j0 < m; j0 += chunk) {
    const int64_t rows = m - j0 < chunk ? m - j0 : chunk;
    VB_HIP(ctx, hipMemcpy2DAsync(A, (size_t)ldd * sizeof(double), lw + j0 * ld, (size_t)ld * sizeof(double),
                                 (size_t)n * sizeof(double), (size_t)rows, hipMemcpyHostToDevice, st));
    PsisBatchArgs a{A, ldd, (int)n, psis_tail_size(n, reff), 0, nullptr, nullptr, kd, nullptr, nullptr};
    VB_TRY(psis_batch_enqueue(ctx, st, a, rows));
    VB_HIP(ctx, hipMemcpy2DAsync(out + j0 * ld, (size_t)ld * sizeof(double), A, (size_t)ldd * sizeof(double),
                                 (size_t)n * sizeof(double), (size_t)rows, hipMemcpyDeviceToHost, st));
    VB_HIP(ctx, hipMemcpyAsync(khat + j0, kd, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost, st));
    VB_HIP(ctx, hipStreamSynchronize(st));
  }
  return VB_OK;
}

int vb_glm_pointwise(vb_ctx* ctx, const double* x, int64_t s, int64_t d, double* ll_out) {
  if (!ctx || !x || !ll_out) return fail(ctx, VB_ERR_INVALID, "NULL argument");
  VB_TRY(glm_check(ctx, s, d));
  VB_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int64_t nd = ctx->model.n_data;
  const GlmLayout L = glm_layout(ctx->model, s, d, true);
  VB_TRY(glm_stage(ctx, st, L, x, s, d));
  double* base = (double*)ctx->loo_work.ptr;
  for (int64_t r0 = 0; r0 < nd; r0 += L.chunk) {      // chunk of observations -> (S x rows) -> columns [r0, r0 + rows) of the result
    const int64_t rows = nd - r0 < L.chunk ? nd - r0 : L.chunk;
    VB_TRY(glm_pointwise_enqueue(ctx, st, L, r0, rows, s, d));
    VB_TRY(pb_transpose(ctx, st, base + L.o_ll, L.lds, rows, s, base + L.o_t, rows));
    VB_HIP(ctx, hipMemcpy2DAsync(ll_out + r0, (size_t)nd * sizeof(double), base + L.o_t, (size_t)rows * sizeof(double),
                                 (size_t)rows * sizeof(double), (size_t)s, hipMemcpyDeviceToHost, st));
    VB_HIP(ctx, hipStreamSynchronize(st));
  }
  return VB_OK;
}

int vb_glm_psis_loo(vb_ctx* ctx, const double* x, int64_t s, int64_t d, const double* log_ratios, const double* log_w,
                    double reff, double* loo, double* khat, double* lpd) {
  if (!ctx || !x || !loo || !khat) return fail(ctx, VB_ERR_INVALID, "NULL argument");
  if ((log_w == nullptr) != (lpd == nullptr))
    return fail(ctx, VB_ERR_INVALID, "log_w and lpd go together (both or neither)");
  VB_TRY(glm_check(ctx, s, d));
  if (s <= 1) return fail(ctx, VB_ERR_INVALID, "More than one draw needed.");
  if (!(reff > 0.0)) return fail(ctx, VB_ERR_INVALID, "Reff must be positive");
  if (!psis_batch_fits(s, reff))
    return fail(ctx, VB_ERR_UNSUPPORTED, "PSIS-LOO on the device takes at most %lld draws with a tail of at most %d values (got %lld "
                                         "draws, tail %d)",
                (long long)kPbMaxN, kPbTailCap, (long long)s, psis_tail_size(s, reff));
  VB_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int64_t nd = ctx->model.n_data;
  const GlmLayout L = glm_layout(ctx->model, s, d, false);
  VB_TRY(glm_stage(ctx, st, L, x, s, d));
  double* base = (double*)ctx->loo_work.ptr;
  double *lr_d = base + L.o_vec, *lw_d = lr_d + L.lds, *res = base + L.o_res;
  if (log_ratios) VB_HIP(ctx, hipMemcpyAsync(lr_d, log_ratios, (size_t)s * sizeof(double), hipMemcpyHostToDevice, st));
  if (log_w) VB_HIP(ctx, hipMemcpyAsync(lw_d, log_w, (size_t)s * sizeof(double), hipMemcpyHostToDevice, st));
  for (int64_t r0 = 0; r0 < nd; r0 += L.chunk) {
    const int64_t rows = nd - r0 < L.chunk ? nd - r0 : L.chunk;
    VB_TRY(glm_pointwise_enqueue(ctx, st, L, r0, rows, s, d));
    PsisBatchArgs a{base + L.o_ll, L.lds, (int)s, psis_tail_size(s, reff), 1, log_ratios ? lr_d : nullptr,
                    log_w ? lw_d : nullptr, res + L.ndp + r0, res + r0, res + 2 * L.ndp + r0};
    VB_TRY(psis_batch_enqueue(ctx, st, a, rows));
  }
  VB_HIP(ctx, hipMemcpyAsync(loo, res, (size_t)nd * sizeof(double), hipMemcpyDeviceToHost, st));
  VB_HIP(ctx, hipMemcpyAsync(khat, res + L.ndp, (size_t)nd * sizeof(double), hipMemcpyDeviceToHost, st));
  if (lpd) VB_HIP(ctx, hipMemcpyAsync(lpd, res + 2 * L.ndp, (size_t)nd * sizeof(double), hipMemcpyDeviceToHost, st));
  VB_HIP(ctx, hipStreamSynchronize(st));
  return VB_OK;
}

int vb_glm_predict(vb_ctx* ctx, const double* x, int64_t s, int64_t d, const double* log_w, const double* x_new, int64_t m,
                   const double* y_new, double* mean, double* var, double* eta_mean, double* eta_var, double* lpd) {
  if (!ctx || !x || !mean || !var || !eta_mean || !eta_var) return fail(ctx, VB_ERR_INVALID, "NULL argument");
  VB_TRY(glm_check(ctx, s, d));
  const ModelDev& md = ctx->model;
  if (m <= 0 || m > 0x7fffffffll) return fail(ctx, VB_ERR_INVALID, "the number of observations to predict must be positive");
  if (!x_new && m != md.n_data)
    return fail(ctx, VB_ERR_INVALID, "without x_new the bound design is predicted: m = %lld, the model has %lld observations",
                (long long)m, (long long)md.n_data);
  if (x_new ? (y_new == nullptr) != (lpd == nullptr) : (y_new && !lpd))
    return fail(ctx, VB_ERR_INVALID, "y_new and lpd go together (both or neither)");
  if (y_new && md.link == VB_GLM_POISSON)
    for (int64_t i = 0; i < m; ++i)
      if (!(y_new[i] >= 0.0)) return fail(ctx, VB_ERR_INVALID, "Poisson counts must be non-negative");
  std::vector<double> wv;
  if (!predict_weights(log_w, s, wv)) return fail(ctx, VB_ERR_INVALID, "no log weight is finite (or one is NaN or +inf)");
  VB_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  struct Drain {      // the host buffers of the asynchronous uploads outlive them on every way out
    hipStream_t st;
    ~Drain() { (void)hipStreamSynchronize(st); }
  } drain{st};
  const PredictLayout L = predict_layout(s, d, m, x_new != nullptr);
  VB_TRY(ensure(ctx, ctx->loo_work, (size_t)L.total * sizeof(double)));
  double* base = (double*)ctx->loo_work.ptr;
  VB_TRY(glm_stage_draws(ctx, st, base + L.o_x, L.ldx, base + L.o_xt, L.lds, x, s, d));
  double *w_d = base + L.o_w, *lw_d = w_d + L.lds, *xn = base + L.o_xn, *res = base + L.o_res;
  VB_HIP(ctx, hipMemcpyAsync(w_d, wv.data(), (size_t)s * sizeof(double), hipMemcpyHostToDevice, st));
  VB_HIP(ctx, hipMemcpyAsync(lw_d, wv.data() + s, (size_t)s * sizeof(double), hipMemcpyHostToDevice, st));
  const double* y_d = x_new ? nullptr : md.p2;
  if (y_new) {
    VB_HIP(ctx, hipMemcpyAsync(base + L.o_y, y_new, (size_t)m * sizeof(double), hipMemcpyHostToDevice, st));
    y_d = base + L.o_y;
  }
  for (int64_t r0 = 0; r0 < m; r0 += L.chunk) {
    const int64_t rows = m - r0 < L.chunk ? m - r0 : L.chunk;
    GemmArgs g;                        // ETA = X_new theta'   [rows x S x D]
    if (x_new) {                       // the chunk of the design, padded like the bound one: row stride ldx, padding zeroed
      if (L.ldx != d) VB_HIP(ctx, hipMemsetAsync(xn, 0, (size_t)rows * L.ldx * sizeof(double), st));
      VB_HIP(ctx, hipMemcpy2DAsync(xn, (size_t)L.ldx * sizeof(double), x_new + r0 * d, (size_t)d * sizeof(double),
                                   (size_t)d * sizeof(double), (size_t)rows, hipMemcpyHostToDevice, st));
      g.A = xn, g.lda = L.ldx;
    } else {
      g.A = md.p0 + r0 * md.ldp, g.lda = md.ldp;
    }
    g.B = base + L.o_xt, g.ldb = L.lds;
    g.M = (int)rows, g.N = (int)s, g.K = (int)d, g.tri_mode = 0;
    gemm_f64_launch<true>(st, g, 1, ctx->prop.multiProcessorCount, EpiStorePlain{base + L.o_eta, L.lds});
    VB_HIP(ctx, hipGetLastError());
    const PredictArgs a{base + L.o_eta, L.lds, (int)s, w_d, lw_d, y_d ? y_d + r0 : nullptr, md.aux,
                        res + r0, res + L.mp + r0, res + 2 * L.mp + r0, res + 3 * L.mp + r0, res + 4 * L.mp + r0};
    VB_TRY(glm_predict_enqueue(ctx, st, md.link, a, rows));
  }
  double* outs[5] = {mean, var, eta_mean, eta_var, y_d ? lpd : nullptr};
  for (int k = 0; k < 5; ++k)
    if (outs[k]) VB_HIP(ctx, hipMemcpyAsync(outs[k], res + k * L.mp, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, st));
  VB_HIP(ctx, hipStreamSynchronize(st));
  return VB_OK;
}

}  // extern "C"
