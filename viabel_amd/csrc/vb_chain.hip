// Device-resident iterate chain and the Markov-chain statistics FASO / RAABBVI take of it (optimization.py:479-633 through
// _mc_diagnostics.py: split R-hat :124-184, effective sample size :40-99, Monte Carlo standard error :102-121).
//
// The chain is ctx->chain: chain_cap x chain_p doubles, row-major, rows [0, chain_rows) filled.  While it is open a device
// fit (FitRun, vb_fit_run.h) stores iterate k straight into row chain_rows + k -- the store the optimiser step does anyway
// for its history -- so the iterates never cross the bus; the statistics below read them where they lie.
//
// Every statistic treats a parameter's column as one chain and puts COLUMNS ON LANES: a wave reads 64 consecutive doubles
// of one row, a coalesced 512-byte segment, and walks down the rows.  Nothing here uses floating-point atomics: partial
// results go to ctx->chain_work and are merged in a fixed order, so that two calls give the same bits.
//
//   chain_rhat_partial_kernel   (count, mean, M2) of one half of one trailing window, per column: 16 rows at a time are
//                               summed and centred in registers (two passes over registers, one over memory) and the
//                               chunk is Chan-merged into the running triple; the four waves of a workgroup take a quarter of
//                               the rows each and merge through LDS in wave order, gridDim.z row splits (small p) go to
//                               chain_work.  Converged iterates have |mean| / sd of 1e2 ... 1e3: no sum of squares of the
//                               raw values is ever formed.
//   chain_rhat_final_kernel     merges the row splits in order, forms R-hat per column, reduces the maximum per workgroup
//   chain_rhat_max_kernel       reduces the workgroups' maxima; a NaN anywhere gives NaN, as np.max does
//   chain_ess_kernel            one wave per 64 columns.  Geyer's rule only looks at the autocorrelations up to the first
//                               non-positive pair sum, so the centred lag products are formed directly, kLagBlock lags per
//                               stream over the column: the last kLagBlock centred values sit in a register window that is
//                               indexed at compile time only (the stream is unrolled kLagBlock-fold, which turns the
//                               window's rotation into a renaming), kLagBlock FMAs per loaded value.  After each block every
//                               lane advances _chain_stats.ess's pair loop over the new lags; the wave stops when all of its
//                               lanes have found their stopping pair (wave vote).
#include "vb_common.h"

#include <cmath>
#include <limits>

namespace vb {

namespace {

constexpr int kMaxWindows = 16;
constexpr int kRhatChunk = 16;
constexpr int kLagBlock = 16;

struct Moments {
  int64_t n;
  double mean, m2;
};

// Chan et al.: the moments of the union of two samples
__device__ __forceinline__ void chan_merge(Moments& a, int64_t nb, double mean_b, double m2_b) {
  if (nb == 0) return;
  if (a.n == 0) {
    a.n = nb, a.mean = mean_b, a.m2 = m2_b;
    return;
  }
  const double na = (double)a.n, nbd = (double)nb, nn = na + nbd;
  const double delta = mean_b - a.mean;
  a.mean += delta * (nbd / nn);
  a.m2 += m2_b + delta * delta * (na * nbd / nn);
  a.n += nb;
}

struct RhatArgs {
  const double* chain;      // row 0 of the chain
  int64_t rows, p;
  int n_windows, n_split;
  int64_t w[kMaxWindows];
  double jitter;
  double* part;             // [(window, half)][split][mean | M2][p]
  double* rhat;             // n_windows x p, or nullptr
  double* block_max;        // n_windows x gridDim.x of the final kernel
  double* max_out;          // n_windows
};

__device__ __forceinline__ int64_t seg_bound(int64_t half, int64_t seg, int64_t n_seg) { return half * seg / n_seg; }

__global__ void __launch_bounds__(256) chain_rhat_partial_kernel(RhatArgs a) {
  __shared__ double sm[4][2][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t j = (int64_t)blockIdx.x * 64 + lane;
  const int64_t jj = j < a.p ? j : a.p - 1;
  const int wh = blockIdx.y, win = wh >> 1, h = wh & 1, z = blockIdx.z;
  const int64_t w = a.w[win], half = (w - (w & 1)) / 2;
  const int64_t n_seg = 4 * (int64_t)a.n_split, seg = 4 * (int64_t)z + wave;
  const int64_t r0 = seg_bound(half, seg, n_seg), r1 = seg_bound(half, seg + 1, n_seg);
  const double* col = a.chain + (a.rows - w + h * half) * a.p + jj;
  Moments m{0, 0.0, 0.0};
  for (int64_t r = r0; r < r1; r += kRhatChunk) {
    const int cnt = r1 - r < kRhatChunk ? (int)(r1 - r) : kRhatChunk;
    double v[kRhatChunk];
#pragma unroll
    for (int u = 0; u < kRhatChunk; ++u) v[u] = col[(r + (u < cnt ? u : cnt - 1)) * a.p];
    double s = 0.0;
#pragma unroll
    for (int u = 0; u < kRhatChunk; ++u)
      if (u < cnt) s += v[u];
    const double mc = s / (double)cnt;
    double q = 0.0;
#pragma unroll
    for (int u = 0; u < kRhatChunk; ++u)
      if (u < cnt) {
        const double d = v[u] - mc;
        q = fma(d, d, q);
      }
    chan_merge(m, cnt, mc, q);
  }
  sm[wave][0][lane] = m.mean;
  sm[wave][1][lane] = m.m2;
  __syncthreads();
  if (wave != 0 || j >= a.p) return;
  Moments t{0, 0.0, 0.0};
#pragma unroll
  for (int q = 0; q < 4; ++q)      // the four quarters, in row order
    chan_merge(t, seg_bound(half, 4 * (int64_t)z + q + 1, n_seg) - seg_bound(half, 4 * (int64_t)z + q, n_seg), sm[q][0][lane],
               sm[q][1][lane]);
  double* out = a.part + ((int64_t)wh * a.n_split + z) * 2 * a.p;
  out[j] = t.mean;
  out[a.p + j] = t.m2;
}

// max over a workgroup of 256 with np.max's NaN rule; the result is valid in thread 0
__device__ __forceinline__ double block_nanmax(double v, double (*sm)[4]) {
  int bad = v != v;
  double x = bad ? -std::numeric_limits<double>::infinity() : v;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double y = __shfl_xor(x, o, 64);
    bad |= __shfl_xor(bad, o, 64);
    x = y > x ? y : x;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) sm[0][wave] = x, sm[1][wave] = (double)bad;
  __syncthreads();
  double r = sm[0][0];
  double b = sm[1][0];
#pragma unroll
  for (int q = 1; q < 4; ++q) {
    r = sm[0][q] > r ? sm[0][q] : r;
    b += sm[1][q];
  }
  return b != 0.0 ? std::numeric_limits<double>::quiet_NaN() : r;
}

__global__ void __launch_bounds__(256) chain_rhat_final_kernel(RhatArgs a) {
  __shared__ double sm[2][4];
  const int win = blockIdx.y;
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t w = a.w[win], half = (w - (w & 1)) / 2, n_seg = 4 * (int64_t)a.n_split;
  double val = -std::numeric_limits<double>::infinity();      // (a column beyond p never wins, and is no NaN)
  if (j < a.p) {
    double mean[2], within[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      Moments t{0, 0.0, 0.0};
      const double* part = a.part + (int64_t)(2 * win + h) * a.n_split * 2 * a.p;
      for (int z = 0; z < a.n_split; ++z)      // the row splits, in row order
        chan_merge(t, seg_bound(half, 4 * (int64_t)z + 4, n_seg) - seg_bound(half, 4 * (int64_t)z, n_seg), part[(int64_t)z * 2 * a.p + j],
                   part[((int64_t)z * 2 + 1) * a.p + j]);
      mean[h] = t.mean;
      within[h] = t.m2 / (double)(half - 1);
    }
    const double mm = (mean[0] + mean[1]) / 2.0;
    const double d0 = mean[0] - mm, d1 = mean[1] - mm;
    const double between = (double)half * (d0 * d0 + d1 * d1);
    // np.nanmean over the two halves
    const bool n0 = within[0] != within[0], n1 = within[1] != within[1];
    const double wmean = n0 ? within[1] : (n1 ? within[0] : (within[0] + within[1]) / 2.0);
    const double W = wmean + a.jitter;
    val = sqrt((double)(half - 1) / (double)half + between / ((double)half * W));
    if (a.rhat) a.rhat[(int64_t)win * a.p + j] = val;
  }
  const double m = block_nanmax(val, sm);
  if (threadIdx.x == 0) a.block_max[(int64_t)win * gridDim.x + blockIdx.x] = m;
}

__global__ void __launch_bounds__(256) chain_rhat_max_kernel(const double* __restrict__ block_max, int64_t n_blocks,
                                                            double* __restrict__ out) {
  __shared__ double sm[2][4];
  const double* src = block_max + (int64_t)blockIdx.x * n_blocks;
  double x = -std::numeric_limits<double>::infinity();
  bool bad = false;
  for (int64_t i = threadIdx.x; i < n_blocks; i += 256) {
    const double v = src[i];
    bad |= v != v;
    x = v > x ? v : x;
  }
  const double m = block_nanmax(bad ? std::numeric_limits<double>::quiet_NaN() : x, sm);
  if (threadIdx.x == 0) out[blockIdx.x] = m;
}

// ---- the mean of a single column ------------------------------------------------------------------------------------------
// With p = 1 the rows are contiguous along the reduced axis and numpy does not add them one by one: add.reduce hands its
// inner loop at most 8192 values at a time, the loop adds each such run by pairwise summation (below 8 values in order; up
// to 128 values eight interleaved partial sums combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the remainder in order;
// above, two halves, the first a multiple of 8), and the runs' sums are added in order.  One thread restates that, the
// recursion unrolled onto a small stack in LDS (a degenerate shape: FASO's parameters are never one number).
__device__ __forceinline__ double pairwise_leaf(const double* a, int n) {
  if (n < 8) {
    double r = 0.0;
    for (int i = 0; i < n; ++i) r += a[i];
    return r;
  }
  double r0 = a[0], r1 = a[1], r2 = a[2], r3 = a[3], r4 = a[4], r5 = a[5], r6 = a[6], r7 = a[7];
  int i = 8;
  for (; i < n - (n % 8); i += 8) {
    r0 += a[i], r1 += a[i + 1], r2 += a[i + 2], r3 += a[i + 3];
    r4 += a[i + 4], r5 += a[i + 5], r6 += a[i + 6], r7 += a[i + 7];
  }
  double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
  for (; i < n; ++i) res += a[i];
  return res;
}

__global__ void __launch_bounds__(64) chain_mean_column_kernel(const double* __restrict__ x, int64_t n, double* __restrict__ out) {
  constexpr int kRun = 8192, kDepth = 16;      // (a run of 8192 halves down to 128 in 6 steps)
  __shared__ int st_off[kDepth], st_n[kDepth], st_state[kDepth];
  __shared__ double st_val[kDepth];
  if (threadIdx.x != 0) return;
  double total = 0.0;
  for (int64_t c0 = 0; c0 < n; c0 += kRun) {
    const double* a = x + c0;
    int sp = 0;
    double ret = 0.0;
    st_off[0] = 0, st_n[0] = (int)(n - c0 < kRun ? n - c0 : kRun), st_state[0] = 0;
    sp = 1;
    while (sp > 0) {
      const int f = sp - 1, off = st_off[f], len = st_n[f];
      int half = len / 2;
      half -= half % 8;
      if (st_state[f] == 0) {
        if (len <= 128) {
          ret = pairwise_leaf(a + off, len);
          --sp;
        } else {
          st_state[f] = 1;
          st_off[sp] = off, st_n[sp] = half, st_state[sp] = 0;
          ++sp;
        }
      } else if (st_state[f] == 1) {
        st_val[f] = ret;
        st_state[f] = 2;
        st_off[sp] = off + half, st_n[sp] = len - half, st_state[sp] = 0;
        ++sp;
      } else {
        ret = st_val[f] + ret;
        --sp;
      }
    }
    total += ret;
  }
  out[0] = total / (double)n;
}

// ---- effective sample size / MCSE ----------------------------------------------------------------------------------------
// _chain_stats.ess's pair loop, one pair at a time
struct Geyer {
  bool done;
  double run_min, kept, ess;
};

__global__ void __launch_bounds__(64) chain_ess_kernel(const double* __restrict__ x, int64_t w, int64_t p, double inv_log10_w,
                                                       double* __restrict__ ess_out, double* __restrict__ mcse_out) {
  constexpr int B = kLagBlock;
  const int64_t j = (int64_t)blockIdx.x * 64 + threadIdx.x;
  const int64_t jj = j < p ? j : p - 1;
  const double* col = x + jj;
  // the column's mean
  double s = 0.0;
  for (int64_t r0 = 0; r0 < w; r0 += 8) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = col[(r0 + u < w ? r0 + u : w - 1) * p];
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (r0 + u < w) s += v[u];
  }
  const double n = (double)w, mean = s / n;
  const int64_t last_pair = w >= 3 ? (w - 3) / 2 : 0;
  Geyer g{j >= p, std::numeric_limits<double>::infinity(), 0.0, std::numeric_limits<double>::quiet_NaN()};
  double s0 = 0.0, chain_var = 0.0, var_plus = 0.0;
  for (int64_t k0 = 0;; k0 += B) {      // lags k0 ... k0 + B - 1
    double acc[B], ring[B];
#pragma unroll
    for (int i = 0; i < B; ++i) acc[i] = 0.0, ring[i] = 0.0;
    // ring[(t - k0) % B] = c[t - k0]; k0 and tb are multiples of B, so at t = tb + u the value c[t - k0 - i] sits in
    // ring[(u - i) % B]: a compile-time index.  Entries not yet written stand for c[negative] = 0.
    for (int64_t tb = k0; tb < w; tb += B) {
      double cur[B], lagged[B];
#pragma unroll
      for (int u = 0; u < B; ++u) {
        const int64_t t = tb + u, tc = t < w ? t : w - 1;
        cur[u] = t < w ? col[tc * p] - mean : 0.0;
        lagged[u] = col[(tc - k0) * p] - mean;
      }
#pragma unroll
      for (int u = 0; u < B; ++u) {
        ring[u] = lagged[u];
#pragma unroll
        for (int i = 0; i < B; ++i) acc[i] = fma(cur[u], ring[(u - i) & (B - 1)], acc[i]);
      }
    }
    if (k0 == 0) {
      s0 = acc[0];
      chain_var = s0 / n * n / (n - 1.0);
      var_plus = chain_var * (n - 1.0) / n;
    }
#pragma unroll
    for (int i = 0; i < B; i += 2) {
      const int64_t pair = (k0 + i) / 2;
      if (!g.done) {
        const double ra = (k0 + i == 0) ? 1.0 : 1.0 - (chain_var - acc[i] / n) / var_plus;
        const double rb = 1.0 - (chain_var - acc[i + 1] / n) / var_plus;
        const double ps = ra + rb;
        if (ra != ra || rb != rb) {
          g.done = true;      // a NaN among the autocorrelations looked at (a constant column): NaN
        } else if (ps <= 0.0 || pair == last_pair) {
          const double tail = pair == 0 ? 1.0 : ((ps >= 0.0 || ra > 0.0) ? ra : 0.0);
          const double tau_raw = -1.0 + 2.0 * g.kept + tail;
          const double tau = tau_raw > inv_log10_w ? tau_raw : inv_log10_w;
          g.ess = n / tau;
          g.done = true;
        } else {
          g.run_min = ps < g.run_min ? ps : g.run_min;
          g.kept += g.run_min;
        }
      }
    }
    if (__all(g.done)) break;
  }
  if (j < p) {
    ess_out[j] = g.ess;
    mcse_out[j] = sqrt(s0 / (n - 1.0)) / sqrt(g.ess);
  }
}

int chain_check_open(vb_ctx* ctx) {
  if (!ctx->chain_open) return fail(ctx, VB_ERR_STATE, "no iterate chain is open (vb_chain_open)");
  return VB_OK;
}

int chain_check_window(vb_ctx* ctx, int64_t w, int64_t least) {
  if (w < least || w > ctx->chain_rows)
    return fail(ctx, VB_ERR_INVALID, "window of %lld rows: must be in [%lld, %lld], the rows the chain holds", (long long)w,
                (long long)least, (long long)ctx->chain_rows);
  return VB_OK;
}

}  // namespace

}  // namespace vb

using namespace vb;

extern "C" {

int vb_chain_open(vb_ctx* ctx, int64_t p, int64_t capacity_rows) {
  if (!ctx) return fail(ctx, VB_ERR_INVALID, "NULL argument");
  if (p <= 0 || capacity_rows <= 0) return fail(ctx, VB_ERR_INVALID, "p and capacity_rows must be positive");
  if (ctx->chain_open) return fail(ctx, VB_ERR_STATE, "an iterate chain is already open (vb_chain_close)");
  if (capacity_rows > (std::numeric_limits<int64_t>::max() / 8) / p)
    return fail(ctx, VB_ERR_INVALID, "a chain of %lld rows x %lld doubles overflows the byte count", (long long)capacity_rows,
                (long long)p);
  const size_t bytes = (size_t)capacity_rows * (size_t)p * sizeof(double);
  VB_HIP(ctx, hipSetDevice(ctx->device));
  if (!ctx->chain.ptr || ctx->chain.bytes < bytes) {
    if (ctx->chain.ptr) {
      VB_TRY(sync_streams(ctx));
      VB_HIP(ctx, ctx->chain.release());
    }
    const hipError_t e = ctx->chain.alloc(bytes);      // (no zero fill: every row is written before it is read)
    if (e != hipSuccess) {
      (void)hipGetLastError();      // (the failed allocation must not show up as a later launch's error)
      return fail(ctx, VB_ERR_HIP, "iterate chain: allocating %zu bytes (%lld rows x %lld doubles) failed: %s", bytes,
                  (long long)capacity_rows, (long long)p, hipGetErrorString(e));
    }
  }
  ctx->chain_p = p, ctx->chain_cap = capacity_rows, ctx->chain_rows = 0;
  ctx->chain_open = true;
  return VB_OK;
}

int vb_chain_close(vb_ctx* ctx) {
  if (!ctx) return fail(ctx, VB_ERR_INVALID, "NULL argument");
  ctx->chain_open = false;
  ctx->chain_p = ctx->chain_cap = ctx->chain_rows = 0;
  if (ctx->chain.ptr) {
    VB_HIP(ctx, hipSetDevice(ctx->device));
    VB_TRY(sync_streams(ctx));
    VB_HIP(ctx, ctx->chain.release());
  }
  return VB_OK;
}

int vb_chain_rows(vb_ctx* ctx, int64_t* rows) {
  if (!ctx || !rows) return fail(ctx, VB_ERR_INVALID, "NULL argument");
  VB_TRY(chain_check_open(ctx));
  *rows = ctx->chain_rows;
  return VB_OK;
}

int vb_chain_append(vb_ctx* ctx, const double* rows_host, int64_t n_rows) {
  if (!ctx || !rows_host) return fail(ctx, VB_ERR_INVALID, "NULL argument");
  VB_TRY(chain_check_open(ctx));
  if (n_rows <= 0 || n_rows > ctx->chain_cap - ctx->chain_rows)
    return fail(ctx, VB_ERR_INVALID, "appending %lld rows: the chain has room for %lld", (long long)n_rows,
                (long long)(ctx->chain_cap - ctx->chain_rows));
  VB_HIP(ctx, hipSetDevice(ctx->device));
  VB_TRY(main_stream_write(ctx));
  const int64_t p = ctx->chain_p;
  VB_HIP(ctx, hipMemcpyAsync((double*)ctx->chain.ptr + ctx->chain_rows * p, rows_host, (size_t)(n_rows * p) * sizeof(double),
                             hipMemcpyHostToDevice, ctx->stream));
  VB_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->chain_rows += n_rows;
  return VB_OK;
}

int vb_chain_fetch(vb_ctx* ctx, int64_t first_row, int64_t n_rows, double* out) {
  if (!ctx || !out) return fail(ctx, VB_ERR_INVALID, "NULL argument");
  VB_TRY(chain_check_open(ctx));
  if (first_row < 0 || n_rows <= 0 || n_rows > ctx->chain_rows - first_row)
    return fail(ctx, VB_ERR_INVALID, "rows [%lld, %lld) are not among the %lld the chain holds", (long long)first_row,
                (long long)(first_row + n_rows), (long long)ctx->chain_rows);
  VB_HIP(ctx, hipSetDevice(ctx->device));
  const int64_t p = ctx->chain_p;
  VB_HIP(ctx, hipMemcpyAsync(out, (const double*)ctx->chain.ptr + first_row * p, (size_t)(n_rows * p) * sizeof(double),
                             hipMemcpyDeviceToHost, ctx->stream));
  VB_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return VB_OK;
}

int vb_chain_mean(vb_ctx* ctx, int64_t w, double* mean) {
  if (!ctx || !mean) return fail(ctx, VB_ERR_INVALID, "NULL argument");
  VB_TRY(chain_check_open(ctx));
  VB_TRY(chain_check_window(ctx, w, 1));
  VB_HIP(ctx, hipSetDevice(ctx->device));
  VB_TRY(main_stream_write(ctx));
  const int64_t p = ctx->chain_p;
  VB_TRY(ensure(ctx, ctx->chain_work, (size_t)p * sizeof(double)));
  double* out = (double*)ctx->chain_work.ptr;
  const double* first = (const double*)ctx->chain.ptr + (ctx->chain_rows - w) * p;
  if (p == 1) {      // (numpy adds a contiguous column pairwise, not row by row)
    hipLaunchKernelGGL(chain_mean_column_kernel, dim3(1), dim3(64), 0, ctx->stream, first, w, out);
    VB_HIP(ctx, hipGetLastError());
  } else {
    VB_TRY(history_mean_enqueue(ctx, first, w, p, out));
  }
  const FetchSeg seg[1] = {{out, (size_t)p * sizeof(double), mean}};
  return fetch_blocking(ctx, ctx->stream, seg, 1);
}

int vb_chain_rhat(vb_ctx* ctx, const int64_t* windows, int n_windows, double jitter, double* max_rhat, double* rhat) {
  if (!ctx || !windows || !max_rhat) return fail(ctx, VB_ERR_INVALID, "NULL argument");
  VB_TRY(chain_check_open(ctx));
  if (n_windows < 1 || n_windows > kMaxWindows)
    return fail(ctx, VB_ERR_INVALID, "n_windows must be in [1, %d]", kMaxWindows);
  int64_t w_max = 0;
  for (int i = 0; i < n_windows; ++i) {
    VB_TRY(chain_check_window(ctx, windows[i], 2));
    w_max = windows[i] > w_max ? windows[i] : w_max;
  }
  VB_HIP(ctx, hipSetDevice(ctx->device));
  VB_TRY(main_stream_write(ctx));
  const int64_t p = ctx->chain_p;
  const int64_t col_blocks = (p + 63) / 64, fin_blocks = (p + 255) / 256;
  // rows over several workgroups when the columns alone do not fill the device (about eight waves per SIMD), each
  // workgroup keeping at least 64 rows per wave
  const int64_t want = ((int64_t)ctx->prop.multiProcessorCount * 8 + col_blocks * 2 * n_windows - 1) / (col_blocks * 2 * n_windows);
  const int64_t most = w_max / 2 / 256 > 1 ? w_max / 2 / 256 : 1;
  int64_t n_split = want < most ? want : most;
  n_split = n_split > 64 ? 64 : (n_split < 1 ? 1 : n_split);
  auto r16 = [](int64_t v) { return round_up(v, 16); };
  const int64_t o_part = 0, o_rhat = o_part + r16(2 * (int64_t)n_windows * n_split * 2 * p);
  const int64_t o_bmax = o_rhat + r16(rhat ? n_windows * p : 0), o_max = o_bmax + r16(n_windows * fin_blocks);
  VB_TRY(ensure(ctx, ctx->chain_work, (size_t)(o_max + r16(n_windows)) * sizeof(double)));
  double* base = (double*)ctx->chain_work.ptr;
  RhatArgs a;
  a.chain = (const double*)ctx->chain.ptr;
  a.rows = ctx->chain_rows, a.p = p;
  a.n_windows = n_windows, a.n_split = (int)n_split;
  for (int i = 0; i < n_windows; ++i) a.w[i] = windows[i];
  a.jitter = jitter;
  a.part = base + o_part;
  a.rhat = rhat ? base + o_rhat : nullptr;
  a.block_max = base + o_bmax;
  a.max_out = base + o_max;
  hipStream_t st = ctx->stream;
  hipLaunchKernelGGL(chain_rhat_partial_kernel, dim3((unsigned)col_blocks, (unsigned)(2 * n_windows), (unsigned)n_split),
                     dim3(256), 0, st, a);
  VB_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(chain_rhat_final_kernel, dim3((unsigned)fin_blocks, (unsigned)n_windows), dim3(256), 0, st, a);
  VB_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(chain_rhat_max_kernel, dim3((unsigned)n_windows), dim3(256), 0, st, (const double*)a.block_max,
                     fin_blocks, a.max_out);
  VB_HIP(ctx, hipGetLastError());
  const FetchSeg seg[2] = {{a.max_out, (size_t)n_windows * sizeof(double), max_rhat},
                           {a.rhat, rhat ? (size_t)(n_windows * p) * sizeof(double) : 0, rhat}};
  return fetch_blocking(ctx, st, seg, rhat ? 2 : 1);
}

int vb_chain_ess_mcse(vb_ctx* ctx, int64_t w, double* ess, double* mcse) {
  if (!ctx || !ess || !mcse) return fail(ctx, VB_ERR_INVALID, "NULL argument");
  VB_TRY(chain_check_open(ctx));
  VB_TRY(chain_check_window(ctx, w, 2));
  VB_HIP(ctx, hipSetDevice(ctx->device));
  VB_TRY(main_stream_write(ctx));
  const int64_t p = ctx->chain_p;
  VB_TRY(ensure(ctx, ctx->chain_work, (size_t)(2 * round_up(p, 16)) * sizeof(double)));
  double* d_ess = (double*)ctx->chain_work.ptr;
  double* d_mcse = d_ess + round_up(p, 16);
  hipStream_t st = ctx->stream;
  hipLaunchKernelGGL(chain_ess_kernel, dim3((unsigned)((p + 63) / 64)), dim3(64), 0, st,
                     (const double*)ctx->chain.ptr + (ctx->chain_rows - w) * p, w, p, 1.0 / std::log10((double)w), d_ess, d_mcse);
  VB_HIP(ctx, hipGetLastError());
  const FetchSeg seg[2] = {{d_ess, (size_t)p * sizeof(double), ess}, {d_mcse, (size_t)p * sizeof(double), mcse}};
  return fetch_blocking(ctx, st, seg, 2);
}

}  // extern "C"
