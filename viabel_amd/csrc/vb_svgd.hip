// Stein variational gradient descent (vb_svgd_direction, vb_svgd_run): Liu & Wang 2016 with the RBF kernel in
// rescaled, centred coordinates.  With c the column means of x, y = (x - c) / scale, g = score * scale and, per pair,
//   r2_ij = sum_k (y_ik - y_jk)^2        kappa_ij = exp(-r2_ij / h)
//   phi_y(i) = 1/n [ sum_j kappa_ij g_j + (2/h) ( y_i sum_j kappa_ij - sum_j kappa_ij y_j ) ]        phi(i) = phi_y(i) / scale
// CENTRE FIRST, THEN SCALE: x / scale - c / scale loses the spread of particles that sit far from the origin.
// DIFFERENCE FORM: r2 is accumulated from the differences themselves (vb_ksd.hip's tiling), never from a Gram product, so
// r2_ij == r2_ji bit for bit, duplicates give exactly 0 and kappa_ii == 1.
// MEDIAN RULE: h = m / log(n + 1), m the lower median of the n (n - 1) / 2 values r2_ij, i < j (0-based rank
// (n (n - 1) / 2 - 1) / 2), selected EXACTLY by a radix selection on the 64-bit patterns (non-negative doubles sort like
// their patterns) with integer counting: five passes of 13, 13, 13, 13 and 12 bits.  n = 1 or m = 0: h = 1.
//
//   svgd_colsum_kernel    column sums of x per 256-row chunk: rows r = lane mod 16 in order, then the 16 lanes in order
//   svgd_colmean_kernel   c = (the chunks' sums in chunk order) / n
//   svgd_stage_kernel     B = [G | Y] (round_up(n, 64) rows of 2 round_up(d, 16) columns, padding zeroed)
//   svgd_pair_kernel      one workgroup per 64 x 64 tile on or below the diagonal: r2 of the tile, stored and mirrored
//   svgd_sel_*_kernel     the selection: histogram of one digit of the values that share the prefix found so far, then one
//                         workgroup that picks the digit's bin, narrows the rank and, after the last pass, forms h
//   svgd_map_kernel       K = exp(-r2 / h) in place (padded rows and columns 0) and its row sums, in a fixed tree
//   (gemm_f64_launch)     K [G | Y] on fp64 MFMA
//   svgd_finish_kernel    -phi (the gradient the optimiser step takes) and every row's sum of phi^2
//   svgd_stats_kernel     (the run) mean log p, h and rms(phi) of the iteration into the histories
// No floating-point atomics, every sum in a fixed order: two calls with the same inputs return the same bits, and the run
// enqueues exactly what the direction entry enqueues, followed by fit_step_enqueue.
// The pair tile's constants and draw order (pair_draw), the 256-thread sum and the host's refusals, row copies, workspace
// carver and stream guard are vb_particles.h's, shared with vb_ksd.hip.
#include <cmath>
#include <vector>

#include "vb_particles.h"

namespace vb {

constexpr int64_t kSvgdMaxParticles = 8192; // the n x n matrix is stored: 512 MiB at the capacity
constexpr int kSvgdBins = 8192;             // bins of one selection pass (13 bits)
constexpr int kSvgdPasses = 5;
// digit p of a pattern: (pattern >> shift[p]) & (2^bits[p] - 1); the digits cover the 64 bits from the top
static const int kSvgdShift[kSvgdPasses] = {51, 38, 25, 12, 0};
static const int kSvgdBits[kSvgdPasses] = {13, 13, 13, 13, 12};

struct SvgdSel {                            // the selection's state, in device memory (h never leaves it during a run)
  unsigned long long prefix;                // the digits found so far, the top one first
  unsigned long long rank;                  // rank of the wanted element among the values that share the prefix
  double h;
  unsigned long long unused;
};

constexpr int kSvgdMeanChunk = 256;          // rows per workgroup of the column-sum kernel

// grid = (ld / 16, ceil(n / 256)): thread (ty, tx) adds column 16 blockIdx.x + tx over the rows ty, ty + 16, ... of the
// workgroup's 256-row chunk in order; the 16 partial sums of a column are then added in lane order
__global__ void __launch_bounds__(256) svgd_colsum_kernel(const double* __restrict__ X, int64_t ld, int64_t n,
                                                           double* __restrict__ part) {
  __shared__ double sh[16][17];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int64_t col = (int64_t)blockIdx.x * 16 + tx;
  const int64_t r0 = (int64_t)blockIdx.y * kSvgdMeanChunk;
  const int64_t r1 = r0 + kSvgdMeanChunk < n ? r0 + kSvgdMeanChunk : n;
  double acc = 0.0;
  for (int64_t r = r0 + ty; r < r1; r += 16) acc += X[r * ld + col];
  sh[ty][tx] = acc;
  __syncthreads();
  if (ty == 0) {
    double s = sh[0][tx];
#pragma unroll
    for (int k = 1; k < 16; ++k) s += sh[k][tx];
    part[(int64_t)blockIdx.y * ld + col] = s;
  }
}

// c = (the chunks' sums in chunk order) / n
__global__ void __launch_bounds__(256) svgd_colmean_kernel(const double* __restrict__ part, int64_t ld, int chunks, int64_t n,
                                                            double* __restrict__ c) {
  const int64_t col = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (col >= ld) return;
  double s = part[col];
  for (int k = 1; k < chunks; ++k) s += part[(int64_t)k * ld + col];
  c[col] = s / (double)n;
}

struct SvgdStageArgs {
  const double* X;          // [n x ld] particles
  const double* G;          // [n x ld] scores
  const double* c;          // [ld] column means
  const double* scale;      // [d] or nullptr (ones)
  double* B;                // [np x 2 ld]: [G | Y]
  int64_t n, ld;
  int d;
};

// grid = np rows
__global__ void __launch_bounds__(256) svgd_stage_kernel(const SvgdStageArgs a) {
  const int64_t row = blockIdx.x;
  const bool live = row < a.n;
  double* b = a.B + row * 2 * a.ld;
  for (int c = threadIdx.x; c < (int)a.ld; c += 256) {
    double yv = 0.0, gv = 0.0;
    if (live && c < a.d) {
      const double l = a.scale ? a.scale[c] : 1.0;
      yv = (a.X[row * a.ld + c] - a.c[c]) / l;
      gv = a.G[row * a.ld + c] * l;
    }
    b[c] = gv;
    b[a.ld + c] = yv;
  }
}

struct SvgdPairArgs {
  const double* Y;          // staged particles: row stride ldy (the right half of B)
  double* R;                // [np x np] squared distances
  int64_t ldy, np;
  int nk;                   // LDS steps: round_up(d, 16) / 16
};

// grid = tiles (tiles + 1) / 2: workgroup t computes tile (rb, cb), cb <= rb, t = rb (rb + 1) / 2 + cb, and stores it at
// (rb, cb) and, transposed, at (cb, rb) -- the same doubles, so the stored matrix is symmetric bit for bit.  256 threads,
// 4 x 4 pairs per thread, operands through LDS: vb_ksd.hip's tiling with two operand streams in place of four.
__global__ void __launch_bounds__(256) svgd_pair_kernel(const SvgdPairArgs a) {
  __shared__ __attribute__((aligned(16))) double sh[2][kPairK][kPairLdsRow];      // [Yi | Yj][coordinate][particle]
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
  const int lr = tid >> 2, lq = tid & 3;        // staging: particle lr, coordinates 2 lq, 2 lq + 1, 8 + 2 lq, 9 + 2 lq
  const int t = blockIdx.x;
  int rb = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
  while ((rb + 1) * (rb + 2) / 2 <= t) ++rb;
  while (rb * (rb + 1) / 2 > t) --rb;
  const int cb = t - rb * (rb + 1) / 2;
  const int64_t off_i = ((int64_t)rb * kPairTile + lr) * a.ldy + 2 * lq;
  const int64_t off_j = ((int64_t)cb * kPairTile + lr) * a.ldy + 2 * lq;

  double r2[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) r2[i][j] = 0.0;
  double2 pre[2][2];
  auto fetch = [&](int ks) {
    const int64_t k0 = (int64_t)ks * kPairK;
    const double* src[2] = {a.Y + off_i + k0, a.Y + off_j + k0};
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      pre[m][0] = *reinterpret_cast<const double2*>(src[m]);
      pre[m][1] = *reinterpret_cast<const double2*>(src[m] + 8);
    }
  };
  fetch(0);
  for (int ks = 0; ks < a.nk; ++ks) {
    __syncthreads();                            // the previous step's reads are done
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      sh[m][2 * lq][lr] = pre[m][0].x;
      sh[m][2 * lq + 1][lr] = pre[m][0].y;
      sh[m][8 + 2 * lq][lr] = pre[m][1].x;
      sh[m][9 + 2 * lq][lr] = pre[m][1].y;
    }
    __syncthreads();
    if (ks + 1 < a.nk) fetch(ks + 1);
#pragma unroll 4
    for (int k = 0; k < kPairK; ++k) {
      double yi[4], yj[4];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const double2 v0 = *reinterpret_cast<const double2*>(&sh[0][k][h * 32 + ty * 2]);
        const double2 v1 = *reinterpret_cast<const double2*>(&sh[1][k][h * 32 + tx * 2]);
        yi[2 * h] = v0.x, yi[2 * h + 1] = v0.y;
        yj[2 * h] = v1.x, yj[2 * h + 1] = v1.y;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const double dy = yi[i] - yj[j];
          r2[i][j] = fma(dy, dy, r2[i][j]);
        }
    }
  }
  // rows pair_draw(ty, i), columns pair_draw(tx, j): q = 0, 1 and q = 2, 3 are adjacent, 16-byte stores both ways
  const int64_t row0 = (int64_t)rb * kPairTile, col0 = (int64_t)cb * kPairTile;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int jp = 0; jp < 2; ++jp) {
      double2 v;
      v.x = r2[i][2 * jp], v.y = r2[i][2 * jp + 1];
      *reinterpret_cast<double2*>(a.R + (row0 + pair_draw(ty, i)) * a.np + col0 + pair_draw(tx, 2 * jp)) = v;
    }
  if (rb != cb) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int ip = 0; ip < 2; ++ip) {
        double2 v;
        v.x = r2[2 * ip][j], v.y = r2[2 * ip + 1][j];
        *reinterpret_cast<double2*>(a.R + (col0 + pair_draw(tx, j)) * a.np + row0 + pair_draw(ty, 2 * ip)) = v;
      }
  }
}

// one workgroup: the selection's start.  fixed_h > 0 (or nothing to select: n = 1) is the bandwidth itself
__global__ void __launch_bounds__(256) svgd_sel_init_kernel(SvgdSel* sel, unsigned* hist, unsigned long long rank,
                                                             double fixed_h) {
  for (int b = threadIdx.x; b < kSvgdBins; b += 256) hist[b] = 0u;
  if (threadIdx.x == 0) {
    sel->prefix = 0ull;
    sel->rank = rank;
    sel->h = fixed_h;
    sel->unused = 0ull;
  }
}

// digit `pass` of the values r2_ij, i < j < n, whose higher digits equal the prefix: counted in LDS, then added to the
// global histogram (integer atomics: the counts do not depend on the order).  Workgroup b takes the rows b, b + gridDim.x, ...
__global__ void __launch_bounds__(256) svgd_sel_hist_kernel(const double* __restrict__ R, int64_t np, int64_t n,
                                                             const SvgdSel* __restrict__ sel, unsigned* __restrict__ hist,
                                                             int pass, int shift, int bits) {
  __shared__ unsigned lh[kSvgdBins];
  for (int b = threadIdx.x; b < kSvgdBins; b += 256) lh[b] = 0u;
  __syncthreads();
  const unsigned long long mask = (1ull << bits) - 1ull, prefix = sel->prefix;
  const int hi = shift + bits;                  // 64 in pass 0: no prefix yet
  for (int64_t i = blockIdx.x; i + 1 < n; i += gridDim.x) {
    const double* row = R + i * np;
    for (int64_t j = i + 1 + threadIdx.x; j < n; j += 256) {
      const unsigned long long v = (unsigned long long)__double_as_longlong(row[j]);
      if (pass == 0 || (v >> hi) == prefix) atomicAdd(&lh[(unsigned)((v >> shift) & mask)], 1u);
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < kSvgdBins; b += 256)
    if (lh[b]) atomicAdd(&hist[b], lh[b]);
}

// one workgroup: the bin that holds the wanted rank becomes the next digit of the prefix, the rank becomes the rank inside
// that bin, the histogram is zeroed for the next pass.  After the last pass the prefix is the median's pattern:
// h = m / log(n + 1), or 1 when m is 0.
__global__ void __launch_bounds__(256) svgd_sel_scan_kernel(SvgdSel* sel, unsigned* hist, int bits, int last, double log_n1) {
  __shared__ unsigned long long tot[256];
  constexpr int kPer = kSvgdBins / 256;
  const int tid = threadIdx.x;
  unsigned cnt[kPer];
  unsigned long long mine = 0ull;
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    cnt[k] = hist[tid * kPer + k];
    hist[tid * kPer + k] = 0u;
    mine += cnt[k];
  }
  tot[tid] = mine;
  __syncthreads();
  const unsigned long long rank = sel->rank, prefix = sel->prefix;
  unsigned long long before = 0ull;
  for (int k = 0; k < tid; ++k) before += tot[k];
  __syncthreads();                              // every thread has read sel before one of them writes it
  if (rank >= before && rank < before + mine) {
    unsigned long long cum = before;
    int bin = tid * kPer;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      if (rank >= cum + cnt[k]) {
        cum += cnt[k];
        bin = tid * kPer + k + 1;
      } else {
        break;
      }
    }
    const unsigned long long found = (prefix << bits) | (unsigned long long)bin;
    sel->prefix = found;
    sel->rank = rank - cum;
    if (last) {
      const double m = __longlong_as_double((long long)found);
      sel->h = m > 0.0 ? m / log_n1 : (m == 0.0 ? 1.0 : m);      // (a NaN median stays a NaN: VB_ERR_NUMERIC at the end)
    }
  }
}

// grid = np rows: K = exp(-r2 / h) in place, 0 in the padded rows and columns; rowsum[row] = sum_j K[row][j], thread t
// adding the columns t, t + 256, ... in order, then the workgroup's fixed tree
__global__ void __launch_bounds__(256) svgd_map_kernel(double* __restrict__ R, int64_t np, int64_t n,
                                                        const SvgdSel* __restrict__ sel, double* __restrict__ rowsum) {
  __shared__ double sh[4];
  const int64_t row = blockIdx.x;
  const double h = sel->h;
  const bool live = row < n;
  double* r = R + row * np;
  double acc = 0.0;
  for (int64_t j = threadIdx.x; j < np; j += 256) {
    double v = 0.0;
    if (live && j < n) v = exp(-r[j] / h);
    r[j] = v;
    acc += v;
  }
  acc = block_sum(acc, sh);
  if (threadIdx.x == 0) rowsum[row] = acc;
}

struct SvgdFinishArgs {
  const double* P;          // [np x 2 ld] the product K [G | Y]
  const double* B;          // [np x 2 ld] [G | Y]
  const double* rowsum;     // [np]
  const SvgdSel* sel;
  const double* scale;      // [d] or nullptr
  double* neg_phi;          // [n x ld]: -phi, 0 in the padded columns (the gradient of the optimiser step)
  double* rowsq;            // [n]: sum_c phi[row][c]^2
  int64_t n, ld;
  int d;
};

// grid = n rows
__global__ void __launch_bounds__(256) svgd_finish_kernel(const SvgdFinishArgs a) {
  __shared__ double sh[4];
  const int64_t row = blockIdx.x;
  const double two_h = 2.0 / a.sel->h, rs = a.rowsum[row], nn = (double)a.n;
  const double* p = a.P + row * 2 * a.ld;
  const double* b = a.B + row * 2 * a.ld;
  double acc = 0.0;
  for (int c = threadIdx.x; c < (int)a.ld; c += 256) {
    double v = 0.0;
    if (c < a.d) {
      const double l = a.scale ? a.scale[c] : 1.0;
      v = (p[c] + two_h * (b[a.ld + c] * rs - p[a.ld + c])) / nn / l;
      a.neg_phi[row * a.ld + c] = -v;
    } else {
      a.neg_phi[row * a.ld + c] = 0.0;
    }
    acc = fma(v, v, acc);
  }
  acc = block_sum(acc, sh);
  if (threadIdx.x == 0) a.rowsq[row] = acc;
}

// one workgroup: value[0] = mean log p (what fit_step_enqueue logs as the iteration's value), h_hist[k] = h,
// rms_hist[k] = sqrt(sum phi^2 / (n d)); thread t adds the rows t, t + 256, ... in order
__global__ void __launch_bounds__(256) svgd_stats_kernel(const double* __restrict__ rowsq, const double* __restrict__ f,
                                                          int64_t n, int d, const SvgdSel* __restrict__ sel,
                                                          double* __restrict__ value, double* __restrict__ h_hist,
                                                          double* __restrict__ rms_hist, int64_t k) {
  __shared__ double sh[4];
  double sq = 0.0, lp = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) sq += rowsq[i], lp += f[i];
  sq = block_sum(sq, sh);
  lp = block_sum(lp, sh);
  if (threadIdx.x == 0) {
    value[0] = lp / (double)n;
    h_hist[k] = sel->h;
    rms_hist[k] = sqrt(sq / ((double)n * (double)d));
  }
}

// Where the pieces of a call live in ctx->svgd_work (doubles from the base); the run's pieces come last
struct SvgdLayout {
  int64_t n, d, np, ld;
  int64_t o_x, o_g, o_f, o_c, o_cpart, o_scale, o_b, o_r, o_rowsum, o_p, o_rowsq, o_sel, o_hist, o_out, o_s1, o_s2, o_val,
      o_hh, o_hr, total;
};
static SvgdLayout svgd_layout(int64_t n, int64_t d, int64_t n_iters) {
  SvgdLayout L;
  L.n = n, L.d = d, L.np = round_up(n, kPairTile), L.ld = round_up(d, 16);
  Carver carve;
  L.o_x = carve(L.np * L.ld), L.o_g = carve(L.np * L.ld), L.o_f = carve(L.np), L.o_c = carve(L.ld), L.o_scale = carve(L.ld);
  L.o_cpart = carve((L.np / kPairTile + 3) / 4 * L.ld);      // one row of column sums per 256-row chunk
  L.o_b = carve(L.np * 2 * L.ld), L.o_r = carve(L.np * L.np), L.o_rowsum = carve(L.np), L.o_p = carve(L.np * 2 * L.ld);
  L.o_rowsq = carve(L.np), L.o_sel = carve(sizeof(SvgdSel) / sizeof(double)), L.o_hist = carve(kSvgdBins / 2);
  L.o_out = carve(1 + L.np * L.ld);      // [value | -phi]: fit_step_enqueue's (value, gradient)
  L.o_s1 = carve(n_iters ? n * L.ld : 0), L.o_s2 = carve(n_iters ? n * L.ld : 0);
  L.o_val = carve(n_iters), L.o_hh = carve(n_iters), L.o_hr = carve(n_iters);
  L.total = carve.off;
  return L;
}

// One direction from the particles at o_x and the scores at o_g, both on the device: -phi to o_out + 1, h to the selection
// state, the rows' sums of phi^2 to o_rowsq.  Enqueued only.
static int svgd_direction_enqueue(vb_ctx* ctx, const SvgdLayout& L, bool has_scale, double bandwidth) {
  hipStream_t st = ctx->stream;
  double* base = (double*)ctx->svgd_work.ptr;
  const int64_t n = L.n, np = L.np, ld = L.ld;
  const double* scale = has_scale ? base + L.o_scale : nullptr;
  double *B = base + L.o_b, *R = base + L.o_r, *P = base + L.o_p;
  SvgdSel* sel = (SvgdSel*)(base + L.o_sel);
  unsigned* hist = (unsigned*)(base + L.o_hist);

  const int chunks = (int)((n + kSvgdMeanChunk - 1) / kSvgdMeanChunk);
  hipLaunchKernelGGL(svgd_colsum_kernel, dim3((unsigned)(ld / 16), (unsigned)chunks), dim3(256), 0, st,
                     (const double*)(base + L.o_x), ld, n, base + L.o_cpart);
  VB_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(svgd_colmean_kernel, dim3((unsigned)((ld + 255) / 256)), dim3(256), 0, st,
                     (const double*)(base + L.o_cpart), ld, chunks, n, base + L.o_c);
  VB_HIP(ctx, hipGetLastError());
  const SvgdStageArgs sa{base + L.o_x, base + L.o_g, base + L.o_c, scale, B, n, ld, (int)L.d};
  hipLaunchKernelGGL(svgd_stage_kernel, dim3((unsigned)np), dim3(256), 0, st, sa);
  VB_HIP(ctx, hipGetLastError());
  const int tiles = (int)(np / kPairTile);
  const SvgdPairArgs pa{B + ld, R, 2 * ld, np, (int)(ld / kPairK)};
  hipLaunchKernelGGL(svgd_pair_kernel, dim3((unsigned)(tiles * (tiles + 1) / 2)), dim3(256), 0, st, pa);
  VB_HIP(ctx, hipGetLastError());

  const unsigned long long pairs = (unsigned long long)n * (unsigned long long)(n - 1) / 2ull;
  const bool select = !(bandwidth > 0.0) && n > 1;
  hipLaunchKernelGGL(svgd_sel_init_kernel, dim3(1), dim3(256), 0, st, sel, hist, select ? (pairs - 1ull) / 2ull : 0ull,
                     bandwidth > 0.0 ? bandwidth : 1.0);
  VB_HIP(ctx, hipGetLastError());
  if (select) {
    const unsigned blocks = (unsigned)(n - 1 < 1024 ? n - 1 : 1024);
    const double log_n1 = std::log((double)n + 1.0);
    for (int p = 0; p < kSvgdPasses; ++p) {
      hipLaunchKernelGGL(svgd_sel_hist_kernel, dim3(blocks), dim3(256), 0, st, (const double*)R, np, n, (const SvgdSel*)sel,
                         hist, p, kSvgdShift[p], kSvgdBits[p]);
      VB_HIP(ctx, hipGetLastError());
      hipLaunchKernelGGL(svgd_sel_scan_kernel, dim3(1), dim3(256), 0, st, sel, hist, kSvgdBits[p],
                         p + 1 == kSvgdPasses ? 1 : 0, log_n1);
      VB_HIP(ctx, hipGetLastError());
    }
  }
  hipLaunchKernelGGL(svgd_map_kernel, dim3((unsigned)np), dim3(256), 0, st, R, np, n, (const SvgdSel*)sel, base + L.o_rowsum);
  VB_HIP(ctx, hipGetLastError());
  gemm_f64_launch<true>(st, gemm_product(R, np, B, 2 * ld, (int)np, (int)(2 * ld), (int)np, 0), 1,
                        ctx->prop.multiProcessorCount, EpiStorePlain{P, 2 * ld});
  VB_HIP(ctx, hipGetLastError());
  const SvgdFinishArgs fa{P, B, base + L.o_rowsum, sel, scale, base + L.o_out + 1, base + L.o_rowsq, n, ld, (int)L.d};
  hipLaunchKernelGGL(svgd_finish_kernel, dim3((unsigned)n), dim3(256), 0, st, fa);
  VB_HIP(ctx, hipGetLastError());
  return VB_OK;
}

// what both entries check of the shapes, the scale and the bandwidth
static int svgd_check(vb_ctx* ctx, const char* name, int64_t n, int64_t d, const double* scale, double bandwidth) {
  if (n < 1) return fail(ctx, VB_ERR_INVALID, "the number of particles must be positive");
  if (n > kSvgdMaxParticles)
    return fail(ctx, VB_ERR_UNSUPPORTED, "%s takes at most %lld particles (got %lld)", name, (long long)kSvgdMaxParticles,
                (long long)n);
  if (d < 1 || d > (1 << 24)) return fail(ctx, VB_ERR_INVALID, "the dimension must lie in [1, 2^24]");
  if (!(bandwidth >= 0.0) || !std::isfinite(bandwidth))
    return fail(ctx, VB_ERR_INVALID, "bandwidth must be positive and finite, or 0 for the median rule");
  if (scale) VB_TRY(positive_finite(ctx, name, "scale", scale, d));
  return VB_OK;
}

}  // namespace vb

using namespace vb;

extern "C" {

int vb_svgd_direction(vb_ctx* ctx, const double* x, int64_t n, int64_t d, const double* scores, const double* scale,
                      double bandwidth, double* phi, double* logp, double* h_used) {
  if (!ctx || !x || !phi || !h_used) return fail(ctx, VB_ERR_INVALID, "NULL argument");
  VB_TRY(svgd_check(ctx, "vb_svgd_direction", n, d, scale, bandwidth));
  if (!scores) {
    VB_TRY(model_bound_refuse(ctx, "vb_svgd_direction", "x", d));
    VB_TRY(model_device_refuse(ctx, "vb_svgd_direction", true, false));
  }
  VB_HIP(ctx, hipSetDevice(ctx->device));
  VB_TRY(main_stream_write(ctx));
  hipStream_t st = ctx->stream;
  StreamDrain drain{st};
  const SvgdLayout L = svgd_layout(n, d, 0);
  VB_TRY(ensure(ctx, ctx->svgd_work, (size_t)L.total * sizeof(double)));
  double* base = (double*)ctx->svgd_work.ptr;
  VB_TRY(upload_rows(ctx, base + L.o_x, x, n, d, L.ld));
  if (scores)
    VB_TRY(upload_rows(ctx, base + L.o_g, scores, n, d, L.ld));
  else
    VB_TRY(model_grad_rows(ctx, base + L.o_x, L.ld, n, d, base + L.o_g, base + L.o_f));
  if (scale)
    VB_HIP(ctx, hipMemcpyAsync(base + L.o_scale, scale, (size_t)d * sizeof(double), hipMemcpyHostToDevice, st));
  VB_TRY(svgd_direction_enqueue(ctx, L, scale != nullptr, bandwidth));
  SvgdSel sel{};
  VB_HIP(ctx, download_rows(ctx, phi, base + L.o_out + 1, n, d, L.ld));
  VB_HIP(ctx, hipMemcpyAsync(&sel, base + L.o_sel, sizeof(SvgdSel), hipMemcpyDeviceToHost, st));
  if (logp && !scores) VB_HIP(ctx, hipMemcpyAsync(logp, base + L.o_f, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
  VB_HIP(ctx, hipStreamSynchronize(st));
  *h_used = sel.h;
  bool finite = std::isfinite(sel.h);
  for (int64_t i = 0; i < n * d; ++i) {
    phi[i] = -phi[i];      // (the device keeps the optimiser's gradient, -phi; the negation is exact)
    finite = finite && std::isfinite(phi[i]);
  }
  if (!finite) return fail(ctx, VB_ERR_NUMERIC, "the direction is not finite: a particle or its score is not finite");
  return VB_OK;
}

int vb_svgd_run(vb_ctx* ctx, const double* x0, int64_t n, int64_t d, const double* scale, double bandwidth, int opt_kind,
                const double hyper[4], int64_t n_iters, double* state, int has_state, double* x, double* logp,
                double* h_hist, double* rms_hist, double* logp_hist) {
  if (!ctx || !x0 || !hyper || !x || !logp || !h_hist || !rms_hist || !logp_hist)
    return fail(ctx, VB_ERR_INVALID, "NULL argument");
  VB_TRY(svgd_check(ctx, "vb_svgd_run", n, d, scale, bandwidth));
  if (n_iters < 1 || n_iters > ((int64_t)1 << 31)) return fail(ctx, VB_ERR_INVALID, "n_iters must lie in [1, 2^31]");
  if (opt_kind < VB_OPT_SGD || opt_kind > VB_OPT_ADAGRAD) return fail(ctx, VB_ERR_INVALID, "unknown optimiser kind %d", opt_kind);
  if (has_state && !state) return fail(ctx, VB_ERR_INVALID, "has_state set without a state buffer");
  if (!std::isfinite(hyper[0])) return fail(ctx, VB_ERR_INVALID, "the learning rate must be finite");
  // the step runs over the padded particle block, whose padding columns have gradient 0: 0 / sqrt(jitter + 0) must be 0
  if (opt_kind != VB_OPT_SGD && !(hyper[3] > 0.0))
    return fail(ctx, VB_ERR_INVALID, "the optimiser's jitter must be positive");
  VB_TRY(model_bound_refuse(ctx, "vb_svgd_run", "x0", d));
  VB_TRY(model_device_refuse(ctx, "vb_svgd_run", true, true));
  VB_HIP(ctx, hipSetDevice(ctx->device));
  VB_TRY(main_stream_write(ctx));
  hipStream_t st = ctx->stream;
  StreamDrain drain{st};
  const SvgdLayout L = svgd_layout(n, d, n_iters);
  VB_TRY(ensure(ctx, ctx->svgd_work, (size_t)L.total * sizeof(double)));
  double* base = (double*)ctx->svgd_work.ptr;
  double *X = base + L.o_x, *G = base + L.o_g, *F = base + L.o_f;
  const int64_t p = n * L.ld;
  VB_TRY(upload_rows(ctx, X, x0, n, d, L.ld));
  if (scale)
    VB_HIP(ctx, hipMemcpyAsync(base + L.o_scale, scale, (size_t)d * sizeof(double), hipMemcpyHostToDevice, st));
  // the optimiser state: [second moment (n x d) | momentum (n x d)] on the host, two n x ld blocks here; what is not
  // uploaded (no state, the padding) is zero
  VB_HIP(ctx, hipMemsetAsync(base + L.o_s1, 0, (size_t)(L.o_val - L.o_s1) * sizeof(double), st));
  if (has_state) {
    VB_TRY(upload_rows(ctx, base + L.o_s1, state, n, d, L.ld));
    VB_TRY(upload_rows(ctx, base + L.o_s2, state + n * d, n, d, L.ld));
  }
  FitStep step;
  step.kind = opt_kind;
  step.p = p;
  step.lr = hyper[0];
  step.beta1 = hyper[1];
  step.one_minus_beta1 = 1.0 - hyper[1];
  step.beta2 = hyper[2];
  step.one_minus_beta2 = 1.0 - hyper[2];
  step.jitter = hyper[3];
  step.out = base + L.o_out;
  step.theta = X;
  step.s1 = base + L.o_s1;
  step.s2 = base + L.o_s2;
  step.values = base + L.o_val;
  const SvgdSel* sel = (const SvgdSel*)(base + L.o_sel);
  for (int64_t k = 0; k < n_iters; ++k) {
    VB_TRY(model_grad_rows(ctx, X, L.ld, n, d, G, F));
    VB_TRY(svgd_direction_enqueue(ctx, L, scale != nullptr, bandwidth));
    hipLaunchKernelGGL(svgd_stats_kernel, dim3(1), dim3(256), 0, st, (const double*)(base + L.o_rowsq), (const double*)F, n,
                       (int)d, sel, base + L.o_out, base + L.o_hh, base + L.o_hr, k);
    VB_HIP(ctx, hipGetLastError());
    step.k = k;
    step.first = (k == 0 && !has_state) ? 1 : 0;
    VB_TRY(fit_step_enqueue(ctx, step));
  }
  VB_TRY(model_grad_rows(ctx, X, L.ld, n, d, G, F));      // log p of the final particles
  VB_HIP(ctx, download_rows(ctx, x, X, n, d, L.ld));
  auto fetch = [&](double* dst, const double* src, int64_t doubles) {
    return hipMemcpyAsync(dst, src, (size_t)doubles * sizeof(double), hipMemcpyDeviceToHost, st);
  };
  VB_HIP(ctx, fetch(logp, F, n));
  VB_HIP(ctx, fetch(h_hist, base + L.o_hh, n_iters));
  VB_HIP(ctx, fetch(rms_hist, base + L.o_hr, n_iters));
  VB_HIP(ctx, fetch(logp_hist, base + L.o_val, n_iters));
  if (state) {
    VB_HIP(ctx, download_rows(ctx, state, base + L.o_s1, n, d, L.ld));
    VB_HIP(ctx, download_rows(ctx, state + n * d, base + L.o_s2, n, d, L.ld));
  }
  VB_HIP(ctx, hipStreamSynchronize(st));      // the run's one synchronisation
  for (int64_t k = 0; k < n_iters; ++k)
    if (!std::isfinite(h_hist[k]) || !std::isfinite(rms_hist[k]) || !std::isfinite(logp_hist[k]))
      return fail(ctx, VB_ERR_NUMERIC, "iteration %lld: bandwidth %g, rms(phi) %g, mean log p %g", (long long)k, h_hist[k],
                  rms_hist[k], logp_hist[k]);
  return VB_OK;
}

}  // extern "C"
