// Full-rank Gaussian family: ExclusiveKL value and gradient on gfx950 fp64 matrix cores.
//
// The reference has no dense Gaussian family; this follows its ApproximationFamily
// contract (viabel/approximations.py:26-182) with MultivariateT's parameter layout
// (approximations.py:315-319): theta = [mu (D) | free Cholesky of Sigma (D(D+1)/2)], L = chol with
// exp on the diagonal, z_n = mu + L eps_n.  The estimator is objectives.py:154-164 (entropy form):
//   value  = -(mean_n f(z_n) + 1/2 D (1 + log 2 pi) + sum_i log L_ii)
//   d/dmu  = -mean_n g_n                       g_n = grad f(z_n)
//   d/dL   = -tril(mean_n g_n eps_n')          free diagonal: dL_ii * L_ii - 1
//
// Pipeline (one HIP stream):
//   fr_unpack          theta -> mu, L^T (dense, zeros below the diagonal of L^T)
//   GEMM 1 (MFMA)      Z = E L^T + mu      [N x D x D, triangular k-range]  fused model epilogue
//   model              gauss_diag: G in the GEMM-1 epilogue; funnel: row kernel Z -> G;
//                      gauss_full: GEMM 2 (MFMA)  G = -(Z - m) P
//                      (from D = 1024 and 3 D samples on, folded: G is linear in the noise and is not formed at all --
//                      M = L' P, S = E' E, C = -tril(M' S) - b s', colsum(G) = -s' M - n b'; see fr_route)
//   fr_colsum          column sums of G (-> d/dmu) and sum_n f(z_n), per 128-row block
//   GEMM 3 (MFMA)      C = G^T E           [D x D x N, lower-triangular tiles, split-K]
//   fr_reduce          fixed-order sum of the split-K slabs / row-block partials -> sum vector
//   [RCCL all-reduce of the sum vector when the Monte-Carlo axis is sharded]
//   fr_epilogue        sum vector -> (value, grad) in the flat free-Cholesky layout
//
// Bound: fp64 MFMA (4 N D^2 flop dense convention vs N D 8 bytes: AI ~ D/2 flop/B >> ridge).
#include "vb_gemm_f64.h"
#include "vb_fit.h"

namespace vb {

constexpr double kLog2PiFr = 1.8378770664093454835606594728112;

__device__ __forceinline__ double fr_wave_sum(double x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
  return x;
}

// block-wide sum (256 threads), total returned to every thread
__device__ __forceinline__ double fr_block_sum(double x, double* sh) {
  x = fr_wave_sum(x);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sh[wave] = x;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// ---- unpack ---------------------------------------------------------------------------------------
// Lt[k][j] = L[j][k] (so Lt is upper triangular), row stride ldl; also copies mu.  A transpose of the packed
// triangle: row j of L is contiguous in theta (offset d + j (j + 1) / 2), column j of Lt is strided.  32 x 32 tiles go
// through LDS so that both the reads (along k within a packed row) and the writes (along j within a row of Lt) are
// contiguous 256-B runs; a thread-per-element gather took 10.6 us at D = 1024, this takes a third of it.  grid =
// (tiles over k, tiles over j); block (32, 8).
// copy != nullptr: theta is read ONCE -- it may be mapped host memory -- and every entry is also written to `copy`
// (the device-resident parameter the triangular inverse and the fit kernels read)
__global__ void __launch_bounds__(256) fr_unpack_kernel(const double* __restrict__ theta, int d,
                                                        int64_t ldl, double* __restrict__ Lt,
                                                        double* __restrict__ mu, double* __restrict__ copy = nullptr) {
  __shared__ double tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int k0 = blockIdx.x * 32, j0 = blockIdx.y * 32;
  if (blockIdx.y == 0) {
    const int i = k0 + (int)threadIdx.x;
    if (threadIdx.x < 32 && i < d) {
      const double v = theta[i];
      mu[i] = v;
      if (copy) copy[i] = v;
    }
  }
  if (k0 > j0 + 31) {            // the whole tile lies below the diagonal of Lt (k > j): zeros
#pragma unroll
    for (int r = ty; r < 32; r += 8) {
      const int k = k0 + r, j = j0 + tx;
      if (k < d && j < d) Lt[(int64_t)k * ldl + j] = 0.0;
    }
    return;
  }
#pragma unroll
  for (int r = ty; r < 32; r += 8) {       // read L[j0 + r][k0 + tx]
    const int j = j0 + r, k = k0 + tx;
    double v = 0.0;
    if (j < d && k <= j) {
      v = theta[d + (int64_t)j * (j + 1) / 2 + k];
      if (copy) copy[d + (int64_t)j * (j + 1) / 2 + k] = v;
      if (k == j) v = exp(v);
    }
    tile[r][tx] = v;
  }
  __syncthreads();
#pragma unroll
  for (int r = ty; r < 32; r += 8) {       // write Lt[k0 + r][j0 + tx]
    const int k = k0 + r, j = j0 + tx;
    if (k < d && j < d) Lt[(int64_t)k * ldl + j] = tile[tx][r];
  }
}

// ---- GEMM epilogues ---------------------------------------------------------------------------------
struct EpiStoreZ {          // Z = acc [* rs_n] + mu - shift   (shift = 0, or the target mean for gauss_full)
  double* Z;
  int64_t ldz;
  const double* mu;
  const double* shift;      // may be nullptr
  const double* rs;         // per-row scale (multivariate t: 1 / s_n), may be nullptr
  __device__ void operator()(int, int row, int col, double acc) const {
    if (rs) acc *= rs[row];
    double z = acc + mu[col];
    if (shift) z -= shift[col];
    Z[(int64_t)row * ldz + col] = z;
  }
  __device__ d2v pair(int, int row, int col, double a0, double a1) const {
    if (rs) a0 *= rs[row], a1 *= rs[row];
    const d2v m = *reinterpret_cast<const d2v*>(mu + col);
    d2v z = (d2v){a0 + m.x, a1 + m.y};
    if (shift) {
      const d2v sh = *reinterpret_cast<const d2v*>(shift + col);
      z.x -= sh.x, z.y -= sh.y;
    }
    *reinterpret_cast<d2v*>(Z + (int64_t)row * ldz + col) = z;
    return z;
  }
};

// regression targets (VB_MODEL_LOGISTIC with a VB_GLM_* likelihood): eta = Z X' -> R = dloglik / deta and the
// log-likelihood sum, then G = R X - Z / prior_sd^2 by glm_grad_enqueue (the two GEMMs of vb_logistic.h behind the
// sampling GEMM)
struct EpiGlm {
  double* R;
  int64_t ldr;
  const double* y;
  double* part;
  int link;
  double aux;
  __device__ double operator()(int, int row, int col, double eta) const {
    double dl;
    const double ll = glm_term(link, aux, y[col], eta, &dl);
    R[(int64_t)row * ldr + col] = dl;
    return ll;
  }
};

struct EpiGaussDiag {       // G = -(z - m) / sd^2  straight from the GEMM-1 accumulators
  double* G;
  int64_t ldz;
  const double* mu;
  const double* mean;
  const double* ivar;
  const double* rs;         // per-row scale, may be nullptr
  __device__ void operator()(int, int row, int col, double acc) const {
    if (rs) acc *= rs[row];
    const double dz = acc + mu[col] - mean[col];
    G[(int64_t)row * ldz + col] = -dz * ivar[col];
  }
};

// ... and, per workgroup, the sum of f = -1/2 (z - m)^2 / sd^2 over the tile (the diagonal Gaussian's log density of the
// samples this tile has just formed): with the column sums of G out of the gradient product no pass over G is left
struct EpiGaussDiagF {
  double* G;
  int64_t ldz;
  const double* mu;
  const double* mean;
  const double* ivar;
  double* part;
  __device__ double operator()(int, int row, int col, double acc) const {
    const double dz = acc + mu[col] - mean[col], iv = ivar[col];
    G[(int64_t)row * ldz + col] = -dz * iv;
    return -0.5 * dz * dz * iv;
  }
  __device__ d2v pair(int, int row, int col, double a0, double a1) const {
    const double d0 = a0 + mu[col] - mean[col], d1 = a1 + mu[col + 1] - mean[col + 1];
    const double i0 = ivar[col], i1 = ivar[col + 1];
    *reinterpret_cast<d2v*>(G + (int64_t)row * ldz + col) = (d2v){-d0 * i0, -d1 * i1};
    return (d2v){-0.5 * d0 * d0 * i0, -0.5 * d1 * d1 * i1};
  }
};

struct EpiNegate {          // G = -acc   (gauss_full: G = -(Z - m) P)
  double* G;
  int64_t ldz;
  __device__ void operator()(int, int row, int col, double acc) const {
    G[(int64_t)row * ldz + col] = -acc;
  }
  __device__ d2v pair(int, int row, int col, double a0, double a1) const {
    const d2v v = (d2v){-a0, -a1};
    *reinterpret_cast<d2v*>(G + (int64_t)row * ldz + col) = v;
    return v;
  }
};

struct EpiAccumulate {      // G += acc   (path derivative: the rows of G take the score's L^-T eps)
  double* G;
  int64_t ldz;
  __device__ void operator()(int, int row, int col, double acc) const { G[(int64_t)row * ldz + col] += acc; }
  __device__ d2v pair(int, int row, int col, double a0, double a1) const {
    d2v* p = reinterpret_cast<d2v*>(G + (int64_t)row * ldz + col);
    const d2v v = *p + (d2v){a0, a1};
    *p = v;
    return v;
  }
};

// G = -acc and, per workgroup, the sum of f = 1/2 (z - m)' g over the tile (gauss_full: log p(z) = c0 - 1/2 (z - m)' P
// (z - m) = c0 + 1/2 (z - m)' g): Zc holds z - m, the very rows this workgroup has just multiplied (L2-resident), read
// back with the store's own 16-byte pattern.  The model's log density of the materialised samples, not an identity of
// the variational family.
struct EpiNegateF {
  double* G;
  int64_t ldz;
  const double* Zc;
  double* part;
  __device__ double operator()(int, int row, int col, double acc) const {
    G[(int64_t)row * ldz + col] = -acc;
    return -0.5 * acc * Zc[(int64_t)row * ldz + col];
  }
  __device__ d2v pair(int, int row, int col, double a0, double a1) const {
    const d2v z = *reinterpret_cast<const d2v*>(Zc + (int64_t)row * ldz + col);
    *reinterpret_cast<d2v*>(G + (int64_t)row * ldz + col) = (d2v){-a0, -a1};
    return (d2v){-0.5 * a0 * z.x, -0.5 * a1 * z.y};
  }
};

// C_split[i][j] = acc, and the column sums of G per split through the kernel's EpiColsum hook (the waves of the diagonal
// tiles that have nothing to multiply add up the A tiles in LDS)
struct EpiSplitSlabCs {
  double* C;
  int64_t ldc, slab;
  double* colsum;
  int64_t colsum_ld;
  __device__ void operator()(int split, int row, int col, double acc) const {
    C[split * slab + (int64_t)row * ldc + col] = acc;
  }
  __device__ d2v pair(int split, int row, int col, double a0, double a1) const {
    const d2v v = (d2v){a0, a1};
    *reinterpret_cast<d2v*>(C + split * slab + (int64_t)row * ldc + col) = v;
    return v;
  }
};

// The folded evaluation's gradient product (fr_route): acc = sum_k M[k][row] S[k][col] over the split's k range, and
// C_split[row][col] = -acc - (split 0: b[row] s[col]) -- the slabs add up to C = G' E = -M' S - b s' itself.  Per
// workgroup, the sum of L[row][col] * C_split[row][col] over the tile's entries on or below the diagonal
// (sum (Z - m) o G = sum_{i >= j} L_ij C_ij + (mu - m) . colsum(G)).  L[row][col] is Lt[col][row]: a lane's fragments
// a, a + 1 are adjacent rows, i.e. adjacent doubles of one row of Lt.  No `colsum` member: no column-sum hook runs.
// The waves of the diagonal tiles also store the entries ABOVE the diagonal that their sub-tiles cover: in slab 0 those are
// -b[row] s[col] (plus a partial product), not zeros -- nobody reads them (fr_reduce_packed_kernel takes j <= i only), but
// the slabs of this route must not be read in full.
struct EpiFoldSlabF {
  double* C;
  int64_t ldc, slab;
  const double* b;          // P (mu - m)
  const double* s;          // colsum(E)
  const double* Lt;
  int64_t ldl;
  double* part;
  __device__ double operator()(int split, int row, int col, double acc) const {
    const double v = split == 0 ? -acc - b[row] * s[col] : -acc;
    C[split * slab + (int64_t)row * ldc + col] = v;
    const double l = Lt[(int64_t)col * ldl + row];
    return col <= row ? l * v : 0.0;
  }
  __device__ d2v pair(int split, int row, int col, double a0, double a1) const {
    d2v v = (d2v){-a0, -a1};
    if (split == 0) {
      const double br = b[row];
      const d2v ss = *reinterpret_cast<const d2v*>(s + col);
      v.x -= br * ss.x, v.y -= br * ss.y;
    }
    *reinterpret_cast<d2v*>(C + split * slab + (int64_t)row * ldc + col) = v;
    const double l0 = Lt[(int64_t)col * ldl + row], l1 = Lt[(int64_t)(col + 1) * ldl + row];
    return (d2v){col <= row ? l0 * v.x : 0.0, col + 1 <= row ? l1 * v.y : 0.0};
  }
};

struct EpiSplitSlab {       // C_split[i][j] = acc
  double* C;
  int64_t ldc, slab;
  __device__ void operator()(int split, int row, int col, double acc) const {
    C[split * slab + (int64_t)row * ldc + col] = acc;
  }
  __device__ d2v pair(int split, int row, int col, double a0, double a1) const {
    const d2v v = (d2v){a0, a1};
    *reinterpret_cast<d2v*>(C + split * slab + (int64_t)row * ldc + col) = v;
    return v;
  }
};

}  // namespace vb
#include "vb_fullrank_fused.h"
namespace vb {

// ---- funnel: row kernel Z -> G, f ---------------------------------------------------------------
// one wave per row; G[n][j] = -z_j w (j != k), G[n][k] = -v/tau^2 - (D-1) + w sum_{j != k} z_j^2
// roww != nullptr: the rows of G leave scaled by the sample's weight (AlphaDivergence: no separate pass over G)
__global__ void __launch_bounds__(256) fr_funnel_kernel(const double* __restrict__ Z, double* __restrict__ G,
                                                        int64_t ldz, int64_t n, int d, ModelDev m,
                                                        double* __restrict__ fpart, const double* __restrict__ roww) {
  __shared__ double sh[4];
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  double f = 0.0;
  if (row < n) {
    const double* z = Z + row * ldz;
    double* g = G + row * ldz;
    const double v = z[m.k];
    const double w = exp(-2.0 * v);
    const double rw = roww ? roww[row] : 1.0;
    double ss = 0.0;
    for (int c = lane; c < d; c += 64) {
      if (c == m.k) continue;
      const double zc = z[c];
      const double gc = -zc * w;
      g[c] = roww ? gc * rw : gc;
      ss = fma(zc, zc, ss);
    }
    ss = fr_wave_sum(ss);
    if (lane == 0) {
      const double it2 = 1.0 / (m.tau * m.tau), dm1 = (double)(d - 1);
      const double gk = fma(-v, it2, -dm1) + w * ss;
      g[m.k] = roww ? gk * rw : gk;
      f = v * fma(-0.5 * v, it2, -dm1) - 0.5 * w * ss;
    }
  }
  f = fr_block_sum(f, sh);
  if (threadIdx.x == 0) fpart[blockIdx.x] = f;
}

// ---- column sums of G and sum of f per 128-row block ------------------------------------------------
// grid (ceil(D / 128), ceil(N / 128)); thread (c = t & 63, q = t >> 6) sums rows r0 + q, q + 4, ... of
// the column pair 2c, 2c + 1 (16-B loads, 16 rows in flight); the 4 row groups are combined through LDS in
// fixed order.  Rows are padded to 16 doubles and pad columns of G / Zc are never written with non-finite
// values by the producers, but they are masked anyway.
// fmode 0: no f here, 1: gauss_diag f = -1/2 g^2 / ivar, 2: gauss_full f = 1/2 zc g,
// 3: regression prior f = -1/2 scal zc^2 (the likelihood part comes from the GEMM epilogue)
typedef double fr_d2 __attribute__((ext_vector_type(2)));
__global__ void __launch_bounds__(256) fr_colsum_kernel(const double* __restrict__ G,
                                                        const double* __restrict__ Zc, int64_t ldz,
                                                        int64_t n, int d, int fmode,
                                                        const double* __restrict__ ivar,
                                                        double* __restrict__ colpart,
                                                        double* __restrict__ fpart, double scal = 0.0,
                                                        const double* __restrict__ roww = nullptr,
                                                        int square = 0, double* __restrict__ Gscaled = nullptr,
                                                        const double* __restrict__ rs_out = nullptr) {
  __shared__ double sh[4];
  __shared__ fr_d2 cs[4][64];
  const int c = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int col = blockIdx.x * 128 + 2 * c;
  const int64_t r0 = (int64_t)blockIdx.y * 128;
  const int64_t r1 = r0 + 128 < n ? r0 + 128 : n;
  const bool ok0 = col < d, ok1 = col + 1 < d;
  fr_d2 s = (fr_d2){0.0, 0.0};
  double f = 0.0;
  if (ok0) {
    fr_d2 hiv = (fr_d2){0.0, 0.0};
    if (fmode == 1) hiv = (fr_d2){-0.5 / ivar[col], ok1 ? -0.5 / ivar[col + 1] : 0.0};
    for (int64_t rb = r0 + q; rb < r1; rb += 64) {      // sixteen rows in flight, summed in row order
      // loads first, all of them, from addresses clamped into the block (a load inside `if (r < r1)` next to the
      // write-back below is waited for before the next one is issued: 21 us instead of 12 at 16 384 x 256)
      fr_d2 g[16], z[16];
      double rw[16], rs[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int64_t r = rb + 4 * i < r1 ? rb + 4 * i : r1 - 1;
        g[i] = *reinterpret_cast<const fr_d2*>(G + r * ldz + col);
        z[i] = fmode >= 2 ? *reinterpret_cast<const fr_d2*>(Zc + r * ldz + col) : (fr_d2){0.0, 0.0};
        rw[i] = roww ? roww[r] : 1.0;
        rs[i] = Gscaled ? rs_out[r] : 1.0;
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int64_t r = rb + 4 * i;
        const bool in = r < r1;
        if (roww) g[i] *= rw[i];
        if (square) g[i] *= g[i];
        if (!in) g[i] = (fr_d2){0.0, 0.0}, z[i] = (fr_d2){0.0, 0.0};
        if (!ok1) g[i].y = 0.0, z[i].y = 0.0;
        // the t family's chain rule wants the rows of G scaled by 1 / s_n AFTER these (unscaled) sums: written back
        // from here instead of by a pass of its own
        if (Gscaled && in) *reinterpret_cast<fr_d2*>(Gscaled + r * ldz + col) = g[i] * rs[i];
        s += g[i];
        if (fmode == 1) f = fma(hiv.x * g[i].x, g[i].x, fma(hiv.y * g[i].y, g[i].y, f));
        if (fmode == 2) f = fma(0.5 * z[i].x, g[i].x, fma(0.5 * z[i].y, g[i].y, f));
        if (fmode == 3) f = fma(-0.5 * scal * z[i].x, z[i].x, fma(-0.5 * scal * z[i].y, z[i].y, f));
      }
    }
  }
  cs[q][c] = s;
  __syncthreads();
  if (q == 0 && ok0) {
    const fr_d2 tot = (cs[0][c] + cs[1][c]) + (cs[2][c] + cs[3][c]);
    colpart[(int64_t)blockIdx.y * ldz + col] = tot.x;
    if (ok1) colpart[(int64_t)blockIdx.y * ldz + col + 1] = tot.y;
  }
  f = fr_block_sum(f, sh);
  if (threadIdx.x == 0) fpart[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = f;
}

// ---- folded evaluation: M = L' P, b = P (mu - m), S = E' E, s = colsum(E) and colsum(G) = -s' M - n b' ---------------------
// The correlated-Gaussian target's G is linear in the noise: G = -(E L' + 1 c') P = -E M - 1 b', c = mu - m, M = L' P,
// b = P c -- a D x D x D product that does not depend on the number of samples instead of the N x D x D sampling product
// (and G itself is never formed: fr_route).
// The Gram product of the noise leaves the lower tiles of E' E in `gsplits` slabs (pieces of the sample axis) and one row
// of column sums of E per slab.  fr_fold_msum_team_kernel or fr_fold_msum_kernel, ONE launch behind it, runs four kinds of
// workgroups that do not depend on each other, in this order:
//   [0, nb_m): the M = L' P product on paired row blocks: 64 x 32 tiles, row blocks b and T - 1 - b of a column tile, each
//     over its whole k range.  They follow the parameter alone and are the longest pieces of the launch, so they are
//     dispatched first and the memory-bound blocks behind them take the wave slots they leave free.  While there are fewer
//     than two of them per CU (D = 1024: 256, one per CU) a workgroup is two four-wave teams with two LDS stages each
//     (gemm_f64_dma_team_pair_tiles: two waves per SIMD, half the chain of slab iterations); from two per CU on it is one
//     four-wave team with three stages that runs the two tiles one after the other (gemm_f64_dma_pair_tiles; D = 2048: 1 024
//     workgroups, four per CU).  The rule and its two measurements: gemm_f64_team_pair_plan;
//   the next nb_b, 8 columns each: b[j] = sum_k P[k][j] c[k] (P is symmetric: its column j).  Thread (pair p = t & 3, k
//     group t >> 2) sums its 64th of the k range, sixteen rows per pass, and the groups are combined through LDS in fixed
//     order;
//   the next nb_s: s itself, one thread per column (the gradient product's epilogue reads b and s);
//   the rest, one per 32 x 32 tile (bi, bj <= bi) of S: the slabs added in slab order,
//     the sum written to S[i][j] and, through LDS, to S[j][i] -- both halves from the same sum, so S is exactly
//     symmetric, and both stores are contiguous runs.  Of a diagonal tile only the entries j <= i are read (the product's
//     waves that lie above the diagonal store zeros there).  Only the lower tiles are dispatched; the tile comes from the
//     block index by arithmetic that is uniform over the block, and no thread divides.
// The launch's LDS is the M tiles' stages, dynamic; the other kinds carve their arrays out of the same allocation.
//   One team: three stages, 36.9 KB, four workgroups per CU.  256 threads per block, no launch bound beyond that: bounded to
//     four waves per SIMD the sum code spills; it stays below 128 registers by itself.
//   Two teams: 512 threads per block, and the other kinds remain the 256-thread blocks they are (fr_fold_sum_blocks).  TWO
//     stages per team, 49.2 KB, three workgroups per CU -- an M tile and two of the others: the launch takes 30.6 us at
//     D = 1024; with three stages per team (73.7 KB, an M tile and one other) 31.8; with one team 38.7.
//     110 registers, no scratch.
// colsum(G), which needs M and s and b, is formed by fr_fold_csg_blocks in a later launch; nobody reads it before the reduction.
// Everything is added in a fixed order: the same inputs give the same bits.

// The blocks of b, s and S (`blk` counts from the first of them) in a launch of THREADS threads per block, 256 or 512.  They
// are 256-thread blocks: in the 512-thread launch threads 256 .. 511 read, add and store nothing -- every sum keeps its order
// of additions.  Those threads stay to the block's one barrier instead of ending in front of it, so that the barrier's count is
// the block's size.
template <int THREADS>
__device__ __forceinline__ void fr_fold_sum_blocks(const int blk, double* fold_lds, const double* __restrict__ Spart, int gsplits,
                                                   int64_t slab, int d, int64_t ldl, const double* __restrict__ colpart,
                                                   int64_t ldz, const double* __restrict__ P, int64_t ldp,
                                                   const double* __restrict__ mu, const double* __restrict__ mean, int nb_b,
                                                   int nb_s, double* __restrict__ S, double* __restrict__ svec,
                                                   double* __restrict__ b) {
  static_assert(THREADS == 256 || THREADS == 512, "256 workers, with or without a second idle half");
  const bool worker = THREADS == 256 || threadIdx.x < 256;
  if (blk < nb_b) {
    fr_d2(*part)[4] = reinterpret_cast<fr_d2(*)[4]>(fold_lds);      // [64][4]
    const int p = threadIdx.x & 3, kg = threadIdx.x >> 2;
    const int col = blk * 8 + 2 * p;
    if (worker) {
      const int colc = col < d ? col : 0;                        // (rows of P have an even stride >= d)
      const int kper = (d + 63) / 64;
      const int k0 = kg * kper, k1 = k0 + kper < d ? k0 + kper : d;
      fr_d2 bacc = (fr_d2){0.0, 0.0};
      for (int kb = k0; kb < k1; kb += 16) {      // sixteen rows in flight
        fr_d2 v[16];
        double c[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          const int k = kb + u < k1 ? kb + u : k1 - 1;
          v[u] = *reinterpret_cast<const fr_d2*>(P + (int64_t)k * ldp + colc);
          c[u] = mu[k] - mean[k];
        }
#pragma unroll
        for (int u = 0; u < 16; ++u)
          if (kb + u < k1) bacc += v[u] * c[u];
      }
      part[kg][p] = bacc;
    }
    __syncthreads();
    if (worker && kg == 0) {
      fr_d2 btot = part[0][p];
#pragma unroll 16
      for (int q = 1; q < 64; ++q) btot += part[q][p];
      if (col < d) b[col] = btot.x;
      if (col + 1 < d) b[col + 1] = btot.y;
    }
    return;
  }
  if (blk < nb_b + nb_s) {      // (no barrier in these blocks)
    const int k = (blk - nb_b) * 256 + (int)threadIdx.x;
    if (!worker || k >= ldz) return;
    double s = 0.0;
    if (k < d) {
      s = colpart[k];
      for (int z = 1; z < gsplits; ++z) s += colpart[(int64_t)z * ldz + k];
    }
    svec[k] = s;
    return;
  }
  int bi = 0, bj = blk - nb_b - nb_s;                    // lower tiles only, row by row: tile row bi has bi + 1 of them
  while (bj > bi) bj -= ++bi;                            // (uniform over the block: scalar arithmetic)
  double(*tile)[33] = reinterpret_cast<double(*)[33]>(fold_lds);      // [32][33]
  const int tx = threadIdx.x & 31, ty = (threadIdx.x >> 5) & 7;
  const int i0 = bi * 32, j0 = bj * 32;
  double v[4];
  if (worker) {
    int64_t idx[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = i0 + ty + 8 * q, j = j0 + tx;
      idx[q] = (i < d && j <= i) ? (int64_t)i * ldl + j : 0;      // (not read by the sum: clamped, not predicated)
      v[q] = 0.0;
    }
    for (int zb = 0; zb < gsplits; zb += 8) {      // eight slabs in flight, added in slab order
      double w[8][4];
#pragma unroll
      for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int q = 0; q < 4; ++q) w[u][q] = Spart[(zb + u < gsplits ? zb + u : gsplits - 1) * slab + idx[q]];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (zb + u < gsplits) {
#pragma unroll
          for (int q = 0; q < 4; ++q) v[q] = (zb + u == 0) ? w[u][q] : v[q] + w[u][q];
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) tile[ty + 8 * q][tx] = v[q];
  }
  __syncthreads();
  if (!worker) return;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = ty + 8 * q;
    if (bi == bj) {                // the tile on the diagonal: its upper half is the mirror image of its lower half
      const int i = i0 + r, j = j0 + tx;
      if (i < d && j < d) S[(int64_t)i * ldl + j] = tx <= r ? v[q] : tile[tx][r];
    } else {
      const int i = i0 + r, j = j0 + tx;
      if (i < d && j < d) S[(int64_t)i * ldl + j] = v[q];
      const int it = j0 + r, jt = i0 + tx;      // row of the mirrored tile, its column
      if (it < d && jt < d) S[(int64_t)it * ldl + jt] = tile[tx][r];
    }
  }
}

struct FoldMsumNoDep : GemmNoDep {};      // (a Dep type of this kernel's own: see gemm_f64_dma_pair_tiles)
struct FoldMsumTeamNoDep : GemmNoDep {};
constexpr int kFoldTeamStages = 2;

#define VB_FOLD_MSUM_PARAMS                                                                                                  \
  const GemmArgs gm, const EpiSplitSlab em, int nb_m, const double *__restrict__ Spart, int gsplits, int64_t slab, int d,     \
      int64_t ldl, const double *__restrict__ colpart, int64_t ldz, const double *__restrict__ P, int64_t ldp,                \
      const double *__restrict__ mu, const double *__restrict__ mean, int nb_b, int nb_s, double *__restrict__ S,             \
      double *__restrict__ svec, double *__restrict__ b
#define VB_FOLD_MSUM_SUM_ARGS Spart, gsplits, slab, d, ldl, colpart, ldz, P, ldp, mu, mean, nb_b, nb_s, S, svec, b

// one four-wave team per M workgroup: two or more of them per CU (fr_grad_folded)
__global__ void __launch_bounds__(256) fr_fold_msum_kernel(VB_FOLD_MSUM_PARAMS) {
  extern __shared__ double fold_lds[];      // (the dynamic allocation the tile body calls gemm_lds)
  if ((int)blockIdx.x < nb_m) {
    gemm_f64_dma_pair_tiles<2, 4, 3, EpiSplitSlab, FoldMsumNoDep>(gm, em, FoldMsumNoDep{}, (int)blockIdx.x, nb_m);
    return;
  }
  fr_fold_sum_blocks<256>((int)blockIdx.x - nb_m, fold_lds, VB_FOLD_MSUM_SUM_ARGS);
}

// two four-wave teams per M workgroup: about one of them per CU
__global__ void __launch_bounds__(512) fr_fold_msum_team_kernel(VB_FOLD_MSUM_PARAMS) {
  extern __shared__ double fold_lds[];
  if ((int)blockIdx.x < nb_m) {
    gemm_f64_dma_team_pair_tiles<2, 4, kFoldTeamStages, EpiSplitSlab, FoldMsumTeamNoDep>(gm, em, FoldMsumTeamNoDep{},
                                                                                         (int)blockIdx.x);
    return;
  }
  fr_fold_sum_blocks<512>((int)blockIdx.x - nb_m, fold_lds, VB_FOLD_MSUM_SUM_ARGS);
}
#undef VB_FOLD_MSUM_PARAMS
#undef VB_FOLD_MSUM_SUM_ARGS

// colsum(G)[j] = -sum_k s[k] M[k][j] - n b[j], eight columns per block `blk`: the arithmetic the b blocks above use, with
// s[k] added up from the rows of `colpart` in row order by the thread that needs it and b[j] read from the vector an
// earlier launch wrote.  `part`: 64 x 4 pairs of LDS.  M, s and b are complete when this runs (earlier launches), and only
// the reduction reads the result.
template <int U>
__device__ __forceinline__ void fr_fold_csg_blocks(const int blk, fr_d2 (*part)[4], const double* __restrict__ colpart,
                                                   int gsplits, int64_t ldz, int d, const double* __restrict__ M,
                                                   const double* __restrict__ b, double n_rows, double* __restrict__ csg) {
  const int p = threadIdx.x & 3, kg = threadIdx.x >> 2;
  const int col = blk * 8 + 2 * p;
  const int colc = col < d ? col : 0;                        // (rows of M have an even stride >= d)
  const int kper = (d + 63) / 64;
  const int k0 = kg * kper, k1 = k0 + kper < d ? k0 + kper : d;
  fr_d2 acc = (fr_d2){0.0, 0.0};
  for (int kb = k0; kb < k1; kb += U) {      // U rows in flight (the sums do not depend on U: every thread adds in k order)
    fr_d2 v[U];
    double c[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = kb + u < k1 ? kb + u : k1 - 1;
      v[u] = *reinterpret_cast<const fr_d2*>(M + (int64_t)k * ldz + colc);
      c[u] = colpart[k];
    }
    for (int z = 1; z < gsplits; ++z)
#pragma unroll
      for (int u = 0; u < U; ++u) c[u] += colpart[(int64_t)z * ldz + (kb + u < k1 ? kb + u : k1 - 1)];
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (kb + u < k1) acc += v[u] * c[u];
  }
  part[kg][p] = acc;
  __syncthreads();
  if (kg == 0) {
    fr_d2 tot = part[0][p];
#pragma unroll 16
    for (int q = 1; q < 64; ++q) tot += part[q][p];
    if (col < d) csg[col] = -tot.x - n_rows * b[col];
    if (col + 1 < d) csg[col + 1] = -tot.y - n_rows * b[col + 1];
  }
}

__global__ void __launch_bounds__(256) fr_fold_csg_kernel(const double* __restrict__ colpart, int gsplits, int64_t ldz, int d,
                                                          const double* __restrict__ M, const double* __restrict__ b,
                                                          double n_rows, double* __restrict__ csg) {
  __shared__ fr_d2 part[64][4];
  fr_fold_csg_blocks<16>((int)blockIdx.x, part, colpart, gsplits, ldz, d, M, b, n_rows, csg);
}

// The same blocks behind the tiles of the C product in ONE launch, for the tile the route takes while the product fits the
// chip at once (cfgc 4: 64 x 64, two LDS stages; D = 1024: 544 of 1 024 slots): block x < nb_tiles is tile x % gx of split
// x / gx -- the linear order of the launcher's (gx, 1, splits) grid -- and the blocks behind take the free slots.  Neither
// kind reads what the other writes.  `part` is carved out of the tiles' dynamic LDS, and a thread keeps eight rows in flight:
// with sixteen the kernel needs scratch under the tile's bound of four workgroups per CU.
struct FoldCsgNoDep : GemmNoDep {};      // (a Dep type of this kernel's own: see gemm_f64_dma_team_pair_tiles)

__global__ void __launch_bounds__(256, 4) fr_fold_ctile_csg_kernel(const GemmArgs g, const EpiFoldSlabF epi, int gx, int nb_tiles,
                                                                   const double* __restrict__ colpart, int gsplits, int64_t ldz,
                                                                   int d, const double* __restrict__ M,
                                                                   const double* __restrict__ b, double n_rows,
                                                                   double* __restrict__ csg) {
  if ((int)blockIdx.x < nb_tiles) {
    const int bz = (int)blockIdx.x / gx, bx = (int)blockIdx.x - bz * gx;
    gemm_f64_dma_tile<false, 2, 8, 2, EpiFoldSlabF, FoldCsgNoDep>(g, epi, FoldCsgNoDep{}, bx, bz, gx);
    return;
  }
  extern __shared__ double fold_lds[];
  fr_fold_csg_blocks<8>((int)blockIdx.x - nb_tiles, reinterpret_cast<fr_d2(*)[4]>(fold_lds), colpart, gsplits, ldz, d, M, b,
                        n_rows, csg);
}

// k splits of the folded gradient product C = -tril(M' S) - b s' (K = D, lower 64 x 64 tiles): pieces of about sixteen
// slabs, as the M product's, and no more of them than fill the chip's four workgroups per CU once -- no second round
// (D = 1024: 4 pieces, 544 workgroups).  The rule is MEASURED AT THE HEADLINE SHAPE ONLY (D = 1024): 128 x 64
// tiles in 7 pieces of ten slabs 35.3 us for the product and 9.7 us for the reduction of its slabs, this 34.4 and 8.0; 2
// or 4 pieces of 128 x 64 tiles and 8 pieces of either tile were 6 to 12 us slower per evaluation.  For larger D it is an
// extrapolation nobody has timed: D = 2048 gets one piece (528 workgroups of 128 slabs on 1 024 slots), D >= ~2 900 the
// unsplit 128 x 64 or three-stage 64 x 64 tiles of fr_route.  `max_splits` does not bind at the shapes inside the gate (D = 1024: 4 of
// 8 slabs, D = 2048: 1 of 2 -- both counts follow the CUs per lower tile): it is there for a gate that moves.
static int fr_fold_csplits(int d, int n_cu, int max_splits) {
  const GemmArgs sc = gemm_product(nullptr, 0, nullptr, 0, d, d, d, 2);
  const long tiles = gemm_count_blocks(sc, 64, 64);
  int s = d / (16 * kGemmBK);
  if ((long)s * tiles > 4L * n_cu) s = (int)(4L * n_cu / tiles);
  if (s > max_splits) s = max_splits;      // (the slabs of C take the place of the Gram product's)
  if (s > 16) s = 16;                      // (the reduction keeps sixteen slabs in flight)
  return s < 1 ? 1 : s;
}

// ---- reduce: split-K slabs, row-block partials -> sum vector ------------------------------------------
// sum vector layout: [F | colsum (ldz) | C (d x ldl)], F at index 0, colsum from 16, C from 16 + ldz

// One thread per pair of adjacent C entries (16-B loads, CHUNK split slabs in flight, summed in slab order); entries above
// the diagonal are not computed by the GEMM and are written as zero.
// Round 6: the three reductions have workgroups of their own -- blocks [0, nb_c) the C pairs, the next ceil(ldz / 256) the
// column sums, the last one the scalars -- where block 0 used to do all three one after the other (at D = 256 with 64 slabs
// and 128 row blocks: ten dependent round trips in one workgroup, 10.6 us for 21 MB); CHUNK = 64 for launches that leave
// the SIMDs a wave or two each anyway (the registers cost nothing there: every slab's load in flight at once).  The sums are
// formed in the same order as before: the same bits.
template <int CHUNK>
__global__ void __launch_bounds__(256) fr_reduce_kernel(const double* __restrict__ Cpart, int splits,
                                                        int64_t slab, int d, int64_t ldl,
                                                        const double* __restrict__ colpart, int n_rb,
                                                        int64_t ldz, const double* __restrict__ fpart,
                                                        int n_fpart, FrSums S, int full,
                                                        const double* __restrict__ wpart, int nb_c) {
  __shared__ double sh[4];
  const int nb_col = (int)((ldz + 255) / 256);
  if ((int)blockIdx.x < nb_c) {
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t idx = 2 * tid;
    const int64_t nC = (int64_t)d * ldl;
    if (idx >= nC) return;
    const int i = (int)(idx / ldl), j = (int)(idx % ldl);
    fr_d2 s = (fr_d2){0.0, 0.0};
    if (full == 1 || j <= i) {
      for (int k0 = 0; k0 < splits; k0 += CHUNK) {
        fr_d2 v[CHUNK];
#pragma unroll
        for (int u = 0; u < CHUNK; ++u)      // (clamped, not predicated: no load behind a branch; the surplus is not added)
          v[u] = *reinterpret_cast<const fr_d2*>(Cpart + (k0 + u < splits ? k0 + u : splits - 1) * slab + idx);
#pragma unroll
        for (int u = 0; u < CHUNK; ++u)
          if (k0 + u < splits) s += v[u];
      }
      if (full != 1 && j + 1 > i) s.y = 0.0;
    }
    if (full == 2) {
      // mirrored: the symmetric matrix given by its lower triangle, both halves written here (entry (i, j <= i) and its
      // image (j, i) by the thread that owns the lower one; the upper entries' own threads write nothing) -- the caller
      // multiplies by it next and needs no symmetrising pass
      double* C = S.sums + S.off_c;
      if (j < d && j <= i) {
        C[idx] = s.x;
        if (j < i) C[(int64_t)j * ldl + i] = s.x;
      } else if (j >= d) {
        C[idx] = 0.0;
      }
      if (j + 1 < d && j + 1 <= i) {
        C[idx + 1] = s.y;
        if (j + 1 < i) C[(int64_t)(j + 1) * ldl + i] = s.y;
      } else if (j + 1 >= d) {
        C[idx + 1] = 0.0;
      }
    } else {
      *reinterpret_cast<fr_d2*>(S.sums + S.off_c + idx) = s;
    }
    return;
  }
  if ((int)blockIdx.x < nb_c + nb_col) {
    const int64_t tid = (int64_t)((int)blockIdx.x - nb_c) * 256 + threadIdx.x;
    if (tid >= ldz) return;
    double s = 0.0;
    if (tid < d) {
      for (int rb0 = 0; rb0 < n_rb; rb0 += 32) {      // 32 loads in flight (16 until round 5), summed in row-block order
        double v[32];
#pragma unroll
        for (int u = 0; u < 32; ++u) v[u] = rb0 + u < n_rb ? colpart[(int64_t)(rb0 + u) * ldz + tid] : 0.0;
#pragma unroll
        for (int u = 0; u < 32; ++u) s += v[u];
      }
    }
    S.sums[S.off_col + tid] = s;
    return;
  }
  double f = 0.0;
  for (int e = threadIdx.x; e < n_fpart; e += 256) f += fpart[e];
  f = fr_block_sum(f, sh);
  if (threadIdx.x == 0) S.sums[0] = f;
  if (wpart) {      // two more scalars given as per-row-block partials (wpart[q n_rb + rb]) -> sums[1], sums[2]
    for (int q = 0; q < 2; ++q) {
      double t = 0.0;
      for (int e = threadIdx.x; e < n_rb; e += 256) t += wpart[(int64_t)q * n_rb + e];
      t = fr_block_sum(t, sh);
      if (threadIdx.x == 0) S.sums[1 + q] = t;
    }
  }
}

// (both launch sites: the C pairs' blocks, the column sums' blocks, one block of scalars)
static void fr_reduce_launch(vb_ctx* ctx, hipStream_t st, const double* Cpart, int splits, int64_t slab, int d, int64_t ldl,
                             const double* colpart, int n_rb, int64_t ldz, const double* fpart, int n_fpart, FrSums S, int full,
                             const double* wpart) {
  const int nb_c = (int)((slab / 2 + 255) / 256), nb_col = (int)((ldz + 255) / 256);
  const dim3 grid((unsigned)(nb_c + nb_col + 1));
  if (splits > 16 && nb_c <= 2 * ctx->prop.multiProcessorCount)
    hipLaunchKernelGGL(fr_reduce_kernel<64>, grid, dim3(256), 0, st, Cpart, splits, slab, d, ldl, colpart, n_rb, ldz, fpart, n_fpart,
                       S, full, wpart, nb_c);
  else
    hipLaunchKernelGGL(fr_reduce_kernel<16>, grid, dim3(256), 0, st, Cpart, splits, slab, d, ldl, colpart, n_rb, ldz, fpart, n_fpart,
                       S, full, wpart, nb_c);
}

// ---- full-rank Gaussian: split reduction straight into the flat (paragami) layout -----------------------
// Same pair-per-thread reduction as fr_reduce_kernel (same summation order), but entry (i, j <= i) lands at the
// packed position i (i + 1) / 2 + j -- the order of the free-Cholesky block of theta -- so a sharded job
// all-reduces D (D + 1) / 2 doubles instead of D x ldl, and entries above the diagonal are never written.
// FUSE (no communicator): the O(P) epilogue arithmetic is applied on the spot and `out` = [value | grad] is
// written directly; otherwise the raw sums go to S for the all-reduce and fr_epilogue_packed_kernel finishes.
template <bool FUSE>
__global__ void __launch_bounds__(256) fr_reduce_packed_kernel(
    const double* __restrict__ Cpart, int splits, int64_t slab, int d, int64_t ldl,
    const double* __restrict__ colpart, int n_rb, int64_t ldz, const double* __restrict__ fpart, int n_fpart,
    FrSums S, const double* __restrict__ theta, double n_local_w, double n_total, double c0,
    double* __restrict__ out, int pd, FrWeighted wm, const double* __restrict__ fold_mu,
    const double* __restrict__ fold_mean) {
  const double ent = pd ? 0.0 : 1.0;      // the entropy's -1 on the free diagonal (absent with the path derivative)
  // weighted mode (AlphaDivergence, objectives.py:458-460): the rows of G carried the weights s_n, the result is
  // scale * [sum s g | tril(sum s g eps') with the free diagonal x L_ii + sum s], the value comes from wm.value
  const bool weighted = wm.scale != 0.0;
  const double wsum = weighted ? wm.wsum[0] : 0.0;
  // folded evaluation (fold_mu != nullptr): block 0 does the scalar tail only -- it walks the column sums once more --
  // and the blocks behind it take the entries (one block more in the grid)
  const int64_t tid = ((int64_t)blockIdx.x - (fold_mu ? 1 : 0)) * 256 + threadIdx.x;
  const int64_t idx = 2 * tid;
  const int64_t nC = (int64_t)d * ldl;
  const double invN = 1.0 / n_total;
  if (tid >= 0 && idx < nC) {
    const int i = (int)(idx / ldl), j = (int)(idx % ldl);
    if (j <= i) {
      fr_d2 s = (fr_d2){0.0, 0.0};
      for (int k0 = 0; k0 < splits; k0 += 16) {      // sixteen slabs in flight (eight until round 5), added in slab order
        fr_d2 v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u)
          v[u] = k0 + u < splits ? *reinterpret_cast<const fr_d2*>(Cpart + (k0 + u) * slab + idx) : (fr_d2){0.0, 0.0};
#pragma unroll
        for (int u = 0; u < 16; ++u) s += v[u];
      }
      const int64_t p = (int64_t)i * (i + 1) / 2 + j;
      if (FUSE && weighted) {
        double g0 = s.x;
        if (j == i) g0 = g0 * exp(theta[d + p]) + wsum;
        out[1 + d + p] = wm.scale * g0;
        if (j + 1 <= i) {
          double g1 = s.y;
          if (j + 1 == i) g1 = g1 * exp(theta[d + p + 1]) + wsum;
          out[1 + d + p + 1] = wm.scale * g1;
        }
      } else if (FUSE) {
        double g0 = -s.x * invN;
        if (j == i) g0 = g0 * exp(theta[d + p]) - ent;              // free (log) diagonal + entropy
        out[1 + d + p] = g0;
        if (j + 1 <= i) {
          double g1 = -s.y * invN;
          if (j + 1 == i) g1 = g1 * exp(theta[d + p + 1]) - ent;
          out[1 + d + p + 1] = g1;
        }
      } else {
        S.sums[S.off_c + p] = s.x;
        if (j + 1 <= i) S.sums[S.off_c + p + 1] = s.y;
      }
    }
  }
  if (tid >= 0 && tid < ldz) {
    double s = 0.0;
    if (tid < d) {
      for (int rb0 = 0; rb0 < n_rb; rb0 += 32) {      // 32 loads in flight (16 until round 5), summed in row-block order
        double v[32];
#pragma unroll
        for (int u = 0; u < 32; ++u) v[u] = rb0 + u < n_rb ? colpart[(int64_t)(rb0 + u) * ldz + tid] : 0.0;
#pragma unroll
        for (int u = 0; u < 32; ++u) s += v[u];
      }
    }
    if (FUSE) {
      if (tid < d) out[1 + tid] = weighted ? wm.scale * s : -s * invN;
    } else {
      S.sums[S.off_col + tid] = s;
    }
  }
  if (blockIdx.x == 0) {
    // The scalar tail: sum of the f partials and sum of the log-diagonal.  One workgroup, so it is written for
    // latency: every load of a pass is requested before anything is summed, and the block sums share one pair of
    // barriers.
    const int tx = threadIdx.x;
    double f = 0.0, t = 0.0;
    for (int e0 = 0; e0 < n_fpart; e0 += 4 * 256) {
      double v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = e0 + u * 256 + tx;
        v[u] = e < n_fpart ? fpart[e] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) f += v[u];
    }
    for (int c0 = 0; c0 < d; c0 += 4 * 256) {
      double dg[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int c = c0 + u * 256 + tx, cc = c < d ? c : 0;
        dg[u] = FUSE ? theta[d + (int64_t)cc * (cc + 1) / 2 + cc] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (c0 + u * 256 + tx < d) t += dg[u];
    }
    // folded evaluation (fold_mu != nullptr): the partials are sum L o tril(C) per tile and split of the gradient
    // product, and sum f = 1/2 (their sum + (mu - m) . colsum(G)); the column sums are formed here once more, in the
    // same row-block order as by the threads that write the gradient
    double dot = 0.0;
    if (fold_mu) {
      for (int c0 = 0; c0 < d; c0 += 4 * 256) {      // four columns per thread and pass, every load requested first
        double s[4] = {0.0, 0.0, 0.0, 0.0}, cc[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int c = c0 + q * 256 + tx, cl = c < d ? c : d - 1;
          cc[q] = c < d ? fold_mu[cl] - fold_mean[cl] : 0.0;
        }
        for (int rb0 = 0; rb0 < n_rb; rb0 += 8) {
          double v[4][8];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int c = c0 + q * 256 + tx, cl = c < d ? c : d - 1;
#pragma unroll
            for (int u = 0; u < 8; ++u) v[q][u] = colpart[(int64_t)(rb0 + u < n_rb ? rb0 + u : n_rb - 1) * ldz + cl];
          }
#pragma unroll
          for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int u = 0; u < 8; ++u)
              if (rb0 + u < n_rb) s[q] += v[q][u];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) dot += cc[q] * s[q];
      }
    }
    __shared__ double sh3[12];
    f = fr_wave_sum(f), t = fr_wave_sum(t), dot = fr_wave_sum(dot);
    if ((tx & 63) == 0) sh3[tx >> 6] = f, sh3[4 + (tx >> 6)] = t, sh3[8 + (tx >> 6)] = dot;
    __syncthreads();
    if (tx == 0) {
      f = (sh3[0] + sh3[1]) + (sh3[2] + sh3[3]);
      if (fold_mu) f = 0.5 * (f + ((sh3[8] + sh3[9]) + (sh3[10] + sh3[11])));
      const double sum_logdiag = (sh3[4] + sh3[5]) + (sh3[6] + sh3[7]);
      if (FUSE) {
        const double F = f + n_local_w * c0;
        const double half_sq = pd ? 0.5 * S.sums[1] * invN : 0.5 * d;    // 1/2 mean ||eps||^2 or its expectation
        const double H = half_sq + 0.5 * d * kLog2PiFr + sum_logdiag;
        out[0] = weighted ? wm.value[0] : -(F * invN + H);
      } else {
        S.sums[0] = f;
      }
    }
  }
}

// epilogue of the sharded job: all-reduced packed sums -> (value, grad)
__global__ void __launch_bounds__(256) fr_epilogue_packed_kernel(FrSums S, const double* __restrict__ theta,
                                                                 int d, double n_local_w, double n_total,
                                                                 double c0, double* __restrict__ out, int pd,
                                                                 FrWeighted wm) {
  __shared__ double sh[4];
  const int64_t np = (int64_t)d * (d + 1) / 2;
  const double invN = 1.0 / n_total;
  // grid-stride: under the overlapped schedule the kernel runs beside the next evaluation's sampling product and is
  // launched with a few dozen workgroups, so that it takes a few slots for a little longer instead of streaming two
  // thousand workgroups through the dispatcher between the product's tiles (which cost that product 18 us)
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < np; p += (int64_t)gridDim.x * 256) {
    int i = (int)((sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
    while ((int64_t)(i + 1) * (i + 2) / 2 <= p) ++i;
    while ((int64_t)i * (i + 1) / 2 > p) --i;
    const bool diag = p == (int64_t)i * (i + 1) / 2 + i;
    if (wm.scale != 0.0) {
      double g = S.sums[S.off_c + p];
      if (diag) g = g * exp(theta[d + p]) + wm.wsum[0];
      out[1 + d + p] = wm.scale * g;
    } else {
      double g = -S.sums[S.off_c + p] * invN;                       // d value / d L_ij
      if (diag) g = g * exp(theta[d + p]) - (pd ? 0.0 : 1.0);
      out[1 + d + p] = g;
    }
  }
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < d; p += (int64_t)gridDim.x * 256)
    out[1 + p] = wm.scale != 0.0 ? wm.scale * S.sums[S.off_col + p] : -S.sums[S.off_col + p] * invN;
  if (blockIdx.x == 0) {
    double t = 0.0;
    for (int i = threadIdx.x; i < d; i += 256) t += theta[d + (int64_t)i * (i + 1) / 2 + i];
    const double sum_logdiag = fr_block_sum(t, sh);
    if (threadIdx.x == 0) {
      const double F = S.sums[0] + n_local_w * c0;
      const double half_sq = pd ? 0.5 * S.sums[1] * invN : 0.5 * d;
      const double H = half_sq + 0.5 * d * kLog2PiFr + sum_logdiag;
      out[0] = wm.scale != 0.0 ? wm.value[0] : -(F * invN + H);
    }
  }
}

// G[n][:] *= rs[n]  (multivariate t: the Gram GEMM then yields sum_n g_n (z_n / s_n)')
__global__ void __launch_bounds__(256) fr_rowscale_kernel(double* __restrict__ G, int64_t ldz, int64_t n, int d,
                                                          const double* __restrict__ rs) {
  const int64_t row = blockIdx.x;            // rows on x: gridDim.y stops at 65 535
  const int c = blockIdx.y * 256 + threadIdx.x;
  if (c < d) G[row * ldz + c] *= rs[row];
}

// ---- path derivative ("sticking the landing", objectives.py:156-159) for the dense Gaussian ----------------
// value = -mean(f(z) - log q(z; stop(theta))): the score -dlog q/dz = L^-T eps is added to the model gradient row by
// row, G~ = G + E L^-1 (one N x D x D / 2 product, fr_score), and the sums of G~ are the entropy form's sums
// without the entropy term; value: 1/2 sum ||eps_n||^2 / N replaces D / 2.  L^-1 = ((L')^-1)' is formed explicitly
// (blocked recursive inversion, see fr_triinv_leaf_kernel and the host loop, then a transposition).  Rounds 2-3 went
// through the noise Gram matrix (C' = C + L^-T sum eps eps'): the same N x D^2 flops for the Gram product plus a
// D x D x D product and a second column pass.
struct EpiStoreD {          // C_z = sign * acc   (z: product index of a batched launch)
  double* C;
  int64_t ld;
  double sign;
  int64_t batch_c;
  __device__ void operator()(int z, int row, int col, double acc) const {
    C[z * batch_c + (int64_t)row * ld + col] = sign * acc;
  }
};

// Inverse of the diagonal blocks of U = L' (rows / columns [s, s + kTriLeaf)): one WAVE per column j of a block's
// inverse, column-oriented back substitution.  Lane r keeps the running sum p_r = sum_{k > i} U[r][k] x_k of "its"
// rows r and r + 64 in registers; step i reads p_i with v_readlane (i is wave-uniform), forms
// x_i = (delta_ij - p_i) / U_ii and adds U[r][i] x_i to every p_r, r < i.  U[.][i] is row i of L -- contiguous in
// the packed parameter; the four waves of a workgroup work on four columns of the same block and first stage the
// block's rows in LDS (128 KB, all loads in flight at once), so the dependent chain per step is a readlane, a
// subtract, a multiply and an FMA fed from LDS.  The D columns of all blocks run in parallel.
constexpr int kTriLeaf = 128;
__device__ __forceinline__ double fr_readlane(double v, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}
__global__ void __launch_bounds__(256) fr_triinv_leaf_kernel(const double* __restrict__ theta,
                                                             const double* __restrict__ U, int d, int64_t ld,
                                                             double* __restrict__ X) {
  extern __shared__ double ls[];                            // ls[i * kTriLeaf + r] = L[s + i][s + r], r < i, else 0
  const int lane = threadIdx.x & 63;
  const int c0 = blockIdx.x * 4;                            // first of the workgroup's four columns
  const int s = c0 / kTriLeaf * kTriLeaf;
  const int jmax = (c0 + 3 < d ? c0 + 3 : d - 1) - s;       // last row any of the four waves needs
  // staging: batches of 16 unconditional loads per thread (addresses clamped into the row, the value selected
  // afterwards) -- written as `r < i ? theta[..] : 0` the compiler branched around each load and waited for it
  // before the next one: 64 dependent round trips, 20 of the kernel's 27 us at D = 256
  const int total = (jmax + 1) * kTriLeaf;
  for (int e0 = threadIdx.x; e0 < total; e0 += 256 * 16) {
    double v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int e = e0 + 256 * k < total ? e0 + 256 * k : total - 1;
      const int i = e / kTriLeaf, r = e % kTriLeaf;
      const int64_t gi = s + i;
      v[k] = theta[d + gi * (gi + 1) / 2 + s + (r < i ? r : 0)];
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int e = e0 + 256 * k;
      if (e < total) ls[e] = (e % kTriLeaf) < (e / kTriLeaf) ? v[k] : 0.0;
    }
  }
  __syncthreads();
  const int c = __builtin_amdgcn_readfirstlane(c0 + (threadIdx.x >> 6));   // this wave's column
  if (c >= d) return;
  const int j = c - s;
  double p0 = 0.0, p1 = 0.0, x0 = 0.0, x1 = 0.0;            // rows lane, lane + 64 of the block
  // 1 / U_ii of "its" rows, computed by all lanes at once and read with v_readlane in the loop
  double q0 = 1.0, q1 = 1.0;
  if (lane <= j) q0 = 1.0 / U[(int64_t)(s + lane) * ld + s + lane];
  if (lane + 64 <= j) q1 = 1.0 / U[(int64_t)(s + lane + 64) * ld + s + lane + 64];
  // two straight-line phases (no per-step selects): pivots in rows >= 64 touch both register slots, pivots in
  // rows < 64 only the first (rows >= 64 lie below them: L[s + i][s + r] = 0 for r >= i).  The row of the NEXT step
  // is read from LDS while this step's chain (readlane, subtract, multiply, FMA) runs.
  int i = j;
  double l0 = ls[i * kTriLeaf + lane], l1 = ls[i * kTriLeaf + lane + 64];
  for (; i >= 64; --i) {
    const int in = i > 0 ? i - 1 : 0;
    const double l0n = ls[in * kTriLeaf + lane], l1n = ls[in * kTriLeaf + lane + 64];
    const double xi = ((i == j ? 1.0 : 0.0) - fr_readlane(p1, i - 64)) * fr_readlane(q1, i - 64);
    if (lane + 64 == i) x1 = xi;
    p0 = fma(l0, xi, p0);
    p1 = fma(l1, xi, p1);
    l0 = l0n;
    l1 = l1n;
  }
  for (; i >= 0; --i) {
    const int in = i > 0 ? i - 1 : 0;
    const double l0n = ls[in * kTriLeaf + lane];
    const double xi = ((i == j ? 1.0 : 0.0) - fr_readlane(p0, i)) * fr_readlane(q0, i);
    if (lane == i) x0 = xi;
    p0 = fma(l0, xi, p0);
    l0 = l0n;
  }
  double* Xb = X + (int64_t)s * ld + s;
  if (lane <= j) Xb[(int64_t)lane * ld + j] = x0;
  if (lane + 64 <= j) Xb[(int64_t)(lane + 64) * ld + j] = x1;
}

// out[j][i] = in[i][j] for a d x d matrix (row stride ld both sides), 32 x 32 tiles through LDS
__global__ void __launch_bounds__(256) fr_transpose_kernel(const double* __restrict__ in, double* __restrict__ out, int d,
                                                           int64_t ld) {
  __shared__ double tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int i0 = blockIdx.y * 32, j0 = blockIdx.x * 32;
  for (int r = ty; r < 32; r += 8) {
    const int i = i0 + r, j = j0 + tx;
    tile[r][tx] = (i < d && j < d) ? in[(int64_t)i * ld + j] : 0.0;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int j = j0 + r, i = i0 + tx;
    if (i < d && j < d) out[(int64_t)j * ld + i] = tile[tx][r];
  }
}

// sum of squares of the n x d noise matrix: one partial per workgroup (rows strided over the grid), summed in a fixed
// order by fr_sumsq_final_kernel
__global__ void __launch_bounds__(256) fr_sumsq_kernel(const double* __restrict__ E, int64_t ld, int64_t n, int d,
                                                       double* __restrict__ part) {
  __shared__ double sh[4];
  double s = 0.0;
  for (int64_t r = blockIdx.x; r < n; r += gridDim.x) {
    const double* e = E + r * ld;
    for (int c = 2 * threadIdx.x; c < d; c += 512) {
      const fr_d2 v = *reinterpret_cast<const fr_d2*>(e + c);
      s = fma(v.x, v.x, s);
      if (c + 1 < d) s = fma(v.y, v.y, s);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
__global__ void __launch_bounds__(256) fr_sumsq_final_kernel(const double* __restrict__ part, int count,
                                                             double* __restrict__ out) {
  __shared__ double sh[4];
  double s = 0.0;
  for (int i = threadIdx.x; i < count; i += 256) s += part[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// theta -> mu, L' (dense, row stride ldl) on stream st
int fr_unpack_enqueue(vb_ctx* ctx, hipStream_t st, const double* theta_dev, int D, int64_t ldl, double* Lt, double* mu,
                      double* theta_copy) {
  hipLaunchKernelGGL(fr_unpack_kernel, dim3((unsigned)((D + 31) / 32), (unsigned)((D + 31) / 32)), dim3(256), 0, st,
                     theta_dev, D, ldl, Lt, mu, theta_copy);
  VB_HIP(ctx, hipGetLastError());
  return VB_OK;
}

// ---- optimiser step + unpack in one kernel (vb_fit, dense family) --------------------------------------------------------
// The loop used to run fit_step_kernel (5.9 us at D = 1024) and, at the top of the next evaluation, fr_unpack_kernel
// (6.6 us) on the parameter it had just written.  Same tiling as the unpack: a 32 x 32 tile of the packed triangle is
// read along its rows -- here together with the gradient entry and the optimiser state of each element -- stepped
// (fit_step_apply: numpy's operation order, no contraction, so the trajectory stays the host loop's bit for bit),
// written back, and transposed through LDS into L'.  Tiles below the diagonal of L' hold zeros from the first
// evaluation's full unpack and are not touched again.
__global__ void __launch_bounds__(256) fr_step_unpack_kernel(FitStep a, int d, int64_t ldl, double* __restrict__ Lt,
                                                             double* __restrict__ mu) {
  __shared__ double tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int k0 = blockIdx.x * 32, j0 = blockIdx.y * 32;
  if (blockIdx.y == 0) {
    const int i = k0 + (int)threadIdx.x;
    if (threadIdx.x < 32 && i < d) {
      double s1, s2, th;
      fit_step_load(a, i, &s1, &s2, &th);
      mu[i] = fit_step_apply_vals(a, i, a.out[1 + i], s1, s2, th);
    }
    if (blockIdx.x == 0 && threadIdx.x == 32) a.values[a.k] = a.out[0];
  }
  if (k0 > j0 + 31) return;            // below the diagonal of L' (k > j): no parameter lives here
#pragma unroll
  for (int r = ty; r < 32; r += 8) {       // L[j0 + r][k0 + tx]
    const int j = j0 + r, k = k0 + tx;
    double v = 0.0;
    if (j < d && k <= j) {
      const int64_t p = d + (int64_t)j * (j + 1) / 2 + k;
      double s1, s2, th;
      fit_step_load(a, p, &s1, &s2, &th);
      v = fit_step_apply_vals(a, p, a.out[1 + p], s1, s2, th);
      if (k == j) v = exp(v);
    }
    tile[r][tx] = v;
  }
  __syncthreads();
#pragma unroll
  for (int r = ty; r < 32; r += 8) {       // L'[k0 + r][j0 + tx]
    const int k = k0 + r, j = j0 + tx;
    if (k < d && j < d && k <= j) Lt[(int64_t)k * ldl + j] = tile[tx][r];
  }
}

int fr_step_unpack_enqueue(vb_ctx* ctx, const FitStep& a, int64_t d) {
  const int64_t ldl = round_up(d, 16);
  if (!ctx->fr_lt.ptr || ctx->fr_lt.bytes < (size_t)(ldl + d * ldl) * sizeof(double))
    return fail(ctx, VB_ERR_STATE, "no unpacked parameter buffer (the first evaluation makes it)");
  double* mu = (double*)ctx->fr_lt.ptr;
  hipLaunchKernelGGL(fr_step_unpack_kernel, dim3((unsigned)((d + 31) / 32), (unsigned)((d + 31) / 32)), dim3(256), 0,
                     ctx->stream, a, (int)d, ldl, mu + ldl, mu);
  VB_HIP(ctx, hipGetLastError());
  ctx->fr_lt_owner = a.theta;
  ctx->fr_lt_d = d;
  return VB_OK;
}

// Xa = (L')^-1 = U^-1 (upper triangular, row stride ldl) by recursive doubling: diagonal blocks of kTriLeaf rows are
// inverted by back substitution (one wave per column), then [[A, B], [0, C]]^-1 = [[A^-1, -A^-1 B C^-1], [0, C^-1]]
// level by level -- two batched GEMMs per level, D^3 / 3 flops in all instead of a triangular solve.  T: D x ldl scratch.
// clean == true: the caller vouches that Xa's strictly lower triangle still holds the zeros of an earlier call on the same
// buffer and layout (nothing here ever writes below the diagonal, and every block of T is written before it is read), so
// the two D x ld memsets are skipped
int fr_tri_inverse_enqueue(vb_ctx* ctx, hipStream_t st, const double* theta_dev, const double* Lt, int D, int64_t ldl,
                           double* Xa, double* T, bool clean) {
  const int n_cu = ctx->prop.multiProcessorCount;
  const int64_t slab = (int64_t)D * ldl;
  if (!clean) {
    VB_HIP(ctx, hipMemsetAsync(Xa, 0, (size_t)slab * sizeof(double), st));
    VB_HIP(ctx, hipMemsetAsync(T, 0, (size_t)slab * sizeof(double), st));
  }
  static const hipError_t leaf_attr = hipFuncSetAttribute(
      reinterpret_cast<const void*>(fr_triinv_leaf_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
      kTriLeaf * kTriLeaf * (int)sizeof(double));         // 128 KB of LDS per workgroup
  VB_HIP(ctx, leaf_attr);
  hipLaunchKernelGGL(fr_triinv_leaf_kernel, dim3((unsigned)((D + 3) / 4)), dim3(256),
                     kTriLeaf * kTriLeaf * sizeof(double), st, theta_dev, Lt, D, ldl, Xa);
  VB_HIP(ctx, hipGetLastError());
  GemmArgs gn;
  gn.lda = ldl;
  gn.ldb = ldl;
  gn.tri_mode = 0;
  for (int b = kTriLeaf; b < D; b *= 2) {
    // the pairs of a level are independent products of one shape: one batched launch (blockIdx.z = pair) for
    // the full pairs, one more for a ragged last pair
    const int full = D / (2 * b);
    const int64_t pair_stride = (int64_t)2 * b * ldl + 2 * b;
    for (int pass = 0; pass < 2; ++pass) {
      const int s0 = pass == 0 ? 0 : full * 2 * b;
      const int count = pass == 0 ? full : (s0 + b < D ? 1 : 0);
      if (count == 0) continue;
      const int b2 = pass == 0 ? b : D - s0 - b;
      const int64_t oa = (int64_t)s0 * ldl + s0, ob = (int64_t)s0 * ldl + s0 + b,
                    oc = (int64_t)(s0 + b) * ldl + s0 + b;
      gn.batch = 1;
      gn.batch_a = pair_stride;
      gn.batch_b = pair_stride;
      gn.A = Lt + ob;      // B block (b x b2)
      gn.B = Xa + oc;      // C^-1 (b2 x b2)
      gn.M = b;
      gn.N = b2;
      gn.K = b2;
      gemm_f64_launch<true>(st, gn, count, n_cu, EpiStoreD{T + ob, ldl, 1.0, pair_stride});
      gn.A = Xa + oa;      // A^-1 (b x b)
      gn.B = T + ob;
      gn.K = b;
      gemm_f64_launch<true>(st, gn, count, n_cu, EpiStoreD{Xa + ob, ldl, -1.0, pair_stride});
    }
  }
  VB_HIP(ctx, hipGetLastError());
  return VB_OK;
}

// ---- wrappers shared with the multivariate-t path (vb_mvt.hip) ---------------------------------------
int fr_colsum_enqueue(vb_ctx* ctx, const double* G, const double* Zc, int64_t ldz, int64_t n, int d, int fmode,
                      const double* ivar, double* colpart, double* fpart, const double* roww, int square) {
  const int n_rb = (int)((n + 127) / 128);
  hipLaunchKernelGGL(fr_colsum_kernel, dim3((unsigned)((d + 127) / 128), (unsigned)n_rb), dim3(256), 0, ctx->stream,
                     G, Zc, ldz, n, d, fmode, ivar, colpart, fpart, 0.0, roww, square);
  VB_HIP(ctx, hipGetLastError());
  return VB_OK;
}

int fr_reduce_enqueue(vb_ctx* ctx, const double* Cpart, int splits, int64_t slab, int d, int64_t ldl,
                      const double* colpart, int n_rb, int64_t ldz, const double* fpart, int n_fpart, FrSums S, bool mirror,
                      const double* wpart) {
  fr_reduce_launch(ctx, ctx->stream, Cpart, splits, slab, d, ldl, colpart, n_rb, ldz, fpart, n_fpart, S, mirror ? 2 : 0, wpart);
  VB_HIP(ctx, hipGetLastError());
  return VB_OK;
}

int gram_lower_enqueue(vb_ctx* ctx, const double* A, const double* B, int64_t ld, int d, int64_t n, int splits,
                       double* Cpart, int64_t ldc, int64_t slab) {
  GemmArgs g3 = gemm_product(A, ld, B, ld, d, d, (int)n, 2);
  const char* xcd_env = getenv("VB_GRAM_XCD");
  g3.xcd_group = xcd_env ? atoi(xcd_env) : 1;
  gemm_f64_launch<false>(ctx->stream, g3, splits, ctx->prop.multiProcessorCount, EpiSplitSlab{Cpart, ldc, slab});
  VB_HIP(ctx, hipGetLastError());
  return VB_OK;
}

// The same product with the column sums of A formed out of the gradient GEMM's LDS tiles (EpiSplitSlabCs: one row of
// `colsum` per split, row stride colsum_ld) -- no separate pass over A.  *fused = false: the shape does not go through
// the LDS-DMA kernel (or there are more splits than rows in the caller's column-sum buffer) and the caller needs
// fr_colsum_enqueue as before.
int gram_lower_colsum_enqueue(vb_ctx* ctx, const double* A, const double* B, int64_t ld, int d, int64_t n, int splits,
                              double* Cpart, int64_t ldc, int64_t slab, double* colsum, int64_t colsum_ld,
                              int colsum_rows, bool* fused) {
  const GemmArgs g3 = gemm_product(A, ld, B, ld, d, d, (int)n, 2);
  *fused = n % kGemmBK == 0 && gemm_uses_dma(g3) && splits <= colsum_rows;
  if (*fused)
    gemm_f64_launch<false>(ctx->stream, g3, splits, ctx->prop.multiProcessorCount,
                           EpiSplitSlabCs{Cpart, ldc, slab, colsum, colsum_ld});
  else
    gemm_f64_launch<false>(ctx->stream, g3, splits, ctx->prop.multiProcessorCount, EpiSplitSlab{Cpart, ldc, slab});
  VB_HIP(ctx, hipGetLastError());
  return VB_OK;
}

// vb_noise_moments: column sums and (optionally) the Gram matrix of a noise slot -> host
int noise_moments(vb_ctx* ctx, const NoiseSlot& ns, int64_t n, int64_t d, double* colsum_host, double* gram_host) {
  if (n <= 0 || n > ns.n || d != ns.d) return fail(ctx, VB_ERR_INVALID, "noise slot shape mismatch");
  const int D = (int)d;
  const int64_t ld = ns.ld, ldl = round_up(d, 16), slab = d * ldl;
  const int n_rb = (int)((n + 127) / 128), cs_gx = (D + 127) / 128;
  const int splits = gram_host ? gram_splits(ctx, D, n) : 0;
  int64_t off = 0;
  auto carve = [&off](int64_t doubles) {
    const int64_t o = off;
    off += round_up(doubles, 16);
    return o;
  };
  const int64_t o_col = carve((int64_t)n_rb * ld), o_f = carve((int64_t)n_rb * cs_gx), o_cpart = carve((int64_t)splits * slab),
                o_sums = carve(16 + ld + slab);
  VB_TRY(ensure(ctx, ctx->scratch, (size_t)off * sizeof(double)));
  double* base = (double*)ctx->scratch.ptr;
  const double* E = (const double*)ns.buf.ptr;
  hipStream_t st = ctx->stream;
  VB_TRY(fr_colsum_enqueue(ctx, E, E, ld, n, D, 0, nullptr, base + o_col, base + o_f, nullptr, 0));
  if (gram_host) VB_TRY(gram_lower_enqueue(ctx, E, E, ld, D, n, splits, base + o_cpart, ldl, slab));
  FrSums S;
  S.sums = base + o_sums;
  S.off_col = 16;
  S.off_c = 16 + ld;
  S.len = 16 + ld + slab;
  VB_TRY(fr_reduce_enqueue(ctx, base + o_cpart, splits, slab, D, ldl, base + o_col, n_rb, ld, base + o_f, 0, S));
  if (ctx->comm) VB_TRY(comm_allreduce_sum(ctx, st, S.sums, (size_t)(gram_host ? S.len : 16 + ld)));
  VB_HIP(ctx, hipMemcpyAsync(colsum_host, S.sums + S.off_col, (size_t)d * sizeof(double), hipMemcpyDeviceToHost, st));
  if (gram_host)
    VB_HIP(ctx, hipMemcpy2DAsync(gram_host, (size_t)d * sizeof(double), S.sums + S.off_c, (size_t)ldl * sizeof(double),
                                 (size_t)d * sizeof(double), (size_t)d, hipMemcpyDeviceToHost, st));
  VB_HIP(ctx, hipStreamSynchronize(st));
  if (gram_host)      // the product fills the lower triangle: mirror it
    for (int64_t i = 0; i < d; ++i)
      for (int64_t j = i + 1; j < d; ++j) gram_host[i * d + j] = gram_host[j * d + i];
  return VB_OK;
}

int gram_splits(vb_ctx* ctx, int d, int64_t n) {
  return gemm_gram_splits(d, n, ctx->prop.multiProcessorCount);
}

// ---- XCD-aware tile order of the lower-triangular product C = G' E ------------------------------------------
// Block x of a launch runs on XCD x % 8 and every XCD has its own 4-MiB L2.  In row-by-row order the tiles that share
// an operand panel (same row block: the same 128 columns of G; same column block: the same 64 columns of E) land on
// eight different XCDs and each XCD streams nearly every panel: 355 MB cross the fabric per launch against 67 MB of
// operands (PMC FETCH_SIZE, D = 1024).  Here the tiles are walked in bands of two row blocks, column by column, and
// cut into eight runs of equal length -- compact 2 x ~4.5 patches that touch few panels -- and run c gets the blocks
// x = c, c + 8, c + 16, ...
static int tri2_tile_map(vb_ctx* ctx, int d, int bm_rows, int bn_cols, const int** map_out, int* blocks_out) {
  if (ctx->tri_map.ptr && ctx->tri_map_key[0] == d && ctx->tri_map_key[1] == bm_rows && ctx->tri_map_key[2] == bn_cols) {
    *map_out = (const int*)ctx->tri_map.ptr;
    *blocks_out = ctx->tri_map_blocks;
    return VB_OK;
  }
  const int tm = gemm_tiles(d, bm_rows), tn = gemm_tiles(d, bn_cols);
  std::vector<std::pair<int, int>> order;
  for (int band = 0; band < tm; band += 2)
    for (int bn = 0; bn < tn; ++bn)
      for (int bm = band; bm < band + 2 && bm < tm; ++bm)
        if (bn * bn_cols <= bm * bm_rows + bm_rows - 1) order.push_back({bm, bn});
  const int total = (int)order.size(), per = (total + 7) / 8, blocks = per * 8;
  std::vector<int> host((size_t)2 * blocks, -1);
  for (int c = 0; c < 8; ++c)
    for (int i = 0; i < per; ++i) {
      const int src = c * per + i;
      if (src >= total) break;
      host[2 * (8 * i + c)] = order[src].first;
      host[2 * (8 * i + c) + 1] = order[src].second;
    }
  VB_TRY(ensure(ctx, ctx->tri_map, host.size() * sizeof(int)));
  VB_HIP(ctx, hipMemcpyAsync(ctx->tri_map.ptr, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice,
                             ctx->stream));
  VB_HIP(ctx, hipStreamSynchronize(ctx->stream));   // `host` is stack-scoped
  ctx->tri_map_key[0] = d;
  ctx->tri_map_key[1] = bm_rows;
  ctx->tri_map_key[2] = bn_cols;
  ctx->tri_map_blocks = blocks;
  *map_out = (const int*)ctx->tri_map.ptr;
  *blocks_out = blocks;
  return VB_OK;
}

// ---- short shards: split-k for the two N x D x D products ------------------------------------------------------------
// With few sample rows (a strong-scaling shard: 512 rows at D = 1024 give 128 tiles of 64 x 64 for 256 CUs) the 64-slab k
// range of ONE tile is the critical path of Z = E L' and of G = -(Z - m) P: 47 and 51 us with three quarters of the chip
// idle.  The k range is then cut into `parts` pieces that run as separate workgroups into slabs of partial products
// (EpiSplitSlab, the triangular one simply finds some of its pieces empty), and these kernels add the slabs in fixed
// order and apply the epilogue of the unsplit product: Z = sum + mu - m, and G = -sum with the per-workgroup sum of
// f = 1/2 (z - m)' g.
__global__ void __launch_bounds__(256) fr_zsum_kernel(const double* __restrict__ P, int parts, int64_t pslab, int64_t n,
                                                      int d, int64_t ldz, const double* __restrict__ mu,
                                                      const double* __restrict__ shift, double* __restrict__ Z) {
  const int64_t idx = 2 * ((int64_t)blockIdx.x * 256 + threadIdx.x);
  if (idx >= n * ldz) return;
  const int c = (int)(idx % ldz);
  fr_d2 s = (fr_d2){0.0, 0.0};
  for (int k = 0; k < parts; ++k) s += *reinterpret_cast<const fr_d2*>(P + k * pslab + idx);
  if (c < d) s.x += mu[c] - (shift ? shift[c] : 0.0);
  else s.x = 0.0;
  if (c + 1 < d) s.y += mu[c + 1] - (shift ? shift[c + 1] : 0.0);
  else s.y = 0.0;
  *reinterpret_cast<fr_d2*>(Z + idx) = s;
}

__global__ void __launch_bounds__(256) fr_gsum_kernel(const double* __restrict__ P, int parts, int64_t pslab, int64_t n,
                                                      int d, int64_t ldz, const double* __restrict__ Zc,
                                                      double* __restrict__ G, double* __restrict__ fpart) {
  __shared__ double sh[4];
  const int64_t idx = 2 * ((int64_t)blockIdx.x * 256 + threadIdx.x);
  double f = 0.0;
  if (idx < n * ldz) {
    const int c = (int)(idx % ldz);
    fr_d2 s = (fr_d2){0.0, 0.0};
    for (int k = 0; k < parts; ++k) s += *reinterpret_cast<const fr_d2*>(P + k * pslab + idx);
    const fr_d2 z = *reinterpret_cast<const fr_d2*>(Zc + idx);
    if (c >= d) s.x = 0.0;
    if (c + 1 >= d) s.y = 0.0;
    *reinterpret_cast<fr_d2*>(G + idx) = (fr_d2){-s.x, -s.y};
    f = -0.5 * s.x * z.x - 0.5 * s.y * z.y;
  }
  f = fr_wave_sum(f);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = f;
  __syncthreads();
  if (threadIdx.x == 0) fpart[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// ---- the fused evaluation's launch (vb_fullrank_fused.h) --------------------------------------------------------------
// phases == 2: Z and G by one persistent launch (returns the number of sum-f partials); phases == 3: C as well.
static int fr_fused_enqueue(vb_ctx* ctx, hipStream_t st, int phases, GemmArgs g1, GemmArgs g2, GemmArgs g3, int splits,
                            double* Z, double* G, int64_t ldz, const double* mu, const double* shift, double* fpart,
                            const EpiSplitSlabCs& e3, unsigned* tiles2_out) {
  const int n_cu = ctx->prop.multiProcessorCount;
  const int n = g1.M, D = g1.N;
  auto fill = [](GemmArgs& g, int splits_) {
    const int ks = gemm_tiles(g.K, splits_);
    g.k_split = gemm_tiles(ks, kGemmBK) * kGemmBK;
    g.tiles_m = gemm_tiles(g.M, 128);
    g.tiles_n = gemm_tiles(g.N, 64);
    g.prio_div = 0;
    g.ev0 = g.ev1 = nullptr;
  };
  fill(g1, 1);
  fill(g2, 1);
  fill(g3, splits);
  const int tm = g1.tiles_m, tn = g1.tiles_n;
  const int n_p1 = tm * tn, n_p2 = tm * tn;
  const int n_p3 = g3.tile_map ? g3.tile_blocks : (int)gemm_count_blocks(g3, 128, 64);
  // shared words: [head | err | 14 pad | zflag tm x tn | gflag tm x tn]
  const size_t words = 16 + 2 * (size_t)tm * tn;
  VB_TRY(ensure(ctx, ctx->fz_words, words * sizeof(unsigned)));      // (a new allocation is zeroed by ensure)
  unsigned* wbase = (unsigned*)ctx->fz_words.ptr;
  const int64_t key[5] = {n, D, splits, phases, n_p3};
  if (memcmp(key, ctx->fz_key, sizeof key) != 0 || !ctx->fz_items.ptr) {
    // the list, in a topological order: every Z tile heaviest k range first; then row block by row block the G tiles,
    // and behind the last row block of a split the C tiles of that split
    std::vector<int> host;
    auto push = [&host](int phase, int bx, int bz) {
      host.push_back(phase), host.push_back(bx), host.push_back(bz), host.push_back(0);
    };
    // (the row blocks cut into groups, each group's Z tiles followed by its G tiles, was measured and dropped:
    // profiles/r04_fused_timeline.txt)
    std::vector<int> map;
    if (phases == 3 && g3.tile_map) {
      map.resize((size_t)2 * n_p3);
      VB_HIP(ctx, hipMemcpy(map.data(), g3.tile_map, map.size() * sizeof(int), hipMemcpyDeviceToHost));
    }
    // block x of the triangular product: idx = x / tm selects the column block (heaviest first), x % tm the row block
    for (int idx = 0; idx < tn; ++idx)
      for (int rb = 0; rb < tm; ++rb) push(0, idx * tm + rb, 0);
    int z_next = 0;
    for (int rb = 0; rb < tm; ++rb) {
      for (int cb = 0; cb < tn; ++cb) push(1, cb * tm + rb, 0);
      while (phases == 3 && z_next < splits) {
        const int64_t last_row = std::min<int64_t>(n, (int64_t)(z_next + 1) * g3.k_split) - 1;
        if (last_row / 128 > rb) break;
        for (int bx = 0; bx < n_p3; ++bx)
          if (map.empty() || map[2 * bx] >= 0) push(2, bx, z_next);
        ++z_next;
      }
    }
    VB_TRY(ensure(ctx, ctx->fz_items, host.size() * sizeof(int)));
    VB_HIP(ctx, hipMemcpyAsync(ctx->fz_items.ptr, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice, st));
    VB_HIP(ctx, hipStreamSynchronize(st));      // `host` is stack-scoped
    memcpy(ctx->fz_key, key, sizeof key);
    ctx->fz_n_items = (int)(host.size() / 4);
  }
  if (++ctx->fz_epoch == 0) ctx->fz_epoch = 1;
  FzArgs a;
  a.g1 = g1, a.g2 = g2, a.g3 = g3;
  a.e1 = EpiStoreZPub{Z, ldz, mu, shift};
  a.G = G, a.ldz = ldz, a.Zc = Z, a.fpart = fpart;
  a.e3 = e3;
  a.s.head = wbase, a.s.err = wbase + 1, a.s.zflag = wbase + 16, a.s.gflag = wbase + 16 + (size_t)tm * tn;
  a.s.epoch = ctx->fz_epoch, a.s.tiles_n = tn;
  a.items = (const int4*)ctx->fz_items.ptr;
  a.n_items = ctx->fz_n_items, a.n_p1 = n_p1, a.n_p2 = n_p2, a.n_p3 = n_p3;
  a.clk = nullptr;
#ifdef VB_FUSED_CLOCK
  VB_TRY(ensure(ctx, ctx->scratch2, (size_t)4 * a.n_items * sizeof(long long)));
  a.clk = (long long*)ctx->scratch2.ptr;
#endif
  constexpr size_t lds = (size_t)3 * (128 * kGemmBK + kGemmBK * 64) * sizeof(double) + 16;
  static bool configured = false;
  if (!configured) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&fr_fused_kernel<2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&fr_fused_kernel<3>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    configured = true;
  }
  const unsigned grid = (unsigned)(2 * n_cu);
  if (phases == 3) hipLaunchKernelGGL(fr_fused_kernel<3>, dim3(grid), dim3(256), lds, st, a);
  else hipLaunchKernelGGL(fr_fused_kernel<2>, dim3(grid), dim3(256), lds, st, a);
  VB_HIP(ctx, hipGetLastError());
#ifdef VB_FUSED_CLOCK
  if (const char* path = getenv("VB_FUSED_CLOCK_DUMP")) {      // per-item clocks of THIS launch (tools/fused_clock.py)
    VB_HIP(ctx, hipStreamSynchronize(st));
    std::vector<long long> h((size_t)4 * a.n_items);
    VB_HIP(ctx, hipMemcpy(h.data(), a.clk, h.size() * sizeof(long long), hipMemcpyDeviceToHost));
    if (FILE* f = fopen(path, "wb")) {
      fwrite(h.data(), sizeof(long long), h.size(), f);
      fclose(f);
    }
  }
#endif
  *tiles2_out = (unsigned)n_p2;
  return VB_OK;
}

// ---- host orchestration ------------------------------------------------------------------------------
// One evaluation is decided once, before its first launch (FrRoute, fr_route), laid out once (FrBufs, fr_carve) and
// then enqueued stage by stage in pipeline order; the stages only read the route.

// correlated-Gaussian target: who forms G
enum FrDense {
  kDenseNoG,             // nobody: the sums of G = -E M - 1 b' from M = L' P and the noise's Gram matrix (the folded
                         // evaluation, below) -- no sampling product, no model product
  kDenseCallerG,         // the caller's G of these very samples (FrWeighted::g_ready)
  kDensePersistent,      // one persistent launch for Z - m and G (fz_mode 3: the gradient product as well)
  kDenseChain            // sampling product, then model product
};

struct FrRoute {
  // the call
  bool mvt = false, pd = false, glm = false, source = false, overlap = false;
  int n_cu = 0;
  // shapes
  int64_t n = 0, d = 0, ldl = 0, ldz = 0, ldr = 0, slab = 0, pslab = 0, np = 0, glm_part = 0;
  int D = 0, n_rb = 0, cs_gx = 0, n_fpart = 0;
  int tri1 = 0, tri3 = 0;       // tri_mode of the sampling and of the gradient product
  // the decisions
  int splits = 1;               // gradient product: pieces of the sample axis
  int kparts = 1;               // short shards: pieces of the k range of the N x D x D products (1: not split)
  unsigned sum_blocks = 0;      // grid of the kernels that add those pieces
  bool fold_shape = false;      // the folded evaluation's buffers are carved
  bool fold = false;
  int csplits = 1;              // its gradient product C = -tril(M' S) - b s': pieces of the k range
  int cfgc = 0;                 // ... and its tile configuration (gemm_f64_launch's cfg)
  int fz_mode = 0;              // 2 / 3: the persistent launch (kDensePersistent)
  FrDense dense = kDenseChain;
  bool model_ksplit = false;    // kDenseChain: the model product is cut like the sampling product
  bool caller_z = false;        // the target reads the caller's samples: no sampling product
  bool fused_sums = false;      // correlated Gaussian: sum f from the model product, column sums from the gradient product
  bool diag_f = false;          // diagonal Gaussian: sum f from the sampling product's epilogue
  bool cs_only = false;         // sum f is there already, the column sums come from the gradient product
  bool g_prescaled = false;     // the target's own kernel writes G already scaled by the row weights
  bool scale_rows_w = false;    // weighted sums: a pass over G scales its rows
  bool two_passes = false;      // path derivative: a column pass for f before the score is added
  bool colpass = false;         // the column pass between the products
  bool colpass_keeps_f = false; // ... and its f partials are the evaluation's (otherwise they go to an unused tail)
  int fmode = 0;                // how the column pass forms f (fr_colsum_kernel)
  bool grad_colsums = false;    // the gradient product forms the column sums of G (one row per split)
  bool grad_launch = true;      // (false: the persistent launch wrote the split slabs already)
  int cfg3 = 0;                 // its tile configuration (0: the launcher's choice; 2: 128 x 64 with the XCD tile map)
  bool f_per_tile = false;      // sum f: one partial per tile of the launch that formed it (tiles2), not n_fpart
};

// Decides the whole evaluation from what is known up front.  No HIP call, no state: of `ctx` it reads the CU count, whether
// a communicator is attached and the fused mode.
static FrRoute fr_route(const vb_ctx* ctx, const ModelDev& m, int64_t n, int64_t d, bool mvt, bool pd, bool row_scaled,
                        const FrWeighted& wm) {
  FrRoute r;
  const bool gauss_diag = m.id == VB_MODEL_GAUSS_DIAG, gauss_full = m.id == VB_MODEL_GAUSS_FULL,
             funnel = m.id == VB_MODEL_FUNNEL;
  r.mvt = mvt;
  r.pd = pd;
  r.glm = m.id == VB_MODEL_LOGISTIC;
  r.source = model_has_rows(m.id);
  r.overlap = !mvt && ctx->comm != nullptr;
  r.n_cu = ctx->prop.multiProcessorCount;
  r.n = n;
  r.d = d;
  r.D = (int)d;
  r.ldl = r.ldz = round_up(d, 16);
  r.slab = d * r.ldl;
  r.pslab = n * r.ldz;
  r.np = d * (d + 1) / 2;
  r.tri1 = mvt ? 0 : 1;
  r.tri3 = mvt ? 0 : 2;
  const int D = r.D, n_cu = r.n_cu;
  // the shapes of the sampling and of the gradient product (what the launcher's own decisions read)
  const GemmArgs s1 = gemm_product(nullptr, 0, nullptr, 0, (int)n, D, D, r.tri1);
  const GemmArgs s3 = gemm_product(nullptr, 0, nullptr, 0, D, D, (int)n, r.tri3);

  const int tiles = gemm_tiles(D, 128);
  const int lower_tiles = mvt ? tiles * tiles : tiles * (tiles + 1) / 2;
  r.splits = n_cu / lower_tiles;   // one wave of workgroups: no second, mostly empty round
  // at least this many sample rows per split: 192 lets D = 512 take 21 splits of its 36 lower 64 x 64 tiles (756
  // workgroups on the 768 resident slots: gradient GEMM 38.9 -> 33.7 us, split reduction 8.5 -> 10.4 us; 256 rows
  // stopped it at 16 splits); D = 1024 takes 7 either way
  const int max_splits = (int)(n / 192) > 0 ? (int)(n / 192) : 1;
  if (r.splits > max_splits) r.splits = max_splits;
  if (r.splits < 1) r.splits = 1;
  r.n_rb = (int)((n + 127) / 128);
  r.cs_gx = (D + 127) / 128;
  // regression targets: the log-likelihood partials of the eta GEMM follow the column-sum kernel's f partials
  r.glm_part = r.glm ? gemm_max_blocks(n, m.n_data) : 0;
  r.ldr = r.glm ? round_up(m.n_data, 16) : 0;
  r.n_fpart = funnel ? (int)((n + 3) / 4) : r.source ? (int)n : r.n_rb * r.cs_gx + (int)r.glm_part;

  // correlated-Gaussian target under the dense Gaussian family: no pass over G and Z between the GEMMs -- sum f comes
  // out of the model GEMM's epilogue (EpiNegateF) and the column sums of G out of the gradient GEMM (EpiSplitSlabCs)
  const bool sums_in_gemms = !mvt && !wm.roww && !row_scaled && n % kGemmBK == 0 && gemm_uses_dma(s1) &&
                             (int64_t)r.splits <= r.n_rb;
  r.fused_sums = gauss_full && sums_in_gemms;
  // diagonal Gaussian target under the dense Gaussian family: sum f out of the sampling product's epilogue
  r.diag_f = gauss_diag && sums_in_gemms;

  // short shards (fewer than two 64 x 64 tiles per CU): the N x D x D products with their k range cut into `kparts`
  // pieces (see fr_zsum_kernel); the slabs of partial products live in the split area of the gradient product, which
  // is not in use yet
  if (!row_scaled && !pd && !gauss_diag) {      // (pd keeps a slab of its own there)
    // measured (tools/fr_bench.py, D = 1024): 512 rows 126 -> 85 us per evaluation, 256 rows 118 -> 61 us, 1 024 rows
    // 133 -> 128 us, 2 048 rows unchanged (not split).  At D = 512 a tile's 32 slabs are no longer than a piece plus
    // the extra kernel: not split (pieces of at least 16 slabs out of at least 48).
    const long tiles64 = gemm_count_blocks(s1, 64, 64);
    if (tiles64 < 2L * n_cu && D >= 48 * kGemmBK) r.kparts = (int)((2L * n_cu + tiles64 - 1) / tiles64);
    if (r.kparts > 4) r.kparts = 4;
    while (r.kparts > 1 && (D % (kGemmBK * r.kparts) != 0 || D / r.kparts < 16 * kGemmBK)) --r.kparts;
    if ((int64_t)r.kparts * r.pslab > (int64_t)(r.splits + 1) * r.slab) r.kparts = 1;
  }
  r.sum_blocks = (unsigned)((r.pslab / 2 + 255) / 256);

  // The folded evaluation.  G is linear in the noise for this target, G = -(E L' + 1 c') P = -E M - 1 b' with c = mu - m,
  // M = L' P and b = P c, and the only other use of Z - m, sum f = 1/2 sum (Z - m) o G, follows from what the gradient
  // product forms anyway:  sum (Z - m) o G = tr((E L' + 1 c')' G) = sum_{i >= j} L_ij C_ij + c . colsum(G),  C = G' E.
  // Nothing the evaluation returns needs G itself: with S = E' E, s = colsum(E) and n the rows of this rank,
  //   C = G' E = -M' S - b s'        colsum(G) = -s' M - n b'
  // so neither N x D x D product is formed and neither Z nor G is stored.  The chain:
  //   Gram product of the noise: the gradient product's own shape, kernel and tile map with A = B = E, `splits` slabs of
  //     the lower tiles of S, one row of column sums of E per slab out of its LDS tiles (EpiSplitSlabCs)
  //   fr_fold_msum_kernel: M = L' P (tri_mode 4, row blocks in pairs: M itself, no slabs) and, in the wave slots its
  //     workgroups leave free, b, S in full (mirrored), s
  //   C slabs = -(M' S) - b s' (lower tiles, K = D in csplits pieces, EpiFoldSlabF: sum L o tril(C) per tile and split)
  //   colsum(G) = -s' M - n b' (fr_fold_csg_blocks), which nobody reads before
  //   fr_reduce_packed_kernel, as for every route: the slabs of C, ONE row of column sums, the f partials.
  // M and S are formed anew in EVERY evaluation: M follows the parameter, which an optimiser steps every time, and S the
  // noise, which every iteration of a fit draws afresh -- nothing is kept per slot, per parameter or per engine.
  // The K axis of the C product: the LDS-DMA kernel reads whole kGemmBK-row slabs of M and S, so a D that is no multiple
  // of kGemmBK is kept OUT of the route -- fused_sums below already asks gemm_uses_dma of a product with K = D -- and the
  // rows of M and S have no pad (ldz = ldl = D).
  // Not with the path derivative (it changes G between the products), not with the caller's own Z or G, not for short
  // shards (kparts), and only from the shapes at which it measures faster (the gate's table).  Ranks of one
  // job may fall on different sides of the gate: both routes hand the same sums [F | colsum | C] of the rank's own rows
  // to the all-reduce.
  r.fold_shape = !mvt && gauss_full && !pd && d >= VB_FR_FOLD_MIN_D && n >= (int64_t)VB_FR_FOLD_MIN_ROWS_PER_D * d;
  r.fold = r.fold_shape && r.fused_sums && r.kparts == 1 && !wm.z_ready && !wm.g_ready && n >= d + 2;      // (fr_carve; cannot bind while the gate asks n >= 3 d)

  // the fused evaluation: 2 = Z and G in one persistent launch, 3 = the gradient product's split slabs as well
  // (its phase 1 is the product the fold removes: where the fold applies it takes precedence; the path derivative changes G
  // between the products; the caller's G leaves nothing to fuse)
  r.fz_mode = ctx->fr_fused_mode;
  if (r.fz_mode < 0) {
    const char* e = getenv("VB_FR_FUSED");
    r.fz_mode = e ? atoi(e) : 0;
  }
  if (!(r.fused_sums && r.kparts == 1 && n % 128 == 0 && D % 64 == 0 && (int64_t)n * r.ldz * 8 < ((int64_t)1 << 31)))
    r.fz_mode = 0;
  if ((r.fz_mode != 2 && r.fz_mode != 3) || pd || r.fold || wm.g_ready) r.fz_mode = 0;
  r.dense = r.fold ? kDenseNoG : wm.g_ready ? kDenseCallerG : r.fz_mode >= 2 ? kDensePersistent : kDenseChain;
  r.model_ksplit = r.kparts > 1 && r.fused_sums;
  // (the caller's samples: see FrWeighted; the correlated Gaussian wants Z - m and forms its own)
  r.caller_z = wm.z_ready != nullptr && (funnel || r.source || r.glm);

  r.g_prescaled = funnel && wm.roww != nullptr;
  r.scale_rows_w = wm.roww != nullptr && !r.g_prescaled;
  // targets whose row kernel leaves sum f behind already (funnel, source models): the column sums of G are all the pass
  // between the products would add, and they come out of the gradient product's LDS tiles as for the correlated Gaussian
  // (weighted sums: the same, once G is scaled -- the column sums of the gradient product's operand tiles ARE sum w g)
  r.cs_only = r.diag_f || (!r.fused_sums && !mvt && (funnel || r.source) && (!wm.roww || r.g_prescaled) && !row_scaled &&
                           n % kGemmBK == 0 && gemm_uses_dma(s3) && (int64_t)r.splits <= r.n_rb);
  // path derivative: sum f belongs to the model's G, the column sums and the gradient product to G~ = G + E L^-1.  Where
  // the column pass forms f from G (every target but the funnel and source models, whose own kernels left it behind) it
  // runs once before the score is added -- for f -- and once after, for the column sums only
  const bool f_from_pass = !(funnel || r.source);
  r.colpass = !r.fused_sums && !r.cs_only;
  r.two_passes = pd && r.colpass && f_from_pass;
  r.colpass_keeps_f = f_from_pass && !r.two_passes;
  // (weighted sums over the caller's G take their value from the weights: no f there)
  r.fmode = gauss_diag ? 1 : r.glm ? 3 : (gauss_full && !wm.g_ready) ? 2 : 0;

  r.grad_launch = r.fz_mode != 3;
  r.grad_colsums = r.fused_sums || r.cs_only;
  // 128 x 64 tiles are the launcher's own choice for this shape, made here so that the XCD tile list fits it
  if (r.grad_launch && r.grad_colsums && gemm_count_blocks(s3, 128, 64) * r.splits * 100 >= 190L * n_cu) r.cfg3 = 2;
  r.f_per_tile = r.fused_sums || r.diag_f;
  if (r.fold) {     // its gradient product: 64 x 64 tiles, two LDS stages, while they fit the chip at once (fr_fold_csplits)
    r.csplits = fr_fold_csplits(D, n_cu, r.splits + 1);
    const GemmArgs sc = gemm_product(nullptr, 0, nullptr, 0, D, D, D, 2);
    if (gemm_count_blocks(sc, 64, 64) * r.csplits <= 4L * n_cu) r.cfgc = 4;
    else r.cfgc = gemm_count_blocks(sc, 128, 64) * r.csplits * 100 >= 190L * n_cu ? 2 : 3;
  }
  return r;
}

// device buffers of one evaluation
struct FrBufs {
  const double* E = nullptr;      // the noise, row stride lde
  int64_t lde = 0;
  double *mu = nullptr, *Lt = nullptr;      // (the dense family's live in ctx->fr_lt: fr_prepare_dense)
  double *Z = nullptr, *G = nullptr, *Cpart = nullptr, *colpart = nullptr, *fpart = nullptr;
  double* Rm = nullptr;                                             // regression targets: the residuals
  double *Mf = nullptr, *bvec = nullptr;                            // folded evaluation: M = L' P; b = P (mu - m)
  double *Sg = nullptr, *svec = nullptr, *csg = nullptr;            // ... S = E' E (D x ldl), s = colsum(E), colsum(G)
  double *Xa = nullptr, *T = nullptr, *sq = nullptr;                // path derivative: (L')^-1, a product buffer (then L^-1),
                                                                    // partial sums of squares of the noise
  FrSums S;
};

// one allocation (ctx->fr_work), carved; `set`: which of the two sum vectors of an overlapped evaluation
static int fr_carve(vb_ctx* ctx, const FrRoute& r, const NoiseSlot& ns, int set, FrBufs* out) {
  const int64_t n = r.n, ldz = r.ldz, slab = r.slab;
  int64_t off = 0;
  auto carve = [&off](int64_t doubles) {
    const int64_t o = off;
    off += round_up(doubles, 16);
    return o;
  };
  const int64_t o_mu = carve(ldz), o_lt = carve(slab), o_z = carve(n * ldz), o_g = carve(n * ldz),
                o_cpart = carve((int64_t)(r.splits + 1) * slab), o_col = carve((int64_t)(r.n_rb + 1) * ldz),
                o_fpart = carve((int64_t)r.n_fpart + (int64_t)r.n_rb * r.cs_gx + gemm_max_blocks(n, r.D) + (n * ldz) / 512 + 1),
                o_r = carve(r.glm ? n * r.ldr : 0);
  const int64_t o_mf = r.fold_shape ? carve(slab) : 0, o_bvec = r.fold_shape ? carve(ldz) : 0;
  const int64_t o_xa = r.pd ? carve(slab) : 0, o_t = r.pd ? carve(slab) : 0, o_m2 = r.pd ? carve(256) : 0;
  // sum vector: the t family takes the full D x ldl matrix; the Gaussian family packs the lower triangle in
  // theta's own order, twice over when the all-reduce of one evaluation overlaps the kernels of the next
  FrBufs b;
  b.S.off_col = 16;
  b.S.off_c = 16 + ldz;
  b.S.len = 16 + ldz + (r.mvt ? slab : round_up(r.np, 16));
  const int64_t o_sums = carve(b.S.len * (r.overlap ? 2 : 1));
  VB_TRY(ensure(ctx, ctx->fr_work, (size_t)off * sizeof(double)));
  double* base = (double*)ctx->fr_work.ptr;
  b.E = (const double*)ns.buf.ptr;
  b.lde = ns.ld;
  b.mu = base + o_mu, b.Lt = base + o_lt, b.Z = base + o_z, b.G = base + o_g, b.Cpart = base + o_cpart;
  b.colpart = base + o_col, b.fpart = base + o_fpart, b.Rm = base + o_r;
  b.Mf = base + o_mf, b.bvec = base + o_bvec;
  // the folded evaluation writes neither Z nor G: S, s and colsum(G) live where G would (n rows of ldz, n >= d + 2); the
  // slabs of the Gram product and then the slabs of C are the split area's (csplits <= splits + 1)
  if (r.fold) b.Sg = b.G, b.svec = b.G + slab, b.csg = b.G + slab + ldz;
  b.Xa = base + o_xa, b.T = base + o_t, b.sq = base + o_m2;
  b.S.sums = base + o_sums + (int64_t)set * b.S.len;
  *out = b;
  return VB_OK;
}

// stream plan (as mf_enqueue's `overlap`): everything up to the split reduction stays in order on the main
// stream; the all-reduce and the epilogue go to `post` behind one event, into sum set `seq & 1`, and the main
// stream only waits for them when that set comes round again two evaluations later.  Returns the set.
static int fr_stream_plan(vb_ctx* ctx, const FrRoute& r, int* set) {
  Pipeline& P = ctx->pipe;
  hipStream_t st = ctx->stream;
  *set = 0;
  if (r.overlap) {
    VB_TRY(pipe_init(ctx));
    *set = (int)(ctx->fr_seq++ & 1);
    if (P.fin_valid[*set]) VB_HIP(ctx, hipStreamWaitEvent(st, P.ev_fin[*set], 0));
  } else if (P.post_pending) {   // order this in-order evaluation after everything `post` has in flight
    VB_HIP(ctx, hipStreamWaitEvent(st, P.ev_fin[P.last_set], 0));
    P.post_pending = false;
  }
  return VB_OK;
}

// Prepare, t family: mu and the dense root into the work buffer
static int fr_prepare_mvt(vb_ctx* ctx, const FrRoute& r, const FrBufs& b, const double* mu_dev, const double* root_dev) {
  hipStream_t st = ctx->stream;
  VB_HIP(ctx, hipMemcpyAsync(b.mu, mu_dev, (size_t)r.d * sizeof(double), hipMemcpyDeviceToDevice, st));
  VB_HIP(ctx, hipMemcpy2DAsync(b.Lt, (size_t)r.ldl * sizeof(double), root_dev, (size_t)r.ldl * sizeof(double),
                               (size_t)r.d * sizeof(double), (size_t)r.d, hipMemcpyDeviceToDevice, st));
  return VB_OK;
}

// Prepare, dense family: mu and L' in a buffer of their own (ctx->fr_lt) -- when the parameter is the resident one
// (vb_fullrank_set_theta) it is unpacked once per upload, not once per evaluation
static int fr_prepare_dense(vb_ctx* ctx, const FrRoute& r, FrBufs* b, const double* theta_dev) {
  const int64_t d = r.d;
  VB_TRY(ensure(ctx, ctx->fr_lt, (size_t)(r.ldz + r.slab) * sizeof(double)));
  b->mu = (double*)ctx->fr_lt.ptr;
  b->Lt = b->mu + r.ldz;
  const bool resident = theta_dev == (const double*)ctx->fr_theta.ptr;
  // ... or vb_fit's parameter, whose step kernel wrote mu and L' of the stepped value itself (fr_step_unpack_enqueue)
  const bool stepped = ctx->fr_lt_owner != nullptr && ctx->fr_lt_owner == theta_dev;
  const bool lt_cached = (resident || stepped) && ctx->fr_lt_d == d;
  if (!stepped) ctx->fr_lt_owner = nullptr;
  ctx->fr_lt_d = (resident || stepped) ? d : 0;     // (a foreign parameter leaves the copy stale for the resident one)
  if (!lt_cached) {
    hipLaunchKernelGGL(fr_unpack_kernel, dim3((unsigned)((d + 31) / 32), (unsigned)((d + 31) / 32)), dim3(256), 0, ctx->stream,
                       theta_dev, r.D, r.ldl, b->Lt, b->mu);
    VB_HIP(ctx, hipGetLastError());
  }
  return VB_OK;
}

// Path derivative (objectives.py:166-168: the score's own parameter dependence is stopped): with z = mu + L eps the
// gradient of -log q along the path is L^-T eps, so every row of G takes that term -- G~ = G + E L^-1, one more
// N x D x D / 2 product (fr_score) -- and the usual sums of G~ finish the job: no entropy term, no noise Gram matrix, no
// D x D x D product (round 4; rounds 2-3 formed L^-T (E'E / N): 620 -> ~500 us at D = 1024, N = 4096).
// The prologue: (L')^-1 = U^-1 by recursive doubling (fr_tri_inverse_enqueue), L^-1 for the product, sum ||eps||^2.
static int fr_score_prologue(vb_ctx* ctx, const FrRoute& r, const FrBufs& b, const double* theta_dev) {
  hipStream_t st = ctx->stream;
  const int D = r.D;
  VB_TRY(fr_tri_inverse_enqueue(ctx, st, theta_dev, b.Lt, D, r.ldl, b.Xa, b.T));
  VB_HIP(ctx, hipGetLastError());
  // L^-1 = (U^-1)' with its rows k-major for the product (T is free again)
  hipLaunchKernelGGL(fr_transpose_kernel, dim3((unsigned)((D + 31) / 32), (unsigned)((D + 31) / 32)), dim3(256), 0, st,
                     (const double*)b.Xa, b.T, D, r.ldl);
  // sum ||eps_n||^2 -> sums[1]: the value's mean log q of the samples (:167)
  const int sq_blocks = (int)(r.n < 256 ? r.n : 256);
  hipLaunchKernelGGL(fr_sumsq_kernel, dim3((unsigned)sq_blocks), dim3(256), 0, st, b.E, b.lde, r.n, D, b.sq);
  hipLaunchKernelGGL(fr_sumsq_final_kernel, dim3(1), dim3(256), 0, st, (const double*)b.sq, sq_blocks, b.S.sums + 1);
  VB_HIP(ctx, hipGetLastError());
  return VB_OK;
}

// GEMM 1: Z[n][j] = sum_k E[n][k] Lt[k][j]   (Lt[k][j] = 0 for k > j), timed as VB_PROF_FR_SAMPLE_GEMM
static GemmArgs fr_sample_product(vb_ctx* ctx, const FrRoute& r, const FrBufs& b) {
  GemmArgs g1 = gemm_product(b.E, b.lde, b.Lt, r.ldl, (int)r.n, r.D, r.D, r.tri1);
  prof_events(ctx, &g1.ev0, &g1.ev1, 1, VB_PROF_FR_SAMPLE_GEMM);
  return g1;
}

// Sample: Z = E L' + mu - shift (the samples, or z - m for the correlated Gaussian target), plain or with the k range
// split; returns the Z the target reads -- the caller's where it brought them
static const double* fr_sample(vb_ctx* ctx, const FrRoute& r, const FrBufs& b, const double* shift, const double* row_scale,
                               const double* z_ready) {
  if (r.caller_z) return z_ready;
  hipStream_t st = ctx->stream;
  const GemmArgs g1 = fr_sample_product(ctx, r, b);
  if (r.kparts > 1) {
    gemm_f64_launch<true>(st, g1, r.kparts, r.n_cu, EpiSplitSlab{b.Cpart, r.ldz, r.pslab});
    hipLaunchKernelGGL(fr_zsum_kernel, dim3(r.sum_blocks), dim3(256), 0, st, (const double*)b.Cpart, r.kparts, r.pslab, r.n,
                       r.D, r.ldz, (const double*)b.mu, shift, b.Z);
  } else {
    gemm_f64_launch<true>(st, g1, 1, r.n_cu, EpiStoreZ{b.Z, r.ldz, b.mu, shift, row_scale});
  }
  return b.Z;
}

// Model, diagonal Gaussian: G out of the sampling product's epilogue, sum f as well where the route says so (a reducing
// epilogue: returns its number of partials)
static unsigned fr_model_gauss_diag(vb_ctx* ctx, const FrRoute& r, const FrBufs& b, const ModelDev& m,
                                    const double* row_scale) {
  const GemmArgs g1 = fr_sample_product(ctx, r, b);
  if (r.diag_f)
    return gemm_f64_launch<true>(ctx->stream, g1, 1, r.n_cu, EpiGaussDiagF{b.G, r.ldz, b.mu, m.p0, m.p1, b.fpart});
  gemm_f64_launch<true>(ctx->stream, g1, 1, r.n_cu, EpiGaussDiag{b.G, r.ldz, b.mu, m.p0, m.p1, row_scale});
  return 0;
}

static int fr_model_funnel(vb_ctx* ctx, const FrRoute& r, const FrBufs& b, const ModelDev& m, const double* Z,
                           const double* roww) {
  hipLaunchKernelGGL(fr_funnel_kernel, dim3((unsigned)((r.n + 3) / 4)), dim3(256), 0, ctx->stream, Z, b.G, r.ldz, r.n, r.D, m,
                     b.fpart, roww);
  return VB_OK;
}

// the user's row kernel: G and one f per sample (summed with the other f partials)
static int fr_model_source(vb_ctx* ctx, const FrRoute& r, const FrBufs& b, const double* Z) {
  return model_rows_enqueue(ctx, ctx->stream, Z, r.ldz, r.n, r.D, b.G, r.ldz, b.fpart);
}

static int fr_model_glm(vb_ctx* ctx, const FrRoute& r, const FrBufs& b, const ModelDev& m, const double* Z) {
  hipStream_t st = ctx->stream;
  double* part = b.fpart + (int64_t)r.n_rb * r.cs_gx;
  VB_HIP(ctx, hipMemsetAsync(part, 0, (size_t)r.glm_part * sizeof(double), st));
  // eta = Z X'   [n x n_data x d]
  const GemmArgs gh = gemm_product(Z, r.ldz, m.p1, m.ldq, (int)r.n, (int)m.n_data, r.D, 0);
  gemm_f64_launch<true>(st, gh, 1, r.n_cu, EpiGlm{b.Rm, r.ldr, m.p2, part, m.link, m.aux});
  VB_HIP(ctx, hipGetLastError());
  return glm_grad_enqueue(ctx, st, m, b.Rm, r.ldr, Z, b.G, r.ldz, r.n, r.D);   // G = R X - Z / sd^2
}

// The folded evaluation (fr_route).  The Gram product S = E' E with s = colsum(E) per slab (timed as VB_PROF_FR_GRAD_GEMM:
// the gradient product's shape); fr_fold_msum_kernel: M = L' P beside b = P (mu - m), s and the slabs of S added up; the
// slabs of C = -tril(M' S) - b s' with one partial of sum L o tril(C) per tile and split; colsum(G) = -s' M - n b', which
// only the reduction reads.  Returns in *tiles3 the number of output tiles of the C product.
static int fr_grad_folded(vb_ctx* ctx, const FrRoute& r, const FrBufs& b, const ModelDev& m, unsigned* tiles3) {
  hipStream_t st = ctx->stream;
  const int D = r.D;
  const double* M = b.Mf;
  GemmArgs gs = gemm_product(b.E, b.lde, b.E, b.lde, D, D, (int)r.n, 2);
  prof_events(ctx, &gs.ev0, &gs.ev1, 1, VB_PROF_FR_GRAD_GEMM);
  if (r.cfg3 == 2) VB_TRY(tri2_tile_map(ctx, D, 128, 64, &gs.tile_map, &gs.tile_blocks));
  gemm_f64_launch<false>(st, gs, r.splits, r.n_cu, EpiSplitSlabCs{b.Cpart, r.ldl, r.slab, b.colpart, r.ldz}, r.cfg3);
  VB_HIP(ctx, hipGetLastError());
  // M[r][j] = sum_{k >= r} Lt[r][k] P[k][j]: 64 x 32 tiles, row blocks b and T - 1 - b by one workgroup -- equal work per
  // workgroup with the k range unsplit, so the launch writes M itself.  Two four-wave teams per workgroup while there are
  // fewer than two workgroups per CU (D = 1024: 256), one team from there on (gemm_f64_team_pair_plan)
  GemmArgs gm = gemm_product(b.Lt, r.ldl, m.p1, m.ldp, D, D, D, 4);
  const unsigned nb_team = gemm_f64_team_pair_plan(&gm, r.n_cu);
  const unsigned nb_m = nb_team ? nb_team : gemm_f64_pair_plan(&gm);
  if (nb_m == 0) return fail(ctx, VB_ERR_STATE, "folded evaluation: D = %d does not go to the LDS-DMA product", D);
  const int nb_cs = (D + 7) / 8, nb_s = (int)((r.ldz + 255) / 256), tiles = (D + 31) / 32;
  constexpr size_t pair_lds = gemm_f64_dma_pair_lds<2, 4, 3>(), team_lds = gemm_f64_dma_team_pair_lds<2, 4, kFoldTeamStages>();
  static_assert(pair_lds >= 64 * 4 * sizeof(fr_d2) && pair_lds >= 32 * 33 * sizeof(double) && team_lds >= pair_lds,
                "the sum blocks' LDS is the tiles'");
  static bool configured = false;
  if (!configured) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&fr_fold_msum_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)pair_lds);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&fr_fold_msum_team_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)team_lds);
    configured = true;
  }
  const dim3 msum_grid(nb_m + (unsigned)(nb_cs + nb_s + tiles * (tiles + 1) / 2));
  const EpiSplitSlab em{b.Mf, r.ldz, r.slab};
  if (nb_team)
    hipLaunchKernelGGL(fr_fold_msum_team_kernel, msum_grid, dim3(512), team_lds, st, gm, em, (int)nb_m, (const double*)b.Cpart,
                       r.splits, r.slab, D, r.ldl, (const double*)b.colpart, r.ldz, m.p1, (int64_t)m.ldp, (const double*)b.mu,
                       m.p0, nb_cs, nb_s, b.Sg, b.svec, b.bvec);
  else
    hipLaunchKernelGGL(fr_fold_msum_kernel, msum_grid, dim3(256), pair_lds, st, gm, em, (int)nb_m, (const double*)b.Cpart,
                       r.splits, r.slab, D, r.ldl, (const double*)b.colpart, r.ldz, m.p1, (int64_t)m.ldp, (const double*)b.mu,
                       m.p0, nb_cs, nb_s, b.Sg, b.svec, b.bvec);
  VB_HIP(ctx, hipGetLastError());
  // C[i][j] = sum_k M[k][i] S[k][j]: the gradient product's form, lower tiles, split over k
  GemmArgs gc = gemm_product(M, r.ldz, b.Sg, r.ldl, D, D, D, 2);
  const EpiFoldSlabF ec{b.Cpart, r.ldl, r.slab, b.bvec, b.svec, b.Lt, r.ldl, b.fpart};
  if (r.cfgc == 4) {      // the blocks of colsum(G) behind the tiles, in the same launch
    const int gx = (int)gemm_f64_tri2_small_plan(&gc, r.csplits, r.n_cu), nb_tiles = gx * r.csplits;
    if (gx == 0) return fail(ctx, VB_ERR_STATE, "folded evaluation: D = %d does not go to the LDS-DMA product", D);
    constexpr size_t lds = (size_t)2 * (64 * kGemmBK + kGemmBK * 64) * sizeof(double);
    static_assert(lds >= 64 * 4 * sizeof(fr_d2), "the colsum(G) blocks' LDS is the tiles'");
    static bool configured_c = false;
    if (!configured_c) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&fr_fold_ctile_csg_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds);
      configured_c = true;
    }
    hipLaunchKernelGGL(fr_fold_ctile_csg_kernel, dim3((unsigned)(nb_tiles + nb_cs)), dim3(256), lds, st, gc, ec, gx, nb_tiles,
                       (const double*)b.colpart, r.splits, r.ldz, D, M, (const double*)b.bvec, (double)r.n, b.csg);
    VB_HIP(ctx, hipGetLastError());
    *tiles3 = (unsigned)gx;
    return VB_OK;
  }
  if (r.cfgc == 2) VB_TRY(tri2_tile_map(ctx, D, 128, 64, &gc.tile_map, &gc.tile_blocks));
  *tiles3 = gemm_f64_launch<false>(st, gc, r.csplits, r.n_cu, ec, r.cfgc);
  VB_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(fr_fold_csg_kernel, dim3((unsigned)nb_cs), dim3(256), 0, st, (const double*)b.colpart, r.splits, r.ldz, D, M,
                     (const double*)b.bvec, (double)r.n, b.csg);
  VB_HIP(ctx, hipGetLastError());
  return VB_OK;
}

// Model, correlated Gaussian: G = -(Z - m) P,  P symmetric: B[k][j] = P[k][j].  Returns the G the later stages read (the
// caller's where it brought it) and, in *tiles2, the number of sum-f partials where the route forms f here.
static int fr_model_gauss_full(vb_ctx* ctx, const FrRoute& r, const FrBufs& b, const ModelDev& m, const double* row_scale,
                               const double* g_ready, double** G, unsigned* tiles2) {
  hipStream_t st = ctx->stream;
  const int D = r.D;
  *G = b.G;
  GemmArgs g2 = gemm_product(b.Z, r.ldz, m.p1, m.ldp, (int)r.n, D, D, 0);
  switch (r.dense) {
    case kDenseNoG:      // (nothing to do here: M = L' P rides in the slab-sum launch behind the Gram product, fr_grad_folded)
      return VB_OK;
    case kDenseCallerG:
      *G = const_cast<double*>(g_ready);
      return VB_OK;
    case kDensePersistent: {      // (and, fz_mode 3, the split slabs of C): vb_fullrank_fused.h
      const GemmArgs g1 = gemm_product(b.E, b.lde, b.Lt, r.ldl, (int)r.n, D, D, r.tri1);
      GemmArgs g3f = gemm_product(b.G, r.ldz, b.E, b.lde, D, D, (int)r.n, 2);
      if (r.fz_mode == 3) VB_TRY(tri2_tile_map(ctx, D, 128, 64, &g3f.tile_map, &g3f.tile_blocks));
      return fr_fused_enqueue(ctx, st, r.fz_mode, g1, g2, g3f, r.splits, b.Z, b.G, r.ldz, b.mu, m.p0, b.fpart,
                              EpiSplitSlabCs{b.Cpart, r.ldl, r.slab, b.colpart, r.ldz}, tiles2);
    }
    case kDenseChain:
      break;
  }
  fr_sample(ctx, r, b, m.p0, row_scale, nullptr);      // Z - m
  VB_HIP(ctx, hipGetLastError());
  if (r.model_ksplit) {
    gemm_f64_launch<true>(st, g2, r.kparts, r.n_cu, EpiSplitSlab{b.Cpart, r.ldz, r.pslab});
    hipLaunchKernelGGL(fr_gsum_kernel, dim3(r.sum_blocks), dim3(256), 0, st, (const double*)b.Cpart, r.kparts, r.pslab, r.n, D,
                       r.ldz, (const double*)b.Z, b.G, b.fpart);
    *tiles2 = r.sum_blocks;
    return VB_OK;
  }
  prof_events(ctx, &g2.ev0, &g2.ev1, 1, VB_PROF_FR_MODEL_GEMM);
  if (r.fused_sums) *tiles2 = gemm_f64_launch<true>(st, g2, 1, r.n_cu, EpiNegateF{b.G, r.ldz, b.Z, b.fpart});
  else gemm_f64_launch<true>(st, g2, 1, r.n_cu, EpiNegate{b.G, r.ldz});
  return VB_OK;
}

// the pass over G (and Z) between the products: column sums of G and, per fmode, the f partials
static int fr_colpass(vb_ctx* ctx, const FrRoute& r, const FrBufs& b, const ModelDev& m, double* G, const double* Z, int fmode,
                      double* fpart, const double* row_scale) {
  hipLaunchKernelGGL(fr_colsum_kernel, dim3((unsigned)r.cs_gx, (unsigned)r.n_rb), dim3(256), 0, ctx->stream, (const double*)G, Z,
                     r.ldz, r.n, r.D, fmode, m.p1, b.colpart, fpart, r.glm ? 1.0 / (m.tau * m.tau) : 0.0,
                     (const double*)nullptr, 0, row_scale ? G : (double*)nullptr, row_scale);
  VB_HIP(ctx, hipGetLastError());
  return VB_OK;
}

static int fr_rowscale(vb_ctx* ctx, const FrRoute& r, double* G, const double* w) {
  hipLaunchKernelGGL(fr_rowscale_kernel, dim3((unsigned)r.n, (unsigned)((r.D + 255) / 256)), dim3(256), 0, ctx->stream, G, r.ldz,
                     r.n, r.D, w);
  VB_HIP(ctx, hipGetLastError());
  return VB_OK;
}

// Score (path derivative): the column pass for f first where the route wants two, then G~ = G + E L^-1
// (L^-1[k][j] = 0 for k < j: tri_mode 3)
static int fr_score(vb_ctx* ctx, const FrRoute& r, const FrBufs& b, const ModelDev& m, double* G, const double* Z) {
  if (r.two_passes) VB_TRY(fr_colpass(ctx, r, b, m, G, Z, r.fmode, b.fpart, nullptr));
  const GemmArgs gy = gemm_product(b.E, b.lde, b.T, r.ldl, (int)r.n, r.D, r.D, 3);
  gemm_f64_launch<true>(ctx->stream, gy, 1, r.n_cu, EpiAccumulate{G, r.ldz});
  VB_HIP(ctx, hipGetLastError());
  return VB_OK;
}

// GEMM 3: C[i][j] = sum_n G[n][i] E[n][j]: lower-triangular tiles (all tiles for the t family), split over the sample
// axis.  Returns in *tiles3 the number of output tiles of the launch.
static int fr_grad_product(vb_ctx* ctx, const FrRoute& r, const FrBufs& b, const ModelDev& m, const double* G,
                           unsigned* tiles3) {
  hipStream_t st = ctx->stream;
  *tiles3 = 0;
  if (r.fold) return fr_grad_folded(ctx, r, b, m, tiles3);     // (no G: from the noise's Gram matrix)
  if (!r.grad_launch) return VB_OK;
  GemmArgs g3 = gemm_product(G, r.ldz, b.E, b.lde, r.D, r.D, (int)r.n, r.tri3);
  prof_events(ctx, &g3.ev0, &g3.ev1, 1, VB_PROF_FR_GRAD_GEMM);
  if (r.cfg3 == 2) VB_TRY(tri2_tile_map(ctx, r.D, 128, 64, &g3.tile_map, &g3.tile_blocks));
  if (r.grad_colsums)
    *tiles3 = gemm_f64_launch<false>(st, g3, r.splits, r.n_cu, EpiSplitSlabCs{b.Cpart, r.ldl, r.slab, b.colpart, r.ldz}, r.cfg3);
  else
    *tiles3 = gemm_f64_launch<false>(st, g3, r.splits, r.n_cu, EpiSplitSlab{b.Cpart, r.ldl, r.slab});
  VB_HIP(ctx, hipGetLastError());
  return VB_OK;
}

// Finish, t family: the raw sums [F | sum g | sum_n g_n (e_n / s_n)' (full D x D)], all-reduced
static int fr_finish_mvt(vb_ctx* ctx, const FrRoute& r, const FrBufs& b, FrSums* sums_out) {
  fr_reduce_launch(ctx, ctx->stream, (const double*)b.Cpart, r.splits, r.slab, r.D, r.ldl, (const double*)b.colpart, r.n_rb, r.ldz,
                   (const double*)b.fpart, r.n_fpart, b.S, 1, nullptr);
  VB_HIP(ctx, hipGetLastError());
  if (ctx->comm) VB_TRY(comm_allreduce_sum(ctx, ctx->stream, b.S.sums, (size_t)b.S.len));
  *sums_out = b.S;
  return VB_OK;
}

// Finish, dense family: the split reduction (rows of column sums and f partials as the route left them); on a single GPU
// it writes (value, grad) itself, in a job its sums are all-reduced and the epilogue follows -- on `post` behind one
// event when the evaluation overlaps the next (fr_stream_plan)
static int fr_finish_dense(vb_ctx* ctx, const FrRoute& r, const FrBufs& b, const ModelDev& m, int set, int n_fpart_red,
                           const double* theta_dev, double* out_dev, int64_t n_total, const FrWeighted& wm) {
  hipStream_t st = ctx->stream;
  // one row of column sums per split; the folded evaluation: its slabs of C, the one row colsum(G)
  const int D = r.D, n_rb_red = r.fold ? 1 : (r.grad_colsums || !r.grad_launch) ? r.splits : r.n_rb;
  const int splits = r.fold ? r.csplits : r.splits;
  const double* colpart = r.fold ? b.csg : b.colpart;
  const int64_t red_items = r.slab / 2 > r.ldz ? r.slab / 2 : r.ldz;
  const dim3 red_grid((unsigned)((red_items + 255) / 256) + (r.fold ? 1u : 0u));
  const double *fold_mu = r.fold ? (const double*)b.mu : nullptr, *fold_m = r.fold ? m.p0 : nullptr;
  if (!ctx->comm) {   // single GPU
    hipLaunchKernelGGL(fr_reduce_packed_kernel<true>, red_grid, dim3(256), 0, st, (const double*)b.Cpart, splits, r.slab, D,
                       r.ldl, colpart, n_rb_red, r.ldz, (const double*)b.fpart, n_fpart_red, b.S, theta_dev,
                       (double)n_total, (double)n_total, m.c0, out_dev, r.pd ? 1 : 0, wm, fold_mu, fold_m);
    VB_HIP(ctx, hipGetLastError());
    return VB_OK;
  }
  hipLaunchKernelGGL(fr_reduce_packed_kernel<false>, red_grid, dim3(256), 0, st, (const double*)b.Cpart, splits, r.slab, D,
                     r.ldl, colpart, n_rb_red, r.ldz, (const double*)b.fpart, n_fpart_red, b.S, theta_dev,
                     (double)n_total, (double)n_total, m.c0, out_dev, r.pd ? 1 : 0, wm, fold_mu, fold_m);
  VB_HIP(ctx, hipGetLastError());
  Pipeline& P = ctx->pipe;
  hipStream_t st_post = st;
  if (r.overlap) {
    VB_HIP(ctx, hipEventRecord(P.ev_k1[set], st));
    st_post = P.post;
    VB_HIP(ctx, hipStreamWaitEvent(st_post, P.ev_k1[set], 0));
  }
  VB_TRY(comm_allreduce_sum(ctx, st_post, b.S.sums, (size_t)b.S.len));
  // one workgroup per CU: 328 -> 310 us per evaluation with a one-rank communicator (64: 312, 16: 350 -- the epilogue
  // then is what the evaluation after next waits for; unlimited = 2 050 workgroups: 328)
  const int64_t epi_full = (r.np + 255) / 256;
  const unsigned epi_grid = (unsigned)((r.overlap && epi_full > r.n_cu) ? r.n_cu : epi_full);
  hipLaunchKernelGGL(fr_epilogue_packed_kernel, dim3(epi_grid), dim3(256), 0, st_post, b.S, theta_dev, D, (double)n_total,
                     (double)n_total, m.c0, out_dev, r.pd ? 1 : 0, wm);
  VB_HIP(ctx, hipGetLastError());
  if (r.overlap) {
    VB_HIP(ctx, hipEventRecord(P.ev_fin[set], st_post));
    P.fin_valid[set] = true;
    P.post_pending = true;
    P.last_set = set;
  }
  return VB_OK;
}

// theta_dev != nullptr: full-rank Gaussian (Z = E L' + mu, lower-triangular gradient, epilogue into the flat layout).
// theta_dev == nullptr: multivariate t (X = (E R) / s + mu with the dense symmetric root R and the per-row scale
// `row_scale`; the caller gets the raw sums [F | sum g | sum_n g_n (e_n / s_n)' (full D x D)] in `sums_out`).
int fr_pipeline_enqueue(vb_ctx* ctx, const NoiseSlot& ns, int64_t n, int64_t d, int64_t n_total,
                        const double* theta_dev, double* out_dev, const double* mu_dev, const double* root_dev,
                        const double* row_scale, FrSums* sums_out, unsigned flags, const FrWeighted* weighted) {
  const ModelDev& m = ctx->model;
  const bool mvt = theta_dev == nullptr;
  FrWeighted wm;
  wm.roww = nullptr;
  wm.scale = 0.0;
  wm.wsum = wm.value = nullptr;
  if (weighted) {   // the t family takes the weighted raw sums (wm.scale / wsum / value are the caller's there)
    if (flags & VB_FLAG_PATH_DERIV)
      return fail(ctx, VB_ERR_UNSUPPORTED, "weighted sums: entropy-form pipeline only");
    wm = *weighted;
  }
  const bool pd = (flags & VB_FLAG_PATH_DERIV) != 0;
  if (pd && mvt) return fail(ctx, VB_ERR_UNSUPPORTED, "path derivative: dense Gaussian family only");
  if (m.id != VB_MODEL_GAUSS_DIAG && m.id != VB_MODEL_FUNNEL && m.id != VB_MODEL_GAUSS_FULL && m.id != VB_MODEL_LOGISTIC &&
      !model_has_rows(m.id))
    return fail(ctx, VB_ERR_UNSUPPORTED, "full-rank path: unsupported model id %d", m.id);
  if (m.dim != d)
    return fail(ctx, VB_ERR_INVALID, "model dimension %d != family dimension %lld", m.dim, (long long)d);
  if (n <= 0 || d <= 0 || n > ns.n || d != ns.d)
    return fail(ctx, VB_ERR_INVALID, "noise slot holds %lld x %lld, evaluation asks %lld x %lld",
                (long long)ns.n, (long long)ns.d, (long long)n, (long long)d);

  const FrRoute r = fr_route(ctx, m, n, d, mvt, pd, row_scale != nullptr, wm);
  int set = 0;
  FrBufs b;
  VB_TRY(fr_stream_plan(ctx, r, &set));
  VB_TRY(fr_carve(ctx, r, ns, set, &b));
  ctx->fr_fold_m = r.fold ? b.Mf : nullptr;      // (vb_fullrank_fold_get_m)
  ctx->fr_fold_d = r.fold ? d : 0, ctx->fr_fold_ld = r.fold ? r.ldz : 0;

  if (mvt) VB_TRY(fr_prepare_mvt(ctx, r, b, mu_dev, root_dev));
  else VB_TRY(fr_prepare_dense(ctx, r, &b, theta_dev));
  if (pd) VB_TRY(fr_score_prologue(ctx, r, b, theta_dev));

  const double* Z = b.Z;
  double* G = b.G;
  unsigned tiles2 = 0, tiles3 = 0;      // partials of sum f that a reducing launch left behind
  if (m.id == VB_MODEL_GAUSS_DIAG) {
    tiles2 = fr_model_gauss_diag(ctx, r, b, m, row_scale);
  } else if (m.id == VB_MODEL_GAUSS_FULL) {
    VB_TRY(fr_model_gauss_full(ctx, r, b, m, row_scale, wm.g_ready, &G, &tiles2));
  } else {
    Z = fr_sample(ctx, r, b, nullptr, row_scale, wm.z_ready);
    VB_HIP(ctx, hipGetLastError());
    if (m.id == VB_MODEL_FUNNEL) VB_TRY(fr_model_funnel(ctx, r, b, m, Z, wm.roww));
    else if (r.source) VB_TRY(fr_model_source(ctx, r, b, Z));
    else VB_TRY(fr_model_glm(ctx, r, b, m, Z));
  }
  VB_HIP(ctx, hipGetLastError());

  if (r.scale_rows_w) VB_TRY(fr_rowscale(ctx, r, G, wm.roww));   // weighted sums: before anything is summed
  if (pd) VB_TRY(fr_score(ctx, r, b, m, G, Z));
  if (r.colpass)
    VB_TRY(fr_colpass(ctx, r, b, m, G, Z, r.two_passes ? 0 : r.fmode, r.colpass_keeps_f ? b.fpart : b.fpart + r.n_fpart,
                      row_scale));
  else if (row_scale) VB_TRY(fr_rowscale(ctx, r, G, row_scale));
  VB_TRY(fr_grad_product(ctx, r, b, m, G, &tiles3));

  if (mvt) return fr_finish_mvt(ctx, r, b, sums_out);
  const int n_fpart_red = r.fold ? (int)tiles3 * r.csplits : r.f_per_tile ? (int)tiles2 : r.n_fpart;
  return fr_finish_dense(ctx, r, b, m, set, n_fpart_red, theta_dev, out_dev, n_total, wm);
}

// Z = E L' + mu into `Z` (n x ldz, ldz = round_up(d, 16)): the samples themselves, for per-row evaluations.
// theta_dev == nullptr: Z = (E root) * row_scale + mu with a full `root` (row stride ldz) as the t family has it
int fr_sample_enqueue(vb_ctx* ctx, const NoiseSlot& ns, int64_t n, int64_t d, const double* theta_dev, double* Z,
                      const double* mu_dev, const double* root_dev, const double* row_scale) {
  if (n <= 0 || d <= 0 || n > ns.n || d != ns.d) return fail(ctx, VB_ERR_INVALID, "noise slot shape mismatch");
  const int D = (int)d;
  const int64_t ldl = round_up(d, 16), ldz = ldl;
  hipStream_t st = ctx->stream;
  const double* E = (const double*)ns.buf.ptr;
  const int n_cu = ctx->prop.multiProcessorCount;
  ctx->fr_fold_m = nullptr, ctx->fr_fold_d = ctx->fr_fold_ld = 0;      // (fr_work is rewritten)
  if (theta_dev) {
    VB_TRY(ensure(ctx, ctx->fr_work, (size_t)(ldz + d * ldl) * sizeof(double)));
    double* mu = (double*)ctx->fr_work.ptr;
    double* Lt = mu + ldz;
    hipLaunchKernelGGL(fr_unpack_kernel, dim3((unsigned)((d + 31) / 32), (unsigned)((d + 31) / 32)), dim3(256), 0, st, theta_dev, D, ldl,
                       Lt, mu);
    gemm_f64_launch<true>(st, gemm_product(E, ns.ld, Lt, ldl, (int)n, D, D, 1), 1, n_cu, EpiStoreZ{Z, ldz, mu, nullptr, row_scale});
  } else {
    gemm_f64_launch<true>(st, gemm_product(E, ns.ld, root_dev, ldl, (int)n, D, D, 0), 1, n_cu,
                          EpiStoreZ{Z, ldz, mu_dev, nullptr, row_scale});
  }
  VB_HIP(ctx, hipGetLastError());
  return VB_OK;
}

int fr_elbo_grad_enqueue(vb_ctx* ctx, const NoiseSlot& ns, int64_t n, int64_t d, int64_t n_total,
                         const double* theta_dev, double* out_dev, unsigned flags, const FrWeighted* weighted) {
  return fr_pipeline_enqueue(ctx, ns, n, d, n_total, theta_dev, out_dev, nullptr, nullptr, nullptr, nullptr, flags,
                             weighted);
}

}  // namespace vb

// ---- C ABI: a look at the folded evaluation's M = L' P and at the slab program of its tiles (include/viabel_hip.h) ---------
int vb_fullrank_fold_get_m(vb_ctx* ctx, double* M_host, int64_t d) {
  using namespace vb;
  if (!ctx || !M_host) return fail(ctx, VB_ERR_INVALID, "NULL argument");
  if (!ctx->fr_fold_m || ctx->fr_fold_d != d)
    return fail(ctx, VB_ERR_STATE, "the last full-rank evaluation was no folded one of dimension %lld", (long long)d);
  VB_HIP(ctx, hipSetDevice(ctx->device));
  VB_TRY(main_stream_write(ctx));
  VB_HIP(ctx, hipMemcpy2DAsync(M_host, (size_t)d * sizeof(double), ctx->fr_fold_m, (size_t)ctx->fr_fold_ld * sizeof(double),
                               (size_t)d * sizeof(double), (size_t)d, hipMemcpyDeviceToHost, ctx->stream));
  VB_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return VB_OK;
}

int vb_fold_m_team_plan(int d, int pair, int* out8) {
  using namespace vb;
  if (!out8 || d <= 0 || d % kGemmBK != 0) return VB_ERR_INVALID;
  const int tiles_m = gemm_tiles(d, 64);
  if (pair < 0 || pair >= (tiles_m + 1) / 2) return VB_ERR_INVALID;
  const GemmTeamPlan p = gemm_f64_team_plan(d, d, tiles_m, pair);
  const int out[8] = {p.H, p.n_h, p.n_l, p.cnt0, p.cnt1, p.sw, gemm_f64_team_barriers(p, 0), gemm_f64_team_barriers(p, 1)};
  for (int i = 0; i < 8; ++i) out8[i] = out[i];
  return VB_OK;
}

int vb_gemm_plan(int m, int n, int k, int splits, int n_cu, int tri_mode, int batch, int a_kcontig, int narrow_ok,
                 int narrow_auto, int cfg, int flags, int* out6) {
  using namespace vb;
  if (!out6 || m <= 0 || n <= 0 || k <= 0 || splits <= 0 || n_cu <= 0) return VB_ERR_INVALID;
  if (tri_mode < 0 || tri_mode > 4 || batch < 0 || cfg < 0 || cfg > 8 || flags < 0) return VB_ERR_INVALID;
  const GemmPlan p = gemm_f64_plan(m, n, k, splits, n_cu, tri_mode, batch, a_kcontig != 0, narrow_ok != 0, narrow_auto != 0, cfg,
                                   flags);
  const int out[6] = {p.cfg, p.dma ? 1 : 0, p.bm_rows, p.bn_cols, p.k_split, (int)p.grid_x};
  for (int i = 0; i < 6; ++i) out6[i] = out[i];
  return VB_OK;
}

int vb_gram_splits_plan(int d, int64_t n, int n_cu, int* splits) {
  if (!splits || d <= 0 || n <= 0 || n_cu <= 0) return VB_ERR_INVALID;
  *splits = vb::gemm_gram_splits(d, n, n_cu);
  return VB_OK;
}

int vb_lowrank_splits_plan(int64_t n, int* splits) {
  if (!splits || n <= 0) return VB_ERR_INVALID;
  *splits = vb::gemm_lr_splits(n);
  return VB_OK;
}
