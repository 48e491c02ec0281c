// Kernel Stein discrepancy of weighted draws (vb_ksd): IMQ base kernel k(x, y) = (c^2 + |x - y|^2)^beta,
// Gorham & Mackey 2017.  With x~ = x / scale, g~ = grad log p(x) * scale and, per pair, sums over the D coordinates
//   r2 = sum (x~_i - x~_j)^2      a = sum g~_i g~_j      b = sum (g~_i - g~_j)(x~_i - x~_j)      u = c^2 + r2
//   k_p(i, j) = a u^beta - 2 beta u^(beta-1) (b + D) - 4 beta (beta - 1) r2 u^(beta-2)
//   rowsums[i] = sum_j w_j k_p(i, j)          ksd2 = sum_i w_i rowsums[i]
// DIFFERENCE FORM: r2 and b are accumulated from the differences themselves, never assembled from Gram products
// (|x_i|^2 + |x_j|^2 - 2 x_i . x_j cancels catastrophically for draws far from the origin relative to their spread), so
// this is a VALU kernel -- two subtractions and three FMAs per pair and coordinate -- and not three MFMA products.
//
//   ksd_stage_kernel   X~, G~ in place (round_up(s, 64) rows of round_up(d, 16) columns, padding zeroed), padded weights 0
//   ksd_pair_kernel    one workgroup per (row block of 64 draws, column split): the hot path, one partial per (row, split)
//   ksd_finish_kernel  rowsums = the partials in split order, ksd2 = sum_i w_i rowsums[i] in one workgroup's fixed tree
// Nothing of order S^2 is stored, no floating-point atomics: two calls with the same inputs return the same bits.
// The pair tile's constants and draw order (pair_draw), the 256-thread sum and the host's refusals, row copies, workspace
// carver and stream guard are vb_particles.h's, shared with vb_svgd.hip.
#include <cmath>
#include <vector>

#include "vb_particles.h"

namespace vb {

constexpr int64_t kKsdMaxDraws = 65536;

struct KsdStageArgs {
  double* X;                // in: x rows (stride ld), out: x / scale
  double* G;                // in: score rows, out: score * scale
  double* w;                // [sp]: entries [s, sp) are zeroed
  const double* scale;      // [d] or nullptr (ones)
  int64_t s, sp, ld;
  int d;
};

// grid = sp rows; in place: every element is read and written by the same thread
__global__ void __launch_bounds__(256) ksd_stage_kernel(const KsdStageArgs a) {
  const int64_t row = blockIdx.x;
  double* x = a.X + row * a.ld;
  double* g = a.G + row * a.ld;
  const bool live = row < a.s;
  for (int c = threadIdx.x; c < (int)a.ld; c += 256) {
    double xv = 0.0, gv = 0.0;
    if (live && c < a.d) {
      const double l = a.scale ? a.scale[c] : 1.0;
      xv = x[c] / l;
      gv = g[c] * l;
    }
    x[c] = xv;
    g[c] = gv;
  }
  if (!live && threadIdx.x == 0) a.w[row] = 0.0;
}

struct KsdPairArgs {
  const double* X;          // [sp x ld] staged draws
  const double* G;          // [sp x ld] staged scores
  const double* w;          // [sp] normalised weights, 0 on padded rows
  double* partial;          // [splits x sp]
  int64_t ld, sp;
  int tiles, splits;
  double c2, beta, dim;     // c^2, beta, D as a double
};

// tiles [first, last) of column split `split`: contiguous ranges whose lengths differ by at most one
__host__ __device__ __forceinline__ int ksd_split_first(int split, int tiles, int splits) {
  return (int)((int64_t)split * tiles / splits);
}

__global__ void __launch_bounds__(256) ksd_pair_kernel(const KsdPairArgs a) {
  // [Xi | Gi | Xj | Gj][coordinate][draw]
  __shared__ __attribute__((aligned(16))) double sh[4][kPairK][kPairLdsRow];
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;       // columns / rows of the thread's 4 x 4 pairs
  const int lr = tid >> 2, lq = tid & 3;        // staging: draw lr of the tile, coordinates 2 lq, 2 lq + 1, 8 + 2 lq, 9 + 2 lq
  const int rb = blockIdx.x, split = blockIdx.y;
  const int t0 = ksd_split_first(split, a.tiles, a.splits), t1 = ksd_split_first(split + 1, a.tiles, a.splits);
  const int nk = (int)(a.ld / kPairK);
  const int64_t off_i = ((int64_t)rb * kPairTile + lr) * a.ld + 2 * lq;
  const double mb2 = -2.0 * a.beta, mb4 = -4.0 * a.beta * (a.beta - 1.0), bm2 = a.beta - 2.0;

  double rowacc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int t = t0; t < t1; ++t) {
    const int64_t off_j = ((int64_t)t * kPairTile + lr) * a.ld + 2 * lq;
    double r2[4][4], aa[4][4], bb[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) r2[i][j] = 0.0, aa[i][j] = 0.0, bb[i][j] = 0.0;

    double2 pre[4][2];                          // the next step's 16 doubles of this thread
    auto fetch = [&](int ks) {
      const int64_t k0 = (int64_t)ks * kPairK;
      const double* src[4] = {a.X + off_i + k0, a.G + off_i + k0, a.X + off_j + k0, a.G + off_j + k0};
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        pre[m][0] = *reinterpret_cast<const double2*>(src[m]);
        pre[m][1] = *reinterpret_cast<const double2*>(src[m] + 8);
      }
    };
    fetch(0);
    for (int ks = 0; ks < nk; ++ks) {
      __syncthreads();                          // the previous step's reads are done
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        sh[m][2 * lq][lr] = pre[m][0].x;
        sh[m][2 * lq + 1][lr] = pre[m][0].y;
        sh[m][8 + 2 * lq][lr] = pre[m][1].x;
        sh[m][9 + 2 * lq][lr] = pre[m][1].y;
      }
      __syncthreads();
      if (ks + 1 < nk) fetch(ks + 1);
#pragma unroll 4
      for (int k = 0; k < kPairK; ++k) {
        double xi[4], gi[4], xj[4], gj[4];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const double2 v0 = *reinterpret_cast<const double2*>(&sh[0][k][h * 32 + ty * 2]);
          const double2 v1 = *reinterpret_cast<const double2*>(&sh[1][k][h * 32 + ty * 2]);
          const double2 v2 = *reinterpret_cast<const double2*>(&sh[2][k][h * 32 + tx * 2]);
          const double2 v3 = *reinterpret_cast<const double2*>(&sh[3][k][h * 32 + tx * 2]);
          xi[2 * h] = v0.x, xi[2 * h + 1] = v0.y;
          gi[2 * h] = v1.x, gi[2 * h + 1] = v1.y;
          xj[2 * h] = v2.x, xj[2 * h + 1] = v2.y;
          gj[2 * h] = v3.x, gj[2 * h + 1] = v3.y;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const double dx = xi[i] - xj[j], dg = gi[i] - gj[j];
            r2[i][j] = fma(dx, dx, r2[i][j]);
            aa[i][j] = fma(gi[i], gj[j], aa[i][j]);
            bb[i][j] = fma(dg, dx, bb[i][j]);
          }
      }
    }

    // the tile's Stein kernel values, weighted and summed over its columns: the thread's four, then the 16 threads that
    // share the rows in a fixed butterfly (every lane ends with the same bits)
    double wj[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) wj[j] = a.w[(int64_t)t * kPairTile + pair_draw(tx, j)];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      double v = 0.0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double u = a.c2 + r2[i][j];
        const double p2 = pow(u, bm2), p1 = p2 * u, p0 = p1 * u;      // u^(beta-2), u^(beta-1), u^beta
        const double kp = fma(aa[i][j], p0, fma(mb2 * p1, bb[i][j] + a.dim, mb4 * r2[i][j] * p2));
        v = fma(wj[j], kp, v);
      }
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 16);
      rowacc[i] += v;
    }
  }
  if (tx == 0) {
    double* out = a.partial + (int64_t)split * a.sp + (int64_t)rb * kPairTile;
#pragma unroll
    for (int i = 0; i < 4; ++i) out[pair_draw(ty, i)] = rowacc[i];
  }
}

// one workgroup: rowsums[i] = the row's partials in split order; ksd2 = sum_i w_i rowsums[i], thread t taking rows
// t + 256 k in order
__global__ void __launch_bounds__(256) ksd_finish_kernel(const double* __restrict__ partial, const double* __restrict__ w,
                                                          int64_t s, int64_t sp, int splits, double* __restrict__ rowsums,
                                                          double* __restrict__ ksd2) {
  __shared__ double sh[4];
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < s; i += 256) {
    double r = 0.0;
    for (int c = 0; c < splits; ++c) r += partial[(int64_t)c * sp + i];
    rowsums[i] = r;
    acc = fma(w[i], r, acc);
  }
  acc = block_sum(acc, sh);
  if (threadIdx.x == 0) *ksd2 = acc;
}

// Where the pieces of a call live in ctx->ksd_work (doubles from the base)
struct KsdLayout {
  int64_t sp, ld;
  int tiles, splits;
  int64_t o_x, o_g, o_w, o_f, o_scale, o_part, o_rows, o_out, total;
};
static void ksd_plan(int64_t s, int n_cu, int* row_blocks, int* splits) {
  const int64_t tiles = (s + kPairTile - 1) / kPairTile;
  // two workgroups per compute unit (what the pair kernel's registers allow) when the column tiles can be dealt that far
  int64_t sp = (2 * (int64_t)n_cu + tiles - 1) / tiles;
  sp = sp < 1 ? 1 : (sp > tiles ? tiles : sp);
  *row_blocks = (int)tiles, *splits = (int)sp;
}
static KsdLayout ksd_layout(int64_t s, int64_t d, int n_cu) {
  KsdLayout L;
  L.sp = round_up(s, kPairTile), L.ld = round_up(d, 16);
  ksd_plan(s, n_cu, &L.tiles, &L.splits);
  Carver carve;
  L.o_x = carve(L.sp * L.ld), L.o_g = carve(L.sp * L.ld), L.o_w = carve(L.sp), L.o_f = carve(L.sp), L.o_scale = carve(L.ld),
  L.o_part = carve((int64_t)L.splits * L.sp), L.o_rows = carve(L.sp), L.o_out = carve(16);
  L.total = carve.off;
  return L;
}

}  // namespace vb

using namespace vb;

extern "C" {

int vb_ksd_plan(int64_t s, int n_cu, int out[2]) {
  if (!out || s < 1 || s > kKsdMaxDraws || n_cu < 1) return VB_ERR_INVALID;
  ksd_plan(s, n_cu, &out[0], &out[1]);
  return VB_OK;
}

int vb_ksd(vb_ctx* ctx, const double* x, int64_t s, int64_t d, const double* scores, const double* log_w,
           const double* scale, double c, double beta, double* ksd2, double* rowsums) {
  if (!ctx || !x || !ksd2) return fail(ctx, VB_ERR_INVALID, "NULL argument");
  if (s < 1) return fail(ctx, VB_ERR_INVALID, "the number of draws must be positive");
  if (s > kKsdMaxDraws)
    return fail(ctx, VB_ERR_UNSUPPORTED, "vb_ksd takes at most %lld draws (got %lld)", (long long)kKsdMaxDraws, (long long)s);
  if (d < 1 || d > 0x7fffffffll - 16) return fail(ctx, VB_ERR_INVALID, "the dimension must be positive");
  if (!(c > 0.0) || !std::isfinite(c)) return fail(ctx, VB_ERR_INVALID, "c must be positive and finite");
  if (!(beta > -1.0 && beta < 0.0)) return fail(ctx, VB_ERR_INVALID, "beta must lie in (-1, 0)");
  if (scale) VB_TRY(positive_finite(ctx, "vb_ksd", "scale", scale, d));
  if (!scores) {
    VB_TRY(model_bound_refuse(ctx, "vb_ksd", "x", d, ", or pass scores"));
    VB_TRY(model_device_refuse(ctx, "vb_ksd", true, false, ", or pass scores"));
  }
  std::vector<double> wv;
  if (!predict_weights(log_w, s, wv)) return fail(ctx, VB_ERR_INVALID, "no log weight is finite (or one is NaN or +inf)");
  VB_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  StreamDrain drain{st};
  const KsdLayout L = ksd_layout(s, d, ctx->prop.multiProcessorCount);
  VB_TRY(ensure(ctx, ctx->ksd_work, (size_t)L.total * sizeof(double)));
  double* base = (double*)ctx->ksd_work.ptr;
  double *X = base + L.o_x, *G = base + L.o_g, *w = base + L.o_w;
  // the s live rows: padding columns zero for the model's row kernels; the staging kernel zeroes them again, and the rows
  // past s, and is the first to read the scores' pads
  VB_TRY(upload_rows(ctx, X, x, s, d, L.ld));
  if (scores)
    VB_TRY(upload_rows(ctx, G, scores, s, d, L.ld, false));
  else
    VB_TRY(model_grad_rows(ctx, X, L.ld, s, d, G, base + L.o_f));
  VB_HIP(ctx, hipMemcpyAsync(w, wv.data(), (size_t)s * sizeof(double), hipMemcpyHostToDevice, st));
  if (scale) VB_HIP(ctx, hipMemcpyAsync(base + L.o_scale, scale, (size_t)d * sizeof(double), hipMemcpyHostToDevice, st));

  const KsdStageArgs sa{X, G, w, scale ? base + L.o_scale : nullptr, s, L.sp, L.ld, (int)d};
  hipLaunchKernelGGL(ksd_stage_kernel, dim3((unsigned)L.sp), dim3(256), 0, st, sa);
  VB_HIP(ctx, hipGetLastError());
  const KsdPairArgs pa{X, G, w, base + L.o_part, L.ld, L.sp, L.tiles, L.splits, c * c, beta, (double)d};
  hipLaunchKernelGGL(ksd_pair_kernel, dim3((unsigned)L.tiles, (unsigned)L.splits), dim3(256), 0, st, pa);
  VB_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(ksd_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)(base + L.o_part), (const double*)w, s, L.sp,
                     L.splits, base + L.o_rows, base + L.o_out);
  VB_HIP(ctx, hipGetLastError());
  double result = 0.0;
  VB_HIP(ctx, hipMemcpyAsync(&result, base + L.o_out, sizeof(double), hipMemcpyDeviceToHost, st));
  if (rowsums) VB_HIP(ctx, hipMemcpyAsync(rowsums, base + L.o_rows, (size_t)s * sizeof(double), hipMemcpyDeviceToHost, st));
  VB_HIP(ctx, hipStreamSynchronize(st));
  *ksd2 = result;
  if (!std::isfinite(result))
    return fail(ctx, VB_ERR_NUMERIC, "the discrepancy is not finite: a draw or its score is not finite");
  return VB_OK;
}

}  // extern "C"
