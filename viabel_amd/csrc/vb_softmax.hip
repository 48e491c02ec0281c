// Multinomial logistic (softmax) regression target, VB_MODEL_SOFTMAX: the one built-in target whose likelihood couples
// several linear predictors of an observation, so it is not an element-wise epilogue of eta = Z X'.
//
//   theta = [b_0 | ... | b_{C-1}] (class-major, b_c of length p), eta_ic = x_i' b_c
//   f(theta) = sum_i [eta_{i, y_i} - logsumexp_c eta_ic] - |theta|^2 / (2 sd^2) - C p (log sd + log(2 pi) / 2)
//   d f / d b_c = sum_i ([y_i = c] - softmax_c(eta_i)) x_i - b_c / sd^2
//
// Per chunk of samples (rows of Z), with the class blocks of a sample taken as C rows of a packed matrix:
//   pack      Zc[(r C + c)][j] = Z[r][c p + j]          (the rows (r, c) of Z have no uniform stride: a copy, one pass)
//   GEMM      H = Zc X'                                  [(rows C) x n_data x p], fp64 MFMA, plain store
//   couple    per (r, i): max_c, logsumexp_c of H[(r C + c)][i]; log-likelihood partial of row r; with a gradient the C
//             values are overwritten by the residuals [y_i = c] - softmax_c
//   GEMM      Gc = R X - Zc / sd^2                       glm_grad_enqueue on the packed shapes (split over n_data included)
//   unpack    G[r][c p + j] = Gc[(r C + c)][j]
// and f[r] = sum of the row's strip partials (fixed order) - |z_r|^2 / (2 sd^2) + f0.  No atomics anywhere: two calls
// give the same bits.
#include "vb_common.h"
#include "vb_gemm_f64.h"

namespace vb {

namespace {

constexpr int kSmStrip = 1024;      // observations per workgroup of the coupling kernel: 256 lanes x 4

struct EpiStoreH {           // H = acc
  double* Y;
  int64_t ldy;
  __device__ void operator()(int, int row, int col, double acc) const { Y[(int64_t)row * ldy + col] = acc; }
  __device__ d2v pair(int, int row, int col, double a0, double a1) const {
    const d2v v = (d2v){a0, a1};
    *reinterpret_cast<d2v*>(Y + (int64_t)row * ldy + col) = v;
    return v;
  }
};

__global__ void __launch_bounds__(256) sm_pack_kernel(const double* __restrict__ Z, int64_t ldz, int64_t rows, int C, int p,
                                                      double* __restrict__ Zc, int64_t ldc) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * C * ldc) return;
  const int j = (int)(idx % ldc);
  const int64_t rc = idx / ldc;
  const int64_t r = rc / C;
  const int c = (int)(rc % C);
  Zc[idx] = j < p ? Z[r * ldz + (int64_t)c * p + j] : 0.0;      // (pad columns zero: the gradient epilogue reads pairs)
}

__global__ void __launch_bounds__(256) sm_unpack_kernel(const double* __restrict__ Gc, int64_t ldc, int64_t rows, int C, int p,
                                                        double* __restrict__ G, int64_t ldg) {
  const int64_t d = (int64_t)C * p;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * d) return;
  const int64_t r = idx / d;
  const int col = (int)(idx % d);
  const int c = col / p, j = col % p;
  G[r * ldg + col] = Gc[(r * C + c) * ldc + j];
}

// MODE 0: log-likelihood partials; 1: ... and H overwritten by the residuals; 2: the per-observation terms to LL, no sums.
// Workgroup (row r, strip s): lanes over consecutive observations, so each of the C class rows is read (and written) as
// contiguous 2-KiB runs; the class loop is the inner one and runs three times over values the first pass brought into
// the cache (maximum, sum of exponentials, residuals) -- C is a run-time number, so nothing is kept in an array.
template <int MODE>
__global__ void __launch_bounds__(256) sm_couple_kernel(double* __restrict__ H, int64_t ldh, int C, int n_data,
                                                        const double* __restrict__ y, int n_strips,
                                                        double* __restrict__ part, double* __restrict__ LL, int64_t ldl) {
  const int64_t r = blockIdx.x / n_strips;
  const int s = blockIdx.x % n_strips;
  double* __restrict__ Hr = H + r * C * ldh;
  double acc = 0.0;
#pragma unroll 1
  for (int u = 0; u < kSmStrip / 256; ++u) {
    const int i = s * kSmStrip + u * 256 + (int)threadIdx.x;
    if (i >= n_data) break;
    const int yi = (int)y[i];
    double mx = Hr[i];
    for (int c = 1; c < C; ++c) mx = fmax(mx, Hr[(int64_t)c * ldh + i]);
    double se = 0.0;
    for (int c = 0; c < C; ++c) se += exp(Hr[(int64_t)c * ldh + i] - mx);
    const double t = (Hr[(int64_t)yi * ldh + i] - mx) - log(se);      // eta_y - logsumexp, overflow-safe
    if (MODE == 2) LL[r * ldl + i] = t;
    else acc += t;
    if (MODE == 1) {
      const double inv = 1.0 / se;
      for (int c = 0; c < C; ++c) {
        const int64_t k = (int64_t)c * ldh + i;
        Hr[k] = (c == yi ? 1.0 : 0.0) - exp(Hr[k] - mx) * inv;
      }
    }
  }
  if (MODE == 2) return;
  __shared__ double wsum[4];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// f[r] = sum_s part[r][s] - |z_r|^2 / (2 sd^2) + f0: one wave per row, a lane adds its strips / columns in order
__global__ void __launch_bounds__(256) sm_rowsum_kernel(const double* __restrict__ part, int n_strips,
                                                        const double* __restrict__ Z, int64_t ldz, int d, double neg_half_ivp,
                                                        double f0, int64_t rows, double* __restrict__ f) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  double ll = 0.0, s2 = 0.0;
  for (int s = lane; s < n_strips; s += 64) ll += part[r * n_strips + s];
  for (int c = lane; c < d; c += 64) s2 = fma(Z[r * ldz + c], Z[r * ldz + c], s2);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    ll += __shfl_down(ll, off, 64);
    s2 += __shfl_down(s2, off, 64);
  }
  if (lane == 0) f[r] = fma(neg_half_ivp, s2, ll) + f0;
}

struct SmLayout {
  int64_t ldc, ldh, chunk, o_zc, o_h, o_gc, o_part, o_x, o_ll, total;
  int n_strips;
};

// rows per chunk bound H to kSoftmaxChunkDoubles; `pointwise`: room for the uploaded draws and the term matrix as well
SmLayout sm_layout(const ModelDev& m, int64_t n, bool grad, bool pointwise) {
  SmLayout L;
  const int64_t C = m.n_classes;
  L.ldc = round_up(m.n_feat, 16);
  L.ldh = m.ldq;
  L.n_strips = (int)((m.n_data + kSmStrip - 1) / kSmStrip);
  int64_t chunk = kSoftmaxChunkDoubles / (C * L.ldh);
  chunk = chunk < 8 ? 8 : chunk;
  L.chunk = chunk > n ? n : chunk;
  int64_t off = 0;
  auto carve = [&off](int64_t doubles) {      // (multiples of 32 doubles: every piece starts 256-B aligned)
    const int64_t o = off;
    off += round_up(doubles, 32);
    return o;
  };
  L.o_zc = carve(L.chunk * C * L.ldc);
  L.o_h = carve(L.chunk * C * L.ldh);
  L.o_gc = carve(grad ? L.chunk * C * L.ldc : 0);
  L.o_part = carve(L.chunk * L.n_strips);
  L.o_x = carve(pointwise ? L.chunk * round_up(m.dim, 16) : 0);
  L.o_ll = carve(pointwise ? L.chunk * L.ldh : 0);
  L.total = off;
  return L;
}

int sm_check(vb_ctx* ctx, int64_t n, int d) {
  const ModelDev& m = ctx->model;
  if (m.id != VB_MODEL_SOFTMAX) return fail(ctx, VB_ERR_STATE, "no softmax regression model bound");
  if (n <= 0 || d != m.dim) return fail(ctx, VB_ERR_INVALID, "softmax rows: %lld x %d samples for a model of dimension %d",
                                        (long long)n, d, m.dim);
  if (n * m.n_classes > 0x7fffffffll)
    return fail(ctx, VB_ERR_INVALID, "softmax rows: %lld samples x %d classes do not fit the GEMM's int shapes", (long long)n,
                m.n_classes);
  return VB_OK;
}

// pack -> H = Zc X' for `rows` samples starting at Z (the chunk's first row)
int sm_predictors(vb_ctx* ctx, hipStream_t st, const SmLayout& L, double* base, const double* Z, int64_t ldz, int64_t rows) {
  const ModelDev& m = ctx->model;
  const int C = m.n_classes, p = m.n_feat;
  const int64_t items = rows * C * L.ldc;
  if ((items + 255) / 256 > 0x7fffffffll) return fail(ctx, VB_ERR_INVALID, "softmax rows: packed chunk too large for one launch");
  hipLaunchKernelGGL(sm_pack_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, Z, ldz, rows, C, p, base + L.o_zc,
                     L.ldc);
  VB_HIP(ctx, hipGetLastError());
  const GemmArgs g = gemm_product(base + L.o_zc, L.ldc, m.p1, m.ldq, (int)(rows * C), (int)m.n_data, p, 0);
  gemm_f64_launch<true>(st, g, 1, ctx->prop.multiProcessorCount, EpiStoreH{base + L.o_h, L.ldh});
  VB_HIP(ctx, hipGetLastError());
  return VB_OK;
}

}  // namespace

int softmax_rows_enqueue(vb_ctx* ctx, hipStream_t st, const double* Z, int64_t ldz, int64_t n, int d, double* G, int64_t ldg,
                         double* f) {
  VB_TRY(sm_check(ctx, n, d));
  const ModelDev& m = ctx->model;
  const int C = m.n_classes, p = m.n_feat;
  const SmLayout L = sm_layout(m, n, G != nullptr, false);
  VB_TRY(ensure(ctx, ctx->sm_work, (size_t)L.total * sizeof(double)));
  double* base = (double*)ctx->sm_work.ptr;
  const double ivp = 1.0 / (m.tau * m.tau);
  for (int64_t r0 = 0; r0 < n; r0 += L.chunk) {
    const int64_t rows = n - r0 < L.chunk ? n - r0 : L.chunk;
    VB_TRY(sm_predictors(ctx, st, L, base, Z + r0 * ldz, ldz, rows));
    const dim3 cgrid((unsigned)(rows * L.n_strips));
    if (G)
      hipLaunchKernelGGL(sm_couple_kernel<1>, cgrid, dim3(256), 0, st, base + L.o_h, L.ldh, C, (int)m.n_data, m.p2, L.n_strips,
                         base + L.o_part, (double*)nullptr, (int64_t)0);
    else
      hipLaunchKernelGGL(sm_couple_kernel<0>, cgrid, dim3(256), 0, st, base + L.o_h, L.ldh, C, (int)m.n_data, m.p2, L.n_strips,
                         base + L.o_part, (double*)nullptr, (int64_t)0);
    VB_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(sm_rowsum_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, (const double*)(base + L.o_part),
                       L.n_strips, Z + r0 * ldz, ldz, d, -0.5 * ivp, m.f0, rows, f + r0);
    VB_HIP(ctx, hipGetLastError());
    if (!G) continue;
    VB_TRY(glm_grad_enqueue(ctx, st, m, base + L.o_h, L.ldh, base + L.o_zc, base + L.o_gc, L.ldc, rows * C, p));
    const int64_t items = rows * d;
    hipLaunchKernelGGL(sm_unpack_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st,
                       (const double*)(base + L.o_gc), L.ldc, rows, C, p, G + r0 * ldg, ldg);
    VB_HIP(ctx, hipGetLastError());
  }
  return VB_OK;
}

int model_rows_enqueue(vb_ctx* ctx, hipStream_t st, const double* Z, int64_t ldz, int64_t n, int d, double* G, int64_t ldg,
                       double* f) {
  if (ctx->model.id == VB_MODEL_SOFTMAX) return softmax_rows_enqueue(ctx, st, Z, ldz, n, d, G, ldg, f);
  if (ctx->model.id == VB_MODEL_MULTILEVEL) return multilevel_rows_enqueue(ctx, st, Z, ldz, n, d, G, ldg, f);
  if (ctx->model.id == VB_MODEL_LOCSCALE) return locscale_rows_enqueue(ctx, st, Z, ldz, n, d, G, ldg, f);
  if (ctx->model.id == VB_MODEL_SPARSE_GLM) return sparse_rows_enqueue(ctx, st, Z, ldz, n, d, G, ldg, f);
  return user_rows_enqueue(ctx, st, Z, ldz, n, d, G, ldg, f);
}

}  // namespace vb

using namespace vb;

extern "C" {

int vb_softmax_pointwise(vb_ctx* ctx, const double* x, int64_t s, int64_t d, double* ll_out) {
  if (!ctx || !x || !ll_out) return fail(ctx, VB_ERR_INVALID, "NULL argument");
  if (ctx->model.id < 0) return fail(ctx, VB_ERR_STATE, "no model bound (vb_set_model)");
  if (ctx->model.id != VB_MODEL_SOFTMAX)
    return fail(ctx, VB_ERR_UNSUPPORTED, "vb_softmax_pointwise needs a softmax regression target (model id %d bound)",
                ctx->model.id);
  if (d != ctx->model.dim)
    return fail(ctx, VB_ERR_INVALID, "x has %lld columns, model dimension is %d", (long long)d, ctx->model.dim);
  if (s <= 0) return fail(ctx, VB_ERR_INVALID, "the number of draws must be positive");
  VB_TRY(sm_check(ctx, s, (int)d));
  VB_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const ModelDev& m = ctx->model;
  const int64_t nd = m.n_data, ldx = round_up(d, 16);
  const SmLayout L = sm_layout(m, s, false, true);
  VB_TRY(ensure(ctx, ctx->sm_work, (size_t)L.total * sizeof(double)));
  double* base = (double*)ctx->sm_work.ptr;
  for (int64_t r0 = 0; r0 < s; r0 += L.chunk) {
    const int64_t rows = s - r0 < L.chunk ? s - r0 : L.chunk;
    VB_HIP(ctx, hipMemcpy2DAsync(base + L.o_x, (size_t)ldx * sizeof(double), x + r0 * d, (size_t)d * sizeof(double),
                                 (size_t)d * sizeof(double), (size_t)rows, hipMemcpyHostToDevice, st));
    VB_TRY(sm_predictors(ctx, st, L, base, base + L.o_x, ldx, rows));
    hipLaunchKernelGGL(sm_couple_kernel<2>, dim3((unsigned)(rows * L.n_strips)), dim3(256), 0, st, base + L.o_h, L.ldh,
                       m.n_classes, (int)nd, m.p2, L.n_strips, (double*)nullptr, base + L.o_ll, L.ldh);
    VB_HIP(ctx, hipGetLastError());
    VB_HIP(ctx, hipMemcpy2DAsync(ll_out + r0 * nd, (size_t)nd * sizeof(double), base + L.o_ll, (size_t)L.ldh * sizeof(double),
                                 (size_t)nd * sizeof(double), (size_t)rows, hipMemcpyDeviceToHost, st));
    VB_HIP(ctx, hipStreamSynchronize(st));
  }
  return VB_OK;
}

}  // extern "C"
