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
#include "vb_rows_target.h"

namespace vb {

namespace {

constexpr int kSmStrip = 1024;      // observations per workgroup of the coupling kernel: 256 lanes x 4

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
  strip_partials_store<1>(acc, 0.0, part);
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
  ll = wave_sum(ll);
  s2 = wave_sum(s2);
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
  L.chunk = rows_chunk(kSoftmaxChunkDoubles, C * L.ldh, n);
  Carver carve;
  L.o_zc = carve(L.chunk * C * L.ldc);
  L.o_h = carve(L.chunk * C * L.ldh);
  L.o_gc = carve(grad ? L.chunk * C * L.ldc : 0);
  L.o_part = carve(L.chunk * L.n_strips);
  L.o_x = carve(pointwise ? L.chunk * round_up(m.dim, 16) : 0);
  L.o_ll = carve(pointwise ? L.chunk * L.ldh : 0);
  L.total = carve.off;
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
  gemm_f64_launch<true>(st, g, 1, ctx->prop.multiProcessorCount, EpiStorePlain{base + L.o_h, L.ldh});
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
  VB_TRY(ensure(ctx, ctx->target_work, (size_t)L.total * sizeof(double)));
  double* base = (double*)ctx->target_work.ptr;
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

int softmax_set_model(vb_ctx* ctx, int64_t dim, const double* dparams, size_t n_dparams, const int64_t* iparams,
                      size_t n_iparams) {
  if (n_iparams != 2 || !iparams || !dparams || iparams[0] <= 0 || iparams[1] < 2 || dim % iparams[1] != 0 ||
      iparams[0] > 0x7fffffffll || dim > 0x7fffffffll ||
      n_dparams != (size_t)(iparams[0] * (dim / iparams[1]) + iparams[0]) + 1)
    return fail(ctx, VB_ERR_INVALID,
                "softmax regression expects dparams = [X(n_data x p) | y(n_data) | prior_sd], iparams = [n_data, n_classes] "
                "and a dimension of n_classes * p");
  const int64_t nd = iparams[0], nc = iparams[1], p = dim / nc;
  const double* ys = dparams + nd * p;
  const double sd = ys[nd];
  if (!(sd > 0.0)) return fail(ctx, VB_ERR_INVALID, "softmax prior_sd must be positive");
  for (int64_t i = 0; i < nd; ++i)
    if (!(ys[i] >= 0.0 && ys[i] < (double)nc) || ys[i] != floor(ys[i]))
      return fail(ctx, VB_ERR_INVALID, "softmax labels must be integers in [0, n_classes) (y[%lld] = %g)", (long long)i, ys[i]);
  ModelDev m;
  m.id = VB_MODEL_SOFTMAX;
  m.dim = (int)dim;
  m.n_data = nd;
  m.n_classes = (int)nc;
  m.n_feat = (int)p;
  m.ldp = round_up(p, 16);
  m.ldq = round_up(nd, 16);
  m.tau = sd;
  m.c0 = 0.0;      // (the rows carry prior and constant themselves, like a source model's: see ModelDev::f0)
  m.f0 = -(double)dim * (log(sd) + 0.5 * kLog2Pi);
  // [X (nd x ldp) | X' (p x ldq) | y (ldq)]: the logistic target's layout with p in place of dim
  const size_t o_xt = (size_t)nd * m.ldp, o_y = o_xt + (size_t)p * m.ldq;
  std::vector<double> dev(o_y + (size_t)m.ldq, 0.0);
  pack_design(dev, 0, dparams, nd, p, m.ldp, m.ldq);
  for (int64_t i = 0; i < nd; ++i) dev[o_y + i] = ys[i];
  VB_TRY(upload_model_params(ctx, dev, &m.p0));
  m.p1 = m.p0 + o_xt;
  m.p2 = m.p0 + o_y;
  ctx->model = m;
  return VB_OK;
}

}  // namespace vb

using namespace vb;

extern "C" {

int vb_softmax_pointwise(vb_ctx* ctx, const double* x, int64_t s, int64_t d, double* ll_out) {
  SmLayout L;
  return rows_pointwise(
      ctx, "vb_softmax_pointwise", VB_MODEL_SOFTMAX, "softmax regression", x, s, d, ll_out,
      [&](RowsPointwisePlan* plan) {
        VB_TRY(sm_check(ctx, s, (int)d));
        L = sm_layout(ctx->model, s, false, true);
        *plan = {L.chunk, L.total, L.o_x, L.o_ll, L.ldh};
        return VB_OK;
      },
      [&](int64_t rows, const double* X, int64_t ldx, double* LL, int64_t ldl) {
        const ModelDev& m = ctx->model;
        double* base = (double*)ctx->target_work.ptr;
        VB_TRY(sm_predictors(ctx, ctx->stream, L, base, X, ldx, rows));
        hipLaunchKernelGGL(sm_couple_kernel<2>, dim3((unsigned)(rows * L.n_strips)), dim3(256), 0, ctx->stream, base + L.o_h,
                           L.ldh, m.n_classes, (int)m.n_data, m.p2, L.n_strips, (double*)nullptr, LL, ldl);
        VB_HIP(ctx, hipGetLastError());
        return VB_OK;
      });
}

}  // extern "C"
