// Data-subsampled GLM target, VB_MODEL_MINIBATCH_GLM: the flat regression targets' density (Bernoulli-logit, Poisson or
// Gaussian observations, N(0, sd) prior, dim = p) on a random batch of B of the n_data observations, the likelihood scaled
// by n_data / B (doubly stochastic variational inference).  Batch number t:
//
//   f_t(theta) = (n_data / B) sum_{j in batch t} l(y_j, x_j' theta) - |theta|^2 / (2 sd^2) + f0
//   df_t/dtheta = (n_data / B) sum_{j in batch t} dl_j x_j - theta / sd^2
//
// f0 holds the prior's constant and the likelihood's constant of ALL n_data observations, so with B = n_data this is the
// dense target's density.  The device holds X once (row-major, n_data x ldp) and y; no X'.
//
// The batch is a pure function of (seed, t).  Batch t owns positions q = t B .. t B + B - 1 of an endless stream; position q
// is slot q mod n_data of epoch q div n_data, and the slot's observation is the slot itself (order 0) or perm_epoch(slot)
// (order 1).  perm_epoch is a balanced Feistel network on 2 w bits, w = max(1, ceil(ceil(log2 n_data) / 2)), cycle-walked
// into [0, n_data):
//   x = slot;  repeat { (L, R) = (x >> w, x & (2^w - 1));  for r = 0 .. 5: (L, R) = (R, L ^ F(r, R));  x = L 2^w + R }
//   until x < n_data
//   F(r, h) = word 0 of philox4x32_10(counter (h, r, epoch mod 2^32, epoch div 2^32), key (seed mod 2^32, seed div 2^32))
//             & (2^w - 1)
// A Feistel network is a bijection of [0, 2^(2 w)) whatever F is, and walking a bijection's cycle from a point below n_data
// comes back below n_data: every epoch visits every observation exactly once.  2^(2 w) <= 4 n_data.
//
// Per evaluation, on the caller's stream (t = ctx->mb_batch, passed by value):
//   index     idx[i] = observation of position t B + i                          one thread per batch slot
//   gather    Xb[i][:] = X[idx[i]][:]  [ldb x ldp], Xb'[j][i]  [p x ldb], yb[i] = y[idx[i]]; ldb = round_up(B, 16); pad rows
//             and pad columns are written as zeros.  A workgroup moves a 64 x 64 tile: rows of X are read as contiguous
//             runs, the transposed tile goes through LDS (65-double rows: conflict-free), both outputs leave coalesced
//   (both skipped when the front of ctx->target_work already holds batch t of this binding: vb_ctx::mb_held)
// and per chunk of samples (rows of Z):
//   GEMM      eta = Z Xb'  [rows x B x p], fp64 MFMA; the epilogue stores the term T and, with a gradient, R = (n_data / B) dl
//   GEMM      G = R Xb - Z / sd^2                glm_grad_enqueue over a view of the batch (its observation split applies to B)
//   rowsum    f[r] = (n_data / B) sum_i T[r][i] - |z_r|^2 / (2 sd^2) + f0: a workgroup per row, a lane adds its elements in
//             index order, the wave by shuffles, the sixteen waves in wave order
// No atomics, every sum in a fixed order: two calls give the same bits.
#include "vb_rows_target.h"
#include "vb_rng.h"

namespace vb {

namespace {

constexpr int kMbRounds = 6;      // Feistel rounds of the epoch permutation

__device__ __forceinline__ int64_t mb_permute(int64_t slot, uint64_t epoch, int64_t n, int w, uint32_t k0, uint32_t k1) {
  const uint32_t mask = (1u << w) - 1u;      // (w <= 16)
  uint64_t x = (uint64_t)slot;
  do {
    uint32_t L = (uint32_t)(x >> w), R = (uint32_t)x & mask;
#pragma unroll 1
    for (uint32_t r = 0; r < (uint32_t)kMbRounds; ++r) {
      Philox4 c;
      c.x = R, c.y = r, c.z = (uint32_t)epoch, c.w = (uint32_t)(epoch >> 32);
      const uint32_t nr = L ^ (philox4x32_10(c, k0, k1).x & mask);
      L = R;
      R = nr;
    }
    x = ((uint64_t)L << w) | R;
  } while (x >= (uint64_t)n);
  return (int64_t)x;
}

// idx[i] = the observation of stream position first + i, i < B
__global__ void __launch_bounds__(256) mb_index_kernel(int* __restrict__ idx, int64_t B, int64_t n, uint64_t first, int shuffle,
                                                       int w, uint32_t k0, uint32_t k1) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= B) return;
  const uint64_t q = first + (uint64_t)i;
  const int64_t slot = (int64_t)(q % (uint64_t)n);
  idx[i] = (int)(shuffle ? mb_permute(slot, q / (uint64_t)n, n, w, k0, k1) : slot);
}

// the 64 x 64 tile (batch rows 64 blockIdx.x .., columns 64 blockIdx.y ..): Xb[b][j] = X[idx[b]][j] for b < B, j < p and 0
// for the other b < ldb, j < ldp; Xbt[j][b] the same for j < p, b < ldb; column block 0 also writes yb[b] (0 for B <= b < ldb)
__global__ void __launch_bounds__(256) mb_gather_kernel(const double* __restrict__ X, int64_t ldx, const double* __restrict__ y,
                                                        const int* __restrict__ idx, int64_t B, int p, double* __restrict__ Xb,
                                                        int64_t ldp, double* __restrict__ Xbt, int64_t ldb,
                                                        double* __restrict__ yb) {
  __shared__ double tile[64][65];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t b0 = (int64_t)blockIdx.x * 64, j0 = (int64_t)blockIdx.y * 64;
#pragma unroll 4
  for (int it = 0; it < 16; ++it) {
    const int r = it * 4 + wave;
    const int64_t b = b0 + r, j = j0 + lane;
    const double v = (b < B && j < p) ? X[(int64_t)idx[b] * ldx + j] : 0.0;
    tile[r][lane] = v;
    if (b < ldb && j < ldp) Xb[b * ldp + j] = v;
  }
  if (blockIdx.y == 0 && threadIdx.x < 64) {
    const int64_t b = b0 + threadIdx.x;
    if (b < ldb) yb[b] = b < B ? y[idx[b]] : 0.0;
  }
  __syncthreads();
#pragma unroll 4
  for (int it = 0; it < 16; ++it) {
    const int jj = it * 4 + wave;
    const int64_t j = j0 + jj, b = b0 + lane;
    if (j < p && b < ldb) Xbt[j * ldb + b] = tile[lane][jj];
  }
}

struct EpiMbTerm {           // T = log-likelihood term of batch slot `col` at eta = acc
  double* T;
  int64_t ldt;
  const double* y;
  int link;
  double aux;
  __device__ void operator()(int, int row, int col, double eta) const {
    double dl;
    T[(int64_t)row * ldt + col] = glm_term(link, aux, y[col], eta, &dl);
  }
};

struct EpiMbTermResidual {   // ... and R = scale times its derivative in eta
  double* T;
  double* R;
  int64_t ldt;
  const double* y;
  int link;
  double aux, scale;
  __device__ void operator()(int, int row, int col, double eta) const {
    double dl;
    T[(int64_t)row * ldt + col] = glm_term(link, aux, y[col], eta, &dl);
    R[(int64_t)row * ldt + col] = scale * dl;
  }
};

struct EpiMbPointwise {      // LL = the normalised, unscaled log-likelihood of batch slot `col`
  double* LL;
  int64_t ldl;
  const double* y;
  int link;
  double aux;
  __device__ void operator()(int, int row, int col, double eta) const {
    double dl;
    const double yi = y[col];
    LL[(int64_t)row * ldl + col] = glm_term(link, aux, yi, eta, &dl) + glm_obs_const(link, aux, yi);
  }
};

// f[r] = scale sum_i T[r][i] + neg_half_ivp |z_r|^2 + f0: a workgroup of sixteen waves per row
__global__ void __launch_bounds__(1024) mb_rowsum_kernel(const double* __restrict__ T, int64_t ldt, int64_t B,
                                                         const double* __restrict__ Z, int64_t ldz, int p, double scale,
                                                         double neg_half_ivp, double f0, double* __restrict__ f) {
  __shared__ double wll[16], wzz[16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r = blockIdx.x;
  const double* __restrict__ Tr = T + r * ldt;
  const double* __restrict__ zr = Z + r * ldz;
  double ll = 0.0, zz = 0.0;
  for (int64_t i = threadIdx.x; i < B; i += 1024) ll += Tr[i];
  for (int c = threadIdx.x; c < p; c += 1024) zz = fma(zr[c], zr[c], zz);
  ll = wave_sum(ll);
  zz = wave_sum(zz);
  if (lane == 0) wll[wave] = ll, wzz[wave] = zz;
  __syncthreads();
  if (threadIdx.x != 0) return;
  double a = wll[0], b = wzz[0];
#pragma unroll
  for (int w = 1; w < 16; ++w) a += wll[w], b += wzz[w];
  f[r] = fma(scale, a, fma(neg_half_ivp, b, f0));
}

// The front of the workspace is the batch (the same for every call of a binding), the chunk's matrices follow.
struct MbLayout {
  int64_t B, ldb, ldp, chunk, o_idx, o_xb, o_xbt, o_yb, o_t, o_r, o_x, total;
};

// rows per chunk: minibatch_chunk_rows (vb_common.h); `pointwise`: room for the uploaded draws as well (the term matrix is T)
MbLayout mb_layout(const ModelDev& m, int64_t n, bool grad, bool pointwise) {
  MbLayout L;
  L.B = m.mb_size;
  L.ldb = round_up(L.B, 16);
  L.ldp = m.ldp;
  const int64_t chunk = minibatch_chunk_rows(L.B);
  L.chunk = chunk > n ? n : chunk;
  Carver carve;
  L.o_idx = carve(L.ldb / 2);
  L.o_xb = carve(L.ldb * L.ldp);
  L.o_xbt = carve((int64_t)m.dim * L.ldb);
  L.o_yb = carve(L.ldb);
  L.o_t = carve(L.chunk * L.ldb);
  L.o_r = carve(grad ? L.chunk * L.ldb : 0);
  L.o_x = carve(pointwise ? L.chunk * round_up(m.dim, 16) : 0);
  L.total = carve.off;
  return L;
}

int mb_check(vb_ctx* ctx, int64_t n, int64_t d) {
  const ModelDev& m = ctx->model;
  if (n <= 0 || d != m.dim)
    return fail(ctx, VB_ERR_INVALID, "minibatch regression rows: %lld x %lld samples for a model of dimension %d", (long long)n,
                (long long)d, m.dim);
  if (n > 0x7fffffffll) return fail(ctx, VB_ERR_INVALID, "minibatch regression rows: at most 2^31 - 1 samples per call");
  return VB_OK;
}

int mb_index_launch(vb_ctx* ctx, hipStream_t st, const ModelDev& m, int64_t t, int* idx) {
  hipLaunchKernelGGL(mb_index_kernel, dim3((unsigned)((m.mb_size + 255) / 256)), dim3(256), 0, st, idx, m.mb_size, m.n_data,
                     (uint64_t)t * (uint64_t)m.mb_size, m.mb_shuffle, m.mb_half_bits, (uint32_t)m.mb_seed,
                     (uint32_t)(m.mb_seed >> 32));
  VB_HIP(ctx, hipGetLastError());
  return VB_OK;
}

// the front of the workspace holds batch ctx->mb_batch on `st` when this returns: the index and the gather kernel, unless
// it does already (same allocation, same batch, nothing bound in between; gathered on the main stream and wanted there)
int mb_batch_ready(vb_ctx* ctx, hipStream_t st, const MbLayout& L) {
  const ModelDev& m = ctx->model;
  double* base = (double*)ctx->target_work.ptr;
  const bool main_stream = st == (hipStream_t)ctx->stream;
  if (main_stream && ctx->mb_held == ctx->mb_batch && ctx->mb_held_at == (const void*)base &&
      ctx->mb_held_bytes == ctx->target_work.bytes)
    return VB_OK;
  ctx->mb_held = -1;
  int* idx = reinterpret_cast<int*>(base + L.o_idx);
  VB_TRY(mb_index_launch(ctx, st, m, ctx->mb_batch, idx));
  const dim3 grid((unsigned)((L.ldb + 63) / 64), (unsigned)((L.ldp + 63) / 64));
  hipLaunchKernelGGL(mb_gather_kernel, grid, dim3(256), 0, st, m.p0, m.ldp, m.p2, (const int*)idx, L.B, m.dim, base + L.o_xb,
                     L.ldp, base + L.o_xbt, L.ldb, base + L.o_yb);
  VB_HIP(ctx, hipGetLastError());
  if (main_stream) ctx->mb_held = ctx->mb_batch, ctx->mb_held_at = base, ctx->mb_held_bytes = ctx->target_work.bytes;
  return VB_OK;
}

}  // namespace

int minibatch_rows_enqueue(vb_ctx* ctx, hipStream_t st, const double* Z, int64_t ldz, int64_t n, int d, double* G, int64_t ldg,
                           double* f) {
  const ModelDev& m = ctx->model;
  if (m.id != VB_MODEL_MINIBATCH_GLM) return fail(ctx, VB_ERR_STATE, "no minibatch regression model bound");
  VB_TRY(mb_check(ctx, n, d));
  VB_TRY(rows_operands_check(ctx, "minibatch regression", Z, ldz, d, G, ldg));
  const MbLayout L = mb_layout(m, n, G != nullptr, false);
  VB_TRY(ensure(ctx, ctx->target_work, (size_t)L.total * sizeof(double)));
  double* base = (double*)ctx->target_work.ptr;
  VB_TRY(mb_batch_ready(ctx, st, L));
  const int n_cu = ctx->prop.multiProcessorCount;
  const double ivp = 1.0 / (m.tau * m.tau), scale = (double)m.n_data / (double)L.B;
  const double* yb = base + L.o_yb;
  double *T = base + L.o_t, *R = base + L.o_r;
  ModelDev batch = m;            // what glm_grad_enqueue reads of a model: the design, its stride, the observations, the prior
  batch.p0 = base + L.o_xb;
  batch.n_data = L.B;
  for (int64_t r0 = 0; r0 < n; r0 += L.chunk) {
    const int64_t rows = n - r0 < L.chunk ? n - r0 : L.chunk;
    const double* Zc = Z + r0 * ldz;
    const GemmArgs g = gemm_product(Zc, ldz, base + L.o_xbt, L.ldb, (int)rows, (int)L.B, d, 0);
    if (G) gemm_f64_launch<true>(st, g, 1, n_cu, EpiMbTermResidual{T, R, L.ldb, yb, m.link, m.aux, scale});
    else gemm_f64_launch<true>(st, g, 1, n_cu, EpiMbTerm{T, L.ldb, yb, m.link, m.aux});
    VB_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(mb_rowsum_kernel, dim3((unsigned)rows), dim3(1024), 0, st, (const double*)T, L.ldb, L.B, Zc, ldz, d,
                       scale, -0.5 * ivp, m.f0, f + r0);
    VB_HIP(ctx, hipGetLastError());
    if (G) VB_TRY(glm_grad_enqueue(ctx, st, batch, R, L.ldb, Zc, G + r0 * ldg, ldz, rows, d));
  }
  return VB_OK;
}

int minibatch_set_model(vb_ctx* ctx, int64_t dim, const double* dparams, size_t n_dparams, const int64_t* iparams,
                        size_t n_iparams) {
  const char* kExpect =
      "minibatch regression expects dparams = [X(n_data x p) | y(n_data) | prior_sd | noise_sd], iparams = [n_data, "
      "batch_size, link, order (0 sequential, 1 shuffle), seed] and a dimension of p, with 1 <= batch_size <= n_data < 2^31";
  if (n_iparams != 5 || !iparams || !dparams || iparams[0] <= 0 || iparams[0] > 0x7fffffffll || iparams[1] < 1 ||
      iparams[1] > iparams[0] || dim > 0x7fffffffll || iparams[2] < VB_GLM_BERNOULLI_LOGIT || iparams[2] > VB_GLM_GAUSSIAN ||
      (iparams[3] != 0 && iparams[3] != 1) || n_dparams != (size_t)(iparams[0] * dim + iparams[0] + 2))
    return fail(ctx, VB_ERR_INVALID, "%s", kExpect);
  const int64_t nd = iparams[0], p = dim;
  const int link = (int)iparams[2];
  const double* ys = dparams + nd * p;
  const double sd = ys[nd], nsd = ys[nd + 1];
  if (!(sd > 0.0)) return fail(ctx, VB_ERR_INVALID, "minibatch regression prior_sd must be positive");
  if (!(nsd > 0.0)) return fail(ctx, VB_ERR_INVALID, "minibatch regression noise_sd must be positive");
  for (int64_t i = 0; i < nd; ++i) {
    const double yi = ys[i];
    if (!std::isfinite(yi)) return fail(ctx, VB_ERR_INVALID, "minibatch regression: y must be finite (y[%lld])", (long long)i);
    if (link == VB_GLM_BERNOULLI_LOGIT && yi != 0.0 && yi != 1.0)
      return fail(ctx, VB_ERR_INVALID, "minibatch regression: logistic responses must lie in {0, 1} (y[%lld] = %g)",
                  (long long)i, yi);
    if (link == VB_GLM_POISSON && !(yi >= 0.0))
      return fail(ctx, VB_ERR_INVALID, "minibatch regression: Poisson counts must be non-negative (y[%lld] = %g)",
                  (long long)i, yi);
  }
  ModelDev m;
  m.id = VB_MODEL_MINIBATCH_GLM;
  m.dim = (int)dim;
  m.n_data = nd;
  m.mb_size = iparams[1];
  m.mb_shuffle = (int)iparams[3];
  m.mb_seed = (uint64_t)iparams[4];
  int bits = 0;                          // ceil(log2 n_data)
  while (((int64_t)1 << bits) < nd) ++bits;
  m.mb_half_bits = bits < 2 ? 1 : (bits + 1) / 2;
  m.ldp = round_up(p, 16);
  m.tau = sd;
  m.link = link;
  m.aux = link == VB_GLM_GAUSSIAN ? nsd : 1.0;
  m.c0 = 0.0;      // (the rows carry prior and constants themselves: see ModelDev::f0)
  m.f0 = glm_const_continue(-(double)p * (log(sd) + 0.5 * kLog2Pi), link, nsd, ys, nd);
  // [X (n_data x ldp) | y (round_up(n_data, 16))], the pad columns zero
  const size_t o_y = (size_t)nd * m.ldp;
  std::vector<double> dev(o_y + (size_t)round_up(nd, 16), 0.0);
  for (int64_t i = 0; i < nd; ++i) {
    memcpy(dev.data() + (size_t)i * m.ldp, dparams + i * p, (size_t)p * sizeof(double));
    dev[o_y + i] = ys[i];
  }
  VB_TRY(upload_model_params(ctx, dev, &m.p0));
  m.p2 = m.p0 + o_y;
  ctx->model = m;
  ctx->mb_batch = 0;
  ctx->mb_held = -1;
  return VB_OK;
}

}  // namespace vb

using namespace vb;

extern "C" {

int vb_minibatch_set_batch(vb_ctx* ctx, int64_t t) {
  if (!ctx) return VB_ERR_INVALID;
  if (ctx->model.id != VB_MODEL_MINIBATCH_GLM) return fail(ctx, VB_ERR_STATE, "no minibatch regression model bound");
  if (t < 0 || t >= ((int64_t)1 << 62) / ctx->model.mb_size - 1)
    return fail(ctx, VB_ERR_INVALID, "the batch number must lie in [0, 2^62 / batch_size - 1) (got %lld)", (long long)t);
  ctx->mb_batch = t;
  return VB_OK;
}

int vb_minibatch_get_batch(vb_ctx* ctx, int64_t* t) {
  if (!ctx || !t) return fail(ctx, VB_ERR_INVALID, "NULL argument");
  if (ctx->model.id != VB_MODEL_MINIBATCH_GLM) return fail(ctx, VB_ERR_STATE, "no minibatch regression model bound");
  *t = ctx->mb_batch;
  return VB_OK;
}

// (the indices land where an evaluation's would: the workspace then holds no complete batch, and says so)
int vb_minibatch_indices(vb_ctx* ctx, int64_t t, int64_t* out) {
  if (!ctx || !out) return fail(ctx, VB_ERR_INVALID, "NULL argument");
  const ModelDev& m = ctx->model;
  if (m.id != VB_MODEL_MINIBATCH_GLM) return fail(ctx, VB_ERR_STATE, "no minibatch regression model bound");
  if (t < 0 || t >= ((int64_t)1 << 62) / m.mb_size - 1)
    return fail(ctx, VB_ERR_INVALID, "the batch number must lie in [0, 2^62 / batch_size - 1) (got %lld)", (long long)t);
  VB_HIP(ctx, hipSetDevice(ctx->device));
  const MbLayout L = mb_layout(m, 1, false, false);
  VB_TRY(ensure(ctx, ctx->target_work, (size_t)L.total * sizeof(double)));
  ctx->mb_held = -1;
  int* idx = reinterpret_cast<int*>((double*)ctx->target_work.ptr + L.o_idx);
  VB_TRY(mb_index_launch(ctx, ctx->stream, m, t, idx));
  std::vector<int> host((size_t)m.mb_size);
  VB_HIP(ctx, hipMemcpyAsync(host.data(), idx, host.size() * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  VB_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int64_t i = 0; i < m.mb_size; ++i) out[i] = host[(size_t)i];
  return VB_OK;
}

// (the term matrix is T of the layout, row stride ldb; B columns of it are downloaded)
int vb_minibatch_pointwise(vb_ctx* ctx, const double* x, int64_t s, int64_t d, double* ll_out) {
  MbLayout L;
  return rows_pointwise(
      ctx, "vb_minibatch_pointwise", VB_MODEL_MINIBATCH_GLM, "minibatch regression", x, s, d, ll_out,
      [&](RowsPointwisePlan* plan) {
        L = mb_layout(ctx->model, s, false, true);
        *plan = {L.chunk, L.total, L.o_x, L.o_t, L.ldb, L.B};
        return mb_check(ctx, s, d);
      },
      [&](int64_t rows, const double* X, int64_t ldx, double* LL, int64_t ldl) {
        const ModelDev& m = ctx->model;
        double* base = (double*)ctx->target_work.ptr;
        VB_TRY(mb_batch_ready(ctx, ctx->stream, L));
        const GemmArgs g = gemm_product(X, ldx, base + L.o_xbt, L.ldb, (int)rows, (int)L.B, m.dim, 0);
        gemm_f64_launch<true>(ctx->stream, g, 1, ctx->prop.multiProcessorCount,
                              EpiMbPointwise{LL, ldl, base + L.o_yb, m.link, m.aux});
        VB_HIP(ctx, hipGetLastError());
        return VB_OK;
      });
}

}  // extern "C"
