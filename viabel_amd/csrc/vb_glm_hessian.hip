// Value, gradient and Hessian of the flat regression target (VB_MODEL_LOGISTIC, any VB_GLM_* likelihood) at ONE point b:
//   f(b) = sum_i [l_i(eta_i) + const_i] - |b|^2 / (2 tau^2) - D (log tau + log(2 pi) / 2),    eta = X b
//   g(b) = X' r - b / tau^2,                       r_i = dl_i / d eta
//   H(b) = -X' diag(w) X - I / tau^2,              w_i = -d^2 l_i / d eta^2
// (Bernoulli-logit w = t / (1 + t)^2 with t = exp(-|eta|) -- glm_predict_term's variance, no 1 - mu --, Poisson w = exp(eta),
// Gaussian w = 1 / aux^2.)  What a Newton step and the Laplace approximation need (vb_glm_value_grad_hessian).
//
// Launch sequence, all on ctx->stream:
//   glmh_link_kernel    ONE streaming pass over the bound X (m.p0, row stride ldp): a 256-thread workgroup walks 32
//                       consecutive observations, thread t holding the column pairs 2 (t + 256 q), q < KP, of the row in
//                       registers (16-byte loads, the next row's issued before this row's arithmetic).  Per row: eta by
//                       the fixed shuffle tree (wave_sum) and (w0 + w1) + (w2 + w3) over the four waves, the term with its
//                       per-observation constant, r and w (glm_predict_term: one exponential), then -- from the registers,
//                       the row is not read again -- r x_i added to the thread's own column sums and, when a Hessian is
//                       wanted, w x_i stored to WX (16-byte stores, pad columns zero).  Leaves colpart[block][column] (the
//                       32 rows in row order) and fpart[block].  X comes from HBM once per call, for value, gradient and
//                       scaled copy together.
//   gram_lower_enqueue  C = X' (WX), lower tiles, split over the observations by gram_splits (Hessian only)
//   glmh_finish_kernel  blocks [0, nb_c): H = -(sum of the split slabs in split order) - I / tau^2, entry (i, j <= i) written
//                       with its mirror image (j, i) by one thread: the matrix that leaves is exactly symmetric;
//                       the next ceil(D / 256) blocks: g_j = sum of colpart[.][j] in block order - b_j / tau^2;
//                       the last block: f = sum of fpart in a fixed order (thread t: entries t, t + 256, ...; shuffle tree;
//                       (w0 + w1) + (w2 + w3)) + prior.
// No floating-point atomics anywhere; every sum has a fixed order: two calls with the same input return the same bits, and
// f and g are the same bits with and without the Hessian (one link kernel, the store of WX its only switch).
//
// Workspace: vb_ctx::hess_work, laid out from scratch by every call -- [b (ldp) | colpart (n_rb x ldp) | fpart (n_rb) |
// g (ldp) | f | WX (n_data x ldp) | split slabs (splits x D x ldp) | H (D x ldp)], the last three with a Hessian only.  Every
// piece is written by this call before it is read (the finishing kernel reads the slabs' lower triangle only, which the product
// writes in every split).  WX is as large as the bound X and is NOT chunked over the observations: the device already holds X
// and X', so a third copy of that size fits wherever the model itself was a sensible thing to bind.
// Capacity: D <= 8192 (KP <= 16 column pairs per thread); VB_ERR_UNSUPPORTED beyond.
// One process's engine only: no all-reduce (like vb_glm_psis_loo).
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; scratch 0 in all; LDS 64 B (link) /
// 32 B (finish) per workgroup, so registers alone bound the occupancy):
//     glmh_link_kernel<1>  (D <=  512):  224 VGPRs -> 2 workgroups per CU
//     glmh_link_kernel<2>  (D <= 1024):  238 VGPRs -> 2 workgroups per CU
//     glmh_link_kernel<4>  (D <= 2048):  256 VGPRs + 14 AGPRs -> 1 workgroup per CU
//     glmh_link_kernel<8>  (D <= 4096):  256 VGPRs + 84 AGPRs -> 1 workgroup per CU
//     glmh_link_kernel<16> (D <= 8192):  256 VGPRs + 218 AGPRs -> 1 workgroup per CU
//     glmh_finish_kernel:                 70 VGPRs -> 7 workgroups per CU
//   (the compiler unrolls the 32-row loop and keeps several rows' loads in flight: that is where the link kernel's registers go.)
// Measured (tools/laplace_bench.py, profiles/laplace_kernel_stats.txt; logistic target, one MI355X): n_data = 65 536, D = 1024 --
// link pass 305 us (1.07 GB read + written: 3.5 TB/s), Gram product 1372 us in 7 splits (50 TFLOP/s of the n D (D + 1) executed
// flops), finishing kernel 141 us; n_data = 16 384, D = 512 -- 62 us (2.2 TB/s), 104 us (41 TFLOP/s), 30 us.
#include "vb_rows_target.h"

#include <climits>
#include <cmath>

namespace vb {

constexpr int kGlmhRows = 32;            // observations per workgroup of the link pass
constexpr int kGlmhMaxPairs = 16;        // column pairs a thread may hold
constexpr int64_t kGlmhMaxLd = (int64_t)512 * kGlmhMaxPairs;

struct GlmhLinkArgs {
  const double* X;         // n x ldp, pad columns zero
  const double* y;         // n
  const double* b;         // ldp, pad columns zero
  int64_t ldp, n;
  int d, link;
  double aux;
  double* WX;              // n x ldp, or nullptr: value and gradient only
  double* colpart;         // gridDim.x x ldp
  double* fpart;           // gridDim.x
};

template <int KP>
__global__ void __launch_bounds__(256) glmh_link_kernel(const GlmhLinkArgs a) {
  __shared__ double sh[2][4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * kGlmhRows;
  const int rows = a.n - r0 < kGlmhRows ? (int)(a.n - r0) : kGlmhRows;
  const d2v zero = (d2v){0.0, 0.0};
  d2v bv[KP], acc[KP], x[KP], xn[KP];
#pragma unroll
  for (int q = 0; q < KP; ++q) {
    const int col = 2 * (t + 256 * q);
    bv[q] = col < a.ldp ? *reinterpret_cast<const d2v*>(a.b + col) : zero;
    acc[q] = zero;
    xn[q] = col < a.ldp ? *reinterpret_cast<const d2v*>(a.X + r0 * a.ldp + col) : zero;
  }
  double fsum = 0.0;
  for (int k = 0; k < rows; ++k) {
    const int64_t row = r0 + k;
    const int64_t next = k + 1 < rows ? row + 1 : row;      // (clamped, not predicated: the last row is loaded twice)
#pragma unroll
    for (int q = 0; q < KP; ++q) {
      const int col = 2 * (t + 256 * q);
      x[q] = xn[q];
      xn[q] = col < a.ldp ? *reinterpret_cast<const d2v*>(a.X + next * a.ldp + col) : zero;
    }
    double e = 0.0;
#pragma unroll
    for (int q = 0; q < KP; ++q) e = fma(x[q].y, bv[q].y, fma(x[q].x, bv[q].x, e));
    e = wave_sum(e);
    if (lane == 0) sh[k & 1][wave] = e;
    __syncthreads();      // (one barrier per row: the slot of row k is next written for row k + 2, behind row k + 1's barrier)
    const double eta = (sh[k & 1][0] + sh[k & 1][1]) + (sh[k & 1][2] + sh[k & 1][3]);
    const double yi = a.y[row];
    double mu, var;
    const double term = glm_predict_term(a.link, a.aux, yi, eta, &mu, &var);
    const double iv = 1.0 / (a.aux * a.aux);
    const double r = a.link == VB_GLM_GAUSSIAN ? (yi - eta) * iv : yi - mu;
    const double w = a.link == VB_GLM_GAUSSIAN ? iv : var;
    fsum += term + glm_obs_const(a.link, a.aux, yi);
#pragma unroll
    for (int q = 0; q < KP; ++q) {
      const int col = 2 * (t + 256 * q);
      acc[q].x = fma(r, x[q].x, acc[q].x);
      acc[q].y = fma(r, x[q].y, acc[q].y);
      if (a.WX && col < a.ldp)      // pad columns: zero whatever w is (an overflowed Poisson weight times 0 is not)
        *reinterpret_cast<d2v*>(a.WX + row * a.ldp + col) = (d2v){col < a.d ? w * x[q].x : 0.0, col + 1 < a.d ? w * x[q].y : 0.0};
    }
  }
#pragma unroll
  for (int q = 0; q < KP; ++q) {
    const int col = 2 * (t + 256 * q);
    if (col < a.ldp) *reinterpret_cast<d2v*>(a.colpart + (int64_t)blockIdx.x * a.ldp + col) = acc[q];
  }
  if (t == 0) a.fpart[blockIdx.x] = fsum;
}

struct GlmhFinishArgs {
  const double* Cpart;     // splits slabs of d x ldh, lower triangle valid
  int splits;
  int64_t slab, ldh;
  int d;
  const double* colpart;   // n_rb x ldh
  const double* fpart;     // n_rb
  int n_rb;
  const double* b;         // ldh
  double ivp, prior_c0;    // 1 / tau^2; -D (log tau + log(2 pi) / 2)
  double* H;               // d x ldh, or nullptr (then nb_c == 0)
  double* g;               // ldh
  double* f;
  int nb_c, nb_g;
};

__global__ void __launch_bounds__(256) glmh_finish_kernel(const GlmhFinishArgs a) {
  __shared__ double sh[4];
  const int t = threadIdx.x;
  if ((int)blockIdx.x < a.nb_c) {
    // one thread per pair of adjacent entries (i, j), (i, j + 1) of the lower triangle, j even; eight slabs in flight
    const int64_t idx = 2 * ((int64_t)blockIdx.x * 256 + t);
    if (idx >= (int64_t)a.d * a.ldh) return;
    const int i = (int)(idx / a.ldh), j = (int)(idx % a.ldh);
    if (j > i) return;                       // (the upper triangle and the pad columns: written as mirror images / not at all)
    const bool two = j + 1 <= i;             // (i, j + 1) is below or on the diagonal too
    d2v s = (d2v){0.0, 0.0};
    for (int k0 = 0; k0 < a.splits; k0 += 8) {
      d2v v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {          // (clamped, not predicated; the surplus is not added)
        const double* p = a.Cpart + (int64_t)(k0 + u < a.splits ? k0 + u : a.splits - 1) * a.slab + idx;
        v[u] = two ? *reinterpret_cast<const d2v*>(p) : (d2v){*p, 0.0};
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (k0 + u < a.splits) s += v[u];
    }
    const double h0 = -s.x - (i == j ? a.ivp : 0.0);
    a.H[idx] = h0;
    if (j < i) a.H[(int64_t)j * a.ldh + i] = h0;
    if (two) {
      const double h1 = -s.y - (i == j + 1 ? a.ivp : 0.0);
      a.H[idx + 1] = h1;
      if (j + 1 < i) a.H[(int64_t)(j + 1) * a.ldh + i] = h1;
    }
    return;
  }
  if ((int)blockIdx.x < a.nb_c + a.nb_g) {
    const int j = ((int)blockIdx.x - a.nb_c) * 256 + t;
    if (j >= a.d) return;
    double s = 0.0;
    for (int rb0 = 0; rb0 < a.n_rb; rb0 += 16) {      // sixteen loads in flight, added in block order
      double v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = a.colpart[(int64_t)(rb0 + u < a.n_rb ? rb0 + u : a.n_rb - 1) * a.ldh + j];
#pragma unroll
      for (int u = 0; u < 16; ++u)
        if (rb0 + u < a.n_rb) s += v[u];
    }
    a.g[j] = fma(-a.ivp, a.b[j], s);
    return;
  }
  double fs = 0.0, ss = 0.0;
  for (int e = t; e < a.n_rb; e += 256) fs += a.fpart[e];
  for (int c = t; c < a.d; c += 256) ss = fma(a.b[c], a.b[c], ss);
  fs = wave_sum(fs);
  if ((t & 63) == 0) sh[t >> 6] = fs;
  __syncthreads();
  const double ftot = (sh[0] + sh[1]) + (sh[2] + sh[3]);
  __syncthreads();
  ss = wave_sum(ss);
  if ((t & 63) == 0) sh[t >> 6] = ss;
  __syncthreads();
  if (t == 0) a.f[0] = ftot + fma(-0.5 * a.ivp, (sh[0] + sh[1]) + (sh[2] + sh[3]), a.prior_c0);
}

static int glmh_link_enqueue(vb_ctx* ctx, hipStream_t st, const GlmhLinkArgs& a, int n_rb) {
  const dim3 grid((unsigned)n_rb), block(256);
  if (a.ldp <= 512) hipLaunchKernelGGL(glmh_link_kernel<1>, grid, block, 0, st, a);
  else if (a.ldp <= 1024) hipLaunchKernelGGL(glmh_link_kernel<2>, grid, block, 0, st, a);
  else if (a.ldp <= 2048) hipLaunchKernelGGL(glmh_link_kernel<4>, grid, block, 0, st, a);
  else if (a.ldp <= 4096) hipLaunchKernelGGL(glmh_link_kernel<8>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(glmh_link_kernel<16>, grid, block, 0, st, a);
  VB_HIP(ctx, hipGetLastError());
  return VB_OK;
}

}  // namespace vb

using namespace vb;

extern "C" {

int vb_glm_value_grad_hessian(vb_ctx* ctx, const double* x, int64_t d, double* f, double* grad, double* hess) {
  if (!ctx || !x || !f || !grad) return fail(ctx, VB_ERR_INVALID, "NULL argument");
  const ModelDev& m = ctx->model;
  if (m.id < 0) return fail(ctx, VB_ERR_STATE, "no model bound (vb_set_model)");
  if (m.id != VB_MODEL_LOGISTIC)
    return fail(ctx, VB_ERR_UNSUPPORTED, "the device Hessian exists for the flat regression targets only (model id %d)", m.id);
  if (d != m.dim) return fail(ctx, VB_ERR_INVALID, "x has %lld entries, model dimension is %d", (long long)d, m.dim);
  if (m.ldp > kGlmhMaxLd)
    return fail(ctx, VB_ERR_UNSUPPORTED, "the device Hessian takes at most %lld coefficients (the model has %d)",
                (long long)kGlmhMaxLd, m.dim);
  if (m.n_data > INT_MAX) return fail(ctx, VB_ERR_UNSUPPORTED, "the device Hessian takes at most %d observations", INT_MAX);
  VB_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int D = (int)d;
  const int64_t ld = m.ldp, n = m.n_data, slab = d * ld;
  const int n_rb = (int)((n + kGlmhRows - 1) / kGlmhRows);
  const int splits = hess ? gram_splits(ctx, D, n) : 0;
  Carver carve;
  const int64_t o_b = carve(ld), o_col = carve((int64_t)n_rb * ld), o_fp = carve(n_rb), o_g = carve(ld), o_f = carve(1),
                o_wx = carve(hess ? n * ld : 0), o_cpart = carve((int64_t)splits * slab), o_h = carve(hess ? slab : 0);
  VB_TRY(ensure(ctx, ctx->hess_work, (size_t)carve.off * sizeof(double)));
  double* base = (double*)ctx->hess_work.ptr;
  VB_HIP(ctx, hipMemsetAsync(base + o_b, 0, (size_t)ld * sizeof(double), st));
  VB_HIP(ctx, hipMemcpyAsync(base + o_b, x, (size_t)d * sizeof(double), hipMemcpyHostToDevice, st));
  const GlmhLinkArgs la{m.p0, m.p2, base + o_b, ld, n, D, m.link, m.aux, hess ? base + o_wx : nullptr, base + o_col, base + o_fp};
  VB_TRY(glmh_link_enqueue(ctx, st, la, n_rb));
  if (hess) VB_TRY(gram_lower_enqueue(ctx, m.p0, base + o_wx, ld, D, n, splits, base + o_cpart, ld, slab));
  GlmhFinishArgs fa;
  fa.Cpart = base + o_cpart, fa.splits = splits, fa.slab = slab, fa.ldh = ld, fa.d = D;
  fa.colpart = base + o_col, fa.fpart = base + o_fp, fa.n_rb = n_rb, fa.b = base + o_b;
  fa.ivp = 1.0 / (m.tau * m.tau), fa.prior_c0 = -(double)d * (log(m.tau) + 0.5 * kLog2Pi);
  fa.H = hess ? base + o_h : nullptr, fa.g = base + o_g, fa.f = base + o_f;
  fa.nb_c = hess ? (int)((slab / 2 + 255) / 256) : 0, fa.nb_g = (D + 255) / 256;
  hipLaunchKernelGGL(glmh_finish_kernel, dim3((unsigned)(fa.nb_c + fa.nb_g + 1)), dim3(256), 0, st, fa);
  VB_HIP(ctx, hipGetLastError());
  VB_HIP(ctx, hipMemcpyAsync(f, base + o_f, sizeof(double), hipMemcpyDeviceToHost, st));
  VB_HIP(ctx, hipMemcpyAsync(grad, base + o_g, (size_t)d * sizeof(double), hipMemcpyDeviceToHost, st));
  if (hess)
    VB_HIP(ctx, hipMemcpy2DAsync(hess, (size_t)d * sizeof(double), base + o_h, (size_t)ld * sizeof(double),
                                 (size_t)d * sizeof(double), (size_t)d, hipMemcpyDeviceToHost, st));
  VB_HIP(ctx, hipStreamSynchronize(st));
  return VB_OK;
}

}  // extern "C"
