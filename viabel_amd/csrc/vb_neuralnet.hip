// One-hidden-layer Bayesian neural network regression target, VB_MODEL_NEURALNET: the softmax target's shape -- several
// linear predictors per observation, coupled -- with a coupling whose coefficients differ from sample to sample.
//
//   theta = [w_0 | ... | w_{h-1} | a | v | c]   (unit-major, w_k of length p; a, v of length h; c scalar), dim = h (p + 2) + 1
//   t_ik = tanh(x_i' w_k + a_k),   eta_i = c + sum_k v_k t_ik
//   f(theta) = sum_i log p(y_i | eta_i) - |theta|^2 / (2 sd^2) - dim (log sd + log(2 pi) / 2)        (any VB_GLM_* likelihood)
//   r_i = d log p(y_i | eta_i) / d eta,   delta_ik = r_i v_k (1 - t_ik^2)
//   d/dc = sum_i r_i - c / sd^2            d/dv_k = sum_i r_i t_ik - v_k / sd^2
//   d/da_k = sum_i delta_ik - a_k / sd^2   d/dw_k = sum_i delta_ik x_i - w_k / sd^2
//
// Per chunk of samples (rows of Z), with the units of a sample taken as h rows of a packed matrix:
//   pack      Zc[(r h + k)][j] = Z[r][k p + j]          (pad columns zero)
//   GEMM      H = Zc X'                                  [(rows h) x n_data x p], fp64 MFMA, plain store
//   forward   workgroup (r, strip), lanes over observations, the unit loop inside: t_ik over H, eta_i, the likelihood term
//             and r_i (to a row buffer); strip partials of the term and of r_i
//   backward  workgroup (r, k), lanes striding the observations: sums of r_i t_ik and of delta_ik, H overwritten by delta
//   GEMM      Gc = Delta X - Zc / sd^2                   glm_grad_enqueue on the packed shapes (split over n_data included)
//   unpack    G[r][k p + j] = Gc[(r h + k)][j]; the a and v entries from the backward sums, the c entry from the strips
// and f[r] = sum of the row's strip partials (fixed order) - |z_r|^2 / (2 sd^2) + f0.  The coefficients a_r, v_r, c_r are read
// from Z where they lie (uniform per workgroup).  No atomics anywhere: two calls give the same bits.
//
// Prediction (vb_nn_predict) wants ETA[observation][draw] for glm_predict_kernel, so its product runs the other way round:
// the draws' weights packed as Wt[j][k lds + s] = w_sk[j] (p x h lds), H = X_new Wt [chunk x (h lds) x p] -- one product per
// chunk of observations, against the bound X or the uploaded design --, and a forward kernel with lanes over the draws
// that writes ETA[i][s] = c_s + sum_k v_sk tanh(H[i][k lds + s] + a_sk): every access coalesced, no transpose.
#include "vb_rows_target.h"

namespace vb {

namespace {

constexpr int kNnStrip = 1024;      // observations per workgroup of the forward kernel: 256 lanes x 4

__global__ void __launch_bounds__(256) nn_pack_kernel(const double* __restrict__ Z, int64_t ldz, int64_t rows, int h, int p,
                                                      double* __restrict__ Zc, int64_t ldc) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * h * ldc) return;
  const int j = (int)(idx % ldc);
  const int64_t rk = idx / ldc;
  const int64_t r = rk / h;
  const int k = (int)(rk % h);
  Zc[idx] = j < p ? Z[r * ldz + (int64_t)k * p + j] : 0.0;      // (pad columns zero: the gradient epilogue reads pairs)
}

// MODE 0: log-likelihood partials; 1: ... and the partials of sum_i r_i, H overwritten by t_ik, r_i to R; 2: the normalised
// per-observation terms to LL, no sums.
// Workgroup (row r, strip s): lanes over consecutive observations, so each of the h unit rows is read (and written) as
// contiguous 2-KiB runs; a_rk and v_rk have one address for the whole workgroup.
template <int MODE>
__global__ void __launch_bounds__(256) nn_forward_kernel(double* __restrict__ H, int64_t ldh, const double* __restrict__ Z,
                                                         int64_t ldz, int h, int p, int n_data, const double* __restrict__ y,
                                                         int link, double aux, int n_strips, double* __restrict__ R,
                                                         double* __restrict__ part, double* __restrict__ LL, int64_t ldl) {
  const int64_t r = blockIdx.x / n_strips;
  const int s = blockIdx.x % n_strips;
  const double* __restrict__ ar = Z + r * ldz + (int64_t)h * p;
  const double* __restrict__ vr = ar + h;
  const double c = vr[h];
  double* __restrict__ Hr = H + r * h * ldh;
  double ll = 0.0, rs = 0.0;
#pragma unroll 1
  for (int u = 0; u < kNnStrip / 256; ++u) {
    const int i = s * kNnStrip + u * 256 + (int)threadIdx.x;
    if (i >= n_data) break;
    double eta = c;
    for (int k = 0; k < h; ++k) {
      const int64_t at = (int64_t)k * ldh + i;
      const double t = tanh(Hr[at] + ar[k]);      // (saturates to +-1 exactly: 1 - t^2 = 0 there)
      if (MODE == 1) Hr[at] = t;
      eta = fma(vr[k], t, eta);
    }
    const double yi = y[i];
    double dl;
    const double term = glm_term(link, aux, yi, eta, &dl);
    if (MODE == 2) LL[r * ldl + i] = term + glm_obs_const(link, aux, yi);
    else ll += term;
    if (MODE == 1) {
      R[r * ldh + i] = dl;
      rs += dl;
    }
  }
  if (MODE == 2) return;
  strip_partials_store<2>(ll, rs, part);
}

// Workgroup (r, k) = row r h + k of H: lanes stride the observations (coalesced), thread t takes i = t, t + 256, ... in
// order; part2[2 (r h + k)] = sum_i r_i t_ik, part2[2 (r h + k) + 1] = sum_i delta_ik, and the row becomes delta.
__global__ void __launch_bounds__(256) nn_backward_kernel(double* __restrict__ H, int64_t ldh, const double* __restrict__ R,
                                                          const double* __restrict__ Z, int64_t ldz, int h, int p, int n_data,
                                                          double* __restrict__ part2) {
  const int64_t r = blockIdx.x / h;
  const int k = blockIdx.x % h;
  const double v = Z[r * ldz + (int64_t)h * p + h + k];
  double* __restrict__ Hk = H + (int64_t)blockIdx.x * ldh;
  const double* __restrict__ Rr = R + r * ldh;
  double srt = 0.0, sdl = 0.0;
  for (int i = threadIdx.x; i < n_data; i += 256) {
    const double t = Hk[i], ri = Rr[i];
    const double dl = (ri * v) * fma(-t, t, 1.0);
    srt = fma(ri, t, srt);
    sdl += dl;
    Hk[i] = dl;
  }
  strip_partials_store<2>(srt, sdl, part2);
}

// G[r][k p + j] = Gc[(r h + k)][j]; G[r][h p + k] = sum_i delta_ik - a_k / sd^2; G[r][h p + h + k] = sum_i r_i t_ik -
// v_k / sd^2 (the c entry is the row-sum kernel's)
__global__ void __launch_bounds__(256) nn_unpack_kernel(const double* __restrict__ Gc, int64_t ldc, int64_t rows, int h, int p,
                                                        const double* __restrict__ part2, const double* __restrict__ Z,
                                                        int64_t ldz, double ivp, double* __restrict__ G, int64_t ldg) {
  const int64_t hp = (int64_t)h * p, w = hp + 2 * h;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * w) return;
  const int64_t r = idx / w;
  const int64_t col = idx % w;
  if (col < hp) {
    const int k = (int)(col / p), j = (int)(col % p);
    G[r * ldg + col] = Gc[(r * h + k) * ldc + j];
    return;
  }
  const int q = (int)(col - hp);
  const double sum = q < h ? part2[2 * (r * h + q) + 1] : part2[2 * (r * h + (q - h))];
  G[r * ldg + col] = fma(-ivp, Z[r * ldz + col], sum);
}

// f[r] = sum_s ll[r][s] - |z_r|^2 / (2 sd^2) + f0 and, with a gradient, G[r][d - 1] = sum_s rs[r][s] - c / sd^2: one wave per
// row, a lane adds its strips / columns in order
__global__ void __launch_bounds__(256) nn_rowsum_kernel(const double* __restrict__ part, int n_strips,
                                                        const double* __restrict__ Z, int64_t ldz, int d, double ivp,
                                                        double f0, int64_t rows, double* __restrict__ f, double* __restrict__ G,
                                                        int64_t ldg) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  double ll = 0.0, rs = 0.0, s2 = 0.0;
  for (int s = lane; s < n_strips; s += 64) {
    ll += part[2 * (r * n_strips + s)];
    rs += part[2 * (r * n_strips + s) + 1];
  }
  for (int c = lane; c < d; c += 64) s2 = fma(Z[r * ldz + c], Z[r * ldz + c], s2);
  ll = wave_sum(ll);
  rs = wave_sum(rs);
  s2 = wave_sum(s2);
  if (lane != 0) return;
  f[r] = fma(-0.5 * ivp, s2, ll) + f0;
  if (G) G[r * ldg + d - 1] = fma(-ivp, Z[r * ldz + d - 1], rs);
}

struct NnLayout {
  int64_t ldc, ldh, chunk, o_zc, o_h, o_r, o_gc, o_part, o_part2, o_x, o_ll, total;
  int n_strips;
};

// rows per chunk bound H to kNeuralNetChunkDoubles; `pointwise`: room for the uploaded draws and the term matrix as well
NnLayout nn_layout(const ModelDev& m, int64_t n, bool grad, bool pointwise) {
  NnLayout L;
  const int64_t h = m.n_hidden;
  L.ldc = round_up(m.n_feat, 16);
  L.ldh = m.ldq;
  L.n_strips = (int)((m.n_data + kNnStrip - 1) / kNnStrip);
  L.chunk = rows_chunk(kNeuralNetChunkDoubles, h * L.ldh, n);
  Carver carve;
  L.o_zc = carve(L.chunk * h * L.ldc);
  L.o_h = carve(L.chunk * h * L.ldh);
  L.o_r = carve(grad ? L.chunk * L.ldh : 0);
  L.o_gc = carve(grad ? L.chunk * h * L.ldc : 0);
  L.o_part = carve(2 * L.chunk * L.n_strips);
  L.o_part2 = carve(grad ? 2 * L.chunk * h : 0);
  L.o_x = carve(pointwise ? L.chunk * round_up(m.dim, 16) : 0);
  L.o_ll = carve(pointwise ? L.chunk * L.ldh : 0);
  L.total = carve.off;
  return L;
}

int nn_check(vb_ctx* ctx, int64_t n, int d) {
  const ModelDev& m = ctx->model;
  if (m.id != VB_MODEL_NEURALNET) return fail(ctx, VB_ERR_STATE, "no neural-network regression model bound");
  if (n <= 0 || d != m.dim)
    return fail(ctx, VB_ERR_INVALID, "neural-network rows: %lld x %d samples for a model of dimension %d", (long long)n, d, m.dim);
  if (n * m.n_hidden > 0x7fffffffll)
    return fail(ctx, VB_ERR_INVALID, "neural-network rows: %lld samples x %d hidden units do not fit the GEMM's int shapes",
                (long long)n, m.n_hidden);
  return VB_OK;
}

// pack -> H = Zc X' for `rows` samples starting at Z (the chunk's first row)
int nn_predictors(vb_ctx* ctx, hipStream_t st, const NnLayout& L, double* base, const double* Z, int64_t ldz, int64_t rows) {
  const ModelDev& m = ctx->model;
  const int h = m.n_hidden, p = m.n_feat;
  const int64_t items = rows * h * L.ldc;
  if ((items + 255) / 256 > 0x7fffffffll || rows * L.n_strips > 0x7fffffffll)
    return fail(ctx, VB_ERR_INVALID, "neural-network rows: packed chunk too large for one launch");
  hipLaunchKernelGGL(nn_pack_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, Z, ldz, rows, h, p, base + L.o_zc,
                     L.ldc);
  VB_HIP(ctx, hipGetLastError());
  const GemmArgs g = gemm_product(base + L.o_zc, L.ldc, m.p1, m.ldq, (int)(rows * h), (int)m.n_data, p, 0);
  gemm_f64_launch<true>(st, g, 1, ctx->prop.multiProcessorCount, EpiStorePlain{base + L.o_h, L.ldh});
  VB_HIP(ctx, hipGetLastError());
  return VB_OK;
}

// ---- prediction -----------------------------------------------------------------------------------------------------
// Wt[j][k lds + s] = X[s][k p + j] (p x h lds; the pad columns s >= n_draws zero) and T[q][s] = X[s][h p + q] for the
// 2 h + 1 coefficients a | v | c ((2 h + 1) x lds): the draws with the draw index fastest
__global__ void __launch_bounds__(256) nn_predict_pack_kernel(const double* __restrict__ X, int64_t ldx, int64_t n_draws, int h,
                                                              int p, int64_t lds, double* __restrict__ Wt,
                                                              double* __restrict__ T) {
  const int64_t n_w = (int64_t)p * h * lds, n_all = n_w + (int64_t)(2 * h + 1) * lds;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n_all) return;
  if (idx < n_w) {
    const int64_t s = idx % lds, jk = idx / lds;
    const int64_t k = jk % h, j = jk / h;
    Wt[idx] = s < n_draws ? X[s * ldx + k * p + j] : 0.0;
  } else {
    const int64_t s = (idx - n_w) % lds, q = (idx - n_w) / lds;
    T[idx - n_w] = s < n_draws ? X[s * ldx + (int64_t)h * p + q] : 0.0;
  }
}

// ETA[i][s] = c_s + sum_k v_sk tanh(H[i][k lds + s] + a_sk): workgroup (observation i, block of 256 draws), lanes over draws
__global__ void __launch_bounds__(256) nn_predict_forward_kernel(const double* __restrict__ H, int64_t ldh, int h, int64_t lds,
                                                                 int n_draws, const double* __restrict__ T, int n_sblocks,
                                                                 double* __restrict__ ETA) {
  const int64_t i = blockIdx.x / n_sblocks;
  const int s = (blockIdx.x % n_sblocks) * 256 + (int)threadIdx.x;
  if (s >= n_draws) return;
  const double* __restrict__ Hi = H + i * ldh;
  double eta = T[(int64_t)(2 * h) * lds + s];
  for (int k = 0; k < h; ++k)
    eta = fma(T[(int64_t)(h + k) * lds + s], tanh(Hi[(int64_t)k * lds + s] + T[(int64_t)k * lds + s]), eta);
  ETA[i * lds + s] = eta;
}

// Where the pieces of a prediction live in ctx->loo_work (doubles from the base); a chunk of observations keeps
// h * chunk * round_up(s, 16) doubles of H within kNeuralNetPredictDoubles
struct NnPredictLayout {
  int64_t lds, ldx, ldn, mp;      // row strides: draws-as-columns, draws-as-rows, design rows; round_up(m, 16)
  int64_t o_x, o_wt, o_t, o_w, o_xn, o_y, o_res, o_h, o_eta, total;
  int64_t chunk;
};
NnPredictLayout nn_predict_layout(const ModelDev& md, int64_t s, int64_t m, bool own_design) {
  NnPredictLayout L;
  const int64_t h = md.n_hidden, p = md.n_feat;
  L.lds = round_up(s, 16), L.ldx = round_up(md.dim, 16), L.ldn = round_up(p, 16), L.mp = round_up(m, 16);
  int64_t chunk = kNeuralNetPredictDoubles / (h * L.lds);
  L.chunk = chunk < 1 ? 1 : (chunk > m ? m : chunk);
  Carver carve;
  L.o_x = carve(s * L.ldx);
  L.o_wt = carve(p * h * L.lds);
  L.o_t = carve((2 * h + 1) * L.lds);
  L.o_w = carve(2 * L.lds);
  L.o_xn = carve(own_design ? L.chunk * L.ldn : 0);
  L.o_y = carve(L.mp);
  L.o_res = carve(5 * L.mp);
  L.o_h = carve(L.chunk * h * L.lds);
  L.o_eta = carve(L.chunk * L.lds);
  L.total = carve.off;
  return L;
}

}  // namespace

int neuralnet_rows_enqueue(vb_ctx* ctx, hipStream_t st, const double* Z, int64_t ldz, int64_t n, int d, double* G, int64_t ldg,
                           double* f) {
  VB_TRY(nn_check(ctx, n, d));
  VB_TRY(rows_operands_check(ctx, "neural-network", Z, ldz, d, G, ldg));
  const ModelDev& m = ctx->model;
  const int h = m.n_hidden, p = m.n_feat;
  const NnLayout L = nn_layout(m, n, G != nullptr, false);
  VB_TRY(ensure(ctx, ctx->target_work, (size_t)L.total * sizeof(double)));
  double* base = (double*)ctx->target_work.ptr;
  const double ivp = 1.0 / (m.tau * m.tau);
  for (int64_t r0 = 0; r0 < n; r0 += L.chunk) {
    const int64_t rows = n - r0 < L.chunk ? n - r0 : L.chunk;
    const double* Zr = Z + r0 * ldz;
    double* Gr = G ? G + r0 * ldg : nullptr;
    VB_TRY(nn_predictors(ctx, st, L, base, Zr, ldz, rows));
    const dim3 fgrid((unsigned)(rows * L.n_strips));
    if (G)
      hipLaunchKernelGGL(nn_forward_kernel<1>, fgrid, dim3(256), 0, st, base + L.o_h, L.ldh, Zr, ldz, h, p, (int)m.n_data, m.p2,
                         m.link, m.aux, L.n_strips, base + L.o_r, base + L.o_part, (double*)nullptr, (int64_t)0);
    else
      hipLaunchKernelGGL(nn_forward_kernel<0>, fgrid, dim3(256), 0, st, base + L.o_h, L.ldh, Zr, ldz, h, p, (int)m.n_data, m.p2,
                         m.link, m.aux, L.n_strips, (double*)nullptr, base + L.o_part, (double*)nullptr, (int64_t)0);
    VB_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(nn_rowsum_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, (const double*)(base + L.o_part),
                       L.n_strips, Zr, ldz, d, ivp, m.f0, rows, f + r0, Gr, ldg);
    VB_HIP(ctx, hipGetLastError());
    if (!G) continue;
    hipLaunchKernelGGL(nn_backward_kernel, dim3((unsigned)(rows * h)), dim3(256), 0, st, base + L.o_h, L.ldh,
                       (const double*)(base + L.o_r), Zr, ldz, h, p, (int)m.n_data, base + L.o_part2);
    VB_HIP(ctx, hipGetLastError());
    VB_TRY(glm_grad_enqueue(ctx, st, m, base + L.o_h, L.ldh, base + L.o_zc, base + L.o_gc, L.ldc, rows * h, p));
    const int64_t items = rows * ((int64_t)d - 1);
    hipLaunchKernelGGL(nn_unpack_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st,
                       (const double*)(base + L.o_gc), L.ldc, rows, h, p, (const double*)(base + L.o_part2), Zr, ldz, ivp, Gr,
                       ldg);
    VB_HIP(ctx, hipGetLastError());
  }
  return VB_OK;
}

int neuralnet_set_model(vb_ctx* ctx, int64_t dim, const double* dparams, size_t n_dparams, const int64_t* iparams,
                        size_t n_iparams) {
  const char* kExpect =
      "neural-network regression expects dparams = [X(n_data x p) | y(n_data) | prior_sd | noise_sd], iparams = [n_data, "
      "n_hidden, link] and a dimension of n_hidden * (p + 2) + 1";
  if (n_iparams != 3 || !iparams || !dparams || iparams[0] <= 0 || iparams[1] < 1 || iparams[0] > 0x7fffffffll ||
      iparams[1] > 0x7fffffffll || dim > 0x7fffffffll || (dim - 1) % iparams[1] != 0 || (dim - 1) / iparams[1] < 3 ||
      iparams[2] < VB_GLM_BERNOULLI_LOGIT || iparams[2] > VB_GLM_GAUSSIAN ||
      n_dparams != (size_t)(iparams[0] * ((dim - 1) / iparams[1] - 2) + iparams[0]) + 2)
    return fail(ctx, VB_ERR_INVALID, "%s", kExpect);
  const int64_t nd = iparams[0], nh = iparams[1], p = (dim - 1) / nh - 2;
  const int link = (int)iparams[2];
  const double* ys = dparams + nd * p;
  const double sd = ys[nd], nsd = ys[nd + 1];
  if (!(sd > 0.0)) return fail(ctx, VB_ERR_INVALID, "neural-network prior_sd must be positive");
  if (!(nsd > 0.0)) return fail(ctx, VB_ERR_INVALID, "neural-network noise_sd must be positive");
  if (link == VB_GLM_POISSON)
    for (int64_t i = 0; i < nd; ++i)
      if (!(ys[i] >= 0.0)) return fail(ctx, VB_ERR_INVALID, "Poisson counts must be non-negative");
  ModelDev m;
  m.id = VB_MODEL_NEURALNET;
  m.dim = (int)dim;
  m.n_data = nd;
  m.n_hidden = (int)nh;
  m.n_feat = (int)p;
  m.ldp = round_up(p, 16);
  m.ldq = round_up(nd, 16);
  m.tau = sd;
  m.link = link;
  m.aux = link == VB_GLM_GAUSSIAN ? nsd : 1.0;
  m.c0 = 0.0;      // (the rows carry prior and constants themselves: see ModelDev::f0)
  m.f0 = glm_const_continue(-(double)dim * (log(sd) + 0.5 * kLog2Pi), link, nsd, ys, nd);
  // [X (nd x ldp) | X' (p x ldq) | y (ldq)]: the softmax target's layout
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

int vb_nn_pointwise(vb_ctx* ctx, const double* x, int64_t s, int64_t d, double* ll_out) {
  NnLayout L;
  return rows_pointwise(
      ctx, "vb_nn_pointwise", VB_MODEL_NEURALNET, "neural-network regression", x, s, d, ll_out,
      [&](RowsPointwisePlan* plan) {
        VB_TRY(nn_check(ctx, s, (int)d));
        L = nn_layout(ctx->model, s, false, true);
        *plan = {L.chunk, L.total, L.o_x, L.o_ll, L.ldh};
        return VB_OK;
      },
      [&](int64_t rows, const double* X, int64_t ldx, double* LL, int64_t ldl) {
        const ModelDev& m = ctx->model;
        double* base = (double*)ctx->target_work.ptr;
        VB_TRY(nn_predictors(ctx, ctx->stream, L, base, X, ldx, rows));
        hipLaunchKernelGGL(nn_forward_kernel<2>, dim3((unsigned)(rows * L.n_strips)), dim3(256), 0, ctx->stream, base + L.o_h,
                           L.ldh, X, ldx, m.n_hidden, m.n_feat, (int)m.n_data, m.p2, m.link, m.aux, L.n_strips,
                           (double*)nullptr, (double*)nullptr, LL, ldl);
        VB_HIP(ctx, hipGetLastError());
        return VB_OK;
      });
}

int vb_nn_predict(vb_ctx* ctx, const double* x, int64_t s, int64_t d, const double* log_w, const double* x_new, int64_t m,
                  const double* y_new, double* mean, double* var, double* eta_mean, double* eta_var, double* lpd) {
  if (!ctx || !x || !mean || !var || !eta_mean || !eta_var) return fail(ctx, VB_ERR_INVALID, "NULL argument");
  if (ctx->model.id < 0) return fail(ctx, VB_ERR_STATE, "no model bound (vb_set_model)");
  if (ctx->model.id != VB_MODEL_NEURALNET)
    return fail(ctx, VB_ERR_UNSUPPORTED, "vb_nn_predict needs a neural-network regression target (model id %d bound)",
                ctx->model.id);
  const ModelDev& md = ctx->model;
  if (d != md.dim) return fail(ctx, VB_ERR_INVALID, "x has %lld columns, model dimension is %d", (long long)d, md.dim);
  if (s <= 0 || s > 0x7fffffffll) return fail(ctx, VB_ERR_INVALID, "the number of draws must be positive");
  if (m <= 0 || m > 0x7fffffffll) return fail(ctx, VB_ERR_INVALID, "the number of observations to predict must be positive");
  if (!x_new && m != md.n_data)
    return fail(ctx, VB_ERR_INVALID, "without x_new the bound design is predicted: m = %lld, the model has %lld observations",
                (long long)m, (long long)md.n_data);
  if (x_new ? (y_new == nullptr) != (lpd == nullptr) : (y_new && !lpd))
    return fail(ctx, VB_ERR_INVALID, "y_new and lpd go together (both or neither)");
  if (y_new && md.link == VB_GLM_POISSON)
    for (int64_t i = 0; i < m; ++i)
      if (!(y_new[i] >= 0.0)) return fail(ctx, VB_ERR_INVALID, "Poisson counts must be non-negative");
  const int h = md.n_hidden, p = md.n_feat;
  const NnPredictLayout L = nn_predict_layout(md, s, m, x_new != nullptr);
  const int64_t n_sblocks = (s + 255) / 256, pack_items = ((int64_t)p * h + 2 * h + 1) * L.lds;
  if ((int64_t)h * L.lds > 0x7fffffffll || (pack_items + 255) / 256 > 0x7fffffffll || L.chunk * n_sblocks > 0x7fffffffll)
    return fail(ctx, VB_ERR_INVALID, "vb_nn_predict: %lld draws x %d hidden units do not fit the GEMM's int shapes", (long long)s,
                h);
  std::vector<double> wv;
  if (!predict_weights(log_w, s, wv)) return fail(ctx, VB_ERR_INVALID, "no log weight is finite (or one is NaN or +inf)");
  VB_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  struct Drain {      // the host buffers of the asynchronous uploads outlive them on every way out
    hipStream_t st;
    ~Drain() { (void)hipStreamSynchronize(st); }
  } drain{st};
  VB_TRY(ensure(ctx, ctx->loo_work, (size_t)L.total * sizeof(double)));
  double* base = (double*)ctx->loo_work.ptr;
  VB_HIP(ctx, hipMemcpy2DAsync(base + L.o_x, (size_t)L.ldx * sizeof(double), x, (size_t)d * sizeof(double),
                               (size_t)d * sizeof(double), (size_t)s, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(nn_predict_pack_kernel, dim3((unsigned)((pack_items + 255) / 256)), dim3(256), 0, st,
                     (const double*)(base + L.o_x), L.ldx, s, h, p, L.lds, base + L.o_wt, base + L.o_t);
  VB_HIP(ctx, hipGetLastError());
  double *w_d = base + L.o_w, *lw_d = w_d + L.lds, *xn = base + L.o_xn, *res = base + L.o_res;
  VB_HIP(ctx, hipMemcpyAsync(w_d, wv.data(), (size_t)s * sizeof(double), hipMemcpyHostToDevice, st));
  VB_HIP(ctx, hipMemcpyAsync(lw_d, wv.data() + s, (size_t)s * sizeof(double), hipMemcpyHostToDevice, st));
  const double* y_d = x_new ? nullptr : md.p2;
  if (y_new) {
    VB_HIP(ctx, hipMemcpyAsync(base + L.o_y, y_new, (size_t)m * sizeof(double), hipMemcpyHostToDevice, st));
    y_d = base + L.o_y;
  }
  const int64_t ldh = (int64_t)h * L.lds;
  for (int64_t r0 = 0; r0 < m; r0 += L.chunk) {
    const int64_t rows = m - r0 < L.chunk ? m - r0 : L.chunk;
    GemmArgs g;                        // H = X_new Wt   [rows x (h lds) x p]
    if (x_new) {                       // the chunk of the design, padded like the bound one: row stride ldn, padding zeroed
      if (L.ldn != p) VB_HIP(ctx, hipMemsetAsync(xn, 0, (size_t)rows * L.ldn * sizeof(double), st));
      VB_HIP(ctx, hipMemcpy2DAsync(xn, (size_t)L.ldn * sizeof(double), x_new + r0 * p, (size_t)p * sizeof(double),
                                   (size_t)p * sizeof(double), (size_t)rows, hipMemcpyHostToDevice, st));
      g.A = xn, g.lda = L.ldn;
    } else {
      g.A = md.p0 + r0 * md.ldp, g.lda = md.ldp;
    }
    g.B = base + L.o_wt, g.ldb = ldh;
    g.M = (int)rows, g.N = (int)ldh, g.K = p, g.tri_mode = 0;
    gemm_f64_launch<true>(st, g, 1, ctx->prop.multiProcessorCount, EpiStorePlain{base + L.o_h, ldh});
    VB_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(nn_predict_forward_kernel, dim3((unsigned)(rows * n_sblocks)), dim3(256), 0, st,
                       (const double*)(base + L.o_h), ldh, h, L.lds, (int)s, (const double*)(base + L.o_t), (int)n_sblocks,
                       base + L.o_eta);
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
