// Location-scale regression target, VB_MODEL_LOCSCALE: the mean and the log-scale of every observation are both linear in
// the parameter -- linear regression with an unknown (or modelled) sigma, Gaussian or Student-t (robust) noise.
//
//   theta = [b (p) | g (q)], eta_i = x_i' b, s_i = w_i' g, sigma_i = exp(s_i), z_i = (y_i - eta_i) exp(-s_i)
//   gaussian : l_i = -s_i - z_i^2 / 2 - log(2 pi) / 2                     dl/deta = z_i exp(-s_i)      dl/ds = z_i^2 - 1
//   student_t: l_i = c(nu) - s_i - (nu + 1) / 2 log1p(z_i^2 / nu)         dl/deta = k_i z_i exp(-s_i)  dl/ds = k_i z_i^2 - 1
//              k_i = (nu + 1) / (nu + z_i^2)
//   f(theta) = sum_i l_i - |b|^2 / (2 sd^2) - |g|^2 / (2 ssd^2) + (the priors' constants);  f0 holds every constant
//   df/db = X' r_eta - b / sd^2;  df/dg = W' r_s - g / ssd^2
//
// Per chunk of samples (rows of Z), general W:
//   GEMM      H = Z[:, :p] X'                           [rows x n_data x p], fp64 MFMA, plain store; the b block leads the
//                                                       parameter, so Z itself is the left operand (lda = ldz)
//   pack      Zs = Z[:, p : p + q]                      a staged copy with its own row stride round_up(q, 16): Z + p is
//                                                       16-byte aligned only for even p and the GEMM moves 16-byte pairs,
//                                                       so no offset pointer into Z or G is ever handed to it
//   GEMM      S = Zs W'                                 [rows x n_data x q]
//   link      per (r, i): l_i; with a gradient H[r][i] <- r_eta and S[r][i] <- r_s in place; a log-likelihood partial per
//             (row, strip)
//   GEMM      G[:, :p] = R_eta X - Z[:, :p] / sd^2      glm_grad_enqueue straight into the caller's G (columns < p only)
//   GEMM      Gs = R_s W - Zs / ssd^2                   glm_grad_enqueue again on a ModelDev copy that names W; same stream,
//                                                       so the two calls use ctx->glm_work one after the other
//   unpack    G[:, p : p + q] = Gs
//   rowsum    f[r] from the row's strip partials, |b|^2, |g|^2 and f0: a wave per row
// With a constant scale (no W: q = 1, s_i = g_0) there is no S, no staging and no second pair of products: the link kernel
// reads s = Z[r][p] once per workgroup, forms exp(-s) once and emits a second strip partial sum_i r_s,i, from which the
// row-sum kernel writes G[r][p].
// Every sum has a fixed order (a lane's elements in index order, the wave by shuffles, the four waves in a fixed tree) and
// there are no atomics anywhere: two calls give the same bits.
#include "vb_rows_target.h"

namespace vb {

namespace {

constexpr int kLsStrip = 1024;           // observations per workgroup of the link kernel: 256 lanes x 4

// Zs[r][j] = Z[r][p + j] (j < q), zero in the pad columns (the products read pairs, the gradient's epilogue too)
__global__ void __launch_bounds__(256) ls_pack_kernel(const double* __restrict__ Z, int64_t ldz, int64_t rows, int p, int q,
                                                      double* __restrict__ Zs, int64_t lds) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * lds) return;
  const int j = (int)(idx % lds);
  const int64_t r = idx / lds;
  Zs[idx] = j < q ? Z[r * ldz + p + j] : 0.0;
}

// G[r][p + j] = Gs[r][j] (j < q)
__global__ void __launch_bounds__(256) ls_unpack_kernel(const double* __restrict__ Gs, int64_t lds, int64_t rows, int p, int q,
                                                        double* __restrict__ G, int64_t ldg) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * q) return;
  const int64_t r = idx / q;
  const int j = (int)(idx % q);
  G[r * ldg + p + j] = Gs[r * lds + j];
}

// MODE 0: log-likelihood partials; 1: ... and H overwritten by r_eta, S by r_s (constant scale: the partials of sum r_s
// instead); 2: the normalised per-observation terms to LL (c_obs is the likelihood's constant), no sums.
// Workgroup (row r, strip s): lanes over consecutive observations, so H and S are read (and written) as contiguous 2-KiB
// runs.  S == NULL is the constant scale: one s and one exp(-s) for the whole workgroup.
template <int MODE>
__global__ void __launch_bounds__(256) ls_link_kernel(double* __restrict__ H, double* __restrict__ S, int64_t ldh,
                                                      const double* __restrict__ Z, int64_t ldz, int p, int n_data,
                                                      const double* __restrict__ y, int lik, double nu, double c_obs,
                                                      int n_strips, double* __restrict__ part, double* __restrict__ LL,
                                                      int64_t ldl) {
  const int64_t r = blockIdx.x / n_strips;
  const int s = blockIdx.x % n_strips;
  double* __restrict__ Hr = H + r * ldh;
  double* __restrict__ Sr = S ? S + r * ldh : nullptr;
  const double s0 = S ? 0.0 : Z[r * ldz + p];
  const double es0 = S ? 0.0 : exp(-s0);
  const double half_nu1 = 0.5 * (nu + 1.0), inv_nu = 1.0 / nu;
  double ll = 0.0, rs = 0.0;
#pragma unroll 1
  for (int u = 0; u < kLsStrip / 256; ++u) {
    const int i = s * kLsStrip + u * 256 + (int)threadIdx.x;
    if (i >= n_data) break;
    const double si = Sr ? Sr[i] : s0;
    const double es = Sr ? exp(-si) : es0;
    const double z = (y[i] - Hr[i]) * es, z2 = z * z;
    double t, k = 1.0;
    if (lik == VB_LOCSCALE_STUDENT_T) {
      t = -si - half_nu1 * log1p(z2 * inv_nu);
      k = (nu + 1.0) / (nu + z2);
    } else {
      t = fma(-0.5, z2, -si);
    }
    if (MODE == 2) LL[r * ldl + i] = t + c_obs;
    else ll += t;
    if (MODE == 1) {
      const double d_s = fma(k, z2, -1.0);
      Hr[i] = k * z * es;
      if (Sr) Sr[i] = d_s;
      else rs += d_s;
    }
  }
  if (MODE == 2) return;
  strip_partials_store<2>(ll, rs, part);
}

// f[r] = sum_s ll[r][s] - |b_r|^2 / (2 sd^2) - |g_r|^2 / (2 ssd^2) + f0 and, with a gradient and a constant scale,
// G[r][p] = sum_s rs[r][s] - g_0 / ssd^2: one wave per row, a lane adds its strips / columns in order
__global__ void __launch_bounds__(256) ls_rowsum_kernel(const double* __restrict__ part, int n_strips,
                                                        const double* __restrict__ Z, int64_t ldz, int p, int q,
                                                        double neg_half_ivp, double ivs, double f0, int64_t rows,
                                                        double* __restrict__ f, double* __restrict__ Gconst, int64_t ldg) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const double* __restrict__ zr = Z + r * ldz;
  double ll = 0.0, rs = 0.0, sb = 0.0, sg = 0.0;
  for (int s = lane; s < n_strips; s += 64) {
    ll += part[2 * (r * n_strips + s)];
    rs += part[2 * (r * n_strips + s) + 1];
  }
  for (int c = lane; c < p; c += 64) sb = fma(zr[c], zr[c], sb);
  for (int c = lane; c < q; c += 64) sg = fma(zr[p + c], zr[p + c], sg);
  ll = wave_sum(ll);
  rs = wave_sum(rs);
  sb = wave_sum(sb);
  sg = wave_sum(sg);
  if (lane != 0) return;
  f[r] = fma(neg_half_ivp, sb, ll) + fma(-0.5 * ivs, sg, f0);
  if (Gconst) Gconst[r * ldg + p] = fma(-ivs, zr[p], rs);
}

struct LsLayout {
  int64_t ldh, lds, chunk, o_h, o_s, o_zs, o_gs, o_part, o_x, o_ll, total;
  int n_strips;
};

// rows per chunk bound H and S together to kLocScaleChunkDoubles (the same number of rows with a constant scale, where S
// does not exist); `pointwise`: room for the uploaded draws and the term matrix as well
LsLayout ls_layout(const ModelDev& m, int64_t n, bool grad, bool pointwise) {
  LsLayout L;
  const bool general = !m.const_scale;
  L.ldh = m.ldq;
  L.lds = round_up(m.n_scale, 16);
  L.n_strips = (int)((m.n_data + kLsStrip - 1) / kLsStrip);
  L.chunk = rows_chunk(kLocScaleChunkDoubles, 2 * L.ldh, n);
  Carver carve;
  L.o_h = carve(L.chunk * L.ldh);
  L.o_s = carve(general ? L.chunk * L.ldh : 0);
  L.o_zs = carve(general ? L.chunk * L.lds : 0);
  L.o_gs = carve(general && grad ? L.chunk * L.lds : 0);
  L.o_part = carve(2 * L.chunk * L.n_strips);
  L.o_x = carve(pointwise ? L.chunk * round_up(m.dim, 16) : 0);
  L.o_ll = carve(pointwise ? L.chunk * L.ldh : 0);
  L.total = carve.off;
  return L;
}

int ls_check(vb_ctx* ctx, const LsLayout& L, int64_t n, int d) {
  const ModelDev& m = ctx->model;
  if (n <= 0 || d != m.dim)
    return fail(ctx, VB_ERR_INVALID, "location-scale rows: %lld x %d samples for a model of dimension %d", (long long)n, d,
                m.dim);
  if (L.chunk * L.n_strips > 0x7fffffffll || (L.chunk * L.lds + 255) / 256 > 0x7fffffffll)
    return fail(ctx, VB_ERR_INVALID, "location-scale rows: a chunk of %lld samples x %d strips does not fit one launch",
                (long long)L.chunk, L.n_strips);
  return VB_OK;
}

// H = Z[:, :p] X' and, with a scale design, Zs = Z[:, p : p + q], S = Zs W', for `rows` samples starting at Z
int ls_predictors(vb_ctx* ctx, hipStream_t st, const LsLayout& L, double* base, const double* Z, int64_t ldz, int64_t rows) {
  const ModelDev& m = ctx->model;
  const int n_cu = ctx->prop.multiProcessorCount;
  const GemmArgs gh = gemm_product(Z, ldz, m.p1, m.ldq, (int)rows, (int)m.n_data, m.n_feat, 0);
  gemm_f64_launch<true>(st, gh, 1, n_cu, EpiStorePlain{base + L.o_h, L.ldh});
  VB_HIP(ctx, hipGetLastError());
  if (m.const_scale) return VB_OK;
  const int64_t items = rows * L.lds;
  hipLaunchKernelGGL(ls_pack_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, Z, ldz, rows, m.n_feat, m.n_scale,
                     base + L.o_zs, L.lds);
  VB_HIP(ctx, hipGetLastError());
  const GemmArgs gs = gemm_product(base + L.o_zs, L.lds, m.w1, m.ldq, (int)rows, (int)m.n_data, m.n_scale, 0);
  gemm_f64_launch<true>(st, gs, 1, n_cu, EpiStorePlain{base + L.o_s, L.ldh});
  VB_HIP(ctx, hipGetLastError());
  return VB_OK;
}

// the constant every per-observation term carries (f0 holds n_data times it)
double ls_obs_const(const ModelDev& m) {
  if (m.link != VB_LOCSCALE_STUDENT_T) return -kHalfLog2Pi;
  return lgamma(0.5 * (m.df + 1.0)) - lgamma(0.5 * m.df) - 0.5 * (log(m.df) + 2.0 * kHalfLog2Pi - log(2.0));
}

}  // namespace

int locscale_rows_enqueue(vb_ctx* ctx, hipStream_t st, const double* Z, int64_t ldz, int64_t n, int d, double* G,
                          int64_t ldg, double* f) {
  const ModelDev& m = ctx->model;
  if (m.id != VB_MODEL_LOCSCALE) return fail(ctx, VB_ERR_STATE, "no location-scale regression model bound");
  const LsLayout L = ls_layout(m, n > 0 ? n : 1, G != nullptr, false);
  VB_TRY(ls_check(ctx, L, n, d));
  VB_TRY(rows_operands_check(ctx, "location-scale", Z, ldz, d, G, ldg));
  const int p = m.n_feat, q = m.n_scale;
  const bool general = !m.const_scale;
  VB_TRY(ensure(ctx, ctx->target_work, (size_t)L.total * sizeof(double)));
  double* base = (double*)ctx->target_work.ptr;
  double* S = general ? base + L.o_s : nullptr;
  const double ivp = 1.0 / (m.tau * m.tau), ivs = 1.0 / (m.scale_sd * m.scale_sd);
  ModelDev ms = m;           // the scale gradient is the same product on the scale design and the scale prior
  ms.p0 = m.w0;
  ms.ldp = m.ldw;
  ms.tau = m.scale_sd;
  for (int64_t r0 = 0; r0 < n; r0 += L.chunk) {
    const int64_t rows = n - r0 < L.chunk ? n - r0 : L.chunk;
    const double* Zc = Z + r0 * ldz;
    VB_TRY(ls_predictors(ctx, st, L, base, Zc, ldz, rows));
    const dim3 lgrid((unsigned)(rows * L.n_strips));
    if (G)
      hipLaunchKernelGGL(ls_link_kernel<1>, lgrid, dim3(256), 0, st, base + L.o_h, S, L.ldh, Zc, ldz, p, (int)m.n_data, m.p2,
                         m.link, m.df, 0.0, L.n_strips, base + L.o_part, (double*)nullptr, (int64_t)0);
    else
      hipLaunchKernelGGL(ls_link_kernel<0>, lgrid, dim3(256), 0, st, base + L.o_h, S, L.ldh, Zc, ldz, p, (int)m.n_data, m.p2,
                         m.link, m.df, 0.0, L.n_strips, base + L.o_part, (double*)nullptr, (int64_t)0);
    VB_HIP(ctx, hipGetLastError());
    double* Gc = G ? G + r0 * ldg : nullptr;
    if (G) {
      // columns < p: the epilogue's pair store is issued for col + 1 < p only and the split reduction skips columns >= p,
      // so neither touches the scale block that is filled next
      VB_TRY(glm_grad_enqueue(ctx, st, m, base + L.o_h, L.ldh, Zc, Gc, ldz, rows, p));
      if (general) {
        // (after the coefficient product in stream order: both may use ctx->glm_work for their split slabs)
        VB_TRY(glm_grad_enqueue(ctx, st, ms, S, L.ldh, base + L.o_zs, base + L.o_gs, L.lds, rows, q));
        hipLaunchKernelGGL(ls_unpack_kernel, dim3((unsigned)((rows * q + 255) / 256)), dim3(256), 0, st,
                           (const double*)(base + L.o_gs), L.lds, rows, p, q, Gc, ldg);
        VB_HIP(ctx, hipGetLastError());
      }
    }
    hipLaunchKernelGGL(ls_rowsum_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, (const double*)(base + L.o_part),
                       L.n_strips, Zc, ldz, p, q, -0.5 * ivp, ivs, m.f0, rows, f + r0, general ? (double*)nullptr : Gc, ldg);
    VB_HIP(ctx, hipGetLastError());
  }
  return VB_OK;
}

int locscale_set_model(vb_ctx* ctx, int64_t dim, const double* dparams, size_t n_dparams, const int64_t* iparams,
                       size_t n_iparams) {
  const char* kExpect =
      "location-scale regression expects dparams = [X(n_data x p) | y(n_data) | W(n_data x q), absent with a constant scale "
      "| prior_sd | scale_prior_sd | df], iparams = [n_data, p, q, likelihood, constant_scale] (constant_scale = 1: q = 1) "
      "and a dimension of p + q";
  if (n_iparams != 5 || !iparams || !dparams || iparams[0] <= 0 || iparams[1] < 1 || iparams[2] < 1 ||
      iparams[0] > 0x7fffffffll || iparams[1] > 0x7fffffffll || iparams[2] > 0x7fffffffll || dim > 0x7fffffffll ||
      dim != iparams[1] + iparams[2] || iparams[3] < VB_LOCSCALE_GAUSSIAN || iparams[3] > VB_LOCSCALE_STUDENT_T ||
      iparams[4] < 0 || iparams[4] > 1 || (iparams[4] == 1 && iparams[2] != 1) ||
      n_dparams != (size_t)(iparams[0] * iparams[1] + iparams[0] + (iparams[4] ? 0 : iparams[0] * iparams[2])) + 3)
    return fail(ctx, VB_ERR_INVALID, "%s", kExpect);
  const int64_t nd = iparams[0], p = iparams[1], q = iparams[2];
  const int lik = (int)iparams[3];
  const bool cs = iparams[4] == 1;
  const double* ys = dparams + nd * p;
  const double* wsrc = ys + nd;
  const double* tail = wsrc + (cs ? 0 : nd * q);
  const double sd = tail[0], ssd = tail[1], nu = tail[2];
  if (!(sd > 0.0)) return fail(ctx, VB_ERR_INVALID, "location-scale prior_sd must be positive");
  if (!(ssd > 0.0)) return fail(ctx, VB_ERR_INVALID, "location-scale scale_prior_sd must be positive");
  if (!(nu > 0.0) || !std::isfinite(nu)) return fail(ctx, VB_ERR_INVALID, "location-scale df must be positive and finite");
  ModelDev m;
  m.id = VB_MODEL_LOCSCALE;
  m.dim = (int)dim;
  m.n_data = nd;
  m.n_feat = (int)p;
  m.n_scale = (int)q;
  m.const_scale = cs ? 1 : 0;
  m.ldp = round_up(p, 16);
  m.ldq = round_up(nd, 16);
  m.ldw = cs ? 0 : round_up(q, 16);
  m.tau = sd;
  m.scale_sd = ssd;
  m.df = nu;
  m.link = lik;
  m.c0 = 0.0;      // (the rows carry priors and constants themselves: see ModelDev::f0)
  // b ~ N(0, sd), g ~ N(0, ssd); the likelihood's constant: n_data times -log(2 pi) / 2, or c(nu) of the Student t
  m.f0 = -(double)p * (log(sd) + 0.5 * kLog2Pi) - (double)q * (log(ssd) + 0.5 * kLog2Pi);
  if (lik == VB_LOCSCALE_STUDENT_T)
    m.f0 += (double)nd * (lgamma(0.5 * (nu + 1.0)) - lgamma(0.5 * nu) - 0.5 * (log(nu) + kLog2Pi - log(2.0)));
  else
    m.f0 -= (double)nd * 0.5 * kLog2Pi;
  // [X (nd x ldp) | X' (p x ldq) | y (ldq) | W (nd x ldw) | W' (q x ldq)]: the softmax target's layout, then the scale
  // design in the same two forms (absent with a constant scale)
  const size_t o_xt = (size_t)nd * m.ldp, o_y = o_xt + (size_t)p * m.ldq, o_w = o_y + (size_t)m.ldq;
  const size_t o_wt = o_w + (size_t)nd * m.ldw;
  std::vector<double> dev(o_wt + (cs ? 0 : (size_t)q * m.ldq), 0.0);
  pack_design(dev, 0, dparams, nd, p, m.ldp, m.ldq);
  for (int64_t i = 0; i < nd; ++i) dev[o_y + i] = ys[i];
  if (!cs) pack_design(dev, o_w, wsrc, nd, q, m.ldw, m.ldq);
  VB_TRY(upload_model_params(ctx, dev, &m.p0));
  m.p1 = m.p0 + o_xt;
  m.p2 = m.p0 + o_y;
  if (!cs) {
    m.w0 = m.p0 + o_w;
    m.w1 = m.p0 + o_wt;
  }
  ctx->model = m;
  return VB_OK;
}

}  // namespace vb

using namespace vb;

extern "C" {

int vb_locscale_pointwise(vb_ctx* ctx, const double* x, int64_t s, int64_t d, double* ll_out) {
  LsLayout L;
  return rows_pointwise(
      ctx, "vb_locscale_pointwise", VB_MODEL_LOCSCALE, "location-scale regression", x, s, d, ll_out,
      [&](RowsPointwisePlan* plan) {
        L = ls_layout(ctx->model, s, false, true);
        *plan = {L.chunk, L.total, L.o_x, L.o_ll, L.ldh};
        return ls_check(ctx, L, s, (int)d);
      },
      [&](int64_t rows, const double* X, int64_t ldx, double* LL, int64_t ldl) {
        const ModelDev& m = ctx->model;
        double* base = (double*)ctx->target_work.ptr;
        VB_TRY(ls_predictors(ctx, ctx->stream, L, base, X, ldx, rows));
        hipLaunchKernelGGL(ls_link_kernel<2>, dim3((unsigned)(rows * L.n_strips)), dim3(256), 0, ctx->stream, base + L.o_h,
                           m.const_scale ? (double*)nullptr : base + L.o_s, L.ldh, X, ldx, m.n_feat, (int)m.n_data, m.p2, m.link,
                           m.df, ls_obs_const(m), L.n_strips, (double*)nullptr, LL, ldl);
        VB_HIP(ctx, hipGetLastError());
        return VB_OK;
      });
}

}  // extern "C"
