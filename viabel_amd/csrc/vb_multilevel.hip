// Varying-intercept (multilevel) GLM target, VB_MODEL_MULTILEVEL: group-level effects whose scale is itself a parameter,
// non-centred and unconstrained.
//
//   theta = [b (p) | u (J) | omega], tau = exp(omega), eta_i = x_i' b + tau u_{g_i}
//   f(theta) = sum_i l(y_i, eta_i) - |b|^2 / (2 sd^2) - |u|^2 / 2 - tau^2 / (2 tau_sd^2) + omega + f0
//   r_i = dl / d eta_i;  df/db = X' r - b / sd^2;  df/du_j = tau sum_{g_i = j} r_i - u_j;
//   df/domega = tau sum_i r_i u_{g_i} - tau^2 / tau_sd^2 + 1
//
// The observations are sorted by group (vb_set_model checks it), so group j owns the contiguous run
// grp_off[j] .. grp_off[j + 1] of every row of the residual matrix.  Per chunk of samples (rows of Z):
//   GEMM      H = Z[:, :p] X'                           [rows x n_data x p], fp64 MFMA, plain store; the b block leads the
//                                                       parameter, so Z itself is the left operand (lda = ldz)
//   link      per (r, i): eta = H[r][i] + tau_r u_{r, g_i}; glm_term; with a gradient H[r][i] is overwritten by r_i; two
//             partials per (row, strip): the log-likelihood and sum r_i u_{g_i}
//   GEMM      G[:, :p] = R X - Z[:, :p] / sd^2          glm_grad_enqueue straight into the caller's G (its epilogue and its
//                                                       split reduction write columns < p only)
//   group     G[r][p + j] = tau_r (sum of R[r] over group j's run) - u_rj: a wave per group, lanes stride the run
//   rowsum    f[r] and G[r][p + J] from the row's strip partials, |b|^2, |u|^2 and omega: a wave per row
// Every sum has a fixed order (a lane's elements in index order, the wave by shuffles, the four waves in a fixed tree) and
// there are no atomics anywhere: two calls give the same bits.
#include "vb_rows_target.h"

namespace vb {

namespace {

constexpr int kMlStrip = 1024;           // observations per workgroup of the link kernel: 256 lanes x 4
constexpr int kMlGroupsPerBlock = 64;    // groups per workgroup of the group kernel: 16 per wave

// MODE 0: log-likelihood partials; 1: ... and the partials of sum r_i u_{g_i}, H overwritten by the residuals r_i; 2: the
// normalised per-observation terms to LL, no sums.
// Workgroup (row r, strip s): lanes over consecutive observations, so H is read (and written) as contiguous 2-KiB runs; the
// group effect of an observation is a gather from the row's u block -- the observations are sorted by group, so the lanes
// of a wave ask for one or two addresses almost everywhere.
template <int MODE>
__global__ void __launch_bounds__(256) ml_link_kernel(double* __restrict__ H, int64_t ldh, const double* __restrict__ Z,
                                                      int64_t ldz, int p, int J, int n_data, const double* __restrict__ y,
                                                      const int* __restrict__ grp_of, int link, double aux, int n_strips,
                                                      double* __restrict__ part, double* __restrict__ LL, int64_t ldl) {
  const int64_t r = blockIdx.x / n_strips;
  const int s = blockIdx.x % n_strips;
  const double* __restrict__ ur = Z + r * ldz + p;
  const double tau = exp(ur[J]);
  double* __restrict__ Hr = H + r * ldh;
  double ll = 0.0, ru = 0.0;
#pragma unroll 1
  for (int q = 0; q < kMlStrip / 256; ++q) {
    const int i = s * kMlStrip + q * 256 + (int)threadIdx.x;
    if (i >= n_data) break;
    const double ug = ur[grp_of[i]];
    const double yi = y[i];
    double dl;
    const double t = glm_term(link, aux, yi, fma(tau, ug, Hr[i]), &dl);
    if (MODE == 2) LL[r * ldl + i] = t + glm_obs_const(link, aux, yi);
    else ll += t;
    if (MODE == 1) {
      Hr[i] = dl;
      ru = fma(dl, ug, ru);
    }
  }
  if (MODE == 2) return;
  strip_partials_store<2>(ll, ru, part);
}

// G[r][p + j] = tau_r sum_{i in run j} R[r][i] - u_rj.  Workgroup (row r, block of 64 groups), a wave per group in turn:
// its lanes stride the run (coalesced, any length: a run longer than a strip of the link kernel is just more steps), an
// empty run leaves the sum at zero and the entry at -u_rj exactly.
__global__ void __launch_bounds__(256) ml_group_kernel(const double* __restrict__ R, int64_t ldh, const double* __restrict__ Z,
                                                       int64_t ldz, int p, int J, const int* __restrict__ grp_off,
                                                       int n_gblocks, double* __restrict__ G, int64_t ldg) {
  const int64_t r = blockIdx.x / n_gblocks;
  const int gb = blockIdx.x % n_gblocks;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double* __restrict__ ur = Z + r * ldz + p;
  const double tau = exp(ur[J]);
  const double* __restrict__ Rr = R + r * ldh;
#pragma unroll 1
  for (int q = wave; q < kMlGroupsPerBlock; q += 4) {
    const int j = gb * kMlGroupsPerBlock + q;
    if (j >= J) break;
    const int end = grp_off[j + 1];
    double sum = 0.0;
    for (int i = grp_off[j] + lane; i < end; i += 64) sum += Rr[i];
    sum = wave_sum(sum);
    if (lane == 0) G[r * ldg + p + j] = fma(tau, sum, -ur[j]);
  }
}

// f[r] = sum_s ll[r][s] - |b_r|^2 / (2 sd^2) - |u_r|^2 / 2 - tau^2 / (2 tau_sd^2) + omega + f0 and, with a gradient,
// G[r][p + J] = tau sum_s ru[r][s] - tau^2 / tau_sd^2 + 1: one wave per row, a lane adds its strips / columns in order
__global__ void __launch_bounds__(256) ml_rowsum_kernel(const double* __restrict__ part, int n_strips,
                                                        const double* __restrict__ Z, int64_t ldz, int p, int J,
                                                        double neg_half_ivp, double ivt, double f0, int64_t rows,
                                                        double* __restrict__ f, double* __restrict__ G, int64_t ldg) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const double* __restrict__ zr = Z + r * ldz;
  double ll = 0.0, ru = 0.0, sb = 0.0, su = 0.0;
  for (int s = lane; s < n_strips; s += 64) {
    ll += part[2 * (r * n_strips + s)];
    ru += part[2 * (r * n_strips + s) + 1];
  }
  for (int c = lane; c < p; c += 64) sb = fma(zr[c], zr[c], sb);
  for (int c = lane; c < J; c += 64) su = fma(zr[p + c], zr[p + c], su);
  ll = wave_sum(ll);
  ru = wave_sum(ru);
  sb = wave_sum(sb);
  su = wave_sum(su);
  if (lane != 0) return;
  const double omega = zr[p + J], tau = exp(omega), t2 = tau * tau;
  f[r] = (fma(neg_half_ivp, sb, ll) - 0.5 * su) + (fma(-0.5 * ivt, t2, omega) + f0);
  if (G) G[r * ldg + p + J] = fma(tau, ru, fma(-ivt, t2, 1.0));
}

struct MlLayout {
  int64_t ldh, chunk, o_h, o_part, o_x, o_ll, total;
  int n_strips, n_gblocks;
};

// rows per chunk bound H to kMultilevelChunkDoubles; `pointwise`: room for the uploaded draws and the term matrix as well
MlLayout ml_layout(const ModelDev& m, int64_t n, bool pointwise) {
  MlLayout L;
  L.ldh = m.ldq;
  L.n_strips = (int)((m.n_data + kMlStrip - 1) / kMlStrip);
  L.n_gblocks = (m.n_groups + kMlGroupsPerBlock - 1) / kMlGroupsPerBlock;
  L.chunk = rows_chunk(kMultilevelChunkDoubles, L.ldh, n);
  Carver carve;
  L.o_h = carve(L.chunk * L.ldh);
  L.o_part = carve(2 * L.chunk * L.n_strips);
  L.o_x = carve(pointwise ? L.chunk * round_up(m.dim, 16) : 0);
  L.o_ll = carve(pointwise ? L.chunk * L.ldh : 0);
  L.total = carve.off;
  return L;
}

int ml_check(vb_ctx* ctx, const MlLayout& L, int64_t n, int d) {
  const ModelDev& m = ctx->model;
  if (n <= 0 || d != m.dim)
    return fail(ctx, VB_ERR_INVALID, "multilevel rows: %lld x %d samples for a model of dimension %d", (long long)n, d, m.dim);
  if (L.chunk * L.n_strips > 0x7fffffffll || L.chunk * L.n_gblocks > 0x7fffffffll)
    return fail(ctx, VB_ERR_INVALID, "multilevel rows: a chunk of %lld samples x %d strips / %d group blocks does not fit one "
                                     "launch", (long long)L.chunk, L.n_strips, L.n_gblocks);
  return VB_OK;
}

// H = Z[:, :p] X' for `rows` samples starting at Z (the chunk's first row)
int ml_predictors(vb_ctx* ctx, hipStream_t st, const MlLayout& L, double* base, const double* Z, int64_t ldz, int64_t rows) {
  const ModelDev& m = ctx->model;
  const GemmArgs g = gemm_product(Z, ldz, m.p1, m.ldq, (int)rows, (int)m.n_data, m.n_feat, 0);
  gemm_f64_launch<true>(st, g, 1, ctx->prop.multiProcessorCount, EpiStorePlain{base + L.o_h, L.ldh});
  VB_HIP(ctx, hipGetLastError());
  return VB_OK;
}

}  // namespace

int multilevel_rows_enqueue(vb_ctx* ctx, hipStream_t st, const double* Z, int64_t ldz, int64_t n, int d, double* G,
                            int64_t ldg, double* f) {
  const ModelDev& m = ctx->model;
  if (m.id != VB_MODEL_MULTILEVEL) return fail(ctx, VB_ERR_STATE, "no multilevel regression model bound");
  const MlLayout L = ml_layout(m, n > 0 ? n : 1, false);
  VB_TRY(ml_check(ctx, L, n, d));
  VB_TRY(rows_operands_check(ctx, "multilevel", Z, ldz, d, G, ldg));
  const int p = m.n_feat, J = m.n_groups;
  VB_TRY(ensure(ctx, ctx->target_work, (size_t)L.total * sizeof(double)));
  double* base = (double*)ctx->target_work.ptr;
  const double ivp = 1.0 / (m.tau * m.tau), ivt = 1.0 / (m.hyper_sd * m.hyper_sd);
  for (int64_t r0 = 0; r0 < n; r0 += L.chunk) {
    const int64_t rows = n - r0 < L.chunk ? n - r0 : L.chunk;
    const double* Zc = Z + r0 * ldz;
    VB_TRY(ml_predictors(ctx, st, L, base, Zc, ldz, rows));
    const dim3 lgrid((unsigned)(rows * L.n_strips));
    if (G)
      hipLaunchKernelGGL(ml_link_kernel<1>, lgrid, dim3(256), 0, st, base + L.o_h, L.ldh, Zc, ldz, p, J, (int)m.n_data, m.p2,
                         m.grp_of, m.link, m.aux, L.n_strips, base + L.o_part, (double*)nullptr, (int64_t)0);
    else
      hipLaunchKernelGGL(ml_link_kernel<0>, lgrid, dim3(256), 0, st, base + L.o_h, L.ldh, Zc, ldz, p, J, (int)m.n_data, m.p2,
                         m.grp_of, m.link, m.aux, L.n_strips, base + L.o_part, (double*)nullptr, (int64_t)0);
    VB_HIP(ctx, hipGetLastError());
    double* Gc = G ? G + r0 * ldg : nullptr;
    if (G) {
      // columns < p: the epilogue's pair store is issued for col + 1 < p only and the split reduction skips columns >= p,
      // so neither touches the u block that the group kernel fills next
      VB_TRY(glm_grad_enqueue(ctx, st, m, base + L.o_h, L.ldh, Zc, Gc, ldz, rows, p));
      hipLaunchKernelGGL(ml_group_kernel, dim3((unsigned)(rows * L.n_gblocks)), dim3(256), 0, st,
                         (const double*)(base + L.o_h), L.ldh, Zc, ldz, p, J, m.grp_off, L.n_gblocks, Gc, ldg);
      VB_HIP(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(ml_rowsum_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, (const double*)(base + L.o_part),
                       L.n_strips, Zc, ldz, p, J, -0.5 * ivp, ivt, m.f0, rows, f + r0, Gc, ldg);
    VB_HIP(ctx, hipGetLastError());
  }
  return VB_OK;
}

int multilevel_set_model(vb_ctx* ctx, int64_t dim, const double* dparams, size_t n_dparams, const int64_t* iparams,
                         size_t n_iparams) {
  const char* kExpect =
      "multilevel regression expects dparams = [X(n_data x p) | y(n_data) | prior_sd | tau_sd | noise_sd], iparams = "
      "[n_data, n_groups, link | offsets(n_groups + 1) | group of each observation(n_data)] and a dimension of "
      "p + n_groups + 1";
  if (n_iparams < 3 || !iparams || !dparams || iparams[0] <= 0 || iparams[1] < 1 || iparams[0] > 0x7fffffffll ||
      iparams[1] > 0x7fffffffll || dim > 0x7fffffffll || dim - iparams[1] - 1 < 1 ||
      iparams[2] < VB_GLM_BERNOULLI_LOGIT || iparams[2] > VB_GLM_GAUSSIAN ||
      n_iparams != (size_t)(3 + iparams[1] + 1 + iparams[0]) ||
      n_dparams != (size_t)(iparams[0] * (dim - iparams[1] - 1) + iparams[0]) + 3)
    return fail(ctx, VB_ERR_INVALID, "%s", kExpect);
  const int64_t nd = iparams[0], ng = iparams[1], p = dim - ng - 1;
  const int link = (int)iparams[2];
  const int64_t* off = iparams + 3;
  const int64_t* grp = off + ng + 1;
  const double* ys = dparams + nd * p;
  const double sd = ys[nd], tsd = ys[nd + 1], nsd = ys[nd + 2];
  if (!(sd > 0.0)) return fail(ctx, VB_ERR_INVALID, "multilevel prior_sd must be positive");
  if (!(tsd > 0.0)) return fail(ctx, VB_ERR_INVALID, "multilevel tau_sd must be positive");
  if (!(nsd > 0.0)) return fail(ctx, VB_ERR_INVALID, "multilevel noise_sd must be positive");
  if (off[0] != 0 || off[ng] != nd)
    return fail(ctx, VB_ERR_INVALID, "multilevel offsets must run from 0 to n_data (offsets[0] = %lld, offsets[%lld] = %lld)",
                (long long)off[0], (long long)ng, (long long)off[ng]);
  for (int64_t j = 0; j < ng; ++j)
    if (off[j + 1] < off[j])
      return fail(ctx, VB_ERR_INVALID, "multilevel offsets must be monotone (offsets[%lld] = %lld > offsets[%lld] = %lld)",
                  (long long)j, (long long)off[j], (long long)(j + 1), (long long)off[j + 1]);
  for (int64_t i = 0; i < nd; ++i)
    if (grp[i] < 0 || grp[i] >= ng)
      return fail(ctx, VB_ERR_INVALID, "multilevel group labels must lie in [0, n_groups) (groups[%lld] = %lld)", (long long)i,
                  (long long)grp[i]);
  for (int64_t j = 0; j < ng; ++j)
    for (int64_t i = off[j]; i < off[j + 1]; ++i)
      if (grp[i] != j)
        return fail(ctx, VB_ERR_INVALID, "multilevel observations must be sorted by group: observation %lld lies in the run of "
                                         "group %lld and carries the label %lld", (long long)i, (long long)j, (long long)grp[i]);
  if (link == VB_GLM_POISSON)
    for (int64_t i = 0; i < nd; ++i)
      if (!(ys[i] >= 0.0)) return fail(ctx, VB_ERR_INVALID, "Poisson counts must be non-negative");
  ModelDev m;
  m.id = VB_MODEL_MULTILEVEL;
  m.dim = (int)dim;
  m.n_data = nd;
  m.n_groups = (int)ng;
  m.n_feat = (int)p;
  m.ldp = round_up(p, 16);
  m.ldq = round_up(nd, 16);
  m.tau = sd;
  m.hyper_sd = tsd;
  m.link = link;
  m.aux = link == VB_GLM_GAUSSIAN ? nsd : 1.0;
  m.c0 = 0.0;      // (the rows carry priors and constants themselves: see ModelDev::f0)
  // b ~ N(0, sd), u ~ N(0, 1), tau ~ HalfNormal(tsd); the likelihood's constant as the flat regression target has it
  m.f0 = -(double)p * (log(sd) + 0.5 * kLog2Pi) - 0.5 * (double)ng * kLog2Pi + log(2.0) - log(tsd) - 0.5 * kLog2Pi;
  m.f0 = glm_const_continue(m.f0, link, nsd, ys, nd);
  // [X (nd x ldp) | X' (p x ldq) | y (ldq) | offsets (ng + 1 ints) | group of each observation (nd ints)]: the logistic
  // target's layout with p in place of dim, then the two int arrays, each starting on a 16-byte boundary
  const size_t o_xt = (size_t)nd * m.ldp, o_y = o_xt + (size_t)p * m.ldq, o_off = o_y + (size_t)m.ldq;
  const size_t o_grp = o_off + (size_t)round_up((ng + 2) / 2, 2);
  std::vector<double> dev(o_grp + (size_t)round_up((nd + 1) / 2, 2), 0.0);
  pack_design(dev, 0, dparams, nd, p, m.ldp, m.ldq);
  for (int64_t i = 0; i < nd; ++i) dev[o_y + i] = ys[i];
  int* off32 = reinterpret_cast<int*>(dev.data() + o_off);
  int* grp32 = reinterpret_cast<int*>(dev.data() + o_grp);
  for (int64_t j = 0; j <= ng; ++j) off32[j] = (int)off[j];
  for (int64_t i = 0; i < nd; ++i) grp32[i] = (int)grp[i];
  VB_TRY(upload_model_params(ctx, dev, &m.p0));
  m.p1 = m.p0 + o_xt;
  m.p2 = m.p0 + o_y;
  m.grp_off = reinterpret_cast<const int*>(m.p0 + o_off);
  m.grp_of = reinterpret_cast<const int*>(m.p0 + o_grp);
  ctx->model = m;
  return VB_OK;
}

}  // namespace vb

using namespace vb;

extern "C" {

int vb_multilevel_pointwise(vb_ctx* ctx, const double* x, int64_t s, int64_t d, double* ll_out) {
  MlLayout L;
  return rows_pointwise(
      ctx, "vb_multilevel_pointwise", VB_MODEL_MULTILEVEL, "multilevel regression", x, s, d, ll_out,
      [&](RowsPointwisePlan* plan) {
        L = ml_layout(ctx->model, s, true);
        *plan = {L.chunk, L.total, L.o_x, L.o_ll, L.ldh};
        return ml_check(ctx, L, s, (int)d);
      },
      [&](int64_t rows, const double* X, int64_t ldx, double* LL, int64_t ldl) {
        const ModelDev& m = ctx->model;
        double* base = (double*)ctx->target_work.ptr;
        VB_TRY(ml_predictors(ctx, ctx->stream, L, base, X, ldx, rows));
        hipLaunchKernelGGL(ml_link_kernel<2>, dim3((unsigned)(rows * L.n_strips)), dim3(256), 0, ctx->stream, base + L.o_h,
                           L.ldh, X, ldx, m.n_feat, m.n_groups, (int)m.n_data, m.p2, m.grp_of, m.link, m.aux, L.n_strips,
                           (double*)nullptr, LL, ldl);
        VB_HIP(ctx, hipGetLastError());
        return VB_OK;
      });
}

}  // extern "C"
