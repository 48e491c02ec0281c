// Sparse-design GLM target, VB_MODEL_SPARSE_GLM: the flat regression targets' density (Bernoulli-logit, Poisson or Gaussian
// observations, N(0, sd) prior, dim = p) with the design matrix held as CSR and, for the gradient, as the CSR of X' (CSC).
//
//   eta_i = sum_k v_k theta[c_k] over row i's entries;  f(theta) = sum_i l(y_i, eta_i) - |theta|^2 / (2 sd^2) + f0
//   df/dtheta_j = sum_k v_k r[i_k] over column j's entries - theta_j / sd^2,  r_i = dl/deta_i
//
// fp64 without MFMA: the work is a gather.  Both products are ONE sparse-times-dense kernel on transposed operands, so that
// lanes run over samples and every gathered operand is a contiguous 512-byte run while the sparse entry (value, index) is
// wave-uniform.  Per chunk of samples (rows of Z; ldt = the chunk rounded up to 64):
//   transpose   Zt[j][r] = Z[r][j]                      [p x ldt], zero in the pad lanes; partial |z_r|^2 per block of 64 columns
//   gather      Ht[i][r] = sum_k v_k Zt[c_k][r]         [n_data x ldt] over the CSR arrays, an fma chain in stored order
//   link        per (i, r): l_i; with a gradient Ht[i][r] <- r_i in place; a log-likelihood partial per (strip of 256
//               observations, sample); pointwise mode: the normalised term in place instead
//   gather      Gt[j][r] = sum_k v_k Rt[i_k][r]         [p x ldt], the same kernel over the CSC arrays
//   transpose   G[r][j] = Gt[j][r] - Z[r][j] / sd^2     back, with the prior
//   rowsum      f[r] = (strip partials in strip order) - (column-block partials of |z_r|^2) / (2 sd^2) + f0
// Lists (rows of X, columns of X) longer than kSparseSegment entries -- an intercept column has n_data -- are not walked by one
// wave: vb_set_model cuts them into segments of kSparseSegment entries, a second launch of the gather kernel gives every
// segment a wave of its own and writes a partial row per segment, and a combine kernel adds each list's partials in segment
// order.  Every sum has a fixed order and there are no atomics anywhere: two calls give the same bits.
#include "vb_rows_target.h"

namespace vb {

namespace {

constexpr int kSpStrip = 256;            // observations per workgroup of the link kernel: 16 waves x 16 in turn

// Zt[j][c0 + r] = Z[r][j] for a 64 x 64 tile (j0 = 64 blockIdx.x, samples 64 blockIdx.y ..), zero where r >= rows; with
// SQ the tile's sum_j Z[r][j]^2 goes to sq[blockIdx.x][sample]: a thread adds its 16 columns in order, the four waves are
// added in a fixed tree
template <bool SQ>
__global__ void __launch_bounds__(256) sp_transpose_in_kernel(const double* __restrict__ Z, int64_t ldz, int64_t rows, int p,
                                                              double* __restrict__ Zt, int64_t ldt, double* __restrict__ sq) {
  __shared__ double tile[64][65];
  __shared__ double wsum[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t j0 = (int64_t)blockIdx.x * 64, r0 = (int64_t)blockIdx.y * 64;
#pragma unroll 4
  for (int it = 0; it < 16; ++it) {
    const int r = it * 4 + wave;
    const int64_t j = j0 + lane;
    tile[r][lane] = (r0 + r < rows && j < p) ? Z[(r0 + r) * ldz + j] : 0.0;
  }
  __syncthreads();
  double s = 0.0;
#pragma unroll 4
  for (int it = 0; it < 16; ++it) {
    const int jj = it * 4 + wave;
    const double v = tile[lane][jj];
    if (j0 + jj < p) Zt[(j0 + jj) * ldt + r0 + lane] = v;
    if (SQ) s = fma(v, v, s);
  }
  if (!SQ) return;
  wsum[wave][lane] = s;
  __syncthreads();
  if (wave == 0) sq[(int64_t)blockIdx.x * ldt + r0 + lane] = (wsum[0][lane] + wsum[1][lane]) + (wsum[2][lane] + wsum[3][lane]);
}

// Out[r][j] = Tt[j][r] - ivp Z[r][j] (Z == NULL: the plain transpose) for r < rows, j < p
__global__ void __launch_bounds__(256) sp_transpose_out_kernel(const double* __restrict__ Tt, int64_t ldt, int64_t rows, int p,
                                                               const double* __restrict__ Z, int64_t ldz, double ivp,
                                                               double* __restrict__ Out, int64_t ldo) {
  __shared__ double tile[64][65];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t j0 = (int64_t)blockIdx.x * 64, r0 = (int64_t)blockIdx.y * 64;
#pragma unroll 4
  for (int it = 0; it < 16; ++it) {
    const int jj = it * 4 + wave;
    tile[jj][lane] = j0 + jj < p ? Tt[(j0 + jj) * ldt + r0 + lane] : 0.0;
  }
  __syncthreads();
#pragma unroll 4
  for (int it = 0; it < 16; ++it) {
    const int r = it * 4 + wave;
    const int64_t j = j0 + lane;
    if (r0 + r >= rows || j >= p) continue;
    double v = tile[lane][r];
    if (Z) v = fma(-ivp, Z[(r0 + r) * ldz + j], v);
    Out[(r0 + r) * ldo + j] = v;
  }
}

// Out[t][c] = sum_k val[k] In[idx[k]][c] over the entries of list t in stored order, as one fma chain: a wave per (list,
// block of 64 samples), lane = sample, the entry wave-uniform.  SEGS == false: the lists of ptr, those longer than
// kSparseSegment left to the segment launch.  SEGS == true: t runs over the segment table (triples destination, begin, end)
// and row t of Out is that segment's partial.
template <bool SEGS>
__global__ void __launch_bounds__(256) sp_gather_kernel(const int* __restrict__ ptr, const int* __restrict__ idx,
                                                        const double* __restrict__ val, const int* __restrict__ seg, int n,
                                                        const double* __restrict__ In, double* __restrict__ Out, int64_t ldt) {
  const int t = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (t >= n) return;
  const int64_t c = (int64_t)blockIdx.y * 64 + (threadIdx.x & 63);
  int b, e;
  if (SEGS) {
    b = seg[3 * (int64_t)t + 1];
    e = seg[3 * (int64_t)t + 2];
  } else {
    b = ptr[t];
    e = ptr[t + 1];
    if (e - b > kSparseSegment) return;
  }
  const double* __restrict__ in = In + c;
  double acc = 0.0;
  int k = b;
  for (; k + 8 <= e; k += 8) {          // eight gathers in flight, added in stored order
    double x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) x[u] = in[(int64_t)idx[k + u] * ldt];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc = fma(val[k + u], x[u], acc);
  }
  for (; k < e; ++k) acc = fma(val[k], in[(int64_t)idx[k] * ldt], acc);
  Out[(int64_t)t * ldt + c] = acc;
}

// sum of wsum[0 .. 15][lane] in wave order (the fixed order in which the sixteen waves of a workgroup are combined)
__device__ __forceinline__ double sp_waves_sum(const double (*wsum)[64], int lane) {
  double acc = wsum[0][lane];
#pragma unroll
  for (int w = 1; w < 16; ++w) acc += wsum[w][lane];
  return acc;
}

// Out[dst][c] = the partials of list dst in segment order; split holds triples (destination, first partial row, segments).
// A workgroup per (cut list, block of 64 samples): wave w adds a contiguous run of ceil(segments / 16) partials in order,
// the sixteen runs are added in wave order.
__global__ void __launch_bounds__(1024) sp_combine_kernel(const int* __restrict__ split, const double* __restrict__ Part,
                                                          double* __restrict__ Out, int64_t ldt) {
  __shared__ double wsum[16][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t c = (int64_t)blockIdx.y * 64 + lane;
  const int64_t t = blockIdx.x;
  const int dst = split[3 * t], first = split[3 * t + 1], n_seg = split[3 * t + 2];
  const int per = (n_seg + 15) / 16;
  const int s0 = wave * per, s1 = s0 + per < n_seg ? s0 + per : n_seg;
  double acc = 0.0;
#pragma unroll 8
  for (int s = s0; s < s1; ++s) acc += Part[(int64_t)(first + s) * ldt + c];
  wsum[wave][lane] = acc;
  __syncthreads();
  if (wave == 0) Out[(int64_t)dst * ldt + c] = sp_waves_sum(wsum, lane);
}

// MODE 0: log-likelihood partials; 1: ... and Ht overwritten by dl/deta; 2: Ht overwritten by the normalised term, no sums.
// Workgroup (strip s, block of 64 samples), sixteen waves: wave w takes the strip's observations w, w + 16, ...; lane =
// sample, so every access to Ht is a 512-byte run and y_i is wave-uniform.  part[s][sample]: a lane adds its observations
// in order, the sixteen waves are added in wave order.
template <int MODE>
__global__ void __launch_bounds__(1024) sp_link_kernel(double* __restrict__ Ht, int64_t ldt, int n_data,
                                                       const double* __restrict__ y, int link, double aux,
                                                       double* __restrict__ part) {
  __shared__ double wsum[16][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t c = (int64_t)blockIdx.y * 64 + lane;
  const int64_t i0 = (int64_t)blockIdx.x * kSpStrip;
  double ll = 0.0;
#pragma unroll 4
  for (int q = wave; q < kSpStrip; q += 16) {
    const int64_t i = i0 + q;
    if (i >= n_data) break;
    const double yi = y[i];
    double dl;
    const double t = glm_term(link, aux, yi, Ht[i * ldt + c], &dl);
    if (MODE == 2) Ht[i * ldt + c] = t + glm_obs_const(link, aux, yi);
    else ll += t;
    if (MODE == 1) Ht[i * ldt + c] = dl;
  }
  if (MODE == 2) return;
  wsum[wave][lane] = ll;
  __syncthreads();
  if (wave == 0) part[(int64_t)blockIdx.x * ldt + c] = sp_waves_sum(wsum, lane);
}

// f[r] = sum_s part[s][r] + neg_half_ivp sum_b sq[b][r] + f0: a workgroup of sixteen waves per 64 samples, wave w adds the
// strips (column blocks) w, w + 16, ... in order, the sixteen waves are added in wave order
__global__ void __launch_bounds__(1024) sp_rowsum_kernel(const double* __restrict__ part, int n_strips,
                                                         const double* __restrict__ sq, int n_cblocks, int64_t ldt,
                                                         double neg_half_ivp, double f0, int64_t rows, double* __restrict__ f) {
  __shared__ double wll[16][64], wzz[16][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t c = (int64_t)blockIdx.x * 64 + lane;
  double ll = 0.0, zz = 0.0;
#pragma unroll 8
  for (int s = wave; s < n_strips; s += 16) ll += part[(int64_t)s * ldt + c];
#pragma unroll 8
  for (int b = wave; b < n_cblocks; b += 16) zz += sq[(int64_t)b * ldt + c];
  wll[wave][lane] = ll;
  wzz[wave][lane] = zz;
  __syncthreads();
  if (wave != 0 || c >= rows) return;
  f[c] = fma(neg_half_ivp, sp_waves_sum(wzz, lane), sp_waves_sum(wll, lane)) + f0;
}

struct SpLayout {
  int64_t chunk, ldt, o_zt, o_ht, o_gt, o_part, o_sq, o_seg, o_x, o_ll, total;
  int n_strips, n_cblocks;
};

// samples per chunk: sparse_chunk_rows (vb_common.h); `pointwise`: room for the uploaded draws and the term matrix as well
SpLayout sp_layout(const ModelDev& m, int64_t n, bool grad, bool pointwise) {
  SpLayout L;
  const int64_t nd = m.n_data, p = m.dim;
  const int64_t chunk = sparse_chunk_rows(nd, p);
  L.chunk = chunk > n ? n : chunk;
  L.ldt = round_up(L.chunk, 64);
  L.n_strips = (int)((nd + kSpStrip - 1) / kSpStrip);
  L.n_cblocks = (int)((p + 63) / 64);
  const int64_t slots = m.sp_n_seg[0] > m.sp_n_seg[1] ? m.sp_n_seg[0] : m.sp_n_seg[1];
  Carver carve;
  L.o_zt = carve(p * L.ldt);
  L.o_ht = carve(nd * L.ldt);
  L.o_gt = carve(grad ? p * L.ldt : 0);
  L.o_part = carve(pointwise ? 0 : L.n_strips * L.ldt);
  L.o_sq = carve(pointwise ? 0 : L.n_cblocks * L.ldt);
  L.o_seg = carve(slots * L.ldt);            // the segment partials of the long lists: at most 2 nnz / kSparseSegment rows
  L.o_x = carve(pointwise ? L.chunk * round_up(p, 16) : 0);
  L.o_ll = carve(pointwise ? L.chunk * nd : 0);
  L.total = carve.off;
  return L;
}

int sp_check(vb_ctx* ctx, const SpLayout& L, int64_t n, int64_t d) {
  const ModelDev& m = ctx->model;
  if (n <= 0 || d != m.dim)
    return fail(ctx, VB_ERR_INVALID, "sparse regression rows: %lld x %lld samples for a model of dimension %d", (long long)n,
                (long long)d, m.dim);
  // x extents: lists / 4, 64-column blocks, strips -- all below 2^31 for n_data, p < 2^31; y extent: 64-sample blocks
  if (L.ldt / 64 > 65535 || (m.n_data + 3) / 4 > 0x7fffffffll || ((int64_t)m.dim + 3) / 4 > 0x7fffffffll)
    return fail(ctx, VB_ERR_INVALID, "sparse regression rows: a chunk of %lld samples does not fit one launch",
                (long long)L.chunk);
  return VB_OK;
}

// Out[t][:] = sum over list t of form `which` (0: CSR, rows of X; 1: CSC, columns of X) of val In[idx][:], n_lists lists
int sp_product(vb_ctx* ctx, hipStream_t st, const SpLayout& L, double* base, unsigned gy, int which, int64_t n_lists,
               const double* In, double* Out) {
  const ModelDev& m = ctx->model;
  hipLaunchKernelGGL(sp_gather_kernel<false>, dim3((unsigned)((n_lists + 3) / 4), gy), dim3(256), 0, st, m.sp_ptr[which],
                     m.sp_idx[which], m.sp_val[which], (const int*)nullptr, (int)n_lists, In, Out, L.ldt);
  VB_HIP(ctx, hipGetLastError());
  if (m.sp_n_seg[which] == 0) return VB_OK;
  hipLaunchKernelGGL(sp_gather_kernel<true>, dim3((unsigned)((m.sp_n_seg[which] + 3) / 4), gy), dim3(256), 0, st,
                     (const int*)nullptr, m.sp_idx[which], m.sp_val[which], m.sp_seg[which], m.sp_n_seg[which], In,
                     base + L.o_seg, L.ldt);
  VB_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(sp_combine_kernel, dim3((unsigned)m.sp_n_split[which], gy), dim3(1024), 0, st, m.sp_split[which],
                     (const double*)(base + L.o_seg), Out, L.ldt);
  VB_HIP(ctx, hipGetLastError());
  return VB_OK;
}

}  // namespace

int sparse_rows_enqueue(vb_ctx* ctx, hipStream_t st, const double* Z, int64_t ldz, int64_t n, int d, double* G, int64_t ldg,
                        double* f) {
  const ModelDev& m = ctx->model;
  if (m.id != VB_MODEL_SPARSE_GLM) return fail(ctx, VB_ERR_STATE, "no sparse regression model bound");
  const SpLayout L = sp_layout(m, n > 0 ? n : 1, G != nullptr, false);
  VB_TRY(sp_check(ctx, L, n, d));
  if (ldz < d || (G && ldg < d))
    return fail(ctx, VB_ERR_INVALID, "sparse regression rows: the row strides (%lld, %lld) must be >= %d", (long long)ldz,
                (long long)ldg, d);
  VB_TRY(ensure(ctx, ctx->target_work, (size_t)L.total * sizeof(double)));
  double* base = (double*)ctx->target_work.ptr;
  const int p = m.dim;
  const int64_t nd = m.n_data;
  const double ivp = 1.0 / (m.tau * m.tau);
  for (int64_t r0 = 0; r0 < n; r0 += L.chunk) {
    const int64_t rows = n - r0 < L.chunk ? n - r0 : L.chunk;
    const double* Zc = Z + r0 * ldz;
    const unsigned gy = (unsigned)((rows + 63) / 64);      // blocks of 64 samples; the pad lanes of the last one hold zeros
    const dim3 tgrid((unsigned)L.n_cblocks, gy);
    hipLaunchKernelGGL(sp_transpose_in_kernel<true>, tgrid, dim3(256), 0, st, Zc, ldz, rows, p, base + L.o_zt, L.ldt,
                       base + L.o_sq);
    VB_HIP(ctx, hipGetLastError());
    VB_TRY(sp_product(ctx, st, L, base, gy, 0, nd, base + L.o_zt, base + L.o_ht));
    const dim3 lgrid((unsigned)L.n_strips, gy);
    if (G)
      hipLaunchKernelGGL(sp_link_kernel<1>, lgrid, dim3(1024), 0, st, base + L.o_ht, L.ldt, (int)nd, m.p2, m.link, m.aux,
                         base + L.o_part);
    else
      hipLaunchKernelGGL(sp_link_kernel<0>, lgrid, dim3(1024), 0, st, base + L.o_ht, L.ldt, (int)nd, m.p2, m.link, m.aux,
                         base + L.o_part);
    VB_HIP(ctx, hipGetLastError());
    if (G) {
      VB_TRY(sp_product(ctx, st, L, base, gy, 1, p, base + L.o_ht, base + L.o_gt));
      hipLaunchKernelGGL(sp_transpose_out_kernel, tgrid, dim3(256), 0, st, (const double*)(base + L.o_gt), L.ldt, rows, p, Zc,
                         ldz, ivp, G + r0 * ldg, ldg);
      VB_HIP(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(sp_rowsum_kernel, dim3((unsigned)((rows + 63) / 64)), dim3(1024), 0, st,
                       (const double*)(base + L.o_part), L.n_strips, (const double*)(base + L.o_sq), L.n_cblocks, L.ldt,
                       -0.5 * ivp, m.f0, rows, f + r0);
    VB_HIP(ctx, hipGetLastError());
  }
  return VB_OK;
}



int sparse_set_model(vb_ctx* ctx, int64_t dim, const double* dparams, size_t n_dparams, const int64_t* iparams,
                     size_t n_iparams) {
  const char* kExpect =
      "sparse regression expects dparams = [csr values (nnz) | csc values (nnz) | y(n_data) | prior_sd | noise_sd], iparams = "
      "[n_data, p, link, nnz | csr indptr (n_data + 1) | csr indices (nnz) | csc indptr (p + 1) | csc indices (nnz)] and a "
      "dimension of p, with n_data, p and nnz below 2^31";
  if (n_iparams < 4 || !iparams || !dparams || iparams[0] <= 0 || iparams[1] <= 0 || iparams[3] < 0 ||
      iparams[0] > 0x7fffffffll || iparams[1] > 0x7fffffffll || iparams[3] > 0x7fffffffll || dim != iparams[1] ||
      iparams[2] < VB_GLM_BERNOULLI_LOGIT || iparams[2] > VB_GLM_GAUSSIAN ||
      n_iparams != (size_t)(4 + iparams[0] + 1 + iparams[1] + 1 + 2 * iparams[3]) ||
      n_dparams != (size_t)(2 * iparams[3] + iparams[0] + 2))
    return fail(ctx, VB_ERR_INVALID, "%s", kExpect);
  const int64_t nd = iparams[0], p = iparams[1], nnz = iparams[3];
  const int link = (int)iparams[2];
  const int64_t* ptr[2] = {iparams + 4, iparams + 4 + nd + 1 + nnz};
  const int64_t* idx[2] = {ptr[0] + nd + 1, ptr[1] + p + 1};
  const double* val[2] = {dparams, dparams + nnz};
  const double* ys = dparams + 2 * nnz;
  const double sd = ys[nd], nsd = ys[nd + 1];
  if (!(sd > 0.0)) return fail(ctx, VB_ERR_INVALID, "sparse regression prior_sd must be positive");
  if (!(nsd > 0.0)) return fail(ctx, VB_ERR_INVALID, "sparse regression noise_sd must be positive");
  const int64_t n_lists[2] = {nd, p}, n_other[2] = {p, nd};
  const char* form[2] = {"csr", "csc"};
  for (int w = 0; w < 2; ++w) {
    const int64_t nl = n_lists[w];
    if (ptr[w][0] != 0 || ptr[w][nl] != nnz)
      return fail(ctx, VB_ERR_INVALID, "sparse regression: the %s indptr must run from 0 to nnz = %lld (indptr[0] = %lld, "
                                       "indptr[%lld] = %lld)", form[w], (long long)nnz, (long long)ptr[w][0], (long long)nl,
                  (long long)ptr[w][nl]);
    for (int64_t t = 0; t < nl; ++t)
      if (ptr[w][t + 1] < ptr[w][t] || ptr[w][t + 1] > nnz)
        return fail(ctx, VB_ERR_INVALID, "sparse regression: the %s indptr must be monotone within [0, nnz] (indptr[%lld] = "
                                         "%lld, indptr[%lld] = %lld)", form[w], (long long)t, (long long)ptr[w][t],
                    (long long)(t + 1), (long long)ptr[w][t + 1]);
    for (int64_t t = 0; t < nl; ++t)
      for (int64_t k = ptr[w][t]; k < ptr[w][t + 1]; ++k) {
        if (idx[w][k] < 0 || idx[w][k] >= n_other[w])
          return fail(ctx, VB_ERR_INVALID, "sparse regression: %s indices must lie in [0, %lld) (indices[%lld] = %lld)", form[w],
                      (long long)n_other[w], (long long)k, (long long)idx[w][k]);
        if (k > ptr[w][t] && idx[w][k] <= idx[w][k - 1])
          return fail(ctx, VB_ERR_INVALID, "sparse regression: %s indices must increase strictly within list %lld "
                                           "(indices[%lld] = %lld after %lld)", form[w], (long long)t, (long long)k,
                      (long long)idx[w][k], (long long)idx[w][k - 1]);
        if (!std::isfinite(val[w][k]))
          return fail(ctx, VB_ERR_INVALID, "sparse regression: %s values must be finite (values[%lld])", form[w], (long long)k);
      }
  }
  {   // the CSC form must be the transpose: walking the CSR in row order meets every column's entries in stored order
    std::vector<int64_t> cur(ptr[1], ptr[1] + p);
    for (int64_t i = 0; i < nd; ++i)
      for (int64_t k = ptr[0][i]; k < ptr[0][i + 1]; ++k) {
        const int64_t j = idx[0][k], c = cur[j]++;
        if (c >= ptr[1][j + 1] || idx[1][c] != i || val[1][c] != val[0][k])
          return fail(ctx, VB_ERR_INVALID, "sparse regression: the csc form is not the transpose of the csr form (csr entry "
                                           "%lld: row %lld, column %lld)", (long long)k, (long long)i, (long long)j);
      }
  }
  for (int64_t i = 0; i < nd; ++i) {
    const double yi = ys[i];
    if (!std::isfinite(yi)) return fail(ctx, VB_ERR_INVALID, "sparse regression: y must be finite (y[%lld])", (long long)i);
    if (link == VB_GLM_BERNOULLI_LOGIT && yi != 0.0 && yi != 1.0)
      return fail(ctx, VB_ERR_INVALID, "sparse regression: logistic responses must lie in {0, 1} (y[%lld] = %g)", (long long)i, yi);
    if (link == VB_GLM_POISSON && !(yi >= 0.0))
      return fail(ctx, VB_ERR_INVALID, "sparse regression: Poisson counts must be non-negative (y[%lld] = %g)", (long long)i, yi);
  }
  ModelDev m;
  m.id = VB_MODEL_SPARSE_GLM;
  m.dim = (int)dim;
  m.n_data = nd;
  m.nnz = nnz;
  m.tau = sd;
  m.link = link;
  m.aux = link == VB_GLM_GAUSSIAN ? nsd : 1.0;
  m.c0 = 0.0;      // (the rows carry prior and constants themselves: see ModelDev::f0)
  m.f0 = glm_const_continue(-(double)p * (log(sd) + 0.5 * kLog2Pi), link, nsd, ys, nd);
  // lists longer than a segment: (list, begin, end) per segment, (list, first segment, segments) per cut list
  std::vector<int> seg[2], split[2];
  for (int w = 0; w < 2; ++w)
    for (int64_t t = 0; t < n_lists[w]; ++t) {
      const int64_t b = ptr[w][t], e = ptr[w][t + 1];
      if (e - b <= kSparseSegment) continue;
      const int first = (int)(seg[w].size() / 3), n_seg = (int)((e - b + kSparseSegment - 1) / kSparseSegment);
      for (int s = 0; s < n_seg; ++s) {
        const int64_t sb = b + (int64_t)s * kSparseSegment;
        seg[w].insert(seg[w].end(), {(int)t, (int)sb, (int)(sb + kSparseSegment < e ? sb + kSparseSegment : e)});
      }
      split[w].insert(split[w].end(), {(int)t, first, n_seg});
    }
  m.sp_n_seg[0] = (int)(seg[0].size() / 3), m.sp_n_seg[1] = (int)(seg[1].size() / 3);
  m.sp_n_split[0] = (int)(split[0].size() / 3), m.sp_n_split[1] = (int)(split[1].size() / 3);
  // [csr values | csc values | y] as doubles, then the int arrays, each starting on a 16-byte boundary: csr indptr, csr
  // indices, csc indptr, csc indices, csr segments, csr cut lists, csc segments, csc cut lists
  const size_t lens[8] = {(size_t)nd + 1, (size_t)nnz, (size_t)p + 1, (size_t)nnz,
                          seg[0].size(), split[0].size(), seg[1].size(), split[1].size()};
  size_t at[8], end = (size_t)round_up(2 * nnz + nd, 2);      // where each int array starts inside the image (in doubles)
  for (int a = 0; a < 8; ++a) {
    at[a] = end;
    end += (size_t)round_up((int64_t)(lens[a] + 1) / 2, 2);
  }
  std::vector<double> dev(end, 0.0);
  for (int64_t k = 0; k < 2 * nnz + nd; ++k) dev[k] = dparams[k];
  for (int w = 0; w < 2; ++w) {
    int* ptr32 = reinterpret_cast<int*>(dev.data() + at[2 * w]);
    int* idx32 = reinterpret_cast<int*>(dev.data() + at[2 * w + 1]);
    for (int64_t t = 0; t <= n_lists[w]; ++t) ptr32[t] = (int)ptr[w][t];
    for (int64_t k = 0; k < nnz; ++k) idx32[k] = (int)idx[w][k];
    if (!seg[w].empty()) memcpy(dev.data() + at[4 + 2 * w], seg[w].data(), seg[w].size() * sizeof(int));
    if (!split[w].empty()) memcpy(dev.data() + at[5 + 2 * w], split[w].data(), split[w].size() * sizeof(int));
  }
  VB_TRY(upload_model_params(ctx, dev, &m.p0));
  m.p2 = m.p0 + 2 * nnz;
  for (int w = 0; w < 2; ++w) {
    m.sp_val[w] = m.p0 + (size_t)w * nnz;
    m.sp_ptr[w] = reinterpret_cast<const int*>(m.p0 + at[2 * w]);
    m.sp_idx[w] = reinterpret_cast<const int*>(m.p0 + at[2 * w + 1]);
    m.sp_seg[w] = reinterpret_cast<const int*>(m.p0 + at[4 + 2 * w]);
    m.sp_split[w] = reinterpret_cast<const int*>(m.p0 + at[5 + 2 * w]);
  }
  ctx->model = m;
  return VB_OK;
}

}  // namespace vb

using namespace vb;

extern "C" {

// (the term matrix is dense [rows x n_data]: ldl = n_data, and the download's 2-D copy with equal pitches is one transfer)
int vb_sparse_glm_pointwise(vb_ctx* ctx, const double* x, int64_t s, int64_t d, double* ll_out) {
  SpLayout L;
  return rows_pointwise(
      ctx, "vb_sparse_glm_pointwise", VB_MODEL_SPARSE_GLM, "sparse regression", x, s, d, ll_out,
      [&](RowsPointwisePlan* plan) {
        L = sp_layout(ctx->model, s, false, true);
        *plan = {L.chunk, L.total, L.o_x, L.o_ll, ctx->model.n_data};
        return sp_check(ctx, L, s, d);
      },
      [&](int64_t rows, const double* X, int64_t ldx, double* LL, int64_t ldl) {
        const ModelDev& m = ctx->model;
        hipStream_t st = ctx->stream;
        double* base = (double*)ctx->target_work.ptr;
        const int64_t nd = m.n_data;
        const unsigned gy = (unsigned)((rows + 63) / 64);
        hipLaunchKernelGGL(sp_transpose_in_kernel<false>, dim3((unsigned)L.n_cblocks, gy), dim3(256), 0, st, X, ldx, rows,
                           m.dim, base + L.o_zt, L.ldt, (double*)nullptr);
        VB_HIP(ctx, hipGetLastError());
        VB_TRY(sp_product(ctx, st, L, base, gy, 0, nd, base + L.o_zt, base + L.o_ht));
        hipLaunchKernelGGL(sp_link_kernel<2>, dim3((unsigned)L.n_strips, gy), dim3(1024), 0, st, base + L.o_ht, L.ldt, (int)nd,
                           m.p2, m.link, m.aux, (double*)nullptr);
        VB_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL(sp_transpose_out_kernel, dim3((unsigned)((nd + 63) / 64), gy), dim3(256), 0, st,
                           (const double*)(base + L.o_ht), L.ldt, rows, (int)nd, (const double*)nullptr, (int64_t)0, 0.0, LL,
                           ldl);
        VB_HIP(ctx, hipGetLastError());
        return VB_OK;
      });
}

}  // extern "C"
