// RealNVP normalizing flow (NVPFlow, viabel/approximations.py:452-550) under ExclusiveKL.
//
// Coupling layer i (mask m = m_i, m' = 1 - m), nets s_i / t_i dense with tanh hidden layers (x W + b, W [in][out]):
//   y = m x,   s = tanh(s_net(y)) m',   t = t_net(y) m',   x_{i+1} = y + m' (x_i exp(s) + t),   log q = log p0(z0) - sum s.
// value = -mean_n [log p(x_K) - log p0(z0) + sum s] in both estimator forms.  Gradients (theta = every W, b):
//   plain form  (total derivative along g, the form the reference means at objectives.py:163): one reverse sweep through
//               g with cotangent grad log p(x_K) on the output and 1 on every unmasked s entry;
//   path form   (use_path_deriv): a reverse sweep through the inverse f with respect to x only gives grad_x log q(x_K)
//               (cotangent grad log p0(z0) on z0, -1 on every unmasked s entry), then the sweep through g with cotangent
//               grad log p(x_K) - grad_x log q(x_K).  Both sweeps reuse the forward pass's activations (x_i, s, hidden
//               layers): f(x_{i+1}) = x_i up to rounding.
// Every dense layer is one gemm_f64_launch (vb_gemm_f64.h) with its own epilogue:
//   forward         H = act(A W + b)                 A = the activations (N x in), B = W (padded copy, [in][out])
//   input gradient  dA = (dH W') * (1 - A^2)         B = W' (padded transposed copy, [out][in])
//   weight gradient [dW | db] = [A | 1]' dH          A k-major (the activation buffers carry a column of ones after their
//                                                     `in` columns, so the last output row is the bias gradient), split
//                                                     over the sample axis into slabs, slabs summed in fixed order
// straight into the gradient at the layer's offset (the flat layout keeps W and b of a layer adjacent).  Weight-gradient
// rows of masked-out inputs are exact zeros: those columns of y are 0.  No atomics: results are bit-reproducible.
#include "vb_common.h"
#include "vb_fit_run.h"
#include "vb_gemm_f64.h"

#include <cmath>

struct vb_flow {
  struct Layer {
    int64_t woff, boff;        // W ([in][out], row-major) and b in theta
    int64_t wp, wt;            // padded copy of W (row stride ldo) / of W' (row stride ldi) in `wpack`
    int in, out, ldo, ldi;
  };
  vb_ctx* ctx = nullptr;
  int64_t d = 0, k = 0, p = 0;
  int nl[2] = {0, 0};          // dense layers of the t-net (0) and the s-net (1)
  std::vector<int> widths[2];  // nl + 1 widths: d, hidden ..., d
  std::vector<Layer> layers;   // coupling i, net q, layer l -> layers[(i * 2 + q) * maxl + l]
  int maxl = 0, maxw = 0;
  vb::DeviceBuffer masks;      // k x d, 0 / 1
  vb::DeviceBuffer table;      // device copy of `layers`
  vb::DeviceBuffer wpack;      // padded W and W' of every layer
  vb::DeviceBuffer theta;      // [theta (p) | prior parameter (2 d)]
  vb::DeviceBuffer out;        // [value | grad (p)]
  vb::DeviceBuffer work;       // activations and sweep buffers for n_cap rows
  int64_t n_cap = 0;
  int64_t wpack_len = 0;
};

namespace vb {

namespace {

constexpr int kFlowChunk = 8192;          // rows per forward pass of vb_flow_sample
constexpr double kLog2PiFlow = 1.8378770664093454835606594728112;

inline int64_t al32(int64_t x) { return round_up(x, 32); }      // 256-B alignment of every sub-buffer

// geometry of the work buffer for `n` rows
struct FlowWork {
  int64_t ldx, ldy, ldm;
  double *X, *Y, *S, *DS, *DT, *P0, *P1, *C, *A, *GY, *F, *LP0, *ROWV, *LQ, *slab;
  std::vector<double*> H;      // [(i * 2 + q) * maxl + l], l < nl[q] - 1
  std::vector<int64_t> ldh;
  int64_t nb;                  // rows per block (the capacity): coupling i's block of X / Y / S starts i * nb rows in
  int64_t slab_stride;
  size_t doubles;
};

constexpr int kMaxSplits = 32;

int wg_splits(int64_t n) {
  int64_t s = n / 128;
  s = s < 1 ? 1 : (s > kMaxSplits ? kMaxSplits : s);
  const int64_t ks = round_up((n + s - 1) / s, kGemmBK);
  return (int)((n + ks - 1) / ks);          // every split has a non-empty k range
}

FlowWork flow_layout(const vb_flow& f, int64_t n, double* base) {
  FlowWork w;
  const int64_t K = f.k, D = f.d;
  w.ldx = round_up(D, 16);
  w.ldy = round_up(D + 2, 16);               // + the column of ones (+1 so that no 16-B pair straddles a row)
  w.ldm = round_up(f.maxw, 16);
  w.nb = n;
  int64_t o = 0;
  auto take = [&](int64_t len) { double* q = base ? base + o : nullptr; o += al32(len); return q; };
  w.X = take((K + 1) * n * w.ldx);
  w.Y = take(K * n * w.ldy);
  w.S = take(K * n * w.ldx);
  w.H.assign((size_t)K * 2 * f.maxl, nullptr);
  w.ldh.assign((size_t)K * 2 * f.maxl, 0);
  for (int64_t i = 0; i < K; ++i)
    for (int q = 0; q < 2; ++q)
      for (int l = 0; l + 1 < f.nl[q]; ++l) {
        const int64_t ld = round_up(f.widths[q][l + 1] + 2, 16);
        w.ldh[(i * 2 + q) * f.maxl + l] = ld;
        w.H[(i * 2 + q) * f.maxl + l] = take(n * ld);
      }
  w.DS = take(n * w.ldm);
  w.DT = take(n * w.ldm);
  w.P0 = take(n * w.ldm);
  w.P1 = take(n * w.ldm);
  w.C = take(n * w.ldx);
  w.A = take(n * w.ldx);
  w.GY = take(n * w.ldx);
  w.F = take(n);
  w.LP0 = take(n);
  w.ROWV = take(n);
  w.LQ = take(n);
  int64_t slab = 0;
  for (const auto& L : f.layers) slab = slab > (int64_t)(L.in + 1) * L.out ? slab : (int64_t)(L.in + 1) * L.out;
  w.slab_stride = al32(slab);
  w.slab = take(kMaxSplits * w.slab_stride);
  w.doubles = (size_t)o + 32;
  return w;
}

// ---- epilogues ---------------------------------------------------------------------------------------------------
struct EpiFlowHidden {            // H = tanh(acc + b)
  double* H;
  int64_t ld;
  const double* b;
  __device__ void operator()(int, int row, int col, double acc) const { H[(int64_t)row * ld + col] = tanh(acc + b[col]); }
};
struct EpiFlowSLast {             // s = tanh(acc + b) (1 - m)
  double* S;
  int64_t ld;
  const double* b;
  const double* m;
  __device__ void operator()(int, int row, int col, double acc) const {
    S[(int64_t)row * ld + col] = tanh(acc + b[col]) * (1.0 - m[col]);
  }
};
struct EpiFlowTLast {             // t = (acc + b) (1 - m); x_{i+1} = m x + (1 - m) (x exp(s) + t); y_{i+1} = m_{i+1} x_{i+1}
  const double* X;
  const double* S;
  double* Xn;
  int64_t ldx;
  double* Yn;
  int64_t ldy;
  const double* b;
  const double* m;
  const double* mn;
  __device__ void operator()(int, int row, int col, double acc) const {
    const int64_t e = (int64_t)row * ldx + col;
    const double mb = 1.0 - m[col];
    const double t = (acc + b[col]) * mb;
    const double x = X[e];
    const double xn = m[col] * x + mb * (x * exp(S[e]) + t);
    Xn[e] = xn;
    if (Yn) Yn[(int64_t)row * ldy + col] = mn[col] * xn;
  }
};
struct EpiFlowStore {
  double* O;
  int64_t ld;
  __device__ void operator()(int, int row, int col, double acc) const { O[(int64_t)row * ld + col] = acc; }
};
struct EpiFlowTanhBack {          // dA = acc (1 - h^2), h the layer's input activation
  double* O;
  int64_t ldo;
  const double* H;
  int64_t ldh;
  __device__ void operator()(int, int row, int col, double acc) const {
    const double h = H[(int64_t)row * ldh + col];
    O[(int64_t)row * ldo + col] = acc * (1.0 - h * h);
  }
};
struct EpiFlowCouple {            // c_i = direct part + m (dy_t + dy_s)
  double* C;
  int64_t ld;
  const double* GY;
  const double* m;
  __device__ void operator()(int, int row, int col, double acc) const {
    const int64_t e = (int64_t)row * ld + col;
    C[e] = C[e] + m[col] * (acc + GY[e]);
  }
};
struct EpiFlowSlab {              // split z's partial [dW | db] (row-major, (in + 1) x out)
  double* slab;
  int64_t stride;
  int ldo;
  __device__ void operator()(int split, int row, int col, double acc) const {
    slab[(int64_t)split * stride + (int64_t)row * ldo + col] = acc;
  }
};

// ---- glue kernels ------------------------------------------------------------------------------------------------
__global__ void flow_pack_kernel(const vb_flow::Layer* table, const double* theta, double* wpack) {
  const vb_flow::Layer L = table[blockIdx.y];
  const int64_t cnt = (int64_t)L.in * L.out;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < cnt; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = e / L.out, c = e - r * L.out;
    const double v = theta[L.woff + e];
    wpack[L.wp + r * L.ldo + c] = v;
    wpack[L.wt + c * L.ldi + r] = v;
  }
}

__global__ void flow_ones_kernel(double* buf, int64_t ld, int64_t col, int64_t n) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n) buf[r * ld + col] = 1.0;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return __shfl(v, 0, 64);
}

// one wave per row: z0 = mu + sigma eps, y_0 = m_0 z0, log p0(z0) and (want_grad) grad log p0(z0)
__global__ void flow_prior_kernel(const double* eps, int64_t lde, int64_t n, int d, const double* prior, int student,
                                  double df, double c0, const double* m0, double* X, int64_t ldx, double* Y, int64_t ldy,
                                  double* A, double* lp0) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= n) return;
  double acc = 0.0;
  for (int j = lane; j < d; j += 64) {
    const double e = eps[row * lde + j];
    const double ls = prior[d + j], isd = exp(-ls);
    const double z = prior[j] + exp(ls) * e;
    X[row * ldx + j] = z;
    Y[row * ldy + j] = m0[j] * z;
    const double r = (z - prior[j]) * isd;
    double term, gr;
    if (student) {
      term = c0 - 0.5 * (df + 1.0) * log1p(r * r / df) - ls;
      gr = -(df + 1.0) / df * r / (1.0 + r * r / df) * isd;
    } else {
      term = -0.5 * r * r - ls - 0.5 * kLog2PiFlow;
      gr = -r * isd;
    }
    acc += term;
    if (A) A[row * ldx + j] = gr;
  }
  acc = wave_sum(acc);
  if (lane == 0) lp0[row] = acc;
}

// Cotangent terms of coupling i (elementwise over n x d).  c = C[e] is the cotangent of the layer's output (mode 0: the
// sweep through g; plus1 = 1 adds the plain form's d(sum s)/ds) or of its input (mode 1: the sweep through f, C = a_i).
// Writes the last-layer deltas of the s-net (DS, through tanh) and the t-net (DT), and the part of the next cotangent that
// does not go through the nets into C.
__global__ void flow_terms_kernel(int mode, double plus1, int64_t n, int d, const double* m, const double* X,
                                  const double* S, int64_t ldx, double* C, double* DS, double* DT, int64_t ldm) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * d) return;
  const int64_t row = e / d;
  const int col = (int)(e - row * d);
  const int64_t ix = row * ldx + col, im = row * ldm + col;
  const double mk = m[col], mb = 1.0 - mk;
  const double c = C[ix], s = S[ix], x = X[ix];
  if (mode == 0) {
    const double es = exp(s);
    DT[im] = mb * c;
    DS[im] = mb * (c * x * es + plus1) * (1.0 - s * s);
    C[ix] = mk * c + mb * c * es;
  } else {
    const double ems = exp(-s);
    DT[im] = -mb * c * ems;
    DS[im] = mb * (-c * x - 1.0) * (1.0 - s * s);
    C[ix] = mk * c + mb * c * ems;
  }
}

__global__ void flow_sub_kernel(double* C, const double* A, int64_t ld, int64_t n, int d) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * d) return;
  const int64_t row = e / d, ix = row * ld + (e - row * d);
  C[ix] = C[ix] - A[ix];
}

// one wave per row: log q = log p0 - sum_i sum_j s_i, and (F) the row's log p - log q
__global__ void flow_rows_kernel(int64_t n, int d, int K, const double* S, int64_t ldx, int64_t layer_stride,
                                 const double* lp0, const double* F, double* lq, double* rowv) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= n) return;
  double acc = 0.0;
  for (int i = 0; i < K; ++i)
    for (int j = lane; j < d; j += 64) acc += S[i * layer_stride + row * ldx + j];
  acc = wave_sum(acc);
  if (lane == 0) {
    const double q = lp0[row] - acc;
    lq[row] = q;
    if (F) rowv[row] = F[row] - q;
  }
}

// out[0] = sum of v[0 .. n) in a fixed order (one workgroup)
__global__ void __launch_bounds__(1024) flow_sum_kernel(const double* v, int64_t n, double* out) {
  __shared__ double red[1024];
  double acc = 0.0;
  for (int64_t r = threadIdx.x; r < n; r += 1024) acc += v[r];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 512; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = red[0];
}

__global__ void flow_slab_sum_kernel(const double* slab, int64_t stride, int splits, int64_t cnt, double* dst) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= cnt) return;
  double acc = slab[e];
  for (int z = 1; z < splits; ++z) acc += slab[(int64_t)z * stride + e];
  dst[e] = acc;
}

__global__ void flow_scale_kernel(double* v, int64_t cnt, double s) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < cnt) v[e] *= s;
}

unsigned blocks_for(int64_t cnt, int per = 256) { return (unsigned)((cnt + per - 1) / per); }

// ---- host side ---------------------------------------------------------------------------------------------------
bool flow_known(vb_ctx* ctx, const vb_flow* f) {
  for (const vb_flow* g : ctx->flows)
    if (g == f) return true;
  return false;
}

int flow_ensure_work(vb_ctx* ctx, vb_flow* f, int64_t n) {
  if (n <= f->n_cap) return VB_OK;
  const FlowWork geo = flow_layout(*f, n, nullptr);
  VB_TRY(ensure(ctx, f->work, geo.doubles * sizeof(double)));
  VB_HIP(ctx, hipMemsetAsync(f->work.ptr, 0, geo.doubles * sizeof(double), ctx->stream));
  const FlowWork w = flow_layout(*f, n, (double*)f->work.ptr);
  // the columns of ones that turn the weight-gradient products into [dW | db]
  for (int64_t i = 0; i < f->k; ++i) {
    hipLaunchKernelGGL(flow_ones_kernel, dim3(blocks_for(n)), dim3(256), 0, ctx->stream, w.Y + i * w.nb * w.ldy, w.ldy,
                       f->d, n);
    for (int q = 0; q < 2; ++q)
      for (int l = 0; l + 1 < f->nl[q]; ++l) {
        const int64_t h = (i * 2 + q) * f->maxl + l;
        hipLaunchKernelGGL(flow_ones_kernel, dim3(blocks_for(n)), dim3(256), 0, ctx->stream, w.H[h], w.ldh[h],
                           (int64_t)f->widths[q][l + 1], n);
      }
  }
  VB_HIP(ctx, hipGetLastError());
  f->n_cap = n;
  return VB_OK;
}

struct FlowCall {
  const double* eps;
  int64_t lde, n;
  int student;
  double df, c0;
};

int flow_check_prior(vb_ctx* ctx, int family, double df, FlowCall& c) {
  if (family == VB_FAMILY_MF_GAUSSIAN) {
    c.student = 0, c.df = 0.0, c.c0 = 0.0;
    return VB_OK;
  }
  if (family == VB_FAMILY_MF_STUDENT_T) {
    if (!(df > 0.0)) return fail(ctx, VB_ERR_INVALID, "NVPFlow prior: df must be positive");
    c.student = 1, c.df = df;
    c.c0 = std::lgamma(0.5 * (df + 1.0)) - std::lgamma(0.5 * df) - 0.5 * std::log(df * 3.14159265358979323846);
    return VB_OK;
  }
  return fail(ctx, VB_ERR_UNSUPPORTED, "NVPFlow prior must be MFGaussian or MFStudentT (family %d)", family);
}

// padded weight copies from the device-resident theta
int flow_pack(vb_ctx* ctx, vb_flow* f) {
  hipStream_t st = ctx->stream;
  const double* th = (const double*)f->theta.ptr;
  int64_t most = 0;
  unsigned n_real = 0;       // the device table holds only the layers that exist: nets of unequal depth leave padding entries
  for (const auto& L : f->layers) {
    most = most > (int64_t)L.in * L.out ? most : (int64_t)L.in * L.out;
    n_real += L.in > 0 ? 1 : 0;
  }
  unsigned gx = blocks_for(most);
  gx = gx > 256 ? 256 : gx;
  hipLaunchKernelGGL(flow_pack_kernel, dim3(gx, n_real), dim3(256), 0, st,
                     (const vb_flow::Layer*)f->table.ptr, th, (double*)f->wpack.ptr);
  VB_HIP(ctx, hipGetLastError());
  return VB_OK;
}

// theta and the prior parameter to the device, padded weight copies
int flow_upload(vb_ctx* ctx, vb_flow* f, const double* theta, const double* prior) {
  hipStream_t st = ctx->stream;
  double* th = (double*)f->theta.ptr;
  VB_HIP(ctx, hipMemcpyAsync(th, theta, (size_t)f->p * sizeof(double), hipMemcpyHostToDevice, st));
  VB_HIP(ctx, hipMemcpyAsync(th + al32(f->p), prior, (size_t)2 * f->d * sizeof(double), hipMemcpyHostToDevice, st));
  return flow_pack(ctx, f);
}

// forward pass g over the rows of the call: x_0 .. x_K, y_i, s_i, hidden activations, log p0
int flow_forward(vb_ctx* ctx, vb_flow* f, const FlowWork& w, const FlowCall& c, bool want_a) {
  hipStream_t st = ctx->stream;
  const int n_cu = ctx->prop.multiProcessorCount;
  const int64_t n = c.n, D = f->d, K = f->k;
  const double* th = (const double*)f->theta.ptr;
  const double* prior = th + al32(f->p);
  const double* wp = (const double*)f->wpack.ptr;
  const double* masks = (const double*)f->masks.ptr;
  hipLaunchKernelGGL(flow_prior_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, c.eps, c.lde, n, (int)D, prior,
                     c.student, c.df, c.c0, masks, w.X, w.ldx, w.Y, w.ldy, want_a ? w.A : (double*)nullptr, w.LP0);
  VB_HIP(ctx, hipGetLastError());
  for (int64_t i = 0; i < K; ++i) {
    const double* m = masks + i * D;
    const double* Yi = w.Y + i * w.nb * w.ldy;
    double* Si = w.S + i * w.nb * w.ldx;
    for (int q = 1; q >= 0; --q) {             // s-net first: the t-net's last epilogue reads s
      const double* Ain = Yi;
      int64_t lda = w.ldy;
      for (int l = 0; l < f->nl[q]; ++l) {
        const vb_flow::Layer& L = f->layers[(i * 2 + q) * f->maxl + l];
        GemmArgs g;
        g.A = Ain, g.lda = lda, g.B = wp + L.wp, g.ldb = L.ldo;
        g.M = (int)n, g.N = L.out, g.K = L.in, g.tri_mode = 0;
        const double* b = th + L.boff;
        if (l + 1 < f->nl[q]) {
          const int64_t h = (i * 2 + q) * f->maxl + l;
          gemm_f64_launch<true>(st, g, 1, n_cu, EpiFlowHidden{w.H[h], w.ldh[h], b});
          Ain = w.H[h], lda = w.ldh[h];
        } else if (q == 1) {
          gemm_f64_launch<true>(st, g, 1, n_cu, EpiFlowSLast{Si, w.ldx, b, m});
        } else {
          const bool more = i + 1 < K;
          gemm_f64_launch<true>(st, g, 1, n_cu,
                                EpiFlowTLast{w.X + i * w.nb * w.ldx, Si, w.X + (i + 1) * w.nb * w.ldx, w.ldx,
                                             more ? w.Y + (i + 1) * w.nb * w.ldy : nullptr, w.ldy, b, m,
                                             more ? m + D : nullptr});
        }
        VB_HIP(ctx, hipGetLastError());
      }
    }
  }
  return VB_OK;
}

// reverse sweep through coupling i's nets: cotangent buffer C (the output's for mode 0, the input's for mode 1)
// becomes the other side's; mode 0 also forms the weight gradients into out_grad (unscaled sums)
int flow_coupling_back(vb_ctx* ctx, vb_flow* f, const FlowWork& w, int64_t n, int64_t i, int mode, double plus1,
                       double* C, double* out_grad, bool need_input) {
  hipStream_t st = ctx->stream;
  const int n_cu = ctx->prop.multiProcessorCount;
  const int64_t D = f->d;
  const double* wp = (const double*)f->wpack.ptr;
  const double* m = (const double*)f->masks.ptr + i * D;
  const int splits = wg_splits(n);
  hipLaunchKernelGGL(flow_terms_kernel, dim3(blocks_for(n * D)), dim3(256), 0, st, mode, plus1, n, (int)D, m,
                     (const double*)(w.X + i * w.nb * w.ldx), (const double*)(w.S + i * w.nb * w.ldx), w.ldx, C, w.DS, w.DT,
                     w.ldm);
  VB_HIP(ctx, hipGetLastError());
  for (int q = 1; q >= 0; --q) {               // s-net, then the t-net (whose first layer closes the cotangent)
    double* delta = q == 1 ? w.DS : w.DT;
    int pp = 0;
    for (int l = f->nl[q] - 1; l >= 0; --l) {
      const vb_flow::Layer& L = f->layers[(i * 2 + q) * f->maxl + l];
      const int64_t hprev = (i * 2 + q) * f->maxl + l - 1;
      const double* Aprev = l == 0 ? w.Y + i * w.nb * w.ldy : w.H[hprev];
      const int64_t lda_prev = l == 0 ? w.ldy : w.ldh[hprev];
      if (mode == 0) {                         // [dW | db] = [A | 1]' delta, split over the samples
        GemmArgs g;
        g.A = Aprev, g.lda = lda_prev, g.B = delta, g.ldb = w.ldm;
        g.M = L.in + 1, g.N = L.out, g.K = (int)n, g.tri_mode = 0;
        gemm_f64_launch<false>(st, g, splits, n_cu, EpiFlowSlab{w.slab, w.slab_stride, L.out});
        VB_HIP(ctx, hipGetLastError());
        const int64_t cnt = (int64_t)(L.in + 1) * L.out;
        hipLaunchKernelGGL(flow_slab_sum_kernel, dim3(blocks_for(cnt)), dim3(256), 0, st, (const double*)w.slab,
                           w.slab_stride, splits, cnt, out_grad + L.woff);
        VB_HIP(ctx, hipGetLastError());
      }
      if (l == 0 && !need_input) break;
      GemmArgs g;                              // delta W'
      g.A = delta, g.lda = w.ldm, g.B = wp + L.wt, g.ldb = L.ldi;
      g.M = (int)n, g.N = L.in, g.K = L.out, g.tri_mode = 0;
      if (l > 0) {
        double* nxt = pp ? w.P1 : w.P0;
        gemm_f64_launch<true>(st, g, 1, n_cu, EpiFlowTanhBack{nxt, w.ldm, w.H[hprev], w.ldh[hprev]});
        delta = nxt;
        pp ^= 1;
      } else if (q == 1) {
        gemm_f64_launch<true>(st, g, 1, n_cu, EpiFlowStore{w.GY, w.ldx});
      } else {
        gemm_f64_launch<true>(st, g, 1, n_cu, EpiFlowCouple{C, w.ldx, w.GY, m});
      }
      VB_HIP(ctx, hipGetLastError());
    }
  }
  return VB_OK;
}

int flow_call_setup(vb_ctx* ctx, vb_flow* f, int slot, int64_t n, int prior_family, double prior_df,
                    const double* prior_param, const double* theta, FlowCall& c) {
  if (!f || !flow_known(ctx, f)) return fail(ctx, VB_ERR_INVALID, "unknown NVPFlow handle for this context");
  if (!prior_param || !theta) return fail(ctx, VB_ERR_INVALID, "NULL argument");
  if (slot < 0 || slot >= VB_MAX_SLOTS) return fail(ctx, VB_ERR_INVALID, "slot %d out of range [0, %d)", slot, VB_MAX_SLOTS);
  const NoiseSlot& ns = ctx->noise[slot];
  if (!ns.buf.ptr) return fail(ctx, VB_ERR_STATE, "noise slot %d is empty", slot);
  if (n <= 0 || n > ns.n || ns.d != f->d)
    return fail(ctx, VB_ERR_INVALID, "noise slot %d holds %lld x %lld, the flow needs %lld x %lld", slot,
                (long long)ns.n, (long long)ns.d, (long long)n, (long long)f->d);
  VB_TRY(flow_check_prior(ctx, prior_family, prior_df, c));
  c.eps = (const double*)ns.buf.ptr;
  c.lde = ns.ld;
  c.n = n;
  VB_HIP(ctx, hipSetDevice(ctx->device));
  VB_TRY(main_stream_write(ctx));
  return flow_upload(ctx, f, theta, prior_param);
}

}  // namespace

void flow_release_all(vb_ctx* ctx) {
  for (vb_flow* f : ctx->flows) delete f;
  ctx->flows.clear();
}

}  // namespace vb

using namespace vb;

int vb_flow_create(vb_ctx* ctx, int64_t d, int64_t k, const double* masks, int64_t n_t, const int64_t* widths_t,
                   int64_t n_s, const int64_t* widths_s, vb_flow** out) {
  if (!ctx || !masks || !widths_t || !widths_s || !out) return fail(ctx, VB_ERR_INVALID, "NULL argument");
  *out = nullptr;
  if (d <= 0 || k <= 0 || n_t <= 0 || n_s <= 0 || d > (1 << 20) || k > 4096 || n_t > 64 || n_s > 64)
    return fail(ctx, VB_ERR_INVALID, "NVPFlow: bad shape (d %lld, k %lld, layers %lld / %lld)", (long long)d,
                (long long)k, (long long)n_t, (long long)n_s);
  for (int64_t e = 0; e < k * d; ++e)
    if (masks[e] != 0.0 && masks[e] != 1.0) return fail(ctx, VB_ERR_INVALID, "NVPFlow: mask entries must be 0 or 1");
  const int64_t* wsrc[2] = {widths_t, widths_s};
  const int64_t nls[2] = {n_t, n_s};
  for (int q = 0; q < 2; ++q) {
    if (wsrc[q][0] != d || wsrc[q][nls[q]] != d) return fail(ctx, VB_ERR_INVALID, "NVPFlow: a net must map d to d");
    for (int64_t l = 0; l <= nls[q]; ++l)
      if (wsrc[q][l] <= 0 || wsrc[q][l] > (1 << 20)) return fail(ctx, VB_ERR_INVALID, "NVPFlow: bad layer width");
  }
  VB_HIP(ctx, hipSetDevice(ctx->device));
  vb_flow* f = new vb_flow;
  f->ctx = ctx, f->d = d, f->k = k;
  for (int q = 0; q < 2; ++q) {
    f->nl[q] = (int)nls[q];
    f->widths[q].assign(wsrc[q], wsrc[q] + nls[q] + 1);
    for (int w : f->widths[q]) f->maxw = f->maxw > w ? f->maxw : w;
  }
  f->maxl = f->nl[0] > f->nl[1] ? f->nl[0] : f->nl[1];
  f->layers.assign((size_t)k * 2 * f->maxl, vb_flow::Layer{0, 0, 0, 0, 0, 0, 0, 0});
  int64_t off = 0, pk = 0;
  for (int64_t i = 0; i < k; ++i)
    for (int q = 0; q < 2; ++q)                // flat layout: coupling i's t-net, then its s-net
      for (int l = 0; l < f->nl[q]; ++l) {
        vb_flow::Layer& L = f->layers[(i * 2 + q) * f->maxl + l];
        L.in = f->widths[q][l], L.out = f->widths[q][l + 1];
        L.ldo = (int)round_up(L.out, 16), L.ldi = (int)round_up(L.in, 16);
        L.woff = off, L.boff = off + (int64_t)L.in * L.out;
        off = L.boff + L.out;
        L.wp = pk;
        pk += al32((int64_t)L.in * L.ldo);
        L.wt = pk;
        pk += al32((int64_t)L.out * L.ldi);
      }
  f->p = off;
  f->wpack_len = pk;
  // the table holds only the layers that exist (padding entries of the shorter net are skipped by the pack kernel's grid)
  std::vector<vb_flow::Layer> real;
  for (const auto& L : f->layers)
    if (L.in > 0) real.push_back(L);
  int rc = VB_OK;
  auto step = [&](hipError_t e) {
    if (e != hipSuccess && rc == VB_OK) rc = fail(ctx, VB_ERR_HIP, "NVPFlow: %s", hipGetErrorString(e));
  };
  step(f->masks.alloc((size_t)k * d * sizeof(double)));
  step(f->table.alloc(real.size() * sizeof(vb_flow::Layer)));
  step(f->wpack.alloc((size_t)(pk + 32) * sizeof(double)));
  step(f->theta.alloc((size_t)(al32(f->p) + 2 * d + 32) * sizeof(double)));
  step(f->out.alloc((size_t)(1 + f->p + 32) * sizeof(double)));
  if (rc == VB_OK) {
    step(hipMemsetAsync(f->wpack.ptr, 0, (size_t)(pk + 32) * sizeof(double), ctx->stream));
    step(hipMemcpyAsync(f->masks.ptr, masks, (size_t)k * d * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    step(hipMemcpyAsync(f->table.ptr, real.data(), real.size() * sizeof(vb_flow::Layer), hipMemcpyHostToDevice,
                        ctx->stream));
    step(hipStreamSynchronize(ctx->stream));
  }
  if (rc != VB_OK) {
    delete f;
    return rc;
  }
  ctx->flows.push_back(f);
  *out = f;
  return VB_OK;
}

int vb_flow_destroy(vb_ctx* ctx, vb_flow* flow) {
  if (!ctx || !flow) return fail(ctx, VB_ERR_INVALID, "NULL argument");
  for (size_t i = 0; i < ctx->flows.size(); ++i)
    if (ctx->flows[i] == flow) {
      (void)hipSetDevice(ctx->device);
      VB_TRY(sync_streams(ctx));
      ctx->flows.erase(ctx->flows.begin() + (long)i);
      delete flow;
      return VB_OK;
    }
  return fail(ctx, VB_ERR_INVALID, "unknown NVPFlow handle for this context");
}

int vb_flow_param_dim(vb_ctx* ctx, const vb_flow* flow, int64_t* p) {
  if (!ctx || !flow || !p) return fail(ctx, VB_ERR_INVALID, "NULL argument");
  if (!flow_known(ctx, flow)) return fail(ctx, VB_ERR_INVALID, "unknown NVPFlow handle for this context");
  *p = flow->p;
  return VB_OK;
}

namespace vb {
namespace {

// [value | grad (p)] of ExclusiveKL over the call's rows at the device-resident theta (f->theta, packed) into `dout`,
// all-reduced over a sharded job's ranks: what vb_flow_elbo_grad copies out and vb_flow_fit steps along
int flow_evaluate(vb_ctx* ctx, vb_flow* f, const FlowCall& c, int64_t n_total, bool path, double* dout) {
  const int64_t n = c.n;
  const FlowWork lw = flow_layout(*f, f->n_cap, (double*)f->work.ptr);
  hipStream_t st = ctx->stream;
  VB_TRY(flow_forward(ctx, f, lw, c, path));
  // the model at x_K: log p into F, grad log p into C (the sweep's cotangent)
  double* XK = lw.X + f->k * lw.nb * lw.ldx;
  VB_TRY(model_grad_rows(ctx, XK, lw.ldx, n, f->d, lw.C, lw.F));
  hipLaunchKernelGGL(flow_rows_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, n, (int)f->d, (int)f->k,
                     (const double*)lw.S, lw.ldx, lw.nb * lw.ldx, (const double*)lw.LP0, (const double*)lw.F, lw.LQ, lw.ROWV);
  hipLaunchKernelGGL(flow_sum_kernel, dim3(1), dim3(1024), 0, st, (const double*)lw.ROWV, n, dout);
  VB_HIP(ctx, hipGetLastError());
  if (path) {                                  // grad_x log q(x_K): sweep through f, a_0 = grad log p0(z0)
    for (int64_t i = 0; i < f->k; ++i) VB_TRY(flow_coupling_back(ctx, f, lw, n, i, 1, 0.0, lw.A, nullptr, true));
    hipLaunchKernelGGL(flow_sub_kernel, dim3(blocks_for(n * f->d)), dim3(256), 0, st, lw.C, (const double*)lw.A, lw.ldx,
                       n, (int)f->d);
    VB_HIP(ctx, hipGetLastError());
  }
  for (int64_t i = f->k - 1; i >= 0; --i)
    VB_TRY(flow_coupling_back(ctx, f, lw, n, i, 0, path ? 0.0 : 1.0, lw.C, dout + 1, i > 0));
  VB_TRY(comm_allreduce_sum(ctx, st, dout, (size_t)(1 + f->p)));
  hipLaunchKernelGGL(flow_scale_kernel, dim3(blocks_for(1 + f->p)), dim3(256), 0, st, dout, 1 + f->p,
                     -1.0 / (double)n_total);
  VB_HIP(ctx, hipGetLastError());
  return VB_OK;
}

}  // namespace
}  // namespace vb

int vb_flow_elbo_grad(vb_ctx* ctx, vb_flow* flow, int slot, int64_t n, int64_t n_total, int prior_family,
                      double prior_df, const double* prior_param, const double* theta, unsigned flags, double* out) {
  if (!ctx || !out) return fail(ctx, VB_ERR_INVALID, "NULL argument");
  if (ctx->model.id < 0) return fail(ctx, VB_ERR_STATE, "no model bound (vb_set_model)");
  if (flags & ~VB_FLAG_PATH_DERIV) return fail(ctx, VB_ERR_UNSUPPORTED, "NVPFlow: unknown flags %u", flags);
  if (n_total < n) return fail(ctx, VB_ERR_INVALID, "n_total must be >= n");
  FlowCall c;
  VB_TRY(flow_call_setup(ctx, flow, slot, n, prior_family, prior_df, prior_param, theta, c));
  if (ctx->model.dim != flow->d) return fail(ctx, VB_ERR_INVALID, "model dimension %d != flow dimension %lld",
                                             ctx->model.dim, (long long)flow->d);
  vb_flow* f = flow;
  VB_TRY(flow_ensure_work(ctx, f, n));
  hipStream_t st = ctx->stream;
  double* dout = (double*)f->out.ptr;
  VB_TRY(flow_evaluate(ctx, f, c, n_total, (flags & VB_FLAG_PATH_DERIV) != 0, dout));
  VB_HIP(ctx, hipMemcpyAsync(out, dout, (size_t)(1 + f->p) * sizeof(double), hipMemcpyDeviceToHost, st));
  VB_HIP(ctx, hipStreamSynchronize(st));
  return comm_check(ctx);
}

int vb_flow_fit(vb_ctx* ctx, vb_flow* flow, int slot, int64_t n, int64_t n_total, int64_t row_offset, int prior_family,
                double prior_df, const double* prior_param, unsigned flags, int noise_kind, double noise_df, uint64_t seed,
                uint64_t first_stream, int opt_kind, const double hyper[4], int64_t n_iters, double* theta, double* state,
                int has_state, double* values, double* history, int64_t hist_len, double* directions, double* gradients) {
  if (!ctx || !hyper || !theta || !values || !prior_param) return fail(ctx, VB_ERR_INVALID, "NULL argument");
  VB_TRY(FitRun::check(ctx, "n", n > 0, n, n_total, n_iters, opt_kind, hist_len, history, has_state, state));
  if (!flow || !flow_known(ctx, flow)) return fail(ctx, VB_ERR_INVALID, "unknown NVPFlow handle for this context");
  if (flags & ~VB_FLAG_PATH_DERIV)
    return fail(ctx, VB_ERR_UNSUPPORTED, "NVPFlow: unknown flags %u", flags);
  vb_flow* f = flow;
  FlowCall c;
  VB_TRY(flow_check_prior(ctx, prior_family, prior_df, c));
  if (ctx->model.dim != f->d)
    return fail(ctx, VB_ERR_INVALID, "model dimension %d != flow dimension %lld", ctx->model.dim, (long long)f->d);
  VB_HIP(ctx, hipSetDevice(ctx->device));
  VB_TRY(main_stream_write(ctx));
  VB_TRY(noise_slot_alloc(ctx, slot, n, f->d));
  NoiseSlot& ns = ctx->noise[slot];
  c.eps = (const double*)ns.buf.ptr;
  c.lde = ns.ld;
  c.n = n;

  FitRun run(ctx);      // (the parameter stays in the flow's own theta)
  VB_TRY(run.begin(f->p, 0, n_iters, opt_kind, hyper, state, has_state, history, hist_len, directions, gradients));
  run.step.theta = (double*)f->theta.ptr;
  VB_TRY(flow_upload(ctx, f, theta, prior_param));
  VB_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the caller's buffers are pageable: copies above are staged
  VB_TRY(flow_ensure_work(ctx, f, n));

  const bool path = (flags & VB_FLAG_PATH_DERIV) != 0;
  for (int64_t k = 0; k < n_iters; ++k) {
    run.iteration(k);
    VB_TRY(rng_fill(ctx, (double*)ns.buf.ptr, ns.ld, noise_kind, noise_df, seed, first_stream + (uint64_t)k, row_offset,
                    n, f->d));
    VB_TRY(flow_evaluate(ctx, f, c, n_total, path, run.out));
    VB_TRY(fit_step_enqueue(ctx, run.step));
    if (k + 1 < n_iters) VB_TRY(flow_pack(ctx, f));      // the padded weight copies of the stepped parameter
    VB_TRY(run.after_step(k));
  }
  return run.finish(theta, values, state);
}

int vb_flow_sample(vb_ctx* ctx, vb_flow* flow, int slot, int64_t n, int prior_family, double prior_df,
                   const double* prior_param, const double* theta, double* x, double* log_q, double* log_p) {
  if (!ctx || !log_q) return fail(ctx, VB_ERR_INVALID, "NULL argument");
  if (log_p && ctx->model.id < 0) return fail(ctx, VB_ERR_STATE, "no model bound (vb_set_model)");
  FlowCall c;
  VB_TRY(flow_call_setup(ctx, flow, slot, n, prior_family, prior_df, prior_param, theta, c));
  if (log_p && ctx->model.dim != flow->d)
    return fail(ctx, VB_ERR_INVALID, "model dimension %d != flow dimension %lld", ctx->model.dim, (long long)flow->d);
  vb_flow* f = flow;
  const int64_t chunk = n < kFlowChunk ? n : kFlowChunk;
  VB_TRY(flow_ensure_work(ctx, f, chunk));
  hipStream_t st = ctx->stream;
  const double* eps0 = c.eps;
  for (int64_t r0 = 0; r0 < n; r0 += chunk) {
    const int64_t rows = n - r0 < chunk ? n - r0 : chunk;
    const FlowWork lw = flow_layout(*f, f->n_cap, (double*)f->work.ptr);
    c.eps = eps0 + r0 * c.lde;
    c.n = rows;
    VB_TRY(flow_forward(ctx, f, lw, c, false));
    double* XK = lw.X + f->k * lw.nb * lw.ldx;
    if (log_p) VB_TRY(model_logp_rows(ctx, XK, lw.ldx, rows, f->d, lw.F));
    hipLaunchKernelGGL(flow_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, rows, (int)f->d, (int)f->k,
                       (const double*)lw.S, lw.ldx, lw.nb * lw.ldx, (const double*)lw.LP0, (const double*)nullptr, lw.LQ,
                       (double*)nullptr);
    VB_HIP(ctx, hipGetLastError());
    if (x)
      VB_HIP(ctx, hipMemcpy2DAsync(x + r0 * f->d, (size_t)f->d * sizeof(double), XK, (size_t)lw.ldx * sizeof(double),
                                   (size_t)f->d * sizeof(double), (size_t)rows, hipMemcpyDeviceToHost, st));
    VB_HIP(ctx, hipMemcpyAsync(log_q + r0, lw.LQ, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost, st));
    if (log_p) VB_HIP(ctx, hipMemcpyAsync(log_p + r0, lw.F, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost, st));
    VB_HIP(ctx, hipStreamSynchronize(st));       // the next chunk reuses the buffers
  }
  return VB_OK;
}
