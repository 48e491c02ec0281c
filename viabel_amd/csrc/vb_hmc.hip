// Many-chain Hamiltonian Monte Carlo on the device gradients (vb_hmc_run): C chains advanced in lock-step are
// the C-row batch model_grad_rows is built for.  Diagonal metric (inv_mass = estimated posterior variances), fixed
// trajectory length L, step size by dual averaging on the chains' mean acceptance during warm-up (Hoffman & Gelman 2014,
// Algorithm 5), one jittered step size per iteration shared by all chains.
//
// One transition (iteration t, Philox stream s = stream_offset + t), all on ctx->stream, no host synchronisation:
//   hmc_begin_kernel   one wave per chain, four chains per workgroup.  Momentum p_j = z_j / sqrt(inv_mass_j) drawn in
//                      registers (philox_normal_pair: the bits vb_noise_generate(seed, stream s) puts at (row c, col j)),
//                      H_0 = -f + 1/2 sum_j inv_mass_j p_j^2 (lane-strided fma, wave_sum), first half kick p += eps/2 g,
//                      first drift xp = x + eps inv_mass p.  The pad columns of xp and p are written as zeros.
//   model_grad_rows    fp, gp = f, grad f at xp                                   (L times)
//   hmc_leap_kernel    element-wise between two gradient calls: p += eps gp, xp += eps inv_mass p      (L - 1 times)
//   hmc_end_kernel     one wave per chain: last half kick, H_1, dH = H_0 - H_1, divergent when dH is not finite or
//                      H_1 - H_0 > 1000 (then a = 0, rejected), a = min(1, exp(dH)), accepted iff log u < dH with u the
//                      chain's uniform; an accepted chain takes xp, fp, gp, a rejected one keeps x, f, g bit for bit.  In the
//                      sampling phase: Welford mean / M2 per chain and coordinate, the accept and divergence counts, and
//                      every thin-th iteration the draw row and f.
//   hmc_adapt_kernel   one workgroup: the mean of a over the chains in a fixed order (thread i: a[i], a[i + 256], ...; shuffle
//                      tree; (w0 + w1) + (w2 + w3)), the dual-averaging update during warm-up, and the NEXT iteration's step
//                      size -- base (1 + jitter (2 v - 1)), v that iteration's uniform -- into device memory, where the
//                      three kernels above read it.  Also launched once before the first transition (t = -1) for eps_0.
// 3 + (L - 1) launches of this file per transition beside the L gradient evaluations (each a memset and the model's kernels).
// No floating-point atomics; every sum has a fixed order: two runs with the same arguments return the same bits.  A chain's
// randomness is a function of (seed, stream, chain index) only, so it does not depend on the number of chains.
//
// Uniforms: u of chain c is u01(o.x, o.y) of philox_sub(c, 0xFFFFFFFE, s, 0, k0, k1), v_t is u01(o.z, o.w) of the same call
// with row 2^64 - 1; k0 = seed_lo, k1 = seed_hi ^ s_hi (the generator's keys).
//
// Workspace: vb_ctx::hmc_work, laid out from scratch by every call -- [x | g | xp | gp | p | mean | m2 (C x ld each) |
// f | fp | H0 | a | count (C each) | inv_mass (ld) | state (8) | step_hist | accept_hist (T each) | n_div (C, int64) |
// draws (n_kept x C x d) | logp (n_kept x C)], ld = round_up(d, 16).  The draw buffer is bounded by kHmcDrawBudgetBytes.
// One process's engine only; host-callback models are refused (their "kernel" is a blocking round trip).
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; scratch 0 and no AGPRs in all):
//     hmc_begin_kernel:  71 VGPRs, 106 SGPRs, no LDS   -> 7 waves per SIMD (the Box-Muller polynomials)
//     hmc_leap_kernel:   13 VGPRs,  27 SGPRs, no LDS   -> 8 waves per SIMD
//     hmc_end_kernel:    40 VGPRs,  54 SGPRs, no LDS   -> 8 waves per SIMD
//     hmc_adapt_kernel:  36 VGPRs,  42 SGPRs, 32 B LDS -> one workgroup
// Measured (tools/hmc_bench.py, profiles/hmc_kernel_stats.txt; one MI355X, 1024 chains, 16 leapfrog steps): logistic target,
// n_data = 16 384, D = 64 -- 5.42 ms per transition, of which sixteen gradient evaluations of 337 us are 5.39; begin 5.4 us,
// leap 4.9 us (2.6 MB: 0.53 TB/s, launch-bound), end 6.4 us, adapt 4.6 us; multilevel target, D = 117 -- 1.24 ms per
// transition, leap 5.2 us (4.8 MB: 0.91 TB/s).  The numpy leapfrog around vb_model_grad takes 8.45 / 5.45 ms.
//
// ---- vb_hmc_run_metric: a dense metric, warm-up-only segments, window moments -------------------------------------------
// Dense metric (VB_HMC_METRIC_DENSE): Sigma = L L' is the inverse mass; the chain carries whitened momenta r (p = L^-T r),
// so H = -f + 1/2 sum r^2, kicks are r += c eps (g L) and drifts x += eps (r L').  One transition:
//   hmc_begin_kernel<true>   r = z (the same Philox positions, unscaled) into p, H_0, xp = x; pads written as zeros
//   kick GEMM                gemm_f64_launch<true>, A = g (C x ld), B = L (padded ld x ld copy, zero for k < j: tri_mode 3),
//                            K = ld, epilogue EpiHmcKick: r += (1/2) eps acc, eps read from state[HS_EPS]
//   L times:  drift GEMM     A = r, B = L' (padded transposed copy, zero for k > j: tri_mode 1), EpiHmcDrift: xp += eps acc
//             model_grad_rows  fp, gp at xp
//             kick GEMM      A = gp, r += eps acc (1/2 eps after the last gradient)
//   hmc_end_kernel<true>     H_1 = -fp + 1/2 sum r^2 from p directly; the rest as above
//   hmc_adapt_kernel         as above
// 3 launches of this file and 2 L + 1 products per transition beside the L gradient evaluations.  The whitened gradient of
// the current state is NOT carried across iterations: the first half kick recomputes g L from the carried g (one more
// product per transition, 1 / (2 L + 1) of them), so a rejected chain still keeps exactly x, f, g and the state per chain is
// what the diagonal kind has.  The GEMMs' N is d, so the pad columns of r and xp are never written and stay zero; their K is
// ld, over the zero pads of g / r and of the factors.  The diagonal kind enqueues what vb_hmc_run always did
// (hmc_begin_kernel<false>, hmc_leap_kernel, hmc_end_kernel<false>): the same bits.
// Window moments (moment_shift given), after every iteration's end kernel:
//   hmc_moment_kernel<DENSE> 64 columns per workgroup, the chains dealt to its four waves (wave w: chains w, w + 4, ...;
//                            (w0 + w1) + (w2 + w3)): S1 += the column sums of x - m0; diagonal kind: S2 += those of its
//                            squares; dense kind: x - m0 stored to xc
//   Gram GEMM (dense)        gemm_f64_launch<false>, A = B = xc (k-major A, K = C) split over the chains into slabs
//                            (EpiHmcSlab; about 128 chains each, at most 32, at most 256 MiB of slabs)
//   hmc_gram_add_kernel      S2[i][j] += the slabs' element (max(i, j), min(i, j)) summed in split order: exactly symmetric
// Workspace after the piece list above, still before the draws (so zeroed by the call): [L | L' (ld x ld each) |
// moment_shift | S1 (ld each) | S2 (ld, or d x d) | xc (C x ld)], and after logp the Gram slabs (splits x ld x ld).
// Capacity of the dense kind: d <= 4096 (kHmcDenseMaxDim).
// Resources of the new kernels (same command; scratch 0 and no AGPRs in all; the templates' <false> instances are the two
// kernels above, unchanged at 71 and 40 VGPRs):
//     hmc_begin_kernel<true>:   49 VGPRs, 106 SGPRs, no LDS     -> 7 waves per SIMD
//     hmc_end_kernel<true>:     40 VGPRs,  54 SGPRs, no LDS     -> 8 waves per SIMD
//     hmc_moment_kernel<D>:     18 VGPRs,  24 SGPRs, 4 KiB LDS  -> 8 waves per SIMD
//     hmc_gram_add_kernel:      13 VGPRs,  30 SGPRs, no LDS     -> 8 waves per SIMD
//     the GEMM instances the launcher picks at <= 2 tiles of 64 x 64 per CU (gemm_f64_dma_kernel<true, 2, 4, 2, .>, 64 x 32
//     tiles, two LDS stages): EpiHmcKick 59 VGPRs / 46 SGPRs, EpiHmcDrift 59 / 51; every other instance (EpiHmcSlab's
//     included) at most 249 VGPRs, scratch 0
// Measured (tools/hmc_metric_bench.py, profiles/hmc_metric_kernel_stats.txt; one MI355X, 1024 chains, 16 leapfrog steps, ms
// per transition diagonal / dense): logistic D = 64 5.33 / 5.53, the 33 products 0.25 ms (kick 8.0 us, drift 7.4 us);
// multilevel D = 117 1.25 / 1.48, products 0.28 ms; correlated Gaussian D = 1024 1.24 / 2.67, products 1.29 ms (kick 39.1 us,
// drift 38.9 us for 1024 x 1024 x 1025 multiply-adds: 27.5 TFLOP/s counting the triangle only, against 44.7 TFLOP/s of the
// same run's dense 1024^3 gradient product and the 52 TFLOP/s the triangular product reaches at 4096 rows -- 512 tiles of
// unequal k range on 256 CUs).
#include "vb_rows_target.h"
#include "vb_rng.h"

#include <cmath>

namespace vb {

constexpr int64_t kHmcDrawBudgetBytes = (int64_t)1 << 30;      // the device copy of the kept draws
constexpr uint32_t kHmcUniformCol = 0xFFFFFFFEu;               // pseudo column of the accept / jitter uniforms
constexpr double kHmcDivergence = 1000.0;                      // an energy error above this is a divergence
constexpr double kHmcGamma = 0.05, kHmcT0 = 10.0, kHmcKappa = 0.75;

// state[]: what the adapt kernel carries from one iteration to the next
enum HmcState { HS_EPS = 0, HS_HBAR, HS_LOG_EPS_BAR, HS_BASE, HS_NUM = 8 };

struct HmcArgs {
  double* x;               // C x ld: current positions (pad columns zero)
  double* g;               // C x ld: gradients there
  double* f;               // C
  double* xp;              // C x ld: proposal
  double* gp;
  double* fp;
  double* p;               // C x ld: momenta
  double* H0;              // C
  double* a;               // C: acceptance probabilities of this iteration
  double* mean;            // C x ld: Welford means of the sampling phase
  double* m2;
  double* count;           // C: accepted sampling proposals
  long long* n_div;        // C: divergent sampling proposals
  const double* inv_mass;  // ld, pad columns zero
  double* state;           // HS_NUM
  int64_t ld, n_chains;
  int d;
};

// DENSE: p holds the whitened momenta r = z, unscaled; H_0 = -f + 1/2 sum z^2; xp = x (the kick and the drift are GEMMs)
template <bool DENSE>
__global__ void __launch_bounds__(256) hmc_begin_kernel(const HmcArgs a, uint32_t k0, uint32_t k1, uint32_t w) {
  const int lane = threadIdx.x & 63;
  const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= a.n_chains) return;
  [[maybe_unused]] const double eps = a.state[HS_EPS], half = 0.5 * eps;
  const int64_t row = c * a.ld;
  double ke = 0.0;
  for (int j = lane; 2 * j < a.ld; j += 64) {
    double z[2];
    philox_normal_pair(k0, k1, (uint64_t)c, (uint32_t)j, w, &z[0], &z[1]);
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int col = 2 * j + e;
      double pj = 0.0, xj = 0.0;
      if constexpr (DENSE) {
        if (col < a.d) {
          pj = z[e];
          ke = fma(pj, pj, ke);
          xj = a.x[row + col];
        }
      } else if (col < a.d) {
        const double im = a.inv_mass[col];
        pj = z[e] / sqrt(im);
        ke = fma(im * pj, pj, ke);
        pj += half * a.g[row + col];
        xj = a.x[row + col] + eps * im * pj;
      }
      a.p[row + col] = pj;
      a.xp[row + col] = xj;
    }
  }
  ke = wave_sum(ke);
  if (lane == 0) a.H0[c] = -a.f[c] + 0.5 * ke;
}

__global__ void __launch_bounds__(256) hmc_leap_kernel(const HmcArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;      // one thread per element of the C x ld matrices
  if (i >= a.n_chains * a.ld) return;
  const int col = (int)(i % a.ld);
  if (col >= a.d) return;                                         // (pad columns stay zero)
  const double eps = a.state[HS_EPS];
  const double pj = a.p[i] + eps * a.gp[i];
  a.p[i] = pj;
  a.xp[i] += eps * a.inv_mass[col] * pj;
}

struct HmcEndArgs {
  uint32_t k0, k1, w;
  int sampling;            // 1: the sampling phase (statistics, counts)
  double k;                // sampling: 1-based index of this sampling iteration (Welford's divisor)
  double* draw_row;        // sampling, a kept iteration: C x d; else nullptr
  double* logp_row;        // ... C; else nullptr
};

// DENSE: the last half kick has been a GEMM; the kinetic energy is 1/2 sum r^2 of the whitened momenta in p
template <bool DENSE>
__global__ void __launch_bounds__(256) hmc_end_kernel(const HmcArgs a, const HmcEndArgs e) {
  const int lane = threadIdx.x & 63;
  const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= a.n_chains) return;
  [[maybe_unused]] const double half = 0.5 * a.state[HS_EPS];
  const int64_t row = c * a.ld;
  double ke = 0.0;
  for (int col = lane; col < a.d; col += 64) {
    if constexpr (DENSE) {
      const double rj = a.p[row + col];
      ke = fma(rj, rj, ke);
    } else {
      const double pj = a.p[row + col] + half * a.gp[row + col];
      ke = fma(a.inv_mass[col] * pj, pj, ke);
    }
  }
  ke = __shfl(wave_sum(ke), 0, 64);
  const double fprop = a.fp[c];
  const double h0 = a.H0[c], h1 = -fprop + 0.5 * ke;
  const double dh = h0 - h1;
  const bool divergent = !isfinite(dh) || h1 - h0 > kHmcDivergence;
  const Philox4 o = philox_sub((uint64_t)c, kHmcUniformCol, e.w, 0, e.k0, e.k1);
  const bool accept = !divergent && log(u01(o.x, o.y)) < dh;
  const double* xs = accept ? a.xp : a.x;
  for (int col = lane; col < a.d; col += 64) {
    const double xj = xs[row + col];
    if (accept) {
      a.x[row + col] = xj;
      a.g[row + col] = a.gp[row + col];
    }
    if (e.sampling) {
      const double m0 = a.mean[row + col], delta = xj - m0;
      const double m1 = m0 + delta / e.k;
      a.mean[row + col] = m1;
      a.m2[row + col] += delta * (xj - m1);
    }
    if (e.draw_row) e.draw_row[c * a.d + col] = xj;
  }
  if (lane == 0) {
    if (accept) a.f[c] = fprop;
    a.a[c] = divergent ? 0.0 : fmin(1.0, exp(dh));
    if (e.sampling) {
      if (accept) a.count[c] += 1.0;
      if (divergent) a.n_div[c] += 1;
    }
    if (e.logp_row) e.logp_row[c] = accept ? fprop : a.f[c];
  }
}

struct HmcAdaptArgs {
  const double* a;         // C
  int64_t n_chains;
  double* state;
  double* step_hist;       // T
  double* accept_hist;     // T
  int64_t t, n_warmup, n_iter;     // t = -1: before the first transition
  double step_size, target, jitter, mu;
  uint32_t k0, k1_next, w_next;    // keys / stream of iteration t + 1
};

__global__ void __launch_bounds__(256) hmc_adapt_kernel(const HmcAdaptArgs q) {
  __shared__ double sh[4];
  const int t = threadIdx.x;
  double s = 0.0;
  if (q.t >= 0)
    for (int64_t c = t; c < q.n_chains; c += 256) s += q.a[c];
  s = wave_sum(s);
  if ((t & 63) == 0) sh[t >> 6] = s;
  __syncthreads();
  if (t != 0) return;
  double base = q.step_size;
  if (q.t >= 0) {
    const double abar = ((sh[0] + sh[1]) + (sh[2] + sh[3])) / (double)q.n_chains;
    q.accept_hist[q.t] = abar;
    base = q.state[HS_BASE];
    if (q.t < q.n_warmup) {
      const double m = (double)(q.t + 1), w = 1.0 / (m + kHmcT0);
      const double hbar = (1.0 - w) * q.state[HS_HBAR] + (q.target - abar) * w;
      const double log_eps = q.mu - sqrt(m) / kHmcGamma * hbar;
      const double eta = pow(m, -kHmcKappa);
      const double log_eps_bar = eta * log_eps + (1.0 - eta) * q.state[HS_LOG_EPS_BAR];
      q.state[HS_HBAR] = hbar;
      q.state[HS_LOG_EPS_BAR] = log_eps_bar;
      base = q.t + 1 < q.n_warmup ? exp(log_eps) : exp(log_eps_bar);
    }
  } else {
    q.state[HS_HBAR] = 0.0;
    q.state[HS_LOG_EPS_BAR] = 0.0;
  }
  q.state[HS_BASE] = base;
  if (q.t + 1 < q.n_iter) {
    const Philox4 o = philox_sub(~(uint64_t)0, kHmcUniformCol, q.w_next, 0, q.k0, q.k1_next);
    const double eps = base * (1.0 + q.jitter * (2.0 * u01(o.z, o.w) - 1.0));
    q.state[HS_EPS] = eps;
    q.step_hist[q.t + 1] = eps;
  }
}

// ---- dense metric: the two triangular products' epilogues (the step size is read from the device-resident state) ----------
struct EpiHmcKick {          // r += c eps acc, acc = (g L)[row][col]; c = 1, or 1/2 for a half kick
  double* r;
  int64_t ld;
  const double* state;
  double c;
  __device__ void operator()(int, int row, int col, double acc) const {
    const int64_t e = (int64_t)row * ld + col;
    r[e] += c * state[HS_EPS] * acc;
  }
};
struct EpiHmcDrift {         // xp += eps acc, acc = (r L')[row][col]
  double* xp;
  int64_t ld;
  const double* state;
  __device__ void operator()(int, int row, int col, double acc) const {
    const int64_t e = (int64_t)row * ld + col;
    xp[e] += state[HS_EPS] * acc;
  }
};
struct EpiHmcSlab {          // split z's part of the Gram product (X - m0)' (X - m0), d x d with row stride ld
  double* slab;
  int64_t stride, ld;
  __device__ void operator()(int split, int row, int col, double acc) const {
    slab[(int64_t)split * stride + (int64_t)row * ld + col] = acc;
  }
};

// ---- window moments --------------------------------------------------------------------------------------------------------
struct HmcMomentArgs {
  const double* x;         // C x ld: the states after this iteration's accept step
  const double* shift;     // d: m0
  double* s1;              // d: running sum of x - m0
  double* s2;              // diagonal kind: d, running sum of (x - m0)^2; dense kind: d x d (row stride d)
  double* xc;              // dense kind: C x ld, x - m0 (pad columns stay zero: never written)
  double* slab;            // dense kind: splits x slab_stride
  int64_t slab_stride, ld, n_chains;
  int d, splits;
};

// 64 columns per workgroup, the chains dealt to its four waves (wave w: chains w, w + 4, ...; then (w0 + w1) + (w2 + w3)):
// this iteration's column sums of x - m0 (and, diagonal kind, of its squares) added to the running sums; the dense kind
// stores x - m0 for the Gram product instead
template <bool DENSE>
__global__ void __launch_bounds__(256) hmc_moment_kernel(const HmcMomentArgs q) {
  __shared__ double sh[2][4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + lane;
  double s = 0.0, ss = 0.0;
  if (col < q.d) {
    const double m0 = q.shift[col];
    for (int64_t c = w; c < q.n_chains; c += 4) {
      const double v = q.x[c * q.ld + col] - m0;
      s += v;
      if constexpr (DENSE) q.xc[c * q.ld + col] = v;
      else ss = fma(v, v, ss);
    }
  }
  sh[0][w][lane] = s;
  sh[1][w][lane] = ss;
  __syncthreads();
  if (w != 0 || col >= q.d) return;
  q.s1[col] += (sh[0][0][lane] + sh[0][1][lane]) + (sh[0][2][lane] + sh[0][3][lane]);
  if constexpr (!DENSE) q.s2[col] += (sh[1][0][lane] + sh[1][1][lane]) + (sh[1][2][lane] + sh[1][3][lane]);
}

// S2[i][j] += the slabs' sum, in split order, of the Gram product's element (max(i, j), min(i, j)): the lower triangle
// serves both halves, so S2 is symmetric bit for bit
__global__ void __launch_bounds__(256) hmc_gram_add_kernel(const HmcMomentArgs q) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)q.d * q.d) return;
  const int64_t i = e / q.d, j = e - i * q.d;
  const int64_t src = (i > j ? i : j) * q.ld + (i > j ? j : i);
  double acc = q.slab[src];
  for (int z = 1; z < q.splits; ++z) acc += q.slab[(int64_t)z * q.slab_stride + src];
  q.s2[e] += acc;
}

constexpr int kHmcDenseMaxDim = 4096;                           // dense metric: two padded d x d factors on the device
constexpr int kHmcMaxSplits = 32;
constexpr int64_t kHmcSlabBudgetDoubles = (int64_t)1 << 25;     // 256 MiB of Gram slabs

// pieces of the chain axis for the Gram product: about 128 chains each, every piece a non-empty whole number of k slabs
int hmc_gram_splits(int64_t n_chains, int64_t ld) {
  int64_t s = n_chains / 128, cap = kHmcSlabBudgetDoubles / (ld * ld);
  cap = cap > kHmcMaxSplits ? kHmcMaxSplits : cap;
  s = s > cap ? cap : s;
  s = s < 1 ? 1 : s;
  const int64_t ks = round_up((n_chains + s - 1) / s, kGemmBK);
  return (int)((n_chains + ks - 1) / ks);
}

struct HmcCall {
  const char* name;        // the entry, for the messages
  int kind;                // VB_HMC_METRIC_*
  const double* metric;    // inv_mass[d], or the lower factor L (d x d)
  const double* moment_shift;
  double* moment_sum;
  double* moment_m2;
};

// vb_hmc_run and vb_hmc_run_metric: the diagonal kind without moments enqueues exactly what vb_hmc_run always did
int hmc_run(vb_ctx* ctx, const HmcCall& hc, const double* x0, int64_t n_chains, int64_t d, int64_t n_warmup, int64_t n_draws,
            int64_t thin, int n_leapfrog, double step_size, double target_accept, double jitter, uint64_t seed,
            uint64_t stream_offset, double* draws, double* logp, double* last_x, double* chain_mean, double* chain_m2,
            double* accept_rate, double* step_hist, double* accept_hist, double* final_step, int64_t* n_divergent) {
  const bool dense = hc.kind == VB_HMC_METRIC_DENSE, moments = hc.moment_shift != nullptr;
  if (thin < 1) return fail(ctx, VB_ERR_INVALID, "thin must be at least 1");
  if (n_leapfrog < 1) return fail(ctx, VB_ERR_INVALID, "n_leapfrog must be at least 1");
  if (!(step_size > 0.0) || !std::isfinite(step_size)) return fail(ctx, VB_ERR_INVALID, "step_size must be positive and finite");
  if (!(target_accept > 0.0 && target_accept < 1.0)) return fail(ctx, VB_ERR_INVALID, "target_accept must lie in (0, 1)");
  if (!(jitter >= 0.0 && jitter < 1.0)) return fail(ctx, VB_ERR_INVALID, "jitter must lie in [0, 1)");
  const ModelDev& m = ctx->model;
  if (m.id < 0) return fail(ctx, VB_ERR_STATE, "no model bound (vb_set_model)");
  if (d != m.dim) return fail(ctx, VB_ERR_INVALID, "x0 has %lld columns, model dimension is %d", (long long)d, m.dim);
  if (dense && d > kHmcDenseMaxDim)
    return fail(ctx, VB_ERR_UNSUPPORTED, "the dense metric takes at most %d dimensions (got %lld)", kHmcDenseMaxDim, (long long)d);
  if (!dense) {
    for (int64_t j = 0; j < d; ++j)
      if (!(hc.metric[j] > 0.0) || !std::isfinite(hc.metric[j]))
        return fail(ctx, VB_ERR_INVALID, "inv_mass[%lld] must be positive and finite", (long long)j);
  } else {
    for (int64_t i = 0; i < d; ++i) {
      if (!(hc.metric[i * d + i] > 0.0) || !std::isfinite(hc.metric[i * d + i]))
        return fail(ctx, VB_ERR_INVALID, "L[%lld][%lld] must be positive and finite", (long long)i, (long long)i);
      for (int64_t j = 0; j < i; ++j)
        if (!std::isfinite(hc.metric[i * d + j]))
          return fail(ctx, VB_ERR_INVALID, "L[%lld][%lld] must be finite", (long long)i, (long long)j);
    }
  }
  if (m.id == VB_MODEL_SOURCE && ctx->user_host_fn)
    return fail(ctx, VB_ERR_UNSUPPORTED, "%s runs without host synchronisation: a host-callback model cannot be its "
                                         "target (write the density as a source model)", hc.name);
  if (ctx->comm) return fail(ctx, VB_ERR_UNSUPPORTED, "%s runs on one process's engine: detach the communicator", hc.name);
  const int64_t n_iter = n_warmup + n_draws, n_kept = (n_draws + thin - 1) / thin;
  if (n_chains > ((int64_t)1 << 31) - 8 || n_iter > ((int64_t)1 << 40) || (double)n_chains * (double)round_up(d, 16) > 0x1p36)
    return fail(ctx, VB_ERR_UNSUPPORTED, "%s takes at most 2^31 - 8 chains, 2^36 chain coordinates (n_chains x "
                                         "round_up(d, 16)) and 2^40 iterations", hc.name);
  if (draws && (double)n_kept * (double)n_chains * (double)d * sizeof(double) > (double)kHmcDrawBudgetBytes)
    return fail(ctx, VB_ERR_UNSUPPORTED, "the kept draws (%lld x %lld x %lld doubles) exceed the device draw buffer's budget of "
                                         "%lld bytes: raise thin or pass no draws",
                (long long)n_kept, (long long)n_chains, (long long)d, (long long)kHmcDrawBudgetBytes);
  VB_HIP(ctx, hipSetDevice(ctx->device));
  VB_TRY(main_stream_write(ctx));
  hipStream_t st = ctx->stream;
  const int n_cu = ctx->prop.multiProcessorCount;
  const int64_t C = n_chains, ld = round_up(d, 16), mat = C * ld;
  const int splits = dense && moments ? hmc_gram_splits(C, ld) : 0;
  const int64_t slab_stride = ld * ld;
  Carver carve;
  const int64_t o_x = carve(mat), o_g = carve(mat), o_xp = carve(mat), o_gp = carve(mat), o_p = carve(mat),
                o_mean = carve(mat), o_m2 = carve(mat), o_f = carve(C), o_fp = carve(C), o_h0 = carve(C), o_a = carve(C),
                o_cnt = carve(C), o_im = carve(ld), o_state = carve(HS_NUM), o_sh = carve(n_iter), o_ah = carve(n_iter),
                o_div = carve(C), o_l = carve(dense ? ld * ld : 0), o_lt = carve(dense ? ld * ld : 0),
                o_shift = carve(moments ? ld : 0), o_s1 = carve(moments ? ld : 0),
                o_s2 = carve(moments ? (dense ? d * d : ld) : 0), o_xc = carve(splits ? mat : 0),
                o_draws = carve(draws ? n_kept * C * d : 0), o_logp = carve(logp ? n_kept * C : 0),
                o_slab = carve((int64_t)splits * slab_stride);
  VB_TRY(ensure(ctx, ctx->hmc_work, (size_t)carve.off * sizeof(double)));
  double* base = (double*)ctx->hmc_work.ptr;
  // everything up to the draws starts from zero: pad columns, Welford sums, counts, state, the factors' pads, the moments
  VB_HIP(ctx, hipMemsetAsync(base, 0, (size_t)o_draws * sizeof(double), st));
  VB_HIP(ctx, hipMemcpy2DAsync(base + o_x, (size_t)ld * sizeof(double), x0, (size_t)d * sizeof(double),
                               (size_t)d * sizeof(double), (size_t)C, hipMemcpyHostToDevice, st));
  std::vector<double> pack;      // (lives until the synchronisation at the end)
  if (!dense) {
    VB_HIP(ctx, hipMemcpyAsync(base + o_im, hc.metric, (size_t)d * sizeof(double), hipMemcpyHostToDevice, st));
  } else {                       // [L | L'], each ld x ld with zeros above / below the diagonal and in the pads
    pack.assign((size_t)(2 * ld * ld), 0.0);
    for (int64_t i = 0; i < d; ++i)
      for (int64_t j = 0; j <= i; ++j) {
        const double v = hc.metric[i * d + j];
        pack[(size_t)(i * ld + j)] = v;
        pack[(size_t)(ld * ld + j * ld + i)] = v;
      }
    VB_HIP(ctx, hipMemcpyAsync(base + o_l, pack.data(), (size_t)(ld * ld) * sizeof(double), hipMemcpyHostToDevice, st));
    VB_HIP(ctx, hipMemcpyAsync(base + o_lt, pack.data() + ld * ld, (size_t)(ld * ld) * sizeof(double), hipMemcpyHostToDevice, st));
  }
  if (moments)
    VB_HIP(ctx, hipMemcpyAsync(base + o_shift, hc.moment_shift, (size_t)d * sizeof(double), hipMemcpyHostToDevice, st));
  HmcArgs a;
  a.x = base + o_x, a.g = base + o_g, a.f = base + o_f, a.xp = base + o_xp, a.gp = base + o_gp, a.fp = base + o_fp;
  a.p = base + o_p, a.H0 = base + o_h0, a.a = base + o_a, a.mean = base + o_mean, a.m2 = base + o_m2;
  a.count = base + o_cnt, a.n_div = (long long*)(base + o_div), a.inv_mass = base + o_im, a.state = base + o_state;
  a.ld = ld, a.n_chains = C, a.d = (int)d;
  VB_TRY(model_grad_rows(ctx, a.x, ld, C, d, a.g, a.f));      // f, g of the start: carried from here on
  HmcMomentArgs mq;
  mq.x = a.x, mq.shift = base + o_shift, mq.s1 = base + o_s1, mq.s2 = base + o_s2, mq.xc = base + o_xc;
  mq.slab = base + o_slab, mq.slab_stride = slab_stride, mq.ld = ld, mq.n_chains = C, mq.d = (int)d, mq.splits = splits;
  // the products of the dense kind: K runs over the padded ld columns (zeros in the states' pads and the factors' pads)
  auto kick = [&](const double* grad, double c) {      // r += c eps (grad L): B = L, zero for k < j
    gemm_f64_launch<true>(st, gemm_product(grad, ld, base + o_l, ld, (int)C, (int)d, (int)ld, 3), 1, n_cu,
                          EpiHmcKick{a.p, ld, a.state, c});
    return hipGetLastError();
  };
  auto drift = [&]() {                                 // xp += eps (r L'): B = L', zero for k > j
    gemm_f64_launch<true>(st, gemm_product(a.p, ld, base + o_lt, ld, (int)C, (int)d, (int)ld, 1), 1, n_cu,
                          EpiHmcDrift{a.xp, ld, a.state});
    return hipGetLastError();
  };

  const uint32_t k0 = (uint32_t)seed, seed_hi = (uint32_t)(seed >> 32);
  HmcAdaptArgs q;
  q.a = a.a, q.n_chains = C, q.state = a.state, q.step_hist = base + o_sh, q.accept_hist = base + o_ah;
  q.n_warmup = n_warmup, q.n_iter = n_iter, q.step_size = step_size, q.target = target_accept, q.jitter = jitter;
  q.mu = log(10.0 * step_size), q.k0 = k0;
  const dim3 chain_grid((unsigned)((C + 3) / 4)), leap_grid((unsigned)((mat + 255) / 256)), block(256);
  for (int64_t t = -1; t < n_iter; ++t) {
    if (t >= 0) {
      const uint64_t s = stream_offset + (uint64_t)t;
      const uint32_t k1 = seed_hi ^ (uint32_t)(s >> 32), w = (uint32_t)s;
      if (dense) {
        hipLaunchKernelGGL(hmc_begin_kernel<true>, chain_grid, block, 0, st, a, k0, k1, w);
        VB_HIP(ctx, hipGetLastError());
        VB_HIP(ctx, kick(a.g, 0.5));
        for (int l = 0; l < n_leapfrog; ++l) {
          VB_HIP(ctx, drift());
          VB_TRY(model_grad_rows(ctx, a.xp, ld, C, d, a.gp, a.fp));
          VB_HIP(ctx, kick(a.gp, l + 1 == n_leapfrog ? 0.5 : 1.0));
        }
      } else {
        hipLaunchKernelGGL(hmc_begin_kernel<false>, chain_grid, block, 0, st, a, k0, k1, w);
        VB_HIP(ctx, hipGetLastError());
        for (int l = 0; l < n_leapfrog; ++l) {
          VB_TRY(model_grad_rows(ctx, a.xp, ld, C, d, a.gp, a.fp));
          if (l + 1 == n_leapfrog) break;
          hipLaunchKernelGGL(hmc_leap_kernel, leap_grid, block, 0, st, a);
          VB_HIP(ctx, hipGetLastError());
        }
      }
      HmcEndArgs e;
      e.k0 = k0, e.k1 = k1, e.w = w;
      const int64_t si = t - n_warmup;
      e.sampling = si >= 0, e.k = (double)(si + 1);
      const bool keep = si >= 0 && si % thin == 0;
      e.draw_row = keep && draws ? base + o_draws + (si / thin) * C * d : nullptr;
      e.logp_row = keep && logp ? base + o_logp + (si / thin) * C : nullptr;
      if (dense) hipLaunchKernelGGL(hmc_end_kernel<true>, chain_grid, block, 0, st, a, e);
      else hipLaunchKernelGGL(hmc_end_kernel<false>, chain_grid, block, 0, st, a, e);
      VB_HIP(ctx, hipGetLastError());
      if (moments) {
        const dim3 col_grid((unsigned)((d + 63) / 64));
        if (dense) {
          hipLaunchKernelGGL(hmc_moment_kernel<true>, col_grid, block, 0, st, mq);
          VB_HIP(ctx, hipGetLastError());
          gemm_f64_launch<false>(st, gemm_product(mq.xc, ld, mq.xc, ld, (int)d, (int)d, (int)C, 0), splits, n_cu,
                                 EpiHmcSlab{mq.slab, slab_stride, ld});
          VB_HIP(ctx, hipGetLastError());
          hipLaunchKernelGGL(hmc_gram_add_kernel, dim3((unsigned)((d * d + 255) / 256)), block, 0, st, mq);
        } else {
          hipLaunchKernelGGL(hmc_moment_kernel<false>, col_grid, block, 0, st, mq);
        }
        VB_HIP(ctx, hipGetLastError());
      }
    }
    const uint64_t sn = stream_offset + (uint64_t)(t + 1);
    q.t = t, q.k1_next = seed_hi ^ (uint32_t)(sn >> 32), q.w_next = (uint32_t)sn;
    hipLaunchKernelGGL(hmc_adapt_kernel, dim3(1), block, 0, st, q);
    VB_HIP(ctx, hipGetLastError());
  }

  // the one synchronisation: download
  const size_t row_bytes = (size_t)d * sizeof(double), ld_bytes = (size_t)ld * sizeof(double);
  VB_HIP(ctx, hipMemcpy2DAsync(last_x, row_bytes, a.x, ld_bytes, row_bytes, (size_t)C, hipMemcpyDeviceToHost, st));
  if (chain_mean)
    VB_HIP(ctx, hipMemcpy2DAsync(chain_mean, row_bytes, a.mean, ld_bytes, row_bytes, (size_t)C, hipMemcpyDeviceToHost, st));
  if (chain_m2)
    VB_HIP(ctx, hipMemcpy2DAsync(chain_m2, row_bytes, a.m2, ld_bytes, row_bytes, (size_t)C, hipMemcpyDeviceToHost, st));
  if (accept_rate) VB_HIP(ctx, hipMemcpyAsync(accept_rate, a.count, (size_t)C * sizeof(double), hipMemcpyDeviceToHost, st));
  VB_HIP(ctx, hipMemcpyAsync(step_hist, base + o_sh, (size_t)n_iter * sizeof(double), hipMemcpyDeviceToHost, st));
  VB_HIP(ctx, hipMemcpyAsync(accept_hist, base + o_ah, (size_t)n_iter * sizeof(double), hipMemcpyDeviceToHost, st));
  VB_HIP(ctx, hipMemcpyAsync(final_step, a.state + HS_BASE, sizeof(double), hipMemcpyDeviceToHost, st));
  if (draws && n_kept)
    VB_HIP(ctx, hipMemcpyAsync(draws, base + o_draws, (size_t)(n_kept * C * d) * sizeof(double), hipMemcpyDeviceToHost, st));
  if (logp && n_kept)
    VB_HIP(ctx, hipMemcpyAsync(logp, base + o_logp, (size_t)(n_kept * C) * sizeof(double), hipMemcpyDeviceToHost, st));
  if (moments) {
    VB_HIP(ctx, hipMemcpyAsync(hc.moment_sum, mq.s1, (size_t)d * sizeof(double), hipMemcpyDeviceToHost, st));
    VB_HIP(ctx, hipMemcpyAsync(hc.moment_m2, mq.s2, (size_t)(dense ? d * d : d) * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  std::vector<long long> div((size_t)C);
  VB_HIP(ctx, hipMemcpyAsync(div.data(), a.n_div, (size_t)C * sizeof(long long), hipMemcpyDeviceToHost, st));
  VB_HIP(ctx, hipStreamSynchronize(st));
  int64_t total = 0;
  for (int64_t c = 0; c < C; ++c) {
    total += div[(size_t)c];
    if (accept_rate && n_draws > 0) accept_rate[c] /= (double)n_draws;
  }
  if (n_divergent) *n_divergent = total;
  return VB_OK;
}

}  // namespace vb

using namespace vb;

extern "C" {

int vb_hmc_run(vb_ctx* ctx, const double* x0, const double* inv_mass, int64_t n_chains, int64_t d, int64_t n_warmup,
               int64_t n_draws, int64_t thin, int n_leapfrog, double step_size, double target_accept, double jitter,
               uint64_t seed, uint64_t stream_offset, double* draws, double* logp, double* last_x, double* chain_mean,
               double* chain_m2, double* accept_rate, double* step_hist, double* accept_hist, double* final_step,
               int64_t* n_divergent) {
  if (!ctx || !x0 || !inv_mass || !last_x || !chain_mean || !chain_m2 || !accept_rate || !step_hist || !accept_hist ||
      !final_step || !n_divergent)
    return fail(ctx, VB_ERR_INVALID, "NULL argument");
  if (n_chains <= 0 || d <= 0 || n_draws <= 0 || n_warmup < 0)
    return fail(ctx, VB_ERR_INVALID, "n_chains, d and n_draws must be positive and n_warmup non-negative");
  const HmcCall hc{"vb_hmc_run", VB_HMC_METRIC_DIAG, inv_mass, nullptr, nullptr, nullptr};
  return hmc_run(ctx, hc, x0, n_chains, d, n_warmup, n_draws, thin, n_leapfrog, step_size, target_accept, jitter, seed,
                 stream_offset, draws, logp, last_x, chain_mean, chain_m2, accept_rate, step_hist, accept_hist, final_step,
                 n_divergent);
}

int vb_hmc_run_metric(vb_ctx* ctx, const double* x0, int metric_kind, const double* metric, int64_t n_chains, int64_t d,
                      int64_t n_warmup, int64_t n_draws, int64_t thin, int n_leapfrog, double step_size, double target_accept,
                      double jitter, uint64_t seed, uint64_t stream_offset, const double* moment_shift, double* moment_sum,
                      double* moment_m2, double* draws, double* logp, double* last_x, double* chain_mean, double* chain_m2,
                      double* accept_rate, double* step_hist, double* accept_hist, double* final_step, int64_t* n_divergent) {
  if (!ctx || !x0 || !metric || !last_x || !step_hist || !accept_hist || !final_step)
    return fail(ctx, VB_ERR_INVALID, "NULL argument");
  if (metric_kind != VB_HMC_METRIC_DIAG && metric_kind != VB_HMC_METRIC_DENSE)
    return fail(ctx, VB_ERR_INVALID, "metric_kind must be VB_HMC_METRIC_DIAG or VB_HMC_METRIC_DENSE");
  if (n_chains <= 0 || d <= 0 || n_draws < 0 || n_warmup < 0 || n_warmup + n_draws < 1)
    return fail(ctx, VB_ERR_INVALID, "n_chains and d must be positive, n_warmup and n_draws non-negative with at least one "
                                     "iteration between them");
  if (n_draws > 0 && (!chain_mean || !chain_m2 || !accept_rate || !n_divergent))
    return fail(ctx, VB_ERR_INVALID, "NULL sampling output with n_draws > 0");
  const int given = (moment_shift != nullptr) + (moment_sum != nullptr) + (moment_m2 != nullptr);
  if (given != 0 && given != 3)
    return fail(ctx, VB_ERR_INVALID, "moment_shift, moment_sum and moment_m2 go together: pass all three or none");
  const HmcCall hc{"vb_hmc_run_metric", metric_kind, metric, moment_shift, moment_sum, moment_m2};
  return hmc_run(ctx, hc, x0, n_chains, d, n_warmup, n_draws, thin, n_leapfrog, step_size, target_accept, jitter, seed,
                 stream_offset, draws, logp, last_x, chain_mean, chain_m2, accept_rate, step_hist, accept_hist, final_step,
                 n_divergent);
}

}  // extern "C"

