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
//
// ---- vb_hmc_run_chees: the trajectory length adapted across the chains (ChEES-HMC) ---------------------------
// One length T for all chains; iteration t takes L_t = clamp(ceil(h_s T_t / eps_t), 1, max_leapfrog) steps, h_s the base-2
// radical inverse of low32(s + 1); warm-up adapts log T by Adam (no first moment) on the cross-chain criterion.  The fixed
// route's kernels and launches are untouched.  A warm-up transition adds, between the last gradient and the end kernel:
//   velocity GEMM (dense)       A = r, B = L' (the drift's operands), EpiHmcVelocity: v' = acc stored to a C x ld buffer of
//                               the zeroed region (N = d: the pads are never written)
//   hmc_chees_mean_kernel       hmc_moment_kernel's layout and order (64 columns per workgroup, wave w: chains w, w + 4, ...;
//                               (w0 + w1) + (w2 + w3)): column sums of x over all chains and of xp over the usable ones
//                               (finite fp), and the usable count; sixteen chains' loads in flight per wave
//   hmc_chees_chain_kernel<D>   one wave per chain: |xp - mean xp|^2, |x - mean x|^2 and (xp - mean xp) . v' by lane-strided
//                               fma and wave_sum; crit[c] = their product form, 0 and flag[c] = 1 for an unusable chain
// and every transition runs, in place of hmc_adapt_kernel,
//   hmc_chees_adapt_kernel      one workgroup: the mean of a and (warm-up) sum a_c, sum a_c crit_c over the unflagged chains,
//                               all in the a-mean's order (thread i: i, i + 256, ...; shuffle tree; (w0 + w1) + (w2 + w3));
//                               dual averaging as above; the Adam step, the clamp to [log base, log(max_leapfrog base)], the
//                               m^-0.75 average; while the next iteration is a warm-up one its eps, T and L into the state
//                               (slots 4 .. 7: log T, v, log T_bar, L_next) and the histories; in the sampling phase it
//                               moves the planned eps of the next iteration from step_hist into the state
//   hmc_chees_plan_kernel       once, when the warm-up has ended: eps_t, T_t = exp(log T_bar), L_t of every sampling iteration
// The host reads L_{t+1} back (8 bytes, fetch_blocking) after every warm-up iteration but the last, and all sampling step
// counts at once after the plan kernel: the sampling phase synchronises only for the download, as above.
// Workspace, in the zeroed region before the draws: [colsum (2 ld) | n_usable | crit (C) | flag (C, int) | v' (C x ld, dense
// with a warm-up) | traj_hist | leap_hist (n_iter each)].
// Resources (same command; scratch 0 and no AGPRs in all; hmc_adapt_kernel and the other kernels above unchanged):
//     hmc_chees_mean_kernel:        112 VGPRs, 106 SGPRs, 4128 B LDS -> 4 waves per SIMD (one workgroup per 64 columns)
//     hmc_chees_chain_kernel<false>: 52 VGPRs,  36 SGPRs, no LDS     -> 8 waves per SIMD
//     hmc_chees_chain_kernel<true>:  46 VGPRs,  32 SGPRs, no LDS     -> 8 waves per SIMD
//     hmc_chees_adapt_kernel:        49 VGPRs,  64 SGPRs, 96 B LDS   -> one workgroup
//     hmc_chees_plan_kernel:         18 VGPRs,  26 SGPRs, no LDS     -> 8 waves per SIMD
//     EpiHmcVelocity's GEMM instances: 59 VGPRs for the 64 x 32 tile the launcher picks here, at most 249, scratch 0
// Measured (tools/hmc_chees_bench.py, profiles/hmc_chees_kernel_stats.txt; one MI355X, 1024 chains): a sampling transition of
// 16.1 steps on average 5.48 ms against 5.44 for n_leapfrog = 16 at the logistic shape (0.3405 / 0.3397 ms per step),
// 1.253 / 1.243 at the multilevel one; a warm-up transition 0.05 - 0.08 ms beyond its own steps; mean kernel 51.4 us at
// D = 64 (one workgroup) and 37.4 us at D = 117 (213 us with one load in flight), chain kernel 4.9 us, velocity product
// 6.0 / 7.4 us, adapt 6.3 us, plan 4.8 us.  Smallest ESS per gradient evaluation against n_leapfrog = 16: 2.5, 2.2 and 1.8
// times at the logistic, multilevel and correlated-logistic shapes; at the logistic shape n_leapfrog = 4 beats it five times.
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

// ---- ChEES: the trajectory length adapted across the chains (vb_hmc_run_chees) --------------------------------
constexpr double kCheesBeta2 = 0.95, kCheesAdamEps = 1e-8;
enum HmcCheesState { HS_LOG_T = 4, HS_V, HS_LOG_TBAR, HS_LNEXT };      // the four slots of state[] the fixed route leaves free

struct HmcCheesBuf {
  double* colsum;          // 2 ld: column sums of x over all chains | of xp over the usable chains
  double* n_usable;        // 1: chains whose proposal has a finite log density
  double* crit;            // C: the criterion's per-chain factor product (0 for an unusable chain)
  int* flag;               // C: 1 for an unusable chain
  const double* vel;       // dense kind: C x ld, v' = r L' (pad columns zero); else nullptr
};

// h_s of the iteration whose stream has low32(s + 1) = n: the base-2 radical inverse, in (0, 1), exact in fp64
__device__ __forceinline__ double chees_halton(uint32_t n) { return ((double)__brev(n) + 0.5) * 0x1p-32; }

// L = clamp(ceil(tau / eps), 1, max_leapfrog); a NaN quotient gives 1
__device__ __forceinline__ long long chees_steps(double tau, double eps, int max_leapfrog) {
  const double r = ceil(tau / eps);
  return r >= (double)max_leapfrog ? (long long)max_leapfrog : (r >= 1.0 ? (long long)r : 1ll);
}

// 64 columns per workgroup, the chains dealt to its four waves (wave w: chains w, w + 4, ...; then (w0 + w1) + (w2 + w3)):
// the column sums of x over all chains and of xp over the usable ones; workgroup 0 also stores the usable count
__global__ void __launch_bounds__(256) hmc_chees_mean_kernel(const HmcArgs a, const HmcCheesBuf b) {
  __shared__ double sh[2][4][64];
  __shared__ double cnt[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + lane;
  double s = 0.0, sp = 0.0, n = 0.0;
  // kMeanAhead chains' loads in flight per wave (one at a time, the loop is a chain of memory latencies: 213 us at 1024
  // chains), added in chain order.  The loads are unconditional, at indices clamped into the matrices, and selected
  // afterwards: a chain that is left out, or beyond the last one, adds +0.0, which changes no bit
  constexpr int kMeanAhead = 16;
  const int lc = col < a.d ? col : a.d - 1;
  for (int64_t c0 = w; c0 < a.n_chains; c0 += 4 * kMeanAhead) {
    double xv[kMeanAhead], pv[kMeanAhead], uv[kMeanAhead];
#pragma unroll
    for (int u = 0; u < kMeanAhead; ++u) {
      const int64_t c = c0 + 4 * u, cc = c < a.n_chains ? c : a.n_chains - 1;
      xv[u] = a.x[cc * a.ld + lc], pv[u] = a.xp[cc * a.ld + lc], uv[u] = a.fp[cc];
    }
#pragma unroll
    for (int u = 0; u < kMeanAhead; ++u) {
      const bool in = c0 + 4 * u < a.n_chains, usable = in && isfinite(uv[u]);
      xv[u] = in && col < a.d ? xv[u] : 0.0, pv[u] = usable && col < a.d ? pv[u] : 0.0, uv[u] = usable ? 1.0 : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kMeanAhead; ++u) s += xv[u], sp += pv[u], n += uv[u];
  }
  sh[0][w][lane] = s;
  sh[1][w][lane] = sp;
  if (lane == 0) cnt[w] = n;
  __syncthreads();
  if (w != 0) return;
  if (col < a.d) {
    b.colsum[col] = (sh[0][0][lane] + sh[0][1][lane]) + (sh[0][2][lane] + sh[0][3][lane]);
    b.colsum[a.ld + col] = (sh[1][0][lane] + sh[1][1][lane]) + (sh[1][2][lane] + sh[1][3][lane]);
  }
  if (blockIdx.x == 0 && lane == 0) b.n_usable[0] = (cnt[0] + cnt[1]) + (cnt[2] + cnt[3]);
}

// one wave per chain, four chains per workgroup: crit_c = (|x' - mean x'|^2 - |x - mean x|^2) ((x' - mean x') . v'), the three
// sums lane-strided fma and wave_sum; v' = inv_mass (p + 1/2 eps gp) (the end kernel's last half kick), or the row of r L'
template <bool DENSE>
__global__ void __launch_bounds__(256) hmc_chees_chain_kernel(const HmcArgs a, const HmcCheesBuf b) {
  const int lane = threadIdx.x & 63;
  const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= a.n_chains) return;
  [[maybe_unused]] const double half = 0.5 * a.state[HS_EPS];
  const double n_all = (double)a.n_chains, n_usable = b.n_usable[0];
  const int64_t row = c * a.ld;
  double n0 = 0.0, n1 = 0.0, dot = 0.0;
  for (int col = lane; col < a.d; col += 64) {
    const double dx = a.x[row + col] - b.colsum[col] / n_all;
    const double dxp = a.xp[row + col] - b.colsum[a.ld + col] / n_usable;
    double vel;
    if constexpr (DENSE) vel = b.vel[row + col];
    else vel = a.inv_mass[col] * (a.p[row + col] + half * a.gp[row + col]);
    n0 = fma(dx, dx, n0);
    n1 = fma(dxp, dxp, n1);
    dot = fma(dxp, vel, dot);
  }
  n0 = wave_sum(n0), n1 = wave_sum(n1), dot = wave_sum(dot);
  if (lane != 0) return;
  const bool usable = isfinite(a.fp[c]);
  b.crit[c] = usable ? (n1 - n0) * dot : 0.0;
  b.flag[c] = usable ? 0 : 1;
}

struct EpiHmcVelocity {      // v' = acc, acc = (r L')[row][col]: the velocity at the proposal (dense kind)
  double* v;
  int64_t ld;
  __device__ void operator()(int, int row, int col, double acc) const { v[(int64_t)row * ld + col] = acc; }
};

struct HmcCheesAdaptArgs {
  const double* crit;      // C
  const int* flag;         // C
  double* traj_hist;       // T: the trajectory length T_t of every iteration
  long long* leap_hist;    // T: its number of leapfrog steps
  double log_t0, v0, log_tbar0, m0;      // t = -1: the state the call starts from
  double lr;
  int max_leapfrog;
};

// hmc_adapt_kernel's sibling for the ChEES route, launched in its place: the same mean of a and dual-averaging update, then
// (warm-up) the two weighted sums over the usable chains in the a-mean's order, the Adam step on log T, its clamp and its
// running average, and -- while the next iteration is a warm-up one -- that iteration's eps, T and L.  The sampling
// iterations' eps, T and L come from hmc_chees_plan_kernel; there this kernel only moves the planned eps into the state.
__global__ void __launch_bounds__(256) hmc_chees_adapt_kernel(const HmcAdaptArgs q, const HmcCheesAdaptArgs z) {
  __shared__ double sh[3][4];
  const int t = threadIdx.x;
  const bool warm = q.t >= 0 && q.t < q.n_warmup;
  double s = 0.0, sa = 0.0, sc = 0.0;
  if (q.t >= 0)
    for (int64_t c = t; c < q.n_chains; c += 256) {
      const double ac = q.a[c];
      s += ac;
      if (warm && !z.flag[c]) {
        sa += ac;
        sc += ac * z.crit[c];
      }
    }
  s = wave_sum(s), sa = wave_sum(sa), sc = wave_sum(sc);
  if ((t & 63) == 0) sh[0][t >> 6] = s, sh[1][t >> 6] = sa, sh[2][t >> 6] = sc;
  __syncthreads();
  if (t != 0) return;
  double base = q.step_size;
  if (q.t >= 0) {
    const double abar = ((sh[0][0] + sh[0][1]) + (sh[0][2] + sh[0][3])) / (double)q.n_chains;
    q.accept_hist[q.t] = abar;
    base = q.state[HS_BASE];
    if (warm) {
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
    q.state[HS_LOG_T] = z.log_t0;
    q.state[HS_V] = z.v0;
    q.state[HS_LOG_TBAR] = z.log_tbar0;
  }
  q.state[HS_BASE] = base;
  if (warm) {
    // low32(s_t + 1) is the low word of the next iteration's stream
    const double tau = chees_halton(q.w_next) * z.traj_hist[q.t];
    const double wsum = (sh[1][0] + sh[1][1]) + (sh[1][2] + sh[1][3]), csum = (sh[2][0] + sh[2][1]) + (sh[2][2] + sh[2][3]);
    const double ghat = tau * csum / wsum;
    const double m = z.m0 + (double)(q.t + 1);
    double log_t = q.state[HS_LOG_T];
    if (wsum != 0.0 && isfinite(ghat)) {
      const double v = kCheesBeta2 * q.state[HS_V] + (1.0 - kCheesBeta2) * ghat * ghat;
      q.state[HS_V] = v;
      log_t += z.lr * ghat / (sqrt(v / (1.0 - pow(kCheesBeta2, m))) + kCheesAdamEps);
    }
    log_t = fmin(fmax(log_t, log(base)), log((double)z.max_leapfrog * base));
    const double eta = pow(m, -kHmcKappa);
    q.state[HS_LOG_T] = log_t;
    q.state[HS_LOG_TBAR] = eta * log_t + (1.0 - eta) * q.state[HS_LOG_TBAR];
  }
  if (q.t + 1 >= q.n_iter) return;
  if (q.t + 1 < q.n_warmup) {
    const Philox4 o = philox_sub(~(uint64_t)0, kHmcUniformCol, q.w_next, 0, q.k0, q.k1_next);
    const double eps = base * (1.0 + q.jitter * (2.0 * u01(o.z, o.w) - 1.0));
    const double traj = exp(q.state[HS_LOG_T]);
    const long long n_leap = chees_steps(chees_halton(q.w_next + 1u) * traj, eps, z.max_leapfrog);
    q.state[HS_EPS] = eps;
    q.step_hist[q.t + 1] = eps;
    z.traj_hist[q.t + 1] = traj;
    z.leap_hist[q.t + 1] = n_leap;
    q.state[HS_LNEXT] = (double)n_leap;
  } else if (q.t >= q.n_warmup) {
    q.state[HS_EPS] = q.step_hist[q.t + 1];
  }
}

struct HmcCheesPlanArgs {
  double* state;
  double* step_hist;
  double* traj_hist;
  long long* leap_hist;
  int64_t n_warmup, n_iter;
  double jitter;
  uint32_t k0, seed_hi;
  uint64_t stream_offset;
  int max_leapfrog;
};

// launched once, when the warm-up has ended: eps_t, T_t = exp(log T_bar) and L_t of every sampling iteration, one thread
// each, from hmc_chees_adapt_kernel's expressions; the first one's eps goes into the state
__global__ void __launch_bounds__(256) hmc_chees_plan_kernel(const HmcCheesPlanArgs q) {
  const int64_t t = q.n_warmup + (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= q.n_iter) return;
  const uint64_t s = q.stream_offset + (uint64_t)t;
  const double base = q.state[HS_BASE];
  const Philox4 o = philox_sub(~(uint64_t)0, kHmcUniformCol, (uint32_t)s, 0, q.k0, q.seed_hi ^ (uint32_t)(s >> 32));
  const double eps = base * (1.0 + q.jitter * (2.0 * u01(o.z, o.w) - 1.0));
  const double traj = exp(q.state[HS_LOG_TBAR]);
  q.step_hist[t] = eps;
  q.traj_hist[t] = traj;
  q.leap_hist[t] = chees_steps(chees_halton((uint32_t)s + 1u) * traj, eps, q.max_leapfrog);
  if (t == q.n_warmup) q.state[HS_EPS] = eps;
}

struct HmcChees {            // vb_hmc_run_chees's own arguments
  int max_leapfrog;
  double lr;
  double* traj_state;      // in / out: log T, v, log T_bar, m
  double* traj_hist;       // n_iter
  int64_t* leap_hist;      // n_iter
};

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
  const HmcChees* chees;   // vb_hmc_run_chees: n_leapfrog is then the largest step count; else nullptr
};

// vb_hmc_run, vb_hmc_run_metric and vb_hmc_run_chees: the diagonal kind without moments and without ChEES enqueues exactly
// what vb_hmc_run always did
int hmc_run(vb_ctx* ctx, const HmcCall& hc, const double* x0, int64_t n_chains, int64_t d, int64_t n_warmup, int64_t n_draws,
            int64_t thin, int n_leapfrog, double step_size, double target_accept, double jitter, uint64_t seed,
            uint64_t stream_offset, double* draws, double* logp, double* last_x, double* chain_mean, double* chain_m2,
            double* accept_rate, double* step_hist, double* accept_hist, double* final_step, int64_t* n_divergent) {
  const bool dense = hc.kind == VB_HMC_METRIC_DENSE, moments = hc.moment_shift != nullptr;
  const HmcChees* ch = hc.chees;
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
                o_cs = carve(ch ? 2 * ld : 0), o_nu = carve(ch ? 1 : 0), o_crit = carve(ch ? C : 0),
                o_flag = carve(ch ? (C + 1) / 2 : 0), o_vel = carve(ch && dense && n_warmup > 0 ? mat : 0),
                o_th = carve(ch ? n_iter : 0), o_lh = carve(ch ? n_iter : 0),
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
  auto velocity = [&](double* vel) {                   // v' = r L' (ChEES, warm-up): the drift's operands, stored
    gemm_f64_launch<true>(st, gemm_product(a.p, ld, base + o_lt, ld, (int)C, (int)d, (int)ld, 1), 1, n_cu,
                          EpiHmcVelocity{vel, ld});
    return hipGetLastError();
  };

  const uint32_t k0 = (uint32_t)seed, seed_hi = (uint32_t)(seed >> 32);
  HmcCheesBuf cb{};
  HmcCheesAdaptArgs cz{};
  if (ch) {
    cb.colsum = base + o_cs, cb.n_usable = base + o_nu, cb.crit = base + o_crit, cb.flag = (int*)(base + o_flag);
    cb.vel = dense && n_warmup > 0 ? base + o_vel : nullptr;
    cz.crit = cb.crit, cz.flag = cb.flag, cz.traj_hist = base + o_th, cz.leap_hist = (long long*)(base + o_lh);
    cz.log_t0 = ch->traj_state[0], cz.v0 = ch->traj_state[1], cz.log_tbar0 = ch->traj_state[2], cz.m0 = ch->traj_state[3];
    cz.lr = ch->lr, cz.max_leapfrog = ch->max_leapfrog;
  }
  // ChEES: the step count of the iteration about to be enqueued -- fetched after every warm-up iteration (8 bytes), and for
  // all sampling iterations at once when the warm-up has ended
  int steps = n_leapfrog;
  auto steps_ok = [&](double l) { return l >= 1.0 && l <= (double)n_leapfrog; };
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
        for (int l = 0; l < steps; ++l) {
          VB_HIP(ctx, drift());
          VB_TRY(model_grad_rows(ctx, a.xp, ld, C, d, a.gp, a.fp));
          VB_HIP(ctx, kick(a.gp, l + 1 == steps ? 0.5 : 1.0));
        }
      } else {
        hipLaunchKernelGGL(hmc_begin_kernel<false>, chain_grid, block, 0, st, a, k0, k1, w);
        VB_HIP(ctx, hipGetLastError());
        for (int l = 0; l < steps; ++l) {
          VB_TRY(model_grad_rows(ctx, a.xp, ld, C, d, a.gp, a.fp));
          if (l + 1 == steps) break;
          hipLaunchKernelGGL(hmc_leap_kernel, leap_grid, block, 0, st, a);
          VB_HIP(ctx, hipGetLastError());
        }
      }
      if (ch && t < n_warmup) {      // the criterion, before the accept step overwrites x
        if (dense) VB_HIP(ctx, velocity(base + o_vel));
        hipLaunchKernelGGL(hmc_chees_mean_kernel, dim3((unsigned)((d + 63) / 64)), block, 0, st, a, cb);
        VB_HIP(ctx, hipGetLastError());
        if (dense) hipLaunchKernelGGL(hmc_chees_chain_kernel<true>, chain_grid, block, 0, st, a, cb);
        else hipLaunchKernelGGL(hmc_chees_chain_kernel<false>, chain_grid, block, 0, st, a, cb);
        VB_HIP(ctx, hipGetLastError());
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
    if (!ch) {
      hipLaunchKernelGGL(hmc_adapt_kernel, dim3(1), block, 0, st, q);
      VB_HIP(ctx, hipGetLastError());
      continue;
    }
    hipLaunchKernelGGL(hmc_chees_adapt_kernel, dim3(1), block, 0, st, q, cz);
    VB_HIP(ctx, hipGetLastError());
    if (t + 1 < n_warmup) {
      double l_next = 0.0;
      const FetchSeg seg{a.state + HS_LNEXT, sizeof(double), &l_next};
      VB_TRY(fetch_blocking(ctx, st, &seg, 1));
      if (!steps_ok(l_next)) return fail(ctx, VB_ERR_NUMERIC, "%s: the device planned %g leapfrog steps", hc.name, l_next);
      steps = (int)l_next;
    } else if (t + 1 == n_warmup && n_draws > 0) {
      HmcCheesPlanArgs pq;
      pq.state = a.state, pq.step_hist = q.step_hist, pq.traj_hist = cz.traj_hist, pq.leap_hist = cz.leap_hist;
      pq.n_warmup = n_warmup, pq.n_iter = n_iter, pq.jitter = jitter, pq.k0 = k0, pq.seed_hi = seed_hi;
      pq.stream_offset = stream_offset, pq.max_leapfrog = ch->max_leapfrog;
      hipLaunchKernelGGL(hmc_chees_plan_kernel, dim3((unsigned)((n_draws + 255) / 256)), block, 0, st, pq);
      VB_HIP(ctx, hipGetLastError());
      const FetchSeg seg{cz.leap_hist + n_warmup, (size_t)n_draws * sizeof(long long), ch->leap_hist + n_warmup};
      VB_TRY(fetch_blocking(ctx, st, &seg, 1));
      for (int64_t i = n_warmup; i < n_iter; ++i)
        if (!steps_ok((double)ch->leap_hist[i]))
          return fail(ctx, VB_ERR_NUMERIC, "%s: the device planned %lld leapfrog steps", hc.name, (long long)ch->leap_hist[i]);
    }
    if (t + 1 >= n_warmup && t + 1 < n_iter) steps = (int)ch->leap_hist[t + 1];
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
  if (ch) {
    VB_HIP(ctx, hipMemcpyAsync(ch->traj_hist, cz.traj_hist, (size_t)n_iter * sizeof(double), hipMemcpyDeviceToHost, st));
    VB_HIP(ctx, hipMemcpyAsync(ch->leap_hist, cz.leap_hist, (size_t)n_iter * sizeof(long long), hipMemcpyDeviceToHost, st));
    VB_HIP(ctx, hipMemcpyAsync(ch->traj_state, a.state + HS_LOG_T, 3 * sizeof(double), hipMemcpyDeviceToHost, st));
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
  if (ch) ch->traj_state[3] += (double)n_warmup;
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
  const HmcCall hc{"vb_hmc_run", VB_HMC_METRIC_DIAG, inv_mass, nullptr, nullptr, nullptr, nullptr};
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
  const HmcCall hc{"vb_hmc_run_metric", metric_kind, metric, moment_shift, moment_sum, moment_m2, nullptr};
  return hmc_run(ctx, hc, x0, n_chains, d, n_warmup, n_draws, thin, n_leapfrog, step_size, target_accept, jitter, seed,
                 stream_offset, draws, logp, last_x, chain_mean, chain_m2, accept_rate, step_hist, accept_hist, final_step,
                 n_divergent);
}

int vb_hmc_run_chees(vb_ctx* ctx, const double* x0, int metric_kind, const double* metric, int64_t n_chains, int64_t d,
                     int64_t n_warmup, int64_t n_draws, int64_t thin, int max_leapfrog, double trajectory_lr, double step_size,
                     double target_accept, double jitter, uint64_t seed, uint64_t stream_offset, const double* moment_shift,
                     double* moment_sum, double* moment_m2, double* draws, double* logp, double* last_x, double* chain_mean,
                     double* chain_m2, double* accept_rate, double* step_hist, double* accept_hist, double* final_step,
                     int64_t* n_divergent, double* traj_state, double* traj_hist, int64_t* leap_hist) {
  if (!ctx || !x0 || !metric || !last_x || !step_hist || !accept_hist || !final_step || !traj_state || !traj_hist || !leap_hist)
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
  if (max_leapfrog < 1) return fail(ctx, VB_ERR_INVALID, "max_leapfrog must be at least 1");
  if (!(trajectory_lr >= 0.0) || !std::isfinite(trajectory_lr))
    return fail(ctx, VB_ERR_INVALID, "trajectory_lr must be non-negative and finite");
  for (int k = 0; k < 4; ++k)
    if (!std::isfinite(traj_state[k])) return fail(ctx, VB_ERR_INVALID, "traj_state[%d] must be finite", k);
  if (traj_state[1] < 0.0 || traj_state[3] < 0.0)
    return fail(ctx, VB_ERR_INVALID, "traj_state: the second moment and the iteration count must be non-negative");
  if (n_chains < 2 && n_warmup > 0)
    return fail(ctx, VB_ERR_INVALID, "the trajectory length is adapted across the chains: n_chains >= 2 with n_warmup > 0");
  const HmcChees ch{max_leapfrog, trajectory_lr, traj_state, traj_hist, leap_hist};
  const HmcCall hc{"vb_hmc_run_chees", metric_kind, metric, moment_shift, moment_sum, moment_m2, &ch};
  return hmc_run(ctx, hc, x0, n_chains, d, n_warmup, n_draws, thin, max_leapfrog, step_size, target_accept, jitter, seed,
                 stream_offset, draws, logp, last_x, chain_mean, chain_m2, accept_rate, step_hist, accept_hist, final_step,
                 n_divergent);
}

}  // extern "C"

