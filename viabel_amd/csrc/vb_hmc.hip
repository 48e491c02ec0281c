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
//
// ---- the host side ------------------------------------------------------------------------------------------------------
// The three entries fill one request (HmcRun) and call hmc_run, whose body is the lists above: hmc_refuse, hmc_layout (one
// named offset per workspace piece), hmc_upload, hmc_bind (the kernels' argument structs on the workspace: HmcDev), then per
// iteration hmc_trajectory, hmc_chees_criterion (ChEES warm-up), hmc_end, hmc_window_moments (moment_shift given) and
// hmc_adapt (ChEES: with the step-count fetches), and at last hmc_download.  A StreamDrain declared before the upload
// synchronises the stream on every way out.  It, the model refusals, the row copies, the uniforms' pseudo column and the
// divergence threshold are vb_particles.h's, shared with vb_smc.hip, vb_svgd.hip and vb_ksd.hip.
#include "vb_particles.h"
#include "vb_rng.h"

namespace vb {

constexpr int64_t kHmcDrawBudgetBytes = (int64_t)1 << 30;      // the device copy of the kept draws
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
  const bool divergent = !isfinite(dh) || h1 - h0 > kDivergence;
  const Philox4 o = philox_sub((uint64_t)c, kUniformCol, e.w, 0, e.k0, e.k1);
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
    const Philox4 o = philox_sub(~(uint64_t)0, kUniformCol, q.w_next, 0, q.k0, q.k1_next);
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
    const Philox4 o = philox_sub(~(uint64_t)0, kUniformCol, q.w_next, 0, q.k0, q.k1_next);
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
  const Philox4 o = philox_sub(~(uint64_t)0, kUniformCol, (uint32_t)s, 0, q.k0, q.seed_hi ^ (uint32_t)(s >> 32));
  const double eps = base * (1.0 + q.jitter * (2.0 * u01(o.z, o.w) - 1.0));
  const double traj = exp(q.state[HS_LOG_TBAR]);
  q.step_hist[t] = eps;
  q.traj_hist[t] = traj;
  q.leap_hist[t] = chees_steps(chees_halton((uint32_t)s + 1u) * traj, eps, q.max_leapfrog);
  if (t == q.n_warmup) q.state[HS_EPS] = eps;
}

// ---- the host driver: one request, then the stages hmc_run lists -------------------------------------------------------------
struct HmcRun {              // one call, as its entry states it: what differs between the entries, then what all three take
  const char* name;        // the entry, for the messages
  int kind;                // VB_HMC_METRIC_*
  const double* metric;    // inv_mass[d], or the lower factor L (d x d)
  int n_leapfrog;          // vb_hmc_run_chees: max_leapfrog, the largest step count
  const double* moment_shift;      // the window moments: all three or none
  double *moment_sum, *moment_m2;
  double trajectory_lr;            // vb_hmc_run_chees's own block: traj_state given, else all zero
  double *traj_state, *traj_hist;  // in / out: log T, v, log T_bar, m; n_iter
  int64_t* leap_hist;              // n_iter
  const double* x0;        // C x d
  int64_t n_chains, d, n_warmup, n_draws, thin;
  double step_size, target_accept, jitter;
  uint64_t seed, stream_offset;
  double *draws, *logp, *last_x, *chain_mean, *chain_m2, *accept_rate, *step_hist, *accept_hist, *final_step;
  int64_t* n_divergent;
  bool dense() const { return kind == VB_HMC_METRIC_DENSE; }
  bool chees() const { return traj_state != nullptr; }
  int64_t n_iter() const { return n_warmup + n_draws; }
  int64_t n_kept() const { return (n_draws + thin - 1) / thin; }
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

// Refusals, in this order: a call that violates two conditions reports the first
static int hmc_refuse(vb_ctx* ctx, const HmcRun& r) {
  const int64_t d = r.d;
  if (r.thin < 1) return fail(ctx, VB_ERR_INVALID, "thin must be at least 1");
  if (r.n_leapfrog < 1) return fail(ctx, VB_ERR_INVALID, "n_leapfrog must be at least 1");
  if (!(r.step_size > 0.0) || !std::isfinite(r.step_size))
    return fail(ctx, VB_ERR_INVALID, "step_size must be positive and finite");
  if (!(r.target_accept > 0.0 && r.target_accept < 1.0)) return fail(ctx, VB_ERR_INVALID, "target_accept must lie in (0, 1)");
  if (!(r.jitter >= 0.0 && r.jitter < 1.0)) return fail(ctx, VB_ERR_INVALID, "jitter must lie in [0, 1)");
  VB_TRY(model_bound_refuse(ctx, r.name, "x0", d));
  if (r.dense() && d > kHmcDenseMaxDim)
    return fail(ctx, VB_ERR_UNSUPPORTED, "the dense metric takes at most %d dimensions (got %lld)", kHmcDenseMaxDim, (long long)d);
  if (!r.dense()) {
    VB_TRY(positive_finite(ctx, r.name, "inv_mass", r.metric, d));
  } else {
    for (int64_t i = 0; i < d; ++i) {
      if (!(r.metric[i * d + i] > 0.0) || !std::isfinite(r.metric[i * d + i]))
        return fail(ctx, VB_ERR_INVALID, "L[%lld][%lld] must be positive and finite", (long long)i, (long long)i);
      for (int64_t j = 0; j < i; ++j)
        if (!std::isfinite(r.metric[i * d + j]))
          return fail(ctx, VB_ERR_INVALID, "L[%lld][%lld] must be finite", (long long)i, (long long)j);
    }
  }
  VB_TRY(model_device_refuse(ctx, r.name, false, true));
  if (r.n_chains > ((int64_t)1 << 31) - 8 || r.n_iter() > ((int64_t)1 << 40) ||
      (double)r.n_chains * (double)round_up(d, 16) > 0x1p36)
    return fail(ctx, VB_ERR_UNSUPPORTED, "%s takes at most 2^31 - 8 chains, 2^36 chain coordinates (n_chains x "
                                         "round_up(d, 16)) and 2^40 iterations", r.name);
  if (r.draws && (double)r.n_kept() * (double)r.n_chains * (double)d * sizeof(double) > (double)kHmcDrawBudgetBytes)
    return fail(ctx, VB_ERR_UNSUPPORTED, "the kept draws (%lld x %lld x %lld doubles) exceed the device draw buffer's budget of "
                                         "%lld bytes: raise thin or pass no draws",
                (long long)r.n_kept(), (long long)r.n_chains, (long long)d, (long long)kHmcDrawBudgetBytes);
  return VB_OK;
}

// Layout: the offset (in doubles) of every piece of vb_ctx::hmc_work, carved in the order of the header's piece lists
struct HmcLayout {
  int64_t x, g, xp, gp, p, mean, m2, f, fp, h0, a, count, inv_mass, state, step_hist, accept_hist, n_div;
  int64_t l, lt, shift, s1, s2, xc, colsum, n_usable, crit, flag, vel, traj_hist, leap_hist;      // dense, moments, ChEES
  int64_t draws, logp, slab;     // not zeroed
  int64_t zeroed, total, ld;     // zeroed: the prefix every call clears (everything before the draws)
  int splits;                    // Gram slabs of the dense moments; else 0
};

static HmcLayout hmc_layout(const HmcRun& r) {
  const bool dense = r.dense(), moments = r.moment_shift != nullptr, ch = r.chees();
  const int64_t C = r.n_chains, d = r.d, T = r.n_iter(), ld = round_up(d, 16), mat = C * ld;
  HmcLayout o;
  Carver carve;
  o.ld = ld, o.splits = dense && moments ? hmc_gram_splits(C, ld) : 0;
  o.x = carve(mat), o.g = carve(mat), o.xp = carve(mat), o.gp = carve(mat), o.p = carve(mat), o.mean = carve(mat);
  o.m2 = carve(mat), o.f = carve(C), o.fp = carve(C), o.h0 = carve(C), o.a = carve(C), o.count = carve(C);
  o.inv_mass = carve(ld), o.state = carve(HS_NUM), o.step_hist = carve(T), o.accept_hist = carve(T), o.n_div = carve(C);
  o.l = carve(dense ? ld * ld : 0), o.lt = carve(dense ? ld * ld : 0), o.shift = carve(moments ? ld : 0);
  o.s1 = carve(moments ? ld : 0), o.s2 = carve(moments ? (dense ? d * d : ld) : 0), o.xc = carve(o.splits ? mat : 0);
  o.colsum = carve(ch ? 2 * ld : 0), o.n_usable = carve(ch ? 1 : 0), o.crit = carve(ch ? C : 0);
  o.flag = carve(ch ? (C + 1) / 2 : 0), o.vel = carve(ch && dense && r.n_warmup > 0 ? mat : 0);
  o.traj_hist = carve(ch ? T : 0), o.leap_hist = carve(ch ? T : 0);
  o.draws = carve(r.draws ? r.n_kept() * C * d : 0), o.logp = carve(r.logp ? r.n_kept() * C : 0);
  o.slab = carve((int64_t)o.splits * ld * ld), o.zeroed = o.draws, o.total = carve.off;
  return o;
}

// Upload: the zeroed prefix, x0, the metric, the shift.  `pack` is read until the stream is next drained.
static int hmc_upload(vb_ctx* ctx, const HmcRun& r, const HmcLayout& o, std::vector<double>& pack) {
  hipStream_t st = ctx->stream;
  double* base = (double*)ctx->hmc_work.ptr;
  const int64_t d = r.d, ld = o.ld;
  // everything up to the draws starts from zero: pad columns, Welford sums, counts, state, the factors' pads, the moments
  VB_HIP(ctx, hipMemsetAsync(base, 0, (size_t)o.zeroed * sizeof(double), st));
  VB_TRY(upload_rows(ctx, base + o.x, r.x0, r.n_chains, d, ld, false));
  if (!r.dense()) {
    VB_HIP(ctx, hipMemcpyAsync(base + o.inv_mass, r.metric, (size_t)d * sizeof(double), hipMemcpyHostToDevice, st));
  } else {                       // [L | L'], each ld x ld with zeros above / below the diagonal and in the pads
    pack.assign((size_t)(2 * ld * ld), 0.0);
    for (int64_t i = 0; i < d; ++i)
      for (int64_t j = 0; j <= i; ++j) {
        const double v = r.metric[i * d + j];
        pack[(size_t)(i * ld + j)] = v;
        pack[(size_t)(ld * ld + j * ld + i)] = v;
      }
    VB_HIP(ctx, hipMemcpyAsync(base + o.l, pack.data(), (size_t)(ld * ld) * sizeof(double), hipMemcpyHostToDevice, st));
    VB_HIP(ctx, hipMemcpyAsync(base + o.lt, pack.data() + ld * ld, (size_t)(ld * ld) * sizeof(double), hipMemcpyHostToDevice, st));
  }
  if (r.moment_shift)
    VB_HIP(ctx, hipMemcpyAsync(base + o.shift, r.moment_shift, (size_t)d * sizeof(double), hipMemcpyHostToDevice, st));
  return VB_OK;
}

// Binding: the kernels' argument structs on the workspace, and what every launch of the call shares
struct HmcDev {
  hipStream_t st;
  int n_cu;
  bool dense;
  double* base;                    // vb_ctx::hmc_work, laid out by o
  HmcLayout o;
  HmcArgs a;
  HmcMomentArgs mq;
  HmcCheesBuf cb;                  // cb, cz: ChEES only
  HmcCheesAdaptArgs cz;
  HmcAdaptArgs q;                  // t, k1_next, w_next: hmc_adapt sets them, the keys and stream of the iteration it precedes
  uint32_t seed_hi;
  dim3 chain_grid, leap_grid, col_grid, block;
};

static HmcDev hmc_bind(vb_ctx* ctx, const HmcRun& r, const HmcLayout& o) {
  double* base = (double*)ctx->hmc_work.ptr;
  const int64_t C = r.n_chains, ld = o.ld;
  HmcDev v{};
  v.st = ctx->stream, v.n_cu = ctx->prop.multiProcessorCount, v.dense = r.dense(), v.base = base, v.o = o;
  v.seed_hi = (uint32_t)(r.seed >> 32);
  v.chain_grid = dim3((unsigned)((C + 3) / 4)), v.leap_grid = dim3((unsigned)((C * ld + 255) / 256));
  v.col_grid = dim3((unsigned)((r.d + 63) / 64)), v.block = dim3(256);
  HmcArgs& a = v.a;
  HmcMomentArgs& mq = v.mq;
  HmcCheesBuf& cb = v.cb;
  HmcCheesAdaptArgs& cz = v.cz;
  HmcAdaptArgs& q = v.q;
  a.x = base + o.x, a.g = base + o.g, a.f = base + o.f, a.xp = base + o.xp, a.gp = base + o.gp, a.fp = base + o.fp;
  a.p = base + o.p, a.H0 = base + o.h0, a.a = base + o.a, a.mean = base + o.mean, a.m2 = base + o.m2;
  a.count = base + o.count, a.n_div = (long long*)(base + o.n_div), a.inv_mass = base + o.inv_mass, a.state = base + o.state;
  a.ld = ld, a.n_chains = C, a.d = (int)r.d;
  mq.x = a.x, mq.shift = base + o.shift, mq.s1 = base + o.s1, mq.s2 = base + o.s2, mq.xc = base + o.xc;
  mq.slab = base + o.slab, mq.slab_stride = ld * ld, mq.ld = ld, mq.n_chains = C, mq.d = (int)r.d, mq.splits = o.splits;
  if (r.chees()) {
    cb.colsum = base + o.colsum, cb.n_usable = base + o.n_usable, cb.crit = base + o.crit, cb.flag = (int*)(base + o.flag);
    cb.vel = v.dense && r.n_warmup > 0 ? base + o.vel : nullptr;
    cz.crit = cb.crit, cz.flag = cb.flag, cz.traj_hist = base + o.traj_hist, cz.leap_hist = (long long*)(base + o.leap_hist);
    cz.log_t0 = r.traj_state[0], cz.v0 = r.traj_state[1], cz.log_tbar0 = r.traj_state[2], cz.m0 = r.traj_state[3];
    cz.lr = r.trajectory_lr, cz.max_leapfrog = r.n_leapfrog;
  }
  q.a = a.a, q.n_chains = C, q.state = a.state, q.step_hist = base + o.step_hist, q.accept_hist = base + o.accept_hist;
  q.n_warmup = r.n_warmup, q.n_iter = r.n_iter(), q.step_size = r.step_size, q.target = r.target_accept, q.jitter = r.jitter;
  q.mu = log(10.0 * r.step_size), q.k0 = (uint32_t)r.seed;
  return v;
}

// a product of the dense kind, rows (C x ld) times a padded factor: K runs over the ld columns (zeros in both operands' pads)
template <class Epi>
static hipError_t hmc_product(const HmcDev& v, const double* rows, const double* factor, int tri_mode, Epi epi) {
  const HmcArgs& a = v.a;
  gemm_f64_launch<true>(v.st, gemm_product(rows, a.ld, factor, a.ld, (int)a.n_chains, a.d, (int)a.ld, tri_mode), 1, v.n_cu, epi);
  return hipGetLastError();
}

// Trajectory, both kinds: the begin kernel (dense: and the first half kick), then `steps` times the drift (diagonal:
// hmc_leap_kernel, kick and drift in one, the first drift being the begin kernel's), the gradient, and (dense) the kick --
// a half one after the last gradient; the diagonal kind's is the end kernel's.  Kick: r += c eps (g L), B = L, zero for
// k < j; drift: xp += eps (r L'), B = L', zero for k > j.
static int hmc_trajectory(vb_ctx* ctx, const HmcDev& v, int steps) {
  const HmcArgs& a = v.a;
  const double *l = v.base + v.o.l, *lt = v.base + v.o.lt;
  if (v.dense) hipLaunchKernelGGL(hmc_begin_kernel<true>, v.chain_grid, v.block, 0, v.st, a, v.q.k0, v.q.k1_next, v.q.w_next);
  else hipLaunchKernelGGL(hmc_begin_kernel<false>, v.chain_grid, v.block, 0, v.st, a, v.q.k0, v.q.k1_next, v.q.w_next);
  VB_HIP(ctx, hipGetLastError());
  if (v.dense) VB_HIP(ctx, hmc_product(v, a.g, l, 3, EpiHmcKick{a.p, a.ld, a.state, 0.5}));
  for (int i = 0; i < steps; ++i) {
    if (v.dense) {
      VB_HIP(ctx, hmc_product(v, a.p, lt, 1, EpiHmcDrift{a.xp, a.ld, a.state}));
    } else if (i > 0) {
      hipLaunchKernelGGL(hmc_leap_kernel, v.leap_grid, v.block, 0, v.st, a);
      VB_HIP(ctx, hipGetLastError());
    }
    VB_TRY(model_grad_rows(ctx, a.xp, a.ld, a.n_chains, a.d, a.gp, a.fp));
    if (v.dense) VB_HIP(ctx, hmc_product(v, a.gp, l, 3, EpiHmcKick{a.p, a.ld, a.state, i + 1 == steps ? 0.5 : 1.0}));
  }
  return VB_OK;
}

// ChEES criterion (warm-up only), between the last gradient and the end kernel: the accept step overwrites x.  Dense: the
// velocity v' = r L' first, the drift's operands
static int hmc_chees_criterion(vb_ctx* ctx, const HmcDev& v) {
  if (v.dense) VB_HIP(ctx, hmc_product(v, v.a.p, v.base + v.o.lt, 1, EpiHmcVelocity{v.base + v.o.vel, v.a.ld}));
  hipLaunchKernelGGL(hmc_chees_mean_kernel, v.col_grid, v.block, 0, v.st, v.a, v.cb);
  VB_HIP(ctx, hipGetLastError());
  if (v.dense) hipLaunchKernelGGL(hmc_chees_chain_kernel<true>, v.chain_grid, v.block, 0, v.st, v.a, v.cb);
  else hipLaunchKernelGGL(hmc_chees_chain_kernel<false>, v.chain_grid, v.block, 0, v.st, v.a, v.cb);
  VB_HIP(ctx, hipGetLastError());
  return VB_OK;
}

// End kernel of iteration t: the accept step, and in the sampling phase the statistics and every thin-th draw
static int hmc_end(vb_ctx* ctx, const HmcRun& r, const HmcDev& v, int64_t t) {
  const int64_t C = r.n_chains, si = t - r.n_warmup;
  HmcEndArgs e;
  e.k0 = v.q.k0, e.k1 = v.q.k1_next, e.w = v.q.w_next;
  e.sampling = si >= 0, e.k = (double)(si + 1);
  const bool keep = si >= 0 && si % r.thin == 0;
  e.draw_row = keep && r.draws ? v.base + v.o.draws + (si / r.thin) * C * r.d : nullptr;
  e.logp_row = keep && r.logp ? v.base + v.o.logp + (si / r.thin) * C : nullptr;
  if (v.dense) hipLaunchKernelGGL(hmc_end_kernel<true>, v.chain_grid, v.block, 0, v.st, v.a, e);
  else hipLaunchKernelGGL(hmc_end_kernel<false>, v.chain_grid, v.block, 0, v.st, v.a, e);
  VB_HIP(ctx, hipGetLastError());
  return VB_OK;
}

// Window moments of the states after the accept step
static int hmc_window_moments(vb_ctx* ctx, const HmcDev& v) {
  const HmcMomentArgs& mq = v.mq;
  if (v.dense) {
    hipLaunchKernelGGL(hmc_moment_kernel<true>, v.col_grid, v.block, 0, v.st, mq);
    VB_HIP(ctx, hipGetLastError());
    gemm_f64_launch<false>(v.st, gemm_product(mq.xc, mq.ld, mq.xc, mq.ld, mq.d, mq.d, (int)mq.n_chains, 0), mq.splits, v.n_cu,
                           EpiHmcSlab{mq.slab, mq.slab_stride, mq.ld});
    VB_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(hmc_gram_add_kernel, dim3((unsigned)(((int64_t)mq.d * mq.d + 255) / 256)), v.block, 0, v.st, mq);
  } else {
    hipLaunchKernelGGL(hmc_moment_kernel<false>, v.col_grid, v.block, 0, v.st, mq);
  }
  VB_HIP(ctx, hipGetLastError());
  return VB_OK;
}

// Adapt step after iteration t (t = -1: before the first): the step size of iteration t + 1, whose keys and stream stay in
// v.q for its begin and end kernels.  ChEES: also its `steps` -- fetched after every warm-up iteration but the last
// (8 bytes), and for all sampling iterations at once, behind the plan kernel, when the warm-up has ended
static int hmc_adapt(vb_ctx* ctx, const HmcRun& r, HmcDev& v, int64_t t, int& steps) {
  const uint64_t sn = r.stream_offset + (uint64_t)(t + 1);
  v.q.t = t, v.q.k1_next = v.seed_hi ^ (uint32_t)(sn >> 32), v.q.w_next = (uint32_t)sn;
  if (r.chees()) hipLaunchKernelGGL(hmc_chees_adapt_kernel, dim3(1), v.block, 0, v.st, v.q, v.cz);
  else hipLaunchKernelGGL(hmc_adapt_kernel, dim3(1), v.block, 0, v.st, v.q);
  VB_HIP(ctx, hipGetLastError());
  if (!r.chees()) return VB_OK;
  auto steps_ok = [&](double l) { return l >= 1.0 && l <= (double)r.n_leapfrog; };
  if (t + 1 < r.n_warmup) {
    double l_next = 0.0;
    const FetchSeg seg{v.a.state + HS_LNEXT, sizeof(double), &l_next};
    VB_TRY(fetch_blocking(ctx, v.st, &seg, 1));
    if (!steps_ok(l_next)) return fail(ctx, VB_ERR_NUMERIC, "%s: the device planned %g leapfrog steps", r.name, l_next);
    steps = (int)l_next;
  } else if (t + 1 == r.n_warmup && r.n_draws > 0) {
    HmcCheesPlanArgs pq;
    pq.state = v.a.state, pq.step_hist = v.q.step_hist, pq.traj_hist = v.cz.traj_hist, pq.leap_hist = v.cz.leap_hist;
    pq.n_warmup = r.n_warmup, pq.n_iter = r.n_iter(), pq.jitter = r.jitter, pq.k0 = v.q.k0, pq.seed_hi = v.seed_hi;
    pq.stream_offset = r.stream_offset, pq.max_leapfrog = r.n_leapfrog;
    hipLaunchKernelGGL(hmc_chees_plan_kernel, dim3((unsigned)((r.n_draws + 255) / 256)), v.block, 0, v.st, pq);
    VB_HIP(ctx, hipGetLastError());
    const FetchSeg seg{v.cz.leap_hist + r.n_warmup, (size_t)r.n_draws * sizeof(long long), r.leap_hist + r.n_warmup};
    VB_TRY(fetch_blocking(ctx, v.st, &seg, 1));
    for (int64_t i = r.n_warmup; i < r.n_iter(); ++i)
      if (!steps_ok((double)r.leap_hist[i]))
        return fail(ctx, VB_ERR_NUMERIC, "%s: the device planned %lld leapfrog steps", r.name, (long long)r.leap_hist[i]);
  }
  if (t + 1 >= r.n_warmup && t + 1 < r.n_iter()) steps = (int)r.leap_hist[t + 1];
  return VB_OK;
}

// Download: the call's one synchronisation (ChEES apart), then the host's share of the outputs
static int hmc_download(vb_ctx* ctx, const HmcRun& r, const HmcDev& v) {
  const HmcArgs& a = v.a;
  hipStream_t st = v.st;
  const size_t W = sizeof(double), C = (size_t)r.n_chains, d = (size_t)r.d, T = (size_t)r.n_iter(), kept = (size_t)r.n_kept() * C;
  auto copy = [&](void* dst, const void* src, size_t bytes) {      // an output the caller left out, or an empty one: skipped
    return dst && bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st) : hipSuccess;
  };
  auto rows = [&](double* dst, const double* src) {                 // C x d out of C x ld
    return dst ? download_rows(ctx, dst, src, r.n_chains, r.d, a.ld) : hipSuccess;
  };
  VB_HIP(ctx, rows(r.last_x, a.x));
  VB_HIP(ctx, rows(r.chain_mean, a.mean));
  VB_HIP(ctx, rows(r.chain_m2, a.m2));
  VB_HIP(ctx, copy(r.accept_rate, a.count, C * W));
  VB_HIP(ctx, copy(r.step_hist, v.q.step_hist, T * W));
  VB_HIP(ctx, copy(r.accept_hist, v.q.accept_hist, T * W));
  VB_HIP(ctx, copy(r.final_step, a.state + HS_BASE, W));
  VB_HIP(ctx, copy(r.draws, v.base + v.o.draws, kept * d * W));
  VB_HIP(ctx, copy(r.logp, v.base + v.o.logp, kept * W));
  VB_HIP(ctx, copy(r.moment_sum, v.mq.s1, d * W));
  VB_HIP(ctx, copy(r.moment_m2, v.mq.s2, (v.dense ? d * d : d) * W));
  VB_HIP(ctx, copy(r.traj_hist, v.cz.traj_hist, T * W));
  VB_HIP(ctx, copy(r.leap_hist, v.cz.leap_hist, T * sizeof(long long)));
  VB_HIP(ctx, copy(r.traj_state, a.state + HS_LOG_T, 3 * W));
  std::vector<long long> div(C);
  VB_HIP(ctx, copy(div.data(), a.n_div, C * sizeof(long long)));
  VB_HIP(ctx, hipStreamSynchronize(st));
  int64_t total = 0;
  for (size_t c = 0; c < C; ++c) {
    total += div[c];
    if (r.accept_rate && r.n_draws > 0) r.accept_rate[c] /= (double)r.n_draws;
  }
  if (r.n_divergent) *r.n_divergent = total;
  if (r.chees()) r.traj_state[3] += (double)r.n_warmup;
  return VB_OK;
}

// vb_hmc_run, vb_hmc_run_metric and vb_hmc_run_chees: the header's transition list.  The diagonal kind without moments and
// without ChEES enqueues exactly what vb_hmc_run always did.
static int hmc_run(vb_ctx* ctx, const HmcRun& r) {
  VB_TRY(hmc_refuse(ctx, r));
  VB_HIP(ctx, hipSetDevice(ctx->device));
  VB_TRY(main_stream_write(ctx));
  const HmcLayout lay = hmc_layout(r);
  VB_TRY(ensure(ctx, ctx->hmc_work, (size_t)lay.total * sizeof(double)));
  std::vector<double> pack;      // the dense factors' staging
  StreamDrain drain{ctx->stream};
  VB_TRY(hmc_upload(ctx, r, lay, pack));
  HmcDev dev = hmc_bind(ctx, r, lay);
  VB_TRY(model_grad_rows(ctx, dev.a.x, lay.ld, r.n_chains, r.d, dev.a.g, dev.a.f));      // f, g of the start: carried from here on
  int steps = r.n_leapfrog;
  VB_TRY(hmc_adapt(ctx, r, dev, -1, steps));                                             // eps_0
  for (int64_t t = 0; t < r.n_iter(); ++t) {
    VB_TRY(hmc_trajectory(ctx, dev, steps));
    if (r.chees() && t < r.n_warmup) VB_TRY(hmc_chees_criterion(ctx, dev));
    VB_TRY(hmc_end(ctx, r, dev, t));
    if (r.moment_shift) VB_TRY(hmc_window_moments(ctx, dev));
    VB_TRY(hmc_adapt(ctx, r, dev, t, steps));
  }
  return hmc_download(ctx, r, dev);
}

// what vb_hmc_run_metric and vb_hmc_run_chees refuse before anything of their own (vb_hmc_run's own checks are stricter)
static int hmc_check_segment(vb_ctx* ctx, const HmcRun& r) {
  if (!ctx || !r.x0 || !r.metric || !r.last_x || !r.step_hist || !r.accept_hist || !r.final_step)
    return fail(ctx, VB_ERR_INVALID, "NULL argument");
  if (r.kind != VB_HMC_METRIC_DIAG && r.kind != VB_HMC_METRIC_DENSE)
    return fail(ctx, VB_ERR_INVALID, "metric_kind must be VB_HMC_METRIC_DIAG or VB_HMC_METRIC_DENSE");
  if (r.n_chains <= 0 || r.d <= 0 || r.n_draws < 0 || r.n_warmup < 0 || r.n_warmup + r.n_draws < 1)
    return fail(ctx, VB_ERR_INVALID, "n_chains and d must be positive, n_warmup and n_draws non-negative with at least one "
                                     "iteration between them");
  if (r.n_draws > 0 && (!r.chain_mean || !r.chain_m2 || !r.accept_rate || !r.n_divergent))
    return fail(ctx, VB_ERR_INVALID, "NULL sampling output with n_draws > 0");
  const int given = (r.moment_shift != nullptr) + (r.moment_sum != nullptr) + (r.moment_m2 != nullptr);
  if (given != 0 && given != 3)
    return fail(ctx, VB_ERR_INVALID, "moment_shift, moment_sum and moment_m2 go together: pass all three or none");
  return VB_OK;
}

}  // namespace vb

using namespace vb;

// the arguments all three entries take under one name, as HmcRun's last fields
#define HMC_SHARED_ARGS                                                                                                  \
  .x0 = x0, .n_chains = n_chains, .d = d, .n_warmup = n_warmup, .n_draws = n_draws, .thin = thin, .step_size = step_size, \
  .target_accept = target_accept, .jitter = jitter, .seed = seed, .stream_offset = stream_offset, .draws = draws,        \
  .logp = logp, .last_x = last_x, .chain_mean = chain_mean, .chain_m2 = chain_m2, .accept_rate = accept_rate,            \
  .step_hist = step_hist, .accept_hist = accept_hist, .final_step = final_step, .n_divergent = n_divergent

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
  return hmc_run(ctx, HmcRun{.name = "vb_hmc_run", .kind = VB_HMC_METRIC_DIAG, .metric = inv_mass, .n_leapfrog = n_leapfrog,
                             HMC_SHARED_ARGS});
}

int vb_hmc_run_metric(vb_ctx* ctx, const double* x0, int metric_kind, const double* metric, int64_t n_chains, int64_t d,
                      int64_t n_warmup, int64_t n_draws, int64_t thin, int n_leapfrog, double step_size, double target_accept,
                      double jitter, uint64_t seed, uint64_t stream_offset, const double* moment_shift, double* moment_sum,
                      double* moment_m2, double* draws, double* logp, double* last_x, double* chain_mean, double* chain_m2,
                      double* accept_rate, double* step_hist, double* accept_hist, double* final_step, int64_t* n_divergent) {
  const HmcRun r{.name = "vb_hmc_run_metric", .kind = metric_kind, .metric = metric, .n_leapfrog = n_leapfrog,
                 .moment_shift = moment_shift, .moment_sum = moment_sum, .moment_m2 = moment_m2, HMC_SHARED_ARGS};
  VB_TRY(hmc_check_segment(ctx, r));
  return hmc_run(ctx, r);
}

int vb_hmc_run_chees(vb_ctx* ctx, const double* x0, int metric_kind, const double* metric, int64_t n_chains, int64_t d,
                     int64_t n_warmup, int64_t n_draws, int64_t thin, int max_leapfrog, double trajectory_lr, double step_size,
                     double target_accept, double jitter, uint64_t seed, uint64_t stream_offset, const double* moment_shift,
                     double* moment_sum, double* moment_m2, double* draws, double* logp, double* last_x, double* chain_mean,
                     double* chain_m2, double* accept_rate, double* step_hist, double* accept_hist, double* final_step,
                     int64_t* n_divergent, double* traj_state, double* traj_hist, int64_t* leap_hist) {
  const HmcRun r{.name = "vb_hmc_run_chees", .kind = metric_kind, .metric = metric, .n_leapfrog = max_leapfrog,
                 .moment_shift = moment_shift, .moment_sum = moment_sum, .moment_m2 = moment_m2, .trajectory_lr = trajectory_lr,
                 .traj_state = traj_state, .traj_hist = traj_hist, .leap_hist = leap_hist, HMC_SHARED_ARGS};
  // (its own three pointers first: any NULL argument is reported before a bad metric_kind, as ever)
  if (!traj_state || !traj_hist || !leap_hist) return fail(ctx, VB_ERR_INVALID, "NULL argument");
  VB_TRY(hmc_check_segment(ctx, r));
  if (max_leapfrog < 1) return fail(ctx, VB_ERR_INVALID, "max_leapfrog must be at least 1");
  if (!(trajectory_lr >= 0.0) || !std::isfinite(trajectory_lr))
    return fail(ctx, VB_ERR_INVALID, "trajectory_lr must be non-negative and finite");
  for (int k = 0; k < 4; ++k)
    if (!std::isfinite(traj_state[k])) return fail(ctx, VB_ERR_INVALID, "traj_state[%d] must be finite", k);
  if (traj_state[1] < 0.0 || traj_state[3] < 0.0)
    return fail(ctx, VB_ERR_INVALID, "traj_state: the second moment and the iteration count must be non-negative");
  if (n_chains < 2 && n_warmup > 0)
    return fail(ctx, VB_ERR_INVALID, "the trajectory length is adapted across the chains: n_chains >= 2 with n_warmup > 0");
  return hmc_run(ctx, r);
}

}  // extern "C"

