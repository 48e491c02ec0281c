// Adaptive tempered sequential Monte Carlo with HMC moves on the device gradients (vb_smc_run, vb_smc_reweight).
// n particles in lock-step are the n-row batch model_grad_rows is built for.  Base q0 = N(loc, diag(scale^2)), normalised;
// target the bound model's log p = f, unnormalised; path log pi_beta = beta f + (1 - beta) log q0 from beta = 0 to exactly 1.
// Per particle: x, f, g = grad f, lq = log q0(x); u = f - lq.  The start draws x = loc + scale z from Philox stream s0 (the
// bits vb_noise_generate(seed, stream s0) puts at (row, col)); stage k = 1, 2, ... then is, all on ctx->stream:
//   smc_reweight_kernel  one workgroup of 1024 threads: max u, v = u - max u, E(delta) = (sum e^{delta v})^2 / (n sum e^{2 delta v})
//                        at delta = 1 - beta and, when that falls short of ess_target, at the 40 midpoints of the sequential
//                        bisection of [0, 1 - beta] (41 evaluations, each one pass over v: thread i takes i, i + 1024, ...; the
//                        wave by shuffles, the 16 waves added in index order by thread 0; every decision is taken on the
//                        broadcast value); then w = e^{delta v} (0 for u = -inf), the evidence increment delta max u +
//                        log(sum w / n), ess = n E(delta), the new beta (exactly 1.0 when the first test passes) and a status
//                        word: 1 a NaN or +inf u, 2 every u = -inf, 3 delta = 0 after the search
//   smc_scan_kernel      1024 weights per workgroup, 4 consecutive ones per thread summed serially, the 256 thread totals
//                        scanned serially by thread 0, the block's total being the scan's last element: the block-local
//                        inclusive prefix sums and one total per block
//   smc_search_kernel    one thread per offspring: the block offsets (the serial scan of at most 64 block totals, formed by
//                        thread 0 of every workgroup in LDS), C_j = (offset[j / 1024] + local_j) / total evaluated where the
//                        search looks, t_i = (i + U) / n, a_i = min(#{j : C_j <= t_i}, n - 1) by binary search; U the stage's
//                        uniform (row 2^64 - 1 of pseudo column 0xFFFFFFFE of the stage's first move stream, words z, w).
//                        Every level of the scan is a serial one and every total is the last element of the level below, so C
//                        is non-decreasing, C_j == C_{j-1} bit for bit where w_j == 0 (a zero-weight particle is never an
//                        ancestor) and C_{n-1} == 1
//   smc_gather_kernel    one wave per particle: the padded rows of x and g, f and lq of the ancestor into the second state
//                        buffer (never in place; the host swaps the two pointers)
//   the host fetches {beta, status} (16 bytes, fetch_blocking): the one synchronisation of a stage
//   n_moves times, Philox stream s = s0 + 1 + (k - 1) n_moves + j:
//     smc_begin_kernel   one wave per particle, four per workgroup: p_j = z_j / scale_j in registers, H_0 = -(beta f +
//                        (1 - beta) lq) + 1/2 sum scale_j^2 p_j^2, half kick with the tempered gradient beta g_j -
//                        (1 - beta) (x_j - loc_j) / scale_j^2, first drift xp = x + eps scale^2 p; pads written as zeros
//     model_grad_rows    fp, gp at xp                                                       (n_leapfrog times)
//     smc_leap_kernel    element-wise: the tempered gradient at xp from gp and xp in registers, p += eps G, xp += eps scale^2 p
//     smc_end_kernel     one wave per particle: last half kick, lq' = log q0(xp) and the kinetic energy by lane-strided fma
//                        and wave_sum, H_1, dH = H_0 - H_1, divergent when dH is not finite or H_1 - H_0 > 1000 (a = 0,
//                        rejected), accepted iff log u < dH; an accepted particle takes xp, fp, gp, lq', a rejected one keeps
//                        x, f, g, lq bit for bit
//     smc_control_kernel one workgroup: the mean of a in hmc_adapt_kernel's order (thread i: a[i], a[i + 256], ...; shuffle
//                        tree; (w0 + w1) + (w2 + w3)), the accepted and divergent counts (integers), the histories, and
//                        log eps += adapt_rate (mean a - target_accept), eps = exp(log eps), into device memory, where the
//                        three kernels above read it.  No jitter.
// 4 + n_moves (3 + (n_leapfrog - 1)) launches of this file per stage beside the n_moves n_leapfrog gradient evaluations and
// one start kernel per run.  No floating-point atomics; every sum has a fixed order: two runs with equal arguments return
// equal bits.  Shared with vb_hmc.hip through vb_particles.h: wave_sum and wave_max, the uniforms' pseudo column and the
// divergence threshold of the Metropolis decision, and the host's refusals, row copies and stream guard.  The leapfrog
// kernels are this file's own: the tempered gradient is another formula than vb_hmc.hip's.
//
// Workspace: vb_ctx::smc_work, laid out from scratch by every call -- [state A | state B (each x | g (n x ld) | f | lq (n)) |
// xp | gp | p (n x ld) | fp | H0 | a (n) | flags (n, int) | w | cdf (n) | block totals (64) | anc (n, int64) | loc | scale |
// scale^2 (ld each) | state (16) | beta | log_z | ess hist (max_stages) | accept | step | n_accepted hist (max_stages x
// n_moves) | ancestors hist (max_stages x n, optional)], ld = round_up(d, 16).
// Capacity: n <= 65 536 (one reweight workgroup, 64 scan blocks).
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; scratch 0 and no AGPRs in all):
//     smc_start_kernel:     55 VGPRs, 106 SGPRs, no LDS      -> 7 waves per SIMD (the Box-Muller polynomials)
//     smc_reweight_kernel:  68 VGPRs,  56 SGPRs, 280 B LDS   -> one workgroup of 16 waves
//     smc_scan_kernel:      48 VGPRs,  25 SGPRs, 2 KiB LDS   -> 8 waves per SIMD
//     smc_search_kernel:    24 VGPRs,  50 SGPRs, 520 B LDS   -> 8 waves per SIMD
//     smc_gather_kernel:    18 VGPRs,  30 SGPRs, no LDS      -> 8 waves per SIMD
//     smc_begin_kernel:     93 VGPRs, 106 SGPRs, no LDS      -> 5 waves per SIMD
//     smc_leap_kernel:      26 VGPRs,  27 SGPRs, no LDS      -> 8 waves per SIMD
//     smc_end_kernel:       54 VGPRs,  50 SGPRs, no LDS      -> 8 waves per SIMD
//     smc_control_kernel:   34 VGPRs,  30 SGPRs, 64 B LDS    -> one workgroup
// Measured (tools/smc_bench.py, profiles/smc_bench.json, profiles/smc_kernel_stats.txt; one MI355X, 2 moves of 8 leapfrog steps):
// logistic target, n_data = 16 384, D = 64 -- 5.60 / 18.5 ms per stage at n = 1024 / 4096, sixteen gradient evaluations of
// 0.340 / 1.143 ms, 2.8 % / 1.4 % of a stage outside them (vb_hmc_run's transition in the same process: 1.4 % / 1.1 %);
// multilevel target, D = 117, n = 1024 -- 1.35 ms per stage, 10.4 % outside (vb_hmc_run: 3.9 %).  Reweight 78.7 us (42 dependent
// passes of 1.9 us: latency-bound), scan 5.0, search 5.3, gather 5.0, begin 6.1, leap 5.0, end 5.2, control 4.8 us: reweight +
// resample + gather (94 us) are below one gradient evaluation at the logistic shape and above one (76 us) at the multilevel
// shape.  The numpy loop around vb_model_grad takes 10.95 / 8.81 ms per stage (n = 1024).
#include "vb_particles.h"
#include "vb_rng.h"

namespace vb {

constexpr int64_t kSmcMaxParticles = 65536;
constexpr int kSmcScanPerThread = 4, kSmcScanBlock = 256 * kSmcScanPerThread;      // 1024 weights per scan workgroup
constexpr int kSmcMaxScanBlocks = (int)(kSmcMaxParticles / kSmcScanBlock);         // 64
constexpr int kSmcBisections = 40;

// state[]: what the kernels carry in device memory (SS_BETA and SS_STATUS adjacent: the stage's one fetch);
// SS_LQ_CONST = -sum_j log scale_j - d/2 log 2 pi, formed once on the host
enum SmcState { SS_EPS = 0, SS_LOG_EPS, SS_BETA, SS_STATUS, SS_DELTA, SS_LOG_Z, SS_INC, SS_ESS, SS_NDIV, SS_LQ_CONST, SS_NUM = 16 };

struct SmcParticles {        // one of the two state buffers
  double* x;               // n x ld (pad columns zero)
  double* g;               // n x ld
  double* f;               // n
  double* lq;              // n: log q0(x)
};

// ---- start -----------------------------------------------------------------------------------------------------------------
struct SmcStartArgs {
  SmcParticles s;
  const double *loc, *scale;       // ld (pads zero / one)
  const double* state;
  int64_t ld, n;
  int d;
  uint32_t k0, k1, w;
};

__global__ void __launch_bounds__(256) smc_start_kernel(const SmcStartArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= a.n) return;
  const int64_t row = c * a.ld;
  double acc = 0.0;
  for (int j = lane; 2 * j < a.ld; j += 64) {
    double z[2];
    philox_normal_pair(a.k0, a.k1, (uint64_t)c, (uint32_t)j, a.w, &z[0], &z[1]);
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int col = 2 * j + e;
      double xj = 0.0;
      if (col < a.d) {
        xj = fma(a.scale[col], z[e], a.loc[col]);
        acc = fma(-0.5 * z[e], z[e], acc);
      }
      a.s.x[row + col] = xj;
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) a.s.lq[c] = acc + a.state[SS_LQ_CONST];
}

// ---- reweight ----------------------------------------------------------------------------------------------------------------
struct SmcReweightArgs {
  const double* f;         // n
  const double* lq;        // n, or nullptr: u = f
  double* w;               // n: v = u - max u, then the weights
  double* state;
  double* beta_hist;       // one entry each for this stage, or nullptr
  double* log_z_hist;
  double* ess_hist;
  int64_t n;
  double ess_target;
};

// (sum e^{delta v}, sum e^{2 delta v}) over the particles, broadcast to every thread; optionally the weights stored
template <bool STORE>
__device__ __forceinline__ void smc_weight_sums(double* v, int64_t n, double delta, double (*sh)[16], double* bc, double* s1,
                                                double* s2) {
  const int t = threadIdx.x;
  double a = 0.0, b = 0.0;
  for (int64_t i = t; i < n; i += 1024) {
    const double vi = v[i];
    const double e = vi == -INFINITY ? 0.0 : exp(delta * vi);
    a += e;
    b = fma(e, e, b);
    if (STORE) v[i] = e;
  }
  a = wave_sum(a), b = wave_sum(b);
  __syncthreads();                 // (the last round's readers of bc are done)
  if ((t & 63) == 0) sh[0][t >> 6] = a, sh[1][t >> 6] = b;
  __syncthreads();
  if (t == 0) {
    double x = sh[0][0], y = sh[1][0];
    for (int k = 1; k < 16; ++k) x += sh[0][k], y += sh[1][k];
    bc[0] = x, bc[1] = y;
  }
  __syncthreads();
  *s1 = bc[0], *s2 = bc[1];
}

__global__ void __launch_bounds__(1024) smc_reweight_kernel(const SmcReweightArgs q) {
  __shared__ double sh[2][16];
  __shared__ double bc[2];
  __shared__ int bad_any;
  const int t = threadIdx.x;
  const double nd = (double)q.n;
  if (t == 0) bad_any = 0;
  __syncthreads();
  double m = -INFINITY;
  int bad = 0;
  for (int64_t i = t; i < q.n; i += 1024) {
    const double u = q.lq ? q.f[i] - q.lq[i] : q.f[i];
    bad |= (u != u) || u == INFINITY;
    m = fmax(m, u);
    q.w[i] = u;
  }
  if (bad) bad_any = 1;            // (every writer stores the same value)
  m = wave_max(m);
  if ((t & 63) == 0) sh[0][t >> 6] = m;
  __syncthreads();
  if (t == 0) {
    double x = sh[0][0];
    for (int k = 1; k < 16; ++k) x = fmax(x, sh[0][k]);
    bc[0] = x;
  }
  __syncthreads();
  const double umax = bc[0];
  const int status0 = bad_any ? 1 : (umax == -INFINITY ? 2 : 0);
  const double beta = q.state[SS_BETA];
  if (status0) {                   // nothing to weigh: uniform weights keep the kernels behind this one on defined values
    for (int64_t i = t; i < q.n; i += 1024) q.w[i] = 1.0;
    if (t == 0) q.state[SS_STATUS] = (double)status0;
    return;
  }
  for (int64_t i = t; i < q.n; i += 1024) q.w[i] -= umax;      // (each thread its own elements: no barrier needed)
  double s1, s2;
  const double full = 1.0 - beta;
  smc_weight_sums<false>(q.w, q.n, full, sh, bc, &s1, &s2);
  double delta = full;
  bool last = s1 * s1 / (nd * s2) >= q.ess_target;
  if (!last) {
    double lo = 0.0, hi = full;
    for (int it = 0; it < kSmcBisections; ++it) {
      const double mid = 0.5 * (lo + hi);
      smc_weight_sums<false>(q.w, q.n, mid, sh, bc, &s1, &s2);
      if (s1 * s1 / (nd * s2) >= q.ess_target) lo = mid;
      else hi = mid;
    }
    delta = lo;
  }
  smc_weight_sums<true>(q.w, q.n, delta, sh, bc, &s1, &s2);
  if (t != 0) return;
  const double inc = delta * umax + log(s1 / nd), ess = s1 * s1 / s2;      // ess = n E(delta)
  const double beta_new = last ? 1.0 : beta + delta;
  q.state[SS_STATUS] = delta > 0.0 ? 0.0 : 3.0;
  q.state[SS_BETA] = beta_new;
  q.state[SS_DELTA] = delta;
  q.state[SS_INC] = inc;
  q.state[SS_ESS] = ess;
  q.state[SS_LOG_Z] += inc;
  if (q.beta_hist) *q.beta_hist = beta_new, *q.log_z_hist = inc, *q.ess_hist = ess;
}

// ---- resample: scan, search, gather --------------------------------------------------------------------------------------------
struct SmcResampleArgs {
  const double* w;         // n weights
  double* cdf;             // n: block-local inclusive prefix sums
  double* block_tot;       // kSmcMaxScanBlocks
  long long* anc;          // n
  long long* anc_hist;     // n: this stage's row of the history, or nullptr
  int64_t n;
  int n_blocks;
  int from_stream;         // 1: U from the keys below; 0: `uniform`
  double uniform;
  uint32_t k0, k1, wlo;
};

__global__ void __launch_bounds__(256) smc_scan_kernel(const SmcResampleArgs q) {
  __shared__ double tot[256];
  const int t = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * kSmcScanBlock + (int64_t)t * kSmcScanPerThread;
  double loc[kSmcScanPerThread];
  double run = 0.0;
#pragma unroll
  for (int e = 0; e < kSmcScanPerThread; ++e) {
    run += base + e < q.n ? q.w[base + e] : 0.0;
    loc[e] = run;
  }
  tot[t] = run;
  __syncthreads();
  if (t == 0) {                    // inclusive serial scan of the thread totals, in place
    double s = 0.0;
    for (int k = 0; k < 256; ++k) {
      s += tot[k];
      tot[k] = s;
    }
    q.block_tot[blockIdx.x] = s;
  }
  __syncthreads();
  const double off = t ? tot[t - 1] : 0.0;
#pragma unroll
  for (int e = 0; e < kSmcScanPerThread; ++e)
    if (base + e < q.n) q.cdf[base + e] = off + loc[e];
}

__global__ void __launch_bounds__(256) smc_search_kernel(const SmcResampleArgs q) {
  __shared__ double boff[kSmcMaxScanBlocks + 1];
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int b = 0; b < q.n_blocks; ++b) {
      boff[b] = s;
      s += q.block_tot[b];
    }
    boff[q.n_blocks] = s;
  }
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= q.n) return;
  double U = q.uniform;
  if (q.from_stream) {
    const Philox4 o = philox_sub(~(uint64_t)0, kUniformCol, q.wlo, 0, q.k0, q.k1);
    U = u01(o.z, o.w);
  }
  const double total = boff[q.n_blocks];
  const double ti = ((double)i + U) / (double)q.n;
  int64_t lo = 0, hi = q.n;        // the first j with C_j > t_i
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    const double c = (boff[mid / kSmcScanBlock] + q.cdf[mid]) / total;
    if (c <= ti) lo = mid + 1;
    else hi = mid;
  }
  const long long a = lo < q.n - 1 ? lo : q.n - 1;
  q.anc[i] = a;
  if (q.anc_hist) q.anc_hist[i] = a;
}

struct SmcGatherArgs {
  SmcParticles src, dst;
  const long long* anc;
  int64_t ld, n;
};

__global__ void __launch_bounds__(256) smc_gather_kernel(const SmcGatherArgs q) {
  const int lane = threadIdx.x & 63;
  const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= q.n) return;
  long long a = q.anc[c];
  a = a < 0 ? 0 : (a >= q.n ? q.n - 1 : a);
  const int64_t from = a * q.ld, to = c * q.ld;
  for (int64_t col = lane; col < q.ld; col += 64) {
    q.dst.x[to + col] = q.src.x[from + col];
    q.dst.g[to + col] = q.src.g[from + col];
  }
  if (lane == 0) {
    q.dst.f[c] = q.src.f[a];
    q.dst.lq[c] = q.src.lq[a];
  }
}

// ---- moves: HMC on pi_beta -------------------------------------------------------------------------------------------------------
struct SmcMoveArgs {
  SmcParticles s;          // current state
  double* xp;              // n x ld: proposal
  double* gp;
  double* fp;
  double* p;               // n x ld: momenta
  double* H0;              // n
  double* a;               // n: acceptance probabilities of this transition
  int* flags;              // n: bit 0 accepted, bit 1 divergent
  const double *loc, *scale, *scale2;      // ld each
  double* state;
  int64_t ld, n;
  int d;
};

__global__ void __launch_bounds__(256) smc_begin_kernel(const SmcMoveArgs a, uint32_t k0, uint32_t k1, uint32_t w) {
  const int lane = threadIdx.x & 63;
  const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= a.n) return;
  const double eps = a.state[SS_EPS], half = 0.5 * eps, beta = a.state[SS_BETA], omb = 1.0 - beta;
  const int64_t row = c * a.ld;
  double ke = 0.0;
  for (int j = lane; 2 * j < a.ld; j += 64) {
    double z[2];
    philox_normal_pair(k0, k1, (uint64_t)c, (uint32_t)j, w, &z[0], &z[1]);
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int col = 2 * j + e;
      double pj = 0.0, xj = 0.0;
      if (col < a.d) {
        const double im = a.scale2[col], x0 = a.s.x[row + col];
        pj = z[e] / a.scale[col];
        ke = fma(im * pj, pj, ke);
        const double grad = beta * a.s.g[row + col] - omb * ((x0 - a.loc[col]) / im);
        pj += half * grad;
        xj = x0 + eps * im * pj;
      }
      a.p[row + col] = pj;
      a.xp[row + col] = xj;
    }
  }
  ke = wave_sum(ke);
  if (lane == 0) a.H0[c] = -(beta * a.s.f[c] + omb * a.s.lq[c]) + 0.5 * ke;
}

__global__ void __launch_bounds__(256) smc_leap_kernel(const SmcMoveArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;      // one thread per element of the n x ld matrices
  if (i >= a.n * a.ld) return;
  const int col = (int)(i % a.ld);
  if (col >= a.d) return;                                         // (pad columns stay zero)
  const double eps = a.state[SS_EPS], beta = a.state[SS_BETA];
  const double im = a.scale2[col], xj = a.xp[i];
  const double grad = beta * a.gp[i] - (1.0 - beta) * ((xj - a.loc[col]) / im);
  const double pj = a.p[i] + eps * grad;
  a.p[i] = pj;
  a.xp[i] = xj + eps * im * pj;
}

__global__ void __launch_bounds__(256) smc_end_kernel(const SmcMoveArgs a, uint32_t k0, uint32_t k1, uint32_t w) {
  const int lane = threadIdx.x & 63;
  const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= a.n) return;
  const double half = 0.5 * a.state[SS_EPS], beta = a.state[SS_BETA], omb = 1.0 - beta;
  const int64_t row = c * a.ld;
  double ke = 0.0, lqp = 0.0;
  for (int col = lane; col < a.d; col += 64) {
    const double im = a.scale2[col], sc = a.scale[col], dx = a.xp[row + col] - a.loc[col];
    const double grad = beta * a.gp[row + col] - omb * (dx / im);
    const double pj = a.p[row + col] + half * grad;
    ke = fma(im * pj, pj, ke);
    const double zj = dx / sc;
    lqp = fma(-0.5 * zj, zj, lqp);
  }
  ke = __shfl(wave_sum(ke), 0, 64);
  lqp = __shfl(wave_sum(lqp), 0, 64) + a.state[SS_LQ_CONST];
  const double fprop = a.fp[c];
  const double h0 = a.H0[c], h1 = -(beta * fprop + omb * lqp) + 0.5 * ke;
  const double dh = h0 - h1;
  const bool divergent = !isfinite(dh) || h1 - h0 > kDivergence;
  const Philox4 o = philox_sub((uint64_t)c, kUniformCol, w, 0, k0, k1);
  const bool accept = !divergent && log(u01(o.x, o.y)) < dh;
  if (accept)
    for (int col = lane; col < a.d; col += 64) {
      a.s.x[row + col] = a.xp[row + col];
      a.s.g[row + col] = a.gp[row + col];
    }
  if (lane == 0) {
    if (accept) a.s.f[c] = fprop, a.s.lq[c] = lqp;
    a.a[c] = divergent ? 0.0 : fmin(1.0, exp(dh));
    a.flags[c] = (accept ? 1 : 0) | (divergent ? 2 : 0);
  }
}

struct SmcControlArgs {
  const double* a;         // n
  const int* flags;        // n
  int64_t n;
  double* state;
  double* accept_hist;     // this transition's entries
  double* step_hist;
  long long* n_acc_hist;
  double target, adapt_rate;
};

__global__ void __launch_bounds__(256) smc_control_kernel(const SmcControlArgs q) {
  __shared__ double sh[4];
  __shared__ int cnt[2][4];
  const int t = threadIdx.x;
  double s = 0.0;
  int na = 0, nd = 0;
  for (int64_t c = t; c < q.n; c += 256) {
    s += q.a[c];
    const int fl = q.flags[c];
    na += fl & 1;
    nd += (fl >> 1) & 1;
  }
  s = wave_sum(s);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) na += __shfl_down(na, off, 64), nd += __shfl_down(nd, off, 64);
  if ((t & 63) == 0) sh[t >> 6] = s, cnt[0][t >> 6] = na, cnt[1][t >> 6] = nd;
  __syncthreads();
  if (t != 0) return;
  const double abar = ((sh[0] + sh[1]) + (sh[2] + sh[3])) / (double)q.n;
  *q.accept_hist = abar;
  *q.step_hist = q.state[SS_EPS];
  *q.n_acc_hist = (long long)(cnt[0][0] + cnt[0][1] + cnt[0][2] + cnt[0][3]);
  q.state[SS_NDIV] += (double)(cnt[1][0] + cnt[1][1] + cnt[1][2] + cnt[1][3]);      // (integers below 2^53: exact)
  const double log_eps = q.state[SS_LOG_EPS] + q.adapt_rate * (abar - q.target);
  q.state[SS_LOG_EPS] = log_eps;
  q.state[SS_EPS] = exp(log_eps);
}

// ---- the host side ---------------------------------------------------------------------------------------------------------------
struct SmcLayout {
  int64_t sa, sb, xp, gp, p, fp, h0, a, flags, w, cdf, block_tot, anc, loc, scale, scale2, state;
  int64_t beta_hist, log_z_hist, ess_hist, accept_hist, step_hist, n_acc_hist, anc_hist;
  int64_t zeroed, total, ld, mat;
};

// state buffer: [x | g (mat each) | f | lq (n each)], every piece 256-B aligned
static int64_t smc_state_doubles(int64_t n, int64_t mat) { return 2 * round_up(mat, 32) + 2 * round_up(n, 32); }

static SmcLayout smc_layout(int64_t n, int64_t d, int64_t max_stages, int64_t n_moves, bool keep_anc) {
  SmcLayout o;
  Carver carve;
  const int64_t ld = round_up(d, 16), mat = n * ld, T = max_stages * n_moves;
  o.ld = ld, o.mat = mat;
  o.sa = carve(smc_state_doubles(n, mat)), o.sb = carve(smc_state_doubles(n, mat));
  o.xp = carve(mat), o.gp = carve(mat), o.p = carve(mat), o.fp = carve(n), o.h0 = carve(n), o.a = carve(n);
  o.flags = carve((n + 1) / 2), o.w = carve(n), o.cdf = carve(n), o.block_tot = carve(kSmcMaxScanBlocks), o.anc = carve(n);
  o.loc = carve(ld), o.scale = carve(ld), o.scale2 = carve(ld), o.state = carve(SS_NUM);
  o.beta_hist = carve(max_stages), o.log_z_hist = carve(max_stages), o.ess_hist = carve(max_stages);
  o.accept_hist = carve(T), o.step_hist = carve(T), o.n_acc_hist = carve(T);
  o.zeroed = carve.off;
  o.anc_hist = carve(keep_anc ? max_stages * n : 0);
  o.total = carve.off;
  return o;
}

static SmcParticles smc_particles(double* at, int64_t n, int64_t mat) {
  SmcParticles s;
  s.x = at, s.g = s.x + round_up(mat, 32), s.f = s.g + round_up(mat, 32), s.lq = s.f + round_up(n, 32);
  return s;
}

// reweight, scan and search of one stage on the weights' inputs f (and lq): what vb_smc_run and vb_smc_reweight both enqueue
static int smc_reweight_enqueue(vb_ctx* ctx, double* base, const SmcLayout& o, const double* f, const double* lq, int64_t n,
                                double ess_target, int64_t stage, bool hist, SmcResampleArgs rs) {
  hipStream_t st = ctx->stream;
  SmcReweightArgs rw;
  rw.f = f, rw.lq = lq, rw.w = base + o.w, rw.state = base + o.state, rw.n = n, rw.ess_target = ess_target;
  rw.beta_hist = hist ? base + o.beta_hist + stage : nullptr;
  rw.log_z_hist = hist ? base + o.log_z_hist + stage : nullptr;
  rw.ess_hist = hist ? base + o.ess_hist + stage : nullptr;
  hipLaunchKernelGGL(smc_reweight_kernel, dim3(1), dim3(1024), 0, st, rw);
  VB_HIP(ctx, hipGetLastError());
  rs.w = base + o.w, rs.cdf = base + o.cdf, rs.block_tot = base + o.block_tot, rs.anc = (long long*)(base + o.anc);
  rs.n = n, rs.n_blocks = (int)((n + kSmcScanBlock - 1) / kSmcScanBlock);
  hipLaunchKernelGGL(smc_scan_kernel, dim3((unsigned)rs.n_blocks), dim3(256), 0, st, rs);
  VB_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(smc_search_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, rs);
  VB_HIP(ctx, hipGetLastError());
  return VB_OK;
}

static int smc_status(vb_ctx* ctx, const char* name, double status, double ess_target) {
  if (status == 0.0) return VB_OK;
  if (status == 1.0) return fail(ctx, VB_ERR_NUMERIC, "%s: a log weight f - log q0 is NaN or +inf", name);
  if (status == 2.0) return fail(ctx, VB_ERR_NUMERIC, "%s: every log weight is -inf: the base has no particle on the support", name);
  return fail(ctx, VB_ERR_NUMERIC, "%s: the temperature search ended at delta = 0: fewer than ess_target = %g of the particles "
                                   "carry weight", name, ess_target);
}

static int smc_refuse_common(vb_ctx* ctx, const char* name, int64_t n, double ess_target) {
  if (n <= 0) return fail(ctx, VB_ERR_INVALID, "%s: n must be positive", name);
  if (!(ess_target > 0.0 && ess_target < 1.0)) return fail(ctx, VB_ERR_INVALID, "%s: ess_target must lie in (0, 1)", name);
  return VB_OK;
}

}  // namespace vb

using namespace vb;

extern "C" {

int vb_smc_reweight(vb_ctx* ctx, const double* u, int64_t n, double beta_prev, double ess_target, double uniform,
                    double out[3], int64_t* ancestors) {
  if (!ctx || !u || !out || !ancestors) return fail(ctx, VB_ERR_INVALID, "NULL argument");
  VB_TRY(smc_refuse_common(ctx, "vb_smc_reweight", n, ess_target));
  if (!(beta_prev >= 0.0 && beta_prev < 1.0)) return fail(ctx, VB_ERR_INVALID, "beta_prev must lie in [0, 1)");
  if (!(uniform >= 0.0 && uniform < 1.0)) return fail(ctx, VB_ERR_INVALID, "uniform must lie in [0, 1)");
  if (n > kSmcMaxParticles)
    return fail(ctx, VB_ERR_UNSUPPORTED, "vb_smc_reweight takes at most %lld particles (got %lld)", (long long)kSmcMaxParticles,
                (long long)n);
  VB_HIP(ctx, hipSetDevice(ctx->device));
  VB_TRY(main_stream_write(ctx));
  const SmcLayout o = smc_layout(n, 0, 1, 1, false);      // (no particle matrices: d = 0)
  VB_TRY(ensure(ctx, ctx->smc_work, (size_t)o.total * sizeof(double)));
  double* base = (double*)ctx->smc_work.ptr;
  hipStream_t st = ctx->stream;
  SmcParticles s = smc_particles(base + o.sa, n, o.mat);
  double state[SS_NUM] = {0.0};
  state[SS_BETA] = beta_prev;
  StreamDrain drain{st};
  VB_HIP(ctx, hipMemcpyAsync(base + o.state, state, sizeof(state), hipMemcpyHostToDevice, st));
  VB_HIP(ctx, hipMemcpyAsync(s.f, u, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
  SmcResampleArgs rs{};
  rs.from_stream = 0, rs.uniform = uniform, rs.anc_hist = nullptr;
  VB_TRY(smc_reweight_enqueue(ctx, base, o, s.f, nullptr, n, ess_target, 0, false, rs));
  VB_HIP(ctx, hipMemcpyAsync(state, base + o.state, sizeof(state), hipMemcpyDeviceToHost, st));
  VB_HIP(ctx, hipMemcpyAsync(ancestors, base + o.anc, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  VB_HIP(ctx, hipStreamSynchronize(st));
  VB_TRY(smc_status(ctx, "vb_smc_reweight", state[SS_STATUS], ess_target));
  out[0] = state[SS_BETA], out[1] = state[SS_INC], out[2] = state[SS_ESS];
  return VB_OK;
}

int vb_smc_run(vb_ctx* ctx, const double* loc, const double* scale, int64_t n, int64_t d, double ess_target, int n_moves,
               int n_leapfrog, double step_size, double target_accept, double adapt_rate, int64_t max_stages, uint64_t seed,
               uint64_t stream_offset, double* x, double* logp, double* log_base, double* log_evidence, int64_t* n_stages,
               double* beta_hist, double* log_z_hist, double* ess_hist, double* accept_hist, double* step_hist,
               int64_t* n_accepted_hist, double* final_step, int64_t* n_divergent, int64_t* ancestors_hist) {
  const char* name = "vb_smc_run";
  if (!ctx || !loc || !scale || !x || !logp || !log_base || !log_evidence || !n_stages || !beta_hist || !log_z_hist ||
      !ess_hist || !accept_hist || !step_hist || !n_accepted_hist || !final_step || !n_divergent)
    return fail(ctx, VB_ERR_INVALID, "NULL argument");
  VB_TRY(smc_refuse_common(ctx, name, n, ess_target));
  if (d <= 0 || n_moves <= 0 || n_leapfrog <= 0 || max_stages <= 0)
    return fail(ctx, VB_ERR_INVALID, "d, n_moves, n_leapfrog and max_stages must be positive");
  if (!(step_size > 0.0) || !std::isfinite(step_size)) return fail(ctx, VB_ERR_INVALID, "step_size must be positive and finite");
  if (!(target_accept > 0.0 && target_accept < 1.0)) return fail(ctx, VB_ERR_INVALID, "target_accept must lie in (0, 1)");
  if (!(adapt_rate >= 0.0) || !std::isfinite(adapt_rate)) return fail(ctx, VB_ERR_INVALID, "adapt_rate must be non-negative and finite");
  VB_TRY(model_bound_refuse(ctx, name, "loc", d));
  for (int64_t j = 0; j < d; ++j) {
    if (!std::isfinite(loc[j])) return fail(ctx, VB_ERR_INVALID, "%s: loc[%lld] must be finite", name, (long long)j);
    if (!(scale[j] > 0.0) || !std::isfinite(scale[j]))
      return fail(ctx, VB_ERR_INVALID, "%s: scale[%lld] must be positive and finite", name, (long long)j);
  }
  VB_TRY(model_device_refuse(ctx, name, false, true));
  if (n > kSmcMaxParticles)
    return fail(ctx, VB_ERR_UNSUPPORTED, "%s takes at most %lld particles (got %lld)", name, (long long)kSmcMaxParticles, (long long)n);
  if ((double)n * (double)round_up(d, 16) > 0x1p36 || (double)max_stages * (double)n_moves > 0x1p31 ||
      (double)max_stages * (double)n > 0x1p33)
    return fail(ctx, VB_ERR_UNSUPPORTED, "%s takes at most 2^36 particle coordinates, 2^31 transitions and 2^33 history ancestors", name);

  VB_HIP(ctx, hipSetDevice(ctx->device));
  VB_TRY(main_stream_write(ctx));
  const SmcLayout o = smc_layout(n, d, max_stages, n_moves, ancestors_hist != nullptr);
  VB_TRY(ensure(ctx, ctx->smc_work, (size_t)o.total * sizeof(double)));
  double* base = (double*)ctx->smc_work.ptr;
  hipStream_t st = ctx->stream;
  const int64_t ld = o.ld, T = max_stages * n_moves;
  const uint32_t k0 = (uint32_t)seed, seed_hi = (uint32_t)(seed >> 32);

  // upload: everything but the ancestor history starts from zero (pads, state, histories); loc | scale | scale^2; the state.
  // pack and state are read until the stream is drained: the guard does that on every way out
  std::vector<double> pack((size_t)(3 * round_up(ld, 32)), 0.0);
  const int64_t stride = round_up(ld, 32);
  for (int64_t j = 0; j < ld; ++j) {
    pack[(size_t)j] = j < d ? loc[j] : 0.0;
    pack[(size_t)(stride + j)] = j < d ? scale[j] : 1.0;
    pack[(size_t)(2 * stride + j)] = j < d ? scale[j] * scale[j] : 1.0;
  }
  double state[SS_NUM] = {0.0};
  state[SS_EPS] = step_size, state[SS_LOG_EPS] = log(step_size);
  for (int64_t j = 0; j < d; ++j) state[SS_LQ_CONST] -= log(scale[j]);
  state[SS_LQ_CONST] -= (double)d * kHalfLog2Pi;
  StreamDrain drain{st};
  VB_HIP(ctx, hipMemsetAsync(base, 0, (size_t)o.zeroed * sizeof(double), st));
  VB_HIP(ctx, hipMemcpyAsync(base + o.loc, pack.data(), pack.size() * sizeof(double), hipMemcpyHostToDevice, st));
  VB_HIP(ctx, hipMemcpyAsync(base + o.state, state, sizeof(state), hipMemcpyHostToDevice, st));

  SmcParticles cur = smc_particles(base + o.sa, n, o.mat), other = smc_particles(base + o.sb, n, o.mat);
  const dim3 block(256), row_grid((unsigned)((n + 3) / 4)), leap_grid((unsigned)((n * ld + 255) / 256));
  auto keys = [&](uint64_t s, uint32_t* k1, uint32_t* w) { *k1 = seed_hi ^ (uint32_t)(s >> 32), *w = (uint32_t)s; };

  // start: x and lq from the noise of stream s0, f and g once
  {
    SmcStartArgs sa;
    sa.s = cur, sa.loc = base + o.loc, sa.scale = base + o.scale, sa.state = base + o.state, sa.ld = ld, sa.n = n, sa.d = (int)d, sa.k0 = k0;
    keys(stream_offset, &sa.k1, &sa.w);
    hipLaunchKernelGGL(smc_start_kernel, row_grid, block, 0, st, sa);
    VB_HIP(ctx, hipGetLastError());
    VB_TRY(model_grad_rows(ctx, cur.x, ld, n, d, cur.g, cur.f));
  }

  SmcMoveArgs mv;
  mv.xp = base + o.xp, mv.gp = base + o.gp, mv.fp = base + o.fp, mv.p = base + o.p, mv.H0 = base + o.h0, mv.a = base + o.a;
  mv.flags = (int*)(base + o.flags), mv.loc = base + o.loc, mv.scale = base + o.scale, mv.scale2 = base + o.scale2;
  mv.state = base + o.state, mv.ld = ld, mv.n = n, mv.d = (int)d;
  SmcControlArgs cq;
  cq.a = mv.a, cq.flags = mv.flags, cq.n = n, cq.state = mv.state, cq.target = target_accept, cq.adapt_rate = adapt_rate;

  int64_t stages = 0;
  double beta = 0.0;
  while (beta < 1.0) {
    if (stages == max_stages)
      return fail(ctx, VB_ERR_NUMERIC, "%s: beta = %.6g after max_stages = %lld stages", name, beta, (long long)max_stages);
    const int64_t k = stages;                      // 0-based stage index
    const uint64_t s_first = stream_offset + 1 + (uint64_t)k * (uint64_t)n_moves;
    SmcResampleArgs rs{};
    rs.from_stream = 1, rs.uniform = 0.0, rs.k0 = k0;
    keys(s_first, &rs.k1, &rs.wlo);
    rs.anc_hist = ancestors_hist ? (long long*)(base + o.anc_hist) + k * n : nullptr;
    VB_TRY(smc_reweight_enqueue(ctx, base, o, cur.f, cur.lq, n, ess_target, k, true, rs));
    SmcGatherArgs ga;
    ga.src = cur, ga.dst = other, ga.anc = (const long long*)(base + o.anc), ga.ld = ld, ga.n = n;
    hipLaunchKernelGGL(smc_gather_kernel, row_grid, block, 0, st, ga);
    VB_HIP(ctx, hipGetLastError());
    std::swap(cur, other);
    double got[2] = {0.0, 0.0};                    // beta, status: adjacent state slots
    const FetchSeg seg{base + o.state + SS_BETA, 2 * sizeof(double), got};
    VB_TRY(fetch_blocking(ctx, st, &seg, 1));
    VB_TRY(smc_status(ctx, name, got[1], ess_target));
    if (!(got[0] > beta && got[0] <= 1.0))
      return fail(ctx, VB_ERR_NUMERIC, "%s: the device moved beta from %.17g to %.17g", name, beta, got[0]);
    beta = got[0];
    ++stages;
    mv.s = cur;
    for (int j = 0; j < n_moves; ++j) {
      uint32_t k1, w;
      keys(s_first + (uint64_t)j, &k1, &w);
      hipLaunchKernelGGL(smc_begin_kernel, row_grid, block, 0, st, mv, k0, k1, w);
      VB_HIP(ctx, hipGetLastError());
      for (int l = 0; l < n_leapfrog; ++l) {
        if (l > 0) {
          hipLaunchKernelGGL(smc_leap_kernel, leap_grid, block, 0, st, mv);
          VB_HIP(ctx, hipGetLastError());
        }
        VB_TRY(model_grad_rows(ctx, mv.xp, ld, n, d, mv.gp, mv.fp));
      }
      hipLaunchKernelGGL(smc_end_kernel, row_grid, block, 0, st, mv, k0, k1, w);
      VB_HIP(ctx, hipGetLastError());
      const int64_t idx = k * n_moves + j;
      cq.accept_hist = base + o.accept_hist + idx, cq.step_hist = base + o.step_hist + idx;
      cq.n_acc_hist = (long long*)(base + o.n_acc_hist) + idx;
      hipLaunchKernelGGL(smc_control_kernel, dim3(1), block, 0, st, cq);
      VB_HIP(ctx, hipGetLastError());
    }
  }

  // download: the run's one other synchronisation
  const size_t W = sizeof(double);
  VB_HIP(ctx, download_rows(ctx, x, cur.x, n, d, ld));
  VB_HIP(ctx, hipMemcpyAsync(logp, cur.f, (size_t)n * W, hipMemcpyDeviceToHost, st));
  VB_HIP(ctx, hipMemcpyAsync(log_base, cur.lq, (size_t)n * W, hipMemcpyDeviceToHost, st));
  VB_HIP(ctx, hipMemcpyAsync(beta_hist, base + o.beta_hist, (size_t)max_stages * W, hipMemcpyDeviceToHost, st));
  VB_HIP(ctx, hipMemcpyAsync(log_z_hist, base + o.log_z_hist, (size_t)max_stages * W, hipMemcpyDeviceToHost, st));
  VB_HIP(ctx, hipMemcpyAsync(ess_hist, base + o.ess_hist, (size_t)max_stages * W, hipMemcpyDeviceToHost, st));
  VB_HIP(ctx, hipMemcpyAsync(accept_hist, base + o.accept_hist, (size_t)T * W, hipMemcpyDeviceToHost, st));
  VB_HIP(ctx, hipMemcpyAsync(step_hist, base + o.step_hist, (size_t)T * W, hipMemcpyDeviceToHost, st));
  VB_HIP(ctx, hipMemcpyAsync(n_accepted_hist, base + o.n_acc_hist, (size_t)T * W, hipMemcpyDeviceToHost, st));
  if (ancestors_hist)
    VB_HIP(ctx, hipMemcpyAsync(ancestors_hist, base + o.anc_hist, (size_t)(stages * n) * W, hipMemcpyDeviceToHost, st));
  VB_HIP(ctx, hipMemcpyAsync(state, base + o.state, sizeof(state), hipMemcpyDeviceToHost, st));
  VB_HIP(ctx, hipStreamSynchronize(st));
  *log_evidence = state[SS_LOG_Z];
  *n_stages = stages;
  *final_step = state[SS_EPS];
  *n_divergent = (int64_t)state[SS_NDIV];
  if (!std::isfinite(*log_evidence)) return fail(ctx, VB_ERR_NUMERIC, "%s: the log evidence is not finite", name);
  return VB_OK;
}

}  // extern "C"
