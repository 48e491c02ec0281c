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

__global__ void __launch_bounds__(256) hmc_begin_kernel(const HmcArgs a, uint32_t k0, uint32_t k1, uint32_t w) {
  const int lane = threadIdx.x & 63;
  const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= a.n_chains) return;
  const double eps = a.state[HS_EPS], half = 0.5 * eps;
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

__global__ void __launch_bounds__(256) hmc_end_kernel(const HmcArgs a, const HmcEndArgs e) {
  const int lane = threadIdx.x & 63;
  const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= a.n_chains) return;
  const double half = 0.5 * a.state[HS_EPS];
  const int64_t row = c * a.ld;
  double ke = 0.0;
  for (int col = lane; col < a.d; col += 64) {
    const double pj = a.p[row + col] + half * a.gp[row + col];
    ke = fma(a.inv_mass[col] * pj, pj, ke);
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
  if (thin < 1) return fail(ctx, VB_ERR_INVALID, "thin must be at least 1");
  if (n_leapfrog < 1) return fail(ctx, VB_ERR_INVALID, "n_leapfrog must be at least 1");
  if (!(step_size > 0.0) || !std::isfinite(step_size)) return fail(ctx, VB_ERR_INVALID, "step_size must be positive and finite");
  if (!(target_accept > 0.0 && target_accept < 1.0)) return fail(ctx, VB_ERR_INVALID, "target_accept must lie in (0, 1)");
  if (!(jitter >= 0.0 && jitter < 1.0)) return fail(ctx, VB_ERR_INVALID, "jitter must lie in [0, 1)");
  const ModelDev& m = ctx->model;
  if (m.id < 0) return fail(ctx, VB_ERR_STATE, "no model bound (vb_set_model)");
  if (d != m.dim) return fail(ctx, VB_ERR_INVALID, "x0 has %lld columns, model dimension is %d", (long long)d, m.dim);
  for (int64_t j = 0; j < d; ++j)
    if (!(inv_mass[j] > 0.0) || !std::isfinite(inv_mass[j]))
      return fail(ctx, VB_ERR_INVALID, "inv_mass[%lld] must be positive and finite", (long long)j);
  if (m.id == VB_MODEL_SOURCE && ctx->user_host_fn)
    return fail(ctx, VB_ERR_UNSUPPORTED, "vb_hmc_run runs without host synchronisation: a host-callback model cannot be its "
                                         "target (write the density as a source model)");
  if (ctx->comm) return fail(ctx, VB_ERR_UNSUPPORTED, "vb_hmc_run runs on one process's engine: detach the communicator");
  const int64_t n_iter = n_warmup + n_draws, n_kept = (n_draws + thin - 1) / thin;
  if (n_chains > ((int64_t)1 << 31) - 8 || n_iter > ((int64_t)1 << 40) || (double)n_chains * (double)round_up(d, 16) > 0x1p36)
    return fail(ctx, VB_ERR_UNSUPPORTED, "vb_hmc_run takes at most 2^31 - 8 chains, 2^36 chain coordinates (n_chains x "
                                         "round_up(d, 16)) and 2^40 iterations");
  if (draws && (double)n_kept * (double)n_chains * (double)d * sizeof(double) > (double)kHmcDrawBudgetBytes)
    return fail(ctx, VB_ERR_UNSUPPORTED, "the kept draws (%lld x %lld x %lld doubles) exceed the device draw buffer's budget of "
                                         "%lld bytes: raise thin or pass no draws",
                (long long)n_kept, (long long)n_chains, (long long)d, (long long)kHmcDrawBudgetBytes);
  VB_HIP(ctx, hipSetDevice(ctx->device));
  VB_TRY(main_stream_write(ctx));
  hipStream_t st = ctx->stream;
  const int64_t C = n_chains, ld = round_up(d, 16), mat = C * ld;
  Carver carve;
  const int64_t o_x = carve(mat), o_g = carve(mat), o_xp = carve(mat), o_gp = carve(mat), o_p = carve(mat),
                o_mean = carve(mat), o_m2 = carve(mat), o_f = carve(C), o_fp = carve(C), o_h0 = carve(C), o_a = carve(C),
                o_cnt = carve(C), o_im = carve(ld), o_state = carve(HS_NUM), o_sh = carve(n_iter), o_ah = carve(n_iter),
                o_div = carve(C), o_draws = carve(draws ? n_kept * C * d : 0), o_logp = carve(logp ? n_kept * C : 0);
  VB_TRY(ensure(ctx, ctx->hmc_work, (size_t)carve.off * sizeof(double)));
  double* base = (double*)ctx->hmc_work.ptr;
  // everything up to the draws starts from zero: pad columns, Welford sums, counts, state
  VB_HIP(ctx, hipMemsetAsync(base, 0, (size_t)o_draws * sizeof(double), st));
  VB_HIP(ctx, hipMemcpy2DAsync(base + o_x, (size_t)ld * sizeof(double), x0, (size_t)d * sizeof(double),
                               (size_t)d * sizeof(double), (size_t)C, hipMemcpyHostToDevice, st));
  VB_HIP(ctx, hipMemcpyAsync(base + o_im, inv_mass, (size_t)d * sizeof(double), hipMemcpyHostToDevice, st));
  HmcArgs a;
  a.x = base + o_x, a.g = base + o_g, a.f = base + o_f, a.xp = base + o_xp, a.gp = base + o_gp, a.fp = base + o_fp;
  a.p = base + o_p, a.H0 = base + o_h0, a.a = base + o_a, a.mean = base + o_mean, a.m2 = base + o_m2;
  a.count = base + o_cnt, a.n_div = (long long*)(base + o_div), a.inv_mass = base + o_im, a.state = base + o_state;
  a.ld = ld, a.n_chains = C, a.d = (int)d;
  VB_TRY(model_grad_rows(ctx, a.x, ld, C, d, a.g, a.f));      // f, g of the start: carried from here on

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
      hipLaunchKernelGGL(hmc_begin_kernel, chain_grid, block, 0, st, a, k0, k1, w);
      VB_HIP(ctx, hipGetLastError());
      for (int l = 0; l < n_leapfrog; ++l) {
        VB_TRY(model_grad_rows(ctx, a.xp, ld, C, d, a.gp, a.fp));
        if (l + 1 == n_leapfrog) break;
        hipLaunchKernelGGL(hmc_leap_kernel, leap_grid, block, 0, st, a);
        VB_HIP(ctx, hipGetLastError());
      }
      HmcEndArgs e;
      e.k0 = k0, e.k1 = k1, e.w = w;
      const int64_t si = t - n_warmup;
      e.sampling = si >= 0, e.k = (double)(si + 1);
      const bool keep = si >= 0 && si % thin == 0;
      e.draw_row = keep && draws ? base + o_draws + (si / thin) * C * d : nullptr;
      e.logp_row = keep && logp ? base + o_logp + (si / thin) * C : nullptr;
      hipLaunchKernelGGL(hmc_end_kernel, chain_grid, block, 0, st, a, e);
      VB_HIP(ctx, hipGetLastError());
    }
    const uint64_t sn = stream_offset + (uint64_t)(t + 1);
    q.t = t, q.k1_next = seed_hi ^ (uint32_t)(sn >> 32), q.w_next = (uint32_t)sn;
    hipLaunchKernelGGL(hmc_adapt_kernel, dim3(1), block, 0, st, q);
    VB_HIP(ctx, hipGetLastError());
  }

  // the one synchronisation: download
  const size_t row_bytes = (size_t)d * sizeof(double), ld_bytes = (size_t)ld * sizeof(double);
  VB_HIP(ctx, hipMemcpy2DAsync(last_x, row_bytes, a.x, ld_bytes, row_bytes, (size_t)C, hipMemcpyDeviceToHost, st));
  VB_HIP(ctx, hipMemcpy2DAsync(chain_mean, row_bytes, a.mean, ld_bytes, row_bytes, (size_t)C, hipMemcpyDeviceToHost, st));
  VB_HIP(ctx, hipMemcpy2DAsync(chain_m2, row_bytes, a.m2, ld_bytes, row_bytes, (size_t)C, hipMemcpyDeviceToHost, st));
  VB_HIP(ctx, hipMemcpyAsync(accept_rate, a.count, (size_t)C * sizeof(double), hipMemcpyDeviceToHost, st));
  VB_HIP(ctx, hipMemcpyAsync(step_hist, base + o_sh, (size_t)n_iter * sizeof(double), hipMemcpyDeviceToHost, st));
  VB_HIP(ctx, hipMemcpyAsync(accept_hist, base + o_ah, (size_t)n_iter * sizeof(double), hipMemcpyDeviceToHost, st));
  VB_HIP(ctx, hipMemcpyAsync(final_step, a.state + HS_BASE, sizeof(double), hipMemcpyDeviceToHost, st));
  if (draws)
    VB_HIP(ctx, hipMemcpyAsync(draws, base + o_draws, (size_t)(n_kept * C * d) * sizeof(double), hipMemcpyDeviceToHost, st));
  if (logp) VB_HIP(ctx, hipMemcpyAsync(logp, base + o_logp, (size_t)(n_kept * C) * sizeof(double), hipMemcpyDeviceToHost, st));
  std::vector<long long> div((size_t)C);
  VB_HIP(ctx, hipMemcpyAsync(div.data(), a.n_div, (size_t)C * sizeof(long long), hipMemcpyDeviceToHost, st));
  VB_HIP(ctx, hipStreamSynchronize(st));
  int64_t total = 0;
  for (int64_t c = 0; c < C; ++c) {
    total += div[(size_t)c];
    accept_rate[c] /= (double)n_draws;
  }
  *n_divergent = total;
  return VB_OK;
}

}  // extern "C"
