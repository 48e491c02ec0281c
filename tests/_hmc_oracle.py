"""Host reference of ``hmc`` / ``vb_hmc_run``: the algorithm as the feature's specification states it, in numpy.

TEST INFRASTRUCTURE ONLY.  Written from the specification (DESIGN.md 4.22 restates it), not from the device code: many
chains in lock-step over a ``value_and_grad(x) -> (f (C,), g (C, D))`` callable, a diagonal metric, ``L`` leapfrog steps
per transition, one jittered step size per iteration, Nesterov dual averaging (Hoffman & Gelman 2014, Algorithm 5) on the
chains' mean acceptance during warm-up.  The per-iteration standard normals are GIVEN (an array ``(T, C, D)`` or a
callable ``t -> (C, D)``); the accept uniforms ``u`` and the jitter uniform ``v_t`` are computed from their definition
with ``_philox_oracle.philox4x32_10`` and ``_u53`` -- integer operations and one exact fp64 scaling.

``perturb`` (a ``RandomState``) adds noise to every model value (size ``1e-12 max|f|``) and every gradient (size
``1e-11 max|g|``): the bounds the project's model tests hold the device to.  What that noise changes in an output is the
yardstick for comparing the device run with this one.
"""
import numpy as np

from _philox_oracle import _keys, _u53, philox4x32_10

UNIFORM_COL = 0xFFFFFFFE
GAMMA, T0, KAPPA = 0.05, 10.0, 0.75
DIVERGENCE = 1000.0
F_NOISE, G_NOISE = 1e-12, 1e-11


def uniforms(seed, stream, n_chains):
    """``(u (C,), v)`` of Philox stream ``stream``: u of chain c from words (0, 1) of the call with counter
    ``(c_lo, c_hi, 0xFFFFFFFE, stream_lo)`` (sub-stream 0), v from words (2, 3) of the call with row ``2^64 - 1``."""
    k0, k1, w = _keys(seed, stream)
    c = np.arange(n_chains, dtype=np.uint64)
    o = philox4x32_10(c & np.uint64(0xFFFFFFFF), c >> np.uint64(32), UNIFORM_COL, w, k0, k1)
    u = _u53(o[0], o[1])
    q = philox4x32_10(np.uint64(0xFFFFFFFF), np.uint64(0xFFFFFFFF), UNIFORM_COL, w, k0, k1)
    v = float(_u53(np.atleast_1d(q[2]), np.atleast_1d(q[3]))[0])
    return u, v


def perturbed(value_and_grad, rng):
    """``value_and_grad`` with the perturbation hook: uniform noise of the stated sizes on every value and gradient."""
    if rng is None:
        return value_and_grad

    def fn(x):
        f, g = value_and_grad(x)
        f, g = np.array(f, dtype=np.float64), np.array(g, dtype=np.float64)
        with np.errstate(invalid='ignore'):
            fmax = np.max(np.abs(f[np.isfinite(f)])) if np.any(np.isfinite(f)) else 0.0
            gmax = np.max(np.abs(g[np.isfinite(g)])) if np.any(np.isfinite(g)) else 0.0
            f = f + F_NOISE * fmax * rng.uniform(-1.0, 1.0, f.shape)
            g = g + G_NOISE * gmax * rng.uniform(-1.0, 1.0, g.shape)
        return f, g
    return fn


def trajectory(value_and_grad, x, p, g, eps, n_leapfrog, inv_mass):
    """``L`` leapfrog steps from ``(x, p)`` with gradient ``g`` at ``x``: ``(x, p, f, g)`` at the end."""
    x, p = np.array(x, dtype=np.float64), np.array(p, dtype=np.float64)
    f = None
    with np.errstate(all='ignore'):
        p = p + 0.5 * eps * g
        for l in range(n_leapfrog):
            x = x + eps * inv_mass * p
            f, g = value_and_grad(x)
            p = p + (0.5 * eps if l + 1 == n_leapfrog else eps) * g
    return x, p, f, g


def energy(f, p, inv_mass):
    with np.errstate(all='ignore'):
        return -f + 0.5 * np.sum(inv_mass * p * p, axis=-1)


def run(value_and_grad, x0, normals, *, inv_mass=None, n_warmup=0, n_draws=1, n_leapfrog=1, step_size=1.0,
        target_accept=0.8, jitter=0.0, seed=1, stream_offset=0, thin=1, perturb=None):
    """The whole run.  Returns the dict ``hmc`` returns (without the printed summary) plus ``accepted`` and ``divergent``
    (T x C booleans), ``a`` (T x C) and ``min_margin``, the smallest ``|log u - dH|`` over the non-divergent proposals."""
    vg = perturbed(value_and_grad, perturb)
    x = np.array(x0, dtype=np.float64)
    n_chains, d = x.shape
    inv_mass = np.ones(d) if inv_mass is None else np.asarray(inv_mass, dtype=np.float64)
    n_iter = n_warmup + n_draws
    f, g = vg(x)
    f, g = np.array(f, dtype=np.float64), np.array(g, dtype=np.float64)
    mu = np.log(10.0 * step_size)
    hbar, log_eps_bar, base = 0.0, 0.0, float(step_size)
    step_hist, accept_hist = np.empty(n_iter), np.empty(n_iter)
    accepted, divergent = np.zeros((n_iter, n_chains), dtype=bool), np.zeros((n_iter, n_chains), dtype=bool)
    a_all = np.empty((n_iter, n_chains))
    draws, logp = [], []
    mean, m2, count, n_div = np.zeros((n_chains, d)), np.zeros((n_chains, d)), np.zeros(n_chains), 0
    min_margin = np.inf
    for t in range(n_iter):
        s = stream_offset + t
        u, v = uniforms(seed, s, n_chains)
        eps = base * (1.0 + jitter * (2.0 * v - 1.0))
        step_hist[t] = eps
        z = np.asarray(normals(t) if callable(normals) else normals[t], dtype=np.float64)
        p = z / np.sqrt(inv_mass)
        h0 = energy(f, p, inv_mass)
        xp, pp, fp, gp = trajectory(vg, x, p, g, eps, n_leapfrog, inv_mass)
        h1 = energy(fp, pp, inv_mass)
        with np.errstate(all='ignore'):
            dh = h0 - h1
            div = ~np.isfinite(dh) | (h1 - h0 > DIVERGENCE)
            a = np.where(div, 0.0, np.minimum(1.0, np.exp(np.where(div, 0.0, dh))))
            log_u = np.log(u)
            acc = ~div & (log_u < dh)
            if np.any(~div):
                min_margin = min(min_margin, float(np.min(np.abs(log_u - dh)[~div])))
        x = np.where(acc[:, None], xp, x)
        g = np.where(acc[:, None], gp, g)
        f = np.where(acc, fp, f)
        accepted[t], divergent[t], a_all[t] = acc, div, a
        abar = a.sum() / n_chains
        accept_hist[t] = abar
        if t < n_warmup:
            m = t + 1.0
            hbar = (1.0 - 1.0 / (m + T0)) * hbar + (target_accept - abar) / (m + T0)
            log_eps = mu - np.sqrt(m) / GAMMA * hbar
            eta = m ** -KAPPA
            log_eps_bar = eta * log_eps + (1.0 - eta) * log_eps_bar
            base = float(np.exp(log_eps) if t + 1 < n_warmup else np.exp(log_eps_bar))
        else:
            k = t - n_warmup + 1.0
            delta = x - mean
            mean = mean + delta / k
            m2 = m2 + delta * (x - mean)
            count += acc
            n_div += int(div.sum())
            if (t - n_warmup) % thin == 0:
                draws.append(x.copy())
                logp.append(f.copy())
    with np.errstate(all='ignore'):
        chain_var = m2 / (n_draws - 1.0) if n_draws > 1 else np.full_like(m2, np.nan)
    return dict(draws=np.array(draws), logp=np.array(logp), last=x, chain_mean=mean, chain_var=chain_var,
                accept_rate=count / n_draws, accept_prob=accept_hist, step_size_history=step_hist, step_size=base,
                n_divergent=n_div, accepted=accepted, divergent=divergent, a=a_all, min_margin=min_margin,
                next_stream=stream_offset + n_iter)


def philox_normals(seed, stream_offset, n_chains, d):
    """``t -> (C, D)`` standard normals of stream ``stream_offset + t`` from the host Philox reference (fp64 roundings of the
    long-double values: within an ulp or two of the device's, good for the statistical tests that have no device)."""
    from _philox_oracle import normals

    def fn(t):
        return normals(seed, stream_offset + t, 0, n_chains, d)[0].astype(np.float64)
    return fn


# ---- the cases the CPU and the GPU tests share --------------------------------------------------------------------------------
# Host models (``logp`` / ``grad`` on rows) of the parity grid, and the two configurations of the statistical test.  Every
# input is a function of the case alone, so the CPU test that vets the seeds and the GPU test that uses them see the same
# numbers.
QUARTIC_SRC = r'''
__device__ double vb_log_density(const double* z, int d, const double* params, double* grad) {
  double f = 0.0;
  for (int j = 0; j < d; ++j) {
    const double a = params[j], x = z[j];
    f -= 0.5 * a * x * x + 0.05 * x * x * x * x;
    if (grad) grad[j] = -a * x - 0.2 * x * x * x;
  }
  return f;
}
'''


class Quartic:
    """``f(x) = -sum_j (a_j x_j^2 / 2 + x_j^4 / 20)``: the host side of the parity grid's source model."""

    def __init__(self, a):
        self.a = np.asarray(a, dtype=np.float64)
        self.dim = self.a.size

    def logp(self, x):
        return -np.sum(0.5 * self.a * x * x + 0.05 * x ** 4, axis=1)

    def grad(self, x):
        return -self.a * x - 0.2 * x ** 3


def value_and_grad_of(host_model):
    def fn(x):
        with np.errstate(all='ignore'):
            return host_model.logp(x), host_model.grad(x)
    return fn


PARITY_MODELS = ('gauss', 'funnel', 'corr', 'logistic', 'softmax', 'source')
PARITY_CHAINS = (1, 4, 5, 9, 64, 257)
PARITY_WARMUP, PARITY_DRAWS = 3, 4
LOGISTIC_N, SOFTMAX_CLASSES, SOFTMAX_P = 33, 3, 2
PARITY_PRIOR_SD = 3.0
# seeds moved off a case whose accept test came closer than MIN_MARGIN on the host (tests/test_hmc_cpu.py vets every case)
MIN_MARGIN = 1e-6
RESEED = {}


def parity_dims(kind):
    if kind == 'softmax':
        return (SOFTMAX_CLASSES * SOFTMAX_P,)
    if kind == 'funnel':
        return (2, 17)                      # (a funnel has a scale coordinate and at least one other)
    return (1, 2, 17)


def parity_problem(kind, d):
    """``(host model, spec)``: the numpy side, and what the GPU test builds the device model from."""
    from oracle import models as omod
    rng = np.random.RandomState(100 * PARITY_MODELS.index(kind) + d)
    if kind == 'gauss':
        mean, sd = rng.randn(d), np.exp(0.3 * rng.randn(d))
        return omod.GaussDiag(mean, sd), dict(mean=mean, sd=sd)
    if kind == 'funnel':
        return omod.Funnel(d), dict()
    if kind == 'corr':
        a = rng.randn(d, d)
        cov = a @ a.T / d + np.eye(d)
        mean = rng.randn(d)
        return omod.GaussFull(mean, np.linalg.inv(cov)), dict(mean=mean, cov=cov)
    if kind == 'logistic':
        X = rng.randn(LOGISTIC_N, d)
        y = (rng.rand(LOGISTIC_N) < 0.5).astype(np.float64)
        return omod.Logistic(X, y, PARITY_PRIOR_SD), dict(X=X, y=y)
    if kind == 'softmax':
        from _softmax_oracle import SoftmaxOracle
        X = rng.randn(LOGISTIC_N, SOFTMAX_P)
        y = rng.randint(SOFTMAX_CLASSES, size=LOGISTIC_N)
        return SoftmaxOracle(X, y, SOFTMAX_CLASSES, PARITY_PRIOR_SD), dict(X=X, y=y)
    a = np.exp(0.3 * rng.randn(d))
    return Quartic(a), dict(a=a)


def parity_cases(kind, n_chains):
    """Every (d, L, thin, jitter) of the grid for one model and chain count, each with its inputs: dicts with ``d``,
    ``n_leapfrog``, ``thin``, ``jitter``, ``seed``, ``x0``, ``inv_mass``, ``step_size``."""
    out = []
    for d in parity_dims(kind):
        for n_leapfrog in (1, 3):
            for thin in (1, 3):
                for jitter in (0.0, 0.2):
                    idx = len(out)
                    key = (kind, n_chains, idx)
                    seed = RESEED.get(key, 10000 * PARITY_MODELS.index(kind) + 100 * PARITY_CHAINS.index(n_chains) + idx + 1)
                    rng = np.random.RandomState(seed)
                    scale = 0.5 if kind == 'funnel' else 1.0
                    out.append(dict(key=key, d=d, n_leapfrog=n_leapfrog, thin=thin, jitter=jitter, seed=seed,
                                    x0=scale * rng.randn(n_chains, d), inv_mass=np.exp(0.2 * rng.randn(d)),
                                    step_size=0.4 * d ** -0.25, stream_offset=3))
    return out


def run_case(host_model, case, normals, perturb=None, **override):
    kw = dict(inv_mass=case['inv_mass'], n_warmup=PARITY_WARMUP, n_draws=PARITY_DRAWS, n_leapfrog=case['n_leapfrog'],
              step_size=case['step_size'], target_accept=0.8, jitter=case['jitter'], seed=case['seed'],
              stream_offset=case['stream_offset'], thin=case['thin'], perturb=perturb)
    kw.update(override)
    return run(value_and_grad_of(host_model), case['x0'], normals, **kw)


STAT_CHAINS, STAT_WARMUP, STAT_DRAWS, STAT_LEAPFROG, STAT_SEED = 64, 150, 100, 8, 11


def stat_config(name):
    """The two configurations of the statistical test: ``(host model, exact mean, exact covariance, inv_mass, start,
    spec)``.  (a) a diagonal Gaussian, D = 16; (b) the linear regression of ``_loo_oracle.linear_problem``, D = 8."""
    from oracle import models as omod
    rng = np.random.RandomState(5 if name == 'a' else 6)
    if name == 'a':
        mean, sd = rng.randn(16), np.exp(rng.randn(16))
        start = mean + 3.0 * sd * rng.randn(STAT_CHAINS, 16)
        return omod.GaussDiag(mean, sd), mean, np.diag(sd ** 2), sd ** 2, start, dict(mean=mean, sd=sd)
    import _loo_oracle as LO
    X, y, prior_sd, noise_sd, _ = LO.linear_problem(1)
    pm, pv = LO.linear_posterior(X, y, prior_sd, noise_sd)
    start = pm + 2.0 * rng.randn(STAT_CHAINS, 8) @ np.linalg.cholesky(pv).T
    return (omod.LinearRegression(X, y, prior_sd, noise_sd), pm, pv, np.diag(pv).copy(), start,
            dict(X=X, y=y, prior_sd=prior_sd, noise_sd=noise_sd))


def combine_chains(chain_mean, chain_var, n):
    """``(mean, sd, rhat)`` as the specification defines them, in plain numpy."""
    w = chain_var.mean(axis=0)
    b = n * chain_mean.var(axis=0, ddof=1)
    var_plus = (n - 1.0) / n * w + b / n
    return chain_mean.mean(axis=0), np.sqrt(var_plus), np.sqrt(var_plus / w)


def stat_conditions(name, res, exact_mean, exact_cov):
    """The figures of the statistical test and whether each holds: ``{label: (value, bound, ok)}``.  ``res`` has ``mean``,
    ``sd``, ``rhat``, ``draws`` (n_kept x C x D), ``accept_rate`` and ``n_divergent``."""
    exact_sd = np.sqrt(np.diag(exact_cov))
    out = {}
    v = float(np.max(np.abs(res['mean'] - exact_mean) / exact_sd))
    out['mean error / sd'] = (v, 0.15, v <= 0.15)
    if name == 'a':
        v = float(np.max(np.abs(res['sd'] / exact_sd - 1.0)))
        out['sd ratio error'] = (v, 0.15, v <= 0.15)
    else:
        flat = res['draws'].reshape(-1, exact_mean.size)
        v = float(np.max(np.abs(np.cov(flat.T) - exact_cov)) / np.max(np.diag(exact_cov)))
        out['covariance error'] = (v, 0.25, v <= 0.25)
    v = float(np.max(res['rhat']))
    out['max rhat'] = (v, 1.05, v <= 1.05)
    v = float(np.mean(res['accept_rate']))
    out['sampling acceptance'] = (v, (0.65, 0.95), 0.65 <= v <= 0.95)
    out['n_divergent'] = (int(res['n_divergent']), 0, int(res['n_divergent']) == 0)
    return out
