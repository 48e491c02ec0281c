"""Host reference of ``hmc(..., metric=, adapt_metric=)`` / ``vb_hmc_run_metric``: the dense-metric transition, the window
moments and the adaptive driver as the feature's specification states them (DESIGN.md 4.22 restates it), in numpy.

TEST INFRASTRUCTURE ONLY.  Written from the specification, not from the device code.  Dense metric: ``Sigma = L L'`` is the
inverse mass; in whitened momenta ``r`` (``p = L^-T r``) an iteration draws ``r = z`` (the stream's normals, unscaled), has
``H = -f + 1/2 sum r^2``, kicks ``r += c eps (g L)`` and drifts ``x += eps (r L')``.  Everything else -- the uniforms, the
divergence rule, the accept test, Welford, the kept draws, dual averaging -- is ``_hmc_oracle``'s, whose pieces
(``uniforms``, ``perturbed``, the case models, the constants) are imported.  A call may have no sampling phase
(``n_draws = 0``) and may return the moments of its own iterations about a given shift.
"""
import numpy as np

import _hmc_oracle as HO
from _hmc_oracle import DIVERGENCE, GAMMA, KAPPA, T0, perturbed, uniforms


def run(value_and_grad, x0, normals, *, L=None, inv_mass=None, n_warmup=0, n_draws=1, n_leapfrog=1, step_size=1.0,
        target_accept=0.8, jitter=0.0, seed=1, stream_offset=0, thin=1, perturb=None, moment_shift=None, t0=0):
    """One engine call.  ``L`` (D x D, lower) selects the dense metric, ``inv_mass`` (D,) the diagonal one.  ``normals`` is an
    array indexed ``[t0 + t]`` or a callable of ``t0 + t``.  Returns what ``_hmc_oracle.run`` returns plus ``moment_sum`` and
    ``moment_m2`` (None without ``moment_shift``); with ``n_draws = 0`` the sampling outputs are empty / None."""
    assert (L is None) != (inv_mass is None)
    dense = L is not None
    vg = perturbed(value_and_grad, perturb)
    x = np.array(x0, dtype=np.float64)
    n_chains, d = x.shape
    if dense:
        L = np.tril(np.asarray(L, dtype=np.float64))
    else:
        inv_mass = np.asarray(inv_mass, dtype=np.float64)
    n_iter = n_warmup + n_draws
    f, g = vg(x)
    f, g = np.array(f, dtype=np.float64), np.array(g, dtype=np.float64)
    mu = np.log(10.0 * step_size)
    hbar, log_eps_bar, base = 0.0, 0.0, float(step_size)
    step_hist, accept_hist = np.empty(n_iter), np.empty(n_iter)
    accepted, divergent = np.zeros((n_iter, n_chains), dtype=bool), np.zeros((n_iter, n_chains), dtype=bool)
    draws, logp = [], []
    mean, m2, count, n_div = np.zeros((n_chains, d)), np.zeros((n_chains, d)), np.zeros(n_chains), 0
    s1 = s2 = None
    if moment_shift is not None:
        moment_shift = np.asarray(moment_shift, dtype=np.float64)
        s1, s2 = np.zeros(d), np.zeros((d, d) if dense else d)
    min_margin = np.inf
    for t in range(n_iter):
        u, v = uniforms(seed, stream_offset + t, n_chains)
        eps = base * (1.0 + jitter * (2.0 * v - 1.0))
        step_hist[t] = eps
        z = np.asarray(normals(t0 + t) if callable(normals) else normals[t0 + t], dtype=np.float64)
        with np.errstate(all='ignore'):
            if dense:
                r = z.copy()
                h0 = -f + 0.5 * np.sum(r * r, axis=1)
                r = r + 0.5 * eps * (g @ L)
                xp, fp, gp = x, f, g
                for l in range(n_leapfrog):
                    xp = xp + eps * (r @ L.T)
                    fp, gp = vg(xp)
                    r = r + (0.5 * eps if l + 1 == n_leapfrog else eps) * (gp @ L)
                h1 = -fp + 0.5 * np.sum(r * r, axis=1)
            else:
                p = z / np.sqrt(inv_mass)
                h0 = HO.energy(f, p, inv_mass)
                xp, pp, fp, gp = HO.trajectory(vg, x, p, g, eps, n_leapfrog, inv_mass)
                h1 = HO.energy(fp, pp, inv_mass)
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
        accepted[t], divergent[t] = acc, div
        abar = a.sum() / n_chains
        accept_hist[t] = abar
        if s1 is not None:
            xc = x - moment_shift
            s1 = s1 + xc.sum(axis=0)
            s2 = s2 + (xc.T @ xc if dense else np.sum(xc * xc, axis=0))
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
    chain_var = None
    if n_draws > 0:
        with np.errstate(all='ignore'):
            chain_var = m2 / (n_draws - 1.0) if n_draws > 1 else np.full_like(m2, np.nan)
    return dict(draws=np.array(draws).reshape(-1, n_chains, d), logp=np.array(logp).reshape(-1, n_chains), last=x,
                chain_mean=mean, chain_var=chain_var, accept_rate=count / max(n_draws, 1), accept_prob=accept_hist,
                step_size_history=step_hist, step_size=base, n_divergent=n_div, accepted=accepted, divergent=divergent,
                min_margin=min_margin, next_stream=stream_offset + n_iter, moment_sum=s1, moment_m2=s2)


# ---- the adaptation schedule and the metric of a window, from the specification ---------------------------------------------
def windows(n_warmup):
    init, term, base = 75, 50, 25
    if init + base + term > n_warmup:
        init, term = int(0.15 * n_warmup), int(0.10 * n_warmup)
        base = n_warmup - init - term
    out, start, size = [], init, base
    while start + size + 2 * size <= n_warmup - term:
        out.append((start, start + size))
        start, size = start + size, 2 * size
    return out + [(start, n_warmup - term)]


def window_metric(shift, s1, s2, n, dense):
    """``cov = (S2 - S1 S1' / n) / (n - 1)``, then ``n / (n + 5) cov + 1e-3 * 5 / (n + 5) I`` (its diagonal for the
    diagonal metric)."""
    if dense:
        cov = (s2 - np.outer(s1, s1) / n) / (n - 1.0)
        return n / (n + 5.0) * cov + 1e-3 * 5.0 / (n + 5.0) * np.eye(s1.size)
    var = (s2 - s1 * s1 / n) / (n - 1.0)
    return n / (n + 5.0) * var + 1e-3 * 5.0 / (n + 5.0)


def run_adaptive(value_and_grad, x0, normals, *, dense, inv_mass, n_warmup, n_draws, n_leapfrog=1, step_size=1.0,
                 target_accept=0.8, jitter=0.0, seed=1, stream_offset=0, thin=1, perturb=None):
    """The adaptive driver: one ``run`` per segment -- the initial buffer, every window (moments about the chains' mean at
    its start), the terminal buffer with the sampling phase --, each from the last one's states, final step and stream.
    ``inv_mass`` is the starting metric, (D,) or (D, D).  Returns the last segment's dict with the histories of all
    segments, ``inv_mass`` (the final metric), ``adapt_windows`` and ``min_margin`` over all segments."""
    wins = windows(n_warmup)
    segments = ([(wins[0][0], 0, False)] if wins[0][0] > 0 else []) + [(e - s, 0, True) for s, e in wins]
    segments.append((n_warmup - wins[-1][1], n_draws, False))
    metric = np.asarray(inv_mass, dtype=np.float64)
    x, step, done = np.array(x0, dtype=np.float64), float(step_size), 0
    hist, margin, accepted = [], np.inf, []
    n_chains = x.shape[0]
    for seg_warmup, seg_draws, is_window in segments:
        kw = dict(L=np.linalg.cholesky(metric)) if dense else dict(inv_mass=metric)
        shift = x.mean(axis=0) if is_window else None
        res = run(value_and_grad, x, normals, n_warmup=seg_warmup, n_draws=seg_draws, n_leapfrog=n_leapfrog, step_size=step,
                  target_accept=target_accept, jitter=jitter, seed=seed, stream_offset=stream_offset + done, thin=thin,
                  perturb=perturb, moment_shift=shift, t0=done, **kw)
        if is_window:
            metric = window_metric(shift, res['moment_sum'], res['moment_m2'], float(n_chains * seg_warmup), dense)
        hist.append((res['step_size_history'], res['accept_prob']))
        accepted.append(res['accepted'])
        margin = min(margin, res['min_margin'])
        x, step, done = res['last'], res['step_size'], done + seg_warmup + seg_draws
    res['step_size_history'] = np.concatenate([h[0] for h in hist])
    res['accept_prob'] = np.concatenate([h[1] for h in hist])
    res['accepted'] = np.concatenate(accepted)
    res.update(inv_mass=metric, adapt_windows=wins, min_margin=margin)
    return res


# ---- the cases the CPU and the GPU tests share --------------------------------------------------------------------------------
PARITY_MODELS = ('gauss', 'funnel', 'corr', 'logistic', 'source')
PARITY_CHAINS = (1, 5, 64, 257)
PARITY_DIMS = (1, 2, 17, 65)                 # the edges of the 16-column pad and of a 64-wide tile
PARITY_WARMUP, PARITY_DRAWS = HO.PARITY_WARMUP, HO.PARITY_DRAWS
# seeds moved off a case whose accept test came closer than HO.MIN_MARGIN on the host (tests/test_hmc_metric_cpu.py vets all)
RESEED = {('corr', 257, 14): 1520315, ('logistic', 257, 0): 1530301, ('source', 257, 15): 2540316,
          ('source', 257, 20): 1540321}


def parity_dims(kind):
    return PARITY_DIMS[1:] if kind == 'funnel' else PARITY_DIMS


def _case(kind, n_chains, idx, d, n_leapfrog, thin, jitter, diagonal):
    key = (kind, n_chains, idx)
    seed = RESEED.get(key, 500000 + 10000 * PARITY_MODELS.index(kind) + 100 * PARITY_CHAINS.index(n_chains) + idx + 1)
    rng = np.random.RandomState(seed)
    x0 = (0.5 if kind == 'funnel' else 1.0) * rng.randn(n_chains, d)
    inv_mass = np.exp(0.2 * rng.randn(d))
    a = rng.randn(d, d)
    sigma = np.diag(inv_mass) if diagonal else a @ a.T / d + np.eye(d)
    return dict(key=key, d=d, n_leapfrog=n_leapfrog, thin=thin, jitter=jitter, seed=seed, x0=x0, inv_mass=inv_mass,
                sigma=sigma, diagonal=diagonal, step_size=0.4 * d ** -0.25, stream_offset=3)


def parity_cases(kind, n_chains):
    """Every (d, L, thin, jitter) of the grid for one model and chain count with ``Sigma = A A' / d + I`` from the case's
    seed, then one case whose ``Sigma`` is the diagonal matrix of ``inv_mass`` (d = 17, three leapfrog steps)."""
    out = []
    for d in parity_dims(kind):
        for n_leapfrog in (1, 3):
            for thin in (1, 3):
                for jitter in (0.0, 0.2):
                    out.append(_case(kind, n_chains, len(out), d, n_leapfrog, thin, jitter, False))
    out.append(_case(kind, n_chains, len(out), 17, 3, 1, 0.2, True))
    return out


def run_case(host_model, case, normals, perturb=None, diag_route=False, **override):
    kw = dict(n_warmup=PARITY_WARMUP, n_draws=PARITY_DRAWS, n_leapfrog=case['n_leapfrog'], step_size=case['step_size'],
              target_accept=0.8, jitter=case['jitter'], seed=case['seed'], stream_offset=case['stream_offset'],
              thin=case['thin'], perturb=perturb)
    kw.update(dict(inv_mass=case['inv_mass']) if diag_route else dict(L=np.linalg.cholesky(case['sigma'])))
    kw.update(override)
    return run(HO.value_and_grad_of(host_model), case['x0'], normals, **kw)


# moments: no warm-up, thin 1, five iterations
MOMENT_CHAINS, MOMENT_DIMS, MOMENT_ITERS = (1, 5, 257), (2, 17, 65), 5


def moment_case(n_chains, d):
    rng = np.random.RandomState(7000 + 100 * d + n_chains)
    mean, sd = rng.randn(d), np.exp(0.3 * rng.randn(d))
    a = rng.randn(d, d)
    return dict(mean=mean, sd=sd, x0=mean + sd * rng.randn(n_chains, d), sigma=a @ a.T / d + np.eye(d),
                inv_mass=np.exp(0.2 * rng.randn(d)), shift=mean + 0.1 * rng.randn(d), seed=7000 + d, step_size=0.3 * d ** -0.25)


# adaptive parity: one window, [6, 36)
ADAPT_WARMUP, ADAPT_DRAWS, ADAPT_CHAINS, ADAPT_DIMS = 40, 4, (5, 64), (2, 17)
ADAPT_RESEED = {}


def adapt_case(n_chains, d, dense):
    """A Gaussian with unequal scales, started over-dispersed, from the unit metric.  The starting step is small: dual
    averaging aims at ten times the step it starts from, and trajectories beyond the leapfrog's stability limit amplify a
    rounding difference exponentially -- with it the perturbation hook's yardstick would allow almost anything."""
    key = (n_chains, d, dense)
    seed = ADAPT_RESEED.get(key, 9000 + 100 * d + n_chains + (50 if dense else 0))
    rng = np.random.RandomState(seed)
    mean, sd = rng.randn(d), np.exp(0.5 * rng.randn(d))
    return dict(key=key, mean=mean, sd=sd, x0=mean + 1.5 * sd * rng.randn(n_chains, d), seed=seed, n_leapfrog=4,
                step_size=0.03 * d ** -0.25, jitter=0.2, stream_offset=2)


# ---- statistics --------------------------------------------------------------------------------------------------------------
ROT_DIM, ROT_COND = 16, 1e4


def rotated_config():
    """A rotated Gaussian, D = 16, covariance condition number 1e4: ``(host model, mean, covariance, start)``."""
    from oracle import models as omod
    rng = np.random.RandomState(21)
    q, _ = np.linalg.qr(rng.randn(ROT_DIM, ROT_DIM))
    cov = (q * np.logspace(0.0, np.log10(ROT_COND), ROT_DIM)) @ q.T
    cov = 0.5 * (cov + cov.T)
    mean = rng.randn(ROT_DIM)
    start = mean + 2.0 * rng.randn(HO.STAT_CHAINS, ROT_DIM) @ np.linalg.cholesky(cov).T
    return omod.GaussFull(mean, np.linalg.inv(cov)), mean, cov, start


# (b): stat_config('a') adapted from the unit metric.  Twelve leapfrog steps instead of HO.STAT_LEAPFROG's eight: from a metric
# that is itself an estimate, eight leave the oracle's max rhat at 1.037 of 1.05; twelve give 0.998
ADAPT_STAT_WARMUP, ADAPT_STAT_LEAPFROG = 300, 12
