#!/usr/bin/env python3
"""Tempered SMC from a mean-field fit, on a funnel and on a logistic regression: a log evidence beside the ELBO and beside
Laplace's estimate, and one kernel Stein discrepancy each for the fit's draws, the SMC particles and HMC draws.

    python examples/smc.py [n_particles]

`smc` starts from the DIAGONAL GAUSSIAN with the fit's mean and standard deviations (for a mean-field fit that is the fit),
tempers it into the target (`vb_smc_run`: temperature search, systematic resampling and HMC moves on the device, one
16-byte round trip per stage) and returns equally weighted particles and `log_evidence`, the log of an unbiased estimate
of the target's normalising constant.  The ELBO (here by plain Monte Carlo over the fit's draws) is a lower bound of that
constant of unknown slack; Laplace's estimate is exact for a Gaussian posterior and unchecked elsewhere.  The funnel's
density is normalised, so its log evidence is 0 and the ELBO's slack is the fit's KL divergence; the regression's posterior
is close to Gaussian, so all three agree there.  `hmc` starts every chain at the fit's draws and trusts the fit to cover the
target; `smc` bridges to it.  `ksd` scores the three samples at one `scale` (the HMC draws' standard deviations).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import viabel_amd as vb   # noqa: E402


def elbo_of(model, approx, var_param, n=4000, seed=7):
    x = approx.sample(var_param, n, seed=seed)
    terms = model(x) - approx.log_density(var_param, x)
    return float(np.mean(terms)), float(np.std(terms, ddof=1) / np.sqrt(n))


def one_target(label, model, n_particles, laplace):
    d = model.dim
    approx = vb.MFGaussian(d, rng='philox', seed=1)
    fit = vb.bbvi(d, log_density=model, approx=approx, num_mc_samples=64, n_iters=3000, adaptive=False, fixed_lr=True,
                  learning_rate=0.02)
    var_param = fit['opt_param']
    elbo, se = elbo_of(model, approx, var_param)
    res = vb.smc(model, n_particles=n_particles, var_param=var_param, approx=approx, seed=1)
    n_chains = 256
    mc = vb.hmc(model, n_chains=n_chains, n_warmup=300, n_draws=max(n_particles // n_chains, 2), n_leapfrog=16,
                var_param=var_param, approx=approx, seed=1)
    draws = mc['draws'].reshape(-1, d)
    scale = draws.std(axis=0)
    samples = {'mean-field fit': approx.sample(var_param, n_particles, seed=2), 'SMC particles': res['particles'],
               'HMC draws': draws}
    scores = {k: vb.ksd(samples=x, model=model, scale=scale)['ksd'] for k, x in samples.items()}
    print()
    print('%s (D = %d): %d stages, %d gradient evaluations per particle' % (label, d, res['n_stages'], res['n_grad_evals']))
    print('  ELBO of the fit           %12.4f  (+- %.4f)' % (elbo, se))
    print('  log evidence, SMC         %12.4f' % res['log_evidence'])
    if laplace:
        print('  log evidence, Laplace     %12.4f' % vb.laplace_approximation(model)['log_evidence'])
    for k, v in scores.items():
        print('  KSD, %-20s %12.4g   sd of the last coordinate %.3f' % (k, v, samples[k][:, -1].std(ddof=1)))
    return dict(elbo=elbo, log_evidence=res['log_evidence'], ksd=scores)


def main(n_particles=1024):
    rng = np.random.RandomState(3)
    n, d = 500, 12
    X = rng.randn(n, d) / np.sqrt(d)
    y = (rng.rand(n) < 1.0 / (1.0 + np.exp(-X @ rng.randn(d)))).astype(np.float64)
    return dict(funnel=one_target('funnel', vb.FunnelModel(4), n_particles, laplace=False),
                logistic=one_target('logistic regression', vb.LogisticRegressionModel(X, y, 3.0), n_particles, laplace=True))


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 1024)
