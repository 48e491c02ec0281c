#!/usr/bin/env python3
"""What a dense metric buys: HMC on a correlated posterior, run three ways at equal cost.

    python examples/hmc_dense.py [n_data]

A logistic regression on strongly correlated columns (neighbouring columns correlate at 0.95) has a posterior whose
covariance is far from diagonal.  `laplace_approximation` supplies a fit; `hmc` then draws from the posterior
  diagonal from the fit   the fit's variances as the metric (hmc's default),
  dense from the fit      its whole covariance (`metric='dense'`),
  adapted from ones       no metric at all: `inv_mass=ones`, `metric='dense', adapt_metric=True` estimates the covariance
                          from the chains during warm-up,
with the same starts, chains, warm-up, draws and leapfrog steps, so every run costs the same number of transitions.
Reported are the largest rhat and the smallest effective sample size over the coordinates, per transition: the diagonal
metric leaves the condition number of the correlation matrix to the trajectory, which at a fixed length mixes slowly
along the long axes.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import viabel_amd as vb   # noqa: E402
from viabel_amd._chain_stats import ess   # noqa: E402

D, RHO = 20, 0.95
N_CHAINS, N_WARMUP, N_DRAWS, N_LEAPFROG = 128, 300, 200, 8


def problem(n_data=500):
    rng = np.random.RandomState(0)
    corr = RHO ** np.abs(np.subtract.outer(np.arange(D), np.arange(D)))
    X = rng.randn(n_data, D) @ np.linalg.cholesky(corr).T / np.sqrt(D)
    y = (rng.rand(n_data) < 1.0 / (1.0 + np.exp(-X @ rng.randn(D)))).astype(np.float64)
    return vb.LogisticRegressionModel(X, y, 10.0)


def quality(res):
    """(max rhat, smallest ESS over the coordinates per transition)."""
    draws = res['draws']                                           # n_kept x C x D
    n, c, d = draws.shape
    smallest = min(ess(draws[:, :, j].T) for j in range(d))
    return float(np.max(res['rhat'])), float(smallest) / (n * c)


def main(n_data=500):
    model = problem(n_data)
    lap = vb.laplace_approximation(model)
    cov = lap['cov']
    sd = np.sqrt(np.diag(cov))
    print('posterior correlation matrix: condition number %.0f' % np.linalg.cond(cov / np.outer(sd, sd)))
    init = lap['approx'].sample(lap['var_param'], N_CHAINS)
    common = dict(n_chains=N_CHAINS, n_warmup=N_WARMUP, n_draws=N_DRAWS, n_leapfrog=N_LEAPFROG, init=init, seed=1)
    runs = (('diagonal from the fit', dict(inv_mass=np.diag(cov).copy())),
            ('dense from the fit', dict(inv_mass=cov, metric='dense')),
            ('adapted from ones', dict(inv_mass=np.ones(D), metric='dense', adapt_metric=True)))
    out = {}
    for name, kw in runs:
        res = vb.hmc(model, **dict(common, **kw))
        out[name] = quality(res) + (res['step_size'],)
    print('%-24s %10s %22s %10s' % ('metric', 'max rhat', 'min ESS / transition', 'step'))
    for name, (rhat, ess_per, step) in out.items():
        print('%-24s %10.3f %22.3f %10.3f' % (name, rhat, ess_per, step))
    return out


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 500)
