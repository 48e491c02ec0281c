#!/usr/bin/env python3
"""How good is the variational fit?  Robust regression checked against Hamiltonian Monte Carlo on the same device model.

    python examples/hmc.py [n_data]

The last step of the reference's docs/source/robust-regression.ipynb, which compares its fits with MCMC draws: the
Student-t `LocationScaleRegressionModel` of examples/robust_regression.py (theta = [intercept, slope, log sigma]) is
fitted by `bbvi` with a mean-field and with a full-rank Gaussian; `hmc` then runs 256 chains from the full-rank fit --
its draws as starts, its variances as the metric -- and the HMC posterior mean and covariance serve as the truth both
fits are measured against: the norm of the error in the mean, in the standard deviations and in the covariance.  The
mean-field family cannot represent the correlation between the coefficients, which shows in its covariance error.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import viabel_amd as vb   # noqa: E402


def accuracy(true_mean, true_cov, var_param, approx):
    """(mean error, sd error, covariance error, covariance scale): Euclidean norms of the differences in the mean and in the
    standard deviations, and the square roots of the spectral norms of the covariance difference and of the covariance."""
    mean, cov = approx.mean_and_cov(var_param)
    sd_err = np.sqrt(np.diag(true_cov)) - np.sqrt(np.diag(cov))
    return (float(np.linalg.norm(true_mean - mean)), float(np.linalg.norm(sd_err)),
            float(np.sqrt(np.linalg.norm(true_cov - cov, ord=2))), float(np.sqrt(np.linalg.norm(true_cov, ord=2))))


def main(n_data=200):
    rng = np.random.RandomState(0)
    x = rng.randn(n_data)
    X = np.column_stack([np.ones(n_data), x])
    y = X @ np.array([1.0, 2.0]) + 0.5 * rng.randn(n_data)
    y[np.argsort(x)[-max(3, n_data // 25):]] -= 12.0              # gross outliers at the largest x
    model = vb.LocationScaleRegressionModel(X, y, likelihood='student_t', df=4.0, prior_sd=10.0, scale_prior_sd=1.0)
    d = model.dim
    fits = {}
    for name, approx in (('mean field', vb.MFGaussian(d, rng='philox', seed=1)),
                         ('full rank', vb.FullRankGaussian(d, rng='philox', seed=1))):
        res = vb.bbvi(d, log_density=model, approx=approx, num_mc_samples=64, n_iters=3000, adaptive=False, fixed_lr=True,
                      learning_rate=0.02)
        fits[name] = (res['opt_param'], approx)
    var_param, approx = fits['full rank']
    res = vb.hmc(model, n_chains=256, n_warmup=300, n_draws=300, n_leapfrog=16, var_param=var_param, approx=approx, seed=1)
    draws = res['draws'].reshape(-1, d)
    true_mean, true_cov = res['mean'], np.cov(draws.T)
    print('HMC posterior mean   ', np.array2string(true_mean, precision=4))
    print('HMC posterior sd     ', np.array2string(np.sqrt(np.diag(true_cov)), precision=4))
    print('%-12s %12s %12s %18s %18s' % ('fit', 'mean error', 'sd error', '||cov error||^1/2', '||true cov||^1/2'))
    out = {}
    for name, (theta, family) in fits.items():
        out[name] = accuracy(true_mean, true_cov, theta, family)
        print('%-12s %12.3g %12.3g %18.3g %18.3g' % ((name,) + out[name]))
    return res, out


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 200)
