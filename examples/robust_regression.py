#!/usr/bin/env python3
"""Robust (Student-t) regression beside ordinary (Gaussian) regression, both with an unknown noise scale.

    python examples/robust_regression.py [n_data]

The use case of the reference's docs/source/robust-regression.ipynb with the built-in target instead of a hand-written
density: a line with intercept 1 and slope 2, a few gross outliers that all pull the slope the same way.  Two
`LocationScaleRegressionModel`s on the same data -- Gaussian and Student-t (df = 4) noise, each with its scale as a
parameter, theta = [intercept, slope, log sigma] -- are fitted by `bbvi` with an `MFGaussian` and checked by
`vi_diagnostics`; the two fitted slopes are printed side by side.  The Gaussian fit follows the outliers (and reports a
large sigma), the Student-t fit stays with the bulk of the data.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import viabel_amd as vb   # noqa: E402


def main(n_data=200):
    rng = np.random.RandomState(0)
    x = rng.randn(n_data)
    X = np.column_stack([np.ones(n_data), x])                     # no intercept in the model: a column of ones
    b_true, sigma_true = np.array([1.0, 2.0]), 0.5
    y = X @ b_true + sigma_true * rng.randn(n_data)
    out = np.argsort(x)[-max(3, n_data // 25):]                   # the largest x: outliers far below the line
    y[out] -= 12.0
    fits = {}
    for likelihood in ('gaussian', 'student_t'):
        model = vb.LocationScaleRegressionModel(X, y, likelihood=likelihood, df=4.0, prior_sd=10.0, scale_prior_sd=1.0)
        approx = vb.MFGaussian(model.dim, rng='philox', seed=1)
        res = vb.bbvi(model.dim, log_density=model, approx=approx, num_mc_samples=64, n_iters=3000, adaptive=False,
                      fixed_lr=True, learning_rate=0.02)
        theta = res['opt_param']
        print('--- %s likelihood: vi_diagnostics' % likelihood)
        vb.vi_diagnostics(theta, objective=res['objective'], n_samples=20000)
        b, g = model.unpack(approx.mean_and_cov(theta)[0])       # at the posterior mean of theta
        fits[likelihood] = (b, float(np.exp(g[0])))
    print('simulated with intercept %.2f, slope %.2f, sigma %.2f; %d of %d observations moved down by 12'
          % (b_true[0], b_true[1], sigma_true, len(out), n_data))
    print('likelihood   intercept    slope    sigma')
    for likelihood, (b, sigma) in fits.items():
        print('%-10s   %9.3f   %6.3f   %6.3f' % (likelihood, b[0], b[1], sigma))
    return fits['gaussian'][0][1], fits['student_t'][0][1]


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 200)
