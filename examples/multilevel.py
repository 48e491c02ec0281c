#!/usr/bin/env python3
"""A varying-intercept (multilevel) logistic regression with black-box variational inference.

    python examples/multilevel.py [observations_per_group]

Target: `MultilevelRegressionModel` on simulated grouped data -- two features and a column of ones as the intercept, J = 12
groups whose effects are drawn from N(0, tau) with tau = 1.2.  The parameter is non-centred, theta = [b | u | log tau] with
group effects tau * u.  `bbvi` fits a `FullRankGaussian` with Philox noise (the device-resident loop); tau and the group
intercepts (intercept + effect) of the fit are printed beside the simulating values, then `vi_diagnostics` of the fit: the
funnel between log tau and u is what its k-hat reports on.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import viabel_amd as vb   # noqa: E402


def main(per_group=100):
    J, tau_true = 12, 1.2
    rng = np.random.RandomState(0)
    n_data = J * per_group
    groups = rng.permutation(np.repeat(np.arange(J), per_group))            # any order: the model sorts by group itself
    X = np.column_stack([rng.randn(n_data, 2), np.ones(n_data)])
    b_true, a_true = np.array([1.0, -0.5, 0.3]), tau_true * rng.randn(J)
    eta = X @ b_true + a_true[groups]
    y = (rng.rand(n_data) < 1.0 / (1.0 + np.exp(-eta))).astype(float)
    model = vb.MultilevelRegressionModel(X, y, groups, J, likelihood='logistic', prior_sd=10.0, tau_sd=1.0)
    approx = vb.FullRankGaussian(model.dim, rng='philox', seed=1)
    res = vb.bbvi(model.dim, log_density=model, approx=approx, num_mc_samples=64, n_iters=3000, adaptive=False,
                  fixed_lr=True, learning_rate=0.02)
    theta = res['opt_param']
    b, u, tau = model.unpack(approx.mean_and_cov(theta)[0])                 # at the posterior mean of theta
    print('coefficients b: fit %s, simulated with %s' % (np.array2string(b, precision=3), b_true))
    print('tau: fit %.3f, simulated with %.3f (sample sd of the simulated effects %.3f)' % (tau, tau_true, a_true.std()))
    # the intercept and a common shift of the group effects are only weakly identified apart: compare their sums
    print('group   fit intercept + tau*u   simulated')
    for j in range(J):
        print('%5d   %21.3f   %9.3f' % (j, b[2] + tau * u[j], b_true[2] + a_true[j]))
    vb.vi_diagnostics(theta, objective=res['objective'], n_samples=20000)
    return float(np.max(np.abs(b[2] + tau * u - b_true[2] - a_true)))


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 100)
