#!/usr/bin/env python3
"""Logistic regression on one-hot factors -- a sparse design -- with black-box variational inference.

    python examples/sparse_regression.py [n_data]

Target: `SparseRegressionModel` on simulated data with an intercept and three categorical factors of 40, 25 and 300 levels,
one-hot coded: p = 366 columns, four non-zeros per row.  The design is handed over as a CSR triple (`scipy.sparse` matrices
are taken as they are; the package itself does not need scipy).  `bbvi` fits an `MFGaussian` with Philox noise (the
device-resident loop); the fitted level effects are compared with the simulating ones, then `vi_diagnostics` of the fit is
printed.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import viabel_amd as vb   # noqa: E402


def main(n_data=20000):
    levels = [40, 25, 300]
    rng = np.random.RandomState(0)
    offsets = 1 + np.concatenate([[0], np.cumsum(levels)[:-1]])               # column 0 is the intercept
    p = 1 + sum(levels)
    codes = np.stack([rng.randint(k, size=n_data) for k in levels], axis=1)
    indices = np.concatenate([np.zeros((n_data, 1), dtype=np.int64), codes + offsets], axis=1)
    data = np.ones(indices.shape)
    indptr = np.arange(n_data + 1) * indices.shape[1]
    theta_true = np.concatenate([[-0.5], 0.7 * rng.randn(p - 1)])
    eta = theta_true[indices].sum(axis=1)
    y = (rng.rand(n_data) < 1.0 / (1.0 + np.exp(-eta))).astype(float)
    model = vb.SparseRegressionModel((data.ravel(), indices.ravel(), indptr), y, likelihood='logistic', prior_sd=2.0,
                                     shape=(n_data, p))
    print('design: %d x %d, %d non-zeros (dense: %.1f MB per copy, sparse: %.1f MB)'
          % (model.n_data, model.n_features, model.nnz, 8e-6 * n_data * p, 12e-6 * model.nnz))
    approx = vb.MFGaussian(model.dim, rng='philox', seed=1)
    res = vb.bbvi(model.dim, log_density=model, approx=approx, num_mc_samples=32, n_iters=3000, adaptive=False,
                  fixed_lr=True, learning_rate=0.02)
    theta = res['opt_param']
    mean = approx.mean_and_cov(theta)[0]
    # the intercept and a common shift of a factor's levels are only weakly identified apart: compare centred effects
    err = 0.0
    for k, o in zip(levels, offsets):
        fit, true = mean[o:o + k] - mean[o:o + k].mean(), theta_true[o:o + k] - theta_true[o:o + k].mean()
        print('factor of %3d levels: correlation of fitted and simulated effects %.3f, largest deviation %.3f'
              % (k, np.corrcoef(fit, true)[0, 1], np.max(np.abs(fit - true))))
        err = max(err, float(np.max(np.abs(fit - true))))
    vb.vi_diagnostics(theta, objective=res['objective'], n_samples=20000)
    return err


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 20000)
