#!/usr/bin/env python3
"""Logistic regression on a data set too large to be pleasant full-batch, fitted on random batches of it.

    python examples/minibatch.py [n_data] [batch_size]

Target: `MinibatchRegressionModel` on simulated data (p = 32 covariates and an intercept).  Every iteration of the fit
evaluates the ELBO gradient on `batch_size` observations, the likelihood scaled by `n_data / batch_size`: the estimator
stays unbiased and an iteration costs the same whatever `n_data` is.  `bbvi` fits an `MFGaussian` with Philox noise (the
device-resident loop; the batch counter advances once per iteration).  The fit is then judged on ALL the data:
`model.full_model()` is the same design and responses as a full-batch target, and `vi_diagnostics` of it is printed beside
the coefficients' distance from the simulating ones.  Prints numbers; asserts nothing.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import viabel_amd as vb   # noqa: E402


def main(n_data=500000, batch_size=4096):
    p = 33
    rng = np.random.RandomState(0)
    X = np.concatenate([np.ones((n_data, 1)), rng.randn(n_data, p - 1)], axis=1)
    theta_true = np.concatenate([[-0.5], 0.5 * rng.randn(p - 1)])
    y = (rng.rand(n_data) < 1.0 / (1.0 + np.exp(-(X @ theta_true)))).astype(float)
    model = vb.MinibatchRegressionModel(X, y, batch_size, likelihood='logistic', prior_sd=5.0, seed=1)
    print('design: %d x %d (%.0f MB on the device, once); batches of %d: %.1f batches per epoch'
          % (model.n_data, model.dim, 8e-6 * n_data * 48, batch_size, n_data / batch_size))
    approx = vb.MFGaussian(model.dim, rng='philox', seed=1)
    n_iters = 3000
    t0 = time.perf_counter()
    res = vb.bbvi(model.dim, log_density=model, approx=approx, num_mc_samples=32, n_iters=n_iters, adaptive=False,
                  fixed_lr=True, learning_rate=0.01)
    dt = time.perf_counter() - t0
    theta = res['opt_param']
    mean, cov = approx.mean_and_cov(theta)
    print('%d iterations in %.2f s (%.3f ms each); the counter stands at batch %d, epoch %d'
          % (n_iters, dt, 1e3 * dt / n_iters, model.batch, model.epoch))
    print('largest deviation of the fitted mean from the simulating coefficients: %.4f (posterior sd about %.4f)'
          % (np.max(np.abs(mean - theta_true)), float(np.sqrt(np.mean(np.diag(cov))))))
    # everything that needs ONE density goes to the full-batch target on the same data
    full = model.full_model()
    vb.vi_diagnostics(theta, model=full, approx=vb.MFGaussian(model.dim, seed=2), n_samples=2000)
    return float(np.max(np.abs(mean - theta_true)))


if __name__ == '__main__':
    main(*(int(a) for a in sys.argv[1:3]))
