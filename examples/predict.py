#!/usr/bin/env python3
"""Posterior prediction on held-out rows, on the device, beside the leave-one-out estimate of the same number.

    python examples/predict.py [n_data] [D] [n_samples]

A logistic regression: a third of the rows is held out, the rest is fitted with a mean-field Gaussian by the
device-resident loop (`vb_fit`).  `viabel_amd.predict` then draws `n_samples` values from the fit, corrects them with
their Pareto-smoothed importance weights, forms the `held-out x n_samples` matrix of linear predictors with one fp64 MFMA
product and reduces it on the device to predictive means, standard deviations and the log predictive density of every
held-out response.  `viabel_amd.loo` estimates the same expected log predictive density per observation from the training
rows alone: the two numbers should agree within their standard errors.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import viabel_amd as vb   # noqa: E402
from viabel_amd.optimization import Adam   # noqa: E402


def fit(model, num_mc_samples=128):
    D = model.dim
    approx = vb.MFGaussian(D, rng='philox')
    objective = vb.ExclusiveKL(approx, model, num_mc_samples)
    theta = np.concatenate([np.zeros(D), np.full(D, -1.0)])
    opt = Adam(0.05, iterate_avg_prop=None)
    for lr, iters in ((0.05, 1500), (0.01, 1500)):
        opt._learning_rate = lr
        theta = opt.optimize(iters, objective, theta)['opt_param']
    return approx, theta


def main(n_data=3000, D=8, n_samples=4096):
    rng = np.random.RandomState(0)
    X = rng.randn(n_data, D) / np.sqrt(D)
    beta = 2.0 * rng.randn(D)
    y = (rng.rand(n_data) < 1.0 / (1.0 + np.exp(-X @ beta))).astype(float)
    held = np.arange(n_data) % 3 == 2
    X_train, y_train, X_test, y_test = X[~held], y[~held], X[held], y[held]
    model = vb.LogisticRegressionModel(X_train, y_train, prior_sd=10.0)
    approx, theta = fit(model)

    print('--- predict: %d held-out rows' % X_test.shape[0])
    t0 = time.perf_counter()
    pred = vb.predict(theta, model=model, approx=approx, X_new=X_test, y_new=y_test, n_samples=n_samples)
    print('predict from %d draws: %.1f ms' % (n_samples, 1e3 * (time.perf_counter() - t0)))
    p_true = 1.0 / (1.0 + np.exp(-X_test @ beta))
    print('predictive mean against the true probability: mean |difference| %.3f; mean predictive sd %.3f'
          % (np.mean(np.abs(pred['mean'] - p_true)), np.mean(pred['sd'])))
    print('accuracy at 1/2: %.3f' % np.mean((pred['mean'] > 0.5) == (y_test > 0.5)))

    print('--- loo: %d training rows' % X_train.shape[0])
    res = vb.loo(theta, model=model, approx=approx, n_samples=n_samples)
    n_test, n_train = X_test.shape[0], X_train.shape[0]
    print('--- expected log predictive density per observation')
    print('held-out elpd / m        = %.4f (SE %.4f)' % (pred['elpd'] / n_test, pred['se_elpd'] / n_test))
    print('elpd_loo / n_data        = %.4f (SE %.4f)' % (res['elpd_loo'] / n_train, res['se_elpd_loo'] / n_train))


if __name__ == '__main__':
    a = [int(v) for v in sys.argv[1:]]
    main(*a)
