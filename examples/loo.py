#!/usr/bin/env python3
"""Model comparison by PSIS leave-one-out cross-validation, on the device.

    python examples/loo.py [n_data] [D] [D_noise] [n_samples]

Two logistic regressions of one data set: on the D informative features, and on those plus a block of D_noise pure-noise
features.  Each is fitted with a mean-field Gaussian by the device-resident loop (`vb_fit`), then `viabel_amd.loo` draws
`n_samples` values from the fit, forms the `n_data x n_samples` matrix of pointwise log-likelihoods with one fp64 MFMA
product, Pareto-smooths every observation's leave-one-out weights in one launch (one workgroup per observation) and
returns `elpd_loo`.  The model with the noise block pays for its extra parameters (`p_loo`) without predicting better.

Last, the batched smoothing against the column loop it replaces (one launch, upload, download and synchronise per
column) on the same weight matrix.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import viabel_amd as vb   # noqa: E402
from viabel_amd import _lib   # noqa: E402
from viabel_amd._psis import psislw   # noqa: E402
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


def column_loop(lw, reff=1.0):
    """The 2-D psislw before the batched kernel: one vb_psis_smooth call per column."""
    eng = _lib.default_engine()
    out = np.empty_like(lw, order='F')
    ks = np.empty(lw.shape[1])
    for j in range(lw.shape[1]):
        out[:, j], ks[j] = eng.psis_smooth(lw.shape[0], np.ascontiguousarray(lw[:, j]), reff=reff)
    return out, ks


def main(n_data=2000, D=8, D_noise=24, n_samples=4096):
    rng = np.random.RandomState(0)
    X = rng.randn(n_data, D) / np.sqrt(D)
    beta = 2.0 * rng.randn(D)
    y = (rng.rand(n_data) < 1.0 / (1.0 + np.exp(-X @ beta))).astype(float)
    X_wide = np.hstack([X, rng.randn(n_data, D_noise) / np.sqrt(D_noise)])
    results = {}
    for name, data in (('informative features', X), ('+ %d noise features' % D_noise, X_wide)):
        model = vb.LogisticRegressionModel(data, y, prior_sd=10.0)
        approx, theta = fit(model)
        print('--- %s (D = %d)' % (name, data.shape[1]))
        t0 = time.perf_counter()
        results[name] = vb.loo(theta, model=model, approx=approx, n_samples=n_samples)
        print('loo of %d observations from %d draws: %.1f ms' % (n_data, n_samples, 1e3 * (time.perf_counter() - t0)))
    a, b = (results[k] for k in results)
    diff = a['pointwise'] - b['pointwise']
    print('--- elpd_loo difference (first - second) = %.2f, SE %.2f'
          % (diff.sum(), np.sqrt(n_data * np.var(diff))))

    lw = np.asfortranarray(2.0 * np.random.RandomState(1).standard_t(3.0, (n_samples, n_data)))
    psislw(lw[:, :8]), column_loop(lw[:, :8])          # warm-up
    t_batch, t_loop = [], []
    for _ in range(3):                                  # alternating; every call ends in a synchronise
        t0 = time.perf_counter()
        sm_b, k_b = psislw(lw)
        t_batch.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        sm_l, k_l = column_loop(lw)
        t_loop.append(time.perf_counter() - t0)
    print('--- psislw of a %d x %d matrix: batched %.1f ms, column loop %.1f ms (median of 3), max |difference| %.1e'
          % (n_samples, n_data, 1e3 * np.median(t_batch), 1e3 * np.median(t_loop), np.max(np.abs(sm_b - sm_l))))


if __name__ == '__main__':
    a = [int(v) for v in sys.argv[1:]]
    main(*a)
