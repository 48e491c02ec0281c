#!/usr/bin/env python3
"""The Laplace approximation of a logistic regression: the mode by Newton steps on the device, the Gaussian at the mode, and
what it is good for next to a variational fit.

    python examples/laplace.py [D] [n_data]

`laplace_approximation(model)` finds the mode with `model.find_mode()` -- every Newton step is one device call
(`vb_glm_value_grad_hessian`: a streaming pass over the design and one fp64 MFMA Gram product), the D x D Cholesky is host
LAPACK -- and returns the mode, the covariance (-H)^-1, a `FullRankGaussian` parameter and the Laplace estimate of the log
evidence.  Three uses:
  1. the diagnostics the package exists for, asked of the Laplace fit: `vi_diagnostics(var_param, model=, approx=)`;
  2. the log evidence estimate beside the ELBO of a `bbvi` fit of the same family;
  3. `bbvi` (FASO, fixed learning rate) started from the Laplace parameter beside the default start: iterations until its
     convergence checks pass.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import viabel_amd as vb   # noqa: E402


def fit(model, approx, init, n_iters, mc):
    t0 = time.perf_counter()
    # FASO at a fixed learning rate: it stops where its convergence checks (R-hat, then MCSE / ESS of the iterate average) pass
    res = vb.bbvi(approx.dim, n_iters=n_iters, num_mc_samples=mc, log_density=model, approx=approx, init_var_param=init,
                  adaptive=True, fixed_lr=True, learning_rate=0.01)
    dt = time.perf_counter() - t0
    n_done = len(res['value_history'])
    elbo = -float(np.mean(res['value_history'][-max(1, n_done // 10):]))
    return res, n_done, elbo, dt


def main(D=20, n_data=2000, n_iters=8000, mc=64):
    rng = np.random.RandomState(0)
    X = rng.randn(n_data, D) / np.sqrt(D)
    beta = rng.randn(D)
    y = (rng.rand(n_data) < 1.0 / (1.0 + np.exp(-X @ beta))).astype(float)
    model = vb.LogisticRegressionModel(X, y, prior_sd=10.0)

    t0 = time.perf_counter()
    lap = vb.laplace_approximation(model)
    dt = time.perf_counter() - t0
    print('Laplace: mode in %d Newton steps (converged: %s), %.1f ms in all; max|grad| at the mode %.1e'
          % (lap['n_iter'], lap['converged'], 1e3 * dt, np.max(np.abs(model.grad(lap['mode'])))))
    print('coefficient error |mode - beta| / |beta| = %.3f, mean posterior sd %.3f'
          % (np.linalg.norm(lap['mode'] - beta) / np.linalg.norm(beta), np.sqrt(np.diag(lap['cov'])).mean()))

    print('\n-- 1. diagnostics of the Laplace fit')
    vb.vi_diagnostics(lap['var_param'], model=model, approx=lap['approx'], n_samples=20000)

    print('\n-- 2. and 3. bbvi with the same family, default start and Laplace start')
    cold, n_cold, elbo_cold, dt_cold = fit(model, vb.FullRankGaussian(D, seed=2), None, n_iters, mc)
    warm, n_warm, elbo_warm, dt_warm = fit(model, lap['approx'], lap['var_param'], n_iters, mc)
    print('log evidence, Laplace estimate: %.3f' % lap['log_evidence'])
    print('ELBO, default start: %.3f after %d iterations (%.1f s)' % (elbo_cold, n_cold, dt_cold))
    print('ELBO, Laplace start: %.3f after %d iterations (%.1f s)' % (elbo_warm, n_warm, dt_warm))
    mean_c, _ = cold['objective'].approx.mean_and_cov(cold['opt_param'])
    mean_w, _ = lap['approx'].mean_and_cov(warm['opt_param'])
    sd = np.sqrt(np.diag(lap['cov']))
    print('fitted mean against the mode, in posterior sd: default start %.3f, Laplace start %.3f'
          % (np.max(np.abs(mean_c - lap['mode']) / sd), np.max(np.abs(mean_w - lap['mode']) / sd)))


if __name__ == '__main__':
    a = sys.argv[1:]
    main(int(a[0]) if a else 20, int(a[1]) if len(a) > 1 else 2000)
