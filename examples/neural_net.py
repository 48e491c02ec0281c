#!/usr/bin/env python3
"""A Bayesian neural network on a noisy sine: fit with a mean-field Gaussian, predict on a grid.

    python examples/neural_net.py [n_data] [n_hidden] [n_iters]

`NeuralNetRegressionModel` is one hidden layer of tanh units with a Gaussian likelihood; every weight carries a N(0, sd)
prior.  `bbvi` fits a `MFGaussian` over its h (p + 2) + 1 = 49 coordinates with `ExclusiveKL`: per iteration the engine
forms all hidden pre-activations of all samples with one fp64 MFMA product, runs the forward and backward kernels and takes
the weight gradient with a second product.  `viabel_amd.predict` then draws from the fit and evaluates the network at
the grid for every draw on the device (`vb_nn_predict`): per grid point the predictive mean, the standard deviation of
the network's output over the draws (`eta_sd`) and that of a new response (`sd`, the noise included) come back.  A
mean-field fit of a network posterior is far from it -- the Pareto k of its importance ratios is about 2 -- so the draws are
taken as they are (`weights=None`) instead of being importance-weighted towards the posterior.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import viabel_amd as vb   # noqa: E402


def main(n_data=400, n_hidden=16, n_iters=4000):
    rng = np.random.RandomState(0)
    noise_sd = 0.2
    x = rng.uniform(-2.0, 2.0, n_data)
    y = np.sin(2.0 * x) + noise_sd * rng.randn(n_data)
    model = vb.NeuralNetRegressionModel(x[:, None], y, n_hidden, likelihood='gaussian', prior_sd=3.0, noise_sd=noise_sd)
    D = model.dim
    approx = vb.MFGaussian(D, rng='philox', seed=1)
    objective = vb.ExclusiveKL(approx, model, 64)
    init = np.concatenate([0.5 * rng.randn(D), np.full(D, -2.0)])
    res = vb.bbvi(D, objective=objective, init_var_param=init, n_iters=n_iters, adaptive=False, fixed_lr=True,
                  learning_rate=0.02)
    theta = res['opt_param']
    hist = np.asarray(res['value_history'])
    print('objective: first 100 iterations %.1f, last 100 iterations %.1f' % (hist[:100].mean(), hist[-100:].mean()))

    grid = np.linspace(-2.5, 2.5, 21)
    pred = vb.predict(theta, model=model, approx=approx, X_new=grid[:, None], n_samples=4096, weights=None)
    print('      x   sin(2x)   mean  eta_sd     sd')
    for g, m, e, s in zip(grid, pred['mean'], pred['eta_sd'], pred['sd']):
        print('%7.2f  %7.3f  %7.3f  %5.3f  %5.3f' % (g, np.sin(2.0 * g), m, e, s))
    inside = np.abs(grid) <= 2.0
    print('inside the data: mean |mean - sin(2x)| %.3f, mean eta_sd %.3f, mean sd %.3f (noise sd %.1f); outside: mean '
          'eta_sd %.3f' % (np.mean(np.abs(pred['mean'] - np.sin(2.0 * grid))[inside]), np.mean(pred['eta_sd'][inside]),
                           np.mean(pred['sd'][inside]), noise_sd, np.mean(pred['eta_sd'][~inside])))


if __name__ == '__main__':
    a = [int(v) for v in sys.argv[1:]]
    main(*a)
