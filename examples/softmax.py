#!/usr/bin/env python3
"""Multiclass (softmax) regression with black-box variational inference.

    python examples/softmax.py [n_data]

Target: `SoftmaxRegressionModel` on a small synthetic 3-class problem -- two features and a column of ones as the
intercept, a N(0, 10) prior on all 3 x 3 coefficients (class-major: theta = [b_0 | b_1 | b_2]).  `bbvi` fits a
`FullRankGaussian` with Philox noise (the device-resident loop); the posterior mean's training accuracy is printed,
then `vi_diagnostics` of the fit.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import viabel_amd as vb   # noqa: E402


def main(n_data=600):
    C = 3
    rng = np.random.RandomState(0)
    centres = np.array([[2.0, 0.0], [-1.0, 1.7], [-1.0, -1.7]])
    y = rng.randint(0, C, size=n_data)
    X = np.column_stack([centres[y] + rng.randn(n_data, 2), np.ones(n_data)])
    p = X.shape[1]
    model = vb.SoftmaxRegressionModel(X, y, C, prior_sd=10.0)
    approx = vb.FullRankGaussian(model.dim, rng='philox', seed=1)
    res = vb.bbvi(model.dim, log_density=model, approx=approx, num_mc_samples=64, n_iters=3000, adaptive=False,
                  fixed_lr=True, learning_rate=0.02)
    theta = res['opt_param']
    b = approx.mean_and_cov(theta)[0].reshape(C, p)             # posterior mean, one row of coefficients per class
    accuracy = np.mean(np.argmax(X @ b.T, axis=1) == y)
    print('training accuracy of the posterior mean: %.3f (%d observations, %d classes)' % (accuracy, n_data, C))
    print('class contrasts b_c - b_0:\n%s' % np.array2string(b[1:] - b[0], precision=3))
    vb.vi_diagnostics(theta, objective=res['objective'], n_samples=20000)
    return accuracy


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 600)
