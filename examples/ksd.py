#!/usr/bin/env python3
"""Which sample is closest to the posterior?  One kernel Stein discrepancy each, from the model's scores alone.

    python examples/ksd.py [n_data]

A logistic regression whose columns are strongly correlated, so that the posterior is too: a mean-field Gaussian cannot
represent it, a full-rank Gaussian can.  Both are fitted with `bbvi`; `hmc` then draws from the posterior itself.  `ksd`
scores five samples of the same size against the target -- each fit raw and PSIS-corrected, and the HMC draws -- at ONE
`scale`, `c` and `beta` (the HMC draws' standard deviations), because the number only means something in comparison.  It
needs neither the density ratio (`vi_diagnostics`) nor ground truth: the HMC row is here to show where a good sample lands.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import viabel_amd as vb   # noqa: E402


def main(n_data=400, n_samples=4096):
    rng = np.random.RandomState(0)
    d = 6
    shared = rng.randn(n_data, 1)
    X = 0.9 * shared + 0.45 * rng.randn(n_data, d)                  # pairwise column correlation 0.8
    beta = np.array([1.5, -1.0, 0.5, 0.0, -0.5, 1.0])
    y = (rng.rand(n_data) < 1.0 / (1.0 + np.exp(-X @ beta))).astype(float)
    model = vb.LogisticRegressionModel(X, y, prior_sd=5.0)

    fits = {}
    for name, approx in (('mean field', vb.MFGaussian(d, rng='philox', seed=1)),
                         ('full rank', vb.FullRankGaussian(d, rng='philox', seed=1))):
        res = vb.bbvi(d, log_density=model, approx=approx, num_mc_samples=64, n_iters=3000, adaptive=False, fixed_lr=True,
                      learning_rate=0.02)
        fits[name] = (res['opt_param'], approx)
    var_param, approx = fits['full rank']
    n_chains = 256
    res = vb.hmc(model, n_chains=n_chains, n_warmup=300, n_draws=n_samples // n_chains, n_leapfrog=16, var_param=var_param,
                 approx=approx, seed=1)
    draws = res['draws'].reshape(-1, d)
    scale = draws.std(axis=0)

    out = {}
    for name, (theta, family) in fits.items():
        for weights in (None, 'psis'):
            label = '%s, %s' % (name, 'PSIS-corrected' if weights else 'raw')
            out[label] = vb.ksd(theta, model=model, approx=family, n_samples=n_samples, weights=weights, scale=scale)
    out['HMC draws'] = vb.ksd(samples=draws, model=model, scale=scale)
    print()
    print('%-28s %10s %10s %8s' % ('sample', 'KSD', 'ESS', 'khat'))
    for label, r in out.items():
        print('%-28s %10.4g %10.1f %8s' % (label, r['ksd'], r['ess'], '-' if r['khat'] is None else '%.2f' % r['khat']))
    return out


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 400)
