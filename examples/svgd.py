#!/usr/bin/env python3
"""A funnel three ways: a mean-field Gaussian fit, SVGD started from it, and HMC.  One kernel Stein discrepancy each.

    python examples/svgd.py [n_particles] [learning_rate ...]

The funnel's scale coordinate `v ~ N(0, 1)` sets the variance `exp(v)` of the others: no Gaussian has that shape, and a
mean-field fit settles on a narrow slice of it.  `svgd` takes the fit's draws as starting particles and its standard
deviations as the kernel's `scale`, and moves the particles along the Stein variational gradient (`vb_svgd_run`: scores,
all pairs, median bandwidth and optimiser step on the device, one synchronisation for the whole run); it needs no family,
no density ratio and no noise.  `hmc` draws from the target itself.  `ksd` then scores the three samples, all of the same
size, at ONE `scale`, `c` and `beta` (the HMC draws' standard deviations), and the table adds what the funnel makes easy
to check: the standard deviation of `v` (1 for the target) and of the first other coordinate (`sqrt(e)` = 1.65).
SVGD minimises a Stein discrepancy, so it wins the KSD column by construction; the standard deviations show what that
column does not, the method's known shrinkage of the spread.  With several learning rates the SVGD row is repeated for
each: `svgd.DEFAULT_LEARNING_RATE` was chosen from such a run.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import viabel_amd as vb   # noqa: E402


def main(n_particles=1024, learning_rates=(None,), n_iters=1000):
    d = 4
    model = vb.FunnelModel(d)
    approx = vb.MFGaussian(d, rng='philox', seed=1)
    fit = vb.bbvi(d, log_density=model, approx=approx, num_mc_samples=64, n_iters=3000, adaptive=False, fixed_lr=True,
                  learning_rate=0.02)
    var_param = fit['opt_param']
    n_chains = 256
    mc = vb.hmc(model, n_chains=n_chains, n_warmup=300, n_draws=n_particles // n_chains, n_leapfrog=16, var_param=var_param,
                approx=approx, seed=1)
    draws = mc['draws'].reshape(-1, d)
    scale = draws.std(axis=0)

    samples = {'mean-field fit': approx.sample(var_param, n_particles, seed=2)}
    for lr in learning_rates:
        optimizer = None if lr is None else vb.Adagrad(lr)
        res = vb.svgd(model, n_particles=n_particles, n_iters=n_iters, var_param=var_param, approx=approx,
                      optimizer=optimizer, seed=2)
        samples['SVGD from it' + ('' if lr is None else ', Adagrad(%g)' % lr)] = res['particles']
    samples['HMC draws'] = draws
    out = {}
    for label, x in samples.items():
        out[label] = dict(vb.ksd(samples=x, model=model, scale=scale), sd=x.std(axis=0, ddof=1))
    print()
    print('%-34s %10s %10s %10s' % ('sample', 'KSD', 'sd(v)', 'sd(x_0)'))
    for label, r in out.items():
        print('%-34s %10.4g %10.3f %10.3f' % (label, r['ksd'], r['sd'][d - 1], r['sd'][0]))
    return out


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 1024,
         tuple(float(a) for a in sys.argv[2:]) if len(sys.argv) > 2 else (None,))
