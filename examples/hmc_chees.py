#!/usr/bin/env python3
"""HMC without a guessed trajectory length: `trajectory='chees'` against fixed numbers of leapfrog steps.

    python examples/hmc_chees.py [n_data]

The posterior is examples/hmc_dense.py's: a logistic regression on strongly correlated columns.  `laplace_approximation`
supplies a fit, whose variances are the (diagonal) metric of every run; the starts, chains, warm-up and draws are the same.
  n_leapfrog = 4, 16, 64   the trajectory length is the user's guess,
  trajectory='chees'       one length shared by the chains, adapted during warm-up (ChEES-HMC) from a single leapfrog step,
  ... adapt_metric=True    the same from the unit metric: step size, metric and trajectory length all adapted -- no tuning
                           constant left.
The number of leapfrog steps is what a transition costs, so the figure to compare is the smallest effective sample size
over the coordinates per gradient evaluation of the sampling phase.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import viabel_amd as vb   # noqa: E402
from viabel_amd._chain_stats import ess   # noqa: E402
import hmc_dense   # noqa: E402

N_CHAINS, N_WARMUP, N_DRAWS = 128, 300, 200


def quality(res):
    """(max rhat, smallest ESS over the coordinates per gradient evaluation of the sampling phase)."""
    draws = res['draws']                                           # n_kept x C x D
    n, c, d = draws.shape
    smallest = min(ess(draws[:, :, j].T) for j in range(d))
    steps = int(res['n_leapfrog_history'][-n:].sum())
    return float(np.max(res['rhat'])), float(smallest) / (c * steps)


def main(n_data=500):
    model = hmc_dense.problem(n_data)
    lap = vb.laplace_approximation(model)
    init = lap['approx'].sample(lap['var_param'], N_CHAINS)
    common = dict(n_chains=N_CHAINS, n_warmup=N_WARMUP, n_draws=N_DRAWS, init=init, seed=1)
    fit = dict(inv_mass=np.diag(lap['cov']).copy())
    runs = [('n_leapfrog = %d' % n, dict(fit, n_leapfrog=n)) for n in (4, 16, 64)]
    runs.append(('chees', dict(fit, trajectory='chees')))
    runs.append(('chees, adapt_metric', dict(inv_mass=np.ones(model.dim), trajectory='chees', adapt_metric=True)))
    out = {}
    for name, kw in runs:
        res = vb.hmc(model, **dict(common, **kw))
        out[name] = quality(res) + (res['trajectory_length'], float(res['n_leapfrog_history'][N_WARMUP:].mean()))
    print('%-22s %10s %24s %8s %8s' % ('trajectory', 'max rhat', 'min ESS / gradient eval', 'T', 'mean L'))
    for name, (rhat, ess_per, traj, steps) in out.items():
        print('%-22s %10.3f %24.5f %8.3f %8.1f' % (name, rhat, ess_per, traj, steps))
    return out


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 500)
