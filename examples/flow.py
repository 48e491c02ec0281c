#!/usr/bin/env python3
"""A RealNVP normalizing flow fitted to a funnel: ``bbvi`` with an ``NVPFlow``, then ``vi_diagnostics``.

The funnel (docs/source/quickstart.ipynb) is what the mean-field families fit badly.  The target is a ``SourceModel``:
its log density and gradient as a HIP device function, compiled for the GPU at first use.  ``bbvi`` builds the plain
``ExclusiveKL`` estimator, which the reference cannot evaluate for a flow (objectives.py:163 raises); here it is the total
gradient of the negative ELBO, the flow's log-determinant included.

The prior draws Philox noise (``rng='philox'``), so the whole fit is device-resident: ``bbvi`` reaches ``vb_flow_fit``,
which chains prior noise -> flow objective -> optimiser step for all ``n_iters`` iterations on one stream, and only the
value history and the averaged iterates come back.  With ``rng='numpy'`` (the default) every iteration would be one
blocking objective call and a numpy step instead -- the same estimator on the reference's noise stream.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import viabel_amd as vb  # noqa: E402

FUNNEL = r"""
// x[d - 1] = v ~ N(0, 1); x[j] ~ N(0, exp(v)) for j < d - 1   (log density up to a constant)
__device__ double vb_log_density(const double* x, int d, const double* p, double* g) {
  const double v = x[d - 1], w = exp(-2.0 * v);
  double f = -0.5 * v * v, gv = -v;
  for (int j = 0; j < d - 1; ++j) {
    f -= 0.5 * x[j] * x[j] * w + v;
    if (g) g[j] = -x[j] * w;
    gv += x[j] * x[j] * w - 1.0;
  }
  if (g) g[d - 1] = gv;
  return f;
}
"""


def main(n_iters=3000):
    D, K = 2, 6
    model = vb.SourceModel(D, FUNNEL)
    masks = np.array([[(j + i) % 2 for j in range(D)] for i in range(K)], dtype=float)
    layers = [[D, 32], [32, 32], [32, D]]
    prior = vb.MFGaussian(D, seed=1, rng='philox')
    flow = vb.NVPFlow(layers, layers, masks, prior, np.zeros(2 * D), D, mc_samples=20000)
    init = 0.01 * np.random.RandomState(0).randn(flow.var_param_dim)
    res = vb.bbvi(D, log_density=model, approx=flow, init_var_param=init, n_iters=n_iters, num_mc_samples=64,
                  adaptive=False, fixed_lr=True, learning_rate=3e-3)
    theta = res['opt_param']
    x = flow.sample(theta, 20000)
    print('flow samples: mean', np.round(x.mean(0), 3), 'std', np.round(x.std(0), 3), '(target: v ~ N(0, 1))')
    vb.vi_diagnostics(theta, model=model, approx=flow, n_samples=20000)


if __name__ == '__main__':
    main()
