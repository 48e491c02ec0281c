"""Dev tool: MultivariateT + ExclusiveKL in parity mode (rng='numpy'): host eigh against the device iterations for the
symmetric root and the Sylvester solve, each D on both routes (objectives._HOST_ROOT_MAX_DIM set in-process)."""
import sys
import time

import numpy as np

sys.path.insert(0, '.')
import viabel_amd as vb
from viabel_amd import objectives

rng = np.random.RandomState(1)
for D in (int(a) for a in sys.argv[1:]):
    model = vb.GaussianModel(0.1 * rng.randn(D), np.exp(0.1 * rng.randn(D)))
    for route, gate in (('host', D), ('device', 0)):
        objectives._HOST_ROOT_MAX_DIM = gate
        fam = vb.MultivariateT(D, 40, seed=3)
        obj = vb.ExclusiveKL(fam, model, 1000)
        theta = fam.init_param()
        for _ in range(5):
            obj(theta)
        t0 = time.perf_counter()
        for _ in range(30):
            obj(theta)
        print('D=%4d %-6s root: %.0f us per call' % (D, route, 1e6 * (time.perf_counter() - t0) / 30))
