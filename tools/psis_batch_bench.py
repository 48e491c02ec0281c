"""Dev tool: the batched smoothing kernel (psis_batch_kernel), one shape per VPT variant: blocking psislw of a 2-D array
(upload + kernel + download) and glm_psis_loo calls (device-resident: 2000 observations, the size of examples/loo.py).
Prints one JSON line: [median, min, max] microseconds per call over ROUNDS timed loops per shape.  To compare two builds
run it once per library (VIABEL_AMD_LIB), alternating."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, '.')
import viabel_amd as vb   # noqa: E402
from viabel_amd import _lib   # noqa: E402
from viabel_amd._psis import psislw   # noqa: E402

ROUNDS = 7
eng = _lib.default_engine()
res = {'lib': os.path.basename(_lib.LIB_PATH)}


def timed(fn, reps):
    fn(), fn()                                   # warm-up of this shape
    meds = []
    for _ in range(ROUNDS):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        meds.append(1e6 * (time.perf_counter() - t0) / reps)
    return float(np.median(meds)), float(min(meds)), float(max(meds))


rng = np.random.RandomState(1)
for S, m, reps in ((1024, 5000, 10), (4096, 5000, 4), (16384, 512, 8)):
    lw = np.asfortranarray(2.0 * rng.standard_t(3.0, (S, m)))
    res['psislw %d x %d' % (S, m)] = timed(lambda: psislw(lw), reps)

# the size of examples/loo.py: 2000 observations, 8 + 24 features, 4096 draws
n_data, D, S = 2000, 32, 4096
X = rng.randn(n_data, D) / np.sqrt(D)
y = (rng.rand(n_data) < 1.0 / (1.0 + np.exp(-X[:, :8] @ (2.0 * rng.randn(8))))).astype(float)
model = vb.LogisticRegressionModel(X, y, prior_sd=10.0)
x = 0.3 * rng.randn(S, D)
log_ratios = 1.5 * rng.standard_t(4.0, S)
log_w, _ = psislw(log_ratios)
eng.set_model(model.device_spec())
res['glm_psis_loo 2000 x 4096'] = timed(lambda: eng.glm_psis_loo(x, n_data, log_ratios=log_ratios, log_w=log_w), 40)
for S2 in (1024, 16384):                          # the other two variants on the device-resident route
    x2 = 0.3 * rng.randn(S2, D)
    lr2 = 1.5 * rng.standard_t(4.0, S2)
    lw2, _ = psislw(lr2)
    res['glm_psis_loo 2000 x %d' % S2] = timed(lambda: eng.glm_psis_loo(x2, n_data, log_ratios=lr2, log_w=lw2), 40 if S2 == 1024 else 10)
print(json.dumps(res), flush=True)
