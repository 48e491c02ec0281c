#!/usr/bin/env python3
"""Times hmc()'s dense metric against its diagonal one on one GPU, and says what the dense metric buys (csrc/vb_hmc.hip,
vb_hmc_run_metric).

    python tools/hmc_metric_bench.py [--transitions T] [--chains C] [--leapfrog L] [--rounds R] [--shapes ...] [--quality]
    rocprofv3 --kernel-trace --stats -d profiles/hmc_metric -- python tools/hmc_metric_bench.py --kernels-only --shapes gauss1024

Shapes: `logistic` and `multilevel` are tools/hmc_bench.py's (n_data = 16 384, D = 64; D = 117); `gauss1024` is a
CorrelatedGaussianModel at D = 1024 (covariance A A' / D + I).  C = 1024 chains, L = 16 leapfrog steps, T transitions
without warm-up at a fixed step (jitter 0.2), no draws kept; one unrecorded run of each kind first.
  diag    Engine.hmc_run_metric with inv_mass = ones (what vb_hmc_run enqueues)
  dense   Engine.hmc_run_metric with the Cholesky factor of a dense covariance (A A' / D + I, scaled to the step): per
          transition 2 L + 1 triangular C x D x D products -- L + 1 kicks r += c eps (g L), L drifts x += eps (r L')
The two alternate, R rounds each, the host clock around each whole run (both end synchronised); reported are all times and
the medians in ms per transition, and `product_flop`, the floating-point operations of one transition's products
(C D (D + 1) each: the triangle only), to set against the kernel times of a profiler run.  --kernels-only: one dense run
per shape and nothing else, for the profiler.  --quality: the three runs of examples/hmc_dense.py (diagonal from the fit,
dense from the fit, adapted from ones) at equal transitions: max rhat, the smallest ESS per transition, the step.  Prints
one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'examples'))
import viabel_amd as vb   # noqa: E402
from viabel_amd import _lib   # noqa: E402


def build(shape):
    if shape != 'gauss1024':
        import hmc_bench
        return hmc_bench.build(shape)
    d = 1024
    rng = np.random.RandomState(0)
    a = rng.randn(d, d)
    return vb.CorrelatedGaussianModel(rng.randn(d), covariance=a @ a.T / d + np.eye(d)), dict()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--transitions', type=int, default=20)
    ap.add_argument('--chains', type=int, default=1024)
    ap.add_argument('--leapfrog', type=int, default=16)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--shapes', nargs='*', default=['logistic', 'multilevel', 'gauss1024'])
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--quality', action='store_true')
    args = ap.parse_args()
    T, C, L = args.transitions, args.chains, args.leapfrog
    eng = _lib.default_engine()
    out = dict(tool='hmc_metric_bench', chains=C, leapfrog=L, transitions=T, shapes=[])
    for shape in args.shapes:
        model, rec = build(shape)
        d = model.dim
        rec.update(shape=shape, D=d, product_flop=(2 * L + 1) * C * d * (d + 1))
        rng = np.random.RandomState(1)
        x0 = 0.05 * rng.randn(C, d)
        a = rng.randn(d, d)
        factor = np.linalg.cholesky(a @ a.T / d + np.eye(d))
        step = 0.02
        eng.set_model(model.device_spec())
        run = lambda metric: eng.hmc_run_metric(x0, metric, 0, T, L, step, jitter=0.2, seed=3, keep_draws=False)   # noqa: E731
        run(factor)
        if args.kernels_only:
            out['shapes'].append(rec)
            continue
        run(np.ones(d))
        diag_s, dense_s = [], []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            run(np.ones(d))
            diag_s.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            got = run(factor)
            dense_s.append(time.perf_counter() - t0)
        diag_ms, dense_ms = 1e3 * float(np.median(diag_s)) / T, 1e3 * float(np.median(dense_s)) / T
        rec.update(diag_ms_per_transition=diag_ms, dense_ms_per_transition=dense_ms, dense_over_diag=dense_ms / diag_ms,
                   diag_ms_all=[1e3 * s / T for s in diag_s], dense_ms_all=[1e3 * s / T for s in dense_s],
                   dense_accept_rate=float(got['accept_rate'].mean()))
        out['shapes'].append(rec)
    if args.quality:
        import hmc_dense
        out['quality'] = {name: dict(max_rhat=r, min_ess_per_transition=e, step_size=s)
                          for name, (r, e, s) in hmc_dense.main().items()}
        out['quality_run'] = dict(D=hmc_dense.D, chains=hmc_dense.N_CHAINS, warmup=hmc_dense.N_WARMUP,
                                  draws=hmc_dense.N_DRAWS, leapfrog=hmc_dense.N_LEAPFROG)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
