#!/usr/bin/env python3
"""Times the softmax regression target (SoftmaxRegressionModel, csrc/vb_softmax.hip) on one GPU.

    python tools/softmax_bench.py [--case a|b|all] [--repeats R] [--calls K] [--warmup W]

 (a) one blocking ExclusiveKL(MFGaussian(rng='philox')) evaluation at C = 10, p = 64, n_data = 4096, N = 1024;
 (b) the same objective at C = 4, p = 32 (D = 128, the largest a SourceModel holds) for this model and for a SourceModel
     restatement of the same density on the same data.

Method: W warm-up calls, then R runs of K blocking calls each, every call ending in the engine's own wait for the
device; the figure is the median over the runs of (run time / K).  Prints one JSON line.  For the kernel shares of (a) run

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/softmax_bench.py --case a --repeats 1 --calls 20

in a run of its own (tracing slows the host: its wall times are not the ones to quote).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import viabel_amd as vb   # noqa: E402

SOFTMAX_SRC = r"""
// params = [n, C, p, sd | X (n x p, row-major) | y (n)]: the density of SoftmaxRegressionModel, one thread per sample
__device__ double vb_log_density(const double* z, int d, const double* P, double* g) {
  const int n = (int)P[0], C = (int)P[1], p = (int)P[2];
  const double sd = P[3];
  const double* X = P + 4;
  const double* y = X + (long long)n * p;
  double f = -(double)d * (log(sd) + 0.91893853320467274178);
  for (int j = 0; j < d; ++j) {
    f -= 0.5 * z[j] * z[j] / (sd * sd);
    if (g) g[j] = -z[j] / (sd * sd);
  }
  for (int i = 0; i < n; ++i) {
    const double* x = X + (long long)i * p;
    const int yi = (int)y[i];
    double mx = -1e300, ey = 0.0;
    for (int c = 0; c < C; ++c) {
      double e = 0.0;
      for (int j = 0; j < p; ++j) e += x[j] * z[c * p + j];
      mx = fmax(mx, e);
      if (c == yi) ey = e;
    }
    double se = 0.0;
    for (int c = 0; c < C; ++c) {
      double e = 0.0;
      for (int j = 0; j < p; ++j) e += x[j] * z[c * p + j];
      se += exp(e - mx);
    }
    f += (ey - mx) - log(se);
    if (g)
      for (int c = 0; c < C; ++c) {
        double e = 0.0;
        for (int j = 0; j < p; ++j) e += x[j] * z[c * p + j];
        const double r = (c == yi ? 1.0 : 0.0) - exp(e - mx) / se;
        for (int j = 0; j < p; ++j) g[c * p + j] += r * x[j];
      }
  }
  return f;
}
"""


def problem(C, p, n_data, seed=0):
    rng = np.random.RandomState(seed)
    X = rng.randn(n_data, p) / np.sqrt(p)
    B = rng.randn(C, p)
    y = np.argmax(X @ B.T + rng.gumbel(size=(n_data, C)), axis=1)
    return X, y


def time_objective(model, N, repeats, calls, warmup):
    D = model.dim
    obj = vb.ExclusiveKL(vb.MFGaussian(D, rng='philox', seed=1), model, N)
    theta = np.concatenate([0.1 * np.sin(np.arange(D)), -1.0 + 0.05 * np.cos(np.arange(D))])
    for _ in range(warmup):
        value, grad = obj(theta)                      # blocking: returns the host copies of value and gradient
    per_call = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(calls):
            value, grad = obj(theta)
        per_call.append((time.perf_counter() - t0) / calls)
    assert np.isfinite(value) and np.all(np.isfinite(grad))
    return float(np.median(per_call)), float(np.min(per_call)), float(np.max(per_call))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--case', default='all', choices=['a', 'b', 'all'])
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    out = {}
    if args.case in ('a', 'all'):
        C, p, n_data, N = 10, 64, 4096, 1024
        X, y = problem(C, p, n_data)
        med, lo, hi = time_objective(vb.SoftmaxRegressionModel(X, y, C), N, args.repeats, args.calls, args.warmup)
        out['a'] = dict(C=C, p=p, n_data=n_data, N=N, median_ms=1e3 * med, min_ms=1e3 * lo, max_ms=1e3 * hi)
    if args.case in ('b', 'all'):
        C, p, n_data, N = 4, 32, 4096, 1024
        X, y = problem(C, p, n_data)
        med, lo, hi = time_objective(vb.SoftmaxRegressionModel(X, y, C), N, args.repeats, args.calls, args.warmup)
        params = np.concatenate([[n_data, C, p, 10.0], X.ravel(), y.astype(float)])
        source = vb.SourceModel(C * p, SOFTMAX_SRC, params)
        x = 0.3 * np.random.RandomState(1).randn(8, C * p)
        agree = float(np.max(np.abs(source(x) - vb.SoftmaxRegressionModel(X, y, C)(x))))
        smed, slo, shi = time_objective(source, N, max(3, args.repeats // 3), max(2, args.calls // 5), 2)
        out['b'] = dict(C=C, p=p, n_data=n_data, N=N, median_ms=1e3 * med, min_ms=1e3 * lo, max_ms=1e3 * hi,
                        source_median_ms=1e3 * smed, source_min_ms=1e3 * slo, source_max_ms=1e3 * shi,
                        source_over_softmax=smed / med, max_abs_f_difference=agree)
    print(json.dumps(dict(softmax_bench=out, repeats=args.repeats, calls=args.calls, warmup=args.warmup)))


if __name__ == '__main__':
    main()
