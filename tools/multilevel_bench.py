#!/usr/bin/env python3
"""Times the multilevel regression target (MultilevelRegressionModel, csrc/vb_multilevel.hip) on one GPU.

    python tools/multilevel_bench.py [--case a|b|all] [--repeats R] [--calls K] [--warmup W]

 (a) logistic, p = 64, J = 512, n_data = 16384 (D = 577, beyond what a SourceModel holds), N = 1024: the rows evaluation
     (`model.grad(x)` on host samples: upload, the five launches, f and G back) and one blocking
     ExclusiveKL(FullRankGaussian(rng='philox')) evaluation;
 (b) logistic, p = 16, J = 100, n_data = 2048 (D = 117 <= 128), N = 1024: the same two figures for this model and for the
     same density written as a SourceModel(grad='auto') on the same data.

Method: W warm-up calls, then R runs of K blocking calls each, every call ending in the engine's own wait for the
device; the figure is the median over the runs of (run time / K).  K = 400 by default: a run of the built-in target then
lasts 0.05 ... 0.2 s (the source model runs K / 5 calls).  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import viabel_amd as vb   # noqa: E402

MULTILEVEL_SRC = r"""
// params = [n, p, J, sd, tau_sd | X (n x d, row-major, row i = [x_i | zeros]) | y (n) | g (n)]: the logistic density of
// MultilevelRegressionModel, differentiated by the engine
template <class T>
__device__ T vb_log_density(vb::vec<T> z, int d, const double* P) {
  const int n = (int)P[0], p = (int)P[1], J = (int)P[2];
  const double sd = P[3], tsd = P[4];
  const double* X = P + 5;
  const double* y = X + (long long)n * d;
  const double* g = y + n;
  const T omega = z[d - 1];
  const T tau = exp(omega);
  T f = -(double)p * (log(sd) + 0.91893853320467274178) - (double)J * 0.91893853320467274178
        + 0.69314718055994530942 - log(tsd) - 0.91893853320467274178;
  for (int j = 0; j < p; ++j) f -= 0.5 * z[j] * z[j] / (sd * sd);
  for (int j = p; j < p + J; ++j) f -= 0.5 * z[j] * z[j];
  f += omega - 0.5 * tau * tau / (tsd * tsd);
  for (int i = 0; i < n; ++i) {
    const T eta = vb::dot(X + (long long)i * d, z, d) + tau * z[p + (int)g[i]];
    f += y[i] * eta - (fmax(eta, 0.0) + log1p(exp(-fabs(eta))));
  }
  return f;
}
"""


def problem(p, J, n_data, seed=0):
    rng = np.random.RandomState(seed)
    X = rng.randn(n_data, p) / np.sqrt(p)
    groups = rng.randint(0, J, size=n_data)
    eta = X @ rng.randn(p) + rng.randn(J)[groups]
    y = (rng.rand(n_data) < 1.0 / (1.0 + np.exp(-eta))).astype(float)
    return X, y, groups


def median_per_call(fn, repeats, calls, warmup):
    for _ in range(warmup):
        fn()
    per_call = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        per_call.append((time.perf_counter() - t0) / calls)
    return dict(median_ms=1e3 * float(np.median(per_call)), min_ms=1e3 * float(np.min(per_call)),
                max_ms=1e3 * float(np.max(per_call)))


def time_model(model, N, repeats, calls, warmup):
    D = model.dim
    x = 0.3 * np.random.RandomState(1).randn(N, D)
    rows = median_per_call(lambda: model.grad(x), repeats, calls, warmup)
    approx = vb.FullRankGaussian(D, rng='philox', seed=1)
    obj = vb.ExclusiveKL(approx, model, N)
    theta = approx.init_param()
    value, grad = obj(theta)
    assert np.isfinite(value) and np.all(np.isfinite(grad))
    return dict(rows=rows, exclusive_kl_fullrank=median_per_call(lambda: obj(theta), repeats, calls, warmup))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--case', default='all', choices=['a', 'b', 'all'])
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--calls', type=int, default=400)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    out = {}
    if args.case in ('a', 'all'):
        p, J, n_data, N = 64, 512, 16384, 1024
        X, y, groups = problem(p, J, n_data)
        model = vb.MultilevelRegressionModel(X, y, groups, J)
        out['a'] = dict(p=p, J=J, n_data=n_data, N=N, D=model.dim, **time_model(model, N, args.repeats, args.calls, args.warmup))
    if args.case in ('b', 'all'):
        p, J, n_data, N = 16, 100, 2048, 1024
        X, y, groups = problem(p, J, n_data)
        model = vb.MultilevelRegressionModel(X, y, groups, J)
        D = model.dim
        Xpad = np.zeros((n_data, D))
        Xpad[:, :p] = X
        params = np.concatenate([[n_data, p, J, model.prior_sd, model.tau_sd], Xpad.ravel(), y, groups.astype(float)])
        source = vb.SourceModel(D, MULTILEVEL_SRC, params, grad='auto')
        x = 0.3 * np.random.RandomState(1).randn(8, D)
        agree_f = float(np.max(np.abs(source(x) - model(x))))
        agree_g = float(np.max(np.abs(source.grad(x) - model.grad(x))))
        built_in = time_model(model, N, args.repeats, args.calls, args.warmup)
        src = time_model(source, N, max(3, args.repeats // 3), max(2, args.calls // 5), 2)
        out['b'] = dict(p=p, J=J, n_data=n_data, N=N, D=D, built_in=built_in, source=src,
                        source_over_built_in_rows=src['rows']['median_ms'] / built_in['rows']['median_ms'],
                        source_over_built_in_exclusive_kl=src['exclusive_kl_fullrank']['median_ms']
                        / built_in['exclusive_kl_fullrank']['median_ms'],
                        max_abs_f_difference=agree_f, max_abs_grad_difference=agree_g)
    print(json.dumps(dict(multilevel_bench=out, repeats=args.repeats, calls=args.calls, warmup=args.warmup)))


if __name__ == '__main__':
    main()
