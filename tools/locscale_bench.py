#!/usr/bin/env python3
"""Times the location-scale regression target (LocationScaleRegressionModel, csrc/vb_locscale.hip) on one GPU.

    python tools/locscale_bench.py [--case a|b|all] [--repeats R] [--calls K] [--warmup W]

 (a) student_t, p = 384, q = 128, n_data = 16384 (D = 512, beyond what a SourceModel holds), N = 1024: the rows evaluation
     (`model.grad(x)` on host samples: upload, the launches, f and G back) and one blocking
     ExclusiveKL(FullRankGaussian(rng='philox')) evaluation;
 (b) student_t, p = 64, q = 32, n_data = 2048 (D = 96 <= 128), N = 1024: the same two figures for this model and for the
     same density written as a SourceModel(grad='auto') on the same data.

Method: W warm-up calls, then R runs of K blocking calls each, every call ending in the engine's own wait for the
device; the figure is the median over the runs of (run time / K).  K = 400 by default (the source model runs K / 5 calls).
Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import viabel_amd as vb   # noqa: E402

LOCSCALE_SRC = r"""
// params = [n, p, q, sd, ssd, nu, c | X (n x d, row i = [x_i | zeros]) | W (n x d, row i = [zeros | w_i]) | y (n)]: the
// Student-t density of LocationScaleRegressionModel (c = every constant of f), differentiated by the engine
template <class T>
__device__ T vb_log_density(vb::vec<T> z, int d, const double* P) {
  const int n = (int)P[0], p = (int)P[1];
  const double sd = P[3], ssd = P[4], nu = P[5];
  const double* X = P + 7;
  const double* W = X + (long long)n * d;
  const double* y = W + (long long)n * d;
  T f = P[6];
  for (int j = 0; j < p; ++j) f -= 0.5 * z[j] * z[j] / (sd * sd);
  for (int j = p; j < d; ++j) f -= 0.5 * z[j] * z[j] / (ssd * ssd);
  for (int i = 0; i < n; ++i) {
    const T eta = vb::dot(X + (long long)i * d, z, d);
    const T s = vb::dot(W + (long long)i * d, z, d);
    const T r = (y[i] - eta) * exp(-s);
    f -= s + 0.5 * (nu + 1.0) * log1p(r * r / nu);
  }
  return f;
}
"""


def problem(p, q, n_data, seed=0):
    rng = np.random.RandomState(seed)
    X = rng.randn(n_data, p) / np.sqrt(p)
    W = rng.randn(n_data, q) / np.sqrt(q)
    y = X @ rng.randn(p) + np.exp(W @ (0.3 * rng.randn(q))) * rng.standard_t(4.0, size=n_data)
    return X, y, W


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


def source_twin(model):
    """The same density as a SourceModel(grad='auto'): the two designs padded to the parameter's width."""
    from scipy.special import gammaln
    n, p, q, D = model.n_data, model.n_features, model.n_scale_features, model.dim
    nu, sd, ssd = model.df, model.prior_sd, model.scale_prior_sd
    l2pi = np.log(2.0 * np.pi)
    const = (-p * (np.log(sd) + 0.5 * l2pi) - q * (np.log(ssd) + 0.5 * l2pi)
             + n * (gammaln(0.5 * (nu + 1.0)) - gammaln(0.5 * nu) - 0.5 * np.log(nu * np.pi)))
    Xpad, Wpad = np.zeros((n, D)), np.zeros((n, D))
    Xpad[:, :p], Wpad[:, p:] = model.X, model.W
    params = np.concatenate([[n, p, q, sd, ssd, nu, const], Xpad.ravel(), Wpad.ravel(), model.y])
    return vb.SourceModel(D, LOCSCALE_SRC, params, grad='auto')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--case', default='all', choices=['a', 'b', 'all'])
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--calls', type=int, default=400)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    out = {}
    if args.case in ('a', 'all'):
        p, q, n_data, N = 384, 128, 16384, 1024
        X, y, W = problem(p, q, n_data)
        model = vb.LocationScaleRegressionModel(X, y, W, likelihood='student_t')
        out['a'] = dict(p=p, q=q, n_data=n_data, N=N, D=model.dim, **time_model(model, N, args.repeats, args.calls, args.warmup))
    if args.case in ('b', 'all'):
        p, q, n_data, N = 64, 32, 2048, 1024
        X, y, W = problem(p, q, n_data)
        model = vb.LocationScaleRegressionModel(X, y, W, likelihood='student_t')
        source = source_twin(model)
        x = 0.3 * np.random.RandomState(1).randn(8, model.dim)
        agree_f = float(np.max(np.abs(source(x) - model(x))))
        agree_g = float(np.max(np.abs(source.grad(x) - model.grad(x))))
        built_in = time_model(model, N, args.repeats, args.calls, args.warmup)
        src = time_model(source, N, max(3, args.repeats // 3), max(2, args.calls // 5), 2)
        out['b'] = dict(p=p, q=q, n_data=n_data, N=N, D=model.dim, built_in=built_in, source=src,
                        source_over_built_in_rows=src['rows']['median_ms'] / built_in['rows']['median_ms'],
                        source_over_built_in_exclusive_kl=src['exclusive_kl_fullrank']['median_ms']
                        / built_in['exclusive_kl_fullrank']['median_ms'],
                        max_abs_f_difference=agree_f, max_abs_grad_difference=agree_g)
    print(json.dumps(dict(locscale_bench=out, repeats=args.repeats, calls=args.calls, warmup=args.warmup)))


if __name__ == '__main__':
    main()
