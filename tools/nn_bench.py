#!/usr/bin/env python3
"""Times the neural-network regression target (NeuralNetRegressionModel, csrc/vb_neuralnet.hip) on one GPU beside the same
density written as a SourceModel(grad='auto'), which is the yardstick.

    python tools/nn_bench.py [--n-data 16384,2048] [--runs 3] [--calls K] [--fit-iters 1000] [--source-budget-s B]
                             [--out FILE] [--profile-only]

Sizes: p = 64, h = 32 (D = 2113), N = 1024, Gaussian likelihood, n_data = 16 384 and 2048.  Two figures per model and
size: one blocking ExclusiveKL(MFGaussian(rng='philox')) call, and a device-resident fit of --fit-iters iterations (per
iteration).  The two models take turns, --runs runs each (built-in, source, built-in, ...); the figure is the median over
the runs.  The source model differentiates the whole network by forward-mode dual numbers with ceil(D / 8) = 265 threads
per sample, each of which walks all observations and units: one call costs seconds, so its share of the run is bounded --
one warm-up call is timed first, and each run of the source model makes as many calls / fit iterations as fit into
--source-budget-s seconds (at least 1 call, at least 2 iterations; the JSON says how many).  Every finished measurement
is appended to --out at once, so a run that is cut short keeps what it has.

--profile-only: 20 blocking calls of the built-in model at the first size and nothing else -- the workload for
`rocprofv3 --kernel-trace --stats` (profiles/nn_kernel_stats.txt).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import viabel_amd as vb   # noqa: E402
from viabel_amd.optimization import Adam   # noqa: E402

NN_SRC = r"""
// params = [n, p, h, 1 / sd^2, 1 / noise_sd^2, c | X (n x p) | y (n)]: the Gaussian-likelihood density of
// NeuralNetRegressionModel (c = every constant of f), differentiated by the engine
template <class T>
__device__ T vb_log_density(vb::vec<T> z, int d, const double* P) {
  const int n = (int)P[0], p = (int)P[1], h = (int)P[2];
  const double ivp = P[3], ivn = P[4];
  const double* X = P + 6;
  const double* y = X + (long long)n * p;
  T f = P[5];
  for (int j = 0; j < d; ++j) f -= 0.5 * ivp * z[j] * z[j];
  for (int i = 0; i < n; ++i) {
    T eta = z[d - 1];
    for (int k = 0; k < h; ++k) {
      T pre = z[h * p + k];
      for (int j = 0; j < p; ++j) pre += X[(long long)i * p + j] * z[k * p + j];
      eta += z[h * p + h + k] * tanh(pre);
    }
    const T r = y[i] - eta;
    f -= 0.5 * ivn * r * r;
  }
  return f;
}
"""


def problem(p, h, n_data, seed=0):
    rng = np.random.RandomState(seed)
    X = rng.randn(n_data, p) / np.sqrt(p)
    W, a, v = rng.randn(h, p), rng.randn(h), rng.randn(h) / np.sqrt(h)
    y = np.tanh(X @ W.T + a) @ v + 0.3 * rng.randn(n_data)
    return X, y


def source_twin(model):
    n, p, h, D = model.n_data, model.n_features, model.n_hidden, model.dim
    sd, ns = model.prior_sd, model.noise_sd
    const = -D * (np.log(sd) + 0.5 * np.log(2.0 * np.pi)) - n * (np.log(ns) + 0.5 * np.log(2.0 * np.pi))
    params = np.concatenate([[n, p, h, 1.0 / sd ** 2, 1.0 / ns ** 2, const], model.X.ravel(), model.y])
    return vb.SourceModel(D, NN_SRC, params, grad='auto')


class Side:
    """One model's objective and how it is timed."""

    def __init__(self, model, N, seed=1):
        self.approx = vb.MFGaussian(model.dim, rng='philox', seed=seed)
        self.obj = vb.ExclusiveKL(self.approx, model, N)
        self.theta = np.concatenate([0.1 * np.random.RandomState(2).randn(model.dim), np.full(model.dim, -2.0)])

    def call_s(self, calls):
        t0 = time.perf_counter()
        for _ in range(calls):
            value, grad = self.obj(self.theta)
        dt = (time.perf_counter() - t0) / calls
        assert np.isfinite(value) and np.all(np.isfinite(grad))
        return dt

    def fit_s(self, iters):
        t0 = time.perf_counter()
        res = Adam(0.01, iterate_avg_prop=None).optimize(iters, self.obj, self.theta, on_device=True)
        dt = (time.perf_counter() - t0) / iters
        assert np.all(np.isfinite(res['opt_param']))
        return dt


def emit(path, record):
    line = json.dumps(record)
    print(line, flush=True)
    if path:
        with open(path, 'a') as f:
            f.write(line + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n-data', default='16384,2048')
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--fit-iters', type=int, default=1000)
    ap.add_argument('--source-budget-s', type=float, default=20.0)
    ap.add_argument('--out', default=None)
    ap.add_argument('--profile-only', action='store_true')
    args = ap.parse_args()
    p, h, N = 64, 32, 1024
    sizes = [int(s) for s in args.n_data.split(',')]
    if args.profile_only:
        X, y = problem(p, h, sizes[0])
        side = Side(vb.NeuralNetRegressionModel(X, y, h, 'gaussian', prior_sd=1.0, noise_sd=0.3), N)
        side.call_s(3)
        emit(args.out, dict(nn_profile=dict(n_data=sizes[0], calls=20, ms_per_call=1e3 * side.call_s(20))))
        return
    for n_data in sizes:
        X, y = problem(p, h, n_data)
        model = vb.NeuralNetRegressionModel(X, y, h, 'gaussian', prior_sd=1.0, noise_sd=0.3)
        source = source_twin(model)
        head = dict(p=p, h=h, D=model.dim, N=N, n_data=n_data)
        x = 0.3 * np.random.RandomState(1).randn(2, model.dim)
        t0 = time.perf_counter()
        fs, gs = source(x), source.grad(x)                      # (compiles the source: not part of any figure)
        fm, gm = model(x), model.grad(x)
        emit(args.out, dict(nn_bench_agreement=dict(head, rel_f=float(np.max(np.abs(fs - fm)) / np.max(np.abs(fm))),
                                                    rel_grad=float(np.max(np.abs(gs - gm)) / np.max(np.abs(gm))),
                                                    bind_and_check_s=time.perf_counter() - t0)))
        built, src = Side(model, N), Side(source, N)
        built.call_s(3)
        first = src.call_s(1)                                   # the source model's warm-up call, timed: sizes its runs
        src_calls = int(max(1, min(args.calls, args.source_budget_s / first)))
        src_iters = int(max(2, min(args.fit_iters, args.source_budget_s / first)))
        call_b, call_s, fit_b, fit_s = [], [], [], []
        for run in range(args.runs):                            # alternated: built-in, source, built-in, ...
            call_b.append(built.call_s(args.calls))
            call_s.append(src.call_s(src_calls))
            emit(args.out, dict(nn_bench_run=dict(head, run=run, what='call', built_in_ms=1e3 * call_b[-1],
                                                  source_ms=1e3 * call_s[-1], built_in_calls=args.calls, source_calls=src_calls)))
        for run in range(args.runs):
            fit_b.append(built.fit_s(args.fit_iters))
            fit_s.append(src.fit_s(src_iters))
            emit(args.out, dict(nn_bench_run=dict(head, run=run, what='fit', built_in_ms_per_iter=1e3 * fit_b[-1],
                                                  source_ms_per_iter=1e3 * fit_s[-1], built_in_iters=args.fit_iters,
                                                  source_iters=src_iters)))
        med = lambda v: 1e3 * float(np.median(v))               # noqa: E731
        emit(args.out, dict(nn_bench=dict(head, runs=args.runs, source_first_call_ms=1e3 * first,
                                          call=dict(built_in_ms=med(call_b), source_ms=med(call_s),
                                                    source_over_built_in=med(call_s) / med(call_b),
                                                    built_in_calls=args.calls, source_calls=src_calls),
                                          fit=dict(built_in_ms_per_iter=med(fit_b), source_ms_per_iter=med(fit_s),
                                                   source_over_built_in=med(fit_s) / med(fit_b),
                                                   built_in_iters=args.fit_iters, source_iters=src_iters))))


if __name__ == '__main__':
    main()
