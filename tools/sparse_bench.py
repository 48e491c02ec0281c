#!/usr/bin/env python3
"""Times the sparse-design regression target (SparseRegressionModel, csrc/vb_sparse.hip) on one GPU.

    python tools/sparse_bench.py [--case a|b|all] [--repeats R] [--calls K] [--warmup W] [--samples N]

 (a) logistic, n_data = 65536, p = 8192, 16 entries per row plus an intercept, N = 256 samples: the rows evaluation
     (`model.grad(x)` on host samples: upload, the launches, f and G back) and one blocking
     ExclusiveKL(MFGaussian(rng='philox')) evaluation, for this model and for LogisticRegressionModel on the same matrix made
     dense (4 GiB per operand copy on the device; the host needs about 20 GiB while it is bound);
 (b) logistic, n_data = 200000, p = 50000, 10 entries per row plus an intercept, N = 256: the same two figures (no dense
     comparator exists), and the traffic model of the two gather passes, nnz * N * 8 bytes each, over the WHOLE rows call --
     a lower bound of the passes' own rate, which a kernel trace gives (rocprofv3 --kernel-trace --stats on this script).

Method: W warm-up calls, then R runs of K blocking calls each, every call ending in the engine's own wait for the
device; the figure is the median over the runs of (run time / K).  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import viabel_amd as vb   # noqa: E402


def problem(n_data, p, per_row, seed=0):
    """CSR triple with an intercept column of ones and `per_row` further entries randn / sqrt(per_row) per row (columns drawn
    with replacement: the constructor sums the few duplicates), and Bernoulli responses."""
    rng = np.random.RandomState(seed)
    cols = np.concatenate([np.zeros((n_data, 1), dtype=np.int64), rng.randint(1, p, size=(n_data, per_row))], axis=1)
    vals = np.concatenate([np.ones((n_data, 1)), rng.randn(n_data, per_row) / np.sqrt(per_row)], axis=1)
    y = (rng.rand(n_data) < 0.5).astype(float)
    return (vals.ravel(), cols.ravel(), np.arange(n_data + 1) * (per_row + 1)), y


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
    x[:, 0] *= 0.1
    rows = median_per_call(lambda: model.grad(x), repeats, calls, warmup)
    approx = vb.MFGaussian(D, rng='philox', seed=1)
    obj = vb.ExclusiveKL(approx, model, N)
    theta = np.concatenate([np.zeros(D), -2.0 * np.ones(D)])
    value, grad = obj(theta)
    assert np.isfinite(value) and np.all(np.isfinite(grad))
    return dict(rows=rows, exclusive_kl_meanfield=median_per_call(lambda: obj(theta), repeats, calls, warmup))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--case', default='all', choices=['a', 'b', 'all'])
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--samples', type=int, default=256)
    args = ap.parse_args()
    N = args.samples
    out = {}
    if args.case in ('a', 'all'):
        n_data, p, per_row = 65536, 8192, 16
        triple, y = problem(n_data, p, per_row)
        model = vb.SparseRegressionModel(triple, y, shape=(n_data, p))
        sparse = time_model(model, N, args.repeats, args.calls, args.warmup)
        dense_model = vb.LogisticRegressionModel(model.to_dense(), y)
        x = 0.3 * np.random.RandomState(2).randn(8, p)
        agree_f = float(np.max(np.abs(dense_model(x) - model(x)) / np.abs(model(x))))
        gs, gd = model.grad(x), dense_model.grad(x)
        agree_g = float(np.max(np.abs(gd - gs)) / np.max(np.abs(gs)))
        dense = time_model(dense_model, N, max(3, args.repeats // 2), max(2, args.calls // 5), 2)
        out['a'] = dict(n_data=n_data, p=p, nnz=model.nnz, N=N, sparse=sparse, dense=dense,
                        dense_over_sparse_rows=dense['rows']['median_ms'] / sparse['rows']['median_ms'],
                        dense_over_sparse_exclusive_kl=dense['exclusive_kl_meanfield']['median_ms']
                        / sparse['exclusive_kl_meanfield']['median_ms'],
                        rel_f_difference=agree_f, rel_grad_difference=agree_g)
        del dense_model
    if args.case in ('b', 'all'):
        n_data, p, per_row = 200000, 50000, 10
        triple, y = problem(n_data, p, per_row, seed=1)
        model = vb.SparseRegressionModel(triple, y, shape=(n_data, p))
        t = time_model(model, N, args.repeats, args.calls, args.warmup)
        gather_bytes = 2.0 * model.nnz * N * 8
        out['b'] = dict(n_data=n_data, p=p, nnz=model.nnz, N=N, gather_model_bytes=gather_bytes,
                        gather_model_gb_per_s_over_whole_rows_call=gather_bytes / (1e-3 * t['rows']['median_ms']) / 1e9,
                        gather_model_gb_per_s_over_whole_exclusive_kl_call=gather_bytes
                        / (1e-3 * t['exclusive_kl_meanfield']['median_ms']) / 1e9, **t)
    print(json.dumps(dict(sparse_bench=out, repeats=args.repeats, calls=args.calls, warmup=args.warmup)))


if __name__ == '__main__':
    main()
