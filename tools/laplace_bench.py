#!/usr/bin/env python3
"""Times the Laplace approximation's pieces on one GPU (csrc/vb_glm_hessian.hip).

    python tools/laplace_bench.py [--repeats R] [--calls K] [--warmup W] [--shapes n,D ...] [--no-difference]
    rocprofv3 --kernel-trace --stats -d profiles/laplace -- python tools/laplace_bench.py --kernels-only

Logistic regression at (n_data, D) = (16 384, 512) and (65 536, 1024).  Per shape:
  hessian        model.hessian(x) at the mode: link pass + lower-triangular Gram product + finishing kernel + D x D download
  value_grad     the same entry without a Hessian (a line search's evaluation)
  find_mode      model.find_mode() from zeros
  laplace        laplace_approximation(model): find_mode + the host Cholesky, inverse and packing
  numpy_hessian  (X.T * w) @ X - I / sd^2 on the host's threads (OMP_NUM_THREADS, reported as host_threads), X and w given
  difference     the generic route on the same model, DeviceModel.hessian: 4 D + 1 device gradients (skipped with
                 --no-difference; one call)
Host clock around calls that end in a synchronise (every engine call here does): W warm-up calls, then R runs of K calls,
the median over the runs of (run time / calls).  From the kernel-trace run's per-kernel times (not from this script) the Gram
product's rate is n_data * D * (D + 1) executed flops over its time against the fp64 MFMA peak, the link pass's rate one read
of X plus one write of WX (2 * n_data * round_up(D, 16) * 8 bytes) over its time against HBM; the script prints both
numerators.  --kernels-only: three Hessian calls per shape and nothing else, for the profiler.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import viabel_amd as vb   # noqa: E402


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


def problem(n_data, D):
    rng = np.random.RandomState(0)
    X = rng.randn(n_data, D) / np.sqrt(D)
    y = (rng.rand(n_data) < 1.0 / (1.0 + np.exp(-X @ rng.randn(D)))).astype(float)
    return X, y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--shapes', nargs='*', default=['16384,512', '65536,1024'])
    ap.add_argument('--no-difference', action='store_true')
    ap.add_argument('--kernels-only', action='store_true')
    args = ap.parse_args()
    out = dict(tool='laplace_bench', host_threads=os.cpu_count() if 'OMP_NUM_THREADS' not in os.environ
               else int(os.environ['OMP_NUM_THREADS']), shapes=[])
    for shape in args.shapes:
        n_data, D = (int(v) for v in shape.split(','))
        X, y = problem(n_data, D)
        model = vb.LogisticRegressionModel(X, y, prior_sd=10.0)
        ld = (D + 15) // 16 * 16
        rec = dict(n_data=n_data, D=D, gram_flops=n_data * D * (D + 1), link_bytes=2 * n_data * ld * 8)
        if args.kernels_only:
            for _ in range(3):
                model.hessian(np.zeros(D))
            out['shapes'].append(rec)
            continue
        found = model.find_mode()
        mode = found['mode']
        rec.update(n_iter=found['n_iter'], converged=bool(found['converged']))
        timed = lambda fn, calls=args.calls: median_per_call(fn, args.repeats, calls, args.warmup)      # noqa: E731
        rec['hessian'] = timed(lambda: model.hessian(mode))
        rec['value_grad'] = timed(lambda: model._value_grad_hessian(mode, False))
        rec['find_mode'] = timed(model.find_mode, 1)
        rec['laplace'] = timed(lambda: vb.laplace_approximation(model), 1)
        eta = X @ mode
        t = np.exp(-np.abs(eta))
        w = t / (1.0 + t) ** 2
        rec['numpy_hessian'] = timed(lambda: -(X.T * w) @ X - np.eye(D) / 100.0, 1)
        H = model.hessian(mode)
        rec['hessian_rel_err_vs_numpy'] = float(np.max(np.abs(H - (-(X.T * w) @ X - np.eye(D) / 100.0))) / np.max(np.abs(H)))
        if not args.no_difference:
            t0 = time.perf_counter()
            Hd = vb.DeviceModel.hessian(model, mode)
            rec['difference'] = dict(one_call_ms=1e3 * (time.perf_counter() - t0),
                                     rel_err_vs_exact=float(np.max(np.abs(Hd - H)) / np.max(np.abs(H))))
        out['shapes'].append(rec)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
