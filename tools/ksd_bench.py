#!/usr/bin/env python3
"""Times the kernel Stein discrepancy on the device (Engine.ksd / ksd_from_draws -> vb_ksd, csrc/vb_ksd.hip) on one GPU.

    python tools/ksd_bench.py [--draws S ...] [--dims D ...] [--n-data N] [--repeats R] [--calls K] [--warmup W]
                              [--host-draws S] [--host-dims D ...]

  given     Engine.ksd(x, scores=g): S x D draws and scores go up, the pair kernel sums all S^2 pairs, ksd2 and the S row
            sums come back -- the whole call, for every S x D of the grid;
  model     LogisticRegressionModel(n_data x 64).ksd_from_draws(x): the scores come from the model's gradient pipeline on
            the device and never cross the bus;
  numpy     the blockwise float64 oracle of tests/_ksd_oracle.py on the host's BLAS threads at S = --host-draws: the host
            route the entry replaces.

Per shape the achieved rate is S^2 D / time pair-coordinates per second; one pair-coordinate is two subtractions and three
fused multiply-adds, 8 floating-point operations.  Method (tools/predict_bench.py): W warm-up calls, then R runs of K
blocking calls each, host clock, the median over the runs of (run time / calls).  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import viabel_amd as vb   # noqa: E402
from viabel_amd import _lib   # noqa: E402
import _ksd_oracle as K   # noqa: E402


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


def with_rate(timing, s, d):
    pair_coords = float(s) * s * d / (1e-3 * timing['median_ms'])
    timing.update(pair_coordinates_per_s=pair_coords, tflops=8e-12 * pair_coords)
    return timing


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--draws', type=int, nargs='+', default=[1024, 4096, 16384])
    ap.add_argument('--dims', type=int, nargs='+', default=[64, 1024])
    ap.add_argument('--n-data', type=int, default=16384)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--host-draws', type=int, default=4096)
    ap.add_argument('--host-dims', type=int, nargs='*', default=[64])
    ap.add_argument('--profile-only', action='store_true',
                    help='three calls with given scores and three with a logistic model\'s (n_data = 4096) at S = 4096, D = 1024: '
                         'the run behind profiles/ksd_kernel_stats.txt')
    args = ap.parse_args()
    rng = np.random.RandomState(0)
    eng = _lib.default_engine()
    if args.profile_only:
        s, d, n_data = 4096, 1024, 4096
        X = rng.randn(n_data, d) / np.sqrt(d)
        beta = rng.randn(d) / np.sqrt(d)
        y = (rng.rand(n_data) < 1.0 / (1.0 + np.exp(-X @ beta))).astype(float)
        model = vb.LogisticRegressionModel(X, y, prior_sd=1.0)
        x = beta + 0.05 * rng.randn(s, d)
        g = model.grad(x)
        given = [eng.ksd(x, scores=g)[0] for _ in range(3)]
        device = [model.ksd_from_draws(x)['ksd2'] for _ in range(3)]
        print(json.dumps(dict(ksd_profile=dict(S=s, D=d, n_data=n_data, ksd2_given=given[0], ksd2_device_scores=device[0],
                                               repeat_bits_equal=len(set(given)) == 1 and len(set(device)) == 1))))
        return
    out = dict(device=eng.device_info()['name'], cus=eng.device_info()['cus'], given={}, model={}, numpy={})

    for d in args.dims:
        for s in args.draws:
            x = rng.randn(s, d)
            g = -x + 0.1 * rng.randn(s, d)
            lw = 0.5 * rng.standard_t(5.0, s)
            timing = median_per_call(lambda: eng.ksd(x, scores=g, log_w=lw), args.repeats, args.calls, args.warmup)
            timing['plan'] = _lib.ksd_plan(s, out['cus'])
            out['given']['S%d_D%d' % (s, d)] = with_rate(timing, s, d)

    d = 64
    X = rng.randn(args.n_data, d) / np.sqrt(d)
    beta = rng.randn(d)
    y = (rng.rand(args.n_data) < 1.0 / (1.0 + np.exp(-X @ beta))).astype(float)
    model = vb.LogisticRegressionModel(X, y, prior_sd=10.0)
    for s in args.draws:
        x = beta + 0.3 * rng.randn(s, d)
        timing = median_per_call(lambda: model.ksd_from_draws(x), args.repeats, args.calls, args.warmup)
        out['model']['S%d_D%d_n%d' % (s, d, args.n_data)] = with_rate(timing, s, d)

    s = args.host_draws
    for d in args.host_dims:
        x = rng.randn(s, d)
        g = -x + 0.1 * rng.randn(s, d)
        K.ROW_BLOCK = max(1, min(64, (1 << 24) // (s * d)))          # three (block x S x D) temporaries of 128 MiB
        ref = K.ksd(x, g)
        dev = eng.ksd(x, scores=g)[0]
        timing = with_rate(median_per_call(lambda: K.ksd(x, g), 3, 1, 0), s, d)
        timing.update(row_block=K.ROW_BLOCK, device_minus_numpy_over_tol_E=abs(dev - ref['ksd2']) / (K.tolerance(s, d) * ref['E']))
        key = 'S%d_D%d' % (s, d)
        out['numpy'][key] = timing
        if key in out['given']:
            timing['numpy_over_device'] = timing['median_ms'] / out['given'][key]['median_ms']
    print(json.dumps(dict(ksd_bench=out, repeats=args.repeats, calls=args.calls, warmup=args.warmup)))


if __name__ == '__main__':
    main()
