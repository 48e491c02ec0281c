#!/usr/bin/env python3
"""Times Stein variational gradient descent on the device (Engine.svgd_run -> vb_svgd_run, csrc/vb_svgd.hip) on one GPU.

    python tools/svgd_bench.py [--particles N ...] [--dims D ...] [--n-data N] [--iters I] [--repeats R] [--calls K]
                               [--warmup W] [--host-particles N] [--host-dims D ...]

  gaussian  Engine.svgd_run on a GaussianModel, plain SGD, I iterations per call: ms per ITERATION (call time / I; the
            call's upload and download are in it) for every n x D of the grid, median rule;
  logistic  the same on LogisticRegressionModel(n_data x 64): the scores are the gradient pipeline's;
  direction one Engine.svgd_direction call with the scores given (particles and scores go up, phi comes back);
  numpy     the host route the entry replaces, in the same run: model.grad(x) plus the float64 evaluation of the oracle's
            direction (tests/_svgd_oracle.py) per iteration, at n = --host-particles.

Method (tools/ksd_bench.py): W warm-up calls, then R runs of K blocking calls each, host clock, the median over the runs of
(run time / calls).  Prints one JSON line.  The per-kernel figures (pair kernel's pair-coordinates per second beside
vb_ksd's, the product's TFLOP/s, the selection's share) are not timed here: --profile-only is the run behind
profiles/svgd_kernel_stats.txt, under rocprofv3 --kernel-trace --stats.
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
import _svgd_oracle as S   # noqa: E402


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


def per_iteration(timing, iters):
    return {key: value / iters for key, value in timing.items()}


def logistic_model(rng, n_data, d, prior_sd=10.0):
    X = rng.randn(n_data, d) / np.sqrt(d)
    beta = rng.randn(d)
    y = (rng.rand(n_data) < 1.0 / (1.0 + np.exp(-X @ beta))).astype(float)
    return vb.LogisticRegressionModel(X, y, prior_sd=prior_sd), beta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--particles', type=int, nargs='+', default=[1024, 4096])
    ap.add_argument('--dims', type=int, nargs='+', default=[64, 1024])
    ap.add_argument('--n-data', type=int, default=16384)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--host-particles', type=int, default=1024)
    ap.add_argument('--host-dims', type=int, nargs='*', default=[64])
    ap.add_argument('--profile-only', action='store_true',
                    help='at n = 4096 and D = 64, 1024: three svgd_direction calls (scores given, median rule) and three '
                         'ksd calls of the same S x D; then three iterations of svgd_run on a logistic model (n_data = 4096, '
                         'D = 64): the run behind profiles/svgd_kernel_stats.txt')
    args = ap.parse_args()
    rng = np.random.RandomState(0)
    eng = _lib.default_engine()
    sgd = (_lib.OPT_SGD, [1e-3, 0.0, 0.0, 0.0])
    if args.profile_only:
        n, info = 4096, {}
        for d in (64, 1024):
            x = rng.randn(n, d)
            g = -x + 0.1 * rng.randn(n, d)
            hs = [eng.svgd_direction(x, scores=g)[1] for _ in range(3)]
            ksd2 = [eng.ksd(x, scores=g)[0] for _ in range(3)]
            info['D%d' % d] = dict(h=hs[0], ksd2=ksd2[0], repeat_bits_equal=len(set(hs)) == 1 and len(set(ksd2)) == 1)
        model, beta = logistic_model(rng, 4096, 64)
        eng.set_model(model.device_spec())
        out = eng.svgd_run(beta + 0.3 * rng.randn(n, 64), 3, *sgd)
        info['logistic_run'] = dict(n=n, D=64, n_data=4096, h=out['bandwidth_history'].tolist())
        print(json.dumps(dict(svgd_profile=info)))
        return
    out = dict(device=eng.device_info()['name'], cus=eng.device_info()['cus'], gaussian={}, logistic={}, direction={}, numpy={})

    for d in args.dims:
        model = vb.GaussianModel(rng.randn(d), np.exp(0.3 * rng.randn(d)))
        for n in args.particles:
            x0 = rng.randn(n, d)
            eng.set_model(model.device_spec())
            timing = median_per_call(lambda: eng.svgd_run(x0, args.iters, *sgd), args.repeats, args.calls, args.warmup)
            out['gaussian']['n%d_D%d' % (n, d)] = per_iteration(timing, args.iters)
            g = model.grad(x0)
            out['direction']['n%d_D%d' % (n, d)] = median_per_call(lambda: eng.svgd_direction(x0, scores=g), args.repeats,
                                                                   args.calls, args.warmup)

    d = 64
    model, beta = logistic_model(rng, args.n_data, d)
    for n in args.particles:
        x0 = beta + 0.3 * rng.randn(n, d)
        eng.set_model(model.device_spec())
        timing = median_per_call(lambda: eng.svgd_run(x0, args.iters, *sgd), args.repeats, args.calls, args.warmup)
        out['logistic']['n%d_D%d_n%d' % (n, d, args.n_data)] = per_iteration(timing, args.iters)

    # the host route: model.grad + the oracle's direction in float64, one iteration
    n = args.host_particles
    for d in args.host_dims:
        host_model = vb.GaussianModel(rng.randn(d), np.exp(0.3 * rng.randn(d)))
        x0 = rng.randn(n, d)
        S.ROW_BLOCK = max(1, min(64, (1 << 24) // (n * d)))

        def host_iteration():
            return S.direction(x0, host_model.grad(x0), dtype=np.float64)

        ref = S.direction(x0, host_model.grad(x0))
        h64 = float(ref['h'])
        ref = S.direction(x0, host_model.grad(x0), bandwidth=h64)
        phi = host_model.svgd_direction(x0, bandwidth=h64)['phi']
        timing = median_per_call(host_iteration, 3, 1, 0)
        timing.update(row_block=S.ROW_BLOCK,
                      device_minus_oracle_over_tol_E=float(np.max(np.abs(phi - ref['phi']) / (S.tolerance(n, d) * ref['E']))))
        key = 'n%d_D%d' % (n, d)
        if key in out['gaussian']:
            timing['numpy_over_device'] = timing['median_ms'] / out['gaussian'][key]['median_ms']
        out['numpy'][key] = timing
    print(json.dumps(dict(svgd_bench=out, iters=args.iters, repeats=args.repeats, calls=args.calls, warmup=args.warmup)))


if __name__ == '__main__':
    main()
