#!/usr/bin/env python3
"""Times ExclusiveKL of an NVPFlow on the device at the NVP config: D = 256, K = 4 coupling layers with alternating
half masks, both nets [[256, 256], [256, 256]], N = 4096, CorrelatedGaussianModel target, MFGaussian(256) prior.

Both estimator forms with numpy and Philox prior noise: the blocking call in ms (median of --reps calls after --warmup).
FLOPs are counted from the shapes (every dense-layer product, 2 M N K; the target's N x D x D product listed apart), so
the TFLOP/s and the share of the 78.6 TFLOP/s fp64 MFMA peak are whole-call figures, not kernel figures.  For context,
torch fp64 autograd of the same objective on the CPU (16 threads).  Prints one JSON line.

--fit times the optimiser loop instead: microseconds per iteration of ``RMSProp.optimize`` (host clock around a call that
ends in a device synchronise, one warm-up fit, --fit-iters iterations per window, --reps windows) for the host loop
(``on_device=False``) and the device-resident loop (``vb_flow_fit``), alternating within the run so that the spread
between repeats shows; at the NVP config and at a small flow (D = 4, K = 4, hidden 16, N = 64) where launch latency is
the cost.  --fit-legs picks the legs (host,device).

Usage:  python tools/nvp_bench.py [--reps 20] [--warmup 5] [--torch-reps 2] [--out FILE]
        python tools/nvp_bench.py --fit [--fit-iters 300] [--reps 3] [--fit-legs host,device] [--out FILE]
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

PEAK_FP64_TFLOPS = 78.6
D, K, WIDTH, N = 256, 4, 256, 4096


def make(rng_kind, seed=7):
    import viabel_amd as vb
    masks = np.array([[(j + i) % 2 for j in range(D)] for i in range(K)], dtype=float)
    layers = [[D, WIDTH], [WIDTH, D]]
    return vb.NVPFlow(layers, layers, masks, vb.MFGaussian(D, seed=seed, rng=rng_kind), np.zeros(2 * D), D)


def flops(flow, path):
    """(dense-layer FLOPs, target FLOPs) of one evaluation, from the shapes."""
    nets = [flow._shapes_t, flow._shapes_s]
    fwd = sum(2 * N * a * b for sh in nets for a, b in sh) * K
    wgrad = sum(2 * N * (a + 1) * b for sh in nets for a, b in sh) * K
    igrad = sum(2 * N * a * b for sh in nets for a, b in sh) * K - sum(2 * N * sh[0][0] * sh[0][1] for sh in nets)
    total = fwd + wgrad + igrad
    if path:
        total += sum(2 * N * a * b for sh in nets for a, b in sh) * K
    return total, 2 * N * D * D


def products(flow, path):
    per = len(flow._shapes_t) + len(flow._shapes_s)
    n = K * per * 3 - 2
    return n + (K * per if path else 0)


def fit_legs(args):
    import viabel_amd as vb
    from viabel_amd import optimization as opt
    legs = args.fit_legs.split(',')
    res = {'mode': 'fit', 'iters_per_window': args.fit_iters, 'legs': {}}
    for label, d, k, width, n in (('nvp', D, K, WIDTH, N), ('small', 4, 4, 16, 64)):
        r = np.random.RandomState(3)
        A = r.randn(d, d)
        model = vb.CorrelatedGaussianModel(0.3 * r.randn(d), covariance=A @ A.T / d + np.eye(d))
        masks = np.array([[(j + i) % 2 for j in range(d)] for i in range(k)], dtype=float)
        layers = [[d, width], [width, d]]

        def window(leg, iters):
            flow = vb.NVPFlow(layers, layers, masks, vb.MFGaussian(d, seed=7, rng='philox'), np.zeros(2 * d), d)
            theta = 0.03 * np.random.RandomState(0).randn(flow.var_param_dim)
            obj = vb.ExclusiveKL(flow, model, n)
            sgo = opt.RMSProp(0.001, iterate_avg_prop=None)
            eng = obj._engine()
            eng.sync()
            t0 = time.perf_counter()
            sgo.optimize(iters, obj, theta, on_device=leg != 'host')
            eng.sync()
            return (time.perf_counter() - t0) / iters * 1e6

        for leg in legs:
            window(leg, max(10, args.fit_iters // 10))          # warm-up: buffers, code objects, pinned ring
        times = {leg: [] for leg in legs}
        for _ in range(args.reps):
            for leg in legs:
                times[leg].append(window(leg, args.fit_iters))
        for leg in legs:
            res['legs']['%s_%s' % (label, leg)] = {'us_per_iter': [round(t, 1) for t in times[leg]],
                                                   'us_per_iter_median': float(np.median(times[leg]))}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--fit', action='store_true')
    ap.add_argument('--fit-iters', type=int, default=300)
    ap.add_argument('--fit-legs', default='host,device')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--torch-reps', type=int, default=2)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.fit:
        line = json.dumps(fit_legs(args))
        print(line)
        if args.out:
            with open(args.out, 'w') as f:
                f.write(line + '\n')
        return
    import viabel_amd as vb
    r = np.random.RandomState(3)
    A = r.randn(D, D)
    model = vb.CorrelatedGaussianModel(0.3 * r.randn(D), covariance=A @ A.T / D + np.eye(D))
    res = {'config': 'nvp D=%d K=%d width=%d N=%d' % (D, K, WIDTH, N), 'peak_fp64_tflops': PEAK_FP64_TFLOPS, 'legs': {}}
    theta = None
    for path in (False, True):
        for rng_kind in ('philox', 'numpy'):
            flow = make(rng_kind)
            if theta is None:
                theta = 0.03 * np.random.RandomState(0).randn(flow.var_param_dim)
            obj = vb.ExclusiveKL(flow, model, N, use_path_deriv=path)
            for _ in range(args.warmup):
                obj(theta)
            ts = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                obj(theta)
                ts.append(time.perf_counter() - t0)
            ms = 1e3 * float(np.median(ts))
            fl, fl_model = flops(flow, path)
            res['legs']['%s_%s' % ('path' if path else 'plain', rng_kind)] = {
                'ms_median': ms, 'ms_min': 1e3 * min(ts), 'products': products(flow, path), 'gflop_layers': fl / 1e9,
                'gflop_target': fl_model / 1e9, 'tflops_call': (fl + fl_model) / (ms * 1e-3) / 1e12,
                'share_of_fp64_peak': (fl + fl_model) / (ms * 1e-3) / 1e12 / PEAK_FP64_TFLOPS}
    res['var_param_dim'] = int(theta.size)
    if args.torch_reps > 0:
        import torch
        import _nvp_oracle as O
        torch.set_num_threads(16)
        flow = make('numpy')
        z0 = flow.prior.sample(flow.prior_param, N)
        for path in (False, True):
            ts = []
            for _ in range(args.torch_reps):
                t0 = time.perf_counter()
                O.objective(flow, model, theta, z0, path)
                ts.append(time.perf_counter() - t0)
            res['torch_cpu_16t_ms_%s' % ('path' if path else 'plain')] = 1e3 * min(ts)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
