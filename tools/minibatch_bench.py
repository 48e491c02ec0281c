#!/usr/bin/env python3
"""Times the data-subsampled regression target (MinibatchRegressionModel, csrc/vb_minibatch.hip) on one GPU.

    python tools/minibatch_bench.py [--n-data 1048576] [--p 64] [--samples 1024] [--batches 1024,4096,16384,65536]
                                    [--repeats R] [--calls K] [--warmup W] [--fit-iters 1000] [--full-fit-iters 100]

Logistic regression, n_data x p design, N samples.  For every batch size B:
  * one blocking ExclusiveKL(MFGaussian(rng='philox')) call and one blocking ExclusiveKL(FullRankGaussian(rng='philox'))
    call (every call takes the next batch, so every call runs the index and the gather kernel);
  * a --fit-iters iteration device-resident RMSProp fit of the MFGaussian, per iteration;
  * the index and gather kernels: the rows call `model.grad(x)` with the batch changing every call minus the same call
    with the batch held (the engine then skips the two kernels), against a device-to-device copy with the same traffic
    (bytes read + bytes written) timed with device events in the same run.
The yardstick, in the same run: the same two objectives and a --full-fit-iters fit on `full_model()`, the dense target on
all n_data observations.

Method: W warm-up calls, then R runs of K blocking calls each, every call ending in the engine's own wait for the device;
the figure is the median over the runs of (run time / K).  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import viabel_amd as vb   # noqa: E402
from viabel_amd.optimization import RMSProp   # noqa: E402


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


def objectives(model, N):
    D = model.dim
    mf = vb.ExclusiveKL(vb.MFGaussian(D, rng='philox', seed=1), model, N)
    fr = vb.ExclusiveKL(vb.FullRankGaussian(D, rng='philox', seed=1), model, N)
    theta_mf = np.concatenate([np.zeros(D), -2.0 * np.ones(D)])
    theta_fr = fr.approx.pack(np.zeros(D), np.exp(-2.0) * np.eye(D))
    return (mf, theta_mf), (fr, theta_fr)


def time_objectives(model, N, repeats, calls, warmup, fit_iters):
    (mf, theta_mf), (fr, theta_fr) = objectives(model, N)
    for obj, theta in ((mf, theta_mf), (fr, theta_fr)):
        value, grad = obj(theta)
        assert np.isfinite(value) and np.all(np.isfinite(grad))
    out = dict(exclusive_kl_meanfield=median_per_call(lambda: mf(theta_mf), repeats, calls, warmup),
               exclusive_kl_fullrank=median_per_call(lambda: fr(theta_fr), repeats, calls, warmup))
    RMSProp(0.01).optimize(10, mf, theta_mf, on_device=True)
    t0 = time.perf_counter()
    res = RMSProp(0.01).optimize(fit_iters, mf, theta_mf, on_device=True)
    dt = time.perf_counter() - t0
    assert np.all(np.isfinite(res['value_history']))
    out['device_fit'] = dict(iters=fit_iters, total_ms=1e3 * dt, per_iter_ms=1e3 * dt / fit_iters)
    return out


def copy_time_ms(n_bytes, repeats, calls):
    """Median time of a device-to-device copy of n_bytes: hipMemcpyAsync on the null stream of the HIP runtime the engine
    itself runs on (loaded already), device events around `calls` copies."""
    import ctypes
    hip = ctypes.CDLL(os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'lib', 'libamdhip64.so'))
    vp = ctypes.c_void_p

    def ok(rc):
        if rc != 0:
            raise RuntimeError('HIP call failed with status %d' % rc)
    src, dst, e0, e1 = vp(), vp(), vp(), vp()
    ok(hip.hipMalloc(ctypes.byref(src), ctypes.c_size_t(n_bytes)))
    ok(hip.hipMalloc(ctypes.byref(dst), ctypes.c_size_t(n_bytes)))
    ok(hip.hipMemset(src, 0, ctypes.c_size_t(n_bytes)))
    ok(hip.hipEventCreate(ctypes.byref(e0)))
    ok(hip.hipEventCreate(ctypes.byref(e1)))
    device_to_device = 3                                 # hipMemcpyDeviceToDevice
    per = []
    try:
        for r in range(repeats + 1):                     # (the first run is the warm-up)
            ok(hip.hipEventRecord(e0, None))
            for _ in range(calls):
                ok(hip.hipMemcpyAsync(dst, src, ctypes.c_size_t(n_bytes), device_to_device, None))
            ok(hip.hipEventRecord(e1, None))
            ok(hip.hipEventSynchronize(e1))
            ms = ctypes.c_float(0.0)
            ok(hip.hipEventElapsedTime(ctypes.byref(ms), e0, e1))
            if r:
                per.append(ms.value / calls)
    finally:
        hip.hipEventDestroy(e0), hip.hipEventDestroy(e1), hip.hipFree(src), hip.hipFree(dst)
    return float(np.median(per))


def time_gather(model, N, repeats, calls, warmup):
    D, B, n = model.dim, model.batch_size, model.n_data
    x = 0.3 * np.random.RandomState(1).randn(min(N, 64), D)
    state = [0]

    def moving():
        state[0] += 1
        model.batch = state[0]
        model.grad(x)

    def held():
        model.grad(x)
    t_moving = median_per_call(moving, repeats, calls, warmup)
    t_held = median_per_call(held, repeats, calls, warmup)
    ldb, ldp = (B + 15) // 16 * 16, (D + 15) // 16 * 16
    read = B * D * 8 + B * 8 + B * 4
    written = ldb * ldp * 8 + D * ldb * 8 + ldb * 8 + B * 4
    traffic = read + written
    copy_ms = copy_time_ms(traffic // 2, repeats, calls)
    ms = t_moving['median_ms'] - t_held['median_ms']
    return dict(rows_call_batch_moving=t_moving, rows_call_batch_held=t_held, index_and_gather_ms=ms,
                traffic_bytes=traffic, copy_same_traffic_ms=copy_ms,
                gather_over_copy=None if not copy_ms else ms / copy_ms, full_design_bytes=n * ldp * 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n-data', type=int, default=1 << 20)
    ap.add_argument('--p', type=int, default=64)
    ap.add_argument('--samples', type=int, default=1024)
    ap.add_argument('--batches', default='1024,4096,16384,65536')
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--fit-iters', type=int, default=1000)
    ap.add_argument('--full-fit-iters', type=int, default=100)
    args = ap.parse_args()
    n, p, N = args.n_data, args.p, args.samples
    rng = np.random.RandomState(0)
    X = rng.randn(n, p) / np.sqrt(p)
    y = (rng.rand(n) < 1.0 / (1.0 + np.exp(-(X @ rng.randn(p))))).astype(float)
    out = dict(n_data=n, p=p, N=N, batches={})
    for B in (int(b) for b in args.batches.split(',')):
        model = vb.MinibatchRegressionModel(X, y, B, seed=1)
        res = time_objectives(model, N, args.repeats, args.calls, args.warmup, args.fit_iters)
        res['gather'] = time_gather(model, N, args.repeats, args.calls, args.warmup)
        out['batches'][str(B)] = res
        del model
    full = vb.MinibatchRegressionModel(X, y, 1).full_model()
    out['full_model'] = time_objectives(full, N, max(3, args.repeats // 2), max(2, args.calls // 4), 2, args.full_fit_iters)
    for B, res in out['batches'].items():
        for key in ('exclusive_kl_meanfield', 'exclusive_kl_fullrank'):
            res['full_over_minibatch_' + key] = out['full_model'][key]['median_ms'] / res[key]['median_ms']
        res['full_over_minibatch_fit_iteration'] = out['full_model']['device_fit']['per_iter_ms'] / res['device_fit']['per_iter_ms']
    print(json.dumps(dict(minibatch_bench=out, repeats=args.repeats, calls=args.calls, warmup=args.warmup)))


if __name__ == '__main__':
    main()
