#!/usr/bin/env python3
"""Times posterior prediction on the device (predict_from_draws -> vb_glm_predict, csrc/vb_psis_batch.hip) on one GPU.

    python tools/predict_bench.py [--m M] [--dim D] [--draws S] [--repeats R] [--calls K] [--host-calls H] [--warmup W]

Logistic regression, m = 16 384 observations, D = 64, S = 4096 weighted draws.  Four routes to the predictions of the
model's own design:
  device        predict_from_draws(x, log_weights=lw): all five outputs, five m-vectors come back;
  device_upload the same with the design handed over as X_new / y_new (what held-out rows cost: m x D doubles go up);
  pointwise     what existed before for the bound design: pointwise_log_likelihood(x) brings the S x m matrix to the host
                (512 MiB at the default shape) and numpy reduces it -- to lpd ALONE, the one output that matrix allows;
  numpy         plain numpy on the same draws: the product, the link and the five weighted reductions.

Method (tools/locscale_bench.py): W warm-up calls, then R runs of K blocking calls each (H for the two host routes, whose
calls take seconds), every device call ending in the engine's own wait; the figure is the median over the runs of
(run time / calls).  Prints one JSON line.
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


def lse(a, axis):
    mx = np.max(a, axis=axis, keepdims=True)
    return np.log(np.sum(np.exp(a - mx), axis=axis)) + np.squeeze(mx, axis=axis)


def predict_numpy(X, y, x, lw):
    """All five outputs for the logistic model (the definitions of vb_glm_predict)."""
    w = np.exp(lw)
    eta = X @ x.T                                            # (m, S)
    t = np.exp(-np.abs(eta))
    mu = np.where(eta >= 0, 1.0, t) / (1.0 + t)
    eta_mean, mean = eta @ w, mu @ w
    eta_var = ((eta - eta_mean[:, None]) ** 2) @ w
    var = (t / (1.0 + t) ** 2) @ w + ((mu - mean[:, None]) ** 2) @ w
    ll = y[:, None] * eta - (np.maximum(eta, 0.0) + np.log1p(t))
    return dict(eta_mean=eta_mean, eta_var=eta_var, mean=mean, var=var, lpd=lse(ll + lw[None, :], 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--m', type=int, default=16384)
    ap.add_argument('--dim', type=int, default=64)
    ap.add_argument('--draws', type=int, default=4096)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--calls', type=int, default=400)
    ap.add_argument('--host-calls', type=int, default=1)
    ap.add_argument('--warmup', type=int, default=2)
    args = ap.parse_args()
    m, D, S = args.m, args.dim, args.draws
    rng = np.random.RandomState(0)
    X = rng.randn(m, D) / np.sqrt(D)
    beta = rng.randn(D)
    y = (rng.rand(m) < 1.0 / (1.0 + np.exp(-X @ beta))).astype(float)
    x = beta + 0.3 * rng.randn(S, D)
    lw = 0.8 * rng.standard_t(5.0, S)
    lw -= lse(lw, 0)
    model = vb.LogisticRegressionModel(X, y, prior_sd=10.0)

    def pointwise_route():
        ll = model.pointwise_log_likelihood(x)               # (S, m) on the host
        return lse(ll + lw[:, None], 0)

    dev = model.predict_from_draws(x, log_weights=lw)
    ref = predict_numpy(X, y, x, lw)
    agree = {k: float(np.max(np.abs(dev[k] - ref[k])) / np.max(np.abs(ref[k]))) for k in ref}
    agree['lpd_vs_pointwise_route'] = float(np.max(np.abs(dev['lpd'] - pointwise_route())) / np.max(np.abs(ref['lpd'])))
    host_repeats = max(3, args.repeats // 2)
    out = dict(
        m=m, D=D, S=S, matrix_mib=m * S * 8 / 2.0 ** 20,
        device=median_per_call(lambda: model.predict_from_draws(x, log_weights=lw), args.repeats, args.calls, args.warmup),
        device_upload=median_per_call(lambda: model.predict_from_draws(x, X_new=X, y_new=y, log_weights=lw), args.repeats,
                                      args.calls, args.warmup),
        pointwise=median_per_call(pointwise_route, host_repeats, args.host_calls, 1),
        numpy=median_per_call(lambda: predict_numpy(X, y, x, lw), host_repeats, args.host_calls, 1),
        max_rel_difference_from_numpy=agree)
    out['pointwise_over_device'] = out['pointwise']['median_ms'] / out['device']['median_ms']
    out['numpy_over_device'] = out['numpy']['median_ms'] / out['device']['median_ms']
    print(json.dumps(dict(predict_bench=out, repeats=args.repeats, calls=args.calls, host_calls=args.host_calls,
                          warmup=args.warmup)))


if __name__ == '__main__':
    main()
