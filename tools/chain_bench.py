#!/usr/bin/env python3
"""Times FASO's convergence checks on the device-resident iterate chain (csrc/vb_chain.hip) against the host's
``_chain_stats`` on the same rows, and ``FASO.optimize`` with ``device_checks`` off and on.

(a) ``chain_ess_mcse``, ``chain_rhat`` (FASO's five trailing windows) and ``chain_mean`` at the headline shape --
    FullRankGaussian(1024) + ExclusiveKL, N = 4096, P = 525 312 -- over the last ``--rows`` (1000) iterates of a chain
    filled by an actual RMSProp device fit, against ``_chain_stats.MCSE`` / ``R_hat_convergence_check`` / ``np.mean`` on
    the rows fetched to the host.  The host MCSE is timed on a ``--host-cols`` (4 096) column slice and scaled by
    P / 4096 (it is a Python loop over the columns: linear in them); the host R-hat search and mean run in full, once.
(b) ``FASO(RMSProp, W_min=200).optimize`` for ``--iters`` (2 000) iterations at the same shape with ``device_checks``
    off (the parent's behaviour: every iterate and gradient downloaded, numpy checks) and on, alternating.
(c) the same at the NVP configuration (tools/nvp_bench.py: D = 256, K = 4, width 256, N = 4096, P = 1 052 672).

Host clock around calls that end in a device synchronise; one warm-up per leg, then ``--reps`` alternating repeats.
``--parts`` picks the parts.  Prints one JSON line.

Usage:  python tools/chain_bench.py [--parts a,b,c] [--rows 1000] [--iters 2000] [--reps 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FR_D, N_MC = 1024, 4096


def headline():
    import viabel_amd as vb
    rng = np.random.RandomState(0)
    A = rng.randn(FR_D, FR_D)
    model = vb.CorrelatedGaussianModel(rng.randn(FR_D), covariance=A @ A.T / FR_D + np.eye(FR_D))
    fr = vb.FullRankGaussian(FR_D)
    init = fr.pack(np.zeros(FR_D), np.exp(-1.0) * np.eye(FR_D))
    return (lambda: vb.ExclusiveKL(vb.FullRankGaussian(FR_D, seed=2, rng='philox'), model, N_MC)), init


def nvp():
    import viabel_amd as vb
    d, k, width = 256, 4, 256
    r = np.random.RandomState(3)
    A = r.randn(d, d)
    model = vb.CorrelatedGaussianModel(0.3 * r.randn(d), covariance=A @ A.T / d + np.eye(d))
    masks = np.array([[(j + i) % 2 for j in range(d)] for i in range(k)], dtype=float)
    layers = [[d, width], [width, d]]

    def make():
        flow = vb.NVPFlow(layers, layers, masks, vb.MFGaussian(d, seed=7, rng='philox'), np.zeros(2 * d), d)
        return vb.ExclusiveKL(flow, model, N_MC)
    p = make().approx.var_param_dim
    return make, 0.03 * np.random.RandomState(0).randn(p)


def timed(fn, eng):
    eng.sync()
    t0 = time.perf_counter()
    out = fn()
    eng.sync()
    return time.perf_counter() - t0, out


def part_a(args):
    from viabel_amd import _chain_stats as cs, optimization as opt
    make, init = headline()
    obj, sgo = make(), opt.RMSProp(0.01)
    eng = obj._engine()
    rows, p = args.rows, init.size
    windows = np.linspace(200, int(0.95 * rows), 5, dtype=int)
    eng.chain_open(p, rows)
    try:
        t_fit, _ = timed(lambda: obj.device_fit(rows, init, sgo._device_kind, sgo._device_hyper(), hist_len=0), eng)
        legs = {'ess_mcse': lambda: eng.chain_ess_mcse(rows), 'rhat_5_windows': lambda: eng.chain_rhat(windows),
                'mean': lambda: eng.chain_mean(rows)}
        for fn in legs.values():
            fn()
        dev = {name: [] for name in legs}
        for _ in range(args.reps):
            for name, fn in legs.items():
                dev[name].append(timed(fn, eng)[0])
        ess, mcse = eng.chain_ess_mcse(rows)
        worst = eng.chain_rhat(windows)
        t_fetch, host_rows = timed(lambda: eng.chain_fetch(0, rows), eng)
    finally:
        eng.chain_close()
    cols = np.linspace(0, p - 1, args.host_cols, dtype=int)
    block = np.ascontiguousarray(host_rows[:, cols])
    t0 = time.perf_counter()
    h_ess, h_mcse = cs.MCSE(block)
    t_mcse = time.perf_counter() - t0
    h_ess = np.asarray(h_ess)
    t0 = time.perf_counter()
    h_conv = cs.R_hat_convergence_check(list(host_rows), windows)
    t_rhat = time.perf_counter() - t0
    t0 = time.perf_counter()
    np.mean(host_rows[-rows:], axis=0)
    t_mean = time.perf_counter() - t0
    best = int(np.argmin(worst))
    return {
        'p': int(p), 'rows': int(rows), 'windows': [int(w) for w in windows], 'fit_ms_per_iter': 1e3 * t_fit / rows,
        'device_ms': {k: {'median': 1e3 * float(np.median(v)), 'all': [round(1e3 * t, 3) for t in v]} for k, v in dev.items()},
        'host_s': {'mcse_%d_cols' % args.host_cols: t_mcse, 'mcse_scaled_to_p': t_mcse * p / args.host_cols,
                   'rhat_5_windows': t_rhat, 'mean': t_mean, 'chain_fetch': t_fetch},
        'agreement': {'ess_max_rel': float(np.nanmax(np.abs(ess[cols] - h_ess) / h_ess)),
                      'mcse_max_rel': float(np.nanmax(np.abs(mcse[cols] - h_mcse) / h_mcse)),
                      'rhat_decision_equal': bool((bool(worst[best] <= 1.1), int(windows[best])) ==
                                                  (bool(h_conv[0]), int(h_conv[1])))},
        'ess_median': float(np.nanmedian(ess)),
    }


def faso_legs(make, init, args, lr):
    from viabel_amd import optimization as opt

    def run(device_checks, iters):
        obj = make()
        eng = obj._engine()
        faso = opt.FASO(opt.RMSProp(lr), W_min=200, device_checks=device_checks)
        t, res = timed(lambda: faso.optimize(iters, obj, init), eng)
        return t, res
    for mode in (False, True):
        run(mode, 250)          # warm-up: buffers, code objects, pinned ring, one stationarity check
    out = {'host_checks_s': [], 'device_checks_s': [], 'k_Rhat': [], 'k_stopped': []}
    for _ in range(args.reps):
        for mode in (False, True):
            t, res = run(mode, args.iters)
            out['device_checks_s' if mode else 'host_checks_s'].append(round(t, 3))
            out['k_Rhat'].append(res['k_Rhat'])
            out['k_stopped'].append(res['k_stopped'])
    out['iters'] = args.iters
    out['p'] = int(init.size)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parts', default='a,b,c')
    ap.add_argument('--rows', type=int, default=1000)
    ap.add_argument('--host-cols', type=int, default=4096)
    ap.add_argument('--iters', type=int, default=2000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    parts = args.parts.split(',')
    res = {}
    if 'a' in parts:
        res['a_statistics_headline'] = part_a(args)
    if 'b' in parts:
        res['b_faso_headline'] = faso_legs(*headline(), args, 0.01)
    if 'c' in parts:
        res['c_faso_nvp'] = faso_legs(*nvp(), args, 0.001)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
