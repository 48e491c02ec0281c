#!/usr/bin/env python3
"""Times many-chain HMC on one GPU (csrc/vb_hmc.hip): the device-resident loop against a numpy leapfrog around
model.grad, which is what a user could write before vb_hmc_run existed.

    python tools/hmc_bench.py [--transitions T] [--chains C] [--leapfrog L] [--rounds R] [--shapes logistic multilevel]
    rocprofv3 --kernel-trace --stats -d profiles/hmc -- python tools/hmc_bench.py --kernels-only

Shapes: `logistic` -- LogisticRegressionModel at n_data = 16 384, D = 64 (tools/predict_bench.py's); `multilevel` --
MultilevelRegressionModel at p = 16, J = 100, n_data = 2048, D = 117 (tools/multilevel_bench.py's (b)).  C = 1024 chains,
L = 16 leapfrog steps, T transitions without warm-up at a fixed step (jitter 0.2), one unrecorded device run first.
  device     Engine.hmc_run(keep_draws=False): one call, one synchronisation
  baseline   tests/_hmc_oracle.run over Engine.model_grad: every leapfrog step one blocking vb_model_grad call with C x D
             doubles up and C x D down.  It is given the device's own momenta (noise_generate / noise_get_host per stream,
             fetched before the clock starts) and computes the same uniforms, so both produce the same chains
The two alternate, R rounds each; the host clock runs around each whole run (both end synchronised); reported are the
medians in ms per transition, their ratio, and chain-leapfrog-steps per second (C L / time per transition).  The final
states are compared at the parity tolerance of tests/test_gpu_hmc.py (ten times what the oracle's perturbation hook moves
them, plus 1e-12 max|ref|).  `leap_bytes` is what one launch of the leap kernel moves: five C x D streams of doubles (p, gp
and xp read, p and xp written).  --kernels-only: one device run per shape and nothing else, for the profiler.  Prints one
JSON line."""
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

NOISE_SLOT = 5


def build(shape):
    rng = np.random.RandomState(0)
    if shape == 'logistic':
        n_data, d = 16384, 64
        X = rng.randn(n_data, d) / np.sqrt(d)
        y = (rng.rand(n_data) < 1.0 / (1.0 + np.exp(-X @ rng.randn(d)))).astype(float)
        return vb.LogisticRegressionModel(X, y, prior_sd=10.0), dict(n_data=n_data)
    p, J, n_data = 16, 100, 2048
    X = rng.randn(n_data, p) / np.sqrt(p)
    groups = rng.randint(0, J, size=n_data)
    eta = X @ rng.randn(p) + rng.randn(J)[groups]
    y = (rng.rand(n_data) < 1.0 / (1.0 + np.exp(-eta))).astype(float)
    return vb.MultilevelRegressionModel(X, y, groups, J), dict(n_data=n_data, p=p, J=J)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--transitions', type=int, default=40)
    ap.add_argument('--chains', type=int, default=1024)
    ap.add_argument('--leapfrog', type=int, default=16)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--shapes', nargs='*', default=['logistic', 'multilevel'])
    ap.add_argument('--kernels-only', action='store_true')
    args = ap.parse_args()
    T, C, L = args.transitions, args.chains, args.leapfrog
    eng = _lib.default_engine()
    out = dict(tool='hmc_bench', chains=C, leapfrog=L, transitions=T, shapes=[])
    for shape in args.shapes:
        model, rec = build(shape)
        d = model.dim
        rec.update(shape=shape, D=d, leap_bytes=5 * C * d * 8)
        rng = np.random.RandomState(1)
        x0 = 0.05 * rng.randn(C, d)
        inv_mass = np.ones(d)
        step = 0.02
        eng.set_model(model.device_spec())
        device = lambda: eng.hmc_run(x0, inv_mass, 0, T, L, step, jitter=0.2, seed=3, keep_draws=False)   # noqa: E731
        device()
        if args.kernels_only:
            out['shapes'].append(rec)
            continue
        import _hmc_oracle as HO
        z = np.empty((T, C, d))
        for t in range(T):
            eng.noise_generate(NOISE_SLOT, C, d, 3, stream=t)
            z[t] = eng.noise_get_host(NOISE_SLOT, C, d)
        baseline = lambda perturb=None: HO.run(eng.model_grad, x0, z, inv_mass=inv_mass, n_warmup=0, n_draws=T,   # noqa: E731
                                               n_leapfrog=L, step_size=step, jitter=0.2, seed=3, perturb=perturb)
        dev_s, base_s = [], []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            got = device()
            dev_s.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            ref = baseline()
            base_s.append(time.perf_counter() - t0)
        pert = baseline(np.random.RandomState(2))
        tol = 10.0 * float(np.max(np.abs(pert['last'] - ref['last']))) + 1e-12 * float(np.max(np.abs(ref['last'])))
        err = float(np.max(np.abs(got['last'] - ref['last'])))
        dev_ms, base_ms = 1e3 * float(np.median(dev_s)) / T, 1e3 * float(np.median(base_s)) / T
        rec.update(device_ms_per_transition=dev_ms, baseline_ms_per_transition=base_ms, speedup=base_ms / dev_ms,
                   device_chain_leapfrog_steps_per_s=C * L / (dev_ms * 1e-3),
                   baseline_chain_leapfrog_steps_per_s=C * L / (base_ms * 1e-3),
                   device_ms_all=[1e3 * s / T for s in dev_s], baseline_ms_all=[1e3 * s / T for s in base_s],
                   accept_rate=float(got['accept_rate'].mean()), same_accepts=bool(np.array_equal(
                       got['accept_rate'], ref['accept_rate'])), last_max_err=err, last_tolerance=tol,
                   last_within_tolerance=bool(err <= tol), min_margin=ref['min_margin'])
        out['shapes'].append(rec)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
