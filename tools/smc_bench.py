#!/usr/bin/env python3
"""Times adaptive tempered SMC with HMC moves on one GPU (csrc/vb_smc.hip): the device-resident run against
the same algorithm as a numpy loop around model.grad, and a stage's own kernels against the gradient evaluations it makes.

    python tools/smc_bench.py [--rounds R] [--configs logistic:1024 logistic:4096 multilevel:1024] [--no-baseline]
    rocprofv3 --kernel-trace --stats -d profiles/smc -- python tools/smc_bench.py --profile-only

Shapes: `logistic` -- LogisticRegressionModel at n_data = 16 384, D = 64; `multilevel` -- MultilevelRegressionModel at
p = 16, J = 100, n_data = 2048, D = 117 (tools/hmc_bench.py's).  The base is N(0, I) -- a poor one, far wider than the posterior: the run takes
dozens of stages (max_stages = 2000) --, n_moves = 2, n_leapfrog = 8, ess_target = 0.5.  Per configuration, R rounds of:
  device      Engine.smc_run: one call, one 16-byte round trip per stage and one download
  short       the same with n_leapfrog = 4.  The stages of both runs differ only from the second stage on (other moves, other
              temperatures), so the per-stage times are compared, not the runs: `ms_per_gradient` is the slope
              (ms_per_stage(8) - ms_per_stage(4)) / (2 * 4) -- one gradient evaluation and one leap kernel --, and
              `outside_gradient_share` = 1 - n_moves * n_leapfrog * ms_per_gradient / ms_per_stage: what the start of a stage
              (reweight, scan, search, gather, the round trip) and the begin, end and control kernels take
  hmc         Engine.hmc_run at the same shape, C = n chains, the same two step counts, no warm-up: the same slope and the
              same share for vb_hmc_run's transition, the yardstick measured in the same process
  baseline    (n = 1024 only, unless --no-baseline) tests/_smc_oracle.run over Engine.model_grad with the device's own
              normals: every gradient one blocking vb_model_grad call.  Its stage count and ancestors are compared with the
              device run's.
`resample_ms` is one Engine.smc_reweight call on the run's last log weights, upload and download included (an upper bound of
the stage's reweight + scan + search; the kernels' own times are in profiles/smc_kernel_stats.txt).  Prints one JSON line."""
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
MOVES, LEAPFROG, SHORT = 2, 8, 4


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


def timed(fn, rounds):
    out, secs = None, []
    for _ in range(rounds):
        t0 = time.perf_counter()
        out = fn()
        secs.append(time.perf_counter() - t0)
    return out, float(np.median(secs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--configs', nargs='*', default=['logistic:1024', 'logistic:4096', 'multilevel:1024'])
    ap.add_argument('--no-baseline', action='store_true')
    ap.add_argument('--profile-only', action='store_true')
    args = ap.parse_args()
    eng = _lib.default_engine()
    out = dict(tool='smc_bench', n_moves=MOVES, n_leapfrog=LEAPFROG, configs=[])
    models = {}
    for config in args.configs:
        shape, n = config.split(':')
        n = int(n)
        if shape not in models:
            models[shape] = build(shape)
        model, info = models[shape]
        d = model.dim
        rec = dict(info, shape=shape, D=d, n=n)
        loc, scale = np.zeros(d), np.ones(d)
        step = 0.5 * d ** -0.25
        eng.set_model(model.device_spec())
        run = lambda L=LEAPFROG: eng.smc_run(loc, scale, n, n_moves=MOVES, n_leapfrog=L, step_size=step, seed=3,   # noqa: E731
                                             max_stages=2000, keep_ancestors=True)
        first = run()
        if args.profile_only:
            rec.update(n_stages=first['n_stages'], log_evidence=first['log_evidence'])
            out['configs'].append(rec)
            continue
        run(SHORT)
        got, secs = timed(run, args.rounds)
        short, short_secs = timed(lambda: run(SHORT), args.rounds)
        per_stage, per_stage_short = 1e3 * secs / got['n_stages'], 1e3 * short_secs / short['n_stages']
        per_grad = (per_stage - per_stage_short) / (MOVES * (LEAPFROG - SHORT))
        u = got['logp'] - (-0.5 * np.sum(((got['particles'] - loc) / scale) ** 2, axis=1))
        eng.smc_reweight(u, 0.0, 0.5, 0.5)
        _, resample_secs = timed(lambda: eng.smc_reweight(u, 0.0, 0.5, 0.5), 5)
        rec.update(n_stages=got['n_stages'], n_stages_short=short['n_stages'], log_evidence=got['log_evidence'],
                   mean_accept=float(got['accept_prob'].mean()), n_divergent=got['n_divergent'], ms_per_stage=per_stage,
                   ms_per_stage_short=per_stage_short, ms_per_gradient=per_grad,
                   outside_gradient_share=1.0 - MOVES * LEAPFROG * per_grad / per_stage, resample_ms=1e3 * resample_secs)
        # vb_hmc_run's own figure at the same shape, in the same process
        x0, inv_mass = loc + scale * np.random.RandomState(1).randn(n, d), scale ** 2
        T = 20
        hmc = lambda L: eng.hmc_run(x0, inv_mass, 0, T, L, step, jitter=0.0, seed=3, keep_draws=False)   # noqa: E731
        hmc(LEAPFROG), hmc(SHORT)
        _, hs = timed(lambda: hmc(LEAPFROG), args.rounds)
        _, hs_short = timed(lambda: hmc(SHORT), args.rounds)
        h_tr, h_tr_short = 1e3 * hs / T, 1e3 * hs_short / T
        h_grad = (h_tr - h_tr_short) / (LEAPFROG - SHORT)
        rec.update(hmc_ms_per_transition=h_tr, hmc_ms_per_gradient=h_grad,
                   hmc_outside_gradient_share=1.0 - LEAPFROG * h_grad / h_tr)
        if n <= 1024 and not args.no_baseline:
            import _smc_oracle as SO
            cache = {}

            def normals(stream):
                if stream not in cache:
                    eng.noise_generate(NOISE_SLOT, n, d, 3, stream=stream)
                    cache[stream] = eng.noise_get_host(NOISE_SLOT, n, d).copy()
                return cache[stream]
            for s in range(1 + MOVES * got['n_stages']):      # fetched before the clock starts
                normals(s)
            t0 = time.perf_counter()
            ref = SO.run(eng.model_grad, loc, scale, normals, n_particles=n, n_moves=MOVES, n_leapfrog=LEAPFROG,
                         step_size=step, seed=3, max_stages=2000)
            base = time.perf_counter() - t0
            rec.update(baseline_ms_per_stage=1e3 * base / ref['n_stages'], speedup=base / secs,
                       same_stages=bool(ref['n_stages'] == got['n_stages']),
                       same_ancestors=bool(ref['n_stages'] == got['n_stages']
                                           and np.array_equal(ref['ancestors'], got['ancestors'])),
                       log_evidence_baseline=ref['log_evidence'])
        out['configs'].append(rec)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
