#!/usr/bin/env python3
"""What adapting the trajectory length buys and costs: hmc(trajectory='chees') against fixed numbers of leapfrog steps on
one GPU (csrc/vb_hmc.hip, vb_hmc_run_chees).

    python tools/hmc_chees_bench.py [--transitions T] [--chains C] [--rounds R] [--shapes ...] [--no-quality]
    rocprofv3 --kernel-trace --stats -d profiles/hmc_chees -- python tools/hmc_chees_bench.py --kernels-only --shapes logistic

Shapes: `logistic` and `multilevel` are tools/hmc_bench.py's (n_data = 16 384, D = 64; D = 117); `corrlogistic` is the
correlated-column logistic regression of examples/hmc_dense.py (D = 20), which tools/hmc_metric_bench.py --quality runs.
All in one process.

Quality (unless --no-quality), per shape: the unit diagonal metric, --quality-chains chains from 0.05 N(0, I), equal warm-up
(--warmup) and equal sampling transitions (--draws) for trajectory='chees' (max_leapfrog 128, from one leapfrog step) and
for n_leapfrog = 4, 16, 64.  Reported per run: max rhat, the smallest effective sample size over the coordinates per
gradient evaluation of the sampling phase (ESS of all chains / (chains x leapfrog steps taken)), the step size, T, and the
mean number of steps.

Cost, per shape, C = 1024 chains, T transitions, jitter 0.2, no draws kept, one unrecorded run of each kind first, R
alternating rounds, medians; the host clock around each whole call (all end synchronised):
  sampling   Engine.hmc_run_chees without warm-up at T_traj = 32 steps (mean 16 steps, at most 64) against
             Engine.hmc_run_metric at the nearest whole n_leapfrog: ms per transition and per leapfrog step of both
  warm-up    a warm-up-only segment with trajectory_lr = 0 (the length moves only with the clamp) against a warm-up-only
             segment of the fixed route at the nearest n_leapfrog; `warmup_overhead_ms_per_transition` is what the ChEES
             segment takes beyond its own number of leapfrog steps at the fixed route's time per step: the 8-byte fetch
             and the two criterion kernels of every iteration
--kernels-only: two ChEES runs per shape (T warm-up and T sampling transitions each; the unit diagonal metric, then a
dense one, whose warm-up has the velocity product) and nothing else, for the profiler.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'examples'))
import viabel_amd as vb   # noqa: E402
from viabel_amd import _lib   # noqa: E402
from viabel_amd._chain_stats import ess   # noqa: E402

FIXED_STEPS = (4, 16, 64)
STEP, MEAN_STEPS, MAX_STEPS = 0.02, 16, 64


def build(shape):
    if shape == 'corrlogistic':
        import hmc_dense
        return hmc_dense.problem(), dict(n_data=500)
    import hmc_bench
    return hmc_bench.build(shape)


def quality(model, args):
    d = model.dim
    init = 0.05 * np.random.RandomState(1).randn(args.quality_chains, d)
    common = dict(n_chains=args.quality_chains, n_warmup=args.warmup, n_draws=args.draws, init=init, inv_mass=np.ones(d), seed=1)
    runs = [('chees', dict(trajectory='chees', max_leapfrog=128))] + [('L=%d' % n, dict(n_leapfrog=n)) for n in FIXED_STEPS]
    out = {}
    for name, kw in runs:
        res = vb.hmc(model, **dict(common, **kw))
        draws = res['draws']
        n, c, _ = draws.shape
        smallest = min(ess(draws[:, :, j].T) for j in range(d))
        sampling_steps = int(res['n_leapfrog_history'][args.warmup:].sum())
        out[name] = dict(max_rhat=float(np.max(res['rhat'])), min_ess=float(smallest),
                         min_ess_per_grad_eval=float(smallest) / (c * sampling_steps), sampling_leapfrog_steps=sampling_steps,
                         warmup_leapfrog_steps=int(res['n_leapfrog_history'][:args.warmup].sum()), step_size=res['step_size'],
                         trajectory_length=float(res['trajectory_length']),
                         mean_steps=float(res['n_leapfrog_history'][args.warmup:].mean()), n_divergent=res['n_divergent'])
    return out


def timed(fn, other, rounds):
    """Median seconds of ``fn`` and ``other`` over alternating rounds, and the last result of each."""
    a_s, b_s, a, b = [], [], None, None
    for _ in range(rounds):
        t0 = time.perf_counter()
        a = fn()
        a_s.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        b = other()
        b_s.append(time.perf_counter() - t0)
    return float(np.median(a_s)), float(np.median(b_s)), a, b, a_s, b_s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--transitions', type=int, default=20)
    ap.add_argument('--chains', type=int, default=1024)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--shapes', nargs='*', default=['logistic', 'multilevel', 'corrlogistic'])
    ap.add_argument('--quality-chains', type=int, default=128)
    ap.add_argument('--warmup', type=int, default=200)
    ap.add_argument('--draws', type=int, default=200)
    ap.add_argument('--no-quality', action='store_true')
    ap.add_argument('--kernels-only', action='store_true')
    args = ap.parse_args()
    T, C = args.transitions, args.chains
    eng = _lib.default_engine()
    out = dict(tool='hmc_chees_bench', chains=C, transitions=T, shapes=[])
    for shape in args.shapes:
        model, rec = build(shape)
        d = model.dim
        rec.update(shape=shape, D=d)
        x0 = 0.05 * np.random.RandomState(1).randn(C, d)
        metric = np.ones(d)
        state = np.array([np.log(2 * MEAN_STEPS * STEP), 0.0, np.log(2 * MEAN_STEPS * STEP), 0.0])
        eng.set_model(model.device_spec())
        common = dict(jitter=0.2, seed=3, keep_draws=False)
        if args.kernels_only:
            a = np.random.RandomState(2).randn(d, d)
            eng.hmc_run_chees(x0, metric, T, T, MAX_STEPS, STEP, state, **common)
            eng.hmc_run_chees(x0, np.linalg.cholesky(a @ a.T / d + np.eye(d)), T, T, MAX_STEPS, STEP, state, **common)
            out['shapes'].append(rec)
            continue
        # sampling
        chees = lambda: eng.hmc_run_chees(x0, metric, 0, T, MAX_STEPS, STEP, state, **common)                 # noqa: E731
        steps = int(chees()['n_leapfrog_history'].sum())
        nearest = max(1, int(round(steps / T)))
        fixed = lambda: eng.hmc_run_metric(x0, metric, 0, T, nearest, STEP, **common)                        # noqa: E731
        fixed()
        chees_s, fixed_s, _, _, chees_all, fixed_all = timed(chees, fixed, args.rounds)
        rec['sampling'] = dict(chees_leapfrog_steps=steps, fixed_n_leapfrog=nearest,
                               chees_ms_per_transition=1e3 * chees_s / T, fixed_ms_per_transition=1e3 * fixed_s / T,
                               chees_ms_per_step=1e3 * chees_s / steps, fixed_ms_per_step=1e3 * fixed_s / (T * nearest),
                               chees_ms_all=[1e3 * s / T for s in chees_all], fixed_ms_all=[1e3 * s / T for s in fixed_all])
        # warm-up: the per-iteration fetch and the criterion kernels
        warm = lambda: eng.hmc_run_chees(x0, metric, T, 0, MAX_STEPS, STEP, state, trajectory_lr=0.0, **common)   # noqa: E731
        steps = int(warm()['n_leapfrog_history'].sum())
        nearest = max(1, int(round(steps / T)))
        fixed_warm = lambda: eng.hmc_run_metric(x0, metric, T, 0, nearest, STEP, **common)                   # noqa: E731
        fixed_warm()
        warm_s, fixed_s, _, _, warm_all, fixed_all = timed(warm, fixed_warm, args.rounds)
        per_step = fixed_s / (T * nearest)
        rec['warmup'] = dict(chees_leapfrog_steps=steps, fixed_n_leapfrog=nearest, chees_ms_per_transition=1e3 * warm_s / T,
                             fixed_ms_per_transition=1e3 * fixed_s / T, chees_ms_per_step=1e3 * warm_s / steps,
                             fixed_ms_per_step=1e3 * per_step,
                             warmup_overhead_ms_per_transition=1e3 * (warm_s - per_step * steps) / T,
                             chees_ms_all=[1e3 * s / T for s in warm_all], fixed_ms_all=[1e3 * s / T for s in fixed_all])
        if not args.no_quality:
            rec['quality'] = quality(model, args)
            rec['quality_run'] = dict(chains=args.quality_chains, warmup=args.warmup, draws=args.draws)
        out['shapes'].append(rec)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
