"""CPU: the dense-metric / adaptive HMC oracle (tests/_hmc_metric_oracle.py) against the properties of the algorithm, the
window schedule, the argument checks of ``hmc``'s two new keywords, the binding of ``vb_hmc_run_metric``, and the vetting
of every case the GPU test uses (accept margins of the parity grids, the statistical configurations)."""
import ctypes
import os

import numpy as np
import pytest

import _hmc_metric_oracle as MO
import _hmc_oracle as HO
from oracle import models as omod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the window schedule ---------------------------------------------------------------------------------------------------
SCHEDULE = {300: [(75, 100), (100, 150), (150, 250)],
            1000: [(75, 100), (100, 150), (150, 250), (250, 450), (450, 950)],
            150: [(75, 100)], 40: [(6, 36)], 20: [(3, 18)]}


@pytest.mark.parametrize('n_warmup', sorted(SCHEDULE))
def test_window_schedule(n_warmup):
    from viabel_amd.mcmc import _adaptation_windows
    assert _adaptation_windows(n_warmup) == SCHEDULE[n_warmup]
    assert MO.windows(n_warmup) == SCHEDULE[n_warmup]


def test_window_schedule_covers_the_slow_phase():
    from viabel_amd.mcmc import _adaptation_windows
    for n in range(20, 1200):
        w = _adaptation_windows(n)
        assert w == MO.windows(n)
        assert all(a[1] == b[0] for a, b in zip(w, w[1:])) and all(e > s for s, e in w)
        assert 0 < w[0][0] and w[-1][1] < n
    with pytest.raises(ValueError):
        _adaptation_windows(19)


# ---- 2. argument errors that need no engine -----------------------------------------------------------------------------------
def test_argument_errors_of_the_new_keywords():
    import viabel_amd as vb
    model = vb.GaussianModel(np.zeros(3), np.ones(3))
    ok = dict(n_chains=4, n_warmup=2, n_draws=2, n_leapfrog=2, init=np.zeros((4, 3)))
    spd = np.array([[2.0, 0.5, 0.0], [0.5, 1.0, 0.1], [0.0, 0.1, 1.5]])
    asym = spd.copy()
    asym[0, 1] += 0.1
    bad = [dict(metric='full'), dict(metric=None), dict(metric=1),
           dict(metric='diag', inv_mass=spd),                                              # a matrix needs metric='dense'
           dict(metric='dense', inv_mass=asym), dict(metric='dense', inv_mass=-spd),
           dict(metric='dense', inv_mass=np.diag([1.0, 0.0, 1.0])),
           dict(metric='dense', inv_mass=np.where(np.eye(3) > 0, np.nan, spd)),
           dict(metric='dense', inv_mass=np.ones((3, 2))), dict(metric='dense', inv_mass=np.ones(2)),
           dict(metric='dense', inv_mass=np.array([1.0, -1.0, 1.0])),
           dict(adapt_metric=True), dict(adapt_metric=True, n_warmup=19),                  # n_warmup < 20
           dict(adapt_metric=True, n_warmup=19, metric='dense')]
    for kw in bad:
        args = dict(ok)
        args.update(kw)
        with pytest.raises(ValueError):
            vb.hmc(model, **args)
    with pytest.raises(NotImplementedError):                                               # the refusals are unchanged
        vb.hmc(vb.CallableModel(3, lambda x: -0.5 * np.sum(x * x, axis=1)), metric='dense', **ok)
    rng = np.random.RandomState(0)
    X = rng.randn(40, 3)
    mini = vb.MinibatchRegressionModel(X, (rng.rand(40) < 0.5).astype(np.float64), 8)
    with pytest.raises(NotImplementedError):
        vb.hmc(mini, metric='dense', adapt_metric=True, **dict(ok, n_warmup=20))


# ---- 3. the binding -----------------------------------------------------------------------------------------------------------
def test_binding_declares_the_entry():
    from viabel_amd import _lib
    restype, argtypes = _lib.SIGNATURES['vb_hmc_run_metric']
    assert restype is ctypes.c_int and len(argtypes) == 28
    header = open(os.path.join(ROOT, 'include', 'viabel_hip.h')).read()
    assert 'int vb_hmc_run_metric(vb_ctx* ctx' in header
    assert '#define VB_HMC_METRIC_DIAG %d' % _lib.HMC_METRIC_DIAG in header
    assert '#define VB_HMC_METRIC_DENSE %d' % _lib.HMC_METRIC_DENSE in header
    assert hasattr(_lib.Engine, 'hmc_run_metric')
    lib = _lib.load()
    assert lib.vb_hmc_run_metric(*[None if t in (_lib._ctx_p, _lib._c_double_p, _lib._c_int64_p) else 0
                                   for t in argtypes]) == _lib.VB_ERR_INVALID


# ---- 4. the dense oracle with a diagonal factor is the diagonal oracle ----------------------------------------------------------
@pytest.mark.parametrize('kind', ['gauss', 'funnel', 'logistic'])
def test_dense_oracle_with_diagonal_factor_is_the_diagonal_oracle(kind):
    case = HO.parity_cases(kind, 9)[-1]
    host, _ = HO.parity_problem(kind, case['d'])
    z = HO.philox_normals(case['seed'], case['stream_offset'], 9, case['d'])
    ref = HO.run_case(host, case, z)
    kw = dict(n_warmup=HO.PARITY_WARMUP, n_draws=HO.PARITY_DRAWS, n_leapfrog=case['n_leapfrog'], step_size=case['step_size'],
              jitter=case['jitter'], seed=case['seed'], stream_offset=case['stream_offset'], thin=case['thin'])
    vg = HO.value_and_grad_of(host)
    dense = MO.run(vg, case['x0'], z, L=np.diag(np.sqrt(case['inv_mass'])), **kw)
    diag = MO.run(vg, case['x0'], z, inv_mass=case['inv_mass'], **kw)
    for k in ('draws', 'logp', 'last', 'chain_mean', 'chain_var', 'accept_prob', 'step_size_history', 'accept_rate'):
        scale = max(1.0, float(np.max(np.abs(ref[k]))))
        assert np.max(np.abs(dense[k] - ref[k])) <= 1e-12 * scale, k
        assert np.array_equal(diag[k], ref[k]), k
    assert np.array_equal(dense['accepted'], ref['accepted']) and dense['n_divergent'] == ref['n_divergent']
    assert dense['step_size'] == pytest.approx(ref['step_size'], rel=1e-12)


# ---- 5. reversibility of the dense trajectory -----------------------------------------------------------------------------------
@pytest.mark.parametrize('n_leapfrog', [1, 7])
def test_dense_trajectory_is_reversible(n_leapfrog):
    rng = np.random.RandomState(4)
    d, c, eps = 5, 6, 0.05
    host = omod.Funnel(d)
    vg = HO.value_and_grad_of(host)
    a = rng.randn(d, d)
    L = np.linalg.cholesky(a @ a.T / d + np.eye(d))

    def trajectory(x, r):
        g = vg(x)[1]
        r = r + 0.5 * eps * (g @ L)
        for l in range(n_leapfrog):
            x = x + eps * (r @ L.T)
            g = vg(x)[1]
            r = r + (0.5 * eps if l + 1 == n_leapfrog else eps) * (g @ L)
        return x, r

    x0, r0 = 0.5 * rng.randn(c, d), rng.randn(c, d)
    x1, r1 = trajectory(x0, r0)
    assert np.max(np.abs(x1 - x0)) > 1e-3
    x2, r2 = trajectory(x1, -r1)
    assert np.max(np.abs(x2 - x0)) < 1e-10 and np.max(np.abs(r2 + r0)) < 1e-10
    # and the oracle's own transition takes that trajectory: one iteration, accepted chains end at x1
    res = MO.run(vg, x0, r0[None], L=L, n_warmup=0, n_draws=1, n_leapfrog=n_leapfrog, step_size=eps)
    acc = res['accepted'][0]
    assert acc.any() and np.allclose(res['last'][acc], x1[acc], rtol=0, atol=1e-13)


# ---- 6. moments and a warm-up-only segment --------------------------------------------------------------------------------------
@pytest.mark.parametrize('dense', [False, True])
def test_oracle_moments_and_segments(dense):
    case = MO.moment_case(5, 17)
    host = omod.GaussDiag(case['mean'], case['sd'])
    vg = HO.value_and_grad_of(host)
    z = HO.philox_normals(case['seed'], 0, 5, 17)
    kw = dict(L=np.linalg.cholesky(case['sigma'])) if dense else dict(inv_mass=case['inv_mass'])
    res = MO.run(vg, case['x0'], z, n_warmup=0, n_draws=MO.MOMENT_ITERS, n_leapfrog=2, step_size=case['step_size'],
                 seed=case['seed'], moment_shift=case['shift'], **kw)
    xc = res['draws'].reshape(-1, 17) - case['shift']
    np.testing.assert_allclose(res['moment_sum'], xc.sum(axis=0), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(res['moment_m2'], xc.T @ xc if dense else np.sum(xc * xc, axis=0), rtol=1e-12, atol=1e-13)
    # 3 warm-up-only iterations, then 2 + 3 sampling ones, continue one 3 + 5 run's states (the step size aside)
    first = MO.run(vg, case['x0'], z, n_warmup=3, n_draws=0, n_leapfrog=2, step_size=case['step_size'], seed=case['seed'], **kw)
    assert first['draws'].shape == (0, 5, 17) and first['chain_var'] is None and first['next_stream'] == 3
    assert first['step_size_history'].shape == (3,) and np.isfinite(first['step_size'])


# ---- 7. vetting of the GPU test's cases ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', MO.PARITY_MODELS)
def test_parity_seeds_leave_a_margin(kind):
    """The GPU test compares accept decisions exactly, so no case may decide one within MIN_MARGIN.  The host normals here
    are within rounding of the device's; the bound is held at ten times the margin to cover that."""
    worst, n_cases = np.inf, 0
    for n_chains in MO.PARITY_CHAINS:
        for case in MO.parity_cases(kind, n_chains):
            host, _ = HO.parity_problem(kind, case['d'])
            z = HO.philox_normals(case['seed'], case['stream_offset'], n_chains, case['d'])
            runs = [MO.run_case(host, case, z)]
            if case['diagonal']:
                runs.append(MO.run_case(host, case, z, diag_route=True))
            for res in runs:
                assert res['min_margin'] >= 10.0 * HO.MIN_MARGIN, (case['key'], res['min_margin'])
                assert np.all(np.isfinite(res['last']))
                worst = min(worst, res['min_margin'])
            n_cases += 1
    print('%s: %d cases, smallest |log u - dH| = %.2e' % (kind, n_cases, worst))


@pytest.mark.parametrize('dense', [False, True])
def test_adaptive_seeds_leave_a_margin(dense):
    for n_chains in MO.ADAPT_CHAINS:
        for d in MO.ADAPT_DIMS:
            case = MO.adapt_case(n_chains, d, dense)
            host = omod.GaussDiag(case['mean'], case['sd'])
            z = HO.philox_normals(case['seed'], case['stream_offset'], n_chains, d)
            res = MO.run_adaptive(HO.value_and_grad_of(host), case['x0'], z, dense=dense,
                                  inv_mass=np.eye(d) if dense else np.ones(d), n_warmup=MO.ADAPT_WARMUP,
                                  n_draws=MO.ADAPT_DRAWS, n_leapfrog=case['n_leapfrog'], step_size=case['step_size'],
                                  jitter=case['jitter'], seed=case['seed'], stream_offset=case['stream_offset'])
            assert res['adapt_windows'] == [(6, 36)]
            assert res['min_margin'] >= 10.0 * HO.MIN_MARGIN, (case['key'], res['min_margin'])
            assert res['step_size_history'].shape == (MO.ADAPT_WARMUP + MO.ADAPT_DRAWS,)
            assert res['inv_mass'].shape == ((d, d) if dense else (d,)) and res['n_divergent'] == 0


def _rotated_figures(kw):
    host, mean, cov, start = MO.rotated_config()
    d = MO.ROT_DIM
    res = MO.run(HO.value_and_grad_of(host), start, HO.philox_normals(HO.STAT_SEED, 0, HO.STAT_CHAINS, d),
                 n_warmup=HO.STAT_WARMUP, n_draws=HO.STAT_DRAWS, n_leapfrog=HO.STAT_LEAPFROG, step_size=d ** -0.25,
                 target_accept=0.8, jitter=0.2, seed=HO.STAT_SEED, **kw)
    res['mean'], res['sd'], res['rhat'] = HO.combine_chains(res['chain_mean'], res['chain_var'], HO.STAT_DRAWS)
    return HO.stat_conditions('b', res, mean, cov), cov


def test_oracle_meets_statistical_conditions_dense_and_not_diagonal():
    """(a) of the GPU test: the rotated Gaussian under the exact dense metric meets the conditions; under the diagonal of
    the same covariance it does not (the trajectory is far too short for condition number 1e4): the case discriminates."""
    assert np.linalg.cond(MO.rotated_config()[2]) == pytest.approx(MO.ROT_COND, rel=1e-6)
    figures, cov = _rotated_figures(dict(L=np.linalg.cholesky(MO.rotated_config()[2])))
    for label, (value, bound, ok) in figures.items():
        print('(dense) %s: %s (bound %s)' % (label, value, bound))
    assert all(ok for _, _, ok in figures.values()), figures
    figures, _ = _rotated_figures(dict(inv_mass=np.diag(cov).copy()))
    for label, (value, bound, ok) in figures.items():
        print('(diagonal) %s: %s (bound %s)' % (label, value, bound))
    assert not figures['covariance error'][2] and not figures['max rhat'][2], figures


def test_oracle_meets_statistical_conditions_adaptive():
    """(b) of the GPU test: stat_config('a') from the unit metric with adaptation, 300 warm-up iterations, twelve leapfrog
    steps."""
    host, exact_mean, exact_cov, _, start, _ = HO.stat_config('a')
    d = exact_mean.size
    res = MO.run_adaptive(HO.value_and_grad_of(host), start, HO.philox_normals(HO.STAT_SEED, 0, HO.STAT_CHAINS, d),
                          dense=False, inv_mass=np.ones(d), n_warmup=MO.ADAPT_STAT_WARMUP, n_draws=HO.STAT_DRAWS,
                          n_leapfrog=MO.ADAPT_STAT_LEAPFROG, step_size=d ** -0.25, target_accept=0.8, jitter=0.2, seed=HO.STAT_SEED)
    res['mean'], res['sd'], res['rhat'] = HO.combine_chains(res['chain_mean'], res['chain_var'], HO.STAT_DRAWS)
    figures = HO.stat_conditions('a', res, exact_mean, exact_cov)
    ratio = res['inv_mass'] / np.diag(exact_cov)
    for label, (value, bound, ok) in figures.items():
        print('(adaptive) %s: %s (bound %s)' % (label, value, bound))
    print('(adaptive) inv_mass / sd^2 in [%.3f, %.3f]' % (ratio.min(), ratio.max()))
    assert all(ok for _, _, ok in figures.values()), figures
    assert 0.5 <= ratio.min() and ratio.max() <= 2.0
    assert res['adapt_windows'] == [(75, 100), (100, 150), (150, 250)]
