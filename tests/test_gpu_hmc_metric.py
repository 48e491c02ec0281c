"""GPU: hmc()'s dense metric and metric adaptation (vb_hmc_run_metric, csrc/vb_hmc.hip, through Engine.hmc_run_metric and
hmc(metric=, adapt_metric=)) against the numpy oracle of tests/_hmc_metric_oracle.py, which is handed the normals the device
draws and computes the uniforms itself.  The scheme is test_gpu_hmc.py's: accept decisions must match exactly, the
real-valued outputs within ten times the change the oracle's perturbation hook produces in that output plus
1e-12 max|ref|."""

import numpy as np
import pytest

import _hmc_metric_oracle as MO
import _hmc_oracle as HO

pytestmark = pytest.mark.gpu

NOISE_SLOT = 5
OUTPUTS = ('draws', 'logp', 'last', 'chain_mean', 'chain_var', 'accept_prob', 'step_size_history')


@pytest.fixture(scope='module')
def vb():
    import viabel_amd
    from viabel_amd import _lib
    _lib.default_engine()
    return viabel_amd


_MODELS = {}


def _model(vb, kind, d):
    """(device model, host model); built once per (kind, d) and shared."""
    if (kind, d) not in _MODELS:
        host, spec = HO.parity_problem(kind, d)
        if kind == 'gauss':
            dev = vb.GaussianModel(spec['mean'], spec['sd'])
        elif kind == 'funnel':
            dev = vb.FunnelModel(d)
        elif kind == 'corr':
            dev = vb.CorrelatedGaussianModel(spec['mean'], covariance=spec['cov'])
        elif kind == 'logistic':
            dev = vb.LogisticRegressionModel(spec['X'], spec['y'], HO.PARITY_PRIOR_SD)
        else:
            dev = vb.SourceModel(d, HO.QUARTIC_SRC, spec['a'])
        _MODELS[(kind, d)] = (dev, host)
    return _MODELS[(kind, d)]


def _device_normals(seed, stream_offset, n_iter, n_chains, d):
    from viabel_amd import _lib
    eng = _lib.default_engine()
    out = np.empty((n_iter, n_chains, d))
    for t in range(n_iter):
        eng.noise_generate(NOISE_SLOT, n_chains, d, seed, stream=stream_offset + t)
        out[t] = eng.noise_get_host(NOISE_SLOT, n_chains, d)
    return out


def _device_run(vb, dev, case, diag_route=False, **override):
    kw = dict(n_chains=case['x0'].shape[0], n_warmup=MO.PARITY_WARMUP, n_draws=MO.PARITY_DRAWS,
              n_leapfrog=case['n_leapfrog'], step_size=case['step_size'], target_accept=0.8, jitter=case['jitter'],
              init=case['x0'], seed=case['seed'], stream_offset=case['stream_offset'], thin=case['thin'])
    kw.update(dict(inv_mass=case['inv_mass']) if diag_route else dict(metric='dense', inv_mass=case['sigma']))
    kw.update(override)
    return vb.hmc(dev, **kw)


def _tolerances(ref, pert, keys=OUTPUTS):
    return {k: 10.0 * float(np.max(np.abs(pert[k] - ref[k]))) + 1e-12 * float(np.max(np.abs(ref[k]))) for k in keys}


def _compare(got, ref, tol, label):
    """Largest error-to-tolerance ratio over the outputs in ``tol``."""
    worst = 0.0
    for k in tol:
        assert got[k].shape == ref[k].shape, (label, k, got[k].shape, ref[k].shape)
        err = float(np.max(np.abs(got[k] - ref[k])))
        print('%s %s: error %.3e, tolerance %.3e' % (label, k, err, tol[k]))
        assert err <= tol[k], (label, k, err, tol[k])
        if tol[k] > 0.0:
            worst = max(worst, err / tol[k])
    return worst


def _decisions_match(got, ref, n_warmup, thin, label, step_rel=1e-9):
    assert got['n_divergent'] == ref['n_divergent'], label
    assert np.array_equal(got['accept_rate'], ref['accept_rate']), label
    if thin == 1:                  # a chain's kept row changes exactly where its proposal was accepted
        moved = np.any(np.diff(got['draws'], axis=0) != 0.0, axis=2)
        assert np.array_equal(moved, ref['accepted'][n_warmup + 1:]), label
    assert got['step_size'] == pytest.approx(ref['step_size'], rel=step_rel), label
    assert got['next_stream'] == ref['next_stream']


# ---- 1. dense trajectory parity; 2. a diagonal matrix against the diagonal route ------------------------------------------------
@pytest.mark.parametrize('n_chains', MO.PARITY_CHAINS)
@pytest.mark.parametrize('kind', MO.PARITY_MODELS)
def test_dense_trajectory_parity(vb, kind, n_chains, capsys):
    worst = 0.0
    n_iter = MO.PARITY_WARMUP + MO.PARITY_DRAWS
    for case in MO.parity_cases(kind, n_chains):
        dev, host = _model(vb, kind, case['d'])
        z = _device_normals(case['seed'], case['stream_offset'], n_iter, n_chains, case['d'])
        ref = MO.run_case(host, case, z)
        pert = MO.run_case(host, case, z, perturb=np.random.RandomState(case['seed']))
        assert ref['min_margin'] >= HO.MIN_MARGIN, (case['key'], ref['min_margin'])
        got = _device_run(vb, dev, case)
        label = '%s C=%d D=%d L=%d thin=%d jitter=%g%s' % (kind, n_chains, case['d'], case['n_leapfrog'], case['thin'],
                                                         case['jitter'], ' diagonal' if case['diagonal'] else '')
        assert got['metric'] == 'dense' and got['adapt_windows'] == [] and np.array_equal(got['inv_mass'], case['sigma'])
        _decisions_match(got, ref, MO.PARITY_WARMUP, case['thin'], label)
        tol = _tolerances(ref, pert)
        worst = max(worst, _compare(got, ref, tol, label))
        if case['diagonal']:       # the same metric through the diagonal route: same decisions, same tolerance
            other = _device_run(vb, dev, case, diag_route=True)
            assert other['metric'] == 'diag'
            _decisions_match(other, ref, MO.PARITY_WARMUP, case['thin'], label + ' (diagonal route)')
            assert np.array_equal(other['accept_rate'], got['accept_rate'])
            for k in OUTPUTS:
                assert np.max(np.abs(other[k] - got[k])) <= tol[k], (label, k)
    capsys.readouterr()
    with capsys.disabled():
        print('\n%s, %d chains: largest error / tolerance = %.2e' % (kind, n_chains, worst))


# ---- 3. the new entry in DIAG kind without moments is today's hmc(), bit for bit -------------------------------------------------
@pytest.mark.parametrize('kind,n_chains', [('funnel', 5), ('logistic', 257)])
def test_diag_kind_without_moments_equals_hmc(vb, kind, n_chains):
    from viabel_amd import _lib
    case = HO.parity_cases(kind, n_chains)[-1]
    dev, _ = _model(vb, kind, case['d'])
    kw = dict(n_warmup=HO.PARITY_WARMUP, n_draws=HO.PARITY_DRAWS, n_leapfrog=case['n_leapfrog'], step_size=case['step_size'],
              target_accept=0.8, jitter=case['jitter'], seed=case['seed'], stream_offset=case['stream_offset'],
              thin=case['thin'])
    old = vb.hmc(dev, n_chains=n_chains, init=case['x0'], inv_mass=case['inv_mass'], **kw)
    eng = _lib.default_engine()
    eng.set_model(dev.device_spec())
    new = eng.hmc_run_metric(case['x0'], case['inv_mass'], kw.pop('n_warmup'), kw.pop('n_draws'), kw.pop('n_leapfrog'),
                             kw.pop('step_size'), **kw)
    for k in ('draws', 'logp', 'last', 'chain_mean', 'accept_rate', 'accept_prob', 'step_size_history'):
        assert np.array_equal(new[k], old[k]), k
    assert np.array_equal(new['chain_m2'] / (HO.PARITY_DRAWS - 1.0), old['chain_var'])
    assert new['step_size'] == old['step_size'] and new['n_divergent'] == old['n_divergent']
    assert new['moment_sum'] is None and new['moment_m2'] is None


# ---- 4. reproducibility and continuation ----------------------------------------------------------------------------------------
def _adaptive_run(vb, case, dense, **override):
    n_chains, d = case['x0'].shape
    kw = dict(n_chains=n_chains, n_warmup=MO.ADAPT_WARMUP, n_draws=MO.ADAPT_DRAWS, n_leapfrog=case['n_leapfrog'],
              step_size=case['step_size'], jitter=case['jitter'], init=case['x0'], inv_mass=np.ones(d), seed=case['seed'],
              stream_offset=case['stream_offset'], metric='dense' if dense else 'diag', adapt_metric=True)
    kw.update(override)
    return vb.hmc(vb.GaussianModel(case['mean'], case['sd']), **kw)


def test_bit_reproducible(vb):
    for kind, n_chains in (('corr', 5), ('logistic', 257)):
        cases = MO.parity_cases(kind, n_chains)
        for case in (cases[0], cases[-2]):
            dev, _ = _model(vb, kind, case['d'])
            one, two = _device_run(vb, dev, case), _device_run(vb, dev, case)
            for k in OUTPUTS + ('accept_rate', 'mean', 'sd', 'rhat'):
                assert np.array_equal(one[k], two[k], equal_nan=True), (kind, n_chains, k)
            assert one['step_size'] == two['step_size'] and one['n_divergent'] == two['n_divergent']
    for dense in (False, True):
        case = MO.adapt_case(64, 17, dense)
        one, two = _adaptive_run(vb, case, dense), _adaptive_run(vb, case, dense)
        for k in OUTPUTS + ('accept_rate', 'mean', 'sd', 'rhat', 'inv_mass'):
            assert np.array_equal(one[k], two[k], equal_nan=True), (dense, k)
        assert one['step_size'] == two['step_size']


@pytest.mark.parametrize('kind', ['funnel', 'logistic'])
def test_dense_continuation(vb, kind):
    case = MO.parity_cases(kind, 5)[-2]
    dev, _ = _model(vb, kind, case['d'])
    whole = _device_run(vb, dev, case, n_warmup=0, n_draws=6, thin=1)
    first = _device_run(vb, dev, case, n_warmup=0, n_draws=3, thin=1)
    assert first['next_stream'] == case['stream_offset'] + 3
    second = _device_run(vb, dev, case, n_warmup=0, n_draws=3, thin=1, init=first['last'], step_size=first['step_size'],
                         stream_offset=first['next_stream'])
    assert np.array_equal(second['last'], whole['last'])
    assert np.array_equal(np.concatenate([first['draws'], second['draws']]), whole['draws'])
    assert np.array_equal(np.concatenate([first['logp'], second['logp']]), whole['logp'])
    assert second['next_stream'] == whole['next_stream']


# ---- 5. moments -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dense', [False, True])
@pytest.mark.parametrize('d', MO.MOMENT_DIMS)
@pytest.mark.parametrize('n_chains', MO.MOMENT_CHAINS)
def test_moments(vb, n_chains, d, dense):
    """S1 and S2 against numpy on the returned draws, componentwise within 4 n 2^-53 sum|terms|: the rounding bound of a
    length-n sum (n = 5 C terms; the subtraction of the shift is exact in neither, and is the same operation in both)."""
    from viabel_amd import _lib
    case = MO.moment_case(n_chains, d)
    eng = _lib.default_engine()
    eng.set_model(vb.GaussianModel(case['mean'], case['sd']).device_spec())
    metric = np.linalg.cholesky(case['sigma']) if dense else case['inv_mass']
    out = eng.hmc_run_metric(case['x0'], metric, 0, MO.MOMENT_ITERS, 2, case['step_size'], jitter=0.2, seed=case['seed'],
                             moment_shift=case['shift'])
    assert out['draws'].shape == (MO.MOMENT_ITERS, n_chains, d)
    xc = out['draws'].reshape(-1, d) - case['shift']
    n = float(xc.shape[0])
    bound = 4.0 * n * 2.0 ** -53
    s1, s1_abs = xc.sum(axis=0), np.abs(xc).sum(axis=0)
    assert np.all(np.abs(out['moment_sum'] - s1) <= bound * s1_abs), np.max(np.abs(out['moment_sum'] - s1) / s1_abs)
    if dense:
        s2, s2_abs = xc.T @ xc, np.abs(xc).T @ np.abs(xc)
        assert out['moment_m2'].shape == (d, d) and np.array_equal(out['moment_m2'], out['moment_m2'].T)
    else:
        s2 = s2_abs = np.sum(xc * xc, axis=0)
        assert out['moment_m2'].shape == (d,)
    err = np.abs(out['moment_m2'] - s2)
    print('C=%d D=%d dense=%s: largest S2 error / bound %.3f' % (n_chains, d, dense, np.max(err / (bound * s2_abs))))
    assert np.all(err <= bound * s2_abs)
    # the moments change nothing else: the same call without them returns the same draws
    plain = eng.hmc_run_metric(case['x0'], metric, 0, MO.MOMENT_ITERS, 2, case['step_size'], jitter=0.2, seed=case['seed'])
    assert np.array_equal(plain['draws'], out['draws']) and plain['moment_sum'] is None


# ---- 6. adaptive parity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dense', [False, True])
@pytest.mark.parametrize('d', MO.ADAPT_DIMS)
@pytest.mark.parametrize('n_chains', MO.ADAPT_CHAINS)
def test_adaptive_parity(vb, n_chains, d, dense):
    from oracle import models as omod
    case = MO.adapt_case(n_chains, d, dense)
    n_iter = MO.ADAPT_WARMUP + MO.ADAPT_DRAWS
    z = _device_normals(case['seed'], case['stream_offset'], n_iter, n_chains, d)
    vg = HO.value_and_grad_of(omod.GaussDiag(case['mean'], case['sd']))
    kw = dict(dense=dense, inv_mass=np.eye(d) if dense else np.ones(d), n_warmup=MO.ADAPT_WARMUP, n_draws=MO.ADAPT_DRAWS,
              n_leapfrog=case['n_leapfrog'], step_size=case['step_size'], jitter=case['jitter'], seed=case['seed'],
              stream_offset=case['stream_offset'])
    ref = MO.run_adaptive(vg, case['x0'], z, **kw)
    pert = MO.run_adaptive(vg, case['x0'], z, perturb=np.random.RandomState(case['seed']), **kw)
    assert ref['min_margin'] >= HO.MIN_MARGIN, (case['key'], ref['min_margin'])
    got = _adaptive_run(vb, case, dense)
    label = 'adaptive C=%d D=%d %s' % (n_chains, d, 'dense' if dense else 'diag')
    assert got['adapt_windows'] == [(6, 36)] == ref['adapt_windows']
    assert got['metric'] == ('dense' if dense else 'diag')
    assert got['inv_mass'].shape == ((d, d) if dense else (d,))
    assert got['step_size_history'].shape == (n_iter,) and got['accept_prob'].shape == (n_iter,)
    # (ref['accepted'] covers all segments' iterations.  The final step is an output like the others here: forty iterations
    # of dual averaging, restarted twice, carry a rounding difference further than the parity grid's three)
    step_rel = 10.0 * abs(pert['step_size'] / ref['step_size'] - 1.0) + 1e-12
    _decisions_match(got, ref, MO.ADAPT_WARMUP, 1, label, step_rel=step_rel)
    _compare(got, ref, _tolerances(ref, pert, OUTPUTS + ('inv_mass',)), label)


# ---- 7. statistics against closed forms -----------------------------------------------------------------------------------------
def test_statistics_dense_on_a_rotated_gaussian(vb):
    """(a) D = 16, covariance condition number 1e4, the exact covariance as the dense metric.  The oracle on host normals:
    mean error / sd 0.059 (bound 0.15), covariance error 0.048 (0.25), max rhat 1.026 (1.05), acceptance 0.80, no
    divergences; with the diagonal of the same covariance it misses: covariance error 0.75, max rhat 3.5."""
    _, mean, cov, start = MO.rotated_config()
    dev = vb.CorrelatedGaussianModel(mean, covariance=cov)
    res = vb.hmc(dev, n_chains=HO.STAT_CHAINS, n_warmup=HO.STAT_WARMUP, n_draws=HO.STAT_DRAWS, n_leapfrog=HO.STAT_LEAPFROG,
                 init=start, inv_mass=cov, metric='dense', seed=HO.STAT_SEED)
    figures = HO.stat_conditions('b', res, mean, cov)
    for label, (value, bound, ok) in figures.items():
        print('(a) %s: %s (bound %s)' % (label, value, bound))
    assert all(ok for _, _, ok in figures.values()), figures


def test_statistics_adapted_from_ones(vb):
    """(b) stat_config('a') from inv_mass = ones with adapt_metric=True, 300 warm-up iterations and twelve leapfrog steps.
    The oracle on host normals: mean error / sd 0.017 (bound 0.15), sd ratio error 0.019 (0.15), max rhat 0.998 (1.05),
    acceptance 0.84, no divergences, adapted inv_mass / sd^2 in [0.970, 1.045] (bound [0.5, 2]); with eight leapfrog
    steps its max rhat is 1.037, too close to the bound."""
    _, exact_mean, exact_cov, _, start, spec = HO.stat_config('a')
    dev = vb.GaussianModel(spec['mean'], spec['sd'])
    res = vb.hmc(dev, n_chains=HO.STAT_CHAINS, n_warmup=MO.ADAPT_STAT_WARMUP, n_draws=HO.STAT_DRAWS,
                 n_leapfrog=MO.ADAPT_STAT_LEAPFROG, init=start, inv_mass=np.ones(16), adapt_metric=True, seed=HO.STAT_SEED)
    figures = HO.stat_conditions('a', res, exact_mean, exact_cov)
    ratio = res['inv_mass'] / np.diag(exact_cov)
    for label, (value, bound, ok) in figures.items():
        print('(b) %s: %s (bound %s)' % (label, value, bound))
    print('(b) inv_mass / sd^2 in [%.3f, %.3f]' % (ratio.min(), ratio.max()))
    assert all(ok for _, _, ok in figures.values()), figures
    assert 0.5 <= ratio.min() and ratio.max() <= 2.0
    assert res['adapt_windows'] == [(75, 100), (100, 150), (150, 250)]
    assert res['step_size_history'].shape == (MO.ADAPT_STAT_WARMUP + HO.STAT_DRAWS,)


# ---- 8. end to end --------------------------------------------------------------------------------------------------------------
def test_end_to_end_dense_from_laplace(vb, capsys):
    rng = np.random.RandomState(8)
    d, n = 10, 300
    X = rng.randn(n, d) / np.sqrt(d)
    y = (rng.rand(n) < 1.0 / (1.0 + np.exp(-X @ rng.randn(d)))).astype(np.float64)
    model = vb.LogisticRegressionModel(X, y, 3.0)
    lap = vb.laplace_approximation(model)
    post_sd = np.sqrt(np.diag(lap['cov']))
    capsys.readouterr()
    res = vb.hmc(model, n_chains=64, n_warmup=100, n_draws=100, n_leapfrog=8, var_param=lap['var_param'],
                 approx=lap['approx'], metric='dense')
    out = capsys.readouterr().out
    assert 'hmc: step size' in out and 'max rhat' in out and 'divergent' in out
    assert res['metric'] == 'dense' and res['inv_mass'].shape == (d, d)
    np.testing.assert_allclose(res['inv_mass'], lap['cov'], rtol=1e-10)
    assert np.max(res['rhat']) <= 1.05
    assert np.all(np.abs(res['mean'] - lap['mode']) <= 0.5 * post_sd)
    assert res['draws'].shape == (100, 64, d) and res['n_divergent'] == 0


# ---- 9. errors at the C entry ---------------------------------------------------------------------------------------------------
def test_errors(vb):
    from viabel_amd import _lib
    eng = _lib.default_engine()
    model = vb.GaussianModel(np.zeros(3), np.ones(3))
    eng.set_model(model.device_spec())
    x0, L = np.zeros((4, 3)), np.eye(3)
    ok = dict(n_warmup=1, n_draws=2, n_leapfrog=2, step_size=0.5)
    still_works = lambda: np.testing.assert_allclose(eng.model_grad(np.ones((2, 3)))[1], -np.ones((2, 3)))   # noqa: E731
    below = np.eye(3)
    below[2, 0] = np.nan
    for bad in (np.diag([1.0, 0.0, 1.0]), np.diag([1.0, -1.0, 1.0]), np.diag([1.0, np.inf, 1.0]), below):
        with pytest.raises(ValueError):
            eng.hmc_run_metric(x0, bad, **ok)
        still_works()
    above = np.eye(3)
    above[0, 2] = np.nan                                # (entries above the diagonal are ignored)
    assert np.all(np.isfinite(eng.hmc_run_metric(x0, above, **ok)['last']))
    for kw in (dict(n_warmup=0, n_draws=0), dict(n_draws=-1), dict(n_warmup=-1), dict(n_leapfrog=0), dict(step_size=0.0)):
        with pytest.raises(ValueError):
            eng.hmc_run_metric(x0, L, **dict(ok, **kw))
        still_works()
    with pytest.raises(ValueError):                     # d different from the model's dimension
        eng.hmc_run_metric(np.zeros((4, 2)), np.eye(2), **ok)
    # a warm-up-only segment: the sampling outputs are None, the histories and the final step are there
    seg = eng.hmc_run_metric(x0, L, 3, 0, 2, 0.5)
    assert seg['draws'] is None and seg['chain_mean'] is None and seg['accept_rate'] is None
    assert seg['last'].shape == (4, 3) and seg['step_size_history'].shape == (3,) and seg['step_size'] > 0.0
    # the raw entry: the kind, and the moments' three pointers together
    lib, ctx = eng._lib, eng._ctx
    p = lambda a: a.ctypes.data                                                                               # noqa: E731
    o = {k: np.zeros(s) for k, s in (('last', (4, 3)), ('sh', 3), ('ah', 3), ('final', 1), ('shift', 3), ('s1', 3),
                                     ('s2', (3, 3)))}

    def call(kind=_lib.HMC_METRIC_DENSE, shift=None, s1=None, s2=None):
        return lib.vb_hmc_run_metric(ctx, p(x0), kind, p(L), 4, 3, 3, 0, 1, 2, 0.5, 0.8, 0.2, 1, 0, shift, s1, s2, None, None,
                                     p(o['last']), None, None, None, p(o['sh']), p(o['ah']), p(o['final']), None)

    assert call() == _lib.VB_OK
    assert call(kind=2) == _lib.VB_ERR_INVALID and call(kind=-1) == _lib.VB_ERR_INVALID
    assert call(shift=p(o['shift'])) == _lib.VB_ERR_INVALID
    assert call(s1=p(o['s1']), s2=p(o['s2'])) == _lib.VB_ERR_INVALID
    assert call(shift=p(o['shift']), s1=p(o['s1']), s2=p(o['s2'])) == _lib.VB_OK
    assert np.array_equal(o['s2'], o['s2'].T) and np.all(np.isfinite(o['s2']))
    still_works()
    # the refusals of vb_hmc_run: a communicator, a host-callback model
    fresh = _lib.Engine()
    try:
        with pytest.raises(_lib.EngineError):
            fresh.hmc_run_metric(x0, L, **ok)
        fresh.set_model(model.device_spec())
        fresh.comm_init_host(lambda arr, op: None, 1, 0)
        with pytest.raises(NotImplementedError) as info:
            fresh.hmc_run_metric(x0, L, **ok)
        assert 'communicator' in str(info.value)
        fresh.comm_destroy()
        callback = vb.CallableModel(3, lambda x: -0.5 * np.sum(x * x, axis=1), lambda x: -x)
        fresh.set_model(callback.device_spec())
        with pytest.raises(NotImplementedError) as info:
            fresh.hmc_run_metric(x0, L, **ok)
        assert 'callback' in str(info.value)
    finally:
        fresh.close()
    # the dense kind's capacity: d <= 4096
    wide = vb.GaussianModel(np.zeros(4097), np.ones(4097))
    eng.set_model(wide.device_spec())
    with pytest.raises(NotImplementedError) as info:
        eng.hmc_run_metric(np.zeros((1, 4097)), np.eye(4097), **ok)
    assert '4096' in str(info.value)
    assert eng.hmc_run_metric(np.zeros((1, 4097)), np.ones(4097), **ok)['last'].shape == (1, 4097)
    eng.set_model(model.device_spec())
    still_works()
