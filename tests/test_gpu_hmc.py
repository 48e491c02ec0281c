"""GPU: many-chain HMC on the device (vb_hmc_run, csrc/vb_hmc.hip, through Engine.hmc_run and hmc()) against the numpy oracle
of tests/_hmc_oracle.py, which is handed the momenta the device draws (noise_generate / noise_get_host per stream) and
computes the uniforms itself.  Accept decisions must match exactly; the real-valued outputs within a tolerance formed per
case and per output from the oracle's own perturbation hook: ten times the largest change that noise of the size the
project's model tests allow (1e-12 max|f| on values, 1e-11 max|g| on gradients) produces in that output, plus
1e-12 max|ref|.  The factor ten is a margin (one random perturbation underestimates an aligned one), not a measurement."""
import ctypes

import numpy as np
import pytest

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
        elif kind == 'softmax':
            dev = vb.SoftmaxRegressionModel(spec['X'], spec['y'], HO.SOFTMAX_CLASSES, HO.PARITY_PRIOR_SD)
        else:
            dev = vb.SourceModel(d, HO.QUARTIC_SRC, spec['a'])
        _MODELS[(kind, d)] = (dev, host)
    return _MODELS[(kind, d)]


def _device_normals(eng, seed, stream_offset, n_iter, n_chains, d):
    out = np.empty((n_iter, n_chains, d))
    for t in range(n_iter):
        eng.noise_generate(NOISE_SLOT, n_chains, d, seed, stream=stream_offset + t)
        out[t] = eng.noise_get_host(NOISE_SLOT, n_chains, d)
    return out


def _device_run(vb, dev, case, **override):
    kw = dict(n_chains=case['x0'].shape[0], n_warmup=HO.PARITY_WARMUP, n_draws=HO.PARITY_DRAWS,
              n_leapfrog=case['n_leapfrog'], step_size=case['step_size'], target_accept=0.8, jitter=case['jitter'],
              init=case['x0'], inv_mass=case['inv_mass'], seed=case['seed'], stream_offset=case['stream_offset'],
              thin=case['thin'])
    kw.update(override)
    return vb.hmc(dev, **kw)


def _tolerances(ref, pert):
    return {k: 10.0 * float(np.max(np.abs(pert[k] - ref[k]))) + 1e-12 * float(np.max(np.abs(ref[k]))) for k in OUTPUTS}


def _compare(got, ref, tol, label):
    """Largest error-to-tolerance ratio over the outputs; asserts the exact parts."""
    worst = 0.0
    for k in OUTPUTS:
        assert got[k].shape == ref[k].shape, (label, k, got[k].shape, ref[k].shape)
        err = float(np.max(np.abs(got[k] - ref[k])))
        print('%s %s: error %.3e, tolerance %.3e' % (label, k, err, tol[k]))
        assert err <= tol[k], (label, k, err, tol[k])
        if tol[k] > 0.0:           # (a tolerance of zero -- an output that is all zeros -- was met exactly)
            worst = max(worst, err / tol[k])
    return worst


# ---- 1. trajectory parity -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_chains', HO.PARITY_CHAINS)
@pytest.mark.parametrize('kind', HO.PARITY_MODELS)
def test_trajectory_parity(vb, kind, n_chains, capsys):
    from viabel_amd import _lib
    eng = _lib.default_engine()
    worst = 0.0
    n_iter = HO.PARITY_WARMUP + HO.PARITY_DRAWS
    for case in HO.parity_cases(kind, n_chains):
        dev, host = _model(vb, kind, case['d'])
        z = _device_normals(eng, case['seed'], case['stream_offset'], n_iter, n_chains, case['d'])
        ref = HO.run_case(host, case, z)
        pert = HO.run_case(host, case, z, perturb=np.random.RandomState(case['seed']))
        assert ref['min_margin'] >= HO.MIN_MARGIN, (case['key'], ref['min_margin'])
        got = _device_run(vb, dev, case)
        label = '%s C=%d D=%d L=%d thin=%d jitter=%g' % (kind, n_chains, case['d'], case['n_leapfrog'], case['thin'],
                                                        case['jitter'])
        # the decisions, exactly: a kept draw row changes exactly where a proposal was accepted
        assert got['n_divergent'] == ref['n_divergent'], label
        assert np.array_equal(got['accept_rate'], ref['accept_rate']), label
        if case['thin'] == 1:      # a chain's kept row changes exactly where its proposal was accepted
            moved = np.any(np.diff(got['draws'], axis=0) != 0.0, axis=2)
            assert np.array_equal(moved, ref['accepted'][HO.PARITY_WARMUP + 1:]), label
        assert got['step_size'] == pytest.approx(ref['step_size'], rel=1e-9), label
        assert got['next_stream'] == ref['next_stream']
        worst = max(worst, _compare(got, ref, _tolerances(ref, pert), label))
    capsys.readouterr()
    with capsys.disabled():
        print('\n%s, %d chains: largest error / tolerance = %.2e' % (kind, n_chains, worst))


# ---- 2. reproducibility; independence of the chain count ------------------------------------------------------------------
@pytest.mark.parametrize('kind', HO.PARITY_MODELS)
def test_bit_reproducible(vb, kind):
    for n_chains in (HO.PARITY_CHAINS[0], HO.PARITY_CHAINS[-1]):
        cases = HO.parity_cases(kind, n_chains)
        for case in (cases[0], cases[-1]):
            dev, _ = _model(vb, kind, case['d'])
            one, two = _device_run(vb, dev, case), _device_run(vb, dev, case)
            for k in OUTPUTS + ('accept_rate', 'mean', 'sd', 'rhat'):
                assert np.array_equal(one[k], two[k], equal_nan=True), (kind, n_chains, k)
            assert one['step_size'] == two['step_size'] and one['n_divergent'] == two['n_divergent']


@pytest.mark.parametrize('kind', HO.PARITY_MODELS)
def test_chains_do_not_depend_on_the_chain_count(vb, kind):
    from viabel_amd import _lib
    eng = _lib.default_engine()
    big = HO.parity_cases(kind, 257)[-1]
    d = big['d']
    dev, host = _model(vb, kind, d)
    small = dict(big, x0=big['x0'][:9].copy())
    a = _device_run(vb, dev, big, n_warmup=0)
    b = _device_run(vb, dev, small, n_chains=9, n_warmup=0)
    z = _device_normals(eng, big['seed'], big['stream_offset'], HO.PARITY_DRAWS, 9, d)
    ref = HO.run_case(host, small, z, n_warmup=0)
    pert = HO.run_case(host, small, z, n_warmup=0, perturb=np.random.RandomState(1))
    assert ref['min_margin'] >= HO.MIN_MARGIN
    tol = _tolerances(ref, pert)
    for k in ('draws', 'last', 'chain_mean', 'chain_var'):
        assert np.max(np.abs(a[k][..., :9, :] - b[k])) <= tol[k], k
    assert np.max(np.abs(a['logp'][:, :9] - b['logp'])) <= tol['logp']
    assert np.array_equal(a['accept_rate'][:9], b['accept_rate'])
    assert np.array_equal(a['step_size_history'], b['step_size_history'])        # no adaptation: the jitter alone


# ---- 3. continuation ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['funnel', 'logistic'])
def test_continuation(vb, kind):
    case = HO.parity_cases(kind, 9)[-1]
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


# ---- 4. statistics against closed forms ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['a', 'b'])
def test_statistics_against_closed_forms(vb, name):
    host, exact_mean, exact_cov, inv_mass, start, spec = HO.stat_config(name)
    if name == 'a':
        dev = vb.GaussianModel(spec['mean'], spec['sd'])
    else:
        dev = vb.LinearRegressionModel(spec['X'], spec['y'], spec['prior_sd'], spec['noise_sd'])
    res = vb.hmc(dev, n_chains=HO.STAT_CHAINS, n_warmup=HO.STAT_WARMUP, n_draws=HO.STAT_DRAWS, n_leapfrog=HO.STAT_LEAPFROG,
                 init=start, inv_mass=inv_mass, seed=HO.STAT_SEED)
    figures = HO.stat_conditions(name, res, exact_mean, exact_cov)
    for label, (value, bound, ok) in figures.items():
        print('(%s) %s: %s (bound %s)' % (name, label, value, bound))
    assert all(ok for _, _, ok in figures.values()), figures


# ---- 5. end to end ------------------------------------------------------------------------------------------------------------
def test_end_to_end_from_laplace_and_bbvi(vb, capsys):
    rng = np.random.RandomState(8)
    d, n = 10, 300
    X = rng.randn(n, d) / np.sqrt(d)
    y = (rng.rand(n) < 1.0 / (1.0 + np.exp(-X @ rng.randn(d)))).astype(np.float64)
    model = vb.LogisticRegressionModel(X, y, 3.0)
    lap = vb.laplace_approximation(model)
    post_sd = np.sqrt(np.diag(lap['cov']))
    capsys.readouterr()
    res = vb.hmc(model, n_chains=64, n_warmup=100, n_draws=100, n_leapfrog=8, var_param=lap['var_param'],
                 approx=lap['approx'])
    out = capsys.readouterr().out
    assert 'hmc: step size' in out and 'max rhat' in out and 'divergent' in out
    assert np.max(res['rhat']) <= 1.05
    assert np.all(np.abs(res['mean'] - lap['mode']) <= 0.5 * post_sd)
    np.testing.assert_allclose(res['inv_mass'], np.diag(lap['cov']), rtol=1e-10)
    assert res['draws'].shape == (100, 64, d) and res['logp'].shape == (100, 64) and res['n_divergent'] == 0
    # the same from bbvi's full-rank fit
    approx = vb.FullRankGaussian(d, seed=2, rng='philox')
    fit = vb.bbvi(d, log_density=model, approx=approx, num_mc_samples=64, n_iters=1500, adaptive=False, fixed_lr=True,
                  learning_rate=0.02)
    capsys.readouterr()
    res2 = vb.hmc(model, n_chains=64, n_warmup=100, n_draws=100, n_leapfrog=8, var_param=fit['opt_param'], approx=approx,
                  keep_draws=False)
    assert 'hmc: step size' in capsys.readouterr().out
    assert res2['draws'] is None and res2['logp'].shape == (100, 64)
    assert np.max(res2['rhat']) <= 1.05
    assert np.all(np.abs(res2['mean'] - lap['mode']) <= 0.5 * post_sd)


# ---- 6. divergences -----------------------------------------------------------------------------------------------------------
def test_divergences_are_counted_and_rejected(vb, capsys):
    d, c, n_draws = 3, 9, 5
    model = vb.GaussianModel(np.zeros(d), 1e-3 * np.ones(d))
    init = 1e-3 * np.random.RandomState(0).randn(c, d)
    res = vb.hmc(model, n_chains=c, n_warmup=0, n_draws=n_draws, n_leapfrog=48, step_size=10.0, jitter=0.0, init=init)
    assert 'WARNING' in capsys.readouterr().out
    assert res['n_divergent'] == n_draws * c
    assert np.array_equal(res['accept_rate'], np.zeros(c)) and np.array_equal(res['accept_prob'], np.zeros(n_draws))
    for t in range(n_draws):
        assert np.array_equal(res['draws'][t], init)
    assert np.array_equal(res['last'], init) and np.array_equal(res['chain_mean'], init)
    np.testing.assert_allclose(res['logp'][0], model(init), rtol=1e-13)
    assert all(np.array_equal(res['logp'][t], res['logp'][0]) for t in range(n_draws))
    for k in OUTPUTS + ('accept_rate', 'mean', 'sd'):
        assert np.all(np.isfinite(res[k])), k
    # (chains that never move have no within-chain variance: rhat = sqrt(var+ / 0) is +inf, which is what it should say)
    assert np.all(res['chain_var'] == 0.0) and np.all(np.isposinf(res['rhat']))
    assert res['step_size'] == 10.0


# ---- 7. a shared engine -------------------------------------------------------------------------------------------------------
def test_shared_engine(vb):
    d = 6
    rng = np.random.RandomState(4)
    target = vb.FunnelModel(d)
    theta = np.concatenate([0.1 * rng.randn(d), -1.0 + 0.1 * rng.randn(d)])
    before = vb.ExclusiveKL(vb.MFGaussian(d, seed=3, rng='philox'), target, 64)(theta)
    X = rng.randn(40, d)
    reg = vb.LogisticRegressionModel(X, (rng.rand(40) < 0.5).astype(np.float64), 3.0)
    vb.hmc(reg, n_chains=5, n_warmup=2, n_draws=3, n_leapfrog=2, init=0.1 * rng.randn(5, d))
    after = vb.ExclusiveKL(vb.MFGaussian(d, seed=3, rng='philox'), target, 64)(theta)
    assert before[0] == after[0] and np.array_equal(before[1], after[1])
    out = vb.predict(np.concatenate([np.zeros(d), -np.ones(d)]), model=reg, approx=vb.MFGaussian(d, seed=1, rng='philox'),
                     n_samples=200)
    assert out['mean'].shape == (40,) and np.all(np.isfinite(out['mean']))


# ---- 8. errors at the C entry -------------------------------------------------------------------------------------------------
def _raw_rc(eng, x, m, n_draws=2):
    """Return code of a plain, well-formed vb_hmc_run call through ctypes (no warm-up, two leapfrog steps, step 0.5)."""
    c, d = x.shape
    out = [np.empty(s) for s in ((n_draws, c, d), (n_draws, c), (c, d), (c, d), (c, d), c, n_draws, n_draws, 1)]
    ndiv = ctypes.c_int64(0)
    return eng._lib.vb_hmc_run(eng._ctx, x.ctypes.data, m.ctypes.data, c, d, 0, n_draws, 1, 2, 0.5, 0.8, 0.2, 1, 0,
                               *[a.ctypes.data for a in out], ctypes.byref(ndiv))


def test_errors(vb):
    from viabel_amd import _lib
    x0, im = np.zeros((4, 3)), np.ones(3)
    ok = dict(n_warmup=1, n_draws=2, n_leapfrog=2, step_size=0.5)
    fresh = _lib.Engine()
    try:
        with pytest.raises(_lib.EngineError):                               # no model bound
            fresh.hmc_run(x0, im, **ok)
        assert _raw_rc(fresh, x0, im) == _lib.VB_ERR_STATE
        fresh.set_model(vb.GaussianModel(np.zeros(3), np.ones(3)).device_spec())
        fresh.comm_init_host(lambda arr, op: None, 1, 0)
        with pytest.raises(NotImplementedError) as info:                    # an attached communicator
            fresh.hmc_run(x0, im, **ok)
        assert 'communicator' in str(info.value)
        assert _raw_rc(fresh, x0, im) == _lib.VB_ERR_UNSUPPORTED
        fresh.comm_destroy()
        assert fresh.hmc_run(x0, im, **ok)['last'].shape == (4, 3)
        assert _raw_rc(fresh, x0, im) == _lib.VB_OK
        callback = vb.CallableModel(3, lambda x: -0.5 * np.sum(x * x, axis=1), lambda x: -x)
        fresh.set_model(callback.device_spec())
        with pytest.raises(NotImplementedError) as info:                    # a host-callback model
            fresh.hmc_run(x0, im, **ok)
        assert 'callback' in str(info.value)
        assert _raw_rc(fresh, x0, im) == _lib.VB_ERR_UNSUPPORTED
        assert np.allclose(fresh.model_logp(x0), 0.0)
    finally:
        fresh.close()
    model = vb.GaussianModel(np.zeros(3), np.ones(3))
    eng = _lib.default_engine()
    eng.set_model(model.device_spec())
    still_works = lambda: np.testing.assert_allclose(eng.model_grad(np.ones((2, 3)))[1], -np.ones((2, 3)))   # noqa: E731
    bad = [dict(n_draws=0), dict(n_warmup=-1), dict(thin=0), dict(n_leapfrog=0), dict(step_size=0.0), dict(step_size=-1.0),
           dict(step_size=np.inf), dict(step_size=np.nan), dict(target_accept=0.0), dict(target_accept=1.0),
           dict(jitter=-0.1), dict(jitter=1.0)]
    for kw in bad:
        args = dict(ok)
        args.update(kw)
        with pytest.raises(ValueError):
            eng.hmc_run(x0, im, **args)
        still_works()
    for bad_im in (np.array([1.0, 0.0, 1.0]), np.array([1.0, -2.0, 1.0]), np.array([1.0, np.inf, 1.0]),
                   np.array([np.nan, 1.0, 1.0])):
        with pytest.raises(ValueError):
            eng.hmc_run(x0, bad_im, **ok)
        still_works()
    with pytest.raises(ValueError):                                         # d different from the model's dimension
        eng.hmc_run(np.zeros((4, 2)), np.ones(2), **ok)
    with pytest.raises(ValueError):                                         # the wrapper's own shape check
        eng.hmc_run(x0, np.ones(2), **ok)
    still_works()
    # the draw budget: 2048 kept iterations x 4096 chains x 17 doubles are above it -- refused before anything is allocated
    big = vb.GaussianModel(np.zeros(17), np.ones(17))
    eng.set_model(big.device_spec())
    with pytest.raises(NotImplementedError) as info:
        eng.hmc_run(np.zeros((4096, 17)), np.ones(17), 0, 2048, 1, 0.5)
    assert 'thin' in str(info.value) and 'budget' in str(info.value)
    assert _raw_rc(eng, np.zeros((4096, 17)), np.ones(17), n_draws=2048) == _lib.VB_ERR_UNSUPPORTED
    small = eng.hmc_run(np.zeros((4096, 17)), np.ones(17), 0, 4, 1, 0.5, keep_draws=False)
    assert small['draws'] is None and small['last'].shape == (4096, 17)
    eng.set_model(model.device_spec())
    still_works()
    # the C entry's own checks, through raw ctypes
    lib, ctx = eng._lib, eng._ctx
    p = lambda a: a.ctypes.data                                                                               # noqa: E731
    o = {k: np.zeros(s) for k, s in (('draws', (2, 4, 3)), ('logp', (2, 4)), ('last', (4, 3)), ('mean', (4, 3)),
                                     ('m2', (4, 3)), ('rate', 4), ('sh', 3), ('ah', 3), ('final', 1))}
    ndiv = ctypes.c_int64(-1)

    def call(ctx_=ctx, x=x0, m=im, c=4, d=3, nw=0, nd=2, thin=1, L=2, step=0.5, target=0.8, jitter=0.2, last=o['last'],
             final=o['final'], div=ctypes.byref(ndiv)):
        return lib.vb_hmc_run(ctx_, None if x is None else p(x), None if m is None else p(m), c, d, nw, nd, thin, L, step,
                              target, jitter, 1, 0, p(o['draws']), p(o['logp']), None if last is None else p(last),
                              p(o['mean']), p(o['m2']), p(o['rate']), p(o['sh']), p(o['ah']),
                              None if final is None else p(final), div)

    invalid = _lib.VB_ERR_INVALID
    assert call(ctx_=None) == invalid
    for kw in (dict(x=None), dict(m=None), dict(last=None), dict(final=None), dict(div=None), dict(c=0), dict(d=0),
               dict(nd=0), dict(nw=-1), dict(thin=0), dict(L=0), dict(step=0.0), dict(step=float('inf')),
               dict(target=0.0), dict(target=1.0), dict(jitter=-0.5), dict(jitter=1.0), dict(d=2),
               dict(m=np.array([1.0, 0.0, 1.0]))):
        assert call(**kw) == invalid, kw
        still_works()
    assert call() == _lib.VB_OK and ndiv.value == 0       # (no warm-up: the step stays at 0.5, stable on a unit Gaussian)
    assert np.all(np.isfinite(o['draws'])) and np.all(o['sh'][:2] > 0) and o['final'][0] == 0.5
