"""GPU: adaptive tempered SMC with HMC moves on the device (vb_smc_reweight, vb_smc_run, csrc/vb_smc.hip, through
Engine.smc_reweight, Engine.smc_run and smc()) against the numpy oracle of tests/_smc_oracle.py, which is handed the normals
the device draws (noise_generate / noise_get_host per stream) and computes the uniforms itself.  Stage counts, ancestors,
accept and divergence counts must match exactly (tests/test_smc_cpu.py vets every case's margins); the real-valued outputs
within a tolerance formed per case and per output from the oracle's perturbation hook: ten times the largest change that
noise of the size the project's model tests allow (1e-12 max|f| on values, 1e-11 max|g| on gradients) produces in that
output, plus 1e-12 max|ref|, and for the temperatures another 2^-39 (a near-tie bisection decision may flip)."""
import ctypes

import numpy as np
import pytest

import _hmc_oracle as HO
import _smc_oracle as SO

pytestmark = pytest.mark.gpu

NOISE_SLOT = 5


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


def _device_normals(eng, seed, n, d):
    """``stream -> (n, D)``: the normals the device draws for that stream, read back once and kept."""
    cache = {}

    def fn(stream):
        if stream not in cache:
            eng.noise_generate(NOISE_SLOT, n, d, seed, stream=stream)
            cache[stream] = eng.noise_get_host(NOISE_SLOT, n, d).copy()
        return cache[stream]
    return fn


def _device_run(vb, dev, case, **override):
    kw = dict(n_particles=case['n'], loc=case['loc'], scale=case['scale'], ess_target=SO.PARITY_ESS, n_moves=case['n_moves'],
              n_leapfrog=case['n_leapfrog'], step_size=case['step_size'], target_accept=0.8, adapt_rate=0.5,
              max_stages=SO.PARITY_MAX_STAGES, seed=case['seed'], stream_offset=case['stream_offset'], keep_ancestors=True)
    kw.update(override)
    return vb.smc(dev, **kw)


# ---- 1. vb_smc_reweight against the oracle --------------------------------------------------------------------------------------
def _perturbed_u(u, rng):
    finite = np.isfinite(u)
    return u + np.where(finite, HO.F_NOISE * np.max(np.abs(u[finite])) * rng.uniform(-1.0, 1.0, u.shape), 0.0)


@pytest.mark.parametrize('n', SO.REWEIGHT_SIZES)
@pytest.mark.parametrize('kind', SO.REWEIGHT_KINDS)
def test_reweight_against_the_oracle(vb, kind, n):
    from viabel_amd import _lib
    eng = _lib.default_engine()
    u, beta_prev, uniform = SO.reweight_input(kind, n)
    ref = SO.reweight(u, beta_prev, SO.REWEIGHT_ESS, uniform)
    pert = SO.reweight(_perturbed_u(u, np.random.RandomState(n)), beta_prev, SO.REWEIGHT_ESS, uniform)
    assert ref['ancestor_margin'] >= SO.MIN_ANCESTOR_MARGIN
    beta, inc, ess, anc = eng.smc_reweight(u, beta_prev, SO.REWEIGHT_ESS, uniform)
    assert anc.dtype == np.int64 and np.array_equal(anc, ref['ancestors']), (kind, n)
    if kind == 'neginf':
        assert not np.any(np.isin(anc, np.flatnonzero(u == -np.inf)))
    for label, got, want, other, slack in (('beta', beta, ref['beta'], ref['beta'], SO.BETA_SLACK + 1e-12),
                                           ('log_z_inc', inc, ref['log_z_inc'], pert['log_z_inc'], 0.0),
                                           ('ess', ess, ref['ess'], pert['ess'], 0.0)):
        tol = slack if label == 'beta' else 10.0 * abs(other - want) + 1e-12 * abs(want)
        print('%s n=%d %s: error %.3e, tolerance %.3e' % (kind, n, label, abs(got - want), tol))
        assert abs(got - want) <= tol, (kind, n, label, got, want, tol)
    if ref['last']:
        assert beta == 1.0


@pytest.mark.parametrize('n', SO.REWEIGHT_SIZES)
def test_reweight_exact_cases(vb, n):
    from viabel_amd import _lib
    eng = _lib.default_engine()
    # all u equal: every weight is 1, the sums are exact, the ancestors are the identity for U = 0.5
    beta, inc, ess, anc = eng.smc_reweight(np.full(n, -3.25), 0.25, 0.5, 0.5)
    assert beta == 1.0 and inc == 0.75 * -3.25 and ess == float(n)
    assert np.array_equal(anc, np.arange(n))
    # one finite u among -inf: its weight is 1, every other 0; E = 1 / n, so the target lies below that
    for index in sorted({0, n // 2, n - 1}):
        u = np.full(n, -np.inf)
        u[index] = 2.5
        beta, inc, ess, anc = eng.smc_reweight(u, 0.0, 0.5 / n, 0.3)
        assert beta == 1.0 and ess == 1.0 and np.array_equal(anc, np.full(n, index))
        assert inc == pytest.approx(2.5 - np.log(n), rel=1e-14, abs=1e-15)


def test_reweight_errors(vb):
    from viabel_amd import _lib
    eng = _lib.default_engine()
    lib, ctx = eng._lib, eng._ctx
    out, anc = np.zeros(3), np.zeros(10, dtype=np.int64)
    p = lambda a: a.ctypes.data                                                                               # noqa: E731
    ap = anc.ctypes.data_as(_lib._c_int64_p)

    def call(u, n=10, beta=0.0, target=0.5, uniform=0.5, ctx_=ctx, out_=out, anc_=ap):
        return lib.vb_smc_reweight(ctx_, None if u is None else p(u), n, beta, target, uniform,
                                   None if out_ is None else p(out_), anc_)

    good = np.linspace(-1.0, 1.0, 10)
    numeric = _lib.VB_ERR_NUMERIC
    for bad in (np.where(np.arange(10) == 4, np.nan, good), np.where(np.arange(10) == 4, np.inf, good),
                np.full(10, -np.inf), np.where(np.arange(10) == 3, 0.0, -np.inf)):      # the last: delta = 0
        bad = np.ascontiguousarray(bad)
        assert call(bad) == numeric
        with pytest.raises(ValueError):
            eng.smc_reweight(bad, 0.0, 0.5, 0.5)
        assert call(good) == _lib.VB_OK                                                  # the context stays usable
    invalid = _lib.VB_ERR_INVALID
    assert call(good, ctx_=None) == invalid
    for kw in (dict(u=None), dict(out_=None), dict(anc_=None), dict(n=0), dict(n=-1), dict(beta=-0.1), dict(beta=1.0),
               dict(target=0.0), dict(target=1.0), dict(uniform=-0.1), dict(uniform=1.0), dict(uniform=float('nan'))):
        args = dict(u=good)
        args.update(kw)
        assert call(**args) == invalid, kw
    assert call(good, n=65537) == _lib.VB_ERR_UNSUPPORTED
    assert call(good) == _lib.VB_OK and out[0] == 1.0


# ---- 2. run parity -----------------------------------------------------------------------------------------------------------------
EXACT = ('n_stages', 'n_divergent', 'next_stream')


@pytest.mark.parametrize('n', SO.PARITY_PARTICLES)
@pytest.mark.parametrize('kind', HO.PARITY_MODELS)
def test_run_parity(vb, kind, n, capsys):
    from viabel_amd import _lib
    eng = _lib.default_engine()
    worst = 0.0
    for case in SO.parity_cases(kind, n):
        dev, host = _model(vb, kind, case['d'])
        normals = _device_normals(eng, case['seed'], n, case['d'])
        ref = SO.run_case(host, case, normals)
        pert = SO.run_case(host, case, normals, perturb=np.random.RandomState(case['seed']))
        label = '%s n=%d D=%d moves=%d L=%d' % (kind, n, case['d'], case['n_moves'], case['n_leapfrog'])
        assert ref['min_accept_margin'] >= SO.MIN_ACCEPT_MARGIN, (label, ref['min_accept_margin'])
        assert ref['min_ancestor_margin'] >= SO.MIN_ANCESTOR_MARGIN, (label, ref['min_ancestor_margin'])
        assert ref['min_ess_margin'] >= SO.MIN_ESS_MARGIN, (label, ref['min_ess_margin'])
        assert pert['n_stages'] == ref['n_stages'], label
        got = _device_run(vb, dev, case)
        for k in EXACT:
            assert got[k] == ref[k], (label, k, got[k], ref[k])
        assert got['betas'][-1] == 1.0, label
        assert np.array_equal(got['ancestors'], ref['ancestors']), label
        assert np.array_equal(got['n_accepted'], ref['n_accepted']), label
        assert got['n_grad_evals'] == 1 + ref['n_stages'] * case['n_moves'] * case['n_leapfrog']
        tol = SO.tolerances(ref, pert)
        for k in SO.OUTPUTS:
            a, b = np.asarray(got[k], dtype=np.float64), np.asarray(ref[k], dtype=np.float64)
            assert a.shape == b.shape, (label, k, a.shape, b.shape)
            err = float(np.max(np.abs(a - b)))
            print('%s %s: error %.3e, tolerance %.3e' % (label, k, err, tol[k]))
            assert err <= tol[k], (label, k, err, tol[k])
            if tol[k] > 0.0:
                worst = max(worst, err / tol[k])
        assert got['step_size'] == pytest.approx(ref['step_size'], rel=1e-9), label
    capsys.readouterr()
    with capsys.disabled():
        print('\n%s, %d particles: largest error / tolerance = %.2e' % (kind, n, worst))


# ---- 3. bit reproducibility ----------------------------------------------------------------------------------------------------------
BITS = ('particles', 'logp', 'betas', 'log_z_increments', 'ess', 'accept_prob', 'n_accepted', 'step_size_history', 'ancestors',
        'mean', 'sd')


def _same_bits(one, two, label):
    for k in BITS:
        assert np.array_equal(one[k], two[k], equal_nan=True), (label, k)
    for k in ('log_evidence', 'step_size', 'n_stages', 'n_divergent', 'next_stream'):
        assert one[k] == two[k], (label, k)


@pytest.mark.parametrize('kind', HO.PARITY_MODELS)
def test_bit_reproducible(vb, kind):
    for n in (SO.PARITY_PARTICLES[1], SO.PARITY_PARTICLES[-1]):
        case = SO.parity_cases(kind, n)[-1]
        dev, _ = _model(vb, kind, case['d'])
        _same_bits(_device_run(vb, dev, case), _device_run(vb, dev, case), (kind, n))


def test_same_bits_after_hmc_and_svgd_as_on_a_fresh_engine(vb):
    from viabel_amd import _lib
    case = SO.parity_cases('logistic', 257)[-1]
    dev, _ = _model(vb, 'logistic', case['d'])
    rng = np.random.RandomState(3)
    other = vb.FunnelModel(5)
    vb.hmc(other, n_chains=300, n_warmup=2, n_draws=3, n_leapfrog=2, init=0.1 * rng.randn(300, 5))
    vb.svgd(other, n_particles=40, n_iters=3, init=0.1 * rng.randn(40, 5))
    used = _device_run(vb, dev, case)
    shared = _lib.default_engine()
    fresh = _lib.Engine()
    try:
        _lib.set_default_engine(fresh)
        clean = _device_run(vb, dev, case)
    finally:
        _lib.set_default_engine(shared)
        fresh.close()
    _same_bits(used, clean, 'after hmc and svgd / fresh')


# ---- 4. statistics against closed forms -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['a', 'b'])
def test_statistics_against_closed_forms(vb, name):
    host, mean, sd, log_z, loc, scale, spec = SO.stat_config(name)
    if name == 'a':
        dev = vb.GaussianModel(spec['mean'], spec['sd'])
    else:
        dev = vb.LinearRegressionModel(spec['X'], spec['y'], spec['prior_sd'], spec['noise_sd'])
    res = vb.smc(dev, n_particles=SO.STAT_PARTICLES, loc=loc, scale=scale, ess_target=SO.STAT_ESS, n_moves=SO.STAT_MOVES,
                 n_leapfrog=SO.STAT_LEAPFROG, seed=SO.STAT_TEST_SEED[name])
    fig, bounds = SO.stat_figures(res, mean, sd, log_z), SO.stat_bounds(name)
    for label, value, bound in zip(('log evidence error', 'mean error / sd', 'sd ratio error'), fig, bounds):
        print('(%s) %s: %.4g (bound %.4g)' % (name, label, value, bound))
    assert abs(fig[0]) <= bounds[0] and fig[1] <= bounds[1] and fig[2] <= bounds[2], (fig, bounds)
    assert res['betas'][-1] == 1.0


# ---- 5. end to end ------------------------------------------------------------------------------------------------------------------------
def test_end_to_end_from_a_mean_field_fit(vb, capsys):
    rng = np.random.RandomState(8)
    d, n = 10, 300
    X = rng.randn(n, d) / np.sqrt(d)
    y = (rng.rand(n) < 1.0 / (1.0 + np.exp(-X @ rng.randn(d)))).astype(np.float64)
    model = vb.LogisticRegressionModel(X, y, 3.0)
    approx = vb.MFGaussian(d, seed=2, rng='philox')
    fit = vb.bbvi(d, log_density=model, approx=approx, num_mc_samples=64, n_iters=1500, adaptive=False, fixed_lr=True,
                  learning_rate=0.02)
    var_param = fit['opt_param']
    capsys.readouterr()
    res = vb.smc(model, n_particles=512, var_param=var_param, approx=approx)
    out = capsys.readouterr().out
    assert out.startswith('smc: 512 particles') and 'log evidence' in out and 'divergent' in out
    fit_mean, fit_cov = approx.mean_and_cov(var_param)
    np.testing.assert_allclose(res['loc'], fit_mean, rtol=1e-14)
    np.testing.assert_allclose(res['scale'], np.sqrt(np.diag(fit_cov)), rtol=1e-14)
    # the fit's ELBO by plain Monte Carlo: a lower bound of the log evidence up to its own standard error
    draws = approx.sample(var_param, 4000, seed=11)
    terms = model(draws) - approx.log_density(var_param, draws)
    elbo, se = float(np.mean(terms)), float(np.std(terms, ddof=1) / np.sqrt(terms.size))
    print('log evidence %.4f, ELBO %.4f +- %.4f' % (res['log_evidence'], elbo, se))
    assert np.isfinite(res['log_evidence']) and res['log_evidence'] >= elbo - 4.0 * se
    assert res['particles'].shape == (512, d) and res['betas'][-1] == 1.0 and res['ancestors'] is None
    assert res['n_grad_evals'] == 1 + res['n_stages'] * 2 * 8 and res['next_stream'] == 1 + 2 * res['n_stages']
    score = vb.ksd(samples=res['particles'], model=model)
    assert np.isfinite(score['ksd']) and score['ksd'] >= 0.0


# ---- 6. refusals and errors -----------------------------------------------------------------------------------------------------------------
def test_refusals_and_errors(vb):
    from viabel_amd import _lib
    loc, scale = np.zeros(3), np.ones(3)
    ok = dict(n=8, n_moves=1, n_leapfrog=2, step_size=0.5, max_stages=20)
    fresh = _lib.Engine()
    try:
        with pytest.raises(_lib.EngineError):                               # no model bound
            fresh.smc_run(loc, scale, **ok)
        fresh.set_model(vb.GaussianModel(np.zeros(3), np.ones(3)).device_spec())
        fresh.comm_init_host(lambda arr, op: None, 1, 0)
        with pytest.raises(NotImplementedError) as info:                    # an attached communicator
            fresh.smc_run(loc, scale, **ok)
        assert 'communicator' in str(info.value)
        fresh.comm_destroy()
        assert fresh.smc_run(loc, scale, **ok)['particles'].shape == (8, 3)
        callback = vb.CallableModel(3, lambda x: -0.5 * np.sum(x * x, axis=1), lambda x: -x)
        fresh.set_model(callback.device_spec())
        with pytest.raises(NotImplementedError) as info:                    # a host-callback model
            fresh.smc_run(loc, scale, **ok)
        assert 'callback' in str(info.value)
        assert np.allclose(fresh.model_logp(np.zeros((4, 3))), 0.0)
    finally:
        fresh.close()
    model = vb.GaussianModel(np.array([3.0, -3.0, 3.0]), 0.5 * np.ones(3))
    eng = _lib.default_engine()
    eng.set_model(model.device_spec())
    still_works = lambda: np.testing.assert_allclose(eng.model_grad(np.array([[3.0, -3.0, 3.0]]))[1], np.zeros((1, 3)))  # noqa: E731
    # the C entry's own checks, through raw ctypes
    lib, ctx = eng._lib, eng._ctx
    p = lambda a: a.ctypes.data                                                                               # noqa: E731
    S, M, N = 20, 2, 8
    o = {k: np.zeros(s) for k, s in (('x', (N, 3)), ('logp', N), ('lq', N), ('ev', 1), ('bh', S), ('zh', S), ('eh', S),
                                     ('ah', (S, M)), ('sh', (S, M)), ('final', 1))}
    nacc = np.zeros((S, M), dtype=np.int64)
    n_stages, ndiv = ctypes.c_int64(-1), ctypes.c_int64(-1)

    def call(ctx_=ctx, loc_=loc, scale_=scale, n=N, d=3, target=0.5, moves=M, L=2, step=0.5, accept=0.8, rate=0.5, stages=S,
             x=o['x'], ev=o['ev'], ns=ctypes.byref(n_stages), final=o['final'], div=ctypes.byref(ndiv),
             na=nacc.ctypes.data_as(_lib._c_int64_p)):
        opt = lambda a: None if a is None else p(a)                                                           # noqa: E731
        return lib.vb_smc_run(ctx_, opt(loc_), opt(scale_), n, d, target, moves, L, step, accept, rate, stages, 1, 0, opt(x),
                              p(o['logp']), p(o['lq']), opt(ev), ns, p(o['bh']), p(o['zh']), p(o['eh']), p(o['ah']),
                              p(o['sh']), na, opt(final), div, None)

    invalid = _lib.VB_ERR_INVALID
    assert call(ctx_=None) == invalid
    for kw in (dict(loc_=None), dict(scale_=None), dict(x=None), dict(ev=None), dict(ns=None), dict(final=None), dict(div=None),
               dict(na=None), dict(n=0), dict(d=0), dict(moves=0), dict(L=0), dict(stages=0), dict(target=0.0),
               dict(target=1.0), dict(step=0.0), dict(step=float('inf')), dict(step=float('nan')), dict(accept=0.0),
               dict(accept=1.0), dict(rate=-0.5), dict(d=2), dict(scale_=np.array([1.0, 0.0, 1.0])),
               dict(scale_=np.array([1.0, np.inf, 1.0])), dict(scale_=np.array([1.0, -1.0, 1.0])),
               dict(loc_=np.array([0.0, np.nan, 0.0]))):
        assert call(**kw) == invalid, kw
        still_works()
    assert call(n=65537) == _lib.VB_ERR_UNSUPPORTED
    still_works()
    assert call() == _lib.VB_OK and n_stages.value > 1 and ndiv.value >= 0 and o['bh'][n_stages.value - 1] == 1.0
    # max_stages = 1 on a case that needs more
    assert call(stages=1) == _lib.VB_ERR_NUMERIC
    still_works()
    with pytest.raises(ValueError) as info:
        vb.smc(model, n_particles=8, loc=loc, scale=scale, max_stages=1)
    assert 'max_stages' in str(info.value)
    still_works()
    # Python's refusals
    with pytest.raises(NotImplementedError):
        vb.smc(vb.CallableModel(3, lambda x: -0.5 * np.sum(x * x, axis=1), lambda x: -x), n_particles=8, loc=loc, scale=scale)
    X = np.random.RandomState(0).randn(20, 3)
    with pytest.raises(NotImplementedError):
        vb.smc(vb.MinibatchRegressionModel(X, (X[:, 0] > 0).astype(float), 5), n_particles=8, loc=loc, scale=scale)
    with pytest.raises(NotImplementedError):
        vb.smc(model, n_particles=65537, loc=loc, scale=scale)
    still_works()
    assert vb.smc(model, n_particles=8, loc=loc, scale=scale)['betas'][-1] == 1.0
