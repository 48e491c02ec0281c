"""GPU: hmc(trajectory='chees') -- the trajectory length adapted across the chains (vb_hmc_run_chees, csrc/vb_hmc.hip, through
Engine.hmc_run_chees and hmc()) -- against the numpy oracle of tests/_hmc_chees_oracle.py, which is handed the normals the
device draws and computes the uniforms and the radical inverse itself.  The scheme is test_gpu_hmc.py's: step counts and
accept decisions must match exactly, the real-valued outputs (the trajectory history among them) within ten times the
change the oracle's perturbation hook produces in that output plus 1e-12 max|ref|.  tests/test_hmc_chees_cpu.py vets every
case: no accept test within 1e-6, no step count within 1e-6 of its boundary, no yardstick above 1e-6 of the history."""
import numpy as np
import pytest

import _hmc_chees_oracle as CO
import _hmc_metric_oracle as MO
import _hmc_oracle as HO

pytestmark = pytest.mark.gpu

NOISE_SLOT = 5
OUTPUTS = CO.OUTPUTS


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


def _device_run(vb, dev, case, **override):
    kw = dict(n_chains=case['x0'].shape[0], n_warmup=CO.PARITY_WARMUP, n_draws=CO.PARITY_DRAWS, trajectory='chees',
              max_leapfrog=CO.PARITY_MAX_LEAPFROG, trajectory_length=case['trajectory_length'], step_size=case['step_size'],
              target_accept=0.8, jitter=case['jitter'], init=case['x0'], seed=case['seed'],
              stream_offset=case['stream_offset'], thin=case['thin'])
    kw.update(dict(metric='dense', inv_mass=case['sigma']) if case['dense'] else dict(inv_mass=case['inv_mass']))
    kw.update(override)
    return vb.hmc(dev, **kw)


def _tolerances(ref, pert, keys=OUTPUTS):
    """test_gpu_hmc.py's rule -- ten times the perturbed oracle's difference plus 1e-12 max|ref| -- over ``keys``."""
    return {k: 10.0 * float(np.max(np.abs(np.asarray(pert[k]) - np.asarray(ref[k])))) +
            1e-12 * float(np.max(np.abs(ref[k]))) for k in keys}


def _compare(got, ref, tol, label):
    """Largest error-to-tolerance ratio over the outputs in ``tol``."""
    worst = 0.0
    for k in tol:
        assert np.shape(got[k]) == np.shape(ref[k]), (label, k, np.shape(got[k]), np.shape(ref[k]))
        err = float(np.max(np.abs(np.asarray(got[k]) - np.asarray(ref[k]))))
        print('%s %s: error %.3e, tolerance %.3e' % (label, k, err, tol[k]))
        assert err <= tol[k], (label, k, err, tol[k])
        if tol[k] > 0.0:
            worst = max(worst, err / tol[k])
    return worst


def _decisions_match(got, ref, n_warmup, label, step_rel=1e-9):
    assert got['n_leapfrog_history'].dtype == np.int64
    assert np.array_equal(got['n_leapfrog_history'], ref['n_leapfrog_history']), (label, got['n_leapfrog_history'],
                                                                                 ref['n_leapfrog_history'])
    assert got['n_divergent'] == ref['n_divergent'], label
    assert np.array_equal(got['accept_rate'], ref['accept_rate']), label
    moved = np.any(np.diff(got['draws'], axis=0) != 0.0, axis=2)      # (thin = 1) a kept row changes where a proposal was accepted
    assert np.array_equal(moved, ref['accepted'][n_warmup + 1:]), label
    assert got['step_size'] == pytest.approx(ref['step_size'], rel=step_rel), label
    assert got['next_stream'] == ref['next_stream']


# ---- 1. parity with the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_chains', CO.PARITY_CHAINS)
@pytest.mark.parametrize('kind', CO.PARITY_MODELS)
def test_chees_parity(vb, kind, n_chains, capsys):
    worst = 0.0
    n_iter = CO.PARITY_WARMUP + CO.PARITY_DRAWS
    for case in CO.parity_cases(kind, n_chains):
        dev, host = _model(vb, kind, case['d'])
        z = _device_normals(case['seed'], case['stream_offset'], n_iter, n_chains, case['d'])
        ref = CO.run_case(host, case, z)
        pert = CO.run_case(host, case, z, perturb=np.random.RandomState(case['seed']))
        assert ref['min_margin'] >= HO.MIN_MARGIN, (case['key'], ref['min_margin'])
        assert ref['min_step_margin'] >= CO.MIN_STEP_MARGIN, (case['key'], ref['min_step_margin'])
        assert CO.history_spread(ref, pert) <= CO.MAX_HISTORY_SPREAD, case['key']
        got = _device_run(vb, dev, case)
        label = '%s C=%d D=%d %s jitter=%g' % (kind, n_chains, case['d'], 'dense' if case['dense'] else 'diag', case['jitter'])
        assert got['metric'] == ('dense' if case['dense'] else 'diag') and got['adapt_windows'] == []
        _decisions_match(got, ref, CO.PARITY_WARMUP, label)
        assert got['trajectory_history'].shape == (n_iter,)
        assert got['trajectory_length'] == got['trajectory_history'][CO.PARITY_WARMUP] == got['trajectory_history'][-1]
        assert got['n_grad_evals'] == int(ref['n_leapfrog_history'].sum()) + 1
        worst = max(worst, _compare(got, ref, _tolerances(ref, pert), label))
    capsys.readouterr()
    with capsys.disabled():
        print('\n%s, %d chains: largest error / tolerance = %.2e' % (kind, n_chains, worst))


# ---- 2. unusable chains -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dense', [False, True])
def test_unusable_chains_are_left_out(vb, dense):
    """Two chains whose proposals have a non-finite log density and two divergent ones with a finite one, in every
    iteration (tests/test_hmc_chees_cpu.py checks the oracle for that): the others adapt the length as the oracle says."""
    case = CO.unusable_case(dense)
    host = HO.parity_problem('funnel', case['d'])[0]
    dev = vb.FunnelModel(case['d'])
    n_iter = CO.PARITY_WARMUP + CO.PARITY_DRAWS
    z = _device_normals(case['seed'], case['stream_offset'], n_iter, CO.UNUSABLE_CHAINS, case['d'])
    ref = CO.run_case(host, case, z)
    pert = CO.run_case(host, case, z, perturb=np.random.RandomState(case['seed']), perturb_groups=case['groups'])
    w = CO.PARITY_WARMUP
    assert (~ref['usable'][:w]).sum() == 2 * w and (ref['divergent'][:w] & ref['usable'][:w]).sum() >= 2 * w
    assert ref['min_margin'] >= HO.MIN_MARGIN and ref['min_step_margin'] >= CO.MIN_STEP_MARGIN
    assert CO.history_spread(ref, pert) <= CO.MAX_HISTORY_SPREAD
    got = _device_run(vb, dev, case)
    label = 'unusable %s' % ('dense' if dense else 'diag')
    _decisions_match(got, ref, w, label)
    assert np.all(np.isfinite(got['trajectory_history']))
    wild = list(CO.UNUSABLE_OVERFLOW + CO.UNUSABLE_DIVERGENT)
    assert np.array_equal(got['last'][wild], case['x0'][wild])                      # never accepted
    # (the kept log densities of the chains that start at v = -300 are of the order 1e260: compared relatively)
    calm = [c for c in range(CO.UNUSABLE_CHAINS) if c not in CO.UNUSABLE_OVERFLOW]
    tol = _tolerances(ref, pert, tuple(k for k in OUTPUTS if k != 'logp'))
    _compare(got, ref, tol, label)
    sub = lambda r: {'logp': r['logp'][:, calm]}                                                              # noqa: E731
    _compare(sub(got), sub(ref), _tolerances(sub(ref), sub(pert), ('logp',)), label)
    over = list(CO.UNUSABLE_OVERFLOW)
    np.testing.assert_allclose(got['logp'][:, over], ref['logp'][:, over], rtol=1e-12)


def test_all_chains_rejected_leaves_the_length(vb):
    dev = vb.GaussianModel(np.zeros(CO.REJECT_DIM), 1e-3 * np.ones(CO.REJECT_DIM))
    init = 1e-3 * np.random.RandomState(0).randn(CO.REJECT_CHAINS, CO.REJECT_DIM)
    res = vb.hmc(dev, n_chains=CO.REJECT_CHAINS, n_warmup=CO.REJECT_WARMUP, n_draws=2, trajectory='chees',
                 max_leapfrog=CO.PARITY_MAX_LEAPFROG, trajectory_length=CO.REJECT_LENGTH, step_size=CO.REJECT_STEP, jitter=0.0,
                 init=init, seed=1)
    assert res['n_divergent'] == 2 * CO.REJECT_CHAINS and np.all(res['accept_prob'] == 0.0)
    assert np.array_equal(res['last'], init)
    # every iteration's sum of acceptance probabilities is zero: (log T, v) stay, and the clamp's interval holds T
    # (to a few ulps of log T = 3.2: the running average of equal numbers rounds)
    hist = res['trajectory_history']
    np.testing.assert_allclose(hist, CO.REJECT_LENGTH, rtol=1e-14)
    assert res['trajectory_length'] == hist[-1]
    ref_steps = [CO.n_steps(CO.halton(t) * hist[t], res['step_size_history'][t], CO.PARITY_MAX_LEAPFROG)[0] for t in range(4)]
    assert list(res['n_leapfrog_history']) == ref_steps


# ---- 3. the clamp: max_leapfrog steps in every iteration is the fixed route ----------------------------------------------------
@pytest.mark.parametrize('dense', [False, True])
@pytest.mark.parametrize('kind,n_chains', [('funnel', 5), ('logistic', 257)])
def test_clamped_chees_equals_fixed(vb, kind, n_chains, dense):
    case = CO.parity_cases(kind, n_chains)[-1 if dense else -3]
    assert case['dense'] == dense and case['jitter'] == 0.2
    dev, _ = _model(vb, kind, case['d'])
    kw = dict(n_warmup=0, n_draws=6)
    chees = _device_run(vb, dev, case, max_leapfrog=3, trajectory_length=1e6, **kw)
    fixed = _device_run(vb, dev, case, trajectory='fixed', n_leapfrog=3, trajectory_length=None, **kw)
    assert np.all(chees['n_leapfrog_history'] == 3)
    for k in ('draws', 'logp', 'last', 'chain_mean', 'chain_var', 'mean', 'sd', 'rhat', 'accept_rate', 'accept_prob',
              'step_size_history', 'n_leapfrog_history'):
        assert np.array_equal(chees[k], fixed[k], equal_nan=True), (kind, n_chains, dense, k)
    assert chees['step_size'] == fixed['step_size'] and chees['n_divergent'] == fixed['n_divergent']
    assert chees['n_grad_evals'] == fixed['n_grad_evals'] == 19 and chees['next_stream'] == fixed['next_stream']


# ---- 4. reproducibility and continuation --------------------------------------------------------------------------------------
def test_bit_reproducible(vb):
    for kind, n_chains in (('funnel', 5), ('logistic', 257)):
        for case in (CO.parity_cases(kind, n_chains)[i] for i in (1, -1)):
            dev, _ = _model(vb, kind, case['d'])
            one, two = _device_run(vb, dev, case), _device_run(vb, dev, case)
            for k in OUTPUTS + ('accept_rate', 'mean', 'sd', 'rhat', 'n_leapfrog_history'):
                assert np.array_equal(one[k], two[k], equal_nan=True), (kind, n_chains, k)
            assert one['step_size'] == two['step_size'] and one['n_divergent'] == two['n_divergent']


@pytest.mark.parametrize('dense', [False, True])
def test_continuation(vb, dense):
    case = CO.parity_cases('logistic', 5)[-1 if dense else -3]
    dev, _ = _model(vb, 'logistic', case['d'])
    whole = _device_run(vb, dev, case, n_warmup=0, n_draws=6)
    first = _device_run(vb, dev, case, n_warmup=0, n_draws=3)
    assert first['next_stream'] == case['stream_offset'] + 3
    second = _device_run(vb, dev, case, n_warmup=0, n_draws=3, init=first['last'], step_size=first['step_size'],
                         stream_offset=first['next_stream'], trajectory_length=first['trajectory_length'])
    assert np.array_equal(second['last'], whole['last'])
    for k in ('draws', 'logp', 'trajectory_history', 'n_leapfrog_history', 'step_size_history', 'accept_prob'):
        assert np.array_equal(np.concatenate([first[k], second[k]]), whole[k]), k
    assert second['next_stream'] == whole['next_stream'] and second['trajectory_length'] == whole['trajectory_length']
    # the radical inverse follows the stream: the step counts are those of streams offset .. offset + 5
    steps = [CO.n_steps(CO.halton(case['stream_offset'] + t) * whole['trajectory_history'][t], whole['step_size_history'][t],
                        CO.PARITY_MAX_LEAPFROG)[0] for t in range(6)]
    assert list(whole['n_leapfrog_history']) == steps and len(set(steps)) > 1


# ---- 5. with adapt_metric ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dense', [False, True])
@pytest.mark.parametrize('d', MO.ADAPT_DIMS)
@pytest.mark.parametrize('n_chains', MO.ADAPT_CHAINS)
def test_adaptive_parity(vb, n_chains, d, dense):
    from oracle import models as omod
    case = MO.adapt_case(n_chains, d, dense)
    n_iter = MO.ADAPT_WARMUP + MO.ADAPT_DRAWS
    z = _device_normals(case['seed'], case['stream_offset'], n_iter, n_chains, d)
    vg = HO.value_and_grad_of(omod.GaussDiag(case['mean'], case['sd']))
    length = CO.ADAPT_LENGTH_STEPS * case['step_size']
    kw = dict(dense=dense, inv_mass=np.eye(d) if dense else np.ones(d), n_warmup=MO.ADAPT_WARMUP, n_draws=MO.ADAPT_DRAWS,
              max_leapfrog=CO.ADAPT_MAX_LEAPFROG, step_size=case['step_size'], trajectory_length=length, jitter=case['jitter'],
              seed=case['seed'], stream_offset=case['stream_offset'])
    ref = CO.run_adaptive(vg, case['x0'], z, **kw)
    pert = CO.run_adaptive(vg, case['x0'], z, perturb=np.random.RandomState(case['seed']), **kw)
    assert ref['min_margin'] >= HO.MIN_MARGIN and ref['min_step_margin'] >= CO.MIN_STEP_MARGIN, case['key']
    assert CO.history_spread(ref, pert) <= CO.MAX_HISTORY_SPREAD, case['key']
    got = vb.hmc(vb.GaussianModel(case['mean'], case['sd']), n_chains=n_chains, n_warmup=MO.ADAPT_WARMUP,
                 n_draws=MO.ADAPT_DRAWS, trajectory='chees', max_leapfrog=CO.ADAPT_MAX_LEAPFROG, trajectory_length=length,
                 step_size=case['step_size'], jitter=case['jitter'], init=case['x0'], inv_mass=np.ones(d), seed=case['seed'],
                 stream_offset=case['stream_offset'], metric='dense' if dense else 'diag', adapt_metric=True)
    label = 'adaptive chees C=%d D=%d %s' % (n_chains, d, 'dense' if dense else 'diag')
    assert got['adapt_windows'] == [(6, 36)] == ref['adapt_windows']
    assert got['trajectory_history'].shape == (n_iter,) and got['n_leapfrog_history'].shape == (n_iter,)
    step_rel = 10.0 * abs(pert['step_size'] / ref['step_size'] - 1.0) + 1e-12
    _decisions_match(got, ref, MO.ADAPT_WARMUP, label, step_rel=step_rel)
    _compare(got, ref, _tolerances(ref, pert, OUTPUTS + ('inv_mass',)), label)
    assert got['n_grad_evals'] == int(ref['n_leapfrog_history'].sum()) + 3          # three engine calls
    # carried across the window ends, not reset: one Adam step (and the clamp) there, and far from T_0 by then
    steps = np.abs(np.diff(np.log(got['trajectory_history'][:MO.ADAPT_WARMUP])))
    assert np.max(steps[[5, 35]]) < 0.5 and abs(np.log(got['trajectory_history'][36] / length)) > 0.5


# ---- 6. the fixed route is untouched ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('route', ['diag', 'dense', 'adaptive'])
def test_fixed_is_untouched(vb, route):
    if route == 'adaptive':
        case = MO.adapt_case(5, 2, False)
        dev = vb.GaussianModel(case['mean'], case['sd'])
        kw = dict(n_chains=5, n_warmup=MO.ADAPT_WARMUP, n_draws=MO.ADAPT_DRAWS, n_leapfrog=case['n_leapfrog'],
                  step_size=case['step_size'], jitter=case['jitter'], init=case['x0'], inv_mass=np.ones(2), seed=case['seed'],
                  stream_offset=case['stream_offset'], adapt_metric=True)
        n_iter, n_calls = MO.ADAPT_WARMUP + MO.ADAPT_DRAWS, 3
    else:
        case = HO.parity_cases('logistic', 9)[-1]
        dev, _ = _model(vb, 'logistic', case['d'])
        kw = dict(n_chains=9, n_warmup=HO.PARITY_WARMUP, n_draws=HO.PARITY_DRAWS, n_leapfrog=case['n_leapfrog'],
                  step_size=case['step_size'], jitter=case['jitter'], init=case['x0'], inv_mass=case['inv_mass'],
                  seed=case['seed'], stream_offset=case['stream_offset'], thin=case['thin'], metric=route)
        n_iter, n_calls = HO.PARITY_WARMUP + HO.PARITY_DRAWS, 1
    plain, fixed = vb.hmc(dev, **kw), vb.hmc(dev, trajectory='fixed', max_leapfrog=7, trajectory_length=3.0, **kw)
    for k in ('draws', 'logp', 'last', 'chain_mean', 'chain_var', 'mean', 'sd', 'rhat', 'accept_rate', 'accept_prob',
              'step_size_history', 'inv_mass', 'trajectory_history', 'n_leapfrog_history'):
        assert np.array_equal(plain[k], fixed[k], equal_nan=True), (route, k)
    assert plain['step_size'] == fixed['step_size'] and plain['n_divergent'] == fixed['n_divergent']
    n_leapfrog = kw['n_leapfrog']
    assert plain['n_leapfrog_history'].dtype == np.int64 and np.array_equal(plain['n_leapfrog_history'],
                                                                            np.full(n_iter, n_leapfrog))
    assert plain['trajectory_length'] == n_leapfrog * plain['step_size']
    assert np.array_equal(plain['trajectory_history'], np.full(n_iter, plain['trajectory_length']))
    assert plain['n_grad_evals'] == n_iter * n_leapfrog + n_calls


# ---- 7. statistics against closed forms ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['a', 'b'])
def test_statistics_against_closed_forms(vb, name, capsys):
    host, exact_mean, exact_cov, inv_mass, start, spec = HO.stat_config(name)
    if name == 'a':
        dev = vb.GaussianModel(spec['mean'], spec['sd'])
    else:
        dev = vb.LinearRegressionModel(spec['X'], spec['y'], spec['prior_sd'], spec['noise_sd'])
    capsys.readouterr()
    res = vb.hmc(dev, n_chains=HO.STAT_CHAINS, n_warmup=HO.STAT_WARMUP, n_draws=HO.STAT_DRAWS, trajectory='chees',
                 max_leapfrog=CO.STAT_MAX_LEAPFROG, init=start, inv_mass=inv_mass, seed=HO.STAT_SEED)
    out = capsys.readouterr().out
    assert 'hmc: step size' in out and ', T = ' in out and 'mean L = ' in out
    figures = HO.stat_conditions(name, res, exact_mean, exact_cov)
    for label, (value, bound, ok) in figures.items():
        print('(%s) %s: %s (bound %s)' % (name, label, value, bound))
    print('(%s) T = %.3f, step %.3f' % (name, res['trajectory_length'], res['step_size']))
    assert all(ok for _, _, ok in figures.values()), figures
    # it started from one leapfrog step (trajectory_length = step_size) and has left it
    assert res['trajectory_history'][0] == pytest.approx(exact_mean.size ** -0.25, rel=1e-15)
    assert res['trajectory_length'] > 2.0 * res['step_size'] and res['n_leapfrog_history'][HO.STAT_WARMUP:].mean() > 2.0


# ---- 8. errors at the C entry -------------------------------------------------------------------------------------------------
def test_errors(vb):
    from viabel_amd import _lib
    eng = _lib.default_engine()
    model = vb.GaussianModel(np.zeros(3), np.ones(3))
    eng.set_model(model.device_spec())
    x0, im = np.zeros((4, 3)), np.ones(3)
    state = CO.initial_state(0.5)
    still_works = lambda: np.testing.assert_allclose(eng.model_grad(np.ones((2, 3)))[1], -np.ones((2, 3)))   # noqa: E731
    ok = dict(n_warmup=2, n_draws=2, max_leapfrog=4, step_size=0.5, traj_state=state)
    out = eng.hmc_run_chees(x0, im, **ok)
    assert out['traj_state'][3] == 2.0 and out['n_leapfrog_history'].shape == (4,) and np.all(state == CO.initial_state(0.5))
    for kw in (dict(max_leapfrog=0), dict(trajectory_lr=-1.0), dict(trajectory_lr=np.nan), dict(traj_state=[np.nan, 0, 0, 0]),
               dict(traj_state=[0.0, np.inf, 0, 0]), dict(traj_state=[0.0, -1.0, 0, 0]), dict(traj_state=[0.0, 0, 0, -1.0]),
               dict(traj_state=[0.0, 0, 0]), dict(step_size=0.0), dict(n_warmup=0, n_draws=0), dict(n_draws=-1)):
        with pytest.raises(ValueError):
            eng.hmc_run_chees(x0, im, **dict(ok, **kw))
        still_works()
    with pytest.raises(ValueError):                                   # one chain and a warm-up
        eng.hmc_run_chees(x0[:1], im, **ok)
    assert eng.hmc_run_chees(x0[:1], im, **dict(ok, n_warmup=0))['last'].shape == (1, 3)
    # a warm-up-only segment: the sampling outputs are None, the histories and the state are there
    seg = eng.hmc_run_chees(x0, np.eye(3), 3, 0, 4, 0.5, state)
    assert seg['draws'] is None and seg['chain_mean'] is None and seg['trajectory_history'].shape == (3,)
    assert seg['traj_state'][3] == 3.0 and np.all(seg['n_leapfrog_history'] >= 1)
    # the raw entry: NULL pointers of its own arguments
    lib, ctx = eng._lib, eng._ctx
    p = lambda a: a.ctypes.data                                                                               # noqa: E731
    o = {k: np.zeros(s) for k, s in (('last', (4, 3)), ('sh', 3), ('ah', 3), ('final', 1), ('th', 3))}
    lh = np.zeros(3, dtype=np.int64)
    st = CO.initial_state(0.5)

    def call(state=p(st), th=p(o['th']), leap=lh.ctypes.data_as(_lib._c_int64_p), max_leapfrog=4, c=4):
        return lib.vb_hmc_run_chees(ctx, p(x0), _lib.HMC_METRIC_DIAG, p(im), c, 3, 3, 0, 1, max_leapfrog, 0.025, 0.5, 0.8, 0.2,
                                    1, 0, None, None, None, None, None, p(o['last']), None, None, None, p(o['sh']),
                                    p(o['ah']), p(o['final']), None, state, th, leap)

    assert call() == _lib.VB_OK and st[3] == 3.0 and np.all(lh >= 1) and np.all(o['th'] > 0.0)
    for kw in (dict(state=None), dict(th=None), dict(leap=None), dict(max_leapfrog=0), dict(c=1)):
        assert call(**kw) == _lib.VB_ERR_INVALID, kw
        still_works()
