"""vb_svgd_direction and vb_svgd_run (csrc/vb_svgd.hip) on the GPU against the extended-precision oracle of
tests/_svgd_oracle.py.

Tolerances (derived, not tuned; _svgd_oracle.tolerance, .bandwidth_tolerance):  |phi - ref| <= tol E per coordinate with
tol = 2 (2 D + n + 64) 2^-53 at the same bandwidth bits on both sides (the oracle's h is passed as `bandwidth`), and
|h - h_ref| <= 2 (D + 4) 2^-53 h_ref for the median rule.  Every check prints the largest fraction of its tolerance it saw
before it asserts.  The run is compared with the host loop bit for bit."""
import ctypes

import numpy as np
import pytest

import _svgd_oracle as S
from test_gpu_ksd import _draws, _models

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 5), (63, 16), (64, 17), (65, 33), (129, 1), (200, 40), (260, 40)]


@pytest.fixture(scope='module')
def vb():
    import viabel_amd
    from viabel_amd import _lib
    _lib.default_engine()
    return viabel_amd


@pytest.fixture(scope='module')
def eng(vb):
    from viabel_amd import _lib
    return _lib.default_engine()


def _scale(d, seed):
    return 10.0 ** np.linspace(-2.0, 2.0, d) * np.exp(0.2 * np.random.RandomState(seed).randn(d))


def _reference(x, g, scale):
    """The oracle's median bandwidth (extended precision), its float64 value, and the oracle's direction at that value."""
    h_ref = S.direction(x, g, scale)['h']
    h64 = float(h_ref)
    return h_ref, h64, S.direction(x, g, scale, bandwidth=h64)


def _check_phi(label, phi, ref, n, d):
    frac = float(np.max(np.abs(phi - ref['phi']) / (S.tolerance(n, d) * ref['E'])))
    print('%s: max |phi - ref| = %.3f tol E (tol %.2e)' % (label, frac, S.tolerance(n, d)))
    assert frac <= 1.0, (label, frac)
    return frac


def _check_h(label, h, h_ref, d):
    frac = float(abs(h - h_ref) / (S.bandwidth_tolerance(d) * h_ref))
    print('%s: |h - ref| = %.3f of its tolerance (h %.6g)' % (label, frac, h))
    assert frac <= 1.0, (label, frac)
    return frac


def _raw_direction(eng, x, scores, scale, bandwidth, n=None, d=None):
    """The C entry as it is, no Python checks: (return code, phi, h)."""
    from viabel_amd._lib import _dptr, _f64
    x = _f64(x)
    n = x.shape[0] if n is None else n
    d = x.shape[1] if d is None else d
    scores = None if scores is None else _f64(scores)
    scale = None if scale is None else _f64(scale)
    phi = np.full((max(n, 1), max(d, 1)), np.nan)
    h = ctypes.c_double(np.nan)
    rc = eng._lib.vb_svgd_direction(eng._ctx, _dptr(x), n, d, None if scores is None else _dptr(scores),
                                    None if scale is None else _dptr(scale), bandwidth, _dptr(phi), None, ctypes.addressof(h))
    return rc, phi, h.value


# ---- 1. the direction against the oracle ----------------------------------------------------------------------------------
@pytest.mark.parametrize('shift', [0.0, 1e6])
@pytest.mark.parametrize('n,d', SHAPES)
def test_direction_matches_the_oracle(eng, n, d, shift):
    x, g = _draws(n, d, 100 * n + d)
    x = x + shift
    for scale in (None, _scale(d, n + d)):
        h_ref, h64, ref = _reference(x, g, scale)
        label = 'n %d D %d shift %g scale %s' % (n, d, shift, 'none' if scale is None else 'given')
        phi, h, logp = eng.svgd_direction(x, scores=g, scale=scale, bandwidth=h64)
        assert h == h64 and logp is None                                     # a fixed bandwidth is returned unchanged
        _check_phi(label, phi, ref, n, d)
        again, h_again, _ = eng.svgd_direction(x, scores=g, scale=scale, bandwidth=h64)
        assert np.array_equal(again, phi) and h_again == h
        # the median rule: h against the oracle's, twice the same bits, and the direction at the device's own h
        phi_m, h_m, _ = eng.svgd_direction(x, scores=g, scale=scale)
        _check_h(label, h_m, float(h_ref), d)
        phi_m2, h_m2, _ = eng.svgd_direction(x, scores=g, scale=scale)
        assert h_m2 == h_m and np.array_equal(phi_m2, phi_m)
        _check_phi(label + ', median rule', phi_m, S.direction(x, g, scale, bandwidth=h_m), n, d)


# ---- 2. the median rule ---------------------------------------------------------------------------------------------------
def test_median_rule_with_ties(eng):
    rng = np.random.RandomState(7)
    n, d = 150, 3
    # integer coordinates and powers of two as scale: every r2 is exact on both sides, many pairs tie, the device's h is the
    # oracle's up to the one division
    x = np.round(2.0 * rng.randn(n, d)) + 0.0
    x -= np.round(x.mean(axis=0))
    x[0] -= x.sum(axis=0)                                                    # column means exactly 0
    assert np.all(x.sum(axis=0) == 0.0)
    g = rng.randn(n, d)
    for scale in (None, np.array([0.5, 2.0, 4.0])):
        h_ref = S.direction(x, g, scale)['h']
        _, h, _ = eng.svgd_direction(x, scores=g, scale=scale)
        _check_h('ties, scale %s' % (scale is not None), h, float(h_ref), d)
        y = x if scale is None else x / scale
        m = S.lower_median(S.squared_distances(y))
        # the exact median and no neighbouring value: distinct distances differ by 1/16 at least
        assert abs(h * np.log(n + 1.0) - float(m)) <= 1e-12 * float(m)
    # more than half of the pairs at distance 0: m = 0, h = 1
    x = np.repeat(rng.randn(3, d), [120, 20, 10], axis=0)
    _, h, _ = eng.svgd_direction(x, scores=g)
    assert h == 1.0 and S.direction(x, g)['h'] == 1.0


def test_median_rule_edge_cases(eng):
    rng = np.random.RandomState(8)
    g = rng.randn(70, 4)
    phi, h, _ = eng.svgd_direction(rng.randn(1, 4), scores=g[:1])            # n = 1
    assert h == 1.0 and np.array_equal(phi, g[:1])
    x = np.tile(rng.randn(1, 4) + 1e3, (70, 1))                              # all particles equal
    phi, h, _ = eng.svgd_direction(x, scores=g)
    assert h == 1.0
    ref = S.direction(x, g, bandwidth=1.0)
    _check_phi('all particles equal', phi, ref, 70, 4)
    np.testing.assert_allclose(phi, np.tile(g.mean(axis=0), (70, 1)), rtol=0.0, atol=1e-13)
    phi, h, _ = eng.svgd_direction(x, scores=g, bandwidth=0.37)              # a fixed bandwidth is returned unchanged
    assert h == 0.37


# ---- 3. device scores -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['gaussian', 'correlated', 'logistic', 'multilevel', 'source'])
def test_device_scores(vb, eng, name):
    model = _models(vb)[name]
    d, n = model.dim, 130
    rng = np.random.RandomState(31)
    x = 0.6 * rng.randn(n, d)
    scale = np.exp(0.3 * rng.randn(d))
    before = model(x)
    g = model.grad(x)
    for kwargs in (dict(), dict(scale=scale)):
        h_ref, h64, ref = _reference(x, g, kwargs.get('scale'))
        res = model.svgd_direction(x, bandwidth=h64, **kwargs)
        assert res['bandwidth'] == h64
        _check_phi('%s %s' % (name, sorted(kwargs)), res['phi'], ref, n, d)
        given, _, _ = eng.svgd_direction(x, scores=g, bandwidth=h64, **kwargs)
        assert np.array_equal(given, res['phi'])
        np.testing.assert_allclose(res['logp'], before, rtol=1e-12, atol=1e-12)
        med = model.svgd_direction(x, **kwargs)
        _check_h('%s %s' % (name, sorted(kwargs)), med['bandwidth'], float(h_ref), d)
        given, h_given, _ = eng.svgd_direction(x, scores=g, **kwargs)
        assert h_given == med['bandwidth'] and np.array_equal(given, med['phi'])
    assert np.array_equal(model(x), before)          # the workspace overlaps nothing the model evaluates through
    assert np.array_equal(model.grad(x), g)


# ---- 4. the run is the host loop, bit for bit -----------------------------------------------------------------------------
def _optimizers(vb):
    return {'sgd': lambda: vb.StochasticGradientOptimizer(0.05), 'rmsprop': lambda: vb.RMSProp(0.05),
            'adam': lambda: vb.Adam(0.05), 'adagrad': lambda: vb.Adagrad(0.3)}


def _host_loop(model, x0, opt, n_iters, scale):
    x, hs = x0.copy(), []
    for _ in range(n_iters):
        res = model.svgd_direction(x, scale=scale)
        direction = opt.descent_direction(-res['phi'])
        x = x - opt._learning_rate * direction
        hs.append(res['bandwidth'])
    return x, np.array(hs)


@pytest.fixture(scope='module')
def run_targets(vb):
    rng = np.random.RandomState(61)
    gauss = vb.GaussianModel(rng.randn(17), np.exp(0.5 * rng.randn(17)))
    logistic = _models(vb)['logistic']
    return {'gaussian': (gauss, rng.randn(65, 17), np.exp(0.3 * rng.randn(17))),
            'logistic': (logistic, 0.5 * rng.randn(65, logistic.dim), None)}


@pytest.mark.parametrize('kind', ['sgd', 'rmsprop', 'adam', 'adagrad'])
@pytest.mark.parametrize('target', ['gaussian', 'logistic'])
def test_run_equals_the_host_loop(vb, eng, run_targets, target, kind):
    model, x0, scale = run_targets[target]
    n, d = x0.shape
    p, iters, first = n * d, 6, 2
    make = _optimizers(vb)[kind]
    opt = make()
    x_host, h_host = _host_loop(model, x0, opt, iters, scale)
    dev = make()
    eng.set_model(model.device_spec())
    out = eng.svgd_run(x0, iters, dev._device_kind, dev._device_hyper(), state=dev._device_state(p), scale=scale)
    assert np.array_equal(out['particles'], x_host)
    assert np.array_equal(out['bandwidth_history'], h_host)
    zeros = np.zeros(p)
    host_state = {'sgd': [zeros, zeros], 'rmsprop': [np.ravel(getattr(opt, '_avg_grad_sq', zeros)), zeros],
                  'adam': [np.ravel(getattr(opt, '_avg_grad_sq', zeros)), np.ravel(getattr(opt, '_momentum', zeros))],
                  'adagrad': [np.ravel(getattr(opt, '_sum_grad_sq', zeros)), zeros]}[kind]
    assert np.array_equal(out['state'], np.concatenate(host_state))
    np.testing.assert_allclose(out['logp'], model(x_host), rtol=1e-12, atol=1e-12)
    assert np.all(np.isfinite(out['phi_rms_history'])) and np.all(out['phi_rms_history'] > 0.0)
    np.testing.assert_allclose(out['logp_history'][0], np.mean(model(x0)), rtol=1e-12)
    # two runs return the same bits
    again = eng.svgd_run(x0, iters, dev._device_kind, dev._device_hyper(), state=None, scale=scale)
    for key in out:
        assert np.array_equal(again[key], out[key]), key
    # a + b iterations = a iterations continued by b
    a = eng.svgd_run(x0, first, dev._device_kind, dev._device_hyper(), state=None, scale=scale)
    b = eng.svgd_run(a['particles'], iters - first, dev._device_kind, dev._device_hyper(),
                     state=None if kind == 'sgd' else a['state'], scale=scale)
    assert np.array_equal(b['particles'], out['particles']) and np.array_equal(b['state'], out['state'])
    assert np.array_equal(b['logp'], out['logp'])
    for key in ('bandwidth_history', 'phi_rms_history', 'logp_history'):
        assert np.array_equal(np.concatenate([a[key], b[key]]), out[key]), key


# ---- 5. end to end --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', [1, 2, 3])
def test_svgd_end_to_end(vb, capsys, seed):
    rng = np.random.RandomState(seed)
    A = rng.randn(4, 4)
    sds = 10.0 ** np.linspace(-1.0, 1.0, 4)
    cov = (A @ A.T / 4.0 + 0.5 * np.eye(4)) * np.outer(sds, sds)
    mean = 3.0 * rng.randn(4)
    x0 = rng.randn(128, 4) * sds
    model = vb.CorrelatedGaussianModel(mean, covariance=cov)
    optimizer = vb.Adagrad(0.5)
    capsys.readouterr()
    res = vb.svgd(model, n_particles=128, n_iters=500, init=x0, scale=sds, optimizer=optimizer)
    printed = capsys.readouterr().out
    assert printed.startswith('svgd: 128 particles, 500 iterations')
    sd_true = np.sqrt(np.diag(cov))
    corr_true = cov / np.outer(sd_true, sd_true)
    corr = res['cov'] / np.outer(res['sd'], res['sd'])
    e_mean = np.max(np.abs(res['mean'] - mean) / sd_true)
    e_sd = np.max(np.abs(res['sd'] / sd_true - 1.0))
    e_corr = np.max(np.abs(corr - corr_true))
    ratio = res['phi_rms_history'][-1] / res['phi_rms_history'][0]
    print('seed %d: mean %.4f sd (bound 0.05), sd %.4f (bound 0.2), correlation %.4f (bound 0.05), rms(phi) ratio %.4g '
          '(bound 0.1)' % (seed, e_mean, e_sd, e_corr, ratio))
    assert e_mean <= 0.05 and e_sd <= 0.2 and e_corr <= 0.05 and ratio < 0.1
    assert res['particles'].shape == (128, 4) and res['logp'].shape == (128,) and res['n_iters'] == 500
    assert res['optimizer'] is optimizer and np.array_equal(res['scale'], sds)
    np.testing.assert_allclose(res['logp'], model(res['particles']), rtol=1e-12, atol=1e-12)
    for key in ('bandwidth_history', 'phi_rms_history', 'logp_history'):
        assert res[key].shape == (500,) and np.all(np.isfinite(res[key]))
    if seed == 1:      # the returned optimiser continues the run: 500 = 300 + 200
        opt2 = vb.Adagrad(0.5)
        part = vb.svgd(model, n_particles=128, n_iters=300, init=x0, scale=sds, optimizer=opt2)
        rest = vb.svgd(model, n_particles=128, n_iters=200, init=part['particles'], scale=sds, optimizer=part['optimizer'])
        assert np.array_equal(rest['particles'], res['particles'])
        # from a fit: the starts and the scale come from the approximation
        approx = vb.MFGaussian(4, seed=5)
        theta = np.concatenate([mean, np.log(sd_true)])
        fit = vb.svgd(model, n_particles=64, n_iters=5, var_param=theta, approx=approx)
        np.testing.assert_allclose(fit['scale'], sd_true, rtol=1e-14)
        assert fit['particles'].shape == (64, 4)


# ---- 6. errors at the C level ---------------------------------------------------------------------------------------------
def test_errors_leave_the_context_usable(vb, eng):
    from viabel_amd import _lib
    from viabel_amd._lib import _dptr
    model = _models(vb)['logistic']
    d = model.dim
    rng = np.random.RandomState(51)
    x = rng.randn(40, d)
    expected = model(x)
    g = model.grad(x)
    INVALID, UNSUPPORTED, NUMERIC, STATE = _lib.VB_ERR_INVALID, _lib.VB_ERR_UNSUPPORTED, _lib.VB_ERR_NUMERIC, _lib.VB_ERR_STATE

    def usable():
        assert np.array_equal(model(x), expected)

    def raw_run(e, x0, n=None, dd=None, scale=None, bandwidth=0.0, kind=_lib.OPT_ADAGRAD, hyper=(0.1, 0.0, 0.0, 1e-8),
                n_iters=2):
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        n = x0.shape[0] if n is None else n
        dd = x0.shape[1] if dd is None else dd
        hyper = np.array(hyper, dtype=np.float64)
        scale = None if scale is None else np.ascontiguousarray(scale, dtype=np.float64)
        out_x, out_lp = np.zeros((max(n, 1), max(dd, 1))), np.zeros(max(n, 1))
        hh, hr, hl = np.zeros(max(n_iters, 1)), np.zeros(max(n_iters, 1)), np.zeros(max(n_iters, 1))
        return e._lib.vb_svgd_run(e._ctx, _dptr(x0), n, dd, None if scale is None else _dptr(scale), bandwidth, kind,
                                  _dptr(hyper), n_iters, None, 0, _dptr(out_x), _dptr(out_lp), _dptr(hh), _dptr(hr), _dptr(hl))

    big = np.zeros((8193, 1))
    bad_scale = np.ones(d)
    bad_scale[2] = 0.0
    nan_scores = g.copy()
    nan_scores[7, 1] = np.nan
    cases = [
        ('wrong d against the bound model', INVALID, dict(x=x[:, :d - 1], scores=None)),
        ('n = 0', INVALID, dict(x=x, scores=g, n=0)),
        ('n = 8193', UNSUPPORTED, dict(x=big, scores=big)),
        ('a zero in scale', INVALID, dict(x=x, scores=g, scale=bad_scale)),
        ('negative bandwidth', INVALID, dict(x=x, scores=g, bandwidth=-1.0)),
        ('a NaN score', NUMERIC, dict(x=x, scores=nan_scores)),
    ]
    eng.set_model(model.device_spec())
    for label, code, kw in cases:
        rc, _, _ = _raw_direction(eng, kw['x'], kw.get('scores'), kw.get('scale'), kw.get('bandwidth', 0.0), n=kw.get('n'))
        assert rc == code, (label, rc, code, eng._lib.vb_last_error(eng._ctx).decode())
        usable()
    eng.set_model(model.device_spec())
    run_cases = [
        ('wrong d', INVALID, dict(x0=x[:, :d - 1])),
        ('n = 0', INVALID, dict(x0=x, n=0)),
        ('n = 8193', UNSUPPORTED, dict(x0=np.zeros((8193, d)))),
        ('a zero in scale', INVALID, dict(x0=x, scale=bad_scale)),
        ('negative bandwidth', INVALID, dict(x0=x, bandwidth=-1.0)),
        ('n_iters = 0', INVALID, dict(x0=x, n_iters=0)),
        ('unknown optimiser', INVALID, dict(x0=x, kind=7)),
    ]
    for label, code, kw in run_cases:
        rc = raw_run(eng, **kw)
        assert rc == code, (label, rc, code, eng._lib.vb_last_error(eng._ctx).decode())
        usable()
        eng.set_model(model.device_spec())
    assert raw_run(eng, x) == _lib.VB_OK
    nan_start = x.copy()
    nan_start[3, 0] = np.nan
    assert raw_run(eng, nan_start) == NUMERIC
    usable()
    # a NULL context
    assert eng._lib.vb_svgd_direction(None, 0, 0, 0, None, None, 0.0, None, None, None) == INVALID
    assert eng._lib.vb_svgd_run(None, 0, 0, 0, None, 0.0, 0, None, 0, None, 0, None, None, None, None, None) == INVALID
    # no model and no scores: a fresh engine; then a minibatch model, a host-callback model and a communicator
    fresh = _lib.Engine()
    try:
        rc, _, _ = _raw_direction(fresh, x, None, None, 0.0)
        assert rc == STATE, rc
        assert raw_run(fresh, x) == STATE
        rc, phi, h = _raw_direction(fresh, x, g, None, 0.0)                   # ... which takes given scores all the same
        ok_phi, ok_h, _ = eng.svgd_direction(x, scores=g)
        assert rc == 0 and h == ok_h and np.array_equal(phi, ok_phi)
        X = rng.randn(30, 3)
        minibatch = vb.MinibatchRegressionModel(X, (X[:, 0] > 0).astype(float), 5)
        fresh.set_model(minibatch.device_spec())
        x3 = rng.randn(10, 3)
        assert _raw_direction(fresh, x3, None, None, 0.0)[0] == UNSUPPORTED and raw_run(fresh, x3) == UNSUPPORTED
        callback = vb.CallableModel(3, lambda z: -0.5 * np.sum(z * z, axis=1), lambda z: -z)
        fresh.set_model(callback.device_spec())
        assert _raw_direction(fresh, x3, None, None, 0.0)[0] == UNSUPPORTED and raw_run(fresh, x3) == UNSUPPORTED
        assert _raw_direction(fresh, x3, -x3, None, 0.0)[0] == 0              # given scores need no device model
        fresh.set_model(model.device_spec())
        fresh.comm_init_host(lambda arr, op: None, 1, 0)
        assert raw_run(fresh, x) == UNSUPPORTED
        fresh.comm_destroy()
        assert raw_run(fresh, x) == _lib.VB_OK
    finally:
        fresh.close()
    with pytest.raises(NotImplementedError):
        minibatch.svgd_direction(x3)
    with pytest.raises(NotImplementedError):
        callback.svgd_direction(x3)
    with pytest.raises(NotImplementedError):
        vb.svgd(callback, n_particles=10, n_iters=2, init=x3)
    usable()
    _, h64, ref = _reference(x, g, None)
    phi, _, _ = eng.svgd_direction(x, scores=g, bandwidth=h64)
    _check_phi('after the errors', phi, ref, 40, d)
