"""vb_ksd (csrc/vb_ksd.hip) on the GPU against the numpy oracle of tests/_ksd_oracle.py.

Tolerance (derived, not tuned; _ksd_oracle.tolerance):  |ksd2 - ref| <= tol E,  |rowsums[i] - ref_i| <= tol E_i  with
tol = 2 (2 D + S + 64) 2^-53 and E, E_i the sums of the absolute values of everything the kernel adds up.  Every check
prints the largest error it saw as a fraction of that tolerance before it asserts."""
import ctypes

import numpy as np
import pytest

import _ksd_oracle as K
from oracle import psis as opsis

pytestmark = pytest.mark.gpu

KERNELS = [(1.0, -0.5), (0.05, -0.9), (30.0, -0.1)]
SHAPES = [(1, 1), (2, 5), (63, 16), (64, 17), (65, 33), (129, 1), (200, 40), (260, 40)]
WEIGHTS = ['none', 'student_t', 'one']


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


def _draws(s, d, seed):
    """Draws and scores whose columns span four decades, the last draw a duplicate of the first."""
    rng = np.random.RandomState(seed)
    x = rng.randn(s, d) * 10.0 ** np.linspace(-2.0, 2.0, d) + rng.randn(d)
    g = rng.randn(s, d) * 10.0 ** np.linspace(1.0, -3.0, d)
    if s > 1:
        x[-1], g[-1] = x[0], g[0]
    return x, g


def _log_weights(kind, s, seed):
    rng = np.random.RandomState(seed + 1)
    if kind == 'none':
        return None
    if kind == 'student_t':
        return 2.0 * rng.standard_t(2.5, size=s)
    lw = np.full(s, -np.inf)
    lw[s // 2] = 0.3
    return lw


def _check(label, ksd2, rowsums, ref, s, d, extra=0.0, rows=None):
    """ksd2 and rowsums within the tolerance of the oracle's `ref`; `extra`: a further relative allowance on the scales
    (0 except where the weights themselves differ); `rows`: the rows to compare (all)."""
    tol = K.tolerance(s, d) + extra
    rows = slice(None) if rows is None else rows
    f2 = abs(ksd2 - ref['ksd2']) / (tol * ref['E'])
    fr = np.max(np.abs(rowsums[rows] - ref['rowsums'][rows]) / (tol * ref['E_rows'][rows]))
    print('%s: |ksd2 - ref| = %.3f tol E, max |rowsums - ref| = %.3f tol E_i (tol %.2e)' % (label, f2, fr, tol))
    assert f2 <= 1.0 and fr <= 1.0, (label, f2, fr)
    return max(f2, fr)


def _raw(eng, x, scores, log_w, scale, c, beta, s=None, d=None, want_rows=True):
    """The C entry as it is, no Python checks: (return code, ksd2, rowsums or None)."""
    from viabel_amd._lib import _dptr, _f64
    x = _f64(x)
    s = x.shape[0] if s is None else s
    d = x.shape[1] if d is None else d
    scores = None if scores is None else _f64(scores)
    log_w = None if log_w is None else _f64(log_w)
    scale = None if scale is None else _f64(scale)
    ksd2 = ctypes.c_double(np.nan)
    rows = np.full(max(s, 1), np.nan) if want_rows else None
    rc = eng._lib.vb_ksd(eng._ctx, _dptr(x), s, d, None if scores is None else _dptr(scores),
                         None if log_w is None else _dptr(log_w), None if scale is None else _dptr(scale), c, beta,
                         ctypes.addressof(ksd2), None if rows is None else _dptr(rows))
    return rc, ksd2.value, rows


# ---- 1. the pair kernel alone -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('weights', WEIGHTS)
@pytest.mark.parametrize('s,d', SHAPES)
def test_pair_kernel_matches_the_oracle(eng, s, d, weights):
    x, g = _draws(s, d, 100 * s + d)
    lw = _log_weights(weights, s, 100 * s + d)
    for c, beta in KERNELS:
        ref = K.ksd(x, g, lw, c=c, beta=beta)
        ksd2, rows = eng.ksd(x, scores=g, log_w=lw, c=c, beta=beta)
        _check('S %d D %d %s c %g beta %g' % (s, d, weights, c, beta), ksd2, rows, ref, s, d)
        again2, again_rows = eng.ksd(x, scores=g, log_w=lw, c=c, beta=beta)
        assert again2 == ksd2 and np.array_equal(again_rows, rows)
        rc, alone, _ = _raw(eng, x, g, lw, None, c, beta, want_rows=False)          # rowsums = NULL
        assert rc == 0 and alone == ksd2


# ---- 2. uneven splits -------------------------------------------------------------------------------------------------
def test_uneven_column_splits(eng):
    from viabel_amd import _lib
    s, d = 1500, 3
    blocks, splits = _lib.ksd_plan(s, eng.device_info()['cus'])
    lengths = {hi - lo for lo, hi in _lib.ksd_split_tiles(blocks, splits)}
    if len(lengths) == 1:
        pytest.skip('ksd_plan(1500, %d) = (%d, %d) deals equal ranges on this device' % (eng.device_info()['cus'], blocks, splits))
    x, g = _draws(s, d, 1500)
    lw = _log_weights('student_t', s, 1500)
    ref = K.ksd(x, g, lw)
    ksd2, rows = eng.ksd(x, scores=g, log_w=lw)
    _check('S 1500 D 3, %d blocks x %d splits' % (blocks, splits), ksd2, rows, ref, s, d)


# ---- 3. zero weights --------------------------------------------------------------------------------------------------
def test_draws_of_zero_weight_add_nothing(eng):
    s, d, extra = 100, 7, 37
    x, g = _draws(s + extra, d, 3)
    lw = np.random.RandomState(3).randn(s + extra)
    dead = np.random.RandomState(4).choice(s + extra, extra, replace=False)
    lw[dead] = -np.inf
    live = np.setdiff1d(np.arange(s + extra), dead)
    ref = K.ksd(x[live], g[live], lw[live], c=0.7, beta=-0.3)
    ksd2, rows = eng.ksd(x, scores=g, log_w=lw, c=0.7, beta=-0.3)
    _check('with %d draws of weight 0' % extra, ksd2, rows[live], ref, s + extra, d)
    without2, without_rows = eng.ksd(x[live], scores=g[live], log_w=lw[live], c=0.7, beta=-0.3)
    _check('without them', without2, without_rows, ref, s, d)
    assert np.all(np.isfinite(rows))


# ---- 4. device scores -------------------------------------------------------------------------------------------------
QUARTIC = r"""
__device__ double vb_log_density(const double* z, int d, const double* p, double* g) {
  double f = 0.0;
  for (int j = 0; j < d; ++j) {
    const double q = z[j] * z[j];
    f -= 0.5 * p[0] * q + 0.1 * q * q;
    if (g) g[j] = -p[0] * z[j] - 0.4 * q * z[j];
  }
  return f;
}
"""


def _models(vb):
    rng = np.random.RandomState(21)
    A = rng.randn(6, 6)
    X = rng.randn(50, 5)
    y = (rng.rand(50) < 0.5).astype(float)
    Xm = rng.randn(60, 3)
    groups = rng.randint(0, 5, size=60)
    ym = (rng.rand(60) < 0.5).astype(float)
    return {
        'gaussian': vb.GaussianModel(rng.randn(4), np.exp(0.5 * rng.randn(4))),
        'correlated': vb.CorrelatedGaussianModel(rng.randn(6), covariance=A @ A.T + 6.0 * np.eye(6)),
        'logistic': vb.LogisticRegressionModel(X, y, prior_sd=2.0),
        'multilevel': vb.MultilevelRegressionModel(Xm, ym, groups, 5),
        'source': vb.SourceModel(3, QUARTIC, np.array([0.8])),
    }


@pytest.mark.parametrize('name', ['gaussian', 'correlated', 'logistic', 'multilevel', 'source'])
def test_device_scores(vb, eng, name):
    model = _models(vb)[name]
    d, s = model.dim, 130
    assert d == dict(gaussian=4, correlated=6, logistic=5, multilevel=9, source=3)[name]
    rng = np.random.RandomState(31)
    x = 0.6 * rng.randn(s, d)
    lw = rng.randn(s)
    scale = np.exp(0.3 * rng.randn(d))
    before = model(x)
    g = model.grad(x)
    for kwargs in (dict(), dict(log_weights=lw, scale=scale, c=0.6, beta=-0.7)):
        res = model.ksd_from_draws(x, **kwargs)
        ref = K.ksd(x, g, kwargs.get('log_weights'), scale=kwargs.get('scale'), c=kwargs.get('c', 1.0),
                    beta=kwargs.get('beta', -0.5))
        _check('%s %s' % (name, sorted(kwargs)), res['ksd2'], res['rowsums'], ref, s, d)
        given2, given_rows = eng.ksd(x, scores=g, log_w=kwargs.get('log_weights'), scale=kwargs.get('scale'),
                                     c=kwargs.get('c', 1.0), beta=kwargs.get('beta', -0.5))
        _check('%s, scores given' % name, given2, given_rows, ref, s, d)
        w = ref['w']
        assert res['ksd'] == np.sqrt(max(res['ksd2'], 0.0)) and res['n_samples'] == s
        assert abs(res['ess'] - 1.0 / np.sum(w * w)) <= 1e-12 * s
        assert (res['c'], res['beta']) == (kwargs.get('c', 1.0), kwargs.get('beta', -0.5))
    assert np.array_equal(model(x), before)          # the workspace overlaps nothing the model evaluates through
    assert np.array_equal(model.grad(x), g)


# ---- 5. scale ---------------------------------------------------------------------------------------------------------
def test_scale_equals_prescaled_inputs(eng):
    s, d = 150, 20
    x, g = _draws(s, d, 5)
    ell = 10.0 ** np.linspace(-2.0, 2.0, d) * np.exp(0.2 * np.random.RandomState(5).randn(d))
    lw = _log_weights('student_t', s, 5)
    ref = K.ksd(x, g, lw, scale=ell)
    scaled2, scaled_rows = eng.ksd(x, scores=g, log_w=lw, scale=ell)
    _check('scale given', scaled2, scaled_rows, ref, s, d)
    pre2, pre_rows = eng.ksd(x / ell, scores=g * ell, log_w=lw)
    assert pre2 == scaled2 and np.array_equal(pre_rows, scaled_rows)      # the staging kernel rounds as numpy does


# ---- 6. end to end ----------------------------------------------------------------------------------------------------
def test_ksd_end_to_end(vb, capsys):
    """vb.ksd from a fit equals the oracle on the same draws; with weights='psis' the device-smoothed log weights differ
    from oracle.psis by up to 1e-9 (the bound tests/test_gpu_predict.py uses for them), which moves the bilinear form
    sum w_i w_j k_p(i, j) by at most (2 * 1e-9 + 1e-18) E: that much is added to the tolerance there and nowhere else."""
    model = _models(vb)['logistic']
    D, n = model.dim, 512
    rng = np.random.RandomState(41)
    theta = np.concatenate([0.3 * rng.randn(D), np.full(D, -1.0) + 0.2 * rng.randn(D)])
    sd = np.exp(theta[D:])
    for weights in ('psis', None):
        capsys.readouterr()
        res = vb.ksd(theta, model=model, approx=vb.MFGaussian(D, seed=5), n_samples=n, weights=weights)
        printed = capsys.readouterr().out
        assert printed.startswith('KSD = ') and '%d draws' % n in printed and 'effective sample size' in printed
        assert ('khat' in printed) == (weights == 'psis')
        samples, log_ratios = vb.samples_and_log_weights(theta, model, vb.MFGaussian(D, seed=5), n)
        log_w = None if weights is None else opsis.psis_smooth(log_ratios, 1.0)[0]
        np.testing.assert_allclose(res['scale'], sd, rtol=1e-14)               # scale='auto': the approximation's sds
        ref = K.ksd(samples, model.grad(samples), log_w, scale=res['scale'])   # (the scale the entry used, to the bit)
        _check('fit, weights %s' % weights, res['ksd2'], res['rowsums'], ref, n, D, extra=0.0 if weights is None else 2.1e-9)
        assert (res['khat'] is None) == (weights is None) and res['n_samples'] == n
        assert res['ksd'] == np.sqrt(max(res['ksd2'], 0.0))
        assert abs(res['ess'] - 1.0 / np.sum(ref['w'] ** 2)) <= 1e-6 * n
    # an objective in place of model and approx, and scale=None
    objective = vb.ExclusiveKL(vb.MFGaussian(D, seed=5), model, 8)
    res = vb.ksd(theta, objective=objective, n_samples=n, weights=None, scale=None)
    assert res['scale'] is None and np.isfinite(res['ksd'])
    # from draws: device scores and given scores, scale='auto' = the weighted sds of the draws
    x = theta[:D] + sd * rng.randn(300, D)
    lw = 0.5 * rng.randn(300)
    w = K.normalised_weights(lw, 300)
    wsd = np.sqrt(w @ (x - w @ x) ** 2)
    g = model.grad(x)
    capsys.readouterr()
    from_model = vb.ksd(samples=x, log_weights=lw, model=model, c=0.9, beta=-0.4)
    printed = capsys.readouterr().out
    assert printed.startswith('KSD = ') and '300 draws' in printed and 'khat' not in printed
    from_scores = vb.ksd(samples=x, log_weights=lw, scores=g, c=0.9, beta=-0.4)
    for label, res in (('draws, model', from_model), ('draws, scores', from_scores)):
        np.testing.assert_allclose(res['scale'], wsd, rtol=1e-13)
        ref = K.ksd(x, g, lw, scale=res['scale'], c=0.9, beta=-0.4)          # (the scale the entry used, to the bit)
        _check(label, res['ksd2'], res['rowsums'], ref, 300, D)
        assert res['khat'] is None
    given = vb.ksd(samples=x, scores=g, scale=np.ones(D))
    plain = vb.ksd(samples=x, scores=g, scale=None)
    assert given['ksd2'] == plain['ksd2']


# ---- 7. errors at the C level -----------------------------------------------------------------------------------------
def test_errors_leave_the_context_usable(vb, eng):
    from viabel_amd import _lib
    model = _models(vb)['logistic']
    d = model.dim
    rng = np.random.RandomState(51)
    x = rng.randn(40, d)
    expected = model(x)
    g = model.grad(x)
    INVALID, UNSUPPORTED, NUMERIC, STATE = _lib.VB_ERR_INVALID, _lib.VB_ERR_UNSUPPORTED, _lib.VB_ERR_NUMERIC, _lib.VB_ERR_STATE

    def usable():
        assert np.array_equal(model(x), expected)

    big = np.zeros((65537, 1))
    bad_scale = np.ones(d)
    bad_scale[2] = 0.0
    nan_scores = g.copy()
    nan_scores[7, 1] = np.nan
    cases = [
        ('wrong d against the bound model', INVALID, dict(x=x[:, :d - 1], scores=None)),
        ('s = 0', INVALID, dict(x=x, scores=g, s=0)),
        ('s = 65537', UNSUPPORTED, dict(x=big, scores=big)),
        ('beta = 0', INVALID, dict(x=x, scores=g, beta=0.0)),
        ('beta = -1', INVALID, dict(x=x, scores=g, beta=-1.0)),
        ('c = 0', INVALID, dict(x=x, scores=g, c=0.0)),
        ('a zero in scale', INVALID, dict(x=x, scores=g, scale=bad_scale)),
        ('all weights -inf', INVALID, dict(x=x, scores=g, log_w=np.full(40, -np.inf))),
        ('a NaN score', NUMERIC, dict(x=x, scores=nan_scores)),
    ]
    for label, code, kw in cases:
        rc, _, _ = _raw(eng, kw['x'], kw.get('scores'), kw.get('log_w'), kw.get('scale'), kw.get('c', 1.0),
                        kw.get('beta', -0.5), s=kw.get('s'))
        assert rc == code, (label, rc, code, eng._lib.vb_last_error(eng._ctx).decode())
        usable()
    assert eng._lib.vb_ksd(None, 0, 0, 0, None, None, None, 0.0, 0.0, None, None) == INVALID
    # no model and no scores: a fresh engine
    fresh = _lib.Engine()
    try:
        rc, _, _ = _raw(fresh, x, None, None, None, 1.0, -0.5)
        assert rc == STATE, rc
        rc, value, _ = _raw(fresh, x, g, None, None, 1.0, -0.5)          # ... which takes given scores all the same
        assert rc == 0 and value == eng.ksd(x, scores=g)[0]
    finally:
        fresh.close()
    usable()
    ok, rows = eng.ksd(x, scores=g)
    ref = K.ksd(x, g)
    _check('after the errors', ok, rows, ref, 40, d)
