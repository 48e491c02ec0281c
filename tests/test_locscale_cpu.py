"""CPU: LocationScaleRegressionModel's host side (constructor validation, device_spec layout with and without a scale
design, unpack, sigma, export) and the numpy oracle the GPU tests compare against (tests/_locscale_oracle.py): its gradient and
Hessian against differences, its per-observation terms against scipy's normal and Student-t log densities, and its float64
form against the extended-precision twin."""
import numpy as np
import pytest

import viabel_amd as vb
from viabel_amd import _lib
from _locscale_oracle import LocScaleOracle

LIKELIHOODS = ['gaussian', 'student_t']
SHAPES = [(1, 1, 1), (5, 3, 33), (17, 1, 130)]                    # (p, q, n_data)


def _data(p, q, n_data, seed=0):
    rng = np.random.RandomState(seed)
    X = rng.randn(n_data, p) / np.sqrt(p)
    W = rng.randn(n_data, q) / np.sqrt(q)
    y = rng.randn(n_data)
    return X, y, W


def test_exported_from_package_and_bound():
    assert vb.LocationScaleRegressionModel is vb.models.LocationScaleRegressionModel
    assert 'LocationScaleRegressionModel' in vb.models.__all__
    assert _lib.MODEL_LOCSCALE == 7 and _lib.MODEL_LOCSCALE in _lib.MODELS_WITH_ROWS
    assert _lib.LOCSCALE_CHUNK_DOUBLES > 0
    assert 'vb_locscale_pointwise' in _lib.SIGNATURES


def test_header_declares_the_model_id_and_chunk_constant():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'viabel_hip.h')).read()
    assert re.search(r'#define\s+VB_MODEL_LOCSCALE\s+7\b', header)
    assert re.search(r'#define\s+VB_LOCSCALE_GAUSSIAN\s+%d\b' % _lib.LOCSCALE_GAUSSIAN, header)
    assert re.search(r'#define\s+VB_LOCSCALE_STUDENT_T\s+%d\b' % _lib.LOCSCALE_STUDENT_T, header)
    assert re.search(r'int\s+vb_locscale_pointwise\s*\(', header)
    common = open(os.path.join(root, 'viabel_amd', 'csrc', 'vb_common.h')).read()
    m = re.search(r'kLocScaleChunkDoubles\s*=\s*\(int64_t\)(\d+)\s*<<\s*(\d+)', common)
    assert m and int(m.group(1)) << int(m.group(2)) == _lib.LOCSCALE_CHUNK_DOUBLES
    assert re.search(r'model_has_rows\(int id\)\s*\{[^}]*VB_MODEL_LOCSCALE', common)


def test_spec_layout_with_a_scale_design():
    X, y, W = _data(3, 2, 11, seed=3)
    m = vb.LocationScaleRegressionModel(X, y, W, likelihood='student_t', df=5.5, prior_sd=2.5, scale_prior_sd=0.7)
    assert m.dim == 5 and m.n_data == 11 and m.n_features == 3 and m.n_scale_features == 2
    model_id, dim, dparams, iparams = m.device_spec()
    assert model_id == _lib.MODEL_LOCSCALE and dim == 5
    assert dparams.dtype == np.float64 and dparams.shape == (11 * 3 + 11 + 11 * 2 + 3,)
    np.testing.assert_array_equal(dparams[:33].reshape(11, 3), X)
    np.testing.assert_array_equal(dparams[33:44], y)
    np.testing.assert_array_equal(dparams[44:66].reshape(11, 2), W)
    assert list(dparams[66:]) == [2.5, 0.7, 5.5]
    assert iparams.dtype == np.int64 and list(iparams) == [11, 3, 2, _lib.LOCSCALE_STUDENT_T, 0]
    assert m.device_spec() is m.device_spec()                     # cached: the engine keys on identity


def test_spec_layout_with_a_constant_scale():
    X, y, _ = _data(3, 1, 11, seed=4)
    m = vb.LocationScaleRegressionModel(X, y)
    assert (m.likelihood, m.df, m.prior_sd, m.scale_prior_sd) == ('gaussian', 4.0, 10.0, 1.0)
    assert m.W is None and m.dim == 4 and m.n_scale_features == 1
    model_id, dim, dparams, iparams = m.device_spec()
    assert model_id == _lib.MODEL_LOCSCALE and dim == 4
    assert dparams.shape == (11 * 3 + 11 + 3,)                    # no W: the constant scale does not carry a design
    np.testing.assert_array_equal(dparams[:33].reshape(11, 3), X)
    np.testing.assert_array_equal(dparams[33:44], y)
    assert list(dparams[44:]) == [10.0, 1.0, 4.0]
    assert list(iparams) == [11, 3, 1, _lib.LOCSCALE_GAUSSIAN, 1]


@pytest.mark.parametrize('kwargs', [
    dict(X=np.zeros(5)),                                          # X not 2-D
    dict(X=np.zeros((5, 0))),                                     # p = 0
    dict(X=np.zeros((0, 2)), y=np.zeros(0)),                      # no observations
    dict(y=np.zeros(4)),                                          # y of the wrong length
    dict(W=np.ones(5)),                                           # W not 2-D
    dict(W=np.ones((4, 2))),                                      # W with the wrong number of rows
    dict(W=np.ones((5, 0))),                                      # q = 0
    dict(y=np.array([0.0, 1.0, np.inf, 1.0, 0.0])),               # y not finite
    dict(y=np.array([0.0, 1.0, np.nan, 1.0, 0.0])),
    dict(X=np.array([[1.0, np.nan]] * 5)),                        # X not finite
    dict(W=np.array([[1.0, np.inf]] * 5)),                        # W not finite
    dict(prior_sd=0.0),
    dict(prior_sd=-1.0),
    dict(scale_prior_sd=0.0),
    dict(scale_prior_sd=-2.0),
    dict(df=0.0),
    dict(df=-3.0),
    dict(df=np.inf),
    dict(likelihood='cauchy'),
])
def test_constructor_validation(kwargs):
    args = dict(X=np.ones((5, 2)), y=np.array([0.0, 1.0, 1.5, -1.0, 0.0]), W=np.ones((5, 3)))
    vb.LocationScaleRegressionModel(**args)                       # the baseline is valid
    args.update(kwargs)
    with pytest.raises(ValueError):
        vb.LocationScaleRegressionModel(**args)


def test_unpack_and_sigma():
    X, y, W = _data(2, 3, 9)
    m = vb.LocationScaleRegressionModel(X, y, W)
    theta = np.random.RandomState(0).randn(4, m.dim)
    b, g = m.unpack(theta)
    assert b.shape == (4, 2) and g.shape == (4, 3)
    np.testing.assert_array_equal(b, theta[:, :2])
    np.testing.assert_array_equal(g, theta[:, 2:])
    b1, g1 = m.unpack(theta[1])
    assert b1.shape == (2,) and g1.shape == (3,)
    sg = m.sigma(theta)
    assert sg.shape == (4, 9) and m.sigma(theta[1]).shape == (9,)
    np.testing.assert_allclose(sg, np.exp(theta[:, 2:] @ W.T), rtol=1e-15)
    np.testing.assert_array_equal(m.sigma(theta[1]), sg[1])
    with pytest.raises(ValueError):
        m.unpack(np.zeros(m.dim + 1))
    c = vb.LocationScaleRegressionModel(X, y)                     # constant scale: sigma = exp(theta[-1]) everywhere
    tc = np.random.RandomState(1).randn(4, c.dim)
    assert c.sigma(tc).shape == (4, 9) and c.sigma(tc[2]).shape == (9,)
    np.testing.assert_array_equal(c.sigma(tc), np.exp(tc[:, -1:]) * np.ones((4, 9)))
    np.testing.assert_array_equal(c.sigma(tc[2]), np.exp(tc[2, -1]) * np.ones(9))


def test_not_a_logistic_subclass_so_loo_declines():
    X, y, W = _data(2, 2, 7)
    m = vb.LocationScaleRegressionModel(X, y, W)
    assert not isinstance(m, vb.LogisticRegressionModel)
    with pytest.raises(NotImplementedError, match='psisloo'):
        vb.loo(model=m, approx=vb.MFGaussian(m.dim), var_param=np.zeros(2 * m.dim), n_samples=10)


def _oracle(likelihood, p, q, n_data, dtype=np.float64):
    X, y, W = _data(p, q, n_data, seed=q + n_data)
    return LocScaleOracle(X, y, W, likelihood, df=3.5, prior_sd=1.7, scale_prior_sd=0.8, dtype=dtype)


@pytest.mark.parametrize('likelihood', LIKELIHOODS)
@pytest.mark.parametrize('p,q,n_data', SHAPES)
def test_oracle_gradient_and_hessian_against_differences(likelihood, p, q, n_data):
    """Central differences at step 1e-6: the gradient below 1e-6 relative; the Hessian against differences of the gradient."""
    o = _oracle(likelihood, p, q, n_data)
    rng = np.random.RandomState(p)
    theta = 0.3 * rng.randn(3, o.dim)
    g = o.grad(theta)
    h = 1e-6
    for j in range(o.dim):
        e = np.zeros(o.dim)
        e[j] = h
        fd = (o.logp(theta + e) - o.logp(theta - e)) / (2 * h)
        assert np.max(np.abs(fd - g[:, j])) < 1e-6 * max(1.0, np.max(np.abs(g)))
    H = o.hessian(theta[0])
    assert np.allclose(H, H.T, rtol=0, atol=1e-13 * np.max(np.abs(H)))
    for j in range(o.dim):
        e = np.zeros(o.dim)
        e[j] = h
        fd = (o.grad(theta[0] + e)[0] - o.grad(theta[0] - e)[0]) / (2 * h)
        assert np.max(np.abs(fd - H[:, j])) < 1e-6 * max(1.0, np.max(np.abs(H)))
    v = rng.randn(2, o.dim)
    np.testing.assert_allclose(o.hvp(theta[0], v), v @ H, rtol=0, atol=1e-13 * np.max(np.abs(H)))


def test_constant_scale_oracle_is_the_column_of_ones():
    X, y, _ = _data(4, 1, 20, seed=5)
    a = LocScaleOracle(X, y, None, 'student_t', 6.0, 2.0, 0.9)
    b = LocScaleOracle(X, y, np.ones((20, 1)), 'student_t', 6.0, 2.0, 0.9)
    theta = 0.4 * np.random.RandomState(2).randn(5, a.dim)
    assert a.dim == 5 and a.q == 1
    np.testing.assert_array_equal(a.logp(theta), b.logp(theta))
    np.testing.assert_array_equal(a.grad(theta), b.grad(theta))


@pytest.mark.parametrize('likelihood', LIKELIHOODS)
def test_oracle_pointwise_is_scipy_logpdf(likelihood):
    from scipy import stats
    o = _oracle(likelihood, 5, 3, 33)
    theta = 0.5 * np.random.RandomState(1).randn(6, o.dim)
    eta, sigma = o.eta(theta), np.exp(o.log_scale(theta))
    if likelihood == 'gaussian':
        want = stats.norm.logpdf(o.y, loc=eta, scale=sigma)
    else:
        want = stats.t.logpdf(o.y, 3.5, loc=eta, scale=sigma)
    np.testing.assert_allclose(o.pointwise(theta), want, rtol=0, atol=1e-13 * np.max(np.abs(want)))
    np.testing.assert_allclose(o.logp(theta) - o.log_prior(theta), want.sum(axis=1), rtol=1e-13)


@pytest.mark.parametrize('likelihood', LIKELIHOODS)
def test_oracle_has_an_extended_precision_twin(likelihood):
    o, ol = _oracle(likelihood, 5, 3, 33), _oracle(likelihood, 5, 3, 33, dtype=np.longdouble)
    t = 0.3 * np.random.RandomState(1).randn(4, o.dim)
    assert ol.logp(t).dtype == np.longdouble and ol.grad(t).dtype == np.longdouble
    assert ol.pointwise(t).dtype == np.longdouble
    np.testing.assert_allclose(o.logp(t), ol.logp(t).astype(float), rtol=1e-14)
    np.testing.assert_allclose(o.grad(t), ol.grad(t).astype(float), rtol=0, atol=1e-13 * np.max(np.abs(o.grad(t))))
    np.testing.assert_allclose(o.pointwise(t), ol.pointwise(t).astype(float), rtol=0, atol=1e-14)
    x = np.random.RandomState(2).randn(3, o.dim)                  # extreme scales and predictors stay finite
    x[:, 5:] *= 30.0 / np.max(np.abs(o.log_scale(x)))
    x[:, :5] *= 1e3 / np.max(np.abs(o.eta(x)))
    assert np.all(np.isfinite(o.logp(x))) and np.all(np.isfinite(o.grad(x)))
