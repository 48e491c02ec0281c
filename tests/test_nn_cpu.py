"""CPU: NeuralNetRegressionModel's host side (constructor validation, dim, unpack, device_spec layout, export), the
C ABI's declarations of the target and its two entries, and the numpy oracle the GPU tests compare against
(tests/_nn_oracle.py): its gradient against central differences of its own f."""
import ctypes
import os
import re

import numpy as np
import pytest

import viabel_amd as vb
from viabel_amd import _lib
from _nn_oracle import KINDS, NeuralNetOracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _data(kind, p, n_data, seed=0):
    rng = np.random.RandomState(seed)
    X = rng.randn(n_data, p) / np.sqrt(p)
    if kind == 'logistic':
        y = rng.randint(0, 2, size=n_data).astype(float)
    elif kind == 'poisson':
        y = rng.poisson(2.0, size=n_data).astype(float)
    else:
        y = rng.randn(n_data)
    return X, y


def test_exported_from_package_and_bound():
    assert vb.NeuralNetRegressionModel is vb.models.NeuralNetRegressionModel
    assert 'NeuralNetRegressionModel' in vb.models.__all__
    assert _lib.MODEL_NEURALNET == 10 and _lib.MODEL_NEURALNET in _lib.MODELS_WITH_ROWS
    assert _lib.NN_CHUNK_DOUBLES == 16 << 20 and _lib.NN_PREDICT_DOUBLES > 0
    assert _lib.nn_chunk_rows(4, 2000) == (16 << 20) // 8000 and _lib.nn_chunk_rows(1 << 20, 1 << 20) == 8
    assert _lib.nn_predict_chunk(16, 4097) == (16 << 20) // (16 * 4112) and _lib.nn_predict_chunk(1 << 20, 1 << 20) == 1
    assert 'vb_nn_pointwise' in _lib.SIGNATURES and 'vb_nn_predict' in _lib.SIGNATURES
    assert callable(_lib.Engine.nn_pointwise) and callable(_lib.Engine.nn_predict)
    assert vb.NeuralNetRegressionModel._pointwise_entry == 'nn_pointwise'


def test_header_common_and_makefile_declare_the_target():
    header = open(os.path.join(ROOT, 'include', 'viabel_hip.h')).read()
    assert re.search(r'#define\s+VB_MODEL_NEURALNET\s+10\b', header)
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    pw = re.search(r'int\s+vb_nn_pointwise\s*\(([^)]*)\)\s*;', code)
    pr = re.search(r'int\s+vb_nn_predict\s*\(([^)]*)\)\s*;', code)
    assert pw and pr
    assert len(pw.group(1).split(',')) == 5 == len(_lib.SIGNATURES['vb_nn_pointwise'][1])
    assert len(pr.group(1).split(',')) == 13 == len(_lib.SIGNATURES['vb_nn_predict'][1])
    assert _lib.SIGNATURES['vb_nn_predict'] == _lib.SIGNATURES['vb_glm_predict']      # the same argument list
    assert _lib.SIGNATURES['vb_nn_pointwise'] == _lib.SIGNATURES['vb_glm_pointwise']
    common = open(os.path.join(ROOT, 'viabel_amd', 'csrc', 'vb_common.h')).read()
    m = re.search(r'kNeuralNetChunkDoubles\s*=\s*\(int64_t\)(\d+)\s*<<\s*(\d+)', common)
    assert m and int(m.group(1)) << int(m.group(2)) == _lib.NN_CHUNK_DOUBLES
    m = re.search(r'kNeuralNetPredictDoubles\s*=\s*\(int64_t\)(\d+)\s*<<\s*(\d+)', common)
    assert m and int(m.group(1)) << int(m.group(2)) == _lib.NN_PREDICT_DOUBLES
    assert re.search(r'model_has_rows\(int id\)\s*\{[^}]*VB_MODEL_NEURALNET', common)
    assert re.search(r'int n_hidden\b', common)
    makefile = open(os.path.join(ROOT, 'viabel_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS\s*:=.*\bvb_neuralnet\.hip\b', makefile, flags=re.M)
    api = open(os.path.join(ROOT, 'viabel_amd', 'csrc', 'vb_api.hip')).read()
    assert re.search(r'case VB_MODEL_NEURALNET:\s*return neuralnet_set_model\(', api)
    rows = open(os.path.join(ROOT, 'viabel_amd', 'csrc', 'vb_rows.hip')).read()
    assert re.search(r'VB_MODEL_NEURALNET\)\s*return neuralnet_rows_enqueue\(', rows)


def test_null_context_is_rejected_by_both_entries():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    buf = np.zeros(8)
    p = ctypes.cast(buf.ctypes.data, ctypes.c_void_p)
    assert lib.vb_nn_pointwise(None, None, 0, 0, None) == _lib.VB_ERR_INVALID
    assert lib.vb_nn_pointwise(None, p, 1, 4, p) == _lib.VB_ERR_INVALID
    assert lib.vb_nn_predict(None, None, 0, 0, None, None, 0, None, None, None, None, None, None) == _lib.VB_ERR_INVALID
    assert lib.vb_nn_predict(None, p, 1, 4, None, p, 1, None, p, p, p, p, None) == _lib.VB_ERR_INVALID


def test_dim_properties_and_spec_layout():
    X, y = _data('poisson', 3, 11, seed=3)
    m = vb.NeuralNetRegressionModel(X, y, 4, likelihood='poisson', prior_sd=2.5, noise_sd=0.7)
    assert m.dim == 4 * (3 + 2) + 1 and m.n_data == 11 and m.n_hidden == 4 and m.n_features == 3
    assert isinstance(m, vb.models.DeviceModel) and not isinstance(m, vb.LogisticRegressionModel)
    model_id, dim, dparams, iparams = m.device_spec()
    assert model_id == _lib.MODEL_NEURALNET and dim == 21
    assert dparams.dtype == np.float64 and dparams.shape == (11 * 3 + 11 + 2,)
    np.testing.assert_array_equal(dparams[:33].reshape(11, 3), X)
    np.testing.assert_array_equal(dparams[33:44], y)
    assert list(dparams[44:]) == [2.5, 0.7]
    assert iparams.dtype == np.int64 and list(iparams) == [11, 4, _lib.GLM_POISSON]
    assert m.device_spec() is m.device_spec()                     # cached: the engine keys on identity
    d = vb.NeuralNetRegressionModel(X, y, 1)
    assert (d.likelihood, d.prior_sd, d.noise_sd, d.dim) == ('gaussian', 1.0, 1.0, 6)
    assert list(d.device_spec()[3]) == [11, 1, _lib.GLM_GAUSSIAN]
    assert list(vb.NeuralNetRegressionModel(X, (y > 1).astype(float), 2, 'logistic').device_spec()[3]) == \
        [11, 2, _lib.GLM_BERNOULLI_LOGIT]
    assert vb.NeuralNetRegressionModel(X, y, np.int64(5)).n_hidden == 5


@pytest.mark.parametrize('kwargs', [
    dict(X=np.zeros(5)),                                          # X not 2-D
    dict(X=np.zeros((5, 0))),                                     # p = 0
    dict(X=np.zeros((0, 2)), y=np.zeros(0)),                      # no observation
    dict(y=np.zeros(4)),                                          # y of the wrong length
    dict(y=np.zeros((5, 1))),
    dict(n_hidden=0),
    dict(n_hidden=-3),
    dict(n_hidden=2.5),
    dict(n_hidden=True),
    dict(prior_sd=0.0),
    dict(prior_sd=-1.0),
    dict(noise_sd=0.0),
    dict(noise_sd=float('nan')),
    dict(likelihood='probit'),
    dict(likelihood='student_t'),
    dict(y=np.array([0.0, 1.0, 2.0, 1.0, 0.0]), likelihood='logistic'),
    dict(y=np.array([0.0, 1.0, -1.0, 1.0, 0.0]), likelihood='poisson'),
    dict(y=np.array([0.0, 1.0, np.inf, 1.0, 0.0])),
    dict(y=np.array([0.0, 1.0, np.nan, 1.0, 0.0]), likelihood='poisson'),
])
def test_constructor_validation(kwargs):
    args = dict(X=np.ones((5, 2)), y=np.array([0.0, 1.0, 1.0, 1.0, 0.0]), n_hidden=3)
    for kind in KINDS:
        vb.NeuralNetRegressionModel(likelihood=kind, **args)      # the baseline is valid under every likelihood
    args.update(kwargs)
    with pytest.raises(ValueError):
        vb.NeuralNetRegressionModel(**args)


def test_unpack():
    X, y = _data('gaussian', 2, 9)
    m = vb.NeuralNetRegressionModel(X, y, 3)
    theta = np.random.RandomState(0).randn(4, m.dim)
    W, a, v, c = m.unpack(theta)
    assert W.shape == (4, 3, 2) and a.shape == (4, 3) and v.shape == (4, 3) and c.shape == (4,)
    np.testing.assert_array_equal(W[:, 1], theta[:, 2:4])         # unit-major: w_1 follows w_0
    np.testing.assert_array_equal(a, theta[:, 6:9])
    np.testing.assert_array_equal(v, theta[:, 9:12])
    np.testing.assert_array_equal(c, theta[:, 12])
    W1, a1, v1, c1 = m.unpack(theta[1])
    assert W1.shape == (3, 2) and a1.shape == (3,) and v1.shape == (3,) and c1.shape == ()
    np.testing.assert_array_equal(W1, W[1])
    o = NeuralNetOracle(X, y, 3)
    for mine, theirs in zip(m.unpack(theta), o.unpack(theta)):
        np.testing.assert_array_equal(mine, theirs)
    eta = np.array([[c[n] + sum(v[n, k] * np.tanh(X[i] @ W[n, k] + a[n, k]) for k in range(3)) for i in range(9)]
                    for n in range(4)])                           # the definition, written out
    np.testing.assert_allclose(o.eta(theta), eta, rtol=0, atol=1e-14)
    with pytest.raises(ValueError):
        m.unpack(np.zeros(m.dim + 1))
    with pytest.raises(ValueError):
        m.unpack(np.zeros((2, 2, m.dim)))


def test_predict_from_draws_checks_its_arguments_before_the_engine():
    X, y = _data('poisson', 3, 7)
    m = vb.NeuralNetRegressionModel(X, y, 2, 'poisson')
    x = np.zeros((4, m.dim))
    for call in (lambda: m.predict_from_draws(np.zeros((4, m.dim + 1))),
                 lambda: m.predict_from_draws(x, X_new=np.zeros((5, m.dim))),          # X_new has p columns, not dim
                 lambda: m.predict_from_draws(x, X_new=np.zeros((0, 3))),
                 lambda: m.predict_from_draws(x, X_new=np.zeros((5, 3)), y_new=np.zeros(4)),
                 lambda: m.predict_from_draws(x, y_new=np.zeros(6)),
                 lambda: m.predict_from_draws(x, y_new=-np.ones(7)),                   # Poisson counts
                 lambda: m.predict_from_draws(x, log_weights=np.zeros(3)),
                 lambda: m.predict_from_draws(x, log_weights=np.full(4, -np.inf))):
        with pytest.raises(ValueError):
            call()


def test_predict_still_refuses_models_without_predict_from_draws():
    rng = np.random.RandomState(4)
    X = rng.randn(30, 2)
    for other in (vb.GaussianModel(np.zeros(6), np.ones(6)), vb.SoftmaxRegressionModel(X, rng.randint(3, size=30), 3)):
        with pytest.raises(NotImplementedError) as info:
            vb.predict(np.zeros(2 * other.dim), model=other, approx=vb.MFGaussian(other.dim))
        assert str(info.value) == (
            'predict covers LogisticRegressionModel, PoissonRegressionModel and LinearRegressionModel; {} has no '
            'predict_from_draws. What exists for it: pointwise_log_likelihood(draws) where the model defines it, to be '
            'reduced on the host'.format(type(other).__name__))
    X, y = _data('gaussian', 2, 9)
    m = vb.NeuralNetRegressionModel(X, y, 3)
    assert callable(m.predict_from_draws)
    with pytest.raises(NotImplementedError, match='psisloo'):     # loo() is not changed
        vb.loo(model=m, approx=vb.MFGaussian(m.dim), var_param=np.zeros(2 * m.dim), n_samples=10)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('h,p,n_data', [(1, 1, 1), (3, 5, 33), (4, 2, 20)])
def test_oracle_gradient_against_differences(kind, h, p, n_data):
    X, y = _data(kind, p, n_data, seed=h)
    o = NeuralNetOracle(X, y, h, kind, prior_sd=1.7, noise_sd=1.3)
    assert o.dim == h * (p + 2) + 1
    theta = 0.5 * np.random.RandomState(p).randn(3, o.dim)
    g = o.grad(theta)
    assert g.shape == (3, o.dim)
    step = 1e-5
    for j in range(o.dim):
        e = np.zeros(o.dim)
        e[j] = step
        fd = (o.logp(theta + e) - o.logp(theta - e)) / (2 * step)
        assert np.max(np.abs(fd - g[:, j])) < 1e-7 * max(1.0, np.max(np.abs(g)))
    np.testing.assert_allclose(o.logp(theta) - o.log_prior(theta), o.pointwise(theta).sum(axis=1), rtol=1e-14)
    assert o.logp(theta[0]).shape == (1,) and o.grad(theta[0]).shape == (1, o.dim)


def test_oracle_structure_and_saturation():
    """v = 0: the hidden layer's entries see the prior only.  Huge pre-activations and outputs stay finite."""
    X, y = _data('logistic', 3, 12, seed=5)
    o = NeuralNetOracle(X, y, 4, 'logistic', prior_sd=2.0)
    theta = np.random.RandomState(1).randn(5, o.dim)
    theta[:, 16:20] = 0.0
    g = o.grad(theta)
    np.testing.assert_array_equal(g[:, :16], -theta[:, :16] / 4.0)
    big = np.random.RandomState(2).randn(5, o.dim)
    big[:, :16] *= 1e4
    big[:, 16:] *= 300.0
    assert np.all(np.isfinite(o.logp(big))) and np.all(np.isfinite(o.grad(big)))
    pr = o.predict(big, X_new=X[:4], y_new=y[:4])
    assert all(np.all(np.isfinite(pr[k])) for k in pr)
    bound = o.predict(theta)
    given = o.predict(theta, X_new=X, y_new=y)
    assert all(np.array_equal(bound[k], given[k]) for k in given)
