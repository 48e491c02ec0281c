"""CPU: SoftmaxRegressionModel's host side (constructor validation, device_spec layout, export) and the numpy oracle the
GPU tests compare against (tests/_softmax_oracle.py): its gradient and Hessian against differences, and its C = 2 case
against the logistic oracle."""
import numpy as np
import pytest

import viabel_amd as vb
from viabel_amd import _lib
from oracle import models as omod
from _softmax_oracle import SoftmaxOracle


def _data(C, p, n_data, seed=0):
    rng = np.random.RandomState(seed)
    X = rng.randn(n_data, p) / np.sqrt(p)
    y = rng.randint(0, C, size=n_data)
    return X, y


def test_exported_from_package():
    assert vb.SoftmaxRegressionModel is vb.models.SoftmaxRegressionModel
    assert 'SoftmaxRegressionModel' in vb.models.__all__
    assert _lib.MODEL_SOFTMAX == 5 and _lib.MODEL_SOFTMAX in _lib.MODELS_WITH_ROWS
    assert _lib.SOFTMAX_CHUNK_DOUBLES > 0
    assert 'vb_softmax_pointwise' in _lib.SIGNATURES


def test_header_declares_the_model_id_and_chunk_constant():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'viabel_hip.h')).read()
    assert re.search(r'#define\s+VB_MODEL_SOFTMAX\s+5\b', header)
    common = open(os.path.join(root, 'viabel_amd', 'csrc', 'vb_common.h')).read()
    m = re.search(r'kSoftmaxChunkDoubles\s*=\s*\(int64_t\)(\d+)\s*<<\s*(\d+)', common)
    assert m and int(m.group(1)) << int(m.group(2)) == _lib.SOFTMAX_CHUNK_DOUBLES


def test_device_spec_layout_and_dim():
    X, y = _data(4, 3, 11)
    m = vb.SoftmaxRegressionModel(X, y, 4, prior_sd=2.5)
    assert m.dim == 12 and m.n_data == 11 and m.n_classes == 4
    model_id, dim, dparams, iparams = m.device_spec()
    assert model_id == _lib.MODEL_SOFTMAX and dim == 12
    assert dparams.dtype == np.float64 and dparams.shape == (11 * 3 + 11 + 1,)
    np.testing.assert_array_equal(dparams[:33].reshape(11, 3), X)
    np.testing.assert_array_equal(dparams[33:44], y.astype(float))
    assert dparams[44] == 2.5
    assert iparams.dtype == np.int64 and list(iparams) == [11, 4]
    assert m.device_spec() is m.device_spec()                 # cached: the engine keys on identity
    # float labels with integral values are accepted and give the same spec
    m2 = vb.SoftmaxRegressionModel(X, y.astype(float), 4, prior_sd=2.5)
    np.testing.assert_array_equal(m2.device_spec()[2], dparams)
    assert vb.SoftmaxRegressionModel(X, y, 4).prior_sd == 10.0


@pytest.mark.parametrize('kwargs', [
    dict(X=np.zeros(5)),                                      # X not 2-D
    dict(y=np.zeros(4, dtype=int)),                           # y of the wrong length
    dict(y=np.zeros((5, 1), dtype=int)),                      # y not 1-D
    dict(y=np.array([0, 1, 2, 3, 1])),                        # label == n_classes
    dict(y=np.array([0, -1, 2, 1, 1])),                       # negative label
    dict(y=np.array([0.0, 1.5, 2.0, 1.0, 1.0])),              # non-integral
    dict(y=np.array([0.0, np.nan, 2.0, 1.0, 1.0])),
    dict(y=np.array(['a', 'b', 'c', 'a', 'b'])),              # not numbers
    dict(n_classes=1),
    dict(n_classes=0),
    dict(n_classes=2.5),
    dict(prior_sd=0.0),
    dict(prior_sd=-1.0),
])
def test_constructor_validation(kwargs):
    args = dict(X=np.ones((5, 2)), y=np.array([0, 1, 2, 1, 0]), n_classes=3, prior_sd=1.0)
    vb.SoftmaxRegressionModel(**args)                         # the baseline is valid
    args.update(kwargs)
    with pytest.raises(ValueError):
        vb.SoftmaxRegressionModel(**args)


def test_not_a_logistic_subclass_so_loo_declines():
    X, y = _data(3, 2, 7)
    m = vb.SoftmaxRegressionModel(X, y, 3)
    assert not isinstance(m, vb.LogisticRegressionModel)
    with pytest.raises(NotImplementedError, match='psisloo'):
        vb.loo(model=m, approx=vb.MFGaussian(m.dim), var_param=np.zeros(2 * m.dim), n_samples=10)


@pytest.mark.parametrize('C,p,n_data', [(2, 1, 1), (3, 5, 33), (7, 4, 20)])
def test_oracle_gradient_and_hessian_against_differences(C, p, n_data):
    X, y = _data(C, p, n_data, seed=C)
    o = SoftmaxOracle(X, y, C, prior_sd=1.7)
    rng = np.random.RandomState(p)
    theta = 0.3 * rng.randn(3, o.dim)
    g = o.grad(theta)
    h = 1e-5
    for j in range(o.dim):
        e = np.zeros(o.dim)
        e[j] = h
        fd = (o.logp(theta + e) - o.logp(theta - e)) / (2 * h)
        assert np.max(np.abs(fd - g[:, j])) < 1e-7 * max(1.0, np.max(np.abs(g)))
    H = o.hessian(theta[0])
    assert np.allclose(H, H.T, rtol=0, atol=1e-13 * np.max(np.abs(H)))
    for j in range(o.dim):
        e = np.zeros(o.dim)
        e[j] = h
        fd = (o.grad(theta[0] + e)[0] - o.grad(theta[0] - e)[0]) / (2 * h)
        assert np.max(np.abs(fd - H[:, j])) < 1e-7 * max(1.0, np.max(np.abs(H)))
    v = rng.randn(2, o.dim)
    np.testing.assert_allclose(o.hvp(theta[0], v), v @ H, rtol=0, atol=1e-13 * np.max(np.abs(H)))


def test_oracle_two_classes_is_the_logistic_likelihood():
    p, n_data = 4, 50
    X, y = _data(2, p, n_data, seed=9)
    sd = 3.0
    o = SoftmaxOracle(X, y, 2, prior_sd=sd)
    lo = omod.Logistic(X, y.astype(float), prior_sd=sd)
    rng = np.random.RandomState(1)
    theta = 0.5 * rng.randn(6, 2 * p)
    beta = theta[:, p:] - theta[:, :p]
    # likelihood = log density minus the (different) priors
    prior_soft = -0.5 * np.sum(theta ** 2, axis=1) / sd ** 2 - 2 * p * (np.log(sd) + 0.5 * np.log(2 * np.pi))
    prior_log = -0.5 * np.sum(beta ** 2, axis=1) / sd ** 2 - p * (np.log(sd) + 0.5 * np.log(2 * np.pi))
    np.testing.assert_allclose(o.logp(theta) - prior_soft, lo.logp(beta) - prior_log, rtol=1e-13, atol=1e-12)
    eta = beta @ X.T
    np.testing.assert_allclose(o.pointwise(theta), y * eta - np.logaddexp(0.0, eta), rtol=0, atol=1e-13)


def test_oracle_is_overflow_safe():
    X, y = _data(3, 2, 9, seed=2)
    o = SoftmaxOracle(X, y, 3)
    theta = 2000.0 * np.random.RandomState(0).randn(2, 6)
    assert np.all(np.isfinite(o.logp(theta))) and np.all(np.isfinite(o.grad(theta)))
