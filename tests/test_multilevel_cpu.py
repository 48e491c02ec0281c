"""CPU: MultilevelRegressionModel's host side (constructor validation, the sort by group, device_spec layout, unpack,
export) and the numpy oracle the GPU tests compare against (tests/_multilevel_oracle.py): its gradient and Hessian against
differences, and its per-observation terms against the flat GLM oracles on the design augmented by the group indicators."""
import numpy as np
import pytest

import viabel_amd as vb
from viabel_amd import _lib
from oracle import models as omod
from _multilevel_oracle import MultilevelOracle

LIKELIHOODS = ['logistic', 'poisson', 'gaussian']


def _data(likelihood, p, J, n_data, seed=0):
    rng = np.random.RandomState(seed)
    X = rng.randn(n_data, p) / np.sqrt(p)
    groups = rng.randint(0, J, size=n_data)
    if likelihood == 'logistic':
        y = rng.randint(0, 2, size=n_data).astype(float)
    elif likelihood == 'poisson':
        y = rng.poisson(2.0, size=n_data).astype(float)
    else:
        y = rng.randn(n_data)
    return X, y, groups


def test_exported_from_package_and_bound():
    assert vb.MultilevelRegressionModel is vb.models.MultilevelRegressionModel
    assert 'MultilevelRegressionModel' in vb.models.__all__
    assert _lib.MODEL_MULTILEVEL == 6 and _lib.MODEL_MULTILEVEL in _lib.MODELS_WITH_ROWS
    assert _lib.MULTILEVEL_CHUNK_DOUBLES > 0
    assert 'vb_multilevel_pointwise' in _lib.SIGNATURES


def test_header_declares_the_model_id_and_chunk_constant():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'viabel_hip.h')).read()
    assert re.search(r'#define\s+VB_MODEL_MULTILEVEL\s+6\b', header)
    common = open(os.path.join(root, 'viabel_amd', 'csrc', 'vb_common.h')).read()
    m = re.search(r'kMultilevelChunkDoubles\s*=\s*\(int64_t\)(\d+)\s*<<\s*(\d+)', common)
    assert m and int(m.group(1)) << int(m.group(2)) == _lib.MULTILEVEL_CHUNK_DOUBLES
    assert re.search(r'model_has_rows\(int id\)\s*\{[^}]*VB_MODEL_MULTILEVEL', common)


def test_sort_permutation_round_trips_and_spec_layout():
    X, y, groups = _data('poisson', 3, 4, 11, seed=3)
    groups[groups == 2] = 3                                       # group 2 stays empty
    m = vb.MultilevelRegressionModel(X, y, groups, 4, likelihood='poisson', prior_sd=2.5, tau_sd=0.7)
    assert m.dim == 3 + 4 + 1 and m.n_data == 11 and m.n_groups == 4 and m.n_features == 3
    assert sorted(m.perm) == list(range(11))
    np.testing.assert_array_equal(m.X, X[m.perm])
    np.testing.assert_array_equal(m.y, y[m.perm])
    np.testing.assert_array_equal(m.groups, groups[m.perm])
    assert np.all(np.diff(m.groups) >= 0)
    assert np.all(np.diff(m.perm)[np.diff(m.groups) == 0] > 0)    # stable: the caller's order inside a group
    back = np.empty_like(X)
    back[m.perm] = m.X
    np.testing.assert_array_equal(back, X)
    assert list(m.offsets) == [0] + list(np.cumsum(np.bincount(groups, minlength=4)))
    assert m.offsets[2] == m.offsets[3]                           # the empty group's run
    model_id, dim, dparams, iparams = m.device_spec()
    assert model_id == _lib.MODEL_MULTILEVEL and dim == 8
    assert dparams.dtype == np.float64 and dparams.shape == (11 * 3 + 11 + 3,)
    np.testing.assert_array_equal(dparams[:33].reshape(11, 3), m.X)
    np.testing.assert_array_equal(dparams[33:44], m.y)
    assert list(dparams[44:]) == [2.5, 0.7, 1.0]
    assert iparams.dtype == np.int64 and list(iparams[:3]) == [11, 4, _lib.GLM_POISSON]
    np.testing.assert_array_equal(iparams[3:8], m.offsets)
    np.testing.assert_array_equal(iparams[8:], m.groups)
    assert m.device_spec() is m.device_spec()                     # cached: the engine keys on identity
    m2 = vb.MultilevelRegressionModel(X, y, groups.astype(float), 4, likelihood='poisson', prior_sd=2.5, tau_sd=0.7)
    np.testing.assert_array_equal(m2.device_spec()[3], iparams)   # float labels with integral values
    d = vb.MultilevelRegressionModel(X, (y > 1).astype(float), groups, 4)
    assert (d.likelihood, d.prior_sd, d.tau_sd, d.noise_sd) == ('logistic', 10.0, 1.0, 1.0)


@pytest.mark.parametrize('kwargs', [
    dict(X=np.zeros(5)),                                          # X not 2-D
    dict(X=np.zeros((5, 0))),                                     # p = 0
    dict(y=np.zeros(4)),                                          # y of the wrong length
    dict(groups=np.zeros(4, dtype=int)),                          # groups of the wrong length
    dict(groups=np.array([0, 1, 2, 3, 1])),                       # label == n_groups
    dict(groups=np.array([0, -1, 2, 1, 1])),                      # negative label
    dict(groups=np.array([0.0, 1.5, 2.0, 1.0, 1.0])),             # non-integral
    dict(groups=np.array([0.0, np.nan, 2.0, 1.0, 1.0])),
    dict(groups=np.array(['a', 'b', 'c', 'a', 'b'])),             # not numbers
    dict(n_groups=0),
    dict(n_groups=-2),
    dict(n_groups=2.5),
    dict(prior_sd=0.0),
    dict(tau_sd=0.0),
    dict(tau_sd=-1.0),
    dict(noise_sd=0.0),
    dict(likelihood='probit'),
    dict(y=np.array([0.0, 1.0, 2.0, 1.0, 0.0])),                  # logistic: y outside {0, 1}
    dict(y=np.array([0.0, 1.0, -1.0, 1.0, 0.0]), likelihood='poisson'),
    dict(y=np.array([0.0, 1.0, np.inf, 1.0, 0.0]), likelihood='gaussian'),
])
def test_constructor_validation(kwargs):
    args = dict(X=np.ones((5, 2)), y=np.array([0.0, 1.0, 1.0, 1.0, 0.0]), groups=np.array([0, 1, 2, 1, 0]), n_groups=3)
    vb.MultilevelRegressionModel(**args)                          # the baseline is valid
    args.update(kwargs)
    with pytest.raises(ValueError):
        vb.MultilevelRegressionModel(**args)


def test_unpack():
    X, y, groups = _data('logistic', 2, 3, 9)
    m = vb.MultilevelRegressionModel(X, y, groups, 3)
    theta = np.random.RandomState(0).randn(4, m.dim)
    b, u, tau = m.unpack(theta)
    assert b.shape == (4, 2) and u.shape == (4, 3) and tau.shape == (4,)
    np.testing.assert_array_equal(b, theta[:, :2])
    np.testing.assert_array_equal(u, theta[:, 2:5])
    np.testing.assert_array_equal(tau, np.exp(theta[:, 5]))
    b1, u1, tau1 = m.unpack(theta[1])
    assert b1.shape == (2,) and u1.shape == (3,) and tau1.shape == ()
    np.testing.assert_array_equal(tau1 * u1, (tau[:, None] * u)[1])
    with pytest.raises(ValueError):
        m.unpack(np.zeros(m.dim + 1))


def test_not_a_logistic_subclass_so_loo_declines():
    X, y, groups = _data('logistic', 2, 3, 7)
    m = vb.MultilevelRegressionModel(X, y, groups, 3)
    assert not isinstance(m, vb.LogisticRegressionModel)
    with pytest.raises(NotImplementedError, match='psisloo'):
        vb.loo(model=m, approx=vb.MFGaussian(m.dim), var_param=np.zeros(2 * m.dim), n_samples=10)


@pytest.mark.parametrize('likelihood', LIKELIHOODS)
@pytest.mark.parametrize('p,J,n_data', [(1, 1, 1), (5, 3, 33), (2, 6, 20)])
def test_oracle_gradient_and_hessian_against_differences(likelihood, p, J, n_data):
    X, y, groups = _data(likelihood, p, J, n_data, seed=J)
    if J == 3:
        groups[groups == 1] = 2                                   # an empty group
    o = MultilevelOracle(X, y, groups, J, likelihood, prior_sd=1.7, tau_sd=0.8, noise_sd=1.3)
    rng = np.random.RandomState(p)
    theta = 0.3 * rng.randn(3, o.dim)
    g = o.grad(theta)
    h = 1e-5
    for j in range(o.dim):
        e = np.zeros(o.dim)
        e[j] = h
        fd = (o.logp(theta + e) - o.logp(theta - e)) / (2 * h)
        assert np.max(np.abs(fd - g[:, j])) < 1e-7 * max(1.0, np.max(np.abs(g)))
    if J == 3:
        np.testing.assert_array_equal(g[:, p + 1], -theta[:, p + 1])      # the empty group sees its prior only
    H = o.hessian(theta[0])
    assert np.allclose(H, H.T, rtol=0, atol=1e-13 * np.max(np.abs(H)))
    for j in range(o.dim):
        e = np.zeros(o.dim)
        e[j] = h
        fd = (o.grad(theta[0] + e)[0] - o.grad(theta[0] - e)[0]) / (2 * h)
        assert np.max(np.abs(fd - H[:, j])) < 1e-7 * max(1.0, np.max(np.abs(H)))
    v = rng.randn(2, o.dim)
    np.testing.assert_allclose(o.hvp(theta[0], v), v @ H, rtol=0, atol=1e-13 * np.max(np.abs(H)))


@pytest.mark.parametrize('likelihood', LIKELIHOODS)
def test_oracle_pointwise_is_the_flat_glm_on_the_augmented_design(likelihood):
    """[X | onehot(groups)] at beta = [b, tau u] has the same predictors; the flat oracles give log densities, so the term
    of observation i is the flat oracle on that one row minus its prior."""
    p, J, n_data, sd = 3, 4, 25, 3.0
    X, y, groups = _data(likelihood, p, J, n_data, seed=9)
    o = MultilevelOracle(X, y, groups, J, likelihood, prior_sd=sd, noise_sd=1.3)
    theta = 0.5 * np.random.RandomState(1).randn(6, o.dim)
    b, u, omega = o.split(theta)
    beta = np.concatenate([b, np.exp(omega)[:, None] * u], axis=1)
    Xa = np.concatenate([X, np.eye(J)[groups]], axis=1)
    np.testing.assert_allclose(o.eta(theta), beta @ Xa.T, rtol=0, atol=1e-14)
    prior = -0.5 * np.sum(beta ** 2, axis=1) / sd ** 2 - (p + J) * (np.log(sd) + 0.5 * np.log(2 * np.pi))
    pw = o.pointwise(theta)
    for i in range(n_data):
        if likelihood == 'logistic':
            flat = omod.Logistic(Xa[i:i + 1], y[i:i + 1], sd)
        elif likelihood == 'poisson':
            flat = omod.Poisson(Xa[i:i + 1], y[i:i + 1], sd)
        else:
            flat = omod.LinearRegression(Xa[i:i + 1], y[i:i + 1], sd, 1.3)
        np.testing.assert_allclose(pw[:, i], flat.logp(beta) - prior, rtol=0, atol=1e-12)
    np.testing.assert_allclose(o.logp(theta) - o.log_prior(theta), pw.sum(axis=1), rtol=1e-14)


def test_oracle_is_overflow_safe_and_has_an_extended_precision_twin():
    X, y, groups = _data('logistic', 2, 3, 9, seed=2)
    o = MultilevelOracle(X, y, groups, 3)
    theta = np.random.RandomState(0).randn(2, o.dim)
    theta[:, :5] *= 2000.0
    assert np.all(np.isfinite(o.logp(theta))) and np.all(np.isfinite(o.grad(theta)))
    ol = MultilevelOracle(X, y, groups, 3, dtype=np.longdouble)
    t = 0.3 * np.random.RandomState(1).randn(4, o.dim)
    assert ol.logp(t).dtype == np.longdouble and ol.grad(t).dtype == np.longdouble
    np.testing.assert_allclose(o.logp(t), ol.logp(t).astype(float), rtol=1e-14)
    np.testing.assert_allclose(o.grad(t), ol.grad(t).astype(float), rtol=0, atol=1e-13)
