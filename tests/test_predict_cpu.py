"""CPU: the plumbing of posterior prediction (the C entry is declared and bound, ``predict`` is exported, the Python-side
validation runs before the engine is touched) and the numpy oracle of tests/test_gpu_predict.py against the closed form
of Bayesian linear regression and scipy."""
import os
import re

import numpy as np
import pytest
from scipy import stats

import _predict_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_is_declared_and_bound():
    from viabel_amd import _lib
    assert 'vb_glm_predict' in _lib.SIGNATURES
    restype, argtypes = _lib.SIGNATURES['vb_glm_predict']
    assert len(argtypes) == 13 and argtypes[0] is _lib._ctx_p
    header = open(os.path.join(ROOT, 'include', 'viabel_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    decl = re.search(r'int\s+vb_glm_predict\s*\(([^)]*)\)', header)
    assert decl and len(decl.group(1).split(',')) == 13
    assert hasattr(_lib.Engine, 'glm_predict')


def test_predict_is_exported():
    import viabel_amd as vb
    from viabel_amd import convenience
    assert 'predict' in convenience.__all__ and callable(vb.predict)
    assert hasattr(vb.LogisticRegressionModel, 'predict_from_draws')
    assert vb.PoissonRegressionModel.predict_from_draws is vb.LogisticRegressionModel.predict_from_draws
    assert vb.LinearRegressionModel.predict_from_draws is vb.LogisticRegressionModel.predict_from_draws


def test_null_context_is_rejected():
    from viabel_amd import _lib
    lib = _lib.load()
    assert lib.vb_glm_predict(None, None, 0, 0, None, None, 0, None, None, None, None, None, None) == _lib.VB_ERR_INVALID


def _engine_must_not_be_touched(monkeypatch):
    from viabel_amd import _lib

    def boom(*a, **kw):
        raise AssertionError('the engine was touched before the arguments were validated')
    monkeypatch.setattr(_lib, 'default_engine', boom)


def test_validation_runs_before_the_engine(monkeypatch):
    import viabel_amd as vb
    _engine_must_not_be_touched(monkeypatch)
    rng = np.random.RandomState(0)
    X, y = rng.randn(20, 3), (rng.rand(20) < 0.5).astype(float)
    model = vb.LogisticRegressionModel(X, y)
    x = rng.randn(8, 3)
    for kw in (dict(X_new=np.zeros((4, 2))),                       # X_new has dim columns
               dict(X_new=np.zeros(3)),
               dict(X_new=np.zeros((0, 3))),
               dict(X_new=np.zeros((4, 3)), y_new=np.zeros(5)),    # y_new has one entry per row of X_new ...
               dict(y_new=np.zeros(19)),                           # ... or of the model's own design
               dict(log_weights=np.zeros(7)),
               dict(log_weights=np.full(8, -np.inf))):
        with pytest.raises(ValueError):
            model.predict_from_draws(x, **kw)
    with pytest.raises(ValueError):
        model.predict_from_draws(np.zeros((8, 4)))                 # the draws have dim columns
    counts = vb.PoissonRegressionModel(X, rng.poisson(1.0, 20).astype(float))
    with pytest.raises(ValueError):
        counts.predict_from_draws(x, X_new=np.zeros((2, 3)), y_new=np.array([1.0, -1.0]))
    with pytest.raises(ValueError):
        counts.predict_from_draws(x, y_new=-np.ones(20))
    with pytest.raises(AssertionError):                            # valid arguments do reach the engine
        model.predict_from_draws(x, X_new=np.zeros((4, 3)), y_new=np.zeros(4))


def test_predict_argument_rules(monkeypatch):
    import viabel_amd as vb
    _engine_must_not_be_touched(monkeypatch)
    rng = np.random.RandomState(1)
    X, y = rng.randn(20, 3), (rng.rand(20) < 0.5).astype(float)
    model, approx, theta = vb.LogisticRegressionModel(X, y), vb.MFGaussian(3), np.zeros(6)
    objective = vb.ExclusiveKL(approx, model, 8)
    for kw in (dict(), dict(model=model), dict(approx=approx), dict(objective=objective, model=model),
               dict(model=model, approx=approx, n_samples=0), dict(model=model, approx=approx, Reff=0.0),
               dict(model=model, approx=approx, weights='tis'), dict(model=model, approx=approx, weights='psis', n_samples=1)):
        with pytest.raises(ValueError):
            vb.predict(theta, **kw)
    others = [vb.GaussianModel(np.zeros(3), np.ones(3)),
              vb.SoftmaxRegressionModel(X, rng.randint(3, size=20), 3),
              vb.MultilevelRegressionModel(X, y, np.arange(20) % 4, 4),
              vb.LocationScaleRegressionModel(X, rng.randn(20))]
    for other in others:
        with pytest.raises(NotImplementedError) as info:
            vb.predict(np.zeros(2 * other.dim), model=other, approx=vb.MFGaussian(other.dim))
        assert 'predict_from_draws' in str(info.value) and 'pointwise_log_likelihood' in str(info.value)


# ---- the oracle ---------------------------------------------------------------------------------------------------------
def test_oracle_gaussian_terms_match_scipy():
    rng = np.random.RandomState(2)
    theta, X_new, y_new = rng.randn(50, 4), rng.randn(7, 4), rng.randn(7)
    lw = 0.8 * rng.standard_t(5.0, 50)
    lw[0] = -np.inf
    out = PO.predict_numpy('linear', theta, X_new, y_new, lw, noise_sd=0.7)
    w = np.exp(lw - np.logaddexp.reduce(lw))
    eta = X_new @ theta.T
    dens = stats.norm.pdf(y_new[:, None], loc=eta, scale=0.7)
    np.testing.assert_allclose(out['lpd'], np.log(dens @ w), rtol=0, atol=1e-13)
    np.testing.assert_allclose(out['eta_mean'], eta @ w, rtol=0, atol=1e-14)
    np.testing.assert_allclose(out['mean'], out['eta_mean'], rtol=0, atol=0)
    np.testing.assert_allclose(out['var'], out['eta_var'] + 0.49, rtol=1e-14, atol=0)
    np.testing.assert_allclose(out['eta_var'], ((eta - (eta @ w)[:, None]) ** 2) @ w, rtol=1e-13, atol=0)
    # the other two likelihoods against scipy's mass functions
    y01 = (rng.rand(7) < 0.5).astype(float)
    lo = PO.predict_numpy('logistic', theta, X_new, y01, lw)
    p = 1.0 / (1.0 + np.exp(-eta))
    np.testing.assert_allclose(lo['lpd'], np.log(stats.bernoulli.pmf(y01[:, None], p) @ w), rtol=0, atol=1e-13)
    np.testing.assert_allclose(lo['mean'], p @ w, rtol=0, atol=1e-14)
    np.testing.assert_allclose(lo['var'], (p * (1 - p)) @ w + ((p - (p @ w)[:, None]) ** 2) @ w, rtol=1e-12, atol=0)
    cnt = rng.poisson(1.0, 7).astype(float)
    po = PO.predict_numpy('poisson', 0.5 * theta, X_new, cnt, lw)
    mu = np.exp(0.5 * eta)
    np.testing.assert_allclose(po['lpd'], np.log(stats.poisson.pmf(cnt[:, None], mu) @ w), rtol=0, atol=1e-12)
    np.testing.assert_allclose(po['var'], mu @ w + ((mu - (mu @ w)[:, None]) ** 2) @ w, rtol=1e-12, atol=0)


def test_oracle_dtypes_agree_and_peaked_weights_pick_one_draw():
    rng = np.random.RandomState(3)
    theta, X_new = rng.randn(257, 17), rng.randn(33, 17) / np.sqrt(17)
    X_new[0] *= 40.0 / np.max(np.abs(theta @ X_new[0]))
    y = (rng.rand(33) < 0.5).astype(float)
    lw = 0.8 * rng.standard_t(5.0, 257)
    lw[0] = -np.inf
    a = PO.predict_numpy('logistic', theta, X_new, y, lw)
    b = PO.predict_numpy('logistic', theta, X_new, y, lw, dtype=np.longdouble)
    for k in a:
        assert np.max(np.abs(a[k] - b[k].astype(np.float64))) <= 1e-14 * np.max(np.abs(a[k])), k
    peaked = np.full(257, -800.0)
    peaked[100] = 0.0
    c = PO.predict_numpy('logistic', theta, X_new, y, peaked)
    one = PO.predict_numpy('logistic', theta[100], X_new, y)
    assert np.all(c['eta_var'] == 0.0)
    for k in ('eta_mean', 'mean', 'var', 'lpd'):      # (the matrix product's rounding depends on its shape: not bit for bit)
        np.testing.assert_allclose(c[k], one[k], rtol=1e-13, atol=1e-13 * np.max(np.abs(one[k])), err_msg=k)


def test_oracle_matches_the_linear_closed_form():
    """q = the exact posterior N(m, V): with S draws the Monte-Carlo error of the weighted sums shrinks like 1 / sqrt(S);
    32 768 exact draws put every output within 4 standard errors of the closed form."""
    X, y, prior_sd, noise_sd, _ = PO.linear_problem(1)
    pm, pV = PO.linear_posterior(X, y, prior_sd, noise_sd)
    X_new, y_new = PO.linear_holdout(33)
    exact = PO.linear_predict_closed_form(X_new, y_new, pm, pV, noise_sd)
    np.testing.assert_allclose(exact['lpd'], stats.norm.logpdf(y_new, X_new @ pm, np.sqrt(exact['var'])), rtol=0, atol=1e-13)
    S = 32768
    theta = pm + np.random.RandomState(5).randn(S, 8) @ np.linalg.cholesky(pV).T
    out = PO.predict_numpy('linear', theta, X_new, y_new, None, noise_sd)
    sd_eta = np.sqrt(exact['eta_var'])
    assert np.all(np.abs(out['eta_mean'] - exact['eta_mean']) <= 4 * sd_eta / np.sqrt(S))
    assert np.all(np.abs(out['eta_var'] - exact['eta_var']) <= 4 * exact['eta_var'] * np.sqrt(2.0 / S))
    assert np.all(np.abs(out['var'] - exact['var']) <= 4 * exact['eta_var'] * np.sqrt(2.0 / S))
    # the density of y_i at the draws is bounded by 1 / (sqrt(2 pi) noise_sd): its mean over S draws is within
    # 4 sd / sqrt(S) of the exact density, sd at most that bound
    bound = 4.0 / (np.sqrt(2.0 * np.pi) * noise_sd * np.sqrt(S))
    assert np.all(np.abs(np.exp(out['lpd']) - np.exp(exact['lpd'])) <= bound)


def test_moment_form_of_the_variance_fails_where_the_deviation_form_holds():
    """The narrow draws of tests/test_gpu_predict.py: against the longdouble oracle the float64 deviation form uses a tiny
    fraction of the tolerance derived from the linear predictors' own, E[eta^2] - E[eta]^2 exceeds it a thousandfold at the worst row."""
    for S in (257, 4097):
        rng = np.random.RandomState(S)
        theta0 = rng.randn(17)
        x = theta0 * (1.0 + 1e-7 * rng.randn(S, 17))
        X_new = rng.randn(33, 17) / np.sqrt(17)
        ref = PO.predict_numpy('linear', x, X_new, dtype=np.longdouble)['eta_var'].astype(np.float64)
        delta = 1e-12 * float(np.max(np.abs(X_new @ x.T)))
        tol = 2.0 * delta * np.sqrt(ref) + delta ** 2 + 1e-12 * ref
        dev = np.abs(PO.predict_numpy('linear', x, X_new)['eta_var'] - ref)
        mom = np.abs(PO.eta_var_moment_form(x, X_new) - ref)
        assert np.max(dev / tol) < 1e-2, (S, np.max(dev / tol))
        print('S %d: deviation form %.3g, moment form max %.3g median %.3g of the tolerance'
              % (S, np.max(dev / tol), np.max(mom / tol), np.median(mom / tol)))
        assert np.max(mom / tol) > 1e3 and np.median(mom / tol) > 10, (S, np.max(mom / tol), np.median(mom / tol))
