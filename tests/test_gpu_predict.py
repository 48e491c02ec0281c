"""GPU: posterior prediction on the device -- vb_glm_predict (csrc/vb_psis_batch.hip: one fp64 MFMA product and the
reduction kernel glm_predict_kernel) through Engine.glm_predict, predict_from_draws and viabel_amd.predict -- against numpy
(tests/_predict_oracle.py), the LOO entry's lpd and a closed form.

Tolerances are the project's own for the same quantities (tests/test_gpu_loo.py): 1e-12 * max|ref| per output vector for
model values and between two device kernels, 1e-9 where the smoothed weights come from the device.
"""
import numpy as np
import pytest

import _predict_oracle as PO
from oracle import psis as opsis

pytestmark = pytest.mark.gpu

KEYS = ('eta_mean', 'eta_var', 'mean', 'var', 'lpd')


@pytest.fixture(scope='module')
def vb():
    import viabel_amd
    from viabel_amd import _lib
    _lib.default_engine()
    return viabel_amd


def _glm(vb, kind, X, y):
    if kind == 'logistic':
        return vb.LogisticRegressionModel(X, y, prior_sd=3.0)
    if kind == 'poisson':
        return vb.PoissonRegressionModel(X, y, prior_sd=3.0)
    return vb.LinearRegressionModel(X, y, prior_sd=3.0, noise_sd=0.7)


def _response(kind, rng, eta):
    if kind == 'logistic':
        return (rng.rand(eta.size) < 0.5).astype(float)
    if kind == 'poisson':
        return rng.poisson(np.exp(eta)).astype(float)
    return eta + 0.7 * rng.randn(eta.size)


def _problem(kind, D, m, S, seed):
    """X_new = randn / sqrt(D), draws randn (x 0.7 for Poisson); logistic: row 0 scaled so that |eta| reaches 40."""
    rng = np.random.RandomState(seed)
    X_new = rng.randn(m, D) / np.sqrt(D)
    x = rng.randn(S, D) * (0.7 if kind == 'poisson' else 1.0)
    if kind == 'logistic':
        X_new[0] *= 40.0 / np.max(np.abs(x @ X_new[0]))
    y_new = _response(kind, rng, X_new @ x[0])
    return X_new, y_new, x


def _log_weights(which, S, rng):
    if which == 'none':
        return None
    if which == 't':
        lw = 0.8 * rng.standard_t(5.0, S)
        if S > 1:                       # (at S = 1 the -inf entry would leave no finite weight: test_errors has that case)
            lw[0] = -np.inf
        return lw
    assert which == 'peaked'
    lw = np.full(S, -800.0)
    lw[rng.randint(S)] = 0.0
    return lw


def _assert_close(out, ref, what, rel=1e-12, keys=KEYS):
    for k in keys:
        tol = rel * np.max(np.abs(ref[k]))
        err = np.max(np.abs(out[k] - ref[k]))
        assert err <= tol, (what, k, err, tol)


# ---- 1. the grid against the float64 oracle ----------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['logistic', 'poisson', 'linear'])
def test_grid_against_oracle(vb, kind):
    """Every (D, m, S, weights) against numpy at 1e-12 * max|ref| per output vector; every call twice, bit for bit; S = 1
    and the peaked weights (one draw carries everything: exp(-800) is 0) give both "between" variances exactly 0 and that
    draw's own values."""
    worst = dict.fromkeys(KEYS, 0.0)
    for D in (1, 17, 64):
        # one bound model per D: the prediction takes dim, link and noise_sd from it, never its data
        rb = np.random.RandomState(D)
        Xb = rb.randn(5, D)
        model = _glm(vb, kind, Xb, _response(kind, rb, np.zeros(5)))
        for m in (1, 33, 300):
            for S in (1, 2, 255, 256, 257, 777, 4097):
                X_new, y_new, x = _problem(kind, D, m, S, seed=100000 * D + 1000 * m + S)
                for which in ('none', 't', 'peaked'):
                    lw = _log_weights(which, S, np.random.RandomState(S + len(which)))
                    what = (kind, D, m, S, which)
                    out = model.predict_from_draws(x, X_new=X_new, y_new=y_new, log_weights=lw)
                    again = model.predict_from_draws(x, X_new=X_new, y_new=y_new, log_weights=lw)
                    ref = PO.predict_numpy(kind, x, X_new, y_new, lw, noise_sd=0.7)
                    for k in KEYS:
                        assert out[k].shape == (m,) and np.array_equal(out[k], again[k]), (what, k)
                        scale = np.max(np.abs(ref[k]))
                        if scale > 0:
                            worst[k] = max(worst[k], np.max(np.abs(out[k] - ref[k])) / scale)
                    _assert_close(out, ref, what)
                    if S == 1 or which == 'peaked':
                        one = PO.predict_numpy(kind, x[0 if S == 1 else int(np.argmax(lw))], X_new, y_new, None, noise_sd=0.7)
                        assert np.all(out['eta_var'] == 0.0), what
                        np.testing.assert_allclose(out['var'], one['var'], rtol=1e-12, atol=0, err_msg=str(what))
                        # (lpd keeps the other draws' terms at log weight -800: a draw that explains y_i e^800 times
                        # better -- Poisson counts far from this draw's mean -- still shows; the oracle above has them)
                        _assert_close(out, one, what, keys=('eta_mean', 'mean') + (('lpd',) if S == 1 else ()))
                    no_y = model.predict_from_draws(x, X_new=X_new, log_weights=lw)
                    assert 'lpd' not in no_y and all(np.array_equal(no_y[k], out[k]) for k in KEYS[:4]), what
    print('%s: largest error / max|ref| per output: %s' % (kind, ', '.join('%s %.3g' % kv for kv in worst.items())))


# ---- 2. narrow draws: the variance is a sum of squared deviations ---------------------------------------------------------
@pytest.mark.parametrize('S', [257, 4097])
def test_narrow_draws(vb, S):
    """theta_s = theta0 * (1 + 1e-7 randn): eta varies in its 7th digit.  Reference: the longdouble oracle.  An error of
    delta = 1e-12 max|eta| in every linear predictor (the tolerance of the product) moves the variance by at most
    2 delta sqrt(var) + delta^2; E[eta^2] - E[eta]^2 in float64 misses that by up to three orders of magnitude
    (tests/test_predict_cpu.py)."""
    D, m = 17, 33
    rng = np.random.RandomState(S)
    theta0 = rng.randn(D)
    x = theta0 * (1.0 + 1e-7 * rng.randn(S, D))
    X_new = rng.randn(m, D) / np.sqrt(D)
    model = _glm(vb, 'linear', rng.randn(5, D), rng.randn(5))
    for which in ('none', 't'):
        lw = _log_weights(which, S, np.random.RandomState(S + 1))
        out = model.predict_from_draws(x, X_new=X_new, log_weights=lw)
        ref = PO.predict_numpy('linear', x, X_new, None, lw, noise_sd=0.7, dtype=np.longdouble)
        eta_max = float(np.max(np.abs(X_new.astype(np.longdouble) @ x.astype(np.longdouble).T)))
        delta = 1e-12 * eta_max
        rv = ref['eta_var'].astype(np.float64)
        tol = 2.0 * delta * np.sqrt(rv) + delta ** 2 + 1e-12 * rv
        err = np.abs(out['eta_var'] - rv)
        print('S %d weights %s: largest |eta_var - ref| / tolerance %.3g (eta_var about %.3g)'
              % (S, which, np.max(err / tol), np.median(rv)))
        assert np.all(err <= tol), (S, which, np.max(err / tol))


# ---- 3. the bound design -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['logistic', 'poisson', 'linear'])
def test_bound_design(vb, kind):
    from viabel_amd import _lib
    D, n, S = 17, 300, 777
    rng = np.random.RandomState(31)
    X = rng.randn(n, D) / np.sqrt(D)
    x = 0.5 * rng.randn(S, D)
    model = _glm(vb, kind, X, _response(kind, rng, X @ x[0]))
    log_w, _ = opsis.psis_smooth(0.8 * rng.standard_t(5.0, S))
    bound = model.predict_from_draws(x, log_weights=log_w)
    given = model.predict_from_draws(x, X_new=model.X, y_new=model.y, log_weights=log_w)
    for k in KEYS:
        assert np.array_equal(bound[k], given[k]), k
    _assert_close(bound, PO.predict_numpy(kind, x, X, model.y, log_w, noise_sd=0.7), kind)
    eng = _lib.default_engine()
    eng.set_model(model.device_spec())
    lpd_loo = eng.glm_psis_loo(x, n, log_ratios=log_w, log_w=log_w)[2]
    err = np.max(np.abs(bound['lpd'] - lpd_loo))
    print('%s: max |lpd - lpd of glm_psis_loo| %.3g (max |ref| %.3g)' % (kind, err, np.max(np.abs(lpd_loo))))
    assert err <= 1e-12 * np.max(np.abs(lpd_loo))
    other_y = _response(kind, rng, X @ x[1])                       # the bound design with other responses
    mixed = model.predict_from_draws(x, y_new=other_y, log_weights=log_w)
    _assert_close(mixed, PO.predict_numpy(kind, x, X, other_y, log_w, noise_sd=0.7), kind)


# ---- 4. chunks of observations --------------------------------------------------------------------------------------------------
def test_chunks_of_observations(vb):
    """More than 1 GiB of linear predictors (8200 observations x 16 384 draws: 8192 observations fit the device budget,
    eight are left for a second pass), with an uploaded design and with the bound one: the observations on both sides of
    the boundary, the first and the last against numpy; everything finite."""
    S, D, m = 16384, 4, 8200
    rng = np.random.RandomState(21)
    X = rng.randn(m, D) / np.sqrt(D)
    y = (rng.rand(m) < 0.5).astype(float)
    x = 0.3 * rng.randn(S, D)
    log_w, _ = opsis.psis_smooth(0.5 * rng.standard_t(6.0, S))
    small = vb.LogisticRegressionModel(X[:5], y[:5], prior_sd=10.0)
    out = small.predict_from_draws(x, X_new=X, y_new=y, log_weights=log_w)
    pick = np.array([0, 1, 8190, 8191, 8192, 8193, 8199])
    ref = PO.predict_numpy('logistic', x, X[pick], y[pick], log_w)
    _assert_close({k: out[k][pick] for k in KEYS}, ref, 'uploaded design')
    assert all(np.all(np.isfinite(out[k])) for k in KEYS)
    bound = vb.LogisticRegressionModel(X, y, prior_sd=10.0).predict_from_draws(x, log_weights=log_w)
    for k in KEYS:
        assert np.array_equal(bound[k], out[k]), k


# ---- 5. against a closed form ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('weights', [None, 'psis'])
def test_predict_against_closed_form(vb, weights, capsys):
    """Linear model, q = the exact Gaussian posterior, 33 new rows.  The Monte-Carlo tolerance is the numpy pipeline's own
    largest error against the closed form on the same draws plus the tolerance between device and numpy (triangle
    inequality): 1e-12 * max|ref| when the draws are taken as they are, 1e-9 when the smoothed weights come from the
    device.  No row is masked."""
    X, y, prior_sd, noise_sd, _ = PO.linear_problem(1)
    pm, pV = PO.linear_posterior(X, y, prior_sd, noise_sd)
    X_new, y_new = PO.linear_holdout(33)
    exact = PO.linear_predict_closed_form(X_new, y_new, pm, pV, noise_sd)
    model = vb.LinearRegressionModel(X, y, prior_sd=prior_sd, noise_sd=noise_sd)
    theta = vb.FullRankGaussian(8).pack(pm, np.linalg.cholesky(pV))
    res = vb.predict(theta, model=model, approx=vb.FullRankGaussian(8), X_new=X_new, y_new=y_new, n_samples=4096,
                     weights=weights)
    capsys.readouterr()
    samples, log_ratios = vb.samples_and_log_weights(theta, model, vb.FullRankGaussian(8), 4096)
    ref, khat = PO.predict_pipeline_numpy('linear', samples, log_ratios, X_new, y_new, weights, noise_sd=noise_sd)
    dev = dict(eta_mean=res['eta_mean'], eta_var=res['eta_sd'] ** 2, mean=res['mean'], var=res['sd'] ** 2, lpd=res['lpd'])
    for k in KEYS:
        between = 1e-12 * np.max(np.abs(ref[k])) if weights is None else 1e-9
        e_np, e_dev = np.max(np.abs(ref[k] - exact[k])), np.max(np.abs(dev[k] - exact[k]))
        print('%s weights %s: numpy %.3g device %.3g from the closed form; device - numpy %.3g'
              % (k, weights, e_np, e_dev, np.max(np.abs(dev[k] - ref[k]))))
        assert np.max(np.abs(dev[k] - ref[k])) <= between, k
        assert e_dev <= e_np + between, k
    assert abs(res['elpd'] - exact['lpd'].sum()) <= abs(ref['lpd'].sum() - exact['lpd'].sum()) + 33e-9
    if weights == 'psis':
        assert res['khat'] < 0.7 and abs(res['khat'] - khat) <= 1e-10 * max(1.0, abs(khat))
    else:
        assert res['khat'] is None


# ---- 6. end to end after a device fit -------------------------------------------------------------------------------------------
def test_predict_end_to_end_after_a_device_fit(vb, capsys):
    from viabel_amd.optimization import Adam
    D, n = 10, 300
    rng = np.random.RandomState(4)
    X = rng.randn(n, D) / np.sqrt(D)
    beta = 2.0 * rng.randn(D)
    y = (rng.rand(n) < 1.0 / (1.0 + np.exp(-X @ beta))).astype(float)
    model = vb.LogisticRegressionModel(X, y, prior_sd=10.0)
    X_new = rng.randn(50, D) / np.sqrt(D)
    y_new = (rng.rand(50) < 1.0 / (1.0 + np.exp(-X_new @ beta))).astype(float)
    objective = vb.ExclusiveKL(vb.MFGaussian(D, seed=3, rng='philox'), model, 64)
    init = np.concatenate([np.zeros(D), np.full(D, -1.0)])
    theta = Adam(0.05, iterate_avg_prop=None).optimize(400, objective, init, on_device=True)['opt_param']
    capsys.readouterr()
    for weights in ('psis', None):
        res = vb.predict(theta, model=model, approx=vb.MFGaussian(D, seed=5), X_new=X_new, y_new=y_new, n_samples=4096,
                         weights=weights)
        printed = capsys.readouterr().out
        assert 'elpd = ' in printed and ('khat' in printed) == (weights == 'psis')
        samples, log_ratios = vb.samples_and_log_weights(theta, model, vb.MFGaussian(D, seed=5), 4096)
        ref, khat = PO.predict_pipeline_numpy('logistic', samples, log_ratios, X_new, y_new, weights)
        dev = dict(eta_mean=res['eta_mean'], eta_var=res['eta_sd'] ** 2, mean=res['mean'], var=res['sd'] ** 2, lpd=res['lpd'])
        print('weights %s: device - numpy %s' % (weights, ', '.join('%s %.3g' % (k, np.max(np.abs(dev[k] - ref[k]))) for k in KEYS)))
        for k in KEYS:
            np.testing.assert_allclose(dev[k], ref[k], rtol=0, atol=1e-9, err_msg=k)
        assert abs(res['elpd'] - ref['lpd'].sum()) <= 50e-9
        assert abs(res['se_elpd'] - np.sqrt(50 * np.var(ref['lpd']))) <= 50e-9
        assert res['n_samples'] == 4096 and np.all(res['sd'] > 0) and np.all((res['mean'] > 0) & (res['mean'] < 1))
        res_o = vb.predict(theta, objective=vb.ExclusiveKL(vb.MFGaussian(D, seed=5), model, 8), X_new=X_new, y_new=y_new,
                           n_samples=4096, weights=weights)
        capsys.readouterr()
        for k in ('mean', 'sd', 'eta_mean', 'eta_sd', 'lpd'):
            assert np.array_equal(res_o[k], res[k]), k
    no_y = vb.predict(theta, model=model, approx=vb.MFGaussian(D, seed=5), X_new=X_new, n_samples=4096)
    assert 'lpd' not in no_y and 'elpd' not in no_y and 'no response' in capsys.readouterr().out


# ---- 7. one engine, several shapes ----------------------------------------------------------------------------------------------
def test_small_call_after_a_large_one(vb):
    from viabel_amd import _lib
    Xl, yl, xl = _problem('logistic', 64, 300, 4097, seed=1)
    Xs, ys, xs = _problem('logistic', 1, 1, 2, seed=2)
    big = vb.LogisticRegressionModel(Xl[:5], yl[:5], prior_sd=3.0)
    small = vb.LogisticRegressionModel(Xs, ys, prior_sd=3.0)
    lws = np.array([-0.3, 0.4])
    big.predict_from_draws(xl, X_new=Xl, y_new=yl)
    after = small.predict_from_draws(xs, X_new=Xs, y_new=ys, log_weights=lws)
    fresh = _lib.Engine()
    try:
        fresh.set_model(small.device_spec())
        first = fresh.glm_predict(xs, log_w=lws, X_new=Xs, y_new=ys)
    finally:
        fresh.close()
    for k in KEYS:
        assert np.array_equal(after[k], first[k]), k
    _assert_close(after, PO.predict_numpy('logistic', xs, Xs, ys, lws), 'small after large')


# ---- 8. errors ------------------------------------------------------------------------------------------------------------------------
def test_errors(vb):
    from viabel_amd import _lib
    fresh = _lib.Engine()
    try:
        with pytest.raises(_lib.EngineError):                               # no model bound
            fresh.glm_predict(np.zeros((4, 3)), X_new=np.zeros((2, 3)))
        with pytest.raises(_lib.EngineError):
            fresh.glm_predict(np.zeros((4, 3)))
        fresh.set_model(vb.GaussianModel(np.zeros(3), np.ones(3)).device_spec())
        with pytest.raises(NotImplementedError):                            # bound, but not a regression target
            fresh.glm_predict(np.zeros((4, 3)), X_new=np.zeros((2, 3)))
        with pytest.raises(NotImplementedError):
            fresh.glm_predict(np.zeros((4, 3)))
    finally:
        fresh.close()
    rng = np.random.RandomState(4)
    X = rng.randn(30, 10)
    model = vb.LogisticRegressionModel(X, (rng.rand(30) < 0.5).astype(float))
    eng = _lib.default_engine()
    eng.set_model(model.device_spec())
    x = np.zeros((8, 10))
    for call in (lambda: eng.glm_predict(np.zeros((8, 9))),                                  # columns of x (the C entry)
                 lambda: eng.glm_predict(x, X_new=np.zeros((4, 9))),                         # columns of X_new
                 lambda: eng.glm_predict(x, log_w=np.zeros(7)),                              # length of log_w
                 lambda: eng.glm_predict(x, X_new=np.zeros((4, 10)), y_new=np.zeros(5)),     # length of y_new
                 lambda: eng.glm_predict(x, y_new=np.zeros(29)),                             # ... against the bound design
                 lambda: eng.glm_predict(x, log_w=np.full(8, -np.inf)),                      # no finite weight
                 lambda: model.predict_from_draws(np.zeros((8, 9))),
                 lambda: model.predict_from_draws(x, X_new=np.zeros((4, 9))),
                 lambda: model.predict_from_draws(x, y_new=np.zeros(29)),
                 lambda: model.predict_from_draws(x, log_weights=np.full(8, -np.inf))):
        with pytest.raises(ValueError):
            call()
    # the C entry's own checks, behind the Python ones
    import ctypes
    p = lambda a: ctypes.cast(a.ctypes.data, ctypes.POINTER(ctypes.c_double))                # noqa: E731
    o = [np.zeros(30) for _ in range(5)]
    xs, Xn, yn, inf = np.zeros((8, 10)), np.zeros((4, 10)), np.zeros(4), np.full(8, -np.inf)
    lib, ctx = eng._lib, eng._ctx
    assert lib.vb_glm_predict(ctx, p(xs), 8, 10, None, p(Xn), 4, p(yn), p(o[0]), p(o[1]), p(o[2]), p(o[3]), None) == _lib.VB_ERR_INVALID
    assert lib.vb_glm_predict(ctx, p(xs), 8, 10, None, p(Xn), 4, None, p(o[0]), p(o[1]), p(o[2]), p(o[3]), p(o[4])) == _lib.VB_ERR_INVALID
    assert lib.vb_glm_predict(ctx, p(xs), 8, 10, None, None, 29, None, p(o[0]), p(o[1]), p(o[2]), p(o[3]), p(o[4])) == _lib.VB_ERR_INVALID
    assert lib.vb_glm_predict(ctx, p(xs), 8, 10, None, p(Xn), 0, None, p(o[0]), p(o[1]), p(o[2]), p(o[3]), None) == _lib.VB_ERR_INVALID
    assert lib.vb_glm_predict(ctx, p(xs), 0, 10, None, p(Xn), 4, None, p(o[0]), p(o[1]), p(o[2]), p(o[3]), None) == _lib.VB_ERR_INVALID
    assert lib.vb_glm_predict(ctx, p(xs), 8, 10, p(inf), p(Xn), 4, None, p(o[0]), p(o[1]), p(o[2]), p(o[3]), None) == _lib.VB_ERR_INVALID
    assert lib.vb_glm_predict(ctx, p(xs), 8, 10, None, p(Xn), 4, None, p(o[0]), p(o[1]), p(o[2]), p(o[3]), None) == _lib.VB_OK
    theta = np.zeros(12)
    y01 = (rng.rand(30) < 0.5).astype(float)
    for other in (vb.SoftmaxRegressionModel(X[:, :2], rng.randint(3, size=30), 3),
                  vb.MultilevelRegressionModel(X[:, :2], y01, np.arange(30) % 3, 3),
                  vb.LocationScaleRegressionModel(X[:, :2], rng.randn(30)),
                  vb.GaussianModel(np.zeros(6), np.ones(6))):
        with pytest.raises(NotImplementedError) as info:
            vb.predict(theta, model=other, approx=vb.MFGaussian(other.dim))
        assert 'predict_from_draws' in str(info.value) and 'pointwise_log_likelihood' in str(info.value)
