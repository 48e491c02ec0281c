"""GPU: PSIS-LOO on the device -- pointwise GLM log-likelihoods (vb_glm_pointwise), the batched smoothing kernel
(csrc/vb_psis_batch.hip through vb_psis_smooth_batch / psislw / psisloo) and viabel_amd.loo (vb_glm_psis_loo) -- against
numpy (oracle/psis.py, tests/_loo_oracle.py), the single-vector device route and a closed form.

Tolerances are the project's own for the same quantities: smoothed log weights 1e-10 absolute and k-hat 1e-10 relative
against the oracle, 1e-12 between two device kernels (tests/test_gpu_psis.py); 1e-9 where the weights themselves come
from the device (test_device_log_weights_and_psis); 1e-12 * max|ref| for model values (test_model_call_dense_targets).
"""
import numpy as np
import pytest

import _loo_oracle as LO
from oracle import psis as opsis

pytestmark = pytest.mark.gpu

KINDS = ['student', 'clustered', 'ties', 'light', 'equal', 'minus_inf', 'narrow', 'two_values']
REFFS = [0.3, 1.0, 2.5]


@pytest.fixture(scope='module')
def vb():
    import viabel_amd
    from viabel_amd import _lib
    _lib.default_engine()
    return viabel_amd


def _weights(kind, m, n, seed):
    """``(n, m)``: m weight vectors of one kind (test_grid_kernel_equals_single_workgroup_kernel's and
    test_grid_kernel_degenerate_inputs' generators)."""
    rng = np.random.RandomState(seed)
    shape = (n, m)
    if kind == 'student':
        return 2.0 * rng.standard_t(3.0, shape)
    if kind == 'clustered':
        return -50.0 + 0.3 * rng.randn(*shape)
    if kind == 'ties':
        return np.round(1.5 * rng.standard_t(4.0, shape), 1)
    if kind == 'light':
        return -0.5 * rng.randn(*shape) ** 2
    if kind == 'equal':
        return np.full(shape, -3.25)
    if kind == 'minus_inf':
        return np.where(rng.rand(*shape) < 0.3, -np.inf, rng.randn(*shape))
    if kind == 'narrow':
        return -10.0 + 1e-9 * rng.rand(*shape)
    assert kind == 'two_values'
    return np.where(rng.rand(*shape) < 0.01, 0.5, -0.5)


def _assert_column(sm, k, ref, rk, atol, what):
    assert LO.close_k(k, rk), (what, k, rk)
    fin = np.isfinite(ref)
    assert np.array_equal(fin, np.isfinite(sm)), what
    np.testing.assert_allclose(sm[fin], ref[fin], rtol=0, atol=atol, err_msg=str(what))
    assert np.array_equal(sm[~fin], ref[~fin], equal_nan=True), what


def _glm(vb, kind, X, y):
    if kind == 'logistic':
        return vb.LogisticRegressionModel(X, y, prior_sd=3.0)
    if kind == 'poisson':
        return vb.PoissonRegressionModel(X, y, prior_sd=3.0)
    return vb.LinearRegressionModel(X, y, prior_sd=3.0, noise_sd=0.7)


# ---- 1. pointwise likelihoods -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['logistic', 'poisson', 'linear'])
def test_pointwise_log_likelihood(vb, kind):
    for D in (1, 17, 64):
        for n_data in (1, 300, 1031):
            rng = np.random.RandomState(1000 * D + n_data)
            X = rng.randn(n_data, D) / np.sqrt(D)
            eta = X @ rng.randn(D)
            if kind == 'logistic':
                y = (rng.rand(n_data) < 1.0 / (1.0 + np.exp(-eta))).astype(float)
            elif kind == 'poisson':
                y = rng.poisson(np.exp(eta)).astype(float)
            else:
                y = eta + 0.7 * rng.randn(n_data)
            model = _glm(vb, kind, X, y)
            for S in (1, 777, 4096):
                x = rng.randn(S, D)
                ll = model.pointwise_log_likelihood(x)
                ref = LO.glm_pointwise_numpy(kind, X, y, x, noise_sd=0.7)
                assert ll.shape == (S, n_data)
                err = np.max(np.abs(ll - ref))
                print('%s D %d n_data %d S %d: max |ll - ref| %.3g (max |ref| %.3g)' % (kind, D, n_data, S, err, np.max(np.abs(ref))))
                np.testing.assert_allclose(ll, ref, rtol=0, atol=1e-12 * np.max(np.abs(ref)))
                # the objective's own density: sum_i ll - model(x) + log N(x; 0, prior_sd) up to its constant is one number
                f = model(x)
                c = ll.sum(axis=1) - f - 0.5 * np.sum(x * x, axis=1) / 3.0 ** 2
                scale = max(np.max(np.abs(ll.sum(axis=1))), np.max(np.abs(f)))
                assert np.max(np.abs(c - c[0])) <= 1e-10 * scale, (kind, D, n_data, S, np.max(np.abs(c - c[0])), scale)
            one = model.pointwise_log_likelihood(x[0])                      # (D,) is one draw
            assert one.shape == (1, n_data) and np.array_equal(one[0], ll[0])


# ---- 2. batched smoothing against the oracle, vector by vector ------------------------------------------------------------
@pytest.mark.parametrize('reff', REFFS)
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('S', [100, 500, 4096, 16384])
def test_batched_smoothing_matches_oracle(vb, S, kind, reff):
    from viabel_amd._psis import batch_capacity, psislw
    assert batch_capacity(S, reff)
    lw = _weights(kind, 257, S, seed=S % 1000 + len(kind))
    refs = [opsis.psis_smooth(lw[:, j], reff) for j in range(257)]
    worst = 0.0
    for m in (1, 3, 257):
        sub = np.array(lw[:, :m], order='F')
        sm, ks = psislw(sub, Reff=reff)
        assert sm.shape == (S, m) and ks.shape == (m,) and sm is not sub and np.array_equal(sub, lw[:, :m])
        for j in range(m):
            _assert_column(sm[:, j], ks[j], refs[j][0], refs[j][1], 1e-10, (S, kind, reff, m, j))
            fin = np.isfinite(refs[j][0])
            worst = max(worst, np.max(np.abs(sm[fin, j] - refs[j][0][fin]), initial=0.0))
        sm2, ks2 = psislw(sub, Reff=reff)                                   # bit-reproducible run to run
        assert np.array_equal(sm, sm2, equal_nan=True) and np.array_equal(ks, ks2, equal_nan=True)
    print('S %d %s Reff %.1f: max |smoothed - oracle| %.3g' % (S, kind, reff, worst))


@pytest.mark.parametrize('reff', REFFS)
@pytest.mark.parametrize('kind', KINDS)
def test_batched_smoothing_5000_columns(vb, kind, reff):
    """m = 5000 at S = 4096: a seeded sample of 64 columns against the oracle, ALL columns against the single-vector
    device route (eng.psis_smooth) at the tolerance between two device kernels."""
    from viabel_amd import _lib
    from viabel_amd._psis import psislw
    S, m = 4096, 5000
    lw = _weights(kind, m, S, seed=77 + len(kind))
    sm, ks = psislw(lw, Reff=reff)
    for j in np.random.RandomState(3).choice(m, 64, replace=False):
        ref, rk = opsis.psis_smooth(lw[:, j], reff)
        _assert_column(sm[:, j], ks[j], ref, rk, 1e-10, (kind, reff, j))
    eng = _lib.default_engine()
    worst = 0.0
    for j in range(m):
        one, k1 = eng.psis_smooth(S, np.ascontiguousarray(lw[:, j]), reff=reff)
        _assert_column(sm[:, j], ks[j], one, k1, 1e-12, (kind, reff, j))
        fin = np.isfinite(one)
        worst = max(worst, np.max(np.abs(sm[fin, j] - one[fin]), initial=0.0))
    print('%s Reff %.1f: max |batched - single-vector| over 5000 columns %.3g' % (kind, reff, worst))


@pytest.mark.parametrize('S', [16385, 40000])
def test_beyond_capacity_takes_the_column_loop(vb, S, monkeypatch):
    from viabel_amd import _lib
    from viabel_amd._psis import batch_capacity, psislw
    assert not batch_capacity(S)
    eng = _lib.default_engine()
    calls = []
    real = eng.psis_smooth
    monkeypatch.setattr(eng, 'psis_smooth', lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    lw = _weights('student', 3, S, seed=S % 1000)
    sm, ks = psislw(lw)
    assert len(calls) == 3
    for j in range(3):
        ref, rk = opsis.psis_smooth(lw[:, j])
        _assert_column(sm[:, j], ks[j], ref, rk, 1e-10, (S, j))
    with pytest.raises(NotImplementedError):                               # the C entry itself refuses such vectors
        eng.psis_smooth_batch(np.ascontiguousarray(lw.T))


# ---- 3. one launch, no per-column traffic -----------------------------------------------------------------------------------
def _logistic_problem(vb, n=300, D=10, seed=4):
    rng = np.random.RandomState(seed)
    X = rng.randn(n, D) / np.sqrt(D)
    y = (rng.rand(n) < 1.0 / (1.0 + np.exp(-X @ (2.0 * rng.randn(D))))).astype(float)
    return X, y, vb.LogisticRegressionModel(X, y, prior_sd=10.0)


def test_no_per_column_calls(vb, monkeypatch, capsys):
    from viabel_amd import _lib
    from viabel_amd._psis import psislw
    eng = _lib.default_engine()
    calls = []
    real = eng.psis_smooth
    monkeypatch.setattr(eng, 'psis_smooth', lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    psislw(_weights('student', 40, 2000, seed=1))
    assert calls == []
    X, y, model = _logistic_problem(vb)
    theta = np.concatenate([np.zeros(10), np.full(10, -1.0)])
    res = vb.loo(theta, model=model, approx=vb.MFGaussian(10, seed=5), n_samples=1024)
    assert len(calls) == 1                                                  # the full-data ratios
    assert res['pointwise'].shape == (300,) and res['n_samples'] == 1024
    assert 'observations have Pareto khat > 0.7' in capsys.readouterr().out


# ---- 4. psisloo with ratios ----------------------------------------------------------------------------------------------------
def test_psisloo_with_ratios(vb):
    rng = np.random.RandomState(11)
    log_lik = -0.5 * rng.randn(2000, 40) ** 2 - 0.3 * rng.rand(2000, 40)
    log_ratios = 0.8 * rng.standard_t(5.0, 2000)
    loo, loos, ks = vb.psisloo(log_lik, log_ratios)
    ref, rks, _ = LO.loo_numpy(log_lik, log_ratios)
    print('psisloo with ratios: max |loos - numpy| %.3g' % np.max(np.abs(loos - ref)))
    np.testing.assert_allclose(loos, ref, rtol=0, atol=1e-10)
    assert all(LO.close_k(k, rk) for k, rk in zip(ks, rks)) and abs(loo - loos.sum()) < 1e-12
    loo0, loos0, ks0 = vb.psisloo(log_lik)
    loo1, loos1, ks1 = vb.psisloo(log_lik, np.zeros(2000))
    assert loo0 == loo1 and np.array_equal(loos0, loos1) and np.array_equal(ks0, ks1)
    ref0, rks0, _ = LO.loo_numpy(log_lik)
    np.testing.assert_allclose(loos0, ref0, rtol=0, atol=1e-10)
    loo_r, loos_r, ks_r = vb.psisloo(log_lik, log_ratios, Reff=0.3)
    ref_r, rks_r, _ = LO.loo_numpy(log_lik, log_ratios, reff=0.3)
    np.testing.assert_allclose(loos_r, ref_r, rtol=0, atol=1e-10)
    assert all(LO.close_k(k, rk) for k, rk in zip(ks_r, rks_r))


# ---- 5. end to end against numpy on the same draws ------------------------------------------------------------------------
def _numpy_loo_of(vb, theta, model, approx, n_samples, kind, noise_sd=1.0, reff=1.0):
    """The draws and ratios loo() forms (a fresh, identically seeded approximation draws the same noise) pushed through
    the numpy pipeline."""
    samples, log_ratios = vb.samples_and_log_weights(theta, model, approx, n_samples)
    log_w, k_full = opsis.psis_smooth(log_ratios, reff)
    ll = LO.glm_pointwise_numpy(kind, model.X, model.y, samples, noise_sd)
    loos, ks, lpd = LO.loo_numpy(ll, log_ratios, reff, log_w)
    return loos, ks, lpd, k_full


def _assert_loo_matches(res, loos, ks, lpd, k_full):
    n = loos.size
    print('loo vs numpy on the same draws: pointwise %.3g lpd %.3g' % (np.max(np.abs(res['pointwise'] - loos)),
                                                                     np.max(np.abs(res['lpd'] - lpd))))
    np.testing.assert_allclose(res['pointwise'], loos, rtol=0, atol=1e-9)
    np.testing.assert_allclose(res['lpd'], lpd, rtol=0, atol=1e-9)
    assert all(LO.close_k(k, rk) for k, rk in zip(res['khat'], ks)), np.max(np.abs(res['khat'] - ks))
    assert LO.close_k(res['khat_full'], k_full)
    assert abs(res['elpd_loo'] - loos.sum()) <= 1e-9 * n
    assert abs(res['se_elpd_loo'] - np.sqrt(n * np.var(loos))) <= 1e-9 * n
    assert abs(res['p_loo'] - np.sum(lpd - loos)) <= 1e-9 * n


def test_loo_end_to_end_after_a_device_fit(vb, capsys):
    from viabel_amd.optimization import Adam
    D = 10
    X, y, model = _logistic_problem(vb)
    objective = vb.ExclusiveKL(vb.MFGaussian(D, seed=3, rng='philox'), model, 64)
    init = np.concatenate([np.zeros(D), np.full(D, -1.0)])
    theta = Adam(0.05, iterate_avg_prop=None).optimize(400, objective, init, on_device=True)['opt_param']
    res = vb.loo(theta, model=model, approx=vb.MFGaussian(D, seed=5), n_samples=4096)
    capsys.readouterr()
    loos, ks, lpd, k_full = _numpy_loo_of(vb, theta, model, vb.MFGaussian(D, seed=5), 4096, 'logistic')
    _assert_loo_matches(res, loos, ks, lpd, k_full)
    assert res['p_loo'] > 0 and np.all(res['lpd'] >= res['pointwise'] - 1e-9)
    res_o = vb.loo(theta, objective=vb.ExclusiveKL(vb.MFGaussian(D, seed=5), model, 8), n_samples=4096)
    capsys.readouterr()
    assert np.array_equal(res_o['pointwise'], res['pointwise'])


def test_loo_in_chunks_of_observations(vb):
    """More than 1 GiB of likelihoods (8200 observations x 16 384 draws: 8192 observations fit the device budget, eight
    are left for a second pass; the host matrix of vb_glm_pointwise goes in passes of 4096): the observations on both
    sides of the boundaries against numpy."""
    from viabel_amd import _lib
    S, D, n_data = 16384, 4, 8200
    rng = np.random.RandomState(21)
    X = rng.randn(n_data, D) / np.sqrt(D)
    y = (rng.rand(n_data) < 0.5).astype(float)
    model = vb.LogisticRegressionModel(X, y, prior_sd=10.0)
    x = 0.3 * rng.randn(S, D)
    log_ratios = 0.5 * rng.standard_t(6.0, S)
    log_w, _ = opsis.psis_smooth(log_ratios)
    eng = _lib.default_engine()
    eng.set_model(model.device_spec())
    loo, khat, lpd = eng.glm_psis_loo(x, n_data, log_ratios=log_ratios, log_w=log_w)
    pick = np.array([0, 1, 4095, 4096, 8190, 8191, 8192, 8193, 8199])
    ll = LO.glm_pointwise_numpy('logistic', X[pick], y[pick], x)
    loos, ks, lpd_ref = LO.loo_numpy(ll, log_ratios, 1.0, log_w)
    np.testing.assert_allclose(loo[pick], loos, rtol=0, atol=1e-9)
    np.testing.assert_allclose(lpd[pick], lpd_ref, rtol=0, atol=1e-9)
    assert all(LO.close_k(k, rk) for k, rk in zip(khat[pick], ks))
    assert np.all(np.isfinite(loo)) and np.all(np.isfinite(lpd))
    full = model.pointwise_log_likelihood(x)
    assert full.shape == (S, n_data)
    np.testing.assert_allclose(full[:, pick], ll, rtol=0, atol=1e-12 * np.max(np.abs(ll)))


# ---- 6. against a closed form ------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def linear(vb):
    X, y, prior_sd, noise_sd, _ = LO.linear_problem(1)
    m, V = LO.linear_posterior(X, y, prior_sd, noise_sd)
    return (vb.LinearRegressionModel(X, y, prior_sd=prior_sd, noise_sd=noise_sd), m, V,
            LO.linear_loo_closed_form(X, y, prior_sd, noise_sd))


def test_loo_against_closed_form(vb, linear, capsys):
    """q = the exact Gaussian posterior.  The Monte-Carlo tolerance is the numpy pipeline's own largest error against the
    closed form on the same draws plus the 1e-9 allowed between device and numpy (triangle inequality); the assertion
    that binds is device-vs-numpy at 1e-9.  No observation is skipped or masked."""
    model, m, V, exact = linear
    theta = vb.FullRankGaussian(8).pack(m, np.linalg.cholesky(V))
    res = vb.loo(theta, model=model, approx=vb.FullRankGaussian(8), n_samples=4096)
    capsys.readouterr()
    loos, ks, lpd, k_full = _numpy_loo_of(vb, theta, model, vb.FullRankGaussian(8), 4096, 'linear')
    _assert_loo_matches(res, loos, ks, lpd, k_full)
    err_np, err_dev = np.abs(loos - exact), np.abs(res['pointwise'] - exact)
    print('closed form: numpy max %.3g mean %.3g, device max %.3g, elpd %.2f vs %.2f, largest khat %.2f'
          % (err_np.max(), err_np.mean(), err_dev.max(), res['elpd_loo'], exact.sum(), res['khat'].max()))
    assert res['khat'].max() < 0.7
    assert err_dev.max() <= err_np.max() + 1e-9
    assert abs(res['elpd_loo'] - exact.sum()) <= abs(loos.sum() - exact.sum()) + 200e-9


@pytest.mark.parametrize('scale', [1.2, 0.9])
def test_loo_needs_the_ratios_for_a_misscaled_q(vb, linear, scale, capsys):
    """q = N(m, scale^2 V): the correction p(theta, y) / q(theta) is wired in -- with it elpd_loo stays at the closed
    form (error below a tenth of the error without it)."""
    from viabel_amd import _lib
    model, m, V, exact = linear
    theta = vb.FullRankGaussian(8).pack(m, scale * np.linalg.cholesky(V))
    res = vb.loo(theta, model=model, approx=vb.FullRankGaussian(8), n_samples=4096)
    capsys.readouterr()
    loos, ks, lpd, k_full = _numpy_loo_of(vb, theta, model, vb.FullRankGaussian(8), 4096, 'linear')
    _assert_loo_matches(res, loos, ks, lpd, k_full)
    samples, _ = vb.samples_and_log_weights(theta, model, vb.FullRankGaussian(8), 4096)
    eng = _lib.default_engine()
    eng.set_model(model.device_spec())
    without, _, _ = eng.glm_psis_loo(samples, model.n_data)                 # the draws taken for posterior draws
    e_with, e_without = abs(res['elpd_loo'] - exact.sum()), abs(without.sum() - exact.sum())
    print('scale %.1f: elpd error with ratios %.3g, without %.3g, largest khat %.2f' % (scale, e_with, e_without, res['khat'].max()))
    assert res['khat'].max() < 0.7
    assert e_with < 0.1 * e_without


# ---- 7. errors ------------------------------------------------------------------------------------------------------------------
def test_errors(vb):
    from viabel_amd import _lib
    theta = np.zeros(6)
    with pytest.raises(NotImplementedError):
        vb.loo(theta, model=vb.GaussianModel(np.zeros(3), np.ones(3)), approx=vb.MFGaussian(3))
    src = ('__device__ double vb_log_density(const double* z, int d, const double*, double* g) {'
           ' double f = 0; for (int j = 0; j < d; ++j) { f -= 0.5 * z[j] * z[j]; if (g) g[j] = -z[j]; } return f; }')
    with pytest.raises(NotImplementedError):
        vb.loo(theta, model=vb.SourceModel(3, src), approx=vb.MFGaussian(3))
    fresh = _lib.Engine()
    try:
        with pytest.raises(_lib.EngineError):                               # no model bound
            fresh.glm_pointwise(np.zeros((4, 3)), 5)
        fresh.set_model(vb.GaussianModel(np.zeros(3), np.ones(3)).device_spec())
        with pytest.raises(NotImplementedError):                            # bound, but without observations
            fresh.glm_pointwise(np.zeros((4, 3)), 5)
        with pytest.raises(NotImplementedError):
            fresh.glm_psis_loo(np.zeros((4, 3)), 5)
    finally:
        fresh.close()
    X, y, model = _logistic_problem(vb)
    with pytest.raises(ValueError):
        model.pointwise_log_likelihood(np.zeros((4, 9)))                    # wrong D, caught by the model
    eng = _lib.default_engine()
    eng.set_model(model.device_spec())
    with pytest.raises(ValueError):
        eng.glm_pointwise(np.zeros((4, 9)), 300)                            # ... and by the C entry
    with pytest.raises(ValueError):
        eng.glm_psis_loo(np.zeros((1, 10)), 300)                            # more than one draw
    with pytest.raises(ValueError):
        eng.glm_psis_loo(np.zeros((8, 10)), 300, log_ratios=np.zeros(7))
    with pytest.raises(ValueError):
        eng.glm_psis_loo(np.zeros((8, 10)), 300, reff=0.0)
    with pytest.raises(ValueError):
        eng.psis_smooth_batch(np.zeros((3, 1)))                             # more than one log weight
