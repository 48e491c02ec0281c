"""CPU: what PSIS-LOO checks before it touches the engine, the C entry points' own argument checks, and the numpy
restatement of the LOO pipeline (tests/_loo_oracle.py: the yardstick of tests/test_gpu_loo.py) against the closed-form
leave-one-out density of a linear regression."""
import numpy as np
import pytest

import _loo_oracle as LO
from oracle import psis as opsis


def test_psisloo_validates_shapes_before_the_engine():
    from viabel_amd._psis import psisloo
    with pytest.raises(ValueError):
        psisloo(np.zeros(10))                                         # not draws x observations
    with pytest.raises(ValueError):
        psisloo(np.zeros((10, 3)), log_ratios=np.zeros(9))            # one ratio per draw
    with pytest.raises(ValueError):
        psisloo(np.zeros((10, 3)), log_ratios=np.zeros((10, 1)))
    with pytest.raises(ValueError):
        psisloo(np.zeros((1, 3)), log_ratios=np.zeros(1))             # more than one draw


def test_loo_validates_arguments_before_the_engine():
    import viabel_amd as vb
    X = np.random.RandomState(0).randn(12, 3)
    y = (X[:, 0] > 0).astype(float)
    model = vb.LogisticRegressionModel(X, y)
    approx = vb.MFGaussian(3)
    theta = np.zeros(6)
    objective = vb.ExclusiveKL(approx, model, 8)
    with pytest.raises(ValueError):
        vb.loo(theta)
    with pytest.raises(ValueError):
        vb.loo(theta, model=model)
    with pytest.raises(ValueError):
        vb.loo(theta, objective=objective, model=model)
    with pytest.raises(ValueError):
        vb.loo(theta, objective=objective, approx=approx)
    with pytest.raises(ValueError):
        vb.loo(theta, model=model, approx=approx, n_samples=1)
    with pytest.raises(ValueError):
        vb.loo(theta, model=model, approx=approx, Reff=0.0)
    # a model without observations: the message names the route for a user-built matrix
    for other in (vb.GaussianModel(np.zeros(3), np.ones(3)), vb.FunnelModel(3),
                  vb.SourceModel(3, '__device__ double vb_log_density(const double*, int, const double*, double*);'),
                  vb.CallableModel(3, lambda z: -0.5 * np.sum(z * z, axis=1))):
        with pytest.raises(NotImplementedError, match=r'psisloo\(log_lik, log_ratios\)'):
            vb.loo(theta, model=other, approx=approx)
    # beyond the batched kernel's capacity: the limit is stated
    with pytest.raises(NotImplementedError, match='16384'):
        vb.loo(theta, model=model, approx=approx, n_samples=16385)
    with pytest.raises(NotImplementedError, match='1024'):
        vb.loo(theta, model=model, approx=approx, n_samples=16384, Reff=0.1)
    assert 'loo' in vb.__dict__ and 'psisloo' in vb.__dict__


def test_batch_capacity_matches_the_tail_rule():
    from viabel_amd._psis import _tail_size, batch_capacity
    for n, reff in ((100, 1.0), (16384, 1.0), (16384, 0.3), (4096, 2.5), (7, 1.0)):
        assert _tail_size(n, reff) == opsis.tail_size(n, reff)
        assert batch_capacity(n, reff)
    assert _tail_size(16384, 1.0) == 384 and _tail_size(16384, 0.3) == 702
    assert not batch_capacity(16385) and not batch_capacity(40000) and not batch_capacity(1)
    assert not batch_capacity(16384, 0.1)                             # tail 1215 > 1024


def test_new_entry_points_reject_bad_arguments_without_a_device():
    """NULL context with otherwise plausible arguments, and NULL buffers / non-positive shapes: an error code, nothing
    dereferenced (no context exists on a machine without a GPU, so nothing past the argument checks can run)."""
    from viabel_amd import _lib
    lib = _lib.load()
    buf = np.zeros(64)
    p = _lib._dptr(buf)
    cases = [
        ('vb_psis_smooth_batch', (None, p, 8, 2, 8, 1.0, p, p)),
        ('vb_psis_smooth_batch', (None, None, 8, 2, 8, 1.0, None, None)),
        ('vb_psis_smooth_batch', (None, p, 0, 0, 0, 0.0, p, p)),
        ('vb_psis_smooth_batch', (None, p, -3, -1, -3, 1.0, p, p)),
        ('vb_glm_pointwise', (None, p, 4, 2, p)),
        ('vb_glm_pointwise', (None, None, 0, 0, None)),
        ('vb_glm_pointwise', (None, p, -1, -1, p)),
        ('vb_glm_psis_loo', (None, p, 8, 2, p, p, 1.0, p, p, p)),
        ('vb_glm_psis_loo', (None, None, 0, 0, None, None, 0.0, None, None, None)),
        ('vb_glm_psis_loo', (None, p, -8, -2, None, None, -1.0, p, p, None)),
    ]
    for name, args in cases:
        rc = getattr(lib, name)(*args)
        assert rc == _lib.VB_ERR_INVALID, (name, args, rc)
    assert isinstance(lib.vb_last_error(None), bytes)


@pytest.fixture(scope='module')
def linear():
    X, y, prior_sd, noise_sd, Z = LO.linear_problem()
    m, V = LO.linear_posterior(X, y, prior_sd, noise_sd)
    return X, y, prior_sd, noise_sd, m, V, LO.linear_loo_closed_form(X, y, prior_sd, noise_sd), Z


def test_closed_form_is_a_density_of_the_left_out_observation(linear):
    """The closed form against brute force: p(y_i | y_-i) = p(y) / p(y_-i) with Gaussian marginal likelihoods."""
    X, y, prior_sd, noise_sd, _, _, exact, _ = linear

    def log_marginal(Xs, ys):
        C = noise_sd ** 2 * np.eye(len(ys)) + prior_sd ** 2 * Xs @ Xs.T
        _, logdet = np.linalg.slogdet(C)
        return -0.5 * (ys @ np.linalg.solve(C, ys) + logdet + len(ys) * np.log(2.0 * np.pi))

    full = log_marginal(X, y)
    for i in (0, 17, 199):
        keep = np.arange(len(y)) != i
        assert abs(exact[i] - (full - log_marginal(X[keep], y[keep]))) < 1e-9


def test_numpy_pipeline_against_closed_form(linear):
    """Draws from the exact posterior (constant ratios): PSIS-LOO is a self-normalised importance-sampling estimate of
    p(y_i | y_-i).  With S = 4096 draws and weights of finite variance (every k-hat below 0.5 here) its relative
    standard error is sqrt((1 + cv^2) / S) with cv the weights' coefficient of variation, O(1) when one of 200
    observations is left out: 1 / sqrt(4096) = 0.016 per observation.  Bound: five of those, 0.078, on the worst of the
    200, and the mean absolute error below one of them."""
    X, y, prior_sd, noise_sd, m, V, exact, Z = linear
    S = Z.shape[0]
    theta = m + Z @ np.linalg.cholesky(V).T
    ll = LO.glm_pointwise_numpy('linear', X, y, theta, noise_sd)
    loos, ks, _ = LO.loo_numpy(ll)
    err = np.abs(loos - exact)
    print('numpy pipeline vs closed form: max %.3g mean %.3g elpd %.3g (elpd %.2f), largest khat %.2f'
          % (err.max(), err.mean(), abs(loos.sum() - exact.sum()), exact.sum(), ks.max()))
    assert ks.max() < 0.7
    assert err.max() < 5.0 / np.sqrt(S) and err.mean() < 1.0 / np.sqrt(S)
    # constant ratios change nothing (they shift every vector, and the smoothing normalises)
    loos_c, ks_c, _ = LO.loo_numpy(ll[:, :5], log_ratios=np.full(S, 3.5))
    np.testing.assert_allclose(loos_c, loos[:5], rtol=0, atol=1e-10)


@pytest.mark.parametrize('scale', [1.2, 0.9])
def test_numpy_pipeline_needs_the_ratios_for_a_misscaled_q(linear, scale):
    """Draws from q = N(m, scale^2 V): with log p(theta, y) - log q(theta) the estimate stays at the closed form, without
    it the draws are treated as posterior draws and elpd_loo is off by units."""
    X, y, prior_sd, noise_sd, m, V, exact, Z = linear
    L = scale * np.linalg.cholesky(V)
    theta = m + Z @ L.T
    ll = LO.glm_pointwise_numpy('linear', X, y, theta, noise_sd)
    ratios = LO.linear_log_joint(X, y, prior_sd, noise_sd, theta) - LO.gaussian_log_density(theta, m, L)
    with_r, ks, _ = LO.loo_numpy(ll, log_ratios=ratios)
    without, _, _ = LO.loo_numpy(ll)
    e_with, e_without = abs(with_r.sum() - exact.sum()), abs(without.sum() - exact.sum())
    print('scale %.1f: elpd error with ratios %.3g, without %.3g, largest khat %.2f' % (scale, e_with, e_without, ks.max()))
    assert ks.max() < 0.7
    assert e_with < 0.1 * e_without
