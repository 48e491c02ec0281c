"""Kernel Stein discrepancy without a GPU: the numpy oracle of tests/_ksd_oracle.py against finite differences of the Stein
kernel and the properties the GPU tests rely on (symmetry, positive semi-definiteness, scale and translation rules,
sensitivity to a wrong sample), the launch plan vb_ksd_plan, and the Python entries' argument errors and refusals, which
must be raised before any engine exists (there is none here: touching it would raise EngineError instead)."""
import numpy as np
import pytest

import _ksd_oracle as K


# ---- the oracle -------------------------------------------------------------------------------------------------------
def _base(x, y, c, beta):
    return (c * c + np.sum((x - y) ** 2)) ** beta


def test_oracle_matches_finite_differences_of_the_stein_kernel():
    """k_p = g_x . g_y k + g_x . grad_y k + g_y . grad_x k + tr grad_x grad_y k at a random pair, c = 0.7, beta = -0.3,
    D = 3, the derivatives of k = (c^2 + |x - y|^2)^beta by central differences."""
    rng = np.random.RandomState(7)
    d, c, beta, h = 3, 0.7, -0.3, 1e-4
    x, y, gx, gy = rng.randn(d), rng.randn(d), rng.randn(d), rng.randn(d)
    eye = np.eye(d)
    grad_x = np.array([(_base(x + h * e, y, c, beta) - _base(x - h * e, y, c, beta)) / (2 * h) for e in eye])
    grad_y = np.array([(_base(x, y + h * e, c, beta) - _base(x, y - h * e, c, beta)) / (2 * h) for e in eye])
    trace = sum((_base(x + h * e, y + h * e, c, beta) - _base(x + h * e, y - h * e, c, beta)
                 - _base(x - h * e, y + h * e, c, beta) + _base(x - h * e, y - h * e, c, beta)) / (4 * h * h) for e in eye)
    fd = gx @ gy * _base(x, y, c, beta) + gx @ grad_y + gy @ grad_x + trace
    kp = K.stein_kernel_matrix(np.stack([x, y]), np.stack([gx, gy]), c=c, beta=beta)
    assert abs(kp[0, 1] - fd) <= 1e-6 * max(1.0, abs(fd)), (kp[0, 1], fd)
    assert kp[0, 1] == kp[1, 0]


@pytest.mark.parametrize('c,beta', [(1.0, -0.5), (0.05, -0.9), (30.0, -0.1)])
def test_stein_kernel_is_symmetric_and_positive_semidefinite(c, beta):
    rng = np.random.RandomState(11)
    x, g = rng.randn(60, 4), rng.randn(60, 4)
    kp = K.stein_kernel_matrix(x, g, c=c, beta=beta)
    np.testing.assert_allclose(kp, kp.T, rtol=0, atol=1e-13 * np.max(np.abs(kp)))
    eig = np.linalg.eigvalsh(0.5 * (kp + kp.T))
    assert eig[0] >= -1e-12 * eig[-1], (eig[0], eig[-1])


def test_scale_equals_prescaled_inputs():
    rng = np.random.RandomState(12)
    x, g = rng.randn(70, 5), rng.randn(70, 5)
    ell = np.exp(rng.randn(5))
    lw = rng.randn(70)
    a = K.ksd(x, g, lw, scale=ell, c=0.8, beta=-0.4)
    b = K.ksd(x / ell, g * ell, lw, c=0.8, beta=-0.4)
    assert a['ksd2'] == b['ksd2'] and np.array_equal(a['rowsums'], b['rowsums'])


def test_translation_invariance_with_translated_scores():
    """Draws of N(m, I) with scores -(x - m): the discrepancy does not depend on m beyond rounding."""
    rng = np.random.RandomState(13)
    z = rng.randn(90, 6)
    a = K.ksd(z, -z)
    m = 3.0 + rng.randn(6)
    x = z + m
    b = K.ksd(x, -(x - m))
    tol = K.tolerance(90, 6)
    assert abs(a['ksd2'] - b['ksd2']) <= 64 * tol * a['E'], (a['ksd2'], b['ksd2'])


def test_misspecified_samples_score_worse_than_the_exact_one():
    """N(0, I), scores -x, D = 8, S = 2048: shifted, too wide and too narrow samples each give more than four times the
    exact sample's ksd2 (the oracle's own ratios are 9.0, 5.2 and 10.7)."""
    rng = np.random.RandomState(2056)
    d, s = 8, 2048
    z = rng.randn(s, d)
    exact = K.ksd(z, -z)['ksd2']
    shift = np.full(d, 0.5 / np.sqrt(d))
    values = dict(shifted=K.ksd(z + shift, -(z + shift))['ksd2'], wide=K.ksd(1.3 * z, -1.3 * z)['ksd2'],
                  narrow=K.ksd(0.7 * z, -0.7 * z)['ksd2'])
    print('exact %.4g, %s' % (exact, ', '.join('%s %.4g (x%.1f)' % (k, v, v / exact) for k, v in values.items())))
    assert 0.0 < exact < 0.02
    for name, v in values.items():
        assert v > 4.0 * exact, (name, v, exact)


# ---- the launch plan --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_cu', [1, 256])
@pytest.mark.parametrize('s', [1, 64, 65, 1500, 65536])
def test_plan_deals_every_column_tile_to_one_split(s, n_cu):
    from viabel_amd import _lib
    blocks, splits = _lib.ksd_plan(s, n_cu)
    assert blocks == (s + 63) // 64 and 1 <= splits <= blocks
    ranges = _lib.ksd_split_tiles(blocks, splits)
    assert len(ranges) == splits and ranges[0][0] == 0 and ranges[-1][1] == blocks
    assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))            # contiguous: each tile in exactly one split
    lengths = [hi - lo for lo, hi in ranges]
    assert min(lengths) >= 1 and max(lengths) - min(lengths) <= 1
    # fills the device where the tiles allow: two workgroups per compute unit
    assert blocks * splits >= min(2 * n_cu, blocks * blocks)


def test_plan_rejections():
    import ctypes
    from viabel_amd import _lib
    lib = _lib.load()
    out = (ctypes.c_int * 2)()
    assert lib.vb_ksd_plan(64, 256, None) == _lib.VB_ERR_INVALID
    assert lib.vb_ksd_plan(0, 256, out) == _lib.VB_ERR_INVALID
    assert lib.vb_ksd_plan(64, 0, out) == _lib.VB_ERR_INVALID
    assert lib.vb_ksd_plan(64, 256, out) == _lib.VB_OK and tuple(out) == (1, 1)
    for bad in ((0, 256), (64, 0), (-3, 4)):
        with pytest.raises(ValueError):
            _lib.ksd_plan(*bad)


# ---- the Python entries -----------------------------------------------------------------------------------------------
def test_ksd_is_exported():
    import viabel_amd
    from viabel_amd import convenience
    assert 'ksd' in convenience.__all__ and viabel_amd.ksd is convenience.ksd


def _gaussian(vb, d=3):
    return vb.GaussianModel(np.zeros(d), np.ones(d))


def test_argument_errors_are_raised_before_any_engine_exists():
    import viabel_amd as vb
    model = _gaussian(vb)
    approx = vb.MFGaussian(3)
    theta = np.zeros(6)
    x = np.random.RandomState(0).randn(10, 3)
    bad_calls = [
        dict(),                                                            # neither a fit nor draws
        dict(var_param=theta, samples=x, model=model),                     # both
        dict(var_param=theta, model=model),                                # approx missing
        dict(var_param=theta, objective=object(), model=model),
        dict(var_param=theta, model=model, approx=approx, beta=0.0),
        dict(var_param=theta, model=model, approx=approx, beta=-1.0),
        dict(var_param=theta, model=model, approx=approx, c=0.0),
        dict(var_param=theta, model=model, approx=approx, c=np.inf),
        dict(var_param=theta, model=model, approx=approx, weights='raw'),
        dict(var_param=theta, model=model, approx=approx, n_samples=1),
        dict(var_param=theta, model=model, approx=approx, Reff=0.0),
        dict(var_param=theta, model=model, approx=approx, scale=np.array([1.0, 0.0, 1.0])),
        dict(var_param=theta, model=model, approx=approx, scale=np.ones(4)),
        dict(var_param=theta, model=model, approx=approx, scale='sd'),
        dict(var_param=theta, model=model, approx=approx, scores=-x),
        dict(samples=x),                                                   # neither model nor scores
        dict(samples=x, model=model, scores=-x),                           # both
        dict(samples=x, scores=-x[:, :2]),
        dict(samples=x[0], scores=-x[0]),
        dict(samples=x, scores=-x, log_weights=np.zeros(9)),
        dict(samples=x, scores=-x, log_weights=np.full(10, -np.inf)),
        dict(samples=np.where(np.arange(30).reshape(10, 3) == 4, np.nan, x), scores=-x),
        dict(samples=x, scores=-x, scale=np.array([1.0, -1.0, 1.0])),
        dict(samples=x, scores=-x, scale=np.array([1.0, np.inf, 1.0])),
        dict(samples=np.ones((10, 3)), scores=-x),                         # scale='auto' without spread
        dict(samples=x[:, :2], model=model),
        dict(samples=x, scores=-x, beta=-1.5),
    ]
    for kwargs in bad_calls:
        with pytest.raises(ValueError):
            vb.ksd(**kwargs)
    from viabel_amd import _lib
    for kwargs in (dict(beta=0.0), dict(c=-1.0), dict(scores=-x[:5]), dict(scale=np.zeros(3)), dict(log_w=np.zeros(3))):
        with pytest.raises(ValueError):
            _lib.ksd_arguments(x, **kwargs)
    with pytest.raises(ValueError):
        model.ksd_from_draws(x, beta=0.5)
    with pytest.raises(ValueError):
        model.ksd_from_draws(x[:, :2])


def test_callable_and_minibatch_models_are_refused():
    import viabel_amd as vb
    x = np.random.RandomState(1).randn(8, 3)
    callable_model = vb.CallableModel(3, lambda z: -0.5 * np.sum(z * z, axis=1), lambda z: -z)
    with pytest.raises(NotImplementedError, match='scores='):
        callable_model.ksd_from_draws(x)
    with pytest.raises(NotImplementedError, match='scores='):
        vb.ksd(samples=x, model=callable_model)
    rng = np.random.RandomState(2)
    X = rng.randn(20, 3)
    y = (rng.rand(20) < 0.5).astype(float)
    minibatch = vb.MinibatchRegressionModel(X, y, 5)
    with pytest.raises(NotImplementedError, match='full_model'):
        minibatch.ksd_from_draws(x)
    with pytest.raises(NotImplementedError, match='full_model'):
        vb.ksd(np.zeros(6), model=minibatch, approx=vb.MFGaussian(3))
