"""CPU: the SVGD oracle against itself in extended precision and against closed forms, the median rank, the argument
checks of svgd() (which raise before an engine is touched), the exports and the header's declarations."""
import os

import numpy as np
import pytest

import _svgd_oracle as S
import viabel_amd as vb
from viabel_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _particles(n, d, seed, shift=0.0):
    rng = np.random.RandomState(seed)
    x = rng.randn(n, d) * 10.0 ** np.linspace(-2.0, 2.0, d) + rng.randn(d) + shift
    g = rng.randn(n, d) * 10.0 ** np.linspace(1.0, -3.0, d)
    return x, g


@pytest.mark.parametrize('shift', [0.0, 1e6])
@pytest.mark.parametrize('n,d', [(2, 5), (65, 33), (200, 40)])
def test_float64_oracle_within_tolerance_of_extended_precision(n, d, shift):
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip('np.longdouble is float64 on this platform')
    x, g = _particles(n, d, 10 * n + d, shift)
    for scale in (None, 10.0 ** np.linspace(-2.0, 2.0, d)):
        ref = S.direction(x, g, scale)
        h64 = float(ref['h'])
        ref = S.direction(x, g, scale, bandwidth=h64)
        low = S.direction(x, g, scale, bandwidth=h64, dtype=np.float64)
        frac = np.max(np.abs(low['phi'] - ref['phi']) / (S.tolerance(n, d) * ref['E']))
        hfrac = abs(float(S.direction(x, g, scale, dtype=np.float64)['h']) - h64) / (S.bandwidth_tolerance(d) * h64)
        print('n %d D %d shift %g: phi %.3f tol E, h %.3f of its tolerance' % (n, d, shift, frac, hfrac))
        assert frac <= 1.0 and hfrac <= 1.0


def test_one_particle():
    g = np.array([[0.3, -2.0, 5.0]])
    for scale in (None, np.array([0.5, 2.0, 8.0])):       # (powers of two: g * s / s is exact)
        out = S.direction(np.array([[1.0, 2.0, 3.0]]), g, scale)
        assert out['h'] == 1.0
        assert np.array_equal(np.asarray(out['phi'], dtype=np.float64), g)


def test_two_particles():
    x = np.array([[0.0, 0.0], [3.0, 4.0]])
    g = np.array([[1.0, -1.0], [0.5, 2.0]])
    out = S.direction(x, g)
    h = 25.0 / np.log(3.0)                                 # the one distance is the median; kappa_12 = exp(-log 3) = 1/3
    assert abs(float(out['h']) - h) <= 1e-15 * h
    y = x - x.mean(axis=0)
    expected = np.array([0.5 * (g[0] + g[1] / 3.0 + (2.0 / h) * (y[0] - y[1]) / 3.0),
                         0.5 * (g[1] + g[0] / 3.0 + (2.0 / h) * (y[1] - y[0]) / 3.0)])
    np.testing.assert_allclose(np.asarray(out['phi'], dtype=np.float64), expected, rtol=1e-14)


def test_all_particles_equal():
    rng = np.random.RandomState(3)
    x = np.tile(rng.randn(1, 4), (7, 1))
    g = rng.randn(7, 4)
    out = S.direction(x, g, scale=np.array([0.5, 1.0, 2.0, 4.0]))
    assert out['h'] == 1.0
    np.testing.assert_allclose(np.asarray(out['phi'], dtype=np.float64), np.tile(g.mean(axis=0), (7, 1)), rtol=1e-14)


@pytest.mark.parametrize('n', [2, 3, 4, 5, 10, 63, 64])
def test_median_rank(n):
    rng = np.random.RandomState(n)
    y = np.round(rng.randn(n, 2) * 2.0)                    # integer coordinates: many ties
    r2 = S.squared_distances(y)
    v = np.sort(r2[np.triu_indices(n, 1)])
    total = n * (n - 1) // 2
    assert v.size == total and S.median_rank(n) == (total - 1) // 2
    assert S.lower_median(r2) == v[(total - 1) // 2]
    assert S.lower_median(r2) == np.partition(r2[np.triu_indices(n, 1)], (total - 1) // 2)[(total - 1) // 2]
    if total % 2 == 1:
        assert S.lower_median(r2) == np.median(v)
    else:
        assert S.lower_median(r2) <= np.median(v)


def test_svgd_argument_checks_raise_before_an_engine_is_touched(monkeypatch):
    def no_engine():
        raise AssertionError('the engine was touched')
    monkeypatch.setattr(_lib, 'default_engine', no_engine)
    model = vb.GaussianModel(np.zeros(3), np.ones(3))
    init = np.zeros((8, 3))
    ok = dict(n_particles=8, n_iters=5, init=init)
    with pytest.raises(TypeError):
        vb.svgd(lambda x: x, **ok)
    with pytest.raises(NotImplementedError):
        vb.svgd(vb.CallableModel(3, lambda x: -0.5 * np.sum(x * x, axis=1), lambda x: -x), **ok)
    X = np.random.RandomState(0).randn(20, 3)
    with pytest.raises(NotImplementedError):
        vb.svgd(vb.MinibatchRegressionModel(X, (X[:, 0] > 0).astype(float), 5), **ok)
    with pytest.raises(ValueError):
        vb.svgd(model, n_particles=8, n_iters=5)                               # neither init nor a fit
    with pytest.raises(ValueError):
        vb.svgd(model, n_particles=8, n_iters=5, var_param=np.zeros(6))        # var_param without approx
    for bad in (dict(n_particles=0), dict(n_iters=0), dict(n_particles=2.5), dict(init=np.zeros((7, 3))),
                dict(init=np.full((8, 3), np.nan)), dict(scale='median'), dict(scale=np.ones(2)),
                dict(scale=np.array([1.0, 0.0, 1.0])), dict(bandwidth='mean'), dict(bandwidth=-1.0), dict(bandwidth=0.0),
                dict(bandwidth=np.inf), dict(optimizer=vb.Adagrad(0.1, weight_decay=0.5)),
                dict(optimizer=vb.RMSProp(np.ones(3)))):
        with pytest.raises(ValueError):
            vb.svgd(model, **dict(ok, **bad))
    with pytest.raises(TypeError):
        vb.svgd(model, **dict(ok, optimizer=vb.WindowedAdagrad(0.1)))
    with pytest.raises(TypeError):
        vb.svgd(model, **dict(ok, optimizer='adagrad'))
    with pytest.raises(NotImplementedError):
        vb.svgd(model, n_particles=_lib.SVGD_MAX_PARTICLES + 1, n_iters=5, init=init)
    # the layer below: shapes, finiteness, the capacity
    with pytest.raises(ValueError):
        _lib.svgd_arguments(np.zeros(3))
    with pytest.raises(ValueError):
        _lib.svgd_arguments(np.zeros((4, 3)), scores=np.zeros((4, 2)))
    with pytest.raises(ValueError):
        _lib.svgd_arguments(np.zeros((4, 3)), scores=np.full((4, 3), np.inf))
    with pytest.raises(NotImplementedError):
        _lib.svgd_arguments(np.zeros((_lib.SVGD_MAX_PARTICLES + 1, 1)))
    assert _lib.svgd_arguments(np.zeros((4, 3)))[3] == 0.0 and _lib.svgd_arguments(np.zeros((4, 3)), bandwidth=2)[3] == 2.0
    with pytest.raises(NotImplementedError):
        vb.MinibatchRegressionModel(X, (X[:, 0] > 0).astype(float), 5).svgd_direction(np.zeros((4, 3)))
    with pytest.raises(NotImplementedError):
        vb.CallableModel(3, lambda x: -0.5 * np.sum(x * x, axis=1), lambda x: -x).svgd_direction(np.zeros((4, 3)))
    with pytest.raises(ValueError):
        model.svgd_direction(np.zeros((4, 2)))


def test_exports():
    import sys
    assert callable(vb.svgd) and vb.svgd is sys.modules['viabel_amd.svgd'].svgd
    assert sys.modules['viabel_amd.svgd'].__all__ == ['svgd']
    assert _lib.SVGD_MAX_PARTICLES == 8192
    for name in ('svgd_direction', 'svgd_run'):
        assert callable(getattr(_lib.Engine, name))
    assert callable(vb.DeviceModel.svgd_direction)
    assert vb.svgd.__kwdefaults__ == dict(n_particles=256, n_iters=1000, init=None, var_param=None, approx=None,
                                          optimizer=None, scale='auto', bandwidth='median', seed=1)


def test_header_declares_both_entries():
    header = open(os.path.join(ROOT, 'include', 'viabel_hip.h')).read()
    assert 'int vb_svgd_direction(vb_ctx* ctx' in header and 'int vb_svgd_run(vb_ctx* ctx' in header
    for name, n_args in (('vb_svgd_direction', 10), ('vb_svgd_run', 16)):
        restype, argtypes = _lib.SIGNATURES[name]
        assert argtypes[0] is _lib._ctx_p and len(argtypes) == n_args
    lib = _lib.load()
    for name in ('vb_svgd_direction', 'vb_svgd_run'):
        argtypes = _lib.SIGNATURES[name][1]
        zeros = [None if t in (_lib._ctx_p, _lib._c_double_p, _lib._c_int64_p) else 0 for t in argtypes]
        assert getattr(lib, name)(*zeros) == _lib.VB_ERR_INVALID
    assert 'vb_svgd.hip' in open(os.path.join(ROOT, 'viabel_amd', 'csrc', 'Makefile')).read()
