"""CPU: the host side of the Laplace approximation -- exports, argument checks, the Newton driver of
``DeviceModel.find_mode`` and the assembly in ``laplace_approximation`` -- on numpy-backed subclasses that override the one
hook both go through (``_value_grad_hessian``).  No engine is created: ``default_engine`` is replaced by a function that
fails the test."""
import inspect
import os
import re
import warnings

import numpy as np
import pytest

import _laplace_oracle as LA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def vb(monkeypatch):
    import viabel_amd
    from viabel_amd import _lib

    def no_engine(*a, **k):
        raise AssertionError('an engine was asked for')
    monkeypatch.setattr(_lib, 'default_engine', no_engine)
    return viabel_amd


def _hooked(vb, dim, hook):
    """A DeviceModel of dimension ``dim`` whose hook is the numpy function ``hook(x, want_hessian)``; it records the calls."""
    class Hooked(vb.DeviceModel):
        def __init__(self):
            super().__init__(dim)
            self.calls = []

        def _value_grad_hessian(self, x, want_hessian=True):
            out = hook(np.asarray(x, dtype=np.float64), want_hessian)
            self.calls.append((np.array(x, dtype=np.float64), out[0], bool(want_hessian)))
            return out
    return Hooked()


def _glm(vb, kind, D=7, n_data=33, seed=5, dtype=np.longdouble):
    """The regression target of the driver tests: its value in long double, rounded once, so that the last steps of a run --
    whose gain is far below a float64 ulp of f -- still see f ordered as it is."""
    X, y = LA.make_problem(kind, D, n_data, seed)
    oracle = LA.GLMOracle(kind, X, y, prior_sd=3.0, noise_sd=0.7, dtype=dtype)
    return _hooked(vb, D, oracle.value_grad_hessian), oracle, X, y


# ---- exports and signatures ---------------------------------------------------------------------------------------------
def test_exports_and_signatures(vb):
    from viabel_amd import _lib, convenience
    assert 'laplace_approximation' in convenience.__all__ and hasattr(vb, 'laplace_approximation')
    assert list(inspect.signature(vb.laplace_approximation).parameters) == ['model', 'x0', 'max_iter', 'tol', 'seed', 'rng']
    sig = inspect.signature(vb.laplace_approximation).parameters
    assert (sig['x0'].default, sig['max_iter'].default, sig['tol'].default, sig['seed'].default, sig['rng'].default) == \
        (None, 100, 1e-10, 1, 'numpy')
    assert list(inspect.signature(vb.DeviceModel.find_mode).parameters) == ['self', 'x0', 'max_iter', 'tol']
    assert list(inspect.signature(vb.DeviceModel.hessian).parameters) == ['self', 'x']
    assert list(inspect.signature(vb.DeviceModel._value_grad_hessian).parameters) == ['self', 'x', 'want_hessian']
    assert list(inspect.signature(_lib.Engine.glm_value_grad_hessian).parameters) == ['self', 'x', 'want_hessian']
    for cls in (vb.LogisticRegressionModel, vb.GaussianModel, vb.CorrelatedGaussianModel):
        assert cls.hessian is not vb.DeviceModel.hessian
    assert vb.PoissonRegressionModel.hessian is vb.LogisticRegressionModel.hessian
    assert vb.LinearRegressionModel._value_grad_hessian is vb.LogisticRegressionModel._value_grad_hessian
    for cls in (vb.SoftmaxRegressionModel, vb.MultilevelRegressionModel, vb.LocationScaleRegressionModel,
                vb.SparseRegressionModel, vb.SourceModel, vb.CallableModel, vb.FunnelModel):
        assert cls.hessian is vb.DeviceModel.hessian
    restype, argtypes = _lib.SIGNATURES['vb_glm_value_grad_hessian']
    assert len(argtypes) == 6
    header = open(os.path.join(ROOT, 'include', 'viabel_hip.h')).read()
    decl = re.search(r'int\s+vb_glm_value_grad_hessian\s*\(([^)]*)\)', header)
    assert decl and len(decl.group(1).split(',')) == 6
    assert 'vb_glm_hessian.hip' in open(os.path.join(ROOT, 'viabel_amd', 'csrc', 'Makefile')).read()


def test_null_context_is_an_error_not_a_crash(vb):
    from viabel_amd import _lib
    lib = _lib.load()
    assert lib.vb_glm_value_grad_hessian(None, None, 0, None, None, None) == _lib.VB_ERR_INVALID


def test_host_hessians_of_the_gaussian_targets(vb):
    rng = np.random.RandomState(0)
    sd = 0.5 + rng.rand(5)
    g = vb.GaussianModel(rng.randn(5), sd)
    assert np.array_equal(g.hessian(np.zeros(5)), -np.diag(1 / sd ** 2))
    assert g.hessian(np.zeros((3, 5))).shape == (3, 5, 5)
    A = rng.randn(5, 5)
    P = A @ A.T + np.eye(5)
    c = vb.CorrelatedGaussianModel(rng.randn(5), precision=P)
    assert np.array_equal(c.hessian(np.ones(5)), -c.precision)
    assert np.array_equal(c.hessian(np.ones((2, 5)))[1], -c.precision)
    with pytest.raises(ValueError):
        g.hessian(np.zeros(4))


# ---- validation, before any engine ----------------------------------------------------------------------------------------
def test_validation_errors_come_before_the_engine(vb):
    X, y = LA.make_problem('logistic', 4, 9, 0)
    model = vb.LogisticRegressionModel(X, y)
    for kwargs in (dict(x0=np.zeros(5)), dict(x0=np.zeros((1, 4))), dict(max_iter=0), dict(max_iter=-3), dict(tol=0.0),
                   dict(tol=-1e-3)):
        with pytest.raises(ValueError):
            model.find_mode(**kwargs)
        with pytest.raises(ValueError):
            vb.laplace_approximation(model, **kwargs)
    big = vb.SparseRegressionModel(([], [], np.zeros(2, dtype=np.int64)), np.zeros(1), shape=(1, 4097))
    with pytest.raises(NotImplementedError, match='4096'):
        big.hessian(np.zeros(4097))
    with pytest.raises(TypeError):
        vb.laplace_approximation(vb.Model(lambda x: -0.5 * np.sum(x * x, axis=-1)))
    with pytest.raises(TypeError):
        vb.laplace_approximation(lambda x: x)


# ---- the Newton driver ------------------------------------------------------------------------------------------------
def test_a_quadratic_is_solved_in_one_step(vb):
    rng = np.random.RandomState(1)
    A = rng.randn(6, 6)
    P = A @ A.T + np.eye(6)
    m = rng.randn(6)
    model = _hooked(vb, 6, lambda x, want: (float(-0.5 * (x - m) @ P @ (x - m)), -P @ (x - m), -P if want else None))
    res = model.find_mode()
    assert res['n_iter'] == 1 and res['converged']
    assert np.max(np.abs(res['mode'] - m)) <= 1e-13 * max(1.0, np.max(np.abs(m))) * np.linalg.cond(P)
    assert set(res) == {'mode', 'value', 'grad', 'hessian', 'n_iter', 'converged'}
    assert np.array_equal(res['hessian'], -P)


@pytest.mark.parametrize('kind', ['logistic', 'poisson'])
def test_glm_reaches_the_oracle_mode_and_never_goes_down(vb, kind):
    model, oracle, X, y = _glm(vb, kind)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        res = model.find_mode()
    ref = LA.newton(oracle.value_grad_hessian, np.zeros(7))
    assert res['converged'] and ref['converged']
    # the same rules on the same function: the same iterates
    assert res['n_iter'] == ref['n_iter'] and np.array_equal(res['mode'], ref['mode'])
    g0 = np.max(np.abs(oracle.grad(np.zeros(7))))
    assert np.max(np.abs(np.asarray(oracle.grad(res['mode']), dtype=float))) <= 1e-8 * g0
    # an independent statement of the mode: the gradient in long double vanishes to the rounding of its float64 inputs
    H = np.asarray(oracle.hessian(res['mode']), dtype=float)
    err = np.linalg.solve(-H, np.asarray(oracle.grad(res['mode']), dtype=float))
    assert np.max(np.abs(err)) <= 1e-13 * max(1.0, np.max(np.abs(res['mode'])))
    iterates = [f for _, f, want in model.calls if want]
    assert len(iterates) >= 3 and all(b >= a for a, b in zip(iterates, iterates[1:])), iterates
    assert res['value'] == iterates[-1]


def test_a_far_poisson_start_engages_the_backtracking(vb):
    # an intercept column, and a start that puts every linear predictor at -8: all means are e^-8, the likelihood's curvature
    # is nothing beside the prior's 1 / 9, and the Newton step ~ 9 X'y lands where exp(eta) is astronomic
    X, y = LA.make_problem('poisson', 7, 33, 5)
    X[:, 0] = 1.0
    oracle = LA.GLMOracle('poisson', X, y, prior_sd=3.0, dtype=np.longdouble)
    model = _hooked(vb, 7, oracle.value_grad_hessian)
    x0 = np.zeros(7)
    x0[0] = -8.0
    trace = []
    ref = LA.newton(oracle.value_grad_hessian, x0, trace=trace)
    assert max(h for _, _, _, h in trace) >= 1
    res = model.find_mode(x0=x0)
    calls = list(model.calls)
    assert res['converged'] and np.array_equal(res['mode'], ref['mode']) and res['n_iter'] == ref['n_iter']
    iterates = [f for _, f, want in calls if want]
    assert all(b >= a for a, b in zip(iterates, iterates[1:]))
    # the halved trials are value-only evaluations: more of those than of full ones
    assert sum(1 for c in calls if not c[2]) > sum(1 for c in calls if c[2])
    near = model.find_mode()
    assert np.max(np.abs(res['mode'] - near['mode'])) <= 1e-9


def test_a_double_well_takes_the_ridge_branch(vb):
    def hook(x, want):
        u = x[0]
        return float(-(u * u - 1.0) ** 2), np.array([-4.0 * u * (u * u - 1.0)]), np.array([[-(12.0 * u * u - 4.0)]]) if want else None
    model = _hooked(vb, 1, hook)
    assert hook(np.array([0.1]), True)[2][0, 0] > 0      # -H is negative there: no Cholesky without a ridge
    res = model.find_mode(x0=np.array([0.1]))
    assert res['converged'] and abs(abs(res['mode'][0]) - 1.0) <= 1e-12
    assert res['mode'][0] > 0                             # ascent from 0.1 goes to +1
    assert res['n_iter'] > 2


def test_an_unbounded_density_ends_unconverged_with_a_warning(vb):
    model = _hooked(vb, 1, lambda x, want: (float(x[0]), np.ones(1), np.zeros((1, 1)) if want else None))
    with pytest.warns(RuntimeWarning, match='without converging'):
        res = model.find_mode(max_iter=20)
    assert res['converged'] is False and res['n_iter'] == 20 and res['mode'][0] > 0
    with pytest.warns(RuntimeWarning):
        res = vb.DeviceModel.find_mode(model, max_iter=1)
    assert res['n_iter'] == 1 and not res['converged']


# ---- assembly ---------------------------------------------------------------------------------------------------------
def test_assembly_and_linear_evidence(vb):
    X, y = LA.make_problem('linear', 7, 33, 11)
    oracle = LA.GLMOracle('linear', X, y, prior_sd=3.0, noise_sd=0.7)
    model = _hooked(vb, 7, oracle.value_grad_hessian)
    res = vb.laplace_approximation(model, seed=4)
    assert set(res) == {'mode', 'hessian', 'n_iter', 'converged', 'cov', 'approx', 'var_param', 'log_evidence'}
    assert res['converged'] and res['n_iter'] == 1
    assert isinstance(res['approx'], vb.FullRankGaussian) and res['approx'].dim == 7
    mean, cov = res['approx'].mean_and_cov(res['var_param'])
    assert np.max(np.abs(mean - res['mode'])) <= 1e-12 * np.max(np.abs(res['mode']))
    assert np.max(np.abs(cov - res['cov'])) <= 1e-12 * np.max(np.abs(res['cov']))
    assert np.array_equal(res['cov'], res['cov'].T)
    ref_mean, ref_cov, _, log_ev = LA.conjugate_linear(X, y, 3.0, 0.7)
    assert abs(res['log_evidence'] - log_ev) <= 1e-9 * max(abs(log_ev), 1.0), (res['log_evidence'], log_ev)
    assert np.max(np.abs(res['mode'] - ref_mean)) <= 1e-12 * np.max(np.abs(ref_mean)) * np.linalg.cond(ref_cov)
    assert np.max(np.abs(res['cov'] - ref_cov)) <= 1e-12 * np.max(np.abs(ref_cov)) * np.linalg.cond(ref_cov)
    # seed and rng reach the family
    assert vb.laplace_approximation(model, seed=9, rng='philox')['approx'].rng == 'philox'


def test_a_saddle_raises(vb):
    S = np.diag([-1.0, 2.0])      # f = x' S x / 2: a saddle at the origin, where the search starts and stays (gradient 0)
    model = _hooked(vb, 2, lambda x, want: (float(0.5 * x @ S @ x), S @ x, S if want else None))
    with pytest.raises(ValueError, match='positive definite'):
        vb.laplace_approximation(model)
