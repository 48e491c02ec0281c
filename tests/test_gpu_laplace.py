"""GPU: the Laplace approximation -- vb_glm_value_grad_hessian (csrc/vb_glm_hessian.hip: the link pass, the lower-triangular
Gram product, the finishing kernel) through Engine.glm_value_grad_hessian and the models' hessian(), the Newton mode finder
on the device, laplace_approximation() into the objectives and the diagnostics, and the difference route of the other
device models -- against the numpy oracle of tests/_laplace_oracle.py and the rows targets' own oracles.  Tolerances are the
project's for the same kinds of quantity (value 1e-12, gradient 1e-11 relative), or are derived in the test from them."""
import warnings

import numpy as np
import pytest

import _golden as G
import _laplace_oracle as LA
import _loo_oracle as LO
from oracle import families as ofam, psis as opsis

pytestmark = pytest.mark.gpu

PRIOR_SD, NOISE_SD = 3.0, 0.7


@pytest.fixture(scope='module')
def vb():
    import viabel_amd
    from viabel_amd import _lib
    _lib.default_engine()
    return viabel_amd


def _device_model(vb, kind, X, y):
    if kind == 'logistic':
        return vb.LogisticRegressionModel(X, y, PRIOR_SD)
    if kind == 'poisson':
        return vb.PoissonRegressionModel(X, y, PRIOR_SD)
    return vb.LinearRegressionModel(X, y, PRIOR_SD, NOISE_SD)


_PROBLEMS = {}


def _problem(vb, kind, D, n_data, scale=None):
    """(device model, oracle, X, y); built once per case and shared."""
    key = (kind, D, n_data, scale)
    if key not in _PROBLEMS:
        X, y = LA.make_problem(kind, D, n_data, 1000 * LA.KINDS.index(kind) + 7 * D + n_data, scale=scale, noise_sd=NOISE_SD)
        _PROBLEMS[key] = (_device_model(vb, kind, X, y), LA.GLMOracle(kind, X, y, PRIOR_SD, NOISE_SD), X, y)
    return _PROBLEMS[key]


def _points(X, D, seed):
    """zero; 0.3 randn; one scaled so that max|eta| is about 30."""
    rng = np.random.RandomState(seed)
    x1, x2 = 0.3 * rng.randn(D), rng.randn(D)
    x2 *= 30.0 / max(np.max(np.abs(X @ x2)), 1e-300)
    return [np.zeros(D), x1, x2]


# ---- 1. the entry against numpy ---------------------------------------------------------------------------------------------
# D: one lane, ragged pads, exactly one 16-stride, 1 / 2 / 3 tile rows of the triangle; n_data: below and above one split of
# 256 and one 32-row block of the link pass, not a multiple of 16; (16, 70 001): many splits and a ragged tail
GRID = [(D, n) for D in (1, 7, 16, 33, 200, 300) for n in (1, 5, 300, 1031)] + [(16, 70001)]
# ... and the link pass's other register tilings (2, 4, 8, 16 column pairs per thread: D above 512, 1024, 2048, 4096), two row
# blocks each
WIDE = [(520, 40), (1030, 40), (2100, 40), (4100, 40)]


def _check_entry(vb, kind, D, n_data):
    from viabel_amd import _lib
    model, oracle, X, y = _problem(vb, kind, D, n_data)
    eng = _lib.default_engine()
    eng.set_model(model.device_spec())
    for k, x in enumerate(_points(X, D, D + n_data)):
        f, g, H = eng.glm_value_grad_hessian(x)
        rf, rg, rH = oracle.value(x), oracle.grad(x), oracle.hessian(x)
        errs = (G.rel_err(f, rf), G.rel_err(g, rg), G.rel_err(H, rH))
        print('%s D=%d n=%d point %d: rel err f %.1e g %.1e H %.1e' % ((kind, D, n_data, k) + errs))
        assert errs[0] < 1e-12 and errs[1] < 1e-11 and errs[2] < 1e-12, (kind, D, n_data, k, errs)
        assert np.array_equal(H, H.T)
        f2, g2, H2 = eng.glm_value_grad_hessian(x)
        assert f2 == f and np.array_equal(g2, g) and np.array_equal(H2, H)
        f3, g3, H3 = eng.glm_value_grad_hessian(x, want_hessian=False)
        assert H3 is None and f3 == f and np.array_equal(g3, g)
        if k == 2 and kind != 'linear':        # max|eta| ~ 30: logistic weights ~1e-13, Poisson weights ~1e13
            # H_jj = -(sum_i w_i x_ij^2) - 1 / sd^2 in that order: at or below -1 / sd^2 exactly iff the weighted sum is >= 0
            assert np.all(np.isfinite(H)) and np.all(np.diag(H) <= -1.0 / PRIOR_SD ** 2)
            assert abs(np.max(np.abs(X @ x)) - 30.0) < 1e-9
            assert np.max(np.abs(np.log(oracle.weights(x)))) > 29.0      # (the one-observation cases may have eta = -30)


@pytest.mark.parametrize('D,n_data', GRID)
@pytest.mark.parametrize('kind', LA.KINDS)
def test_entry_against_numpy(vb, kind, D, n_data):
    _check_entry(vb, kind, D, n_data)


@pytest.mark.parametrize('D,n_data', WIDE)
def test_entry_against_numpy_wide_rows(vb, D, n_data):
    _check_entry(vb, 'logistic', D, n_data)


def test_model_hessian_shapes(vb):
    model, oracle, X, y = _problem(vb, 'poisson', 7, 300)
    x = 0.2 * np.random.RandomState(3).randn(3, 7)
    H = model.hessian(x)
    assert H.shape == (3, 7, 7) and model.hessian(x[1]).shape == (7, 7)
    assert np.array_equal(H[1], model.hessian(x[1]))
    for n in range(3):
        assert G.rel_err(H[n], oracle.hessian(x[n])) < 1e-12
    f, g, Hh = model._value_grad_hessian(x[2])
    assert np.array_equal(Hh, H[2])
    assert G.rel_err(g, model.grad(x[2])) < 1e-11 and G.rel_err(f, model(x[2])[0]) < 1e-12      # vb_model_grad / vb_model_logp


# ---- 2. workspace reuse ------------------------------------------------------------------------------------------------------
def test_small_call_after_a_large_one(vb):
    from viabel_amd import _lib
    big, _, Xb, _ = _problem(vb, 'logistic', 300, 1031)
    small, oracle, Xs, _ = _problem(vb, 'logistic', 7, 5)
    xs = _points(Xs, 7, 1)[1]
    eng = _lib.default_engine()
    eng.set_model(big.device_spec())
    eng.glm_value_grad_hessian(_points(Xb, 300, 2)[1])
    eng.set_model(small.device_spec())
    after = eng.glm_value_grad_hessian(xs)
    fresh = _lib.Engine()
    try:
        fresh.set_model(small.device_spec())
        first = fresh.glm_value_grad_hessian(xs)
    finally:
        fresh.close()
    assert after[0] == first[0] and np.array_equal(after[1], first[1]) and np.array_equal(after[2], first[2])
    assert G.rel_err(after[2], oracle.hessian(xs)) < 1e-12


# ---- 3. find_mode against the oracle's Newton ----------------------------------------------------------------------------------
@pytest.mark.parametrize('D,n_data', [(7, 33), (50, 200), (200, 1031)])
@pytest.mark.parametrize('kind', LA.KINDS)
def test_find_mode_against_oracle_newton(vb, kind, D, n_data):
    model, oracle, X, y = _problem(vb, kind, D, n_data)
    ref = LA.newton(oracle.value_grad_hessian, np.zeros(D))
    g0 = float(np.max(np.abs(oracle.grad(np.zeros(D)))))
    assert ref['converged'] and np.max(np.abs(oracle.grad(ref['mode']))) <= 1e-8 * g0      # the oracle run meets the cap
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        res = model.find_mode()
    assert res['converged']
    # the project's gradient parity (1e-11 of the largest gradient met) carried through the Newton map
    bound = np.max(np.sum(np.abs(np.linalg.inv(-ref['hessian'])), axis=1)) * 1e-11 * g0
    err = float(np.max(np.abs(res['mode'] - ref['mode'])))
    gm = float(np.max(np.abs(model.grad(res['mode']))))
    print('%s D=%d n=%d: n_iter %d (oracle %d), mode error %.2e (bound %.2e), max|grad| at the mode %.2e (cap %.2e)'
          % (kind, D, n_data, res['n_iter'], ref['n_iter'], err, bound, gm, 1e-8 * g0))
    assert err <= bound
    assert gm <= 1e-8 * g0
    if kind == 'linear':
        assert res['n_iter'] == 1
        mean = LA.conjugate_linear(X, y, PRIOR_SD, NOISE_SD)[0]
        assert np.max(np.abs(res['mode'] - mean)) <= bound


# ---- 4. the Laplace approximation of a linear model is exact ------------------------------------------------------------------
def test_linear_laplace_is_exact(vb):
    D, n_data = 12, 90
    model, oracle, X, y = _problem(vb, 'linear', D, n_data, scale=1.0)
    mean, cov, prec, log_ev = LA.conjugate_linear(X, y, PRIOR_SD, NOISE_SD)
    cond = np.linalg.cond(prec)
    print('condition number of the precision matrix: %.1f' % cond)
    assert cond < 1e3
    res = vb.laplace_approximation(model, seed=3)
    assert res['converged'] and res['n_iter'] == 1
    assert G.rel_err(res['cov'], cov) < 1e-9
    assert abs(res['log_evidence'] - log_ev) <= 1e-9 * max(abs(log_ev), 1.0), (res['log_evidence'], log_ev)
    value, grad = vb.ExclusiveKL(res['approx'], model, 64, use_path_deriv=True)(res['var_param'])
    assert abs(value + log_ev) <= 1e-9 * max(abs(log_ev), 1.0), (value, -log_ev)
    scale = np.max(np.abs(X.T @ y)) / NOISE_SD ** 2 + 1.0
    assert np.max(np.abs(grad)) <= 1e-9 * scale, np.max(np.abs(grad))


# ---- 5. Laplace into the diagnostics -------------------------------------------------------------------------------------------
KHAT_SEED = 0


def _khat_problem():
    return LA.make_problem('logistic', 10, 300, KHAT_SEED)


def _khat_numpy(X, y, seed, n_samples=4096):
    """The pipeline in numpy: the oracle's mode and Hessian, numpy ``randn`` of the family's seed, oracle/psis.py."""
    oracle = LA.GLMOracle('logistic', X, y, PRIOR_SD)
    ref = LA.newton(oracle.value_grad_hessian, np.zeros(10))
    cov = np.linalg.inv(-ref['hessian'])
    fam = ofam.FullRankGaussian(10)
    theta = fam.pack(ref['mode'], np.linalg.cholesky(0.5 * (cov + cov.T)))
    z = fam.sample_from_noise(theta, np.random.RandomState(seed).randn(n_samples, 10))
    lw = np.array([oracle.value(row) for row in z]) - fam.log_density(theta, z)
    return float(opsis.psis_smooth(lw)[1])


def test_laplace_into_the_diagnostics(vb):
    """Logistic regression, n_data = 300, D = 10.  With data seed KHAT_SEED = 0 the pipeline in numpy (the oracle's mode,
    numpy ``randn`` of the family's seed 6, oracle/psis.py) gives k-hat = 0.1418 (checked without a GPU; seeds 1, 2, 3 give
    0.209, 0.332, 0.274): below 0.5, so the device run must come out below 0.7 and agree with it."""
    from viabel_amd._psis import psislw
    X, y = _khat_problem()
    model = vb.LogisticRegressionModel(X, y, PRIOR_SD)
    res = vb.laplace_approximation(model, seed=6)
    samples, lw = vb.samples_and_log_weights(res['var_param'], model, res['approx'], 4096)
    khat = float(psislw(lw)[1])
    ref = _khat_numpy(X, y, 6)
    print('k-hat: device %.12f, numpy %.12f' % (khat, ref))
    assert ref < 0.5
    assert khat < 0.7
    assert LO.close_k(khat, ref)
    out = vb.vi_diagnostics(res['var_param'], model=model, approx=res['approx'], n_samples=4096)
    assert out['khat'] < 0.7 and 'd2' in out


def test_laplace_starts_bbvi_and_feeds_loo_and_predict(vb, capsys):
    X, y = _khat_problem()
    model = vb.LogisticRegressionModel(X, y, PRIOR_SD)
    res = vb.laplace_approximation(model, seed=6)
    fit = vb.bbvi(10, n_iters=20, num_mc_samples=32, log_density=model, approx=res['approx'],
                  init_var_param=res['var_param'], adaptive=False, fixed_lr=True, learning_rate=1e-4)
    assert np.all(np.isfinite(fit['opt_param'])) and np.max(np.abs(fit['opt_param'][:10] - res['mode'])) < 0.05
    loo = vb.loo(res['var_param'], model=model, approx=res['approx'], n_samples=1000)
    assert np.isfinite(loo['elpd_loo']) and loo['khat_full'] < 0.7
    pred = vb.predict(res['var_param'], model=model, approx=res['approx'], n_samples=1000)
    assert np.all((pred['mean'] > 0) & (pred['mean'] < 1))
    capsys.readouterr()


# ---- 6. the difference route on the device --------------------------------------------------------------------------------------
def _rows_target(vb, name):
    """(device model, its test module's oracle) at that module's small size."""
    if name == 'softmax':
        import test_gpu_softmax as T
        return T._problem(vb, *T.SMALL[:3])
    if name == 'multilevel':
        import test_gpu_multilevel as T
        return T._shape_problem(vb, T.SMALL)
    if name == 'locscale':
        import test_gpu_locscale as T
        return T._shape_problem(vb, T.SMALL)
    if name == 'sparse':
        import test_gpu_sparse_glm as T
        return T._problem(vb, 'odd', 'poisson')[:2]
    import test_gpu_source_model as T
    return T._problem(vb, 7, 40)


@pytest.mark.parametrize('name', ['softmax', 'multilevel', 'locscale', 'sparse', 'source'])
def test_difference_route_on_the_device(vb, name):
    model, oracle = _rows_target(vb, name)
    D = model.dim
    assert type(model).hessian is vb.DeviceModel.hessian
    for seed, scale in ((0, 0.0), (1, 0.3), (2, 1.5)):
        x = scale * np.random.RandomState(seed).randn(D)
        H = model.hessian(x)
        H_np, gmax = LA.stencil_hessian(oracle.grad, x)
        # the project's gradient parity (1e-11 of the largest gradient met) through the stencil's coefficients (8 + 8 + 1 + 1) / 12 h
        bound = (1.5 / LA.stencil_step(x)) * 1e-11 * gmax
        H_exact = oracle.hessian(x)
        own = float(np.max(np.abs(H_np - H_exact)))
        print('%s D=%d |x| scale %.1f: device against the numpy stencil %.2e (bound %.2e), against the analytic Hessian %.2e, '
              'numpy stencil against analytic %.2e' % (name, D, scale, np.max(np.abs(H - H_np)), bound,
                                                       np.max(np.abs(H - H_exact)), own))
        assert H.shape == (D, D) and np.array_equal(H, H.T)
        assert np.max(np.abs(H - H_np)) <= bound
        assert np.max(np.abs(H - H_exact)) <= bound + own
    assert model.hessian(np.zeros((2, D))).shape == (2, D, D)


def test_find_mode_multilevel(vb):
    model, oracle = _rows_target(vb, 'multilevel')
    D = model.dim
    x0 = np.zeros(D)
    g0 = float(np.max(np.abs(oracle.grad(x0))))

    def hook(x, want):      # the oracle's Newton with the stencil Hessian: the run the device repeats
        return float(oracle.logp(x)[0]), oracle.grad(x)[0], LA.stencil_hessian(oracle.grad, x)[0] if want else None
    ref = LA.newton(hook, x0)
    assert ref['converged'] and np.max(np.abs(oracle.grad(ref['mode']))) <= 1e-8 * g0
    res = model.find_mode()
    gm = float(np.max(np.abs(oracle.grad(res['mode']))))
    print('multilevel D=%d: n_iter %d (oracle %d), oracle gradient at the device mode %.2e (cap %.2e), modes differ by %.2e'
          % (D, res['n_iter'], ref['n_iter'], gm, 1e-8 * g0, np.max(np.abs(res['mode'] - ref['mode']))))
    assert res['converged']
    assert gm <= 1e-8 * g0
    lap = vb.laplace_approximation(model)
    assert lap['converged'] and np.array_equal(lap['mode'], res['mode']) and np.isfinite(lap['log_evidence'])


# ---- 7. errors ----------------------------------------------------------------------------------------------------------------
def test_errors(vb):
    from viabel_amd import _lib
    fresh = _lib.Engine()
    try:
        with pytest.raises(_lib.EngineError):                               # no model bound
            fresh.glm_value_grad_hessian(np.zeros(3))
        fresh.set_model(vb.GaussianModel(np.zeros(3), np.ones(3)).device_spec())
        with pytest.raises(NotImplementedError):                            # bound, but not a flat regression target
            fresh.glm_value_grad_hessian(np.zeros(3))
        assert np.allclose(fresh.model_logp(np.zeros((1, 3))), -1.5 * np.log(2 * np.pi))
    finally:
        fresh.close()
    model, oracle, X, y = _problem(vb, 'logistic', 7, 33)
    eng = _lib.default_engine()
    eng.set_model(model.device_spec())
    with pytest.raises(ValueError):                                         # wrong d
        eng.glm_value_grad_hessian(np.zeros(8))
    with pytest.raises(ValueError):
        eng.glm_value_grad_hessian(np.zeros((1, 7)))
    x = _points(X, 7, 0)[1]
    assert G.rel_err(eng.glm_value_grad_hessian(x)[2], oracle.hessian(x)) < 1e-12      # the bound model still evaluates
    assert G.rel_err(model(x)[0], oracle.value(x)) < 1e-12
    # beyond the capacity of the link pass: refused, and the model stays usable
    wide = vb.LogisticRegressionModel(np.ones((1, 8200)) / 8200.0, np.ones(1))
    eng.set_model(wide.device_spec())
    with pytest.raises(NotImplementedError, match='8192'):
        eng.glm_value_grad_hessian(np.zeros(8200))
    assert np.isfinite(wide(np.zeros(8200))[0])
