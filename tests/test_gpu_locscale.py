"""LocationScaleRegressionModel (VB_MODEL_LOCSCALE, csrc/vb_locscale.hip) on the GPU against the numpy oracle of
tests/_locscale_oracle.py: the row pipeline (two predictor GEMMs, the staged scale block, link kernel, two gradient GEMMs, row
sums; the constant-scale route without the second design), and the target under every objective x family route a SourceModel
takes (tests/test_gpu_multilevel.py is the template, with its tolerances: value 1e-12, gradient 1e-11 relative, 1e-10 / 1e-9
where the source-model, softmax and multilevel tests of the same route use them)."""
import numpy as np
import pytest

import _golden as G
from _locscale_oracle import LocScaleOracle
from oracle import families as ofam, objectives as oobj

pytestmark = pytest.mark.gpu

# (likelihood, p, q, n_data, N): D = 5 with a scale design, D = 64 with a constant scale (q = None)
SMALL, LARGE = ('student_t', 2, 3, 30, 100), ('gaussian', 63, None, 400, 333)
SHAPES = [SMALL, LARGE]


@pytest.fixture(scope='module')
def vb():
    import viabel_amd
    from viabel_amd import _lib
    _lib.default_engine()
    return viabel_amd


_PROBLEMS = {}


def _problem(vb, lik, p, q, n_data, df=4.5, prior_sd=3.0, scale_prior_sd=0.8, ones=False):
    """(device model, oracle) on X = randn / sqrt(p), W = randn / sqrt(q) (q = None: the constant scale; `ones`: q = 1 with an
    explicit column of ones), y simulated with coefficients of scale 0.3 and log-scales of scale 0.3; built once per shape and
    shared."""
    key = (lik, p, q, n_data, ones)
    if key not in _PROBLEMS:
        rng = np.random.RandomState(1000 * (q or 0) + 10 * p + n_data)
        X = rng.randn(n_data, p) / np.sqrt(p)
        W = None if q is None else rng.randn(n_data, q) / np.sqrt(q)
        s = 0.3 * rng.randn() if q is None else W @ (0.3 * rng.randn(q))
        noise = rng.standard_t(df, size=n_data) if lik == 'student_t' else rng.randn(n_data)
        y = X @ (0.3 * rng.randn(p)) + np.exp(s) * noise
        if ones:
            W = np.ones((n_data, 1))
        args = (X, y, W, lik, df, prior_sd, scale_prior_sd)
        _PROBLEMS[key] = (vb.LocationScaleRegressionModel(*args), LocScaleOracle(*args))
    return _PROBLEMS[key]


def _shape_problem(vb, shape):
    return _problem(vb, *shape[:4])


def _round_up(x, m):
    return (x + m - 1) // m * m


def _oracle_rows(omodel, x):
    """f, gradient and per-observation terms of the oracle in slices of 512 rows (its (rows, n_data) temporaries, bounded)."""
    rows = x.shape[0]
    fo, go, po = np.empty(rows), np.empty((rows, omodel.dim)), np.empty((rows, omodel.n_data))
    for r0 in range(0, rows, 512):
        s = slice(r0, r0 + 512)
        fo[s], go[s], po[s] = omodel.logp(x[s]), omodel.grad(x[s]), omodel.pointwise(x[s])
    return fo, go, po


# ---- 1. rows ---------------------------------------------------------------------------------------------------------
def _rows_cases():
    from viabel_amd import _lib
    chunk = max(8, _lib.LOCSCALE_CHUNK_DOUBLES // (2 * _round_up(2500, 16)))
    return [('gaussian', 1, None, 1, 1), ('student_t', 5, 3, 33, 100), ('gaussian', 17, None, 130, 257),
            ('student_t', 16, 40, 300, 64), ('gaussian', 3, 2, 2500, 2 * chunk + 5)]


@pytest.mark.parametrize('lik,p,q,n_data,rows', _rows_cases())
def test_rows_against_oracle(vb, lik, p, q, n_data, rows):
    """model(x), model.grad(x), pointwise_log_likelihood(x).  (1, None, 1): the smallest shape, constant scale; (5, 3): odd p,
    so the scale block starts at an odd column of Z and G (the staged copy is what the products see), odd q; p = 17 with a
    constant scale: the coefficient gradient's last column is a single store next to the scale entry the row-sum kernel
    writes; n_data = 300: the split branch of the gradient GEMM, taken by both gradient products; the last case: three row
    chunks (two full ones and a remainder) and several strips of the link kernel."""
    from viabel_amd import _lib
    if n_data == 2500:
        chunk = max(8, _lib.LOCSCALE_CHUNK_DOUBLES // (2 * _round_up(n_data, 16)))
        assert 2 * chunk < rows <= 3 * chunk                      # exactly three chunks
    model, omodel = _problem(vb, lik, p, q, n_data)
    assert model.dim == p + (q or 1) == omodel.dim
    x = 0.3 * np.random.RandomState(rows).randn(rows, model.dim)
    fo, go, po = _oracle_rows(omodel, x)
    f, g, pw = model(x), model.grad(x), model.pointwise_log_likelihood(x)
    assert f.shape == (rows,) and g.shape == (rows, model.dim) and pw.shape == (rows, n_data)
    ef, eg, ep = G.rel_err(f, fo), G.rel_err(g, go), G.rel_err(pw, po)
    print('rows %s p=%d q=%s n_data=%d rows=%d: rel err f %.2e grad %.2e pointwise %.2e' % (lik, p, q, n_data, rows, ef, eg, ep))
    assert ef < 1e-12 and eg < 1e-11 and ep < 1e-12, (ef, eg, ep)
    assert model.check_gradient(x[:3]) < 1e-6
    assert np.array_equal(model(x), f) and np.array_equal(model.grad(x), g)        # no atomics: the same bits
    assert np.array_equal(model.pointwise_log_likelihood(x), pw)
    assert model(x[0]).shape == (1,) and model.grad(x[0]).shape == (model.dim,)
    assert model.pointwise_log_likelihood(x[0]).shape == (1, n_data)


# ---- 2. the constant scale against an explicit column of ones --------------------------------------------------------
@pytest.mark.parametrize('lik', ['gaussian', 'student_t'])
def test_constant_scale_matches_a_column_of_ones(vb, lik):
    """W=None (one s per row, the scale gradient from strip partials) and W = ones (the second pair of products) are the same
    density; the two routes sum in different orders, so agreement to 1e-13, not bit equality."""
    p, n_data = 7, 1300                                           # two strips, the split branch of the gradient products
    const, _ = _problem(vb, lik, p, None, n_data)
    ones, _ = _problem(vb, lik, p, None, n_data, ones=True)
    assert const.W is None and ones.W.shape == (n_data, 1) and const.dim == ones.dim == p + 1
    np.testing.assert_array_equal(const.y, ones.y)
    x = 0.3 * np.random.RandomState(3).randn(50, const.dim)
    ef, eg = G.rel_err(const(x), ones(x)), G.rel_err(const.grad(x), ones.grad(x))
    ep = G.rel_err(const.pointwise_log_likelihood(x), ones.pointwise_log_likelihood(x))
    print('constant scale vs ones %s: rel err f %.2e grad %.2e pointwise %.2e' % (lik, ef, eg, ep))
    assert ef < 1e-13 and eg < 1e-13 and ep < 1e-13, (ef, eg, ep)


# ---- 3. reduction to the flat target ---------------------------------------------------------------------------------
def test_fixed_scale_reduces_to_linear_regression(vb):
    p, n_data, s0 = 6, 45, 1.7
    model, omodel = _problem(vb, 'gaussian', p, None, n_data)
    flat = vb.LinearRegressionModel(omodel.X, omodel.y, prior_sd=3.0, noise_sd=s0)
    theta = 0.3 * np.random.RandomState(4).randn(20, model.dim)
    theta[:, -1] = np.log(s0)
    b = np.ascontiguousarray(theta[:, :p])
    a, c = model.pointwise_log_likelihood(theta), flat.pointwise_log_likelihood(b)
    ga, gc = model.grad(theta)[:, :p], flat.grad(b)
    print('flat: rel err pointwise %.2e grad %.2e' % (G.rel_err(a, c), G.rel_err(ga, gc)))
    assert G.rel_err(a, c) < 1e-12, G.rel_err(a, c)
    assert G.rel_err(ga, gc) < 1e-11, G.rel_err(ga, gc)


# ---- 4. extreme scales -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lik,q', [('gaussian', 3), ('student_t', 3), ('gaussian', None), ('student_t', None)])
def test_extreme_scales_stay_finite(vb, lik, q):
    """max |s_i| = 30 (both signs among the rows, and with a scale design among the observations of a row) and
    max |eta_i| = 1e3: z^2 reaches 1e32 and exp(-s) 1e13, far from overflow, and no quotient degenerates."""
    p, n_data = 5, 33
    model, omodel = _problem(vb, lik, p, q, n_data)
    ol = LocScaleOracle(omodel.X, omodel.y, None if q is None else omodel.W, lik, 4.5, 3.0, 0.8, dtype=np.longdouble)
    x = np.random.RandomState(2).randn(40, model.dim)
    x[:, p:] *= 30.0 / np.max(np.abs(omodel.log_scale(x)))
    x[:, :p] *= 1e3 / np.max(np.abs(omodel.eta(x)))
    s = omodel.log_scale(x)
    assert 29.9 < np.max(s) <= 30.01 or 29.9 < -np.min(s) <= 30.01
    assert np.max(s) > 10 and np.min(s) < -10                     # both signs
    assert 999.0 < np.max(np.abs(omodel.eta(x))) < 1001.0
    f, g = model(x), model.grad(x)
    assert np.all(np.isfinite(f)) and np.all(np.isfinite(g))
    ef, eg = G.rel_err(f, ol.logp(x).astype(float)), G.rel_err(g, ol.grad(x).astype(float))
    print('extreme %s q=%s: rel err f %.2e grad %.2e' % (lik, q, ef, eg))
    assert ef < 1e-12 and eg < 1e-11, (ef, eg)


# ---- 5. ExclusiveKL --------------------------------------------------------------------------------------------------
def _mf_theta(D, seed):
    rng = np.random.RandomState(seed)
    return np.concatenate([0.3 * rng.randn(D), -1.0 + 0.1 * rng.randn(D)])


@pytest.mark.parametrize('shape', SHAPES, ids=['small', 'large'])
@pytest.mark.parametrize('rng_kind', ['numpy', 'philox'])
@pytest.mark.parametrize('pd', [False, True])
def test_exclusive_kl_meanfield(vb, shape, rng_kind, pd):
    from viabel_amd import _lib
    from viabel_amd.objectives import _NOISE_SLOT
    model, omodel = _shape_problem(vb, shape)
    D, N = model.dim, shape[4]
    theta = _mf_theta(D, D + N)
    for fam, ofamily in ((vb.MFGaussian(D, seed=5, rng=rng_kind), ofam.MFGaussian(D)),
                         (vb.MFStudentT(D, 8.0, seed=5, rng=rng_kind), ofam.MFStudentT(D, 8.0))):
        value, grad = vb.ExclusiveKL(fam, model, N, use_path_deriv=pd)(theta)
        if rng_kind == 'numpy':
            noise = ofamily.draw_noise(np.random.RandomState(5), N)
        else:                                                     # the device's draws, read back
            noise = _lib.default_engine().noise_get_host(_NOISE_SLOT, N, D)
        ov, og = oobj.exclusive_kl(ofamily, omodel, theta, noise, use_path_deriv=pd)
        ev, eg = G.rel_err(value, ov), G.rel_err(grad, og)
        print('ekl %s %s D=%d pd=%d: rel err value %.2e grad %.2e' % (type(fam).__name__, rng_kind, D, pd, ev, eg))
        assert ev < 1e-12, (type(fam).__name__, value, ov)
        assert eg < 1e-11, (type(fam).__name__, eg)


def _fr_theta(D, seed):
    rng = np.random.RandomState(seed)
    L = np.tril(0.05 * rng.randn(D, D), -1) + np.diag(np.exp(-1.0 + 0.2 * rng.randn(D)))
    return ofam.FullRankGaussian(D).pack(0.3 * rng.randn(D), L)


@pytest.mark.parametrize('shape', SHAPES, ids=['small', 'large'])
@pytest.mark.parametrize('pd', [False, True])
def test_exclusive_kl_fullrank(vb, shape, pd):
    model, omodel = _shape_problem(vb, shape)
    D, N = model.dim, shape[4]
    theta = _fr_theta(D, D)
    value, grad = vb.ExclusiveKL(vb.FullRankGaussian(D, seed=4), model, N, use_path_deriv=pd)(theta)
    noise = np.random.RandomState(4).randn(N, D)
    ov, og = oobj.exclusive_kl(ofam.FullRankGaussian(D), omodel, theta, noise, use_path_deriv=pd)
    ev, eg = G.rel_err(value, ov), G.rel_err(grad, og)
    print('ekl fullrank D=%d pd=%d: rel err value %.2e grad %.2e' % (D, pd, ev, eg))
    assert ev < 1e-12, (value, ov)
    assert eg < 1e-11, eg


@pytest.mark.parametrize('shape', SHAPES, ids=['small', 'large'])
@pytest.mark.parametrize('pd', [False, True])
def test_exclusive_kl_multivariate_t(vb, shape, pd):
    model, omodel = _shape_problem(vb, shape)
    D, N = model.dim, shape[4]
    rng = np.random.RandomState(D)
    B = rng.randn(D, D)
    theta = np.concatenate([0.3 * rng.randn(D), ofam.psd_to_free(0.05 * (B @ B.T / D + 0.5 * np.eye(D)))])
    value, grad = vb.ExclusiveKL(vb.MultivariateT(D, 9.0, seed=6), model, N, use_path_deriv=pd)(theta)
    noise = ofam.MultivariateT(D, 9.0).draw_noise(np.random.RandomState(6), N)
    ov, og = oobj.exclusive_kl(ofam.MultivariateT(D, 9.0), omodel, theta, noise, pd)
    print('ekl mvt D=%d pd=%d: rel err value %.2e grad %.2e' % (D, pd, G.rel_err(value, ov), G.rel_err(grad, og)))
    assert abs(value - ov) <= 1e-12 * abs(ov), (value, ov)
    np.testing.assert_allclose(grad, og, rtol=0, atol=1e-10 * np.max(np.abs(og)))      # (the source-model test's 1e-10)


@pytest.mark.parametrize('shape', SHAPES, ids=['small', 'large'])
def test_exclusive_kl_multivariate_t_philox(vb, shape):
    """rng='philox': samples through the Cholesky factor; the device's draws are read back and the estimator is written
    out by hand, as tests/test_gpu_objectives.py does for the built-in targets."""
    from viabel_amd import _lib
    from viabel_amd.objectives import _NOISE_SLOT
    model, omodel = _shape_problem(vb, shape)
    D, N, df = model.dim, shape[4], 9.0
    rng = np.random.RandomState(D + N)
    A = rng.randn(D, D)
    theta = np.concatenate([0.3 * rng.randn(D), ofam.psd_to_free(0.05 * (A @ A.T / D + np.eye(D)))])
    value, grad = vb.ExclusiveKL(vb.MultivariateT(D, df, seed=3, rng='philox'), model, N)(theta)
    eng = _lib.default_engine()
    chi, z = eng.chisq_get_host(N), eng.noise_get_host(_NOISE_SLOT, N, D)
    mu, L = theta[:D], ofam.free_to_chol(theta[D:], D)
    zs = z / np.sqrt(chi / df)[:, None]
    x = mu + zs @ L.T
    g = omodel.grad(x)
    ov = -(np.mean(omodel.logp(x)) + np.sum(np.log(np.diag(L))))
    dL = np.tril(g.T @ zs) / N
    dL[np.diag_indices(D)] = np.diag(dL) * np.diag(L) + 1.0
    og = -np.concatenate([g.mean(0), dL[np.tril_indices(D)]])
    print('ekl mvt philox D=%d: rel err value %.2e grad %.2e' % (D, G.rel_err(value, ov), G.rel_err(grad, og)))
    assert G.rel_err(value, ov) < 1e-12, (value, ov)
    assert G.rel_err(grad, og) < 1e-11, G.rel_err(grad, og)


@pytest.mark.parametrize('shape', SHAPES, ids=['small', 'large'])
@pytest.mark.parametrize('k', [1, 7, 20])
@pytest.mark.parametrize('pd', [False, True])
def test_exclusive_kl_lowrank(vb, shape, k, pd):
    """k = 20 takes the any-rank route (k > 16)."""
    model, omodel = _shape_problem(vb, shape)
    D, N = model.dim, shape[4]
    rng = np.random.RandomState(D + N + k)
    fam, ofamily = vb.LRGaussian(D, seed=7, k=k), ofam.LRGaussian(D, k)
    theta = fam.pack(0.3 * rng.randn(D), -1.0 + 0.1 * rng.randn(D), 0.2 * rng.randn(D, k) / np.sqrt(k))
    value, grad = vb.ExclusiveKL(fam, model, N, use_path_deriv=pd)(theta)
    noise = ofamily.draw_noise(np.random.RandomState(7), N)
    ov, og = oobj.exclusive_kl(ofamily, omodel, theta, noise, pd)
    print('ekl lr D=%d k=%d pd=%d: rel err value %.2e grad %.2e' % (D, k, pd, G.rel_err(value, ov), G.rel_err(grad, og)))
    assert G.rel_err(value, ov) < (1e-10 if pd else 1e-12), (value, ov)                # (the source-model test's bounds)
    assert G.rel_err(grad, og) < (1e-9 if pd else 1e-11), G.rel_err(grad, og)


def _torch_logp_of(omodel):
    """The same density in torch (the flow oracle differentiates it with autograd)."""
    import torch
    X, W = torch.from_numpy(np.asarray(omodel.X, dtype=float)), torch.from_numpy(np.asarray(omodel.W, dtype=float))
    y = torch.from_numpy(np.asarray(omodel.y, dtype=float))
    p, q, n, lik, nu = omodel.p, omodel.q, omodel.n_data, omodel.likelihood, float(omodel.df)
    sd, ssd = float(omodel.prior_sd), float(omodel.scale_prior_sd)
    l2pi = np.log(2.0 * np.pi)
    const = -p * (np.log(sd) + 0.5 * l2pi) - q * (np.log(ssd) + 0.5 * l2pi) + n * float(omodel.obs_const)

    def logp(x):
        b, g = x[:, :p], x[:, p:]
        s = g @ W.T
        z2 = ((y - b @ X.T) * torch.exp(-s)) ** 2
        ll = -s - (0.5 * (nu + 1.0) * torch.log1p(z2 / nu) if lik == 'student_t' else 0.5 * z2)
        return (torch.sum(ll, dim=1) - 0.5 * torch.sum(b * b, dim=1) / sd ** 2 - 0.5 * torch.sum(g * g, dim=1) / ssd ** 2
                + const)
    return logp


@pytest.mark.parametrize('shape', SHAPES, ids=['small', 'large'])
@pytest.mark.parametrize('pd', [False, True])
def test_exclusive_kl_nvp_flow(vb, shape, pd):
    import _nvp_oracle as O
    model, omodel = _shape_problem(vb, shape)
    model._torch_logp = _torch_logp_of(omodel)
    D, N, K = model.dim, shape[4], 2
    masks = np.array([[(j + i) % 2 for j in range(D)] for i in range(K)], dtype=float)

    def make():
        prior = vb.MFGaussian(D, seed=3)
        r = np.random.RandomState(D + K)
        return vb.NVPFlow([[D, 10], [10, D]], [[D, 10], [10, D]], masks, prior,
                          np.concatenate([0.1 * r.randn(D), -1.0 + 0.1 * r.randn(D)]), D)
    flow, twin = make(), make()
    theta = 0.1 * np.random.RandomState(D * 7 + K + N).randn(flow.var_param_dim)
    value, grad = vb.ExclusiveKL(flow, model, N, use_path_deriv=pd)(theta)
    z0 = twin.prior_param[:D] + np.exp(twin.prior_param[D:]) * twin.prior._base_noise(N)
    ov, og = O.objective(twin, model, theta, z0, pd)
    print('ekl flow D=%d pd=%d: rel err value %.2e grad %.2e' % (D, pd, abs(value - ov) / max(1.0, abs(ov)), G.rel_err(grad, og)))
    assert abs(value - ov) <= 1e-12 * max(1.0, abs(ov)), (value, ov)
    assert G.rel_err(grad, og) <= 1e-10, G.rel_err(grad, og)                         # (the flow tests' bound)


# ---- 6. AlphaDivergence ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', ['mf_gaussian', 'mf_student_t', 'fullrank', 'multivariate_t', 'lr_gaussian'])
@pytest.mark.parametrize('alpha', [0.5, 2.0])
def test_alpha_divergence(vb, family, alpha):
    model, omodel = _shape_problem(vb, SMALL)
    D, N = model.dim, SMALL[4]
    rng = np.random.RandomState(D)
    tol_v, tol_g = 1e-12, 1e-11
    if family == 'mf_gaussian':
        approx, ofamily, theta = vb.MFGaussian(D), ofam.MFGaussian(D), _mf_theta(D, 1)
    elif family == 'mf_student_t':
        approx, ofamily, theta = vb.MFStudentT(D, 12), ofam.MFStudentT(D, 12), _mf_theta(D, 2)
    elif family == 'fullrank':
        approx, ofamily, theta = vb.FullRankGaussian(D), ofam.FullRankGaussian(D), _fr_theta(D, 3)
    elif family == 'multivariate_t':
        approx, ofamily = vb.MultivariateT(D, 40.0), ofam.MultivariateT(D, 40.0)
        L = np.tril(0.05 * rng.randn(D, D), -1) + np.diag(np.exp(-1.0 + 0.2 * rng.randn(D)))
        theta = np.concatenate([0.3 * rng.randn(D), ofam.chol_to_free(L)])
        tol_g = 1e-10                                             # (the source-model test of this route)
    else:
        k = 2
        approx, ofamily = vb.LRGaussian(D, seed=2, k=k), ofam.LRGaussian(D, k)
        theta = np.concatenate([0.3 * rng.randn(D), -0.7 + 0.2 * rng.randn(D), 0.3 * rng.randn(D * k) / np.sqrt(k)])
        tol_v, tol_g = 1e-11, 1e-9                                # (the source-model test of this route)
    np.random.seed(11)
    value, grad = vb.AlphaDivergence(approx, model, N, alpha)(theta)
    np.random.seed(11)
    noise = ofamily.draw_noise(np.random.RandomState(np.random.randint(2 ** 32)), N)
    ov, og = oobj.alpha_divergence(ofamily, omodel, theta, noise, alpha)
    print('alpha %s %.1f: rel err value %.2e grad %.2e' % (family, alpha, G.rel_err(value, ov), G.rel_err(grad, og)))
    assert G.rel_err(value, ov) < tol_v, (value, ov)
    assert G.rel_err(grad, og) < tol_g, G.rel_err(grad, og)


# ---- 7. DISInclusiveKL -----------------------------------------------------------------------------------------------
def _dis_case(vb, family, D):
    rng = np.random.RandomState(9)
    if family == 'mf_gaussian':
        return vb.MFGaussian(D, seed=6), ofam.MFGaussian(D), np.concatenate([0.1 * rng.randn(D), -0.5 + 0.1 * rng.randn(D)])
    if family == 'mf_student_t':
        return (vb.MFStudentT(D, 12.0, seed=6), ofam.MFStudentT(D, 12.0),
                np.concatenate([0.1 * rng.randn(D), -0.5 + 0.1 * rng.randn(D)]))
    if family == 'lr_gaussian':
        k = 2
        return (vb.LRGaussian(D, seed=6, k=k), ofam.LRGaussian(D, k),
                np.concatenate([0.1 * rng.randn(D), -0.5 + 0.1 * rng.randn(D), 0.2 * rng.randn(D * k) / np.sqrt(k)]))
    A = rng.randn(D, D)
    theta = np.concatenate([0.1 * rng.randn(D), ofam.psd_to_free(A @ A.T / D + 0.7 * np.eye(D))])
    if family == 'multivariate_t':
        return vb.MultivariateT(D, 40, seed=6), ofam.MultivariateT(D, 40), theta
    return vb.FullRankGaussian(D, seed=6), ofam.FullRankGaussian(D), theta


@pytest.mark.parametrize('family', ['mf_gaussian', 'mf_student_t', 'multivariate_t', 'fullrank', 'lr_gaussian'])
@pytest.mark.parametrize('use_resampling', [True, False])
def test_dis_inclusive_kl(vb, family, use_resampling):
    """Three calls with a moving theta (refresh on even steps), the structure of the source-model DIS tests."""
    N, ess = 600, 150
    model, omodel = _shape_problem(vb, SMALL)
    D = model.dim
    approx, ofamily, theta = _dis_case(vb, family, D)
    prior = np.concatenate([np.zeros(D), np.log(3.0) * np.ones(D)])
    kw = dict(use_resampling=use_resampling, num_resampling_batches=2)
    obj = vb.DISInclusiveKL(approx, model, N, ess_target=ess, temper_prior=vb.MFGaussian(D),
                            temper_prior_params=prior, **kw)
    ref = oobj.DISInclusiveKL(ofamily, omodel, N, ess, ofam.MFGaussian(D), prior, **kw)
    rs = np.random.RandomState(6)
    np.random.seed(12)
    for step in range(3):
        state = np.random.get_state()
        value, grad = obj(theta)
        np.random.set_state(state)
        noise = ofamily.draw_noise(rs, N) if ref.needs_refresh() else None
        if use_resampling:
            if ref.needs_refresh():
                ref.refresh(theta, noise)
            idx = np.random.choice(N, size=ref._resampling_batch_size, p=ref._state_w_normalized)
            ref._objective_step += 1
            xs = ref._state_samples[idx]
            scale = ref._state_w_sum / N
            ov = np.mean(-ofamily.log_density(theta, xs)) * scale
            og = -ofamily.log_density_grad_weighted(theta, xs, np.ones(len(idx))) / len(idx) * scale
        else:
            ov, og = ref(theta, noise=noise)
        assert G.rel_err(obj._eps, ref._eps) < 1e-10
        assert G.rel_err(value, ov) < 1e-10, (step, value, ov)
        assert G.rel_err(grad, og) < 1e-9, (step, G.rel_err(grad, og))
        theta = theta - 0.01 * grad / (1 + np.abs(grad))


def test_dis_inclusive_kl_psis_smoothed(vb):
    from oracle import psis as opsis
    N = 2048
    model, omodel = _shape_problem(vb, SMALL)
    D = model.dim
    approx, ofamily, theta = _dis_case(vb, 'mf_gaussian', D)
    approx = vb.MFGaussian(D, seed=3)
    prior = np.concatenate([np.zeros(D), np.log(3.0) * np.ones(D)])
    obj = vb.DISInclusiveKL(approx, model, N, temper_prior=vb.MFGaussian(D), temper_prior_params=prior, psis_smooth=True,
                            ess_target=400, use_resampling=False)
    value, grad = obj(theta)
    ref = oobj.DISInclusiveKL(ofamily, omodel, N, 400, ofam.MFGaussian(D), prior, use_resampling=False)
    ref.refresh(theta, ofamily.draw_noise(np.random.RandomState(3), N))
    w = ref._state_w_clipped
    smoothed, khat = opsis.psis_smooth(np.log(w))
    w_s = np.sum(w) * np.exp(smoothed)
    assert G.rel_err(obj._state_w_clipped, w_s) < 1e-9
    assert abs(obj._khat - khat) < 1e-8
    lq = ofamily.log_density(theta, ref._state_samples)
    ov = -np.inner(w_s, lq) / N
    og = -ofamily.log_density_grad_weighted(theta, ref._state_samples, w_s) / N
    assert G.rel_err(value, ov) < 1e-9
    assert G.rel_err(grad, og) < 1e-8


# ---- 8. control variates, Hessian-vector product ---------------------------------------------------------------------
@pytest.mark.parametrize('method', ['full', 'mean_only', 'loo_diag_approx', 'loo_direct_approx'])
def test_control_variates_against_literal_rge(vb, method):
    N = 512
    model, omodel = _shape_problem(vb, LARGE)
    D = model.dim
    theta = np.concatenate([_mf_theta(D, 17)[:D], -1.2 + 0.2 * np.random.RandomState(18).randn(D)])
    obj = vb.ExclusiveKL(vb.MFGaussian(D, seed=5), model, N, hessian_approx_method=method)
    value, grad = obj(theta)
    noise = np.random.RandomState(5).randn(N, D)
    ov, og = oobj.rge_literal(ofam.MFGaussian(D), omodel, theta, noise, method)
    print('cv %s: rel err value %.2e grad %.2e' % (method, G.rel_err(value, ov), G.rel_err(grad, og)))
    assert G.rel_err(value, ov) < 1e-12, (value, ov)
    assert G.rel_err(grad, og) < 1e-8, G.rel_err(grad, og)                            # (the source-model test's bound)
    plain = vb.ExclusiveKL(vb.MFGaussian(D, seed=5), model, N)(theta)[1]
    assert G.rel_err(grad, plain) > 1e-4                     # the control variate really changed the estimate
    assert not obj.supports_device_fit()


def test_hessian_vector_product(vb):
    N = 256
    model, omodel = _shape_problem(vb, SMALL)
    D = model.dim
    rng = np.random.RandomState(18)
    theta = _mf_theta(D, 19)
    x = rng.randn(2 * D)
    hv = vb.ExclusiveKL(vb.MFGaussian(D, seed=9), model, N)._hessian_vector_product(theta, x)
    noise = np.random.RandomState(9).randn(N, D)
    # the oracle's: z_n = mu + sigma e_n; d^2 / d theta^2 of -mean f(z_n) through the model's closed-form Hessian
    mu, sg = theta[:D], np.exp(theta[D:])
    xm, xs = x[:D], x[D:]
    z = mu + sg * noise
    gz = omodel.grad(z)
    dz = xm + sg * noise * xs                                 # directional derivative of z_n along x
    Hdz = np.stack([omodel.hvp(z[n], dz[n])[0] for n in range(N)])
    ref_m = -Hdz.mean(0)
    ref_s = -((Hdz * sg * noise).mean(0) + (gz * sg * noise).mean(0) * xs)
    ref = np.concatenate([ref_m, ref_s])
    assert G.rel_err(hv, ref) < 1e-6, G.rel_err(hv, ref)      # (second difference of the device gradient: the source-model bound)


# ---- 9. device-resident fit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', ['mf_gaussian', 'fullrank'])
def test_device_fit_matches_host_loop(vb, capsys, family):
    from viabel_amd.optimization import RMSProp
    model, _ = _shape_problem(vb, SMALL)
    D = model.dim
    hist = {}
    for on_device in (False, True):
        fam = vb.MFGaussian(D, rng='philox', seed=3) if family == 'mf_gaussian' else vb.FullRankGaussian(D, rng='philox', seed=3)
        obj = vb.ExclusiveKL(fam, model, 128)
        assert obj.supports_device_fit()
        res = RMSProp(0.02).optimize(60, obj, fam.init_param(), on_device=on_device)
        hist[on_device] = np.asarray(res['value_history'])
    capsys.readouterr()
    np.testing.assert_array_equal(hist[False], hist[True])


# ---- 10. samples_and_log_weights / vi_diagnostics --------------------------------------------------------------------
def test_log_weights_and_diagnostics(vb, capsys):
    from viabel_amd import convenience
    model, omodel = _shape_problem(vb, SMALL)
    D = model.dim
    approx = vb.MFGaussian(D, seed=3)
    theta = np.concatenate([0.1 * np.arange(D), -0.7 * np.ones(D)])
    assert convenience._on_device_weights(model, approx)
    # the device route of psis_correction (vb_log_weights_meanfield on staged noise), its raw weights fetched
    from viabel_amd import _lib
    n = 2000
    eng = _lib.default_engine()
    eng.set_model(model.device_spec())
    noise = np.random.RandomState(8).randn(n, D)
    eng.noise_set_host(convenience._DIAG_SLOT, noise)
    family, df = approx._device_family()
    lw = eng.log_weights_meanfield(convenience._DIAG_SLOT, n, D, theta, family, df=df, fetch=True)
    samples = theta[:D] + np.exp(theta[D:]) * noise
    want = model(samples) - approx.log_density(theta, samples)
    assert G.rel_err(lw, want) < 1e-11, G.rel_err(lw, want)
    assert G.rel_err(lw, omodel.logp(samples) - ofam.MFGaussian(D).log_density(theta, samples)) < 1e-11
    samples2, lw2 = convenience.samples_and_log_weights(theta, model, vb.MFGaussian(D, seed=3), 500)
    assert G.rel_err(lw2, omodel.logp(samples2) - ofam.MFGaussian(D).log_density(theta, samples2)) < 1e-11
    res = vb.vi_diagnostics(theta, model=model, approx=vb.MFGaussian(D, seed=3), n_samples=4000)
    capsys.readouterr()
    assert np.isfinite(res['khat'])


# ---- 11. a fit that learns -------------------------------------------------------------------------------------------
def fit_problem():
    """The data of test_bbvi_fit_learns_the_robust_line and its CPU-side numbers: (X, y, oracle, MAP, Laplace standard
    deviations at the MAP).  A line with intercept 1 and slope 2, t_4 noise of scale 0.5, and every 25th observation moved
    up by 15: a Student-t likelihood with a constant unknown scale, theta = (intercept, slope, log sigma)."""
    from scipy.optimize import minimize
    n_data = 300
    rng = np.random.RandomState(7)
    X = np.stack([np.ones(n_data), rng.randn(n_data)], axis=1)
    y = X @ np.array([1.0, 2.0]) + 0.5 * rng.standard_t(4.0, size=n_data)
    y[::25] += 15.0
    omodel = LocScaleOracle(X, y, None, 'student_t', 4.0, 10.0, 1.0)
    r = minimize(lambda t: -omodel.logp(t)[0], np.zeros(omodel.dim), jac=lambda t: -omodel.grad(t)[0], method='BFGS',
                 options=dict(gtol=1e-10))
    sd = np.sqrt(np.diag(np.linalg.inv(-omodel.hessian(r.x))))
    return X, y, omodel, r.x, sd


def test_bbvi_fit_learns_the_robust_line(vb, capsys):
    """bbvi with an MFGaussian(rng='philox'), fixed seed, on t-noise data with gross outliers.  e = max_j |mean_j - MAP_j| /
    (Laplace sd)_j, the MAP by BFGS on the oracle.  With 300 observations the zero start lies many standard deviations
    from the MAP and a mean-field mean sits well within one of it: e1 < e0 / 3 is required.  Measured on an MI355X:
    e0 = 50.249, e1 = 0.155."""
    X, y, omodel, t_map, sd = fit_problem()
    model = vb.LocationScaleRegressionModel(X, y, None, 'student_t', 4.0, 10.0, 1.0)
    D = model.dim

    def err(theta):
        return float(np.max(np.abs(theta[:D] - t_map) / sd))
    approx = vb.MFGaussian(D, seed=3, rng='philox')
    init = approx.init_param()
    e0 = err(init)
    obj = vb.ExclusiveKL(approx, model, 64)
    res = vb.bbvi(D, objective=obj, init_var_param=init, n_iters=2000, adaptive=False, fixed_lr=True, learning_rate=0.05)
    capsys.readouterr()
    e1 = err(res['opt_param'])
    print('fit: e0 = %.3f, e1 = %.3f Laplace sd (MAP %s, sd %s)' % (e0, e1, np.round(t_map, 3), np.round(sd, 4)))
    assert e1 < e0 / 3, (e0, e1)


# ---- 12. errors ------------------------------------------------------------------------------------------------------
def test_errors_leave_the_context_usable(vb):
    from viabel_amd import _lib
    eng = _lib.default_engine()
    p, q, n_data = 5, 3, 33
    model, omodel = _problem(vb, 'student_t', p, q, n_data)
    good = model.device_spec()
    x = 0.3 * np.random.RandomState(0).randn(5, model.dim)
    f_before = model(x)                                           # binds the model: the failures below must leave it bound
    with pytest.raises(ValueError):                               # dim != p + q
        eng.set_model((_lib.MODEL_LOCSCALE, good[1] + 1, good[2].copy(), good[3].copy()))
    bad = good[3].copy()
    bad[2] = q + 1                                                # dim == p + q again, but q disagrees with the dparams length
    with pytest.raises(ValueError):
        eng.set_model((_lib.MODEL_LOCSCALE, good[1] + 1, good[2].copy(), bad))
    bad = good[3].copy()
    bad[3] = 2                                                    # an unknown likelihood
    with pytest.raises(ValueError):
        eng.set_model((_lib.MODEL_LOCSCALE, good[1], good[2].copy(), bad))
    bad = good[3].copy()
    bad[4] = 1                                                    # a constant scale with q = 3
    with pytest.raises(ValueError):
        eng.set_model((_lib.MODEL_LOCSCALE, good[1], good[2].copy(), bad))
    bad_d = good[2].copy()
    bad_d[-1] = -1.0                                              # df <= 0, past the Python check
    with pytest.raises(ValueError):
        eng.set_model((_lib.MODEL_LOCSCALE, good[1], bad_d, good[3].copy()))
    with pytest.raises(ValueError):
        model(np.zeros((2, model.dim + 1)))
    assert G.rel_err(eng.model_logp(x), omodel.logp(x)) < 1e-12   # the engine still holds the model bound before
    assert np.array_equal(model(x), f_before)
    assert G.rel_err(model.grad(x), omodel.grad(x)) < 1e-11
    with pytest.raises(NotImplementedError, match='psisloo'):
        vb.loo(np.zeros(2 * model.dim), model=model, approx=vb.MFGaussian(model.dim), n_samples=10)
    linear = vb.LinearRegressionModel(omodel.X, omodel.y)
    linear(np.zeros(p))
    with pytest.raises(NotImplementedError):                      # vb_locscale_pointwise with another model bound
        eng.locscale_pointwise(np.zeros((2, p)), n_data)
    assert np.array_equal(model(x), f_before)                     # and the next good call succeeds
    assert G.rel_err(model.pointwise_log_likelihood(x), omodel.pointwise(x)) < 1e-12
