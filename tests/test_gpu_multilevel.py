"""MultilevelRegressionModel (VB_MODEL_MULTILEVEL, csrc/vb_multilevel.hip) on the GPU against the numpy oracle of
tests/_multilevel_oracle.py: the row pipeline (predictor GEMM, link kernel, coefficient-gradient GEMM, group kernel, row
sums), and the target under every objective x family route a SourceModel takes (tests/test_gpu_softmax.py is the template,
with its tolerances: value 1e-12, gradient 1e-11 relative, 1e-10 / 1e-9 where the source-model and softmax tests of the same
route use them)."""
import numpy as np
import pytest

import _golden as G
from _multilevel_oracle import MultilevelOracle
from oracle import families as ofam, objectives as oobj

pytestmark = pytest.mark.gpu

SMALL, LARGE = ('logistic', 2, 3, 30, 100), ('poisson', 13, 50, 400, 333)      # (likelihood, p, J, n_data, N): D = 6 and 64
SHAPES = [SMALL, LARGE]


@pytest.fixture(scope='module')
def vb():
    import viabel_amd
    from viabel_amd import _lib
    _lib.default_engine()
    return viabel_amd


_PROBLEMS = {}


def _simulate(rng, lik, eta, noise_sd):
    if lik == 'logistic':
        return (rng.rand(eta.size) < 1.0 / (1.0 + np.exp(-eta))).astype(float)
    if lik == 'poisson':
        return rng.poisson(np.exp(eta)).astype(float)
    return eta + noise_sd * rng.randn(eta.size)


def _problem(vb, lik, p, J, n_data, sizes=None, empty=(), prior_sd=3.0, tau_sd=0.8, noise_sd=1.3):
    """(device model, oracle) on X = randn / sqrt(p), labels in random (unsorted) order, y simulated from coefficients and
    group effects of scale 0.3; built once per shape and shared.  `sizes`: the group sizes; `empty`: groups left without
    observations."""
    key = (lik, p, J, n_data, sizes, empty)
    if key not in _PROBLEMS:
        rng = np.random.RandomState(1000 * J + 10 * p + n_data)
        X = rng.randn(n_data, p) / np.sqrt(p)
        if sizes is not None:
            groups = rng.permutation(np.repeat(np.arange(J), sizes))
        else:
            groups = rng.randint(0, J, size=n_data)
            for e in empty:
                groups[groups == e] = (e + 1) % J
        assert groups.shape == (n_data,) and not any(np.any(groups == e) for e in empty)
        y = _simulate(rng, lik, X @ (0.3 * rng.randn(p)) + (0.3 * rng.randn(J))[groups], noise_sd)
        args = (X, y, groups, J, lik, prior_sd, tau_sd, noise_sd)
        _PROBLEMS[key] = (vb.MultilevelRegressionModel(*args), MultilevelOracle(*args))
    return _PROBLEMS[key]


def _shape_problem(vb, shape):
    return _problem(vb, *shape[:4])


def _round_up(x, m):
    return (x + m - 1) // m * m


# ---- 1. rows ---------------------------------------------------------------------------------------------------------
def _rows_cases():
    from viabel_amd import _lib
    chunk = max(8, _lib.MULTILEVEL_CHUNK_DOUBLES // _round_up(2500, 16))
    return [('logistic', 1, 1, 1, 1), ('poisson', 5, 3, 33, 100), ('gaussian', 17, 7, 130, 257),
            ('logistic', 16, 40, 300, 64), ('logistic', 3, 3, 2500, 2 * chunk + 5)]


@pytest.mark.parametrize('lik,p,J,n_data,rows', _rows_cases())
def test_rows_against_oracle(vb, lik, p, J, n_data, rows):
    """model(x), model.grad(x), pointwise_log_likelihood(x).  (1, 1, 1): the smallest shape; poisson: group 1 is empty (its
    gradient entry is -u_1 exactly) and the labels arrive unsorted; p = 17: odd, the coefficient gradient's last column is a
    single store next to the u block; n_data = 300: the split branch of the gradient GEMM; the last case: group sizes
    [2100, 0, 400], so a run spans several strips of the link kernel, and three row chunks (two full ones and a
    remainder)."""
    from viabel_amd import _lib
    kw = {}
    if lik == 'poisson':
        kw = dict(empty=(1,))
    if n_data == 2500:
        kw = dict(sizes=(2100, 0, 400))
        assert rows > 2 * max(8, _lib.MULTILEVEL_CHUNK_DOUBLES // _round_up(n_data, 16))      # at least three chunks
    model, omodel = _problem(vb, lik, p, J, n_data, **kw)
    assert not np.all(np.diff(omodel.groups) >= 0) or n_data == 1            # the caller's labels are unsorted
    x = 0.3 * np.random.RandomState(rows).randn(rows, model.dim)
    fo, go, po = np.empty(rows), np.empty((rows, model.dim)), np.empty((rows, n_data))
    for r0 in range(0, rows, 512):                               # (the oracle's (rows, n_data) temporaries, bounded)
        s = slice(r0, r0 + 512)
        fo[s], go[s], po[s] = omodel.logp(x[s]), omodel.grad(x[s]), omodel.pointwise(x[s])
    f, g, pw = model(x), model.grad(x), model.pointwise_log_likelihood(x)
    assert f.shape == (rows,) and g.shape == (rows, model.dim) and pw.shape == (rows, n_data)
    ef, eg, ep = G.rel_err(f, fo), G.rel_err(g, go), G.rel_err(pw, po)
    print('rows %s p=%d J=%d n_data=%d rows=%d: rel err f %.2e grad %.2e pointwise %.2e' % (lik, p, J, n_data, rows, ef, eg, ep))
    assert ef < 1e-12 and eg < 1e-11 and ep < 1e-12, (ef, eg, ep)
    for e in kw.get('empty', ()) + ((1,) if n_data == 2500 else ()):
        assert np.array_equal(g[:, p + e], -x[:, p + e])         # an empty group: just -u_j
    assert model.check_gradient(x[:3]) < 1e-6
    assert np.array_equal(model(x), f) and np.array_equal(model.grad(x), g)        # no atomics: the same bits
    assert np.array_equal(model.pointwise_log_likelihood(x), pw)
    assert model(x[0]).shape == (1,) and model.grad(x[0]).shape == (model.dim,)
    assert model.pointwise_log_likelihood(x[0]).shape == (1, n_data)


# ---- 2. against the flat device models on the augmented design -------------------------------------------------------
@pytest.mark.parametrize('lik', ['logistic', 'poisson'])
def test_pointwise_matches_the_flat_device_model(vb, lik):
    p, J, n_data = 7, 5, 45
    model, omodel = _problem(vb, lik, p, J, n_data)
    Xa = np.concatenate([omodel.X, np.eye(J)[omodel.groups]], axis=1)
    flat = (vb.LogisticRegressionModel if lik == 'logistic' else vb.PoissonRegressionModel)(Xa, omodel.y)
    theta = 0.3 * np.random.RandomState(4).randn(20, model.dim)
    b, u, tau = model.unpack(theta)
    a = model.pointwise_log_likelihood(theta)
    c = flat.pointwise_log_likelihood(np.concatenate([b, tau[:, None] * u], axis=1))
    assert G.rel_err(a, c) < 1e-12, G.rel_err(a, c)


# ---- 3. overflow -----------------------------------------------------------------------------------------------------
def test_large_predictors_do_not_overflow(vb):
    model, omodel = _problem(vb, 'logistic', 5, 3, 33)
    x = np.random.RandomState(2).randn(40, model.dim)
    x[:, -1] *= 0.3                                              # tau stays moderate; eta is linear in (b, u)
    x[:, :-1] *= 800.0 / np.max(np.abs(omodel.eta(x)))
    assert 799.0 < np.max(np.abs(omodel.eta(x))) < 801.0
    f, g = model(x), model.grad(x)
    assert np.all(np.isfinite(f)) and np.all(np.isfinite(g))
    ef, eg = G.rel_err(f, omodel.logp(x)), G.rel_err(g, omodel.grad(x))
    print('overflow: rel err f %.2e grad %.2e' % (ef, eg))
    assert ef < 1e-12 and eg < 1e-11, (ef, eg)


# ---- 4. ExclusiveKL --------------------------------------------------------------------------------------------------
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
    X, y = torch.from_numpy(np.asarray(omodel.X, dtype=float)), torch.from_numpy(np.asarray(omodel.y, dtype=float))
    g = torch.from_numpy(omodel.groups)
    cst = torch.from_numpy(np.asarray(omodel.obs_const, dtype=float))
    p, J, lik = omodel.p, omodel.J, omodel.likelihood
    sd, tsd, nsd = float(omodel.prior_sd), float(omodel.tau_sd), float(omodel.noise_sd)
    l2pi = np.log(2.0 * np.pi)
    const = -p * (np.log(sd) + 0.5 * l2pi) - 0.5 * J * l2pi + np.log(2.0) - np.log(tsd) - 0.5 * l2pi

    def logp(x):
        b, u, omega = x[:, :p], x[:, p:p + J], x[:, -1]
        tau = torch.exp(omega)
        eta = b @ X.T + tau[:, None] * u[:, g]
        if lik == 'poisson':
            ll = y * eta - torch.exp(eta)
        elif lik == 'gaussian':
            ll = -0.5 * (y - eta) ** 2 / nsd ** 2
        else:
            ll = y * eta - torch.nn.functional.softplus(eta)
        return (torch.sum(ll + cst, dim=1) - 0.5 * torch.sum(b * b, dim=1) / sd ** 2 - 0.5 * torch.sum(u * u, dim=1)
                - 0.5 * tau ** 2 / tsd ** 2 + omega + const)
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


# ---- 5. AlphaDivergence ----------------------------------------------------------------------------------------------
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


# ---- 6. DISInclusiveKL -----------------------------------------------------------------------------------------------
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


# ---- 7. control variates, Hessian-vector product ---------------------------------------------------------------------
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


# ---- 8. device-resident fit ------------------------------------------------------------------------------------------
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


# ---- 9. samples_and_log_weights / vi_diagnostics ---------------------------------------------------------------------
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


# ---- 10. a fit that learns -------------------------------------------------------------------------------------------
def fit_problem():
    """The data of test_bbvi_fit_learns_the_group_effects and its CPU-side numbers: (X, y, groups, oracle, MAP, Laplace
    standard deviations of (b, tau u, log tau) at the MAP by the delta method)."""
    from scipy.optimize import minimize
    p, J, per_group = 2, 8, 200
    rng = np.random.RandomState(7)
    n_data = J * per_group
    X = rng.randn(n_data, p)
    groups = rng.permutation(np.repeat(np.arange(J), per_group))
    b_true, a_true = np.array([2.5, -2.0]), 1.0 * rng.randn(J)
    y = _simulate(rng, 'logistic', X @ b_true + a_true[groups], 1.0)
    omodel = MultilevelOracle(X, y, groups, J, 'logistic', 10.0, 1.0)
    D = omodel.dim
    start = np.concatenate([np.zeros(p), 0.1 * np.ones(J), [0.0]])      # (off u = 0, where the gradient in omega vanishes)
    r = minimize(lambda t: -omodel.logp(t)[0], start, jac=lambda t: -omodel.grad(t)[0], method='BFGS',
                 options=dict(gtol=1e-10))
    S = np.linalg.inv(-omodel.hessian(r.x))
    tau = np.exp(r.x[-1])
    T = np.eye(D)                                              # rows: d (b, tau u, log tau) / d theta at the MAP
    T[p:p + J, p:p + J] *= tau
    T[p:p + J, -1] = tau * r.x[p:p + J]
    sd = np.sqrt(np.diag(T @ S @ T.T))
    return X, y, groups, omodel, r.x, sd


def _fit_coords(theta, p, J):
    return np.concatenate([theta[:p], np.exp(theta[p + J]) * theta[p:p + J], [theta[p + J]]])


def test_bbvi_fit_learns_the_group_effects(vb, capsys):
    """Logistic, p = 2, J = 8, 200 observations per group, simulated with b = (2.5, -2) and tau = 1; bbvi with a
    FullRankGaussian(rng='philox'), path derivative, fixed seed, 2000 iterations.  e = max |(b, tau u, log tau)_fit - MAP|,
    the MAP by BFGS on the oracle.  Numbers worked out on the CPU from the oracle for exactly this data (fit_problem): the
    Laplace standard deviations of the eleven coordinates at the MAP are 0.116 ... 0.261 (the largest: log tau), so five of
    them are 1.303; the error of the initial parameter (mean zero) is 2.49.  Threshold 1.5: above 1.303, below 2.49; after
    the fit e must be below 0.75."""
    X, y, groups, omodel, t_map, sd = fit_problem()
    p, J = omodel.p, omodel.J
    model = vb.MultilevelRegressionModel(X, y, groups, J, 'logistic', 10.0, 1.0)
    D = model.dim
    threshold = 1.5
    assert 5.0 * max(sd) <= threshold, max(sd)

    def err(theta):
        return float(np.max(np.abs(_fit_coords(theta[:D], p, J) - _fit_coords(t_map, p, J))))
    approx = vb.FullRankGaussian(D, seed=3, rng='philox')
    init = approx.init_param()
    e0 = err(init)
    assert threshold < e0, e0
    obj = vb.ExclusiveKL(approx, model, 64, use_path_deriv=True)
    res = vb.bbvi(D, objective=obj, init_var_param=init, n_iters=2000, adaptive=False, fixed_lr=True, learning_rate=0.05)
    capsys.readouterr()
    e1 = err(res['opt_param'])
    print('fit: e0 = %.3f, e1 = %.3f, 5 Laplace sd = %.3f' % (e0, e1, 5.0 * max(sd)))
    assert e1 < threshold / 2, (e0, e1)


# ---- 11. errors ------------------------------------------------------------------------------------------------------
def test_errors_leave_the_context_usable(vb):
    from viabel_amd import _lib
    eng = _lib.default_engine()
    p, J, n_data = 5, 3, 33
    model, omodel = _problem(vb, 'logistic', p, J, n_data)
    good = model.device_spec()
    x = 0.3 * np.random.RandomState(0).randn(5, model.dim)
    f_before = model(x)                                           # binds the model: the failures below must leave it bound
    bad = good[3].copy()
    bad[3 + J + 1 + n_data - 1] = J                               # a label == n_groups, past the Python check
    with pytest.raises(ValueError):
        eng.set_model((_lib.MODEL_MULTILEVEL, good[1], good[2].copy(), bad))
    bad = good[3].copy()
    bad[3 + 1], bad[3 + 2] = good[3][3 + 2], good[3][3 + 1] - 1   # non-monotone offsets
    assert bad[3 + 2] < bad[3 + 1]
    with pytest.raises(ValueError):
        eng.set_model((_lib.MODEL_MULTILEVEL, good[1], good[2].copy(), bad))
    with pytest.raises(ValueError):                               # dim != p + n_groups + 1
        eng.set_model((_lib.MODEL_MULTILEVEL, good[1] + 1, good[2].copy(), good[3].copy()))
    with pytest.raises(ValueError):
        model(np.zeros((2, model.dim + 1)))
    assert G.rel_err(eng.model_logp(x), omodel.logp(x)) < 1e-12   # the engine still holds the model bound before
    assert np.array_equal(model(x), f_before)
    assert G.rel_err(model.grad(x), omodel.grad(x)) < 1e-11
    with pytest.raises(NotImplementedError, match='psisloo'):
        vb.loo(np.zeros(2 * model.dim), model=model, approx=vb.MFGaussian(model.dim), n_samples=10)
    logit = vb.LogisticRegressionModel(omodel.X, omodel.y)
    logit(np.zeros(p))
    with pytest.raises(NotImplementedError):                      # vb_multilevel_pointwise with another model bound
        eng.multilevel_pointwise(np.zeros((2, p)), n_data)
