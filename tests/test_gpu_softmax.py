"""SoftmaxRegressionModel (VB_MODEL_SOFTMAX, csrc/vb_softmax.hip) on the GPU against the numpy oracle of
tests/_softmax_oracle.py: the row pipeline (pack, predictor GEMM, coupling kernel, gradient GEMM, unpack), and the target
under every objective x family route a SourceModel takes (tests/test_gpu_source_model.py is the template, with its
tolerances: value 1e-12, gradient 1e-11 relative, 1e-10 / 1e-9 where the source-model test of the same route uses them)."""
import numpy as np
import pytest

import _golden as G
from _softmax_oracle import SoftmaxOracle
from oracle import families as ofam, objectives as oobj

pytestmark = pytest.mark.gpu

SMALL, LARGE = (3, 2, 30, 100), (5, 13, 40, 333)            # (C, p, n_data, N): D = 6 and 65
SHAPES = [SMALL, LARGE]


@pytest.fixture(scope='module')
def vb():
    import viabel_amd
    from viabel_amd import _lib
    _lib.default_engine()
    return viabel_amd


_PROBLEMS = {}


def _problem(vb, C, p, n_data, seed=0, prior_sd=3.0):
    """(device model, oracle) on X = randn / sqrt(p), uniform labels; built once per shape and shared."""
    key = (C, p, n_data, seed, prior_sd)
    if key not in _PROBLEMS:
        rng = np.random.RandomState(1000 * C + 10 * p + n_data + seed)
        X = rng.randn(n_data, p) / np.sqrt(p)
        y = rng.randint(0, C, size=n_data)
        _PROBLEMS[key] = (vb.SoftmaxRegressionModel(X, y, C, prior_sd), SoftmaxOracle(X, y, C, prior_sd))
    return _PROBLEMS[key]


def _round_up(x, m):
    return (x + m - 1) // m * m


# ---- 1. rows ---------------------------------------------------------------------------------------------------------
def _rows_cases():
    from viabel_amd import _lib
    chunk = max(8, _lib.SOFTMAX_CHUNK_DOUBLES // (4 * _round_up(2000, 16)))
    return [(2, 1, 1, 1), (3, 5, 33, 100), (7, 17, 130, 257), (33, 16, 300, 64), (4, 3, 2000, 2 * chunk + 5)]


@pytest.mark.parametrize('C,p,n_data,rows', _rows_cases())
def test_rows_against_oracle(vb, C, p, n_data, rows):
    """model(x), model.grad(x), pointwise_log_likelihood(x).  p = 17: odd, no multiple of 16; n_data = 300: the split
    branch of the gradient GEMM; the last case: three row chunks (two full ones and a remainder)."""
    from viabel_amd import _lib
    model, omodel = _problem(vb, C, p, n_data)
    chunk = max(8, _lib.SOFTMAX_CHUNK_DOUBLES // (C * _round_up(n_data, 16)))
    if n_data == 2000:
        assert rows > 2 * chunk                                  # at least three chunks
    x = 0.3 * np.random.RandomState(rows).randn(rows, model.dim)
    fo, go, po = np.empty(rows), np.empty((rows, model.dim)), np.empty((rows, n_data))
    for r0 in range(0, rows, 512):                               # (the oracle's (rows, n_data, C) temporaries, bounded)
        s = slice(r0, r0 + 512)
        fo[s], go[s], po[s] = omodel.logp(x[s]), omodel.grad(x[s]), omodel.pointwise(x[s])
    f, g, pw = model(x), model.grad(x), model.pointwise_log_likelihood(x)
    assert f.shape == (rows,) and g.shape == (rows, model.dim) and pw.shape == (rows, n_data)
    ef, eg, ep = G.rel_err(f, fo), G.rel_err(g, go), G.rel_err(pw, po)
    print('rows C=%d p=%d n_data=%d rows=%d: rel err f %.2e grad %.2e pointwise %.2e' % (C, p, n_data, rows, ef, eg, ep))
    assert ef < 1e-12 and eg < 1e-11 and ep < 1e-12, (ef, eg, ep)
    assert model.check_gradient(x[:3]) < 1e-6
    assert np.array_equal(model(x), f) and np.array_equal(model.grad(x), g)        # no atomics: the same bits
    assert np.array_equal(model.pointwise_log_likelihood(x), pw)
    assert model(x[0]).shape == (1,) and model.grad(x[0]).shape == (model.dim,)


# ---- 2. overflow -----------------------------------------------------------------------------------------------------
def test_large_predictors_do_not_overflow(vb):
    C, p, n_data = 3, 5, 33
    model, omodel = _problem(vb, C, p, n_data)
    x = np.random.RandomState(2).randn(40, model.dim)
    x *= 800.0 / np.max(np.abs(omodel.eta(x)))
    assert 799.0 < np.max(np.abs(omodel.eta(x))) < 801.0
    f, g = model(x), model.grad(x)
    assert np.all(np.isfinite(f)) and np.all(np.isfinite(g))
    assert G.rel_err(f, omodel.logp(x)) < 1e-12
    assert G.rel_err(g, omodel.grad(x)) < 1e-11


# ---- 3. two classes against the logistic device model ----------------------------------------------------------------
def test_two_classes_match_the_logistic_device_model(vb):
    p, n_data = 7, 45
    rng = np.random.RandomState(4)
    X = rng.randn(n_data, p) / np.sqrt(p)
    y = rng.randint(0, 2, size=n_data)
    soft = vb.SoftmaxRegressionModel(X, y, 2)
    logit = vb.LogisticRegressionModel(X, y.astype(float))
    theta = 0.3 * rng.randn(20, 2 * p)
    a = soft.pointwise_log_likelihood(theta)
    b = logit.pointwise_log_likelihood(theta[:, p:] - theta[:, :p])
    assert G.rel_err(a, b) < 1e-12, G.rel_err(a, b)


# ---- 4. ExclusiveKL --------------------------------------------------------------------------------------------------
def _mf_theta(D, seed):
    rng = np.random.RandomState(seed)
    return np.concatenate([0.3 * rng.randn(D), -1.0 + 0.1 * rng.randn(D)])


@pytest.mark.parametrize('C,p,n_data,N', SHAPES)
@pytest.mark.parametrize('rng_kind', ['numpy', 'philox'])
@pytest.mark.parametrize('pd', [False, True])
def test_exclusive_kl_meanfield(vb, C, p, n_data, N, rng_kind, pd):
    from viabel_amd import _lib
    from viabel_amd.objectives import _NOISE_SLOT
    model, omodel = _problem(vb, C, p, n_data)
    D = model.dim
    theta = _mf_theta(D, D + N)
    for fam, ofamily in ((vb.MFGaussian(D, seed=5, rng=rng_kind), ofam.MFGaussian(D)),
                         (vb.MFStudentT(D, 8.0, seed=5, rng=rng_kind), ofam.MFStudentT(D, 8.0))):
        value, grad = vb.ExclusiveKL(fam, model, N, use_path_deriv=pd)(theta)
        if rng_kind == 'numpy':
            noise = ofamily.draw_noise(np.random.RandomState(5), N)
        else:                                                     # the device's draws, read back
            noise = _lib.default_engine().noise_get_host(_NOISE_SLOT, N, D)
        ov, og = oobj.exclusive_kl(ofamily, omodel, theta, noise, use_path_deriv=pd)
        assert G.rel_err(value, ov) < 1e-12, (type(fam).__name__, value, ov)
        assert G.rel_err(grad, og) < 1e-11, (type(fam).__name__, G.rel_err(grad, og))


def _fr_theta(D, seed):
    rng = np.random.RandomState(seed)
    L = np.tril(0.05 * rng.randn(D, D), -1) + np.diag(np.exp(-1.0 + 0.2 * rng.randn(D)))
    return ofam.FullRankGaussian(D).pack(0.3 * rng.randn(D), L)


@pytest.mark.parametrize('C,p,n_data,N', SHAPES)
@pytest.mark.parametrize('pd', [False, True])
def test_exclusive_kl_fullrank(vb, C, p, n_data, N, pd):
    model, omodel = _problem(vb, C, p, n_data)
    D = model.dim
    theta = _fr_theta(D, D)
    value, grad = vb.ExclusiveKL(vb.FullRankGaussian(D, seed=4), model, N, use_path_deriv=pd)(theta)
    noise = np.random.RandomState(4).randn(N, D)
    ov, og = oobj.exclusive_kl(ofam.FullRankGaussian(D), omodel, theta, noise, use_path_deriv=pd)
    assert G.rel_err(value, ov) < 1e-12, (value, ov)
    assert G.rel_err(grad, og) < 1e-11, G.rel_err(grad, og)


@pytest.mark.parametrize('C,p,n_data,N', SHAPES)
@pytest.mark.parametrize('pd', [False, True])
def test_exclusive_kl_multivariate_t(vb, C, p, n_data, N, pd):
    model, omodel = _problem(vb, C, p, n_data)
    D = model.dim
    rng = np.random.RandomState(D)
    B = rng.randn(D, D)
    theta = np.concatenate([0.3 * rng.randn(D), ofam.psd_to_free(0.05 * (B @ B.T / D + 0.5 * np.eye(D)))])
    value, grad = vb.ExclusiveKL(vb.MultivariateT(D, 9.0, seed=6), model, N, use_path_deriv=pd)(theta)
    noise = ofam.MultivariateT(D, 9.0).draw_noise(np.random.RandomState(6), N)
    ov, og = oobj.exclusive_kl(ofam.MultivariateT(D, 9.0), omodel, theta, noise, pd)
    assert abs(value - ov) <= 1e-12 * abs(ov), (value, ov)
    np.testing.assert_allclose(grad, og, rtol=0, atol=1e-10 * np.max(np.abs(og)))      # (the source-model test's 1e-10)


@pytest.mark.parametrize('C,p,n_data,N', SHAPES)
def test_exclusive_kl_multivariate_t_philox(vb, C, p, n_data, N):
    """rng='philox': samples through the Cholesky factor; the device's draws are read back and the estimator is written
    out by hand, as tests/test_gpu_objectives.py does for the built-in targets."""
    from viabel_amd import _lib
    from viabel_amd.objectives import _NOISE_SLOT
    model, omodel = _problem(vb, C, p, n_data)
    D, df = model.dim, 9.0
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
    assert G.rel_err(value, ov) < 1e-12, (value, ov)
    assert G.rel_err(grad, og) < 1e-11, G.rel_err(grad, og)


@pytest.mark.parametrize('C,p,n_data,N', SHAPES)
@pytest.mark.parametrize('k', [1, 7, 20])
@pytest.mark.parametrize('pd', [False, True])
def test_exclusive_kl_lowrank(vb, C, p, n_data, N, k, pd):
    """k = 20 takes the any-rank route (k > 16)."""
    model, omodel = _problem(vb, C, p, n_data)
    D = model.dim
    rng = np.random.RandomState(D + N + k)
    fam, ofamily = vb.LRGaussian(D, seed=7, k=k), ofam.LRGaussian(D, k)
    theta = fam.pack(0.3 * rng.randn(D), -1.0 + 0.1 * rng.randn(D), 0.2 * rng.randn(D, k) / np.sqrt(k))
    value, grad = vb.ExclusiveKL(fam, model, N, use_path_deriv=pd)(theta)
    noise = ofamily.draw_noise(np.random.RandomState(7), N)
    ov, og = oobj.exclusive_kl(ofamily, omodel, theta, noise, pd)
    assert G.rel_err(value, ov) < (1e-10 if pd else 1e-12), (value, ov)                # (the source-model test's bounds)
    assert G.rel_err(grad, og) < (1e-9 if pd else 1e-11), G.rel_err(grad, og)


def _torch_logp_of(omodel):
    import torch
    Xt, sd = torch.from_numpy(omodel.X), omodel.prior_sd
    yi = torch.from_numpy(omodel.y)[None, :, None]
    const = omodel.dim * (np.log(sd) + 0.5 * np.log(2.0 * np.pi))

    def logp(x):
        eta = torch.einsum('ncj,ij->nic', x.reshape(-1, omodel.C, omodel.p), Xt)
        picked = torch.gather(eta, 2, yi.expand(eta.shape[0], -1, -1))[:, :, 0]
        return torch.sum(picked - torch.logsumexp(eta, dim=2), dim=1) - 0.5 * torch.sum(x * x, dim=1) / sd ** 2 - const
    return logp


@pytest.mark.parametrize('C,p,n_data,N', SHAPES)
@pytest.mark.parametrize('pd', [False, True])
def test_exclusive_kl_nvp_flow(vb, C, p, n_data, N, pd):
    import _nvp_oracle as O
    model, omodel = _problem(vb, C, p, n_data)
    model._torch_logp = _torch_logp_of(omodel)
    D, K = model.dim, 2
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
    assert abs(value - ov) <= 1e-12 * max(1.0, abs(ov)), (value, ov)
    assert G.rel_err(grad, og) <= 1e-10, G.rel_err(grad, og)                         # (the flow tests' bound)


# ---- 5. AlphaDivergence ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', ['mf_gaussian', 'mf_student_t', 'fullrank', 'multivariate_t', 'lr_gaussian'])
@pytest.mark.parametrize('alpha', [0.5, 2.0])
def test_alpha_divergence(vb, family, alpha):
    C, p, n_data, N = SMALL
    model, omodel = _problem(vb, C, p, n_data)
    D = model.dim
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
    C, p, n_data, _ = SMALL
    N, ess = 600, 150
    model, omodel = _problem(vb, C, p, n_data)
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
    C, p, n_data, _ = SMALL
    N = 2048
    model, omodel = _problem(vb, C, p, n_data)
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
    C, p, n_data, _ = LARGE
    N = 512
    model, omodel = _problem(vb, C, p, n_data)
    D = model.dim
    theta = np.concatenate([_mf_theta(D, 17)[:D], -1.2 + 0.2 * np.random.RandomState(18).randn(D)])
    obj = vb.ExclusiveKL(vb.MFGaussian(D, seed=5), model, N, hessian_approx_method=method)
    value, grad = obj(theta)
    noise = np.random.RandomState(5).randn(N, D)
    ov, og = oobj.rge_literal(ofam.MFGaussian(D), omodel, theta, noise, method)
    assert G.rel_err(value, ov) < 1e-12, (value, ov)
    assert G.rel_err(grad, og) < 1e-8, G.rel_err(grad, og)                            # (the source-model test's bound)
    plain = vb.ExclusiveKL(vb.MFGaussian(D, seed=5), model, N)(theta)[1]
    assert G.rel_err(grad, plain) > 1e-4                     # the control variate really changed the estimate
    assert not obj.supports_device_fit()


def test_hessian_vector_product(vb):
    C, p, n_data, _ = SMALL
    N = 256
    model, omodel = _problem(vb, C, p, n_data)
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
    C, p, n_data, _ = SMALL
    model, _ = _problem(vb, C, p, n_data)
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
    C, p, n_data, _ = SMALL
    model, omodel = _problem(vb, C, p, n_data)
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
def test_bbvi_fit_learns_the_class_contrasts(vb, capsys):
    """C = 3, p = 3, n_data = 2000 from coefficients of scale 2; bbvi with a FullRankGaussian, path derivative, fixed seed.
    e = max |(b_c - b_0)_fit - (b_c - b_0)_MAP| (the contrasts: the likelihood does not see a common shift of the b_c).
    Numbers worked out on the CPU from the oracle for exactly this data: the Laplace standard deviations of the six
    contrasts at the MAP are 0.114 ... 0.161, so five of them are 0.805; the error of the initial parameter (mean zero)
    is 3.53.  Threshold 1.0: above 0.805, below 3.53; after the fit e must be below 0.5."""
    from scipy.optimize import minimize
    C, p, n_data = 3, 3, 2000
    rng = np.random.RandomState(7)
    B = 2.0 * rng.randn(C, p)
    X = rng.randn(n_data, p) / np.sqrt(p)
    y = np.argmax(X @ B.T + rng.gumbel(size=(n_data, C)), axis=1)
    model, omodel = vb.SoftmaxRegressionModel(X, y, C, 10.0), SoftmaxOracle(X, y, C, 10.0)
    D = model.dim
    r = minimize(lambda t: -omodel.logp(t)[0], np.zeros(D), jac=lambda t: -omodel.grad(t)[0], method='BFGS',
                 options=dict(gtol=1e-10))
    b_map = r.x.reshape(C, p)
    S = np.linalg.inv(-omodel.hessian(r.x))
    sd = [np.sqrt(S[c * p + j, c * p + j] + S[j, j] - 2 * S[c * p + j, j]) for c in range(1, C) for j in range(p)]
    threshold = 1.0
    assert 5.0 * max(sd) <= threshold, max(sd)

    def err(theta):
        b = theta[:D].reshape(C, p)
        return float(np.max(np.abs((b[1:] - b[0]) - (b_map[1:] - b_map[0]))))
    approx = vb.FullRankGaussian(D, seed=3, rng='philox')
    init = approx.init_param()
    e0 = err(init)
    assert e0 > threshold, e0
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
    model, omodel = _problem(vb, 3, 5, 33)
    good = model.device_spec()
    with pytest.raises(ValueError):                               # dim is no multiple of n_classes
        eng.set_model((_lib.MODEL_SOFTMAX, good[1] + 1, good[2].copy(), good[3].copy()))
    with pytest.raises(ValueError):                               # dim != n_classes * p
        eng.set_model((_lib.MODEL_SOFTMAX, 2 * good[1], good[2].copy(), good[3].copy()))
    bad_y = good[2].copy()
    bad_y[33 * 5] = 3.0                                           # a label == n_classes, past the Python check
    with pytest.raises(ValueError):
        eng.set_model((_lib.MODEL_SOFTMAX, good[1], bad_y, good[3].copy()))
    with pytest.raises(ValueError):
        model(np.zeros((2, model.dim + 1)))
    x = 0.3 * np.random.RandomState(0).randn(5, model.dim)
    assert G.rel_err(model(x), omodel.logp(x)) < 1e-12          # the context still works
    with pytest.raises(NotImplementedError, match='psisloo'):
        vb.loo(np.zeros(2 * model.dim), model=model, approx=vb.MFGaussian(model.dim), n_samples=10)
    logit = vb.LogisticRegressionModel(omodel.X, (omodel.y > 0).astype(float))
    logit(np.zeros(5))
    with pytest.raises(NotImplementedError):                      # vb_softmax_pointwise with another model bound
        eng.softmax_pointwise(np.zeros((2, 5)), 33)
