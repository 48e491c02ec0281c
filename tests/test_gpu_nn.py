"""NeuralNetRegressionModel (VB_MODEL_NEURALNET, csrc/vb_neuralnet.hip) on the GPU against the numpy oracle of
tests/_nn_oracle.py: the row pipeline (pack, pre-activation GEMM, forward and backward kernels, gradient GEMM, unpack), the
pointwise entry, the target under the objective x family routes a SourceModel takes (tests/test_gpu_softmax.py is the
template, with its tolerances: value 1e-12, gradient 1e-11 relative, 1e-10 / 1e-9 where that test uses them), and the
prediction entry vb_nn_predict (tests/test_gpu_predict.py is the template: 1e-12 * max|ref| per output vector, 1e-9 where
the smoothed weights come from the device)."""
import ctypes

import numpy as np
import pytest

import _golden as G
from _nn_oracle import KINDS, NeuralNetOracle, response
from oracle import families as ofam, objectives as oobj, psis as opsis

pytestmark = pytest.mark.gpu

SMALL, LARGE = (2, 2, 30, 100, 'gaussian'), (5, 11, 40, 333, 'logistic')      # (h, p, n_data, N, likelihood): D = 9 and 66
SHAPES = [SMALL, LARGE]
PKEYS = ('eta_mean', 'eta_var', 'mean', 'var', 'lpd')


@pytest.fixture(scope='module')
def vb():
    import viabel_amd
    from viabel_amd import _lib
    _lib.default_engine()
    return viabel_amd


_PROBLEMS = {}


def _problem(vb, h, p, n_data, kind, seed=0, prior_sd=1.5, noise_sd=0.7):
    """(device model, oracle) on X = randn / sqrt(p) and responses drawn at a random network; built once and shared."""
    key = (h, p, n_data, kind, seed, prior_sd, noise_sd)
    if key not in _PROBLEMS:
        rng = np.random.RandomState(1000 * h + 10 * p + n_data + seed)
        X = rng.randn(n_data, p) / np.sqrt(p)
        truth = NeuralNetOracle(X, np.zeros(n_data), h, kind)
        y = response(kind, rng, truth.eta(rng.randn(truth.dim))[0], noise_sd)
        _PROBLEMS[key] = (vb.NeuralNetRegressionModel(X, y, h, kind, prior_sd, noise_sd),
                          NeuralNetOracle(X, y, h, kind, prior_sd, noise_sd))
    return _PROBLEMS[key]


def _oracle_rows(omodel, x, pointwise=True):
    """f, grad and pointwise terms of the oracle, its (rows, n_data, h) temporaries bounded."""
    rows = x.shape[0]
    fo, go = np.empty(rows), np.empty((rows, omodel.dim))
    po = np.empty((rows, omodel.n_data)) if pointwise else None
    for r0 in range(0, rows, 512):
        s = slice(r0, r0 + 512)
        fo[s], go[s] = omodel.logp(x[s]), omodel.grad(x[s])
        if pointwise:
            po[s] = omodel.pointwise(x[s])
    return fo, go, po


# ---- 1. rows ---------------------------------------------------------------------------------------------------------
def _rows_cases():
    from viabel_amd import _lib
    chunk = _lib.nn_chunk_rows(4, 2000)
    return [(1, 1, 1, 1), (3, 5, 33, 100), (7, 17, 130, 257), (2, 3, 1023, 9), (2, 3, 1024, 9), (2, 3, 1025, 9),
            (32, 16, 300, 600), (4, 3, 2000, 2 * chunk + 5)]


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('h,p,n_data,rows', _rows_cases())
def test_rows_against_oracle(vb, h, p, n_data, rows, kind):
    """model(x), model.grad(x), pointwise_log_likelihood(x), each called twice.  p = 17: odd, no multiple of 16; n_data =
    1023 / 1024 / 1025: the forward kernel's strip of 1024 observations, and (few output tiles, n_data >= 256) the split
    branch of the gradient GEMM; (3, 5, 33): its unsplit branch for a short contraction, (32, 16, 300, 600): for 300 output
    tiles; the last case: three row chunks (two full ones and a remainder)."""
    from viabel_amd import _lib
    model, omodel = _problem(vb, h, p, n_data, kind)
    assert model.dim == h * (p + 2) + 1
    if n_data == 2000:
        assert 2 * _lib.nn_chunk_rows(h, n_data) < rows <= 3 * _lib.nn_chunk_rows(h, n_data)      # three chunks
    x = 0.5 * np.random.RandomState(rows).randn(rows, model.dim)
    fo, go, po = _oracle_rows(omodel, x)
    f, g, pw = model(x), model.grad(x), model.pointwise_log_likelihood(x)
    assert f.shape == (rows,) and g.shape == (rows, model.dim) and pw.shape == (rows, n_data)
    ef, eg, ep = G.rel_err(f, fo), G.rel_err(g, go), G.rel_err(pw, po)
    print('rows %s h=%d p=%d n_data=%d rows=%d: rel err f %.2e grad %.2e pointwise %.2e' % (kind, h, p, n_data, rows, ef, eg, ep))
    assert ef < 1e-12 and eg < 1e-11 and ep < 1e-12, (ef, eg, ep)
    assert np.array_equal(model(x), f) and np.array_equal(model.grad(x), g)        # no atomics: the same bits
    assert np.array_equal(model.pointwise_log_likelihood(x), pw)
    assert model(x[0]).shape == (1,) and model.grad(x[0]).shape == (model.dim,)
    # the row sums of the pointwise terms plus the prior are the log density
    assert G.rel_err(pw.sum(axis=1) + omodel.log_prior(x), f) < 1e-12


# ---- 2. exact structure ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('h,p,n_data', [(3, 5, 33), (2, 3, 1025)])
def test_zero_output_weights_leave_the_hidden_layer_its_prior(vb, h, p, n_data, kind):
    """v = 0: delta = 0, so the w and a entries of the gradient are -theta / sd^2 (both branches of the gradient GEMM)."""
    model, omodel = _problem(vb, h, p, n_data, kind)
    x = 0.5 * np.random.RandomState(3).randn(20, model.dim)
    x[:, h * p + h:h * p + 2 * h] = 0.0
    g = model.grad(x)
    want = -x[:, :h * p + h] / model.prior_sd ** 2
    assert np.max(np.abs(g[:, :h * p + h] - want)) <= 1e-15 * np.max(np.abs(want))
    assert G.rel_err(g, omodel.grad(x)) < 1e-11


@pytest.mark.parametrize('kind', KINDS)
def test_permuting_the_hidden_units_permutes_the_gradient(vb, kind):
    h, p, n_data = 7, 17, 130
    model, _ = _problem(vb, h, p, n_data, kind)
    rng = np.random.RandomState(8)
    x = 0.5 * rng.randn(12, model.dim)
    perm = rng.permutation(h)
    assert not np.array_equal(perm, np.arange(h))

    def permuted(t):
        W, a, v, c = model.unpack(t)
        return np.concatenate([W[:, perm].reshape(t.shape[0], h * p), a[:, perm], v[:, perm], c[:, None]], axis=1)
    xp = permuted(x)
    f, fp = model(x), model(xp)
    assert np.max(np.abs(f - fp)) <= 1e-13 * np.max(np.abs(f))
    assert G.rel_err(model.grad(xp), permuted(model.grad(x))) < 1e-13


# ---- 3. saturation -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
def test_saturated_units_and_large_outputs_stay_finite(vb, kind):
    """Row 0 of X is scaled until its pre-activations reach +-40 (t = +-1, delta = 0 there); for the logistic likelihood the
    output weights are scaled until |eta| reaches 40 as well."""
    h, p, n_data = 3, 5, 33
    rng = np.random.RandomState(5)
    X = rng.randn(n_data, p) / np.sqrt(p)
    x = rng.randn(40, h * (p + 2) + 1)
    x[:, h * p:h * p + h] *= 0.5
    probe = NeuralNetOracle(X, np.zeros(n_data), h, kind)
    X[0] *= 40.0 / np.max(np.abs(probe.pre(x)[:, 0, :] - x[:, h * p:h * p + h]))      # (x_0' w_k: the biases do not scale)
    probe = NeuralNetOracle(X, np.zeros(n_data), h, kind)
    assert 36.0 < np.max(np.abs(probe.pre(x))) < 44.0
    if kind == 'logistic':
        x[:, h * p + h:h * p + 2 * h] *= 40.0 / np.max(np.abs(probe.eta(x) - x[:, -1:]))
        x[:, -1] *= 0.5
        assert 36.0 < np.max(np.abs(probe.eta(x))) < 44.0
    else:
        x[:, h * p + h:] *= 0.3
    y = response(kind, rng, probe.eta(x[0])[0], 0.7)
    model = vb.NeuralNetRegressionModel(X, y, h, kind, prior_sd=2.0, noise_sd=0.7)
    omodel = NeuralNetOracle(X, y, h, kind, prior_sd=2.0, noise_sd=0.7)
    f, g, pw = model(x), model.grad(x), model.pointwise_log_likelihood(x)
    assert np.all(np.isfinite(f)) and np.all(np.isfinite(g)) and np.all(np.isfinite(pw))
    assert G.rel_err(f, omodel.logp(x)) < 1e-12
    assert G.rel_err(g, omodel.grad(x)) < 1e-11
    assert G.rel_err(pw, omodel.pointwise(x)) < 1e-12
    out = model.predict_from_draws(x, X_new=X[:4], y_new=y[:4])
    ref = omodel.predict(x, X[:4], y[:4])
    for k in PKEYS:
        assert np.all(np.isfinite(out[k])) and np.max(np.abs(out[k] - ref[k])) <= 1e-12 * np.max(np.abs(ref[k])), k


# ---- 4. gradient self-check ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
def test_check_gradient(vb, kind):
    model, _ = _problem(vb, 3, 5, 33, kind)
    x = 0.5 * np.random.RandomState(1).randn(3, model.dim)
    assert model.check_gradient(x) < 1e-6


# ---- 5. ExclusiveKL ------------------------------------------------------------------------------------------------------
def _mf_theta(D, seed):
    rng = np.random.RandomState(seed)
    return np.concatenate([0.3 * rng.randn(D), -1.0 + 0.1 * rng.randn(D)])


@pytest.mark.parametrize('h,p,n_data,N,kind', SHAPES)
@pytest.mark.parametrize('rng_kind', ['numpy', 'philox'])
@pytest.mark.parametrize('pd', [False, True])
def test_exclusive_kl_meanfield(vb, h, p, n_data, N, kind, rng_kind, pd):
    from viabel_amd import _lib
    from viabel_amd.objectives import _NOISE_SLOT
    model, omodel = _problem(vb, h, p, n_data, kind)
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


@pytest.mark.parametrize('h,p,n_data,N,kind', SHAPES)
@pytest.mark.parametrize('pd', [False, True])
def test_exclusive_kl_fullrank(vb, h, p, n_data, N, kind, pd):
    model, omodel = _problem(vb, h, p, n_data, kind)
    D = model.dim
    theta = _fr_theta(D, D)
    value, grad = vb.ExclusiveKL(vb.FullRankGaussian(D, seed=4), model, N, use_path_deriv=pd)(theta)
    noise = np.random.RandomState(4).randn(N, D)
    ov, og = oobj.exclusive_kl(ofam.FullRankGaussian(D), omodel, theta, noise, use_path_deriv=pd)
    assert G.rel_err(value, ov) < 1e-12, (value, ov)
    assert G.rel_err(grad, og) < 1e-11, G.rel_err(grad, og)


@pytest.mark.parametrize('h,p,n_data,N,kind', SHAPES)
@pytest.mark.parametrize('pd', [False, True])
def test_exclusive_kl_multivariate_t(vb, h, p, n_data, N, kind, pd):
    model, omodel = _problem(vb, h, p, n_data, kind)
    D = model.dim
    rng = np.random.RandomState(D)
    B = rng.randn(D, D)
    theta = np.concatenate([0.3 * rng.randn(D), ofam.psd_to_free(0.05 * (B @ B.T / D + 0.5 * np.eye(D)))])
    value, grad = vb.ExclusiveKL(vb.MultivariateT(D, 9.0, seed=6), model, N, use_path_deriv=pd)(theta)
    noise = ofam.MultivariateT(D, 9.0).draw_noise(np.random.RandomState(6), N)
    ov, og = oobj.exclusive_kl(ofam.MultivariateT(D, 9.0), omodel, theta, noise, pd)
    assert abs(value - ov) <= 1e-12 * abs(ov), (value, ov)
    np.testing.assert_allclose(grad, og, rtol=0, atol=1e-10 * np.max(np.abs(og)))      # (the softmax test's 1e-10)


@pytest.mark.parametrize('h,p,n_data,N,kind', SHAPES)
@pytest.mark.parametrize('k', [1, 20])
@pytest.mark.parametrize('pd', [False, True])
def test_exclusive_kl_lowrank(vb, h, p, n_data, N, kind, k, pd):
    """k = 20 takes the any-rank route (k > 16)."""
    model, omodel = _problem(vb, h, p, n_data, kind)
    D = model.dim
    rng = np.random.RandomState(D + N + k)
    fam, ofamily = vb.LRGaussian(D, seed=7, k=k), ofam.LRGaussian(D, k)
    theta = fam.pack(0.3 * rng.randn(D), -1.0 + 0.1 * rng.randn(D), 0.2 * rng.randn(D, k) / np.sqrt(k))
    value, grad = vb.ExclusiveKL(fam, model, N, use_path_deriv=pd)(theta)
    noise = ofamily.draw_noise(np.random.RandomState(7), N)
    ov, og = oobj.exclusive_kl(ofamily, omodel, theta, noise, pd)
    assert G.rel_err(value, ov) < (1e-10 if pd else 1e-12), (value, ov)                # (the softmax test's bounds)
    assert G.rel_err(grad, og) < (1e-9 if pd else 1e-11), G.rel_err(grad, og)


def _torch_logp_of(o):
    import torch
    X, y = torch.from_numpy(o.X), torch.from_numpy(o.y)
    h, p, sd, ns = o.h, o.p, o.prior_sd, o.noise_sd
    const = o.dim * (np.log(sd) + 0.5 * np.log(2.0 * np.pi))

    def logp(x):
        W = x[:, :h * p].reshape(-1, h, p)
        a, v, c = x[:, h * p:h * p + h], x[:, h * p + h:h * p + 2 * h], x[:, -1]
        t = torch.tanh(torch.einsum('nkj,ij->nik', W, X) + a[:, None, :])
        eta = c[:, None] + torch.sum(t * v[:, None, :], dim=2)
        if o.kind == 'gaussian':
            ll = -0.5 * ((y - eta) / ns) ** 2 - np.log(ns) - 0.5 * np.log(2.0 * np.pi)
        else:
            assert o.kind == 'logistic'
            ll = y * eta - torch.nn.functional.softplus(eta)
        return torch.sum(ll, dim=1) - 0.5 * torch.sum(x * x, dim=1) / sd ** 2 - const
    return logp


@pytest.mark.parametrize('h,p,n_data,N,kind', SHAPES)
@pytest.mark.parametrize('pd', [False, True])
def test_exclusive_kl_nvp_flow(vb, h, p, n_data, N, kind, pd):
    import _nvp_oracle as O
    model, omodel = _problem(vb, h, p, n_data, kind)
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


# ---- 6. AlphaDivergence ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', ['mf_gaussian', 'mf_student_t', 'fullrank', 'multivariate_t', 'lr_gaussian'])
@pytest.mark.parametrize('alpha', [0.5, 2.0])
def test_alpha_divergence(vb, family, alpha):
    h, p, n_data, N, _ = SMALL
    model, omodel = _problem(vb, h, p, n_data, 'poisson')
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
        tol_g = 1e-10                                             # (the softmax test of this route)
    else:
        k = 2
        approx, ofamily = vb.LRGaussian(D, seed=2, k=k), ofam.LRGaussian(D, k)
        theta = np.concatenate([0.3 * rng.randn(D), -0.7 + 0.2 * rng.randn(D), 0.3 * rng.randn(D * k) / np.sqrt(k)])
        tol_v, tol_g = 1e-11, 1e-9                                # (the softmax test of this route)
    np.random.seed(11)
    value, grad = vb.AlphaDivergence(approx, model, N, alpha)(theta)
    np.random.seed(11)
    noise = ofamily.draw_noise(np.random.RandomState(np.random.randint(2 ** 32)), N)
    ov, og = oobj.alpha_divergence(ofamily, omodel, theta, noise, alpha)
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
    """Three calls with a moving theta (refresh on even steps), the structure of the softmax DIS tests."""
    h, p, n_data, _, kind = SMALL
    N, ess = 600, 150
    model, omodel = _problem(vb, h, p, n_data, kind)
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


# ---- 8. device-resident fit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', ['mf_gaussian', 'fullrank'])
def test_device_fit_matches_host_loop(vb, capsys, family):
    from viabel_amd.optimization import RMSProp
    h, p, n_data, _, kind = SMALL
    model, _ = _problem(vb, h, p, n_data, kind)
    D = model.dim
    hist = {}
    for on_device in (False, True):
        fam = vb.MFGaussian(D, rng='philox', seed=3) if family == 'mf_gaussian' else vb.FullRankGaussian(D, rng='philox', seed=3)
        obj = vb.ExclusiveKL(fam, model, 128)
        assert obj.supports_device_fit()
        res = RMSProp(0.02).optimize(50, obj, fam.init_param(), on_device=on_device)
        hist[on_device] = np.asarray(res['value_history'])
    capsys.readouterr()
    assert hist[True].shape == (50,)
    np.testing.assert_array_equal(hist[False], hist[True])


# ---- 9. prediction -----------------------------------------------------------------------------------------------------
def _log_weights(which, S, rng):
    """The three weight vectors of tests/test_gpu_predict.py."""
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


def _assert_close(out, ref, what, rel=1e-12, keys=PKEYS):
    for k in keys:
        tol = rel * np.max(np.abs(ref[k]))
        err = np.max(np.abs(out[k] - ref[k]))
        assert err <= tol, (what, k, err, tol)


@pytest.mark.parametrize('kind', KINDS)
def test_predict_grid_against_oracle(vb, kind):
    """Every (m, S, weights) against numpy at 1e-12 * max|ref| per output vector; every call twice, bit for bit; without a
    response the four other vectors are the same bits."""
    h, p = 3, 5
    model, omodel = _problem(vb, h, p, 5, kind)            # the prediction takes h, p, link and noise_sd from the model
    worst = dict.fromkeys(PKEYS, 0.0)
    for m in (1, 33, 300):
        for S in (1, 2, 255, 256, 257, 4097):
            rng = np.random.RandomState(1000 * m + S)
            X_new = rng.randn(m, p) / np.sqrt(p)
            x = 0.7 * rng.randn(S, model.dim)
            y_new = response(kind, rng, omodel.eta(x[:1], X_new)[0], 0.7)
            for which in ('none', 't', 'peaked'):
                lw = _log_weights(which, S, np.random.RandomState(S + len(which)))
                what = (kind, m, S, which)
                out = model.predict_from_draws(x, X_new=X_new, y_new=y_new, log_weights=lw)
                again = model.predict_from_draws(x, X_new=X_new, y_new=y_new, log_weights=lw)
                ref = omodel.predict(x, X_new, y_new, lw)
                for k in PKEYS:
                    assert out[k].shape == (m,) and np.array_equal(out[k], again[k]), (what, k)
                    scale = np.max(np.abs(ref[k]))
                    if scale > 0:
                        worst[k] = max(worst[k], np.max(np.abs(out[k] - ref[k])) / scale)
                _assert_close(out, ref, what)
                if S == 1 or which == 'peaked':
                    assert np.all(out['eta_var'] == 0.0), what
                no_y = model.predict_from_draws(x, X_new=X_new, log_weights=lw)
                assert 'lpd' not in no_y and all(np.array_equal(no_y[k], out[k]) for k in PKEYS[:4]), what
    print('%s: largest error / max|ref| per output: %s' % (kind, ', '.join('%s %.3g' % kv for kv in worst.items())))


@pytest.mark.parametrize('kind', KINDS)
def test_predict_bound_design(vb, kind):
    h, p, n, S = 3, 5, 300, 777
    model, omodel = _problem(vb, h, p, n, kind)
    rng = np.random.RandomState(31)
    x = 0.5 * rng.randn(S, model.dim)
    log_w, _ = opsis.psis_smooth(0.8 * rng.standard_t(5.0, S))
    bound = model.predict_from_draws(x, log_weights=log_w)
    given = model.predict_from_draws(x, X_new=model.X, y_new=model.y, log_weights=log_w)
    for k in PKEYS:
        assert np.array_equal(bound[k], given[k]), k
    _assert_close(bound, omodel.predict(x, log_w=log_w), kind)
    other_y = response(kind, rng, omodel.eta(x[1:2])[0], 0.7)      # the bound design with other responses
    mixed = model.predict_from_draws(x, y_new=other_y, log_weights=log_w)
    _assert_close(mixed, omodel.predict(x, y_new=other_y, log_w=log_w), kind)
    for k in PKEYS[:4]:
        assert np.array_equal(mixed[k], bound[k]), k
    # the lpd of the bound design is the weighted log-mean-exp of the pointwise terms
    pw = model.pointwise_log_likelihood(x)
    lw = log_w - np.logaddexp.reduce(log_w)
    want = np.logaddexp.reduce(lw[:, None] + pw, axis=0)
    assert np.max(np.abs(bound['lpd'] - want)) <= 1e-12 * np.max(np.abs(want))


def test_predict_chunks_of_observations(vb):
    """h = 16 and 4097 draws: 255 observations fit the budget of one pass, 45 are left for a second.  The observations on
    both sides of the boundary, the first and the last against numpy, with an uploaded design and with the bound one."""
    from viabel_amd import _lib
    h, p, m, S = 16, 2, 300, 4097
    chunk = _lib.nn_predict_chunk(h, S)
    assert chunk < m <= 2 * chunk
    model, omodel = _problem(vb, h, p, m, 'logistic')
    rng = np.random.RandomState(21)
    x = 0.5 * rng.randn(S, model.dim)
    log_w, _ = opsis.psis_smooth(0.5 * rng.standard_t(6.0, S))
    small, _ = _problem(vb, h, p, 5, 'logistic')
    out = small.predict_from_draws(x, X_new=model.X, y_new=model.y, log_weights=log_w)
    pick = np.array([0, 1, chunk - 2, chunk - 1, chunk, chunk + 1, m - 1])
    ref = omodel.predict(x, model.X[pick], model.y[pick], log_w)
    _assert_close({k: out[k][pick] for k in PKEYS}, ref, 'uploaded design')
    assert all(np.all(np.isfinite(out[k])) for k in PKEYS)
    bound = model.predict_from_draws(x, log_weights=log_w)
    for k in PKEYS:
        assert np.array_equal(bound[k], out[k]), k


def test_predict_end_to_end_after_a_device_fit(vb, capsys):
    """A noisy sine, h = 8: the fit lowers the objective, and predict() equals the oracle on the same draws and
    device-smoothed weights."""
    from viabel_amd.optimization import Adam
    h, n = 8, 200
    rng = np.random.RandomState(4)
    X = np.linspace(-2.0, 2.0, n)[:, None]
    y = np.sin(2.0 * X[:, 0]) + 0.2 * rng.randn(n)
    model = vb.NeuralNetRegressionModel(X, y, h, 'gaussian', prior_sd=3.0, noise_sd=0.2)
    omodel = NeuralNetOracle(X, y, h, 'gaussian', prior_sd=3.0, noise_sd=0.2)
    D = model.dim
    X_new = np.linspace(-2.2, 2.2, 50)[:, None]
    y_new = np.sin(2.0 * X_new[:, 0]) + 0.2 * rng.randn(50)
    objective = vb.ExclusiveKL(vb.MFGaussian(D, seed=3, rng='philox'), model, 64)
    init = np.concatenate([0.5 * rng.randn(D), np.full(D, -2.0)])
    fit = Adam(0.02, iterate_avg_prop=None).optimize(600, objective, init, on_device=True)
    capsys.readouterr()
    hist = np.asarray(fit['value_history'])
    assert hist.shape == (600,) and np.all(np.isfinite(hist))
    assert np.mean(hist[-100:]) < np.mean(hist[:100]), (np.mean(hist[:100]), np.mean(hist[-100:]))
    theta = fit['opt_param']
    for weights in ('psis', None):
        res = vb.predict(theta, model=model, approx=vb.MFGaussian(D, seed=5), X_new=X_new, y_new=y_new, n_samples=4096,
                         weights=weights)
        printed = capsys.readouterr().out
        assert 'elpd = ' in printed and ('khat' in printed) == (weights == 'psis')
        samples, log_ratios = vb.samples_and_log_weights(theta, model, vb.MFGaussian(D, seed=5), 4096)
        log_w = None if weights is None else opsis.psis_smooth(log_ratios, 1.0)[0]
        ref = omodel.predict(samples, X_new, y_new, log_w)
        dev = dict(eta_mean=res['eta_mean'], eta_var=res['eta_sd'] ** 2, mean=res['mean'], var=res['sd'] ** 2, lpd=res['lpd'])
        print('weights %s: device - numpy %s' % (weights, ', '.join('%s %.3g' % (k, np.max(np.abs(dev[k] - ref[k]))) for k in PKEYS)))
        for k in PKEYS:
            np.testing.assert_allclose(dev[k], ref[k], rtol=0, atol=1e-9, err_msg=k)
        assert abs(res['elpd'] - ref['lpd'].sum()) <= 50e-9
        assert res['n_samples'] == 4096 and np.all(res['sd'] > 0)
    no_y = vb.predict(theta, model=model, approx=vb.MFGaussian(D, seed=5), X_new=X_new, n_samples=4096)
    assert 'lpd' not in no_y and 'elpd' not in no_y and 'no response' in capsys.readouterr().out


# ---- 10. errors ------------------------------------------------------------------------------------------------------
def test_errors_leave_the_context_usable(vb):
    from viabel_amd import _lib
    fresh = _lib.Engine()
    try:
        with pytest.raises(_lib.EngineError):                               # no model bound
            fresh.nn_predict(np.zeros((4, 6)), 1, X_new=np.zeros((2, 1)))
        with pytest.raises(_lib.EngineError):
            fresh.nn_pointwise(np.zeros((4, 6)), 3)
        fresh.set_model(vb.GaussianModel(np.zeros(6), np.ones(6)).device_spec())
        with pytest.raises(NotImplementedError):                            # bound, but another target
            fresh.nn_predict(np.zeros((4, 6)), 1, X_new=np.zeros((2, 1)))
        with pytest.raises(NotImplementedError):
            fresh.nn_pointwise(np.zeros((4, 6)), 3)
    finally:
        fresh.close()
    eng = _lib.default_engine()
    h, p, n = 3, 5, 33
    model, omodel = _problem(vb, h, p, n, 'logistic')
    D = model.dim
    x = 0.5 * np.random.RandomState(0).randn(8, D)
    X_new = np.random.RandomState(1).randn(4, p)

    def still_works():
        eng.set_model(model.device_spec())
        assert G.rel_err(model(x), omodel.logp(x)) < 1e-12
        _assert_close(model.predict_from_draws(x, X_new=X_new), omodel.predict(x, X_new), 'after an error', keys=PKEYS[:4])
    still_works()
    good = model.device_spec()
    for bad in ((_lib.MODEL_NEURALNET, good[1] + 1, good[2].copy(), good[3].copy()),                 # dim != h (p + 2) + 1
                (_lib.MODEL_NEURALNET, good[1], good[2][:-1].copy(), good[3].copy()),               # no noise_sd
                (_lib.MODEL_NEURALNET, good[1], good[2].copy(), np.array([n, h, 7], dtype=np.int64))):      # unknown link
        with pytest.raises(ValueError):
            eng.set_model(bad)
        still_works()
    for call in (lambda: model(np.zeros((2, D + 1))),
                 lambda: eng.nn_pointwise(np.zeros((2, D - 1)), n),                                  # a wrong d (the C entry)
                 lambda: eng.nn_predict(np.zeros((8, D - 1)), p),
                 lambda: eng.nn_predict(x, p, X_new=np.zeros((4, p + 1))),                           # columns of X_new
                 lambda: eng.nn_predict(x, p, log_w=np.zeros(7)),                                    # length of log_w
                 lambda: eng.nn_predict(x, p, X_new=X_new, y_new=np.zeros(5)),                       # length of y_new
                 lambda: eng.nn_predict(x, p, y_new=np.zeros(n - 1)),                                # ... against the bound design
                 lambda: eng.nn_predict(x, p, log_w=np.full(8, -np.inf)),                            # no finite weight
                 lambda: model.predict_from_draws(x, log_weights=np.full(8, -np.inf))):
        with pytest.raises(ValueError):
            call()
        still_works()
    # the C entry's own checks, behind the Python ones
    ptr = lambda a: ctypes.cast(a.ctypes.data, ctypes.POINTER(ctypes.c_double))                # noqa: E731
    o = [np.zeros(n) for _ in range(5)]
    xs, Xn, yn, inf = np.ascontiguousarray(x), np.ascontiguousarray(X_new), np.zeros(4), np.full(8, -np.inf)
    lib, ctx = eng._lib, eng._ctx
    call = lib.vb_nn_predict
    assert call(ctx, ptr(xs), 8, D, None, ptr(Xn), 4, ptr(yn), ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(o[3]), None) == _lib.VB_ERR_INVALID
    assert call(ctx, ptr(xs), 8, D, None, ptr(Xn), 4, None, ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(o[3]), ptr(o[4])) == _lib.VB_ERR_INVALID
    assert call(ctx, ptr(xs), 8, D, None, None, n - 1, None, ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(o[3]), ptr(o[4])) == _lib.VB_ERR_INVALID
    assert call(ctx, ptr(xs), 8, D, None, ptr(Xn), 0, None, ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(o[3]), None) == _lib.VB_ERR_INVALID
    assert call(ctx, ptr(xs), 0, D, None, ptr(Xn), 4, None, ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(o[3]), None) == _lib.VB_ERR_INVALID
    assert call(ctx, ptr(xs), 8, D + 1, None, ptr(Xn), 4, None, ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(o[3]), None) == _lib.VB_ERR_INVALID
    assert call(ctx, ptr(xs), 8, D, ptr(inf), ptr(Xn), 4, None, ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(o[3]), None) == _lib.VB_ERR_INVALID
    assert call(ctx, ptr(xs), 8, D, None, ptr(Xn), 4, None, ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(o[3]), None) == _lib.VB_OK
    still_works()
    logit = vb.LogisticRegressionModel(omodel.X, omodel.y)
    logit(np.zeros(p))
    with pytest.raises(NotImplementedError):                      # another model bound
        eng.nn_pointwise(np.zeros((2, p)), n)
    with pytest.raises(NotImplementedError):
        eng.nn_predict(np.zeros((2, p)), p)
    still_works()
    with pytest.raises(NotImplementedError, match='psisloo'):     # loo() is not changed
        vb.loo(np.zeros(2 * D), model=model, approx=vb.MFGaussian(D), n_samples=10)
