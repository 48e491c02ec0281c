"""SparseRegressionModel (VB_MODEL_SPARSE_GLM, csrc/vb_sparse.hip) on the GPU: the row pipeline (transpose, CSR gather, link,
CSC gather, transpose back, row sums; the segment route of long rows and columns; three row chunks) against the numpy oracle
of tests/_sparse_oracle.py and against the dense device targets on ``model.to_dense()``; a design the dense targets cannot
hold against numpy on the CSR arrays; the target under the objective x family routes a SourceModel takes, against the same
objective on the dense target with the same seeds where the dense target takes the route (ExclusiveKL with the mean-field
and full-rank families, NVPFlow) and against the oracle's objective on the same noise where it does not (the control
variates, AlphaDivergence, DISInclusiveKL, LRGaussian); the device-resident fit; interleaving with a dense model on one engine;
errors.  Tolerances are the rows targets' (tests/test_gpu_locscale.py): value and pointwise 1e-12, gradient 1e-11 relative,
1e-10 / 1e-9 where the source-model tests of the same route use them.  Matrices are built with numpy alone."""
import math

import numpy as np
import pytest

import _golden as G
from _sparse_oracle import SparseGLMOracle, terms

pytestmark = pytest.mark.gpu

LIKELIHOODS = ['logistic', 'poisson', 'gaussian']
PRIOR_SD, NOISE_SD = 3.0, 0.8


@pytest.fixture(scope='module')
def vb():
    import viabel_amd
    from viabel_amd import _lib
    _lib.default_engine()
    return viabel_amd


def _random_rows(rng, n_data, p, per_row):
    """(n_data, p) with `per_row` non-zeros randn / sqrt(per_row) in every row."""
    A = np.zeros((n_data, p))
    k = min(per_row, p)
    for i in range(n_data):
        A[i, rng.choice(p, size=k, replace=False)] = rng.randn(k) / np.sqrt(k)
    return A


def _design(name):
    """The dense form of the case's design and its number of sample rows."""
    from viabel_amd import _lib
    S = _lib.SPARSE_SEGMENT
    rng = np.random.RandomState(sum(map(ord, name)))
    if name == 'smallest':
        return _random_rows(rng, 1, 1, 1), 1
    if name == 'odd':
        return _random_rows(rng, 33, 17, 3), 100
    if name == 'full':
        return _random_rows(rng, 130, 5, 5), 257
    if name == 'empty':
        A = _random_rows(rng, 300, 38, 2)
        A = np.concatenate([np.zeros((300, 1)), A, np.zeros((300, 1))], axis=1)      # columns 0 and 39 empty
        A[7:9] = 0.0                                                                 # rows 7 and 8 empty
        return A, 64
    if name == 'long_column':
        n = 2 * S + 5
        A = np.zeros((n, 7))
        A[:, 0] = 1.0                                                                # the intercept: three segments
        A[:, 1:] = _random_rows(rng, n, 6, 2)
        A[:, 1:3] = 0.0
        A[rng.choice(n, size=S, replace=False), 1] = rng.randn(S) / np.sqrt(2.0)     # exactly one segment
        A[rng.choice(n, size=S + 1, replace=False), 2] = rng.randn(S + 1) / np.sqrt(2.0)      # one entry past it
        return A, 65
    if name == 'long_row':
        p = 2 * S + 5
        A = _random_rows(rng, 12, p, 3)
        A[3] = rng.randn(p) / np.sqrt(p)                                             # a full row: three segments
        A[5], A[6] = 0.0, 0.0
        A[5, rng.choice(p, size=S, replace=False)] = rng.randn(S) / np.sqrt(S)
        A[6, rng.choice(p, size=S + 1, replace=False)] = rng.randn(S + 1) / np.sqrt(S + 1)
        return A, 65
    if name == 'chunks':
        return _random_rows(rng, 2500, 30, 4), 2 * _lib.sparse_chunk_rows(2500, 30) + 5
    raise KeyError(name)


CASES = ['smallest', 'odd', 'full', 'empty', 'long_column', 'long_row', 'chunks']
_DESIGNS, _PROBLEMS = {}, {}


def _response(lik, eta, rng):
    if lik == 'logistic':
        return (rng.rand(eta.size) < 1.0 / (1.0 + np.exp(-eta))).astype(float)
    if lik == 'poisson':
        return rng.poisson(np.exp(eta)).astype(float)
    return eta + NOISE_SD * rng.randn(eta.size)


def _problem(vb, name, lik):
    """(sparse model, oracle, the dense device model on the same matrix, sample rows); built once per case and shared."""
    if (name, lik) not in _PROBLEMS:
        if name not in _DESIGNS:
            _DESIGNS[name] = _design(name)
        A, rows = _DESIGNS[name]
        rng = np.random.RandomState(7 + len(name))
        y = _response(lik, A @ (0.3 * rng.randn(A.shape[1])), rng)
        model = vb.SparseRegressionModel.from_dense(A, y, likelihood=lik, prior_sd=PRIOR_SD, noise_sd=NOISE_SD)
        if lik == 'logistic':
            dense = vb.LogisticRegressionModel(A, y, PRIOR_SD)
        elif lik == 'poisson':
            dense = vb.PoissonRegressionModel(A, y, PRIOR_SD)
        else:
            dense = vb.LinearRegressionModel(A, y, PRIOR_SD, NOISE_SD)
        _PROBLEMS[(name, lik)] = (model, SparseGLMOracle(A, y, lik, PRIOR_SD, NOISE_SD), dense, rows)
    return _PROBLEMS[(name, lik)]


def _oracle_rows(omodel, x):
    """f, gradient and per-observation terms of the oracle in slices of 512 rows (its (rows, n_data) temporaries, bounded)."""
    rows = x.shape[0]
    fo, go, po = np.empty(rows), np.empty((rows, omodel.dim)), np.empty((rows, omodel.n_data))
    for r0 in range(0, rows, 512):
        s = slice(r0, r0 + 512)
        fo[s], go[s], po[s] = omodel.logp(x[s]), omodel.grad(x[s]), omodel.pointwise(x[s])
    return fo, go, po


# ---- 1. rows ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', CASES)
@pytest.mark.parametrize('lik', LIKELIHOODS)
def test_rows_against_oracle_and_dense_target(vb, lik, name):
    """model(x), model.grad(x), pointwise_log_likelihood(x) against the numpy oracle and against the dense device target on
    the same matrix.  'smallest': (1, 1, 1) and one row; 'odd': p = 17, 100 rows (no multiple of 64); 'full': every row full,
    a dense matrix given sparsely, 257 rows (five blocks of samples); 'empty': rows 7, 8 and columns 0, 39 without entries;
    'long_column': an intercept of 2 SEGMENT + 5 ones (three segments), a column of exactly SEGMENT entries (the last one a
    single wave takes) and one of SEGMENT + 1 (two segments); 'long_row': the same for rows; 'chunks': exactly three row
    chunks (two full ones and a remainder of 5 rows)."""
    from viabel_amd import _lib
    model, omodel, dense, rows = _problem(vb, name, lik)
    n_data, p = omodel.n_data, omodel.dim
    S = _lib.SPARSE_SEGMENT
    if name == 'chunks':
        chunk = _lib.sparse_chunk_rows(n_data, p)
        assert 2 * chunk < rows <= 3 * chunk                      # exactly three chunks
    if name == 'long_column':
        assert sorted(np.diff(model.csc[2])[:3]) == [S, S + 1, 2 * S + 5]
    if name == 'long_row':
        assert list(np.diff(model.csr[2])[[3, 5, 6]]) == [2 * S + 5, S, S + 1]
    if name == 'empty':
        assert np.diff(model.csr[2])[7] == np.diff(model.csr[2])[8] == 0
        assert np.diff(model.csc[2])[0] == np.diff(model.csc[2])[39] == 0
    if name == 'full':
        assert model.nnz == n_data * p
    assert model.dim == p and model.n_data == n_data
    x = 0.3 * np.random.RandomState(rows).randn(rows, p)
    fo, go, po = _oracle_rows(omodel, x)
    f, g, pw = model(x), model.grad(x), model.pointwise_log_likelihood(x)
    assert f.shape == (rows,) and g.shape == (rows, p) and pw.shape == (rows, n_data)
    ef, eg, ep = G.rel_err(f, fo), G.rel_err(g, go), G.rel_err(pw, po)
    print('rows %s %s n_data=%d p=%d rows=%d: rel err f %.2e grad %.2e pointwise %.2e' % (name, lik, n_data, p, rows, ef, eg, ep))
    assert np.array_equal(model(x), f) and np.array_equal(model.grad(x), g)        # no atomics: the same bits
    assert np.array_equal(model.pointwise_log_likelihood(x), pw)
    xd = x[:512]                                                  # the dense device target on the same matrix
    df, dg, dp = G.rel_err(f[:512], dense(xd)), G.rel_err(g[:512], dense.grad(xd)), \
        G.rel_err(pw[:512], dense.pointwise_log_likelihood(xd))
    print('     against the dense target: rel err f %.2e grad %.2e pointwise %.2e' % (df, dg, dp))
    cg = model.check_gradient(x[:3])
    print('     check_gradient %.2e' % cg)
    assert ef < 1e-12 and eg < 1e-11 and ep < 1e-12, (ef, eg, ep)
    assert df < 1e-12 and dg < 1e-11 and dp < 1e-12, (df, dg, dp)
    assert cg < 1e-6
    assert model(x[0]).shape == (1,) and model.grad(x[0]).shape == (p,)
    assert model.pointwise_log_likelihood(x[0]).shape == (1, n_data)


# ---- 2. a design the dense targets cannot hold -----------------------------------------------------------------------
def test_large_design_against_numpy_on_the_csr_arrays(vb):
    """n_data = 200 000, p = 50 000, ten entries per row (drawn with replacement: the few duplicates are summed by the
    constructor) plus an intercept, 64 draws.  Dense it would be 80 GB per operand copy.  The reference walks the CSR arrays
    with bincount; f is taken with math.fsum so that the reference's own rounding is not in the comparison."""
    n_data, p, k, rows = 200000, 50000, 10, 64
    rng = np.random.RandomState(11)
    cols = np.concatenate([np.zeros((n_data, 1), dtype=np.int64), rng.randint(1, p, size=(n_data, k))], axis=1)
    vals = np.concatenate([np.ones((n_data, 1)), rng.randn(n_data, k) / np.sqrt(k)], axis=1)
    y = (rng.rand(n_data) < 0.5).astype(float)
    model = vb.SparseRegressionModel((vals.ravel(), cols.ravel(), np.arange(n_data + 1) * (k + 1)), y, prior_sd=PRIOR_SD,
                                     shape=(n_data, p))
    v, c, ptr = model.csr
    assert (k + 1) * n_data - 1000 < model.nnz <= (k + 1) * n_data and np.diff(model.csc[2])[0] == n_data
    r = np.repeat(np.arange(n_data), np.diff(ptr))
    x = 0.3 * rng.randn(rows, p)
    x[:, 0] *= 0.1
    f, g = model(x), model.grad(x)
    assert np.array_equal(model(x), f) and np.array_equal(model.grad(x), g)
    fo, go = np.empty(rows), np.empty((rows, p))
    c0 = -p * (math.log(PRIOR_SD) + 0.5 * math.log(2.0 * math.pi))
    for s in range(rows):
        eta = np.bincount(r, weights=v * x[s, c], minlength=n_data)
        t, dl = terms('logistic', y, eta)
        fo[s] = math.fsum(t) + math.fsum(-0.5 * x[s] * x[s] / PRIOR_SD ** 2) + c0
        go[s] = np.bincount(c, weights=v * dl[r], minlength=p) - x[s] / PRIOR_SD ** 2
    ef, eg = G.rel_err(f, fo), G.rel_err(g, go)
    print('large design nnz=%d: rel err f %.2e grad %.2e' % (model.nnz, ef, eg))
    assert ef < 1e-12 and eg < 1e-11, (ef, eg)
    pw = model.pointwise_log_likelihood(x[:2])
    eta = np.stack([np.bincount(r, weights=v * x[s, c], minlength=n_data) for s in range(2)])
    ep = G.rel_err(pw, terms('logistic', y, eta)[0])
    print('large design: rel err pointwise %.2e' % ep)
    assert ep < 1e-12, ep


# ---- 3. under the objectives: the same objective on the dense target, the same seeds ---------------------------------
OBJ_N = 200


def _objective_problem(vb):
    """n_data = 300, p = 12, three entries per row and an intercept; logistic."""
    if 'objective' not in _PROBLEMS:
        rng = np.random.RandomState(21)
        A = _random_rows(rng, 300, 12, 3)
        A[:, 0] = 1.0
        y = _response('logistic', A @ (0.3 * rng.randn(12)), rng)
        _PROBLEMS['objective'] = (vb.SparseRegressionModel.from_dense(A, y, prior_sd=PRIOR_SD),
                                  vb.LogisticRegressionModel(A, y, PRIOR_SD))
    return _PROBLEMS['objective']


def _mf_theta(D, seed):
    rng = np.random.RandomState(seed)
    return np.concatenate([0.3 * rng.randn(D), -1.0 + 0.1 * rng.randn(D)])


def _chol_theta(vb, D, seed):
    rng = np.random.RandomState(seed)
    L = np.tril(0.05 * rng.randn(D, D), -1) + np.diag(np.exp(-1.0 + 0.2 * rng.randn(D)))
    return vb.FullRankGaussian(D).pack(0.3 * rng.randn(D), L)


def _compare(label, make, theta, tol_v=1e-12, tol_g=1e-11):
    """`make(model)` builds the objective: the sparse target's against the dense target's, the same seeds."""
    (v, g), (dv, dg) = (make(model)(theta) for model in make.models)
    ev, eg = G.rel_err(v, dv), G.rel_err(g, dg)
    print('%s: rel err value %.2e grad %.2e' % (label, ev, eg))
    assert ev < tol_v, (label, v, dv)
    assert eg < tol_g, (label, eg)


def _maker(vb, fn):
    fn.models = _objective_problem(vb)
    return fn


@pytest.mark.parametrize('family', ['mf_gaussian', 'mf_student_t', 'fullrank'])
@pytest.mark.parametrize('pd', [False, True])
def test_exclusive_kl(vb, family, pd):
    D = 12
    if family == 'mf_gaussian':
        make, theta = (lambda m: vb.ExclusiveKL(vb.MFGaussian(D, seed=5), m, OBJ_N, use_path_deriv=pd)), _mf_theta(D, 1)
    elif family == 'mf_student_t':
        make, theta = (lambda m: vb.ExclusiveKL(vb.MFStudentT(D, 8.0, seed=5), m, OBJ_N, use_path_deriv=pd)), _mf_theta(D, 2)
    else:
        make, theta = (lambda m: vb.ExclusiveKL(vb.FullRankGaussian(D, seed=4), m, OBJ_N, use_path_deriv=pd)), \
            _chol_theta(vb, D, 3)
    _compare('ekl %s pd=%d' % (family, pd), _maker(vb, make), theta)


def test_exclusive_kl_philox_meanfield(vb):
    D = 12
    _compare('ekl mf philox', _maker(vb, lambda m: vb.ExclusiveKL(vb.MFGaussian(D, seed=5, rng='philox'), m, OBJ_N)),
             _mf_theta(D, 4))


def test_control_variate(vb):
    """The dense regression targets take no control variates (the engine refuses them), so this route has no dense twin:
    the value is the plain estimator's, compared with the dense target's plain value on the same noise, and the gradient is
    compared with the literal per-sample RGE of the oracle."""
    from oracle import families as ofam, objectives as oobj
    D, N, method = 12, 512, 'mean_only'
    sparse, dense = _objective_problem(vb)
    omodel = _oracle_of(sparse)
    theta = _mf_theta(D, 5)
    obj = vb.ExclusiveKL(vb.MFGaussian(D, seed=5), sparse, N, hessian_approx_method=method)
    value, grad = obj(theta)
    noise = np.random.RandomState(5).randn(N, D)
    ov, og = oobj.rge_literal(ofam.MFGaussian(D), omodel, theta, noise, method)
    dv, dplain = vb.ExclusiveKL(vb.MFGaussian(D, seed=5), dense, N)(theta)
    ev, ed, eg = G.rel_err(value, ov), G.rel_err(value, dv), G.rel_err(grad, og)
    print('cv %s: rel err value %.2e (dense target %.2e) grad %.2e' % (method, ev, ed, eg))
    assert ev < 1e-12 and ed < 1e-12, (value, ov, dv)
    assert eg < 1e-11, eg
    assert G.rel_err(grad, dplain) > 1e-4                    # the control variate really changed the estimate
    assert not obj.supports_device_fit()


def _oracle_of(sparse):
    return SparseGLMOracle(sparse.to_dense(), sparse.y, sparse.likelihood, sparse.prior_sd, sparse.noise_sd)


# The dense regression targets are refused by AlphaDivergence, DISInclusiveKL and the low-rank family (the engine takes the
# gauss_diag, funnel and rows targets there), so these three routes have no dense twin: they are compared with the oracle's
# objective on the same noise, as tests/test_gpu_locscale.py compares them.
def test_alpha_divergence(vb):
    from oracle import families as ofam, objectives as oobj
    D, alpha = 12, 0.5
    sparse, _ = _objective_problem(vb)
    theta = _mf_theta(D, 6)
    np.random.seed(11)
    value, grad = vb.AlphaDivergence(vb.MFGaussian(D), sparse, OBJ_N, alpha)(theta)
    np.random.seed(11)
    noise = ofam.MFGaussian(D).draw_noise(np.random.RandomState(np.random.randint(2 ** 32)), OBJ_N)
    ov, og = oobj.alpha_divergence(ofam.MFGaussian(D), _oracle_of(sparse), theta, noise, alpha)
    print('alpha mf: rel err value %.2e grad %.2e' % (G.rel_err(value, ov), G.rel_err(grad, og)))
    assert G.rel_err(value, ov) < 1e-12, (value, ov)
    assert G.rel_err(grad, og) < 1e-11, G.rel_err(grad, og)


def test_dis_inclusive_kl_multivariate_t(vb):
    """Two steps with a moving theta (a refresh, then a step on the kept state), the structure of the source-model DIS tests
    and their bounds."""
    from oracle import families as ofam, objectives as oobj
    D, N, ess = 12, 600, 150
    sparse, _ = _objective_problem(vb)
    rng = np.random.RandomState(9)
    A = rng.randn(D, D)
    theta = np.concatenate([0.1 * rng.randn(D), ofam.psd_to_free(A @ A.T / D + 0.7 * np.eye(D))])
    prior = np.concatenate([np.zeros(D), np.log(3.0) * np.ones(D)])
    kw = dict(use_resampling=False, num_resampling_batches=2)
    obj = vb.DISInclusiveKL(vb.MultivariateT(D, 40, seed=6), sparse, N, ess_target=ess, temper_prior=vb.MFGaussian(D),
                            temper_prior_params=prior, **kw)
    ofamily = ofam.MultivariateT(D, 40)
    ref = oobj.DISInclusiveKL(ofamily, _oracle_of(sparse), N, ess, ofam.MFGaussian(D), prior, **kw)
    rs = np.random.RandomState(6)
    np.random.seed(12)
    for step in range(2):
        value, grad = obj(theta)
        noise = ofamily.draw_noise(rs, N) if ref.needs_refresh() else None
        ov, og = ref(theta, noise=noise)
        print('dis mvt step %d: rel err eps %.2e value %.2e grad %.2e' % (step, G.rel_err(obj._eps, ref._eps),
                                                                        G.rel_err(value, ov), G.rel_err(grad, og)))
        assert G.rel_err(obj._eps, ref._eps) < 1e-10
        assert G.rel_err(value, ov) < 1e-10, (step, value, ov)
        assert G.rel_err(grad, og) < 1e-9, (step, G.rel_err(grad, og))
        theta = theta - 0.01 * grad / (1 + np.abs(grad))


def test_exclusive_kl_lowrank(vb):
    from oracle import families as ofam, objectives as oobj
    D, k = 12, 2
    sparse, _ = _objective_problem(vb)
    rng = np.random.RandomState(D + k)
    fam, ofamily = vb.LRGaussian(D, seed=7, k=k), ofam.LRGaussian(D, k)
    theta = fam.pack(0.3 * rng.randn(D), -1.0 + 0.1 * rng.randn(D), 0.2 * rng.randn(D, k) / np.sqrt(k))
    value, grad = vb.ExclusiveKL(fam, sparse, OBJ_N)(theta)
    noise = ofamily.draw_noise(np.random.RandomState(7), OBJ_N)
    ov, og = oobj.exclusive_kl(ofamily, _oracle_of(sparse), theta, noise, False)
    print('ekl lr: rel err value %.2e grad %.2e' % (G.rel_err(value, ov), G.rel_err(grad, og)))
    assert G.rel_err(value, ov) < 1e-12, (value, ov)
    assert G.rel_err(grad, og) < 1e-11, G.rel_err(grad, og)


def test_exclusive_kl_nvp_flow(vb):
    D, K = 12, 2
    masks = np.array([[(j + i) % 2 for j in range(D)] for i in range(K)], dtype=float)

    def make(m):
        r = np.random.RandomState(D + K)
        flow = vb.NVPFlow([[D, 10], [10, D]], [[D, 10], [10, D]], masks, vb.MFGaussian(D, seed=3),
                          np.concatenate([0.1 * r.randn(D), -1.0 + 0.1 * r.randn(D)]), D)
        make.dim = flow.var_param_dim
        return vb.ExclusiveKL(flow, m, OBJ_N)
    make(_objective_problem(vb)[0])
    theta = 0.1 * np.random.RandomState(D * 7 + K).randn(make.dim)
    _compare('ekl flow', _maker(vb, make), theta, tol_v=1e-12, tol_g=1e-10)        # (the flow tests' gradient bound)


# ---- 4. device-resident fit ------------------------------------------------------------------------------------------
def test_device_fit_matches_host_loop(vb, capsys):
    from viabel_amd.optimization import Adam
    model, _ = _objective_problem(vb)
    D = model.dim
    hist, last = {}, {}
    for on_device in (False, True):
        fam = vb.MFGaussian(D, rng='philox', seed=3)
        obj = vb.ExclusiveKL(fam, model, 128)
        assert obj.supports_device_fit()
        res = Adam(0.02).optimize(50, obj, fam.init_param(), on_device=on_device)
        hist[on_device], last[on_device] = np.asarray(res['value_history']), res['opt_param']
    np.testing.assert_array_equal(hist[False], hist[True])
    np.testing.assert_array_equal(last[False], last[True])
    res = vb.vi_diagnostics(last[True], model=model, approx=vb.MFGaussian(D, seed=3), n_samples=2000)
    capsys.readouterr()
    assert np.isfinite(res['khat'])


# ---- 5. interleaving on one engine -----------------------------------------------------------------------------------
def test_interleaved_with_a_dense_model_on_one_engine(vb):
    """A larger sparse model, a dense one, then a smaller sparse one and the larger again on ONE engine: every result equals
    the one a fresh engine gives, bit for bit (the workspace is carved anew per call out of bytes the earlier calls left)."""
    from _engine_subjects import _fresh_engine
    big, _, dense, _ = _problem(vb, 'long_column', 'poisson')
    small, _, _, _ = _problem(vb, 'odd', 'logistic')
    xb = 0.3 * np.random.RandomState(1).randn(200, big.dim)
    xs = 0.3 * np.random.RandomState(2).randn(37, small.dim)

    def run(model, x):
        return model(x), model.grad(x), model.pointwise_log_likelihood(x)
    solo = {}
    for key, (model, x) in dict(big=(big, xb), small=(small, xs), dense=(dense, xb)).items():
        with _fresh_engine():
            solo[key] = run(model, x)
    with _fresh_engine():
        for key, model, x in (('big', big, xb), ('dense', dense, xb), ('small', small, xs), ('big', big, xb),
                              ('small', small, xs)):
            for a, b in zip(run(model, x), solo[key]):
                np.testing.assert_array_equal(a, b)


# ---- 6. errors -------------------------------------------------------------------------------------------------------
def test_errors_leave_the_context_usable(vb):
    from viabel_amd import _lib
    eng = _lib.default_engine()
    model, omodel, dense, _ = _problem(vb, 'odd', 'logistic')
    n_data, p, nnz = model.n_data, model.dim, model.nnz
    good = model.device_spec()
    x = 0.3 * np.random.RandomState(0).randn(5, p)
    f_before = model(x)                                           # binds the model: the failures below must leave it bound
    o_ptr, o_idx = 4, 4 + n_data + 1
    o_tptr = o_idx + nnz
    o_tidx = o_tptr + p + 1

    def refused(dparams=None, iparams=None, dim=p, match=None):
        spec = (_lib.MODEL_SPARSE_GLM, dim, good[2].copy() if dparams is None else dparams,
                good[3].copy() if iparams is None else iparams)
        with pytest.raises(ValueError, match=match):
            eng.set_model(spec)
        assert np.array_equal(eng.model_logp(x), f_before)        # the model bound before still answers
    bad = good[3].copy()
    bad[o_ptr + n_data] -= 1                                      # the csr pointer does not end at nnz
    refused(iparams=bad, match='indptr')
    bad = good[3].copy()
    bad[o_tptr + p] += 1                                          # nor the csc pointer
    refused(iparams=bad, match='indptr')
    bad = good[3].copy()
    bad[o_ptr + 2] = bad[o_ptr + 1] - 1                           # not monotone
    refused(iparams=bad, match='monotone')
    bad = good[3].copy()
    bad[o_idx] = p                                                # a column index out of range
    refused(iparams=bad, match=r'indices\[0\]')
    bad = good[3].copy()
    bad[o_tidx + 1] = -1                                          # a row index out of range
    refused(iparams=bad, match='csc indices')
    bad = good[3].copy()
    bad[o_idx], bad[o_idx + 1] = bad[o_idx + 1], bad[o_idx]       # an unsorted row
    refused(iparams=bad, match='increase strictly')
    refused(iparams=good[3][:-1].copy())                          # wrong lengths
    refused(dparams=good[2][:-1].copy())
    refused(dim=p + 1)
    bad = good[3].copy()
    bad[2] = 3                                                    # an unknown likelihood
    refused(iparams=bad)
    bad_d = good[2].copy()
    bad_d[-2] = 0.0                                               # prior_sd, past the Python check
    refused(dparams=bad_d, match='prior_sd')
    bad_d = good[2].copy()
    bad_d[2 * nnz] = 2.0                                          # a logistic response outside {0, 1}
    refused(dparams=bad_d, match='y\\[0\\]')
    bad_d = good[2].copy()
    bad_d[nnz] = bad_d[nnz] + 1.0                                 # a csc value that is not the csr's
    refused(dparams=bad_d, match='transpose')
    with pytest.raises(ValueError):
        model(np.zeros((2, p + 1)))
    with pytest.raises(ValueError):                               # a wrong d at the C entry
        eng.sparse_glm_pointwise(np.zeros((2, p + 1)), n_data)
    assert np.array_equal(model(x), f_before)
    assert G.rel_err(model.grad(x), omodel.grad(x)) < 1e-11
    with pytest.raises(NotImplementedError, match='psisloo'):
        vb.loo(np.zeros(2 * p), model=model, approx=vb.MFGaussian(p), n_samples=10)
    dense(np.zeros(p))
    with pytest.raises(NotImplementedError):                      # vb_sparse_glm_pointwise with another model bound
        eng.sparse_glm_pointwise(np.zeros((2, p)), n_data)
    assert np.array_equal(model(x), f_before)                     # and the next good call succeeds
    assert G.rel_err(model.pointwise_log_likelihood(x), omodel.pointwise(x)) < 1e-12
