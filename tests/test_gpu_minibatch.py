"""MinibatchRegressionModel (VB_MODEL_MINIBATCH_GLM, csrc/vb_minibatch.hip) on the GPU: the index kernel against the
restatement of tests/_minibatch_oracle.py; the row pipeline (gather, the two products, row sums; the gradient product's
observation split; three row chunks) against the numpy oracle on X[idx]; B = n_data against full_model(); the exact mean
over an epoch's batches; a smaller batch after a larger one on one engine; the batch counter under model calls, under
ExclusiveKL with the six families and under interleaving; the device-resident fit against the host loop; errors.
Tolerances are the rows targets' (tests/test_gpu_locscale.py): value and pointwise 1e-12, gradient 1e-11 relative to the
largest entry; 1e-10 where the tests of the same route use it (NVPFlow, MultivariateT gradients)."""
import numpy as np
import pytest

import _golden as G
import _minibatch_oracle as O

pytestmark = pytest.mark.gpu

LIKELIHOODS = ['logistic', 'poisson', 'gaussian']
PRIOR_SD, NOISE_SD, SEED = 3.0, 0.8, 20241


@pytest.fixture(scope='module')
def vb():
    import viabel_amd
    from viabel_amd import _lib
    _lib.default_engine()
    return viabel_amd


_DATA = {}


def _data(n_data, p, lik, seed=0):
    """(X, y) of the case, built once and shared."""
    key = (n_data, p, lik, seed)
    if key not in _DATA:
        rng = np.random.RandomState(1000 * seed + n_data + p)
        X = rng.randn(n_data, p) / np.sqrt(p)
        eta = X @ (0.5 * rng.randn(p))
        if lik == 'logistic':
            y = (rng.rand(n_data) < 1.0 / (1.0 + np.exp(-eta))).astype(float)
        elif lik == 'poisson':
            y = rng.poisson(np.exp(eta)).astype(float)
        else:
            y = eta + NOISE_SD * rng.randn(n_data)
        _DATA[key] = (X, y)
    return _DATA[key]


def _model(vb, n_data, p, B, lik, order='shuffle', seed=SEED):
    X, y = _data(n_data, p, lik)
    return vb.MinibatchRegressionModel(X, y, B, likelihood=lik, prior_sd=PRIOR_SD, noise_sd=NOISE_SD, seed=seed, order=order)


def _oracle(model, idx):
    return O.MinibatchOracle(model.X, model.y, idx, model.likelihood, model.prior_sd, model.noise_sd)


def _oracle_rows(omodel, x):
    """f, gradient and per-observation terms of the oracle in slices of 512 rows (its (rows, B) temporaries, bounded)."""
    rows = x.shape[0]
    fo, go, po = np.empty(rows), np.empty((rows, omodel.dim)), np.empty((rows, omodel.batch_size))
    for r0 in range(0, rows, 512):
        s = slice(r0, r0 + 512)
        fo[s], go[s], po[s] = omodel.logp(x[s]), omodel.grad(x[s]), omodel.pointwise(x[s])
    return fo, go, po


# ---- 1. rows ---------------------------------------------------------------------------------------------------------
# name: (n_data, p, B, sample rows (None: 2 chunks + 5), the batches evaluated)
CASES = {
    'smallest': (1, 1, 1, 1, (0, 3)),
    'odd': (33, 17, 7, 100, (0, 4, 5, 9, 1 << 33)),       # t = 4: positions 28 .. 34 end epoch 0 and begin epoch 1; t = 9 likewise
    'tile65': (200, 65, 65, 64, (0, 3)),                  # one row and one column past a 64 x 64 gather tile
    'tile64': (200, 64, 64, 64, (0, 3)),                  # exactly one tile
    'domain64': (64, 3, 16, 37, (0, 4)),                  # the Feistel domain 2^6 exactly: no cycle walk
    'domain65': (65, 3, 16, 37, (0, 4)),                  # domain 2^8 for 65 observations: the longest walks
    'split': (3000, 8, 2048, 64, (1,)),                   # one output tile: the gradient product splits the batch 16 ways
    'chunks': (5000, 30, 2500, None, (1,)),               # exactly three row chunks
}
_INDICES = {}


def _oracle_indices(t, n_data, B, order='shuffle', seed=SEED):
    key = (t, n_data, B, order, seed)
    if key not in _INDICES:
        fn = O.batch_indices if B <= 128 else O.batch_indices_array      # (the same definition; the array form for thousands)
        _INDICES[key] = fn(t, n_data, B, seed, order)
    return _INDICES[key]


@pytest.mark.parametrize('name', list(CASES))
@pytest.mark.parametrize('lik', LIKELIHOODS)
def test_rows_against_oracle(vb, lik, name):
    from viabel_amd import _lib
    n_data, p, B, rows, batches = CASES[name]
    if rows is None:
        chunk = _lib.minibatch_chunk_rows(B)
        rows = 2 * chunk + 5
        assert 2 * chunk < rows <= 3 * chunk                      # exactly three chunks
    if name == 'split':
        assert B // 128 >= 16                                     # room for the 16 splits one output tile asks for
    model = _model(vb, n_data, p, B, lik)
    eng = _lib.default_engine()
    x = 0.3 * np.random.RandomState(rows).randn(rows, p)
    for t in batches:
        model.batch = t
        idx = _oracle_indices(t, n_data, B)
        f, g, pw = model(x), model.grad(x), model.pointwise_log_likelihood(x)
        assert model.batch == t
        assert np.array_equal(eng.minibatch_indices(t, B), idx)
        assert np.array_equal(model.batch_indices(), idx)
        assert f.shape == (rows,) and g.shape == (rows, p) and pw.shape == (rows, B)
        fo, go, po = _oracle_rows(_oracle(model, idx), x)
        ef, eg, ep = G.rel_err(f, fo), G.rel_err(g, go), G.rel_err(pw, po)
        print('rows %s %s t=%d n_data=%d p=%d B=%d rows=%d: rel err f %.2e grad %.2e pointwise %.2e'
              % (name, lik, t, n_data, p, B, rows, ef, eg, ep))
        assert ef < 1e-12 and eg < 1e-11 and ep < 1e-12, (t, ef, eg, ep)
        # no atomics, and the index query in between has not disturbed the batch: the same bits
        assert np.array_equal(model(x), f) and np.array_equal(model.grad(x), g)
        assert np.array_equal(model.pointwise_log_likelihood(x), pw)
    cg = model.check_gradient(x[:3])
    print('     check_gradient %.2e' % cg)
    assert cg < 1e-6 and model.batch == batches[-1]
    assert model(x[0]).shape == (1,) and model.grad(x[0]).shape == (p,)
    assert model.pointwise_log_likelihood(x[0]).shape == (1, B)


@pytest.mark.parametrize('order', ['shuffle', 'sequential'])
def test_sequential_and_shuffled_indices_on_the_device(vb, order):
    from viabel_amd import _lib
    model = _model(vb, 10, 2, 4, 'logistic', order=order, seed=3)
    model(np.zeros(2))
    got = [list(_lib.default_engine().minibatch_indices(t, 4)) for t in range(6)]
    assert got == [list(O.batch_indices(t, 10, 4, 3, order)) for t in range(6)]
    if order == 'sequential':
        assert got[2] == [8, 9, 0, 1]                             # across the end of epoch 0


# ---- 2. the whole data as one batch ----------------------------------------------------------------------------------
@pytest.mark.parametrize('order', ['shuffle', 'sequential'])
@pytest.mark.parametrize('lik', LIKELIHOODS)
def test_whole_batch_is_the_full_model(vb, lik, order):
    n_data, p = 130, 9
    model = _model(vb, n_data, p, n_data, lik, order=order)
    full = model.full_model()
    x = 0.3 * np.random.RandomState(5).randn(70, p)
    for t in (0, 2):
        model.batch = t
        assert sorted(model.batch_indices()) == list(range(n_data))
        ef, eg = G.rel_err(model(x), full(x)), G.rel_err(model.grad(x), full.grad(x))
        print('whole batch %s %s t=%d: rel err f %.2e grad %.2e' % (lik, order, t, ef, eg))
        assert ef < 1e-12 and eg < 1e-11, (ef, eg)


# ---- 3. exact unbiasedness over an epoch -----------------------------------------------------------------------------
@pytest.mark.parametrize('lik', LIKELIHOODS)
def test_mean_over_an_epochs_batches_is_the_full_density(vb, lik):
    n_data, p, B = 96, 5, 8
    model = _model(vb, n_data, p, B, lik)
    full = model.full_model()
    x = 0.3 * np.random.RandomState(6).randn(40, p)
    f_full, g_full = full(x), full.grad(x)
    seen = []
    for epoch in (0, 1):
        fs, gs = [], []
        for t in range(12 * epoch, 12 * epoch + 12):
            model.batch = t
            fs.append(model(x))
            gs.append(model.grad(x))
        seen.append(np.concatenate([model.batch_indices(t) for t in range(12 * epoch, 12 * epoch + 12)]))
        assert sorted(seen[-1]) == list(range(n_data))
        ef, eg = G.rel_err(np.mean(fs, axis=0), f_full), G.rel_err(np.mean(gs, axis=0), g_full)
        print('epoch %d %s: rel err of the mean f %.2e grad %.2e; one batch is off by %.2e'
              % (epoch, lik, ef, eg, G.rel_err(fs[0], f_full)))
        assert ef < 1e-12 and eg < 1e-11, (ef, eg)
        assert G.rel_err(fs[0], f_full) > 1e-6                    # a single batch is not the full density
    assert not np.array_equal(seen[0], seen[1])                   # the second epoch is shuffled anew


# ---- 4. a smaller batch after a larger one ---------------------------------------------------------------------------
@pytest.mark.parametrize('lik', LIKELIHOODS)
def test_stale_workspace(vb, lik):
    """A larger-batch model, then a smaller one on the same engine: the smaller one's results equal its results on a fresh
    engine bit for bit, whatever the larger one left in the shared workspace."""
    from _engine_subjects import _fresh_engine
    big = _model(vb, 500, 40, 300, lik)
    small = _model(vb, 50, 5, 7, lik)
    xb = 0.3 * np.random.RandomState(1).randn(130, 40)
    xs = 0.3 * np.random.RandomState(2).randn(37, 5)

    def run(model, x):
        model.batch = 3
        return model(x), model.grad(x), model.pointwise_log_likelihood(x)
    with _fresh_engine():
        solo = run(small, xs)
    with _fresh_engine():
        run(big, xb)
        for a, b in zip(run(small, xs), solo):
            np.testing.assert_array_equal(a, b)
        run(big, xb)
        for a, b in zip(run(small, xs), solo):
            np.testing.assert_array_equal(a, b)


# ---- 5. the batch counter --------------------------------------------------------------------------------------------
def test_model_calls_do_not_advance_the_counter(vb):
    model = _model(vb, 200, 6, 32, 'poisson')
    x = 0.3 * np.random.RandomState(3).randn(20, 6)
    model.batch = 4
    g = model.grad(x)
    assert np.array_equal(model.grad(x), g) and model.batch == 4
    f, pw = model(x), model.pointwise_log_likelihood(x)
    assert np.array_equal(model(x), f) and np.array_equal(model.pointwise_log_likelihood(x), pw) and model.batch == 4
    model.batch = 5
    assert not np.array_equal(model.grad(x), g)
    model.batch = 4
    assert np.array_equal(model.grad(x), g) and np.array_equal(model(x), f)


OBJ_N, OBJ_D, OBJ_NDATA, OBJ_B = 200, 12, 240, 60


def _mf_theta(D, seed):
    rng = np.random.RandomState(seed)
    return np.concatenate([0.3 * rng.randn(D), -1.0 + 0.1 * rng.randn(D)])


def _family_case(vb, family):
    """(make(model) -> objective, theta, the oracle family or None, gradient tolerance)."""
    from oracle import families as ofam
    D = OBJ_D
    rng = np.random.RandomState(len(family))
    if family == 'mf_gaussian':
        return (lambda m: vb.ExclusiveKL(vb.MFGaussian(D, seed=5), m, OBJ_N)), _mf_theta(D, 1), None, 1e-11
    if family == 'mf_student_t':
        return (lambda m: vb.ExclusiveKL(vb.MFStudentT(D, 8.0, seed=5), m, OBJ_N)), _mf_theta(D, 2), None, 1e-11
    if family == 'fullrank':
        L = np.tril(0.05 * rng.randn(D, D), -1) + np.diag(np.exp(-1.0 + 0.2 * rng.randn(D)))
        theta = vb.FullRankGaussian(D).pack(0.3 * rng.randn(D), L)
        return (lambda m: vb.ExclusiveKL(vb.FullRankGaussian(D, seed=4), m, OBJ_N)), theta, None, 1e-11
    if family == 'nvp_flow':
        K = 2
        masks = np.array([[(j + i) % 2 for j in range(D)] for i in range(K)], dtype=float)

        def make(m):
            r = np.random.RandomState(D + K)
            flow = vb.NVPFlow([[D, 10], [10, D]], [[D, 10], [10, D]], masks, vb.MFGaussian(D, seed=3),
                              np.concatenate([0.1 * r.randn(D), -1.0 + 0.1 * r.randn(D)]), D)
            make.dim = flow.var_param_dim
            return vb.ExclusiveKL(flow, m, OBJ_N)
        make(vb.GaussianModel(np.zeros(D), np.ones(D)))
        return make, 0.1 * np.random.RandomState(D * 7 + K).randn(make.dim), None, 1e-10      # (the flow tests' bound)
    if family == 'multivariate_t':
        A = rng.randn(D, D)
        theta = np.concatenate([0.3 * rng.randn(D), ofam.psd_to_free(0.05 * (A @ A.T / D + 0.5 * np.eye(D)))])
        return ((lambda m: vb.ExclusiveKL(vb.MultivariateT(D, 9.0, seed=6), m, OBJ_N)), theta,
                (ofam.MultivariateT(D, 9.0), 6), 1e-10)                                       # (the source-model test's bound)
    assert family == 'lr_gaussian'
    k = 2
    fam = vb.LRGaussian(D, seed=7, k=k)
    theta = fam.pack(0.3 * rng.randn(D), -1.0 + 0.1 * rng.randn(D), 0.2 * rng.randn(D, k) / np.sqrt(k))
    return (lambda m: vb.ExclusiveKL(vb.LRGaussian(D, seed=7, k=k), m, OBJ_N)), theta, (ofam.LRGaussian(D, k), 7), 1e-11


@pytest.mark.parametrize('family', ['mf_gaussian', 'mf_student_t', 'fullrank', 'multivariate_t', 'lr_gaussian', 'nvp_flow'])
def test_exclusive_kl_uses_one_batch_and_advances_by_one(vb, family):
    """One call evaluates batch model.batch and leaves the counter one higher.  The mean-field, full-rank and flow families
    are compared with the same objective, the same seeds, on a dense target that has the batch's density: logistic (no
    likelihood constant) with n_data = 4 B, so the rows X[idx_t] stacked four times sum to (n_data / B) times the batch's
    sum.  The dense targets do not take the low-rank family, and the multivariate t is compared as the other rows targets
    compare it: both against the oracle's objective on the same noise, where the scale enters through the oracle."""
    from oracle import objectives as oobj
    make, theta, ofamily, tol_g = _family_case(vb, family)
    model = _model(vb, OBJ_NDATA, OBJ_D, OBJ_B, 'logistic')
    for t in (5, 6):                                              # t = 5: positions 300 .. 359, epoch 1
        model.batch = t
        idx = model.batch_indices(t)
        assert np.array_equal(idx, O.batch_indices(t, OBJ_NDATA, OBJ_B, SEED))
        value, grad = make(model)(theta)
        assert model.batch == t + 1
        if ofamily is None:
            reps = OBJ_NDATA // OBJ_B
            twin = vb.LogisticRegressionModel(np.tile(model.X[idx], (reps, 1)), np.tile(model.y[idx], reps), PRIOR_SD)
            ov, og = make(twin)(theta)
        else:
            noise = ofamily[0].draw_noise(np.random.RandomState(ofamily[1]), OBJ_N)
            ov, og = oobj.exclusive_kl(ofamily[0], _oracle(model, idx), theta, noise, False)
        ev, eg = G.rel_err(value, ov), G.rel_err(grad, og)
        print('ekl %s t=%d: rel err value %.2e grad %.2e' % (family, t, ev, eg))
        assert ev < 1e-12, (family, value, ov)
        assert eg < tol_g, (family, eg)
    # setting the counter back replays the same bits
    model.batch = 5
    v1, g1 = make(model)(theta)
    model.batch = 5
    v2, g2 = make(model)(theta)
    assert v1 == v2 and np.array_equal(g1, g2) and model.batch == 6
    v3, _ = make(model)(theta)
    assert v3 != v1 and model.batch == 7


def test_one_objective_walks_the_batches(vb):
    """Consecutive calls of ONE objective take consecutive batches (the family's noise stream moves too: each call is
    compared with a fresh objective whose stream and batch are set to the same place)."""
    D = OBJ_D
    model = _model(vb, OBJ_NDATA, D, OBJ_B, 'gaussian')
    theta = _mf_theta(D, 3)
    fam = vb.MFGaussian(D, seed=9, rng='philox')
    obj = vb.ExclusiveKL(fam, model, 64)
    model.batch = 2
    got = [obj(theta) for _ in range(3)]
    assert model.batch == 5
    for k, (v, g) in enumerate(got):
        twin_model = _model(vb, OBJ_NDATA, D, OBJ_B, 'gaussian')
        twin_model.batch = 2 + k
        twin_fam = vb.MFGaussian(D, seed=9, rng='philox')
        twin_fam._philox_calls = k
        tv, tg = vb.ExclusiveKL(twin_fam, twin_model, 64)(theta)
        assert tv == v and np.array_equal(tg, g)


def test_interleaved_models_keep_their_sequences(vb):
    """Two minibatch models and a GaussianModel taking turns on one engine: every call returns the bits of the same call
    in a run of its model alone."""
    D = 6
    theta = _mf_theta(D, 4)

    def parts():
        a = _model(vb, 200, D, 32, 'logistic', seed=1)
        b = _model(vb, 150, D, 20, 'poisson', seed=2)
        gauss = vb.GaussianModel(np.zeros(D), np.ones(D))
        return (vb.ExclusiveKL(vb.MFGaussian(D, seed=5), a, 50), vb.ExclusiveKL(vb.MFGaussian(D, seed=6), b, 50),
                vb.ExclusiveKL(vb.MFGaussian(D, seed=7), gauss, 50), a, b)
    oa, ob, og, a, b = parts()
    solo = dict(a=[oa(theta) for _ in range(3)], b=[ob(theta) for _ in range(3)], g=[og(theta) for _ in range(2)])
    assert a.batch == 3 and b.batch == 3
    assert solo['a'][0][0] != solo['a'][1][0]
    oa, ob, og, a, b = parts()
    objs, count = dict(a=oa, b=ob, g=og), dict(a=0, b=0, g=0)
    x = 0.3 * np.random.RandomState(0).randn(4, D)
    for key in 'abgababg':
        value, grad = objs[key](theta)
        ref = solo[key][count[key]]
        assert value == ref[0] and np.array_equal(grad, ref[1]), (key, count[key])
        count[key] += 1
        if key == 'b':                                            # a plain model call in between binds and does not advance
            fa = a(x)
            assert np.array_equal(a(x), fa)
    assert a.batch == 3 and b.batch == 3


# ---- 6. device-resident fit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', ['mf_gaussian', 'fullrank', 'nvp_flow'])
def test_device_fit_matches_host_loop(vb, family):
    from viabel_amd.optimization import RMSProp
    n_data, D, B, n_iters = 512, 6, 32, 20
    hist, last, batch = {}, {}, {}
    for on_device in (False, True):
        model = _model(vb, n_data, D, B, 'logistic')
        model.batch = 7
        if family == 'mf_gaussian':
            fam = vb.MFGaussian(D, rng='philox', seed=3)
        elif family == 'fullrank':
            fam = vb.FullRankGaussian(D, rng='philox', seed=3)
        else:
            masks = np.array([[(j + i) % 2 for j in range(D)] for i in range(2)], dtype=float)
            r = np.random.RandomState(D)
            fam = vb.NVPFlow([[D, 10], [10, D]], [[D, 10], [10, D]], masks, vb.MFGaussian(D, seed=3, rng='philox'),
                             np.concatenate([0.1 * r.randn(D), -1.0 + 0.1 * r.randn(D)]), D)
        obj = vb.ExclusiveKL(fam, model, 64)
        assert obj.supports_device_fit()
        init = 0.1 * np.random.RandomState(1).randn(fam.var_param_dim) if family == 'nvp_flow' else fam.init_param()
        res = RMSProp(0.01, diagnostics=True).optimize(n_iters, obj, init, on_device=on_device)
        hist[on_device] = (np.asarray(res['value_history']), np.asarray(res['variational_param_history']))
        last[on_device], batch[on_device] = res['opt_param'], model.batch
    assert batch[False] == batch[True] == 7 + n_iters
    np.testing.assert_array_equal(hist[False][0], hist[True][0])
    np.testing.assert_array_equal(hist[False][1], hist[True][1])
    np.testing.assert_array_equal(last[False], last[True])
    assert len(set(hist[True][0])) == n_iters


@pytest.mark.parametrize('rng', ['numpy', 'philox'])
@pytest.mark.parametrize('kw', [dict(adaptive=True, fixed_lr=True), dict(adaptive=True, fixed_lr=False),
                                dict(adaptive=False, fixed_lr=True)], ids=['faso', 'raabbvi', 'rmsprop'])
def test_bbvi_takes_one_batch_per_iteration(vb, capsys, kw, rng):
    """bbvi() with FASO, RAABBVI and plain RMSProp, on the host loop (numpy noise) and through the device-resident fit
    (Philox noise): the counter ends at the number of objective values the optimiser recorded."""
    model = _model(vb, 512, 6, 32, 'logistic')
    res = vb.bbvi(6, log_density=model, approx=vb.MFGaussian(6, rng=rng, seed=1), num_mc_samples=16, n_iters=60, **kw)
    capsys.readouterr()
    assert 0 < model.batch == len(res['value_history']) <= 60
    assert np.all(np.isfinite(res['opt_param'])) and np.all(np.isfinite(res['value_history']))


# ---- 7. errors -------------------------------------------------------------------------------------------------------
def test_errors_leave_the_context_usable(vb):
    from viabel_amd import _lib
    eng = _lib.default_engine()
    model = _model(vb, 33, 17, 7, 'logistic')
    p, B = 17, 7
    x = 0.3 * np.random.RandomState(0).randn(5, p)
    model.batch = 2
    f_before = model(x)                                           # binds the model: the failures below must leave it bound
    good = model.device_spec()

    def refused(dparams=None, iparams=None, dim=p, match=None):
        spec = (_lib.MODEL_MINIBATCH_GLM, dim, good[2].copy() if dparams is None else dparams,
                good[3].copy() if iparams is None else iparams, [2])
        with pytest.raises(ValueError, match=match):
            eng.set_model(spec)
        assert np.array_equal(model(x), f_before)                 # rebinding the good model answers as before
    for pos, bad_value in ((1, 0), (1, 34), (2, 3), (3, 2), (0, 0)):      # batch_size, likelihood, order, n_data
        bad = good[3].copy()
        bad[pos] = bad_value
        refused(iparams=bad)
    refused(iparams=good[3][:-1].copy())
    refused(dparams=good[2][:-1].copy())
    refused(dim=p + 1)
    bad_d = good[2].copy()
    bad_d[-2] = 0.0
    refused(dparams=bad_d, match='prior_sd')
    bad_d = good[2].copy()
    bad_d[33 * 17] = 2.0                                          # a logistic response outside {0, 1}, past the Python check
    refused(dparams=bad_d, match='y\\[0\\]')
    with pytest.raises(ValueError):
        model(np.zeros((2, p + 1)))
    with pytest.raises(ValueError):                               # a wrong d at the C entry
        eng.minibatch_pointwise(np.zeros((2, p + 1)), B)
    with pytest.raises(ValueError):                               # a batch number the stream position would overflow with
        eng._check(eng._lib.vb_minibatch_set_batch(eng._ctx, (1 << 62) // B))
    with pytest.raises(ValueError):
        eng.minibatch_indices(-1, B)
    assert eng.minibatch_get_batch() == 2
    assert np.array_equal(model(x), f_before)
    vb.GaussianModel(np.zeros(p), np.ones(p))(np.zeros(p))        # another model bound: the minibatch entries refuse
    with pytest.raises(NotImplementedError):
        eng.minibatch_pointwise(np.zeros((2, p)), B)
    for call in (lambda: eng.minibatch_get_batch(), lambda: eng.minibatch_indices(0, B),
                 lambda: eng._check(eng._lib.vb_minibatch_set_batch(eng._ctx, 0))):
        with pytest.raises(_lib.EngineError, match='no minibatch regression model bound'):
            call()
    assert np.array_equal(model(x), f_before)                     # and the next good call succeeds, on the same batch
    with pytest.raises(NotImplementedError, match='full_model'):
        vb.vi_diagnostics(np.zeros(2 * p), model=model, approx=vb.MFGaussian(p), n_samples=100)
