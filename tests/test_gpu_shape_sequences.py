"""GPU: ragged shapes after larger ones on ONE engine, bit for bit.

An engine keeps its device buffers for life: they only grow, and they are zero-filled only when they are allocated.  Every
later call of a smaller or differently shaped problem carves its layout out of the same bytes, which then hold what the
previous layout left there.  Row strides are ``round_up(d, 16)``, so a layout has pad columns ``[d, ld)`` unless ``d`` is a
multiple of 16, and kernels that stream ``ld`` columns, GEMMs over a padded width and cached "this is clean" flags all
rely on what those columns hold.

Contract: a call of shape S that runs after other work of other shapes returns EXACTLY (``==`` on the value,
``assert_array_equal`` on the gradient) what it returns as the first and only work of a fresh engine -- every reduction
runs in a fixed order.  The objectives here come one after another (each is deleted before the next is made), so no call
has a reason to be refused: an ``EngineError`` fails the case.

Shapes: ``d`` = 37 and 21 (``ld`` = 48 and 32: pad columns in both), 37 and 48 share ``ld`` = 48; ``n`` is off every row tile
(4, 16, 128).  The prelude P has the largest shape, so later work reuses its buffers instead of allocating, and it is LOUD:
target, prior and parameters shifted to 1e3 and stretched by 10 (``_engine_subjects._problem``), so that a stale byte
cannot hide in rounding.  The small regime (n < 4096) takes the host-root routes of the t family, the resident regime
(n >= 4096) its device-resident ones (``objectives.py``, ``_RESIDENT_GATE``).  The anchor compares the solo runs with the
oracle, so the numbers are the reference's and not merely repeatable ones."""
import gc

import numpy as np
import pytest

import _shape_subjects as S

pytestmark = pytest.mark.gpu

#           prelude      A            B            C
SHAPES = {'small': [(48, 1500), (37, 1003), (21, 1100), (37, 1030)],
          'resident': [(48, 6000), (37, 4099), (21, 4300), (37, 4200)]}
REGIMES = list(SHAPES)
# T's prelude, then S: pairs that share ctx->scratch, rowvec, mvt_state, glm_work, lg_work or the noise slots
PAIRS = [('ekl_mvt_np', 'alpha_fr_px'), ('dis_mvt_np', 'ekl_mvt_np'), ('dis_lr', 'ekl_lr'), ('ekl_nvp', 'ekl_mf_px'),
         ('dis_fr_px', 'dis_mvt_px')]
PAIRS = PAIRS + [(b, a) for a, b in PAIRS]


@pytest.fixture(scope='module')
def vb():
    import viabel_amd
    from viabel_amd import _lib
    _lib.default_engine()
    return viabel_amd


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('sid', S.SUBJECTS)
def test_after_a_larger_loud_prelude(vb, sid, regime):
    """S@P (loud), S@A."""
    P, A, _, _ = SHAPES[regime]
    S.run_sequence(vb, [(sid,) + P + (True,), (sid,) + A + (False,)])


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('sid', S.SUBJECTS)
def test_another_dimension_in_between(vb, sid, regime):
    """S@A, S@B (loud, another d and ld), S@A again: a new instance with the same seeds."""
    _, A, B, _ = SHAPES[regime]
    S.run_sequence(vb, [(sid,) + A + (False,), (sid,) + B + (True,), (sid,) + A + (False,)])


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('sid', S.SUBJECTS)
def test_another_sample_count_in_between(vb, sid, regime):
    """S@A, S@C (loud, same d, another n: the paths whose cleaning is keyed on the layout), S@A again."""
    _, A, _, C = SHAPES[regime]
    S.run_sequence(vb, [(sid,) + A + (False,), (sid,) + C + (True,), (sid,) + A + (False,)])


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('t,s', PAIRS)
def test_after_another_subjects_prelude(vb, t, s, regime):
    """T@P (loud), S@A: T leaves its bytes in buffers S shares with it."""
    P, A, _, _ = SHAPES[regime]
    S.run_sequence(vb, [(t,) + P + (True,), (s,) + A + (False,)])


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('sid', S.ANCHORED)
def test_solo_run_is_the_oracles(vb, sid, regime):
    """The first call of the solo run at shape A against the oracle on the same draws."""
    d, n = SHAPES[regime][1]
    value, grad = S.solo(vb, sid, d, n)[0]
    ov, og, scale, vtol, gtol = S.oracle_first_call(vb, sid, d, n)
    gmax = max(np.max(np.abs(og)), 1e-300)
    print('{} ({}, {}): value error {:.3g} of its scale, gradient error {:.3g} of max|grad|'.format(
        sid, d, n, abs(value - ov) / scale, np.max(np.abs(grad - og)) / gmax))
    assert abs(value - ov) <= vtol * scale, (value, ov)
    np.testing.assert_allclose(grad, og, rtol=0, atol=gtol * gmax)


# ---- 2. targets that carry data --------------------------------------------------------------------------------------------
# One engine, one kind of family (throughput mode: no host generator to keep in step), the target changed between
# objectives: rows_work, glm_work and target_work -- the ONE chunk workspace of the softmax, multilevel, location-scale and
# sparse pipelines -- are laid out from (n_data, p, classes / groups / scale columns / entries); ldq = round_up(n_data, 16)
# and ldp = round_up(p, 16) are ragged at every size here.  The sparse targets carry a column of ones: n_data entries, more
# than SPARSE_SEGMENT = 256 at n_data = 333 (the segment and combine kernels run) and fewer at n_data = 77 (they do not).
N_DRAWS = 203
TARGET_CALLS = 2
GAUSS_SRC = r'''
__device__ double vb_log_density(const double* z, int d, const double* p, double* g) {
  double f = 0.0;
  for (int j = 0; j < d; ++j) {
    const double r = (z[j] - p[j]) / p[d + j];
    f -= 0.5 * r * r;
    if (g) g[j] = -r / p[d + j];
  }
  return f;
}
'''


def _target(vb, name):
    kind, a, b, c = name
    rng = np.random.RandomState(sum(map(ord, kind)) + 7 * a + 11 * b + 13 * c)
    if kind == 'source':                             # (dim, -, -)
        return vb.SourceModel(a, GAUSS_SRC, np.concatenate([0.3 * rng.randn(a), np.exp(0.2 * rng.randn(a))]))
    n_data, p = a, b
    X = rng.randn(n_data, p) / np.sqrt(p)
    eta = X @ rng.randn(p)
    if kind == 'logistic':                           # (n_data, p, -)
        return vb.LogisticRegressionModel(X, (rng.rand(n_data) < 1.0 / (1.0 + np.exp(-eta))).astype(float), prior_sd=3.0)
    if kind == 'poisson':
        return vb.PoissonRegressionModel(X, rng.poisson(np.exp(eta)).astype(float), prior_sd=3.0)
    if kind == 'softmax':                            # (n_data, p, classes)
        return vb.SoftmaxRegressionModel(X, rng.randint(c, size=n_data), c, prior_sd=3.0)
    if kind == 'multilevel':                         # (n_data, p, groups)
        return vb.MultilevelRegressionModel(X, (rng.rand(n_data) < 0.5).astype(float), rng.randint(c, size=n_data), c,
                                            prior_sd=3.0)
    if kind in ('locscale', 'locscale_const'):       # (n_data, p, q): Student-t, with a scale design / a constant scale
        W = rng.randn(n_data, c) / np.sqrt(c) if kind == 'locscale' else None
        y = eta + np.exp(0.3 * rng.randn(n_data)) * rng.standard_t(4.5, size=n_data)
        return vb.LocationScaleRegressionModel(X, y, W, 'student_t', 4.5, prior_sd=3.0, scale_prior_sd=0.8)
    assert kind == 'sparse'                          # (n_data, p, entries per row): logistic, plus a column of ones
    A = np.zeros((n_data, p + 1))
    for i in range(n_data):
        A[i, rng.choice(p, size=c, replace=False)] = rng.randn(c) / np.sqrt(c)
    A[:, p] = 1.0
    y = (rng.rand(n_data) < 1.0 / (1.0 + np.exp(-A[:, :p] @ rng.randn(p)))).astype(float)
    return vb.SparseRegressionModel.from_dense(A, y, likelihood='logistic', prior_sd=3.0)


def _target_calls(vb, family, name):
    """TARGET_CALLS calls of ExclusiveKL over a fresh family of the kind on the target, on the current default engine."""
    model = _target(vb, name)
    d = model.dim
    rng = np.random.RandomState(d)
    if family == 'fr':
        fam = vb.FullRankGaussian(d, seed=4, rng='philox')
        th = fam.pack(0.1 * rng.randn(d), np.tril(0.02 * rng.randn(d, d), -1) + 0.3 * np.eye(d))
    else:
        fam = vb.MFGaussian(d, seed=4, rng='philox')
        th = np.concatenate([0.1 * rng.randn(d), -1.0 + 0.1 * rng.randn(d)])
    obj = vb.ExclusiveKL(fam, model, N_DRAWS)
    out = []
    for _ in range(TARGET_CALLS):
        v, g = obj(th)
        out.append((v, g.copy()))
        th = th - 0.01 * g / (1.0 + np.abs(g))
    del obj, fam, model
    gc.collect()
    return out


_TARGET_SOLO = {}


def _target_solo(vb, family, name):
    if (family, name) not in _TARGET_SOLO:
        with S._fresh_engine():
            _TARGET_SOLO[family, name] = _target_calls(vb, family, name)
    return _TARGET_SOLO[family, name]


LOGI, LOGI_S = ('logistic', 333, 37, 0), ('logistic', 77, 37, 0)
POIS, POIS_S = ('poisson', 333, 37, 0), ('poisson', 77, 37, 0)
SOFT, SOFT_S = ('softmax', 333, 9, 5), ('softmax', 77, 7, 3)             # dim 45 and 21
MULT, MULT_S = ('multilevel', 333, 14, 11), ('multilevel', 77, 9, 6)     # dim 26 and 16
LOCS, LOCS_S = ('locscale', 333, 14, 5), ('locscale', 77, 9, 3)           # dim 19 and 12
LOCC, LOCC_S = ('locscale_const', 333, 14, 5), ('locscale_const', 77, 9, 3)      # dim 15 and 10 (q = 1)
SPAR, SPAR_S = ('sparse', 333, 14, 5), ('sparse', 77, 9, 3)               # dim 15 and 10
TARGET_SEQUENCES = {
    'logistic': [LOGI, LOGI_S, LOGI],
    'poisson': [POIS, POIS_S],
    'softmax': [SOFT, SOFT_S, SOFT],
    'multilevel': [MULT, MULT_S, MULT],
    'locscale': [LOCS, LOCS_S, LOCS],
    'locscale_const': [LOCC, LOCC_S, LOCC],
    'sparse': [SPAR, SPAR_S, SPAR],
    'source': [('source', 48, 0, 0), ('source', 37, 0, 0)],
    'mixed': [LOGI, SOFT_S, POIS_S, MULT_S, SOFT, LOGI_S, MULT],
    # the four rows targets on one workspace: large, small, large, each in the order softmax, sparse, location-scale,
    # multilevel, then softmax again
    'rows_mixed': [SOFT, SPAR, LOCS, MULT, SOFT_S, SPAR_S, LOCS_S, MULT_S, SOFT, SPAR, LOCS, MULT, SOFT],
}


@pytest.mark.parametrize('family', ['fr', 'mf'])
@pytest.mark.parametrize('seq', list(TARGET_SEQUENCES))
def test_targets_with_data_one_after_another(vb, seq, family):
    names = TARGET_SEQUENCES[seq]
    want = [_target_solo(vb, family, name) for name in names]
    with S._fresh_engine():
        for pos, name in enumerate(names):
            S.same(want[pos], _target_calls(vb, family, name), 'step {}: {} under {}'.format(pos, name, family))


# ---- 3. engine entry points without an objective ---------------------------------------------------------------------------
# Each entry: `run(vb, eng, large)` makes the call on the (default) engine `eng` with the large or the small input and
# returns its outputs as arrays; `check(vb, outs)` compares the SMALL call's outputs with numpy or the oracle at the
# tolerance of the entry's own test module.  The large inputs are loud where the entry lets the caller choose them.
def _heavy(n, m=None):
    rng = np.random.RandomState(n % 1000 + 7)
    return 2.0 * rng.standard_t(3.0, n if m is None else (m, n))         # test_gpu_psis.py's 'student' weights


def _close_k(k, ref):
    return np.isinf(k) if np.isinf(ref) else abs(k - ref) <= 1e-10 * max(1.0, abs(ref))


def _run_psis(vb, eng, large):
    n = 70000 if large else 1500
    sm, k = eng.psis_smooth(n, _heavy(n))
    return sm, np.array(k)


def _check_psis(vb, outs):
    from oracle import psis as opsis
    ref, rk = opsis.psis_smooth(_heavy(1500))
    assert _close_k(float(outs[1]), rk)
    np.testing.assert_allclose(outs[0], ref, rtol=0, atol=1e-10)


def _run_psis_batch(vb, eng, large):
    # the batched kernel takes vectors of at most PSIS_BATCH_MAX_N = 16 384 values (longer ones are refused by the entry)
    m, n = (5, 16384) if large else (3, 1500)
    return eng.psis_smooth_batch(_heavy(n, m))


def _check_psis_batch(vb, outs):
    from oracle import psis as opsis
    lw = _heavy(1500, 3)
    for j in range(3):
        ref, rk = opsis.psis_smooth(lw[j])
        assert _close_k(outs[1][j], rk)
        np.testing.assert_allclose(outs[0][j], ref, rtol=0, atol=1e-10)


def _loo_inputs(vb, large):
    from oracle import psis as opsis
    model = _target(vb, LOGI if large else LOGI_S)
    s = 1031 if large else 515
    rng = np.random.RandomState(s)
    x = 0.3 * rng.randn(s, 37)
    log_ratios = 0.5 * rng.standard_t(6.0, s)
    return model, x, log_ratios, opsis.psis_smooth(log_ratios)[0]


def _run_loo(vb, eng, large):
    model, x, log_ratios, log_w = _loo_inputs(vb, large)
    eng.set_model(model.device_spec())
    return eng.glm_psis_loo(x, model.X.shape[0], log_ratios=log_ratios, log_w=log_w)


def _check_loo(vb, outs):
    import _loo_oracle as LO
    model, x, log_ratios, log_w = _loo_inputs(vb, False)
    loos, ks, lpd = LO.loo_numpy(LO.glm_pointwise_numpy('logistic', model.X, model.y, x), log_ratios, 1.0, log_w)
    np.testing.assert_allclose(outs[0], loos, rtol=0, atol=1e-9)
    np.testing.assert_allclose(outs[2], lpd, rtol=0, atol=1e-9)
    assert all(LO.close_k(k, rk) for k, rk in zip(outs[1], ks))


def _chain(large):
    rows, p = (300, 65) if large else (120, 37)
    rs = np.random.RandomState(rows + p)
    e = rs.randn(rows, p)
    x = np.empty_like(e)
    x[0] = e[0]
    for t in range(1, rows):
        x[t] = 0.9 * x[t - 1] + e[t]
    return (1e3 + 10.0 * x) if large else (3.0 + 1e-2 * x)               # test_gpu_chain_stats.py's chains; the large one loud


def _run_chain(vb, eng, large):
    chain = _chain(large)
    rows, p = chain.shape
    eng.chain_open(p, rows)          # "no zero fill: every row is written before it is read"
    try:
        eng.chain_append(chain)
        worst, rhat = eng.chain_rhat([rows, rows - 1], per_column=True)
        out = [eng.chain_mean(rows).copy(), eng.chain_mean(rows - 1).copy(), worst, rhat]
        for w in (rows, rows - 1):
            out.extend(eng.chain_ess_mcse(w))
    finally:
        eng.chain_close()
    return tuple(np.array(o) for o in out)


def _check_chain(vb, outs):
    from viabel_amd import _chain_stats as cs
    from test_gpu_chain_stats import ESS_TOL, RHAT_TOL, _host_smallest_examined_pair_sum
    chain = _chain(False)
    rows, p = chain.shape
    np.testing.assert_array_equal(outs[0], np.mean(chain, axis=0))
    np.testing.assert_array_equal(outs[1], np.mean(chain[1:], axis=0))
    for i, w in enumerate((rows, rows - 1)):
        ref = cs.compute_R_hat(chain[-w:])
        np.testing.assert_allclose(outs[3][i], ref, rtol=RHAT_TOL, atol=0)
        assert abs(outs[2][i] - np.max(ref)) <= RHAT_TOL * np.max(ref)
        ess, mcse = outs[4 + 2 * i], outs[5 + 2 * i]
        ref_ess, ref_mcse = cs.MCSE(chain[-w:])
        err = np.maximum(np.abs(ess - ref_ess) / ref_ess, np.abs(mcse - ref_mcse) / ref_mcse)
        off = np.flatnonzero(~(err <= ESS_TOL))
        excused = [j for j in off if _host_smallest_examined_pair_sum(chain[-w:, j]) < 1e-8]
        assert len(excused) == len(off) and len(excused) <= p // 100, (off, err[off])


def _sqrt_inputs(large):
    from test_gpu_linalg import _spd
    d, cond = (130, 1e4) if large else (37, 1e2)
    a = _spd(d, cond, 100 + d) * (1e3 if large else 1.0)
    e = np.random.RandomState(d).randn(d, d)
    return a, 0.5 * (e + e.T) * 37.0


def _run_sqrt(vb, eng, large):
    root, x, info = eng.sym_sqrt(*_sqrt_inputs(large))
    return root, x, np.array(info)


def _check_sqrt(vb, outs):
    from test_gpu_linalg import _reference
    a, e = _sqrt_inputs(False)
    want_root, want_x = _reference(a, e)
    np.testing.assert_allclose(outs[0], want_root, rtol=0, atol=1e-13 * np.linalg.norm(want_root))
    np.testing.assert_allclose(outs[1], want_x, rtol=0, atol=1e-11 * np.linalg.norm(want_x))


def _path_inputs(large):
    D, k, N = (70, 5, 513) if large else (37, 3, 130)
    rng = np.random.RandomState(D + k)
    return D, k, N, rng.randn(D, k), rng.randn(N, D), rng.randn(N, k)


def _run_path_terms(vb, eng, large):
    D, k, N, sw, E, Z = _path_inputs(large)
    loud = (1e3, 10.0) if large else (0.0, 1.0)
    eng.noise_set_host(50, loud[0] + loud[1] * E)
    eng.noise_set_host(51, loud[0] + loud[1] * Z)
    return eng.lowrank_path_terms(50, 51, N, D, k, sw)


def _check_path_terms(vb, outs):
    D, k, N, sw, E, Z = _path_inputs(False)
    T = np.concatenate([Z, E @ sw], axis=1)
    for got, ref in zip(outs, (E.T @ T, T.T @ T, E.sum(0), (E * E).sum(0), T.sum(0))):
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12 * max(1.0, np.max(np.abs(ref))))


def _grad_inputs(vb, kind, large):
    from oracle import models as omod
    N, D = (777, 45) if large else (64, 37)
    rng = np.random.RandomState(N + D)
    if kind == 'gauss_full':
        A = rng.randn(D, D)
        Sg = A @ A.T / D + np.eye(D)
        mean = rng.randn(D)
        model, omodel = vb.CorrelatedGaussianModel(mean, covariance=Sg), omod.GaussFull(mean, np.linalg.inv(Sg))
    else:
        X = rng.randn(3 * D + 7, D) / np.sqrt(D)
        y = (rng.rand(3 * D + 7) < 0.5).astype(float)
        model, omodel = vb.LogisticRegressionModel(X, y, prior_sd=3.0), omod.Logistic(X, y, prior_sd=3.0)
    return model, omodel, (30.0 if large else 0.4) * rng.randn(N, D)


def _run_grad(kind):
    def run(vb, eng, large):
        model, _, x = _grad_inputs(vb, kind, large)
        return (model.grad(x),)
    return run


def _check_grad(kind):
    def check(vb, outs):
        _, omodel, x = _grad_inputs(vb, kind, False)
        go = omodel.grad(x)
        np.testing.assert_allclose(outs[0], go, rtol=0, atol=1e-12 * np.max(np.abs(go)))
    return check


ENTRIES = {
    'psis_smooth': (_run_psis, _check_psis),
    'psis_smooth_batch': (_run_psis_batch, _check_psis_batch),
    'glm_psis_loo': (_run_loo, _check_loo),
    'chain': (_run_chain, _check_chain),
    'sym_sqrt': (_run_sqrt, _check_sqrt),
    'lowrank_path_terms': (_run_path_terms, _check_path_terms),
    'model_grad_gauss_full': (_run_grad('gauss_full'), _check_grad('gauss_full')),
    'model_grad_logistic': (_run_grad('logistic'), _check_grad('logistic')),
}


@pytest.mark.parametrize('entry', list(ENTRIES))
def test_entry_point_large_small_large(vb, entry):
    run, check = ENTRIES[entry]
    fresh = {}
    for large in (True, False):
        with S._fresh_engine() as eng:
            fresh[large] = run(vb, eng, large)
    check(vb, fresh[False])
    with S._fresh_engine() as eng:
        for pos, large in enumerate((True, False, True)):
            got = run(vb, eng, large)
            assert len(got) == len(fresh[large])
            for i, (a, b) in enumerate(zip(fresh[large], got)):
                np.testing.assert_array_equal(b, a, err_msg='{}: call {} ({}), output {}'.format(
                    entry, pos, 'large' if large else 'small', i))
