"""CPU: MinibatchRegressionModel's host side -- export and wiring, constructor validation, full_model(), the batch counter,
batch_indices against the plain-int restatement of tests/_minibatch_oracle.py, the permutation's properties (every epoch a
permutation, epochs differ, marginal uniformity of a slot), the refusals that need no GPU -- and the oracle's own gradient
against central differences."""
import math
import os
import re

import numpy as np
import pytest

import viabel_amd as vb
from viabel_amd import _lib
import _minibatch_oracle as O

LIKELIHOODS = ['logistic', 'poisson', 'gaussian']
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _data(n_data, p, lik='logistic', seed=0):
    rng = np.random.RandomState(seed)
    X = rng.randn(n_data, p) / np.sqrt(p)
    if lik == 'logistic':
        y = (rng.rand(n_data) < 0.5).astype(float)
    elif lik == 'poisson':
        y = rng.poisson(2.0, size=n_data).astype(float)
    else:
        y = rng.randn(n_data)
    return X, y


def test_exported_from_package_and_bound():
    assert vb.MinibatchRegressionModel is vb.models.MinibatchRegressionModel
    assert 'MinibatchRegressionModel' in vb.models.__all__
    assert _lib.MODEL_MINIBATCH_GLM == 9 and _lib.MODEL_MINIBATCH_GLM in _lib.MODELS_WITH_ROWS
    for name in ('vb_minibatch_set_batch', 'vb_minibatch_get_batch', 'vb_minibatch_indices', 'vb_minibatch_pointwise'):
        assert name in _lib.SIGNATURES
    assert _lib.SIGNATURES['vb_minibatch_pointwise'] == _lib.SIGNATURES['vb_sparse_glm_pointwise']
    assert not issubclass(vb.MinibatchRegressionModel, vb.LogisticRegressionModel)


def test_header_and_common_mirror_the_constants():
    header = open(os.path.join(ROOT, 'include', 'viabel_hip.h')).read()
    assert re.search(r'#define\s+VB_MODEL_MINIBATCH_GLM\s+9\b', header)
    for name in ('vb_minibatch_set_batch', 'vb_minibatch_get_batch', 'vb_minibatch_indices', 'vb_minibatch_pointwise'):
        assert re.search(r'int\s+%s\s*\(' % name, header)
    common = open(os.path.join(ROOT, 'viabel_amd', 'csrc', 'vb_common.h')).read()
    assert re.search(r'model_has_rows\(int id\)\s*\{[^}]*VB_MODEL_MINIBATCH_GLM', common)
    m = re.search(r'kMinibatchChunkDoubles\s*=\s*\(int64_t\)(\d+)\s*<<\s*(\d+)', common)
    assert m and int(m.group(1)) << int(m.group(2)) == _lib.MINIBATCH_CHUNK_DOUBLES
    assert 'vb_minibatch.hip' in open(os.path.join(ROOT, 'viabel_amd', 'csrc', 'Makefile')).read()
    source = open(os.path.join(ROOT, 'viabel_amd', 'csrc', 'vb_minibatch.hip')).read()
    m = re.search(r'kMbRounds\s*=\s*(\d+)\s*;', source)
    assert m and int(m.group(1)) == O.ROUNDS == vb.MinibatchRegressionModel.FEISTEL_ROUNDS >= 4


def test_chunk_rule():
    """max(8, budget / (2 round_up(B, 16))): the term and the residual matrix of a chunk together stay within the budget."""
    budget = _lib.MINIBATCH_CHUNK_DOUBLES
    assert _lib.minibatch_chunk_rows(1) == budget // 32
    assert _lib.minibatch_chunk_rows(16) == budget // 32 and _lib.minibatch_chunk_rows(17) == budget // 64
    assert _lib.minibatch_chunk_rows(2500) == budget // (2 * 2512)
    assert _lib.minibatch_chunk_rows(1 << 22) == 8


def test_argument_errors():
    X, y = _data(20, 3)
    M = vb.MinibatchRegressionModel
    for bad in (0, 21, -1, 2.0, True, None):
        with pytest.raises(ValueError, match='batch_size'):
            M(X, y, bad)
    M(X, y, 1), M(X, y, 20), M(X, y, np.int64(5))
    with pytest.raises(ValueError):
        M(X, y[:-1], 4)
    with pytest.raises(ValueError):
        M(X[:, :0], y, 4)
    with pytest.raises(ValueError, match='likelihood'):
        M(X, y, 4, likelihood='probit')
    with pytest.raises(ValueError, match='order'):
        M(X, y, 4, order='random')
    with pytest.raises(ValueError):
        M(X, y, 4, prior_sd=0.0)
    with pytest.raises(ValueError):
        M(X, y, 4, likelihood='gaussian', noise_sd=-1.0)
    for bad in (-1, 1 << 64, 1.5):
        with pytest.raises(ValueError, match='seed'):
            M(X, y, 4, seed=bad)
    M(X, y, 4, seed=(1 << 64) - 1)
    with pytest.raises(ValueError):                     # the responses, as the dense targets check them
        M(X, y + 0.5, 4)
    with pytest.raises(ValueError):
        M(X, -np.ones(20), 4, likelihood='poisson')
    with pytest.raises(ValueError):
        M(X, np.full(20, np.nan), 4, likelihood='gaussian')


def test_properties_counter_and_spec():
    X, y = _data(10, 3)
    m = vb.MinibatchRegressionModel(X, y, 4, seed=(1 << 64) - 2, order='sequential')
    assert (m.dim, m.n_data, m.batch_size, m.batch, m.epoch) == (3, 10, 4, 0, 0)
    m.batch = 3
    assert m.batch == 3 and m.epoch == 1                 # positions 12 .. 15: epoch 1
    m.batch = np.int64(5)
    assert m.batch == 5 and m.epoch == 2 and isinstance(m.batch, int)
    for bad in (-1, 1.0, True, None, (1 << 62) // 4):
        with pytest.raises(ValueError):
            m.batch = bad
    assert m.batch == 5
    spec = m.device_spec()
    assert spec[0] == _lib.MODEL_MINIBATCH_GLM and spec[1] == 3
    assert spec[2].size == 10 * 3 + 10 + 2 and spec[3].dtype == np.int64
    assert list(spec[3]) == [10, 4, _lib.GLM_BERNOULLI_LOGIT, 0, -2]       # the seed's 64 bits as an int64
    assert spec[4] == [5] and m.device_spec() is spec
    m.batch = 6
    assert spec[4] == [6]                                # the binding reads the model's own counter


@pytest.mark.parametrize('lik', LIKELIHOODS)
def test_full_model(lik):
    X, y = _data(12, 3, lik)
    full = vb.MinibatchRegressionModel(X, y, 5, likelihood=lik, prior_sd=2.5, noise_sd=0.7).full_model()
    cls = dict(logistic=vb.LogisticRegressionModel, poisson=vb.PoissonRegressionModel, gaussian=vb.LinearRegressionModel)[lik]
    assert type(full) is cls
    assert full.X is X and np.array_equal(full.y, y) and full.prior_sd == 2.5
    if lik == 'gaussian':
        assert full.noise_sd == 0.7


def test_vectorised_oracle_equals_the_plain_one():
    for n_data, seed in ((5, 3), (64, 1 << 40), (65, 7), (1000, 0)):
        slots = np.arange(n_data)[:min(n_data, 40)]
        for epoch in (0, 3, (1 << 33) + 1):
            ref = [O.permute(int(s), epoch, n_data, seed)[0] for s in slots]
            assert list(O.permute_array(slots, epoch, n_data, seed)) == ref
    for order in ('shuffle', 'sequential'):
        for t in (0, 9, 10, 1 << 30):                  # (t = 9, 10: a batch across an epoch's end, the next epoch)
            assert np.array_equal(O.batch_indices_array(t, 65, 7, 11, order), O.batch_indices(t, 65, 7, 11, order))


@pytest.mark.parametrize('n_data,B', [(1, 1), (2, 1), (3, 2), (33, 7), (64, 16), (65, 16), (1000, 96)])
def test_batch_indices_equal_the_oracle(n_data, B):
    X, y = _data(n_data, 1)
    for seed in (0, 12345, (1 << 63) + 5):
        m = vb.MinibatchRegressionModel(X, y, B, seed=seed)
        for t in (0, 1, 2, n_data // B, 5 * n_data + 3, (1 << 40) // B):
            got = m.batch_indices(t)
            assert got.dtype == np.int64 and got.shape == (B,)
            assert np.array_equal(got, O.batch_indices(t, n_data, B, seed)), (n_data, B, seed, t)
        m.batch = 2
        assert np.array_equal(m.batch_indices(), m.batch_indices(2))
    with pytest.raises(ValueError):
        m.batch_indices(-1)


@pytest.mark.parametrize('n_data', [1, 2, 3, 64, 65, 1000])
def test_every_epoch_is_a_permutation_and_epochs_differ(n_data):
    """B = 1: batch t is position t, so n_data consecutive batches are one epoch.  The oracle's whole epoch and the
    model's, both a permutation of range(n_data); three epochs that differ from each other (n_data >= 64: the chance that two
    independent permutations coincide is 1 / 64!)."""
    X, y = _data(n_data, 1)
    seed = 99
    m = vb.MinibatchRegressionModel(X, y, 1, seed=seed)
    perms = []
    for epoch in (0, 1, 7):
        ref = O.epoch_permutation(epoch, n_data, seed)
        assert sorted(ref) == list(range(n_data))
        got = np.concatenate([m.batch_indices(epoch * n_data + s) for s in range(min(n_data, 70))])
        assert np.array_equal(got, ref[:got.size])
        perms.append(ref)
    if n_data >= 64:
        assert not np.array_equal(perms[0], perms[1]) and not np.array_equal(perms[1], perms[2])
        assert not np.array_equal(perms[0], perms[2])
    # a whole epoch through batches that do not divide it
    if n_data >= 3:
        B = 3 if n_data % 3 else 2
        mb = vb.MinibatchRegressionModel(X, y, B, seed=seed)
        stream = np.concatenate([mb.batch_indices(t) for t in range(-(-2 * n_data // B))])
        assert sorted(stream[:n_data]) == list(range(n_data)) and sorted(stream[n_data:2 * n_data]) == list(range(n_data))


def test_walk_lengths_at_the_domain_edges():
    """n_data = 64 fills the Feistel domain 2^6 exactly (no walk is ever longer than one pass); n_data = 65 has the domain
    2^8, almost four times itself: the longest walks."""
    assert O.half_bits(64) == 3 and O.half_bits(65) == 4 and O.half_bits(1) == 1 and O.half_bits(2) == 1
    assert O.half_bits(5) == 2 and O.half_bits(17) == 3 and O.half_bits((1 << 31) - 1) == 16
    assert max(O.permute(s, 0, 64, 5)[1] for s in range(64)) == 1
    assert max(O.permute(s, 0, 65, 5)[1] for s in range(65)) > 3


def test_sequential_order_and_a_batch_across_an_epoch_boundary():
    X, y = _data(10, 1)
    seq = vb.MinibatchRegressionModel(X, y, 4, order='sequential')
    for t in range(8):
        assert list(seq.batch_indices(t)) == [(4 * t + i) % 10 for i in range(4)]
    assert list(seq.batch_indices(2)) == [8, 9, 0, 1]              # positions 8 .. 11: the end of epoch 0, the start of epoch 1
    shuf = vb.MinibatchRegressionModel(X, y, 4, seed=3)
    p0, p1 = O.epoch_permutation(0, 10, 3), O.epoch_permutation(1, 10, 3)
    assert list(shuf.batch_indices(2)) == [p0[8], p0[9], p1[0], p1[1]]
    assert list(shuf.batch_indices(2)) == list(O.batch_indices(2, 10, 4, 3))


def _chi2_quantiles(df):
    """(0.001, 0.999) quantiles of chi-square(df): scipy's, or Wilson and Hilferty's cube-root normal approximation."""
    try:
        from scipy.stats import chi2
        return float(chi2.ppf(0.001, df)), float(chi2.ppf(0.999, df))
    except ImportError:
        z = 3.090232306167813                                      # the 0.999 quantile of the standard normal
        c = 2.0 / (9.0 * df)
        return df * (1.0 - c - z * math.sqrt(c)) ** 3, df * (1.0 - c + z * math.sqrt(c)) ** 3


def test_a_slot_is_marginally_uniform():
    """The observation of slot 0 over 25 600 epochs at n_data = 256, seed fixed: 100 expected per observation, the chi-square
    statistic within the (0.001, 0.999) quantiles of chi-square(255) -- too even is as wrong as too uneven."""
    n_data, epochs, seed = 256, 25600, 2024
    obs = O.permute_array(0, np.arange(epochs), n_data, seed)
    counts = np.bincount(obs, minlength=n_data)
    expected = epochs / n_data
    stat = float(np.sum((counts - expected) ** 2) / expected)
    lo, hi = _chi2_quantiles(n_data - 1)
    print('chi-square statistic %.1f, bounds (%.1f, %.1f)' % (stat, lo, hi))
    assert lo < stat < hi, (stat, lo, hi)
    X, y = _data(n_data, 1)
    m = vb.MinibatchRegressionModel(X, y, 1, seed=seed)
    assert [int(m.batch_indices(e * n_data)[0]) for e in range(50)] == list(obs[:50])


@pytest.mark.parametrize('lik', LIKELIHOODS)
def test_oracle_density(lik):
    """The oracle's gradient against central differences of its value; B = n_data in natural order is the flat GLM density;
    the mean over the batches of an epoch is the full density."""
    from _sparse_oracle import SparseGLMOracle
    n_data, p, B = 24, 3, 6
    X, y = _data(n_data, p, lik, seed=4)
    theta = 0.3 * np.random.RandomState(1).randn(2, p)
    full = SparseGLMOracle(X, y, lik, 2.0, 0.7)
    whole = O.MinibatchOracle(X, y, np.arange(n_data), lik, 2.0, 0.7)
    assert np.allclose(whole.logp(theta), full.logp(theta), rtol=1e-13, atol=0)
    assert np.allclose(whole.grad(theta), full.grad(theta), rtol=1e-12, atol=1e-13)
    assert np.allclose(whole.pointwise(theta), full.pointwise(theta), rtol=1e-13, atol=0)
    batches = [O.MinibatchOracle(X, y, O.batch_indices(t, n_data, B, 8), lik, 2.0, 0.7) for t in range(n_data // B)]
    assert np.allclose(np.mean([b.logp(theta) for b in batches], axis=0), full.logp(theta), rtol=1e-13, atol=0)
    assert np.allclose(np.mean([b.grad(theta) for b in batches], axis=0), full.grad(theta), rtol=1e-12, atol=1e-13)
    b, h = batches[1], 1e-6
    assert b.pointwise(theta).shape == (2, B)
    for j in range(p):
        e = np.zeros(p)
        e[j] = h
        fd = (b.logp(theta + e) - b.logp(theta - e)) / (2 * h)
        assert np.allclose(fd, b.grad(theta)[:, j], rtol=1e-6, atol=1e-6)


def test_refusals_that_need_no_gpu():
    X, y = _data(30, 3)
    m = vb.MinibatchRegressionModel(X, y, 10)
    theta = np.zeros(6)
    with pytest.raises(NotImplementedError, match='biased'):
        vb.DISInclusiveKL(vb.MFGaussian(3), m, 50, ess_target=20, temper_prior=vb.MFGaussian(3),
                          temper_prior_params=np.zeros(6))
    with pytest.raises(NotImplementedError, match='biased'):
        vb.AlphaDivergence(vb.MFGaussian(3), m, 50, 0.5)
    for method in ('full', 'mean_only', 'loo_diag_approx', 'loo_direct_approx'):
        with pytest.raises(NotImplementedError, match='full_model'):
            vb.ExclusiveKL(vb.MFGaussian(3), m, 50, hessian_approx_method=method)
    obj = vb.ExclusiveKL(vb.MFGaussian(3), m, 50)                   # admitted: building it touches no engine
    with pytest.raises(NotImplementedError, match='full_model'):
        obj._hessian_vector_product(theta, np.ones(6))
    with pytest.raises(NotImplementedError, match='full_model'):
        m.find_mode()
    with pytest.raises(NotImplementedError, match='full_model'):
        m.hessian(np.zeros(3))
    with pytest.raises(NotImplementedError, match='full_model'):
        vb.laplace_approximation(m)
    with pytest.raises(NotImplementedError, match='full_model'):
        vb.hmc(m, init=np.zeros((4, 3)), n_chains=4)
    for fn in (vb.vi_diagnostics, vb.loo, vb.predict):
        with pytest.raises(NotImplementedError, match='full_model'):
            fn(theta, model=m, approx=vb.MFGaussian(3), n_samples=100)
        with pytest.raises(NotImplementedError, match='full_model'):
            fn(theta, objective=obj, n_samples=100)
    with pytest.raises(NotImplementedError, match='full_model'):
        vb.samples_and_log_weights(theta, m, vb.MFGaussian(3), 100)
    assert m.batch == 0


def test_a_sharded_engine_refuses_the_binding():
    """Engine.set_model refuses before it touches the library: an engine object without a context stands in."""
    X, y = _data(30, 3)
    m = vb.MinibatchRegressionModel(X, y, 10)
    eng = _lib.Engine.__new__(_lib.Engine)
    eng._ctx, eng._model_key, eng.n_ranks, eng.rank = None, None, 2, 0
    with pytest.raises(NotImplementedError, match='sharded'):
        eng.set_model(m.device_spec())
