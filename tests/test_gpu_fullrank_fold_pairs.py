"""GPU: the folded full-rank evaluation forms M = L' P in ONE launch that writes M itself -- a workgroup computes row
blocks b and T - 1 - b (64 rows each, T of them) of a column tile, each over its whole k range (vb_gemm_f64_dma.h,
gemm_f64_dma_pair_kernel) -- and b = P (mu - m) in the blocks of fr_fold_ssum_kernel that form colsum(G).

The shapes are the smallest at which the route runs and the pairing can go wrong: (1024, 3072) T = 16, every block paired;
(1040, 3120) T = 17, the middle block unpaired, D no multiple of 32 (ragged last column tile and last row block);
(1088, 3328) T = 17 with D a multiple of 64.  Tolerances are the project's: value 1e-12 relative, gradient 1e-11 of its
largest entry."""
import functools

import numpy as np
import pytest

from oracle import families as ofam
from oracle import models as omod
from oracle import objectives as oobj

pytestmark = pytest.mark.gpu

SLOT = 3
SHAPES = [(1024, 3072), (1040, 3120), (1088, 3328)]


@functools.lru_cache(maxsize=None)
def _model(D):
    import viabel_amd as vb
    rng = np.random.RandomState(3)
    A = rng.randn(D, D)
    cov = A @ A.T / D + np.eye(D)
    return vb.CorrelatedGaussianModel(rng.randn(D), covariance=cov)


def _mu_and_root(D, model, mu_offset, seed=8, tri=0.3):
    """mu = m + mu_offset * (random signs and sizes in [0.5, 1.5]); L with a dense strict lower triangle of the diagonal's
    size, so that M = L' P is dense in every row block."""
    rng = np.random.RandomState(seed)
    L = np.tril(tri * rng.randn(D, D), -1) + np.diag(np.exp(-1.0 + 0.1 * rng.randn(D)))
    mu = model.mean + mu_offset * rng.choice([-1.0, 1.0], D) * (0.5 + rng.rand(D))
    return mu, L


def _theta(D, model, mu_offset):
    import viabel_amd as vb
    return vb.FullRankGaussian(D).pack(*_mu_and_root(D, model, mu_offset))


@functools.lru_cache(maxsize=None)
def _unit_noise(D, N):
    """Row i < 3 D is the unit vector e_(i mod D), the other rows are zero: S = E' E = 3 I and s = colsum(E) = 3 * 1."""
    noise = np.zeros((N, D))
    i = np.arange(3 * D)
    noise[i, i % D] = 1.0
    noise.setflags(write=False)
    return noise


@functools.lru_cache(maxsize=None)
def _random_noise(D, N, seed):
    noise = np.random.RandomState(seed).randn(N, D) + 0.5
    noise[:, D // 3] -= 2.0
    noise.setflags(write=False)
    return noise


def _evaluate(eng, model, theta, D, n, noise):
    """(value, grad) of the `n` rows of `noise`, uploaded to slot SLOT; asserts that the folded route ran (no sampling and
    no model product, one launch timed as the gradient product)."""
    from viabel_amd import _lib
    eng.set_model(model.device_spec())
    eng.noise_set_host(SLOT, noise)
    eng.fullrank_set_theta(theta, D)
    kernels = (_lib.PROF_FR_SAMPLE_GEMM, _lib.PROF_FR_MODEL_GEMM, _lib.PROF_FR_GRAD_GEMM)
    eng.profile_enable(True)
    try:
        for k in kernels:
            eng.profile_read(reset=True, kernel=k)
        eng.elbo_grad_fullrank_enqueue(SLOT, n, D)
        out = eng.fullrank_get(D)
        launches = tuple(eng.profile_read(reset=True, kernel=k)[0] for k in kernels)
    finally:
        eng.profile_enable(False)
    assert launches == (0, 0, 1)
    return out


def _gradient_from_m(D, N, model, mu, L):
    """The gradient for `_unit_noise` from M = L' P formed in numpy.  With S = 3 I and s = 3 * 1:
      tril(C) = -3 tril(M') - b s'   and   colsum(G) = -3 colsum(M) - N b,      b = P (mu - m),
    and the result is  d/dmu = -colsum(G) / N,  d/dL_ij = -C_ij / N  (free diagonal: times L_ii, then - 1), the lower
    triangle packed row by row behind mu."""
    P = model.precision
    M = L.T @ P
    b = P @ (mu - model.mean)
    C = -3.0 * M.T - 3.0 * b[:, None]
    gL = -C / N
    d = np.arange(D)
    gL[d, d] = gL[d, d] * L[d, d] - 1.0
    g_mu = (3.0 * M.sum(axis=0) + N * b) / N
    return np.concatenate([g_mu, gL[np.tril_indices(D)]])


@pytest.mark.parametrize('mu_offset', [0.0, 10.0])
@pytest.mark.parametrize('D,N', SHAPES)
def test_every_row_block_of_m_lands_where_it_belongs(D, N, mu_offset):
    """With unit-vector noise the gradient IS M, entry by entry: its upper triangle through C, every column through the
    column sums.  A row block computed over the wrong k range, written to the wrong rows or left out misses the bound by
    orders of magnitude.  Once with mu = m (b = 0 exactly) and once with |mu - m| of order 10."""
    from viabel_amd import _lib
    model = _model(D)
    mu, L = _mu_and_root(D, model, mu_offset)
    if mu_offset == 0.0:
        assert np.array_equal(mu, model.mean)
    theta = _theta(D, model, mu_offset)
    noise = _unit_noise(D, N)
    v, g = _evaluate(_lib.default_engine(), model, theta, D, N, noise)

    ov, og = oobj.exclusive_kl(ofam.FullRankGaussian(D), omod.GaussFull(model.mean, model.precision), theta, noise)
    rel_v = abs(v - ov) / abs(ov)
    rel_g = np.max(np.abs(g - og)) / np.max(np.abs(og))
    gm = _gradient_from_m(D, N, model, mu, L)
    rel_m = np.max(np.abs(g - gm)) / np.max(np.abs(gm))
    print('D=%d N=%d mu_offset=%g: rel err value %.2e, gradient %.2e (oracle) %.2e (from numpy L\' P) of its largest entry'
          % (D, N, mu_offset, rel_v, rel_g, rel_m))
    assert rel_v < 1e-12
    assert rel_g < 1e-11
    assert rel_m < 1e-11


def test_same_inputs_same_bits():
    """(1040, 3120): twice on one engine and once on a fresh engine -- every sum is in a fixed order."""
    from viabel_amd import _lib
    D, N = SHAPES[1]
    model = _model(D)
    theta = _theta(D, model, 3.0)
    noise = _random_noise(D, N, 31)
    eng = _lib.default_engine()
    v1, g1 = _evaluate(eng, model, theta, D, N, noise)
    v2, g2 = _evaluate(eng, model, theta, D, N, noise)
    fresh = _lib.Engine(eng.device)
    try:
        vf, gf = _evaluate(fresh, model, theta, D, N, noise)
    finally:
        fresh.close()
    assert v2 == v1 and vf == v1
    np.testing.assert_array_equal(g2, g1)
    np.testing.assert_array_equal(gf, g1)


def test_m_buffer_holds_nothing_from_before():
    """(1088, 3328) and then (1024, 3072) on one engine: the second result has the bits of a fresh engine's, so every entry
    of M the smaller shape reads was written by its own launch."""
    from viabel_amd import _lib
    (D1, N1), (D0, N0) = SHAPES[2], SHAPES[0]
    eng = _lib.default_engine()
    m1 = _model(D1)
    _evaluate(eng, m1, _theta(D1, m1, 3.0), D1, N1, _random_noise(D1, N1, 41))
    m0 = _model(D0)
    theta, noise = _theta(D0, m0, 3.0), _random_noise(D0, N0, 42)
    v, g = _evaluate(eng, m0, theta, D0, N0, noise)
    fresh = _lib.Engine(eng.device)
    try:
        vf, gf = _evaluate(fresh, m0, theta, D0, N0, noise)
    finally:
        fresh.close()
    assert v == vf
    np.testing.assert_array_equal(g, gf)
