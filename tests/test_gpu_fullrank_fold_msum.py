"""GPU: the folded full-rank evaluation forms M = L' P in the same launch as the slab sums (fr_fold_msum_kernel: the paired
M tiles first, then the blocks of b = P (mu - m), of s = colsum(E) and of the 32 x 32 tiles of S), and colsum(G) =
-s' M - n b' behind the C product, from the b vector that launch wrote (fr_fold_csg_blocks).

The shapes are the smallest at which the route runs and the block arithmetic can go wrong: (1024, 3072) T = 16 row blocks,
every one paired; (1040, 3120) T = 17, D no multiple of 32 or 64 (ragged last S tile, last column tile and last row block);
(1088, 3328) T = 17 with D a multiple of 64.  The route asks D % 16 == 0, so D = 1028 is not admitted and every 8-column
block of b and colsum(G) is full at every shape of the route (1040: 130 of them); 1040 and 1088 are the shapes whose block
counts are no power of two.  Tolerances are the project's: value 1e-12 relative, gradient 1e-11 of its largest entry."""
import functools

import numpy as np
import pytest

from oracle import families as ofam
from oracle import models as omod
from oracle import objectives as oobj

pytestmark = pytest.mark.gpu

SLOT = 3
SHAPES = [(1024, 3072), (1040, 3120), (1088, 3328)]
BELOW_GATE = (512, 2048)
FOLD = (0, 0, 1)


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
def _random_noise(D, N, seed):
    """Non-zero column means (so that s != 0), one column shifted the other way."""
    noise = np.random.RandomState(seed).randn(N, D) + 0.5
    noise[:, D // 3] -= 2.0
    noise.setflags(write=False)
    return noise


def _evaluate(eng, model, theta, D, n, noise):
    """(value, grad) of the `n` rows of `noise`, uploaded to slot SLOT, and the launch counts of the three profiled kinds
    (sampling product, model product, gradient product): (0, 0, 1) is the folded route."""
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
    return out, launches


def _evaluate_fold(eng, model, theta, D, n, noise):
    out, launches = _evaluate(eng, model, theta, D, n, noise)
    assert launches == FOLD
    return out


@functools.lru_cache(maxsize=None)
def _case(D, N, mu_offset):
    """One evaluation on the default engine and its oracle, shared by the tests below: (value, grad, oracle value, oracle
    grad)."""
    from viabel_amd import _lib
    model = _model(D)
    theta = _theta(D, model, mu_offset)
    noise = _random_noise(D, N, 21)
    v, g = _evaluate_fold(_lib.default_engine(), model, theta, D, N, noise)
    ov, og = oobj.exclusive_kl(ofam.FullRankGaussian(D), omod.GaussFull(model.mean, model.precision), theta, noise)
    g = np.array(g)
    g.setflags(write=False)
    og.setflags(write=False)
    return v, g, ov, og


@pytest.mark.parametrize('mu_offset', [0.0, 10.0])
@pytest.mark.parametrize('D,N', SHAPES)
def test_value_and_gradient_against_the_oracle(D, N, mu_offset):
    """Noise with non-zero column means, |mu - m| of order 10 (b weighs in) and once mu = m (b = 0 exactly)."""
    if mu_offset == 0.0:
        model = _model(D)
        assert np.array_equal(_mu_and_root(D, model, mu_offset)[0], model.mean)
    v, g, ov, og = _case(D, N, mu_offset)
    rel_v = abs(v - ov) / abs(ov)
    rel_g = np.max(np.abs(g - og)) / np.max(np.abs(og))
    print('D=%d N=%d mu_offset=%g: rel err value %.2e, gradient %.2e of its largest entry' % (D, N, mu_offset, rel_v, rel_g))
    assert rel_v < 1e-12
    assert rel_g < 1e-11


@pytest.mark.parametrize('D,N', SHAPES)
def test_column_sums_of_g_formed_behind_the_c_product(D, N):
    """The first D entries of the gradient are -colsum(G) / N = (s' M + n b') / N: against numpy's M = L' P, s and b."""
    model = _model(D)
    mu, L = _mu_and_root(D, model, 10.0)
    _, g, _, _ = _case(D, N, 10.0)
    P = model.precision
    M = L.T @ P
    s = _random_noise(D, N, 21).sum(axis=0)
    b = P @ (mu - model.mean)
    assert np.max(np.abs(s)) > 100.0 and np.max(np.abs(b)) > 1.0
    want = (s @ M + N * b) / N
    rel = np.max(np.abs(g[:D] - want)) / np.max(np.abs(want))
    print('D=%d N=%d: colsum(G) rel err %.2e of its largest entry' % (D, N, rel))
    assert rel < 1e-11


def test_same_inputs_same_bits():
    """(1040, 3120): twice on one engine and once on a fresh engine -- every sum is in a fixed order."""
    from viabel_amd import _lib
    D, N = SHAPES[1]
    model = _model(D)
    theta = _theta(D, model, 3.0)
    noise = _random_noise(D, N, 31)
    eng = _lib.default_engine()
    v1, g1 = _evaluate_fold(eng, model, theta, D, N, noise)
    v2, g2 = _evaluate_fold(eng, model, theta, D, N, noise)
    fresh = _lib.Engine(eng.device)
    try:
        vf, gf = _evaluate_fold(fresh, model, theta, D, N, noise)
    finally:
        fresh.close()
    assert v2 == v1 and vf == v1
    np.testing.assert_array_equal(g2, g1)
    np.testing.assert_array_equal(gf, g1)


@pytest.mark.parametrize('between', ['larger', 'below_gate'])
def test_nothing_from_before(between):
    """(1088, 3328) and then (1024, 3072) on one engine, or a below-gate evaluation (512, 2048: the sampling product's chain)
    between two fold evaluations: the last result has the bits of a fresh engine's -- the shared workspace, the launch's
    dynamic LDS and the M / S / b / colsum(G) buffers hold nothing that a later evaluation reads."""
    from viabel_amd import _lib
    (D1, N1), (D0, N0) = SHAPES[2], SHAPES[0]
    eng = _lib.default_engine()
    m0 = _model(D0)
    theta, noise = _theta(D0, m0, 3.0), _random_noise(D0, N0, 42)
    if between == 'larger':
        m1 = _model(D1)
        _evaluate_fold(eng, m1, _theta(D1, m1, 3.0), D1, N1, _random_noise(D1, N1, 41))
    else:
        Db, Nb = BELOW_GATE
        mb = _model(Db)
        _evaluate_fold(eng, m0, _theta(D0, m0, 5.0), D0, N0, _random_noise(D0, N0, 43))
        _, launches = _evaluate(eng, mb, _theta(Db, mb, 3.0), Db, Nb, _random_noise(Db, Nb, 44))
        assert launches[0] == 1
    v, g = _evaluate_fold(eng, m0, theta, D0, N0, noise)
    fresh = _lib.Engine(eng.device)
    try:
        vf, gf = _evaluate_fold(fresh, m0, theta, D0, N0, noise)
    finally:
        fresh.close()
    assert v == vf
    np.testing.assert_array_equal(g, gf)
