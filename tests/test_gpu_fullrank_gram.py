"""GPU: the folded full-rank evaluation forms its sums from the noise's Gram matrix (vb_fullrank.hip, fr_route):
with M = L' P, b = P (mu - m), S = E' E, s = colsum(E) and n rows,  G' E = -M' S - b s'  and  colsum(G) = -s' M - n b'
-- no N x D x D product, G is never stored.  At the smallest shapes at which the route runs (the gate shape of `_lib` and
its ragged neighbour), against `oracle.objectives.exclusive_kl` with the project's tolerances (value 1e-12 relative,
gradient 1e-11 of its largest entry): which route ran, the rank-one terms b s' and n b', that S follows the noise, the
mirrored half of S and ragged edges, and that the sums of two shards add up."""
import functools

import numpy as np
import pytest

from oracle import families as ofam
from oracle import models as omod
from oracle import objectives as oobj

pytestmark = pytest.mark.gpu

SLOT = 3


def _gate():
    from viabel_amd import _lib
    d0 = _lib.FR_FOLD_MIN_D
    n0 = -(-d0 * _lib.FR_FOLD_MIN_ROWS_PER_D // 128) * 128
    return d0, n0


@functools.lru_cache(maxsize=None)
def _model(D):
    import viabel_amd as vb
    rng = np.random.RandomState(3)
    A = rng.randn(D, D)
    cov = A @ A.T / D + np.eye(D)
    return vb.CorrelatedGaussianModel(rng.randn(D), covariance=cov)


def _theta(D, model, mu_offset, seed=4, tri=0.05):
    """mu = m + mu_offset * (random signs and sizes in [0.5, 1.5]); a dense strict lower triangle of scale `tri`."""
    import viabel_amd as vb
    rng = np.random.RandomState(seed)
    L = np.tril(tri * rng.randn(D, D), -1) + np.diag(np.exp(-1.0 + 0.1 * rng.randn(D)))
    mu = model.mean + mu_offset * rng.choice([-1.0, 1.0], D) * (0.5 + rng.rand(D))
    return vb.FullRankGaussian(D).pack(mu, L)


def _shifted_noise(N, D, seed):
    """Column means far from zero: s = colsum(E) is of the order of n, one column pulls the other way."""
    noise = np.random.RandomState(seed).randn(N, D) + 0.5
    noise[:, D // 3] -= 2.0
    return noise


def _evaluate(eng, model, theta, D, n, n_total=None, noise=None, seed=5):
    """(value, grad) of rows [0, n) of slot SLOT (uploaded first when `noise` is given, else generated), and the launch
    counts of the sampling, model and gradient products."""
    from viabel_amd import _lib
    eng.set_model(model.device_spec())
    if noise is not None:
        eng.noise_set_host(SLOT, noise)
    else:
        eng.noise_generate(SLOT, n, D, seed=seed, stream=1)
    eng.fullrank_set_theta(theta, D)
    kernels = (_lib.PROF_FR_SAMPLE_GEMM, _lib.PROF_FR_MODEL_GEMM, _lib.PROF_FR_GRAD_GEMM)
    eng.profile_enable(True)
    try:
        for k in kernels:
            eng.profile_read(reset=True, kernel=k)
        eng.elbo_grad_fullrank_enqueue(SLOT, n, D, n_total=n_total)
        out = eng.fullrank_get(D)
        launches = tuple(eng.profile_read(reset=True, kernel=k)[0] for k in kernels)
    finally:
        eng.profile_enable(False)
    return out, launches


def _check_oracle(out, model, theta, noise, D):
    v, g = out
    ov, og = oobj.exclusive_kl(ofam.FullRankGaussian(D), omod.GaussFull(model.mean, model.precision), theta, noise)
    rel_v = abs(v - ov) / abs(ov)
    rel_g = np.max(np.abs(g - og)) / np.max(np.abs(og))
    print('D=%d N=%d: rel err value %.2e, gradient %.2e of its largest entry' % (D, noise.shape[0], rel_v, rel_g))
    assert rel_v < 1e-12
    assert rel_g < 1e-11


def test_which_route_ran():
    """Above the gate: no sampling and no model product, one launch timed as the gradient product (the Gram product of
    the noise).  Below it (N0 - 128): the model product runs."""
    from viabel_amd import _lib
    D, N = _gate()
    model = _model(D)
    theta = _theta(D, model, 0.2)
    eng = _lib.default_engine()
    _, launches = _evaluate(eng, model, theta, D, N)
    assert launches == (0, 0, 1)
    _, launches = _evaluate(eng, model, theta, D, N - 128)
    assert launches[1] == 1


@pytest.mark.parametrize('mu_offset', [10.0, 0.0])
def test_rank_one_terms(mu_offset):
    """|mu - m| of order 10 and column means of the noise of order 1: b s' and n b' dominate C and colsum(G), so a
    dropped, doubled or mis-signed term misses the bound by orders of magnitude.  And mu = m exactly: b = 0."""
    from viabel_amd import _lib
    D, N = _gate()
    model = _model(D)
    theta = _theta(D, model, mu_offset)
    if mu_offset == 0.0:
        assert np.array_equal(theta[:D], model.mean)
    noise = _shifted_noise(N, D, seed=11)
    out, launches = _evaluate(_lib.default_engine(), model, theta, D, N, noise=noise)
    assert launches == (0, 0, 1)
    _check_oracle(out, model, theta, noise, D)


def test_gram_matrix_follows_the_noise():
    """Noise A, then noise B in the same slot at the same shape: the second result has the bits of a fresh engine's
    evaluation of B -- a Gram matrix (or column sums) kept from A fails this -- and differs from the first."""
    from viabel_amd import _lib
    D, N = _gate()
    model = _model(D)
    theta = _theta(D, model, 1.0)
    noise_a, noise_b = _shifted_noise(N, D, seed=21), _shifted_noise(N, D, seed=22)
    eng = _lib.default_engine()
    (va, ga), _ = _evaluate(eng, model, theta, D, N, noise=noise_a)
    (vb_, gb), launches = _evaluate(eng, model, theta, D, N, noise=noise_b)
    assert launches == (0, 0, 1)
    fresh = _lib.Engine(eng.device)
    try:
        (vf, gf), _ = _evaluate(fresh, model, theta, D, N, noise=noise_b)
    finally:
        fresh.close()
    assert vb_ == vf
    np.testing.assert_array_equal(gb, gf)
    assert vb_ != va
    assert not np.array_equal(gb, ga)
    # ... and through the generator with another seed
    (vc, gc), _ = _evaluate(eng, model, theta, D, N, seed=6)
    (vd, gd), _ = _evaluate(eng, model, theta, D, N, seed=7)
    assert vd != vc and not np.array_equal(gd, gc)
    _check_oracle((vd, gd), model, theta, eng.noise_get_host(SLOT, N, D), D)


def test_symmetry_and_ragged_edges():
    """(D0 + 16, N0 + 48): D no multiple of 32, 64 or 128, N none of 128.  The strict lower triangle of L is dense and of
    the diagonal's size down to the last row, so M = L' P is dense in every row and the mirrored half of S and the last
    slab of the K axis enter the gradient at full weight."""
    from viabel_amd import _lib
    d0, n0 = _gate()
    D, N = d0 + 16, n0 + 48
    model = _model(D)
    theta = _theta(D, model, 3.0, seed=8, tri=0.3)
    noise = _shifted_noise(N, D, seed=31)
    out, launches = _evaluate(_lib.default_engine(), model, theta, D, N, noise=noise)
    assert launches == (0, 0, 1)
    _check_oracle(out, model, theta, noise, D)


def test_two_shards_add_up():
    """Rows [0, n1) and [n1, N) of one noise matrix as two evaluations with n_total = N on ONE engine without a
    communicator (the raw sums are reached through the results, which are linear in them: the second shard is uploaded
    as a slot of its own, an evaluation reads a slot from its first row).  Each result is
      value = -(F_k / N + c0 + H),  d/dmu = -colsum_k / N,  d/dL = -tril(C_k) / N  (free diagonal: x L_ii, then - 1)
    so the shards' gradients add up to the whole's but for one entropy term on the diagonal, and the values but for one
    c0 + H.  n1 is a multiple of 128, the parts are uneven and both above the gate: `n` of colsum(G) = -s' M - n b' is
    the shard's own row count, not n_total."""
    from viabel_amd import _lib
    D, n0 = _gate()
    n1, N = n0, 2 * n0 + 128
    model = _model(D)
    theta = _theta(D, model, 10.0)
    noise = _shifted_noise(N, D, seed=41)
    eng = _lib.default_engine()
    (v1, g1), l1 = _evaluate(eng, model, theta, D, n1, n_total=N, noise=noise[:n1])
    (v2, g2), l2 = _evaluate(eng, model, theta, D, N - n1, n_total=N, noise=noise[n1:])
    assert l1 == (0, 0, 1) and l2 == (0, 0, 1)
    diag = D + np.arange(D) * (np.arange(D) + 1) // 2 + np.arange(D)      # the free diagonal in the flat layout
    g = g1 + g2
    g[diag] += 1.0
    c0 = 0.5 * model.logdet_precision - 0.5 * D * np.log(2.0 * np.pi)
    H = 0.5 * D * (1.0 + np.log(2.0 * np.pi)) + np.sum(theta[diag])
    v = v1 + v2 + (c0 + H)
    _check_oracle((v, g), model, theta, noise, D)
