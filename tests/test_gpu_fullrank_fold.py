"""GPU: the folded full-rank evaluation on the correlated-Gaussian target (vb_fullrank.hip, fr_pipeline_enqueue):
G = -E (L' P) - 1 (P (mu - m))' instead of Z = E L' + mu, G = -(Z - m) P, and sum f from
sum L o tril(G' E) + (mu - m) . colsum(G).  Against the oracle with the project's tolerances (1e-12 relative for the
value, 1e-11 of the largest entry for the gradient), which route ran (the sampling product's launch count), that
M = L' P follows the parameter, determinism, and the sharded code path."""
import numpy as np
import pytest

from oracle import families as ofam
from oracle import models as omod
from oracle import objectives as oobj

pytestmark = pytest.mark.gpu


def _gate():
    from viabel_amd import _lib
    d0 = _lib.FR_FOLD_MIN_D
    n0 = -(-d0 * _lib.FR_FOLD_MIN_ROWS_PER_D // 128) * 128
    return d0, n0


def _problem(D, seed=3):
    """As tests/test_gpu_fused.py::_problem: mu != m, a random strict lower triangle, a non-constant diagonal."""
    import viabel_amd as vb
    rng = np.random.RandomState(seed)
    A = rng.randn(D, D)
    S = A @ A.T / D + np.eye(D)
    mean = rng.randn(D)
    model = vb.CorrelatedGaussianModel(mean, covariance=S)
    approx = vb.FullRankGaussian(D, seed=2)
    L = np.tril(0.05 * rng.randn(D, D), -1) + np.diag(np.exp(-1.0 + 0.1 * rng.randn(D)))
    theta = approx.pack(0.2 * rng.randn(D), L)
    return vb, model, theta


def _theta_b(vb, D):
    rng = np.random.RandomState(9)
    L = np.tril(0.1 * rng.randn(D, D), -1) + np.diag(np.exp(-0.3 + 0.2 * rng.randn(D)))
    return vb.FullRankGaussian(D).pack(1.5 * rng.randn(D), L)


def _evaluate(eng, model, theta, D, N, slot=3, stream=1, flags=0):
    """(value, grad), launches of the sampling product, the noise."""
    from viabel_amd import _lib
    eng.set_model(model.device_spec())
    eng.noise_generate(slot, N, D, seed=5, stream=stream)
    eng.fullrank_set_theta(theta, D)
    eng.profile_enable(True)
    try:
        eng.profile_read(reset=True, kernel=_lib.PROF_FR_SAMPLE_GEMM)
        eng.elbo_grad_fullrank_enqueue(slot, N, D, flags=flags)
        out = eng.fullrank_get(D)
        launches = eng.profile_read(reset=True, kernel=_lib.PROF_FR_SAMPLE_GEMM)[0]
    finally:
        eng.profile_enable(False)
    return out, launches, eng.noise_get_host(slot, N, D)


def _check_oracle(out, model, theta, noise, D, use_path_deriv=False, omodel=None):
    v, g = out
    if omodel is None:
        omodel = omod.GaussFull(model.mean, model.precision)
    ov, og = oobj.exclusive_kl(ofam.FullRankGaussian(D), omodel, theta, noise, use_path_deriv=use_path_deriv)
    rel_v = abs(v - ov) / abs(ov)
    rel_g = np.max(np.abs(g - og)) / np.max(np.abs(og))
    print('D=%d N=%d: rel err value %.2e, gradient %.2e of its largest entry' % (D, noise.shape[0], rel_v, rel_g))
    assert rel_v < 1e-12
    assert rel_g < 1e-11


def _shapes():
    d0, n0 = _gate()
    return [(d0, n0), (d0 + 16, n0 + 48)]


@pytest.mark.parametrize('which', [0, 1])
def test_folded_evaluation_matches_the_oracle_without_a_sampling_product(which):
    """(D0, N0) at the gate, and (D0 + 16, N0 + 48): D no multiple of 64, N none of 128 -- ragged tiles in the M product,
    in its k-range clamp and in the bias."""
    from viabel_amd import _lib
    D, N = _shapes()[which]
    vb, model, theta = _problem(D)
    out, launches, noise = _evaluate(_lib.default_engine(), model, theta, D, N)
    assert launches == 0
    _check_oracle(out, model, theta, noise, D)


def test_below_the_gate_the_sampling_product_runs():
    from viabel_amd import _lib
    D, n0 = _gate()
    N = n0 - 128
    vb, model, theta = _problem(D)
    out, launches, noise = _evaluate(_lib.default_engine(), model, theta, D, N)
    assert launches == 1
    _check_oracle(out, model, theta, noise, D)
    D = D - 64
    vb, model, theta = _problem(D)
    out, launches, noise = _evaluate(_lib.default_engine(), model, theta, D, n0)
    assert launches == 1
    _check_oracle(out, model, theta, noise, D)


def _objective_call(objective, theta):
    """One call of a viabel_amd objective on the default engine: (value, grad), launches of the sampling product."""
    from viabel_amd import _lib
    eng = _lib.default_engine()
    eng.profile_enable(True)
    try:
        eng.profile_read(reset=True, kernel=_lib.PROF_FR_SAMPLE_GEMM)
        out = objective(theta)
        launches = eng.profile_read(reset=True, kernel=_lib.PROF_FR_SAMPLE_GEMM)[0]
    finally:
        eng.profile_enable(False)
    return out, launches


def test_path_derivative_keeps_the_sampling_product():
    """pd changes G between the products: not folded, at a shape that folds without it."""
    D, N = _gate()
    vb, model, theta = _problem(D)
    approx = vb.FullRankGaussian(D, seed=2)
    out, launches = _objective_call(vb.ExclusiveKL(approx, model, N, use_path_deriv=True), theta)
    assert launches == 1
    noise = np.random.RandomState(2).randn(N, D)
    _check_oracle(out, model, theta, noise, D, use_path_deriv=True)


def test_funnel_target_keeps_the_sampling_product():
    D, N = _gate()
    vb, _, theta = _problem(D)
    approx = vb.FullRankGaussian(D, seed=2)
    out, launches = _objective_call(vb.ExclusiveKL(approx, vb.FunnelModel(D), N), theta)
    assert launches == 1
    noise = np.random.RandomState(2).randn(N, D)
    _check_oracle(out, None, theta, noise, D, omodel=omod.Funnel(D))


def _fresh(device, model, theta, D, N, stream, seed=5):
    """The evaluation at `theta` by an engine that has never seen another parameter."""
    from viabel_amd import _lib
    eng = _lib.Engine(device)
    try:
        eng.set_model(model.device_spec())
        eng.noise_generate(3, N, D, seed=seed, stream=stream)
        eng.fullrank_set_theta(theta, D)
        eng.elbo_grad_fullrank_enqueue(3, N, D)
        return eng.fullrank_get(D)
    finally:
        eng.close()


def test_m_follows_the_parameter_and_results_are_deterministic():
    """theta_a, then theta_b through fullrank_set_theta in the same buffers, then two iterations of vb_fit (the second
    at the stepped parameter): each the same bits as a fresh engine's evaluation there -- an M = L' P kept from an
    earlier parameter fails this.  And the same inputs twice give the same bits."""
    from viabel_amd import _lib
    D, N = _gate()
    vb, model, theta_a = _problem(D)
    theta_b = _theta_b(vb, D)
    eng = _lib.default_engine()
    eng.set_model(model.device_spec())
    eng.noise_generate(3, N, D, seed=5, stream=1)
    got = []
    for th in (theta_a, theta_a, theta_b):
        eng.fullrank_set_theta(th, D)
        eng.elbo_grad_fullrank_enqueue(3, N, D)
        got.append(eng.fullrank_get(D))
    assert got[1][0] == got[0][0]
    np.testing.assert_array_equal(got[1][1], got[0][1])
    for th, (v, g) in ((theta_a, got[0]), (theta_b, got[2])):
        fv, fg = _fresh(eng.device, model, th, D, N, stream=1)
        assert v == fv
        np.testing.assert_array_equal(g, fg)
    assert got[2][0] != got[0][0]

    _, values, history, _, _, grads = eng.fit(4, N, D, _lib.FAMILY_FULLRANK_GAUSSIAN, theta_b, 2, _lib.OPT_RMSPROP,
                                              [0.01, 0.9, 0.9, 1e-8], seed=7, first_stream=11, hist_len=2,
                                              log_gradients=True)
    assert not np.array_equal(history[0], theta_b)
    for k, th in enumerate((theta_b, history[0])):
        fv, fg = _fresh(eng.device, model, th, D, N, stream=11 + k, seed=7)
        assert values[k] == fv
        np.testing.assert_array_equal(grads[k], fg)


def test_one_rank_communicator():
    """The sharded code path (raw sums -> all-reduce -> epilogue kernel): the gradient's sums are formed in the same
    order, the value's scalar sums are not (4e-15 relative, as tests/test_gpu_fused.py allows for that)."""
    from viabel_amd import _lib
    D, N = _gate()
    vb, model, theta = _problem(D)
    plain = _lib.default_engine()
    (v0, g0), launches, _ = _evaluate(plain, model, theta, D, N)
    assert launches == 0
    comm = _lib.Engine(plain.device)
    try:
        comm.comm_init(_lib.Engine.comm_unique_id(), 1, 0)
        (v1, g1), launches, _ = _evaluate(comm, model, theta, D, N)
        comm.comm_destroy()
    finally:
        comm.close()
    assert launches == 0
    np.testing.assert_array_equal(g1, g0)
    assert abs(v1 - v0) <= 4e-15 * abs(v0)
