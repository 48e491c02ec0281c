"""NVPFlow under ExclusiveKL on the device (vb_flow.hip) against a literal torch fp64 autograd oracle
(tests/_nvp_oracle.py): both estimator forms, both priors, numpy and Philox noise, every kind of target; the
device diagnostics route; a fit; a two-rank job; the unsupported combinations."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, 'tests')
sys.path.insert(0, TESTS)

import _nvp_oracle as O  # noqa: E402
import viabel_amd as vb  # noqa: E402

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


def half_masks(D, K):
    return np.array([[(j + i) % 2 for j in range(D)] for i in range(K)], dtype=float)


def net(D, widths):
    dims = [D] + list(widths) + [D]
    return [[a, b] for a, b in zip(dims[:-1], dims[1:])]


def make_flow(D, K, hid_t, hid_s, prior_kind, rng, seed=3, prior_scale=0.0):
    prior = vb.MFGaussian(D, seed=seed, rng=rng) if prior_kind == 'gauss' else vb.MFStudentT(D, 5.0, seed=seed, rng=rng)
    r = np.random.RandomState(D + K)
    prior_param = np.concatenate([prior_scale * r.randn(D), prior_scale * r.randn(D)])
    return vb.NVPFlow(net(D, hid_t), net(D, hid_s), half_masks(D, K), prior, prior_param, D)


def make_model(kind, D):
    r = np.random.RandomState(11 + D)
    mean, sd = 0.3 * r.randn(D), np.exp(0.2 * r.randn(D))
    if kind == 'gauss':
        return vb.GaussianModel(mean, sd)
    if kind == 'funnel':
        return vb.FunnelModel(D) if D >= 2 else vb.GaussianModel(mean, sd)
    if kind == 'corr':
        A = r.randn(D, D)
        return vb.CorrelatedGaussianModel(mean, covariance=A @ A.T / D + np.eye(D))
    if kind == 'source':
        m = vb.SourceModel(D, GAUSS_SRC, np.concatenate([mean, sd]))
    elif kind == 'callable':
        def f(x):
            return np.sum(-0.5 * ((x - mean) / sd) ** 2, axis=1)

        def gr(x):
            return -(x - mean) / sd ** 2
        m = vb.CallableModel(D, f, gr)
    else:
        raise ValueError(kind)
    import torch
    tm, ts = torch.from_numpy(mean), torch.from_numpy(sd)
    m._torch_logp = lambda x: torch.sum(-0.5 * ((x - tm) / ts) ** 2, dim=1)
    return m


def prior_draws(flow_twin, n):
    """The prior draws the objective's first call consumes: the same draw from an identical, fresh prior."""
    p = flow_twin.prior
    if p.rng == 'philox':
        from viabel_amd.approximations import _philox_host_copy
        eps = _philox_host_copy(p, n, None)
    else:
        eps = p._base_noise(n)
    D = p.dim
    return flow_twin.prior_param[:D] + np.exp(flow_twin.prior_param[D:]) * eps


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1e-300, np.max(np.abs(b))))


def check_case(D, K, hid_t, hid_s, prior_kind, rng, model_kind, N, path, theta_scale=0.1, prior_scale=0.1):
    flow = make_flow(D, K, hid_t, hid_s, prior_kind, rng, prior_scale=prior_scale)
    twin = make_flow(D, K, hid_t, hid_s, prior_kind, rng, prior_scale=prior_scale)
    model = make_model(model_kind, D)
    theta = theta_scale * np.random.RandomState(D * 7 + K + N).randn(flow.var_param_dim)
    value, grad = vb.ExclusiveKL(flow, model, N, use_path_deriv=path)(theta)
    z0 = prior_draws(twin, N)
    ov, og = O.objective(twin, model, theta, z0, path)
    assert abs(value - ov) <= 1e-12 * max(1.0, abs(ov)), (value, ov)
    assert rel(grad, og) <= 1e-10, rel(grad, og)
    return flow, theta, grad


SWEEP = [
    # D, K, t hidden, s hidden, prior, rng, model, N, path
    (2, 1, [10], [10], 'gauss', 'numpy', 'gauss', 1, True),
    (2, 2, [33, 10], [10, 33], 'student', 'philox', 'funnel', 100, False),
    (17, 6, [33], [10], 'gauss', 'numpy', 'corr', 100, True),
    (17, 2, [], [], 'student', 'numpy', 'source', 4097, False),
    (64, 1, [256], [256], 'gauss', 'philox', 'callable', 100, True),
    (64, 6, [10, 10], [33, 256], 'student', 'philox', 'gauss', 4097, True),
    (256, 2, [256], [33], 'gauss', 'numpy', 'funnel', 100, False),
    (256, 1, [10, 256], [256, 10], 'student', 'philox', 'corr', 1, False),
    (2, 6, [256, 33], [33, 256], 'gauss', 'philox', 'source', 4097, True),
    (17, 1, [10], [33], 'gauss', 'philox', 'callable', 1, False),
]


@pytest.mark.parametrize('case', SWEEP, ids=lambda c: 'D%d_K%d_%s_%s_%s_N%d_%s' % (c[0], c[1], c[4], c[5], c[6], c[7],
                                                                                 'pd' if c[8] else 'plain'))
def test_flow_matches_torch_oracle(case):
    check_case(*case)


@pytest.mark.parametrize('path', [False, True])
@pytest.mark.parametrize('rng', ['numpy', 'philox'])
def test_nvp_config_full_size(path, rng):
    """The measured configuration: D = 256, K = 4 half masks, nets [[256, 256], [256, 256]], N = 4096."""
    check_case(256, 4, [256], [256], 'gauss', rng, 'corr', 4096, path, theta_scale=0.03, prior_scale=0.0)


def test_masked_rows_are_zero_and_calls_reproduce():
    D, K = 17, 2
    flow = make_flow(D, K, [33], [10], 'gauss', 'philox')
    theta = 0.1 * np.random.RandomState(0).randn(flow.var_param_dim)
    obj = vb.ExclusiveKL(flow, make_model('funnel', D), 1000)
    flow.prior._philox_calls = 0
    v1, g1 = obj(theta)
    flow.prior._philox_calls = 0
    v2, g2 = obj(theta)
    assert v1 == v2 and np.array_equal(g1, g2)
    p = flow.fold(g1)
    for i in range(K):
        masked = flow.mask[i] == 0
        for net in 't', 's':
            W0 = p[str(i) + net]['0']
            assert np.all(W0[masked] == 0.0)
            assert np.any(W0[~masked] != 0.0)


def test_host_and_device_log_weights_agree_and_diagnostics_run():
    from viabel_amd.convenience import samples_and_log_weights
    D = 4
    model = make_model('gauss', D)
    for rng in ('numpy', 'philox'):
        a = make_flow(D, 4, [8, 8], [6, 5], 'student', rng, prior_scale=0.1)
        b = make_flow(D, 4, [8, 8], [6, 5], 'student', rng, prior_scale=0.1)
        theta = 0.1 * np.random.RandomState(1).randn(a.var_param_dim)
        xs, lw = samples_and_log_weights(theta, model, a, 3000)
        xh = b.sample(theta, 3000)
        lwh = model(xh) - b.log_density(theta, xh)
        assert rel(xs, xh) <= 1e-11 and rel(lw, lwh) <= 1e-11
        assert np.array_equal(a.prior._rs.randn(3), b.prior._rs.randn(3))
    flow = make_flow(D, 4, [8], [8], 'gauss', 'numpy')
    flow.mc_samples = 2000
    res = vb.vi_diagnostics(0.05 * np.random.RandomState(2).randn(flow.var_param_dim), model=model, approx=flow,
                            n_samples=5000)
    assert np.isfinite(res['khat'])


def test_bbvi_fits_a_gaussian():
    D = 4
    m, s = np.array([1.0, -1.0, 0.5, 2.0]), np.array([0.5, 1.5, 1.0, 2.0])
    flow = vb.NVPFlow(net(D, [16]), net(D, [16]), half_masks(D, 4), vb.MFGaussian(D, seed=4), np.zeros(2 * D), D)
    init = 0.01 * np.random.RandomState(5).randn(flow.var_param_dim)

    def errors(theta):
        x = flow.sample(theta, 20000)
        return np.max(np.abs(x.mean(0) - m)), np.max(np.abs(x.std(0) - s))
    mean_thr, sd_thr = 0.5, 0.3
    e0 = errors(init)
    assert e0[0] > mean_thr and e0[1] > sd_thr, e0
    res = vb.bbvi(D, log_density=vb.GaussianModel(m, s), approx=flow, init_var_param=init, n_iters=3000,
                  num_mc_samples=50, adaptive=False, fixed_lr=True, learning_rate=0.01)
    e1 = errors(res['opt_param'])
    assert e1[0] < mean_thr / 2 and e1[1] < sd_thr / 2, e1


def test_unsupported_combinations_raise():
    D = 3
    flow = make_flow(D, 2, [10], [10], 'gauss', 'numpy')
    model = make_model('gauss', D)
    with pytest.raises(NotImplementedError, match='NVPFlow'):
        vb.ExclusiveKL(flow, model, 10, hessian_approx_method='full')
    with pytest.raises(NotImplementedError, match='NVPFlow'):
        vb.ExclusiveKL(flow, model, 10)._hessian_vector_product(np.zeros(flow.var_param_dim), np.ones(flow.var_param_dim))
    with pytest.raises(NotImplementedError):
        vb.DISInclusiveKL(flow, model, 10, 0.5, vb.MFGaussian(D), np.zeros(2 * D))
    with pytest.raises(NotImplementedError):
        vb.AlphaDivergence(flow, model, 10, 0.5)
    assert not vb.ExclusiveKL(flow, model, 10).supports_device_fit()


WORKER = r'''
import os, sys
sys.path.insert(0, %(root)r)
import numpy as np
from viabel_amd import _lib, distributed
import viabel_amd as vb
eng = _lib.Engine(0)
_lib.set_default_engine(eng)
group = distributed.SocketGroup.from_env(timeout=120.0)
distributed.attach(eng, group, transport='host')
D = 17
masks = np.array([[(j + i) %% 2 for j in range(D)] for i in range(3)], dtype=float)
flow = vb.NVPFlow([[D, 33], [33, D]], [[D, 10], [10, D]], masks, vb.MFStudentT(D, 5.0, seed=9, rng='philox'),
                  np.zeros(2 * D), D)
theta = 0.1 * np.random.RandomState(0).randn(flow.var_param_dim)
model = vb.FunnelModel(D)
out = {}
for path in (False, True):
    out['v%%d' %% path], out['g%%d' %% path] = vb.ExclusiveKL(flow, model, 1001, use_path_deriv=path)(theta)
np.savez(os.path.join(%(out)r, 'rank%%d.npz' %% group.rank), **out)
group.barrier()
group.close()
print('{"rank": %%d, "done": true}' %% group.rank)
'''


def test_two_ranks_match_one(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    script = tmp_path / 'worker.py'
    script.write_text(WORKER % {'root': ROOT, 'out': str(tmp_path)})
    rc, lines = bench.spawn_ranks(2, [sys.executable, str(script)], timeout_s=600)
    assert rc == 0, lines[-5:]
    D = 17
    flow = vb.NVPFlow(net(D, [33]), net(D, [10]), half_masks(D, 3), vb.MFStudentT(D, 5.0, seed=9, rng='philox'),
                      np.zeros(2 * D), D)
    theta = 0.1 * np.random.RandomState(0).randn(flow.var_param_dim)
    for r in (0, 1):
        got = np.load(tmp_path / ('rank%d.npz' % r))
        fresh = vb.NVPFlow(net(D, [33]), net(D, [10]), half_masks(D, 3), vb.MFStudentT(D, 5.0, seed=9, rng='philox'),
                           np.zeros(2 * D), D)
        for path in (False, True):
            v, g = vb.ExclusiveKL(fresh, vb.FunnelModel(D), 1001, use_path_deriv=path)(theta)
            assert abs(got['v%d' % path] - v) <= 1e-12 * abs(v)
            assert rel(got['g%d' % path], g) <= 1e-12
    del flow


NVP_DIR = os.path.join(TESTS, 'golden', 'nvp')
FIXTURES = sorted(p for p in os.listdir(NVP_DIR) if p.endswith('.npz'))


@pytest.mark.parametrize('name', FIXTURES, ids=[p[:-4] for p in FIXTURES])
def test_reference_fixtures_on_the_device(name):
    """The reference's own path-form value (numpy noise), the torch gradient, the prior generator's state after."""
    import _golden
    fx = _golden.load(os.path.join(NVP_DIR, name))
    D = int(fx['dim'])

    def flow():
        prior = (vb.MFGaussian(D, seed=int(fx['seed'])) if str(fx['prior_kind']) == 'mf_gaussian'
                 else vb.MFStudentT(D, float(fx['df']), seed=int(fx['seed'])))
        return vb.NVPFlow(fx['layers_t'].tolist(), fx['layers_s'].tolist(), fx['masks'], prior, fx['prior_param'], D)
    model = (vb.GaussianModel(fx['model_mean'], fx['model_stdev']) if str(fx['model_kind']) == 'gauss_diag'
             else vb.FunnelModel(D, int(fx['model_scale_index']), float(fx['model_log_sigma_stdev'])))
    for path in (True, False):
        f = flow()
        value, grad = vb.ExclusiveKL(f, model, int(fx['n']), use_path_deriv=path)(fx['theta'])
        st = f.prior._rs.get_state()
        assert np.array_equal(st[1], fx['rs_key_after']) and st[2] == int(fx['rs_pos_after'])
        ov, og = O.objective(f, model, fx['theta'], fx['z0'], path)
        assert abs(value - fx['value']) <= 1e-12 * max(1.0, abs(fx['value']))
        assert rel(grad, og) <= 1e-10
