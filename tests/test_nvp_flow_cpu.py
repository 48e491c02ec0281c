"""NVPFlow on the host (no GPU): the fixtures written from the reference's own code (tests/golden/nvp), the host
methods against them, the constructor's errors, and the torch fp64 oracle of both estimator forms
(tests/_nvp_oracle.py) against the reference's value and finite-difference gradient -- which ties the oracle the GPU
tests use to the reference."""
import glob
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, 'tests')
NVP_DIR = os.path.join(TESTS, 'golden', 'nvp')
sys.path.insert(0, TESTS)

import _golden  # noqa: E402
import viabel_amd as vb  # noqa: E402

PATHS = sorted(glob.glob(os.path.join(NVP_DIR, '*.npz')))
IDS = [os.path.basename(p)[:-4] for p in PATHS]


def load(path):
    return _golden.load(path)


def flow_of(fx):
    D = int(fx['dim'])
    if str(fx['prior_kind']) == 'mf_gaussian':
        prior = vb.MFGaussian(D, seed=int(fx['seed']))
    else:
        prior = vb.MFStudentT(D, float(fx['df']), seed=int(fx['seed']))
    return vb.NVPFlow(fx['layers_t'].tolist(), fx['layers_s'].tolist(), fx['masks'], prior, fx['prior_param'], D)


def model_of(fx):
    D = int(fx['dim'])
    if str(fx['model_kind']) == 'gauss_diag':
        return vb.GaussianModel(fx['model_mean'], fx['model_stdev'])
    return vb.FunnelModel(D, int(fx['model_scale_index']), float(fx['model_log_sigma_stdev']))


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1e-300, np.max(np.abs(b))))


def test_fixtures_match_their_digests():
    assert len(PATHS) == 15
    recorded = _golden.read_digests(os.path.join(NVP_DIR, 'digests.json'))
    assert _golden.fixture_digests(NVP_DIR) == recorded


@pytest.mark.parametrize('path', PATHS, ids=IDS)
def test_host_methods_match_the_reference(path):
    fx = load(path)
    flow = flow_of(fx)
    theta = fx['theta']
    assert flow.var_param_dim == theta.size
    assert np.array_equal(flow.flatten(flow.fold(theta)), theta)
    x = flow.sample(theta, int(fx['n']))
    assert np.max(np.abs(x - fx['sample'])) <= 1e-13 * max(1.0, np.max(np.abs(fx['sample'])))
    lq = flow.log_density(theta, fx['sample'])
    assert np.max(np.abs(lq - fx['log_density'])) <= 1e-13 * max(1.0, np.max(np.abs(fx['log_density'])))
    st = flow.prior._rs.get_state()
    assert np.array_equal(st[1], fx['rs_key_after']) and st[2] == int(fx['rs_pos_after'])


def test_fold_layout():
    D = 4
    flow = vb.NVPFlow([[4, 8], [8, 4]], [[4, 6], [6, 4]], [[1, 0, 1, 0], [0, 1, 0, 1]], vb.MFGaussian(D), np.zeros(8), D)
    theta = np.arange(flow.var_param_dim, dtype=float)
    p = flow.fold(theta)
    assert list(p) == ['0t', '0s', '1t', '1s']
    assert list(p['0t']) == ['0', '0_b', '1', '1_b']
    assert np.array_equal(p['0t']['0'], np.arange(32.0).reshape(4, 8))
    assert np.array_equal(p['0t']['0_b'], np.arange(32.0, 40.0))
    assert p['0s']['0'][0, 0] == 4 * 8 + 8 + 8 * 4 + 4
    assert flow.var_param_dim == 2 * ((4 * 8 + 8 + 8 * 4 + 4) + (4 * 6 + 6 + 6 * 4 + 4))


def test_constructor_errors():
    D = 3
    pr = vb.MFGaussian(D)
    good = dict(layers_t=[[3, 5], [5, 3]], layers_s=[[3, 5], [5, 3]], mask=[[1, 0, 1], [0, 1, 0]], prior=pr,
                prior_param=np.zeros(2 * D), dim=D)
    vb.NVPFlow(**good)

    def bad(exc, **kw):
        with pytest.raises(exc):
            vb.NVPFlow(**dict(good, **kw))
    bad(ValueError, mask=[[1, 0], [0, 1]])
    bad(ValueError, mask=[1, 0, 1])
    bad(ValueError, mask=[[1, 0, 0.5]])
    bad(ValueError, layers_s=[[3, 3]])
    bad(ValueError, layers_t=[[2, 5], [5, 3]])
    bad(ValueError, layers_t=[[3, 5], [5, 2]])
    bad(ValueError, layers_t=[[3, 5], [4, 3]])
    bad(ValueError, prior_param=np.zeros(D))
    bad(NotImplementedError, prior=vb.FullRankGaussian(D))
    bad(NotImplementedError, activation=np.sin)
    vb.NVPFlow(**dict(good, activation='tanh'))
    flow = vb.NVPFlow(**good)
    assert not flow.supports_entropy and not flow.supports_kl and not flow.supports_pth_moment(2)
    from viabel_amd import approximations
    assert 'NVPFlow' in approximations.__all__ and vb.NVPFlow is approximations.NVPFlow


def _oracle():
    import _nvp_oracle
    return _nvp_oracle


@pytest.mark.parametrize('path', PATHS, ids=IDS)
def test_torch_oracle_matches_the_reference(path):
    """The torch oracle of the path form reproduces the reference's value and FD gradient; the plain form has no
    reference value (objectives.py:163 raises), so it is checked against the oracle's own path form plus the
    expectation identity it rests on: both forms share the value, and at N -> infinity the same gradient."""
    O = _oracle()
    fx = load(path)
    flow = flow_of(fx)
    model = model_of(fx)
    v, g = O.objective(flow, model, fx['theta'], fx['z0'], True)
    assert abs(v - fx['value']) <= 1e-12 * max(1.0, abs(fx['value']))
    assert rel(g, fx['grad_fd']) <= 1e-7
    vp, gp = O.objective(flow, model, fx['theta'], fx['z0'], False)
    assert vp == pytest.approx(v, rel=1e-14, abs=1e-14)
    assert np.all(np.isfinite(gp))


def test_plain_form_is_the_total_derivative():
    """The plain form's gradient is the finite-difference gradient of -mean[log p(g(z0)) - log q(g(z0))] with theta
    everywhere (fixed z0)."""
    O = _oracle()
    fx = load(os.path.join(NVP_DIR, 'nvp_d4_funnel_n7.npz'))
    flow, model = flow_of(fx), model_of(fx)
    theta, z0 = fx['theta'], fx['z0']
    _, g = O.objective(flow, model, theta, z0, False)

    def value(th):
        return O.objective(flow, model, th, z0, False)[0]
    idx = np.random.RandomState(0).choice(theta.size, 25, replace=False)
    for i in idx:
        h = 1e-5
        e = np.zeros_like(theta)
        e[i] = h
        fd = (value(theta + e) - value(theta - e)) / (2 * h)
        assert abs(fd - g[i]) <= 1e-7 * max(1.0, np.max(np.abs(g)))
