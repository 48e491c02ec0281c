"""GPU: small results and parameters through mapped memory + a polled completion word (fetch_blocking / push_small,
vb_api.hip) against the plain copies + stream synchronisation they replace (VB_FETCH_FLAGSYNC=0): the same numbers through
another door -- bit-identical -- on every family of blocking entry points that uses them."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def env():
    import viabel_amd as vb
    from viabel_amd import _lib
    return vb, _lib.default_engine(), _lib


def _both(call):
    old = os.environ.get('VB_FETCH_FLAGSYNC')
    try:
        os.environ['VB_FETCH_FLAGSYNC'] = '0'
        plain = call()
        os.environ['VB_FETCH_FLAGSYNC'] = '1'
        flagged = call()
    finally:
        if old is None:
            os.environ.pop('VB_FETCH_FLAGSYNC', None)
        else:
            os.environ['VB_FETCH_FLAGSYNC'] = old
    return plain, flagged


def _same(a, b):
    if isinstance(a, (tuple, list)):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            _same(x, y)
    elif isinstance(a, np.ndarray):
        np.testing.assert_array_equal(a, b)
    else:
        assert a == b or (a != a and b != b)


@pytest.mark.parametrize('d,n', [(3, 17), (64, 1000), (300, 513)])
def test_fullrank_blocking_call(env, d, n):
    vb, eng, _lib = env
    rng = np.random.RandomState(d)
    A = rng.randn(d, d)
    model = vb.CorrelatedGaussianModel(rng.randn(d), covariance=A @ A.T / d + np.eye(d))
    fam = vb.FullRankGaussian(d)
    theta = fam.pack(0.1 * rng.randn(d), np.exp(-1.0) * np.eye(d) + 0.01 * np.tril(rng.randn(d, d)))

    def call():
        eng.set_model(model.device_spec())
        eng.noise_generate(5, n, d, seed=3, stream=1)
        return eng.elbo_grad_fullrank(5, n, d, theta)
    _same(*_both(call))


@pytest.mark.parametrize('k', [4, 32])
def test_lowrank_blocking_calls(env, k):
    vb, eng, _lib = env
    D, N = 200, 1000
    rng = np.random.RandomState(k)
    fam = vb.LRGaussian(D, k=k)
    theta = fam.pack(0.1 * rng.randn(D), -np.ones(D), 0.05 * rng.randn(D, k))

    def call():
        eng.set_model(vb.FunnelModel(D).device_spec())
        eng.noise_generate(0, N, D, seed=1, stream=0)
        eng.noise_generate(1, N, k, seed=2, stream=0)
        return (eng.elbo_sums_lowrank(0, 1, N, D, k, theta) if k > 16 else eng.elbo_grad_lowrank(0, 1, N, D, k, theta))
    _same(*_both(call))


def test_psis_and_dis_and_t_family(env):
    vb, eng, _lib = env
    from viabel_amd._psis import psislw
    rng = np.random.RandomState(1)
    lw = 2.0 * rng.standard_t(3.0, 5000)
    _same(*_both(lambda: psislw(lw)))
    D, N = 40, 2048

    def dis():
        r = np.random.RandomState(7)
        model = vb.GaussianModel(0.3 + 0.3 * r.randn(D), np.exp(0.2 * r.randn(D)))
        prior = np.zeros(2 * D)
        obj = vb.DISInclusiveKL(vb.MFGaussian(D, seed=11, rng='philox'), model, N, ess_target=N // 8, temper_prior=vb.MFGaussian(D),
                                temper_prior_params=prior, use_resampling=False)
        v, g = obj(prior + 0.02 * r.randn(2 * D))
        return v, g, obj._eps, obj._ess
    _same(*_both(dis))

    def mvt():
        r = np.random.RandomState(9)
        approx = vb.MultivariateT(D, 30.0, seed=4, rng='philox')
        model = vb.GaussianModel(0.2 * r.randn(D), np.exp(0.1 * r.randn(D)))
        theta = approx.init_param() * 0.3
        v1, g1 = vb.ExclusiveKL(approx, model, N)(theta)
        np.random.seed(3)
        v2, g2 = vb.AlphaDivergence(vb.MultivariateT(D, 30.0, seed=4, rng='philox'), model, N, 0.5)(theta)
        return v1, g1, v2, g2
    _same(*_both(mvt))


# ---- the blocking full-rank call above 1 MB of parameter (plain copies instead of the mapped staging) ------------------
@pytest.mark.parametrize('d,n', [(1024, 4096), (512, 4096), (1008, 1000), (576, 257), (2048, 512)])
@pytest.mark.parametrize('target', ['gauss_full', 'funnel', 'gauss_diag'])
def test_fullrank_blocking_large_parameter_is_the_resident_evaluation(env, d, n, target):
    """vb_elbo_grad_fullrank above 1 MB of parameter against the resident route (vb_fullrank_set_theta + enqueue + get) on
    the same noise: the same evaluation, so value and gradient are bit-identical -- back to back with changing
    parameters, targets whose first product has a reducing epilogue (gauss_diag) and shards too short for the plain
    product (k-split) included."""
    vb, eng, _lib = env
    rng = np.random.RandomState(d + n)
    if target == 'gauss_full':
        A = rng.randn(d, d)
        model = vb.CorrelatedGaussianModel(rng.randn(d), covariance=A @ A.T / d + np.eye(d))
    elif target == 'funnel':
        model = vb.FunnelModel(d, d // 3)
    else:
        model = vb.GaussianModel(rng.randn(d), np.exp(0.1 * rng.randn(d)))
    fam = vb.FullRankGaussian(d)
    thetas = [fam.pack(0.1 * rng.randn(d), np.exp(-1.0) * np.eye(d) + 0.01 * np.tril(rng.randn(d, d))) for _ in range(3)]

    def blocking():
        eng.set_model(model.device_spec())
        out = []
        for k, theta in enumerate(thetas):
            eng.noise_generate(5, n, d, seed=3, stream=k)
            out.append(eng.elbo_grad_fullrank(5, n, d, theta))
        return out

    def resident():
        eng.set_model(model.device_spec())
        out = []
        for k, theta in enumerate(thetas):
            eng.noise_generate(5, n, d, seed=3, stream=k)
            eng.fullrank_set_theta(theta, d)
            eng.elbo_grad_fullrank_enqueue(5, n, d)
            out.append(eng.fullrank_get(d))
        return out
    _same(blocking(), resident())


def test_fullrank_new_parameter_stays_behind_asynchronous_evaluations(env):
    """A new parameter (the blocking call's, or vb_fullrank_set_theta's) must stay behind evaluations still reading the
    PREVIOUS one (vb_elbo_grad_fullrank_enqueue leaves work in flight) and in front of everything that reads the new one."""
    vb, eng, _lib = env
    d, n = 1024, 4096
    rng = np.random.RandomState(9)
    A = rng.randn(d, d)
    model = vb.CorrelatedGaussianModel(rng.randn(d), covariance=A @ A.T / d + np.eye(d))
    fam = vb.FullRankGaussian(d)
    th = [fam.pack(0.1 * rng.randn(d), np.exp(-1.0) * np.eye(d) + 0.01 * np.tril(rng.randn(d, d))) for _ in range(2)]
    eng.set_model(model.device_spec())
    for s in range(4):
        eng.noise_generate(20 + s, n, d, seed=4, stream=s)
    want = [eng.elbo_grad_fullrank(20 + s, n, d, th[s & 1]) for s in range(4)]
    eng.fullrank_set_theta(th[0], d)
    for rep in range(3):
        for s in (0, 2):
            eng.elbo_grad_fullrank_enqueue(20 + s, n, d)              # in flight on the old parameter ...
        got1 = eng.elbo_grad_fullrank(21, n, d, th[1])                  # ... when the new one starts to arrive
        _same(want[1], got1)
        eng.elbo_grad_fullrank_enqueue(23, n, d)                        # the resident parameter is the uploaded one
        _same(want[3], eng.fullrank_get(d))
        eng.fullrank_set_theta(th[0], d)
        eng.elbo_grad_fullrank_enqueue(22, n, d)
        _same(want[2], eng.fullrank_get(d))


def test_pinned_result_arrays_are_ordinary_arrays_and_recycled(env):
    vb, eng, _lib = env
    a = _lib.pinned_array(200000)
    assert isinstance(a, np.ndarray) and a.flags.writeable and a.dtype == np.float64 and a.shape == (200000,)
    a[:] = 1.5
    view = a[10:20]
    addr = a.ctypes.data
    del a
    assert view[0] == 1.5                       # a view keeps the block
    b = _lib.pinned_array(200000)
    assert b.ctypes.data != addr
    del view
    c = _lib.pinned_array(200000)               # ... and the block comes back once the last view is gone
    assert c.ctypes.data == addr
    assert type(_lib.pinned_array(10)) is np.ndarray


def test_pinned_pool_stops_pinning_for_callers_that_keep_everything(env):
    """A caller that keeps every gradient (FASO's history) must not pin the host's memory: beyond MAX_OUTSTANDING the result
    arrays are ordinary pageable ones again -- and pinned ones come back once the kept arrays are dropped."""
    vb, eng, _lib = env
    pool = _lib.PinnedPool(_lib.load(), keep=2)
    pool.MAX_OUTSTANDING = 3 * 8 * 200000
    kept = [pool.array(200000) for _ in range(5)]
    for a in kept:
        a[:] = 2.0
    assert pool._out == 3 * 8 * 200000             # three page-locked blocks out, the other two arrays pageable
    del kept, a
    assert pool._out == 0 and pool.idle_blocks() == 2      # (keep = 2: the third block was freed)
    b = pool.array(200000)
    assert pool._out == 8 * 200000 and pool.idle_blocks() == 1


# ---- the plain-copy route with the look-ahead of numpy's streams ----------------------------------------------------------
_NUMPY_LOOP = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import viabel_amd as vb
from viabel_amd import _lib
from oracle import families as ofam
eng = _lib.default_engine()
D, N = 64, 8192
rng = np.random.RandomState(3)
model = vb.GaussianModel(0.2 * rng.randn(D), np.exp(0.1 * rng.randn(D)))
th_mf = np.concatenate([0.1 * rng.randn(D), -0.5 + 0.1 * rng.randn(D)])
A = rng.randn(D, D)
th_ch = np.concatenate([0.1 * rng.randn(D), ofam.psd_to_free(0.7 * (A @ A.T / D + np.eye(D)))])
prior = np.concatenate([np.zeros(D), 0.3 * np.ones(D)])
objs = {
    'ekl_mf': (vb.ExclusiveKL(vb.MFGaussian(D, seed=5), model, N), th_mf),
    'ekl_mft': (vb.ExclusiveKL(vb.MFStudentT(D, 7.0, seed=5), model, N), th_mf),
    'ekl_mvt': (vb.ExclusiveKL(vb.MultivariateT(D, 9.0, seed=5), model, N), th_ch),
    'dis_mvt': (vb.DISInclusiveKL(vb.MultivariateT(D, 9.0, seed=5), model, N, ess_target=1000,
                                  temper_prior=vb.MFGaussian(D), temper_prior_params=prior, use_resampling=True), th_ch),
}
out = {}
for name, (obj, th) in objs.items():
    np.random.seed(4)
    before = eng.legacy_ahead_stats()[1]
    for it in range(6):
        v, g = obj(th)
        out['%s_v%d' % (name, it)] = np.array(v)
        out['%s_g%d' % (name, it)] = g.copy()
        th = th - 0.01 * g / (1.0 + np.abs(g))
    st = obj.approx._rs.get_state()
    out[name + '_key'] = np.asarray(st[1])
    out[name + '_rest'] = np.array([st[2], st[3], st[4]], dtype=np.float64)
    out[name + '_adopted'] = np.array(eng.legacy_ahead_stats()[1] - before)
np.savez(sys.argv[2], **out)
"""


def test_flagsync_off_with_numpy_look_ahead(tmp_path):
    """VB_FETCH_FLAGSYNC=0 with the look-ahead of numpy's streams on: the look-ahead's draw copies the generator's key with
    push_small, whose plain-copy route polls the look-ahead -- from inside the look-ahead's own enqueue, which used to start
    the job again and recurse until the host stack ran out.  Each mode runs in a child process (a regression is a failed
    return code, not a dead test session): values, gradients and the families' generator states equal to the mapped
    route's, and the look-ahead really served the calls."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for flag in ('0', '1'):
        env = dict(os.environ, VB_FETCH_FLAGSYNC=flag, VB_LEGACY_AHEAD='1')
        path = str(tmp_path / ('flagsync%s.npz' % flag))
        r = subprocess.run([sys.executable, '-c', _NUMPY_LOOP, root, path], env=env, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, (flag, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        res[flag] = dict(np.load(path))
    plain, flagged = res['0'], res['1']
    assert sorted(plain) == sorted(flagged)
    for key in plain:
        if key.endswith('_adopted'):
            assert plain[key] >= 3, (key, plain[key])
        else:
            np.testing.assert_array_equal(plain[key], flagged[key], err_msg=key)
