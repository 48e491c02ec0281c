"""CPU: the host side of ``FASO(device_checks=True)`` -- argument checks, forwarding, and the loop's bookkeeping on a stub
engine whose iterate chain is a numpy array served by ``_chain_stats`` (the GPU tests run the real one)."""
import types

import numpy as np
import pytest

from viabel_amd import _chain_stats as cs, optimization as opt
from viabel_amd.approximations import MFGaussian


class StubEngine:
    """``Engine.chain_*`` over a numpy array."""

    def __init__(self):
        self.chain = None
        self.opened = self.closed = 0

    def chain_open(self, p, capacity_rows):
        assert self.chain is None
        self.chain, self.capacity = np.empty((0, p)), capacity_rows
        self.opened += 1

    def chain_close(self):
        self.chain = None
        self.closed += 1

    def chain_rows(self):
        return self.chain.shape[0]

    def chain_fetch(self, first_row, n_rows):
        return self.chain[first_row:first_row + n_rows].copy()

    def chain_mean(self, w):
        return np.mean(self.chain[-w:], axis=0)

    def chain_rhat(self, windows, jitter=1e-8):
        return np.array([np.max(cs.compute_R_hat(self.chain[-w:], jitter=jitter)) for w in windows])

    def chain_ess_mcse(self, w):
        ess, mcse = cs.MCSE(self.chain[-w:])
        return np.asarray(ess), mcse


class StubObjective:
    """SGD on a noisy quadratic behind the ``device_fit`` contract; coordinate 1 never gets a gradient."""

    def __init__(self, eng, p, approx=None, device=True):
        self.eng, self.p, self.device = eng, p, device
        self.approx = approx if approx is not None else types.SimpleNamespace(supports_kl=False)
        self.rs = np.random.RandomState(5)
        self.target = np.linspace(-1.0, 1.0, p)
        self.calls = []

    def supports_device_fit(self):
        return self.device

    def _engine(self):
        return self.eng

    def device_fit(self, n_iters, init_param, opt_kind, hyper, state=None, hist_len=0, log_directions=False,
                   log_gradients=False):
        self.calls.append((n_iters, hist_len, log_directions, log_gradients))
        theta = np.array(init_param, dtype=float)
        values, rows, grads = np.empty(n_iters), np.empty((n_iters, self.p)), np.empty((n_iters, self.p))
        for k in range(n_iters):
            g = theta - self.target + self.rs.randn(self.p)
            g[1] = 0.0
            values[k] = 0.5 * np.sum((theta - self.target) ** 2)
            theta = theta - hyper[0] * g
            rows[k], grads[k] = theta, g
        if self.eng.chain is not None:
            assert hist_len == 0 and self.eng.chain.shape[0] + n_iters <= self.eng.capacity
            self.eng.chain = np.concatenate([self.eng.chain, rows])
        return (theta, values, rows[n_iters - hist_len:], np.zeros(2 * self.p), grads.copy() if log_directions else None,
                grads if log_gradients else None)


def _faso(device_checks, diagnostics=True, **kw):
    sgo = opt.StochasticGradientOptimizer(0.05, diagnostics=diagnostics)
    return opt.FASO(sgo, **dict(dict(W_min=100, k_check=50, device_checks=device_checks), **kw))


def test_device_checks_need_the_device_loop():
    init = np.zeros(6)
    with pytest.raises(NotImplementedError, match='device-resident loop'):
        _faso(True).optimize(300, StubObjective(StubEngine(), 6), init, on_device=False)
    with pytest.raises(NotImplementedError, match='device-resident loop'):       # an objective without supports_device_fit()
        _faso(True).optimize(300, StubObjective(StubEngine(), 6, device=False), init)
    with pytest.raises(NotImplementedError, match='device-resident loop'):
        _faso(True).optimize(300, StubObjective(StubEngine(), 6, device=False), init, on_device=True)


def test_byte_budget(monkeypatch):
    eng = StubEngine()
    monkeypatch.setattr(opt, '_DEVICE_CHAIN_BYTES', 300 * 6 * 8 - 1)
    with pytest.raises(ValueError) as err:
        _faso(True).optimize(300, StubObjective(eng, 6), np.zeros(6))
    assert str(300 * 6 * 8) in str(err.value) and str(300 * 6 * 8 - 1) in str(err.value)
    assert eng.opened == 0
    monkeypatch.setattr(opt, '_DEVICE_CHAIN_BYTES', 300 * 6 * 8)
    _faso(True).optimize(300, StubObjective(eng, 6), np.zeros(6))
    assert eng.opened == eng.closed == 1 and eng.capacity == 300
    assert opt.FASO.__init__.__kwdefaults__['device_checks'] is False


def test_raabbvi_forwards_the_switch():
    sgo = opt.RMSProp(0.01)
    assert opt.RAABBVI(sgo, device_checks=True)._device_checks is True
    assert opt.RAABBVI(sgo)._device_checks is False and opt.FASO(sgo)._device_checks is False


@pytest.mark.parametrize('meanfield', [False, True], ids=['generic', 'mf_gaussian'])
@pytest.mark.parametrize('diagnostics', [False, True], ids=['plain', 'diagnostics'])
def test_loop_bookkeeping_on_a_stub_engine(diagnostics, meanfield):
    p = 8
    approx = MFGaussian(p // 2) if meanfield else None
    init = np.zeros(p)
    # a threshold the first check cannot meet (the generic family's frozen coordinate has a NaN ESS anyway)
    kw = dict(diagnostics=diagnostics, mcse_threshold=1e-9)
    host_obj, dev_eng = StubObjective(StubEngine(), p, approx), StubEngine()
    dev_obj = StubObjective(dev_eng, p, approx)
    host = _faso(False, **kw).optimize(1200, host_obj, init)
    dev = _faso(True, **kw).optimize(1200, dev_obj, init)
    assert dev_eng.opened == dev_eng.closed == 1 and dev_eng.chain is None
    assert all(c[1:] == (0, False, False) for c in dev_obj.calls) and all(c[1] == c[0] and c[3] for c in host_obj.calls)
    assert set(dev) == set(host)
    assert host['k_Rhat'] is not None and dev['k_Rhat'] == host['k_Rhat'] and dev['k_conv'] == host['k_conv']
    assert dev['k_stopped'] == host['k_stopped']
    n = min(len(dev['value_history']), len(host['value_history']))
    np.testing.assert_array_equal(dev['value_history'][:n], host['value_history'][:n])
    for key in ('variational_param_history', 'grad_history') + (('descent_dir_history',) if diagnostics else ()):
        assert dev[key].shape == (0, p) and host[key].shape[1] == p
    assert ('descent_dir_history' in dev) == diagnostics
    assert dev['opt_param'].shape == (p,)
    if diagnostics:      # the first MCSE check sees the same rows in both modes
        np.testing.assert_array_equal(dev['iterate_average_history'][1], host['iterate_average_history'][1])
        np.testing.assert_array_equal(dev['ess_history'][0], host['ess_history'][0])
        np.testing.assert_array_equal(dev['mcse_history'][0], host['mcse_history'][0])
        assert len(dev['ess_history'][0]) == (p - 1 if meanfield else p)      # the frozen coordinate is dropped


def test_chain_is_closed_when_the_loop_raises():
    eng = StubEngine()
    obj = StubObjective(eng, 6)

    def boom(*a, **k):
        raise RuntimeError('boom')
    obj.device_fit = boom
    with pytest.raises(RuntimeError, match='boom'):
        _faso(True).optimize(300, obj, np.zeros(6))
    assert eng.opened == eng.closed == 1


def test_device_convergence_check_logic():
    eng = StubEngine()
    eng.chain_open(3, 400)
    rs = np.random.RandomState(0)
    eng.chain = np.concatenate([np.linspace(0, 5, 200)[:, None] + rs.randn(200, 3), rs.randn(200, 3)])
    windows = np.linspace(50, 380, 5, dtype=int)
    for threshold in (1.01, 1.1, 3.0):
        assert cs.device_R_hat_convergence_check(eng, windows, threshold) == \
            cs.R_hat_convergence_check(list(eng.chain), windows, threshold)
    ess, mcse = cs.device_MCSE(eng, 150)
    ref = cs.MCSE(eng.chain[-150:])
    np.testing.assert_array_equal(ess, ref[0])
    np.testing.assert_array_equal(mcse, ref[1])
