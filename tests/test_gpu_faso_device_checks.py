"""GPU: ``FASO(device_checks=True)`` -- iterates kept in the engine's chain, stationarity and MCSE checks on the device --
against the default mode on a twin objective with the same seed.

Both modes run the same device fit on the same Philox noise, so the values and the iterates are the same bits; the iterate
averages are numpy's additions in numpy's order (``array_equal``); R-hat maxima agree to 1e-11 and ESS / MCSE to 1e-10 (the
tolerances of tests/test_gpu_chain_stats.py), so ``k_Rhat`` / ``k_conv`` are equal.  After the first MCSE check the pacing
of the re-checks depends on wall-clock ratios in either mode, so nothing later is compared."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import viabel_amd as vb  # noqa: E402
from viabel_amd import _lib, optimization as opt  # noqa: E402

ESS_TOL = 1e-10


def _target(D):
    rng = np.random.RandomState(4)
    return rng.randn(D), np.exp(0.3 * rng.randn(D))


def _meanfield():
    D = 12
    mean, sd = _target(D)
    return (lambda: vb.ExclusiveKL(vb.MFGaussian(D, seed=3, rng='philox'), vb.GaussianModel(mean, sd), 32),
            np.concatenate([np.zeros(D), np.zeros(D)]), 0.05)


def _fullrank():
    D = 10
    mean, sd = _target(D)
    fr = vb.FullRankGaussian(D)
    return (lambda: vb.ExclusiveKL(vb.FullRankGaussian(D, seed=2, rng='philox'), vb.GaussianModel(mean, sd), 32),
            fr.pack(np.zeros(D), np.eye(D)), 0.05)


def _flow():
    from test_gpu_nvp_flow import make_flow
    D = 6
    mean, sd = _target(D)

    def make():
        return vb.ExclusiveKL(make_flow(D, 2, [10], [10], 'gauss', 'philox', prior_scale=0.1), vb.GaussianModel(mean, sd), 64)
    p = make_flow(D, 2, [10], [10], 'gauss', 'philox').var_param_dim
    # multiples of 2^-10: a weight behind a mask never gets a gradient, and the sum of w copies of such a value is exact, so
    # that column is exactly constant after centring in the host's arithmetic and the device's alike (ESS NaN in both)
    return make, np.round(0.1 * np.random.RandomState(0).randn(p) * 1024) / 1024, 0.02


PROBLEMS = {'meanfield': _meanfield, 'fullrank': _fullrank, 'nvp': _flow}


def _run(make, init, lr, device_checks, n_iters=3000, **faso):
    sgo = opt.RMSProp(lr, diagnostics=True)
    faso = dict(dict(W_min=100, k_check=50), **faso)
    return opt.FASO(sgo, device_checks=device_checks, **faso).optimize(n_iters, make(), init)


@pytest.mark.parametrize('name', sorted(PROBLEMS))
def test_device_checks_reproduce_the_default_mode(name):
    make, init, lr = PROBLEMS[name]()
    p = init.size
    # a threshold no MCSE can meet: the run goes on after the first check (whose ESS / MCSE are compared)
    host = _run(make, init, lr, False, mcse_threshold=1e-12)
    dev = _run(make, init, lr, True, mcse_threshold=1e-12)
    if name != 'nvp':      # (a flow's weakly determined weights wander: it need not be declared stationary this soon)
        assert host['k_Rhat'] is not None, 'the problem must reach stationarity for the test to mean anything'
    assert dev['k_Rhat'] == host['k_Rhat'] and dev['k_conv'] == host['k_conv']
    n = min(len(host['value_history']), len(dev['value_history']))
    assert n == 3000 or n > host['k_Rhat']
    np.testing.assert_array_equal(dev['value_history'][:n], host['value_history'][:n])
    # every stationarity check up to the first MCSE check (all of them if there is none) chose the same window: the
    # iterate average over it is recorded, and is numpy's mean of the same rows
    if host['k_Rhat'] is not None:
        first_mcse = host['ess_and_mcse_k_history'][0]
        assert dev['ess_and_mcse_k_history'][0] == first_mcse == host['k_Rhat']
        upto = int(np.searchsorted(host['iterate_average_k_history'], first_mcse, side='right'))
    else:
        upto = len(host['iterate_average_k_history'])
        assert len(dev['iterate_average_k_history']) == upto
    assert upto >= 2
    np.testing.assert_array_equal(dev['iterate_average_k_history'][:upto], host['iterate_average_k_history'][:upto])
    for a, b in zip(dev['iterate_average_history'][:upto], host['iterate_average_history'][:upto]):
        np.testing.assert_array_equal(a, b)
    for key in ('ess_history', 'mcse_history') if host['k_Rhat'] is not None else ():
        a, b = np.asarray(dev[key][0], dtype=float), np.asarray(host[key][0], dtype=float)
        # (a parameter that never gets a gradient -- a flow's weights behind a mask -- is a constant column: NaN in both)
        np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
        live = ~np.isnan(b)
        assert live.sum() >= p // 2
        err = float(np.max(np.abs(a[live] - b[live]) / np.abs(b[live])))
        print('%s %s: largest relative error %.3g over %d of %d parameters' % (name, key, err, live.sum(), p))
        assert err <= ESS_TOL
    # the histories that stayed on the device come back empty, of the right width; every key is there
    assert set(dev) == set(host)
    for key in ('variational_param_history', 'grad_history', 'descent_dir_history'):
        assert dev[key].shape == (0, p) and host[key].shape[1] == p


@pytest.mark.parametrize('name', sorted(PROBLEMS))
def test_first_mcse_check_stops_both_modes_alike(name):
    make, init, lr = PROBLEMS[name]()
    host = _run(make, init, lr, False, mcse_threshold=1e6, ESS_min=1)
    dev = _run(make, init, lr, True, mcse_threshold=1e6, ESS_min=1)
    assert dev['k_stopped'] == host['k_stopped']
    assert dev['k_Rhat'] == host['k_Rhat'] and dev['k_conv'] == host['k_conv']
    if name != 'nvp':      # (a flow's weights behind a mask never move: their ESS is NaN, which no threshold passes)
        assert host['k_stopped'] is not None
    if host['k_stopped'] is not None:
        np.testing.assert_array_equal(dev['opt_param'], host['opt_param'])
        np.testing.assert_array_equal(dev['value_history'], host['value_history'])
        assert len(dev['iterate_average_history']) == len(host['iterate_average_history'])
        for a, b in zip(dev['iterate_average_history'], host['iterate_average_history']):
            np.testing.assert_array_equal(a, b)


def test_bbvi_raabbvi_with_device_checks():
    D = 8
    mean, sd = _target(D)
    approx = vb.MFGaussian(D, seed=5, rng='philox')
    obj = vb.ExclusiveKL(approx, vb.GaussianModel(mean, sd), 32)
    res = vb.bbvi(D, n_iters=2500, objective=obj, learning_rate=0.05,
                  RAABBVI_kwargs=dict(W_min=100, k_check=50, device_checks=True))
    p = approx.var_param_dim
    assert res['opt_param'].shape == (p,) and np.isfinite(res['opt_param']).all()
    assert res['variational_param_history'].shape[1] == p and res['grad_history'].shape[1] == p
    assert len(res['value_history']) > 100
    assert abs(res['opt_param'][:D] - mean).max() < 0.5


def test_nothing_of_length_p_is_logged(monkeypatch):
    """A spy on ``Engine.fit`` / ``flow_fit``: with ``device_checks`` no call asks for history, directions or gradients."""
    eng = _lib.default_engine()
    asked = []
    for attr in ('fit', 'flow_fit'):
        real = getattr(eng, attr)

        def spy(*args, _real=real, _attr=attr, **kw):
            asked.append((_attr, kw.get('hist_len', 0), bool(kw.get('log_directions')), bool(kw.get('log_gradients'))))
            return _real(*args, **kw)
        monkeypatch.setattr(eng, attr, spy)
    for name in ('meanfield', 'nvp'):
        make, init, lr = PROBLEMS[name]()
        _run(make, init, lr, True, n_iters=400)
    assert {a[0] for a in asked} == {'fit', 'flow_fit'}
    assert all(a[1:] == (0, False, False) for a in asked), asked
    asked.clear()
    make, init, lr = PROBLEMS['meanfield']()
    _run(make, init, lr, False, n_iters=200)
    assert asked and all(a[1] > 0 and a[3] for a in asked)      # the default mode does ask: the spy sees what it should
    with pytest.raises(_lib.EngineError):
        eng.chain_rows()                                        # the chain was closed behind each run
