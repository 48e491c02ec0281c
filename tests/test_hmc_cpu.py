"""CPU: the HMC oracle (tests/_hmc_oracle.py) against the properties of the algorithm -- reversibility, what dual averaging
converges to, the statistical conditions the GPU test holds the device to --, the seeds of the GPU parity grid, the argument
checks of ``hmc`` that need no engine, and the result algebra (mean, sd, rhat) against plain numpy."""
import os

import numpy as np
import pytest

import _hmc_oracle as HO
from oracle import models as omod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. reversibility ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['gauss', 'funnel'])
@pytest.mark.parametrize('n_leapfrog', [1, 7])
def test_reversibility(kind, n_leapfrog):
    rng = np.random.RandomState(3)
    d, c = 5, 6
    host = omod.GaussDiag(rng.randn(d), np.exp(0.5 * rng.randn(d))) if kind == 'gauss' else omod.Funnel(d)
    vg = HO.value_and_grad_of(host)
    inv_mass = np.exp(0.3 * rng.randn(d))
    x0 = 0.5 * rng.randn(c, d)
    p0 = rng.randn(c, d) / np.sqrt(inv_mass)
    g0 = vg(x0)[1]
    x1, p1, _, g1 = HO.trajectory(vg, x0, p0, g0, 0.05, n_leapfrog, inv_mass)
    assert np.max(np.abs(x1 - x0)) > 1e-3                                  # it moved
    x2, p2, _, _ = HO.trajectory(vg, x1, -p1, g1, 0.05, n_leapfrog, inv_mass)
    assert np.max(np.abs(x2 - x0)) < 1e-10 and np.max(np.abs(p2 + p0)) < 1e-10


# ---- 2. dual averaging --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', [2, 16, 64])
def test_dual_averaging_reaches_the_target(d):
    rng = np.random.RandomState(d)
    mean, sd = rng.randn(d), np.exp(rng.randn(d))
    c = 32
    res = HO.run(HO.value_and_grad_of(omod.GaussDiag(mean, sd)), mean + sd * rng.randn(c, d),
                 HO.philox_normals(7, 0, c, d), inv_mass=sd ** 2, n_warmup=150, n_draws=100, n_leapfrog=8,
                 step_size=d ** -0.25, target_accept=0.8, jitter=0.2, seed=7)
    acc = float(np.mean(res['accept_prob'][150:]))
    print('D = %d: sampling acceptance %.3f at step %.3f' % (d, acc, res['step_size']))
    assert 0.65 <= acc <= 0.95
    assert res['n_divergent'] == 0
    # the histories: warm-up starts at step_size (jitter aside), the sampling phase holds one base step
    assert abs(res['step_size_history'][0] / d ** -0.25 - 1.0) <= 0.2 + 1e-12
    assert np.all(np.abs(res['step_size_history'][150:] / res['step_size'] - 1.0) <= 0.2 + 1e-12)


def test_no_warmup_keeps_the_step():
    rng = np.random.RandomState(0)
    res = HO.run(HO.value_and_grad_of(omod.GaussDiag(np.zeros(3), np.ones(3))), rng.randn(4, 3),
                 HO.philox_normals(1, 0, 4, 3), n_warmup=0, n_draws=5, n_leapfrog=2, step_size=0.37, jitter=0.0)
    assert res['step_size'] == 0.37 and np.all(res['step_size_history'] == 0.37)


# ---- 3. the statistical conditions of the GPU test, met by the oracle alone -----------------------------------------------
@pytest.mark.parametrize('name', ['a', 'b'])
def test_oracle_meets_statistical_conditions(name):
    host, exact_mean, exact_cov, inv_mass, start, _ = HO.stat_config(name)
    d = exact_mean.size
    res = HO.run(HO.value_and_grad_of(host), start, HO.philox_normals(HO.STAT_SEED, 0, HO.STAT_CHAINS, d),
                 inv_mass=inv_mass, n_warmup=HO.STAT_WARMUP, n_draws=HO.STAT_DRAWS, n_leapfrog=HO.STAT_LEAPFROG,
                 step_size=d ** -0.25, target_accept=0.8, jitter=0.2, seed=HO.STAT_SEED)
    res['mean'], res['sd'], res['rhat'] = HO.combine_chains(res['chain_mean'], res['chain_var'], HO.STAT_DRAWS)
    figures = HO.stat_conditions(name, res, exact_mean, exact_cov)
    for label, (value, bound, ok) in figures.items():
        print('(%s) %s: %s (bound %s)' % (name, label, value, bound))
    assert all(ok for _, _, ok in figures.values()), figures


# ---- the seeds of the GPU parity grid: no accept test closer than the margin --------------------------------------------------
@pytest.mark.parametrize('kind', HO.PARITY_MODELS)
def test_parity_seeds_leave_a_margin(kind):
    """The GPU test compares accept decisions exactly, so no case may decide one within MIN_MARGIN.  The host normals here
    are within rounding of the device's; the bound is held at ten times the margin to cover that."""
    worst = np.inf
    n_cases = 0
    for n_chains in HO.PARITY_CHAINS:
        for case in HO.parity_cases(kind, n_chains):
            host, _ = HO.parity_problem(kind, case['d'])
            res = HO.run_case(host, case, HO.philox_normals(case['seed'], case['stream_offset'], n_chains, case['d']))
            assert res['min_margin'] >= 10.0 * HO.MIN_MARGIN, (case['key'], res['min_margin'])
            assert np.all(np.isfinite(res['last']))
            worst = min(worst, res['min_margin'])
            n_cases += 1
    print('%s: %d cases, smallest |log u - dH| = %.2e' % (kind, n_cases, worst))


# ---- 4. argument errors that need no engine -----------------------------------------------------------------------------------
def test_argument_errors():
    import viabel_amd as vb
    model = vb.GaussianModel(np.zeros(3), np.ones(3))
    init = np.zeros((4, 3))
    ok = dict(n_chains=4, n_warmup=2, n_draws=2, n_leapfrog=2, init=init)
    with pytest.raises(TypeError):
        vb.hmc(lambda x: -0.5 * np.sum(x * x, axis=1), **ok)
    with pytest.raises(TypeError):
        vb.hmc(vb.Model(lambda x: -0.5 * np.sum(x * x, axis=1)), **ok)
    with pytest.raises(NotImplementedError):
        vb.hmc(vb.CallableModel(3, lambda x: -0.5 * np.sum(x * x, axis=1)), **ok)
    approx = vb.MFGaussian(3)
    bad = [dict(n_chains=0), dict(n_chains=2.5), dict(n_warmup=-1), dict(n_draws=0), dict(n_leapfrog=0), dict(thin=0),
           dict(step_size=0.0), dict(step_size=-1.0), dict(step_size=np.inf), dict(step_size=np.nan),
           dict(target_accept=0.0), dict(target_accept=1.0), dict(jitter=-0.1), dict(jitter=1.0),
           dict(init=np.zeros((4, 2))), dict(init=np.zeros((3, 3))), dict(init=np.zeros(3)),
           dict(inv_mass=np.ones(2)), dict(inv_mass=np.array([1.0, 0.0, 1.0])), dict(inv_mass=np.array([1.0, -1.0, 1.0])),
           dict(inv_mass=np.array([1.0, np.inf, 1.0])),
           dict(var_param=np.zeros(6)), dict(approx=approx),              # only one of the two
           dict(init=None)]                                               # neither init nor a fit
    for kw in bad:
        args = dict(ok)
        args.update(kw)
        with pytest.raises(ValueError):
            vb.hmc(model, **args)


def test_binding_declares_the_entry():
    import ctypes
    from viabel_amd import _lib
    restype, argtypes = _lib.SIGNATURES['vb_hmc_run']
    assert restype is ctypes.c_int and len(argtypes) == 24
    header = open(os.path.join(ROOT, 'include', 'viabel_hip.h')).read()
    assert 'int vb_hmc_run(vb_ctx* ctx' in header
    assert 'vb_hmc.hip' in open(os.path.join(ROOT, 'viabel_amd', 'csrc', 'Makefile')).read()
    lib = _lib.load()
    assert lib.vb_hmc_run(*[None if t in (_lib._ctx_p, _lib._c_double_p, _lib._c_int64_p) else 0 for t in argtypes]) \
        == _lib.VB_ERR_INVALID


# ---- 5. result algebra --------------------------------------------------------------------------------------------------------
def test_result_algebra_matches_numpy():
    from viabel_amd.mcmc import _combine_chains
    rng = np.random.RandomState(2)
    d, c, n = 4, 8, 30
    host = omod.GaussDiag(rng.randn(d), np.exp(rng.randn(d)))
    res = HO.run(HO.value_and_grad_of(host), rng.randn(c, d), HO.philox_normals(3, 0, c, d), n_warmup=10, n_draws=n,
                 n_leapfrog=4, step_size=0.5, jitter=0.2, seed=3)
    draws = res['draws']                                                   # (n, C, D), thin = 1
    assert draws.shape == (n, c, d)
    np.testing.assert_allclose(res['chain_mean'], draws.mean(axis=0), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(res['chain_var'], draws.var(axis=0, ddof=1), rtol=1e-11, atol=1e-13)
    mean, sd, rhat = _combine_chains(res['chain_mean'], res['chain_var'], n)
    w = draws.var(axis=0, ddof=1).mean(axis=0)
    b = n * draws.mean(axis=0).var(axis=0, ddof=1)
    var_plus = (n - 1.0) / n * w + b / n
    np.testing.assert_allclose(mean, draws.mean(axis=(0, 1)), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(sd, np.sqrt(var_plus), rtol=1e-11)
    np.testing.assert_allclose(rhat, np.sqrt(var_plus / w), rtol=1e-11)
    o_mean, o_sd, o_rhat = HO.combine_chains(res['chain_mean'], res['chain_var'], n)
    np.testing.assert_allclose(sd, o_sd, rtol=1e-13)
    np.testing.assert_allclose(rhat, o_rhat, rtol=1e-13)
    # thinning keeps every thin-th sampling iteration, the first included, and leaves the statistics alone
    res3 = HO.run(HO.value_and_grad_of(host), rng.randn(c, d), HO.philox_normals(3, 0, c, d), n_warmup=0, n_draws=7,
                  n_leapfrog=2, step_size=0.5, thin=3, seed=3)
    assert res3['draws'].shape == (3, c, d) and res3['logp'].shape == (3, c)
    assert np.array_equal(res3['draws'][-1], res3['last'])                 # iteration 6 is kept and is the last
