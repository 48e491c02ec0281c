"""CPU: the ChEES-HMC oracle (tests/_hmc_chees_oracle.py) against hand values and properties of the algorithm, the vetting
of every case the GPU test uses (accept margins, step-count margins, the size of the perturbation yardstick), the argument
checks of ``hmc``'s trajectory keywords and the binding of ``vb_hmc_run_chees``."""
import ctypes
import os

import numpy as np
import pytest

import _hmc_chees_oracle as CO
import _hmc_metric_oracle as MO
import _hmc_oracle as HO
from oracle import models as omod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the radical inverse and the step count --------------------------------------------------------------------------------
def test_halton_hand_values():
    half_cell = 2.0 ** -33
    for s, value in ((0, 0.5), (1, 0.25), (2, 0.75), (3, 0.125), (4, 0.625), (7, 0.0625)):
        assert CO.halton(s) == value + half_cell, s
    # the low 32 bits of s + 1 wrap: s + 1 = 2^32 is index 0, s + 1 = 2^32 + 1 is index 1; s + 1 = 2^32 - 1 is all ones
    assert CO.halton(2 ** 32 - 1) == half_cell
    assert CO.halton(2 ** 32) == 0.5 + half_cell
    assert CO.halton(5 * 2 ** 32 + 2) == 0.75 + half_cell
    assert CO.halton(2 ** 32 - 2) == 1.0 - half_cell
    assert all(0.0 < CO.halton(s) < 1.0 for s in range(2000))


def test_step_count_and_margin():
    assert CO.n_steps(0.3, 0.1, 10)[0] == 3 or CO.n_steps(0.3, 0.1, 10)[0] == 4       # (0.3 / 0.1 is not 3 in fp64)
    assert CO.n_steps(0.25, 0.1, 10) == (3, 0.5)
    assert CO.n_steps(0.01, 0.1, 10)[0] == 1 and CO.n_steps(0.01, 0.1, 10)[1] == pytest.approx(0.1)
    assert CO.n_steps(5.0, 0.1, 10) == (10, np.inf)                                    # the clamp is active: no margin
    assert CO.n_steps(1.0, 0.125, 8) == (8, 0.0)                                       # exactly at the bound: not clamped
    assert CO.n_steps(np.nan, 0.1, 10) == (1, np.inf)


# ---- 2. vetting of the GPU test's cases ---------------------------------------------------------------------------------------
def _vet(res, pert, key):
    assert res['min_margin'] >= 10.0 * HO.MIN_MARGIN, (key, 'accept margin', res['min_margin'])
    assert res['min_step_margin'] >= 10.0 * CO.MIN_STEP_MARGIN, (key, 'step-count margin', res['min_step_margin'])
    assert np.array_equal(res['n_leapfrog_history'], pert['n_leapfrog_history']), key
    spread = CO.history_spread(res, pert)
    assert spread <= CO.MAX_HISTORY_SPREAD, (key, 'perturbed trajectory history', spread)
    assert np.all(np.isfinite(res['last'])) and np.all(np.isfinite(res['trajectory_history']))
    return spread


@pytest.mark.parametrize('kind', CO.PARITY_MODELS)
def test_parity_seeds(kind):
    """No case may decide an accept test within MIN_MARGIN or a step count within MIN_STEP_MARGIN of the boundary (the GPU
    test compares both exactly; the bounds are held at ten times the margins because the host normals here are only within
    rounding of the device's), and the perturbation hook may not move the trajectory history by more than 1e-6: a yardstick
    that loose would hide a failure."""
    worst, n_cases, counts = 0.0, 0, np.zeros(CO.PARITY_MAX_LEAPFROG + 1, dtype=int)
    for n_chains in CO.PARITY_CHAINS:
        for case in CO.parity_cases(kind, n_chains):
            host, _ = HO.parity_problem(kind, case['d'])
            z = HO.philox_normals(case['seed'], case['stream_offset'], n_chains, case['d'])
            res = CO.run_case(host, case, z)
            pert = CO.run_case(host, case, z, perturb=np.random.RandomState(case['seed']))
            worst = max(worst, _vet(res, pert, case['key']))
            # (a warm-up iteration in which no chain has a positive acceptance probability does not adapt: two chains do that)
            assert res['adapted'][:CO.PARITY_WARMUP].sum() >= 3 and not res['adapted'][CO.PARITY_WARMUP:].any(), case['key']
            counts += np.bincount(res['n_leapfrog_history'], minlength=counts.size)
            n_cases += 1
    print('%s: %d cases, largest history spread %.2e, step counts 1..%d used %s times' % (
        kind, n_cases, worst, CO.PARITY_MAX_LEAPFROG, counts[1:]))
    assert np.all(counts[1:] > 0)                     # every step count up to the clamp occurs somewhere in the grid


@pytest.mark.parametrize('dense', [False, True])
def test_unusable_case_has_what_it_is_for(dense):
    case = CO.unusable_case(dense)
    host = omod.Funnel(case['d'])
    z = HO.philox_normals(case['seed'], case['stream_offset'], CO.UNUSABLE_CHAINS, case['d'])
    res = CO.run_case(host, case, z)
    pert = CO.run_case(host, case, z, perturb=np.random.RandomState(case['seed']), perturb_groups=case['groups'])
    _vet(res, pert, case['key'])
    w = CO.PARITY_WARMUP
    not_finite = ~res['usable'][:w]
    divergent_finite = res['divergent'][:w] & res['usable'][:w]
    assert np.all(not_finite[:, list(CO.UNUSABLE_OVERFLOW)]) and not_finite.sum() == 2 * w
    assert np.all(divergent_finite[:, list(CO.UNUSABLE_DIVERGENT)])
    assert res['adapted'][:w].all()                                     # the other chains still adapt the length
    assert np.all(res['a'][:w][not_finite] == 0.0)
    assert np.array_equal(res['last'][list(CO.UNUSABLE_OVERFLOW)], case['x0'][list(CO.UNUSABLE_OVERFLOW)])


def test_all_chains_rejected_leaves_the_length():
    host = omod.GaussDiag(np.zeros(CO.REJECT_DIM), 1e-3 * np.ones(CO.REJECT_DIM))
    x0 = 1e-3 * np.random.RandomState(0).randn(CO.REJECT_CHAINS, CO.REJECT_DIM)
    res = CO.run(HO.value_and_grad_of(host), x0, HO.philox_normals(1, 0, CO.REJECT_CHAINS, CO.REJECT_DIM),
                 inv_mass=np.ones(CO.REJECT_DIM), n_warmup=CO.REJECT_WARMUP, n_draws=2, max_leapfrog=CO.PARITY_MAX_LEAPFROG,
                 step_size=CO.REJECT_STEP, trajectory_length=CO.REJECT_LENGTH, jitter=0.0, seed=1)
    assert res['divergent'].all() and not res['adapted'].any() and np.all(res['a'] == 0.0)
    assert res['traj_state'][1] == 0.0 and res['traj_state'][3] == CO.REJECT_WARMUP      # v untouched, m advanced
    # the clamp's interval [eps_base, 5 eps_base] holds T throughout, so the history is the length it started from
    base = np.append(res['step_size_history'][1:CO.REJECT_WARMUP], res['step_size'])
    assert np.all(base < CO.REJECT_LENGTH) and np.all(CO.REJECT_LENGTH < CO.PARITY_MAX_LEAPFROG * base)
    np.testing.assert_allclose(res['trajectory_history'], CO.REJECT_LENGTH, rtol=1e-14)      # (a few ulps of log T = 3.2)


@pytest.mark.parametrize('dense', [False, True])
def test_adaptive_seeds(dense):
    for n_chains in MO.ADAPT_CHAINS:
        for d in MO.ADAPT_DIMS:
            case = MO.adapt_case(n_chains, d, dense)
            host = omod.GaussDiag(case['mean'], case['sd'])
            z = HO.philox_normals(case['seed'], case['stream_offset'], n_chains, d)
            kw = dict(dense=dense, inv_mass=np.eye(d) if dense else np.ones(d), n_warmup=MO.ADAPT_WARMUP,
                      n_draws=MO.ADAPT_DRAWS, max_leapfrog=CO.ADAPT_MAX_LEAPFROG, step_size=case['step_size'],
                      trajectory_length=CO.ADAPT_LENGTH_STEPS * case['step_size'], jitter=case['jitter'], seed=case['seed'],
                      stream_offset=case['stream_offset'])
            res = CO.run_adaptive(HO.value_and_grad_of(host), case['x0'], z, **kw)
            pert = CO.run_adaptive(HO.value_and_grad_of(host), case['x0'], z, perturb=np.random.RandomState(case['seed']), **kw)
            _vet(res, pert, case['key'])
            assert res['adapt_windows'] == [(6, 36)] and res['n_divergent'] == 0
            assert res['trajectory_history'].shape == (MO.ADAPT_WARMUP + MO.ADAPT_DRAWS,)
            assert res['traj_state'][3] == MO.ADAPT_WARMUP            # m counts the warm-up iterations of all segments
            # carried, not reset: across a window end the length moves by one Adam step (and the clamp), not back to T_0
            steps = np.abs(np.diff(np.log(res['trajectory_history'][:MO.ADAPT_WARMUP])))
            assert np.max(steps[[5, 35]]) < 0.5 and abs(np.log(res['trajectory_history'][36] / kw['trajectory_length'])) > 0.5


# ---- 3. properties ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dense', [False, True])
def test_scale_equivariance(dense):
    """The target N(0, (k s)^2 I) from starts k x0 with step k eps and length k T0 gives k times the trajectory history and
    the same step counts and decisions.  (The criterion scales as k^4, Adam's step by nothing but its 1e-8: the base scale
    s = 10 makes the estimates ~1e4, so that term is far below the tolerance.)"""
    rng = np.random.RandomState(12)
    d, c, s, k = 6, 16, 10.0, 3.0
    x0, z = s * rng.randn(c, d), HO.philox_normals(5, 0, c, d)
    a = rng.randn(d, d)
    metric = dict(L=np.linalg.cholesky(a @ a.T / d + np.eye(d))) if dense else dict(inv_mass=np.exp(0.2 * rng.randn(d)))
    kw = dict(n_warmup=12, n_draws=4, max_leapfrog=8, jitter=0.2, seed=5, **metric)
    one = CO.run(HO.value_and_grad_of(omod.GaussDiag(np.zeros(d), s * np.ones(d))), x0, z, step_size=0.1 * s,
                 trajectory_length=0.4 * s, **kw)
    two = CO.run(HO.value_and_grad_of(omod.GaussDiag(np.zeros(d), k * s * np.ones(d))), k * x0, z, step_size=0.1 * s * k,
                 trajectory_length=0.4 * s * k, **kw)
    assert one['adapted'][:12].all() and len(set(one['n_leapfrog_history'])) > 2
    assert one['min_step_margin'] > 1e-6 and one['min_margin'] > 1e-6
    np.testing.assert_allclose(two['trajectory_history'], k * one['trajectory_history'], rtol=1e-9)
    np.testing.assert_allclose(two['step_size_history'], k * one['step_size_history'], rtol=1e-9)
    assert np.array_equal(two['n_leapfrog_history'], one['n_leapfrog_history'])
    assert np.array_equal(two['accepted'], one['accepted'])
    np.testing.assert_allclose(two['last'], k * one['last'], rtol=1e-8)


@pytest.mark.parametrize('kind', ['gauss', 'funnel', 'logistic'])
def test_clamped_oracle_is_the_fixed_oracle(kind):
    """With max_leapfrog = L, no warm-up and a length so large that the clamp is always active, every iteration takes L
    steps: the run equals _hmc_oracle.run(n_leapfrog=L) exactly."""
    case = HO.parity_cases(kind, 9)[-1]
    host, _ = HO.parity_problem(kind, case['d'])
    z = HO.philox_normals(case['seed'], case['stream_offset'], 9, case['d'])
    ref = HO.run_case(host, case, z, n_warmup=0, n_draws=6, n_leapfrog=3)
    res = CO.run(HO.value_and_grad_of(host), case['x0'], z, inv_mass=case['inv_mass'], n_warmup=0, n_draws=6, max_leapfrog=3,
                 step_size=case['step_size'], trajectory_length=1e6, jitter=case['jitter'], seed=case['seed'],
                 stream_offset=case['stream_offset'], thin=case['thin'])
    assert np.all(res['n_leapfrog_history'] == 3) and res['min_step_margin'] == np.inf
    for k in ('draws', 'logp', 'last', 'chain_mean', 'chain_var', 'accept_prob', 'step_size_history', 'accept_rate',
              'accepted', 'divergent'):
        assert np.array_equal(res[k], ref[k]), k
    assert res['step_size'] == ref['step_size'] and res['n_divergent'] == ref['n_divergent']
    np.testing.assert_allclose(res['trajectory_history'], 1e6, rtol=1e-15)


def test_oracle_segments_continue_one_run():
    """A call that is handed the last one's trajectory state continues it: m adds up, its warm-up starts from exp(log T),
    its sampling phase uses exp(log T_bar)."""
    rng = np.random.RandomState(3)
    d, c = 4, 8
    host = omod.GaussDiag(np.zeros(d), np.ones(d))
    z = HO.philox_normals(2, 0, c, d)
    kw = dict(inv_mass=np.ones(d), max_leapfrog=6, jitter=0.2, seed=2)
    first = CO.run(HO.value_and_grad_of(host), rng.randn(c, d), z, n_warmup=5, n_draws=0, step_size=0.1, trajectory_length=0.3,
                   **kw)
    assert first['traj_state'][3] == 5.0 and first['traj_state'][1] > 0.0 and first['draws'].shape == (0, c, d)
    second = CO.run(HO.value_and_grad_of(host), first['last'], z, n_warmup=4, n_draws=2, step_size=first['step_size'],
                    traj_state=first['traj_state'], stream_offset=5, t0=5, **kw)
    assert second['traj_state'][3] == 9.0
    assert second['trajectory_history'][0] == np.exp(first['traj_state'][0])          # warm-up continues from log T
    assert np.all(second['trajectory_history'][4:] == np.exp(second['traj_state'][2]))  # sampling uses exp(log T_bar)
    assert second['trajectory_length'] == second['trajectory_history'][-1]


@pytest.mark.parametrize('name', ['a', 'b'])
def test_oracle_meets_statistical_conditions(name):
    """The GPU test's statistical configurations, from a trajectory of one leapfrog step, which the adaptation must leave."""
    host, exact_mean, exact_cov, inv_mass, start, _ = HO.stat_config(name)
    d = exact_mean.size
    kw = dict(inv_mass=inv_mass, n_warmup=HO.STAT_WARMUP, n_draws=HO.STAT_DRAWS, step_size=d ** -0.25, target_accept=0.8,
              jitter=0.2, seed=HO.STAT_SEED)
    res = CO.run(HO.value_and_grad_of(host), start, HO.philox_normals(HO.STAT_SEED, 0, HO.STAT_CHAINS, d),
                 max_leapfrog=CO.STAT_MAX_LEAPFROG, **kw)
    res['mean'], res['sd'], res['rhat'] = HO.combine_chains(res['chain_mean'], res['chain_var'], HO.STAT_DRAWS)
    figures = HO.stat_conditions(name, res, exact_mean, exact_cov)
    for label, (value, bound, ok) in figures.items():
        print('(%s) %s: %s (bound %s)' % (name, label, value, bound))
    print('(%s) T = %.3f, step %.3f, mean L %.2f' % (name, res['trajectory_length'], res['step_size'],
                                                      res['n_leapfrog_history'][HO.STAT_WARMUP:].mean()))
    assert all(ok for _, _, ok in figures.values()), figures
    assert res['trajectory_length'] > 2.0 * res['step_size'] and res['n_leapfrog_history'][HO.STAT_WARMUP:].mean() > 2.0


# ---- 4. argument errors that need no engine -----------------------------------------------------------------------------------
def test_argument_errors_of_the_trajectory_keywords():
    import viabel_amd as vb
    model = vb.GaussianModel(np.zeros(3), np.ones(3))
    ok = dict(n_chains=4, n_warmup=2, n_draws=2, init=np.zeros((4, 3)), trajectory='chees')
    bad = [dict(trajectory='nuts'), dict(trajectory=None), dict(trajectory=1), dict(trajectory='CHEES'),
           dict(max_leapfrog=0), dict(max_leapfrog=-3), dict(max_leapfrog=2.5), dict(max_leapfrog=True),
           dict(max_leapfrog=2 ** 31),
           dict(trajectory_length=0.0), dict(trajectory_length=-1.0), dict(trajectory_length=np.inf),
           dict(trajectory_length=np.nan),
           dict(trajectory_lr=-0.1), dict(trajectory_lr=np.inf), dict(trajectory_lr=np.nan),
           dict(n_chains=1, init=np.zeros((1, 3))),                                        # one chain and a warm-up
           dict(n_chains=1, init=np.zeros((1, 3)), metric='dense')]
    for kw in bad:
        args = dict(ok)
        args.update(kw)
        with pytest.raises(ValueError):
            vb.hmc(model, **args)
    for kw in (dict(max_leapfrog=0), dict(trajectory_length=0.0), dict(trajectory_lr=-1.0)):
        with pytest.raises(ValueError):                                                    # also on the fixed route
            vb.hmc(model, **dict(ok, trajectory='fixed', **kw))
    with pytest.raises(NotImplementedError):                                               # the refusals are unchanged
        vb.hmc(vb.CallableModel(3, lambda x: -0.5 * np.sum(x * x, axis=1)), **ok)


# ---- 5. the binding -----------------------------------------------------------------------------------------------------------
def test_binding_declares_the_entry():
    from viabel_amd import _lib
    restype, argtypes = _lib.SIGNATURES['vb_hmc_run_chees']
    metric_args = _lib.SIGNATURES['vb_hmc_run_metric'][1]
    assert restype is ctypes.c_int and len(argtypes) == len(metric_args) + 4 == 32
    header = open(os.path.join(ROOT, 'include', 'viabel_hip.h')).read()
    assert 'int vb_hmc_run_chees(vb_ctx* ctx' in header
    assert hasattr(_lib.Engine, 'hmc_run_chees')
    lib = _lib.load()
    assert lib.vb_hmc_run_chees(*[None if t in (_lib._ctx_p, _lib._c_double_p, _lib._c_int64_p) else 0
                                  for t in argtypes]) == _lib.VB_ERR_INVALID
