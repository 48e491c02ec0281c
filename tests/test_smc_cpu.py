"""CPU: the numpy oracle of tempered SMC (tests/_smc_oracle.py) -- the margins of every case the GPU test compares exactly,
closed forms, the resampler's properties, the constants of the statistical test -- and ``smc()``'s argument checks."""
import os

import numpy as np
import pytest

import _hmc_oracle as HO
import _smc_oracle as SO
import viabel_amd as vb
from viabel_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- margins: every parity case, none left out ---------------------------------------------------------------------------------
@pytest.mark.parametrize('n', SO.PARITY_PARTICLES)
@pytest.mark.parametrize('kind', HO.PARITY_MODELS)
def test_parity_cases_keep_their_margins(kind, n):
    cases = SO.parity_cases(kind, n)
    assert len(cases) == 4 * len(HO.parity_dims(kind))
    for case in cases:
        host, _ = HO.parity_problem(kind, case['d'])
        normals = SO.philox_normals(case['seed'], n, case['d'])
        ref = SO.run_case(host, case, normals)
        print(case['key'], ref['n_stages'], ref['min_accept_margin'], ref['min_ancestor_margin'], ref['min_ess_margin'])
        # the yardstick of the GPU comparison is a perturbed run: it must take the plain run's decisions
        pert = SO.run_case(host, case, normals, perturb=np.random.RandomState(case['seed']))
        assert pert['n_stages'] == ref['n_stages'] and pert['n_divergent'] == ref['n_divergent'], case['key']
        assert np.array_equal(pert['ancestors'], ref['ancestors']), case['key']
        assert np.array_equal(pert['n_accepted'], ref['n_accepted']), case['key']
        assert ref['min_accept_margin'] >= SO.MIN_ACCEPT_MARGIN, case['key']
        assert ref['min_ancestor_margin'] >= SO.MIN_ANCESTOR_MARGIN, case['key']
        assert ref['min_ess_margin'] >= SO.MIN_ESS_MARGIN, case['key']
        assert ref['betas'][-1] == 1.0 and np.all(np.diff(ref['betas']) > 0.0)
        assert ref['next_stream'] == case['stream_offset'] + 1 + ref['n_stages'] * case['n_moves']
        if n >= 64:            # the bases are poor enough to need a path
            assert ref['n_stages'] >= SO.PARITY_MIN_STAGES, (case['key'], ref['n_stages'])
        if n == 1:
            assert ref['n_stages'] == 1


def test_reseeded_cases_exist():
    for kind, n, idx in SO.PARITY_RESEED:
        assert kind in HO.PARITY_MODELS and n in SO.PARITY_PARTICLES and idx < len(SO.parity_cases(kind, n))
    for kind, n in SO.REWEIGHT_RESEED:
        assert kind in SO.REWEIGHT_KINDS and n in SO.REWEIGHT_SIZES


@pytest.mark.parametrize('kind', SO.REWEIGHT_KINDS)
def test_reweight_inputs_keep_their_ancestor_margin(kind):
    for n in SO.REWEIGHT_SIZES:
        u, beta_prev, uniform = SO.reweight_input(kind, n)
        ref = SO.reweight(u, beta_prev, SO.REWEIGHT_ESS, uniform)
        assert ref['ancestor_margin'] >= SO.MIN_ANCESTOR_MARGIN, (kind, n, ref['ancestor_margin'])
        if kind == 'neginf':
            assert not np.any(np.isin(ref['ancestors'], np.flatnonzero(u == -np.inf)))
        if kind == 'heavy' and n >= 63:
            assert 20.0 < np.std(u) < 60.0


# ---- closed forms on the oracle ------------------------------------------------------------------------------------------------
def test_target_equal_to_the_base_is_one_stage_with_log_evidence_zero():
    d, n = 5, 64
    loc, scale = np.zeros(d), np.ones(d)

    def vg(x):
        return SO.log_base(x, loc, scale), -(x - loc) / scale ** 2
    res = SO.run(vg, loc, scale, SO.philox_normals(3, n, d), n_particles=n, seed=3)
    assert res['n_stages'] == 1 and np.array_equal(res['betas'], [1.0])
    assert res['log_evidence'] == 0.0 and res['ess'][0] == n


def test_one_particle_is_one_stage_with_its_own_weight():
    host, _ = HO.parity_problem('logistic', 2)
    loc, scale = np.array([0.5, -1.0]), np.array([1.5, 0.7])
    normals = SO.philox_normals(4, 1, 2)
    res = SO.run(HO.value_and_grad_of(host), loc, scale, normals, n_particles=1, seed=4, n_moves=1, n_leapfrog=2)
    z = normals(0)
    u0 = host.logp(loc + scale * z)[0] - SO.log_base_from_z(z, scale)[0]
    assert res['n_stages'] == 1 and res['betas'][-1] == 1.0
    assert res['log_evidence'] == u0
    assert np.array_equal(res['ancestors'], [[0]])


def test_numeric_errors():
    for u in ([0.0, np.nan], [0.0, np.inf], [-np.inf, -np.inf]):
        with pytest.raises(SO.SmcNumericError):
            SO.reweight(np.array(u), 0.0, 0.5, 0.5)
    with pytest.raises(SO.SmcNumericError):                          # one particle in ten on the support: delta = 0
        SO.reweight(np.where(np.arange(10) == 3, 0.0, -np.inf), 0.0, 0.5, 0.5)
    host, _ = HO.parity_problem('gauss', 2)
    case = SO.parity_cases('gauss', 64)[4]
    with pytest.raises(SO.SmcNumericError):
        SO.run_case(host, case, SO.philox_normals(case['seed'], 64, case['d']), max_stages=1)


# ---- the resampler ----------------------------------------------------------------------------------------------------------------
def _weights():
    rng = np.random.RandomState(7)
    out = []
    for n in (1, 2, 3, 64, 257, 1000):
        out.append(rng.rand(n))
        out.append(np.exp(30.0 * rng.randn(n)))                      # a few particles carry everything
        w = np.zeros(n)
        w[rng.randint(n)] = 1.0
        out.append(w)                                                # one particle
        out.append(np.ones(n))
        out.append(np.where(rng.rand(n) < 0.5, 0.0, rng.rand(n)) + np.where(np.arange(n) == n // 2, 1e-300, 0.0))
        out.append(np.concatenate([np.full(n - 1, 1e-17), [1.0]]))   # increments lost in the prefix sums' rounding
    return out


def test_resampler_properties():
    rng = np.random.RandomState(8)
    for w in _weights():
        n = w.size
        # (U stays 2^-40 below 1: (n - 1 + U) / n must not round to 1.0, where the clamp to n - 1 would take over)
        for uniform in (0.0, 0.5, rng.rand(), 1.0 - 2.0 ** -40):
            anc, _ = SO.systematic(w, uniform)
            assert anc.shape == (n,) and anc.min() >= 0 and anc.max() <= n - 1
            assert np.all(np.diff(anc) >= 0)
            counts = np.bincount(anc, minlength=n)
            expect = n * (w / np.cumsum(w)[-1])
            # floor or ceil of n w~_i, up to the rounding of the prefix sums (relative 1e-12 of n)
            assert np.all(counts >= np.floor(expect - 1e-12 * n)) and np.all(counts <= np.ceil(expect + 1e-12 * n))
            assert not np.any(counts[w == 0.0])
    anc, _ = SO.systematic(np.ones(7), 0.5)
    assert np.array_equal(anc, np.arange(7))


# ---- the statistical test's constants -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['a', 'b'])
def test_stat_constants_and_the_test_seed(name):
    rows = np.array(SO.STAT_ORACLE[name])
    assert rows.shape == (len(SO.STAT_SEEDS), 3) and len(SO.STAT_SEEDS) == 8
    bounds = SO.stat_bounds(name)
    assert bounds[0] == 4.0 * np.std(rows[:, 0], ddof=1) and bounds[1] == 4.0 * rows[:, 1].max()
    seed = SO.STAT_TEST_SEED[name]
    _, fig = SO.stat_run(name, seed)
    print(name, fig, bounds)
    if seed in SO.STAT_SEEDS:      # the table is this function's output
        np.testing.assert_allclose(fig, rows[SO.STAT_SEEDS.index(seed)], rtol=1e-6)
    assert abs(fig[0]) <= bounds[0] and fig[1] <= bounds[1] and fig[2] <= bounds[2]


def test_perturbation_yardstick_is_small():
    case = SO.parity_cases('logistic', 64)[-1]
    host, _ = HO.parity_problem('logistic', case['d'])
    normals = SO.philox_normals(case['seed'], 64, case['d'])
    ref = SO.run_case(host, case, normals)
    pert = SO.run_case(host, case, normals, perturb=np.random.RandomState(1))
    assert np.array_equal(ref['ancestors'], pert['ancestors']) and np.array_equal(ref['n_accepted'], pert['n_accepted'])
    tol = SO.tolerances(ref, pert)
    assert 0.0 < tol['particles'] < 1e-6 and SO.BETA_SLACK <= tol['betas'] < 1e-6


# ---- smc(): argument checks, exports, the header --------------------------------------------------------------------------------------
def test_smc_argument_checks_raise_before_an_engine_is_touched(monkeypatch):
    def no_engine():
        raise AssertionError('the engine was touched')
    monkeypatch.setattr(_lib, 'default_engine', no_engine)
    model = vb.GaussianModel(np.zeros(3), np.ones(3))
    ok = dict(n_particles=8, loc=np.zeros(3), scale=np.ones(3))
    with pytest.raises(TypeError):
        vb.smc(lambda x: x, **ok)
    with pytest.raises(NotImplementedError):
        vb.smc(vb.CallableModel(3, lambda x: -0.5 * np.sum(x * x, axis=1), lambda x: -x), **ok)
    X = np.random.RandomState(0).randn(20, 3)
    with pytest.raises(NotImplementedError):
        vb.smc(vb.MinibatchRegressionModel(X, (X[:, 0] > 0).astype(float), 5), **ok)
    with pytest.raises(ValueError):
        vb.smc(model, n_particles=8)                                     # neither a base nor a fit
    with pytest.raises(ValueError):
        vb.smc(model, n_particles=8, loc=np.zeros(3))                    # loc without scale
    with pytest.raises(ValueError):
        vb.smc(model, n_particles=8, var_param=np.zeros(6))              # var_param without approx
    for bad in (dict(n_particles=0), dict(n_particles=2.5), dict(n_particles=True), dict(n_moves=0), dict(n_leapfrog=0),
                dict(max_stages=0), dict(ess_target=0.0), dict(ess_target=1.0), dict(ess_target=np.nan),
                dict(target_accept=0.0), dict(target_accept=1.0), dict(adapt_rate=-0.1), dict(adapt_rate=np.inf),
                dict(step_size=0.0), dict(step_size=np.inf), dict(seed=-1), dict(stream_offset=-1),
                dict(loc=np.zeros(2)), dict(loc=np.array([0.0, np.nan, 0.0])), dict(scale=np.ones(4)),
                dict(scale=np.array([1.0, 0.0, 1.0])), dict(scale=np.array([1.0, np.inf, 1.0]))):
        with pytest.raises(ValueError):
            vb.smc(model, **dict(ok, **bad))


def test_exports_and_defaults():
    import sys
    assert callable(vb.smc) and vb.smc is sys.modules['viabel_amd.smc'].smc
    assert sys.modules['viabel_amd.smc'].__all__ == ['smc']
    for name in ('smc_reweight', 'smc_run'):
        assert callable(getattr(_lib.Engine, name))
    assert vb.smc.__kwdefaults__ == dict(n_particles=1024, var_param=None, approx=None, loc=None, scale=None, ess_target=0.5,
                                         n_moves=2, n_leapfrog=8, step_size=None, target_accept=0.8, adapt_rate=0.5,
                                         max_stages=200, seed=1, stream_offset=0, keep_ancestors=False)
    assert 'not the fit itself' in vb.smc.__doc__.lower()


def test_header_declares_both_entries():
    header = open(os.path.join(ROOT, 'include', 'viabel_hip.h')).read()
    assert 'int vb_smc_reweight(vb_ctx* ctx' in header and 'int vb_smc_run(vb_ctx* ctx' in header
    for name, n_args in (('vb_smc_reweight', 8), ('vb_smc_run', 28)):
        restype, argtypes = _lib.SIGNATURES[name]
        assert argtypes[0] is _lib._ctx_p and len(argtypes) == n_args
    lib = _lib.load()
    for name in ('vb_smc_reweight', 'vb_smc_run'):
        argtypes = _lib.SIGNATURES[name][1]
        zeros = [None if t in (_lib._ctx_p, _lib._c_double_p, _lib._c_int64_p) else 0 for t in argtypes]
        assert getattr(lib, name)(*zeros) == _lib.VB_ERR_INVALID
    assert 'vb_smc.hip' in open(os.path.join(ROOT, 'viabel_amd', 'csrc', 'Makefile')).read()


def test_hmc_shares_its_argument_checks():
    import sys
    mcmc, smc = sys.modules['viabel_amd.mcmc'], sys.modules['viabel_amd.smc']
    for name in ('_require_device_target', '_require_integers', '_require_open_unit', '_require_fit_pair', '_resolve_step_size'):
        assert getattr(smc, name) is getattr(mcmc, name)
