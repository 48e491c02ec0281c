"""GPU: the device-resident iterate chain (csrc/vb_chain.hip) and its statistics against the host's ``_chain_stats``.

The yardstick is ``viabel_amd._chain_stats`` (numpy; itself pinned to the reference by tests/golden/chainstats.npz).

Inputs: seeded AR(1) chains ``x[t] = phi x[t-1] + e[t]`` drawn in order from one ``RandomState(7)``, shifted and scaled to
``3 + 1e-2 x`` (|mean| / sd of a few hundred, like converged iterates), uploaded with ``chain_append``.

Tolerances.  R-hat: relative 1e-11 -- a two-pass / Chan accumulation over <= 2 048 rows is good to about n eps = 2e-13 on
the variances, which leaves a factor of about 50.  ESS and MCSE: relative 1e-10 -- autocovariance sums of <= 2 048 terms are
good to about 2e-13 and the pair sums add <= 710 of them.  A column may be left out of the ESS comparison only when one of
the pair sums the HOST examined, up to and including its stopping pair, is below 1e-8 in magnitude (there a rounding-level
difference may move the truncation), and at most 1 % of a case's columns; on these inputs the host leaves out none (the
smallest examined pair sum is 6.6e-7).  The means are compared with ``array_equal``."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import viabel_amd as vb  # noqa: E402
from viabel_amd import _chain_stats as cs, _lib, optimization as opt  # noqa: E402

CASES = [(200, 1500, 0.9), (1000, 600, 0.97), (513, 800, 0.5), (2048, 200, 0.99)]
RHAT_TOL = 1e-11
ESS_TOL = 1e-10


def _chains():
    rs = np.random.RandomState(7)
    out = []
    for w, p, phi in CASES:
        e = rs.randn(w, p)
        x = np.empty_like(e)
        x[0] = e[0]
        for t in range(1, w):
            x[t] = phi * x[t - 1] + e[t]
        out.append(3.0 + 1e-2 * x)
    return out


CHAINS = _chains()


@pytest.fixture
def eng():
    engine = _lib.default_engine()
    engine.chain_close()
    yield engine
    engine.chain_close()


def _upload(eng, chain, capacity=None):
    eng.chain_open(chain.shape[1], chain.shape[0] if capacity is None else capacity)
    eng.chain_append(chain)
    assert eng.chain_rows() == chain.shape[0]


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b)))


def _host_smallest_examined_pair_sum(col):
    """min |pair sum| over the pairs ``_chain_stats.ess`` looks at for this column (its stopping pair included)."""
    n = col.size
    acov = cs.autocov(col[np.newaxis, :], axis=1).mean(axis=0)
    chain_var = acov[0] * n / (n - 1.0)
    var_plus = chain_var * (n - 1.0) / n
    r = 1.0 - (chain_var - acov) / var_plus
    r[0] = 1.0
    last_pair = max((n - 3) // 2, 0)
    pair_sum = r[0:2 * last_pair + 1:2] + r[1:2 * last_pair + 2:2]
    stop = np.flatnonzero(pair_sum <= 0)
    jl = int(stop[0]) if stop.size else last_pair
    return float(np.min(np.abs(pair_sum[:jl + 1])))


@pytest.mark.parametrize('case', range(len(CASES)), ids=lambda i: 'w%d_p%d' % CASES[i][:2])
def test_chain_mean_is_numpys(eng, case):
    chain = CHAINS[case]
    rows = chain.shape[0]
    _upload(eng, chain)
    for w in (1, 2, 7, 8, 9, 10, rows // 2, rows - 1, rows):
        np.testing.assert_array_equal(eng.chain_mean(w), np.mean(chain[-w:], axis=0), err_msg='w = %d' % w)
    np.testing.assert_array_equal(eng.chain_fetch(3, 5), chain[3:8])


@pytest.mark.parametrize('case', range(len(CASES)), ids=lambda i: 'w%d_p%d' % CASES[i][:2])
def test_chain_rhat_matches_compute_R_hat(eng, case):
    chain = CHAINS[case]
    rows = chain.shape[0]
    _upload(eng, chain)
    W_min = 100
    search = np.linspace(W_min, int(0.95 * rows), 5, dtype=int)
    windows = list(search) + [rows - 1 if (rows - 1) % 2 else rows - 2, 4]
    assert windows[-2] % 2 == 1
    worst, rhat = eng.chain_rhat(windows, per_column=True)
    errs = []
    for i, w in enumerate(windows):
        ref = cs.compute_R_hat(chain[-w:])
        errs.append(_rel(rhat[i], ref))
        assert worst[i] == np.max(rhat[i])
        assert abs(worst[i] - np.max(ref)) <= RHAT_TOL * np.max(ref)
    print('chain_rhat case %s: largest relative error %.3g' % (CASES[case], max(errs)))
    assert max(errs) <= RHAT_TOL, errs
    np.testing.assert_array_equal(eng.chain_rhat(windows), worst)
    host = [cs.R_hat_convergence_check(list(chain), search, t) for t in (1.1, 1.01, 1.5)]
    dev = [cs.device_R_hat_convergence_check(eng, search, t) for t in (1.1, 1.01, 1.5)]
    assert [(bool(a), int(b)) for a, b in dev] == [(bool(a), int(b)) for a, b in host]


@pytest.mark.parametrize('case', range(len(CASES)), ids=lambda i: 'w%d_p%d' % CASES[i][:2])
def test_chain_ess_mcse_matches_MCSE(eng, case):
    chain = CHAINS[case]
    rows, p = chain.shape
    _upload(eng, chain)
    for w in (rows, rows - 37):
        ess, mcse = eng.chain_ess_mcse(w)
        ref_ess, ref_mcse = cs.MCSE(chain[-w:])
        ref_ess = np.asarray(ref_ess)
        err = np.maximum(np.abs(ess - ref_ess) / ref_ess, np.abs(mcse - ref_mcse) / ref_mcse)
        off = np.flatnonzero(~(err <= ESS_TOL))
        excused = [j for j in off if _host_smallest_examined_pair_sum(chain[-w:, j]) < 1e-8]
        print('chain_ess_mcse case %s w = %d: largest relative error %.3g over %d columns, %d left out'
              % (CASES[case], w, np.max(np.delete(err, excused)), p - len(excused), len(excused)))
        assert len(excused) == len(off), (off, err[off])
        assert len(excused) <= p // 100


def test_edge_cases(eng):
    rs = np.random.RandomState(11)
    for p in (1, 63, 65):
        chain = 0.5 + 1e-3 * np.cumsum(rs.randn(300, p), axis=0) * 0.05 + 1e-3 * rs.randn(300, p)
        if p > 1:
            chain[:, p // 2] = 0.75      # a constant column
        _upload(eng, chain)
        for w in (300, 299, 4, 3):
            ess, mcse = eng.chain_ess_mcse(w)
            ref_ess, ref_mcse = cs.MCSE(chain[-w:])
            live = np.ones(p, dtype=bool)
            if p > 1:
                live[p // 2] = False
                assert np.isnan(ess[p // 2]) and np.isnan(mcse[p // 2]) and np.isnan(ref_ess[p // 2])
            np.testing.assert_allclose(ess[live], np.asarray(ref_ess)[live], rtol=ESS_TOL, atol=0)
            np.testing.assert_allclose(mcse[live], ref_mcse[live], rtol=ESS_TOL, atol=0)
            again = eng.chain_ess_mcse(w)
            np.testing.assert_array_equal(again[0], ess)
            np.testing.assert_array_equal(again[1], mcse)
        windows = [300, 151, 4]
        worst, rhat = eng.chain_rhat(windows, per_column=True)
        assert np.isfinite(rhat).all()
        for i, w in enumerate(windows):
            np.testing.assert_allclose(rhat[i], cs.compute_R_hat(chain[-w:]), rtol=RHAT_TOL, atol=0)
        worst2, rhat2 = eng.chain_rhat(windows, per_column=True)
        np.testing.assert_array_equal(worst2, worst)
        np.testing.assert_array_equal(rhat2, rhat)
        np.testing.assert_array_equal(eng.chain_mean(300), np.mean(chain, axis=0))
        eng.chain_close()


def test_single_column_mean_is_numpys_pairwise_sum(eng):
    """With one column the reduced axis is contiguous: numpy adds runs of 8192 values pairwise, not row by row."""
    chain = 3.0 + 1e-2 * np.random.RandomState(2).randn(70001, 1)
    _upload(eng, chain)
    for w in (1, 7, 8, 9, 127, 128, 129, 300, 1000, 8191, 8192, 8193, 20000, 70000, 70001):
        np.testing.assert_array_equal(eng.chain_mean(w), np.mean(chain[-w:], axis=0), err_msg='w = %d' % w)


def test_rhat_max_propagates_nan(eng):
    chain = CHAINS[0][:, :130].copy()
    chain[-1, 77] = np.nan
    _upload(eng, chain)
    worst, rhat = eng.chain_rhat([100, 51], per_column=True)
    assert np.isnan(worst[0]) and np.isnan(rhat[0, 77]) and np.isfinite(np.delete(rhat[0], 77)).all()
    # the odd window drops its last row, the NaN with it
    assert np.isfinite(worst[1]) and worst[1] == np.max(cs.compute_R_hat(chain[-51:]))


def test_rows_split_over_workgroups_is_reproducible(eng):
    """Few columns and many rows: the rows of a half go to several workgroups, whose partials are merged in a fixed order."""
    rs = np.random.RandomState(3)
    chain = 3.0 + 1e-2 * rs.randn(6000, 70)
    _upload(eng, chain)
    windows = [6000, 5999, 3000, 600]
    worst, rhat = eng.chain_rhat(windows, per_column=True)
    for i, w in enumerate(windows):
        np.testing.assert_allclose(rhat[i], cs.compute_R_hat(chain[-w:]), rtol=RHAT_TOL, atol=0)
    for _ in range(3):
        worst2, rhat2 = eng.chain_rhat(windows, per_column=True)
        np.testing.assert_array_equal(rhat2, rhat)
        np.testing.assert_array_equal(worst2, worst)


def _mf_problem():
    D = 24
    return (lambda: vb.ExclusiveKL(vb.MFGaussian(D, seed=3, rng='philox'), vb.FunnelModel(D), 64),
            np.concatenate([np.zeros(D), -np.ones(D)]), False)


def _fullrank_problem():
    D = 256        # rows of 265 KB: logged gradients leave through the pinned ring while the iterates go to the chain
    rng = np.random.RandomState(1)
    mean, sd = rng.randn(D), np.exp(0.2 * rng.randn(D))
    fr = vb.FullRankGaussian(D)
    return (lambda: vb.ExclusiveKL(vb.FullRankGaussian(D, seed=2, rng='philox'), vb.GaussianModel(mean, sd), 32),
            fr.pack(np.zeros(D), np.exp(-1.0) * np.eye(D)), True)


def _flow_problem():
    from test_gpu_nvp_flow import make_flow, make_model
    D = 17

    def make():
        return vb.ExclusiveKL(make_flow(D, 3, [33, 10], [10, 33], 'gauss', 'philox', prior_scale=0.1),
                              make_model('funnel', D), 100)
    flow = make_flow(D, 3, [33, 10], [10, 33], 'gauss', 'philox')
    return make, 0.1 * np.random.RandomState(0).randn(flow.var_param_dim), False


@pytest.mark.parametrize('problem', [_mf_problem, _fullrank_problem, _flow_problem], ids=['meanfield', 'fullrank', 'nvp'])
def test_device_fit_fills_the_chain(eng, problem):
    """Two legs of a device fit with an open chain leave, row for row, the iterates a twin fit returns as its history."""
    make, init, with_grads = problem()
    legs = (13, 9)
    outs = []
    for chained in (True, False):
        obj, sgo = make(), opt.RMSProp(0.01)
        p = init.size
        if chained:
            eng.chain_open(p, sum(legs) + 2)
        theta, rows = init, []
        for n in legs:
            theta, values, hist, state, _, grads = obj.device_fit(
                n, theta, sgo._device_kind, sgo._device_hyper(), state=sgo._device_state(p),
                hist_len=0 if chained else n, log_gradients=with_grads)
            sgo._set_device_state(state, p)
            rows.append((values, hist, grads))
        if chained:
            assert eng.chain_rows() == sum(legs)
            assert all(h.shape == (0, p) for _, h, _ in rows)
            history = eng.chain_fetch(0, sum(legs))
            mean = np.array(eng.chain_mean(sum(legs)))
            eng.chain_close()
        else:
            history = np.concatenate([h for _, h, _ in rows])
            mean = np.mean(history, axis=0)
        outs.append((theta, np.concatenate([v for v, _, _ in rows]), history, mean,
                     np.concatenate([g for _, _, g in rows]) if with_grads else None))
    for a, b in zip(outs[0], outs[1]):
        if b is not None:
            np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(outs[0][2][-1], outs[0][0])      # the last row is the returned parameter


def test_argument_errors(eng):
    chain = CHAINS[0][:, :40]
    with pytest.raises(_lib.EngineError):       # no open chain
        eng.chain_rows()
    for call in (lambda: eng.chain_mean(1), lambda: eng.chain_rhat([4]), lambda: eng.chain_ess_mcse(4),
                 lambda: eng.chain_append(chain), lambda: eng.chain_fetch(0, 1)):
        with pytest.raises(_lib.EngineError):
            call()
    _upload(eng, chain, capacity=chain.shape[0] + 10)
    with pytest.raises(_lib.EngineError):       # a second chain
        eng.chain_open(3, 3)
    rows = chain.shape[0]
    for call in (lambda: eng.chain_mean(rows + 1), lambda: eng.chain_rhat([100, rows + 1]),
                 lambda: eng.chain_ess_mcse(rows + 1), lambda: eng.chain_mean(0), lambda: eng.chain_rhat([1]),
                 lambda: eng.chain_rhat(list(range(4, 40))), lambda: eng.chain_fetch(rows - 1, 2),
                 lambda: eng.chain_append(chain[:11]),                  # beyond the capacity
                 lambda: eng.chain_append(CHAINS[0][:2, :41])):         # the wrong p
        with pytest.raises(ValueError):
            call()
    assert eng.chain_rows() == rows
    make, init, _ = _mf_problem()
    obj, sgo = make(), opt.RMSProp(0.01)
    fit = lambda n, x0, **kw: obj.device_fit(n, x0, sgo._device_kind, sgo._device_hyper(), **kw)       # noqa: E731
    with pytest.raises(ValueError, match='chain'):       # the wrong p: the chain holds rows of 40, the fit's has 48
        fit(5, init)
    eng.chain_close()
    eng.chain_open(init.size, 8)
    with pytest.raises(ValueError, match='room'):        # capacity exceeded by a fit
        fit(9, init)
    with pytest.raises(ValueError, match='hist_len'):    # a history asked for while the chain is open
        fit(5, init, hist_len=5)
    assert eng.chain_rows() == 0
    fit(8, init)
    assert eng.chain_rows() == 8
    with pytest.raises(ValueError, match='room'):
        fit(1, init)
    eng.chain_close()
    with pytest.raises(ValueError, match='overflow'):    # p x capacity x 8 does not fit 63 bits
        eng.chain_open(1 << 40, 1 << 40)
    with pytest.raises(_lib.EngineError, match=str(1 << 48)):      # 256 TiB: the allocation is refused, with its size
        eng.chain_open(1 << 20, 1 << 25)
    # ... and the engine is none the worse for it
    _upload(eng, chain)
    np.testing.assert_array_equal(eng.chain_mean(rows), np.mean(chain, axis=0))
    # without a chain a fit behaves as ever
    eng.chain_close()
    theta, values, hist, _, _, _ = fit(5, init, hist_len=5)
    assert hist.shape == (5, init.size)
    np.testing.assert_array_equal(hist[-1], theta)
