"""GPU: everything an engine allocates is released with it.

Every device buffer, page-locked block, event and stream of the engine is held by an owning type
(``viabel_amd/csrc/vb_resource.h``), and the library counts the live ones (``_lib.resource_counts()``).  Free memory as the
runtime reports it is device-wide -- on a GPU that others use it moves by itself -- so the counts are the way to see a
release: an engine that has run every kind of work the binding offers, with every buffer grown once, leaves them exactly
where they stood before it was made.  A DIS state parked by its objective owns its buffers and outlives the engine."""
import gc

import numpy as np
import pytest

from _engine_subjects import D, N, SUBJECTS, Runner, _fresh_engine, _problem

pytestmark = pytest.mark.gpu

GAUSS_SRC = ('__device__ double vb_log_density(const double* z, int d, const double*, double* g) {'
             ' double f = 0; for (int j = 0; j < d; ++j) { f -= 0.5 * z[j] * z[j]; if (g) g[j] = -z[j]; } return f; }')


@pytest.fixture(scope='module')
def vb():
    import viabel_amd
    from viabel_amd import _lib
    _lib.default_engine()       # (made before any baseline is read: it stays alive behind the fresh engines)
    return viabel_amd


def _exercise(vb, eng, monkeypatch):
    """One call of everything that allocates; the objects that keep engine state alive are returned."""
    from viabel_amd import _lib
    held = []
    for n in (64, N):           # small first: the second call makes every buffer and pinned block grow
        for sid in SUBJECTS:
            held.append(Runner(vb, sid, 0, D, n))
            held[-1].step()
    model_mean, model_sd, _, th_mf, _ = _problem(D)
    # a PSIS smoothing
    smoothed, khat = eng.psis_smooth(N, np.random.RandomState(5).standard_t(3.0, N))
    assert np.isfinite(smoothed).all() and np.isfinite(khat)
    # a target compiled from source, and one that is a host callable
    for model in (vb.SourceModel(D, GAUSS_SRC), vb.CallableModel(D, value_and_grad=lambda z: (-0.5 * (z * z).sum(axis=1), -z))):
        for n in (64, N):
            value, grad = vb.ExclusiveKL(vb.MFGaussian(D, seed=2, rng='philox'), model, n)(th_mf)
            assert np.isfinite(value) and np.isfinite(grad).all()
    # a device fit whose rows leave through the copy stream and the pinned ring (forced for these short rows)
    monkeypatch.setenv('VB_FIT_STREAM_ROWS', '1')
    monkeypatch.setenv('VB_FIT_STREAM_MIN_BYTES', '0')
    for d in (12, D):
        rng = np.random.RandomState(3)
        eng.set_model(vb.GaussianModel(rng.randn(d), np.exp(0.2 * rng.randn(d))).device_spec())
        out = eng.fit(4, 40, d, _lib.FAMILY_MF_GAUSSIAN, np.concatenate([np.zeros(d), -np.ones(d)]), 6, _lib.OPT_RMSPROP,
                      [0.01, 0.9, 0.0, 1e-8], seed=9, hist_len=4, log_directions=True, log_gradients=True)
        assert out[2].shape == (4, 2 * d) and np.isfinite(out[2]).all()
    # an iterate chain: opened, filled, closed -- and a larger one left open for the engine to release
    eng.chain_open(5, 8)
    eng.chain_append(np.ones((3, 5)))
    eng.chain_close()
    eng.chain_open(7, 64)
    eng.chain_append(np.ones((2, 7)))
    # profiling events
    eng.profile_enable(True)
    held[SUBJECTS.index('ekl_mf_px')].step()
    eng.profile_enable(False)
    # two kept-weights DIS objectives of one kind taking turns: the first one's state is parked
    pair = [Runner(vb, 'dis_mf_np'), Runner(vb, 'dis_mf_np', 1)]
    for _ in range(2):
        for r in pair:
            r.step()
    assert pair[0].obj._parked is not None or pair[1].obj._parked is not None
    return held + pair


def _cycle(vb, monkeypatch):
    from viabel_amd import _lib
    base = _lib.resource_counts()
    with _fresh_engine() as eng:
        held = _exercise(vb, eng, monkeypatch)
        live = _lib.resource_counts()
        assert all(now > before for now, before in zip(live, base)), (base, live)       # the counters are wired
        del held
        gc.collect()
    assert _lib.resource_counts() == base


def test_engine_releases_everything_it_allocated(vb, monkeypatch):
    _cycle(vb, monkeypatch)
    _cycle(vb, monkeypatch)         # ... and again: nothing of the first engine is needed by, or left to, the second


def test_parked_dis_state_outlives_the_engine(vb):
    from viabel_amd import _lib
    base = _lib.resource_counts()
    with _fresh_engine():
        first, second = Runner(vb, 'dis_mf_np', 0, D, 64), Runner(vb, 'dis_mf_np', 1, D, 64)
        first.step()
        second.step()               # refreshes over the first one's kept state: that state is parked
        assert first.obj._parked is not None
        del second
        gc.collect()
    after_close = _lib.resource_counts()
    assert after_close[0] > base[0] and after_close[1:] == base[1:], (base, after_close)   # the handle's buffers alone
    del first
    gc.collect()
    assert _lib.resource_counts() == base
