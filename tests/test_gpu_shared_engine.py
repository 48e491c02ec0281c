"""GPU: objectives of different kinds taking turns on ONE engine.

Every objective of a process runs on the engine of ``_lib.default_engine()`` unless the caller gives it another one, and that
engine keeps state between calls: the noise slots, one DIS state per family kind with its generation counter, the Philox
look-ahead shadows, the look-ahead job of numpy's streams, the flows' device copies.  The reference keeps all of this per
object (``viabel/objectives.py:391-403``), so two of its objectives that take turns never see each other's state.  Here every
subject below is run alone, and then in turn with every other subject (and in triples that make DIS states park across
kinds): each objective's values and gradients must be EXACTLY what it computes alone -- the engine's reductions run in a
fixed order -- or, where an interleaving cannot be served, the call raises an ``EngineError`` that names the remedy.  Never
another number.  The anchor at the end compares interleaved runs with the oracle, so the numbers are the reference's and not
merely repeatable ones."""
import gc
import itertools

import numpy as np
import pytest

import _golden as G
from _engine_subjects import CALLS, D, N, SUBJECTS, Runner, _fresh_engine, _problem
from oracle import families as ofam
from oracle import models as omod
from oracle import objectives as oobj

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def vb():
    import viabel_amd
    from viabel_amd import _lib
    _lib.default_engine()
    return viabel_amd


@pytest.fixture
def engine(vb):
    with _fresh_engine() as eng:
        yield eng


_SOLO = {}


def solo(vb, sid, variant=0, d=D, n=N):
    key = (sid, variant, d, n)
    if key not in _SOLO:
        with _fresh_engine():
            r = Runner(vb, sid, variant, d, n)
            for _ in range(CALLS):
                r.step()
            _SOLO[key] = r.out
            del r
    return _SOLO[key]


def _same(want, got, label):
    assert len(want) == len(got), label
    for i, ((v0, g0), (v1, g1)) in enumerate(zip(want, got)):
        assert v0 == v1, (label, i, v0, v1)
        np.testing.assert_array_equal(g0, g1, err_msg='{} call {}'.format(label, i))


def _turns(runners):
    for _ in range(CALLS):
        for r in runners:
            r.step()


@pytest.mark.parametrize('a,b', list(itertools.permutations(SUBJECTS, 2)))
def test_pair_takes_turns_on_one_engine(vb, engine, a, b):
    """A's calls, one call of B after each: both exactly as alone."""
    want_a, want_b = solo(vb, a), solo(vb, b)
    ra, rb = Runner(vb, a), Runner(vb, b)
    _turns([ra, rb])
    _same(want_a, ra.out, a)
    _same(want_b, rb.out, b)


@pytest.mark.parametrize('a,c', [('dis_mf_np', 'dis_fr_px'), ('dis_fr_px', 'dis_mf_np'), ('dis_lr', 'dis_mf_np'),
                                 ('dis_mvt_np', 'dis_mft_px'), ('dis_mft_px', 'dis_lr'), ('dis_mf_np', 'dis_mvt_np')])
def test_triple_parks_states_across_kinds(vb, engine, a, c):
    """Two kept-weights objectives of one kind (their states park and come back) and one of another kind, in turn."""
    want = [solo(vb, a), solo(vb, a, 1), solo(vb, c)]
    runners = [Runner(vb, a), Runner(vb, a, 1), Runner(vb, c)]
    _turns(runners)
    for w, r, label in zip(want, runners, (a, a + "'", c)):
        _same(w, r.out, label)


@pytest.mark.parametrize('a,b', [('dis_mf_np', 'dis_fr_px'), ('dis_mf_np', 'dis_lr'), ('dis_mf_np', 'dis_mf_np'),
                                 ('dis_fr_px', 'dis_mf_np'), ('dis_mvt_np', 'dis_mvt_np'), ('dis_lr', 'dis_lr'),
                                 ('ekl_mvt_np', 'dis_mvt_np'), ('dis_mvt_np', 'ekl_mvt_np'), ('dis_mft_px', 'ekl_mf_px')])
def test_shape_mismatch_is_exact_or_refused(vb, a, b):
    """B has another dimension and more samples: A and B compute what they compute alone, or the call raises an
    EngineError that tells the user to give each objective its own engine -- never another number, never a crash.  The
    second partner shape is ragged (d2 = 37: pad columns up to the row stride of 48, which it shares with D): a refusal
    there must not stand in for a wrong number, so a pair refused at the ragged shape must be refused at (32, 6000) too."""
    from viabel_amd import _lib
    refused = {}
    for d2, n2 in [(32, 6000), (37, 4099)]:
        want_a, want_b = solo(vb, a), solo(vb, b, 0, d2, n2)
        with _fresh_engine():
            ra, rb = Runner(vb, a), Runner(vb, b, 0, d2, n2)
            try:
                _turns([ra, rb])
                refused[d2] = False
            except _lib.EngineError as e:
                assert 'own engine' in str(e), str(e)
                refused[d2] = True
            _same(want_a[:len(ra.out)], ra.out, (a, d2, n2))
            _same(want_b[:len(rb.out)], rb.out, (b, d2, n2))
            del ra, rb
            gc.collect()
    assert refused[32] or not refused[37], 'refused at (37, 4099) but served at (32, 6000)'


@pytest.mark.parametrize('partner', ['dis_fr_px', 'dis_lr'])
def test_meanfield_dis_interleaved_against_oracle(vb, engine, partner):
    """dis_mf_np with a dense / low-rank DIS refreshing in between, step by step against the oracle: on refresh steps
    the oracle draws the family's own normals, the resampling indices come from the same global-generator state."""
    model_mean, model_sd, _, _, prior = _problem(D)
    ra, rb = Runner(vb, 'dis_mf_np'), Runner(vb, partner)
    ofamily = ofam.MFGaussian(D)
    ref = oobj.DISInclusiveKL(ofamily, omod.GaussDiag(model_mean, model_sd), N, N // 6, ofam.MFGaussian(D), prior,
                              use_resampling=True, num_resampling_batches=3)
    rs = np.random.RandomState(1)           # the family's generator (seed 1)
    for step in range(CALLS):
        theta, state = ra.th.copy(), ra.state
        ra.step()
        value, grad = ra.out[-1]
        np.random.set_state(state)
        if ref.needs_refresh():
            ref.refresh(theta, ofamily.draw_noise(rs, N))
        idx = np.random.choice(N, size=ref._resampling_batch_size, p=ref._state_w_normalized)
        ref._objective_step += 1
        xs = ref._state_samples[idx]
        scale = ref._state_w_sum / N
        ov = np.mean(-ofamily.log_density(theta, xs)) * scale
        og = -ofamily.log_density_grad_weighted(theta, xs, np.ones(len(idx))) / len(idx) * scale
        assert G.rel_err(ra.obj._eps, ref._eps) < 1e-10, step
        assert G.rel_err(value, ov) < 1e-10, (step, value, ov)
        assert G.rel_err(grad, og) < 1e-9, (step, G.rel_err(grad, og))
        rb.step()
