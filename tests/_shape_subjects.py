"""The subjects of ``test_gpu_shape_sequences.py``: the ten of ``_engine_subjects`` and six more objectives that keep or
reuse engine buffers the ten do not reach, the solo runs they are compared with, and the oracle's value of a subject's
first call."""
import gc

import numpy as np

import _engine_subjects as ES
from _engine_subjects import Runner, _fresh_engine, _problem, lowrank_start
from oracle import families as ofam
from oracle import models as omod
from oracle import objectives as oobj

CALLS = 3
EXTRA = ['alpha_mvt_np', 'alpha_lr', 'dis_mvt_px', 'ekl_fr_px_pd', 'ekl_mf_np_loo', 'ekl_lr17']
SUBJECTS = ES.SUBJECTS + EXTRA
ANCHORED = [s for s in SUBJECTS if s.startswith(('ekl_', 'alpha_'))]


def make(vb, sid, variant=0, d=ES.D, n=ES.N, loud=False):
    if sid in ES.SUBJECTS:
        return ES.make(vb, sid, variant, d, n, loud)
    model_mean, model_sd, th_ch, th_mf, prior = _problem(d, loud)
    model = vb.GaussianModel(model_mean, model_sd)
    seed = 1 + 10 * variant
    if sid == 'alpha_mvt_np':
        return vb.AlphaDivergence(vb.MultivariateT(d, 9.0, seed=seed), model, n, 0.5), th_ch
    if sid == 'alpha_lr':
        fam = vb.LRGaussian(d, seed=seed, k=3)
        return vb.AlphaDivergence(fam, model, n, 0.5), lowrank_start(fam, d, 3, loud)
    if sid == 'dis_mvt_px':      # throughput mode: the factor algebra of the refresh stays on the device
        dis = dict(ess_target=n // 6, temper_prior=vb.MFGaussian(d), temper_prior_params=prior, use_resampling=True)
        return vb.DISInclusiveKL(vb.MultivariateT(d, 9.0, seed=seed, rng='philox'), model, n, num_resampling_batches=2,
                                 **dis), th_ch
    if sid == 'ekl_fr_px_pd':
        return vb.ExclusiveKL(vb.FullRankGaussian(d, seed=seed, rng='philox'), model, n, use_path_deriv=True), th_ch
    if sid == 'ekl_mf_np_loo':
        return vb.ExclusiveKL(vb.MFGaussian(d, seed=seed), model, n, hessian_approx_method='loo_diag_approx'), th_mf
    if sid == 'ekl_lr17':        # k > 16: the any-rank route, sums from GEMMs over the padded widths
        fam = vb.LRGaussian(d, seed=seed, k=17)
        return vb.ExclusiveKL(fam, model, n), lowrank_start(fam, d, 17, loud)
    raise ValueError(sid)


def np_seed(sid, variant=0, d=ES.D):
    return 1000 + 37 * SUBJECTS.index(sid) + 7 * variant + d


def runner(vb, sid, variant=0, d=ES.D, n=ES.N, loud=False):
    return Runner(vb, sid, variant, d, n, loud, make=make, np_seed=np_seed)


_SOLO = {}


def solo(vb, sid, d, n, loud=False):
    """`CALLS` calls of the subject as the first and only work of a fresh engine."""
    key = (sid, d, n, loud)
    if key not in _SOLO:
        with _fresh_engine():
            r = runner(vb, sid, 0, d, n, loud)
            for _ in range(CALLS):
                r.step()
            _SOLO[key] = r.out
            del r
            gc.collect()
    return _SOLO[key]


def same(want, got, label):
    assert len(want) == len(got), label
    for i, ((v0, g0), (v1, g1)) in enumerate(zip(want, got)):
        assert v0 == v1, (label, 'call', i, v0, v1)
        np.testing.assert_array_equal(g0, g1, err_msg='{} call {}'.format(label, i))


def run_sequence(vb, steps):
    """Each `(sid, d, n, loud)` of `steps` in order on ONE fresh engine: an objective makes its calls, is compared with its
    solo run and is deleted before the next one is made.  No call may be refused."""
    with _fresh_engine():
        for pos, (sid, d, n, loud) in enumerate(steps):
            want = solo(vb, sid, d, n, loud)
            r = runner(vb, sid, 0, d, n, loud)
            for _ in range(CALLS):
                r.step()
            out = r.out
            del r
            gc.collect()
            same(want, out, 'step {} of {}: {}@({}, {}){}'.format(pos, len(steps), sid, d, n, ' loud' if loud else ''))


def _philox_normals(n, d, seed):
    with _fresh_engine() as eng:
        eng.noise_generate(9, n, d, seed=seed, stream=0)
        return eng.noise_get_host(9, n, d)


def oracle_first_call(vb, sid, d, n):
    """`(value, grad, value scale, value tol, grad tol)` of the subject's first call from the oracle on the same draws.
    The tolerances are those of ``test_gpu_property.py`` for the family: value 1e-12 on the scale of its terms and
    gradient 1e-10 of max|grad|; control variates gradient 1e-9; alpha value 1e-11."""
    model_mean, model_sd, th_ch, th_mf, _ = _problem(d)
    omodel = omod.GaussDiag(model_mean, model_sd)
    draw_seed = int(np.random.RandomState(np_seed(sid, 0, d)).randint(2 ** 32))     # AlphaDivergence's (objectives.py:455)

    def terms(ofamily, th, noise, ov):
        z = ofamily.sample_from_noise(th, noise)
        return max(abs(ov), np.mean(np.abs(omodel.logp(z))), 1.0)

    if sid in ('ekl_mf_px', 'ekl_mf_np_loo'):
        of = ofam.MFGaussian(d)
        if sid == 'ekl_mf_px':
            noise = _philox_normals(n, d, 1)
            ov, og = oobj.exclusive_kl(of, omodel, th_mf, noise)
            return ov, og, terms(of, th_mf, noise, ov), 1e-12, 1e-10
        noise = np.random.RandomState(1).randn(n, d)
        ov, og = oobj.rge_reduced(of, omodel, th_mf, noise, 'loo_diag_approx')
        return ov, og, terms(of, th_mf, noise, ov), 1e-12, 1e-9
    if sid == 'ekl_mvt_np':
        of = ofam.MultivariateT(d, 9.0)
        noise = of.draw_noise(np.random.RandomState(1), n)
        ov, og = oobj.exclusive_kl(of, omodel, th_ch, noise, use_path_deriv=True)
        return ov, og, terms(of, th_ch, noise, ov), 1e-12, 1e-10
    if sid in ('ekl_lr', 'ekl_lr17'):
        k = 17 if sid == 'ekl_lr17' else 3
        of = ofam.LRGaussian(d, k)
        th = lowrank_start(vb.LRGaussian(d, k=k), d, k)
        noise = of.draw_noise(np.random.RandomState(1), n)
        ov, og = oobj.exclusive_kl(of, omodel, th, noise)
        return ov, og, max(abs(ov), 1.0), 1e-12, 1e-10
    if sid == 'ekl_fr_px_pd':
        of = ofam.FullRankGaussian(d)
        ov, og = oobj.exclusive_kl(of, omodel, th_ch, _philox_normals(n, d, 1), True)
        return ov, og, max(abs(ov), 1.0), 1e-12, 1e-10
    if sid == 'ekl_nvp':
        import _nvp_oracle as O
        with _fresh_engine():      # a twin flow whose fresh prior makes the draws the objective's first call consumed
            obj, th = make(vb, sid, 0, d, n)
            twin = obj.approx
            z0 = twin.prior_param[:d] + np.exp(twin.prior_param[d:]) * twin.prior._base_noise(n)
            ov, og = O.objective(twin, obj.model, th, z0, False)
            del obj, twin
            gc.collect()
        return ov, og, max(abs(ov), 1.0), 1e-12, 1e-10
    if sid == 'alpha_fr_px':
        ov, og = oobj.alpha_divergence(ofam.FullRankGaussian(d), omodel, th_ch, _philox_normals(n, d, draw_seed), 0.5)
        return ov, og, max(abs(ov), 1.0), 1e-11, 1e-10
    if sid == 'alpha_mvt_np':
        of = ofam.MultivariateT(d, 9.0)
        ov, og = oobj.alpha_divergence(of, omodel, th_ch, of.draw_noise(np.random.RandomState(draw_seed), n), 0.5)
        return ov, og, max(abs(ov), 1.0), 1e-11, 1e-10
    if sid == 'alpha_lr':
        of = ofam.LRGaussian(d, 3)
        th = lowrank_start(vb.LRGaussian(d, k=3), d, 3)
        ov, og = oobj.alpha_divergence(of, omodel, th, of.draw_noise(np.random.RandomState(draw_seed), n), 0.5)
        return ov, og, max(abs(ov), 1.0), 1e-11, 1e-10
    raise ValueError(sid)
