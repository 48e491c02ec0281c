"""The subjects of the shared-engine tests: one objective of every kind that keeps state in the engine between calls, the
problem they share, and a runner that gives each its own view of numpy's global generator.  Used by
``test_gpu_shared_engine.py`` (objectives taking turns compute what they compute alone) and by
``test_gpu_engine_resources.py`` (everything they make the engine allocate is released with it)."""
import contextlib

import numpy as np

from oracle import families as ofam

D, N = 48, 4200         # one shape for every subject: each cross-kind overwrite fits the shape checks
CALLS = 6

# DIS subjects keep weights between refreshes (num_resampling_batches > 1): kind 0 (mean-field), 1 (dense), 2 (low-rank)
SUBJECTS = ['dis_mf_np', 'dis_mft_px', 'dis_fr_px', 'dis_mvt_np', 'dis_lr',
            'ekl_mf_px', 'ekl_mvt_np', 'ekl_lr', 'ekl_nvp', 'alpha_fr_px']


@contextlib.contextmanager
def _fresh_engine():
    """A new engine as the process's default for the objectives made inside: every case (and every solo run) starts from
    an empty engine, so one case's leftovers cannot decide another's outcome."""
    from viabel_amd import _lib
    old, eng = _lib.default_engine(), _lib.Engine(0)
    _lib.set_default_engine(eng)
    try:
        yield eng
    finally:
        _lib.set_default_engine(old)
        eng.close()


LOUD_SHIFT, LOUD_SCALE = 1e3, 10.0


def _problem(d, loud=False):
    """`loud`: the same problem moved to LOUD_SHIFT and stretched by LOUD_SCALE (target, prior and parameters alike, so it is
    as well conditioned as the quiet one): every buffer it fills holds values of order 1e3 and scales of order 10."""
    rng = np.random.RandomState(3 + d)
    shift, scale = (LOUD_SHIFT, LOUD_SCALE) if loud else (0.0, 1.0)
    model_mean, model_sd = shift + scale * 0.2 * rng.randn(d), scale * np.exp(0.1 * rng.randn(d))
    A = rng.randn(d, d)
    th_ch = np.concatenate([shift + scale * 0.1 * rng.randn(d),
                            ofam.psd_to_free(scale ** 2 * 0.7 * (A @ A.T / d + np.eye(d)))])
    th_mf = np.concatenate([shift + scale * 0.1 * rng.randn(d), np.log(scale) - 0.5 + 0.1 * rng.randn(d)])
    prior = np.concatenate([shift * np.ones(d), (np.log(scale) + 0.3) * np.ones(d)])
    return model_mean, model_sd, th_ch, th_mf, prior


def lowrank_start(fam, d, k, loud=False):
    shift, scale = (LOUD_SHIFT, LOUD_SCALE) if loud else (0.0, 1.0)
    return fam.pack(shift * np.ones(d), (np.log(scale) - 0.5) * np.ones(d), scale * 0.1 * np.ones((d, k)))


def make(vb, sid, variant=0, d=D, n=N, loud=False):
    """A fresh objective of subject `sid` and its starting parameter.  `variant` 1 is a second objective of the same
    subject (other family seed); `d`, `n` another shape; `loud` the shifted and stretched problem of `_problem`."""
    model_mean, model_sd, th_ch, th_mf, prior = _problem(d, loud)
    model = vb.GaussianModel(model_mean, model_sd)
    seed = 1 + 10 * variant
    dis = dict(ess_target=n // 6, temper_prior=vb.MFGaussian(d), temper_prior_params=prior, use_resampling=True)
    if sid == 'dis_mf_np':
        return vb.DISInclusiveKL(vb.MFGaussian(d, seed=seed), model, n, num_resampling_batches=3, **dis), th_mf
    if sid == 'dis_mft_px':
        return vb.DISInclusiveKL(vb.MFStudentT(d, 7.0, seed=seed, rng='philox'), model, n, num_resampling_batches=3,
                                 **dis), th_mf
    if sid == 'dis_fr_px':
        return vb.DISInclusiveKL(vb.FullRankGaussian(d, seed=seed, rng='philox'), model, n, num_resampling_batches=2,
                                 **dis), th_ch
    if sid == 'dis_mvt_np':
        return vb.DISInclusiveKL(vb.MultivariateT(d, 9.0, seed=seed), model, n, num_resampling_batches=2, **dis), th_ch
    if sid == 'dis_lr':
        fam = vb.LRGaussian(d, seed=seed, k=3)
        return vb.DISInclusiveKL(fam, model, n, num_resampling_batches=2, **dis), lowrank_start(fam, d, 3, loud)
    if sid == 'ekl_mf_px':
        return vb.ExclusiveKL(vb.MFGaussian(d, seed=seed, rng='philox'), model, n), th_mf
    if sid == 'ekl_mvt_np':
        return vb.ExclusiveKL(vb.MultivariateT(d, 9.0, seed=seed), model, n, use_path_deriv=True), th_ch
    if sid == 'ekl_lr':
        fam = vb.LRGaussian(d, seed=seed, k=3)
        return vb.ExclusiveKL(fam, model, n), lowrank_start(fam, d, 3, loud)
    if sid == 'ekl_nvp':
        masks = np.array([[(j + i) % 2 for j in range(d)] for i in range(2)], dtype=float)
        flow = vb.NVPFlow([[d, 32], [32, d]], [[d, 32], [32, d]], masks, vb.MFStudentT(d, 5.0, seed=seed),
                          prior if loud else np.zeros(2 * d), d)
        return vb.ExclusiveKL(flow, model, n), 0.05 * np.random.RandomState(7).randn(flow.var_param_dim)
    if sid == 'alpha_fr_px':
        return vb.AlphaDivergence(vb.FullRankGaussian(d, seed=seed, rng='philox'), model, n, 0.5), th_ch
    raise ValueError(sid)


def _np_seed(sid, variant=0, d=D):
    return 1000 + 37 * SUBJECTS.index(sid) + 7 * variant + d


class Runner:
    """One objective's turns: it gets back the global numpy generator it would see alone before each call."""

    def __init__(self, vb, sid, variant=0, d=D, n=N, loud=False, make=make, np_seed=_np_seed):
        self.obj, self.th = make(vb, sid, variant, d, n, loud)
        self.state = np.random.RandomState(np_seed(sid, variant, d)).get_state()
        self.out = []

    def step(self):
        np.random.set_state(self.state)
        v, g = self.obj(self.th)
        self.state = np.random.get_state()
        self.out.append((v, g.copy()))
        self.th = self.th - 0.01 * g / (1.0 + np.abs(g))
