"""``bbvi``: one-call black-box variational inference (``viabel/convenience.py:14-94``).

Same keyword interface, validation errors and optimiser wiring as the reference:
``adaptive and not fixed_lr`` -> RAABBVI(RMSProp), ``adaptive and fixed_lr`` -> FASO(RMSProp),
``not adaptive and fixed_lr`` -> RMSProp.  ``log_density`` is a device model
(``viabel_amd.models.DeviceModel``), HIP source, or a Python callable (bound as a ``CallableModel``: evaluated on the
host between the device's sampling and reduction kernels); ``fit`` (PyStan) is not supported.
"""
import numpy as np

from . import _lib
from ._psis import _tail_size, batch_capacity, psislw, psisloo
from .approximations import FullRankGaussian, MFGaussian, MFStudentT, NVPFlow
from .diagnostics import all_diagnostics
from .models import CallableModel, DeviceModel, LogisticRegressionModel, SourceModel, ksd_results, refuse_minibatch
from .objectives import ExclusiveKL, _stage_prior_noise
from .optimization import FASO, RAABBVI, RMSProp

__all__ = ['bbvi', 'vi_diagnostics', 'psis_correction', 'samples_and_log_weights', 'loo', 'psisloo', 'predict',
           'laplace_approximation', 'ksd']


def bbvi(dimension, *, n_iters=10000, num_mc_samples=10, log_density=None, approx=None, objective=None,
         fit=None, adaptive=True, fixed_lr=False, init_var_param=None, learning_rate=0.01,
         RMS_kwargs=dict(), FASO_kwargs=dict(), RAABBVI_kwargs=dict(), grad_log_density=None):
    """Fit a model with black-box variational inference; returns the optimiser's result dict plus
    ``'objective'`` (``convenience.py:92-94``).  ``log_density``: a device model, HIP source, or -- the reference's
    own form -- a callable ``(N, D) -> (N,)``, optionally with ``grad_log_density`` ``(N, D) -> (N, D)`` (an addition:
    the reference differentiates the callable with autograd; without a gradient the engine uses central differences)."""
    if objective is not None:
        if fit is not None or log_density is not None or approx is not None:
            raise ValueError('if objective is specified, cannot specify fit, log_density, or approx')
        approx = objective.approx
    else:
        if log_density is None:
            if fit is None:
                raise ValueError('either log_density or fit must be specified if objective not given')
            raise NotImplementedError('PyStan fits are not supported by the HIP engine; pass a device model')
        elif fit is not None:
            raise ValueError('log_density and fit cannot both be specified')
        if isinstance(log_density, (str, bytes)):      # the log density as HIP source (models.SourceModel)
            src = log_density.encode() if isinstance(log_density, str) else bytes(log_density)
            # a density written generically over vb::vec<T> carries no gradient: the engine differentiates it
            log_density = SourceModel(dimension, log_density, grad='auto' if b'vb::vec' in src else 'explicit')
        if not isinstance(log_density, DeviceModel):
            # the reference's front door (convenience.py:69-75: Model(log_density) + autograd): a host callable, with
            # `grad_log_density` when the caller has one (the StanModel contract, models.py:80-104)
            if not callable(log_density):
                raise TypeError('log_density must be a viabel_amd device model (GaussianModel, FunnelModel, '
                                'CorrelatedGaussianModel, a regression model, a SourceModel / HIP source string '
                                'defining vb_log_density) or a callable (N, D) -> (N,)')
            log_density = CallableModel(dimension, log_density, grad_log_density)
        elif grad_log_density is not None:
            raise ValueError('grad_log_density goes with a callable log_density')
        if approx is None:
            approx = MFGaussian(dimension)
        objective = ExclusiveKL(approx, log_density, num_mc_samples)
    if init_var_param is None:
        init_var_param = approx.init_param()
    base_opt = RMSProp(learning_rate, diagnostics=True, **RMS_kwargs)
    if adaptive and not fixed_lr:
        opt = RAABBVI(base_opt, **RAABBVI_kwargs)
    elif adaptive and fixed_lr:
        opt = FASO(base_opt, **FASO_kwargs)
    elif not adaptive and fixed_lr:
        opt = base_opt
    else:
        raise ValueError('if fixed_lr is False, adaptive must be True')
    results = opt.optimize(n_iters, objective, init_var_param)
    results['objective'] = objective
    return results


def vi_diagnostics(var_param, *, objective=None, model=None, approx=None, n_samples=100000):
    """Pareto k-hat and 2-divergence diagnostics with mean / std / covariance error bounds
    (``convenience.py:97-133``).  Returns a dict that also holds the samples and smoothed log weights."""
    if objective is None:
        if model is None or approx is None:
            raise ValueError('either objective or both model and approx must be specified')
    elif model is not None or approx is not None:
        raise ValueError('model and/or approx cannot be specified if objective is')
    else:
        model, approx = objective.model, objective.approx
    if n_samples <= 0:
        raise ValueError('n_samples must be positive')
    refuse_minibatch(model, 'vi_diagnostics')
    return _vi_diagnostics(var_param, model, approx, n_samples)


def _vi_diagnostics(var_param, model, approx, n_samples):      # convenience.py:136-163
    samples, smoothed_log_weights, khat = psis_correction(var_param, model, approx, n_samples)
    results = dict(samples=samples, smoothed_log_weights=smoothed_log_weights, khat=khat)
    print('Pareto k is estimated to be khat = {:.2f}'.format(khat))
    if khat > 0.7:
        print('WARNING: khat > 0.7 means importance sampling is not feasible.')
        print('WARNING: not running further diagnostics')
        return results
    print()
    moment_bound_fn = None
    if approx.supports_pth_moment(2) and approx.supports_pth_moment(4):
        def moment_bound_fn(p):
            return approx.pth_moment(var_param, p)
    _, q_var = approx.mean_and_cov(var_param)
    # NB the reference hands all_diagnostics the (D, n) transpose that psis_correction returns; with
    # pth_moment available (every in-scope family) the samples are not touched, so the orientation is moot
    results.update(all_diagnostics(smoothed_log_weights, samples=samples, moment_bound_fn=moment_bound_fn,
                                   q_var=q_var))
    print('The 2-divergence is estimated to be d2 = {:.2g}'.format(results['d2']))
    if results['d2'] > 4.6:
        print('WARNING: d2 > 4.6 means the approximation is very inaccurate')
    elif results['d2'] > 0.1:
        print('WARNING: 0.1 < d2 < 4.6 means the approximation is somewhat '
              'inaccurate. Use importance sampling to decrease error.')
    else:
        print('\nAll diagnostics pass.')
    return results


def psis_correction(var_param, model, approx, n_samples):
    """Samples (transposed, as the reference returns them), PSIS-smoothed log weights and k-hat
    (``convenience.py:166-169``).  For the mean-field families on an elementwise / funnel target the log
    weights never leave the GPU between their evaluation and the smoothing."""
    var_param = np.asarray(var_param, dtype=np.float64)
    refuse_minibatch(model, 'psis_correction')
    if _on_device_weights(model, approx):
        eng = _lib.default_engine()
        eng.set_model(model.device_spec())
        if approx.rng == 'philox':          # base noise drawn on the GPU; read back only for the returned samples
            kind, kdf = approx._philox_kind()
            eng.noise_generate(_DIAG_SLOT, n_samples, approx.dim, approx._seed, approx._next_philox_stream(),
                               kind=kind, df=kdf)
            noise = eng.noise_get_host(_DIAG_SLOT, n_samples, approx.dim)
        else:
            noise = approx._base_noise(n_samples)
            eng.noise_set_host(_DIAG_SLOT, noise)
        family, df = approx._device_family()
        eng.log_weights_meanfield(_DIAG_SLOT, n_samples, approx.dim, var_param, family, df=df, fetch=False)
        smoothed, khat = eng.psis_smooth(n_samples)
        samples = var_param[:approx.dim] + np.exp(var_param[approx.dim:]) * noise
        return samples.T, smoothed, khat
    samples, log_weights = samples_and_log_weights(var_param, model, approx, n_samples)
    smoothed, khat = psislw(log_weights, overwrite_lw=True)
    return samples.T, smoothed, khat


_DIAG_SLOT = 2      # device noise slot used by the diagnostics (objectives use 0 and 1)


def _on_device_weights(model, approx):
    return (isinstance(approx, (MFGaussian, MFStudentT)) and isinstance(model, DeviceModel)
            and model.device_spec()[0] in (_lib.MODEL_GAUSS_DIAG, _lib.MODEL_FUNNEL) + _lib.MODELS_WITH_ROWS)


def samples_and_log_weights(var_param, model, approx, n_samples):
    """Samples from the approximation and their importance log weights (``convenience.py:176-179``);
    the model log density is evaluated on the GPU."""
    refuse_minibatch(model, 'samples_and_log_weights')
    if isinstance(approx, NVPFlow) and isinstance(model, DeviceModel):
        # the flow's forward pass and the model on the device over the prior draws approx.sample would consume; log q
        # from the forward pass (log p0(z0) - sum s), which equals the inverse pass's up to rounding
        var_param = np.asarray(var_param, dtype=np.float64)
        if var_param.shape != (approx.var_param_dim,):
            raise ValueError('var_param must have shape ({},)'.format(approx.var_param_dim))
        eng = _lib.default_engine()
        eng.set_model(model.device_spec())
        handle = approx._device_handle(eng)
        n_ranks, rank = eng.n_ranks, eng.rank
        eng.n_ranks, eng.rank = 1, 0          # (every process draws all of its own diagnostics samples)
        try:
            _stage_prior_noise(eng, approx.prior, n_samples, _DIAG_SLOT)
        finally:
            eng.n_ranks, eng.rank = n_ranks, rank
        family, df, prior_param = approx._device_prior()
        samples, log_q, log_p = eng.flow_sample(handle, _DIAG_SLOT, n_samples, approx.dim, family, df, prior_param,
                                                var_param, want_x=True, want_log_p=True)
        return samples, log_p - log_q
    samples = approx.sample(var_param, n_samples)
    return samples, model(samples) - approx.log_density(var_param, samples)


def loo(var_param, *, objective=None, model=None, approx=None, n_samples=4000, Reff=1.0):
    """PSIS leave-one-out cross-validation of a fitted regression model, for comparing models by out-of-sample
    predictive accuracy (``psisloo``, ``viabel/_psis.py:69-110``, made to work from a variational fit).

    ``n_samples`` draws ``theta_s ~ q`` and their log ratios ``log p(theta_s, y) - log q(theta_s)``
    (:func:`samples_and_log_weights`); observation ``i``'s leave-one-out weights are the Pareto-smoothed, normalised
    ``log ratio_s - log p(y_i | theta_s)``.  The ``n_data x n_samples`` likelihood matrix is formed, smoothed and reduced
    on the device (``vb_glm_psis_loo``); only three ``n_data``-vectors come back.  Returns a dict: ``elpd_loo`` (sum of
    ``pointwise``), ``se_elpd_loo = sqrt(n_data var(pointwise))``, ``p_loo = sum(lpd - pointwise)``, ``pointwise``
    (``log p(y_i | y_-i)``), ``lpd`` (``log p(y_i | y)`` under the smoothed full-data weights), ``khat`` (per
    observation), ``khat_full`` (of the full-data ratios) and ``n_samples``.  Runs on the calling process's engine."""
    if objective is None:
        if model is None or approx is None:
            raise ValueError('either objective or both model and approx must be specified')
    elif model is not None or approx is not None:
        raise ValueError('model and/or approx cannot be specified if objective is')
    else:
        model, approx = objective.model, objective.approx
    if n_samples < 2:
        raise ValueError('n_samples must be at least 2')
    if not (Reff > 0):
        raise ValueError('Reff must be positive')
    refuse_minibatch(model, 'loo')
    if not isinstance(model, LogisticRegressionModel):
        raise NotImplementedError(
            'loo needs a target with per-observation structure (LogisticRegressionModel, PoissonRegressionModel, '
            'LinearRegressionModel); {} has none. Build the (draws x observations) log-likelihood matrix yourself and '
            'call psisloo(log_lik, log_ratios)'.format(type(model).__name__))
    if not batch_capacity(n_samples, Reff):
        raise NotImplementedError(
            'loo keeps the likelihood matrix on the device and smooths it with the batched kernel, which takes at most '
            '{} draws with a tail of at most {} values (n_samples = {}, Reff = {} has a tail of {}); use fewer draws, or '
            'psisloo(log_lik, log_ratios) on a host matrix'.format(_lib.PSIS_BATCH_MAX_N, _lib.PSIS_BATCH_MAX_TAIL,
                                                                  n_samples, Reff, _tail_size(n_samples, Reff)))
    var_param = np.asarray(var_param, dtype=np.float64)
    samples, log_ratios = samples_and_log_weights(var_param, model, approx, n_samples)
    log_w, khat_full = psislw(log_ratios, Reff=Reff)
    eng = _lib.default_engine()
    eng.set_model(model.device_spec())
    pointwise, khat, lpd = eng.glm_psis_loo(samples, model.n_data, log_ratios=log_ratios, log_w=log_w, reff=Reff)
    n = pointwise.size
    results = dict(elpd_loo=float(pointwise.sum()), se_elpd_loo=float(np.sqrt(n * np.var(pointwise))),
                   p_loo=float(np.sum(lpd - pointwise)), pointwise=pointwise, lpd=lpd, khat=khat,
                   khat_full=float(khat_full), n_samples=int(n_samples))
    n_bad = int(np.sum(khat > 0.7))
    print('elpd_loo = {:.2f} (SE {:.2f}), p_loo = {:.2f}'.format(results['elpd_loo'], results['se_elpd_loo'],
                                                                 results['p_loo']))
    print('{} of {} observations have Pareto khat > 0.7 (full-data ratios: khat = {:.2f})'.format(n_bad, n, khat_full))
    if n_bad:
        print('WARNING: khat > 0.7 means the leave-one-out terms of those observations are unreliable.')
    return results


def predict(var_param, *, objective=None, model=None, approx=None, X_new=None, y_new=None, n_samples=4000, weights='psis',
            Reff=1.0):
    """Posterior prediction with a fitted regression model: predictive means, standard deviations and -- with responses
    -- the log predictive density of each observation, at the rows of ``X_new`` (the model's own design without it;
    ``y_new=None`` then means its own responses).

    ``n_samples`` draws ``theta_s ~ q`` and their log ratios ``log p(theta_s, y) - log q(theta_s)``
    (:func:`samples_and_log_weights`).  ``weights='psis'`` corrects the draws towards the posterior with the
    Pareto-smoothed, normalised ratios (``psislw``); ``weights=None`` takes the draws as they are.  The
    ``m x n_samples`` matrix of linear predictors is formed and reduced on the device (``vb_glm_predict``,
    :meth:`LogisticRegressionModel.predict_from_draws`; any model that has a ``predict_from_draws`` is taken -- a
    ``NeuralNetRegressionModel`` predicts its network output, ``vb_nn_predict``); five ``m``-vectors come back.
    Returns a dict: ``mean`` and ``sd``
    of the response, ``eta_mean`` and ``eta_sd`` of the linear predictor, ``khat`` (of the ratios; None with
    ``weights=None``), ``n_samples`` and, with a response, ``lpd`` (``log p(y_i | y)`` per observation), ``elpd``
    (their sum: on held-out rows the number ``loo()``'s ``elpd_loo`` estimates) and ``se_elpd = sqrt(m var(lpd))``.
    Runs on the calling process's engine."""
    if objective is None:
        if model is None or approx is None:
            raise ValueError('either objective or both model and approx must be specified')
    elif model is not None or approx is not None:
        raise ValueError('model and/or approx cannot be specified if objective is')
    else:
        model, approx = objective.model, objective.approx
    if n_samples < 1:
        raise ValueError('n_samples must be positive')
    if weights not in ('psis', None):
        raise ValueError("weights must be 'psis' or None")
    if weights == 'psis' and n_samples < 2:
        raise ValueError('n_samples must be at least 2 to smooth the weights')
    if not (Reff > 0):
        raise ValueError('Reff must be positive')
    refuse_minibatch(model, 'predict')
    if not callable(getattr(model, 'predict_from_draws', None)):
        raise NotImplementedError(
            'predict covers LogisticRegressionModel, PoissonRegressionModel and LinearRegressionModel; {} has no '
            'predict_from_draws. What exists for it: pointwise_log_likelihood(draws) where the model defines it, to be '
            'reduced on the host'.format(type(model).__name__))
    var_param = np.asarray(var_param, dtype=np.float64)
    samples, log_ratios = samples_and_log_weights(var_param, model, approx, n_samples)
    log_w, khat = None, None
    if weights == 'psis':
        log_w, khat = psislw(log_ratios, Reff=Reff)
        khat = float(khat)
    out = model.predict_from_draws(samples, X_new=X_new, y_new=y_new, log_weights=log_w)
    m = out['mean'].size
    results = dict(mean=out['mean'], sd=np.sqrt(out['var']), eta_mean=out['eta_mean'], eta_sd=np.sqrt(out['eta_var']),
                   khat=khat, n_samples=int(n_samples))
    if 'lpd' in out:
        lpd = out['lpd']
        results.update(lpd=lpd, elpd=float(lpd.sum()), se_elpd=float(np.sqrt(m * np.var(lpd))))
        print('elpd = {:.2f} (SE {:.2f}) over {} observations, {:.4f} per observation'.format(
            results['elpd'], results['se_elpd'], m, results['elpd'] / m))
    else:
        print('predicted {} observations from {} draws (no response: no elpd)'.format(m, int(n_samples)))
    if khat is not None:
        print('Pareto k is estimated to be khat = {:.2f}'.format(khat))
        if khat > 0.7:
            print('WARNING: khat > 0.7 means importance sampling is not feasible.')
    return results


def ksd(var_param=None, *, objective=None, model=None, approx=None, samples=None, log_weights=None, scores=None,
        n_samples=4096, weights='psis', Reff=1.0, scale='auto', c=1.0, beta=-0.5):
    """Kernel Stein discrepancy (Gorham & Mackey 2017, inverse multiquadric kernel ``(c^2 + |x - y|^2)^beta``) of a
    weighted sample against a target, from the target's scores ``grad log p`` alone: no normalising constant, no density
    ratio, no reference sample.  All ``S^2`` pairs are summed on the device (``vb_ksd``); nothing of that order is stored.

    What the number is for: COMPARING samples of ONE target at the same ``scale``, ``c`` and ``beta`` -- a mean-field
    fit against a full-rank one, raw draws against PSIS-corrected ones, each of them against an ``hmc()`` baseline of the
    same size.  Smaller is closer; an exact sample of ``S`` draws does not give 0 but a value that shrinks like
    ``1 / sqrt(S)``.  It is not an absolute threshold.

    Exactly one of ``var_param`` and ``samples`` is given.

    **From a fit**: ``var_param`` with ``objective``, or with ``model`` and ``approx`` (the rules of :func:`predict`).
    ``n_samples`` draws and their log ratios come from :func:`samples_and_log_weights`; ``weights='psis'`` smooths the
    ratios (``psislw``) and reports ``khat``, ``weights=None`` takes the draws as they are.  ``scale='auto'``: the
    approximation's standard deviations (``approx.mean_and_cov(var_param)``).  The scores are the model's device
    gradient.

    **From draws**: ``samples`` (S x D) -- ``hmc()``'s draws reshaped to ``(chains * draws, D)``, or draws produced
    elsewhere -- with optional ``log_weights`` (S,) and either ``model`` (device scores) or ``scores`` (S x D, given).
    ``scale='auto'``: the weighted standard deviations of the draws.

    In both modes ``scale=None`` means ones and an array is taken as given.  Returns a dict: ``ksd``, ``ksd2``,
    ``rowsums`` (``ksd2 = sum_i w_i rowsums[i]``), ``ess`` (``1 / sum w^2``), ``n_samples``, ``c``, ``beta``, ``khat``
    (None without smoothing) and ``scale``.  Argument errors raise ``ValueError`` before the engine is touched.  Runs on
    the calling process's engine."""
    if (var_param is None) == (samples is None):
        raise ValueError('exactly one of var_param (a fit) and samples (draws) must be given')
    c, beta = float(c), float(beta)
    if not (c > 0.0 and np.isfinite(c)):
        raise ValueError('c must be positive and finite')
    if not (-1.0 < beta < 0.0):
        raise ValueError('beta must lie in (-1, 0)')
    auto = isinstance(scale, str)
    if auto and scale != 'auto':
        raise ValueError("scale must be 'auto', None or an array")
    khat = None
    if samples is None:
        if objective is None:
            if model is None or approx is None:
                raise ValueError('either objective or both model and approx must be specified')
        elif model is not None or approx is not None:
            raise ValueError('model and/or approx cannot be specified if objective is')
        else:
            model, approx = objective.model, objective.approx
        if log_weights is not None or scores is not None:
            raise ValueError('log_weights and scores go with samples; a fit supplies its own')
        if n_samples < 1:
            raise ValueError('n_samples must be positive')
        if weights not in ('psis', None):
            raise ValueError("weights must be 'psis' or None")
        if weights == 'psis' and n_samples < 2:
            raise ValueError('n_samples must be at least 2 to smooth the weights')
        if not (Reff > 0):
            raise ValueError('Reff must be positive')
        if not auto and scale is not None:
            _lib.ksd_arguments(np.zeros((1, approx.dim)), scale=scale)
        if not isinstance(model, DeviceModel):
            raise TypeError('ksd needs a viabel_amd device model (its scores are device code); got {}. For other targets '
                            'pass samples= and scores='.format(type(model).__name__))
        model._refuse_ksd()
        var_param = np.asarray(var_param, dtype=np.float64)
        if auto:
            scale = np.sqrt(np.diag(approx.mean_and_cov(var_param)[1]))
        samples, log_ratios = samples_and_log_weights(var_param, model, approx, n_samples)
        if weights == 'psis':
            log_weights, khat = psislw(log_ratios, Reff=Reff)
            khat = float(khat)
    else:
        if objective is not None or approx is not None:
            raise ValueError('objective and approx go with var_param; with samples give model or scores')
        if (model is None) == (scores is None):
            raise ValueError('with samples exactly one of model and scores must be given')
        if model is not None and not isinstance(model, DeviceModel):
            raise TypeError('model must be a viabel_amd device model; got {}. Pass scores= instead'.format(
                type(model).__name__))
        samples, scores, log_weights, scale_arr, _, _ = _lib.ksd_arguments(samples, scores, log_weights,
                                                                           None if auto else scale, c, beta)
        if model is not None:
            if samples.shape[1] != model.dim:
                raise ValueError('samples must have shape (S, {})'.format(model.dim))
            model._refuse_ksd()
        if auto:
            w = np.full(samples.shape[0], 1.0 / samples.shape[0]) if log_weights is None else \
                np.exp(log_weights - np.max(log_weights))
            w = w / np.sum(w)
            mean = w @ samples
            scale = np.sqrt(w @ (samples - mean) ** 2)
            if not np.all(np.isfinite(scale) & (scale > 0.0)):
                raise ValueError("scale='auto' needs draws that vary in every coordinate; pass scale=None or an array")
        else:
            scale = scale_arr
    scale = None if scale is None else np.ascontiguousarray(scale, dtype=np.float64)
    if scores is None:
        results = model.ksd_from_draws(samples, log_weights=log_weights, scale=scale, c=c, beta=beta)
    else:
        ksd2, rowsums = _lib.default_engine().ksd(samples, scores, log_weights, scale, c, beta)
        results = ksd_results(ksd2, rowsums, log_weights, c, beta)
    results.update(khat=khat, scale=scale)
    print('KSD = {:.4g} (squared: {:.4g}) from {} draws, effective sample size {:.1f}'.format(
        results['ksd'], results['ksd2'], results['n_samples'], results['ess']))
    if khat is not None:
        print('Pareto k is estimated to be khat = {:.2f}'.format(khat))
        if khat > 0.7:
            print('WARNING: khat > 0.7 means importance sampling is not feasible.')
    return results


def laplace_approximation(model, x0=None, max_iter=100, tol=1e-10, seed=1, rng='numpy'):
    """The Gaussian at the mode of a device model: ``N(mode, (-H)^-1)`` with ``H`` the Hessian of the log density there.

    The mode comes from :meth:`DeviceModel.find_mode` (damped Newton from ``x0``; for the flat regression targets every
    evaluation is one device call -- a streaming pass over the design and an fp64 MFMA Gram product --, for every other
    device model the Hessian is a fourth-order difference of the device gradient); the ``D x D`` factorisations are host
    LAPACK.  Returns a dict: ``mode``, ``hessian``, ``n_iter``, ``converged`` (as ``find_mode`` gives them),
    ``cov = (-H)^-1`` (symmetrised), ``approx = FullRankGaussian(dim, seed=seed, rng=rng)``,
    ``var_param = approx.pack(mode, cholesky(cov))`` and the Laplace evidence estimate
    ``log_evidence = f(mode) + D / 2 log(2 pi) - 1/2 log det(-H)``, to be read beside an ELBO.  ``var_param`` and
    ``approx`` go as they are into ``vi_diagnostics(var_param, model=, approx=)``, ``bbvi(..., approx=, init_var_param=)``,
    ``loo`` and ``predict``.  Raises ``ValueError`` when ``-H`` at the returned point is not positive definite (a saddle, a
    search that did not converge: there is no Gaussian there) and ``TypeError`` for a model that is not a
    ``DeviceModel``."""
    from scipy.linalg import cho_factor, cho_solve
    if not isinstance(model, DeviceModel):
        raise TypeError('laplace_approximation needs a viabel_amd device model (its gradient and Hessian are device code); '
                        'got {}'.format(type(model).__name__))
    refuse_minibatch(model, 'laplace_approximation')
    found = model.find_mode(x0=x0, max_iter=max_iter, tol=tol)
    mode, H = found['mode'], found['hessian']
    d = model.dim
    try:
        if not np.all(np.isfinite(H)):
            raise np.linalg.LinAlgError('non-finite Hessian')
        factor = cho_factor(-H, lower=True)
    except np.linalg.LinAlgError:
        raise ValueError('the negated Hessian at the point find_mode returned is not positive definite: no Gaussian '
                         'there (converged = {})'.format(found['converged'])) from None
    cov = cho_solve(factor, np.eye(d))
    cov = 0.5 * (cov + cov.T)
    approx = FullRankGaussian(d, seed=seed, rng=rng)
    var_param = approx.pack(mode, np.linalg.cholesky(cov))
    log_det = 2.0 * float(np.sum(np.log(np.diag(factor[0]))))
    log_evidence = found['value'] + 0.5 * d * np.log(2.0 * np.pi) - 0.5 * log_det
    return dict(mode=mode, hessian=H, n_iter=found['n_iter'], converged=found['converged'], cov=cov, approx=approx,
                var_param=var_param, log_evidence=float(log_evidence))
