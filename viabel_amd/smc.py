"""Adaptive tempered sequential Monte Carlo with HMC moves on the device: equally weighted draws from the target and an
unbiased estimate of its normalising constant, from nothing more than a fit's mean and marginal standard deviations.

The particles start as draws from the diagonal Gaussian base ``q0 = N(loc, diag(scale^2))`` and follow the path
``log pi_beta = beta log p + (1 - beta) log q0`` from ``beta = 0`` to ``beta = 1`` (Del Moral, Doucet & Jasra 2006).  Every
stage picks the next temperature so that the effective sample size of the incremental weights is ``ess_target n`` (Jasra et
al. 2011), resamples systematically, and moves every particle by HMC transitions on ``pi_beta`` (Buchholz, Chopin & Jacob
2021).  Where ``hmc()`` trusts that the fit covers the posterior, the path bridges a poor fit to the target; where the only
log evidence was Laplace's, the product of the stages' mean incremental weights estimates it without a Gaussian assumption.
:func:`smc` is one device-resident run (``vb_smc_run``, ``csrc/vb_smc.hip``; ``DESIGN.md`` 4.28)."""
import numpy as np

from viabel_amd import _lib
from viabel_amd.mcmc import (_require_device_target, _require_fit_pair, _require_integers, _require_open_unit,
                             _resolve_step_size)
from viabel_amd.models import refuse_minibatch

__all__ = ['smc']


def _check_arguments(model, n_particles, var_param, approx, loc, scale, ess_target, n_moves, n_leapfrog, step_size,
                     target_accept, adapt_rate, max_stages, seed, stream_offset):
    """Everything that can be refused without an engine; returns ``(loc, scale, step_size)``, ``loc`` / ``scale`` arrays or
    None (the fit supplies them)."""
    _require_device_target(model, 'smc', 'particles')
    _require_integers(('n_particles', n_particles, 1), ('n_moves', n_moves, 1), ('n_leapfrog', n_leapfrog, 1),
                      ('max_stages', max_stages, 1), ('seed', seed, 0), ('stream_offset', stream_offset, 0))
    _require_open_unit('ess_target', ess_target)
    _require_open_unit('target_accept', target_accept)
    if not (adapt_rate >= 0.0 and np.isfinite(adapt_rate)):
        raise ValueError('adapt_rate must be non-negative and finite')
    _require_fit_pair(var_param, approx)
    if var_param is None and (loc is None or scale is None):
        raise ValueError('either both loc and scale or both var_param and approx must be given')
    d = model.dim
    step_size = _resolve_step_size(step_size, d)
    if loc is not None:
        loc = np.ascontiguousarray(loc, dtype=np.float64)
        if loc.shape != (d,):
            raise ValueError('loc must have shape ({},); got {}'.format(d, loc.shape))
        if not np.all(np.isfinite(loc)):
            raise ValueError('loc must be finite')
    if scale is not None:
        scale = np.ascontiguousarray(scale, dtype=np.float64)
        if scale.shape != (d,):
            raise ValueError('scale must have shape ({},); got {}'.format(d, scale.shape))
        if not (np.all(scale > 0.0) and np.all(np.isfinite(scale))):
            raise ValueError('scale must be positive and finite')
    return loc, scale, step_size


def smc(model, *, n_particles=1024, var_param=None, approx=None, loc=None, scale=None, ess_target=0.5, n_moves=2,
        n_leapfrog=8, step_size=None, target_accept=0.8, adapt_rate=0.5, max_stages=200, seed=1, stream_offset=0,
        keep_ancestors=False):
    """Adaptive tempered sequential Monte Carlo on a device model: ``n_particles`` particles carried from a diagonal
    Gaussian base to the target in one device call (``vb_smc_run``).

    THE BASE IS THE DIAGONAL GAUSSIAN ``N(loc, diag(scale^2))``, NOT THE FIT ITSELF.  With ``var_param`` and ``approx`` (as
    ``bbvi`` or ``laplace_approximation`` return them) ``loc`` and ``scale`` default to the mean and to the square roots of
    the diagonal of ``approx.mean_and_cov(var_param)``: a full-rank, low-rank or flow fit contributes its first two marginal
    moments only, and its correlations or tails are not used.  Without a fit both ``loc`` and ``scale`` (D,) are required.

    Every stage (a) finds the next temperature ``beta`` by 40 bisection steps so that the effective sample size of the
    weights ``(p / q0)^(beta - beta_prev)`` is ``ess_target * n_particles`` -- or jumps to exactly 1 when that already
    holds there --, (b) resamples systematically, and (c) applies ``n_moves`` HMC transitions of ``n_leapfrog`` steps on
    ``p^beta q0^(1 - beta)`` under the metric ``scale^2``.  After every transition the step size follows
    ``log eps += adapt_rate (mean acceptance probability - target_accept)``; ``step_size=None`` starts from
    ``D ** -0.25``.  The random numbers are Philox streams ``stream_offset`` (the start), then one per transition; a run is
    a pure function of its arguments, bit for bit.  ``max_stages`` bounds the stages: ``ValueError`` when ``beta`` has not
    reached 1 by then, when a weight is NaN or ``+inf``, and when fewer than ``ess_target`` of the base's draws lie on the
    target's support.

    Returns a dict: ``particles`` (n x D; equally weighted draws from the target), ``logp`` (n,); ``log_evidence`` (the
    sum of ``log_z_increments``: the log of an unbiased estimate of the normalising constant of ``model``'s density);
    ``betas``, ``log_z_increments`` and ``ess`` (n_stages,; ``betas[-1] == 1.0``); ``accept_prob``, ``n_accepted`` and
    ``step_size_history`` (n_stages x n_moves); ``step_size`` (after the last update); ``n_stages``; ``n_divergent``;
    ``ancestors`` (n_stages x n, int64; None without ``keep_ancestors``); ``mean`` and ``sd`` (``ddof=1``) of the
    particles; ``n_grad_evals`` (gradient evaluations per particle, ``1 + n_stages * n_moves * n_leapfrog``); ``loc``,
    ``scale``, ``seed`` and ``next_stream`` (the first Philox stream the run did not use).
    Runs on the calling process's engine; raises ``NotImplementedError`` for a ``CallableModel``, a
    ``MinibatchRegressionModel``, a sharded engine and more than 65 536 particles."""
    refuse_minibatch(model, 'smc')
    loc, scale, step_size = _check_arguments(model, n_particles, var_param, approx, loc, scale, ess_target, n_moves,
                                             n_leapfrog, step_size, target_accept, adapt_rate, max_stages, seed, stream_offset)
    n, d, n_moves, n_leapfrog = int(n_particles), model.dim, int(n_moves), int(n_leapfrog)
    if loc is None or scale is None:
        mean, cov = approx.mean_and_cov(np.asarray(var_param, dtype=np.float64))
        if loc is None:
            loc = np.ascontiguousarray(mean, dtype=np.float64).reshape(-1)
            if loc.shape != (d,) or not np.all(np.isfinite(loc)):
                raise ValueError('the approximation has no finite mean of shape ({},) to take loc from; pass loc'.format(d))
        if scale is None:
            scale = np.ascontiguousarray(np.sqrt(np.diag(cov)), dtype=np.float64)
            if scale.shape != (d,) or not (np.all(scale > 0.0) and np.all(np.isfinite(scale))):
                raise ValueError('the approximation has no finite positive variances to take scale from; pass scale')
    eng = _lib.default_engine()
    if eng.n_ranks > 1:
        raise NotImplementedError('smc runs on one process\'s engine; a sharded engine ({} ranks) is not supported'.format(
            eng.n_ranks))
    eng.set_model(model.device_spec())
    out = eng.smc_run(loc, scale, n, ess_target=ess_target, n_moves=n_moves, n_leapfrog=n_leapfrog, step_size=step_size,
                      target_accept=target_accept, adapt_rate=adapt_rate, max_stages=int(max_stages), seed=int(seed),
                      stream_offset=int(stream_offset), keep_ancestors=keep_ancestors)
    x, k = out['particles'], out['n_stages']
    results = dict({key: out[key] for key in ('particles', 'logp', 'log_evidence', 'betas', 'log_z_increments', 'ess',
                                              'accept_prob', 'n_accepted', 'step_size_history', 'step_size', 'n_stages',
                                              'n_divergent', 'ancestors')},
                   mean=x.mean(axis=0), sd=x.std(axis=0, ddof=1) if n > 1 else np.full(d, np.nan),
                   n_grad_evals=1 + k * n_moves * n_leapfrog, loc=loc, scale=scale, seed=int(seed),
                   next_stream=int(stream_offset) + 1 + k * n_moves)
    print('smc: {} particles, {} stages, log evidence = {:.6g}, smallest ess = {:.1f}, mean acceptance = {:.3f}, step size = '
          '{:.4g}, {} divergent of {} proposals'.format(n, k, results['log_evidence'], float(np.min(results['ess'])),
                                                        float(np.mean(results['accept_prob'])), results['step_size'],
                                                        results['n_divergent'], n * k * n_moves))
    if results['n_divergent'] > 0:
        print('WARNING: divergent proposals mean the step size is too large for parts of the path; the moves there are '
              'rejected. Lower step_size, raise target_accept, or start from a better base.')
    return results
