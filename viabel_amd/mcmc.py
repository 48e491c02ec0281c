"""Many-chain Hamiltonian Monte Carlo on the device gradients: the ground truth a variational fit is checked against.

The reference's documentation compares its fits with MCMC draws (``docs/source/robust-regression.ipynb``:
``check_accuracy(true_mean, true_cov, var_param, approx)``); :func:`hmc` produces those draws here, from the gradient
pipeline the objectives use (``vb_hmc_run`` / ``vb_hmc_run_metric`` / ``vb_hmc_run_chees``, ``csrc/vb_hmc.hip``;
``DESIGN.md`` 4.22 and 4.25)."""
from functools import partial

import numpy as np

from viabel_amd import _lib
from viabel_amd.models import CallableModel, DeviceModel, refuse_minibatch

__all__ = ['hmc']


def _combine_chains(chain_mean, chain_var, n):
    """``(mean, sd, rhat)`` over the chains from their means and ``ddof=1`` variances of ``n`` draws each: ``W`` the mean
    chain variance, ``B = n var(chain means, ddof=1)``, ``var+ = (n - 1) / n W + B / n``, ``sd = sqrt(var+)``,
    ``rhat = sqrt(var+ / W)`` (Gelman et al., BDA3 11.4).  One chain has no between-chain variance: ``B = 0``."""
    chain_mean, chain_var = np.asarray(chain_mean, dtype=np.float64), np.asarray(chain_var, dtype=np.float64)
    w = chain_var.mean(axis=0)
    b_over_n = chain_mean.var(axis=0, ddof=1) if chain_mean.shape[0] > 1 else np.zeros(chain_mean.shape[1])
    var_plus = (n - 1.0) / n * w + b_over_n
    with np.errstate(divide='ignore', invalid='ignore'):
        rhat = np.sqrt(var_plus / w)
    return chain_mean.mean(axis=0), np.sqrt(var_plus), rhat


MIN_ADAPT_WARMUP = 20          # the shortest warm-up the window schedule divides
ADAPT_REG_WEIGHT, ADAPT_REG_VAR = 5.0, 1e-3


def _adaptation_windows(n_warmup):
    """The slow-phase windows ``[(start, end), ...]`` of an ``n_warmup``-iteration warm-up (Stan's schedule): an initial
    buffer of 75, a terminal buffer of 50 and a first window of 25 iterations -- or 15 % / 10 % / the rest when those do not
    fit --, each window twice as long as the last, the last one stretched to the terminal buffer when the next would not
    fit in front of it."""
    n = int(n_warmup)
    if n < MIN_ADAPT_WARMUP:
        raise ValueError('adapt_metric needs n_warmup >= {}'.format(MIN_ADAPT_WARMUP))
    init, term, base = 75, 50, 25
    if init + base + term > n:
        init, term = int(0.15 * n), int(0.10 * n)
        base = n - init - term
    end_slow = n - term
    windows, start, size = [], init, base
    while True:
        end = start + size
        if end + 2 * size > end_slow:
            windows.append((start, end_slow))
            return windows
        windows.append((start, end))
        start, size = end, 2 * size


def _window_metric(s1, s2, n, dense, window):
    """The regularised metric of one window from the moments of its ``n`` states about a shift (which only conditions the
    sums): ``cov = (S2 - S1 S1' / n) / (n - 1)`` shrunk as Stan does, ``n / (n + 5) cov + 1e-3 * 5 / (n + 5) I`` -- the
    matrix and its lower Cholesky factor (dense), or the variances twice (diagonal)."""
    n = float(n)
    w = n / (n + ADAPT_REG_WEIGHT)
    floor = ADAPT_REG_VAR * ADAPT_REG_WEIGHT / (n + ADAPT_REG_WEIGHT)
    if not dense:
        var = w * ((s2 - s1 * s1 / n) / (n - 1.0)) + floor
        if not (np.all(var > 0.0) and np.all(np.isfinite(var))):
            raise ValueError('adaptation window {}: the chains\' variances are not finite and positive'.format(window))
        return var, var
    cov = w * ((s2 - np.outer(s1, s1) / n) / (n - 1.0)) + floor * np.eye(s1.size)
    try:
        return cov, np.linalg.cholesky(cov)
    except np.linalg.LinAlgError as err:
        raise np.linalg.LinAlgError('adaptation window {}: the chains\' covariance has no Cholesky factor ({})'.format(
            window, err)) from err


def _dense_factor(cov, what):
    """Lower Cholesky factor of a symmetric (to rounding), finite, positive definite matrix, else ``ValueError``."""
    if not np.all(np.isfinite(cov)):
        raise ValueError('{} must be finite'.format(what))
    if np.max(np.abs(cov - cov.T)) > 1e-8 * np.max(np.abs(cov)):
        raise ValueError('{} must be symmetric'.format(what))
    try:
        return np.linalg.cholesky(cov)
    except np.linalg.LinAlgError:
        raise ValueError('{} must be positive definite'.format(what))


# ---- argument checks hmc() shares with smc() (viabel_amd/smc.py): none of them touches an engine -----------------------------
def _require_device_target(model, what, moved):
    """``TypeError`` unless ``model`` is a device model, ``NotImplementedError`` for a host callback; ``what`` is the calling
    function's name, ``moved`` what it advances ('chains', 'particles')."""
    if not isinstance(model, DeviceModel):
        raise TypeError('{} needs a viabel_amd device model (its gradient is device code); got {}'.format(
            what, type(model).__name__))
    if isinstance(model, CallableModel):
        raise NotImplementedError('{} advances the {} without host synchronisation: a CallableModel (a host callback) '
                                  'cannot be its target; write the density as a SourceModel'.format(what, moved))


def _require_integers(*triples):
    """Every ``(name, value, lowest)``: an integer (no bool) that is at least ``lowest``."""
    for name, v, low in triples:
        if isinstance(v, bool) or int(v) != v or v < low:
            raise ValueError('{} must be an integer >= {}'.format(name, low))


def _require_open_unit(name, v):
    if not (0.0 < v < 1.0):
        raise ValueError('{} must lie in (0, 1)'.format(name))


def _require_fit_pair(var_param, approx):
    if (var_param is None) != (approx is None):
        raise ValueError('var_param and approx must be given together')


def _resolve_step_size(step_size, d):
    """``step_size`` as a float, ``D ** -0.25`` for None; positive and finite."""
    step_size = d ** -0.25 if step_size is None else float(step_size)
    if not (step_size > 0.0 and np.isfinite(step_size)):
        raise ValueError('step_size must be positive and finite')
    return step_size


def _check_arguments(model, n_chains, n_warmup, n_draws, n_leapfrog, step_size, target_accept, jitter, init, inv_mass,
                     var_param, approx, thin, metric='diag', adapt_metric=False, trajectory='fixed', max_leapfrog=256,
                     trajectory_length=None, trajectory_lr=0.025):
    """Everything that can be refused without an engine; returns ``(init, inv_mass, step_size)`` as arrays / float."""
    if metric not in ('diag', 'dense'):
        raise ValueError('metric must be \'diag\' or \'dense\'; got {!r}'.format(metric))
    if trajectory not in ('fixed', 'chees'):
        raise ValueError('trajectory must be \'fixed\' or \'chees\'; got {!r}'.format(trajectory))
    if isinstance(max_leapfrog, bool) or int(max_leapfrog) != max_leapfrog or not (1 <= max_leapfrog < 2 ** 31):
        raise ValueError('max_leapfrog must be an integer >= 1')
    if trajectory_length is not None and not (trajectory_length > 0.0 and np.isfinite(trajectory_length)):
        raise ValueError('trajectory_length must be positive and finite')
    if not (trajectory_lr >= 0.0 and np.isfinite(trajectory_lr)):
        raise ValueError('trajectory_lr must be non-negative and finite')
    _require_device_target(model, 'hmc', 'chains')
    _require_integers(('n_chains', n_chains, 1), ('n_warmup', n_warmup, 0), ('n_draws', n_draws, 1),
                      ('n_leapfrog', n_leapfrog, 1), ('thin', thin, 1))
    if trajectory == 'chees' and n_chains < 2 and n_warmup > 0:
        raise ValueError('trajectory=\'chees\' adapts the trajectory length across the chains: it needs n_chains >= 2 '
                         '(or n_warmup = 0)')
    _require_open_unit('target_accept', target_accept)
    if not (0.0 <= jitter < 1.0):
        raise ValueError('jitter must lie in [0, 1)')
    _require_fit_pair(var_param, approx)
    if var_param is None and init is None:
        raise ValueError('either init or both var_param and approx must be given')
    if adapt_metric and n_warmup < MIN_ADAPT_WARMUP:
        raise ValueError('adapt_metric needs n_warmup >= {}'.format(MIN_ADAPT_WARMUP))
    d = model.dim
    step_size = _resolve_step_size(step_size, d)
    if init is not None:
        init = np.ascontiguousarray(init, dtype=np.float64)
        if init.shape != (n_chains, d):
            raise ValueError('init must have shape ({}, {}); got {}'.format(n_chains, d, init.shape))
        if not np.all(np.isfinite(init)):
            raise ValueError('init must be finite')
    if inv_mass is not None:
        inv_mass = np.ascontiguousarray(inv_mass, dtype=np.float64)
        if metric == 'dense' and inv_mass.shape == (d, d):
            _dense_factor(inv_mass, 'inv_mass')
            return init, inv_mass, step_size
        if inv_mass.shape != (d,):
            raise ValueError('inv_mass must have shape ({0},){1}; got {2}'.format(
                d, ' or ({0}, {0})'.format(d) if metric == 'dense' else '', inv_mass.shape))
        if not (np.all(inv_mass > 0.0) and np.all(np.isfinite(inv_mass))):
            raise ValueError('inv_mass must be positive and finite')
        if metric == 'dense':
            inv_mass = np.diag(inv_mass)
    return init, inv_mass, step_size


def _segments(n_warmup, n_draws, windows):
    """``[(n_warmup, n_draws, window or None), ...]``: the engine calls of an adaptive run -- the initial buffer, every
    window, the terminal buffer together with the sampling phase."""
    out = [(windows[0][0], 0, None)] if windows[0][0] > 0 else []
    out += [(end - start, 0, (start, end)) for start, end in windows]
    return out + [(n_warmup - windows[-1][1], n_draws, None)]


def _resolve_start(fit, shape, init, inv_mass, dense):
    """``(init, inv_mass)``, ``shape = (n_chains, D)``: what the caller left out comes from ``fit = (approx, var_param)``
    when there is one; without it the metric is the unit one."""
    if fit is not None:
        approx, var_param = fit
        if inv_mass is None and dense:
            inv_mass = np.ascontiguousarray(approx.mean_and_cov(var_param)[1], dtype=np.float64)
            if inv_mass.shape != (shape[1], shape[1]):
                raise ValueError('approx.mean_and_cov returned a covariance of shape {}'.format(inv_mass.shape))
            _dense_factor(inv_mass, 'the approximation\'s covariance')
        elif inv_mass is None:
            inv_mass = np.ascontiguousarray(np.diag(approx.mean_and_cov(var_param)[1]), dtype=np.float64)
            if not (np.all(inv_mass > 0.0) and np.all(np.isfinite(inv_mass))):
                raise ValueError('the approximation has no finite positive variances to take the metric from; pass inv_mass')
        if init is None:
            init = np.ascontiguousarray(approx.sample(var_param, shape[0]), dtype=np.float64)
            if init.shape != shape:
                raise ValueError('approx.sample returned shape {}, expected ({}, {})'.format(init.shape, *shape))
    if inv_mass is None:
        inv_mass = np.eye(shape[1]) if dense else np.ones(shape[1])
    return init, inv_mass


def _run_segments(method, segments, out, inv_mass, stream):
    """One call of ``method`` (an ``Engine.hmc_run*`` with the run's own arguments bound) per segment ``(n_warmup, n_draws,
    window)``, each continuing from the last one's ``out`` -- states, final step, trajectory state; at first the start's --
    and stream; a window's call also returns the moments the next metric is estimated from.  Returns the last call's
    outputs with the histories of all calls stitched together, the sampling phase's ``inv_mass`` and ``n_calls``."""
    dense = inv_mass.ndim == 2
    factor, calls = np.linalg.cholesky(inv_mass) if dense else inv_mass, []
    for n_warmup, n_draws, window in segments:
        x, own = out['last'], ({'traj_state': out['traj_state']} if 'traj_state' in out else {})
        if window is not None:
            own['moment_shift'] = x.mean(axis=0)
        out = method(x, factor, n_warmup, n_draws, step_size=out['step_size'], stream_offset=stream, **own)
        calls.append(out)
        if window is not None:
            inv_mass, factor = _window_metric(out['moment_sum'], out['moment_m2'], x.shape[0] * n_warmup, dense, window)
        stream += n_warmup + n_draws
    for key in ('step_size_history', 'accept_prob', 'trajectory_history', 'n_leapfrog_history'):
        if key in out:
            out[key] = np.concatenate([call[key] for call in calls])
    return dict(out, inv_mass=inv_mass, n_calls=len(calls))


def _results(out, n_draws, **run):
    """``hmc``'s result dict from the stitched outputs and the run's own entries (``run``), and the printed summary."""
    with np.errstate(divide='ignore', invalid='ignore'):
        chain_var = out['chain_m2'] / (n_draws - 1.0) if n_draws > 1 else np.full_like(out['chain_m2'], np.nan)
    mean, sd, rhat = _combine_chains(out['chain_mean'], chain_var, n_draws)
    leap_hist = out['n_leapfrog_history']
    results = dict({key: out[key] for key in ('draws', 'logp', 'last', 'chain_mean', 'accept_rate', 'accept_prob',
                                              'step_size_history', 'step_size', 'n_divergent', 'inv_mass',
                                              'trajectory_history', 'n_leapfrog_history')},
                   chain_var=chain_var, mean=mean, sd=sd, rhat=rhat, n_grad_evals=int(leap_hist.sum()) + out['n_calls'], **run)
    max_rhat = float(np.max(rhat[~np.isnan(rhat)])) if not np.all(np.isnan(rhat)) else float('nan')
    print('hmc: step size = {:.4g}, T = {:.4g}, mean L = {:.1f}, mean acceptance = {:.3f}, max rhat = {:.3f}, {} divergent of '
          '{} proposals'.format(results['step_size'], run['trajectory_length'], float(leap_hist.mean()),
                                float(out['accept_rate'].mean()), max_rhat, results['n_divergent'], n_draws * out['last'].shape[0]))
    if max_rhat > 1.05 or results['n_divergent'] > 0:
        print('WARNING: rhat > 1.05 means the chains have not mixed; divergences mean the step size is too large for '
              'parts of the posterior. Run longer, start from a better fit, or lower step_size.')
    return results


def hmc(model, *, n_chains=256, n_warmup=300, n_draws=300, n_leapfrog=16, step_size=None, target_accept=0.8, jitter=0.2,
        init=None, inv_mass=None, var_param=None, approx=None, seed=1, stream_offset=0, thin=1, keep_draws=True,
        metric='diag', adapt_metric=False, trajectory='fixed', max_leapfrog=256, trajectory_length=None,
        trajectory_lr=0.025):
    """Hamiltonian Monte Carlo draws from a device model: ``n_chains`` chains advanced in lock-step on the GPU, each
    iteration one trajectory of ``n_leapfrog`` leapfrog steps under a diagonal or dense metric and an accept test; the step
    size is adapted by dual averaging on the chains' mean acceptance during ``n_warmup`` iterations (target
    ``target_accept``) and jittered by ``+- jitter`` per iteration.  The metric comes from a fit, or, with
    ``adapt_metric=True``, from the chains themselves.  The trajectory length is ``n_leapfrog`` steps, or, with
    ``trajectory='chees'``, adapted across the chains.

    ``trajectory='chees'`` (ChEES-HMC; Hoffman, Radul & Sountsov 2021; no NUTS: per-chain tree depths would break the
    lock-step batch) keeps one trajectory length ``T`` shared by all chains: iteration ``t`` takes
    ``clamp(ceil(h_t T / step size), 1, max_leapfrog)`` leapfrog steps with ``h_t`` in (0, 1) the base-2 radical inverse of
    its stream index plus one, so the mean trajectory is ``T / 2``.  During warm-up ``T`` follows a stochastic gradient
    ascent (Adam without first moment, learning rate ``trajectory_lr``) on the "change in the estimator of the expected
    square" across the chains, from ``trajectory_length`` (default: the initial step size, one leapfrog step); sampling
    uses the average of its iterates.  ``n_leapfrog`` is ignored then.  It needs ``n_chains >= 2`` when there is a warm-up,
    works with both metrics and with ``adapt_metric`` (the trajectory state is carried across the windows, as the step
    size is), and costs one 8-byte host round trip per warm-up iteration; the sampling phase still runs without one.

    ``metric='dense'`` takes the whole covariance as the inverse mass (two triangular ``n_chains x D x D`` products per
    leapfrog step): ``inv_mass`` may then be (D, D) -- symmetric, positive definite -- or (D,), and defaults to the full
    ``approx.mean_and_cov(var_param)[1]`` with a fit and to the identity without one.  ``adapt_metric=True``
    (``n_warmup >= 20``) re-estimates the metric during warm-up from the cross-chain moments of doubling windows (Stan's
    schedule and regularisation; ``_adaptation_windows``): each window end costs one host round trip, and the step-size
    adaptation restarts there from the step it had reached.  With neither keyword the run is ``vb_hmc_run``'s, as ever.

    With ``var_param`` and ``approx`` (as ``bbvi`` or ``laplace_approximation`` return them) the chains start at
    ``approx.sample(var_param, n_chains)`` unless ``init`` (n_chains x D) is given, and the metric is the diagonal of
    ``approx.mean_and_cov(var_param)[1]`` unless ``inv_mass`` (D,; estimated posterior variances) is given.  Without
    them ``init`` is required and ``inv_mass`` defaults to ones.  ``step_size=None`` means ``D ** -0.25``.

    Returns a dict: ``draws`` (n_kept x C x D; None with ``keep_draws=False``) and ``logp`` (n_kept x C) of every
    ``thin``-th sampling iteration, ``n_kept = ceil(n_draws / thin)``; ``last`` (C x D); ``chain_mean`` and ``chain_var``
    (C x D; ``ddof=1`` over all ``n_draws`` sampling iterations, thinned or not); ``mean``, ``sd`` and ``rhat`` (D,) from
    them (``W`` the mean chain variance, ``B = n var(chain means)``, ``var+ = (n - 1) / n W + B / n``, ``sd = sqrt(var+)``,
    ``rhat = sqrt(var+ / W)``); ``accept_rate`` (C,); ``accept_prob`` and ``step_size_history`` (n_warmup + n_draws,);
    ``step_size`` (the sampling phase's); ``n_divergent``; ``inv_mass`` (the metric the sampling phase used: (D,), or
    (D, D) for the dense metric); ``metric``; ``adapt_windows`` (the windows ``[(start, end), ...]``, empty without
    adaptation); ``trajectory_length`` (the sampling phase's ``T``; for ``'fixed'``, ``n_leapfrog`` times the sampling
    phase's step size), ``trajectory_history`` and ``n_leapfrog_history`` (n_warmup + n_draws,; for ``'fixed'`` the
    constants ``trajectory_length`` and ``n_leapfrog``); ``n_grad_evals`` (gradient evaluations per chain: the leapfrog
    steps of all iterations plus one for the start of every engine call); ``seed`` and ``next_stream``.  A continuation
    passes ``init=res['last']``, ``step_size=res['step_size']``, ``n_warmup=0`` and ``stream_offset=res['next_stream']``,
    and, for ``'chees'``, ``trajectory='chees'`` and ``trajectory_length=res['trajectory_length']``.
    Runs on the calling process's engine; raises ``NotImplementedError`` for a ``CallableModel`` and for a sharded
    engine."""
    refuse_minibatch(model, 'hmc')
    init, inv_mass, step_size = _check_arguments(model, n_chains, n_warmup, n_draws, n_leapfrog, step_size, target_accept,
                                                 jitter, init, inv_mass, var_param, approx, thin, metric, adapt_metric,
                                                 trajectory, max_leapfrog, trajectory_length, trajectory_lr)
    dense, chees = metric == 'dense', trajectory == 'chees'
    n_chains, n_warmup, n_draws, n_leapfrog = int(n_chains), int(n_warmup), int(n_draws), int(n_leapfrog)
    fit = None if var_param is None else (approx, np.asarray(var_param, dtype=np.float64))
    init, inv_mass = _resolve_start(fit, (n_chains, model.dim), init, inv_mass, dense)
    windows = _adaptation_windows(n_warmup) if adapt_metric else []
    eng = _lib.default_engine()
    if eng.n_ranks > 1:
        raise NotImplementedError('hmc runs on one process\'s engine; a sharded engine ({} ranks) is not supported'.format(
            eng.n_ranks))
    eng.set_model(model.device_spec())
    # the route: with neither a dense metric, nor adaptation, nor ChEES, one segment through vb_hmc_run
    kw = dict(target_accept=target_accept, jitter=jitter, seed=seed, thin=thin, keep_draws=keep_draws)
    start, n_iter = dict(last=init, step_size=step_size), n_warmup + n_draws
    if chees:
        log_t0 = np.log(step_size if trajectory_length is None else float(trajectory_length))
        start['traj_state'] = np.array([log_t0, 0.0, log_t0, 0.0])
        method = partial(eng.hmc_run_chees, max_leapfrog=max_leapfrog, trajectory_lr=trajectory_lr, **kw)
    else:
        method = partial(eng.hmc_run_metric if dense or adapt_metric else eng.hmc_run, n_leapfrog=n_leapfrog, **kw)
    segments = _segments(n_warmup, n_draws, windows) if adapt_metric else [(n_warmup, n_draws, None)]
    out = _run_segments(method, segments, start, inv_mass, int(stream_offset))
    if not chees:
        out.update(trajectory_history=np.full(n_iter, n_leapfrog * out['step_size']),
                   n_leapfrog_history=np.full(n_iter, n_leapfrog, dtype=np.int64))
    traj = float(out['trajectory_history'][n_warmup])
    if chees and n_warmup == 0 and trajectory_length is not None:      # a continuation passes the length on unchanged
        traj = float(trajectory_length)
    return _results(out, n_draws, metric=metric, adapt_windows=windows, trajectory_length=traj, seed=int(seed),
                    next_stream=int(stream_offset) + n_iter)
