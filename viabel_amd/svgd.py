"""Stein variational gradient descent on the device: a non-parametric variational method for the targets on which the
Gaussian families are visibly wrong.

Liu & Wang (2016) move a set of particles along

    phi(x_i) = 1/n sum_j [ k(x_j, x_i) grad log p(x_j) + grad_{x_j} k(x_j, x_i) ]

which needs no family, no density ratio and no noise.  :func:`svgd` is one device-resident run (``vb_svgd_run``,
``csrc/vb_svgd.hip``; ``DESIGN.md`` 4.27): scores from the gradient pipeline the objectives use, all pairs on the device,
the package's optimisers as the step, one host synchronisation."""
import numpy as np

from viabel_amd import _lib
from viabel_amd.models import CallableModel, DeviceModel, refuse_minibatch
from viabel_amd.optimization import Adagrad, StochasticGradientOptimizer

__all__ = ['svgd']

# The default optimiser is Adagrad(DEFAULT_LEARNING_RATE).  Adagrad's first step moves every coordinate by the learning
# rate whatever the size of the direction, so the rate is a length in the target's own units.  Chosen from
# `python examples/svgd.py 1024 0.03 0.1 0.3` (a four-dimensional funnel, 1024 particles started from a mean-field fit,
# 1000 iterations): the kernel Stein discrepancy of the particles ends at 0.051 / 0.054 / 0.106 and the standard deviation
# of the funnel's scale coordinate (1 for the target, 0.38 for the fit) at 0.79 / 0.84 / 0.84 -- 0.1 is the largest rate
# that does not cost discrepancy.  Targets whose scales are far from 1 want a rate of their size (tests/test_gpu_svgd.py
# runs a Gaussian with standard deviations from 0.1 to 10 at 0.5).
DEFAULT_LEARNING_RATE = 0.1


def _check_arguments(model, n_particles, n_iters, init, var_param, approx, optimizer, scale, bandwidth):
    """Everything that can be refused without an engine; returns ``(init, scale, optimizer)``: ``init`` an array or None
    (the fit supplies the starts), ``scale`` an array, None or ``'auto'``."""
    if not isinstance(model, DeviceModel):
        raise TypeError('svgd needs a viabel_amd device model (its scores are device code); got {}'.format(
            type(model).__name__))
    if isinstance(model, CallableModel):
        raise NotImplementedError('svgd moves the particles without host synchronisation: a CallableModel (a host callback) '
                                  'cannot be its target; write the density as a SourceModel')
    for name, v in (('n_particles', n_particles), ('n_iters', n_iters)):
        if isinstance(v, bool) or int(v) != v or v < 1:
            raise ValueError('{} must be an integer >= 1'.format(name))
    if n_particles > _lib.SVGD_MAX_PARTICLES:
        raise NotImplementedError('svgd takes at most {} particles; got {}'.format(_lib.SVGD_MAX_PARTICLES, n_particles))
    if (var_param is None) != (approx is None):
        raise ValueError('var_param and approx must be given together')
    if var_param is None and init is None:
        raise ValueError('either init or both var_param and approx must be given')
    d = model.dim
    if init is not None:
        init = np.ascontiguousarray(init, dtype=np.float64)
        if init.shape != (n_particles, d):
            raise ValueError('init must have shape ({}, {}); got {}'.format(n_particles, d, init.shape))
        if not np.all(np.isfinite(init)):
            raise ValueError('init must be finite')
    if isinstance(scale, str):
        if scale != 'auto':
            raise ValueError("scale must be 'auto', None or an array")
        if var_param is None:
            scale = None      # without a fit there is nothing to take it from
    elif scale is not None:
        _lib.svgd_arguments(np.zeros((1, d)), scale=scale)
        scale = np.ascontiguousarray(scale, dtype=np.float64)
    _lib.svgd_arguments(np.zeros((1, d)), bandwidth=bandwidth)
    if optimizer is None:
        optimizer = Adagrad(DEFAULT_LEARNING_RATE)
    if not isinstance(optimizer, StochasticGradientOptimizer) or optimizer._device_kind is None:
        raise TypeError('optimizer must be one of StochasticGradientOptimizer, RMSProp, Adam and Adagrad; got {}'.format(
            type(optimizer).__name__))
    if np.ndim(optimizer._learning_rate) != 0:
        raise ValueError('the optimizer needs a scalar learning rate')
    if optimizer._weight_decay != 0:
        raise ValueError('svgd does not apply weight decay to the particles; pass an optimizer with weight_decay=0')
    return init, scale, optimizer


def svgd(model, *, n_particles=256, n_iters=1000, init=None, var_param=None, approx=None, optimizer=None, scale='auto',
         bandwidth='median', seed=1):
    """Stein variational gradient descent (Liu & Wang 2016) on a device model: ``n_particles`` particles moved for
    ``n_iters`` iterations along ``phi`` (above) with the RBF kernel ``exp(-|y - y'|^2 / h)`` of the rescaled, centred
    coordinates ``y = (x - mean) / scale``, the whole run in one device call (``vb_svgd_run``).

    With ``var_param`` and ``approx`` (as ``bbvi`` or ``laplace_approximation`` return them) the particles start at
    ``approx.sample(var_param, n_particles)`` unless ``init`` (n_particles x D) is given, and ``scale='auto'`` is the
    approximation's standard deviations.  Without them ``init`` is required and ``scale='auto'`` means None (ones).  An
    array ``scale`` (D,) is taken as given.  ``bandwidth``: ``'median'`` (``h`` = the lower median of the squared pair
    distances over ``log(n + 1)``, selected exactly on the device in every iteration) or a positive number.

    ``optimizer``: one of the package's ``StochasticGradientOptimizer`` / ``RMSProp`` / ``Adam`` / ``Adagrad`` objects,
    stepping with gradient ``-phi`` in their own arithmetic; the default is ``Adagrad(0.1)`` (``DEFAULT_LEARNING_RATE``:
    Adagrad's first step moves every coordinate by the learning rate, so the rate is a length in the target's units).
    The optimiser's state is set when the call returns: a second call with ``init=res['particles']`` and
    ``optimizer=res['optimizer']`` continues the run.  ``seed`` is ``approx.sample``'s (the starts: a fresh
    ``RandomState(seed)``); the run itself uses no random numbers.

    Returns a dict: ``particles`` (n x D) and their ``logp`` (n,); ``mean``, ``sd`` (``ddof=1``) and ``cov`` of the
    particles; ``bandwidth_history``, ``phi_rms_history`` (``sqrt(mean phi^2)``) and ``logp_history`` (the particles' mean
    log density), each (n_iters,) and taken at the start of the iteration; ``optimizer``; ``scale`` and ``n_iters``.
    Runs on the calling process's engine; raises ``NotImplementedError`` for a ``CallableModel``, a
    ``MinibatchRegressionModel`` and a sharded engine."""
    refuse_minibatch(model, 'svgd')
    init, scale, optimizer = _check_arguments(model, n_particles, n_iters, init, var_param, approx, optimizer, scale,
                                              bandwidth)
    n, d, n_iters = int(n_particles), model.dim, int(n_iters)
    if var_param is not None:
        var_param = np.asarray(var_param, dtype=np.float64)
        if isinstance(scale, str):
            scale = np.ascontiguousarray(np.sqrt(np.diag(approx.mean_and_cov(var_param)[1])), dtype=np.float64)
            if not (np.all(scale > 0.0) and np.all(np.isfinite(scale))):
                raise ValueError('the approximation has no finite positive variances to take the scale from; pass scale')
        if init is None:
            init = np.ascontiguousarray(approx.sample(var_param, n, seed=seed), dtype=np.float64)
            if init.shape != (n, d):
                raise ValueError('approx.sample returned shape {}, expected ({}, {})'.format(init.shape, n, d))
    eng = _lib.default_engine()
    if eng.n_ranks > 1:
        raise NotImplementedError('svgd runs on one process\'s engine; a sharded engine ({} ranks) is not supported'.format(
            eng.n_ranks))
    eng.set_model(model.device_spec())
    p = n * d
    out = eng.svgd_run(init, n_iters, optimizer._device_kind, optimizer._device_hyper(), state=optimizer._device_state(p),
                       scale=scale, bandwidth=bandwidth)
    state = out['state']
    optimizer._set_device_state(state, p)
    x = out['particles']
    results = dict(particles=x, logp=out['logp'], mean=x.mean(axis=0),
                   sd=x.std(axis=0, ddof=1) if n > 1 else np.full(d, np.nan),
                   cov=np.atleast_2d(np.cov(x, rowvar=False)) if n > 1 else np.full((d, d), np.nan),
                   bandwidth_history=out['bandwidth_history'], phi_rms_history=out['phi_rms_history'],
                   logp_history=out['logp_history'], optimizer=optimizer, scale=scale, n_iters=n_iters)
    print('svgd: {} particles, {} iterations: rms(phi) {:.4g} -> {:.4g}, mean log p {:.4g} -> {:.4g}, bandwidth {:.4g}'.format(
        n, n_iters, results['phi_rms_history'][0], results['phi_rms_history'][-1], results['logp_history'][0],
        float(np.mean(results['logp'])), results['bandwidth_history'][-1]))
    return results
