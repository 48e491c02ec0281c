"""Pareto smoothed importance sampling (``viabel/_psis.py``), smoothed on the GPU.

``psislw`` keeps the reference's signature and return convention (``_psis.py:113-209``): log weights of shape
``(n,)`` or ``(n, m)`` (m sets, one per column), smoothed weights normalised so that each set's log-sum-exp is 0,
and the Pareto tail indices.  The tail selection, the generalised-Pareto fit (``gpdfitnew``, ``_psis.py:212-332``)
and the quantile replacement (``gpinv``, ``:335-377``) run in one HIP kernel (``csrc/vb_psis.hip``) through
``vb_psis_smooth``, for the columns of a matrix in one launch of ``csrc/vb_psis_batch.hip`` (``vb_psis_smooth_batch``);
they are not re-exported as host functions.
"""
import numpy as np

from . import _lib

__all__ = ['psislw', 'psisloo', 'sumlogs']


def sumlogs(x, axis=None):
    """``log(sum(exp(x)))`` along ``axis`` without overflow (``_psis.py:380-396``)."""
    x = np.asarray(x, dtype=np.float64)
    m = np.max(x, axis=axis, keepdims=True)
    return np.log(np.sum(np.exp(x - m), axis=axis)) + np.squeeze(m, axis=axis)


def _tail_size(n, Reff):
    """Number of tail values the smoothing fits (``_psis.py:158``)."""
    return int(np.ceil(min(0.2 * n, 3.0 * np.sqrt(n / Reff))))


def batch_capacity(n, Reff=1.0):
    """Does a weight vector of length ``n`` fit the batched kernel (``csrc/vb_psis_batch.hip``: at most 16 384 values
    with a tail of at most 1024)?  Longer ones are smoothed one launch per vector."""
    return 2 <= n <= _lib.PSIS_BATCH_MAX_N and Reff > 0 and _tail_size(n, Reff) <= _lib.PSIS_BATCH_MAX_TAIL


def psislw(lw, Reff=1.0, overwrite_lw=False):
    """Pareto smoothed importance sampling of log weights (``_psis.py:113-209``).  A 2-D ``lw`` holds one weight set per
    column; all columns are smoothed by one kernel launch (``vb_psis_smooth_batch``) when their length fits
    (:func:`batch_capacity`), column by column otherwise."""
    lw = np.asarray(lw, dtype=np.float64)
    if lw.ndim not in (1, 2):
        raise ValueError('Argument `lw` must be 1 or 2 dimensional.')
    n = lw.shape[0]
    if n <= 1:
        raise ValueError('More than one log-weight needed.')
    eng = _lib.default_engine()
    if lw.ndim == 1:
        out, k = eng.psis_smooth(n, lw, reff=Reff)
        if overwrite_lw:
            lw[...] = out
            out = lw
        return out, k
    if batch_capacity(n, Reff) and lw.shape[1] > 0:
        # the kernel wants each vector contiguous: the transpose of a Fortran-ordered argument is that already (and is
        # smoothed in place under overwrite_lw), anything else is copied once
        out = lw if overwrite_lw else np.empty_like(lw, order='F')
        rows = np.ascontiguousarray(lw.T)
        dst = out.T if out.T.flags.c_contiguous else np.empty_like(rows)
        _, ks = eng.psis_smooth_batch(rows, reff=Reff, out=dst)
        if dst is not out.T:
            out[...] = dst.T
        return out, ks
    out = lw if overwrite_lw else np.empty_like(lw, order='F')
    ks = np.empty(lw.shape[1])
    for j in range(lw.shape[1]):
        out[:, j], ks[j] = eng.psis_smooth(n, np.ascontiguousarray(lw[:, j]), reff=Reff)
    return out, ks


def psisloo(log_lik, log_ratios=None, **kwargs):
    """PSIS leave-one-out log predictive densities (``_psis.py:70-110``): ``log_lik`` is ``(n, m)``, ``n`` draws by ``m``
    observations; returns ``(loo, loos, ks)``.  The reference assumes draws from the exact posterior; for draws of an
    approximation ``q`` pass ``log_ratios[s] = log p(theta_s, y) - log q(theta_s)`` and the vectors smoothed are
    ``log_ratios[:, None] - log_lik``."""
    log_lik = np.asarray(log_lik, dtype=np.float64)
    if log_lik.ndim != 2:
        raise ValueError('Argument `log_lik` must be 2 dimensional (draws by observations).')
    kwargs.pop('overwrite_lw', None)
    if log_ratios is None:
        lw, ks = psislw(-log_lik, **kwargs)
    else:
        log_ratios = np.asarray(log_ratios, dtype=np.float64)
        if log_ratios.shape != (log_lik.shape[0],):
            raise ValueError('log_ratios must have shape ({},): one ratio per draw'.format(log_lik.shape[0]))
        lw, ks = psislw(log_ratios[:, np.newaxis] - log_lik, **kwargs)
    loos = sumlogs(lw + log_lik, axis=0)
    return loos.sum(), loos, ks
