"""TEST INFRASTRUCTURE ONLY -- posterior prediction of the regression targets in numpy: the five definitions of
``vb_glm_predict`` restated (float64 or longdouble), the numpy pipeline behind ``viabel_amd.predict`` and the closed form
for Bayesian linear regression with known noise when q is the exact posterior.  Shared by tests/test_predict_cpu.py (which
checks the restatement against the closed form and scipy) and tests/test_gpu_predict.py (which checks the device against
it)."""
import math

import numpy as np

import _loo_oracle as LO
from oracle import psis as opsis

linear_problem = LO.linear_problem
linear_posterior = LO.linear_posterior


def _lse(a, axis):
    mx = np.max(a, axis=axis, keepdims=True)
    mx = np.where(np.isfinite(mx), mx, 0.0)
    return np.log(np.sum(np.exp(a - mx), axis=axis)) + np.squeeze(mx, axis=axis)


def normalised_weights(log_w, n, dtype=np.float64):
    """``(w, log w)``: ``w_s = exp(log_w[s] - logsumexp(log_w))``; uniform without ``log_w``."""
    if log_w is None:
        log_w = np.zeros(n)
    log_w = np.asarray(log_w).astype(dtype)
    lw = log_w - _lse(log_w, 0)
    return np.exp(lw), lw


def predict_numpy(kind, theta, X_new, y_new=None, log_w=None, noise_sd=1.0, dtype=np.float64):
    """dict of ``eta_mean``, ``eta_var``, ``mean``, ``var`` and (with ``y_new``) ``lpd``, each ``(m,)``: weighted sums over
    the draws ``theta`` (S, D) with eta = X_new theta', the variances as weighted squared deviations from the weighted
    means, ``lpd`` a log-sum-exp of normalised densities.  ``dtype=np.longdouble`` carries every step in extended
    precision (the linear predictors included)."""
    theta = np.atleast_2d(np.asarray(theta)).astype(dtype)
    X_new = np.asarray(X_new).astype(dtype)
    s = theta.shape[0]
    w, lw = normalised_weights(log_w, s, dtype)
    eta = X_new @ theta.T                                  # (m, S)
    if kind == 'logistic':
        t = np.exp(-np.abs(eta))
        mu = np.where(eta >= 0, 1.0 / (1.0 + t), t / (1.0 + t))
        v = t / (1.0 + t) ** 2
    elif kind == 'poisson':
        mu = np.exp(eta)
        v = mu
    else:
        mu = eta
        v = np.full_like(eta, dtype(noise_sd) ** 2)
    live = w > 0                                           # a weight of zero adds nothing, whatever the value
    wsum = lambda a: np.sum(np.where(live, w * a, dtype(0.0)), axis=1)      # noqa: E731
    out = dict(eta_mean=wsum(eta), mean=wsum(mu))
    out['eta_var'] = wsum((eta - out['eta_mean'][:, None]) ** 2)
    out['var'] = wsum(v) + wsum((mu - out['mean'][:, None]) ** 2)
    if y_new is not None:
        y = np.asarray(y_new).astype(dtype)[:, None]
        if kind == 'logistic':
            ll = y * eta - (np.maximum(eta, 0) + np.log1p(np.exp(-np.abs(eta))))
        elif kind == 'poisson':
            ll = y * eta - np.exp(eta) - np.array([math.lgamma(float(c) + 1.0) for c in y[:, 0]], dtype=dtype)[:, None]
        else:
            ll = (-0.5 * ((y - eta) / dtype(noise_sd)) ** 2 - np.log(dtype(noise_sd))
                  - 0.5 * np.log(2.0 * np.pi * dtype(1.0)))
        out['lpd'] = _lse(lw[None, :] + ll, 1)
    return out


def eta_var_moment_form(theta, X_new, log_w=None):
    """The formula the entry must NOT use: ``E[eta^2] - E[eta]^2`` in float64."""
    theta = np.atleast_2d(theta)
    w, _ = normalised_weights(log_w, theta.shape[0])
    eta = X_new @ theta.T
    return np.sum(w * eta * eta, axis=1) - np.sum(w * eta, axis=1) ** 2


def predict_pipeline_numpy(kind, samples, log_ratios, X_new, y_new, weights='psis', reff=1.0, noise_sd=1.0):
    """What ``viabel_amd.predict`` computes from the same draws and ratios, in numpy: ``(result dict, khat)``."""
    log_w, khat = (None, None) if weights is None else opsis.psis_smooth(log_ratios, reff)
    return predict_numpy(kind, samples, X_new, y_new, log_w, noise_sd), khat


def linear_predict_closed_form(X_new, y_new, post_mean, post_cov, noise_sd):
    """Linear model, q = the exact posterior N(post_mean, post_cov): eta_i ~ N(x_i' m, x_i' V x_i), y_i ~ N(x_i' m,
    x_i' V x_i + noise_sd^2)."""
    em = X_new @ post_mean
    ev = np.einsum('ij,jk,ik->i', X_new, post_cov, X_new)
    var = ev + noise_sd ** 2
    out = dict(eta_mean=em, eta_var=ev, mean=em.copy(), var=var)
    if y_new is not None:
        out['lpd'] = -0.5 * np.log(2.0 * np.pi * var) - 0.5 * (y_new - em) ** 2 / var
    return out


def linear_holdout(n_new=33, seed=7):
    """``n_new`` fresh rows for the problem of ``linear_problem``: same design law, same coefficients' scale."""
    rng = np.random.RandomState(seed)
    X_new = rng.randn(n_new, 8) / np.sqrt(8.0)
    y_new = X_new @ rng.randn(8) + rng.randn(n_new)
    return X_new, y_new
