"""TEST INFRASTRUCTURE ONLY -- the PSIS-LOO pipeline in numpy on top of ``oracle.psis`` and the closed-form leave-one-out
predictive density of Bayesian linear regression with known noise.  Shared by tests/test_loo_cpu.py (which checks this
restatement against the closed form) and tests/test_gpu_loo.py (which checks the device against it)."""
import math

import numpy as np

from oracle import psis as opsis


def close_k(k, ref):
    """k-hat agreement: 1e-10 relative; inf matches inf, NaN matches NaN."""
    if np.isnan(ref):
        return bool(np.isnan(k))
    if np.isinf(ref):
        return bool(np.isinf(k)) and (k > 0) == (ref > 0)
    return bool(abs(k - ref) <= 1e-10 * max(1.0, abs(ref)))


def loo_numpy(log_lik, log_ratios=None, reff=1.0, log_w=None):
    """``(loos, ks, lpd)`` for ``log_lik`` (draws x observations): observation i's weights are the Pareto-smoothed
    ``log_ratios - log_lik[:, i]`` (``-log_lik[:, i]`` without ratios, as ``viabel/_psis.py:99-106``); ``lpd`` under the
    full-data smoothed log weights ``log_w`` (None without them)."""
    log_lik = np.asarray(log_lik, dtype=np.float64)
    n_obs = log_lik.shape[1]
    loos, ks = np.empty(n_obs), np.empty(n_obs)
    lpd = np.empty(n_obs) if log_w is not None else None
    for i in range(n_obs):
        lw = -log_lik[:, i] if log_ratios is None else log_ratios - log_lik[:, i]
        s, ks[i] = opsis.psis_smooth(lw, reff)
        loos[i] = opsis.log_sum_exp(s + log_lik[:, i])
        if log_w is not None:
            lpd[i] = opsis.log_sum_exp(log_w + log_lik[:, i])
    return loos, ks, lpd


def glm_pointwise_numpy(kind, X, y, theta, noise_sd=1.0):
    """Normalised ``log p(y_i | x_i' theta_s)``, ``(S, n_data)``, of the three regression likelihoods."""
    eta = np.atleast_2d(theta) @ X.T
    if kind == 'logistic':
        return y * eta - np.logaddexp(0.0, eta)
    if kind == 'poisson':
        return y * eta - np.exp(eta) - np.array([math.lgamma(v + 1.0) for v in y])
    return -0.5 * ((y - eta) / noise_sd) ** 2 - math.log(noise_sd) - 0.5 * math.log(2.0 * math.pi)


def linear_posterior(X, y, prior_sd, noise_sd):
    """Mean and covariance of the Gaussian posterior of ``y ~ N(X b, noise_sd)``, ``b ~ N(0, prior_sd)``."""
    P = np.eye(X.shape[1]) / prior_sd ** 2 + X.T @ X / noise_sd ** 2
    V = np.linalg.inv(P)
    return V @ (X.T @ y) / noise_sd ** 2, 0.5 * (V + V.T)


def linear_loo_closed_form(X, y, prior_sd, noise_sd):
    """``log p(y_i | y_-i) = log N(y_i; x_i' m_-i, noise_sd^2 + x_i' V_-i x_i)`` with the posterior of the other
    observations (the rank-one downdate of the full posterior, formed directly)."""
    n, d = X.shape
    P = np.eye(d) / prior_sd ** 2 + X.T @ X / noise_sd ** 2
    b = X.T @ y / noise_sd ** 2
    out = np.empty(n)
    for i in range(n):
        Vi = np.linalg.inv(P - np.outer(X[i], X[i]) / noise_sd ** 2)
        mi = Vi @ (b - X[i] * y[i] / noise_sd ** 2)
        var = noise_sd ** 2 + X[i] @ Vi @ X[i]
        out[i] = -0.5 * math.log(2.0 * math.pi * var) - 0.5 * (y[i] - X[i] @ mi) ** 2 / var
    return out


def linear_problem(n_draws=4096):
    """The inputs of the closed-form comparison: X = RandomState(1).randn(200, 8) / sqrt(8), y = X b + randn,
    prior_sd = 10, noise_sd = 1; and the next ``n_draws x 8`` standard normals of the same stream, from which the CPU
    tests form their posterior draws."""
    rng = np.random.RandomState(1)
    X = rng.randn(200, 8) / np.sqrt(8.0)
    b = rng.randn(8)
    y = X @ b + rng.randn(200)
    return X, y, 10.0, 1.0, rng.randn(n_draws, 8)


def gaussian_log_density(theta, mean, chol):
    """log N(theta_s; mean, chol chol') for the rows of theta."""
    d = mean.size
    z = np.linalg.solve(chol, (theta - mean).T)
    return -0.5 * np.sum(z * z, axis=0) - np.sum(np.log(np.diag(chol))) - 0.5 * d * math.log(2.0 * math.pi)


def linear_log_joint(X, y, prior_sd, noise_sd, theta):
    """log p(theta_s, y) of the linear regression (normalised likelihood and prior)."""
    ll = glm_pointwise_numpy('linear', X, y, theta, noise_sd).sum(axis=1)
    d = X.shape[1]
    return ll - 0.5 * np.sum(theta ** 2, axis=1) / prior_sd ** 2 - d * (math.log(prior_sd) + 0.5 * math.log(2.0 * math.pi))
