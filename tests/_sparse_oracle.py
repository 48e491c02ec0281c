"""Numpy float64 restatement of the flat GLM density on a dense design matrix -- what ``SparseRegressionModel`` must equal on
``model.to_dense()`` -- with the interface of ``oracle/models.py`` (``logp``, ``grad``) plus ``pointwise``, so the functions of
``oracle.objectives`` serve as objective oracles unchanged.  No scipy: ``log y!`` through ``math.lgamma``.

    f(theta) = sum_i log p(y_i | x_i' theta) - |theta|^2 / (2 sd^2) - p (log sd + log(2 pi) / 2)
    logistic: y eta - log(1 + exp(eta));  poisson: y eta - exp(eta) - log y!;
    gaussian: -(y - eta)^2 / (2 s^2) - log s - log(2 pi) / 2
"""
import math

import numpy as np

LOG_2PI = math.log(2.0 * math.pi)


def terms(likelihood, y, eta, noise_sd=1.0):
    """(normalised log-likelihood terms, d term / d eta), element-wise."""
    if likelihood == 'logistic':
        return y * eta - np.logaddexp(0.0, eta), y - 0.5 * (1.0 + np.tanh(0.5 * eta))
    if likelihood == 'poisson':
        mu = np.exp(eta)
        lfact = np.array([math.lgamma(v + 1.0) for v in np.ravel(y)]).reshape(np.shape(y))
        return y * eta - mu - lfact, y - mu
    if likelihood == 'gaussian':
        r = (y - eta) / noise_sd ** 2
        return -0.5 * r * (y - eta) - math.log(noise_sd) - 0.5 * LOG_2PI, r
    raise ValueError(likelihood)


class SparseGLMOracle:
    def __init__(self, X, y, likelihood='logistic', prior_sd=10.0, noise_sd=1.0):
        self.X = np.asarray(X, dtype=np.float64)
        self.y = np.asarray(y, dtype=np.float64).ravel()
        self.n_data, self.dim = self.X.shape
        self.likelihood, self.prior_sd, self.noise_sd = likelihood, float(prior_sd), float(noise_sd)

    @staticmethod
    def _as2d(x):
        x = np.asarray(x, dtype=np.float64)
        return x[np.newaxis, :] if x.ndim == 1 else x

    def pointwise(self, theta):
        """(N, n_data): log p(y_i | eta_i), normalised."""
        return terms(self.likelihood, self.y, self._as2d(theta) @ self.X.T, self.noise_sd)[0]

    def log_prior(self, theta):
        theta = self._as2d(theta)
        return -0.5 * np.sum(theta * theta, axis=1) / self.prior_sd ** 2 - self.dim * (math.log(self.prior_sd) + 0.5 * LOG_2PI)

    def logp(self, theta):
        return np.sum(self.pointwise(theta), axis=1) + self.log_prior(theta)

    def grad(self, theta):
        theta = self._as2d(theta)
        r = terms(self.likelihood, self.y, theta @ self.X.T, self.noise_sd)[1]
        return r @ self.X - theta / self.prior_sd ** 2

    def hessian(self, m):
        """Closed form at one point: X' diag(d^2 l_i / d eta_i^2) X - I / sd^2."""
        eta = self.X @ np.asarray(m, dtype=np.float64).ravel()
        if self.likelihood == 'logistic':
            mu = 0.5 * (1.0 + np.tanh(0.5 * eta))
            w = -mu * (1.0 - mu)
        elif self.likelihood == 'poisson':
            w = -np.exp(eta)
        else:
            w = -np.ones_like(eta) / self.noise_sd ** 2
        return self.X.T @ (w[:, None] * self.X) - np.eye(self.dim) / self.prior_sd ** 2

    def hvp(self, m, v):
        return self._as2d(v) @ self.hessian(m).T
