"""Numpy oracle of the varying-intercept (multilevel) GLM target, with the interface of ``oracle/models.py`` (``logp``,
``grad``, ``hessian``, ``hvp``) plus ``pointwise`` and ``eta``, so the functions of ``oracle.objectives`` serve as objective
oracles unchanged.

``theta = [b (p) | u (J) | omega]``, ``tau = exp(omega)``, ``eta_i = x_i' b + tau u_{g_i}``; ``b ~ N(0, prior_sd)``,
``u ~ N(0, 1)``, ``tau ~ HalfNormal(tau_sd)`` with the Jacobian of ``omega -> tau``.  The observations stay in the caller's
order (the device model sorts them by group; the oracle does not).  ``dtype=np.longdouble`` evaluates everything in extended
precision, for telling the oracle's own rounding from the device's."""
import numpy as np
from scipy.special import gammaln

LOG_2PI = np.log(2.0 * np.pi)


class MultilevelOracle:
    def __init__(self, X, y, groups, n_groups, likelihood='logistic', prior_sd=10.0, tau_sd=1.0, noise_sd=1.0,
                 dtype=np.float64):
        self.dtype = dtype
        self.X = np.asarray(X, dtype=dtype)
        self.y = np.asarray(y, dtype=dtype).ravel()
        self.groups = np.asarray(groups).astype(np.int64).ravel()
        self.J = int(n_groups)
        self.n_data, self.p = self.X.shape
        self.likelihood = likelihood
        self.prior_sd, self.tau_sd, self.noise_sd = dtype(prior_sd), dtype(tau_sd), dtype(noise_sd)
        self.dim = self.p + self.J + 1
        self.onehot = np.zeros((self.n_data, self.J), dtype=dtype)
        self.onehot[np.arange(self.n_data), self.groups] = 1.0
        if likelihood == 'poisson':
            self.obs_const = -np.asarray(gammaln(np.asarray(self.y, dtype=np.float64) + 1.0), dtype=dtype)
        elif likelihood == 'gaussian':
            self.obs_const = np.full(self.n_data, -(np.log(self.noise_sd) + dtype(0.5) * dtype(LOG_2PI)), dtype=dtype)
        else:
            self.obs_const = np.zeros(self.n_data, dtype=dtype)

    def _as2d(self, x):
        x = np.asarray(x, dtype=self.dtype)
        return x[np.newaxis, :] if x.ndim == 1 else x

    def split(self, theta):
        theta = self._as2d(theta)
        return theta[:, :self.p], theta[:, self.p:self.p + self.J], theta[:, -1]

    def eta(self, theta):
        """(N, n_data) linear predictors."""
        b, u, omega = self.split(theta)
        return b @ self.X.T + np.exp(omega)[:, None] * u[:, self.groups]

    def _terms(self, eta):
        """l(y, eta) with its normalising constant, r = dl / d eta, a = d^2 l / d eta^2."""
        y = self.y
        if self.likelihood == 'poisson':
            mu = np.exp(eta)
            return y * eta - mu + self.obs_const, y - mu, -mu
        if self.likelihood == 'gaussian':
            s2 = self.noise_sd ** 2
            return -0.5 * (y - eta) ** 2 / s2 + self.obs_const, (y - eta) / s2, np.full_like(eta, -1.0 / s2)
        t = np.exp(-np.abs(eta))
        s = np.where(eta >= 0, 1.0 / (1.0 + t), t / (1.0 + t))
        return y * eta - (np.maximum(eta, 0.0) + np.log1p(t)), y - s, -s * (1.0 - s)

    def pointwise(self, theta):
        """(N, n_data): log p(y_i | eta_i), normalised."""
        return self._terms(self.eta(theta))[0]

    def log_prior(self, theta):
        b, u, omega = self.split(theta)
        tau = np.exp(omega)
        half = self.dtype(0.5)
        pb = -half * np.sum(b * b, axis=1) / self.prior_sd ** 2 - self.p * (np.log(self.prior_sd) + half * LOG_2PI)
        pu = -half * np.sum(u * u, axis=1) - self.J * half * LOG_2PI
        pt = np.log(self.dtype(2.0)) - np.log(self.tau_sd) - half * LOG_2PI - half * tau ** 2 / self.tau_sd ** 2 + omega
        return pb + pu + pt

    def logp(self, theta):
        return np.sum(self.pointwise(theta), axis=1) + self.log_prior(theta)

    def grad(self, theta):
        b, u, omega = self.split(theta)
        tau = np.exp(omega)
        r = self._terms(self.eta(theta))[1]
        gb = r @ self.X - b / self.prior_sd ** 2
        gu = tau[:, None] * (r @ self.onehot) - u
        go = tau * np.sum(r * u[:, self.groups], axis=1) - tau ** 2 / self.tau_sd ** 2 + 1.0
        return np.concatenate([gb, gu, go[:, None]], axis=1)

    def hessian(self, m):
        """Closed form: H = sum_i a_i J_i J_i' + sum_i r_i d^2 eta_i + priors, J_i = d eta_i / d theta = [x_i | tau e_{g_i} |
        tau u_{g_i}]; d^2 eta_i / du_j domega = tau [g_i = j], d^2 eta_i / domega^2 = tau u_{g_i}."""
        m = np.asarray(m, dtype=self.dtype).ravel()
        b, u, omega = self.split(m)
        u, tau = u[0], np.exp(omega[0])
        _, r, a = self._terms(self.eta(m))
        r, a = r[0], a[0]
        p, J, D = self.p, self.J, self.dim
        Jm = np.concatenate([self.X, tau * self.onehot, (tau * u[self.groups])[:, None]], axis=1)      # (n_data, D)
        H = Jm.T @ (a[:, None] * Jm)
        mixed = tau * (r @ self.onehot)
        H[p:p + J, D - 1] += mixed
        H[D - 1, p:p + J] += mixed
        H[D - 1, D - 1] += tau * np.sum(r * u[self.groups])
        idx = np.arange(D)
        H[idx[:p], idx[:p]] -= 1.0 / self.prior_sd ** 2
        H[idx[p:p + J], idx[p:p + J]] -= 1.0
        H[D - 1, D - 1] -= 2.0 * tau ** 2 / self.tau_sd ** 2
        return H

    def hvp(self, m, v):
        return self._as2d(v) @ self.hessian(m).T
