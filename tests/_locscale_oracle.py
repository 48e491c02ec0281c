"""Numpy oracle of the location-scale regression target, with the interface of ``oracle/models.py`` (``logp``, ``grad``,
``hessian``, ``hvp``) plus ``pointwise``, ``eta`` and ``log_scale``, so the functions of ``oracle.objectives`` serve as
objective oracles unchanged.

``theta = [b (p) | g (q)]``, ``eta_i = x_i' b``, ``s_i = w_i' g``, ``z_i = (y_i - eta_i) exp(-s_i)``; ``b ~ N(0, prior_sd)``,
``g ~ N(0, scale_prior_sd)``; Gaussian or Student-t (fixed ``df``) observations.  ``W=None`` is the constant scale: a column of
ones.  ``dtype=np.longdouble`` evaluates everything in extended precision, for telling the oracle's own rounding from the
device's."""
import numpy as np
from scipy.special import gammaln

LOG_2PI = np.log(2.0 * np.pi)


class LocScaleOracle:
    def __init__(self, X, y, W=None, likelihood='gaussian', df=4.0, prior_sd=10.0, scale_prior_sd=1.0, dtype=np.float64):
        self.dtype = dtype
        self.X = np.asarray(X, dtype=dtype)
        self.y = np.asarray(y, dtype=dtype).ravel()
        self.n_data, self.p = self.X.shape
        self.W = np.ones((self.n_data, 1), dtype=dtype) if W is None else np.asarray(W, dtype=dtype)
        self.q = self.W.shape[1]
        self.likelihood = likelihood
        self.df, self.prior_sd, self.scale_prior_sd = dtype(df), dtype(prior_sd), dtype(scale_prior_sd)
        self.dim = self.p + self.q
        if likelihood == 'student_t':
            nu = float(df)
            self.obs_const = dtype(gammaln(0.5 * (nu + 1.0)) - gammaln(0.5 * nu)) - dtype(0.5) * np.log(self.df * dtype(np.pi))
        else:
            self.obs_const = -dtype(0.5) * dtype(LOG_2PI)

    def _as2d(self, x):
        x = np.asarray(x, dtype=self.dtype)
        return x[np.newaxis, :] if x.ndim == 1 else x

    def split(self, theta):
        theta = self._as2d(theta)
        return theta[:, :self.p], theta[:, self.p:]

    def eta(self, theta):
        """(N, n_data) mean predictors."""
        return self.split(theta)[0] @ self.X.T

    def log_scale(self, theta):
        """(N, n_data) log-scale predictors s_i."""
        return self.split(theta)[1] @ self.W.T

    def _terms(self, eta, s):
        """l_i with its normalising constant; its derivatives (l_eta, l_s); the second derivatives (l_ee, l_es, l_ss)."""
        es = np.exp(-s)
        z = (self.y - eta) * es
        z2 = z * z
        if self.likelihood == 'student_t':
            nu = self.df
            ll = self.obs_const - s - (nu + 1) / 2 * np.log1p(z2 / nu)
            phi = (nu + 1) * z / (nu + z2)                   # k_i z_i
            dphi = (nu + 1) * (nu - z2) / (nu + z2) ** 2
        else:
            ll = self.obs_const - s - z2 / 2
            phi, dphi = z, np.ones_like(z)
        mixed = dphi * z + phi
        return ll, (phi * es, phi * z - 1), (-dphi * es * es, -mixed * es, -mixed * z)

    def pointwise(self, theta):
        """(N, n_data): log p(y_i | eta_i, sigma_i), normalised."""
        return self._terms(self.eta(theta), self.log_scale(theta))[0]

    def log_prior(self, theta):
        b, g = self.split(theta)
        half = self.dtype(0.5)
        pb = -half * np.sum(b * b, axis=1) / self.prior_sd ** 2 - self.p * (np.log(self.prior_sd) + half * LOG_2PI)
        pg = -half * np.sum(g * g, axis=1) / self.scale_prior_sd ** 2 - self.q * (np.log(self.scale_prior_sd) + half * LOG_2PI)
        return pb + pg

    def logp(self, theta):
        return np.sum(self.pointwise(theta), axis=1) + self.log_prior(theta)

    def grad(self, theta):
        b, g = self.split(theta)
        r_eta, r_s = self._terms(self.eta(theta), self.log_scale(theta))[1]
        return np.concatenate([r_eta @ self.X - b / self.prior_sd ** 2, r_s @ self.W - g / self.scale_prior_sd ** 2], axis=1)

    def hessian(self, m):
        """Closed form: both predictors are linear in theta, so with J = [X 0; 0 W] the Hessian is J' diag(a) J over the
        three second derivatives of l_i in (eta_i, s_i) -- the (b, b), (g, g) blocks and the cross terms -- plus the priors."""
        m = np.asarray(m, dtype=self.dtype).ravel()
        l_ee, l_es, l_ss = (a[0] for a in self._terms(self.eta(m), self.log_scale(m))[2])
        p, D = self.p, self.dim
        H = np.zeros((D, D), dtype=self.dtype)
        H[:p, :p] = self.X.T @ (l_ee[:, None] * self.X)
        H[:p, p:] = self.X.T @ (l_es[:, None] * self.W)
        H[p:, :p] = H[:p, p:].T
        H[p:, p:] = self.W.T @ (l_ss[:, None] * self.W)
        idx = np.arange(D)
        H[idx[:p], idx[:p]] -= 1.0 / self.prior_sd ** 2
        H[idx[p:], idx[p:]] -= 1.0 / self.scale_prior_sd ** 2
        return H

    def hvp(self, m, v):
        return self._as2d(v) @ self.hessian(m).T
