"""TEST INFRASTRUCTURE ONLY -- numpy oracle of the one-hidden-layer neural-network regression target, with the interface of
``oracle/models.py`` (``logp``, ``grad``), so the functions of ``oracle.objectives`` serve as objective oracles unchanged;
plus the pointwise terms and the prediction of ``vb_nn_predict`` restated.

Parameter layout unit-major, ``theta = [w_0 | ... | w_{h-1} | a | v | c]`` with ``w_k`` of length ``p``; every coordinate
carries the ``N(0, prior_sd)`` prior::

    t_ik = tanh(x_i' w_k + a_k),   eta_i = c + sum_k v_k t_ik
    f    = sum_i log p(y_i | eta_i) - |theta|^2 / (2 sd^2) - dim (log sd + log(2 pi) / 2)
"""
import math

import numpy as np

LOG_2PI = np.log(2.0 * np.pi)
KINDS = ('gaussian', 'logistic', 'poisson')


def _as2d(x):
    x = np.asarray(x, dtype=np.float64)
    return x[np.newaxis, :] if x.ndim == 1 else x


def _lse(a, axis):
    mx = np.max(a, axis=axis, keepdims=True)
    mx = np.where(np.isfinite(mx), mx, 0.0)
    return np.log(np.sum(np.exp(a - mx), axis=axis)) + np.squeeze(mx, axis=axis)


def log_lik(kind, y, eta, noise_sd=1.0):
    """Normalised ``log p(y | eta)``, ``y`` broadcast against ``eta``; overflow-safe for the logit."""
    if kind == 'logistic':
        return y * eta - (np.maximum(eta, 0.0) + np.log1p(np.exp(-np.abs(eta))))
    if kind == 'poisson':
        lg = np.vectorize(lambda c: math.lgamma(c + 1.0))(np.asarray(y, dtype=np.float64))
        return y * eta - np.exp(eta) - lg
    return -0.5 * ((y - eta) / noise_sd) ** 2 - np.log(noise_sd) - 0.5 * LOG_2PI


def residual(kind, y, eta, noise_sd=1.0):
    """``d log p(y | eta) / d eta``."""
    if kind == 'logistic':
        t = np.exp(-np.abs(eta))
        return y - np.where(eta >= 0, 1.0 / (1.0 + t), t / (1.0 + t))
    if kind == 'poisson':
        return y - np.exp(eta)
    return (y - eta) / noise_sd ** 2


class NeuralNetOracle:
    def __init__(self, X, y, n_hidden, likelihood='gaussian', prior_sd=1.0, noise_sd=1.0):
        assert likelihood in KINDS
        self.X = np.asarray(X, dtype=np.float64)
        self.y = np.asarray(y, dtype=np.float64).ravel()
        self.h = int(n_hidden)
        self.n_data, self.p = self.X.shape
        self.kind = likelihood
        self.prior_sd, self.noise_sd = float(prior_sd), float(noise_sd)
        self.dim = self.h * (self.p + 2) + 1

    def unpack(self, theta):
        theta = _as2d(theta)
        h, p = self.h, self.p
        return (theta[:, :h * p].reshape(-1, h, p), theta[:, h * p:h * p + h], theta[:, h * p + h:h * p + 2 * h],
                theta[:, -1])

    def pre(self, theta, X=None):
        """(N, n, h) pre-activations ``x_i' w_k + a_k`` at the rows of ``X`` (the bound design without it)."""
        W, a, _, _ = self.unpack(theta)
        return np.einsum('nkj,ij->nik', W, self.X if X is None else X) + a[:, None, :]

    def eta(self, theta, X=None):
        """(N, n) network outputs."""
        _, _, v, c = self.unpack(theta)
        return c[:, None] + np.einsum('nik,nk->ni', np.tanh(self.pre(theta, X)), v)

    def pointwise(self, theta):
        return log_lik(self.kind, self.y[None, :], self.eta(theta), self.noise_sd)

    def log_prior(self, theta):
        theta = _as2d(theta)
        return -0.5 * np.sum(theta * theta, axis=1) / self.prior_sd ** 2 - self.dim * (np.log(self.prior_sd) + 0.5 * LOG_2PI)

    def logp(self, theta):
        return np.sum(self.pointwise(theta), axis=1) + self.log_prior(theta)

    def grad(self, theta):
        theta = _as2d(theta)
        _, _, v, c = self.unpack(theta)
        t = np.tanh(self.pre(theta))                                          # (N, n, h)
        eta = c[:, None] + np.einsum('nik,nk->ni', t, v)
        r = residual(self.kind, self.y[None, :], eta, self.noise_sd)          # (N, n)
        delta = r[:, :, None] * v[:, None, :] * (1.0 - t * t)                 # (N, n, h)
        gw = np.einsum('nik,ij->nkj', delta, self.X).reshape(theta.shape[0], self.h * self.p)
        g = np.concatenate([gw, delta.sum(axis=1), np.einsum('ni,nik->nk', r, t), r.sum(axis=1)[:, None]], axis=1)
        return g - theta / self.prior_sd ** 2

    def predict(self, theta, X_new=None, y_new=None, log_w=None):
        """dict of ``eta_mean``, ``eta_var``, ``mean``, ``var`` and (with a response) ``lpd``, each ``(m,)``: the
        definitions of ``vb_glm_predict`` with the network's output as eta; ``X_new=None``: the bound design, whose
        responses ``y_new=None`` then means."""
        theta = _as2d(theta)
        if X_new is None:
            X_new = self.X
            y_new = self.y if y_new is None else y_new
        s = theta.shape[0]
        lw = np.zeros(s) if log_w is None else np.asarray(log_w, dtype=np.float64)
        lw = lw - _lse(lw, 0)
        w = np.exp(lw)
        eta = self.eta(theta, np.asarray(X_new, dtype=np.float64)).T           # (m, S)
        if self.kind == 'logistic':
            t = np.exp(-np.abs(eta))
            mu = np.where(eta >= 0, 1.0 / (1.0 + t), t / (1.0 + t))
            var = t / (1.0 + t) ** 2
        elif self.kind == 'poisson':
            mu = np.exp(eta)
            var = mu
        else:
            mu = eta
            var = np.full_like(eta, self.noise_sd ** 2)
        live = w > 0                                                          # a weight of zero adds nothing
        wsum = lambda a: np.sum(np.where(live, w * a, 0.0), axis=1)           # noqa: E731
        out = dict(eta_mean=wsum(eta), mean=wsum(mu))
        out['eta_var'] = wsum((eta - out['eta_mean'][:, None]) ** 2)
        out['var'] = wsum(var) + wsum((mu - out['mean'][:, None]) ** 2)
        if y_new is not None:
            ll = log_lik(self.kind, np.asarray(y_new, dtype=np.float64)[:, None], eta, self.noise_sd)
            out['lpd'] = _lse(lw[None, :] + ll, 1)
        return out


def response(kind, rng, eta, noise_sd=1.0):
    """Responses of the likelihood ``kind`` at the outputs ``eta``."""
    if kind == 'logistic':
        return (rng.rand(eta.size) < 1.0 / (1.0 + np.exp(-eta))).astype(float)
    if kind == 'poisson':
        return rng.poisson(np.exp(np.clip(eta, -5.0, 3.0))).astype(float)
    return eta + noise_sd * rng.randn(eta.size)
