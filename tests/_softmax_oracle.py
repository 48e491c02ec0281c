"""Numpy oracle of the softmax (multinomial logistic) regression target, with the interface of ``oracle/models.py``
(``logp``, ``grad``, ``hessian``, ``hvp``), so the functions of ``oracle.objectives`` serve as objective oracles unchanged.

Parameter layout class-major, ``theta = [b_0 | ... | b_{C-1}]`` with ``b_c`` of length ``p``; every coordinate carries
the ``N(0, prior_sd)`` prior; no reference class is pinned."""
import numpy as np
from scipy.special import logsumexp

LOG_2PI = np.log(2.0 * np.pi)


def _as2d(x):
    x = np.asarray(x, dtype=np.float64)
    return x[np.newaxis, :] if x.ndim == 1 else x


class SoftmaxOracle:
    def __init__(self, X, y, n_classes, prior_sd=10.0):
        self.X = np.asarray(X, dtype=np.float64)
        self.y = np.asarray(y).astype(np.int64).ravel()
        self.C = int(n_classes)
        self.p = self.X.shape[1]
        self.n_data = self.X.shape[0]
        self.prior_sd = float(prior_sd)
        self.dim = self.C * self.p
        self.onehot = np.zeros((self.n_data, self.C))
        self.onehot[np.arange(self.n_data), self.y] = 1.0

    def eta(self, theta):
        """(N, n_data, C) linear predictors."""
        b = _as2d(theta).reshape(-1, self.C, self.p)
        return np.einsum('ncj,ij->nic', b, self.X)

    def pointwise(self, theta):
        """(N, n_data): eta_{i, y_i} - logsumexp_c eta_ic."""
        eta = self.eta(theta)
        picked = np.take_along_axis(eta, self.y[None, :, None], axis=2)[:, :, 0]
        return picked - logsumexp(eta, axis=2)

    def logp(self, theta):
        theta = _as2d(theta)
        pr = -0.5 * np.sum(theta * theta, axis=1) / self.prior_sd ** 2 - self.dim * (np.log(self.prior_sd) + 0.5 * LOG_2PI)
        return np.sum(self.pointwise(theta), axis=1) + pr

    def grad(self, theta):
        theta = _as2d(theta)
        eta = self.eta(theta)
        soft = np.exp(eta - logsumexp(eta, axis=2, keepdims=True))
        res = self.onehot[None, :, :] - soft                                  # (N, n_data, C)
        g = np.einsum('nic,ij->ncj', res, self.X).reshape(theta.shape[0], self.dim)
        return g - theta / self.prior_sd ** 2

    def hessian(self, m):
        """Closed form: block (c, c') = -sum_i s_ic ([c = c'] - s_ic') x_i x_i' - [c = c'] I / sd^2."""
        m = np.asarray(m, dtype=np.float64).ravel()
        eta = self.eta(m)[0]
        s = np.exp(eta - logsumexp(eta, axis=1, keepdims=True))              # (n_data, C)
        W = s[:, :, None] * (np.eye(self.C)[None, :, :] - s[:, None, :])     # (n_data, C, C)
        H = -np.einsum('icd,ij,ik->cjdk', W, self.X, self.X).reshape(self.dim, self.dim)
        return H - np.eye(self.dim) / self.prior_sd ** 2

    def hvp(self, m, v):
        return _as2d(v) @ self.hessian(m).T
