"""numpy oracle of the Laplace tests: value, gradient and Hessian of the flat regression target under its three likelihoods
(float64, or longdouble for a value that resolves the last steps of a Newton run), a Newton loop with the rules of
``DeviceModel.find_mode``, the conjugate linear posterior with its log evidence (the formulas of
``tests/test_gpu_property.py:121-130``) and the fourth-order difference stencil of ``DeviceModel.hessian`` applied to any
``grad``."""
import math

import numpy as np
from scipy.linalg import cho_factor, cho_solve
from scipy.special import gammaln

KINDS = ('logistic', 'poisson', 'linear')


class GLMOracle:
    """f(b) = sum_i log p(y_i | x_i' b) - |b|^2 / (2 sd^2) - D (log sd + log(2 pi) / 2), normalised densities."""

    def __init__(self, kind, X, y, prior_sd=10.0, noise_sd=1.0, dtype=np.float64):
        assert kind in KINDS
        self.kind, self.dtype = kind, dtype
        self.X, self.y = np.asarray(X, dtype=dtype), np.asarray(y, dtype=dtype)
        self.prior_sd, self.noise_sd = float(prior_sd), float(noise_sd)
        self.n_data, self.dim = self.X.shape
        self.obs_const = -np.asarray(gammaln(np.asarray(y, dtype=np.float64) + 1.0), dtype=dtype) if kind == 'poisson' else None

    def _terms(self, b):
        """(log-likelihood terms with their constants, d / d eta, -d^2 / d eta^2) at one point."""
        return self._terms_eta(self.X @ np.asarray(b, dtype=self.dtype))

    def _terms_eta(self, eta):
        """The same three at given linear predictors."""
        y = self.y
        if self.kind == 'poisson':
            mu = np.exp(eta)
            return y * eta - mu + self.obs_const, y - mu, mu
        if self.kind == 'linear':
            s2 = self.dtype(self.noise_sd) ** 2
            const = -self.dtype(0.5) * np.log(2 * self.dtype(np.pi) * s2)
            return -(y - eta) ** 2 / (2 * s2) + const, (y - eta) / s2, np.full(eta.shape, 1 / s2, dtype=self.dtype)
        t = np.exp(-np.abs(eta))
        p = np.where(eta >= 0, 1 / (1 + t), t / (1 + t))
        return y * eta - (np.maximum(eta, 0) + np.log1p(t)), y - p, t / (1 + t) ** 2

    def value(self, b):
        b = np.asarray(b, dtype=self.dtype)
        sd = self.dtype(self.prior_sd)
        prior = -(b @ b) / (2 * sd * sd) - self.dim * (np.log(sd) + self.dtype(0.5) * np.log(2 * self.dtype(np.pi)))
        return np.sum(self._terms(b)[0]) + prior

    def grad(self, x):
        """(D,) -> (D,), (N, D) -> (N, D), like ``DeviceModel.grad``."""
        x = np.asarray(x, dtype=self.dtype)
        if x.ndim == 2:
            return np.stack([self.grad(row) for row in x])
        return self.X.T @ self._terms(x)[1] - x / self.dtype(self.prior_sd) ** 2

    def hessian(self, b):
        w = self._terms(b)[2]
        return -(self.X.T * w) @ self.X - np.eye(self.dim, dtype=self.dtype) / self.dtype(self.prior_sd) ** 2

    def weights(self, b):
        return self._terms(b)[2]

    def value_grad_hessian(self, b, want_hessian=True):
        """The hook's contract in float64, whatever the oracle computes in: ``(f, g, H or None)``."""
        return (float(self.value(b)), np.asarray(self.grad(b), dtype=np.float64),
                np.asarray(self.hessian(b), dtype=np.float64) if want_hessian else None)


def newton(vgh, x0, max_iter=100, tol=1e-10, trace=None):
    """``find_mode``'s rules on a hook ``vgh(x, want_hessian) -> (f, g, H or None)``: Cholesky of ``-H`` with a ridge from
    ``1e-6 max|diag H|`` times 10, Armijo backtracking with constant 1e-4 and at most 30 halvings, a full step that fails the
    test taken all the same once the promised gain ``g' delta / 2`` is below ``64 eps max(1, |f|)``, a step of at most
    ``tol max(1, max|x|)`` applied, not counted and the last.  ``trace``: a list that receives ``(x, f, t, halvings)`` of
    every point the search moves to.  Returns ``find_mode``'s dict."""
    x = np.array(x0, dtype=np.float64)
    d = x.size
    f, g, H = vgh(x, True)
    n_iter, converged = 0, False
    if trace is not None:
        trace.append((x.copy(), f, 0.0, 0))
    while np.all(np.isfinite(H)) and np.all(np.isfinite(g)) and np.isfinite(f):
        lam = 0.0
        while True:
            try:
                A = lam * np.eye(d) - H
                factor = cho_factor(A, lower=True)
                # (a ridge that clears the negative curvature by less than a thousandth of itself has not: in one dimension
                # the sequence passes through |H| itself, and the step would be astronomic)
                if lam == 0.0 or np.min(np.diag(factor[0])) ** 2 >= 1e-3 * lam:
                    delta = cho_solve(factor, g)
                    break
            except np.linalg.LinAlgError:
                pass
            lam = 10.0 * lam if lam > 0.0 else 1e-6 * (float(np.max(np.abs(np.diag(H)))) or 1.0)
        slope = float(g @ delta)
        t, halvings, taken = 1.0, 0, False
        while True:
            f_try = vgh(x + t * delta, False)[0]
            if f_try >= f + 1e-4 * t * slope:
                taken = True
            elif t == 1.0 and math.isfinite(f_try) and 0.5 * slope <= 64.0 * np.finfo(float).eps * max(1.0, abs(f)):
                taken = True
            if taken or halvings == 30:
                break
            t, halvings = 0.5 * t, halvings + 1
        if not taken:
            break
        step = t * delta
        small = float(np.max(np.abs(step))) <= tol * max(1.0, float(np.max(np.abs(x))))
        if not small and n_iter == max_iter:
            break
        x = x + step
        f, g, H = vgh(x, True)
        if trace is not None:
            trace.append((x.copy(), f, t, halvings))
        if small:
            converged = True
            break
        n_iter += 1
    return dict(mode=x, value=float(f), grad=g, hessian=H, n_iter=n_iter, converged=converged)


def conjugate_linear(X, y, prior_sd, noise_sd):
    """(mean, cov, precision, log evidence) of linear regression with known noise (tests/test_gpu_property.py:121-130)."""
    n_data, D = X.shape
    s, sd = noise_sd, prior_sd
    prec = X.T @ X / s ** 2 + np.eye(D) / sd ** 2
    cov = np.linalg.inv(prec)
    cov = 0.5 * (cov + cov.T)
    mean = cov @ X.T @ y / s ** 2
    log_ev = (-0.5 * n_data * np.log(2 * np.pi * s ** 2) - D * np.log(sd) - 0.5 * np.linalg.slogdet(prec)[1]
              - 0.5 * (y @ y / s ** 2 - mean @ prec @ mean))
    return mean, cov, prec, float(log_ev)


def stencil_step(x):
    return 2e-3 * max(1.0, float(np.max(np.abs(x))))


def stencil_points(x):
    """The 4 D + 1 points of ``DeviceModel.hessian`` at ``x`` (D,): x, x +- h e_j, x +- 2 h e_j."""
    x = np.asarray(x, dtype=np.float64)
    h, eye = stencil_step(x), np.eye(x.size)
    return np.concatenate([x[None, :], x + h * eye, x - h * eye, x + 2 * h * eye, x - 2 * h * eye])


def stencil_hessian(grad, x):
    """Fourth-order central differences of ``grad`` ((N, D) -> (N, D)) at ``x`` (D,), symmetrised: ``DeviceModel.hessian``'s
    default in numpy.  Returns ``(H, max|g| over the stencil points)``."""
    x = np.asarray(x, dtype=np.float64)
    d, h = x.size, stencil_step(x)
    g = np.asarray(grad(stencil_points(x)), dtype=np.float64)
    d1 = g[1:1 + d] - g[1 + d:1 + 2 * d]
    d2 = g[1 + 2 * d:1 + 3 * d] - g[1 + 3 * d:]
    ht = (8.0 * d1 - d2) / (12.0 * h)
    return 0.5 * (ht + ht.T), float(np.max(np.abs(g)))


def make_problem(kind, D, n_data, seed, scale=None, noise_sd=0.7):
    """(X, y) of a regression problem: X = randn * scale (default 1 / sqrt(D)), y simulated from coefficients of scale 0.5."""
    rng = np.random.RandomState(seed)
    X = rng.randn(n_data, D) * (1.0 / np.sqrt(D) if scale is None else scale)
    eta = X @ (0.5 * rng.randn(D))
    if kind == 'logistic':
        y = (rng.rand(n_data) < 1.0 / (1.0 + np.exp(-eta))).astype(float)
    elif kind == 'poisson':
        y = rng.poisson(np.exp(eta)).astype(float)
    else:
        y = eta + noise_sd * rng.randn(n_data)
    return X, y
