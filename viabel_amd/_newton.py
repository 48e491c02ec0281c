"""The damped Newton ascent behind ``DeviceModel.find_mode``: host LAPACK on ``D x D`` matrices around one evaluation hook.

Everything of the order of the data stays where the hook puts it (for the flat regression targets: one device call per
evaluation, ``vb_glm_value_grad_hessian``); what is here is the O(D^3) algebra between those calls, the same division of
labour as for the dense families' factor algebra."""
import warnings

import numpy as np
from scipy.linalg import cho_factor, cho_solve


def newton_ascent(value_grad_hessian, x, max_iter, tol):
    """Maximise from ``x`` (D,) with ``value_grad_hessian(x, want_hessian) -> (f, g, H or None)``; the rules and the result
    are those of ``DeviceModel.find_mode`` (arguments already validated)."""
    d = x.shape[0]
    f, g, H = value_grad_hessian(x, True)
    n_iter, converged, why = 0, False, 'the iteration limit ({})'.format(max_iter)
    while True:
        if not (np.all(np.isfinite(H)) and np.all(np.isfinite(g)) and np.isfinite(f)):
            why = 'a non-finite value, gradient or Hessian'
            break
        lam = 0.0
        while True:
            try:
                factor = cho_factor(lam * np.eye(d) - H, lower=True)
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
            f_try = value_grad_hessian(x + t * delta, False)[0]
            if f_try >= f + 1e-4 * t * slope:      # (a NaN value fails)
                taken = True
                break
            # the gain a full Newton step promises is below the rounding of f: the values cannot order the two points, the
            # step is accurate all the same
            if t == 1.0 and np.isfinite(f_try) and 0.5 * slope <= 64.0 * np.finfo(float).eps * max(1.0, abs(f)):
                taken = True
                break
            if halvings == 30:
                break
            t, halvings = 0.5 * t, halvings + 1
        if not taken:
            why = 'the line search (30 halvings)'
            break
        step = t * delta
        small = float(np.max(np.abs(step))) <= tol * max(1.0, float(np.max(np.abs(x))))
        if not small and n_iter == max_iter:
            break
        x = x + step
        f, g, H = value_grad_hessian(x, True)
        if small:
            converged = True
            break
        n_iter += 1
    if not converged:
        warnings.warn('find_mode stopped at {} without converging (max|grad| = {:.3g})'.format(
            why, float(np.max(np.abs(g)))), RuntimeWarning, stacklevel=3)
    return dict(mode=x, value=float(f), grad=g, hessian=H, n_iter=n_iter, converged=converged)
