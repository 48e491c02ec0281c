"""numpy float64 oracle of the kernel Stein discrepancy (vb_ksd, csrc/vb_ksd.hip): the IMQ Stein kernel in DIFFERENCE
FORM, with explicit differences, blockwise over the rows so that S = 1500 fits, and the error scales the tolerance of the
GPU tests multiplies.

    r2 = sum (x~_i - x~_j)^2     a = sum g~_i g~_j     b = sum (g~_i - g~_j)(x~_i - x~_j)     u = c^2 + r2
    k_p(i, j) = a u^beta - 2 beta u^(beta-1) (b + D) - 4 beta (beta-1) r2 u^(beta-2)
    A_ij = (sum |g~_i g~_j|) u^beta + 2 |beta| u^(beta-1) (sum |(g~_i - g~_j)(x~_i - x~_j)| + D) + 4 |beta (beta-1)| r2 u^(beta-2)
    rowsums[i] = sum_j w_j k_p(i, j)   ksd2 = sum_i w_i rowsums[i]     E_i = sum_j w_j A_ij   E = sum_i w_i E_i
"""
import numpy as np

ROW_BLOCK = 64


def normalised_weights(log_w, s):
    """Uniform without log weights, else exp(log_w - logsumexp(log_w)): what the entry forms (predict_weights)."""
    if log_w is None:
        return np.full(s, 1.0 / s)
    log_w = np.asarray(log_w, dtype=np.float64)
    mx = np.max(log_w)
    return np.exp(log_w - (mx + np.log(np.sum(np.exp(log_w - mx)))))


def stein_kernel_block(xi, gi, xj, gj, c, beta, with_scale=False):
    """k_p (and A) between the rows of (xi, gi) and of (xj, gj), already rescaled."""
    d = xi.shape[1]
    dx = xi[:, None, :] - xj[None, :, :]
    dg = gi[:, None, :] - gj[None, :, :]
    r2 = np.sum(dx * dx, axis=2)
    a = gi @ gj.T
    b = np.sum(dg * dx, axis=2)
    u = c * c + r2
    p2 = u ** (beta - 2.0)
    p1, p0 = p2 * u, p2 * u * u
    kp = a * p0 - 2.0 * beta * p1 * (b + d) - 4.0 * beta * (beta - 1.0) * r2 * p2
    if not with_scale:
        return kp
    a_abs = np.abs(gi) @ np.abs(gj).T
    b_abs = np.sum(np.abs(dg * dx), axis=2)
    A = a_abs * p0 + 2.0 * abs(beta) * p1 * (b_abs + d) + 4.0 * abs(beta * (beta - 1.0)) * r2 * p2
    return kp, A


def stein_kernel_matrix(x, g, scale=None, c=1.0, beta=-0.5):
    """The whole S x S matrix k_p (small S only)."""
    x, g = np.asarray(x, dtype=np.float64), np.asarray(g, dtype=np.float64)
    if scale is not None:
        x, g = x / scale, g * scale
    return stein_kernel_block(x, g, x, g, c, beta)


def ksd(x, g, log_w=None, scale=None, c=1.0, beta=-0.5):
    """dict(ksd2, rowsums, E, E_rows, w): the discrepancy of the weighted draws and the error scales."""
    x, g = np.asarray(x, dtype=np.float64), np.asarray(g, dtype=np.float64)
    s = x.shape[0]
    if scale is not None:
        scale = np.asarray(scale, dtype=np.float64)
        x, g = x / scale, g * scale
    w = normalised_weights(log_w, s)
    rowsums, e_rows = np.empty(s), np.empty(s)
    for i0 in range(0, s, ROW_BLOCK):
        kp, A = stein_kernel_block(x[i0:i0 + ROW_BLOCK], g[i0:i0 + ROW_BLOCK], x, g, c, beta, with_scale=True)
        rowsums[i0:i0 + ROW_BLOCK] = kp @ w
        e_rows[i0:i0 + ROW_BLOCK] = A @ w
    return dict(ksd2=float(w @ rowsums), rowsums=rowsums, E=float(w @ e_rows), E_rows=e_rows, w=w)


def tolerance(s, d):
    """2 (2 D + S + 64) 2^-53: D-term sums of products whose factors are each rounded once (2 D), the weighted sum over
    the draws in any order (S), pow, the combination and the reduction trees (64); both sides round (the leading 2)."""
    return 2.0 * (2 * d + s + 64) * 2.0 ** -53
