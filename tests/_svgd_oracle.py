"""numpy oracle of the SVGD direction (vb_svgd_direction, csrc/vb_svgd.hip) in extended precision (np.longdouble), with
explicit differences, the median rule exactly as the header defines it, and the error scale the GPU tests multiply.

    c = column means of x            y_i = (x_i - c) / scale          g_i = score_i * scale
    r2_ij = sum_k (y_ik - y_jk)^2    kappa_ij = exp(-r2_ij / h)
    phi_y(i) = 1/n [ sum_j kappa_ij g_j + (2/h) ( y_i sum_j kappa_ij - sum_j kappa_ij y_j ) ]      phi(i) = phi_y(i) / scale
    E_i = 1/n sum_j kappa_ij (1 + r2_ij/h) ( |g_j| + (2/h)(|y_i| + |y_j|) ) / scale                  (per coordinate)
    h = m / log(n + 1), m the element of 0-based rank (n (n - 1) / 2 - 1) // 2 of the r2_ij with i < j; 1 if n = 1 or m = 0
"""
import numpy as np

ROW_BLOCK = 64


def squared_distances(y):
    """r2 (n x n) from the differences themselves, blockwise over the rows."""
    n = y.shape[0]
    r2 = np.empty((n, n), dtype=y.dtype)
    for i0 in range(0, n, ROW_BLOCK):
        diff = y[i0:i0 + ROW_BLOCK, None, :] - y[None, :, :]
        r2[i0:i0 + ROW_BLOCK] = np.sum(diff * diff, axis=2)
    return r2


def median_rank(n):
    """0-based rank of the lower median of the n (n - 1) / 2 pair distances."""
    return (n * (n - 1) // 2 - 1) // 2


def lower_median(r2):
    """The element of rank ``median_rank(n)`` of the strict upper triangle of r2 (None when n = 1)."""
    n = r2.shape[0]
    if n < 2:
        return None
    v = r2[np.triu_indices(n, 1)]
    k = median_rank(n)
    return np.partition(v, k)[k]


def median_bandwidth(r2):
    n = r2.shape[0]
    m = lower_median(r2)
    if m is None or m == 0:
        return r2.dtype.type(1.0)
    return m / np.log(r2.dtype.type(n + 1))


def direction(x, g, scale=None, bandwidth=None, dtype=np.longdouble):
    """dict(phi, h, E, r2): the direction at bandwidth ``h`` (None: the median rule) and the error scale, in ``dtype``."""
    x, g = np.asarray(x, dtype=dtype), np.asarray(g, dtype=dtype)
    n, d = x.shape
    s = np.ones(d, dtype=dtype) if scale is None else np.asarray(scale, dtype=dtype)
    c = np.sum(x, axis=0) / dtype(n)
    y, gs = (x - c) / s, g * s
    r2 = squared_distances(y)
    h = median_bandwidth(r2) if bandwidth is None else dtype(bandwidth)
    kappa = np.exp(-r2 / h)
    rowsum = np.sum(kappa, axis=1)
    two_h = dtype(2.0) / h
    phi = (kappa @ gs + two_h * (y * rowsum[:, None] - kappa @ y)) / dtype(n) / s
    w = kappa * (1 + r2 / h)
    E = (w @ np.abs(gs) + two_h * (np.abs(y) * np.sum(w, axis=1)[:, None] + w @ np.abs(y))) / dtype(n) / s
    return dict(phi=phi, h=h, E=E, r2=r2)


def tolerance(n, d):
    """2 (2 D + n + 64) 2^-53, as _ksd_oracle.tolerance: D-term sums of products whose factors are each rounded once (2 D),
    the sum over the particles in any order (n), exp, the combination and the reduction trees (64); both sides round."""
    return 2.0 * (2 * d + n + 64) * 2.0 ** -53


def bandwidth_tolerance(d):
    """2 (D + 4) 2^-53, relative: a D-term sum of squared differences whose terms are each rounded a few times, the
    division by log(n + 1); both sides round."""
    return 2.0 * (d + 4) * 2.0 ** -53
