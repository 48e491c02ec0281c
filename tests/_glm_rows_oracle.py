"""Reference and input sets of the flat regression target's row entries (tests/test_gpu_glm_rows.py, and
tests/test_glm_rows_oracle_cpu.py, which holds this module itself to 50 digits).  Host only.

``rows(oracle, x, counts)`` evaluates a ``GLMOracle`` (tests/_laplace_oracle.py: normalised densities, overflow-safe logit)
at every row of ``x`` and returns, beside ``f`` and ``g``, a first-order rounding bound of each WITHOUT the unit roundoff,
formed in longdouble from reference quantities only.  With eta_i = x_i' b, a_i = sum_k |b_k X_ik|, dl_i the term's
derivative in eta, w_i its curvature and c_i the multiplicity of observation i:

    bound_f    = sum_i c_i (|pieces of t_i| + |dl_i| a_i) + |b|^2 / (2 sd^2) + sum_i c_i |obs_const_i| + |prior const|
    bound_g[j] = sum_i c_i (m_i + w_i a_i) |X_ij| + |b_j| / sd^2

    link       pieces of t_i                              m_i                      w_i
    logit      |y eta|, max(eta, 0), log1p(exp(-|eta|))   |y| + p                  p (1 - p)
    Poisson    |y eta|, mu = exp(eta)                     |y| + mu                 mu
    Gaussian   (y - eta)^2 / (2 s^2)                      (|y| + |eta|) / s^2      1 / s^2

(the Gaussian's m carries the 1 / s^2 of dl = (y - eta) / s^2 on both parts; every Gaussian input set below has s > 1,
where this is the smaller of the two readings "|y| + |eta| / s^2" and "(|y| + |eta|) / s^2").  The pass criterion is per
row and per element

    |dev - ref| <= (n_data + d + 16) 2^-53 bound

n_data + d: the two accumulation chains at their worst, whatever the summation order; 16: the few-ulp exp, log1p and
division and the final additions.  A derived worst case, not a measurement: the float64 oracle stays below 2.4 (f) and
8.1 (g) times 2^-53 bound where 324 and more are allowed, and a misplaced row, a swapped branch or a dropped tile misses
by many orders of magnitude.  The Poisson constant -log(y!) comes from a float64 ``gammaln`` in either dtype: one float64
rounding of a quantity that bound_f contains.

The input sets of the GPU tests are defined here so that the CPU test can hold the float64 oracle to the same criterion
on exactly them."""
import copy
import functools

import numpy as np

from _laplace_oracle import GLMOracle, KINDS

L = np.longdouble
U = 2.0 ** -53
PRIOR_SD = {'logistic': 3.0, 'poisson': 2.0, 'linear': 4.0}
NOISE_SD = 1.5                                   # > 1: see the module docstring
CYCLE = 61                                       # prime: a shift by any tile width changes the residue


def rows(oracle, x, counts=None):
    """``(f, g, bound_f, bound_g)`` at every row of ``x`` (N, D): f and g in the oracle's dtype from the oracle's own
    term formulas, the bounds in longdouble; evaluated in blocks of rows.  ``counts`` (n,): the oracle's design holds
    distinct observations and observation j stands ``counts[j]`` times in the design meant."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    dt, kind = oracle.dtype, oracle.kind
    n, d = oracle.X.shape
    c = np.ones(n) if counts is None else np.asarray(counts, dtype=np.float64)
    same = dt is L
    wide = oracle if same else GLMOracle(kind, oracle.X, oracle.y, oracle.prior_sd, oracle.noise_sd, dtype=L)
    col, wcol = _columnwise(oracle), _columnwise(wide)
    X, Xt = np.ascontiguousarray(oracle.X), np.ascontiguousarray(oracle.X.T)
    XL, aXL, aXLt = np.ascontiguousarray(wide.X), np.abs(wide.X), np.ascontiguousarray(np.abs(wide.X).T)
    yL, cd, cL = wide.y[:, None], c.astype(dt)[:, None], c.astype(L)[:, None]
    sd2, sd2L = dt(oracle.prior_sd) ** 2, L(oracle.prior_sd) ** 2
    s2L = L(oracle.noise_sd) ** 2
    prior_const = -d * (np.log(dt(oracle.prior_sd)) + dt(0.5) * np.log(2 * dt(np.pi)))
    if kind == 'poisson':
        consts = np.abs(wide.obs_const)
    elif kind == 'linear':
        consts = np.full(n, np.abs(L(0.5) * np.log(2 * L(np.pi) * s2L)))
    else:
        consts = np.zeros(n, dtype=L)
    const_bound = np.sum(cL[:, 0] * consts) + d * np.abs(np.log(L(oracle.prior_sd)) + L(0.5) * np.log(2 * L(np.pi)))
    N = x.shape[0]
    block = max(8, min(256, (1 << 17) // n))                               # temporaries of about 2 MB
    f, g = np.empty(N, dtype=dt), np.empty((N, d), dtype=dt)
    bf, bg = np.empty(N, dtype=L), np.empty((N, d), dtype=L)
    for r0 in range(0, N, block):
        s = slice(r0, r0 + block)
        xb, xl = x[s].astype(dt), x[s].astype(L)
        eta = _dot(X, xb)                                                  # (n, B), as are t, dl, w
        t, dl, w = col._terms_eta(eta)
        f[s] = np.sum(cd * t, axis=0) + (-np.sum(xb * xb, axis=1) / (2 * sd2) + prior_const)
        g[s] = _dot(np.ascontiguousarray((cd * dl).T), Xt) - xb / sd2
        if not same:
            eta = _dot(XL, xl)
            t, dl, w = wcol._terms_eta(eta)
        a = _dot(aXL, np.abs(xl))
        if kind == 'poisson':
            mu = np.exp(eta)
            pieces, m = np.abs(yL * eta) + mu, np.abs(yL) + mu
        elif kind == 'linear':
            pieces, m = (yL - eta) ** 2 / (2 * s2L), (np.abs(yL) + np.abs(eta)) / s2L
        else:
            e = np.exp(-np.abs(eta))
            pieces, m = np.abs(yL * eta) + np.maximum(eta, 0) + np.log1p(e), np.abs(yL) + (yL - dl)      # p = y - dl
        bf[s] = np.sum(cL * (pieces + np.abs(dl) * a), axis=0) + np.sum(xl * xl, axis=1) / (2 * sd2L) + const_bound
        bg[s] = _dot(np.ascontiguousarray((cL * (m + w * a)).T), aXLt) + np.abs(xl) / sd2L
    return f, g, bf, bg


def _dot(a, b):
    """``a @ b.T`` of two C-contiguous matrices: every sum runs along the contiguous axis of both (numpy's longdouble
    matrix product is several times slower)."""
    return np.einsum('ik,jk->ij', a, b)


def _columnwise(oracle):
    """The oracle with its responses as a column, so that ``_terms_eta`` takes the (n, B) predictors of a block of points."""
    col = copy.copy(oracle)
    col.y = oracle.y[:, None]
    if oracle.obs_const is not None:
        col.obs_const = oracle.obs_const[:, None]
    return col


def allowed(n_data, d):
    """The criterion's factor in units of ``2^-53 bound``."""
    return n_data + d + 16


def excess(dev, ref, bound):
    """``|dev - ref| / (2^-53 bound)`` per element (float64; NaN where ``dev`` is not finite, 0 / 0 is 0)."""
    err = np.abs(np.asarray(dev, dtype=L) - np.asarray(ref, dtype=L))
    with np.errstate(invalid='ignore', divide='ignore'):
        r = err / (L(U) * np.asarray(bound, dtype=L))
    return np.asarray(np.where((err == 0) & (bound == 0), 0, r), dtype=np.float64)


# ---- input sets ------------------------------------------------------------------------------------------------------
class Case:
    """One input set: a flat regression problem (``X``, ``y`` the DISTINCT observations, ``counts`` their multiplicities
    or None), the points ``x`` and the longdouble reference, computed once and left alone."""

    def __init__(self, name, kind, X, y, x, n_data, counts=None):
        self.name, self.kind, self.X, self.y, self.x, self.counts = name, kind, X, y, x, counts
        self.n_data, self.dim = int(n_data), X.shape[1]
        self.prior_sd, self.noise_sd = PRIOR_SD[kind], NOISE_SD
        self._ref = None

    def oracle(self, dtype=L):
        return GLMOracle(self.kind, self.X, self.y, self.prior_sd, self.noise_sd, dtype=dtype)

    def design(self):
        """The design the device model gets: observation i is distinct observation i mod len(X)."""
        if self.counts is None:
            return self.X, self.y
        idx = np.arange(self.n_data) % self.X.shape[0]
        return self.X[idx], self.y[idx]

    def reference(self):
        if self._ref is None:
            self._ref = rows(self.oracle(L), self.x, self.counts)
            for arr in self._ref:
                arr.setflags(write=False)
        return self._ref

    @property
    def limit(self):
        return allowed(self.n_data, self.dim)


def _responses(kind, rng, X):
    eta = X @ (0.5 * rng.randn(X.shape[1]))
    if kind == 'logistic':
        return (rng.rand(X.shape[0]) < 1.0 / (1.0 + np.exp(-eta))).astype(float)
    if kind == 'poisson':
        return rng.poisson(2.0, size=X.shape[0]).astype(float)
    return eta + NOISE_SD * rng.randn(X.shape[0])


def cycle_counts(n_data):
    return np.bincount(np.arange(n_data) % CYCLE, minlength=CYCLE).astype(float)


@functools.lru_cache(maxsize=None)
def cycle_case(kind, D, n_data, N):
    """``n_data`` observations that cycle through CYCLE distinct ones, N distinct points 0.4 randn."""
    rng = np.random.RandomState(7 * D + n_data % 1000 + KINDS.index(kind))
    X = rng.randn(CYCLE, D) / np.sqrt(D)
    y = _responses(kind, rng, X)
    x = 0.4 * np.random.RandomState(N).randn(N, D)
    return Case('cycle %s D=%d n_data=%d N=%d' % (kind, D, n_data, N), kind, X, y, x, n_data, cycle_counts(n_data))


@functools.lru_cache(maxsize=None)
def dense_case(kind, D, n_data, N):
    """A plain random problem (every observation distinct), N points 0.4 randn."""
    rng = np.random.RandomState(11 * D + n_data + 3 * N + KINDS.index(kind))
    X = rng.randn(n_data, D) / np.sqrt(D)
    y = _responses(kind, rng, X)
    x = 0.4 * rng.randn(N, D)
    return Case('dense %s D=%d n_data=%d N=%d' % (kind, D, n_data, N), kind, X, y, x, n_data)


# the three-chunk crossing: (32 << 20) // round_up(70001, 16) = 479 rows per chunk of the gradient entry, 958 of the
# log-density entry
CROSS_N_DATA, CROSS_D, CROSS_CHUNK_GRAD, CROSS_CHUNK_LOGP = 70001, 3, 479, 958
CROSS_N_GRAD, CROSS_N_LOGP = 2 * CROSS_CHUNK_GRAD + 5, 2 * CROSS_CHUNK_LOGP + 5
# the 128-row floor: round_up(262200, 16) > (32 << 20) / 128
FLOOR_N_DATA, FLOOR_D, FLOOR_N = 262200, 2, 128 + 5
EDGE_N_DATA = (1, 15, 16, 17, 127, 128, 129)                 # at D = 5, N = 7
# three slabs of exactly 128 observations: n_data a multiple of 16 sends the gradient product to the GEMM's other kernel
# (operands straight into LDS), which the ragged n_data of the ladder never reach with more than one slab
WHOLE_SLABS = (70, 5, 384)                                   # (rows, D, n_data)


def ladder_cases(n_cu):
    """``(regime, rows, D, n_data)`` of the split ladder on a device of ``n_cu`` compute units; ``ladder_regime`` gives
    the regime back.  The middle case has 24 tiles, 2 n_cu / 24 splits and room for 27; the cap case has three tiles
    where 2 n_cu / 3 exceeds 64, one tile on a smaller device; every split case's n_data is no multiple of 16 splits."""
    side = 64 * int(np.ceil(np.sqrt(n_cu)))
    return [('floor', 70, 5, 100), ('max_splits', 70, 5, 300), ('cu_bound', 64 * 24 - 3, 2, 27 * 128 + 1),
            ('cap', 130 if 2 * n_cu // 3 > 64 else 61, 2, 8327), ('one_launch', side, side, 257)]


def ladder_regime(rows, d, n_data, n_cu):
    """Which rule of ``glm_grad_splits`` decides, and the split count it gives: 'tie' where two rules give the same."""
    tiles = ((rows + 63) // 64) * ((d + 63) // 64)
    if tiles >= n_cu:
        return 'one_launch', 1
    by_cu, by_data = 2 * n_cu // tiles, n_data // 128
    if by_data == 0:
        return 'floor', 1
    if by_data < min(by_cu, 64):
        return 'max_splits', by_data
    if by_cu < min(by_data, 64):
        return 'cu_bound', by_cu
    if 64 < min(by_cu, by_data):
        return 'cap', 64
    return 'tie', min(by_cu, by_data, 64)


# ---- link tails ------------------------------------------------------------------------------------------------------
TAIL_N_DATA, TAIL_D, TAIL_N = 301, 7, 300
TAIL_SCALES = {'logistic': (15.0, 300.0), 'poisson': (6.0, 12.0), 'linear': (1e6,)}
TAIL_BAD_ROWS = (17, 203)                                    # row isolation: all NaN, all +inf


@functools.lru_cache(maxsize=None)
def tail_case(kind, scale):
    """Points ``scale * randn`` and four placed rows: x = +0, x = -0 (eta = +-0.0 at every observation) and
    x = +-scale e_0 -- the design's first column is positive, so every eta of such a row has one sign and each branch of
    the logit's p runs alone.  Poisson responses include 0 and 1e6."""
    rng = np.random.RandomState(int(scale) % 1000 + 17 * KINDS.index(kind))
    X = rng.randn(TAIL_N_DATA, TAIL_D) / np.sqrt(TAIL_D)
    X[:, 0] = 0.5 + np.abs(X[:, 0])
    y = _responses(kind, rng, X)
    if kind == 'poisson':
        y[0], y[1] = 0.0, 1e6
    if kind == 'linear':
        y = y + 1e6 * rng.randn(TAIL_N_DATA) * (rng.rand(TAIL_N_DATA) < 0.1)       # a tenth of the residuals near 1e6
    x = scale * rng.randn(TAIL_N, TAIL_D)
    x[-4], x[-3] = 0.0, -0.0
    x[-2], x[-1] = 0.0, 0.0
    x[-2, 0], x[-1, 0] = scale, -scale
    return Case('tail %s scale=%g' % (kind, scale), kind, X, y, x, TAIL_N_DATA)


def tail_cases():
    return [(kind, scale) for kind in KINDS for scale in TAIL_SCALES[kind]]


def all_cases(n_cu):
    """Every input set of tests/test_gpu_glm_rows.py on a device of ``n_cu`` compute units."""
    out = []
    for kind in KINDS:
        out += [cycle_case(kind, CROSS_D, CROSS_N_DATA, CROSS_N_GRAD), cycle_case(kind, CROSS_D, CROSS_N_DATA, CROSS_N_LOGP),
                cycle_case(kind, FLOOR_D, FLOOR_N_DATA, FLOOR_N)]
        out += [dense_case(kind, D, n_data, rows_) for _, rows_, D, n_data in ladder_cases(n_cu)]
        out += [dense_case(kind, 5, n_data, 7) for n_data in EDGE_N_DATA]
        out += [dense_case(kind, WHOLE_SLABS[1], WHOLE_SLABS[2], WHOLE_SLABS[0])]
    return out + [tail_case(kind, scale) for kind, scale in tail_cases()]
