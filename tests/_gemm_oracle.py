"""Inputs, references and cases of tests/test_gpu_gemm_raw.py: the fp64 GEMM (csrc/vb_gemm_f64.h, vb_gemm_f64_dma.h) through
the three public entries that return a bare product.  Host only; tests/test_gemm_plan_cpu.py holds this module to account.

  A  ``Engine.model_grad`` on ``CorrelatedGaussianModel(m, precision=P)``: G = -(x - m) P.  A row-major, dense, one split,
     M = n, N = K = d; a plain-store epilogue, so the 64 x 32 tiles are open to it.
  B  ``Engine.noise_moments(slot, n, d, want_gram=True)``: E'E.  A k-major, tri_mode 2 (lower tiles, mirrored on the host),
     M = N = d, K = n in ``_lib.gram_splits(d, n, n_cu)`` splits, then a slab sum; and the column sums of E.
  C  ``Engine.lowrank_path_terms``: U = E sw (A row-major, M = n, N = k, K = d), then with T = [Z | U] the products E'T
     (M = d, N = 2k, K = n) and T'T (M = N = 2k), A k-major, dense, in ``_lib.lowrank_splits(n)`` splits; the column sums of
     E, E^2 and T.  A case is filed under the variant of its E'T product.

A VARIANT is (entry, kernel, cfg, feature): the kernel is 'dma' (operands straight into LDS, K % 16 == 0) or 'reg'
(register-staged), cfg the launcher's tile code (1: 128 x 128, 2: 128 x 64, 3: 64 x 64, 6: 128 x 128 with two LDS stages,
7: 64 x 32) and the feature one of
  ''           more than one split or a single one, the last split not empty (B: and the XCD grouping off)
  'xcd'        B, LDS-DMA kernel: splits a multiple of 8, so the workgroups of a split are grouped on one XCD; several tiles
  'xcd-1tile'  the same with d <= 64: one tile per split
  'empty'      the last k split starts at or beyond K: its workgroups skip the k loop and must still write zeros (B: with
               splits no multiple of 8;  C: at the cap of 32 splits)
  '1split'     B: one split and d two past a tile edge;  C: one split
Which variant a shape takes is decided by ``_lib.gemm_plan`` -- the launcher's own function -- never by a copy of its rules.
The case builders search, smallest first, a fixed candidate list of RAGGED shapes (last row tile and last column tile
partial; K no multiple of 16 for the register-staged kernel, which is the only way to reach it) and cap every array at
256 MB.  TABLE_256 holds the shapes the issue listed for 256 compute units; they are checked against the plan as written.

Exact pass: small integers in float64 (entries in [-7, 7]; P symmetric with off-diagonals in [-3, 3] and 4 d on the
diagonal, m = 0).  Every product and every partial sum of |terms| is an integer below 2^53 (asserted per case), so any
summation order, tile and split gives the same bits as numpy's float64 product.

Real pass: entries sign * exp(1.5 randn), P = A A' / d + I, m != 0 (the reference's left operand is the float64 x - m,
the device's own single rounding).  Per element, for ANY order of summation with or without FMA (Higham, Accuracy and
Stability of Numerical Algorithms, section 3.1: a sum of t products carries at most t roundings per term),

    |dev - exact| <= g(K + s) (|A| |B|)_ij,      g(t) = t u / (1 - t u),  u = 2^-53,

K the contraction length and s the number of k splits (the slab sum adds s - 1 more roundings).  numpy's float64 product
obeys the same bound, so against it the criterion is 2 g over the WHOLE matrix; against a longdouble product (whose own
error, K 2^-64, is 2^-11 of g) it is 1 g on at most 64 rows and all columns -- the first and the last row of the row tiles
at both ends and of as many tiles between them as fit, the rest seeded at random.
Entry C chains products: T holds the device's own U = E sw.  Both references take the float64 U; the two differ by e,
|e| <= 2 g(d + 1) |E| |sw| (each is within g of the exact product), and the criterion grows by what e contributes, first
and second order, whichever reference is used:
    E'T, columns k .. 2k:  |E|' e          T'T:  e'|T| + |T|'e + e'e  (e extended by zeros over the Z columns)
    column sums of T:      sum_n e
Sums of n terms (column sums) use g(n); the sum of squares g(n + 1)."""
import functools

import numpy as np

from viabel_amd import _lib

L = np.longdouble
U = 2.0 ** -53
CAP_BYTES = 256 << 20
MAX_SAMPLE_ROWS = 64


def gamma(t):
    """g(t) = t u / (1 - t u)."""
    return t * U / (1.0 - t * U)


# ---- inputs ----------------------------------------------------------------------------------------------------------
def int_matrix(rng, n, d):
    return rng.randint(-7, 8, size=(n, d)).astype(np.float64)


def int_precision(rng, d):
    """Symmetric, integer, diagonally dominant: off-diagonals in [-3, 3] (row sums of at most 3 (d - 1)), 4 d on the diagonal."""
    a = np.triu(rng.randint(-3, 4, size=(d, d)), 1).astype(np.float64)
    return a + a.T + 4.0 * d * np.eye(d)


def real_matrix(rng, n, d):
    return np.where(rng.rand(n, d) < 0.5, -1.0, 1.0) * np.exp(1.5 * rng.randn(n, d))


def real_precision(rng, d):
    a = real_matrix(rng, d, d)
    p = a @ a.T / d + np.eye(d)
    return 0.5 * (p + p.T)


def assert_exact(*bounds):
    """Every |A| |B| of an exact case stays below 2^53: all partial sums are integers float64 holds."""
    for b in bounds:
        assert float(np.max(b)) < 2.0 ** 53


# ---- products ----------------------------------------------------------------------------------------------------------
def dot_t(a, b):
    """``a @ b.T`` of two C-contiguous matrices of one dtype, every sum along the contiguous axis (numpy's longdouble
    matrix product is several times slower)."""
    return np.einsum('ik,jk->ij', np.ascontiguousarray(a), np.ascontiguousarray(b))


def sample_rows(m, bm, seed):
    """At most MAX_SAMPLE_ROWS rows of an ``m``-row output with row tiles of ``bm``: the first and last row of the tiles,
    from both ends inwards, then seeded random rows."""
    tiles = -(-m // bm)
    order = []
    for i in range(tiles):                                       # tiles 0, last, 1, last - 1, ...
        t = i // 2 if i % 2 == 0 else tiles - 1 - i // 2
        order += [t * bm, min(m, (t + 1) * bm) - 1]
    rows = []
    for r in order:
        if r not in rows and len(rows) < MAX_SAMPLE_ROWS:
            rows.append(r)
    rest = np.random.RandomState(seed).permutation(m)
    for r in rest:
        if len(rows) >= min(m, MAX_SAMPLE_ROWS):
            break
        if int(r) not in rows:
            rows.append(int(r))
    return np.array(sorted(rows), dtype=np.int64)


class Check:
    """One output of an entry and what it is held to: ``|dev - ref| <= factor g(terms) bound + extra`` per element with
    factor 2 against ``ref`` (float64, all of it) and factor 1 against ``ref_rows`` (longdouble, the rows ``rows``)."""

    def __init__(self, name, ref, bound, terms, extra=None, rows=None, ref_rows=None, bound_rows=None, extra_rows=None):
        self.name, self.ref, self.bound, self.terms, self.extra = name, ref, bound, terms, extra
        self.rows, self.ref_rows, self.bound_rows, self.extra_rows = rows, ref_rows, bound_rows, extra_rows

    def ratios(self, dev):
        """``(max ratio against float64, max ratio against longdouble or None)``: |dev - ref| over what is allowed, inf for
        a non-finite device value, 0 for 0 / 0."""
        dev = np.asarray(dev, dtype=np.float64)
        assert dev.shape == self.ref.shape, (self.name, dev.shape, self.ref.shape)
        r64 = _ratio(dev, self.ref, 2.0 * gamma(self.terms) * self.bound + (0.0 if self.extra is None else self.extra))
        if self.rows is None:
            return r64, None
        sub = dev[self.rows] if dev.ndim == 2 else dev
        extra = L(0) if self.extra_rows is None else self.extra_rows
        return r64, _ratio(sub.astype(L), self.ref_rows, L(gamma(self.terms)) * self.bound_rows + extra)


def _ratio(dev, ref, allowed):
    err = np.abs(dev - ref)
    with np.errstate(invalid='ignore', divide='ignore'):
        r = np.where((err == 0) & (allowed == 0), 0, err / allowed)
    r = np.asarray(r, dtype=np.float64)
    return float(np.max(np.where(np.isnan(r), np.inf, r))) if r.size else 0.0


def product_check(name, a, b, terms, bm, seed):
    """C = a b' for C-contiguous ``a`` (M, K) and ``b`` (N, K): the float64 product and bound, and the longdouble ones on
    the sampled rows."""
    ref, bound = a @ b.T, np.abs(a) @ np.abs(b).T
    rows = sample_rows(a.shape[0], bm, seed)
    al, bl = a[rows].astype(L), b.astype(L)
    return Check(name, ref, bound, terms, rows=rows, ref_rows=dot_t(al, bl), bound_rows=dot_t(np.abs(al), np.abs(bl)))


def sum_check(name, a, terms):
    """Column sums of ``a`` (n, d), a sum of ``terms`` roundings at most; all of it in longdouble too."""
    al = a.astype(L)
    return Check(name, a.sum(0), np.abs(a).sum(0), terms, rows=slice(None), ref_rows=al.sum(0), bound_rows=np.abs(al).sum(0))


# ---- the entries: inputs and what their outputs are held to ----------------------------------------------------------------
def inputs_a(n, d, kind, seed=0):
    """``(P, mean, x)`` of entry A."""
    rng = np.random.RandomState(1000003 * seed + 7 * n + d)
    if kind == 'exact':
        return int_precision(rng, d), np.zeros(d), int_matrix(rng, n, d)
    return real_precision(rng, d), real_matrix(rng, 1, d)[0], real_matrix(rng, n, d)


def checks_a(P, mean, x, bm):
    n, d = x.shape
    xc = x - mean                                                # the device's one rounding (none with mean = 0)
    c = product_check('G', xc, np.ascontiguousarray(-P.T), d + 1, bm, n + d)
    return [c]


def inputs_b(d, n, kind, seed=0):
    rng = np.random.RandomState(1000003 * seed + 11 * n + d)
    return int_matrix(rng, n, d) if kind == 'exact' else real_matrix(rng, n, d)


def checks_b(E, splits, bm):
    n, d = E.shape
    Et = np.ascontiguousarray(E.T)
    return [product_check('gram', Et, Et, n + splits, bm, n + d), sum_check('colsum', E, n)]


def inputs_c(d, k, n, kind, seed=0):
    """``(E, Z, sw)`` of entry C."""
    rng = np.random.RandomState(1000003 * seed + 13 * n + 5 * d + k)
    if kind == 'exact':
        return int_matrix(rng, n, d), int_matrix(rng, n, k), int_matrix(rng, d, k)
    return real_matrix(rng, n, d), real_matrix(rng, n, k), real_matrix(rng, d, k)


def checks_c(E, Z, sw, splits, bm):
    """E'T (d, 2k), T'T (2k, 2k), sum E, sum E^2, sum T -- the order ``Engine.lowrank_path_terms`` returns them in.  Both
    references take T = [Z | U] with the float64 U = E sw; ``e`` bounds |device U - float64 U| (module docstring)."""
    n, d = E.shape
    k = Z.shape[1]
    t = np.concatenate([Z, E @ sw], axis=1)
    e = np.concatenate([np.zeros((n, k)), 2.0 * gamma(d + 1) * (np.abs(E) @ np.abs(sw))], axis=1)
    at, ae = np.abs(t), np.abs(E)
    rows_et, rows_tt = sample_rows(d, bm, n + d), sample_rows(2 * k, 64, n + k)
    ttl = np.ascontiguousarray(t.T).astype(L)                    # (2k, n)
    etl = np.ascontiguousarray(E.T[rows_et]).astype(L)           # (rows, n)
    x_et = ae.T @ e
    et = Check('E\'T', E.T @ t, ae.T @ at, n + splits, extra=x_et, rows=rows_et, ref_rows=dot_t(etl, ttl),
               bound_rows=dot_t(np.abs(etl), np.abs(ttl)), extra_rows=x_et[rows_et].astype(L))
    x = e.T @ at
    x_tt = x + x.T + e.T @ e
    tt = Check('T\'T', t.T @ t, at.T @ at, n + splits, extra=x_tt, rows=rows_tt, ref_rows=dot_t(ttl[rows_tt], ttl),
               bound_rows=dot_t(np.abs(ttl[rows_tt]), np.abs(ttl)), extra_rows=x_tt[rows_tt].astype(L))
    st = Check('sum T', t.sum(0), at.sum(0), n, extra=e.sum(0), rows=slice(None), ref_rows=ttl.sum(1),
               bound_rows=np.abs(ttl).sum(1), extra_rows=e.sum(0).astype(L))
    el = E.astype(L)
    sq = Check('sum E^2', (E * E).sum(0), (E * E).sum(0), n + 1, rows=slice(None), ref_rows=(el * el).sum(0),
               bound_rows=(el * el).sum(0))
    return [et, tt, sum_check('sum E', E, n), sq, st]


# ---- plans and variants ------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, entry, kernel, cfg, feature, shape):
        self.entry, self.kernel, self.cfg, self.feature, self.shape = entry, kernel, cfg, feature, tuple(shape)

    @property
    def variant(self):
        return (self.entry, self.kernel, self.cfg, self.feature)

    @property
    def name(self):
        return variant_name(self.variant) + ' ' + 'x'.join(str(v) for v in self.shape)

    def __repr__(self):
        return self.name


def variant_name(v):
    return '%s-%s-cfg%d%s' % (v[0], v[1], v[2], '-' + v[3] if v[3] else '')


def _kernel(p):
    return 'dma' if p['dma'] else 'reg'


def _empty_last(p, splits, k):
    return (splits - 1) * p['k_split'] >= k


def plan_a(n, d, n_cu):
    p = _lib.gemm_plan(n, d, d, 1, n_cu)
    p['splits'], p['empty'] = 1, False
    return p


def plan_b(d, n, n_cu):
    splits = _lib.gram_splits(d, n, n_cu)
    p = _lib.gemm_plan(d, d, n, splits, n_cu, tri_mode=2, a_kcontig=False)
    p['splits'], p['empty'] = splits, _empty_last(p, splits, n)
    return p


def plan_c(d, k, n, n_cu):
    """The plan of E'T, with those of U = E sw and of T'T under 'u' and 'tt'."""
    splits = _lib.lowrank_splits(n)
    p = _lib.gemm_plan(d, 2 * k, n, splits, n_cu, a_kcontig=False)
    p['splits'], p['empty'] = splits, _empty_last(p, splits, n)
    p['u'] = _lib.gemm_plan(n, k, d, 1, n_cu)
    p['tt'] = _lib.gemm_plan(2 * k, 2 * k, n, splits, n_cu, a_kcontig=False)
    return p


def _ragged(m, n, p):
    return m % p['bm_rows'] != 0 and n % p['bn_cols'] != 0


def classify_a(n, d, n_cu):
    p = plan_a(n, d, n_cu)
    return ('A', _kernel(p), p['cfg'], '') if _ragged(n, d, p) else None


def classify_b(d, n, n_cu):
    p = plan_b(d, n, n_cu)
    s, ragged = p['splits'], _ragged(d, d, p)
    grouped = p['dma'] and s % 8 == 0
    if p['empty']:
        feature = None if grouped or not ragged else 'empty'
    elif grouped:
        feature = 'xcd-1tile' if d == 64 and p['grid_x'] == 1 else ('xcd' if ragged and p['grid_x'] > 1 else None)
    elif s == 1 and d % 64 == 2:
        feature = '1split'
    else:
        feature = '' if ragged else None
    return None if feature is None else ('B', _kernel(p), p['cfg'], feature)


def classify_c(d, k, n, n_cu):
    p = plan_c(d, k, n, n_cu)
    if not _ragged(d, 2 * k, p):
        return None
    if p['empty']:
        return ('C', _kernel(p), p['cfg'], 'empty') if p['splits'] == 32 else None
    return ('C', _kernel(p), p['cfg'], '1split' if p['splits'] == 1 else '')


CLASSIFY = {'A': classify_a, 'B': classify_b, 'C': classify_c}

# the variants the three entries are expected to reach on 256 compute units (the issue's tables)
VARIANTS = {
    'A': [('A', 'dma', 7, ''), ('A', 'dma', 3, ''), ('A', 'dma', 2, ''), ('A', 'dma', 6, ''), ('A', 'reg', 3, ''),
          ('A', 'reg', 2, ''), ('A', 'reg', 1, '')],
    'B': [('B', 'dma', 3, 'xcd-1tile'), ('B', 'dma', 3, 'xcd'), ('B', 'dma', 3, 'empty'), ('B', 'dma', 2, ''),
          ('B', 'reg', 3, 'empty'), ('B', 'reg', 2, ''), ('B', 'reg', 1, ''), ('B', 'dma', 3, '1split')],
    'C': [('C', 'dma', 6, ''), ('C', 'dma', 2, ''), ('C', 'dma', 3, 'empty'), ('C', 'reg', 1, ''), ('C', 'reg', 3, 'empty'),
          ('C', 'reg', 3, '1split')],
}

# (entry, kernel, cfg, splits, last split empty, shape) as the issue lists them for 256 compute units; shapes are (n, d) of
# A, (d, n) of B and (d, k, n) of C
TABLE_256 = [
    ('A', 'dma', 7, 1, False, (70, 272)), ('A', 'dma', 7, 1, False, (1000, 272)), ('A', 'dma', 3, 1, False, (6000, 208)),
    ('A', 'dma', 2, 1, False, (15566, 208)), ('A', 'dma', 6, 1, False, (21850, 272)), ('A', 'reg', 3, 1, False, (300, 200)),
    ('A', 'reg', 2, 1, False, (15566, 200)), ('A', 'reg', 1, 1, False, (32700, 200)),
    ('B', 'dma', 3, 8, False, (64, 2048)), ('B', 'dma', 3, 16, False, (200, 4096)), ('B', 'dma', 3, 20, True, (100, 5136)),
    ('B', 'dma', 2, 7, False, (1000, 1808)), ('B', 'reg', 3, 20, True, (100, 5128)), ('B', 'reg', 2, 7, False, (1000, 1800)),
    ('B', 'reg', 1, 1, False, (4096, 264)), ('B', 'dma', 3, 1, False, (130, 304)),
    ('C', 'dma', 6, 8, False, (2048, 256, 2048)), ('C', 'dma', 2, 32, False, (1536, 64, 8192)),
    ('C', 'dma', 3, 32, True, (300, 17, 8208)), ('C', 'reg', 1, 8, False, (2000, 250, 2056)),
    ('C', 'reg', 3, 32, True, (300, 17, 8200)), ('C', 'reg', 3, 1, False, (70, 5, 255)),
]
PLAN = {'A': plan_a, 'B': plan_b, 'C': plan_c}


def _round16(v):
    return (v + 15) // 16 * 16


def _candidates_a():
    """(cost, (n, d)): d = 208 and 272 (multiples of 16 that no tile width divides) and 200; n six past a multiple of 64."""
    out = []
    for d in (200, 208, 272):
        for t in range(1, CAP_BYTES // (8 * _round16(d) * 64)):
            out.append(((64 * t + 6) * d, (64 * t + 6, d)))
    return sorted(out)


def _candidates_b(n_cu):
    """(cost, (d, n)): d = 64 (one tile), 130 (two past a tile edge), 100, 200 and 72 past a multiple of 128; n a multiple of
    8 -- of 16 for the LDS-DMA kernel, 8 past one for the other; the cost counts the slabs."""
    out = []
    for d in (64, 100, 130, 200) + tuple(128 * t + 72 for t in range(1, 41)):
        for n in range(256, 8457, 8):
            splits = _lib.gram_splits(d, n, n_cu)
            if 8 * splits * d * _round16(d) <= CAP_BYTES:
                out.append((n * d + splits * d * d, (d, n)))
    return sorted(out)


def _candidates_c():
    """(cost, (d, k, n)): k of 5, 17, 60 and 250 (2k divides by no tile width), d = 70, 300 and 72 past a multiple of 128."""
    out = []
    for k in (5, 17, 60, 250):
        for d in (70, 300) + tuple(128 * t + 72 for t in range(3, 17)):
            for n in range(248, 8457, 8):
                out.append((n * (d + 2 * k) + _lib.lowrank_splits(n) * d * 2 * k, (d, k, n)))
    return sorted(out)


@functools.lru_cache(maxsize=None)
def cases(entry, n_cu):
    """The smallest candidate of every variant of ``entry`` that is reachable on ``n_cu`` compute units, in the order of
    VARIANTS; ``missing(entry, n_cu)`` names the others."""
    cand = {'A': _candidates_a, 'B': lambda: _candidates_b(n_cu), 'C': _candidates_c}[entry]()
    want, found = list(VARIANTS[entry]), {}
    for _, shape in cand:
        v = CLASSIFY[entry](*shape, n_cu)
        if v in want and v not in found:
            found[v] = Case(*v, shape)
            if len(found) == len(want):
                break
    return tuple(found[v] for v in want if v in found)


def missing(entry, n_cu):
    have = {c.variant for c in cases(entry, n_cu)}
    return [v for v in VARIANTS[entry] if v not in have]


# the edges of M and N: entry A at its smallest variant, exact pass
EDGE_N = (1, 63, 64, 65, 127, 128, 129)
EDGE_D = (1, 15, 16, 17, 63, 64, 65)
