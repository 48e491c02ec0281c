"""Host reference of the throughput-mode generator (``rng='philox'``): what every element must be.

TEST INFRASTRUCTURE ONLY.  numpy, ``fractions`` and nothing else; written from the definitions -- Salmon et al.'s
Philox4x32-10 (SC'11), the Box-Muller transform, Bailey's polar method (Math. Comp. 62 (1994) 779-781) and Marsaglia and
Tsang's gamma method (ACM TOMS 26 (2000) 363-372) -- and from the layout DESIGN.md documents ("Philox layout"), not from
the device code: the transforms are evaluated in ``np.longdouble`` (64-bit mantissa) with libm's functions, where the
device uses its own fp64 polynomials.

Layout (element (row, col) is a pure function of (seed, stream, row, col)):

* key ``k0 = seed_lo``, ``k1 = seed_hi ^ stream_hi``;
* normals: counter ``(qid_lo, qid_hi, j, stream_lo)``, ``j = col >> 1``, ``qid = ((g >> 3) << 2) | (g & 3)``: rows g and
  g ^ 4 share a call; words 0 / 2 are the radius uniforms of the row with bit 2 clear / set, words 1 / 3 their angles;
  uniforms ``(k + 1/2) 2^-32``; a radius word below 4096 takes 32 more bits from sub-stream 0xEE of the same counter
  (word 0 for the row with bit 2 clear, word 2 for the other) and is scaled by 2^-64;
* sub-stream s of a counter: ``c.w + 0x9E3779B9 s``, ``k1 ^ (0x85EBCA6B s)`` (both mod 2^32);
* Student-t: counter ``(row_lo, row_hi, j, stream_lo)``, attempt a of column e of pair j is sub-stream 2 a + e; words
  (0, 1) and (2, 3) are two 53-bit uniforms ``((x >> 11) + 1/2) 2^-53`` formed in fp64;
* chi-square: pseudo column ``j = 0xFFFFFFFF``, attempt t takes its normal from sub-stream 2 t and its uniform from 2 t + 1.
"""
import functools
from fractions import Fraction

import numpy as np

LD = np.longdouble
_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
_PHILOX_M0, _PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_WEYL0, _WEYL1 = 0x9E3779B9, 0xBB67AE85
_SUB_C, _SUB_K = 0x9E3779B9, 0x85EBCA6B          # sub-stream steps of the counter's last word and of k1
_TAIL_SUB = 0xEE
_TWO_PI = LD(8) * np.arctan(LD(1))
_ATTEMPTS = 64                                   # the device gives up after this many rejections (never observed)


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32 with 10 rounds on uint64 arrays that hold 32-bit words (broadcast against each other)."""
    c0, c1, c2, c3, k0, k1 = (_u64(x) & _M32 for x in (c0, c1, c2, c3, k0, k1))
    for r in range(10):
        p0, p1 = _PHILOX_M0 * c0, _PHILOX_M1 * c2              # 32 x 32 -> 64: no overflow in uint64
        ka = (k0 + _u64((_WEYL0 * r) & 0xFFFFFFFF)) & _M32       # Weyl key schedule: round r uses key + r * W
        kb = (k1 + _u64((_WEYL1 * r) & 0xFFFFFFFF)) & _M32
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ ka, p1 & _M32, (p0 >> _S32) ^ c3 ^ kb, p0 & _M32
    return c0, c1, c2, c3


def _keys(seed, stream):
    seed, stream = int(seed), int(stream)
    assert 0 <= seed < 1 << 64 and 0 <= stream < 1 << 64
    return seed & 0xFFFFFFFF, (seed >> 32) ^ (stream >> 32), stream & 0xFFFFFFFF


def _rows(row_offset, n):
    return (np.arange(n, dtype=np.uint64) + np.uint64(int(row_offset)))[:, None]


def _sub(k1, w, sub):
    """Key word k1 and counter word w of sub-stream `sub` (an int or a uint64 array)."""
    if isinstance(sub, (int, np.integer)):
        return k1 ^ ((_SUB_K * int(sub)) & 0xFFFFFFFF), (w + _SUB_C * int(sub)) & 0xFFFFFFFF
    sub = _u64(sub)
    return _u64(k1) ^ ((np.uint64(_SUB_K) * sub) & _M32), (_u64(w) + np.uint64(_SUB_C) * sub) & _M32


def quad_id(g):
    g = _u64(g)
    return ((g >> np.uint64(3)) << np.uint64(2)) | (g & np.uint64(3))


def normal_words(seed, stream, row_offset, n, pairs):
    """(radius word, angle word, extra word of the tail call) of column pairs 0 .. pairs - 1 of n rows, as uint64."""
    k0, k1, w = _keys(seed, stream)
    g = _rows(row_offset, n)
    j = np.arange(pairs, dtype=np.uint64)[None, :]
    qid = quad_id(g)
    o = philox4x32_10(qid & _M32, qid >> _S32, j, w, k0, k1)
    k1t, wt = _sub(k1, w, _TAIL_SUB)
    e = philox4x32_10(qid & _M32, qid >> _S32, j, wt, k0, k1t)
    hi = ((g >> np.uint64(2)) & np.uint64(1)).astype(bool)
    hi = np.broadcast_to(hi, o[0].shape)
    return np.where(hi, o[2], o[0]), np.where(hi, o[3], o[1]), np.where(hi, e[2], e[0])


def normals(seed, stream, row_offset, n, d):
    """Rows [row_offset, row_offset + n) of the n_total x d matrix of standard normals of (seed, stream).

    Returns ``(z, r, tail)``: the matrix (long double), the Box-Muller radius of every element and the mask of the
    elements whose radius uniform came through the tail rule."""
    pairs = (d + 1) // 2
    rad, ang, extra = normal_words(seed, stream, row_offset, n, pairs)
    tail = rad < np.uint64(4096)
    u = (rad.astype(LD) + LD(0.5)) * LD(2) ** -32
    u64 = (rad.astype(LD) * LD(2) ** 32 + extra.astype(LD) + LD(0.5)) * LD(2) ** -64     # 44 bits + 1/2: exact
    u = np.where(tail, u64, u)
    r = np.sqrt(LD(-2) * np.log(u))
    phi = _TWO_PI * ((ang.astype(LD) + LD(0.5)) * LD(2) ** -32)
    z = np.empty((n, 2 * pairs), dtype=LD)
    z[:, 0::2] = r * np.cos(phi)
    z[:, 1::2] = r * np.sin(phi)
    return z[:, :d], np.repeat(r, 2, axis=1)[:, :d], np.repeat(tail, 2, axis=1)[:, :d]


def _u53(hi, lo):
    """The 53-bit uniform of two words, formed in fp64 as the generator defines it: ((x >> 11) + 1/2) 2^-53 (the sum
    rounds to even from 2^52 on; that rounded value IS the uniform)."""
    x = ((hi << _S32) | lo) >> np.uint64(11)
    return (x.astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)


_fused_w = np.frompyfunc(lambda u, v2: float(Fraction(u) * Fraction(u) + Fraction(v2)), 2, 1)


def student_t(seed, stream, row_offset, n, d, df):
    """Student-t(df) base noise by Bailey's polar method.  Returns ``(t, undecidable)``; t is long double.

    w = fma(u, u, v v) is the correctly rounded fused value of the fp64 u and the fp64 product v v (the formula is
    ill-conditioned in w next to 1, so both sides must start from the same fp64 w); everything after is long double."""
    k0, k1, w0 = _keys(seed, stream)
    g = np.broadcast_to(_rows(row_offset, n), (n, d)).ravel()
    col = np.broadcast_to(np.arange(d, dtype=np.uint64)[None, :], (n, d)).ravel()
    j, e = col >> np.uint64(1), col & np.uint64(1)
    size = n * d
    u_fin, w_fin = np.zeros(size), np.ones(size)
    undecidable = np.zeros(size, dtype=bool)
    todo = np.arange(size)
    for attempt in range(_ATTEMPTS):
        if todo.size == 0:
            break
        k1s, ws = _sub(k1, w0, np.uint64(2 * attempt) + e[todo])
        o = philox4x32_10(g[todo] & _M32, g[todo] >> _S32, j[todo], ws, k0, k1s)
        u = 2.0 * _u53(o[0], o[1]) - 1.0
        v = 2.0 * _u53(o[2], o[3]) - 1.0
        w = _fused_w(u, v * v).astype(np.float64)
        undecidable[todo] |= np.abs(w - 1.0) < 1e-12
        u_fin[todo], w_fin[todo] = u, w
        todo = todo[~((w <= 1.0) & (w > 0.0))]
    wl, ul, dfl = w_fin.astype(LD), u_fin.astype(LD), LD(df)
    t = ul * np.sqrt(dfl * np.expm1(LD(-2) / dfl * np.log(wl)) / wl)
    return t.reshape(n, d), undecidable.reshape(n, d)


def chisquare(seed, stream, row_offset, n, df):
    """n chi-square(df) draws, df > 2: twice a Gamma(df / 2) variate by Marsaglia and Tsang.  Returns
    ``(x, undecidable)``; x is long double.  Undecidable: an attempt with |t| < 1e-12 or whose acceptance test was
    closer than 1e-10."""
    k0, k1, w0 = _keys(seed, stream)
    g = _rows(row_offset, n).ravel()
    a = LD(df) / LD(2)
    dd = a - LD(1) / LD(3)
    c = LD(1) / np.sqrt(LD(9) * dd)
    v_fin = np.ones(n, dtype=LD)
    undecidable = np.zeros(n, dtype=bool)
    todo = np.arange(n)
    col = np.uint64(0xFFFFFFFF)
    for attempt in range(_ATTEMPTS):
        if todo.size == 0:
            break
        gt = g[todo]
        k1s, ws = _sub(k1, w0, 2 * attempt)
        o = philox4x32_10(gt & _M32, gt >> _S32, col, ws, k0, k1s)
        u1, u2 = _u53(o[0], o[1]).astype(LD), _u53(o[2], o[3]).astype(LD)
        x = np.sqrt(LD(-2) * np.log(u1)) * np.cos(_TWO_PI * u2)
        t = LD(1) + c * x
        undecidable[todo] |= np.abs(t) < 1e-12
        pos = t > 0
        v = np.where(pos, t * t * t, LD(1))
        k1s, ws = _sub(k1, w0, 2 * attempt + 1)
        q = philox4x32_10(gt & _M32, gt >> _S32, col, ws, k0, k1s)
        margin = LD(0.5) * x * x + dd - dd * v + dd * np.log(v) - np.log(_u53(q[0], q[1]).astype(LD))
        undecidable[todo] |= pos & (np.abs(margin) < 1e-10)
        accept = pos & (margin > 0)
        v_fin[todo[pos]] = v[pos]
        todo = todo[~accept]
    return LD(2) * dd * v_fin, undecidable


def find_tail_hits(seeds, n, d, stream=0):
    """Every (seed, row, pair, word) of the n x d matrices of `seeds` (row offset 0) whose radius word is below 4096:
    word 0 is the row with bit 2 clear, word 2 its partner row + 4.  Sorted by seed."""
    pairs = (d + 1) // 2
    lo_rows = np.array([g for g in range(n) if not g & 4], dtype=np.uint64)
    qid = quad_id(lo_rows)[None, :, None]
    j = np.arange(pairs, dtype=np.uint64)[None, None, :]
    _, k1, w = _keys(0, stream)
    seeds = np.asarray(list(seeds), dtype=np.uint64)
    hits = []
    for s0 in range(0, seeds.size, 512):
        chunk = seeds[s0:s0 + 512]
        k0 = (chunk & _M32)[:, None, None]
        kk1 = (chunk >> _S32)[:, None, None] ^ np.uint64(k1)
        o = philox4x32_10(qid & _M32, qid >> _S32, j, w, k0, kk1)
        for word in (0, 2):
            for si, ri, ji in zip(*np.nonzero(o[word] < np.uint64(4096))):
                row = int(lo_rows[ri]) + (4 if word else 0)
                if row < n:
                    hits.append((int(chunk[si]), row, int(ji), word))
    return sorted(hits)


@functools.lru_cache(maxsize=None)
def tail_hits_64():
    """The scan the tests share: seeds 0 .. 8191 at n = d = 64, stream 0 (8.4e6 Philox calls, 16 hits expected)."""
    return tuple(find_tail_hits(range(8192), 64, 64, 0))
