"""The host reference of the Philox generator (tests/_philox_oracle.py) checked on its own, without a GPU: the
published known-answer vectors, its layout properties and the three distributions -- so that a wrong reference cannot
pass tests/test_gpu_philox_reference.py by agreeing with a wrong kernel."""
import numpy as np
import pytest
from scipy import stats

import _philox_oracle as P

R_TAIL = np.sqrt(2 * 20 * np.log(2))       # radius at u = 2^-20: every tail element lies beyond, no other does


def test_long_double_has_a_64_bit_mantissa():
    assert np.finfo(np.longdouble).nmant >= 63


@pytest.mark.parametrize('ctr,key,want', [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_random123_known_answers(ctr, key, want):
    got = P.philox4x32_10(*ctr, *key)
    assert tuple(int(x) for x in got) == want
    # vectorised: the same answers from arrays
    got = P.philox4x32_10(*[np.array([c, c], dtype=np.uint64) for c in ctr], *key)
    assert all(int(x[1]) == w for x, w in zip(got, want))


@pytest.mark.parametrize('offset', [0, 13, (1 << 32) + 5])
def test_reference_is_shard_invariant(offset):
    seed, stream, d = 21, (3 << 32) | 9, 9
    z, r, tail = P.normals(seed, stream, offset, 40, d)
    zs, rs, _ = P.normals(seed, stream, offset + 13, 16, d)
    assert np.array_equal(z[13:29], zs) and np.array_equal(r[13:29], rs)
    t, _ = P.student_t(seed, stream, offset, 40, d, 7.0)
    assert np.array_equal(t[13:29], P.student_t(seed, stream, offset + 13, 16, d, 7.0)[0])
    c, _ = P.chisquare(seed, stream, offset, 40, 9.0)
    assert np.array_equal(c[13:29], P.chisquare(seed, stream, offset + 13, 16, 9.0)[0])


def test_rows_g_and_g_xor_4_share_a_call():
    """Row g (bit 2 clear) takes words 0 / 1 and row g + 4 words 2 / 3 of the call at counter (quad id, pair)."""
    seed, stream, n, d = 5, 2, 24, 6
    rad, ang, _ = P.normal_words(seed, stream, 8, n, d // 2)
    for g in range(8, 8 + n):
        if g & 4:
            continue
        qid = ((g >> 3) << 2) | (g & 3)
        assert qid == int(P.quad_id(g)) == int(P.quad_id(g ^ 4))
        for j in range(d // 2):
            o = [int(x) for x in P.philox4x32_10(qid, 0, j, stream, seed, 0)]
            assert [int(rad[g - 8, j]), int(ang[g - 8, j])] == o[0:2]
            assert [int(rad[g - 4, j]), int(ang[g - 4, j])] == o[2:4]
    # distinct quads and distinct pairs never share a counter: all radius words differ
    assert np.unique(rad).size == rad.size


def test_key_and_counter_words():
    """seed_lo -> k0, seed_hi ^ stream_hi -> k1, stream_lo -> the counter's last word, rows >= 2^32 -> its second."""
    base = P.normals(0, 0, 0, 8, 4)[0]
    for seed, stream in [(1, 0), (1 << 32, 0), (0, 1), (0, 1 << 32), (0, 0xFFFFFFFF)]:
        assert not np.any(P.normals(seed, stream, 0, 8, 4)[0] == base)
    assert not np.any(P.normals(0, 0, 1 << 35, 8, 4)[0] == base)
    # the layout's known identity: the high words only enter through their XOR
    assert np.array_equal(P.normals(7 << 32, 7 << 32, 0, 8, 4)[0], base)


def test_reference_distributions():
    n = 100000
    z = P.normals(3, 1, 0, n // 10, 10)[0].astype(np.float64).ravel()
    assert stats.kstest(z, 'norm').pvalue > 1e-3
    assert abs(np.corrcoef(z[0::2], z[1::2])[0, 1]) < 0.02          # the two columns of a pair
    t, und = P.student_t(3, 1, 0, n // 10, 10, 3.5)
    assert not und.any()
    assert stats.kstest(t.astype(np.float64).ravel(), stats.t(3.5).cdf).pvalue > 1e-3
    c, und = P.chisquare(3, 1, 0, n, 2.5)
    assert not und.any()
    assert stats.kstest(c.astype(np.float64), stats.chi2(2.5).cdf).pvalue > 1e-3
    c, _ = P.chisquare(4, 0, 0, n, 100.0)
    assert stats.kstest(c.astype(np.float64), stats.chi2(100.0).cdf).pvalue > 1e-3


def test_tail_finder():
    hits = P.tail_hits_64()
    assert 6 <= len(hits) <= 32                      # 16 expected (8.4e6 calls, two words each, 2^-20 per word)
    assert {w for _, _, _, w in hits} == {0, 2}      # both kinds
    for seed, row, pair, word in hits:
        assert bool(row & 4) == (word == 2)
        z, r, tail = P.normals(seed, 0, 0, 64, 64)
        assert tail[row, 2 * pair] and tail[row, 2 * pair + 1]
        assert np.all(r[tail] > R_TAIL) and np.all(r[~tail] <= R_TAIL)
        assert np.all(np.isfinite(z.astype(np.float64)))
    # a seed without a hit has an empty mask
    clean = next(s for s in range(8192) if s not in {h[0] for h in hits})
    assert not P.normals(clean, 0, 0, 64, 64)[2].any()
