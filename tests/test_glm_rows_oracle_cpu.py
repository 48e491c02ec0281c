"""The reference of tests/test_gpu_glm_rows.py, held to account on the host: ``rows()`` in longdouble against mpmath at 50
digits in the links' tails, the ``counts`` shortcut against the expanded design, the float64 oracle against the GPU
tests' own criterion on every input set they use, and the Python mirrors of the chunk and split rules."""
import os
import re

import mpmath as mp
import numpy as np
import pytest

import _glm_rows_oracle as O
from _laplace_oracle import GLMOracle, KINDS
from viabel_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = np.longdouble
N_CUS = (64, 256, 304)
SD, S, XI = 10.0, 1.5, 0.5                      # prior_sd, noise_sd and the one design entry of the 50-digit checks


def _mp(v):
    """A longdouble as an mpf, exactly."""
    hi = float(v)
    return mp.mpf(hi) + mp.mpf(float(L(v) - L(hi)))


def _truth(kind, y, eta):
    """(f, g) of one observation with design entry XI at x = eta / XI, 50 digits."""
    y, eta, x = mp.mpf(y), mp.mpf(eta), mp.mpf(eta) / mp.mpf(XI)
    if kind == 'logistic':
        term, dl = y * eta - mp.log(1 + mp.exp(eta)), y - 1 / (1 + mp.exp(-eta))
    elif kind == 'poisson':
        term, dl = y * eta - mp.exp(eta) - mp.loggamma(y + 1), y - mp.exp(eta)
    else:
        s2 = mp.mpf(S) ** 2
        term, dl = -(y - eta) ** 2 / (2 * s2) - mp.log(2 * mp.pi * s2) / 2, (y - eta) / s2
    sd2 = mp.mpf(SD) ** 2
    return term - x * x / (2 * sd2) - (mp.log(mp.mpf(SD)) + mp.log(2 * mp.pi) / 2), dl * mp.mpf(XI) - x / sd2


# the Poisson responses stay small: -log(y!) enters the oracle through a float64 gammaln, which is 1e-17 of f only then
TAILS = ([('logistic', y, eta) for y in (0.0, 1.0) for eta in (0.0, -0.0, 37.0, -37.0, 745.0, -745.0, 2000.0, -2000.0)]
         + [('poisson', y, eta) for y in (0.0, 3.0) for eta in (-745.0, -30.0, 30.0, 80.0)]
         + [('linear', 1e6 + 0.25, 0.25), ('linear', -1e6, 0.75)])


@pytest.mark.parametrize('kind,y,eta', TAILS)
def test_longdouble_rows_match_50_digits_in_the_tails(kind, y, eta):
    with mp.workdps(50):
        oracle = GLMOracle(kind, [[XI]], [y], prior_sd=SD, noise_sd=S, dtype=L)
        f, g, bf, bg = O.rows(oracle, [[eta / XI]])
        tf, tg = _truth(kind, y, eta)
        ef, eg = abs(_mp(f[0]) - tf) / abs(tf), abs(_mp(g[0, 0]) - tg) / abs(tg)
        print('%s y=%g eta=%g: rel err f %s g %s' % (kind, y, eta, mp.nstr(ef, 3), mp.nstr(eg, 3)))
        assert ef <= mp.mpf('1e-17') and eg <= mp.mpf('1e-17')
        assert np.isfinite(bf[0]) and np.isfinite(bg[0, 0]) and bf[0] >= abs(f[0]) and bg[0, 0] >= abs(g[0, 0])


@pytest.mark.parametrize('kind', KINDS)
def test_counts_equal_the_expanded_design(kind):
    """n_data = 500 observations that cycle through 61: the shortcut's sums differ from the full ones in their order only."""
    case = O.cycle_case(kind, 3, 500, 40)
    assert case.X.shape[0] == 61 and case.counts.sum() == 500 and set(case.counts) == {8.0, 9.0}
    Xf, yf = case.design()
    assert Xf.shape == (500, 3) and np.array_equal(Xf[61 + 5], case.X[5]) and yf[499] == case.y[499 % 61]
    f, g, bf, bg = O.rows(case.oracle(L), case.x, case.counts)
    ff, gf, bff, bgf = O.rows(GLMOracle(kind, Xf, yf, case.prior_sd, case.noise_sd, dtype=L), case.x)
    assert np.all(np.abs(f - ff) <= L(1e-17) * bf) and np.all(np.abs(g - gf) <= L(1e-17) * bg)
    assert np.all(np.abs(bf - bff) <= L(1e-17) * bf) and np.all(np.abs(bg - bgf) <= L(1e-17) * bg)


@pytest.mark.parametrize('case', O.all_cases(256), ids=lambda case: case.name)      # the MI355X has 256 compute units
def test_float64_oracle_passes_the_criterion(case):
    """The reference alone stays inside the bound the device is held to, on every input set of the GPU tests."""
    f, g, bf, bg = case.reference()
    assert f.dtype == L and np.all(np.isfinite(f)) and np.all(np.isfinite(g))
    assert np.all(np.isfinite(bf)) and np.all(np.isfinite(bg)) and np.all(bf > 0)
    f64, g64, bf64, bg64 = O.rows(case.oracle(np.float64), case.x, case.counts)
    assert f64.dtype == np.float64 and np.array_equal(bf64, bf) and np.array_equal(bg64, bg)     # bounds: reference only
    ef, eg = O.excess(f64, f, bf).max(), O.excess(g64, g, bg).max()
    print('%s: float64 oracle f %.2f g %.2f of %d allowed' % (case.name, ef, eg, case.limit))
    assert ef <= case.limit and eg <= case.limit
    assert case.limit >= 22


def test_excess_flags_what_it_should():
    one = np.ones(3)
    r = O.excess([1.0, 1.0 + 2.0 ** -50, np.nan], one, one)
    assert r[0] == 0.0 and r[1] == 8.0 and np.isnan(r[2])
    assert O.excess([0.0], [0.0], np.zeros(1, dtype=L))[0] == 0.0 and np.isinf(O.excess([1.0], [0.0], np.zeros(1, dtype=L))[0])


def test_tail_inputs_are_what_they_claim():
    for kind, scale in O.tail_cases():
        case = O.tail_case(kind, scale)
        eta = case.x @ case.X.T
        assert case.x.shape == (O.TAIL_N, O.TAIL_D) and case.X.shape == (O.TAIL_N_DATA, O.TAIL_D)
        assert not case.x[-4].any() and not case.x[-3].any() and np.all(np.signbit(case.x[-3])) and not np.any(np.signbit(case.x[-4]))
        assert np.all(eta[-2] > 0) and np.all(eta[-1] < 0)
        lo, hi = {('logistic', 15.0): (80, 130), ('logistic', 300.0): (1600, 2600), ('poisson', 6.0): (32, 52),
                  ('poisson', 12.0): (64, 104), ('linear', 1e6): (4e6, 2e7)}[kind, scale]
        assert lo < np.abs(eta).max() < hi, (kind, scale, np.abs(eta).max())
        if kind == 'poisson':
            assert case.y[0] == 0.0 and case.y[1] == 1e6 and np.exp(np.abs(eta).max()) < 1e45
        if kind == 'linear':
            assert np.abs(case.y[:, None] - eta.T).max() >= 1e6
    assert len(set(O.TAIL_BAD_ROWS)) == 2 and max(O.TAIL_BAD_ROWS) < O.TAIL_N - 4


# ---- the mirrors -----------------------------------------------------------------------------------------------------
def test_chunk_mirror_matches_the_source_and_the_cases():
    src = open(os.path.join(ROOT, 'viabel_amd', 'csrc', 'vb_rows.hip')).read()
    for name, value in (('kGlmRowsLogpDoubles', _lib.GLM_ROWS_LOGP_DOUBLES), ('kGlmRowsGradDoubles', _lib.GLM_ROWS_GRAD_DOUBLES)):
        m = re.search(name + r'\s*=\s*\(int64_t\)(\d+)\s*<<\s*(\d+)', src)
        assert m and int(m.group(1)) << int(m.group(2)) == value
        assert len(re.findall(name + r' / ldt', src)) == 1
    m = re.search(r'kGlmRowsMinChunk\s*=\s*(\d+)', src)
    assert m and int(m.group(1)) == _lib.GLM_ROWS_MIN_CHUNK == 128
    assert len(re.findall(r'chunk < kGlmRowsMinChunk \? kGlmRowsMinChunk : \(chunk > n \? n : chunk\)', src)) == 2
    assert _lib.glm_rows_chunk(O.CROSS_N_DATA, True) == O.CROSS_CHUNK_GRAD == (32 << 20) // 70016
    assert _lib.glm_rows_chunk(O.CROSS_N_DATA, False) == O.CROSS_CHUNK_LOGP == (64 << 20) // 70016
    assert -(-O.CROSS_N_GRAD // O.CROSS_CHUNK_GRAD) == 3 and O.CROSS_N_GRAD % O.CROSS_CHUNK_GRAD == 5
    assert -(-O.CROSS_N_GRAD // O.CROSS_CHUNK_LOGP) == 2 and O.CROSS_N_GRAD % O.CROSS_CHUNK_LOGP == 5
    assert -(-O.CROSS_N_LOGP // O.CROSS_CHUNK_LOGP) == 3 and O.CROSS_N_LOGP % O.CROSS_CHUNK_LOGP == 5
    assert (32 << 20) // 262208 == 127 and _lib.glm_rows_chunk(O.FLOOR_N_DATA, True) == 128      # the floor binds
    assert _lib.glm_rows_chunk(O.FLOOR_N_DATA, False) == 255 and O.FLOOR_N == 133
    assert _lib.glm_rows_chunk(1, True) == 32 << 16 and _lib.glm_rows_chunk(16, False) == 64 << 16
    assert _lib.glm_rows_chunk(17, True) == 32 << 15


def _splits_transcribed(rows, d, n_data, n_cu):
    """``glm_grad_splits`` of csrc/vb_rows.hip, statement by statement."""
    tiles = ((rows + 63) // 64) * ((d + 63) // 64)
    if tiles >= n_cu:
        return 1
    splits = 2 * n_cu // tiles
    max_splits = n_data // 128
    if splits > max_splits:
        splits = max_splits
    if splits > 64:
        splits = 64
    if splits < 1:
        splits = 1
    return splits


def test_split_mirror_matches_the_source():
    src = open(os.path.join(ROOT, 'viabel_amd', 'csrc', 'vb_rows.hip')).read()
    body = re.search(r'inline int glm_grad_splits\(int64_t rows, int d, int64_t n_data, int n_cu\)\s*\{(.*?)\n\}', src, flags=re.S)
    assert body
    for piece in ('gemm_max_blocks(rows, d)', 'if (tiles >= n_cu) return 1;', '(int)(2 * n_cu / tiles)', '(int)(n_data / 128)',
                  'if (splits > max_splits) splits = max_splits;', 'if (splits > 64) splits = 64;', 'if (splits < 1) splits = 1;'):
        assert piece in body.group(1), piece
    assert 'glm_grad_splits(n, d, m.n_data, n_cu)' in src
    gemm = open(os.path.join(ROOT, 'viabel_amd', 'csrc', 'vb_gemm_f64.h')).read()
    assert 'gemm_max_blocks(int64_t M, int64_t N) { return ((M + 63) / 64) * ((N + 63) / 64); }' in gemm
    for n_cu in N_CUS + (1, 32, 33):
        for rows in (1, 5, 64, 65, 130, 479, 1024, 1533, 20000):
            for d in (1, 2, 64, 65, 1024):
                for n_data in (1, 100, 127, 128, 255, 256, 300, 3457, 8191, 8192, 8327, 70001):
                    assert _lib.glm_grad_splits(rows, d, n_data, n_cu) == _splits_transcribed(rows, d, n_data, n_cu)


@pytest.mark.parametrize('n_cu', N_CUS)
def test_ladder_cases_reach_their_regimes(n_cu):
    want = {'floor': 1, 'max_splits': 2, 'cap': 64, 'one_launch': 1}
    cases = O.ladder_cases(n_cu)
    assert [c[0] for c in cases] == ['floor', 'max_splits', 'cu_bound', 'cap', 'one_launch']
    for regime, rows, d, n_data in cases:
        got, splits = O.ladder_regime(rows, d, n_data, n_cu)
        assert got == regime and splits == _lib.glm_grad_splits(rows, d, n_data, n_cu), (regime, got, splits)
        if regime == 'cu_bound':
            assert 2 < splits < 64 and splits == 2 * n_cu // 24 < n_data // 128
        else:
            assert splits == want[regime]
        if splits > 1:
            assert n_data % (16 * splits) != 0
    assert cases[0][3] == 100 and cases[1][3] == 300 and cases[3][1:] == (130 if n_cu >= 98 else 61, 2, 8327)
    side = 64 * int(np.ceil(np.sqrt(n_cu)))
    assert cases[4][1:] == (side, side, 257) and (side // 64) ** 2 >= n_cu
    rows, d, n_data = O.WHOLE_SLABS
    assert n_data % 16 == 0 and _lib.glm_grad_splits(rows, d, n_data, n_cu) == 3 and n_data == 3 * 128
    for n_data in O.EDGE_N_DATA:                             # below 256 observations there is one slab
        assert _lib.glm_grad_splits(7, 5, n_data, n_cu) == 1
    # what the three-chunk and the floor cases hit: full chunks and their 5-row remainders
    for rows, d, n_data in ((O.CROSS_CHUNK_GRAD, O.CROSS_D, O.CROSS_N_DATA), (5, O.CROSS_D, O.CROSS_N_DATA),
                            (128, O.FLOOR_D, O.FLOOR_N_DATA), (5, O.FLOOR_D, O.FLOOR_N_DATA)):
        assert _lib.glm_grad_splits(rows, d, n_data, n_cu) == min(64, 2 * n_cu // ((rows + 63) // 64))
