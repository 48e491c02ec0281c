"""Host only: the fp64 GEMM launcher's decision (vb_gemm_plan: the function gemm_f64_launch itself calls) and the two split
rules behind the raw entries, and tests/_gemm_oracle.py -- the cases, references and criterion of
tests/test_gpu_gemm_raw.py -- held to account: the issue's 256-CU table against the plan, the plan's invariants over a seeded
sweep, the case builders at 64, 256 and 304 compute units, the float64 reference against Python integers and the bound
against mpmath at 50 digits."""
import ctypes
import os

import mpmath as mp
import numpy as np
import pytest

import _gemm_oracle as O
from viabel_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = np.longdouble
N_CUS = (64, 256, 304)
TILE = {1: (128, 128), 2: (128, 64), 3: (64, 64), 4: (64, 64), 5: (128, 64), 6: (128, 128), 7: (64, 32), 8: (64, 32)}


def _src(name):
    with open(os.path.join(ROOT, 'viabel_amd', 'csrc', name)) as f:
        return f.read()


# ---- the issue's table -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('row', O.TABLE_256, ids=lambda r: '%s-%s-cfg%d-%s' % (r[0], r[1], r[2], 'x'.join(map(str, r[5]))))
def test_table_for_256_compute_units(row):
    """Every row as the issue wrote it (none needed a correction): kernel, cfg, split count, and whether the last split is
    empty."""
    entry, kernel, cfg, splits, empty, shape = row
    p = O.PLAN[entry](*shape, 256)
    assert ('dma' if p['dma'] else 'reg', p['cfg'], p['splits'], p['empty']) == (kernel, cfg, splits, empty)
    k = shape[1] if entry == 'A' else shape[-1]
    assert p['dma'] == (k % 16 == 0)
    if empty:
        assert (splits - 1) * p['k_split'] >= k > (splits - 2) * p['k_split']       # exactly one empty split
        assert splits - 1 > k // (16 * splits)                                     # the issue's condition for it


def test_table_covers_every_variant():
    seen = {(e, kern, cfg) for e, kern, cfg, _, _, _ in O.TABLE_256}
    assert seen == {v[:3] for e in 'ABC' for v in O.VARIANTS[e]}
    assert sum(len(v) for v in O.VARIANTS.values()) == 21 and len(O.TABLE_256) == 22    # (A's cfg 7 is listed twice)


# ---- the plan's invariants -------------------------------------------------------------------------------------------
def _count_tiles(m, n, tri_mode, bm, bn):
    tm, tn = -(-m // bm), -(-n // bn)
    if tri_mode != 2:
        return tm * tn
    return sum(min((r * bm + bm - 1) // bn + 1, tn) for r in range(tm))           # lower tiles: bn * c <= last row of r


def _sweep(n_cu, count):
    rng = np.random.RandomState(n_cu)
    sizes = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200, 208, 272, 1000, 1024, 4096, 8200, 8208, 32700)
    for _ in range(count):
        m, n, k = (int(rng.choice(sizes)) if rng.rand() < 0.5 else int(rng.randint(1, 5000)) for _ in range(3))
        tri = int(rng.choice((0, 0, 0, 1, 2, 2, 3, 4)))
        if tri == 2:
            n = m
        yield dict(m=m, n=n, k=k, splits=int(rng.choice((1, 1, 2, 7, 8, 16, 20, 32, 64))), n_cu=n_cu, tri_mode=tri,
                   batch=int(rng.choice((0, 0, 0, 1))), a_kcontig=bool(rng.rand() < 0.5), narrow_ok=bool(rng.rand() < 0.5),
                   narrow_auto=bool(rng.rand() < 0.5), cfg=int(rng.choice((0, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8))),
                   flags=int(rng.rand() < 0.2))


@pytest.mark.parametrize('n_cu', N_CUS)
def test_plan_invariants(n_cu):
    seen = set()
    for a in _sweep(n_cu, 1500):
        a['narrow_ok'] = a['narrow_ok'] and a['a_kcontig']           # the launcher's kNarrowOk implies A_KCONTIG ...
        a['narrow_auto'] = a['narrow_auto'] and a['narrow_ok']       # ... and its kNarrowAuto kNarrowOk
        p = _lib.gemm_plan(**a)
        where = (a, p)
        seen.add((p['dma'], p['cfg']))
        assert p['k_split'] % 16 == 0 and p['k_split'] > 0, where
        if a['batch']:
            assert a['k'] <= p['k_split'] < a['k'] + 16, where       # batch mode: every product runs over the whole K
        else:
            assert a['splits'] * p['k_split'] >= a['k'], where
            assert p['k_split'] - 16 < -(-a['k'] // a['splits']) <= p['k_split'], where
        assert p['dma'] == (a['k'] % 16 == 0 and not a['flags'] & 1), where
        assert p['cfg'] in (TILE if p['dma'] else (1, 2, 3)), where
        assert (p['bm_rows'], p['bn_cols']) == TILE[p['cfg']], where
        assert p['grid_x'] == _count_tiles(a['m'], a['n'], a['tri_mode'], p['bm_rows'], p['bn_cols']), where
        if p['bn_cols'] == 32:
            assert a['narrow_ok'] and p['dma'], where
            assert a['cfg'] >= 7 or a['narrow_auto'], where
        if a['cfg'] in (1, 2, 3):
            assert p['cfg'] == a['cfg'], where                      # a tile both kernels have is the caller's to choose
        if a['cfg'] == 0 and p['cfg'] == 7:
            assert a['tri_mode'] in (0, 3, 4) and not a['batch'], where      # (3 and 4 fall back to dense in places)
            assert _count_tiles(a['m'], a['n'], 0, 64, 64) * a['splits'] <= n_cu, where
        if a['cfg'] == 0 and p['cfg'] in (1, 6) and not a['batch']:
            assert _count_tiles(a['m'], a['n'], a['tri_mode'], 128, 128) * a['splits'] >= 2 * n_cu, where
    assert {(True, c) for c in (2, 3, 4, 6, 7, 8)} | {(False, c) for c in (1, 2, 3)} <= seen      # the sweep is no stub


def test_plan_argument_errors():
    lib = _lib.load()
    out = (ctypes.c_int * 6)()
    good = [70, 272, 272, 1, 256, 0, 0, 1, 1, 1, 0, 0]
    assert lib.vb_gemm_plan(*good, out) == _lib.VB_OK and tuple(out) == (7, 1, 64, 32, 272, 18)
    assert lib.vb_gemm_plan(*good, None) == _lib.VB_ERR_INVALID
    for index in range(5):                                           # m, n, k, splits, n_cu
        for bad in (0, -1):
            args = list(good)
            args[index] = bad
            assert lib.vb_gemm_plan(*args, out) == _lib.VB_ERR_INVALID, (index, bad)
    for index, bad in ((5, -1), (5, 5), (6, -1), (10, -1), (10, 9), (11, -1)):      # tri_mode, batch, cfg, flags
        args = list(good)
        args[index] = bad
        assert lib.vb_gemm_plan(*args, out) == _lib.VB_ERR_INVALID, (index, bad)
    with pytest.raises(ValueError):
        _lib.gemm_plan(0, 1, 1)
    n = ctypes.c_int(0)
    assert lib.vb_gram_splits_plan(100, 5136, 256, None) == _lib.VB_ERR_INVALID
    assert lib.vb_lowrank_splits_plan(8200, None) == _lib.VB_ERR_INVALID
    for args in ((0, 5136, 256), (100, 0, 256), (100, 5136, 0)):
        assert lib.vb_gram_splits_plan(*args, ctypes.byref(n)) == _lib.VB_ERR_INVALID
        with pytest.raises(ValueError):
            _lib.gram_splits(*args)
    assert lib.vb_lowrank_splits_plan(0, ctypes.byref(n)) == _lib.VB_ERR_INVALID
    with pytest.raises(ValueError):
        _lib.lowrank_splits(0)


def test_split_rules():
    """The two exported rules against their statements, and the sources: one copy of each, called by the entries."""
    for n_cu in N_CUS + (1, 8):
        for d in (1, 64, 100, 128, 129, 200, 1000, 1024, 4096):
            for n in (1, 255, 256, 264, 1800, 2048, 5128, 5136, 100000):
                tiles = -(-d // 128)
                want = max(1, min(n_cu // (tiles * (tiles + 1) // 2), max(1, n // 256)))
                assert _lib.gram_splits(d, n, n_cu) == want, (d, n, n_cu)
    for n in (1, 255, 256, 511, 512, 2056, 8191, 8192, 8200, 8208, 100000):
        assert _lib.lowrank_splits(n) == max(1, min(32, n // 256)), n
    linalg, lowrank, fullrank, gemm = (_src(f) for f in ('vb_linalg.hip', 'vb_lowrank_obj.hip', 'vb_fullrank.hip', 'vb_gemm_f64.h'))
    assert 'const int splits = gemm_lr_splits(n);' in linalg and 'n / 256' not in linalg
    assert 'const int splits = gemm_lr_splits(n);' in lowrank and 'n / 256' not in lowrank
    assert 'return gemm_gram_splits(d, n, ctx->prop.multiProcessorCount);' in fullrank and 'n / 256' not in fullrank
    assert gemm.count('n / 256') == 4                               # the two rules, statement and comment each ...
    assert gemm.count('const GemmPlan plan = gemm_f64_plan(g.M, g.N, g.K, splits, n_cu, g.tri_mode, g.batch, A_KCONTIG,') == 1
    assert gemm.count('cfg = 7;') == 1 and gemm.count('cfg = 6;') == 1      # ... and one copy of the tile decision


# ---- the case builders -----------------------------------------------------------------------------------------------
def _bytes(entry, shape, p):
    if entry == 'A':
        n, d = shape
        return [8 * n * O._round16(d)]
    if entry == 'B':
        d, n = shape
        return [8 * n * O._round16(d), 8 * p['splits'] * d * O._round16(d)]
    d, k, n = shape
    ldt = max(32, O._round16(2 * k))
    return [8 * n * O._round16(d), 8 * n * ldt, 8 * p['splits'] * d * ldt]


@pytest.mark.parametrize('n_cu', N_CUS)
@pytest.mark.parametrize('entry', 'ABC')
def test_case_builders_reach_their_variants(entry, n_cu):
    cases = O.cases(entry, n_cu)
    print(n_cu, [c.name for c in cases], 'missing', O.missing(entry, n_cu))
    assert [c.variant for c in cases] == [v for v in O.VARIANTS[entry] if v not in O.missing(entry, n_cu)]
    if n_cu == 256:
        assert O.missing(entry, n_cu) == [] and len(cases) == len(O.VARIANTS[entry])
    for c in cases:
        p = O.PLAN[entry](*c.shape, n_cu)
        m, n, k = {'A': lambda s: (s[0], s[1], s[1]), 'B': lambda s: (s[0], s[0], s[1]),
                   'C': lambda s: (s[0], 2 * s[1], s[2])}[entry](c.shape)
        assert (c.entry, 'dma' if p['dma'] else 'reg', p['cfg']) == (entry, c.kernel, c.cfg), c
        assert p['dma'] == (k % 16 == 0), c
        assert max(_bytes(entry, c.shape, p)) <= O.CAP_BYTES, c
        last_starts = (p['splits'] - 1) * p['k_split']
        assert (c.feature == 'empty') == (last_starts >= k), c
        if c.feature != 'xcd-1tile' and not (entry == 'B' and c.feature == '1split'):
            assert m % p['bm_rows'] != 0 and n % p['bn_cols'] != 0, c                # ragged both ways
        if entry == 'A':
            assert p['splits'] == 1 and c.feature == ''
        if entry == 'B':
            grouped = p['dma'] and p['splits'] % 8 == 0
            assert grouped == c.feature.startswith('xcd'), c
            if c.feature == 'xcd-1tile':
                assert p['grid_x'] == 1 and p['splits'] >= 8
            if c.feature == 'xcd':
                assert p['grid_x'] > 1 and p['splits'] >= 8
            if c.feature == '1split':
                assert p['splits'] == 1 and m % 64 == 2 and p['grid_x'] > 1
        if entry == 'C':
            assert (c.feature == '1split') == (p['splits'] == 1), c
            if c.feature == 'empty':
                assert p['splits'] == 32
            assert c.shape[1] <= 256                                                 # the entry's own limit on k


def test_edge_shapes_take_the_smallest_tiles():
    for d in O.EDGE_D:
        for n in O.EDGE_N:
            p = O.plan_a(n, d, 256)
            assert (p['dma'], p['cfg']) == ((True, 7) if d % 16 == 0 else (False, 3)), (n, d)


# ---- the oracle ------------------------------------------------------------------------------------------------------
def test_float64_reference_is_exact_on_integer_inputs():
    rng = np.random.RandomState(5)
    a, b = O.int_matrix(rng, 9, 300), O.int_matrix(rng, 5, 300)
    assert a.min() == -7 and a.max() == 7 and np.array_equal(a, np.rint(a))
    c = O.product_check('c', a, b, 301, 64, 0)
    exact = [[sum(int(x) * int(y) for x, y in zip(ra, rb)) for rb in b] for ra in a]
    bound = [[sum(abs(int(x) * int(y)) for x, y in zip(ra, rb)) for rb in b] for ra in a]
    assert c.ref.tolist() == exact and c.bound.tolist() == bound
    assert [[int(v) for v in row] for row in c.ref_rows] == exact
    O.assert_exact(c.bound)
    assert c.ratios(c.ref) == (0.0, 0.0)
    with pytest.raises(AssertionError):
        O.assert_exact(np.array([2.0 ** 53]))
    p = O.int_precision(rng, 17)
    assert np.array_equal(p, p.T) and np.all(np.diag(p) == 68) and np.abs(p - np.diag(np.diag(p))).max() <= 3
    assert np.linalg.slogdet(p)[0] == 1.0 and np.array_equal(0.5 * (p + p.T), p)
    P, mean, x = O.inputs_a(5, 17, 'exact')
    assert not mean.any() and np.array_equal(x, np.rint(x)) and np.abs(x).max() <= 7
    P, mean, x = O.inputs_a(5, 17, 'real')
    assert mean.all() and np.array_equal(P, P.T) and np.all(np.linalg.eigvalsh(P) >= 1.0 - 1e-9)


def _mp(v):
    hi = float(v)
    return mp.mpf(hi) + mp.mpf(float(L(v) - L(hi)))


def test_bound_against_50_digits_on_an_ill_cancelling_product():
    """Rows of b that nearly cancel against a: the float64 product, the longdouble product and the bound against exact
    arithmetic."""
    rng = np.random.RandomState(11)
    m, n, k = 4, 3, 60
    a, b = O.real_matrix(rng, m, k), O.real_matrix(rng, n, k)
    for i in range(n):                                               # row i of b cancels row i of a to ~1e-16 of the terms
        b[i, -1] = -(a[i, :-1] @ b[i, :-1]) / a[i, -1]
    with mp.workdps(50):
        c = O.product_check('c', a, b, k + 1, 64, 0)
        assert list(c.rows) == list(range(m))
        worst64 = worstl = mp.mpf(0)
        for i in range(m):
            for j in range(n):
                exact = mp.fsum(mp.mpf(a[i, t]) * mp.mpf(b[j, t]) for t in range(k))
                bound = mp.fsum(abs(mp.mpf(a[i, t]) * mp.mpf(b[j, t])) for t in range(k))
                assert abs(_mp(c.bound_rows[i, j]) - bound) <= mp.mpf(k) * mp.mpf(2) ** -64 * bound
                assert abs(mp.mpf(c.bound[i, j]) - bound) <= mp.mpf(O.gamma(k)) * bound
                worst64 = max(worst64, abs(mp.mpf(c.ref[i, j]) - exact) / (mp.mpf(O.gamma(k)) * bound))
                worstl = max(worstl, abs(_mp(c.ref_rows[i, j]) - exact) / (mp.mpf(k) * mp.mpf(2) ** -64 * bound))
        cancel = min(abs(c.ref[i, i]) / c.bound[i, i] for i in range(n))
        print('float64 %s of g(K) bound, longdouble %s of K 2^-64 bound; |c| / bound down to %.1e'
              % (mp.nstr(worst64, 3), mp.nstr(worstl, 3), cancel))
        assert worst64 <= 1 and worstl <= 1 and cancel < 1e-13
    r64, rl = c.ratios(c.ref)
    assert r64 == 0.0 and rl <= 1.0                                  # the float64 product passes the longdouble criterion
    bad = c.ref.copy()
    bad[2, 1] += 3.0 * O.gamma(k + 1) * c.bound[2, 1]
    assert c.ratios(bad)[0] > 1.0 and c.ratios(bad)[1] > 1.0
    bad[2, 1] = np.nan
    assert c.ratios(bad) == (np.inf, np.inf)


def test_criterion_accepts_another_order_and_refuses_a_missing_piece():
    """Entry B and C on the host: the same sums in another order (per-split partial sums, float32-free) pass; a dropped
    16-row slab, a split left out of the slab sum and a stale non-zero slab do not."""
    n, d, k, splits = 1000, 37, 5, 3
    E = O.inputs_b(d, n, 'real')
    gram, colsum = O.checks_b(E, splits, 64)
    parts = [E[s::splits].T @ E[s::splits] for s in range(splits)]          # interleaved splits: another order entirely
    for got in (parts[0] + parts[1] + parts[2], parts[2] + (parts[1] + parts[0])):
        r = gram.ratios(got)
        assert r[0] <= 1.0 and r[1] <= 1.0
    assert min(gram.ratios(parts[0] + parts[1])) > 1e3                       # a split left out
    assert min(gram.ratios(E[:-16].T @ E[:-16])) > 1e3                       # the last slab dropped
    assert min(gram.ratios(gram.ref + 1e-9 * parts[0])) > 1.0                # a stale slab, scaled down a billion times
    assert max(colsum.ratios(E[::-1].sum(0))) <= 1.0 and min(colsum.ratios(E[1:].sum(0))) > 1e3
    E, Z, sw = O.inputs_c(d, k, n, 'real')
    checks = O.checks_c(E, Z, sw, splits, 64)
    assert [c.name for c in checks] == ["E'T", "T'T", 'sum E', 'sum E^2', 'sum T']
    u = np.stack([np.sum((E * sw[:, j])[:, ::-1], axis=1) for j in range(k)], axis=1)      # U summed backwards
    t = np.concatenate([Z, u], axis=1)
    outs = [E[::-1].T @ t[::-1], t[::-1].T @ t[::-1], E.sum(0), (E * E)[::-1].sum(0), t[::-1].sum(0)]
    for c, got in zip(checks, outs):
        r = c.ratios(got)
        assert r[0] <= 1.0 and r[1] <= 1.0, (c.name, r)
    t_bad = t.copy()
    t_bad[:, k] = 0.0                                                        # one column of U never written
    for c, got in zip(checks[:2], (E.T @ t_bad, t_bad.T @ t_bad)):
        assert min(c.ratios(got)) > 1e3, c.name
    E, Z, sw = O.inputs_c(d, k, 64, 'exact')
    for c in O.checks_c(E, Z, sw, 1, 64):
        O.assert_exact(c.bound)
        assert np.array_equal(c.ref, np.rint(c.ref)) and np.array_equal(c.ref_rows.astype(np.float64), c.ref[c.rows])


def test_sample_rows():
    for m, bm in ((1, 64), (70, 64), (130, 128), (4040, 128), (32646, 128)):
        rows = O.sample_rows(m, bm, 3)
        assert len(rows) == min(m, O.MAX_SAMPLE_ROWS) == len(set(rows.tolist())) and np.all(np.diff(rows) > 0)
        assert rows[0] == 0 and rows[-1] == m - 1
        tiles = -(-m // bm)
        for r in (bm - 1, bm, (tiles - 1) * bm - 1, (tiles - 1) * bm):      # the edges of the first and of the last tile
            if 0 <= r < m:
                assert r in rows, (m, bm, r)
        assert np.array_equal(rows, O.sample_rows(m, bm, 3))
