"""GPU: the fp64 GEMM's tile variants through the three public entries that return a bare product -- operand fetch, tiling,
k loop, ragged edges and k splits of both kernels (csrc/vb_gemm_f64.h register-staged, vb_gemm_f64_dma.h LDS-DMA) for both
layouts of A.  Entries, variants, inputs and the criterion are defined in tests/_gemm_oracle.py (tests/test_gemm_plan_cpu.py
checks them on the host):

  A  Engine.model_grad on CorrelatedGaussianModel        G = -(x - m) P         A row-major, one split
  B  Engine.noise_moments(want_gram=True)                E'E, column sums       A k-major, lower tiles, gram_splits
  C  Engine.lowrank_path_terms                           U = E sw, E'T, T'T, three column sums      lowrank_splits

Every case is built for the engine's own CU count through vb_gemm_plan -- the launcher's decision function -- and the test
asserts through it which kernel and tile the case takes.  Then
  exact pass   integer inputs: every output equals numpy's float64 product bit for bit (B: and gram == gram')
  real pass    |dev - ref| <= 2 g (|A| |B|)_ij against float64 over the whole output, <= 1 g against longdouble on 64 rows,
               g = (K + s) u / (1 - (K + s) u); run twice, equal bits
The cases whose last k split is empty run right after a larger case of the same entry and kernel, whose partial slabs are
still in the shared workspace: a slab that is not written would show as a stale one.
The edges of M and N: n in {1, 63, 64, 65, 127, 128, 129} x d in {1, 15, 16, 17, 63, 64, 65} through entry A, exact.

OUT OF SCOPE, covered by their consumers' tests only: tri_mode 1 and 3, the sampling product and the tile cfgs 4 and 8;
tri_mode 4 (held entry by entry in test_gpu_fold_m_teams.py); batch mode; the epilogue hooks -- pair stores, column sums, row
sums and reducing epilogues.

Observed on an MI355X (256 CUs): all 21 listed variants hit, none out of reach, every exact pass bit for bit.  Per case
(shape as n x d of A, d x n of B, d x k x n of C; splits; tiles per split) the max |dev - ref| / allowed over its outputs
as float64 / longdouble, 1 allowed:
  A-dma-cfg7   70 x 208       1 split    14 tiles   0.000 / 0.059      A-reg-cfg3   70 x 200       8 tiles    0.000 / 0.053
  A-dma-cfg3   4102 x 208     1          260        0.000 / 0.043      A-reg-cfg2   15494 x 200    488        0.000 / 0.048
  A-dma-cfg2   15494 x 208    1          488        0.000 / 0.054      A-reg-cfg1   32646 x 200    512        0.000 / 0.068
  A-dma-cfg6   21766 x 272    1          513        0.000 / 0.030
    (0.000 is exactly 0: the device's G had numpy's bits in all seven cases -- with one split both kernels add the k terms
    of an element in index order with FMAs, as the host's BLAS evidently does at these K; the longdouble column shows what
    that common order costs, and B and C, whose sums are split, differ from numpy)
  B-dma-cfg3-xcd-1tile  64 x 2048    8 splits   1 tile     0.002 / 0.003
  B-dma-cfg3-xcd        100 x 2048   8          3          0.002 / 0.006
  B-dma-cfg3-empty      100 x 4624   18         3          0.001 / 0.001      (after B-dma-cfg2; split 17 starts at 4624)
  B-dma-cfg2            456 x 6400   25         20         0.001 / 0.001
  B-reg-cfg3-empty      100 x 4616   18         3          0.001 / 0.001      (after B-reg-cfg2)
  B-reg-cfg2            456 x 6536   25         20         0.001 / 0.001
  B-reg-cfg1            4040 x 264   1          528        0.013 / 0.067      (the 131 MB Gram matrix: 0.8 s, kept)
  B-dma-cfg3-1split     130 x 256    1          6          0.008 / 0.054
  C-dma-cfg6            1992 x 250 x 2048   8 splits   64 tiles   0.011 / 0.005      U reg cfg3, T'T dma cfg3
  C-dma-cfg2            1992 x 250 x 1024   4          128        0.015 / 0.011      U reg cfg3, T'T dma cfg3
  C-dma-cfg3-empty      70 x 5 x 8208       32         2          0.004 / 0.001      (after C-dma-cfg2)
  C-reg-cfg1            1992 x 250 x 2056   8          64         0.012 / 0.005      U reg cfg3, T'T reg cfg3
  C-reg-cfg3-empty      70 x 5 x 8200       32         2          0.004 / 0.001      (after C-reg-cfg1)
  C-reg-cfg3-1split     70 x 5 x 248        1          2          0.023 / 0.028
Wall time, references and both passes included: the slowest three are C-dma-cfg6 1.8 s, B-reg-cfg2 1.5 s and B-dma-cfg2
1.5 s; the module takes 13 s.
"""
import time

import numpy as np
import pytest

import _gemm_oracle as O

pytestmark = pytest.mark.gpu

SLOT_E, SLOT_Z = 40, 41


@pytest.fixture(scope='module')
def vb():
    import viabel_amd
    from viabel_amd import _lib
    _lib.default_engine()
    return viabel_amd


@pytest.fixture(scope='module')
def eng(vb):
    from viabel_amd import _lib
    return _lib.default_engine()


@pytest.fixture(scope='module')
def n_cu(eng):
    return eng.device_info()['cus']


def _run(vb, eng, case, kind):
    """``(device outputs, checks)`` of one case on ``kind`` inputs, outputs in the order of the checks."""
    p = O.PLAN[case.entry](*case.shape, eng.device_info()['cus'])
    if case.entry == 'A':
        n, d = case.shape
        P, mean, x = O.inputs_a(n, d, kind)
        model = vb.CorrelatedGaussianModel(mean, precision=P)
        assert np.array_equal(model.precision, P)

        def call():
            eng.set_model(model.device_spec())
            return [eng.model_grad(x)[1]]
        checks = O.checks_a(P, mean, x, p['bm_rows'])
    elif case.entry == 'B':
        d, n = case.shape
        E = O.inputs_b(d, n, kind)

        def call():
            eng.noise_set_host(SLOT_E, E)
            colsum, gram = eng.noise_moments(SLOT_E, n, d, want_gram=True)
            return [gram, colsum]
        checks = O.checks_b(E, p['splits'], p['bm_rows'])
    else:
        d, k, n = case.shape
        E, Z, sw = O.inputs_c(d, k, n, kind)

        def call():
            eng.noise_set_host(SLOT_E, E)
            eng.noise_set_host(SLOT_Z, Z)
            return list(eng.lowrank_path_terms(SLOT_E, SLOT_Z, n, d, k, sw))
        checks = O.checks_c(E, Z, sw, p['splits'], p['bm_rows'])
    return call, checks


def _assert_variant(case, n_cu):
    """Through vb_gemm_plan: the case takes the kernel, the tile and the split feature it is filed under."""
    p = O.PLAN[case.entry](*case.shape, n_cu)
    assert ('dma' if p['dma'] else 'reg', p['cfg']) == (case.kernel, case.cfg), (case, p)
    assert p['empty'] == (case.feature == 'empty'), (case, p)
    assert O.CLASSIFY[case.entry](*case.shape, n_cu) == case.variant, (case, p)
    return p


def _parity(vb, eng, case, n_cu):
    t0 = time.time()
    p = _assert_variant(case, n_cu)
    call, checks = _run(vb, eng, case, 'exact')
    O.assert_exact(*(c.bound for c in checks))
    for c, dev in zip(checks, call()):
        assert dev.shape == c.ref.shape and np.array_equal(dev, c.ref), '%s exact pass: %s differs in %d of %d elements' % (
            case.name, c.name, int(np.sum(dev != c.ref)), c.ref.size)
        if case.entry == 'B' and c.name == 'gram':
            assert np.array_equal(dev, dev.T)
    call, checks = _run(vb, eng, case, 'real')
    first, second = call(), call()
    worst = [0.0, 0.0]
    for c, dev, again in zip(checks, first, second):
        assert np.array_equal(dev, again), '%s real pass: %s differs between two calls' % (case.name, c.name)
        r = c.ratios(dev)
        worst = [max(worst[0], r[0]), max(worst[1], r[1])]
        assert r[0] <= 1.0 and r[1] <= 1.0, '%s real pass: %s at %.3g (float64) / %.3g (longdouble) of the bound' % (
            case.name, c.name, r[0], r[1])
    extra = ''
    if case.entry == 'C':
        extra = '  [U %s cfg%d, T\'T %s cfg%d]' % (O._kernel(p['u']), p['u']['cfg'], O._kernel(p['tt']), p['tt']['cfg'])
    print('%s: %d splits of %d, %d tiles; max |dev - ref| / allowed %.3g (float64) %.3g (longdouble); %.1f s%s'
          % (case.name, p['splits'], p['k_split'], p['grid_x'], worst[0], worst[1], time.time() - t0, extra))


def _case(variant, n_cu):
    for c in O.cases(variant[0], n_cu):
        if c.variant == variant:
            return c
    assert n_cu != 256, 'no case of %s on 256 compute units' % O.variant_name(variant)
    pytest.skip('%s: out of reach of the candidate shapes under the size cap on %d compute units'
                % (O.variant_name(variant), n_cu))


_PLAIN = [v for e in 'ABC' for v in O.VARIANTS[e] if v[3] != 'empty']
_EMPTY = [v for e in 'ABC' for v in O.VARIANTS[e] if v[3] == 'empty']


@pytest.mark.parametrize('variant', _PLAIN, ids=O.variant_name)
def test_parity(vb, eng, n_cu, variant):
    _parity(vb, eng, _case(variant, n_cu), n_cu)


@pytest.mark.parametrize('variant', _EMPTY, ids=O.variant_name)
def test_empty_trailing_split_after_a_larger_case(vb, eng, n_cu, variant):
    """The larger case of the same entry and kernel first -- its slabs of the real pass stay in the workspace, and it has more
    of them, each larger -- then the whole parity of the case whose last split has no k range."""
    entry, kernel = variant[:2]
    larger = {('B', 'dma'): ('B', 'dma', 2, ''), ('B', 'reg'): ('B', 'reg', 2, ''), ('C', 'dma'): ('C', 'dma', 2, ''),
              ('C', 'reg'): ('C', 'reg', 1, '')}[entry, kernel]
    case, big = _case(variant, n_cu), _case(larger, n_cu)
    p, pb = O.PLAN[entry](*case.shape, n_cu), O.PLAN[entry](*big.shape, n_cu)
    assert p['empty'] and not pb['empty']
    slab = {'B': lambda s: s[0] * O._round16(s[0]), 'C': lambda s: s[0] * max(32, O._round16(2 * s[1]))}[entry]
    assert pb['splits'] * slab(big.shape) >= p['splits'] * slab(case.shape)         # the stale data covers every slab
    call, _ = _run(vb, eng, big, 'real')
    assert all(np.all(np.isfinite(out)) and np.any(out != 0) for out in call())
    _parity(vb, eng, case, n_cu)


def test_variant_coverage(n_cu):
    """The union of the cases above holds every listed variant; on 256 compute units none is out of reach."""
    hit = set()
    for entry in 'ABC':
        for case in O.cases(entry, n_cu):
            _assert_variant(case, n_cu)
            hit.add(case.variant)
    missing = [v for e in 'ABC' for v in O.missing(e, n_cu)]
    listed = {v for e in 'ABC' for v in O.VARIANTS[e]}
    print('%d compute units: hit %s; out of reach %s' % (n_cu, ', '.join(sorted(map(O.variant_name, hit))),
                                                          ', '.join(map(O.variant_name, missing)) or 'none'))
    assert hit | set(missing) == listed and not hit & set(missing)
    if n_cu == 256:
        assert missing == [] and hit == listed
    assert set(_PLAIN) | set(_EMPTY) == listed


@pytest.mark.parametrize('d', O.EDGE_D)
def test_edges_of_m_and_n(vb, eng, n_cu, d):
    rng = np.random.RandomState(d)
    P = O.int_precision(rng, d)
    model = vb.CorrelatedGaussianModel(np.zeros(d), precision=P)
    for n in O.EDGE_N:
        p = O.plan_a(n, d, n_cu)
        assert (p['dma'], p['cfg']) == ((True, 7) if d % 16 == 0 else (False, 3)), (n, d, p)
        x = O.int_matrix(rng, n, d)
        O.assert_exact(np.abs(x) @ np.abs(P))
        eng.set_model(model.device_spec())
        g = eng.model_grad(x)[1]
        assert g.shape == (n, d) and np.array_equal(g, -(x @ P)), (n, d)
