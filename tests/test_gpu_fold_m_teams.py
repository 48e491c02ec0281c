"""GPU: M = L' P of the folded full-rank evaluation, formed by two four-wave teams per workgroup on paired 64-row blocks
(gemm_f64_dma_team_pair_tiles in fr_fold_msum_team_kernel: every shape with fewer than two such workgroups per CU), read back with Engine.fullrank_fold_m and compared entry by entry.

Shapes, the smallest the gate admits, each with N = 3 D + 48:
  D = 1024: 16 row blocks, eight pairs, every tile whole;
  D = 1040: 17 row blocks -- the middle one is split between the teams, the last has 16 rows (one slab: team 0 changes
            tiles after its first slab) and the last column tile is 16 wide;
  D = 1088: 17 whole row blocks and 34 column tiles.

Bound.  Entry (i, j) of M is a sum of at most D products, on the device in two parts that are added at the end; for either
order of summation |fl(sum) - sum| <= gamma_D (|L'| |P|)_ij with gamma_D ~ D 2^-53, so the device and numpy's L.T @ P may
differ by 4 D 2^-53 (|L'| |P|)_ij: gamma_D for each of the two sums, doubled for the regrouping.  (numpy's product alone
against an 80-bit product, every sixteenth row at D = 1024: at most 0.0028 of that bound.)"""
import functools

import numpy as np
import pytest

from test_gpu_fullrank_fold import _check_oracle, _evaluate, _problem, _theta_b

pytestmark = pytest.mark.gpu

SHAPES = [1024, 1040, 1088]


def _rows(D):
    from viabel_amd import _lib
    N = 3 * D + 48
    assert D >= _lib.FR_FOLD_MIN_D and N >= _lib.FR_FOLD_MIN_ROWS_PER_D * D      # inside the fold gate
    return N


def _reference(vb, model, theta, D):
    """numpy's M = L' P and the bound on an entry's difference."""
    _, L = vb.FullRankGaussian(D)._unpack(theta)
    P = model.precision
    return L.T @ P, 4.0 * D * 2.0 ** -53 * (np.abs(L.T) @ np.abs(P))


@functools.lru_cache(maxsize=None)
def _case(D):
    """One folded evaluation of _problem(D) on the default engine: (value, grad), M, launches of the sampling product,
    the noise, and the problem."""
    from viabel_amd import _lib
    vb, model, theta = _problem(D)
    eng = _lib.default_engine()
    out, launches, noise = _evaluate(eng, model, theta, D, _rows(D))
    M = eng.fullrank_fold_m(D)
    return out, M, launches, noise, (vb, model, theta)


@pytest.mark.parametrize('D', SHAPES)
def test_m_entry_by_entry(D):
    out, M, launches, _, (vb, model, theta) = _case(D)
    assert launches == 0                       # the folded route ran
    want, bound = _reference(vb, model, theta, D)
    assert M.shape == want.shape and np.all(np.isfinite(M))
    ratio = np.abs(M - want) / bound           # (every entry of |L'| |P| is positive: P is dense)
    i, j = np.unravel_index(np.argmax(ratio), ratio.shape)
    print('D=%d: largest |M - L.T @ P| / bound %.3g at (%d, %d); largest |M - L.T @ P| %.3g'
          % (D, ratio[i, j], i, j, np.max(np.abs(M - want))))
    assert np.all(bound > 0.0)
    assert np.all(ratio <= 1.0)


def test_evaluation_against_the_oracle_at_17_whole_row_blocks():
    """D = 1088: value 1e-12 relative, gradient 1e-11 of its largest entry."""
    D = 1088
    out, _, launches, noise, (_, model, theta) = _case(D)
    assert launches == 0
    _check_oracle(out, model, theta, noise, D)


def test_same_inputs_same_bits_and_m_follows_the_parameter():
    """D = 1040 (the split middle block): twice the same inputs, then another parameter through fullrank_set_theta."""
    from viabel_amd import _lib
    D = 1040
    N = _rows(D)
    (v0, g0), M0, _, _, (vb, model, theta) = _case(D)
    eng = _lib.default_engine()
    (v1, g1), launches, _ = _evaluate(eng, model, theta, D, N)
    M1 = eng.fullrank_fold_m(D)
    assert launches == 0
    assert v1 == v0
    np.testing.assert_array_equal(g1, g0)
    np.testing.assert_array_equal(M1, M0)

    theta_b = _theta_b(vb, D)
    eng.fullrank_set_theta(theta_b, D)
    eng.elbo_grad_fullrank_enqueue(3, N, D)
    eng.fullrank_get(D)
    Mb = eng.fullrank_fold_m(D)
    want, bound = _reference(vb, model, theta_b, D)
    assert np.all(np.abs(Mb - want) <= bound)
    assert np.max(np.abs(Mb - M0)) > 1e3 * np.max(bound)      # (not the M of the first parameter)


def test_no_m_without_a_folded_evaluation():
    """Below the gate the sampling product runs: the getter reports that there is no M."""
    from viabel_amd import _lib
    D = 512
    vb, model, theta = _problem(D)
    eng = _lib.default_engine()
    _, launches, _ = _evaluate(eng, model, theta, D, 2048)
    assert launches == 1
    with pytest.raises(_lib.EngineError) as err:
        eng.fullrank_fold_m(D)
    assert 'folded' in str(err.value)
