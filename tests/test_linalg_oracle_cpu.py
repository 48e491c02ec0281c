"""The references of the matrix-root tests (tests/_linalg_oracle.py) checked on their own, without a GPU: the 50-digit
truth against the defining equations in longdouble, LAPACK's distance from it (the yardstick of tests/test_gpu_linalg.py),
and the numpy model of the host entry's control -- that it reaches the accuracy the GPU tests demand of every case up to
condition number 1e6, and that it is exact under scaling by powers of two."""
import numpy as np
import pytest

import _linalg_oracle as O

_IDS = [O.case_id(c) for c in O.CASES]


def test_case_list_is_what_the_gpu_tests_rely_on():
    assert len(set(O.CASES)) == len(O.CASES) == 28
    assert {c.d for c in O.CASES if c.cond == 1e2} == {1, 2, 7, 8, 9, 16, 17, 32, 33}
    for cond in (1.0, 1e4, 1e6, 1e8, 1e9):
        assert {c.d for c in O.CASES if c.cond == cond and c.spectrum == 'geometric'} == {8, 17, 33}
    assert {c.spectrum for c in O.CASES} == {'geometric', 'two_clusters', 'one_small', 'identity_multiple', 'diagonal'}
    for c in O.CASES:
        t = O.truth(c)
        assert np.array_equal(t.a, t.a.T)
        assert np.array_equal(t.e, t.e.T) == (c.seed % 2 == 0 or c.d == 1)
        w = np.linalg.eigvalsh(t.a)
        assert w[0] > 0 and abs(np.log10(w[-1] / w[0]) - np.log10(c.cond if c.d > 1 else 1.0)) < 1e-3


@pytest.mark.parametrize('case', O.CASES, ids=_IDS)
def test_exact_matrices_satisfy_their_equations_to_the_longdouble_floor(case):
    t = O.truth(case)
    R, Z, X = O.exact(t.a, t.e, dtype=O.LD)
    res = O.residuals_ld(t.a, R, Z, X, t.e)
    print(O.case_id(case), {k: '%.1e' % v for k, v in res.items()})
    for name in ('rr', 'zr', 'zaz', 'sylv'):
        assert res[name] < 1e-17, (name, res)
    # the double-rounded matrices every other test compares with are these, rounded once more (double rounding: 1 ulp)
    for q, q_ld in ((t.R, R), (t.Z, Z), (t.X, X)):
        assert np.all(np.abs(q - q_ld.astype(np.float64)) <= np.spacing(np.abs(q)))


@pytest.mark.parametrize('case', O.CASES, ids=_IDS)
def test_lapack_errors_against_the_truth_are_finite(case):
    t = O.truth(case)
    errs = [O.rel_err(got, want) for got, want in ((t.lapack_R, t.R), (t.lapack_Z, t.Z), (t.lapack_X, t.X))]
    print('%s: eigh route against the 50-digit truth: R %.1e Z %.1e X %.1e' % ((O.case_id(case),) + tuple(errs)))
    assert np.all(np.isfinite(errs))
    # a loose sanity bound on the yardstick itself: eigh is backward stable, so its forward error is of order cond * eps
    assert max(errs) < 64 * case.d * O.EPS * max(case.cond, 1.0)


@pytest.mark.parametrize('case', [c for c in O.CASES if c.cond <= 1e6], ids=[O.case_id(c) for c in O.CASES if c.cond <= 1e6])
@pytest.mark.parametrize('with_e', [False, True], ids=['root', 'sylvester'])
def test_model_of_the_control_resolves_every_case_up_to_cond_1e6(case, with_e):
    t = O.truth(case)
    out = O.model(t.a, t.e if with_e else None)
    print(O.case_id(case), 'steps %d acc %.1e' % (out['steps'], out['acc']))
    assert out['acc'] < 1e-13 and out['steps'] < 60
    assert O.rel_err(out['R'], t.R) < 1e-10 and O.rel_err(out['Z'], t.Z) < 1e-8      # (it is the root, not only a fixed point)
    if with_e:
        assert O.rel_err(out['X'], t.X) < 1e-8


@pytest.mark.parametrize('case', [c for c in O.CASES if c.d in (9, 17, 24)], ids=[O.case_id(c) for c in O.CASES if c.d in (9, 17, 24)])
def test_model_is_bit_exact_under_power_of_two_scaling(case):
    t = O.truth(case)
    base = O.model(t.a, t.e)
    for k in (-50, -1, 3, 50):
        scaled = O.model(4.0 ** k * t.a, t.e)
        assert scaled['steps'] == base['steps']
        np.testing.assert_array_equal(scaled['R'], 2.0 ** k * base['R'])
        np.testing.assert_array_equal(scaled['Z'], 2.0 ** -k * base['Z'])
        np.testing.assert_array_equal(scaled['X'], 2.0 ** -k * base['X'])      # R X + X R = E: X scales with 1 / R
    for j in (-31, 1, 31):
        scaled = O.model(t.a, 2.0 ** j * t.e)
        np.testing.assert_array_equal(scaled['R'], base['R'])
        np.testing.assert_array_equal(scaled['X'], 2.0 ** j * base['X'])


def test_model_roots_the_symmetric_part_and_zero_direction_gives_zero():
    t = O.truth(O.CASES[4])
    a = np.round(t.a * 2.0 ** 20) / 2.0 ** 20                     # few mantissa bits: a + s and a - s are exact
    s = np.triu(np.random.RandomState(5).randint(-8, 9, a.shape), 1) / 2.0 ** 20
    np.testing.assert_array_equal(0.5 * ((a + s - s.T) + (a + s - s.T).T), a)
    base, skewed = O.model(a, t.e), O.model(a + s - s.T, t.e)
    for name in ('R', 'Z', 'X'):
        np.testing.assert_array_equal(skewed[name], base[name])
    zero = O.model(a, np.zeros_like(a))
    np.testing.assert_array_equal(zero['X'], np.zeros_like(a))
    assert O.rel_err(zero['R'], O.model(a)['R']) < 64 * O.EPS
