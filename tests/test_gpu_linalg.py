"""GPU: the Newton-Schulz symmetric square root / Sylvester solve (vb_sym_sqrt) against LAPACK.

`scipy.linalg.sqrtm(Sigma)` is what MultivariateT.sample takes (approximations.py:348); the eigen-decomposition
gives the same matrix and, for the derivative, the closed form X~_ij = E~_ij / (r_i + r_j) in the eigenbasis.

The second half holds the three host entries (`Engine.sym_sqrt(a)`, `sym_sqrt(a, e)`, `sym_sqrt_inv(a)`) to a 50-digit
truth (tests/_linalg_oracle.py) instead of eigh, which is itself off by cond * eps.  The yardstick is the error of the eigh
route -- what objectives.py falls back to -- against the same truth; "accepted" means info[2] < objectives._ROOT_TOL.
Every margin asserted below is four times the largest ratio measured on an MI355X, rounded up to a power of two (the
factor four: GEMM tile choices depend on the CU count, and other LAPACK builds move the yardstick):

  forward error, err_dev / max(err_eigh, 8 eps sqrt(d)), largest over the accepted cases of O.CASES
      R 2.223 (d 8, cond 1e8, with e)   -> 16      X 3.274 (d 17, cond 1e4) -> 16      Z 1.718 (d 33, cond 1e8) -> 8
      (at cond 1e8: X 1.2e-9 / 5.7e-10 / 9.4e-10 against eigh's 5.9e-10 / 4.5e-10 / 3.6e-10 at d 8 / 17 / 33)
  info[2]: (true - d eps) / info[2], true = ||R R - a_s||_F / c in longdouble, every case: 0.982 -> 4
  edges (cond 1e3), residual of the device / the same residual of the eigh route, normalised as in the oracle:
      R R - a 1.514 -> 8      Z R - I 0.650 -> 4      Z a Z - I 1.044 -> 8      R X + X R - e 57.65 -> 256
      The last one is the method, not the kernels: the numpy model of the iteration gives 44-55 on the same inputs.  The
      iteration is forward stable (X as accurate as eigh's, see above) but not backward stable, and eigh's X satisfies
      the equation to 1.4e-16 where its own forward error is 1e-14.

Where the entries stop accepting: the geometric spectra are accepted at every condition number of O.CASES (info[2]
6e-13 at 1e9); two equal clusters and one small eigenvalue at cond 1e8 are declined (info[2] 2.4e-12 and 1.4e-12, with
forward errors still below eigh's).  No accepted case comes near the 32x at which the gates would need tightening."""
import functools

import numpy as np
import pytest

import _linalg_oracle as O

pytestmark = pytest.mark.gpu


def _spd(d, cond, seed):
    rng = np.random.RandomState(seed)
    Q, _ = np.linalg.qr(rng.randn(d, d))
    ev = np.exp(np.linspace(0.0, np.log(cond), d)) * 0.37
    return (Q * ev) @ Q.T


def _reference(a, e=None):
    w, U = np.linalg.eigh(a)
    r = np.sqrt(w)
    root = (U * r) @ U.T
    if e is None:
        return root, None
    x = U @ ((U.T @ e @ U) / (r[:, None] + r[None, :])) @ U.T
    return root, x


@pytest.mark.parametrize('d,cond', [(1, 1.0), (5, 10.0), (64, 1e3), (130, 1e4), (256, 1e2), (256, 1e6), (300, 1e8)])
def test_symmetric_root_matches_eigh(d, cond):
    from viabel_amd import _lib
    eng = _lib.default_engine()
    a = _spd(d, cond, d)
    root, x, info = eng.sym_sqrt(a)
    want, _ = _reference(a)
    assert x is None
    np.testing.assert_array_equal(root, root.T)
    scale = np.linalg.norm(want)
    # forward error and residual grow (mildly) with sqrt(cond)
    assert np.linalg.norm(root - want) / scale < 2e-15 * max(10.0, np.sqrt(cond)) * np.sqrt(d)
    resid_tol = max(5e-14, 3e-16 * np.sqrt(cond * d))
    assert np.linalg.norm(root @ root - a) / np.linalg.norm(a) < resid_tol
    assert info[2] < resid_tol and 0 <= info[0] < 60


@pytest.mark.parametrize('d,cond', [(3, 5.0), (40, 1e2), (128, 1e4), (256, 1e3)])
def test_root_derivative_solves_the_sylvester_equation(d, cond):
    from viabel_amd import _lib
    eng = _lib.default_engine()
    a = _spd(d, cond, 100 + d)
    rng = np.random.RandomState(d)
    e = rng.randn(d, d)
    e = 0.5 * (e + e.T) * 37.0
    root, x, info = eng.sym_sqrt(a, e)
    want_root, want_x = _reference(a, e)
    np.testing.assert_allclose(root, want_root, rtol=0, atol=1e-13 * np.linalg.norm(want_root))
    np.testing.assert_allclose(x, want_x, rtol=0, atol=1e-11 * np.linalg.norm(want_x))
    resid = root @ x + x @ root - e
    assert np.linalg.norm(resid) / np.linalg.norm(e) < 1e-11
    # general (non-symmetric) directions work as well: the equation is linear
    e2 = rng.randn(d, d)
    _, x2, _ = eng.sym_sqrt(a, e2)
    assert np.linalg.norm(want_root @ x2 + x2 @ want_root - e2) / np.linalg.norm(e2) < 1e-11


def test_sym_sqrt_errors():
    from viabel_amd import _lib
    eng = _lib.default_engine()
    with pytest.raises(Exception):
        eng.sym_sqrt(np.zeros((4, 4)))
    root, _, info = eng.sym_sqrt(np.diag([4.0, 9.0, 16.0]))
    np.testing.assert_allclose(root, np.diag([2.0, 3.0, 4.0]), atol=1e-14)


# ---- against the exact truth (tests/_linalg_oracle.py) --------------------------------------------------------------
# Asserted margins: four times the largest ratio measured on the MI355X (module docstring), rounded up to a power of two.
MARGIN_FORWARD = {'R': 16.0, 'X': 16.0, 'Z': 8.0}                    # measured 2.223, 3.274, 1.718
MARGIN_INFO2 = 4.0                                                    # measured 0.982
MARGIN_EDGE = {'rr': 8.0, 'zr': 4.0, 'zaz': 8.0, 'sylv': 256.0}      # measured 1.514, 0.650, 1.044, 57.65
EDGE_COND = 1e3
EDGE_ROOT_DIMS = (15, 31, 63, 64, 65, 127, 128, 129)
EDGE_SYLVESTER_DIMS = (31, 32, 33, 63, 64, 65)
_CASE_IDS = [O.case_id(c) for c in O.CASES]


def _engine():
    from viabel_amd import _lib
    return _lib.default_engine()


def _declined():
    """How the entry declines: Engine._check raises ValueError for the C side's numeric refusals ('iteration diverged',
    'zero or non-finite matrix') and EngineError for its other error codes."""
    from viabel_amd import _lib
    return (ValueError, _lib.EngineError)


def _accepted(info):
    from viabel_amd import objectives
    return bool(info[2] < objectives._ROOT_TOL)


def _call(fn, *args):
    """The entry's result, or None when it declined by raising."""
    try:
        return fn(*args)
    except _declined():
        return None


@functools.lru_cache(maxsize=None)
def _device(case):
    """The three entries on one case, once: {'root': (R, None, info), 'sylvester': (R, X, info), 'inverse': (R, Z, info)}."""
    eng, t = _engine(), O.truth(case)
    return {'root': _call(eng.sym_sqrt, t.a), 'sylvester': _call(eng.sym_sqrt, t.a, t.e),
            'inverse': _call(eng.sym_sqrt_inv, t.a)}


def forward_ratios(case):
    """[(entry, quantity, accepted, err_dev, err_lapack, ratio)] with ratio = err_dev / max(err_lapack, 8 eps sqrt(d)); the
    errors are relative Frobenius errors against the 50-digit truth.  Checks conditions (a) and (b) on the way."""
    t, rows = O.truth(case), []
    floor = 8 * O.EPS * np.sqrt(case.d)
    for entry, out in _device(case).items():
        if out is None:
            assert case.cond > 1e6, '(b) %s declined %s by raising' % (entry, O.case_id(case))
            continue
        root, second, info = out
        assert np.all(np.isfinite(root)) and np.all(np.isfinite(info)), '(a) %s returned a non-finite root' % entry
        assert second is None or np.all(np.isfinite(second)), '(a) %s returned a non-finite matrix' % entry
        assert case.cond > 1e6 or _accepted(info), '(b) %s: info[2] = %.2e at cond %.0e' % (entry, info[2], case.cond)
        got = [('R', root, t.R, t.lapack_R)]
        if entry == 'sylvester':
            got.append(('X', second, t.X, t.lapack_X))
        if entry == 'inverse':
            got.append(('Z', second, t.Z, t.lapack_Z))
        for name, dev, want, lap in got:
            err_dev, err_lap = O.rel_err(dev, want), O.rel_err(lap, want)
            rows.append((entry, name, _accepted(info), err_dev, err_lap, err_dev / max(err_lap, floor)))
    return rows


@pytest.mark.parametrize('case', O.CASES, ids=_CASE_IDS)
def test_forward_error_against_the_exact_truth(case):
    rows = forward_ratios(case)
    for entry, name, accepted, err_dev, err_lap, ratio in rows:
        print('%s %s %s: accepted %d  device %.2e  eigh %.2e  ratio %.2f' % (O.case_id(case), entry, name, accepted, err_dev,
                                                                              err_lap, ratio))
    for entry, name, accepted, err_dev, err_lap, ratio in rows:
        if accepted:
            assert ratio <= MARGIN_FORWARD[name], (entry, name, err_dev, err_lap, ratio)


def _skewed_case():
    """A non-symmetric input: info[2] refers to its symmetric part, which is what the entry roots."""
    t = O.truth(O.CASES[6])
    s = 1e-2 * np.random.RandomState(9).randn(*t.a.shape)
    return t.a + (s - s.T), t.e


def info2_ratios(a, e):
    """[(entry, info[2], true, (true - d eps) / info[2])] over the entries that returned; true = ||R R - a_s||_F / c in longdouble."""
    eng, d = _engine(), a.shape[0]
    a_s = 0.5 * (a + a.T)
    rows = []
    for entry, out in (('root', _call(eng.sym_sqrt, a)), ('sylvester', _call(eng.sym_sqrt, a, e)),
                       ('inverse', _call(eng.sym_sqrt_inv, a))):
        if out is None:
            continue
        true = O.residuals_ld(a_s, out[0])['info2']
        excess = true - d * O.EPS
        rows.append((entry, float(out[2][2]), true, excess / out[2][2] if excess > 0 else 0.0))
    return rows


@pytest.mark.parametrize('case', O.CASES + ['skewed'], ids=_CASE_IDS + ['skewed'])
def test_info2_does_not_understate_the_residual_of_the_returned_root(case):
    a, e = _skewed_case() if case == 'skewed' else O.truth(case)[:2]
    rows = info2_ratios(a, e)
    for entry, claimed, true, ratio in rows:
        print('%s %s: info[2] %.2e  true %.2e  (true - d eps) / info[2] %.2f' % (case if case == 'skewed' else O.case_id(case),
                                                                              entry, claimed, true, ratio))
    for entry, claimed, true, ratio in rows:
        assert true <= MARGIN_INFO2 * claimed + a.shape[0] * O.EPS, (entry, claimed, true)


@functools.lru_cache(maxsize=None)
def _edge_inputs(d):
    a, e = O.spd('geometric', d, EDGE_COND, d), O.direction(d, d)
    for m in (a, e):
        m.setflags(write=False)
    return a, e, O.lapack(a, e)


def edge_ratios(d, sylvester):
    """{residual: (device, eigh route, ratio)} in longdouble at a size on the edge of the 16-column padding / the 64-wide tile."""
    eng = _engine()
    a, e, (lap_R, lap_Z, lap_X) = _edge_inputs(d)
    if sylvester:
        root, x, info = eng.sym_sqrt(a, e)
        dev, lap = O.residuals_ld(a, root, None, x, e), O.residuals_ld(a, lap_R, None, lap_X, e)
        np.testing.assert_array_equal(root, root.T)
    else:
        root, z, info = eng.sym_sqrt_inv(a)
        dev, lap = O.residuals_ld(a, root, z), O.residuals_ld(a, lap_R, lap_Z)
        np.testing.assert_array_equal(root, root.T)
        np.testing.assert_array_equal(z, z.T)
    assert _accepted(info), info
    return {k: (dev[k], lap[k], dev[k] / lap[k]) for k in dev if k != 'info2'}


@pytest.mark.parametrize('d,sylvester', [(d, False) for d in EDGE_ROOT_DIMS] + [(d, True) for d in EDGE_SYLVESTER_DIMS])
def test_residuals_at_the_edges_of_padding_and_tile(d, sylvester):
    rows = edge_ratios(d, sylvester)
    for name, (dev, lap, ratio) in rows.items():
        print('d %d %s %s: device %.2e  eigh %.2e  ratio %.2f' % (d, 'sylvester' if sylvester else 'inverse', name, dev, lap, ratio))
    for name, (dev, lap, ratio) in rows.items():
        assert dev <= MARGIN_EDGE[name] * lap, (name, dev, lap)


# ---- exact properties -----------------------------------------------------------------------------------------------
_EXACT_CASES = [O.CASES[4], O.CASES[6], O.CASES[15]]      # d = 9, 17 at cond 1e2 and d = 8 at cond 1e6
_EXACT_IDS = [O.case_id(c) for c in _EXACT_CASES]


@pytest.mark.parametrize('case', _EXACT_CASES, ids=_EXACT_IDS)
def test_scaling_by_powers_of_two_is_exact(case):
    eng, t = _engine(), O.truth(case)
    root, x, _ = eng.sym_sqrt(t.a, t.e)
    plain, _, _ = eng.sym_sqrt(t.a)
    _, z, _ = eng.sym_sqrt_inv(t.a)
    for k in (-50, 50):
        np.testing.assert_array_equal(eng.sym_sqrt(4.0 ** k * t.a)[0], 2.0 ** k * plain)
        np.testing.assert_array_equal(eng.sym_sqrt_inv(4.0 ** k * t.a)[1], 2.0 ** -k * z)
    for j in (-31, 31):
        root_j, x_j, _ = eng.sym_sqrt(t.a, 2.0 ** j * t.e)
        np.testing.assert_array_equal(root_j, root)
        np.testing.assert_array_equal(x_j, 2.0 ** j * x)


@pytest.mark.parametrize('case', _EXACT_CASES, ids=_EXACT_IDS)
def test_zero_direction_gives_exactly_zero(case):
    eng, t = _engine(), O.truth(case)
    root, x, info = eng.sym_sqrt(t.a, np.zeros_like(t.a))
    np.testing.assert_array_equal(x, np.zeros_like(t.a))
    assert _accepted(info)
    assert O.rel_err(root, t.R) <= MARGIN_FORWARD['R'] * max(O.rel_err(t.lapack_R, t.R), 8 * O.EPS * np.sqrt(case.d))


@pytest.mark.parametrize('case', _EXACT_CASES, ids=_EXACT_IDS)
def test_the_same_call_twice_returns_the_same_bits(case):
    eng, t = _engine(), O.truth(case)
    for fn, args in ((eng.sym_sqrt, (t.a,)), (eng.sym_sqrt, (t.a, t.e)), (eng.sym_sqrt_inv, (t.a,))):
        first, second = fn(*args), fn(*args)
        for p, q in zip(first, second):
            assert (p is None and q is None) or np.array_equal(p, q)


@pytest.mark.parametrize('case', _EXACT_CASES, ids=_EXACT_IDS)
def test_a_skew_symmetric_part_is_ignored_bit_for_bit(case):
    eng, t = _engine(), O.truth(case)
    a = np.round(t.a * 2.0 ** 20) / 2.0 ** 20                     # few mantissa bits: a + s and a - s are exact
    s = np.triu(np.random.RandomState(5).randint(-8, 9, a.shape), 1) * 2.0 ** -6
    skewed = a + s - s.T
    assert not np.array_equal(skewed, skewed.T)
    np.testing.assert_array_equal(0.5 * (skewed + skewed.T), a)
    for fn, args in ((eng.sym_sqrt, ()), (eng.sym_sqrt, (t.e,)), (eng.sym_sqrt_inv, ())):
        want, got = fn(a, *args), fn(skewed, *args)
        assert _accepted(want[2])
        for p, q in zip(want, got):
            assert (p is None and q is None) or np.array_equal(p, q)


# ---- rejections -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lowest', [-0.1, -1e-9])
@pytest.mark.parametrize('entry', ['root', 'sylvester', 'inverse'])
def test_a_matrix_that_is_not_positive_definite_never_looks_accepted(lowest, entry):
    eng, d = _engine(), 12
    rng = np.random.RandomState(3)
    Q, _ = np.linalg.qr(rng.randn(d, d))
    w = np.linspace(0.5, 2.0, d)
    w[0] = lowest
    a = (Q * w) @ Q.T
    a = 0.5 * (a + a.T)
    assert np.linalg.eigvalsh(a)[0] < 0.5 * lowest
    try:
        out = {'root': lambda: eng.sym_sqrt(a), 'sylvester': lambda: eng.sym_sqrt(a, O.direction(d, 1)),
               'inverse': lambda: eng.sym_sqrt_inv(a)}[entry]()
    except _declined():
        return
    print('lowest eigenvalue %g, %s: returned with info %s' % (lowest, entry, out[2]))
    assert not _accepted(out[2])


@pytest.mark.parametrize('bad', [np.nan, np.inf, -np.inf])
def test_non_finite_entries_raise(bad):
    eng, t = _engine(), O.truth(O.CASES[4])
    a = t.a.copy()
    a[2, 5] = a[5, 2] = bad
    e = t.e.copy()
    e[1, 3] = bad
    for fn, args in ((eng.sym_sqrt, (a,)), (eng.sym_sqrt, (a, t.e)), (eng.sym_sqrt_inv, (a,)), (eng.sym_sqrt, (t.a, e))):
        with pytest.raises(_declined()):
            fn(*args)


def test_wrong_shapes_raise_before_any_native_call(monkeypatch):
    eng = _engine()
    called = []

    class _Native:      # stands in for the loaded library: any entry reached counts as a native call
        def __getattr__(self, name):
            called.append(name)
            raise AssertionError('native entry %s reached' % name)

    good = O.truth(O.CASES[4]).a
    monkeypatch.setattr(eng, '_lib', _Native())
    for a in (np.ones((3, 4)), np.ones((4, 3)), np.ones(9), np.ones((2, 2, 2)), np.ones((0, 0)), np.float64(4.0)):
        with pytest.raises(ValueError):
            eng.sym_sqrt(a)
        with pytest.raises(ValueError):
            eng.sym_sqrt_inv(a)
    for e in (np.ones((8, 8)), np.ones((9, 8)), np.ones(81), np.ones((9, 9, 1))):
        with pytest.raises(ValueError):
            eng.sym_sqrt(good, e)
    assert called == []
