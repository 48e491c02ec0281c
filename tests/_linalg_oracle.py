"""Exact references for the device matrix root (``vb_sym_sqrt`` / ``vb_sym_sqrt_inv``, viabel_amd/csrc/vb_linalg.hip).

TEST INFRASTRUCTURE ONLY; host only (numpy and mpmath, no engine).  For a symmetric positive definite ``a`` and a direction
``e`` the three matrices the device entry returns are

    R = a^(1/2),      Z = a^(-1/2),      X with R X + X R = e   (the root's Frechet derivative in direction e).

* ``exact``        50-digit eigen-decomposition (``mpmath.eigsy``) of the DOUBLE matrix as given, rounded once at the end:
                   the truth every forward error below refers to.  ``numpy.linalg.eigh`` is not that: at condition number
                   1e8 its root is off by ~1e-13 and its X and Z by ~6e-10, relative.
* ``lapack``       the same three matrices by ``numpy.linalg.eigh`` -- the route objectives.py takes when it does not trust
                   the device result.  Its error against ``exact`` is the yardstick the device is held to.
* ``residuals_ld`` how well R, Z, X satisfy their defining equations, evaluated in ``numpy.longdouble`` (64-bit mantissa).
* ``model``        a plain-numpy model of the host entry's CONTROL (scale, block matrix, groups of steps, stopping rules),
                   with numpy's matmul in place of the MFMA GEMMs.  It says nothing about the kernels; it shows that what
                   the GPU tests demand of the control can be met at all, and that the control is exact under scaling by
                   powers of two.

Normalisation of the residuals.  Each is a Frobenius norm over the norms of the factors that form it,

    rr   = ||R R - a|| / ||a||                  zr   = ||Z R - I|| / (||Z|| ||R||)
    zaz  = ||Z a Z - I|| / (||Z||^2 ||a||)      sylv = ||R X + X R - e|| / (2 ||R|| ||X|| + ||e||)

because only then is there a floor that does not depend on the condition number: rounding Z to ANY format with unit
roundoff u moves ``Z R - I`` by u ||Z|| ||R|| = u sqrt(cond) relative to ||I||, so relative to the right-hand side alone not
even the exactly rounded truth would reach a fixed bound.  With the factors' norms underneath the longdouble-rounded
truth sits at a few u_ld ~ 1e-19 for every case (tests/test_linalg_oracle_cpu.py asserts 1e-17).
"""
import collections
import functools

import mpmath
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, 'numpy.longdouble must carry a 64-bit mantissa here (x87 extended)'
EPS = float(np.finfo(np.float64).eps)
_DPS = 50

# ------------------------------------------------------------------------------------------------ generators
Case = collections.namedtuple('Case', 'spectrum d cond seed')


def geometric(d, cond):
    return np.exp(np.linspace(0.0, np.log(cond), d))


def two_clusters(d, cond):
    return np.where(np.arange(d) < d // 2, 1.0, float(cond))


def one_small(d, cond):
    w = np.ones(d)
    w[0] = 1.0 / cond
    return w


_SPECTRA = {'geometric': geometric, 'two_clusters': two_clusters, 'one_small': one_small}


def spd(spectrum, d, cond, seed):
    """``A = Q diag(0.37 w) Q'``, symmetrised, Q from a seeded QR; ``identity_multiple``: 0.37 I exactly; ``diagonal``: the
    geometric spectrum on the diagonal (shuffled), exactly diagonal."""
    rng = np.random.RandomState(1000 + seed)
    if spectrum == 'identity_multiple':
        return 0.37 * np.eye(d)
    if spectrum == 'diagonal':
        return np.diag(0.37 * rng.permutation(geometric(d, cond)))
    Q, _ = np.linalg.qr(rng.randn(d, d))
    a = (Q * (0.37 * _SPECTRA[spectrum](d, cond))) @ Q.T
    return 0.5 * (a + a.T)


def direction(d, seed):
    """The right-hand side E: symmetric for even seeds, general for odd ones."""
    e = 37.0 * np.random.RandomState(2000 + seed).randn(d, d)
    return 0.5 * (e + e.T) if seed % 2 == 0 else e


def _cases():
    out = [('geometric', d, 1e2) for d in (1, 2, 7, 8, 9, 16, 17, 32, 33)]
    out += [('geometric', d, cond) for cond in (1.0, 1e4, 1e6, 1e8, 1e9) for d in (8, 17, 33)]
    out += [('two_clusters', 24, 1e8), ('one_small', 24, 1e8), ('identity_multiple', 9, 1.0), ('diagonal', 17, 1e4)]
    return [Case(s, d, cond, seed) for seed, (s, d, cond) in enumerate(out)]


CASES = _cases()


def case_id(case):
    return '%s-d%d-cond%.0e-%s' % (case.spectrum, case.d, case.cond, 'sym' if case.seed % 2 == 0 else 'gen')


# ------------------------------------------------------------------------------------------------ the truth
def _to_mp(a):
    return mpmath.matrix([[mpmath.mpf(float(v)) for v in row] for row in np.asarray(a, dtype=np.float64)])


def _from_mp(m, d, dtype):
    out = np.empty((d, d), dtype=dtype)
    for i in range(d):
        for j in range(d):
            hi = float(m[i, j])
            out[i, j] = hi if dtype is np.float64 else LD(hi) + LD(float(m[i, j] - hi))
    return out


def exact(a, e=None, dtype=np.float64):
    """``(R, Z, X or None)`` of the double matrix ``a`` as given, from a 50-digit symmetric eigen-decomposition, each rounded
    to ``dtype`` (double; ``numpy.longdouble`` for the oracle's own check).  ~0.1 s at d = 8, ~1 s at d = 33: d <= 33 only."""
    a = np.asarray(a, dtype=np.float64)
    d = a.shape[0]
    assert a.shape == (d, d) and d <= 33 and np.array_equal(a, a.T)
    with mpmath.workdps(_DPS):
        w, U = mpmath.eigsy(_to_mp(a))
        assert all(w[i] > 0 for i in range(d)), 'exact(): the matrix is not positive definite'
        r = [mpmath.sqrt(w[i]) for i in range(d)]
        Ur, Uz = U.copy(), U.copy()
        for i in range(d):
            for j in range(d):
                Ur[i, j] = U[i, j] * r[j]
                Uz[i, j] = U[i, j] / r[j]
        Ut = U.T
        R, Z = Ur * Ut, Uz * Ut
        X = None
        if e is not None:
            S = Ut * _to_mp(e) * U
            for i in range(d):
                for j in range(d):
                    S[i, j] = S[i, j] / (r[i] + r[j])
            X = _from_mp(U * S * Ut, d, dtype)
        return _from_mp(R, d, dtype), _from_mp(Z, d, dtype), X


def lapack(a, e=None):
    """``(R, Z, X or None)`` by ``numpy.linalg.eigh``: the host route of objectives.py."""
    w, U = np.linalg.eigh(a)
    r = np.sqrt(w)
    X = None if e is None else U @ ((U.T @ e @ U) / (r[:, None] + r[None, :])) @ U.T
    return (U * r) @ U.T, (U / r) @ U.T, X


Truth = collections.namedtuple('Truth', 'a e R Z X lapack_R lapack_Z lapack_X')


@functools.lru_cache(maxsize=None)
def truth(case):
    """Inputs, exact matrices and LAPACK's, computed once per case and shared read-only by every test."""
    a, e = spd(*case), direction(case.d, case.seed)
    out = Truth(a, e, *exact(a, e), *lapack(a, e))
    for m in out:
        m.setflags(write=False)
    return out


def rel_err(q, want):
    """Relative Frobenius error of ``q`` against ``want`` (the difference taken in longdouble)."""
    return float(_fro(np.asarray(q, dtype=LD) - np.asarray(want, dtype=LD)) / _fro(np.asarray(want, dtype=LD)))


# ------------------------------------------------------------------------------------------------ residuals
def _fro(m):
    return np.sqrt(np.sum(m * m))


def residuals_ld(a, R, Z=None, X=None, e=None):
    """Residuals of the defining equations in longdouble (normalised as the module docstring says): a dict with ``rr``, and
    ``zr``, ``zaz`` when Z is given, ``sylv`` when X and e are; ``info2`` = ||R R - a||_F / c with c = max_i sum_j |a_ij|,
    the quantity the device entry reports as info[2]."""
    a, R = np.asarray(a, dtype=LD), np.asarray(R, dtype=LD)
    d = a.shape[0]
    eye = np.eye(d, dtype=LD)
    rr = _fro(R @ R - a)
    out = {'rr': float(rr / _fro(a)), 'info2': float(rr / np.max(np.sum(np.abs(a), axis=1)))}
    if Z is not None:
        Z = np.asarray(Z, dtype=LD)
        out['zr'] = float(_fro(Z @ R - eye) / (_fro(Z) * _fro(R)))
        out['zaz'] = float(_fro(Z @ a @ Z - eye) / (_fro(Z) ** 2 * _fro(a)))
    if X is not None:
        X, e = np.asarray(X, dtype=LD), np.asarray(e, dtype=LD)
        scale = 2 * _fro(R) * _fro(X) + _fro(e)
        out['sylv'] = float(_fro(R @ X + X @ R - e) / scale) if scale > 0 else 0.0
    return out


# ------------------------------------------------------------------------------------------------ model of the control
def model(a, e=None, max_steps=100):
    """The host entry ``sym_sqrt`` of vb_linalg.hip with numpy's matmul for the GEMMs: the symmetric part of ``a`` is
    staged, c = max row sum, the block matrix [[a, es e], [0, a]] / c with es = 0.1 c / ||e||_F, steps in groups of four,
    then what is known to be missing, else one, every step of a group applied.  Returns a dict: R, Z, X (or None), steps,
    acc = ||Y Y - M0||_F over the leading d x d block (what info[2] is)."""
    a = np.asarray(a, dtype=np.float64)
    a = 0.5 * (a + a.T)
    d = a.shape[0]
    m = 2 * d if e is not None else d
    c = np.max(np.sum(np.abs(a), axis=1))
    fro_e = np.sqrt(np.sum(e * e)) if e is not None else 0.0
    es = 0.1 * c / fro_e if fro_e > 0.0 else 0.0
    M0 = np.zeros((m, m))
    M0[:d, :d] = a / c
    if e is not None:
        M0[d:, d:] = M0[:d, :d]
        M0[:d, d:] = e * es / c
    Y, Z, eye = M0.copy(), np.eye(m), np.eye(m)
    it, prev, stop_at, converged, floor_tol = 0, 1e300, max_steps + 1, False, 4e-16 * m
    while not converged and it < max_steps:
        group = 4 if it == 0 else (stop_at - it if stop_at <= max_steps else 1)
        residual = []
        for _ in range(group):
            P = Z @ Y
            residual.append(np.sqrt(np.sum((eye - P) ** 2)))
            T = 1.5 * eye - 0.5 * P
            Y, Z = Y @ T, T @ Z
        for k, res in enumerate(residual):
            if converged:
                break
            assert np.isfinite(res), 'the iteration diverged'
            if res < floor_tol or (res < 1e-7 and res > 0.5 * prev):
                converged = True
            if res < 1e-4 and stop_at > max_steps:
                stop_at = it + k + 2
            prev = res
        it += group
        converged = converged or it >= stop_at
    acc = np.sqrt(np.sum(((Y @ Y - M0)[:d, :d]) ** 2))
    sc = np.sqrt(c)
    Yd, Zd = Y[:d, :d], Z[:d, :d]
    X = None if e is None else Y[:d, d:] * (sc / es if es > 0.0 else 0.0)
    return {'R': 0.5 * (Yd + Yd.T) * sc, 'Z': 0.5 * (Zd + Zd.T) / sc, 'X': X, 'steps': it, 'acc': float(acc)}
