"""CPU: SparseRegressionModel's host side (export, canonicalisation of the CSR input, the CSC form, constructor validation,
device_spec layout, the refusal of loo() and predict()) and the numpy oracle the GPU tests compare against
(tests/_sparse_oracle.py), checked against central differences."""
import os
import re

import numpy as np
import pytest

import viabel_amd as vb
from viabel_amd import _lib
from _sparse_oracle import SparseGLMOracle

LIKELIHOODS = ['logistic', 'poisson', 'gaussian']
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _response(lik, n, rng):
    if lik == 'logistic':
        return (rng.rand(n) < 0.5).astype(float)
    if lik == 'poisson':
        return rng.poisson(2.0, size=n).astype(float)
    return rng.randn(n)


def _dense(n_data, p, per_row, seed=0):
    rng = np.random.RandomState(seed)
    A = np.zeros((n_data, p))
    for i in range(n_data):
        A[i, rng.choice(p, size=min(per_row, p), replace=False)] = rng.randn(min(per_row, p)) / np.sqrt(per_row)
    return A


def _triple(A):
    rows, cols = np.nonzero(A)
    ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=A.shape[0]))])
    return A[rows, cols], cols, ptr


def test_exported_from_package_and_bound():
    assert vb.SparseRegressionModel is vb.models.SparseRegressionModel
    assert 'SparseRegressionModel' in vb.models.__all__
    assert _lib.MODEL_SPARSE_GLM == 8 and _lib.MODEL_SPARSE_GLM in _lib.MODELS_WITH_ROWS
    assert 'vb_sparse_glm_pointwise' in _lib.SIGNATURES
    assert _lib.SIGNATURES['vb_sparse_glm_pointwise'] == _lib.SIGNATURES['vb_locscale_pointwise']
    assert hasattr(_lib.Engine, 'sparse_glm_pointwise')
    assert not issubclass(vb.SparseRegressionModel, vb.LogisticRegressionModel)


def test_header_and_common_mirror_the_constants():
    header = open(os.path.join(ROOT, 'include', 'viabel_hip.h')).read()
    assert re.search(r'#define\s+VB_MODEL_SPARSE_GLM\s+8\b', header)
    assert re.search(r'int\s+vb_sparse_glm_pointwise\s*\(', header)
    common = open(os.path.join(ROOT, 'viabel_amd', 'csrc', 'vb_common.h')).read()
    assert re.search(r'model_has_rows\(int id\)\s*\{[^}]*VB_MODEL_SPARSE_GLM', common)
    m = re.search(r'kSparseSegment\s*=\s*(\d+)\s*;', common)
    assert m and int(m.group(1)) == _lib.SPARSE_SEGMENT
    m = re.search(r'kSparseChunkDoubles\s*=\s*\(int64_t\)(\d+)\s*<<\s*(\d+)', common)
    assert m and int(m.group(1)) << int(m.group(2)) == _lib.SPARSE_CHUNK_DOUBLES
    makefile = open(os.path.join(ROOT, 'viabel_amd', 'csrc', 'Makefile')).read()
    assert 'vb_sparse.hip' in makefile


def test_chunk_rows_arithmetic():
    assert _lib.sparse_chunk_rows(1, 1) == 8192                           # the cap
    assert _lib.sparse_chunk_rows(200000, 50000) == 64                    # the floor
    r = _lib.sparse_chunk_rows(2500, 30)
    assert r % 64 == 0 and r == _lib.SPARSE_CHUNK_DOUBLES // (2 * 2530) // 64 * 64 and 64 < r < 8192


def test_canonical_form_of_unsorted_duplicated_input():
    # row 0: (2, 1.0), (0, 2.0), (2, 0.5) -> (0, 2.0), (2, 1.5); row 1: (1, 3.0), (1, -3.0) sums to 0 -> dropped, and an
    # explicit zero; row 2 empty; row 3: one entry
    data = np.array([1.0, 2.0, 0.5, 3.0, -3.0, 0.0, 4.0])
    indices = np.array([2, 0, 2, 1, 1, 3, 3])
    indptr = np.array([0, 3, 6, 6, 7])
    m = vb.SparseRegressionModel((data, indices, indptr), np.zeros(4), shape=(4, 5))
    v, c, ptr = m.csr
    assert v.dtype == np.float64 and c.dtype == np.int32 and ptr.dtype == np.int64
    np.testing.assert_array_equal(v, [2.0, 1.5, 4.0])
    np.testing.assert_array_equal(c, [0, 2, 3])
    np.testing.assert_array_equal(ptr, [0, 2, 2, 2, 3])
    assert (m.n_data, m.n_features, m.nnz, m.likelihood, m.dim) == (4, 5, 3, 'logistic', 5)
    want = np.zeros((4, 5))
    want[0, 0], want[0, 2], want[3, 3] = 2.0, 1.5, 4.0
    np.testing.assert_array_equal(m.to_dense(), want)


def test_duplicates_are_summed_in_input_order():
    vals = np.array([1e16, 1.0, -1e16, 1.0])                              # ((1e16 + 1) - 1e16) + 1 = 1, not 2 or 0
    m = vb.SparseRegressionModel((vals, np.zeros(4, dtype=int), np.array([0, 4])), np.zeros(1), shape=(1, 1))
    want = ((vals[0] + vals[1]) + vals[2]) + vals[3]
    assert m.csr[0][0] == want


def test_from_dense_round_trip_and_csc():
    A = _dense(23, 9, 3, seed=1)
    A[5] = 0.0                                                            # an empty row
    A[:, 4] = 0.0                                                         # an empty column
    m = vb.SparseRegressionModel.from_dense(A, np.zeros(23))
    np.testing.assert_array_equal(m.to_dense(), A)
    assert m.nnz == np.count_nonzero(A)
    vt, r, ptr_t = m.csc
    assert vt.dtype == np.float64 and r.dtype == np.int32 and ptr_t.dtype == np.int64 and ptr_t.shape == (10,)
    tv, tc, tptr = _triple(A.T.copy())                                    # the CSR of the transpose
    np.testing.assert_array_equal(vt, tv)
    np.testing.assert_array_equal(r, tc)
    np.testing.assert_array_equal(ptr_t, tptr)
    for j in range(9):
        assert np.all(np.diff(r[ptr_t[j]:ptr_t[j + 1]]) > 0)              # rows increase within every column
    assert ptr_t[5] == ptr_t[4]                                           # the empty column
    same = vb.SparseRegressionModel(_triple(A), np.zeros(23), shape=A.shape)
    for a, b in zip(m.csr + m.csc, same.csr + same.csc):
        np.testing.assert_array_equal(a, b)


def test_scipy_matrix_is_accepted():
    sp = pytest.importorskip('scipy.sparse')
    A = _dense(12, 7, 2, seed=2)
    for X in (sp.csr_matrix(A), sp.coo_matrix(A), sp.csc_matrix(A)):
        m = vb.SparseRegressionModel(X, np.zeros(12))
        np.testing.assert_array_equal(m.to_dense(), A)


def test_anything_with_tocsr_is_accepted_without_scipy():
    A = _dense(6, 4, 2, seed=3)

    class Duck:
        shape = A.shape

        def tocsr(self):
            class CSR:
                pass
            out = CSR()
            out.data, out.indices, out.indptr = _triple(A)
            out.shape = A.shape
            return out
    np.testing.assert_array_equal(vb.SparseRegressionModel(Duck(), np.zeros(6)).to_dense(), A)
    source = open(vb.models.__file__).read()
    assert not re.search(r'^\s*(import|from)\s+scipy', source, re.M)      # the package does not import scipy


def test_dense_array_is_refused_with_a_pointer():
    A = _dense(6, 4, 2)
    with pytest.raises(ValueError, match='from_dense') as e:
        vb.SparseRegressionModel(A, np.zeros(6))
    assert 'LogisticRegressionModel' in str(e.value)
    with pytest.raises(ValueError, match='from_dense'):
        vb.SparseRegressionModel(_triple(A), np.zeros(6))                 # a triple without its shape


def _good():
    A = _dense(6, 4, 2, seed=4)
    d, i, p = _triple(A)
    return dict(X=(d.copy(), i.copy(), p.copy()), y=np.zeros(6), shape=(6, 4))


@pytest.mark.parametrize('name,change', [
    ('nan value', lambda k: k['X'][0].__setitem__(0, np.nan)),
    ('inf value', lambda k: k['X'][0].__setitem__(1, np.inf)),
    ('indptr not from 0', lambda k: k['X'][2].__setitem__(0, 1)),
    ('indptr not to nnz', lambda k: k['X'][2].__setitem__(-1, k['X'][2][-1] - 1)),
    ('indptr not monotone', lambda k: k['X'][2].__setitem__(2, 0)),
    ('indptr of the wrong length', lambda k: k.__setitem__('X', (k['X'][0], k['X'][1], k['X'][2][:-1]))),
    ('index too large', lambda k: k['X'][1].__setitem__(0, 4)),
    ('index negative', lambda k: k['X'][1].__setitem__(0, -1)),
    ('n_data too large', lambda k: k.__setitem__('shape', (2 ** 31, 4))),
    ('p too large', lambda k: k.__setitem__('shape', (6, 2 ** 31))),
    ('y of the wrong shape', lambda k: k.__setitem__('y', np.zeros(5))),
    ('y 2-D', lambda k: k.__setitem__('y', np.zeros((6, 1)))),
    ('y outside {0, 1}', lambda k: k.__setitem__('y', np.full(6, 0.5))),
    ('negative counts', lambda k: (k.__setitem__('y', -np.ones(6)), k.__setitem__('likelihood', 'poisson'))),
    ('y not finite', lambda k: (k.__setitem__('y', np.full(6, np.nan)), k.__setitem__('likelihood', 'gaussian'))),
    ('prior_sd', lambda k: k.__setitem__('prior_sd', 0.0)),
    ('noise_sd', lambda k: k.__setitem__('noise_sd', -1.0)),
    ('likelihood', lambda k: k.__setitem__('likelihood', 'probit')),
])
def test_constructor_refuses(name, change):
    kwargs = _good()
    vb.SparseRegressionModel(**kwargs)                                    # the unchanged arguments are fine
    change(kwargs)
    with pytest.raises(ValueError):
        vb.SparseRegressionModel(**kwargs)


@pytest.mark.parametrize('lik', LIKELIHOODS)
def test_spec_layout(lik):
    rng = np.random.RandomState(5)
    A = _dense(11, 6, 2, seed=5)
    A[3] = 0.0                                                            # an all-empty row
    A[:, 2] = 0.0                                                         # an all-empty column
    y = _response(lik, 11, rng)
    m = vb.SparseRegressionModel.from_dense(A, y, likelihood=lik, prior_sd=2.5, noise_sd=0.7)
    nnz = m.nnz
    model_id, dim, dparams, iparams = m.device_spec()
    assert model_id == _lib.MODEL_SPARSE_GLM and dim == 6
    assert dparams.dtype == np.float64 and dparams.shape == (2 * nnz + 11 + 2,)
    np.testing.assert_array_equal(dparams[:nnz], m.csr[0])
    np.testing.assert_array_equal(dparams[nnz:2 * nnz], m.csc[0])
    np.testing.assert_array_equal(dparams[2 * nnz:2 * nnz + 11], y)
    assert list(dparams[-2:]) == [2.5, 0.7]
    assert iparams.dtype == np.int64 and iparams.shape == (4 + 12 + nnz + 7 + nnz,)
    assert list(iparams[:4]) == [11, 6, vb.SparseRegressionModel._LINKS[lik], nnz]
    o = 4
    np.testing.assert_array_equal(iparams[o:o + 12], m.csr[2])
    np.testing.assert_array_equal(iparams[o + 12:o + 12 + nnz], m.csr[1])
    o += 12 + nnz
    np.testing.assert_array_equal(iparams[o:o + 7], m.csc[2])
    np.testing.assert_array_equal(iparams[o + 7:], m.csc[1])
    assert m.csr[2][4] == m.csr[2][3] and m.csc[2][3] == m.csc[2][2]      # the empty row and the empty column
    assert m.device_spec() is m.device_spec()                             # cached: the engine keys on identity


def test_spec_of_an_all_empty_matrix():
    m = vb.SparseRegressionModel((np.zeros(0), np.zeros(0, dtype=int), np.zeros(4, dtype=int)), np.zeros(3), shape=(3, 2))
    _, dim, dparams, iparams = m.device_spec()
    assert dim == 2 and dparams.shape == (3 + 2,) and list(iparams) == [3, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0]


def test_loo_and_predict_refuse_the_model():
    m = vb.SparseRegressionModel.from_dense(_dense(6, 4, 2), np.zeros(6))
    with pytest.raises(NotImplementedError, match='psisloo'):
        vb.loo(np.zeros(8), model=m, approx=vb.MFGaussian(4), n_samples=10)
    with pytest.raises(NotImplementedError):
        vb.predict(np.zeros(8), model=m, approx=vb.MFGaussian(4), n_samples=10)
    assert 'psisloo' in vb.SparseRegressionModel.__doc__


@pytest.mark.parametrize('lik', LIKELIHOODS)
def test_oracle_against_central_differences(lik):
    rng = np.random.RandomState(6)
    A = _dense(40, 7, 3, seed=6)
    y = _response(lik, 40, rng)
    o = SparseGLMOracle(A, y, lik, prior_sd=3.0, noise_sd=0.8)
    x = 0.3 * rng.randn(4, 7)
    g = o.grad(x)
    h = 1e-6
    fd = np.empty_like(g)
    for j in range(7):
        e = np.zeros(7)
        e[j] = h
        fd[:, j] = (o.logp(x + e) - o.logp(x - e)) / (2 * h)
    assert np.max(np.abs(g - fd)) / np.max(np.abs(g)) < 1e-7
    H = o.hessian(x[0])
    Hfd = np.stack([(o.grad(x[0] + h * e)[0] - o.grad(x[0] - h * e)[0]) / (2 * h) for e in np.eye(7)])
    assert np.max(np.abs(H - Hfd)) / np.max(np.abs(H)) < 1e-7 and np.array_equal(o.hvp(x[0], x[1:3]), x[1:3] @ H.T)
    np.testing.assert_allclose(o.pointwise(x).sum(1) + o.log_prior(x), o.logp(x), rtol=1e-14)
    assert o.pointwise(x[0]).shape == (1, 40) and o.logp(x[0]).shape == (1,)


def test_oracle_terms_are_normalised_densities():
    """sum over the support (logistic, Poisson) / a Riemann sum (Gaussian) of exp(term) is 1."""
    from _sparse_oracle import terms
    eta = 0.37
    assert abs(sum(np.exp(terms('logistic', np.array([v]), eta)[0][0]) for v in (0.0, 1.0)) - 1.0) < 1e-14
    assert abs(np.sum(np.exp(terms('poisson', np.arange(60.0), eta)[0])) - 1.0) < 1e-13
    grid = np.linspace(-12.0, 12.0, 48001)
    assert abs(np.sum(np.exp(terms('gaussian', grid, eta, 0.8)[0])) * (grid[1] - grid[0]) - 1.0) < 1e-10
