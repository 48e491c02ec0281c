"""GPU: the row entries of the flat regression target -- LogisticRegressionModel, PoissonRegressionModel and
LinearRegressionModel through ``Model.__call__`` (vb_model_logp -> logistic_rows) and ``Model.grad`` / ``Engine.model_grad``
(vb_model_grad -> model_grad_rows -> glm_grad_enqueue) -- against the longdouble oracle of tests/_glm_rows_oracle.py, every
row and every element held to its own bound

    |dev - ref| <= (n_data + d + 16) 2^-53 bound          (derived there; tests/test_glm_rows_oracle_cpu.py checks the oracle)

  a. three row chunks of either entry (n_data = 70001: 479 rows per chunk of the gradient entry, 958 of the other), the
     observations cycling through 61 distinct ones so that the reference costs N x 61
  b. the 128-row floor of a chunk (n_data = 262200)
  c. the split ladder of the gradient product: one slab because n_data < 128, two because n_data / 128 binds, 2 n_cu / tiles
     slabs, the cap of 64, one launch at tiles >= n_cu; and n_data of 1 ... 129
  d. the links' tails: |eta| to 2000 (logit), mu to 1e39 (Poisson), residuals of 1e7 (Gaussian), calm rows beside them
  e. a NaN row and an inf row leave every other row bit for bit alone
  f. wherever both entries ran, their f agree within twice the bound (they share glm_term, not the chunking)

Observed max |dev - ref| / (2^-53 bound) on an MI355X (256 CUs), as logistic / Poisson / Gaussian, f of either entry (the two
gave the same bits in every case) then g, against the n_data + d + 16 allowed:
  a. N = 963 (3 chunks of the gradient entry, 2 of the other; 64 slabs in the full chunks and in the remainder)
       f 51.0 / 2006 / 13.9    g 18.5 / 12.3 / 20.2    of 70020;    N = 1921 (3 chunks), f 49.4 / 1983 / 13.9
  b. N = 133 (a 128-row chunk and 5 rows, 64 slabs each)    f 106 / 3113 / 39.7    g 23.8 / 27.8 / 78.1    of 262218
     The Poisson f of a and b is the constant, not the rows: sum_i -log(y_i!) is added up on the host one observation
     after the other, and over a design that repeats 61 observations the roundings do not cancel -- 2003 and 3086 of the
     figures above (computed on the host from the same sum), inside the bound, which allows every addition its half ulp.
  c. 1 slab (n_data 100)  f 1.57 / 2.53 / 1.61  g 0.99 / 1.02 / 1.79  of 121;    2 slabs (300)  f 1.01 / 1.20 / 1.67
     g 0.64 / 0.78 / 1.18  of 321;    21 slabs (1533 x 2 x 3457)  f 2.28 / 45.2 / 1.82  g 1.20 / 0.98 / 1.83  of 3475;
     64 slabs (130 x 2 x 8327)  f 1.60 / 151 / 2.13  g 0.84 / 0.94 / 1.34  of 8345;    one launch (1024 x 1024 x 257)
     f 1.92 / 14.6 / 1.04  g 0.75 / 0.71 / 0.94  of 1297;    3 whole slabs (70 x 5 x 384)  f 1.50 / 2.18 / 2.23
     g 0.45 / 0.66 / 2.09  of 405;    n_data 1 ... 129: f at most 2.72, g at most 3.61 (Gaussian, n_data 129) of 22 ... 150
  d. logit scale 15 (max |eta| 104)  f 0.63  g 3.52;    scale 300 (1980)  f 0.86  g 1.97;    Poisson scale 6 (37.8)  f 29.7
     g 16.5;    scale 12 (91.9)  f 33.0  g 11.3;    Gaussian 1e6 (7.6e6)  f 1.16  g 3.54;    each of 324
     (the Poisson f: the roundings of eta times dl_i = y_i - mu_i, which reaches 1e6 and 1e39 -- the |dl_i| a_i part of
     the bound; the float64 numpy oracle gives the same 29.7 and 33.0)
"""
import numpy as np
import pytest

import _glm_rows_oracle as O
from _laplace_oracle import KINDS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def vb():
    import viabel_amd
    from viabel_amd import _lib
    _lib.default_engine()
    return viabel_amd


@pytest.fixture(scope='module')
def n_cu(vb):
    from viabel_amd import _lib
    return _lib.default_engine().device_info()['cus']


_MODELS, _RUNS = {}, {}


def _model(vb, case):
    if case.name not in _MODELS:
        X, y = case.design()
        if case.kind == 'logistic':
            model = vb.LogisticRegressionModel(X, y, prior_sd=case.prior_sd)
        elif case.kind == 'poisson':
            model = vb.PoissonRegressionModel(X, y, prior_sd=case.prior_sd)
        else:
            model = vb.LinearRegressionModel(X, y, prior_sd=case.prior_sd, noise_sd=case.noise_sd)
        _MODELS[case.name] = model
    return _MODELS[case.name]


def _run(vb, case, x=None, call=True, grad=True):
    """The device's rows at the case's points (or at ``x``): f of Model.__call__, (f, g) of Engine.model_grad, Model.grad."""
    from viabel_amd import _lib
    model = _model(vb, case)
    out = {}
    if call:
        out['f_call'] = model(case.x if x is None else x)
    if grad:
        eng = _lib.default_engine()
        eng.set_model(model.device_spec())
        out['f_grad'], out['g_grad'] = eng.model_grad(case.x if x is None else x)
        out['g_model'] = model.grad(case.x if x is None else x)
    return out


def _run_case(vb, case, call=True, grad=True):
    key = (case.name, call, grad)
    if key not in _RUNS:
        _RUNS[key] = _run(vb, case, call=call, grad=grad)
    return _RUNS[key]


def _check(case, out):
    """Every row of every entry that ran against the reference, then the two f against each other."""
    f, g, bf, bg = case.reference()
    worst = {}
    for name, dev in out.items():
        ref, bound = (f, bf) if name.startswith('f') else (g, bg)
        assert dev.shape == ref.shape and np.all(np.isfinite(dev)), (case.name, name)
        worst[name] = O.excess(dev, ref, bound)
    print('%s: %s of %d allowed' % (case.name, ' '.join('%s %.2f' % (k, v.max()) for k, v in worst.items()), case.limit))
    for name, r in worst.items():
        bad = np.argwhere(~(r <= case.limit))
        assert bad.size == 0, '%s %s: %d elements over the bound, the first at %s with %.3g' % (
            case.name, name, len(bad), tuple(bad[0]), r[tuple(bad[0])])
    if 'f_call' in out and 'f_grad' in out:
        r = O.excess(out['f_call'], out['f_grad'], bf)
        print('%s: f_call against f_grad %.2f of %d allowed' % (case.name, r.max(), 2 * case.limit))
        assert np.all(r <= 2 * case.limit), (case.name, r.max())
    if 'g_model' in out:
        assert np.array_equal(out['g_model'], out['g_grad'])             # the same entry: the same bits


# ---- a. three chunks, every row --------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
def test_three_chunks_every_row(vb, n_cu, kind):
    """Two full chunks and a 5-row remainder of the gradient entry, which is one full chunk and the remainder of the
    log-density entry; then the same crossing of the log-density entry.  Points all distinct: a row in another row's place,
    or a remainder computed with a full chunk's workspace, is wrong by its whole value."""
    from viabel_amd import _lib
    chunk_g, chunk_f = _lib.glm_rows_chunk(O.CROSS_N_DATA, True), _lib.glm_rows_chunk(O.CROSS_N_DATA, False)
    assert (chunk_g, chunk_f) == (O.CROSS_CHUNK_GRAD, O.CROSS_CHUNK_LOGP)
    assert O.CROSS_N_GRAD == 2 * chunk_g + 5 == chunk_f + 5 and O.CROSS_N_LOGP == 2 * chunk_f + 5      # 3 and 2, then 3 chunks
    print('splits of a full chunk %d, of the remainder %d' % (
        _lib.glm_grad_splits(chunk_g, O.CROSS_D, O.CROSS_N_DATA, n_cu), _lib.glm_grad_splits(5, O.CROSS_D, O.CROSS_N_DATA, n_cu)))
    case = O.cycle_case(kind, O.CROSS_D, O.CROSS_N_DATA, O.CROSS_N_GRAD)
    assert len(np.unique(case.x, axis=0)) == O.CROSS_N_GRAD
    _check(case, _run_case(vb, case))
    case = O.cycle_case(kind, O.CROSS_D, O.CROSS_N_DATA, O.CROSS_N_LOGP)
    _check(case, _run_case(vb, case, grad=False))


# ---- b. chunk minimum ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
def test_chunk_minimum(vb, n_cu, kind):
    """(32 << 20) / round_up(n_data, 16) is 127: the 128-row floor makes the chunk, and 133 rows are a chunk and 5 rows."""
    from viabel_amd import _lib
    assert (32 << 20) // ((O.FLOOR_N_DATA + 15) // 16 * 16) < 128 == _lib.glm_rows_chunk(O.FLOOR_N_DATA, True)
    assert O.FLOOR_N == 128 + 5
    case = O.cycle_case(kind, O.FLOOR_D, O.FLOOR_N_DATA, O.FLOOR_N)
    _check(case, _run_case(vb, case, call=False))


# ---- c. split ladder -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('step', range(5))
def test_split_ladder(vb, n_cu, step, kind):
    from viabel_amd import _lib
    regime, rows, d, n_data = O.ladder_cases(n_cu)[step]
    got, splits = O.ladder_regime(rows, d, n_data, n_cu)
    assert got == regime and splits == _lib.glm_grad_splits(rows, d, n_data, n_cu)
    assert rows <= _lib.glm_rows_chunk(n_data, True)                      # one chunk: the split count above is the one used
    assert splits == 1 or n_data % (16 * splits) != 0
    print('%s: rows %d d %d n_data %d on %d CUs: %d splits' % (regime, rows, d, n_data, n_cu, splits))
    case = O.dense_case(kind, d, n_data, rows)
    _check(case, _run_case(vb, case))


@pytest.mark.parametrize('kind', KINDS)
def test_split_on_whole_slabs(vb, n_cu, kind):
    """n_data = 3 x 128, a multiple of 16: three slabs on the GEMM kernel that takes whole 16-observation steps only."""
    from viabel_amd import _lib
    rows, d, n_data = O.WHOLE_SLABS
    assert n_data % 16 == 0 and _lib.glm_grad_splits(rows, d, n_data, n_cu) == 3 == n_data // 128
    case = O.dense_case(kind, d, n_data, rows)
    _check(case, _run_case(vb, case))


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n_data', O.EDGE_N_DATA)
def test_few_observations(vb, n_data, kind):
    case = O.dense_case(kind, 5, n_data, 7)
    _check(case, _run_case(vb, case))


# ---- d. link tails ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,scale', O.tail_cases())
def test_link_tails(vb, kind, scale):
    """Saturated and calm rows side by side, each element held to its own bound; the placed rows x = +0, x = -0 and
    x = +-scale e_0 (every eta of one sign: one branch of the logit's p at a time) are the last four."""
    case = O.tail_case(kind, scale)
    out = _run_case(vb, case)
    print('%s: max |eta| %.4g' % (case.name, np.abs(case.x @ case.X.T).max()))
    _check(case, out)


# ---- e. row isolation ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,scale', O.tail_cases())
def test_row_isolation(vb, kind, scale):
    """A row of NaN and a row of +inf among the points of the tails: those two rows of f and g are not finite, every other
    row has the bits it had without them."""
    case = O.tail_case(kind, scale)
    clean = _run_case(vb, case)
    x = case.x.copy()
    x[O.TAIL_BAD_ROWS[0]], x[O.TAIL_BAD_ROWS[1]] = np.nan, np.inf
    out = _run(vb, case, x=x)
    bad = np.zeros(len(x), dtype=bool)
    bad[list(O.TAIL_BAD_ROWS)] = True
    for name, dev in out.items():
        rows_finite = np.isfinite(dev) if dev.ndim == 1 else np.isfinite(dev).all(axis=1)
        rows_none = ~np.isfinite(dev) if dev.ndim == 1 else (~np.isfinite(dev)).all(axis=1)
        assert np.array_equal(rows_finite, ~bad) and np.array_equal(rows_none, bad), (case.name, name)
        assert np.array_equal(dev[~bad], clean[name][~bad]), (case.name, name)
