"""GPU: the throughput-mode generator (``rng='philox'``, vb_rng.h / vb_rng.hip and the in-register sites of
vb_meanfield.hip) element by element against the host reference tests/_philox_oracle.py.

Every element is a pure function of (seed, stream, row, col), so the reference states what each must be; the reference
itself is checked without a GPU in tests/test_philox_oracle_cpu.py.

Bounds ("Philox layout"):

* normals: ``|z_dev - z_ref| <= 1e-15 max(1, r_ref)``.  The device's log is good to 3.1e-16 relative and its sin / cos to
  1.5e-16 absolute (tools/rng_math_check.hip); with the roundings of the square root and of the product that bounds the
  error at about 5.3e-16 r; a host port of the two functions measured 3.3e-16 max(1, r) against long double over
  1.7e7 normals.  1e-15 is a margin of two to three; a layout or constant bug is off by O(1).
* Student-t: relative 1e-13, chi-square: relative 1e-12 (its draws with t = 1 + c x next to 0 amplify; the reference in
  fp64 against itself in long double showed 2.1e-14 at df = 2.5).
* the objective on in-register noise: the project's tolerances (value 1e-12, gradient 1e-11 of its largest entry).

Each test prints the maximum it observed (``pytest -s`` shows it).  The rejection samplers' references also mark draws
whose accept / reject decision fp64 and long double might not share; a test leaves out at most one such element, prints
it, and fails on more.
"""
import functools
import os

import numpy as np
import pytest

import _philox_oracle as P
from oracle import families as ofam
from oracle import models as omod
from oracle import objectives as oobj

pytestmark = pytest.mark.gpu

HI = 1 << 32


@pytest.fixture(scope='module')
def env():
    import viabel_amd as vb
    from viabel_amd import _lib
    return vb, _lib.default_engine(), _lib


def _report(name, what, value):
    print('\nPHILOX-REF %s: %s = %.3e' % (name, what, value))


def _normal_ratio(eng, n, d, seed, stream, row_offset, slot=5):
    """max |z_dev - z_ref| / max(1, r_ref) over the block, and the reference's tail mask."""
    eng.noise_generate(slot, n, d, seed=seed, stream=stream, row_offset=row_offset)
    dev = eng.noise_get_host(slot, n, d)
    z, r, tail = P.normals(seed, stream, row_offset, n, d)
    assert np.all(np.isfinite(dev))
    ratio = np.abs(dev.astype(P.LD) - z) / np.maximum(1.0, r)
    return float(ratio.max()), tail


NORMAL_CASES = {
    # name: (n, d, seed, stream, row_offset)
    'plain': (64, 64, 9, 3, 0),
    'd1': (16, 1, 9, 3, 0),
    'd7': (16, 7, 9, 3, 0),
    'd515_two_workgroups_in_x': (16, 515, 9, 3, 0),
    'n5': (5, 6, 9, 3, 0),
    'n12': (12, 6, 9, 3, 0),
    'n13': (13, 6, 9, 3, 0),
    'offset3_row_by_row': (20, 10, 9, 3, 3),
    'offset1001_row_by_row': (20, 10, 9, 3, 1001),
    'offset_2p32_aligned': (20, 10, 9, 3, HI),
    'offset_2p32_plus_5': (20, 10, 9, 3, HI + 5),
    'offset_2p35_plus_12': (20, 10, 9, 3, (1 << 35) + 12),
    'seed_high_word': (24, 10, (5 << 32) | 77, 3, 0),
    'stream_high_word': (24, 10, 77, (9 << 32) | 3, 0),
    'both_high_words': (24, 10, (5 << 32) | 77, (9 << 32) | 3, 4),
    'stream_low_bits_only': (24, 10, 77, 0xFFFFFFFF, 0),
    # the only case far above a few thousand elements: rng_fill launches once per 65535 * 8 rows (gridDim.y), and the
    # second launch's pointer and row offsets are met by nothing smaller
    'second_launch_of_a_long_matrix': (65535 * 8 + 11, 2, 4, 1, 0),
}


@pytest.mark.parametrize('case', list(NORMAL_CASES))
def test_normals_element_by_element(env, case):
    _, eng, _ = env
    n, d, seed, stream, row_offset = NORMAL_CASES[case]
    ratio, _ = _normal_ratio(eng, n, d, seed, stream, row_offset)
    _report('normals[%s]' % case, 'max |z_dev - z_ref| / max(1, r)', ratio)
    assert ratio <= 1e-15


def test_high_words_enter_only_through_their_xor(env):
    """The layout's known identity, stated so that nobody "fixes" it silently: k1 = seed_hi ^ stream_hi, so
    (seed, stream) = (a 2^32, a 2^32) gives the matrix of (0, 0) -- callers keep streams below 2^32."""
    _, eng, _ = env
    n, d = 16, 10
    eng.noise_generate(5, n, d, seed=0, stream=0)
    base = eng.noise_get_host(5, n, d)
    eng.noise_generate(6, n, d, seed=7 << 32, stream=7 << 32)
    np.testing.assert_array_equal(eng.noise_get_host(6, n, d), base)
    z, r, _ = P.normals(0, 0, 0, n, d)
    assert np.max(np.abs(base.astype(P.LD) - z) / np.maximum(1.0, r)) <= 1e-15
    # ... and either high word alone changes every element
    for seed, stream in [(7 << 32, 0), (0, 7 << 32)]:
        eng.noise_generate(6, n, d, seed=seed, stream=stream)
        assert not np.any(eng.noise_get_host(6, n, d) == base)


def _window_start(row):
    """An unaligned first row at most two rows before the hit (None: the hit is in row 0 or 1 of an aligned start)."""
    for start in (row - 1, row - 2):
        if start >= 0 and start & 7:
            return start
    return row if row & 7 else None


def test_tail_of_the_normal_distribution(env):
    """Every radius word below 4096 that a host scan of seeds 0 .. 8191 finds at n = d = 64: the aligned block of eight
    rows around it (the quad path) and a window starting just before it at an unaligned offset (the row-by-row path)."""
    _, eng, _ = env
    hits = P.tail_hits_64()
    assert {w for _, _, _, w in hits} == {0, 2}
    compared, worst, both_paths = 0, 0.0, set()
    for seed, row, pair, word in hits:
        ratio, tail = _normal_ratio(eng, 8, 64, seed, 0, row & ~7)
        assert tail[row & 7, 2 * pair] and tail[row & 7, 2 * pair + 1]
        assert ratio <= 1e-15, (seed, row, pair, word, 'aligned block', ratio)
        compared += int(tail.sum())
        worst = max(worst, ratio)
        start = _window_start(row)
        if start is None:
            continue
        ratio, tail = _normal_ratio(eng, 6, 64, seed, 0, start)
        assert tail[row - start, 2 * pair] and tail[row - start, 2 * pair + 1]
        assert ratio <= 1e-15, (seed, row, pair, word, 'window at %d' % start, ratio)
        compared += int(tail.sum())
        worst = max(worst, ratio)
        both_paths.add(word)
    assert both_paths == {0, 2}          # a row with bit 2 clear and a g + 4 partner, each through both kernel paths
    _report('tail', 'tail elements compared', compared)
    _report('tail', 'max |z_dev - z_ref| / max(1, r)', worst)


def _drop_undecidable(name, err, undecidable):
    """At most one undecidable element may be left out (printed); more fail."""
    count = int(undecidable.sum())
    print('\nPHILOX-REF %s: undecidable = %d' % (name, count))
    assert count <= 1, np.argwhere(undecidable)
    if count:
        print('PHILOX-REF %s: left out element %s' % (name, np.argwhere(undecidable)[0]))
    return np.where(undecidable, 0.0, err)


STUDENT_SHAPES = {
    # name: (n, d, seed, stream, row_offset)
    '300x33': (300, 33, 13, 2, 0),
    '64x7_offset701': (64, 7, (3 << 32) | 13, (1 << 32) | 2, 701),
}


@pytest.mark.parametrize('df', [2.5, 7.0, 100.0])
@pytest.mark.parametrize('shape', list(STUDENT_SHAPES))
def test_student_t_element_by_element(env, shape, df):
    _, eng, _lib = env
    n, d, seed, stream, row_offset = STUDENT_SHAPES[shape]
    eng.noise_generate(5, n, d, seed=seed, stream=stream, row_offset=row_offset, kind=_lib.NOISE_STUDENT_T, df=df)
    dev = eng.noise_get_host(5, n, d)
    t, undecidable = P.student_t(seed, stream, row_offset, n, d, df)
    name = 'student_t[%s, df=%g]' % (shape, df)
    rel = _drop_undecidable(name, np.abs(dev.astype(P.LD) - t) / np.abs(t), undecidable)
    _report(name, 'max relative error', float(rel.max()))
    assert rel.max() <= 1e-13


@pytest.mark.parametrize('df,seed,stream,row_offset', [(2.5, 21, 4, 0), (9.0, (2 << 32) | 21, (6 << 32) | 4, HI + 3),
                                                       (100.0, 21, 5, 17)])
def test_chisquare_element_by_element(env, df, seed, stream, row_offset):
    _, eng, _ = env
    n = 20000
    eng.chisq_generate(df, n, seed=seed, stream=stream, row_offset=row_offset)
    dev = eng.chisq_get_host(n)
    x, undecidable = P.chisquare(seed, stream, row_offset, n, df)
    name = 'chisquare[df=%g]' % df
    rel = _drop_undecidable(name, np.abs(dev.astype(P.LD) - x) / x, undecidable)
    _report(name, 'max relative error', float(rel.max()))
    assert rel.max() <= 1e-12


# ---- in-register generation ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tail_seed_64():
    return P.tail_hits_64()[0][0]


def _register_cases():
    # name: (d, n, seed, stream, row_offset, n_total)
    return {
        'tail_seed_64x64': (64, 64, None, 0, 0, 64),
        'offset1003_shard_of_4n': (64, 64, 31, 6, 1003, 256),
        '257x1000': (257, 1000, 9, 77, 0, 1000),
    }


@functools.lru_cache(maxsize=None)
def _reference_noise(family, case):
    """The host reference's noise of a case as fp64, computed once and shared (read only)."""
    d, n, seed, stream, row_offset, _ = _register_cases()[case]
    seed = _tail_seed_64() if seed is None else seed
    if family == 'student':
        t, undecidable = P.student_t(seed, stream, row_offset, n, d, 7.0)
        assert not undecidable.any()
        noise = t.astype(np.float64)
    else:
        z, _, tail = P.normals(seed, stream, row_offset, n, d)
        assert tail.any() or case != 'tail_seed_64x64'
        noise = z.astype(np.float64)
    noise.setflags(write=False)
    return seed, noise


@pytest.mark.parametrize('one_launch', ['1', '0'])
@pytest.mark.parametrize('target', ['gauss', 'funnel'])
@pytest.mark.parametrize('family', ['gaussian', 'student'])
@pytest.mark.parametrize('case', list(_register_cases()))
def test_in_register_noise_against_the_oracle_on_reference_noise(env, case, family, target, one_launch):
    """``elbo_grad_meanfield_philox`` against ``oracle.objectives.exclusive_kl`` on the HOST REFERENCE's noise (the
    existing in-register tests hand the oracle the device's own draws).  In the 64 x 64 case the seed is one whose
    matrix holds a tail element: it alone moves the value by about 0.7 %.

    A shard of a larger job (n_total > n) divides the data term by n_total and keeps the entropy term whole
    (tests/test_gpu_comm.py::test_shard_of_a_larger_job): with H the entropy the oracle adds, value = -(F / n_total + H)
    where the oracle's own value is -(F / n + H), and the same for the gradient, whose entropy part is 1 per log sigma."""
    vb, eng, _lib = env
    d, n, _, stream, row_offset, n_total = _register_cases()[case]
    seed, noise = _reference_noise(family, case)
    rng = np.random.RandomState(d + n)
    if target == 'gauss':
        mean, sd = rng.randn(d), np.exp(0.2 * rng.randn(d))
        model, omodel = vb.GaussianModel(mean, sd), omod.GaussDiag(mean, sd)
    else:
        model, omodel = vb.FunnelModel(d, scale_index=d // 3), omod.Funnel(d, d // 3)
    student = family == 'student'
    fam, df = (_lib.FAMILY_MF_STUDENT_T, 7.0) if student else (_lib.FAMILY_MF_GAUSSIAN, 0.0)
    ofamily = ofam.MFStudentT(d, df) if student else ofam.MFGaussian(d)
    theta = np.concatenate([0.3 * rng.randn(d), -1.0 + 0.2 * rng.randn(d)])
    ov, og = oobj.exclusive_kl(ofamily, omodel, theta, noise)
    if n_total != n:
        share, H = n / n_total, ofamily.entropy(theta)
        ov = (ov + H) * share - H
        og = og * share
        og[d:] -= 1.0 - share
    eng.set_model(model.device_spec())
    before = os.environ.get('VB_MF_ONE')
    os.environ['VB_MF_ONE'] = one_launch
    try:
        value, grad = eng.elbo_grad_meanfield_philox(0, n, d, theta, fam, seed, stream, df=df, n_total=n_total,
                                                     row_offset=row_offset)
    finally:
        if before is None:
            del os.environ['VB_MF_ONE']
        else:
            os.environ['VB_MF_ONE'] = before
    err_v, err_g = abs(value - ov) / abs(ov), np.max(np.abs(grad - og)) / np.max(np.abs(og))
    name = 'in_register[%s, %s, %s, VB_MF_ONE=%s]' % (case, family, target, one_launch)
    _report(name, 'value rel err', err_v)
    _report(name, 'gradient err / max |grad|', err_g)
    assert err_v <= 1e-12 and err_g <= 1e-11


# ---- Python plumbing: which (seed, stream) a family's calls use -------------------------------------------------------
# sample(theta, n) of a family built with (seed=s, rng='philox'): its c-th call without `seed=` draws the base noise of
# (seed s, stream c), c = 0, 1, ...; a call with `seed=t` draws (seed t, stream 0) and does not count.
#
# Bounds: x = fl(mu + fl(sigma e)) with e the device's draw: the draw's own bound times sigma, plus two roundings
# (2^-53 each, 2.3e-16 together) of a quantity no larger than |mu| + sigma |e|.
def test_mf_gaussian_sample_uses_seed_and_call_number(env):
    vb, _, _ = env
    d, n, seed = 9, 21, 17          # a family's seed also seeds its numpy stream: below 2^32, as numpy requires
    approx = vb.MFGaussian(d, seed=seed, rng='philox')
    rng = np.random.RandomState(0)
    mu, ls = rng.randn(d), -1.0 + 0.3 * rng.randn(d)
    theta, sig = np.concatenate([mu, ls]), np.exp(ls)

    def check(x, s, stream):
        z, r, _ = P.normals(s, stream, 0, n, d)
        bound = 1e-15 * sig * np.maximum(1.0, r) + 2.3e-16 * (np.abs(mu) + sig * np.abs(z))
        assert np.all(np.abs(x.astype(P.LD) - (mu + sig * z)) <= bound), (s, stream)
    check(approx.sample(theta, n), seed, 0)
    check(approx.sample(theta, n), seed, 1)
    check(approx.sample(theta, n, seed=99), 99, 0)
    check(approx.sample(theta, n), seed, 2)


def test_mf_student_t_sample_uses_seed_and_call_number(env):
    vb, _, _ = env
    d, n, seed, df = 9, 21, 23, 7.0
    approx = vb.MFStudentT(d, df, seed=seed, rng='philox')
    rng = np.random.RandomState(1)
    mu, ls = rng.randn(d), -1.0 + 0.3 * rng.randn(d)
    theta, sig = np.concatenate([mu, ls]), np.exp(ls)
    for call in range(2):
        x = approx.sample(theta, n)
        t, undecidable = P.student_t(seed, call, 0, n, d, df)
        assert not undecidable.any()
        bound = 1e-13 * sig * np.abs(t) + 2.3e-16 * (np.abs(mu) + sig * np.abs(t))
        assert np.all(np.abs(x.astype(P.LD) - (mu + sig * t)) <= bound), call


def test_multivariate_t_sample_uses_seed_and_call_number(env):
    """The normals of call c are Philox (seed, stream c); the chi-square draws come from the family's numpy stream
    (``RandomState(seed).chisquare``, consecutive calls continue it).  x = mu + (z R) / s, R the symmetric root of
    L L' by eigh on both sides: the normals' bound through |R| / s, plus 1e-14 (|mu| + |z|_1 ||R||_2 / s) for the
    (d + 2)-term fp64 sums, the division and the two eigendecompositions' rounding, which is relative to the norm of R
    and not to its entries (d = 5, condition number < 10; 1e-14 is 45 roundings).  That term dominates: this test pins
    which (seed, stream) and which chi-square draws a call uses -- a wrong one is off by O(1) -- and is no accuracy check
    of the sample path."""
    vb, _, _ = env
    d, n, seed, df = 5, 40, 11, 6.0
    approx = vb.MultivariateT(d, df, seed=seed, rng='philox')
    rng = np.random.RandomState(2)
    mu = rng.randn(d)
    L = np.tril(0.05 * rng.randn(d, d), -1) + np.diag(np.exp(-1.0 + 0.1 * rng.randn(d)))
    theta = np.concatenate([mu, ofam.chol_to_free(L)])
    w, U = np.linalg.eigh(L @ L.T)
    R = (U * np.sqrt(w)) @ U.T
    rs = np.random.RandomState(seed)
    for call in range(2):
        x = approx.sample(theta, n)
        s = np.sqrt(rs.chisquare(df, n) / df)[:, None]
        z, r, _ = P.normals(seed, call, 0, n, d)
        want = mu + (z @ R.astype(P.LD)) / s
        znorm = np.sum(np.abs(z), axis=1, keepdims=True) * np.linalg.norm(R, 2)
        bound = (1e-15 * np.maximum(1.0, r)) @ np.abs(R) / s + 1e-14 * (np.abs(mu) + znorm / s)
        assert np.all(np.abs(x.astype(P.LD) - want) <= bound), call


def test_lr_gaussian_base_noise_uses_streams_2c_and_2c_plus_1(env):
    """Call c of an LRGaussian draws its n x D block from stream 2 c and its n x k block from stream 2 c + 1 (the
    convention of ``vb_fit``); an explicit seed uses streams 0 / 1 of that seed and does not count."""
    vb, _, _ = env
    d, k, n, seed = 9, 3, 21, 29
    approx = vb.LRGaussian(d, seed=seed, k=k, rng='philox')

    def check(noise, s, c):
        for got, stream, cols in [(noise[1], 2 * c, d), (noise[0], 2 * c + 1, k)]:
            z, r, _ = P.normals(s, stream, 0, n, cols)
            assert np.max(np.abs(got.astype(P.LD) - z) / np.maximum(1.0, r)) <= 1e-15, (s, c, stream)
    check(approx._base_noise(n), seed, 0)
    check(approx._base_noise(n), seed, 1)
    check(approx._base_noise(n, seed=99), 99, 0)
    check(approx._base_noise(n), seed, 2)
