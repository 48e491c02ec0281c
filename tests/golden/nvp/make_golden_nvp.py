#!/usr/bin/env python3
"""Generate the NVPFlow golden vectors from the upstream reference itself.

Needs a checkout of the upstream reference (``--reference DIR``, the directory that holds its ``viabel`` package);
writes ``tests/golden/nvp/*.npz`` and their digests, ``tests/golden/nvp/digests.json``.  The reference is imported
through the shims of ``tests/golden/_ref_stubs.py``: the flow's forward and inverse passes, the prior and the
ExclusiveKL closure are the reference's own code; the gradient is Richardson central differences of that closure with
the prior's generator restored before every evaluation (``approx.prior._rs``: the flow's own ``_rs`` is never used).

Each fixture stores theta, the masks, the prior draws z0, ``sample``, ``log_density(theta, sample)``, the path-form
value and FD gradient, and the prior generator's state after the objective call.

Usage:  python tests/golden/nvp/make_golden_nvp.py --reference DIR [--check]
"""
import os
import sys
import tempfile

import numpy as np
import scipy.stats

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.dirname(HERE)
TESTS = os.path.dirname(GOLDEN)
ROOT = os.path.dirname(TESTS)
sys.path.insert(0, GOLDEN)
sys.path.insert(0, TESTS)
sys.path.insert(0, ROOT)

if '--reference' not in sys.argv[1:-1]:
    sys.exit(__doc__.strip().splitlines()[-1])
_i = sys.argv.index('--reference')
REFERENCE_ROOT = os.path.abspath(sys.argv.pop(_i + 1))
sys.argv.pop(_i)

import _ref_stubs  # noqa: E402
import _golden     # noqa: E402

_ref_stubs.install(REFERENCE_ROOT)

from viabel import approximations as ref_approx  # noqa: E402  (the reference)
from viabel import objectives as ref_obj         # noqa: E402

norm = scipy.stats.norm
DIGESTS = os.path.join(HERE, 'digests.json')


class _AnyDerivative:
    """NeuralNet.forward also forms a log-determinant through elementwise_grad (discarded by NVPFlow); the shim
    routes elementwise_grad to STATE['model'], so give it something that evaluates."""

    def grad(self, x):
        return np.ones_like(x)


def log_p_of(kind, D, rng):
    if kind == 'gauss_diag':
        mean = rng.randn(D)[np.newaxis, :]
        stdev = np.exp(0.5 * rng.randn(D))[np.newaxis, :]

        def log_p(x):      # viabel/tests/test_objectives.py:18-19
            return np.sum(norm.logpdf(np.atleast_2d(x), loc=mean, scale=stdev), axis=1)
        return log_p, dict(model_kind='gauss_diag', model_mean=mean[0], model_stdev=stdev[0])
    k, tau = D - 1, 1.0

    def log_p(x):          # docs/source/quickstart.ipynb:23-29 generalised to D dims
        x = np.atleast_2d(x)
        out = norm.logpdf(x[:, k], 0, tau)
        for d in range(D):
            if d != k:
                out = out + norm.logpdf(x[:, d], 0, np.exp(x[:, k]))
        return out
    return log_p, dict(model_kind='funnel', model_scale_index=k, model_log_sigma_stdev=tau)


def half_masks(D, pairs):         # viabel/tests/test_approximations.py:134-138
    half, halfplus = D // 2, (D + 1) // 2
    m1 = np.hstack([[0] * half, [1] * halfplus])
    m2 = np.hstack([[1] * half, [0] * halfplus])
    return np.array(list(np.vstack([m1, m2])) * pairs)


CONFIGS = [
    # name, D, layers_t, layers_s, prior kind, df, coupling pairs, prior_param scale
    ('d1', 1, [[1, 10], [10, 1]], [[1, 10], [10, 1]], 'mf_gaussian', 0, 3, 0.0),
    ('d3', 3, [[3, 10], [10, 3]], [[3, 10], [10, 3]], 'mf_gaussian', 0, 3, 0.0),
    ('d4', 4, [[4, 8], [8, 8], [8, 4]], [[4, 6], [6, 5], [5, 4]], 'mf_student_t', 5.0, 2, 0.3),
]


def generate(out_dir):
    rng = np.random.RandomState(452)
    names = []
    _ref_stubs.STATE['model'] = _AnyDerivative()
    for name, D, lt, ls, pkind, df, pairs, pscale in CONFIGS:
        for mkind in ('gauss_diag', 'funnel'):
            if mkind == 'funnel' and D < 2:
                continue
            for N in (1, 7, 64):
                seed = 1
                prior = (ref_approx.MFGaussian(D, seed=seed) if pkind == 'mf_gaussian'
                         else ref_approx.MFStudentT(D, df, seed=seed))
                prior_param = pscale * rng.randn(2 * D)
                mask = half_masks(D, pairs)
                approx = ref_approx.NVPFlow(lt, ls, mask, prior, prior_param, D)
                theta = rng.randn(approx.var_param_dim) / 100
                log_p, mspec = log_p_of(mkind, D, rng)
                st0 = prior._rs.get_state()
                z0 = prior.sample(prior_param, N)
                prior._rs.set_state(st0)
                sample = approx.sample(theta, N)
                log_q = approx.log_density(theta, sample)
                prior._rs.set_state(st0)

                def hook():
                    prior._rs.set_state(st0)
                objective = ref_obj.ExclusiveKL(approx, log_p, N, use_path_deriv=True)
                _ref_stubs.STATE['before_eval'] = hook
                value, grad_fd = objective(theta)
                _ref_stubs.STATE['before_eval'] = None
                st1 = prior._rs.get_state()
                fname = 'nvp_%s_%s_n%d' % (name, mkind, N)
                np.savez(os.path.join(out_dir, fname + '.npz'), dim=D, layers_t=np.array(lt), layers_s=np.array(ls),
                         prior_kind=pkind, df=float(df), prior_param=prior_param, masks=mask.astype(float),
                         seed=seed, n=N, theta=theta, z0=z0, sample=sample, log_density=log_q, value=value,
                         grad_fd=grad_fd, rs_key_after=st1[1], rs_pos_after=st1[2], **mspec,
                         provenance='reference NVPFlow sample / log_density and ExclusiveKL(use_path_deriv=True) '
                                    'closure; grad_fd: Richardson central differences of that closure with the '
                                    "prior's generator restored before every evaluation")
                names.append(fname)
    return names


def compare(fresh_dir, names):
    problems = []
    for name in names:
        old = os.path.join(HERE, name + '.npz')
        if not os.path.exists(old):
            problems.append('%s: not committed' % name)
            continue
        a, b = np.load(os.path.join(fresh_dir, name + '.npz')), np.load(old)
        if set(a.files) != set(b.files):
            problems.append('%s: keys differ' % name)
            continue
        for k in a.files:
            if a[k].shape != b[k].shape or not np.array_equal(a[k], b[k]):
                problems.append('%s[%s] differs' % (name, k))
    return problems


if __name__ == '__main__':
    if sys.argv[1:] == ['--check']:
        with tempfile.TemporaryDirectory() as tmp:
            names = generate(tmp)
            diffs = compare(tmp, names)
            if _golden.fixture_digests(tmp) != _golden.read_digests(DIGESTS):
                diffs.append('digests.json: does not match the regenerated fixtures')
        for d in diffs:
            print('DRIFT ' + d)
        print('checked %d fixtures: %s' % (len(names), 'no drift' if not diffs else '%d differences' % len(diffs)))
        sys.exit(1 if diffs else 0)
    for f in os.listdir(HERE):
        if f.endswith('.npz'):
            os.remove(os.path.join(HERE, f))
    names = generate(HERE)
    _golden.write_digests(_golden.fixture_digests(HERE), DIGESTS)
    print('wrote %d fixtures to %s' % (len(names), HERE))
