"""Helpers shared by the oracle tests and the GPU parity tests: load fixtures, rebuild specs."""
import glob
import hashlib
import json
import os

import numpy as np

from oracle import families as ofam
from oracle import models as omod

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
# sha256 of every fixture's arrays as make_golden.py wrote them from the reference's own code
DIGESTS_PATH = os.path.join(GOLDEN_DIR, 'digests.json')


def fixtures(prefix):
    paths = sorted(glob.glob(os.path.join(GOLDEN_DIR, prefix + '*.npz')))
    assert paths, 'no golden fixtures named %s*' % prefix
    return paths


def load(path):
    with np.load(path, allow_pickle=False) as z:
        return {k: (z[k].item() if z[k].ndim == 0 else z[k]) for k in z.files}


def oracle_family(fx):
    kind, D = str(fx['family_kind']), int(fx['dim'])
    if kind == 'mf_gaussian':
        return ofam.MFGaussian(D)
    if kind == 'mf_student_t':
        return ofam.MFStudentT(D, float(fx['df']))
    if kind == 'multivariate_t':
        return ofam.MultivariateT(D, float(fx['df']))
    if kind == 'lr_gaussian':
        return ofam.LRGaussian(D, int(fx['rank']))
    raise ValueError(kind)


def oracle_prior_family(fx):
    """The tempering prior of a `disprior_*` fixture as an oracle family."""
    kind, D = str(fx['prior_kind']), int(fx['dim'])
    if kind == 'mf_student_t':
        return ofam.MFStudentT(D, float(fx['prior_df']))
    if kind == 'multivariate_t':
        return ofam.MultivariateT(D, float(fx['prior_df']))
    if kind == 'lr_gaussian':
        return ofam.LRGaussian(D, int(fx['prior_rank']))
    raise ValueError(kind)


def oracle_model(fx):
    kind = str(fx['model_kind'])
    if kind == 'gauss_diag':
        return omod.GaussDiag(fx['model_mean'], fx['model_stdev'])
    if kind == 'funnel':
        return omod.Funnel(int(fx['dim']), int(fx['model_scale_index']),
                           float(fx['model_log_sigma_stdev']))
    raise ValueError(kind)


def noise_of(fx):
    if 'noise' in fx:
        return fx['noise']
    if 'noise_eps' in fx:                      # LRGaussian: low-rank block first (approximations.py:639-640)
        return fx['noise_z'], fx['noise_eps']
    return fx['noise_chi'], fx['noise_z']


def rel_err(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def ids(paths):
    return [os.path.splitext(os.path.basename(p))[0] for p in paths]


def fixture_digest(path):
    """sha256 over a fixture's arrays (names, dtypes, shapes, bytes in key order): independent of the zip container,
    whose member timestamps change with every write."""
    h = hashlib.sha256()
    with np.load(path, allow_pickle=False) as z:
        for k in sorted(z.files):
            a = np.ascontiguousarray(z[k])
            h.update(('%s|%s|%s|' % (k, a.dtype.str, a.shape)).encode())
            h.update(a.tobytes())
    return h.hexdigest()


def fixture_digests(directory=GOLDEN_DIR):
    """{fixture name: digest} of every ``*.npz`` in ``directory``."""
    return {os.path.basename(p)[:-4]: fixture_digest(p) for p in sorted(glob.glob(os.path.join(directory, '*.npz')))}


def write_digests(digests, path=DIGESTS_PATH):
    with open(path, 'w') as f:
        json.dump(digests, f, indent=1, sort_keys=True)
        f.write('\n')


def read_digests(path=DIGESTS_PATH):
    with open(path) as f:
        return json.load(f)
