"""CPU: the environment variables the library reads are exactly the listed ones, and each is documented.

Every quoted ``VB_*`` / ``VIABEL_AMD_*`` string literal in the library's sources (``viabel_amd/``, ``include/``) counts as
a variable it reads.  The kept set is three kinds: switches a test sets to reach a second route and compare it with the
default one, product configuration, and pure diagnostics.  A new switch has to be added here, and to README.md or
INTEGRATION.md, on purpose."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# switches that tests set to compare two routes
TESTED = {
    'VB_DIS_BISECT', 'VB_DIS_RESIDENT', 'VB_DIS_ROUNDS', 'VB_FETCH_FLAGSYNC', 'VB_FIT_STREAM_MIN_BYTES',
    'VB_FIT_STREAM_ROWS', 'VB_FR_FUSED', 'VB_GRAM_XCD', 'VB_LEGACY_AHEAD', 'VB_LEGACY_BUDGET_SCALE',
    'VB_MF_ONE', 'VB_MVT_CHAIN', 'VB_MVT_CHAIN_FETCH', 'VB_MVT_DIRECT', 'VB_MVT_EPI_ROWS', 'VB_MVT_FLAGSYNC',
    'VB_MVT_FUSED_ROWS', 'VB_MVT_SIDE_INVERSE', 'VB_MVT_UNPACK', 'VB_NOISE_AHEAD', 'VB_NS_HINT', 'VB_PSIS_FUSED_IO',
    'VB_PSIS_GRID',
}
# product configuration
CONFIG = {
    'VB_IPC_POLL_LOG2', 'VB_IPC_TIMEOUT_S', 'VIABEL_AMD_CHECK_POINTERS', 'VIABEL_AMD_CONTROL_PORT',
    'VIABEL_AMD_HOST_BLAS_THREADS', 'VIABEL_AMD_IPC_DOUBLES', 'VIABEL_AMD_JOB_ID', 'VIABEL_AMD_LIB',
    'VIABEL_AMD_NO_GLIBC_LOG', 'VIABEL_AMD_RNG_THREADS', 'VIABEL_AMD_TRANSPORT',
}
# diagnostics: they only report, the computation is the same
DIAGNOSTICS = {'VB_DIS_TRACE', 'VB_FUSED_CLOCK_DUMP', 'VB_PSIS_TRACE'}

KEPT = TESTED | CONFIG | DIAGNOSTICS

_LITERAL = re.compile(r'''["']((?:VB|VIABEL_AMD)_[A-Z0-9_]+)["']''')


def _sources():
    files = []
    for ext in ('hip', 'h', 'cpp', 'py'):
        files += glob.glob(os.path.join(ROOT, 'viabel_amd', '**', '*.' + ext), recursive=True)
    files += [p for p in glob.glob(os.path.join(ROOT, 'include', '**', '*'), recursive=True) if os.path.isfile(p)]
    return sorted(files)


def read_names():
    names = set()
    for path in _sources():
        with open(path, encoding='utf-8', errors='replace') as f:
            names.update(_LITERAL.findall(f.read()))
    return names


def test_kept_set_is_37_distinct_names():
    assert len(TESTED) + len(CONFIG) + len(DIAGNOSTICS) == len(KEPT) == 37


def test_library_reads_exactly_the_kept_switches():
    names = read_names()
    assert not names - KEPT, 'unlisted environment variables: %s' % sorted(names - KEPT)
    assert not KEPT - names, 'listed but no longer read: %s' % sorted(KEPT - names)


def test_every_kept_switch_is_documented():
    docs = ''
    for name in ('README.md', 'INTEGRATION.md'):
        with open(os.path.join(ROOT, name), encoding='utf-8') as f:
            docs += f.read()
    missing = [v for v in sorted(KEPT) if not re.search(r'(?<![A-Z0-9_])%s(?![A-Z0-9_])' % v, docs)]
    assert not missing, 'not in README.md or INTEGRATION.md: %s' % missing
