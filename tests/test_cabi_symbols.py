"""CPU-side checks of the C-ABI boundary: the library loads and exports every declared symbol."""
import os
import re

import pytest

from viabel_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def _declared_symbols():
    text = open(os.path.join(ROOT, 'include', 'viabel_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(vb_[a-z_0-9]+)\s*\(', text)))


def test_header_symbols_exported(lib):
    names = _declared_symbols()
    assert len(names) >= 20
    for name in names:
        assert hasattr(lib, name), 'libviabel_hip.so does not export %s' % name


def test_binding_covers_header(lib):
    assert sorted(_lib.SIGNATURES) == _declared_symbols()


_PROBE_HEAD = r'''
#include <cstdio>
#include <type_traits>
#include "viabel_hip.h"
template <class T> void one() {          // " pointer,floating,signed,size,pointee-is-char" of one type (void: all zero)
    if constexpr (std::is_void_v<T>) {
        std::printf(" 0,0,0,0,0");
    } else {
        using pointee = std::remove_cv_t<std::remove_pointer_t<T>>;
        std::printf(" %d,%d,%d,%d,%d", int(std::is_pointer_v<T>), int(std::is_floating_point_v<T>),
                    int(std::is_signed_v<T>), int(sizeof(T)), int(std::is_pointer_v<T> && std::is_same_v<pointee, char>));
    }
}
template <class R, class... A> void show(const char* name, R (*)(A...)) {
    std::printf("%s", name);
    one<R>();
    (one<A>(), ...);
    std::printf("\n");
}
int main() {
'''


def _binding_shape(t):
    """(pointer, floating, signed, size, pointee-is-char) of a ctypes type as the probe prints a C type; ``signed`` is
    None where the comparison does not look at it (pointers, floating point)."""
    import ctypes
    if t is None:
        return (0, 0, 0, 0, 0)
    code = getattr(t, '_type_', None)
    if not isinstance(code, str) or code in 'Pz':        # POINTER(T), a CFUNCTYPE, c_void_p, c_char_p
        return (1, 0, None, ctypes.sizeof(ctypes.c_void_p), int(t is ctypes.c_char_p))
    if code in 'fdg':
        return (0, 1, None, ctypes.sizeof(t), 0)
    return (0, 0, int(t(-1).value < 0), ctypes.sizeof(t), 0)


def test_binding_matches_compiler(tmp_path):
    """What the host C++ compiler makes of every declaration in the header -- argument count, then per argument pointer /
    integer / floating point, size and integer signedness -- is what SIGNATURES tells ctypes.  The compiler reads the
    header itself: nothing here goes through the parser of ``_lib``."""
    import shutil
    import subprocess
    cxx = next((p for p in map(shutil.which, ('c++', 'g++', 'clang++')) if p), None)
    if cxx is None:
        pytest.skip('no host C++ compiler')
    names = _declared_symbols()
    assert len(names) >= 131
    source = _PROBE_HEAD + ''.join('    show("%s", decltype(&%s)(nullptr));\n' % (n, n) for n in names) + '    return 0;\n}\n'
    (tmp_path / 'probe.cpp').write_text(source)
    exe = str(tmp_path / 'probe')
    subprocess.run([cxx, '-std=c++17', '-I', os.path.join(ROOT, 'include'), '-o', exe, str(tmp_path / 'probe.cpp')],
                   check=True)
    out = subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout
    compiled = {}
    for line in out.splitlines():
        name, *types = line.split()
        compiled[name] = [tuple(int(v) for v in t.split(',')) for t in types]
    assert sorted(compiled) == names == sorted(_lib.SIGNATURES)
    for name in names:
        restype, argtypes = _lib.SIGNATURES[name]
        ret, *args = compiled[name]
        assert len(argtypes) == len(args), '%s: the binding passes %d arguments, the header declares %d' % (
            name, len(argtypes), len(args))
        for index, (bound, seen) in enumerate([(restype, ret)] + list(zip(argtypes, args)), start=-1):
            where = '%s, %s' % (name, 'return type' if index < 0 else 'parameter %d' % index)
            want = _binding_shape(bound)
            assert want[:2] == seen[:2], '%s: pointer / floating-point class differs: %r binds %r' % (where, seen, bound)
            assert want[3] == seen[3], '%s: %d bytes in the header, %r in the binding' % (where, seen[3], bound)
            assert want[4] == seen[4], '%s: char pointer in one, not the other: %r' % (where, bound)
            if want[2] is not None:
                assert want[2] == seen[2], '%s: integer signedness differs: %r' % (where, bound)


# every integer #define of include/viabel_hip.h as _lib exposes it (VB_ prefix dropped; the status codes under both
# names).  The values are ABI: a change here is a change of the library's contract.
_PINNED = {
    'OK': 0, 'ERR_INVALID': 1, 'ERR_HIP': 2, 'ERR_UNSUPPORTED': 3, 'ERR_STATE': 4, 'ERR_NUMERIC': 5, 'ERR_COMM': 6,
    'ERR_CALLBACK': 7,
    'VB_OK': 0, 'VB_ERR_INVALID': 1, 'VB_ERR_HIP': 2, 'VB_ERR_UNSUPPORTED': 3, 'VB_ERR_STATE': 4, 'VB_ERR_NUMERIC': 5,
    'VB_ERR_COMM': 6, 'VB_ERR_CALLBACK': 7,
    'FAMILY_MF_GAUSSIAN': 0, 'FAMILY_MF_STUDENT_T': 1, 'FAMILY_FULLRANK_GAUSSIAN': 2, 'FAMILY_MULTIVARIATE_T': 3,
    'FAMILY_LOWRANK_GAUSSIAN': 4,
    'MODEL_GAUSS_DIAG': 0, 'MODEL_FUNNEL': 1, 'MODEL_GAUSS_FULL': 2, 'MODEL_LOGISTIC': 3, 'MODEL_SOURCE': 4,
    'MODEL_SOFTMAX': 5, 'MODEL_MULTILEVEL': 6, 'MODEL_LOCSCALE': 7, 'MODEL_SPARSE_GLM': 8, 'MODEL_MINIBATCH_GLM': 9,
    'MODEL_NEURALNET': 10,
    'LOCSCALE_GAUSSIAN': 0, 'LOCSCALE_STUDENT_T': 1,
    'GLM_BERNOULLI_LOGIT': 0, 'GLM_POISSON': 1, 'GLM_GAUSSIAN': 2,
    'NOISE_NORMAL': 0, 'NOISE_STUDENT_T': 1,
    'FLAG_PATH_DERIV': 1,
    'CV_NONE': 0, 'CV_FULL': 1, 'CV_MEAN_ONLY': 2, 'CV_LOO_DIAG': 3, 'CV_LOO_DIRECT': 4,
    'MAX_SLOTS': 64,
    'PRIOR_DIAG_GAUSSIAN': 0, 'PRIOR_DIAG_STUDENT_T': 1, 'PRIOR_DENSE': 2,
    'HMC_METRIC_DIAG': 0, 'HMC_METRIC_DENSE': 1,
    'OPT_SGD': 0, 'OPT_RMSPROP': 1, 'OPT_ADAM': 2, 'OPT_ADAGRAD': 3,
    'COMM_ID_BYTES': 128, 'HOST_SUM': 0, 'HOST_MAX': 1, 'IPC_HANDLE_BYTES': 64,
    'PROF_MF_ACCUM': 0, 'PROF_FR_SAMPLE_GEMM': 1, 'PROF_FR_MODEL_GEMM': 2, 'PROF_FR_GRAD_GEMM': 3, 'PROF_NUM': 4,
    'FR_FOLD_MIN_D': 1024, 'FR_FOLD_MIN_ROWS_PER_D': 3,
}


def test_constants_pinned():
    for name, value in _PINNED.items():
        assert getattr(_lib, name, None) == value and type(getattr(_lib, name)) is int, name
    assert _lib.CV_MODES == {None: 0, 'full': 1, 'mean_only': 2, 'loo_diag_approx': 3, 'loo_direct_approx': 4}
    assert _lib.Engine.IPC_HANDLE_BYTES == 64
    # nothing the header defines is missing from the pins
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'viabel_hip.h')).read(), flags=re.S)
    defined = re.findall(r'^\s*#\s*define\s+VB_(\w+)\s+\d', header, flags=re.M)
    assert sorted(defined) == sorted(k for k in _PINNED if not k.startswith('VB_'))


def test_version_and_error_text(lib):
    assert lib.vb_version().decode().startswith('viabel_hip')
    assert isinstance(lib.vb_last_error(None), bytes)


def test_no_gpu_fails_loudly():
    """Without a GPU the engine must raise, never fall back to a CPU path."""
    import ctypes
    n = ctypes.c_int(0)
    lib = _lib.load()
    rc = lib.vb_device_count(ctypes.byref(n))
    if rc == 0 and n.value > 0:
        pytest.skip('a GPU is visible')
    with pytest.raises(_lib.EngineError):
        _lib.Engine(0)
    import numpy as np
    import viabel_amd as vb
    _lib.set_default_engine(None)
    obj = vb.ExclusiveKL(vb.MFGaussian(4), vb.GaussianModel(np.zeros(4), np.ones(4)), 8)
    with pytest.raises(_lib.EngineError):
        obj(np.zeros(8))
