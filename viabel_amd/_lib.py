"""ctypes binding of ``libviabel_hip.so`` (the C ABI in ``include/viabel_hip.h``).

The shared library is the product: there is no CPU fallback.  If it is missing, or
no MI355X is visible, every compute call raises -- loudly -- instead of silently
computing something else.
"""
import ctypes
import re
import weakref
import os
import subprocess
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# VIABEL_AMD_LIB: load another build of the same C ABI (the host-sanitizer build libviabel_hip_asan.so, `make asan`)
LIB_PATH = os.environ.get('VIABEL_AMD_LIB') or os.path.join(_HERE, 'libviabel_hip.so')
CSRC_DIR = os.path.join(_HERE, 'csrc')
# the declaration of the C ABI (what csrc/Makefile compiles against): the one source of SIGNATURES and of the VB_* constants
HEADER_PATH = os.path.join(os.path.dirname(_HERE), 'include', 'viabel_hip.h')


class EngineError(RuntimeError):
    """The HIP engine is unavailable or a HIP call failed."""


# `const double*` / `double*` parameters are declared void*: ctypes then takes the array's address as a plain integer
# (`_dptr`), half the cost of building a POINTER(c_double) per argument on calls that last tens of microseconds
_c_double_p = ctypes.c_void_p
_c_int64_p = ctypes.POINTER(ctypes.c_int64)
_ctx_p = ctypes.c_void_p

# The binding's type rule.  What the header declares decides the ctypes type; a type outside the rule is an error.
#   int, unsigned, double, int64_t, uint64_t, uint32_t, size_t      the ctypes scalar of that type
#   double*, const double*                                          c_void_p, always: the hot path passes integer addresses
#   vb_ctx*, vb_flow*, vb_legacy_rng*, void*, the callback typedefs  c_void_p
#   char*, char x[N], const char*                                   c_char_p
#   T*, T x[N] for the integer types above                          POINTER(T)
#   T**                                                             POINTER(c_void_p)
#   return void                                                     None
_SCALARS = {'int': ctypes.c_int, 'unsigned': ctypes.c_uint, 'double': ctypes.c_double, 'int64_t': ctypes.c_int64,
            'uint64_t': ctypes.c_uint64, 'uint32_t': ctypes.c_uint32, 'size_t': ctypes.c_size_t}
_OPAQUE = ('vb_ctx', 'vb_flow', 'vb_legacy_rng', 'void')
_CALLBACKS = ('vb_model_callback', 'vb_host_collective_fn')
_COMMENT = re.compile(r'/\*.*?\*/', re.S)
_DEFINE = re.compile(r'^[ \t]*#[ \t]*define[ \t]+VB_(\w+)[ \t]+(\d+)u?[ \t]*$', re.M)
_NOT_DECLARATIONS = re.compile(r'^[ \t]*#.*$|extern\s+"C"\s*\{|\}', re.M)
_FUNCTION = re.compile(r'(.+?)\b(vb_\w+)\s*\((.*)\)', re.S)
_TYPE = re.compile(r'(?:const\s+)?(\w+)\s*(\**)\s*(?:\w+\s*(\[\w*\])?)?')       # [const] base [*...] [name [[N]]]


def _ctype(text, where):
    m = _TYPE.fullmatch(text.strip())
    if m:
        base, depth = m.group(1), len(m.group(2)) + (m.group(3) is not None)
        if depth == 0 and base in _SCALARS:
            return _SCALARS[base]
        if (depth == 0 and base in _CALLBACKS) or (depth == 1 and (base == 'double' or base in _OPAQUE)):
            return ctypes.c_void_p
        if depth == 1 and base == 'char':
            return ctypes.c_char_p
        if depth == 1 and base in _SCALARS:
            return ctypes.POINTER(_SCALARS[base])
        if depth == 2 and base in _OPAQUE:
            return ctypes.POINTER(ctypes.c_void_p)
    raise EngineError('%s: %s: the type of `%s` is outside the binding\'s type rule (viabel_amd/_lib.py)'
                      % (HEADER_PATH, where, ' '.join(text.split())))


def _parse_header(path):
    """``(signatures, constants)`` of the C header at ``path``: ``name -> (restype, argtypes)`` for every function it
    declares, ``NAME -> value`` for every ``#define VB_NAME <integer>``."""
    try:
        with open(path) as f:
            text = _COMMENT.sub(' ', f.read())
    except OSError as exc:
        raise EngineError('cannot read the C ABI header %s: %s' % (path, exc))
    constants = {name: int(value) for name, value in _DEFINE.findall(text)}
    signatures = {}
    for decl in _NOT_DECLARATIONS.sub('', text).split(';'):
        decl = decl.strip()
        if not decl or decl.startswith('typedef'):
            continue
        m = _FUNCTION.fullmatch(decl)
        if not m:
            raise EngineError('%s: not a function declaration the binding can read: `%s`' % (path, ' '.join(decl.split())))
        restype, name, params = m.groups()
        params = [] if params.strip() in ('', 'void') else params.split(',')
        signatures[name] = (None if restype.strip() == 'void' else _ctype(restype, name + ', return type'),
                            [_ctype(p, '%s, parameter %d' % (name, i)) for i, p in enumerate(params)])
    return signatures, constants


# name -> (restype, argtypes) of every symbol include/viabel_hip.h declares, and its integer constants without their VB_
# prefix (FAMILY_*, MODEL_*, GLM_*, NOISE_*, CV_*, OPT_*, PRIOR_*, HMC_METRIC_*, PROF_*, MAX_SLOTS, ...) as module attributes
SIGNATURES, _CONSTANTS = _parse_header(HEADER_PATH)
globals().update(_CONSTANTS)
# the status codes keep the prefix as well: the package says VB_OK, VB_ERR_INVALID
globals().update({'VB_' + name: value for name, value in _CONSTANTS.items() if name == 'OK' or name.startswith('ERR_')})

# targets that hand every pipeline finished rows (f, grad f): a softmax, multilevel, location-scale or sparse regression
# target goes wherever a source model goes; the minibatch target forms its rows the same way (the objectives decide what
# may take a density that changes from batch to batch)
MODELS_WITH_ROWS = (MODEL_SOURCE, MODEL_SOFTMAX, MODEL_MULTILEVEL, MODEL_LOCSCALE, MODEL_SPARSE_GLM, MODEL_MINIBATCH_GLM,
                    MODEL_NEURALNET)
# doubles of predictor matrix one row chunk of the softmax pipeline may hold (csrc/vb_common.h: kSoftmaxChunkDoubles);
# a chunk is max(8, SOFTMAX_CHUNK_DOUBLES // (n_classes * round_up(n_data, 16))) rows
SOFTMAX_CHUNK_DOUBLES = 16 << 20
# ... and of the multilevel pipeline (kMultilevelChunkDoubles): a chunk is max(8, MULTILEVEL_CHUNK_DOUBLES //
# round_up(n_data, 16)) rows
MULTILEVEL_CHUNK_DOUBLES = 16 << 20
# ... and of the location-scale pipeline (kLocScaleChunkDoubles), whose two predictor matrices share the bound: a chunk is
# max(8, LOCSCALE_CHUNK_DOUBLES // (2 * round_up(n_data, 16))) rows
LOCSCALE_CHUNK_DOUBLES = 16 << 20
# entries of a row or column of a sparse design that one wave sums (csrc/vb_common.h: kSparseSegment); longer lists are cut
# into segments of this many entries, summed by separate waves and combined in segment order
SPARSE_SEGMENT = 256
# doubles of workspace per chunk of samples of the sparse pipeline (kSparseChunkDoubles)
SPARSE_CHUNK_DOUBLES = 16 << 20


def sparse_chunk_rows(n_data, p):
    """Samples per chunk of the sparse regression pipeline for an ``(n_data, p)`` design: the arithmetic of
    ``sparse_chunk_rows`` in ``csrc/vb_common.h``."""
    return min(8192, max(64, SPARSE_CHUNK_DOUBLES // (2 * (int(n_data) + int(p))) // 64 * 64))


# doubles of the term and the residual matrix together per chunk of samples of the minibatch pipeline (kMinibatchChunkDoubles)
MINIBATCH_CHUNK_DOUBLES = 16 << 20


def minibatch_chunk_rows(batch_size):
    """Samples per chunk of the minibatch regression pipeline for batches of ``batch_size`` observations: the arithmetic of
    ``minibatch_chunk_rows`` in ``csrc/vb_common.h``."""
    return max(8, MINIBATCH_CHUNK_DOUBLES // (2 * ((int(batch_size) + 15) // 16 * 16)))


# doubles of the hidden-unit matrix per chunk of samples of the neural-network pipeline (kNeuralNetChunkDoubles), and of the
# matrix of hidden pre-activations per chunk of OBSERVATIONS of vb_nn_predict (kNeuralNetPredictDoubles)
NN_CHUNK_DOUBLES = 16 << 20
NN_PREDICT_DOUBLES = 16 << 20


def nn_chunk_rows(n_hidden, n_data):
    """Samples per chunk of the neural-network pipeline: a sample holds ``n_hidden * round_up(n_data, 16)`` doubles of the
    hidden-unit matrix (``csrc/vb_common.h``: kNeuralNetChunkDoubles; a call of fewer samples is one chunk)."""
    return max(8, NN_CHUNK_DOUBLES // (int(n_hidden) * ((int(n_data) + 15) // 16 * 16)))


def nn_predict_chunk(n_hidden, n_draws):
    """Observations per chunk of ``vb_nn_predict``: an observation holds ``n_hidden * round_up(n_draws, 16)`` doubles
    (``csrc/vb_common.h``: kNeuralNetPredictDoubles)."""
    return max(1, NN_PREDICT_DOUBLES // (int(n_hidden) * ((int(n_draws) + 15) // 16 * 16)))


# doubles of the term matrix per row chunk of the flat regression target's row entries (csrc/vb_rows.hip:
# kGlmRowsLogpDoubles of vb_model_logp, kGlmRowsGradDoubles of vb_model_grad) and the fewest rows of a chunk (kGlmRowsMinChunk)
GLM_ROWS_LOGP_DOUBLES = 64 << 20
GLM_ROWS_GRAD_DOUBLES = 32 << 20
GLM_ROWS_MIN_CHUNK = 128


def glm_rows_chunk(n_data, grad):
    """Rows per chunk of ``vb_model_grad`` (``grad``) or ``vb_model_logp`` on a flat regression target of ``n_data``
    observations; a call of fewer rows is one chunk.  Must equal the chunk arithmetic of ``model_grad_rows`` and
    ``logistic_rows`` in ``csrc/vb_rows.hip``."""
    doubles = GLM_ROWS_GRAD_DOUBLES if grad else GLM_ROWS_LOGP_DOUBLES
    return max(GLM_ROWS_MIN_CHUNK, doubles // ((int(n_data) + 15) // 16 * 16))


def glm_grad_splits(rows, d, n_data, n_cu):
    """Slabs into which the gradient product ``[rows x d x n_data]`` of one row chunk splits its observations on a device
    of ``n_cu`` compute units (1: one launch that writes the gradient itself).  Must equal ``glm_grad_splits`` in
    ``csrc/vb_rows.hip``."""
    tiles = ((int(rows) + 63) // 64) * ((int(d) + 63) // 64)
    if tiles >= n_cu:
        return 1
    return max(1, min(2 * int(n_cu) // tiles, int(n_data) // 128, 64))


KSD_MAX_DRAWS = 65536      # capacity of vb_ksd (csrc/vb_ksd.hip: kKsdMaxDraws)


def ksd_plan(s, n_cu):
    """``(row blocks, column splits)`` of the pair kernel of ``vb_ksd`` for ``s`` draws on a device of ``n_cu`` compute
    units (``vb_ksd_plan``: the host function the launch uses; no GPU needed).  ``ValueError`` for what it rejects."""
    out = (ctypes.c_int * 2)()
    if load().vb_ksd_plan(int(s), int(n_cu), out) != VB_OK:
        raise ValueError('ksd_plan needs 1 <= s <= {} and n_cu >= 1; got s = {}, n_cu = {}'.format(KSD_MAX_DRAWS, s, n_cu))
    return int(out[0]), int(out[1])


def gemm_plan(m, n, k, splits=1, n_cu=256, tri_mode=0, batch=0, a_kcontig=True, narrow_ok=None, narrow_auto=None, cfg=0,
              flags=0):
    """What the fp64 GEMM launcher decides for an ``m x n`` product of contraction length ``k`` in ``splits`` k pieces on a
    device of ``n_cu`` compute units (``vb_gemm_plan``: the host function the launcher calls; no GPU needed): a dict of
    ``cfg`` (1 .. 8), ``dma`` (the LDS-DMA kernel, else the register-staged one), ``bm_rows``, ``bn_cols``, ``k_split``
    and ``grid_x``.  ``narrow_ok`` and ``narrow_auto`` default to what a plain-store epilogue gives: ``a_kcontig``.
    ``ValueError`` for what the function rejects."""
    narrow_ok = bool(a_kcontig) if narrow_ok is None else bool(narrow_ok)
    narrow_auto = narrow_ok if narrow_auto is None else bool(narrow_auto)
    out = (ctypes.c_int * 6)()
    args = (int(m), int(n), int(k), int(splits), int(n_cu), int(tri_mode), int(batch), int(bool(a_kcontig)), int(narrow_ok),
            int(narrow_auto), int(cfg), int(flags))
    if load().vb_gemm_plan(*args, out) != VB_OK:
        raise ValueError('gemm_plan rejects (m, n, k, splits, n_cu, tri_mode, batch, a_kcontig, narrow_ok, narrow_auto, cfg, '
                         'flags) = {}'.format(args))
    return {'cfg': int(out[0]), 'dma': bool(out[1]), 'bm_rows': int(out[2]), 'bn_cols': int(out[3]), 'k_split': int(out[4]),
            'grid_x': int(out[5])}


def gram_splits(d, n, n_cu):
    """k splits of the lower-tile Gram product of an ``n x d`` matrix on a device of ``n_cu`` compute units
    (``vb_gram_splits_plan``: the rule behind ``Engine.noise_moments``)."""
    out = ctypes.c_int(0)
    if load().vb_gram_splits_plan(int(d), int(n), int(n_cu), ctypes.byref(out)) != VB_OK:
        raise ValueError('gram_splits needs d, n, n_cu >= 1; got {}'.format((d, n, n_cu)))
    return int(out.value)


def lowrank_splits(n):
    """k splits of the low-rank family's products over ``n`` samples (``vb_lowrank_splits_plan``: the rule behind
    ``Engine.lowrank_path_terms``)."""
    out = ctypes.c_int(0)
    if load().vb_lowrank_splits_plan(int(n), ctypes.byref(out)) != VB_OK:
        raise ValueError('lowrank_splits needs n >= 1; got {}'.format(n))
    return int(out.value)


def ksd_split_tiles(tiles, splits):
    """The column tiles ``[first, last)`` of every split of the pair kernel: the rule of ``vb_ksd_plan`` in
    ``include/viabel_hip.h`` (split ``k`` of ``n`` takes ``[k * tiles // n, (k + 1) * tiles // n)``)."""
    return [(k * int(tiles) // int(splits), (k + 1) * int(tiles) // int(splits)) for k in range(int(splits))]


def _pair_arguments(x, scores, scale, entry, noun, axis, cap, log_w=None):
    """What :func:`ksd_arguments` and :func:`svgd_arguments` share, in the order both report it: ``x`` (two axes, at most
    ``cap`` rows, finite), ``scores`` (the shape of ``x``, finite), ksd's ``log_w`` and ``scale`` (one positive finite
    entry per column).  ``noun`` and ``axis`` name the rows in the messages.  Returns ``(x, scores, log_w, scale)``."""
    x = _f64(x)
    if x.ndim != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError('x must be ({0}, D) with {0} >= 1 and D >= 1; got shape {1}'.format(axis, x.shape))
    n, d = x.shape
    if n > cap:
        raise NotImplementedError('{} takes at most {} {}; got {}'.format(entry, cap, noun, n))
    if not np.all(np.isfinite(x)):
        raise ValueError('the {} must be finite'.format(noun))
    if scores is not None:
        scores = _f64(scores)
        if scores.shape != (n, d):
            raise ValueError('scores must have the shape of x, {}; got {}'.format((n, d), scores.shape))
        if not np.all(np.isfinite(scores)):
            raise ValueError('the scores must be finite')
    if log_w is not None:
        if np.shape(log_w) != (n,):
            raise ValueError('log_w must have shape ({},)'.format(n))
        log_w = _f64(log_w)
        if np.any(np.isnan(log_w)) or np.any(log_w == np.inf) or not np.any(np.isfinite(log_w)):
            raise ValueError('no log weight is finite (or one is NaN or +inf)')
    if scale is not None:
        if np.shape(scale) != (d,):
            raise ValueError('scale must have shape ({},)'.format(d))
        scale = _f64(scale)
        if not np.all(np.isfinite(scale) & (scale > 0.0)):
            raise ValueError('scale must be positive and finite')
    return x, scores, log_w, scale


def ksd_arguments(x, scores=None, log_w=None, scale=None, c=1.0, beta=-0.5):
    """The arguments of ``vb_ksd`` checked and made contiguous doubles: ``(x, scores, log_w, scale, c, beta)``.
    ``ValueError`` for a wrong shape, non-finite draws or scores, no finite log weight, a scale that is not positive and
    finite, ``c`` not positive and finite and ``beta`` outside (-1, 0); ``NotImplementedError`` for more than
    ``KSD_MAX_DRAWS`` draws.  Touches no engine."""
    c, beta = float(c), float(beta)
    if not (c > 0.0 and np.isfinite(c)):
        raise ValueError('c must be positive and finite')
    if not (-1.0 < beta < 0.0):
        raise ValueError('beta must lie in (-1, 0)')
    x, scores, log_w, scale = _pair_arguments(x, scores, scale, 'ksd', 'draws', 'S', KSD_MAX_DRAWS, log_w)
    return x, scores, log_w, scale, c, beta


SVGD_MAX_PARTICLES = 8192      # capacity of vb_svgd_direction / vb_svgd_run (csrc/vb_svgd.hip: kSvgdMaxParticles)


def svgd_arguments(x, scores=None, scale=None, bandwidth='median'):
    """The arguments of ``vb_svgd_direction`` / ``vb_svgd_run`` checked and made contiguous doubles:
    ``(x, scores, scale, bandwidth)`` with ``bandwidth`` as the C entries take it (0.0: the median rule).  ``ValueError``
    for a wrong shape, non-finite particles or scores, a scale that is not positive and finite and a bandwidth that is
    neither ``'median'`` nor positive and finite; ``NotImplementedError`` for more than ``SVGD_MAX_PARTICLES`` particles.
    Touches no engine."""
    if isinstance(bandwidth, str):
        if bandwidth != 'median':
            raise ValueError("bandwidth must be 'median' or a positive number")
        bandwidth = 0.0
    else:
        bandwidth = float(bandwidth)
        if not (bandwidth > 0.0 and np.isfinite(bandwidth)):
            raise ValueError("bandwidth must be 'median' or a positive finite number")
    x, scores, _, scale = _pair_arguments(x, scores, scale, 'svgd', 'particles', 'n', SVGD_MAX_PARTICLES)
    return x, scores, scale, bandwidth


CV_MODES = {None: CV_NONE, 'full': CV_FULL, 'mean_only': CV_MEAN_ONLY, 'loo_diag_approx': CV_LOO_DIAG,
            'loo_direct_approx': CV_LOO_DIRECT}
# capacity of the batched smoothing kernel (csrc/vb_psis_batch.hip: kPbMaxN, kPbTailCap)
PSIS_BATCH_MAX_N, PSIS_BATCH_MAX_TAIL = 16384, 1024
# int fn(void* user, const double* z, int64 n, int64 d, double* f, double* grad)   (include/viabel_hip.h: vb_model_callback)
MODEL_CALLBACK_TYPE = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_int64,
                                       ctypes.c_int64, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double))
# int fn(void* user, double* buf, size_t count, int op)   (include/viabel_hip.h: vb_host_collective_fn)
HOST_COLLECTIVE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_size_t,
                                      ctypes.c_int)

_lib = None
_lib_lock = threading.Lock()


def build(verbose=False):
    """Compile ``libviabel_hip.so`` for gfx950 with hipcc (cross-compiles without a GPU)."""
    cmd = ['make', '-C', CSRC_DIR, '-j8']
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout)
    if res.returncode != 0:
        raise EngineError('building libviabel_hip.so failed (see output above)')
    return LIB_PATH


def load():
    """Load the shared library and declare every entry point (no GPU needed for this)."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise EngineError(
                'libviabel_hip.so not found at %s: build it with '
                '`python -c "import __graft_entry__ as g; g.build()"` or `make -C viabel_amd/csrc`. '
                'There is no CPU fallback.' % LIB_PATH)
        try:
            lib = ctypes.CDLL(LIB_PATH)
        except OSError as exc:
            raise EngineError('cannot load %s: %s' % (LIB_PATH, exc))
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = restype
            fn.argtypes = argtypes
        _lib = lib
        return lib


_DPTR_CHECKS = bool(os.environ.get('VIABEL_AMD_CHECK_POINTERS'))


def _dptr(a):
    """Address of a contiguous float64 array (the caller keeps the array alive across the call: every call site
    passes a local NAME, never a temporary -- ``tests/test_host_logic.py::test_dptr_call_sites_pass_names`` enforces it,
    and ``VIABEL_AMD_CHECK_POINTERS=1`` checks dtype and contiguity on every call)."""
    if _DPTR_CHECKS:
        assert isinstance(a, np.ndarray) and a.flags.c_contiguous and a.dtype in (np.float64, np.int64, np.int32), \
            'C-ABI array argument must be a contiguous float64 / int array'
    return a.__array_interface__['data'][0]


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _root_arguments(a, e):
    """``a`` (and ``e``) as contiguous doubles for ``vb_sym_sqrt``; the C side reads ``d * d`` doubles from each, so anything
    but a non-empty square ``a`` and an ``e`` of the same shape is refused here."""
    a = _f64(a)
    if a.ndim != 2 or a.shape[0] != a.shape[1] or a.shape[0] == 0:
        raise ValueError('a must be a non-empty square matrix; got shape {}'.format(a.shape))
    if e is not None:
        e = _f64(e)
        if e.shape != a.shape:
            raise ValueError('e must have the shape of a, {}; got {}'.format(a.shape, e.shape))
    return a, e


def device_count():
    """GPUs visible to HIP (0 without one)."""
    n = ctypes.c_int(0)
    return n.value if load().vb_device_count(ctypes.byref(n)) == VB_OK else 0


def resource_counts():
    """``(device buffers, pinned blocks, events, streams)`` the engine holds in this process (``vb_resource_counts``):
    back at their earlier values once every engine, flow and parked DIS state created since has been released."""
    out = (ctypes.c_uint64 * 4)()
    if load().vb_resource_counts(out) != VB_OK:
        raise EngineError('vb_resource_counts failed')
    return tuple(int(v) for v in out)


class PinnedPool:
    """Page-locked host blocks (``vb_host_alloc``) handed out as the float64 arrays the engine RETURNS.

    The reference returns a freshly allocated gradient per call (``objectives.py:32-44``); so does this binding, but a
    4.2-MB gradient copied into pageable memory is staged by the runtime (118 us at D = 1024: 36 GB/s), while the copy
    engine writes straight into a pinned block.  ``array(n)`` is an ordinary ``ndarray`` whose memory is such a block; when
    the array (and every view of it) is gone the block returns to the free list of its size and the next call reuses it --
    an optimiser loop that drops its gradients cycles through two or three blocks.  At most ``keep`` idle blocks per size
    stay allocated; arrays smaller than ``MIN_BYTES`` are plain ``np.empty`` (the small-result path copies through the
    engine's own mapped buffer anyway)."""

    MIN_BYTES = 1 << 20
    MAX_OUTSTANDING = 1 << 30      # page-locked bytes in the callers' hands; beyond it the arrays are pageable again (a caller
                                   # that KEEPS every gradient -- FASO's history -- must not pin the host's memory)

    def __init__(self, lib, keep=4):
        self._lib, self._keep, self._free, self._out = lib, keep, {}, 0

    def array(self, n):
        nbytes = 8 * int(n)
        if nbytes < self.MIN_BYTES or self._out + nbytes > self.MAX_OUTSTANDING:
            return np.empty(n, dtype=np.float64)
        free = self._free.setdefault(nbytes, [])
        if free:
            ptr = free.pop()
        else:
            box = ctypes.c_void_p()
            if self._lib.vb_host_alloc(nbytes, ctypes.byref(box)) != VB_OK or not box.value:
                return np.empty(n, dtype=np.float64)          # (no pinned memory left: a pageable array still works)
            ptr = box.value
        buf = (ctypes.c_double * int(n)).from_address(ptr)
        fin = weakref.finalize(buf, self._give_back, nbytes, ptr)     # buf is the array's base: it dies with the last view
        fin.atexit = False      # (at interpreter exit the HIP runtime may be gone before the arrays: the OS takes the pages back)
        self._out += nbytes
        return np.frombuffer(buf, dtype=np.float64)

    def _give_back(self, nbytes, ptr):
        self._out -= nbytes
        free = self._free.setdefault(nbytes, [])
        if len(free) < self._keep:
            free.append(ptr)
        else:
            self._lib.vb_host_free(ptr)

    def idle_blocks(self):
        return sum(len(v) for v in self._free.values())


_pinned_pool = None


def pinned_array(n):
    """A float64 result array of ``n`` entries in page-locked memory (see :class:`PinnedPool`)."""
    global _pinned_pool
    if _pinned_pool is None:
        _pinned_pool = PinnedPool(load())
    return _pinned_pool.array(n)


class Engine:
    """One HIP context on one GPU (``vb_ctx``).  Calls are synchronous unless named ``*_async``."""

    def __init__(self, device=None):
        self._lib = load()
        from_env = device is None
        if from_env:
            device = int(os.environ.get('LOCAL_RANK', '0'))
        n = ctypes.c_int(0)
        rc = self._lib.vb_device_count(ctypes.byref(n))
        if rc != VB_OK or n.value == 0:
            raise EngineError('no MI355X visible to HIP (%s); the engine has no CPU fallback'
                              % self._lib.vb_last_error(None).decode())
        if from_env and device >= n.value == 1 and any(
                os.environ.get(v) for v in ('HIP_VISIBLE_DEVICES', 'ROCR_VISIBLE_DEVICES', 'CUDA_VISIBLE_DEVICES')):
            # a launcher that masks the devices per rank: this rank's one visible GPU is its own
            device = 0
        ctx = _ctx_p()
        # no wrap-around: a rank whose LOCAL_RANK has no GPU must fail, not share another rank's device
        rc = self._lib.vb_create(int(device), ctypes.byref(ctx))
        if rc != VB_OK:
            raise EngineError('vb_create(device=%d) failed: %s (%d device(s) visible)'
                              % (int(device), self._lib.vb_last_error(None).decode(), n.value))
        self._ctx = ctx
        self.device = int(device)
        self._model_key = None
        self.n_ranks, self.rank = 1, 0

    def close(self):
        if getattr(self, '_ctx', None):
            self._lib.vb_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ errors
    def _check(self, rc):
        if rc == VB_OK:
            # IPC transport: a device-side wait that gave up has poisoned the results with NaN -- every call says so
            if getattr(self, '_ipc_on', False) and self._lib.vb_comm_check(self._ctx) != VB_OK:
                rc = VB_ERR_COMM
            else:
                return
        msg = self._lib.vb_last_error(self._ctx).decode()
        if rc == VB_ERR_CALLBACK:                    # a host model callable raised: hand its own exception on
            holder = getattr(self, '_callback_error', None)
            if holder and holder[0] is not None:
                exc, holder[0] = holder[0], None
                raise exc
        if rc == VB_ERR_INVALID or rc == VB_ERR_NUMERIC:
            raise ValueError(msg)
        if rc == VB_ERR_UNSUPPORTED:
            raise NotImplementedError(msg)
        raise EngineError(msg)

    # ------------------------------------------------------------------ info
    def device_info(self):
        name = ctypes.create_string_buffer(256)
        cu = ctypes.c_int(0)
        hbm = ctypes.c_uint64(0)
        self._check(self._lib.vb_device_info(self._ctx, name, 256, ctypes.byref(cu), ctypes.byref(hbm)))
        return {'name': name.value.decode(), 'cus': cu.value, 'hbm_bytes': hbm.value}

    def sync(self):
        self._check(self._lib.vb_sync(self._ctx))

    # ------------------------------------------------------------------ noise
    def noise_set_host(self, slot, eps):
        eps = _f64(eps)
        n, d = eps.shape
        self._check(self._lib.vb_noise_set_host(self._ctx, slot, _dptr(eps), n, d))

    def noise_hint_seed(self, slot_mask, seed, with_chi=False):
        """Tell the look-ahead generator the seed of the NEXT call's Philox requests (``vb_noise_hint_seed``): a
        prediction only -- a shadow that does not match the request is never adopted."""
        self._check(self._lib.vb_noise_hint_seed(self._ctx, int(slot_mask), 1 if with_chi else 0, int(seed)))

    def noise_ahead_stats(self):
        """``(generated, adopted)``: look-ahead buffers this engine has generated / requests that adopted one."""
        g, a = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._check(self._lib.vb_noise_ahead_stats(self._ctx, ctypes.byref(g), ctypes.byref(a)))
        return int(g.value), int(a.value)

    def noise_generate(self, slot, n, d, seed, stream=0, row_offset=0, kind=NOISE_NORMAL, df=0.0):
        self._check(self._lib.vb_noise_generate(self._ctx, slot, kind, float(df), int(seed), int(stream),
                                                int(row_offset), int(n), int(d)))

    def chisq_generate(self, df, n, seed, stream=0, row_offset=0):
        """``n`` chi-square(df) draws on the device (kept in the context for ``dis_refresh_mvt(chi=None)``)."""
        self._check(self._lib.vb_chisq_generate(self._ctx, float(df), int(seed), int(stream), int(row_offset), int(n)))

    def chisq_get_host(self, n):
        out = np.empty(n, dtype=np.float64)
        self._check(self._lib.vb_chisq_get_host(self._ctx, _dptr(out), n))
        return out

    def noise_legacy_randn(self, slot, rng_handle, n_total, d, row_begin=0, rows=None):
        """Rows ``[row_begin, row_begin + rows)`` of ``RandomState.randn(n_total, d)`` generated ON THE DEVICE into
        ``slot``, bit for bit numpy's stream (``vb_legacy_rng_randn_device``); ``rng_handle`` is the ``vb_legacy_rng*``
        of a ``LegacyRandomState`` and is advanced as numpy would advance it.  Returns False when the request is outside
        the device path's range (the generator is untouched then: draw on the host and upload)."""
        rows = n_total - row_begin if rows is None else rows
        rc = self._lib.vb_legacy_rng_randn_device(self._ctx, rng_handle, slot, n_total, d, row_begin, rows)
        if rc == VB_ERR_UNSUPPORTED:
            return False
        self._check(rc)
        return True

    def noise_legacy_standard_t(self, slot, rng_handle, df, n_total, d, row_begin=0, rows=None):
        """Rows ``[row_begin, row_begin + rows)`` of ``RandomState.standard_t(df, (n_total, d))`` generated ON THE DEVICE
        into ``slot``, values and generator state bit for bit numpy's (``vb_legacy_rng_standard_t_device``).  False: the
        request is outside the device path's range, the generator is untouched."""
        rows = n_total - row_begin if rows is None else rows
        rc = self._lib.vb_legacy_rng_standard_t_device(self._ctx, rng_handle, float(df), slot, n_total, d, row_begin, rows)
        if rc == VB_ERR_UNSUPPORTED:
            return False
        self._check(rc)
        return True

    def chisq_legacy(self, rng_handle, df, n, to_host=True):
        """``RandomState.chisquare(df, n)`` generated ON THE DEVICE into the context's chi-square buffer (where
        ``chisq_generate`` puts the throughput mode's), bit for bit numpy's; returns the host copy (``to_host``), True, or
        None when the request is outside the device path's range (generator untouched)."""
        out = np.empty(n, dtype=np.float64) if to_host else None
        rc = self._lib.vb_legacy_rng_chisquare_device(self._ctx, rng_handle, float(df), n,
                                                      _dptr(out) if to_host else None)
        if rc == VB_ERR_UNSUPPORTED:
            return None
        self._check(rc)
        return out if to_host else True

    def legacy_round_end(self, rng_handle):
        """A call's device draws from ``rng_handle`` are done (``vb_legacy_round_end``): the engine may start the next call's
        -- the same requests, from the generator's current state -- beside the kernels that follow."""
        self._check(self._lib.vb_legacy_round_end(self._ctx, rng_handle))

    def legacy_ahead_stats(self):
        """``(launched, adopted, discarded)`` of the look-ahead generation of numpy's streams."""
        a, b, c = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._check(self._lib.vb_legacy_ahead_stats(self._ctx, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, c.value

    def noise_get_host(self, slot, n, d):
        out = np.empty((n, d), dtype=np.float64)
        self._check(self._lib.vb_noise_get_host(self._ctx, slot, _dptr(out), n, d))
        return out

    # ------------------------------------------------------------------ model
    def set_model(self, spec):
        """``spec`` = (model_id, dim, dparams ndarray, iparams ndarray) from ``DeviceModel.device_spec``."""
        model_id, dim, dparams, iparams = spec[:4]
        # models hand out the same (cached) parameter arrays every time: identity is the cache key
        key = (model_id, dim, id(dparams), id(iparams)) + tuple(id(x) for x in spec[4:])
        # a minibatch target's spec = (id, dim, dparams, iparams, [batch counter]): the model object owns the counter (the
        # engine's is lost with the binding), and every binding -- a repeated one included -- pushes it
        minibatch = model_id == MODEL_MINIBATCH_GLM
        if minibatch and self.n_ranks > 1:
            raise NotImplementedError('MinibatchRegressionModel on a sharded engine ({} ranks): every rank would have to '
                                      'advance the same batch counter; not supported'.format(self.n_ranks))
        if key == self._model_key:
            if minibatch:
                self._check(self._lib.vb_minibatch_set_batch(self._ctx, int(spec[4][0])))
            return
        self._model_arrays = tuple(spec[2:])         # keep them alive so the ids stay unique
        if model_id == MODEL_SOURCE and isinstance(spec[4], MODEL_CALLBACK_TYPE):
            # spec = (id, dim, -, -, ctypes callback, error holder): a host callable with its gradient
            self._check(self._lib.vb_set_model_callback(self._ctx, dim, ctypes.cast(spec[4], ctypes.c_void_p), None))
            self._callback_error = spec[5]
            self._model_key = key
            return
        if model_id == MODEL_SOURCE:                 # spec = (id, dim, params, iparams (unused), source bytes)
            params = _f64(dparams)
            self._check(self._lib.vb_set_model_source(self._ctx, dim, spec[4], _dptr(params) if params.size else None,
                                                      params.size))
            self._model_key = key
            return
        dparams = _f64(dparams)
        iparams = np.ascontiguousarray(iparams, dtype=np.int64)
        self._check(self._lib.vb_set_model(
            self._ctx, model_id, dim, _dptr(dparams) if dparams.size else None, dparams.size,
            iparams.ctypes.data_as(_c_int64_p) if iparams.size else None, iparams.size))
        self._model_key = key
        if minibatch:
            self._check(self._lib.vb_minibatch_set_batch(self._ctx, int(spec[4][0])))

    def model_logp(self, x):
        x = _f64(x)
        n, d = x.shape
        out = np.empty(n, dtype=np.float64)
        self._check(self._lib.vb_model_logp(self._ctx, _dptr(x), n, d, _dptr(out)))
        return out

    def model_grad(self, x):
        """(f(x_n), grad f(x_n)) of the bound model for host points x (N x D)."""
        x = _f64(x)
        n, d = x.shape
        f = np.empty(n, dtype=np.float64)
        g = np.empty((n, d), dtype=np.float64)
        self._check(self._lib.vb_model_grad(self._ctx, _dptr(x), n, d, _dptr(f), _dptr(g)))
        return f, g

    def elbo_sums_lowrank(self, slot_eps, slot_z, n, d, k, theta):
        """(sum f, sum g (d), sum g eps (d), sum g z' (d x k)) of the low-rank family's ExclusiveKL at any rank."""
        theta = _f64(theta)
        out = np.empty(1 + 2 * d + d * k, dtype=np.float64)
        self._check(self._lib.vb_elbo_sums_lowrank(self._ctx, slot_eps, slot_z, n, d, k, _dptr(theta), _dptr(out)))
        return out[0], out[1:1 + d], out[1 + d:1 + 2 * d], out[1 + 2 * d:].reshape(d, k)

    def elbo_grad_mvt_chol(self, slot, n, d, theta, df, n_total=None):
        """Throughput-mode ExclusiveKL of the multivariate t (Cholesky sampling, device chi-square draws)."""
        theta = _f64(theta)
        value = ctypes.c_double(0.0)
        grad = np.empty(d + d * (d + 1) // 2, dtype=np.float64)
        self._check(self._lib.vb_elbo_grad_mvt_chol(self._ctx, slot, n, d, n if n_total is None else n_total, float(df),
                                                    _dptr(theta), ctypes.byref(value), _dptr(grad)))
        return value.value, grad

    def noise_moments(self, slot, n, d, want_gram=False):
        """(sum_n eps_n (d), sum_n eps_n eps_n' (d x d) or None) of the first n rows of a noise slot, summed over the
        ranks of a sharded job."""
        colsum = np.empty(d, dtype=np.float64)
        gram = np.empty((d, d), dtype=np.float64) if want_gram else None
        self._check(self._lib.vb_noise_moments(self._ctx, slot, n, d, _dptr(colsum),
                                               _dptr(gram) if want_gram else None))
        return colsum, gram

    # ------------------------------------------------------------------ ExclusiveKL, mean field
    def elbo_grad_meanfield(self, slot, n, d, theta, family, df=0.0, flags=0, cv_mode=0, n_total=None):
        theta = _f64(theta)
        value = ctypes.c_double(0.0)
        grad = np.empty(2 * d, dtype=np.float64)
        self._check(self._lib.vb_elbo_grad_meanfield(
            self._ctx, slot, n, d, n if n_total is None else n_total, family, float(df), _dptr(theta),
            flags, cv_mode, ctypes.byref(value), _dptr(grad)))
        return value.value, grad

    def elbo_grad_meanfield_async(self, slot, n, d, theta, family, rslot, df=0.0, flags=0, cv_mode=0,
                                  n_total=None):
        theta = _f64(theta)
        self._check(self._lib.vb_elbo_grad_meanfield_async(
            self._ctx, slot, n, d, n if n_total is None else n_total, family, float(df), _dptr(theta),
            flags, cv_mode, rslot))

    def elbo_grad_meanfield_batch_async(self, slots, n, d, thetas, family, rslots, df=0.0, flags=0,
                                        cv_mode=0, n_total=None):
        """Enqueue ``len(slots)`` independent evaluations; ``thetas`` is ``(count, 2d)``."""
        thetas = _f64(thetas)
        count = len(slots)
        if thetas.shape != (count, 2 * d):
            raise ValueError('thetas must have shape (count, 2 * d)')
        c_slots = (ctypes.c_int * count)(*slots)
        c_rslots = (ctypes.c_int * count)(*rslots)
        self._check(self._lib.vb_elbo_grad_meanfield_batch_async(
            self._ctx, count, c_slots, n, d, n if n_total is None else n_total, family, float(df),
            _dptr(thetas), flags, cv_mode, c_rslots))

    def result_get(self, rslot, p):
        value = ctypes.c_double(0.0)
        grad = np.empty(p, dtype=np.float64)
        self._check(self._lib.vb_result_get(self._ctx, rslot, ctypes.byref(value), _dptr(grad), p))
        return value.value, grad

    # ------------------------------------------------------------------ ExclusiveKL, multivariate t
    def elbo_sums_mvt(self, slot, n, d, mu, sqrt_sigma, inv_s, n_total=None):
        """(sum f, sum g (D,), sum g (z / s)' (D, D)) over the samples x = mu + (z sqrt_sigma) / s."""
        mu, sqrt_sigma, inv_s = _f64(mu), _f64(sqrt_sigma), _f64(inv_s)
        f = ctypes.c_double(0.0)
        g = np.empty(d, dtype=np.float64)
        c = np.empty((d, d), dtype=np.float64)
        self._check(self._lib.vb_elbo_sums_mvt(self._ctx, slot, n, d, n if n_total is None else n_total,
                                               _dptr(mu), _dptr(sqrt_sigma), _dptr(inv_s), ctypes.byref(f),
                                               _dptr(g), _dptr(c)))
        return f.value, g, c

    def elbo_grad_meanfield_philox(self, slot, n, d, theta, family, seed, stream, df=0.0, flags=0, cv_mode=0,
                                   n_total=None, row_offset=0):
        """ExclusiveKL on fresh Philox noise generated inside the streaming kernel
        (``vb_elbo_grad_meanfield_philox``)."""
        theta = _f64(theta)
        value = ctypes.c_double(0.0)
        grad = np.empty(2 * d, dtype=np.float64)
        self._check(self._lib.vb_elbo_grad_meanfield_philox(
            self._ctx, slot, n, d, n if n_total is None else n_total, int(row_offset), family, float(df),
            _dptr(theta), flags, cv_mode, int(seed), int(stream), ctypes.byref(value), _dptr(grad)))
        return value.value, grad

    # ------------------------------------------------------------------ ExclusiveKL, low-rank Gaussian
    def elbo_grad_lowrank(self, slot_eps, slot_z, n, d, k, theta, flags=0, n_total=None):
        theta = _f64(theta)
        value = ctypes.c_double(0.0)
        grad = np.empty(2 * d + d * k, dtype=np.float64)
        self._check(self._lib.vb_elbo_grad_lowrank(self._ctx, slot_eps, slot_z, n, d, k,
                                                   n if n_total is None else n_total, _dptr(theta), flags,
                                                   ctypes.byref(value), _dptr(grad)))
        return value.value, grad

    # ------------------------------------------------------------------ importance weights, PSIS
    def log_weights_meanfield(self, slot, n, d, theta, family, df=0.0, fetch=True):
        """log p(z_n) - log q(z_n) for the staged noise; the weights also stay on the device for
        :meth:`psis_smooth`."""
        theta = _f64(theta)
        lw = np.empty(n, dtype=np.float64) if fetch else None
        self._check(self._lib.vb_log_weights_meanfield(self._ctx, slot, n, d, family, float(df), _dptr(theta),
                                                       _dptr(lw) if fetch else None))
        return lw

    def psis_smooth(self, n, log_weights=None, reff=1.0):
        """Pareto-smoothed, normalised log weights and k-hat; ``log_weights=None`` smooths the weights
        left on the device by :meth:`log_weights_meanfield`."""
        out = np.empty(n, dtype=np.float64)
        khat = ctypes.c_double(0.0)
        src = None
        if log_weights is not None:
            log_weights = _f64(log_weights)
            if log_weights.shape != (n,):
                raise ValueError('log_weights must have shape ({},)'.format(n))
            src = _dptr(log_weights)
        self._check(self._lib.vb_psis_smooth(self._ctx, src, n, float(reff), _dptr(out), ctypes.byref(khat)))
        return out, khat.value

    def psis_smooth_batch(self, lw, reff=1.0, out=None):
        """``lw``: ``(m, n)`` C-contiguous, one weight vector per ROW; all rows smoothed in one launch
        (``vb_psis_smooth_batch``).  Returns ``(smoothed (m, n), khat (m,))``; ``out`` may be ``lw`` itself."""
        lw = _f64(lw)
        m, n = lw.shape
        if out is None:
            out = np.empty_like(lw)
        khat = np.empty(m, dtype=np.float64)
        self._check(self._lib.vb_psis_smooth_batch(self._ctx, _dptr(lw), n, m, n, float(reff), _dptr(out), _dptr(khat)))
        return out, khat

    def _pointwise(self, symbol, x, n_data):
        x = _f64(x)
        s, d = x.shape
        out = np.empty((s, int(n_data)), dtype=np.float64)
        self._check(getattr(self._lib, symbol)(self._ctx, _dptr(x), s, d, _dptr(out)))
        return out

    def glm_pointwise(self, x, n_data):
        """``(S, n_data)`` pointwise log-likelihoods of the bound regression target (``n_data`` observations) at the
        draws ``x`` (S x D)."""
        return self._pointwise('vb_glm_pointwise', x, n_data)

    def softmax_pointwise(self, x, n_data):
        """``(S, n_data)`` terms ``eta_{i, y_i} - logsumexp_c eta_ic`` of the bound softmax regression target at the draws
        ``x`` (S x D)."""
        return self._pointwise('vb_softmax_pointwise', x, n_data)

    def multilevel_pointwise(self, x, n_data):
        """``(S, n_data)`` normalised terms ``log p(y_i | x_i' b + tau u_{g_i})`` of the bound multilevel regression target
        at the draws ``x`` (S x D), observations in the bound (group-sorted) order."""
        return self._pointwise('vb_multilevel_pointwise', x, n_data)

    def locscale_pointwise(self, x, n_data):
        """``(S, n_data)`` normalised terms ``log p(y_i | x_i' b, exp(w_i' g))`` of the bound location-scale regression
        target at the draws ``x`` (S x D)."""
        return self._pointwise('vb_locscale_pointwise', x, n_data)

    def sparse_glm_pointwise(self, x, n_data):
        """``(S, n_data)`` normalised terms ``log p(y_i | x_i' theta)`` of the bound sparse regression target at the draws
        ``x`` (S x D)."""
        return self._pointwise('vb_sparse_glm_pointwise', x, n_data)

    def nn_pointwise(self, x, n_data):
        """``(S, n_data)`` normalised terms ``log p(y_i | eta_i)`` of the bound neural-network regression target at the
        draws ``x`` (S x D), ``eta_i`` the network's output at observation ``i``."""
        return self._pointwise('vb_nn_pointwise', x, n_data)

    def minibatch_pointwise(self, x, batch_size):
        """``(S, batch_size)`` normalised, unscaled terms ``log p(y_j | x_j' theta)`` of the current batch of the bound
        minibatch regression target at the draws ``x`` (S x D), in batch order."""
        return self._pointwise('vb_minibatch_pointwise', x, batch_size)

    def minibatch_get_batch(self):
        """The engine's batch counter of the bound minibatch regression target (a device fit has advanced it)."""
        t = ctypes.c_int64(0)
        self._check(self._lib.vb_minibatch_get_batch(self._ctx, ctypes.byref(t)))
        return int(t.value)

    def minibatch_indices(self, t, batch_size):
        """The observation indices of batch ``t`` of the bound minibatch regression target as the index kernel computes
        them: int64 ``(batch_size,)``."""
        out = np.empty(int(batch_size), dtype=np.int64)
        self._check(self._lib.vb_minibatch_indices(self._ctx, int(t), out.ctypes.data_as(_c_int64_p)))
        return out

    def glm_psis_loo(self, x, n_data, log_ratios=None, log_w=None, reff=1.0):
        """PSIS-LOO of the bound regression target (``n_data`` observations) from the draws ``x``
        (``vb_glm_psis_loo``): ``(loo, khat, lpd)``, each ``(n_data,)``; ``lpd`` is None without ``log_w``."""
        x = _f64(x)
        s, d = x.shape
        n_data = int(n_data)
        loo, khat = np.empty(n_data, dtype=np.float64), np.empty(n_data, dtype=np.float64)
        lpd = np.empty(n_data, dtype=np.float64) if log_w is not None else None
        for name, v in (('log_ratios', log_ratios), ('log_w', log_w)):
            if v is not None and np.shape(v) != (s,):
                raise ValueError('{} must have shape ({},)'.format(name, s))
        log_ratios = None if log_ratios is None else _f64(log_ratios)
        log_w = None if log_w is None else _f64(log_w)
        self._check(self._lib.vb_glm_psis_loo(self._ctx, _dptr(x), s, d,
                                              None if log_ratios is None else _dptr(log_ratios),
                                              None if log_w is None else _dptr(log_w), float(reff), _dptr(loo),
                                              _dptr(khat), None if lpd is None else _dptr(lpd)))
        return loo, khat, lpd

    def glm_predict(self, x, log_w=None, X_new=None, y_new=None):
        """Posterior prediction with the bound regression target from the draws ``x`` (S x D) and their log weights
        ``log_w`` (S,; None: uniform; normalised by the entry) (``vb_glm_predict``).  ``X_new`` (m x D): the design to
        predict at, ``y_new`` (m,) its responses; ``X_new=None`` predicts the bound design and ``y_new=None`` then means
        the bound responses.  Returns a dict of ``(m,)`` arrays: ``mean``, ``var``, ``eta_mean``, ``eta_var`` and -- with
        a response -- ``lpd``.  The (m x S) matrix of linear predictors stays on the device."""
        return self._predict('vb_glm_predict', x, None, log_w, X_new, y_new)

    def nn_predict(self, x, n_features, log_w=None, X_new=None, y_new=None):
        """:meth:`glm_predict` for the bound neural-network regression target (``vb_nn_predict``): the same arguments and
        the same dict, with ``X_new`` (m x ``n_features``) and ``eta`` the network's output."""
        return self._predict('vb_nn_predict', x, int(n_features), log_w, X_new, y_new)

    def _predict(self, symbol, x, n_cols, log_w, X_new, y_new):
        """The argument checks and the call shared by the prediction entries; ``n_cols``: columns of ``X_new`` (None: D)."""
        x = _f64(x)
        if x.ndim != 2:
            raise ValueError('x must be (S, D)')
        s, d = x.shape
        if log_w is not None:
            if np.shape(log_w) != (s,):
                raise ValueError('log_w must have shape ({},)'.format(s))
            log_w = _f64(log_w)
            if not np.any(np.isfinite(log_w)):
                raise ValueError('no log weight is finite')
        if X_new is None:
            # the bound design: its row count is the first integer parameter of the regression targets (0 lets the C
            # entry say what is wrong: no model bound, or one without observations)
            iparams = self._model_arrays[1] if self._model_key is not None and len(self._model_arrays) > 1 else ()
            m = int(iparams[0]) if len(iparams) else 0
        else:
            X_new = _f64(X_new)
            n_cols = d if n_cols is None else n_cols
            if X_new.ndim != 2 or X_new.shape[1] != n_cols:
                raise ValueError('X_new must be (m, {}); got {}'.format(n_cols, X_new.shape))
            m = X_new.shape[0]
        if y_new is not None:
            if np.shape(y_new) != (m,):
                raise ValueError('y_new must have shape ({},)'.format(m))
            y_new = _f64(y_new)
        mean, var, eta_mean, eta_var = (np.empty(m, dtype=np.float64) for _ in range(4))
        lpd = np.empty(m, dtype=np.float64) if X_new is None or y_new is not None else None
        self._check(getattr(self._lib, symbol)(self._ctx, _dptr(x), s, d, None if log_w is None else _dptr(log_w),
                                               None if X_new is None else _dptr(X_new), m,
                                               None if y_new is None else _dptr(y_new), _dptr(mean), _dptr(var),
                                               _dptr(eta_mean), _dptr(eta_var), None if lpd is None else _dptr(lpd)))
        out = dict(mean=mean, var=var, eta_mean=eta_mean, eta_var=eta_var)
        if lpd is not None:
            out['lpd'] = lpd
        return out

    def glm_value_grad_hessian(self, x, want_hessian=True):
        """``(f, grad, hess)`` of the bound regression target at the one point ``x`` (D,) (``vb_glm_value_grad_hessian``):
        the log density with all constants, its gradient ``(D,)`` and the exactly symmetric Hessian ``(D, D)`` --
        ``None`` with ``want_hessian=False``, which skips the scaled copy of the design and the Gram product and returns
        the same ``f`` and ``grad`` bits."""
        x = _f64(x)
        if x.ndim != 1:
            raise ValueError('x must be (D,)')
        d = x.shape[0]
        f = ctypes.c_double(0.0)
        grad = np.empty(d, dtype=np.float64)
        hess = np.empty((d, d), dtype=np.float64) if want_hessian else None
        self._check(self._lib.vb_glm_value_grad_hessian(self._ctx, _dptr(x), d, ctypes.addressof(f), _dptr(grad),
                                                        None if hess is None else _dptr(hess)))
        return f.value, grad, hess

    def ksd(self, x, scores=None, log_w=None, scale=None, c=1.0, beta=-0.5):
        """Squared kernel Stein discrepancy of the weighted draws ``x`` (S x D) with the IMQ kernel
        ``(c^2 + |x - y|^2)^beta`` (``vb_ksd``): ``(ksd2, rowsums)``, ``rowsums`` (S,) with
        ``ksd2 = sum_i w_i rowsums[i]``.  ``scores`` (S x D): ``grad log p`` at the draws; None: the bound model's,
        evaluated on the device.  ``log_w`` (S,; None: uniform; normalised by the entry), ``scale`` (D,; None: ones): the
        discrepancy is that of ``x / scale`` with scores ``scores * scale``.  The arguments are checked before the call
        (:func:`ksd_arguments`)."""
        x, scores, log_w, scale, c, beta = ksd_arguments(x, scores, log_w, scale, c, beta)
        s, d = x.shape
        ksd2 = ctypes.c_double(0.0)
        rowsums = np.empty(s, dtype=np.float64)
        self._check(self._lib.vb_ksd(self._ctx, _dptr(x), s, d, None if scores is None else _dptr(scores),
                                     None if log_w is None else _dptr(log_w), None if scale is None else _dptr(scale), c,
                                     beta, ctypes.addressof(ksd2), _dptr(rowsums)))
        return ksd2.value, rowsums

    def svgd_direction(self, x, scores=None, scale=None, bandwidth='median'):
        """One SVGD direction (``vb_svgd_direction``) of the particles ``x`` (n x D) with the RBF kernel of
        ``(x - mean) / scale``: ``(phi, h, logp)``.  ``scores`` (n x D): ``grad log p`` at the particles; None: the bound
        model's, evaluated on the device (``logp`` (n,) is then its log density, else None).  ``scale`` (D,; None: ones);
        ``bandwidth``: ``'median'`` (``h = median r2 / log(n + 1)``, selected exactly on the device) or a positive number.
        The arguments are checked before the call (:func:`svgd_arguments`)."""
        x, scores, scale, bandwidth = svgd_arguments(x, scores, scale, bandwidth)
        n, d = x.shape
        phi = np.empty((n, d), dtype=np.float64)
        logp = np.empty(n, dtype=np.float64) if scores is None else None
        h = ctypes.c_double(0.0)
        self._check(self._lib.vb_svgd_direction(self._ctx, _dptr(x), n, d, None if scores is None else _dptr(scores),
                                                None if scale is None else _dptr(scale), bandwidth, _dptr(phi),
                                                None if logp is None else _dptr(logp), ctypes.addressof(h)))
        return phi, h.value, logp

    def svgd_run(self, x0, n_iters, opt_kind, hyper, state=None, scale=None, bandwidth='median'):
        """``n_iters`` iterations of SVGD on the bound model in one call (``vb_svgd_run``): the scores, the direction of
        :meth:`svgd_direction` and one optimiser step (``opt_kind`` one of ``OPT_SGD`` / ``OPT_RMSPROP`` / ``OPT_ADAM`` /
        ``OPT_ADAGRAD``, ``hyper = [learning rate, beta or beta1, beta2, jitter]``) per iteration, without host
        synchronisation in between.  ``state``: the optimiser state ``[second moment (n D) | momentum (n D)]`` of an
        earlier run (None: fresh).  Returns a dict: ``particles`` (n x D), ``logp`` (n,), ``state`` (2 n D,) and
        ``bandwidth_history``, ``phi_rms_history``, ``logp_history`` (n_iters,; at the start of every iteration)."""
        x0, _, scale, bandwidth = svgd_arguments(x0, None, scale, bandwidth)
        n, d = x0.shape
        n_iters = int(n_iters)
        if n_iters < 1:
            raise ValueError('n_iters must be positive')
        hyper = np.array(hyper, dtype=np.float64)
        if hyper.shape != (4,):
            raise ValueError('hyper must have four entries (learning rate, beta / beta1, beta2, jitter)')
        has_state = state is not None
        state = np.array(state, dtype=np.float64).ravel() if has_state else np.zeros(2 * n * d, dtype=np.float64)
        if state.shape != (2 * n * d,):
            raise ValueError('state must have {} entries'.format(2 * n * d))
        x = np.empty((n, d), dtype=np.float64)
        logp = np.empty(n, dtype=np.float64)
        h_hist, rms_hist, logp_hist = (np.empty(n_iters, dtype=np.float64) for _ in range(3))
        self._check(self._lib.vb_svgd_run(self._ctx, _dptr(x0), n, d, None if scale is None else _dptr(scale), bandwidth,
                                          int(opt_kind), _dptr(hyper), n_iters, _dptr(state), int(has_state), _dptr(x),
                                          _dptr(logp), _dptr(h_hist), _dptr(rms_hist), _dptr(logp_hist)))
        return dict(particles=x, logp=logp, state=state, bandwidth_history=h_hist, phi_rms_history=rms_hist,
                    logp_history=logp_hist)

    def smc_reweight(self, u, beta_prev, ess_target, uniform):
        """One stage's reweight and resample of tempered SMC on the host log weights ``u`` (n,) (``vb_smc_reweight``, the
        kernels ``smc_run`` uses): the next temperature by the 40-step bisection on the effective sample size (exactly 1.0
        when ``1 - beta_prev`` already keeps ``ess_target``), the log-evidence increment, and the systematic resampling's
        ancestors for the uniform ``uniform`` in [0, 1).  Returns ``(beta, log_z_inc, ess, ancestors (n,) int64)``.
        ``ValueError`` for a NaN or ``+inf`` weight, for all ``-inf`` and when fewer than ``ess_target`` of the particles
        carry weight; no model needs to be bound."""
        u = _f64(u)
        if u.ndim != 1 or u.size < 1:
            raise ValueError('u must be (n,) with n >= 1; got shape {}'.format(u.shape))
        out = np.zeros(3, dtype=np.float64)
        ancestors = np.zeros(u.size, dtype=np.int64)
        self._check(self._lib.vb_smc_reweight(self._ctx, _dptr(u), u.size, float(beta_prev), float(ess_target), float(uniform),
                                              _dptr(out), ancestors.ctypes.data_as(_c_int64_p)))
        return float(out[0]), float(out[1]), float(out[2]), ancestors

    def smc_run(self, loc, scale, n, ess_target=0.5, n_moves=2, n_leapfrog=8, step_size=1.0, target_accept=0.8,
                adapt_rate=0.5, max_stages=200, seed=1, stream_offset=0, keep_ancestors=False):
        """Adaptive tempered SMC with HMC moves on the bound model (``vb_smc_run``) from the base ``N(loc, diag(scale^2))``:
        ``n`` particles, per stage the temperature search, systematic resampling and ``n_moves`` HMC transitions of
        ``n_leapfrog`` steps under the metric ``scale^2``, the step size adapted in device memory; one 16-byte host round
        trip per stage.  Returns a dict: ``particles`` (n x D), ``logp`` and ``log_base`` (n,), ``log_evidence``,
        ``n_stages``, ``betas``, ``log_z_increments``, ``ess`` (n_stages,), ``accept_prob``, ``step_size_history`` and
        ``n_accepted`` (n_stages x n_moves), ``step_size`` (after the last update), ``n_divergent`` and ``ancestors``
        (n_stages x n, int64; None without ``keep_ancestors``)."""
        loc, scale = _f64(loc), _f64(scale)
        if loc.ndim != 1 or loc.size < 1 or scale.shape != loc.shape:
            raise ValueError('loc and scale must be (D,) with D >= 1; got shapes {} and {}'.format(loc.shape, scale.shape))
        n, d, n_moves, max_stages = int(n), loc.size, int(n_moves), int(max_stages)
        if n < 1 or n_moves < 1 or max_stages < 1:
            raise ValueError('n, n_moves and max_stages must be positive')
        x = np.empty((n, d), dtype=np.float64)
        logp, log_base = np.empty(n, dtype=np.float64), np.empty(n, dtype=np.float64)
        beta_hist, log_z_hist, ess_hist = (np.zeros(max_stages, dtype=np.float64) for _ in range(3))
        accept_hist, step_hist = (np.zeros((max_stages, n_moves), dtype=np.float64) for _ in range(2))
        n_acc_hist = np.zeros((max_stages, n_moves), dtype=np.int64)
        anc_hist = np.zeros((max_stages, n), dtype=np.int64) if keep_ancestors else None
        log_ev, final = ctypes.c_double(0.0), ctypes.c_double(0.0)
        n_stages, n_div = ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self._lib.vb_smc_run(
            self._ctx, _dptr(loc), _dptr(scale), n, d, float(ess_target), n_moves, int(n_leapfrog), float(step_size),
            float(target_accept), float(adapt_rate), max_stages, int(seed), int(stream_offset), _dptr(x), _dptr(logp),
            _dptr(log_base), ctypes.addressof(log_ev), ctypes.byref(n_stages), _dptr(beta_hist), _dptr(log_z_hist),
            _dptr(ess_hist), _dptr(accept_hist), _dptr(step_hist), n_acc_hist.ctypes.data_as(_c_int64_p),
            ctypes.addressof(final), ctypes.byref(n_div),
            None if anc_hist is None else anc_hist.ctypes.data_as(_c_int64_p)))
        k = int(n_stages.value)
        return dict(particles=x, logp=logp, log_base=log_base, log_evidence=log_ev.value, n_stages=k, betas=beta_hist[:k].copy(),
                    log_z_increments=log_z_hist[:k].copy(), ess=ess_hist[:k].copy(), accept_prob=accept_hist[:k].copy(),
                    step_size_history=step_hist[:k].copy(), n_accepted=n_acc_hist[:k].copy(), step_size=final.value,
                    n_divergent=int(n_div.value), ancestors=None if anc_hist is None else anc_hist[:k].copy())

    def hmc_run(self, x0, inv_mass, n_warmup, n_draws, n_leapfrog, step_size, target_accept=0.8, jitter=0.2, seed=1,
                stream_offset=0, thin=1, keep_draws=True):
        """Many-chain HMC on the bound model (``vb_hmc_run``): ``x0`` (C x D) starts, ``inv_mass`` (D,) the diagonal
        metric.  The whole run is one call; the outputs are allocated here.  Returns a dict: ``draws`` (n_kept x C x D, or
        None with ``keep_draws=False``), ``logp`` (n_kept x C), ``last`` (C x D), ``chain_mean`` and ``chain_m2`` (C x D),
        ``accept_rate`` (C,), ``step_size_history`` and ``accept_prob`` (n_warmup + n_draws,), ``step_size`` (the
        sampling phase's) and ``n_divergent``."""
        run = [int(n_warmup), int(n_draws), int(thin), int(n_leapfrog), float(step_size), float(target_accept), float(jitter),
               int(seed), int(stream_offset)]
        return self._hmc_call('vb_hmc_run', x0, inv_mass, run, keep_draws)

    def _hmc_call(self, entry, x0, metric, run, keep_draws, moment_shift=None, traj_state=None):
        """What ``hmc_run``, ``hmc_run_metric`` and ``hmc_run_chees`` share: the arrays coerced and checked, the outputs
        allocated, the entry's argument list, the result dict.  ``run`` holds the entry's scalars from ``n_warmup`` to
        ``stream_offset`` as the C entry takes them; ``vb_hmc_run`` takes a diagonal metric only, no metric kind and no
        moments, and always samples; ``traj_state`` is ``vb_hmc_run_chees``'s."""
        plain, chees = entry == 'vb_hmc_run', entry == 'vb_hmc_run_chees'
        x0, metric = _f64(x0), _f64(metric)
        if x0.ndim != 2:
            raise ValueError('x0 must be (n_chains, D)')
        c, d = x0.shape
        if plain and metric.shape != (d,):
            raise ValueError('inv_mass must have shape ({},)'.format(d))
        if metric.shape not in ((d,), (d, d)):
            raise ValueError('metric must have shape ({0},) or ({0}, {0})'.format(d))
        if chees:
            state = np.array(traj_state, dtype=np.float64)
            if state.shape != (4,):
                raise ValueError('traj_state must have four entries (log T, v, log T_bar, m)')
        dense = metric.ndim == 2
        n_warmup, n_draws, thin = run[:3]
        n_iter = max(n_warmup, 0) + max(n_draws, 0)
        n_kept = -(-max(n_draws, 0) // thin) if thin >= 1 else 0
        sampling = plain or n_draws > 0
        draws = np.empty((n_kept, c, d), dtype=np.float64) if keep_draws and sampling else None
        logp = np.empty((n_kept, c), dtype=np.float64) if sampling else None
        last = np.empty((c, d), dtype=np.float64)
        mean, m2 = (np.empty((c, d), dtype=np.float64) if sampling else None for _ in range(2))
        rate = np.empty(c, dtype=np.float64) if sampling else None
        step_hist, accept_hist = np.empty(n_iter, dtype=np.float64), np.empty(n_iter, dtype=np.float64)
        shift = s1 = s2 = None
        if moment_shift is not None:
            shift = _f64(moment_shift)
            if shift.shape != (d,):
                raise ValueError('moment_shift must have shape ({},)'.format(d))
            s1, s2 = np.empty(d, dtype=np.float64), np.empty((d, d) if dense else d, dtype=np.float64)
        final, n_div = ctypes.c_double(0.0), ctypes.c_int64(0)
        opt = lambda a: None if a is None else _dptr(a)                                                       # noqa: E731
        args = [self._ctx, _dptr(x0)] + ([] if plain else [HMC_METRIC_DENSE if dense else HMC_METRIC_DIAG])
        args += [_dptr(metric), c, d] + run + ([] if plain else [opt(shift), opt(s1), opt(s2)])
        args += [opt(draws), opt(logp), _dptr(last), opt(mean), opt(m2), opt(rate), _dptr(step_hist), _dptr(accept_hist),
                 ctypes.addressof(final), ctypes.byref(n_div)]
        if chees:
            traj_hist, leap_hist = np.empty(n_iter, dtype=np.float64), np.zeros(n_iter, dtype=np.int64)
            args += [_dptr(state), _dptr(traj_hist), leap_hist.ctypes.data_as(_c_int64_p)]
        self._check(getattr(self._lib, entry)(*args))
        out = dict(draws=draws, logp=logp, last=last, chain_mean=mean, chain_m2=m2, accept_rate=rate,
                   step_size_history=step_hist, accept_prob=accept_hist, step_size=final.value,
                   n_divergent=int(n_div.value))
        if not plain:
            out.update(moment_sum=s1, moment_m2=s2)
        if chees:
            out.update(traj_state=state, trajectory_history=traj_hist, n_leapfrog_history=leap_hist)
        return out

    def hmc_run_metric(self, x0, metric, n_warmup, n_draws, n_leapfrog, step_size, target_accept=0.8, jitter=0.2, seed=1,
                       stream_offset=0, thin=1, keep_draws=True, moment_shift=None):
        """``hmc_run`` with a choice of metric (``vb_hmc_run_metric``): ``metric`` (D,) is the diagonal metric
        ``inv_mass``, ``metric`` (D, D) the lower Cholesky factor ``L`` of the dense one (``Sigma = L L'``).  ``n_draws``
        may be 0 (a warm-up-only segment: the sampling outputs come back as None).  With ``moment_shift`` (D,) the dict
        also has ``moment_sum`` (D,) and ``moment_m2`` ((D,) or (D, D)): the sums of ``x - shift`` and of its squares /
        outer products over the chains and all iterations of the call."""
        run = [int(n_warmup), int(n_draws), int(thin), int(n_leapfrog), float(step_size), float(target_accept), float(jitter),
               int(seed), int(stream_offset)]
        return self._hmc_call('vb_hmc_run_metric', x0, metric, run, keep_draws, moment_shift)

    def hmc_run_chees(self, x0, metric, n_warmup, n_draws, max_leapfrog, step_size, traj_state, trajectory_lr=0.025,
                      target_accept=0.8, jitter=0.2, seed=1, stream_offset=0, thin=1, keep_draws=True, moment_shift=None):
        """``hmc_run_metric`` with the trajectory length adapted across the chains (``vb_hmc_run_chees``; ChEES-HMC) in
        place of ``n_leapfrog``: at most ``max_leapfrog`` steps per iteration.  ``traj_state`` is ``(log T, v, log T_bar,
        m)`` -- ``(log T0, 0, log T0, 0)`` for a first call, the last call's ``traj_state`` for a continuation.  The dict
        has ``hmc_run_metric``'s entries plus ``traj_state`` (the state after the call), ``trajectory_history`` (float64)
        and ``n_leapfrog_history`` (int64), both of length ``n_warmup + n_draws``."""
        run = [int(n_warmup), int(n_draws), int(thin), int(max_leapfrog), float(trajectory_lr), float(step_size),
               float(target_accept), float(jitter), int(seed), int(stream_offset)]
        return self._hmc_call('vb_hmc_run_chees', x0, metric, run, keep_draws, moment_shift, traj_state)

    # ------------------------------------------------------------------ AlphaDivergence, mean field
    def alpha_grad_meanfield(self, slot, n, d, theta, family, alpha, df=0.0, n_total=None):
        theta = _f64(theta)
        value = ctypes.c_double(0.0)
        grad = np.empty(2 * d, dtype=np.float64)
        self._check(self._lib.vb_alpha_grad_meanfield(self._ctx, slot, n, d, n if n_total is None else n_total,
                                                      family, float(df), _dptr(theta),
                                                      float(alpha), ctypes.byref(value), _dptr(grad)))
        return value.value, grad

    # ------------------------------------------------------------------ DISInclusiveKL
    def dis_set_temper_prior(self, spec):
        """Install a tempering prior that is not an MFGaussian (``vb_dis_set_temper_prior``); ``spec`` =
        ``(kind, df, loc, scale, log_det_l)`` or ``None`` for the refresh calls' own ``prior_theta`` argument.  The
        spec object's identity is the cache key: objectives hand out the same tuple every time."""
        if spec is getattr(self, '_temper_spec', None):
            return
        if spec is None:
            self._check(self._lib.vb_dis_set_temper_prior(self._ctx, PRIOR_DIAG_GAUSSIAN, 0, 0.0, None, None, 0.0))
        else:
            kind, df, loc, scale, log_det_l = spec
            loc, scale = _f64(loc), _f64(scale)
            self._check(self._lib.vb_dis_set_temper_prior(self._ctx, int(kind), loc.size, float(df), _dptr(loc),
                                                          _dptr(scale), float(log_det_l)))
        self._temper_spec = spec

    def dis_refresh_meanfield(self, slot, n, d, theta, prior_theta, family, eps_prev, ess_target,
                              max_bisection_its=50, df=0.0, n_total=None):
        """``n`` local rows; the returned weights / log p / log q cover all ``n_total`` samples."""
        theta, prior_theta = _f64(theta), _f64(prior_theta)
        n_total = n if n_total is None else n_total
        eps, ess = ctypes.c_double(0.0), ctypes.c_double(0.0)
        w, lp, lq = (np.empty(n_total, dtype=np.float64) for _ in range(3))
        self._check(self._lib.vb_dis_refresh_meanfield(
            self._ctx, slot, n, d, n_total, family, float(df), _dptr(theta), _dptr(prior_theta), float(eps_prev),
            float(ess_target), int(max_bisection_its), ctypes.byref(eps), ctypes.byref(ess), _dptr(w),
            _dptr(lp), _dptr(lq)))
        return eps.value, ess.value, w, lp, lq

    def dis_grad_meanfield(self, slot, n, d, theta, weights, scale, family, df=0.0):
        theta, weights = _f64(theta), _f64(weights)
        value = ctypes.c_double(0.0)
        grad = np.empty(2 * d, dtype=np.float64)
        self._check(self._lib.vb_dis_grad_meanfield(self._ctx, slot, n, d, family, float(df), _dptr(theta),
                                                    _dptr(weights), float(scale), ctypes.byref(value),
                                                    _dptr(grad)))
        return value.value, grad

    # ------------------------------------------------------------------ DISInclusiveKL, multivariate t
    # ------------------------------------------------------------------ low-rank Gaussian under DIS / alpha
    def dis_refresh_lowrank(self, slot_eps, slot_z, n, d, k, mu, log_sigma, B, m_inv, log_q_const, prior_theta,
                            eps_prev, ess_target, max_bisection_its=50, n_total=None):
        mu, log_sigma, B, m_inv, prior_theta = (_f64(a) for a in (mu, log_sigma, B, m_inv, prior_theta))
        n_total = n if n_total is None else n_total
        eps, ess = ctypes.c_double(0.0), ctypes.c_double(0.0)
        w, lp, lq = (np.empty(n_total, dtype=np.float64) for _ in range(3))
        self._check(self._lib.vb_dis_refresh_lowrank(
            self._ctx, slot_eps, slot_z, n, d, k, n_total, _dptr(mu), _dptr(log_sigma), _dptr(B), _dptr(m_inv),
            float(log_q_const), _dptr(prior_theta), float(eps_prev), float(ess_target), int(max_bisection_its),
            ctypes.byref(eps), ctypes.byref(ess), _dptr(w), _dptr(lp), _dptr(lq)))
        return eps.value, ess.value, w, lp, lq

    def dis_grad_lowrank(self, n, d, k, mu, log_sigma, B, m_inv, log_q_const, weights):
        """``(sum w rho tau' (d, k), sum w tau tau' (k, k), sum w rho, sum w rho^2, sum w tau, sum w, sum w log q)``."""
        mu, log_sigma, B, m_inv, weights = (_f64(a) for a in (mu, log_sigma, B, m_inv, weights))
        out = np.empty(d * k + k * k + 2 * d + k + 2, dtype=np.float64)
        self._check(self._lib.vb_dis_grad_lowrank(self._ctx, n, d, k, _dptr(mu), _dptr(log_sigma), _dptr(B),
                                                  _dptr(m_inv), float(log_q_const), _dptr(weights), _dptr(out)))
        a, b = d * k, d * k + k * k
        return (out[:a].reshape(d, k), out[a:b].reshape(k, k), out[b:b + d], out[b + d:b + 2 * d],
                out[b + 2 * d:b + 2 * d + k], out[-2], out[-1])

    def alpha_sums_lowrank(self, slot_eps, slot_z, n, d, k, alpha, mu, log_sigma, B, m_inv, log_q_const, n_total=None):
        """``(value, sum s, sum s g z' (d, k), sum s eps t' (d, k), sum s t t' (k, k), sum s g, sum s g eps)``."""
        mu, log_sigma, B, m_inv = (_f64(a) for a in (mu, log_sigma, B, m_inv))
        out = np.empty(2 * d * k + k * k + 2 * d, dtype=np.float64)
        value, w_sum = ctypes.c_double(0.0), ctypes.c_double(0.0)
        self._check(self._lib.vb_alpha_sums_lowrank(
            self._ctx, slot_eps, slot_z, n, d, k, n if n_total is None else n_total, float(alpha), _dptr(mu),
            _dptr(log_sigma), _dptr(B), _dptr(m_inv), float(log_q_const), ctypes.byref(value), ctypes.byref(w_sum),
            _dptr(out)))
        a, b, c = d * k, 2 * d * k, 2 * d * k + k * k
        return (value.value, w_sum.value, out[:a].reshape(d, k), out[a:b].reshape(d, k), out[b:c].reshape(k, k),
                out[c:c + d], out[c + d:])

    def dis_generation(self, kind):
        """Refresh counter of the DIS state of one family kind (0 mean-field, 1 dense, 2 low-rank)."""
        g = ctypes.c_uint64(0)
        self._check(self._lib.vb_dis_generation(self._ctx, int(kind), ctypes.byref(g)))
        return g.value

    def dis_state_park(self, kind, slot=-1):
        """Detach the context's DIS state of ``kind`` (and noise slot ``slot``) into a handle (``vb_dis_state_park``)."""
        h = ctypes.c_void_p()
        self._check(self._lib.vb_dis_state_park(self._ctx, int(kind), int(slot), ctypes.byref(h)))
        return h

    def dis_state_unpark(self, handle):
        self._check(self._lib.vb_dis_state_unpark(self._ctx, handle))

    def dis_state_drop(self, handle):
        self._lib.vb_dis_state_drop(handle)

    def dis_state_get(self, dense, n_total):
        """(log p, log q) of the state samples of the last DIS refresh."""
        lp, lq = np.empty(n_total, dtype=np.float64), np.empty(n_total, dtype=np.float64)
        self._check(self._lib.vb_dis_state_get(self._ctx, int(bool(dense)), _dptr(lp), _dptr(lq), n_total))
        return lp, lq

    def dis_refresh_mvt(self, slot, n, d, df, theta, chi, sqrt_sigma, l_inv, prior_theta, eps_prev, ess_target,
                        max_bisection_its=50, n_total=None, fetch_logs=True):
        theta, prior_theta = _f64(theta), _f64(prior_theta)
        sqrt_sigma = None if sqrt_sigma is None else _f64(sqrt_sigma)   # both None: factors from theta on the device
        l_inv = None if l_inv is None else _f64(l_inv)
        chi = None if chi is None else _f64(chi)       # None: the device draws of chisq_generate
        n_total = n if n_total is None else n_total
        eps, ess = ctypes.c_double(0.0), ctypes.c_double(0.0)
        w = np.empty(n_total, dtype=np.float64)
        lp, lq = ((np.empty(n_total, dtype=np.float64), np.empty(n_total, dtype=np.float64)) if fetch_logs
                  else (None, None))
        self._check(self._lib.vb_dis_refresh_mvt(
            self._ctx, slot, n, d, n_total, float(df), _dptr(theta), None if chi is None else _dptr(chi),
            None if sqrt_sigma is None else _dptr(sqrt_sigma), None if l_inv is None else _dptr(l_inv),
            _dptr(prior_theta), float(eps_prev), float(ess_target), int(max_bisection_its), ctypes.byref(eps),
            ctypes.byref(ess), _dptr(w), None if lp is None else _dptr(lp), None if lq is None else _dptr(lq)))
        return eps.value, ess.value, w, lp, lq

    def dis_refresh_mvt_deferred(self, slot, n, d, df, theta, prior_theta, eps_prev, ess_target, max_bisection_its=50,
                                 n_total=None):
        """Throughput-mode refresh that only ENQUEUES: samples, log p / log q, tempering bisection and the weights stay
        on the device; ``dis_step_mvt_packed`` reads them and synchronises once.  Sharded jobs: ``n`` rows of ``n_total``
        (the three per-sample vectors are gathered on the device, the weights formed redundantly on every rank)."""
        theta, prior_theta = _f64(theta), _f64(prior_theta)
        self._check(self._lib.vb_dis_refresh_mvt(
            self._ctx, slot, n, d, n if n_total is None else n_total, float(df), _dptr(theta), None, None, None,
            _dptr(prior_theta), float(eps_prev), float(ess_target), int(max_bisection_its), None, None, None, None, None))

    def elbo_grad_mvt_symroot(self, slot, n, d, df, theta, path_deriv=False, n_total=None):
        """``(value, grad)`` of the t family's ExclusiveKL in the reference-identical mode, resident on the device
        (``vb_elbo_grad_mvt_symroot`` / ``_path``: symmetric root and its Frechet derivative by device iterations), or None
        when an iteration did not resolve (take the host route)."""
        theta = _f64(theta)
        value = ctypes.c_double(0.0)
        grad = np.empty(d + d * (d + 1) // 2, dtype=np.float64)
        info = np.zeros(4, dtype=np.float64)
        fn = self._lib.vb_elbo_grad_mvt_symroot_path if path_deriv else self._lib.vb_elbo_grad_mvt_symroot
        rc = fn(self._ctx, slot, n, d, n if n_total is None else n_total, float(df), _dptr(theta), ctypes.byref(value),
                _dptr(grad), _dptr(info))
        if rc == VB_ERR_UNSUPPORTED:
            return None
        self._check(rc)
        self.last_root_info = info
        return value.value, grad

    def alpha_grad_mvt_symroot(self, slot, n, d, df, alpha, theta, n_total=None):
        """``(value, grad)`` of the t family's AlphaDivergence in the reference-identical mode, resident on the device
        (``vb_alpha_grad_mvt_symroot``), or None when a root iteration did not resolve (take the host route)."""
        theta = _f64(theta)
        value = ctypes.c_double(0.0)
        grad = np.empty(d + d * (d + 1) // 2, dtype=np.float64)
        info = np.zeros(4, dtype=np.float64)
        rc = self._lib.vb_alpha_grad_mvt_symroot(self._ctx, slot, n, d, n if n_total is None else n_total, float(df),
                                                 float(alpha), _dptr(theta), ctypes.byref(value), _dptr(grad), _dptr(info))
        if rc == VB_ERR_UNSUPPORTED:
            return None
        self._check(rc)
        self.last_root_info = info
        return value.value, grad

    def dis_refresh_mvt_symroot(self, slot, n, d, df, theta, prior_theta, eps_prev, ess_target, max_bisection_its=50,
                                n_total=None):
        """The reference-identical refresh resident on the device (``vb_dis_refresh_mvt_symroot``): the noise in ``slot``
        and the context's chi-square draws are numpy's stream, the samples go through the symmetric root of ``Sigma``
        formed on the device.  Returns ``info = [steps, residual, accuracy]`` of the root, or None when the iteration did
        not resolve it (nothing was installed: take the host route)."""
        theta, prior_theta = _f64(theta), _f64(prior_theta)
        info = np.zeros(3, dtype=np.float64)
        rc = self._lib.vb_dis_refresh_mvt_symroot(self._ctx, slot, n, d, n if n_total is None else n_total, float(df),
                                                  _dptr(theta), _dptr(prior_theta), float(eps_prev), float(ess_target),
                                                  int(max_bisection_its), _dptr(info))
        if rc == VB_ERR_UNSUPPORTED:
            return None
        self._check(rc)
        return info

    def dis_step_mvt_packed(self, n, d, df, theta, scale, resample_m=0, seed=0, stream=0):
        """``(value, grad, eps, ess)``: gradient of ``-scale sum w log q`` on the device-resident tempered weights, or
        on ``resample_m`` multinomial draws from them (then ``scale`` multiplies ``sum w`` on the device)."""
        theta = _f64(theta)
        value, eps, ess, khat = ctypes.c_double(0.0), ctypes.c_double(0.0), ctypes.c_double(0.0), ctypes.c_double(0.0)
        grad = np.empty(theta.size, dtype=np.float64)
        self._check(self._lib.vb_dis_step_mvt_packed(
            self._ctx, n, d, float(df), _dptr(theta), int(resample_m), int(seed), int(stream), float(scale),
            ctypes.byref(eps), ctypes.byref(ess), ctypes.byref(khat), ctypes.byref(value), _dptr(grad)))
        self.last_khat = khat.value          # tail shape of the last dis_psis_mvt (0.0 without one)
        return value.value, grad, eps.value, ess.value

    def dis_psis_mvt(self, n_total, reff=1.0):
        """Enqueue the Pareto smoothing of the device-resident tempered weights (between ``dis_refresh_mvt_deferred``
        and ``dis_step_mvt_packed``; ``last_khat`` after the step)."""
        self._check(self._lib.vb_dis_psis_mvt(self._ctx, int(n_total), float(reff)))

    def dis_clip_mvt(self, n_total, threshold):
        """Enqueue the weight clipping (``objectives.py:370-386``) of the device-resident weights, in place."""
        self._check(self._lib.vb_dis_clip_mvt(self._ctx, int(n_total), float(threshold)))

    def dis_scalars_get(self):
        """``(eps, ess, khat)`` of the last device-resident refresh."""
        out = np.zeros(4, dtype=np.float64)
        self._check(self._lib.vb_dis_scalars_get(self._ctx, _dptr(out)))
        return out[0], out[1], out[3]

    def dis_weights_get(self, n_total, resampled=False):
        w = np.empty(n_total, dtype=np.float64)
        self._check(self._lib.vb_dis_weights_get(self._ctx, _dptr(w), n_total, 1 if resampled else 0))
        return w

    def dis_grad_mvt_packed(self, n, d, df, theta, weights, scale):
        """``(value, grad)`` of ``-scale sum_n w_n log q(x_n; theta)`` with the factor algebra and the chain rule on
        the device (``vb_dis_grad_mvt_packed``)."""
        theta, weights = _f64(theta), _f64(weights)
        value = ctypes.c_double(0.0)
        grad = np.empty(theta.size, dtype=np.float64)
        self._check(self._lib.vb_dis_grad_mvt_packed(self._ctx, n, d, float(df), _dptr(theta), _dptr(weights),
                                                     float(scale), ctypes.byref(value), _dptr(grad)))
        return value.value, grad

    def dis_grad_mvt(self, n, d, df, theta, l_inv, weights):
        theta, l_inv, weights = _f64(theta), _f64(l_inv), _f64(weights)
        w_sum, w_logq = ctypes.c_double(0.0), ctypes.c_double(0.0)
        d_mu = np.empty(d, dtype=np.float64)
        gram = np.empty((d, d), dtype=np.float64)
        self._check(self._lib.vb_dis_grad_mvt(self._ctx, n, d, float(df), _dptr(theta), _dptr(l_inv),
                                              _dptr(weights), ctypes.byref(w_sum), ctypes.byref(w_logq),
                                              _dptr(d_mu), _dptr(gram)))
        return w_sum.value, w_logq.value, d_mu, gram

    # ------------------------------------------------------------------ NVPFlow
    def flow_create(self, d, masks, widths_t, widths_s):
        """A handle holding one flow's masks, architecture and workspace on this context (``vb_flow_create``)."""
        masks = _f64(masks)
        wt = np.ascontiguousarray(widths_t, dtype=np.int64)
        ws = np.ascontiguousarray(widths_s, dtype=np.int64)
        h = ctypes.c_void_p()
        self._check(self._lib.vb_flow_create(self._ctx, int(d), int(masks.shape[0]), _dptr(masks), wt.size - 1,
                                             wt.ctypes.data_as(_c_int64_p), ws.size - 1, ws.ctypes.data_as(_c_int64_p),
                                             ctypes.byref(h)))
        return h.value

    def flow_destroy(self, handle):
        if getattr(self, '_ctx', None):
            self._check(self._lib.vb_flow_destroy(self._ctx, handle))

    def flow_elbo_grad(self, handle, slot, n, n_total, prior_family, prior_df, prior_param, theta, flags):
        """``(value, grad)`` of ExclusiveKL for the flow over the prior draws in ``slot`` (``vb_flow_elbo_grad``)."""
        prior_param = _f64(prior_param)
        theta = _f64(theta)
        out = pinned_array(1 + theta.size)
        self._check(self._lib.vb_flow_elbo_grad(self._ctx, handle, slot, int(n), int(n_total), int(prior_family),
                                                float(prior_df), _dptr(prior_param), _dptr(theta), int(flags),
                                                _dptr(out)))
        return float(out[0]), out[1:]

    def flow_sample(self, handle, slot, n, d, prior_family, prior_df, prior_param, theta, want_x=True, want_log_p=False):
        """``(x or None, log q, log p or None)`` of the flow's forward pass over the prior draws in ``slot``."""
        prior_param = _f64(prior_param)
        theta = _f64(theta)
        x = np.empty((n, d), dtype=np.float64) if want_x else None
        log_q = np.empty(n, dtype=np.float64)
        log_p = np.empty(n, dtype=np.float64) if want_log_p else None
        self._check(self._lib.vb_flow_sample(self._ctx, handle, slot, int(n), int(prior_family), float(prior_df),
                                             _dptr(prior_param), _dptr(theta), _dptr(x) if want_x else None,
                                             _dptr(log_q), _dptr(log_p) if want_log_p else None))
        return x, log_q, log_p

    def flow_fit(self, handle, slot, n, n_total, row_offset, prior_family, prior_df, prior_param, theta, n_iters,
                 opt_kind, hyper, *, flags=0, noise_kind=NOISE_NORMAL, noise_df=0.0, seed=1, first_stream=0,
                 state=None, hist_len=0, log_directions=False, log_gradients=False):
        """``n_iters`` iterations of {Philox prior noise -> flow objective -> optimiser step} enqueued back to back
        (``vb_flow_fit``).  Returns (theta, values, history, state, directions or None, gradients or None) as ``fit``."""
        prior_param = _f64(prior_param)

        def call(hyper_p, theta_p, p, tail):
            return self._lib.vb_flow_fit(
                self._ctx, handle, slot, int(n), int(n_total), int(row_offset), int(prior_family), float(prior_df),
                _dptr(prior_param), int(flags), int(noise_kind), float(noise_df), int(seed), int(first_stream),
                int(opt_kind), hyper_p, int(n_iters), theta_p, *tail)
        return self._fit_call(call, theta, n_iters, hyper, state, hist_len, log_directions, log_gradients)

    # ------------------------------------------------------------------ ExclusiveKL, full rank
    def elbo_grad_fullrank(self, slot, n, d, theta, flags=0, n_total=None):
        theta = _f64(theta)
        p = d + d * (d + 1) // 2
        value = ctypes.c_double(0.0)
        grad = pinned_array(p)
        self._check(self._lib.vb_elbo_grad_fullrank(
            self._ctx, slot, n, d, n if n_total is None else n_total, _dptr(theta), flags,
            ctypes.byref(value), _dptr(grad)))
        return value.value, grad

    def fullrank_set_theta(self, theta, d):
        theta = _f64(theta)
        self._check(self._lib.vb_fullrank_set_theta(self._ctx, _dptr(theta), d))

    def elbo_grad_fullrank_enqueue(self, slot, n, d, flags=0, n_total=None):
        self._check(self._lib.vb_elbo_grad_fullrank_enqueue(
            self._ctx, slot, n, d, n if n_total is None else n_total, flags))

    def fullrank_get(self, d):
        p = d + d * (d + 1) // 2
        value = ctypes.c_double(0.0)
        grad = pinned_array(p)
        self._check(self._lib.vb_fullrank_get(self._ctx, ctypes.byref(value), _dptr(grad), p))
        return value.value, grad

    def fullrank_fold_m(self, d):
        """``M = L' P`` (d x d) of the last folded full-rank evaluation (``vb_fullrank_fold_get_m``)."""
        m = np.empty((d, d), dtype=np.float64)
        self._check(self._lib.vb_fullrank_fold_get_m(self._ctx, _dptr(m), d))
        return m

    # ------------------------------------------------------------------ small dense linear algebra
    def sym_sqrt(self, a, e=None):
        """Symmetric square root of an SPD matrix on the device (``vb_sym_sqrt``); with ``e`` also the solution
        ``x`` of ``root x + x root = e``.  Returns ``(root, x or None, info)`` with
        ``info = [iterations, final residual, ||root root - a||_F / max_i sum_j |a_ij|]``.  Only the symmetric part of
        ``a`` is read.  ``ValueError`` unless ``a`` is a non-empty square matrix and ``e`` has its shape."""
        a, e = _root_arguments(a, e)
        d = a.shape[0]
        root = np.empty((d, d), dtype=np.float64)
        info = np.zeros(3, dtype=np.float64)
        if e is None:
            self._check(self._lib.vb_sym_sqrt(self._ctx, _dptr(a), None, d, _dptr(root), None, _dptr(info)))
            return root, None, info
        x = np.empty((d, d), dtype=np.float64)
        self._check(self._lib.vb_sym_sqrt(self._ctx, _dptr(a), _dptr(e), d, _dptr(root), _dptr(x), _dptr(info)))
        return root, x, info

    def alpha_grad_mvt_chol(self, slot, n, d, df, theta, alpha, n_total=None):
        """AlphaDivergence of the multivariate t in throughput mode (Cholesky sampling, device chi-square draws): value
        and the gradient in the flat layout, nothing of order D^2 on the host."""
        theta = _f64(theta)
        value = ctypes.c_double(0.0)
        grad = np.empty(d + d * (d + 1) // 2, dtype=np.float64)
        self._check(self._lib.vb_alpha_grad_mvt_chol(self._ctx, slot, n, d, n if n_total is None else n_total, float(df),
                                                     _dptr(theta), float(alpha), ctypes.byref(value), _dptr(grad)))
        return value.value, grad

    def alpha_grad_fullrank(self, slot, n, d, theta, alpha, n_total=None):
        theta = _f64(theta)
        p = d + d * (d + 1) // 2
        value = ctypes.c_double(0.0)
        grad = np.empty(p, dtype=np.float64)
        self._check(self._lib.vb_alpha_grad_fullrank(self._ctx, slot, n, d, n if n_total is None else n_total,
                                                     _dptr(theta), float(alpha), ctypes.byref(value), _dptr(grad)))
        return value.value, grad

    def sym_sqrt_inv(self, a):
        """``(root, inverse root, info)`` of an SPD matrix (``vb_sym_sqrt_inv``)."""
        a, _ = _root_arguments(a, None)
        d = a.shape[0]
        root, inv_root = np.empty((d, d), dtype=np.float64), np.empty((d, d), dtype=np.float64)
        info = np.zeros(3, dtype=np.float64)
        self._check(self._lib.vb_sym_sqrt_inv(self._ctx, _dptr(a), None, d, _dptr(root), None, _dptr(info),
                                              _dptr(inv_root)))
        return root, inv_root, info

    def lowrank_path_terms(self, slot_eps, slot_z, n, d, k, sw, n_total=None):
        """Noise-only second moments of the low-rank family's path-derivative estimator (``vb_lowrank_path_terms``):
        ``(E'T (d, 2k), T'T (2k, 2k), sum eps (d), sum eps^2 (d), sum T (2k))`` with ``T = [z | eps sw]``."""
        sw = _f64(sw)
        out = np.empty(d * 2 * k + 4 * k * k + 2 * d + 2 * k, dtype=np.float64)
        self._check(self._lib.vb_lowrank_path_terms(self._ctx, slot_eps, slot_z, n, d, k,
                                                    n if n_total is None else n_total, _dptr(sw), _dptr(out)))
        a, b = d * 2 * k, d * 2 * k + 4 * k * k
        return (out[:a].reshape(d, 2 * k), out[a:b].reshape(2 * k, 2 * k), out[b:b + d], out[b + d:b + 2 * d],
                out[b + 2 * d:])

    def mvt_path_terms(self, slot, n, d, df, inv_s, n_total=None):
        """Noise-only sums of the t family's path-derivative estimator (``vb_mvt_path_terms``):
        ``(m_w, e_w, log1p_sum)``."""
        inv_s = _f64(inv_s)
        m_w = np.empty((d, d), dtype=np.float64)
        e_w = np.empty(d, dtype=np.float64)
        l1p = ctypes.c_double(0.0)
        self._check(self._lib.vb_mvt_path_terms(self._ctx, slot, n, d, n if n_total is None else n_total, float(df),
                                                _dptr(inv_s), _dptr(m_w), _dptr(e_w), ctypes.byref(l1p)))
        return m_w, e_w, l1p.value

    def alpha_sums_mvt(self, slot, n, d, df, alpha, mu, root, inv_s, sum_log_diag, n_total=None):
        """Weighted sample sums of AlphaDivergence over a multivariate t (``vb_alpha_sums_mvt``):
        ``(value, w_sum, g_sum, C)``."""
        mu, root = _f64(mu), _f64(root)
        inv_s = None if inv_s is None else _f64(inv_s)      # None: the device chi-square draws (chisq_generate)
        g_sum = np.empty(d, dtype=np.float64)
        C = np.empty((d, d), dtype=np.float64)
        value, w_sum = ctypes.c_double(0.0), ctypes.c_double(0.0)
        self._check(self._lib.vb_alpha_sums_mvt(self._ctx, slot, n, d, n if n_total is None else n_total, float(df),
                                                float(alpha), _dptr(mu), _dptr(root),
                                                None if inv_s is None else _dptr(inv_s),
                                                float(sum_log_diag), ctypes.byref(value), ctypes.byref(w_sum),
                                                _dptr(g_sum), _dptr(C)))
        return value.value, w_sum.value, g_sum, C

    # ------------------------------------------------------------------ device-resident fit
    def fit(self, slot, n, d, family, theta, n_iters, opt_kind, hyper, *, df=0.0, flags=0, cv_mode=0,
            n_total=None, row_offset=0, noise_kind=NOISE_NORMAL, noise_df=0.0, seed=1, first_stream=0,
            state=None, hist_len=0, log_directions=False, log_gradients=False, slot_aux=-1):
        """``n_iters`` iterations of {Philox noise -> objective -> optimiser step} enqueued back to back
        (``vb_fit``).  Returns (theta, values, history, state, directions or None, gradients or None)."""
        def call(hyper_p, theta_p, p, tail):
            return self._lib.vb_fit(
                self._ctx, slot, slot_aux, n, d, n if n_total is None else n_total, int(row_offset), family, float(df),
                flags, cv_mode, noise_kind, float(noise_df), int(seed), int(first_stream), opt_kind, hyper_p,
                int(n_iters), theta_p, p, *tail)
        return self._fit_call(call, theta, n_iters, hyper, state, hist_len, log_directions, log_gradients)

    def _fit_call(self, call, theta, n_iters, hyper, state, hist_len, log_directions, log_gradients):
        """The buffers every device fit takes and returns.  ``call(hyper, theta, p, tail)`` invokes the C entry point, ``tail``
        being its last seven arguments (state, has_state, values, history, hist_len, directions, gradients)."""
        theta = _f64(theta).copy()
        p = theta.size
        hyper = _f64(np.asarray(hyper, dtype=np.float64))
        has_state = state is not None
        state = _f64(state).copy() if has_state else np.zeros(2 * p, dtype=np.float64)
        values = np.empty(max(int(n_iters), 0), dtype=np.float64)      # (a bad n_iters is the C check's to report)
        history = np.empty((hist_len, p), dtype=np.float64)
        directions = np.empty((n_iters, p), dtype=np.float64) if log_directions else None
        gradients = np.empty((n_iters, p), dtype=np.float64) if log_gradients else None
        self._check(call(_dptr(hyper), _dptr(theta), p, (
            _dptr(state), int(has_state), _dptr(values), _dptr(history) if hist_len else None, int(hist_len),
            _dptr(directions) if log_directions else None, _dptr(gradients) if log_gradients else None)))
        return theta, values, history, state, directions, gradients

    def mvt_route_stats(self):
        """(refreshes that took log p / log prior from the sampling product's epilogue, steps whose chain-rule kernel stored the
        gradient into the mapped result buffer itself) -- ``vb_mvt_route_stats``."""
        a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._check(self._lib.vb_mvt_route_stats(self._ctx, ctypes.byref(a), ctypes.byref(b)))
        return int(a.value), int(b.value)

    def fit_history_mean(self, rows, p):
        """``np.mean(history[-rows:], axis=0)`` of the iterates the last ``fit`` kept, formed on the device from the rows still
        resident there (``vb_fit_history_mean``): the same additions in the same order, without the host's pass over them."""
        mean = pinned_array(p)
        self._check(self._lib.vb_fit_history_mean(self._ctx, int(rows), int(p), _dptr(mean)))
        return mean

    # ------------------------------------------------------------------ device-resident iterate chain
    def chain_open(self, p, capacity_rows):
        """Open the engine's iterate chain: room for ``capacity_rows`` rows of ``p`` doubles on the device, none filled
        (``vb_chain_open``).  While it is open, ``fit`` / ``flow_fit`` with ``hist_len=0`` append their iterates to it."""
        self._check(self._lib.vb_chain_open(self._ctx, int(p), int(capacity_rows)))
        self._chain_p = int(p)

    def chain_close(self):
        """Detach and free the chain (``vb_chain_close``); a no-op when none is open."""
        self._chain_p = None
        self._check(self._lib.vb_chain_close(self._ctx))

    def _chain_dim(self):
        p = getattr(self, '_chain_p', None)
        if p is None:
            raise EngineError('no iterate chain is open (chain_open)')
        return p

    def chain_rows(self):
        """Rows the open chain holds."""
        rows = ctypes.c_int64(0)
        self._check(self._lib.vb_chain_rows(self._ctx, ctypes.byref(rows)))
        return int(rows.value)

    def chain_append(self, rows):
        """Upload ``rows`` (``(n, p)``) behind the chain's last row (``vb_chain_append``)."""
        p = self._chain_dim()
        rows = _f64(np.atleast_2d(rows))
        if rows.ndim != 2 or rows.shape[1] != p:
            raise ValueError('rows must have shape (n, {}), the open chain\'s row length'.format(p))
        self._check(self._lib.vb_chain_append(self._ctx, _dptr(rows), rows.shape[0]))

    def chain_fetch(self, first_row, n_rows):
        """Rows ``[first_row, first_row + n_rows)`` of the chain as an array (``vb_chain_fetch``)."""
        p = self._chain_dim()
        out = np.empty((max(int(n_rows), 0), p), dtype=np.float64)
        self._check(self._lib.vb_chain_fetch(self._ctx, int(first_row), int(n_rows), _dptr(out) if out.size else None))
        return out

    def chain_mean(self, w):
        """``np.mean(chain[-w:], axis=0)`` bit for bit, formed on the device (``vb_chain_mean``)."""
        mean = pinned_array(self._chain_dim())
        self._check(self._lib.vb_chain_mean(self._ctx, int(w), _dptr(mean)))
        return mean

    def chain_rhat(self, windows, jitter=1e-8, per_column=False):
        """``np.max(compute_R_hat(chain[-w:], jitter=jitter))`` for every trailing window ``w`` (``vb_chain_rhat``);
        with ``per_column`` also the ``(len(windows), p)`` values the maxima were taken of."""
        p = self._chain_dim()
        windows = np.ascontiguousarray(np.asarray(windows, dtype=np.int64).ravel())
        worst = np.empty(windows.size, dtype=np.float64)
        rhat = np.empty((windows.size, p), dtype=np.float64) if per_column else None
        self._check(self._lib.vb_chain_rhat(
            self._ctx, windows.ctypes.data_as(_c_int64_p), int(windows.size), float(jitter), _dptr(worst),
            _dptr(rhat) if per_column else None))
        return (worst, rhat) if per_column else worst

    def chain_ess_mcse(self, w):
        """``(ess, mcse)`` arrays of ``_chain_stats.MCSE(chain[-w:])`` (``vb_chain_ess_mcse``)."""
        p = self._chain_dim()
        ess, mcse = np.empty(p, dtype=np.float64), np.empty(p, dtype=np.float64)
        self._check(self._lib.vb_chain_ess_mcse(self._ctx, int(w), _dptr(ess), _dptr(mcse)))
        return ess, mcse

    # ------------------------------------------------------------------ multi-GPU
    @staticmethod
    def comm_unique_id():
        lib = load()
        buf = ctypes.create_string_buffer(COMM_ID_BYTES)
        rc = lib.vb_comm_unique_id(buf)
        if rc != VB_OK:
            raise EngineError('vb_comm_unique_id failed: ' + lib.vb_last_error(None).decode())
        return buf.raw

    def comm_init(self, unique_id, n_ranks, rank):
        self._check(self._lib.vb_comm_init(self._ctx, unique_id, n_ranks, rank))
        self.n_ranks, self.rank = n_ranks, rank

    IPC_HANDLE_BYTES = IPC_HANDLE_BYTES

    def comm_ipc_window(self, cap_doubles=1 << 21):
        """Allocate this rank's window of the xGMI-native transport; returns its IPC handle (64 bytes)."""
        buf = ctypes.create_string_buffer(self.IPC_HANDLE_BYTES)
        self._check(self._lib.vb_comm_ipc_window(self._ctx, int(cap_doubles), buf))
        return buf.raw

    def comm_init_ipc(self, handles, n_ranks, rank):
        """``handles``: the ranks' window handles in rank order (``n_ranks * 64`` bytes)."""
        blob = b''.join(handles)
        if len(blob) != n_ranks * self.IPC_HANDLE_BYTES:
            raise ValueError('expected %d window handles of %d bytes' % (n_ranks, self.IPC_HANDLE_BYTES))
        self._check(self._lib.vb_comm_init_ipc(self._ctx, blob, n_ranks, rank))
        self.n_ranks, self.rank = n_ranks, rank
        self._ipc_on = True

    def comm_init_host(self, collective, n_ranks, rank):
        """Host-staged transport (``vb_comm_init_host``): ``collective(array, op)`` must overwrite the float64
        ``array`` in place with the ranks' elementwise sum (``op == 0``) or maximum (``op == 1``)."""
        def trampoline(_user, buf, count, op):
            try:
                collective(np.ctypeslib.as_array(buf, shape=(count,)), op)
                return 0
            except Exception:                # an exception must not unwind through the C frames
                import traceback
                traceback.print_exc()
                return 1
        cb = HOST_COLLECTIVE_FN(trampoline)
        self._check(self._lib.vb_comm_init_host(self._ctx, ctypes.cast(cb, ctypes.c_void_p), None, n_ranks, rank))
        self._host_collective = cb           # the library keeps the pointer: keep the thunk alive with the engine
        self.n_ranks, self.rank = n_ranks, rank

    def comm_destroy(self):
        self._ipc_on = False
        self._check(self._lib.vb_comm_destroy(self._ctx))
        self._host_collective = None
        self.n_ranks, self.rank = 1, 0

    def comm_allreduce_time(self, count, warm=5, reps=50):
        """Microseconds per sum all-reduce of ``count`` doubles, the collective alone (``vb_comm_allreduce_time``; every
        rank calls it)."""
        us = ctypes.c_double(0.0)
        self._check(self._lib.vb_comm_allreduce_time(self._ctx, int(count), int(warm), int(reps), ctypes.byref(us)))
        return us.value

    def comm_info(self):
        """(ranks, rank) as the RCCL communicator reports them; (1, 0) without a communicator."""
        n, r = ctypes.c_int(0), ctypes.c_int(0)
        self._check(self._lib.vb_comm_info(self._ctx, ctypes.byref(n), ctypes.byref(r)))
        return n.value, r.value

    # ------------------------------------------------------------------ measurement
    def profile_enable(self, on=True):
        self._check(self._lib.vb_profile_enable(self._ctx, int(bool(on))))

    def profile_read(self, reset=True, kernel=PROF_MF_ACCUM):
        """(launches, evaluations, total ms) of one profiled kernel (``PROF_*``) since the last reset."""
        n = ctypes.c_int64(0)
        ev = ctypes.c_int64(0)
        ms = ctypes.c_double(0.0)
        self._check(self._lib.vb_profile_read_kernel(self._ctx, int(kernel), ctypes.byref(n), ctypes.byref(ev),
                                                     ctypes.byref(ms), int(reset)))
        return n.value, ev.value, ms.value


_default_engine = None


_blas_controller = None


def small_lapack(dim):
    """Context manager for the O(D^3) host factorisations that stay on the CPU (``eigh`` of the D x D scale for
    the symmetric root, ``approximations.py:348``): runs them on one BLAS thread when the matrix is small.
    OpenBLAS's threaded ``dsyevd`` is an order of magnitude SLOWER than the serial one at these sizes (256 x 256:
    94 vs 8 ms on 8 cores, 70-95 vs 5 ms on the 256-core GPU host), which made the whole MultivariateT objective
    call host-bound.  No-op when ``threadpoolctl`` is unavailable or ``dim`` > 1024."""
    global _blas_controller
    import contextlib
    if dim > 1024:
        return contextlib.nullcontext()
    if _blas_controller is None:
        try:
            from threadpoolctl import ThreadpoolController
            _blas_controller = ThreadpoolController()
        except Exception:           # pragma: no cover
            _blas_controller = False
    if not _blas_controller:
        return contextlib.nullcontext()
    return _blas_controller.limit(limits=1, user_api='blas')


_blas_sticky = None


def set_host_blas_threads(n=1):
    """Limit the BLAS thread pool of this process (sticky, via ``threadpoolctl``); returns True when applied.

    The host side of the dense-covariance objectives is a handful of D x D numpy products per call.  A threaded
    OpenBLAS leaves its worker threads spinning for ~30 ms after each of them (``OPENBLAS_THREAD_TIMEOUT``);
    inside a CPU-quota cgroup (the MI355X boxes of this pool: 256 visible cores, 64 BLAS threads) the spinning
    exhausts the quota and every few objective calls stall for 30-85 ms -- a 4.6 ms MultivariateT / DIS call
    then averages 25 ms.  One or a few threads are the right setting for matrices of this size;
    ``OPENBLAS_NUM_THREADS=1`` in the environment does the same."""
    global _blas_sticky
    try:
        from threadpoolctl import threadpool_limits
    except Exception:               # pragma: no cover
        return False
    _blas_sticky = threadpool_limits(limits=int(n), user_api='blas')
    return True


_blas_policy_done = False


def apply_host_blas_policy():
    """Called once by the dense-covariance objectives before their first D x D host product: limits the BLAS pool
    to ``VIABEL_AMD_HOST_BLAS_THREADS`` threads (default 1; ``0`` leaves the pool alone) -- see
    ``set_host_blas_threads`` for why."""
    global _blas_policy_done
    if _blas_policy_done:
        return
    _blas_policy_done = True
    try:
        n = int(os.environ.get('VIABEL_AMD_HOST_BLAS_THREADS', '1'))
    except ValueError:
        n = 1
    if n > 0 and _blas_sticky is None:
        set_host_blas_threads(n)


def default_engine():
    """Process-wide engine on device ``LOCAL_RANK`` (0 if unset); created on first use."""
    global _default_engine
    if _default_engine is None:
        _default_engine = Engine()
    return _default_engine


def set_default_engine(engine):
    global _default_engine
    _default_engine = engine
