"""CPU: bookkeeping of the engine's state that no GPU test would notice going wrong.

- every GPU resource is held by an owning type, so ``vb_destroy`` has no list from which a buffer could be missing
  (``tests/test_gpu_engine_resources.py`` counts the live resources on the GPU);
- the noise slots the objectives keep state in between calls are distinct, so that objectives of different kinds taking
  turns on one engine never read each other's draws (``tests/test_gpu_shared_engine.py`` runs the interleavings)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'viabel_amd', 'csrc')


def _strip_comments(src):
    return re.sub(r'//[^\n]*', '', re.sub(r'/\*.*?\*/', '', src, flags=re.S))


def _block(src, opener):
    """The text between the brace that follows `opener` and its matching closing brace."""
    at = src.index(opener)
    start = src.index('{', at)
    depth = 0
    for i in range(start, len(src)):
        if src[i] == '{':
            depth += 1
        elif src[i] == '}':
            depth -= 1
            if depth == 0:
                return src[start + 1:i]
    raise AssertionError('unbalanced braces after ' + opener)


# the runtime calls that make or release a device buffer, a page-locked block, an event or a stream
RESOURCE_API = [r'\bhipMalloc\(', r'\bhipFree\(', r'\bhipHostMalloc\(', r'\bhipHostFree\(', r'\bhipEventCreate',
                r'\bhipEventDestroy\(', r'\bhipStreamCreate', r'\bhipStreamDestroy\(']
RESOURCE_HEADER = 'vb_resource.h'
# ... and the only functions outside the resource header that may use them
ALLOWED = [('vb_comm.hip', 'int vb_comm_ipc_window('),         # IPC set-up: a protocol with the peers,
           ('vb_comm.hip', 'int vb_comm_destroy('),            # ... and its teardown
           ('vb_comm.hip', 'int vb_comm_allreduce_time('),     # two local timing events
           ('vb_api.hip', 'int vb_host_alloc('),               # blocks that belong to the caller
           ('vb_api.hip', 'int vb_host_free(')]
CTX_ALIASES = {'mvt_ev_fork', 'result_stream'}                 # non-owning handles of vb_ctx


def _uses(text):
    return [pat for pat in RESOURCE_API if re.search(pat, text)]


def test_resources_are_owned_by_the_resource_types():
    """Ownership is in the types of vb_resource.h, so that ``delete ctx`` releases everything and a new buffer cannot be
    forgotten: nothing else in the engine allocates, creates, frees or destroys, ``vb_destroy`` least of all, and the
    context keeps no raw event or stream of its own."""
    sources = {}
    for name in sorted(os.listdir(CSRC)):
        if name.endswith(('.hip', '.h', '.cpp')):
            with open(os.path.join(CSRC, name)) as f:
                sources[name] = _strip_comments(f.read())
    assert _uses(sources[RESOURCE_HEADER])
    destroy = _block(sources['vb_api.hip'], 'int vb_destroy(vb_ctx* ctx)')
    assert not _uses(destroy), _uses(destroy)
    assert 'delete ctx' in destroy
    for name, opener in ALLOWED:
        body = _block(sources[name], opener)
        assert _uses(body), 'stale allow-list entry: %s %s' % (name, opener)
        sources[name] = sources[name].replace(body, '')
    stray = {name: _uses(text) for name, text in sources.items() if name != RESOURCE_HEADER and _uses(text)}
    assert not stray, stray
    ctx = _block(sources['vb_common.h'], 'struct vb_ctx {')
    raw = [re.match(r'\W*(\w+)', decl).group(1)
           for m in re.finditer(r'\bhip(?:Event|Stream)_t\b([^;(]*);', ctx) for decl in m.group(1).split(',')]
    assert set(raw) == CTX_ALIASES, raw


def test_objective_state_slots_are_distinct():
    """Slot 0: a call's noise; 3: the low-rank block; 2: the diagnostics; the last: sample(); one DIS slot per kind."""
    from viabel_amd import _lib
    from viabel_amd.convenience import _DIAG_SLOT
    from viabel_amd.objectives import _DIS_SLOTS, _LR_SLOT, _NOISE_SLOT
    assert sorted(_DIS_SLOTS) == [0, 1, 2]
    slots = [_NOISE_SLOT, _LR_SLOT, _DIAG_SLOT, _lib.MAX_SLOTS - 1] + list(_DIS_SLOTS.values())
    assert len(set(slots)) == len(slots), slots
    assert all(0 <= s < _lib.MAX_SLOTS for s in slots)
