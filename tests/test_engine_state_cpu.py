"""CPU: bookkeeping of the engine's state that no GPU test would notice going wrong.

- ``vb_destroy`` frees every device buffer of the context (a buffer it does not name leaks with every destroyed engine);
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


def ctx_device_buffers():
    """Every ``DeviceBuffer`` member of ``struct vb_ctx``, nested structs' members qualified (``temper.buf``)."""
    with open(os.path.join(CSRC, 'vb_common.h')) as f:
        body = _block(_strip_comments(f.read()), 'struct vb_ctx {')
    levels = [[]]           # DeviceBuffer members of the struct being read, innermost last
    text, inner = '', None
    for tok in re.split(r'([{};])', body):
        if tok == '{':      # a nested struct, or a braced initializer
            levels.append([])
            text, inner = '', None
        elif tok == '}':
            inner = levels.pop()
            text = ''
        elif tok == ';':
            if inner is not None:       # `} member;` ends a nested struct: its buffers are the member's
                member = re.fullmatch(r'\s*(\w+)(?:\[\w*\])?\s*', text)
                if member:
                    levels[-1].extend(member.group(1) + '.' + n for n in inner)
            else:
                m = re.match(r'\s*(?:vb::)?DeviceBuffer\s+(.+)$', text, flags=re.S)
                if m:
                    levels[-1].extend(re.match(r'\s*(\w+)', decl).group(1) for decl in m.group(1).split(','))
            text, inner = '', None
        else:
            text += tok
    assert len(levels) == 1
    return levels[0]


def test_destroy_frees_every_device_buffer_of_the_context():
    buffers = ctx_device_buffers()
    assert {'dis_state', 'mvt_state', 'lr_obj', 'temper.buf', 'temper.work', 'fz_words', 'fz_items'} <= set(buffers), buffers
    with open(os.path.join(CSRC, 'vb_api.hip')) as f:
        destroy = _block(_strip_comments(f.read()), 'int vb_destroy(vb_ctx* ctx)')
    missing = [b for b in buffers if not re.search(r'ctx->' + re.escape(b) + r'\b', destroy)]
    assert not missing, 'vb_destroy does not free: ' + ', '.join(missing)


def test_objective_state_slots_are_distinct():
    """Slot 0: a call's noise; 3: the low-rank block; 2: the diagnostics; the last: sample(); one DIS slot per kind."""
    from viabel_amd import _lib
    from viabel_amd.convenience import _DIAG_SLOT
    from viabel_amd.objectives import _DIS_SLOTS, _LR_SLOT, _NOISE_SLOT
    assert sorted(_DIS_SLOTS) == [0, 1, 2]
    slots = [_NOISE_SLOT, _LR_SLOT, _DIAG_SLOT, _lib.MAX_SLOTS - 1] + list(_DIS_SLOTS.values())
    assert len(set(slots)) == len(slots), slots
    assert all(0 <= s < _lib.MAX_SLOTS for s in slots)
