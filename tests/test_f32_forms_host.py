"""f32_forms.py without a GPU: the workspace's range-report state machine (word, mark, latch) on a CPU workspace, the re-entrant
form blocks, what a failed launch resets, the detectors' workspace following their device, and the module's layout."""
import ast
import os
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'tf_eager_object_detection_amd')
MOVED = ('_F32_CTX', 'current_f32_form', 'f32_form', '_GRAD_CTX', 'GRAD_FORMS', 'current_grad_form', 'check_grad_form', 'grad_form',
         'carries_grad_form', 'split_bf16x3', 'f16x2_exponent', 'split_f16x2', 'X3Workspace', '_X3_WS', '_x3_workspace',
         '_F32_FORMS', '_f32_sym', '_f32_call')


def _workspace():
    from tf_eager_object_detection_amd import f32_forms, _lib
    ws = f32_forms.X3Workspace('cpu')
    return ws, int(_lib.lib().odet_x2_status_offset())


def test_workspace_report_state_machine():
    """the status word, the mark (unchecked launches went before) and the latch (a report the caller has not seen)"""
    ws, off = _workspace()
    assert ws.passed() and ws.range_ok()
    # a checked pass's own report: the pass is repeated, the caller is not bothered
    ws.range_flag().fill_(1)
    assert not ws.passed() and int(ws.range_flag().item()) == 0
    assert ws.range_ok()
    # unchecked launches went before: the report cannot be the checked pass's alone, it stays for the caller -- once
    ws.mark_unchecked()
    ws.range_flag().fill_(1)
    assert not ws.passed() and int(ws.range_flag().item()) == 0
    assert not ws.range_ok()
    assert ws.range_ok()
    # a clear word takes the mark away: a word set later is the next pass's own
    ws.mark_unchecked()
    assert ws.passed()
    ws.range_flag().fill_(1)
    assert not ws.passed()
    assert ws.range_ok()
    # the caller's read takes word, latch and mark
    ws.mark_unchecked()
    ws.range_flag().fill_(1)
    assert not ws.range_ok() and int(ws.range_flag().item()) == 0
    ws.range_flag().fill_(1)
    assert not ws.passed() and ws.range_ok()
    # reset(): every ticket byte, never the word
    ws.buf[8] = 7
    ws.buf[off - 1] = 3
    ws.range_flag().fill_(1)
    ws.reset()
    assert int(ws.buf[:off].max().item()) == 0 and int(ws.range_flag().item()) == 1
    assert not ws.range_ok()
    assert ws.range_ok()


@pytest.mark.parametrize('kind', ['f32', 'grad'])
@pytest.mark.parametrize('unwind', [False, True])
def test_form_blocks_are_reentrant(kind, unwind):
    """ONE block object entered twice, nested, around another block: every exit restores what its own entry replaced, on the
    normal way out and when an exception unwinds the blocks"""
    from tf_eager_object_detection_amd import f32_forms as ff
    if kind == 'f32':
        block, current, outer, inner = ff.f32_form, ff.current_f32_form, 'x3', 'x2'
    else:
        block, current, outer, inner = ff.grad_form, ff.current_grad_form, 'x3', 'exact'
    base = current()
    assert base == 'exact'
    seen = []
    again = block(outer)
    try:
        with again:
            seen.append(current())
            try:
                with again:
                    seen.append(current())
                    try:
                        with block(inner):
                            seen.append(current())
                            if unwind:
                                raise KeyError('unwind')
                    finally:
                        seen.append(current())
            finally:
                seen.append(current())
    except KeyError:
        assert unwind
    else:
        assert not unwind
    seen.append(current())
    assert seen == [outer, outer, inner, outer, outer, 'exact']
    assert not again._tokens


def test_failed_launch_resets_the_tickets_of_its_own_workspace_only(monkeypatch):
    from tf_eager_object_detection_amd import f32_forms as ff, _lib
    used, other = ff.X3Workspace('cpu'), ff.X3Workspace('cpu')
    for ws in (used, other):
        ws.buf[4] = 1
        ws.range_flag().fill_(1)
    calls = []

    def fail(sym, *args):
        calls.append((sym, args))
        raise _lib.OdetError('launch failed')
    monkeypatch.setattr(_lib, 'call', fail)
    with pytest.raises(_lib.OdetError, match='launch failed'):
        ff._f32_call(used, 'odet_pointwise_x2', 1, 2)
    assert calls == [('odet_pointwise_x2', (1, 2))]
    assert int(used.buf[4].item()) == 0 and int(used.range_flag().item()) == 1           # tickets reset, the report kept
    assert int(other.buf[4].item()) == 1 and int(other.range_flag().item()) == 1         # not the launch's: untouched
    with pytest.raises(_lib.OdetError):
        ff._f32_call(None, 'odet_pointwise_f32')                                         # ('exact' / float16: nothing to reset)
    assert int(other.buf[4].item()) == 1


def test_detector_workspace_follows_the_parameters_device(monkeypatch):
    from tf_eager_object_detection_amd import ops
    from tf_eager_object_detection_amd.model import detector_base
    made = []

    class Recorder:
        def __init__(self, device):
            self.buf = types.SimpleNamespace(device=device)
            made.append(self)
    monkeypatch.setattr(ops, 'X3Workspace', Recorder)

    class Stub:
        device = torch.device('cuda', 0)

        def parameters(self):
            return iter([types.SimpleNamespace(device=self.device)])
    model = Stub()
    first = detector_base._x3_workspace_of(model)
    assert detector_base._x3_workspace_of(model) is first and made == [first] and first.buf.device == torch.device('cuda', 0)
    model.device = torch.device('cuda', 1)
    second = detector_base._x3_workspace_of(model)
    assert second is not first and second.buf.device == torch.device('cuda', 1)
    assert detector_base._x3_workspace_of(model) is second and made == [first, second]
    off_gpu = Stub()
    off_gpu.device = torch.device('cpu')
    assert detector_base._x3_workspace_of(off_gpu) is None and made == [first, second]       # (nothing launches there: none made)


def test_module_layout():
    """ops hands out f32_forms' own objects; f32_forms knows nothing of ops; ops.py imports only in its header"""
    from tf_eager_object_detection_amd import derived, f32_forms, ops
    for name in MOVED:
        assert getattr(ops, name) is getattr(f32_forms, name), name
    assert ops.invalidate_planes is derived.invalidate and not hasattr(f32_forms, 'invalidate_planes')

    def imports(path):
        tree = ast.parse(open(path).read())
        return tree, [n for n in ast.walk(tree) if isinstance(n, (ast.Import, ast.ImportFrom))]
    _, found = imports(os.path.join(PKG, 'f32_forms.py'))
    package = set()                              # what it imports from its own package: `from . import a`, `from .b import c`
    for node in found:
        if isinstance(node, ast.ImportFrom) and node.level:
            package |= {node.module} if node.module else {a.name for a in node.names}
        else:
            assert 'tf_eager_object_detection_amd' not in ast.dump(node)
    assert package == {'_lib', 'derived'}
    tree, found = imports(os.path.join(PKG, 'ops.py'))
    header = 0                                   # the module's leading statements: docstring, then imports
    for node in tree.body[1:]:
        if not isinstance(node, (ast.Import, ast.ImportFrom)):
            break
        header = node.end_lineno
    assert header and all(node.end_lineno <= header for node in found), [n.lineno for n in found if n.end_lineno > header]
