"""The split-precision backward without a GPU (csrc/grad_gemm.h: dg_tile_x3; odet_dense_dgrad_x3, odet_dense_wgrad_x3,
odet_conv3x3_wgrad_x3_levels): the ABI, the refusals before any device call, the plan and workspace queries as functions of the
shape, which instantiation every shape of the GPU grids reaches, ops.grad_form, the models' keyword, and the proofs of the data
tests/test_grad_x3_gpu.py runs."""
import os
import re
import threading

import numpy as np
import pytest
import torch

import conv_tile_cases as ct
import exact_data as ed
import grad_x3_cases as gx
import test_conv_grad_host as cgh
import test_dense_grad_host as dgh

NEW = ('odet_dense_grad_x3_workspace_bytes', 'odet_dense_grad_x3_plan', 'odet_dense_dgrad_x3', 'odet_dense_wgrad_x3',
       'odet_conv3x3_wgrad_x3_workspace_bytes', 'odet_conv3x3_wgrad_x3_plan', 'odet_conv3x3_wgrad_x3_levels')


def test_header_library_and_binding_agree_on_the_new_symbols():
    from tf_eager_object_detection_amd import _lib
    header = open(os.path.join(gx.ROOT, 'include', 'odet.h')).read()
    L = _lib.lib()
    for name in NEW:
        assert re.search(r'\b%s\(' % name, header), name
        assert name in _lib.SIGNATURES and getattr(L, name) is not None
        assert 'debug' not in name and 'diag' not in name
    assert L.odet_version() == 103
    # the exact form's signatures, argument for argument
    for x3, f32 in (('odet_dense_dgrad_x3', 'odet_dense_dgrad_f32'), ('odet_dense_wgrad_x3', 'odet_dense_wgrad_f32'),
                    ('odet_conv3x3_wgrad_x3_levels', 'odet_conv3x3_wgrad_f32_levels'),
                    ('odet_dense_grad_x3_workspace_bytes', 'odet_dense_grad_workspace_bytes'),
                    ('odet_conv3x3_wgrad_x3_workspace_bytes', 'odet_conv3x3_wgrad_workspace_bytes')):
        assert _lib.SIGNATURES[x3] == _lib.SIGNATURES[f32]


@pytest.mark.parametrize('kind', ['dgrad', 'wgrad'])
def test_dense_entry_points_refuse_bad_arguments_before_any_device_call(kind):
    L = gx.lib()
    fn, who = getattr(L, 'odet_dense_%s_x3' % kind), b'odet_dense_%s_x3' % kind.encode()
    for label, bad in dgh._ROWS[kind]:
        args = dict(dgh._GOOD)
        args.update(bad)
        rc = fn(*[args[n] for n in dgh._NAMES[kind]])
        msg = L.odet_last_error()
        assert rc == -1, '%s: %s returned %d: %r' % (kind, label, rc, msg)
        assert msg.startswith(who) and b' failed: ' not in msg, msg                                  # (no HIP call was made)
    s = dgh._SPLIT[kind]
    assert gx.dense_plan(kind, (s['rows'], s['cin'], s['cout']))[1] > 1
    need = L.odet_dense_grad_x3_workspace_bytes(1 if kind == 'wgrad' else 0, s['rows'], s['cin'], s['cout'])
    assert need >= 2 * 4 * s['cin'] * (s['cout'] if kind == 'wgrad' else s['rows'])
    for label, bad, want in (('no workspace', dict(ws=None, ws_bytes=need), -2), ('one byte short', dict(ws=0x100000, ws_bytes=need - 1), -2),
                             ('workspace of 0 bytes', dict(ws=0x100000, ws_bytes=0), -2),
                             ('misaligned workspace', dict(ws=0x100004, ws_bytes=need), -1)):
        args = dict(dgh._GOOD, **s)
        args.update(bad)
        rc = fn(*[args[n] for n in dgh._NAMES[kind]])
        msg = L.odet_last_error()
        assert rc == want and msg.startswith(who) and b' failed: ' not in msg, (label, rc, msg)
        assert want != -2 or b'odet_dense_grad_x3_workspace_bytes' in msg


def _conv_call(L, **over):
    a = dict(cgh._GOOD, **over)
    lv = cgh._levels(a['levels']) if a['levels'] is not None else None
    n = len(a['levels']) if a['n'] is None else a['n']
    return L.odet_conv3x3_wgrad_x3_levels(lv, n, a['dw'], a['db'], a['batch'], a['cin'], a['cout'], a['ws'], a['ws_bytes'], None)


def test_conv_entry_point_refuses_bad_arguments_before_any_device_call():
    from tf_eager_object_detection_amd import _lib
    L = gx.lib()
    LEVEL, GOOD = cgh._LEVEL, cgh._GOOD
    lvl = lambda **k: [tuple(k.get(n, v) for n, v in zip(('x', 'dy', 'y', 'H', 'W'), LEVEL))]
    rows = [('null levels', dict(levels=None, n=1)), ('null dw', dict(dw=None)), ('null x', dict(levels=lvl(x=None))),
            ('null dy', dict(levels=lvl(dy=None))), ('cin 48', dict(cin=48)), ('cin 0', dict(cin=0)), ('cout 96', dict(cout=96)),
            ('cout 0', dict(cout=0)), ('B 0', dict(batch=0)), ('B -1', dict(batch=-1)), ('H 0', dict(levels=lvl(H=0))),
            ('W 0', dict(levels=lvl(W=0))), ('0 levels', dict(n=0)), ('MAX + 1 levels', dict(levels=[LEVEL] * (_lib.MAX_LEVELS + 1))),
            ('misaligned x', dict(levels=lvl(x=LEVEL[0] + 4))), ('misaligned dy', dict(levels=lvl(dy=LEVEL[1] + 4))),
            ('misaligned y_relu', dict(levels=lvl(y=LEVEL[2] + 4))), ('misaligned dw', dict(dw=GOOD['dw'] + 4)),
            ('misaligned db', dict(db=GOOD['db'] + 2)), ('a bad second level', dict(levels=[LEVEL, LEVEL[:3] + (0, 3)]))]
    for label, bad in rows:
        rc = _conv_call(L, **bad)
        msg = L.odet_last_error()
        assert rc == -1, '%s returned %d: %r' % (label, rc, msg)
        assert msg.startswith(b'odet_conv3x3_wgrad_x3_levels') and b' failed: ' not in msg, msg
    split = dict(levels=[LEVEL[:3] + (17, 40)])
    need = L.odet_conv3x3_wgrad_x3_workspace_bytes(cgh._levels(split['levels']), 1, 1, 64, 64)
    assert need == gx.conv_plan(([(17, 40)], 1, 64, 64))[1] * 64 * 9 * 64 * 4 > 0
    for label, bad, want in (('no workspace', dict(ws=None, ws_bytes=need), -2), ('one byte short', dict(ws=0x100000, ws_bytes=need - 1), -2),
                             ('workspace of 0 bytes', dict(ws=0x100000, ws_bytes=0), -2),
                             ('misaligned workspace', dict(ws=0x100004, ws_bytes=need), -1)):
        rc = _conv_call(L, **dict(split, **bad))
        msg = L.odet_last_error()
        assert rc == want and msg.startswith(b'odet_conv3x3_wgrad_x3_levels') and b' failed: ' not in msg, (label, rc, msg)
        assert want != -2 or b'odet_conv3x3_wgrad_x3_workspace_bytes' in msg


def test_plan_queries_refuse_what_the_entry_points_refuse():
    import ctypes as C
    L = gx.lib()
    t, p = C.c_int(), C.c_int()
    for bad in ((0, 0, 64, 64), (1, 5, 48, 64), (1, 5, 64, 96), (0, 5, 32, 64)):
        assert L.odet_dense_grad_x3_plan(*bad, C.byref(t), C.byref(p)) == -1 and L.odet_last_error().startswith(b'odet_dense_grad_x3_plan')
    assert L.odet_dense_grad_x3_plan(1, 5, 64, 64, None, C.byref(p)) == -1
    lv = gx.levels([(5, 7)])
    for bad in ((0, 1, 64, 64), (9, 1, 64, 64), (1, 0, 64, 64), (1, 1, 48, 64), (1, 1, 64, 96)):
        assert L.odet_conv3x3_wgrad_x3_plan(lv, *bad, C.byref(t), C.byref(p)) == -1
        assert L.odet_last_error().startswith(b'odet_conv3x3_wgrad_x3_plan')
    assert L.odet_conv3x3_wgrad_x3_plan(None, 1, 1, 64, 64, C.byref(t), C.byref(p)) == -1
    assert L.odet_conv3x3_wgrad_x3_plan(gx.levels([(0, 7)]), 1, 1, 64, 64, C.byref(t), C.byref(p)) == -1


def test_plan_and_workspace_are_functions_of_the_shape_alone():
    """asked twice, in two orders, with different pointers in the levels: the same answers; the workspace is parts x the output
    where the plan cuts the contraction and 0 where it does not; the contraction is cut into parts of at least 128 k on average
    (K // parts >= 128: the rule the header, DESIGN and include/odet.h state)"""
    L = gx.lib()
    first = {}
    for rnd in range(2):
        for shape in (gx.DENSE_SHAPES if rnd == 0 else gx.DENSE_SHAPES[::-1]):
            rows, cin, cout = shape
            for kind in ('dgrad', 'wgrad'):
                t, parts = gx.dense_plan(kind, shape)
                ws = L.odet_dense_grad_x3_workspace_bytes(1 if kind == 'wgrad' else 0, *shape)
                K, N = (rows, cout) if kind == 'wgrad' else (cout, rows)
                assert t in (64, 128) and 1 <= parts <= 8 and (parts == 1 or K // parts >= 128)
                assert ws == (parts * N * cin * 4 if parts > 1 else 0)
                assert first.setdefault((kind, shape), (t, parts, ws)) == (t, parts, ws)
        for case in (gx.CONV_CASES if rnd == 0 else gx.CONV_CASES[::-1]):
            maps, batch, cin, cout = case
            t, parts = gx.conv_plan(case)
            lv = gx.levels(maps, ptrs=(0x1000 * (rnd + 1), 0x2000, None))                 # (the queries read no pointer)
            ws = L.odet_conv3x3_wgrad_x3_workspace_bytes(lv, len(maps), batch, cin, cout)
            K = gx.conv_pixels(maps, batch)
            assert t == (128 if cin % 128 == 0 and cout % 128 == 0 else 64) and 1 <= parts <= 16
            assert parts == 1 or (K >= 256 and K // parts >= 128)
            assert ws == (parts * cout * 9 * cin * 4 if parts > 1 else 0)
            key = ('conv', str(case))
            assert first.setdefault(key, (t, parts, ws)) == (t, parts, ws)
    assert L.odet_dense_grad_x3_workspace_bytes(1, 0, 64, 64) == 0
    assert L.odet_conv3x3_wgrad_x3_workspace_bytes(None, 1, 1, 64, 64) == 0
    # the 800 x 1333 pyramid of the RPN head: 72 tiles of 128^2, 7 parts
    assert gx.conv_plan(([(200, 334), (100, 167), (50, 84), (25, 42), (13, 21)], 1, 256, 512)) == (128, 7)


def test_every_instantiation_split_and_unsplit_is_reached_by_the_gpu_grids():
    """The launcher has k_dense_grad<4 | 2, K-major | N-major B, X3> and k_conv3x3_wgrad<4 | 2, X3>.  Each is reached split and
    unsplit, except the 128-edge dense tile split: the plan takes that tile from 256 tiles on and splits up to 128 (dgx_plan)."""
    for (kind, edge, split), shape in gx.DENSE_REACH.items():
        assert shape in gx.DENSE_SHAPES
        t, parts = gx.dense_plan(kind, shape)
        assert (t, parts > 1) == (edge, split), (kind, shape, t, parts)
    seen = {(kind, gx.dense_plan(kind, s)[0], gx.dense_plan(kind, s)[1] > 1) for s in gx.DENSE_SHAPES for kind in ('dgrad', 'wgrad')}
    assert seen == set(gx.DENSE_REACH)
    for (edge, split), case in gx.CONV_REACH.items():
        assert case in gx.CONV_CASES
        t, parts = gx.conv_plan(case)
        assert (t, parts > 1) == (edge, split), (case, t, parts)
    assert {(gx.conv_plan(c)[0], gx.conv_plan(c)[1] > 1) for c in gx.CONV_CASES} == set(gx.CONV_REACH)


# ---- ops.grad_form ----------------------------------------------------------------------------------------------------------------
def test_grad_form_default_values_and_refusals():
    from tf_eager_object_detection_amd import ops
    assert ops.current_grad_form() == 'exact'
    with ops.grad_form('x3'):
        assert ops.current_grad_form() == 'x3'
        with ops.grad_form('exact'):
            assert ops.current_grad_form() == 'exact'
        assert ops.current_grad_form() == 'x3'
        assert ops.current_f32_form() == 'exact'                                     # (beside f32_form, not part of it)
    assert ops.current_grad_form() == 'exact'
    for bad in ('x2', 'X3', 'bf16', '', None, 3):
        with pytest.raises(ValueError, match='grad form'):
            ops.grad_form(bad)


def test_grad_form_is_per_thread_context():
    from tf_eager_object_detection_amd import ops
    seen, go, done = {}, threading.Event(), threading.Event()

    def other():
        seen['start'] = ops.current_grad_form()
        with ops.grad_form('x3'):
            go.set()
            done.wait(10)
            seen['inside'] = ops.current_grad_form()
        seen['after'] = ops.current_grad_form()

    t = threading.Thread(target=other)
    with ops.grad_form('x3'):
        t.start()
        assert go.wait(10)
    assert ops.current_grad_form() == 'exact'                 # the other thread is still inside its block
    done.set()
    t.join(10)
    assert seen == {'start': 'exact', 'inside': 'x3', 'after': 'exact'}


def test_fronts_still_refuse_the_split_f32_forms_whatever_the_grad_form():
    from tf_eager_object_detection_amd import ops
    dy, w, x = torch.zeros(5, 64), torch.zeros(64, 64), torch.zeros(5, 64)
    m = [torch.zeros(1, 3, 4, 64)]
    for f32 in ('x3', 'x2'):
        with ops.f32_form(f32), ops.grad_form('x3'):
            for call in (lambda: ops.dense_dgrad(dy, w), lambda: ops.dense_wgrad(dy, x), lambda: ops.dense_trainable(x, w, None),
                         lambda: ops.conv3x3_wgrad_f32_levels(m, m), lambda: ops.conv3x3_dgrad_f32_levels(m, torch.zeros(64, 3, 3, 64)),
                         lambda: ops.conv3x3_trainable_levels(m, torch.zeros(64, 3, 3, 64), None)):
                with pytest.raises(ValueError, match="only under f32_form 'exact'"):
                    call()
    with ops.grad_form('x3'):                                 # the fronts' other rules are the exact form's: no CPU path
        with pytest.raises(ValueError, match='must be a GPU tensor'):
            ops.dense_wgrad(dy, x)
        with pytest.raises(ValueError, match='float32'):
            ops.dense_dgrad(dy.half(), w.half())


def test_model_keyword():
    from tf_eager_object_detection_amd.model.base_faster_rcnn_model import ResNetFasterRcnn, TrainableResNetFasterRcnn, Vgg16FasterRcnn
    from tf_eager_object_detection_amd.model.base_fpn_model import ResnetV1Fpn
    for cls in (ResnetV1Fpn, Vgg16FasterRcnn, TrainableResNetFasterRcnn):
        m = cls(device='cpu')
        assert m.grad_form == 'exact' and m.dense.grad_form == 'exact'
        for bad in ('x2', 'junk', None):
            with pytest.raises(ValueError, match='grad form'):
                cls(device='cpu', grad_form=bad)
        # what the train keywords refuse today, they refuse with grad_form='x3' too, in the same words
        for kw in (dict(f32_form='x3'), dict(dtype=torch.float16)):
            with pytest.raises(ValueError, match="needs dtype=torch.float32 and f32_form='exact'"):
                cls(device='cpu', grad_form='x3', train_roi_head=True, **kw)
    m = ResnetV1Fpn(device='cpu', grad_form='x3', train_roi_head=True, train_rpn_head=True, train_neck=True, train_extractor=True)
    assert m.grad_form == 'x3' and m.dense.grad_form == 'x3'
    with pytest.raises(TypeError):
        ResNetFasterRcnn(device='cpu', grad_form='x3')
    assert ResNetFasterRcnn(device='cpu').grad_form == 'exact'


# ---- the data of the GPU tests ----------------------------------------------------------------------------------------------------
def test_the_header_states_the_six_products_of_the_forward_form():
    assert gx.kept_products() == ct.kept_products(3)


def test_integer_data_lives_in_the_top_limb_alone():
    a, b, _ = gx.integer_operands(ed.Gen(1), 96, 64, 64)
    assert gx.dense_plan('wgrad', (96, 64, 64)) == (64, 1)                         # (the launch this data is for: one tile, whole)
    for t in (a, b, gx.gates(ed.Gen(2), (8, 8)) * 0 + 3.0):
        top, mid, low = ct.split_limbs(t, 3)
        assert torch.equal(top, t) and not mid.any() and not low.any()
    prods, _ = gx.limb_products(a, b)
    assert torch.equal(prods[(1, 1)], b.t() @ a) and all(not v.any() for k, v in prods.items() if k != (1, 1))


def test_limb_sensitive_data_exercises_every_kept_product_and_no_dropped_one():
    kept, dropped = gx.kept_products()
    hit = set()
    for kind in gx.LIMB_KINDS:
        a, b, q = gx.limb_operands(ed.Gen(7), kind, 64, 64, 64)
        prods, abs_total = gx.limb_products(a, b)
        ed.prove_f32_exact(abs_total, q, quanta=(a, b))
        full = sum(prods[p] for p in kept)
        assert torch.equal(full, b.t() @ a)                   # nothing dropped is missing: the kept sum IS the product
        f32 = lambda t: t.float()
        assert torch.equal(f32(full).double(), full)
        # (A limb, B limb): conv_tile_cases names (x limb, w limb) with x = A
        for p in ct.LIMB_KIND_PRODUCTS[(3, kind)]:
            assert p in kept and prods[p].any()
            assert not torch.equal(f32(full - prods[p]), f32(full)), (kind, p)       # leaving it out changes the float32 result
            hit.add(p)
        for p in prods:
            if p not in ct.LIMB_KIND_PRODUCTS[(3, kind)]:
                assert not prods[p].any(), (kind, p)
    assert hit == set(kept) and not hit & set(dropped)


def test_the_witness_separates_the_kept_products_from_the_exact_form():
    a, b, kept_want, exact_want = gx.witness_operands(17, 64, 64)
    value, abs_total = gx.kept_value(a, b)
    assert torch.equal(value, torch.full((64, 64), kept_want, dtype=torch.float64))
    ed.prove_f32_exact(abs_total, 2.0 ** -18, quanta=(a, b))               # every partial sum of limb products, in any order
    prods, _ = gx.limb_products(a, b)
    _, dropped = gx.kept_products()
    assert torch.equal(sum(prods[p] for p in dropped), torch.full((64, 64), 2.0 ** -27, dtype=torch.float64))
    assert torch.equal(prods[(2, 3)], torch.full((64, 64), 2.0 ** -27, dtype=torch.float64))
    assert gx.fused_chain(a[:, 0], b[:, 0]) == exact_want == 2.0 ** -27 != kept_want
    assert torch.equal(b.t() @ a, torch.full((64, 64), 2.0 ** -27, dtype=torch.float64))           # (the float64 truth is the exact form's)
