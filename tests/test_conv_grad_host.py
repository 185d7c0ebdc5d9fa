"""The 3x3 convolution backward without a GPU: the float64 statement (tests/conv_grad_np.py) against torch.autograd of
F.conv2d(padding=1), the refusal rules of odet_conv3x3_wgrad_f32_levels through the built library (each returns before any HIP
call), its workspace query against the restated plan, the Python fronts' argument errors on CPU tensors, and the pack / unpack
index maps."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_grad_np as cg

EDGE_MAPS = [(1, 1), (1, 5), (5, 1), (2, 2), (3, 7)]
PYRAMID = [(12, 20), (6, 10), (3, 5), (2, 3), (1, 2)]


def _nchw(a):
    return torch.tensor(np.ascontiguousarray(a.transpose(0, 3, 1, 2)), requires_grad=True)


@pytest.mark.parametrize('batch', [1, 2])
@pytest.mark.parametrize('shapes', [[s] for s in EDGE_MAPS] + [PYRAMID[2:]], ids=lambda s: '+'.join('%dx%d' % t for t in s))
def test_statement_equals_torch_autograd(shapes, batch):
    """dw, db, dx of relu(conv2d(x, w, b, padding=1)) summed over levels that share the weights, in float64; integer data makes
    pre-activations EXACTLY zero, whose gradient must be zero (y > 0 is strict)"""
    rng = np.random.default_rng(len(shapes) * 10 + batch)
    cin, cout = 3, 4
    w = rng.integers(-2, 3, (cout, 3, 3, cin)).astype(np.float64)
    b = rng.integers(-2, 3, (cout,)).astype(np.float64)
    xs = [rng.integers(-2, 3, (batch, h, ww, cin)).astype(np.float64) for h, ww in shapes]
    dys = [rng.standard_normal((batch, h, ww, cout)) for h, ww in shapes]
    for relu in (True, False):
        tw = torch.tensor(np.ascontiguousarray(w.transpose(0, 3, 1, 2)), requires_grad=True)
        tb = torch.tensor(b, requires_grad=True)
        txs = [_nchw(x) for x in xs]
        pres = [F.conv2d(tx, tw, tb, padding=1) for tx in txs]
        outs = [torch.relu(p) if relu else p for p in pres]
        torch.autograd.backward(outs, [torch.tensor(np.ascontiguousarray(d.transpose(0, 3, 1, 2))) for d in dys])
        ys = [o.detach().numpy().transpose(0, 2, 3, 1) for o in outs] if relu else None
        if relu and sum(x.size for x in xs) > 30:
            assert any((p.detach().numpy() == 0).any() for p in pres)
        dw, db = cg.wgrad(xs, dys, ys)
        np.testing.assert_allclose(dw, tw.grad.numpy().transpose(0, 2, 3, 1), rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(db, tb.grad.numpy(), rtol=1e-13, atol=1e-13)
        dzs = [cg.masked_dy(d, y) for d, y in zip(dys, ys or [None] * len(dys))]
        for dx, tx in zip(cg.dgrad(dzs, w), txs):
            np.testing.assert_allclose(dx, tx.grad.numpy().transpose(0, 2, 3, 1), rtol=1e-13, atol=1e-13)
    # a NaN under a closed gate does not pass (a select, not a product)
    ys = [np.where(rng.integers(0, 2, d.shape) > 0, 1.0, -1.0) for d in dys]
    bad = [np.where(y > 0, d, np.nan) for d, y in zip(dys, ys)]
    assert np.isfinite(cg.wgrad(xs, bad, ys)[0]).all()


# ---- the refusal rules, through the built library: pointer-VALUED integers nothing dereferences (as tests/test_dense_grad_host.py);
# every row returns before any HIP call, so this runs without a GPU
def _levels(specs):
    from tf_eager_object_detection_amd import _lib
    lv = (_lib.OdetConvGradLevel * max(1, len(specs)))()
    for i, (x, dy, y, h, w) in enumerate(specs):
        lv[i].x, lv[i].dy, lv[i].y_relu, lv[i].H, lv[i].W = x, dy, y, h, w
    return lv


_LEVEL = (0x10000, 0x20000, 0x30000, 5, 7)
_GOOD = dict(levels=[_LEVEL], n=None, dw=0x50000, db=0x60000, batch=1, cin=64, cout=64, ws=None, ws_bytes=0)


def _call(L, **over):
    a = dict(_GOOD, **over)
    lv = _levels(a['levels']) if a['levels'] is not None else None
    n = len(a['levels']) if a['n'] is None else a['n']
    return L.odet_conv3x3_wgrad_f32_levels(lv, n, a['dw'], a['db'], a['batch'], a['cin'], a['cout'], a['ws'], a['ws_bytes'], None)


def test_entry_point_refuses_bad_arguments_before_any_device_call():
    from tf_eager_object_detection_amd import _lib
    L = _lib.lib()
    lvl = lambda **k: [tuple(k.get(n, v) for n, v in zip(('x', 'dy', 'y', 'H', 'W'), _LEVEL))]
    rows = [('null levels', dict(levels=None, n=1)), ('null dw', dict(dw=None)), ('null x', dict(levels=lvl(x=None))),
            ('null dy', dict(levels=lvl(dy=None))), ('cin 48', dict(cin=48)), ('cin 0', dict(cin=0)), ('cout 96', dict(cout=96)),
            ('cout 0', dict(cout=0)), ('B 0', dict(batch=0)), ('B -1', dict(batch=-1)), ('H 0', dict(levels=lvl(H=0))),
            ('W 0', dict(levels=lvl(W=0))), ('0 levels', dict(n=0)), ('MAX + 1 levels', dict(levels=[_LEVEL] * (_lib.MAX_LEVELS + 1))),
            ('misaligned x', dict(levels=lvl(x=_LEVEL[0] + 4))), ('misaligned dy', dict(levels=lvl(dy=_LEVEL[1] + 4))),
            ('misaligned y_relu', dict(levels=lvl(y=_LEVEL[2] + 4))), ('misaligned dw', dict(dw=_GOOD['dw'] + 4)),
            ('misaligned db', dict(db=_GOOD['db'] + 2)),
            ('a bad second level', dict(levels=[_LEVEL, _LEVEL[:3] + (0, 3)]))]
    for label, bad in rows:
        rc = _call(L, **bad)
        msg = L.odet_last_error()
        print('%s -> %d %r' % (label, rc, msg))
        assert rc == -1, '%s returned %d: %r' % (label, rc, msg)                                      # ODET_E_INVALID
        assert msg.startswith(b'odet_conv3x3_wgrad_f32_levels') and b' failed: ' not in msg, msg     # (no HIP call was made)
    # a workspace that is missing, too small or misaligned where the launch needs one
    split = dict(levels=[_LEVEL[:3] + (17, 40)])
    need = L.odet_conv3x3_wgrad_workspace_bytes(_levels(split['levels']), 1, 1, 64, 64)
    assert need == cg.workspace_bytes([(17, 40)], 1, 64, 64) > 0
    for label, bad, want in (('no workspace', dict(ws=None, ws_bytes=need), -2), ('one byte short', dict(ws=0x100000, ws_bytes=need - 1), -2),
                             ('workspace of 0 bytes', dict(ws=0x100000, ws_bytes=0), -2),
                             ('misaligned workspace', dict(ws=0x100004, ws_bytes=need), -1)):
        rc = _call(L, **dict(split, **bad))
        msg = L.odet_last_error()
        print('%s -> %d %r' % (label, rc, msg))
        assert rc == want and b' failed: ' not in msg, (label, rc, msg)
    # and the unpack
    good = dict(ds=0x1000, ss=600, so=0, dd=0x2000, dst=1200, do=0, px=100, A=3, B=2, ch=64, out=0x3000, st=None)
    un = lambda **k: L.odet_rpn_unpack_pair(*[dict(good, **k)[n] for n in good])
    for bad in (dict(ds=None), dict(dd=None), dict(out=None), dict(A=0), dict(ch=12), dict(px=101), dict(so=-2)):
        assert un(**bad) == -1 and b' failed: ' not in L.odet_last_error(), bad


def test_workspace_query_is_the_restated_plan():
    """0 exactly where the plan does not cut the contraction, else parts * cout * 9 * cin * 4"""
    from tf_eager_object_detection_amd import _lib
    L = _lib.lib()
    seen = set()
    cases = [([s], b, ci, co) for s in EDGE_MAPS + [(9, 33), (17, 40)] for b in (1, 2) for ci in (64, 96) for co in (64, 192)]
    cases += [(PYRAMID, b, 64, 64) for b in (1, 2)] + [([(16, 24), (8, 12), (4, 6), (2, 3), (1, 2)], 1, 256, 512)]
    cases += [([(200, 334), (100, 167), (50, 84), (25, 42), (13, 21)], 1, 256, 512)]            # the 800 x 1333 pyramid
    for shapes, b, ci, co in cases:
        lv = _levels([(None, None, None, h, w) for h, w in shapes])                           # (the query reads no pointer)
        got = L.odet_conv3x3_wgrad_workspace_bytes(lv, len(shapes), b, ci, co)
        T, parts, kper = cg.plan(shapes, b, ci, co)
        assert got == (parts * co * 9 * ci * 4 if parts > 1 else 0), (shapes, b, ci, co)
        assert kper % 32 == 0 and (parts - 1) * kper < b * sum(h * w for h, w in shapes) <= parts * kper
        seen.add(parts > 1)
    assert seen == {True, False}
    assert cg.plan([(200, 334), (100, 167), (50, 84), (25, 42), (13, 21)], 1, 256, 512)[:2] == (128, 7)
    lv = _levels([(None, None, None, 5, 7)])
    for bad in ((0, 1, 64, 64), (9, 1, 64, 64), (1, 0, 64, 64), (1, 1, 0, 64), (1, 1, 64, 0)):
        assert L.odet_conv3x3_wgrad_workspace_bytes(lv, *bad) == 0
    assert L.odet_conv3x3_wgrad_workspace_bytes(None, 1, 1, 64, 64) == 0


def test_python_fronts_refuse_on_cpu_tensors():
    from tf_eager_object_detection_amd import ops
    x, dy, w = torch.zeros(1, 4, 5, 64), torch.zeros(1, 4, 5, 64), torch.zeros(64, 3, 3, 64)
    calls = (lambda **k: ops.conv3x3_wgrad_f32_levels([k.get('x', x)], [k.get('dy', dy)], [k['y']] if 'y' in k else None),
             lambda **k: ops.conv3x3_dgrad_f32_levels([k.get('dy', dy)], k.get('w', w)))
    for i, call in enumerate(calls):
        with pytest.raises(ValueError, match='float32'):
            call(dy=dy.half())
        for form in ('x3', 'x2'):
            with ops.f32_form(form):
                with pytest.raises(ValueError, match="only under f32_form 'exact'"):
                    call()
        with pytest.raises(ValueError, match='contiguous'):
            call(dy=torch.zeros(1, 4, 64, 5).permute(0, 1, 3, 2))
        with pytest.raises(ValueError, match='GPU'):                 # (and no CPU path behind the checks)
            call()
    with pytest.raises(ValueError, match='float32'):
        calls[0](x=x.half())
    with pytest.raises(ValueError, match='float32'):
        calls[0](y=dy.double())
    with pytest.raises(ValueError, match='contiguous'):
        calls[0](x=torch.zeros(1, 4, 64, 5).permute(0, 1, 3, 2))
    with pytest.raises(ValueError, match='float32'):
        calls[1](w=w.half())
    with pytest.raises(ValueError, match='multiple of 32'):
        ops.conv3x3_wgrad_f32_levels([torch.zeros(1, 4, 5, 48)], [dy])
    with pytest.raises(ValueError, match='multiple of 64'):
        ops.conv3x3_wgrad_f32_levels([x], [torch.zeros(1, 4, 5, 96)])
    with pytest.raises(ValueError, match='multiple of 64'):         # the forward's rules with the roles exchanged
        ops.conv3x3_dgrad_f32_levels([dy], torch.zeros(64, 3, 3, 96))
    with pytest.raises(ValueError, match='multiple of 32'):
        ops.conv3x3_dgrad_f32_levels([torch.zeros(1, 4, 5, 48)], torch.zeros(48, 3, 3, 64))
    with pytest.raises(ValueError, match='as many'):
        ops.conv3x3_wgrad_f32_levels([x, x], [dy])
    with pytest.raises(ValueError, match='does not go with'):
        ops.conv3x3_wgrad_f32_levels([x], [torch.zeros(1, 4, 6, 64)])
    with ops.f32_form('x3'):
        with pytest.raises(ValueError, match="only under f32_form 'exact'"):
            ops.conv3x3_trainable_levels([x], w, None)
    with pytest.raises(ValueError, match='float32'):
        ops.conv3x3_trainable_levels([x.half()], w.half(), None)


def test_flipped_weight_is_the_statement_of_the_input_gradient():
    """the forward convolution of dz with w'[ci][ky][kx][co] = w[co][2-ky][2-kx][ci] is dx"""
    from tf_eager_object_detection_amd import ops
    rng = np.random.default_rng(3)
    w = rng.standard_normal((4, 3, 3, 5)).astype(np.float32)
    dz = rng.standard_normal((2, 3, 4, 4))
    wf = ops.conv3x3_flipped_weight(torch.from_numpy(w))
    assert tuple(wf.shape) == (5, 3, 3, 4) and wf.is_contiguous()
    assert np.array_equal(wf.numpy(), w[:, ::-1, ::-1, :].transpose(3, 1, 2, 0))
    same = ops.conv3x3_flipped_weight(torch.from_numpy(np.ascontiguousarray(w.transpose(0, 3, 1, 2))))       # [cout,cin,3,3]
    assert torch.equal(same, wf)
    fwd = F.conv2d(torch.tensor(dz.transpose(0, 3, 1, 2)), wf.double().permute(0, 3, 1, 2), padding=1).numpy().transpose(0, 2, 3, 1)
    np.testing.assert_allclose(fwd, cg.dgrad([dz], w)[0], rtol=1e-12, atol=1e-12)


def test_unpack_and_pack_are_inverse_on_the_index_maps():
    A, B, chp = 3, 2, 64
    pix = [12, 5]
    N = sum(pix) * A
    rng = np.random.default_rng(4)
    ds, dd = rng.standard_normal((B, N, 2)), rng.standard_normal((B, N, 4))
    s2, d2 = np.full_like(ds, np.nan), np.full_like(dd, np.nan)
    off = 0
    covered_s, covered_d = [], []
    for p in pix:
        g = cg.unpack(ds, dd, A, p, off, chp)
        assert g.shape == (B * p, chp) and (g[:, 6 * A:] == 0).all()
        cg.pack(g.reshape(B, p, chp)[:, :, :6 * A], np.zeros(6 * A), A, s2, d2, off)
        si, di = cg.pack_index(p, A, off)
        covered_s.append(si.ravel())
        covered_d.append(di.ravel())
        off += p * A
    assert np.array_equal(s2, ds) and np.array_equal(d2, dd)                   # pack(unpack(g)) with a zero bias returns g
    # the levels' maps tile the concatenated arrays: every element exactly once
    assert np.array_equal(np.sort(np.concatenate(covered_s)), np.arange(N * 2))
    assert np.array_equal(np.sort(np.concatenate(covered_d)), np.arange(N * 4))


def test_caller_model_refuses_train_rpn_head_outside_the_exact_float32_form():
    import inspect
    from tf_eager_object_detection_amd.model.base_fpn_model import BaseFPN, ResnetV1Fpn
    for cls in (BaseFPN, ResnetV1Fpn):
        assert inspect.signature(cls.__init__).parameters['train_rpn_head'].default is False
    with pytest.raises(ValueError, match='train_rpn_head'):
        ResnetV1Fpn(depth=50, train_rpn_head=True, f32_form='x3', device='cpu')
    with pytest.raises(ValueError, match='train_rpn_head'):
        ResnetV1Fpn(depth=50, train_rpn_head=True, dtype=torch.float16, device='cpu')
