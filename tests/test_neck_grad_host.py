"""The FPN neck's backward without a GPU: the float32 statement of odet_fpn_topdown_backward_f32 (tests/neck_grad_np.py) is the
TRANSPOSE of oracle_np.tf_resize_bilinear_legacy, its other terms are applied in the stated order, the float64 statement of the
whole neck equals torch.autograd of the plain neck, the entry point's refusal rules through the built library (each returns
before any HIP call), the header / library / binding agree on the symbol, and the Python fronts' argument errors on CPU tensors."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import neck_grad_np as ng
from oracle import oracle_np

CASES = ng.CASES
EXACT = [((1, 1), (1, 1)), ((3, 5), (6, 10)), ((5, 4), (5, 4))]          # ratio exactly 1 or 2: weights in {0, 1/4, 1/2, 3/4, 1}
_ID = lambda c: '%dx%d' % tuple(c) if isinstance(c, tuple) and isinstance(c[0], int) else None


def _resize_matrix(top_hw, fine_hw):
    """R [H*W, h*w] float32: column (Y, X) is the forward applied to the one-hot coarse map of (Y, X)"""
    h, w = top_hw
    onehot = np.eye(h * w, dtype=np.float32).reshape(h * w, h, w, 1)
    up = oracle_np.tf_resize_bilinear_legacy(onehot, fine_hw)                    # [h*w, H, W, 1]
    return up.reshape(h * w, -1).T


@pytest.mark.parametrize('top_hw,fine_hw', CASES, ids=_ID)
def test_statement_is_the_transpose_of_the_forward(top_hw, fine_hw):
    h, w = top_hw
    H, W = fine_hw
    R = _resize_matrix(top_hw, fine_hw).astype(np.float64)
    rng = np.random.default_rng(h * 1000 + W)
    B, Cc = 2, 4
    n = ng.tap_counts(top_hw, fine_hw).reshape(-1)
    assert n.sum() == 4 * H * W
    dead = np.abs(R).sum(axis=0) == 0                   # coarse pixels that only taps of weight zero (or none) land on
    if (top_hw, fine_hw) == ((6, 5), (3, 4)):
        assert (dead.sum() >= 15)                                                # the downscale leaves coarse rows no weight reaches
    if (top_hw, fine_hw) == ((7, 5), (2, 4)):
        assert (n == 0).any() and (n > 0).any()                                  # ... and this one pixels no tap lands on
    if (top_hw, fine_hw) in EXACT:
        g = rng.integers(-3, 4, (B, H, W, Cc)).astype(np.float32)
        want = np.einsum('fc,bfk->bck', R, g.reshape(B, H * W, Cc).astype(np.float64)).reshape(B, h, w, Cc)
        got = ng.topdown_backward(g, top_hw)
        assert np.array_equal(got.astype(np.float64), want)
    g = rng.standard_normal((B, H, W, Cc)).astype(np.float32)
    g64 = g.reshape(B, H * W, Cc).astype(np.float64)
    want = np.einsum('fc,bfk->bck', R, g64)
    mag = np.einsum('fc,bfk->bck', np.abs(R), np.abs(g64))
    got = ng.topdown_backward(g, top_hw).reshape(B, h * w, Cc).astype(np.float64)
    bound = (n[None, :, None] + 4) * 2.0 ** -23 * mag
    err = np.abs(got - want)
    print('worst fraction of the bound: %.3f' % float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all()
    assert (got[:, dead] == 0).all() and not np.signbit(got[:, dead]).any()                        # +0
    # the float64 transpose used by neck_backward is the same operator (R's float32 one-hot weights carry up to three roundings)
    assert (np.abs(ng.resize_t(g, top_hw).reshape(B, h * w, Cc) - want) <= 4 * 2.0 ** -24 * mag + 1e-300).all()
    np.testing.assert_allclose(ng.resize(want.reshape(B, h, w, Cc), fine_hw).reshape(B, H * W, Cc),
                               np.einsum('fc,bck->bfk', R, want), rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize('top_hw', [(5, 4), (4, 6), (3, 5), (1, 1)], ids=_ID)
def test_base_sub_and_scale_are_applied_in_the_stated_order(top_hw):
    """out_scale * ((base + sub at the even pixels) + S), each step rounded to float32; absent terms skipped; odd and even h, w"""
    h, w = top_hw
    H, W = 2 * h - 1, 2 * w + 1
    rng = np.random.default_rng(h * 10 + w)
    B, Cc = 2, 4
    fine = rng.standard_normal((B, H, W, Cc)).astype(np.float32)
    base = (rng.standard_normal((B, h, w, Cc)) * 1000).astype(np.float32)       # magnitudes apart: the order of the sums shows
    sub = (rng.standard_normal((B, (h + 1) // 2, (w + 1) // 2, Cc)) * 30).astype(np.float32)
    S = ng.topdown_backward(fine, top_hw)
    placed = np.zeros((B, h, w, Cc), np.float32)
    placed[:, ::2, ::2] = sub
    even = np.zeros((h, w), bool)
    even[::2, ::2] = True
    even = even[None, :, :, None]
    f32 = lambda a: a.astype(np.float32)
    for scale in (0.5, 1.0, 3.0):
        s = np.float32(scale)
        assert np.array_equal(ng.topdown_backward(fine, top_hw, out_scale=scale), f32(s * S))
        assert np.array_equal(ng.topdown_backward(fine, top_hw, base=base, out_scale=scale), f32(s * f32(base + S)))
        assert np.array_equal(ng.topdown_backward(fine, top_hw, base=base, sub=sub, out_scale=scale),
                              f32(s * f32(np.where(even, f32(base + placed), base) + S)))
        assert np.array_equal(ng.topdown_backward(fine, top_hw, sub=sub, out_scale=scale),
                              f32(s * np.where(even, f32(placed + S), S)))
        assert np.array_equal(ng.topdown_backward(None, top_hw, base=base, sub=sub, out_scale=scale),
                              f32(s * np.where(even, f32(base + placed), base)))
        assert np.array_equal(ng.topdown_backward(None, top_hw, sub=sub, out_scale=scale), f32(s * placed))
        assert np.array_equal(ng.topdown_backward(None, top_hw, base=base, out_scale=scale), f32(s * base))
    if h * w > 1:
        # the other order of the same three terms gives other bits somewhere: the stated order is a statement
        other = f32(np.float32(1) * f32(base + f32(np.where(even, f32(placed + S), S))))
        assert not np.array_equal(ng.topdown_backward(fine, top_hw, base=base, sub=sub), other)


def _plain_neck(cs, params):
    """the plain neck on torch tensors (NCHW float64): tf_legacy_resize_bilinear + F.conv2d"""
    from tf_eager_object_detection_amd.model.layers import tf_legacy_resize_bilinear
    c2, c3, c4, c5 = cs
    lin = lambda x, n: F.conv2d(x, params[n][0], params[n][1])
    p5 = lin(c5, 'p5')
    m4 = 0.5 * tf_legacy_resize_bilinear(p5, c4.shape[2:]) + 0.5 * lin(c4, 'l4')
    m3 = 0.5 * tf_legacy_resize_bilinear(m4, c3.shape[2:]) + 0.5 * lin(c3, 'l3')
    m2 = 0.5 * tf_legacy_resize_bilinear(m3, c2.shape[2:]) + 0.5 * lin(c2, 'l2')
    conv = lambda m, n: F.conv2d(m, params[n][0], params[n][1], padding=1)
    return conv(m2, 's2'), conv(m3, 's3'), conv(m4, 's4'), p5, p5[:, :, ::2, ::2]


@pytest.mark.parametrize('absent', [(), (4,), (0, 3), (0, 1, 2)], ids=lambda a: 'without_' + '_'.join('P%d' % (i + 2) for i in a) if a else 'all')
def test_float64_neck_statement_equals_torch_autograd(absent):
    rng = np.random.default_rng(7)
    B, top = 2, 6
    shapes = [(13, 21), (7, 11), (4, 6), (2, 3)]
    cins = [5, 6, 7, 8]
    cs = [rng.standard_normal((B, h, w, c)) for (h, w), c in zip(shapes, cins)]
    params = {}
    for name, cin in zip(('l2', 'l3', 'l4', 'p5'), cins):
        params[name] = (rng.standard_normal((top, cin)), rng.standard_normal(top))
    for name in ('s2', 's3', 's4'):
        params[name] = (rng.standard_normal((top, 3, 3, top)), rng.standard_normal(top))
    out_shapes = shapes + [(1, 2)]
    d_ps = [None if i in absent else rng.standard_normal((B, h, w, top)) for i, (h, w) in enumerate(out_shapes)]
    grads, d_cs = ng.neck_backward(cs, params, d_ps)

    nchw = lambda a: torch.tensor(np.ascontiguousarray(a.transpose(0, 3, 1, 2)), requires_grad=True)
    tcs = [nchw(c) for c in cs]
    tparams = {}
    for name, (w, b) in params.items():
        tw = w.reshape(top, -1, 1, 1) if w.ndim == 2 else w.transpose(0, 3, 1, 2)
        tparams[name] = (torch.tensor(np.ascontiguousarray(tw), requires_grad=True), torch.tensor(b, requires_grad=True))
    outs = _plain_neck(tcs, tparams)
    fwd = ng.neck_forward(cs, params)[1]
    for o, f in zip(outs, fwd):
        np.testing.assert_allclose(o.detach().numpy().transpose(0, 2, 3, 1), f, rtol=1e-6, atol=1e-6)   # (float32 lerps in torch's)
    keep = [i for i in range(5) if i not in absent]
    torch.autograd.backward([outs[i] for i in keep],
                            [torch.tensor(np.ascontiguousarray(d_ps[i].transpose(0, 3, 1, 2))) for i in keep])
    for name in ng.LAYERS:
        tw, tb = tparams[name]
        if tw.grad is None:
            assert name not in grads, name
            continue
        gw = tw.grad.numpy()
        gw = gw.reshape(top, -1) if params[name][0].ndim == 2 else gw.transpose(0, 2, 3, 1)
        np.testing.assert_allclose(grads[name][0], gw, rtol=1e-6, atol=1e-6, err_msg=name)
        np.testing.assert_allclose(grads[name][1], tb.grad.numpy(), rtol=1e-6, atol=1e-6, err_msg=name)
    for d, tc in zip(d_cs, tcs):
        if tc.grad is None:
            assert d is None
        else:
            np.testing.assert_allclose(d, tc.grad.numpy().transpose(0, 2, 3, 1), rtol=1e-6, atol=1e-6)


# ---- the refusal rules, through the built library: pointer-VALUED integers nothing dereferences (as tests/test_conv_grad_host.py);
# every row returns before any HIP call, so this runs without a GPU
_GOOD = dict(fine=0x10000, H=6, W=10, base=0x20000, sub=0x30000, out_scale=0.5, d_top=0x40000, h=3, w=5, B=1, C=8, stream=None)


def _call(L, **over):
    a = dict(_GOOD, **over)
    return L.odet_fpn_topdown_backward_f32(*[a[k] for k in _GOOD])


def test_entry_point_refuses_bad_arguments_before_any_device_call():
    from tf_eager_object_detection_amd import _lib
    L = _lib.lib()
    rows = [('null d_top', dict(d_top=None)), ('no term', dict(fine=None, base=None, sub=None)), ('h 0', dict(h=0)), ('w 0', dict(w=0)),
            ('H 0', dict(H=0)), ('W 0', dict(W=0)), ('h -1', dict(h=-1)), ('B -1', dict(B=-1)), ('C 6', dict(C=6)), ('C 0', dict(C=0)),
            ('C -4', dict(C=-4)), ('misaligned fine', dict(fine=0x10004)), ('misaligned base', dict(base=0x20008)),
            ('misaligned sub', dict(sub=0x30004)), ('misaligned d_top', dict(d_top=0x40004)),
            ('H 0 without fine', dict(fine=None, H=0))]
    for label, bad in rows:
        rc = _call(L, **bad)
        msg = L.odet_last_error()
        print('%s -> %d %r' % (label, rc, msg))
        assert rc == -1, '%s returned %d: %r' % (label, rc, msg)                                      # ODET_E_INVALID
        assert msg.startswith(b'odet_fpn_topdown_backward_f32') and b' failed: ' not in msg, msg      # (no HIP call was made)
    # B == 0 is a no-op that returns OK, with any of the terms absent
    for ok in (dict(B=0), dict(B=0, fine=None), dict(B=0, base=None, sub=None)):
        assert _call(L, **ok) == 0, ok


def test_header_library_and_binding_agree_on_the_symbol():
    from tf_eager_object_detection_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'odet.h')).read()
    assert 'int odet_fpn_topdown_backward_f32(const float* fine, int H, int W, const float* base, const float* sub, float out_scale,' in header
    assert 'resnet_fpn.py:385-398' in header.split('int odet_fpn_topdown_backward_f32(')[0].rsplit('/*', 1)[1]
    assert '#define ODET_VERSION 103' in header
    res, args = _lib.SIGNATURES['odet_fpn_topdown_backward_f32']
    assert res is C.c_int and len(args) == 12 and args[5] is C.c_float
    assert hasattr(C.CDLL(_lib.LIB_PATH), 'odet_fpn_topdown_backward_f32')


def test_python_front_refuses_on_cpu_tensors():
    from tf_eager_object_detection_amd import ops
    fine, base, sub = torch.zeros(1, 6, 10, 8), torch.zeros(1, 3, 5, 8), torch.zeros(1, 2, 3, 8)
    call = lambda **k: ops.fpn_topdown_backward(k.get('fine', fine), k.get('hw', (3, 5)), base=k.get('base', base), sub=k.get('sub', sub))
    with pytest.raises(ValueError, match='at least one'):
        call(fine=None, base=None, sub=None)
    for name in ('fine', 'base', 'sub'):
        with pytest.raises(ValueError, match='float32'):
            call(**{name: dict(fine=fine, base=base, sub=sub)[name].half()})
    for form in ('x3', 'x2'):
        with ops.f32_form(form):
            with pytest.raises(ValueError, match="only under f32_form 'exact'"):
                call()
    with pytest.raises(ValueError, match='contiguous'):
        call(fine=torch.zeros(1, 6, 8, 10).permute(0, 1, 3, 2))
    with pytest.raises(ValueError, match='contiguous'):
        call(base=torch.zeros(3, 5, 8))
    with pytest.raises(ValueError, match='multiple of 4'):
        call(fine=torch.zeros(1, 6, 10, 6), base=None, sub=None)
    with pytest.raises(ValueError, match='positive'):
        call(hw=(0, 5))
    for bad in (dict(base=torch.zeros(2, 3, 5, 8)), dict(base=torch.zeros(1, 3, 5, 4)), dict(base=torch.zeros(1, 3, 4, 8)),
                dict(sub=torch.zeros(1, 1, 3, 8)), dict(sub=torch.zeros(1, 2, 2, 8)), dict(fine=None, sub=torch.zeros(2, 2, 3, 8))):
        with pytest.raises(ValueError, match='does not go with'):
            call(**bad)
    with pytest.raises(ValueError, match='GPU'):                     # (and no CPU path behind the checks)
        call()


def test_caller_model_refuses_train_neck_without_a_trainable_head_or_outside_the_exact_float32_form():
    import inspect
    from tf_eager_object_detection_amd.model.base_fpn_model import BaseFPN, ResnetV1Fpn
    for cls in (BaseFPN, ResnetV1Fpn):
        assert inspect.signature(cls.__init__).parameters['train_neck'].default is False
    with pytest.raises(ValueError, match='train_neck'):
        ResnetV1Fpn(depth=50, train_neck=True, device='cpu')
    with pytest.raises(ValueError, match='train_neck'):
        BaseFPN(train_neck=True)
    with pytest.raises(ValueError, match='train_neck'):
        ResnetV1Fpn(depth=50, train_neck=True, train_rpn_head=True, train_roi_head=True, dtype=torch.float16, device='cpu')
    for form in ('x3', 'x2'):
        with pytest.raises(ValueError, match='train_neck|train_rpn_head|train_roi_head'):
            ResnetV1Fpn(depth=50, train_neck=True, train_rpn_head=True, f32_form=form, device='cpu')
