"""The ResNet bottleneck's backward without a GPU: the NumPy statements of odet_stride_gather_f32 and odet_block_input_grad_f32
(tests/block_grad_np.py; the scatter is the gather's transpose), the float64 statement of a whole block's backward against torch
autograd of the plain F.conv2d block, the integer data set of the GPU tests proved exact, the two entry points' refusal rules through
the built library (each returns before any HIP call), header / library / binding agreeing on the symbols, and the Python fronts' and
the constructors' argument errors on CPU tensors."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import block_grad_np as bg

SIZES = [(1, 1), (1, 2), (2, 3), (5, 4), (6, 6), (7, 11)]
_ID = lambda c: '%dx%d' % tuple(c) if isinstance(c, tuple) else None


@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('hw', SIZES, ids=_ID)
def test_scatter_is_the_transpose_of_gather(hw, stride):
    """<gather(x), g> == <x, scatter(g)>, exactly on integers; the gather reaches the last row / column exactly when it is even"""
    H, W = hw
    rng = np.random.default_rng(H * 100 + W * 10 + stride)
    B, Cc = 2, 4
    x = rng.integers(-3, 4, (B, H, W, Cc)).astype(np.float32)
    xs = bg.stride_gather(x, stride)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    assert xs.shape == (B, Ho, Wo, Cc) and xs.flags['C_CONTIGUOUS']
    for i in range(Ho):
        for j in range(Wo):
            assert np.array_equal(xs[:, i, j], x[:, i * stride, j * stride])
    assert ((Ho - 1) * stride == H - 1) == (stride == 1 or H % 2 == 1)
    g = rng.integers(-3, 4, xs.shape).astype(np.float32)
    g2 = rng.integers(-3, 4, xs.shape).astype(np.float32)
    sc = bg.input_grad_conv(g, None, stride, hw)
    assert sc.shape == x.shape and sc.dtype == np.float32
    assert float((xs.astype(np.float64) * g).sum()) == float((x.astype(np.float64) * sc).sum())
    assert np.array_equal(bg.input_grad_conv(g, g2, stride, hw), sc + bg.input_grad_conv(g2, None, stride, hw))
    off = np.ones((H, W), bool)
    off[::stride, ::stride] = False
    both = bg.input_grad_conv(g, g2, stride, hw)
    assert (both[:, off] == 0).all() and not np.signbit(both[:, off]).any()                          # +0 elsewhere


def test_identity_join_statement():
    """(y > 0 ? dy : +0) + d1 in float32: the gate is strict (y == +0 and y == -0 close it), a closed gate adds +0, one rounding"""
    y = np.array([1.0, 0.0, -0.0, -2.0, 1e-45, np.float32(3.0)], np.float32).reshape(1, 1, 1, 6)
    dy = np.array([5.0, 5.0, 5.0, 5.0, 5.0, 2.0 ** 24], np.float32).reshape(1, 1, 1, 6)
    d1 = np.array([1.0, -0.0, 7.0, -0.0, 0.5, 1.0], np.float32).reshape(1, 1, 1, 6)
    got = bg.input_grad_identity(dy, y, d1)
    assert got.dtype == np.float32
    want = np.array([6.0, 0.0, 7.0, 0.0, 5.5, 2.0 ** 24], np.float32)
    assert np.array_equal(got.reshape(-1).view(np.int32), want.view(np.int32))                       # (+0 + -0 = +0)


def _torch_block(x, P, stride, dy):
    """torch autograd of the plain F.conv2d bottleneck (NCHW float64) -> (y, {layer: (dw, db)}, dx) as NHWC arrays"""
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, requires_grad=True)
    tx = t(x.transpose(0, 3, 1, 2))
    T = {k: t(v) for k, v in P.items()}
    w1x1 = lambda w: w[:, :, None, None]
    a = F.relu(F.conv2d(tx, w1x1(T['w1']), T['b1'], stride=stride))
    b = F.relu(F.conv2d(a, T['w2'].permute(0, 3, 1, 2), T['b2'], padding=1))
    y = F.conv2d(b, w1x1(T['w3']), T['b3'])
    y = F.relu(y + (F.conv2d(tx, w1x1(T['ws']), T['bs'], stride=stride) if 'ws' in P else tx))
    y.backward(torch.tensor(np.ascontiguousarray(dy.transpose(0, 3, 1, 2))))
    g = lambda k: T[k].grad.numpy()
    grads = {'c1': (g('w1'), g('b1')), 'c2': (g('w2'), g('b2')), 'c3': (g('w3'), g('b3'))}
    if 'ws' in P:
        grads['short'] = (g('ws'), g('bs'))
    return y.detach().numpy().transpose(0, 2, 3, 1), grads, tx.grad.numpy().transpose(0, 2, 3, 1)


@pytest.mark.parametrize('cin,f,stride,short', [(12, 5, 1, False), (7, 3, 1, True), (6, 4, 2, True)],
                         ids=['identity', 'conv_s1', 'conv_s2'])
@pytest.mark.parametrize('hw', [(1, 1), (2, 3), (5, 4), (7, 6)], ids=_ID)
def test_float64_block_statement_equals_torch_autograd(hw, cin, f, stride, short):
    rng = np.random.default_rng(hw[0] * 10 + hw[1] + cin)
    n = lambda *s: rng.standard_normal(s)
    cin = 4 * f if not short else cin
    P = {'w1': n(f, cin), 'b1': n(f), 'w2': n(f, 3, 3, f), 'b2': n(f), 'w3': n(4 * f, f), 'b3': n(4 * f)}
    if short:
        P['ws'], P['bs'] = n(4 * f, cin), n(4 * f)
    B, (H, W) = 2, hw
    x = n(B, H, W, cin)
    dy = n(B, (H - 1) // stride + 1, (W - 1) // stride + 1, 4 * f)
    y, grads, dx, _ = bg.block_backward(x, P, stride, dy)
    ty, tgrads, tdx = _torch_block(x, P, stride, dy)
    np.testing.assert_allclose(y, ty, rtol=1e-12, atol=1e-12)
    assert sorted(grads) == sorted(tgrads)
    for name in grads:
        np.testing.assert_allclose(grads[name][0], tgrads[name][0], rtol=1e-10, atol=1e-10, err_msg=name)
        np.testing.assert_allclose(grads[name][1], tgrads[name][1], rtol=1e-10, atol=1e-10, err_msg=name)
    np.testing.assert_allclose(dx, tdx, rtol=1e-10, atol=1e-10)


@pytest.mark.parametrize('B', [1, 2])
@pytest.mark.parametrize('hw', bg.MAPS, ids=_ID)
@pytest.mark.parametrize('kind', list(bg.KINDS))
def test_integer_data_set_is_exact_in_float32(kind, hw, B):
    """every case the GPU test runs: all intermediates of the float64 statement (and every contraction on magnitudes) are integers
    below 2^24, every ReLU gate has open and closed elements, every gradient is non-zero, and the statement equals torch's"""
    x, P, dy = bg.integer_case(kind, hw, B)
    y, grads, dx, rec = bg.block_backward(x, P, bg.KINDS[kind][2], dy)
    worst = bg.assert_exact_in_float32(rec)
    print('largest magnitude: %.0f (2^24 = %d)' % (worst, 2 ** 24))
    for name, (dw, db) in grads.items():
        assert np.abs(dw).max() > 0 and np.abs(db).max() > 0, name
    assert np.abs(dx).max() > 0
    ty, tgrads, tdx = _torch_block(x, P, bg.KINDS[kind][2], dy)
    assert np.array_equal(y, ty) and np.array_equal(dx, tdx)
    for name in grads:
        assert np.array_equal(grads[name][0], tgrads[name][0]) and np.array_equal(grads[name][1], tgrads[name][1]), name


# ---- the refusal rules, through the built library: pointer-VALUED integers nothing dereferences (as tests/test_neck_grad_host.py);
# every row returns before any HIP call, so this runs without a GPU
_GATHER = dict(x=0x10000, B=1, H=5, W=4, C=8, stride=2, out=0x20000, stream=None)
_JOIN = dict(dy=None, y=None, d1=0x30000, d2=0x40000, dx=0x50000, B=1, H=5, W=4, C=8, stride=2, stream=None)
_IDENT = dict(_JOIN, dy=0x10000, y=0x20000, d2=None, stride=1)


def _call(L, name, good, **over):
    a = dict(good, **over)
    return getattr(L, name)(*[a[k] for k in good])


def test_entry_points_refuse_bad_arguments_before_any_device_call():
    from tf_eager_object_detection_amd import _lib
    L = _lib.lib()
    sizes = [('H 0', dict(H=0)), ('W 0', dict(W=0)), ('H -1', dict(H=-1)), ('B -1', dict(B=-1)), ('C 6', dict(C=6)), ('C 0', dict(C=0)),
             ('C -4', dict(C=-4)), ('stride 0', dict(stride=0)), ('stride 3', dict(stride=3)), ('stride -2', dict(stride=-2))]
    rows = [('odet_stride_gather_f32', _GATHER, label, bad) for label, bad in sizes + [
        ('null x', dict(x=None)), ('null out', dict(out=None)), ('misaligned x', dict(x=0x10004)), ('misaligned out', dict(out=0x20008))]]
    rows += [('odet_block_input_grad_f32', _JOIN, label, bad) for label, bad in sizes + [
        ('null dx', dict(dx=None)), ('null d1', dict(d1=None)), ('dy without y', dict(dy=0x10000)), ('y without dy', dict(y=0x20000)),
        ('all four', dict(dy=0x10000, y=0x20000, stride=1)), ('misaligned d1', dict(d1=0x30004)), ('misaligned d2', dict(d2=0x40008)),
        ('misaligned dx', dict(dx=0x5000c))]]
    rows += [('odet_block_input_grad_f32', _IDENT, label, bad) for label, bad in [
        ('identity at stride 2', dict(stride=2)), ('identity with d2', dict(d2=0x40000)), ('identity without d1', dict(d1=None)),
        ('misaligned dy', dict(dy=0x10004)), ('misaligned y', dict(y=0x20004)), ('C 2', dict(C=2)), ('W 0', dict(W=0))]]
    for name, good, label, bad in rows:
        rc = _call(L, name, good, **bad)
        msg = L.odet_last_error()
        print('%s: %s -> %d %r' % (name, label, rc, msg))
        assert rc == -1, '%s: %s returned %d: %r' % (name, label, rc, msg)                            # ODET_E_INVALID
        assert msg.startswith(name.encode()) and b' failed: ' not in msg, msg                         # (no HIP call was made)
    # B == 0 is a no-op that returns OK, in every form
    assert _call(L, 'odet_stride_gather_f32', _GATHER, B=0) == 0
    for good in (_JOIN, _IDENT, dict(_JOIN, d2=None), dict(_JOIN, stride=1)):
        assert _call(L, 'odet_block_input_grad_f32', good, B=0) == 0, good


def test_header_library_and_binding_agree_on_the_symbols():
    from tf_eager_object_detection_amd import _build, _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'odet.h')).read()
    assert 'int odet_stride_gather_f32(const float* x, int B, int H, int W, int C, int stride, float* out, odet_stream_t stream);' in header
    assert ('int odet_block_input_grad_f32(const float* dy, const float* y, const float* d1, const float* d2, float* dx, int B, int H, '
            'int W,') in header
    for sym in ('odet_stride_gather_f32', 'odet_block_input_grad_f32'):
        assert 'resnet_fpn.py:154-205' in header.split('int %s(' % sym)[0].rsplit('/*', 1)[1], sym
        assert sym in header.split('#define ODET_VERSION')[0], sym                                    # the list of additions
        assert hasattr(C.CDLL(_lib.LIB_PATH), sym), sym
    assert '#define ODET_VERSION 103' in header and _lib.ODET_VERSION == 103
    res, args = _lib.SIGNATURES['odet_stride_gather_f32']
    assert res is C.c_int and len(args) == 8 and args[:1] + args[6:] == [C.c_void_p] * 3 and args[1:6] == [C.c_int] * 5
    res, args = _lib.SIGNATURES['odet_block_input_grad_f32']
    assert res is C.c_int and len(args) == 11 and args[:5] + args[10:] == [C.c_void_p] * 6 and args[5:10] == [C.c_int] * 5
    assert 'block_grad.hip' in _build.SOURCES


def test_python_fronts_refuse_on_cpu_tensors():
    from tf_eager_object_detection_amd import ops
    x = torch.zeros(1, 5, 4, 8)
    for bad, match in ((x.half(), 'float32'), (x.double(), 'float32'), (x.permute(0, 2, 1, 3), 'contiguous'), (x[0], 'contiguous'),
                       (torch.zeros(1, 5, 4, 6), 'multiple of 4'), (torch.zeros(1, 0, 4, 8), 'positive')):
        with pytest.raises(ValueError, match=match):
            ops.stride_gather(bad, 2)
    for stride in (0, 3, 1.5, None):
        with pytest.raises(ValueError, match='stride must be 1 or 2'):
            ops.stride_gather(x, stride)
    for form in ('x3', 'x2'):
        with ops.f32_form(form):
            with pytest.raises(ValueError, match="only under f32_form 'exact'"):
                ops.stride_gather(x, 2)
            with pytest.raises(ValueError, match="only under f32_form 'exact'"):
                ops.block_input_grad(x, dy=x, y=x)
    with pytest.raises(ValueError, match='GPU'):                     # (and no CPU path behind the checks)
        ops.stride_gather(x, 2)
    d = torch.zeros(1, 3, 2, 8)
    join = ops.block_input_grad
    with pytest.raises(ValueError, match='come together'):
        join(x, dy=x)
    with pytest.raises(ValueError, match='come together'):
        join(x, y=x)
    with pytest.raises(ValueError, match='identity form'):
        join(x, dy=x, y=x, d2=x)
    with pytest.raises(ValueError, match='identity form'):
        join(x, dy=x, y=x, stride=2, in_hw=(9, 8))
    for name in ('dy', 'y'):
        with pytest.raises(ValueError, match='does not go with'):
            join(x, **dict(dict(dy=x, y=x), **{name: torch.zeros(1, 5, 4, 4)}))
        with pytest.raises(ValueError, match='float32'):
            join(x, **dict(dict(dy=x, y=x), **{name: x.half()}))
    with pytest.raises(ValueError, match='float32'):
        join(d.half(), d2=d.half(), stride=2, in_hw=(5, 4))
    with pytest.raises(ValueError, match='does not go with'):
        join(d, d2=torch.zeros(1, 3, 3, 8), stride=2, in_hw=(5, 4))
    with pytest.raises(ValueError, match='contiguous'):
        join(d, d2=torch.zeros(1, 2, 3, 8).permute(0, 2, 1, 3), stride=2, in_hw=(5, 4))
    with pytest.raises(ValueError, match='multiple of 4'):
        join(torch.zeros(1, 3, 2, 6), stride=2, in_hw=(5, 4))
    with pytest.raises(ValueError, match='in_hw'):
        join(d, d2=d, stride=2)
    for hw in ((7, 4), (5, 5), (3, 2), (0, 0)):
        with pytest.raises(ValueError, match='in_hw'):
            join(d, d2=d, stride=2, in_hw=hw)
    with pytest.raises(ValueError, match='in_hw'):
        join(d, d2=d, stride=1, in_hw=(5, 4))
    with pytest.raises(ValueError, match='stride must be 1 or 2'):
        join(d, d2=d, stride=3, in_hw=(5, 4))
    for call in (lambda: join(d, d2=d, stride=2, in_hw=(5, 4)), lambda: join(d, stride=2, in_hw=(6, 3)), lambda: join(d, d2=d),
                 lambda: join(x, dy=x, y=x)):
        with pytest.raises(ValueError, match='GPU'):
            call()


def test_block_and_extractor_trainable_refuse_other_forms_without_a_gpu():
    from tf_eager_object_detection_amd import ops
    from tf_eager_object_detection_amd.model.extractor_trainable import block_trainable, extractor_trainable
    from tf_eager_object_detection_amd.model.fpn_detector import ResNetFpnDetector
    from tf_eager_object_detection_amd.model.layers import _Block
    blk = _Block(256, 64, 1, False)
    with pytest.raises(ValueError, match='block_trainable needs'):
        block_trainable(blk, torch.zeros(1, 256, 2, 3, dtype=torch.float16))
    for form in ('x3', 'x2'):
        with ops.f32_form(form):
            with pytest.raises(ValueError, match='block_trainable needs'):
                block_trainable(blk, torch.zeros(1, 256, 2, 3))
    det = ResNetFpnDetector(50, 21, (64, 64), 1, dtype=torch.float32)
    for attr, bad in (('f32_form', 'x3'), ('f32_form', 'x2'), ('dtype', torch.float16)):
        good = getattr(det, attr)
        setattr(det, attr, bad)
        try:
            with pytest.raises(ValueError, match='extractor_trainable needs'):
                extractor_trainable(det, torch.zeros(1, 64, 64, 3))
        finally:
            setattr(det, attr, good)


def test_caller_model_refuses_train_extractor_without_the_trainable_neck_or_outside_the_exact_float32_form():
    import inspect
    from tf_eager_object_detection_amd.model.base_fpn_model import BaseFPN, ResnetV1Fpn
    for cls in (BaseFPN, ResnetV1Fpn):
        assert inspect.signature(cls.__init__).parameters['train_extractor'].default is False
    with pytest.raises(ValueError, match='train_extractor=True needs train_neck=True'):
        ResnetV1Fpn(depth=50, train_extractor=True, device='cpu')
    with pytest.raises(ValueError, match='train_extractor=True needs train_neck=True'):
        ResnetV1Fpn(depth=50, train_extractor=True, train_rpn_head=True, train_roi_head=True, device='cpu')
    with pytest.raises(ValueError, match='train_extractor'):
        BaseFPN(train_extractor=True)
    with pytest.raises(ValueError, match='train_neck'):                        # ... and the neck still needs a head
        ResnetV1Fpn(depth=50, train_extractor=True, train_neck=True, device='cpu')
    with pytest.raises(ValueError, match='train_extractor=True needs dtype'):
        ResnetV1Fpn(depth=50, train_extractor=True, train_neck=True, train_rpn_head=True, train_roi_head=True, dtype=torch.float16,
                    device='cpu')
    for form in ('x3', 'x2'):
        with pytest.raises(ValueError, match='train_extractor=True needs dtype'):
            ResnetV1Fpn(depth=50, train_extractor=True, train_neck=True, train_rpn_head=True, f32_form=form, device='cpu')
