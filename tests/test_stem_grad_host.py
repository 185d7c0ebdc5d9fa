"""The FPN stem's backward without a GPU: the NumPy statements of tests/stem_grad_np.py against torch's CPU float64 autograd (the
overlapping max-pooling behind a ReLU on data with ties and zeros, conv1's weight and bias gradient on a 9 x 11 image), the 'order'
data set shown to tell summation orders apart, the train_stem dependency rule, the C entry point's refusals (host-side checks: no
launch) and the header, the library and the binding agreeing on the new symbol."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import stem_grad_np as sg

_ID = lambda s: 'x'.join(str(v) for v in s)


# ---- 1. the pooling statement ---------------------------------------------------------------------------------------------------------
def _torch_pool_backward(z, bias, dpool):
    z64 = torch.tensor(z, dtype=torch.float64).permute(0, 3, 1, 2).contiguous().requires_grad_()
    b64 = torch.tensor(bias, dtype=torch.float64)
    y = F.max_pool2d(F.relu(z64 + b64[None, :, None, None]), 3, 2, 1)
    y.backward(torch.tensor(dpool, dtype=torch.float64).permute(0, 3, 1, 2))
    return y.detach().permute(0, 2, 3, 1).numpy(), z64.grad.permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize('shape', sg.SHAPES + sg.EDGE_SHAPES, ids=_ID)
def test_pooling_statement_equals_float64_autograd_on_integer_data(shape):
    """integers in -3..3: every sum of up to four dpool terms is exact in float32, so the statement equals float64 autograd of
    max_pool2d(relu(z + b), 3, 2, 1) -- torch's CPU pooling also keeps the first maximum in row-major order, and its ReLU passes
    nothing at 0"""
    z, bias, dpool = sg.pool_case('int', shape)
    y64, dz64 = _torch_pool_backward(z, bias, dpool)
    assert sg.relu_maxpool3_forward_np(z, bias).shape == y64.shape == dpool.shape
    assert np.array_equal(sg.relu_maxpool3_forward_np(z, bias).astype(np.float64), y64)
    got = sg.relu_maxpool3_backward_np(z, bias, dpool)
    assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), dz64), shape
    windows, ties, dead = sg.window_census(z, bias)
    if windows >= 64:
        assert ties > windows // 8 and dead > 0, (windows, ties, dead)          # the data does hold ties and windows <= 0
        assert ((z + bias) == 0).any()


def test_pooling_statement_tie_and_partial_winner():
    """hand-made maps, one channel used.  (a) window (0,0) holds its maximum at (0,0) and (1,1); (1,1) is shared with windows
    (0,1), (1,0), (1,1) of a 4 x 4 map: the first tap (0,0) takes window (0,0)'s gradient, (1,1) the other three.  (b) a pixel that
    is one window's maximum but not another's takes only the first one's."""
    z = np.zeros((1, 4, 4, 4), np.float32)
    z[0, 0, 0, 0] = z[0, 1, 1, 0] = 2.0
    dpool = np.zeros((1, 2, 2, 4), np.float32)
    dpool[0, :, :, 0] = [[1.0, 10.0], [100.0, 1000.0]]
    dz = sg.relu_maxpool3_backward_np(z, np.zeros(4, np.float32), dpool)
    assert dz[0, 0, 0, 0] == 1.0 and dz[0, 1, 1, 0] == 1110.0 and np.count_nonzero(dz) == 2
    z = np.zeros((1, 4, 4, 4), np.float32)
    z[0, 1, 1, 0], z[0, 3, 1, 0] = 2.0, 3.0             # (1,1) wins windows (0,0), (0,1); (3,1) beats it in (1,0), (1,1)
    dz = sg.relu_maxpool3_backward_np(z, np.zeros(4, np.float32), dpool)
    assert dz[0, 1, 1, 0] == 11.0 and dz[0, 3, 1, 0] == 1100.0 and np.count_nonzero(dz) == 2


def test_pooling_statement_nan_takes_no_gradient_and_minus_zero_is_kept():
    z, bias, dpool = sg.pool_case('normal', (1, 7, 9, 64))
    z[0, 3, 3, :] = np.nan
    dz = sg.relu_maxpool3_backward_np(z, bias, dpool)
    assert (dz[0, 3, 3] == 0).all() and np.isfinite(dz).all()
    clean = z.copy()
    clean[0, 3, 3, :] = -100.0                                                  # a tap that never wins either: the same function
    assert np.array_equal(dz.view(np.uint32), sg.relu_maxpool3_backward_np(clean, bias, dpool).view(np.uint32))
    # the sum starts from the first term itself: a single -0 term stays -0
    z = np.zeros((1, 1, 1, 4), np.float32) + 1
    dz = sg.relu_maxpool3_backward_np(z, np.zeros(4, np.float32), np.full((1, 1, 1, 4), -0.0, np.float32))
    assert np.signbit(dz).all()


@pytest.mark.parametrize('shape', [s for s in sg.SHAPES + sg.EDGE_SHAPES if s[1] >= 3 and s[2] >= 3], ids=_ID)
def test_order_data_set_tells_summation_orders_apart(shape):
    """on 'order' the declared ascending order and the descending one give different float32 bits (2^24 + 1 - 2^24 + 1 is 1, 2 or 0
    by the order): a kernel that added a pixel's terms in another order would fail on it.  In exact arithmetic both are equal."""
    z, bias, dpool = sg.pool_case('order', shape)
    up, down = sg.relu_maxpool3_backward_np(z, bias, dpool), sg.relu_maxpool3_backward_np(z, bias, dpool, descending=True)
    assert not np.array_equal(up.view(np.uint32), down.view(np.uint32))
    _, dz64 = _torch_pool_backward(z, bias, dpool)
    assert (np.abs(up - dz64) <= 2.0).all() and (up != dz64).any()              # the same winners: only the rounding differs
    # a peak with all four windows holds the four terms
    if shape[1] >= 4 and shape[2] >= 4:
        assert set(np.unique(np.abs(dpool[0, :2, :2, 0]))) == {1.0, sg.BIG}


# ---- 2. conv1's gradients ---------------------------------------------------------------------------------------------------------------
def test_stem_weight_gradient_statement_equals_float64_autograd():
    rng = np.random.default_rng(3)
    B, H, W = 2, 9, 11
    Ho, Wo = sg.pooled_shape(H, W)
    img, w = rng.standard_normal((B, H, W, 3)), rng.standard_normal((64, 7, 7, 3))
    dz = rng.standard_normal((B, Ho, Wo, 64))
    x64 = torch.tensor(img).permute(0, 3, 1, 2)
    w64 = torch.tensor(w).permute(0, 3, 1, 2).contiguous().requires_grad_()
    b64 = torch.zeros(64, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x64, w64, b64, stride=2, padding=3)
    assert tuple(y.shape) == (B, 64, Ho, Wo)
    assert np.allclose(sg.stem_conv_np(img, w), y.detach().permute(0, 2, 3, 1).numpy(), rtol=0, atol=1e-12)
    y.backward(torch.tensor(dz).permute(0, 3, 1, 2))
    dw, db = sg.stem_wgrad_np(img, dz)
    assert dw.shape == (64, 7, 7, 3) and np.allclose(dw, w64.grad.permute(0, 2, 3, 1).numpy(), rtol=0, atol=1e-11)
    assert np.allclose(db, b64.grad.numpy(), rtol=0, atol=1e-12)
    adw, adb = sg.stem_wgrad_np(img, dz, absolute=True)
    assert (adw >= np.abs(dw) - 1e-12).all() and (adb >= np.abs(db) - 1e-12).all()


# ---- 3. the dependency rule ---------------------------------------------------------------------------------------------------------------
def test_train_stem_needs_train_extractor():
    from tf_eager_object_detection_amd.model.caller_base import check_train_dependencies
    with pytest.raises(ValueError, match='train_stem=True needs train_extractor=True: '):
        check_train_dependencies(False, True, True, True, has_neck=True, train_stem=True)
    with pytest.raises(ValueError, match='train_stem=True needs train_extractor=True: '):
        check_train_dependencies(False, False, False, False, has_neck=True, train_stem=True)
    check_train_dependencies(True, True, True, True, has_neck=True, train_stem=True)
    check_train_dependencies(True, True, False, True, has_neck=True, train_stem=True)
    check_train_dependencies(True, True, True, True, has_neck=True)                         # (the default: off)
    with pytest.raises(ValueError, match='train_extractor=True needs train_neck=True'):    # the older rules still speak first
        check_train_dependencies(True, False, True, True, has_neck=True, train_stem=True)


# ---- 4. the C entry point ---------------------------------------------------------------------------------------------------------------
_POOL = dict(z=0x10000, bias=0x20000, dpool=0x30000, dz=0x40000, B=1, H=5, W=4, C=8)


def _call(L, **bad):
    a = dict(_POOL, **bad)
    return L.odet_relu_maxpool3_backward_f32(a['z'], a['bias'], a['dpool'], a['dz'], a['B'], a['H'], a['W'], a['C'], None)


def test_entry_point_refuses_bad_arguments_before_any_device_call():
    from tf_eager_object_detection_amd import _lib
    L = _lib.lib()
    for label, bad in [('H 0', dict(H=0)), ('W 0', dict(W=0)), ('H -1', dict(H=-1)), ('B -1', dict(B=-1)), ('C 6', dict(C=6)),
                       ('C 0', dict(C=0)), ('C -4', dict(C=-4)), ('null z', dict(z=None)), ('null bias', dict(bias=None)),
                       ('null dpool', dict(dpool=None)), ('null dz', dict(dz=None)), ('misaligned z', dict(z=0x10004)),
                       ('misaligned bias', dict(bias=0x20008)), ('misaligned dpool', dict(dpool=0x3000c)),
                       ('misaligned dz', dict(dz=0x40004)),
                       ('2^31 workgroups', dict(B=1 << 20, H=12 * 64, W=30 * 32, C=64))]:
        rc = _call(L, **bad)
        msg = L.odet_last_error()
        assert rc == -1, '%s returned %d: %r' % (label, rc, msg)                                      # ODET_E_INVALID
        assert msg.startswith(b'odet_relu_maxpool3_backward_f32') and b' failed: ' not in msg, msg    # (no HIP call was made)
    assert _call(L, B=0) == 0                                                                         # nothing to do


def test_header_library_and_binding_agree_on_the_symbol():
    from tf_eager_object_detection_amd import _build, _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'odet.h')).read()
    sym = 'odet_relu_maxpool3_backward_f32'
    assert ('int odet_relu_maxpool3_backward_f32(const float* z, const float* bias, const float* dpool, float* dz, int B, int H, int W, '
            'int C,') in header
    assert sym in header.split('#define ODET_VERSION')[0]                                             # the list of additions
    assert hasattr(C.CDLL(_lib.LIB_PATH), sym)
    assert 'resnet_fpn.py:233-242' in header
    assert '#define ODET_VERSION 103' in header and _lib.ODET_VERSION == 103
    assert 'stem_grad.hip' in _build.SOURCES
    res, args = _lib.SIGNATURES[sym]
    assert res is C.c_int and args == [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_void_p]


def test_python_front_refuses_cpu_and_malformed_operands(monkeypatch):
    """the rules of the backward ops' shared front, in its order: dtype, form, contiguity, shapes, device -- all before any call"""
    from tf_eager_object_detection_amd import ops
    z, b, g = torch.zeros(1, 5, 4, 8), torch.zeros(8), torch.zeros(1, 3, 2, 8)
    with pytest.raises(ValueError, match='relu_maxpool3_backward: z must be a GPU tensor'):
        ops.relu_maxpool3_backward(z, b, g)
    with pytest.raises(ValueError, match='dpool must be a float32 tensor'):
        ops.relu_maxpool3_backward(z, b, g.half())
    with pytest.raises(ValueError, match='z must be contiguous'):
        ops.relu_maxpool3_backward(z.permute(0, 2, 1, 3), b, g)
    with pytest.raises(ValueError, match=r'dpool \(1, 3, 3, 8\) does not go with z \(1, 5, 4, 8\) \(the pooled map is \(1, 3, 2, 8\)\)'):
        ops.relu_maxpool3_backward(z, b, torch.zeros(1, 3, 3, 8))
    with pytest.raises(ValueError, match='C a positive multiple of 4'):
        ops.relu_maxpool3_backward(torch.zeros(1, 5, 4, 6), torch.zeros(6), torch.zeros(1, 3, 2, 6))
    with pytest.raises(ValueError, match='bias .* does not go with z'):
        ops.relu_maxpool3_backward(z, torch.zeros(4), g)
    with ops.f32_form('x3'):
        with pytest.raises(ValueError, match="runs only under f32_form 'exact'"):
            ops.relu_maxpool3_backward(z, b, g)
    img, w = torch.zeros(1, 9, 11, 3), torch.zeros(64, 3, 7, 7)
    with pytest.raises(ValueError, match='stem_trainable: images must be a GPU tensor'):
        ops.stem_trainable(img, w, torch.zeros(64))
    with pytest.raises(ValueError, match=r'weight \(64, 3, 3, 3\) and bias \(64,\) must be'):
        ops.stem_trainable(img, torch.zeros(64, 3, 3, 3), torch.zeros(64))
    with pytest.raises(ValueError, match='images must be a float32 tensor'):
        ops.stem_trainable(img.half(), w, torch.zeros(64))
    # one patch group only
    monkeypatch.setattr(ops, 'PATCH_BYTES_MAX', 5 * 6 * 160 * 4 - 1)
    with pytest.raises(ValueError, match=r'takes 19200 bytes, more than one group of 19199'):
        ops.stem_trainable(img, w, torch.zeros(64))
