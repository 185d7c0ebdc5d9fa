"""The VGG16 training graph's two new operators without a GPU: the NumPy statements of odet_relu_maxpool2_backward_f32 and
odet_dropout_f32 / odet_dropout_backward_f32 (tests/vgg_grad_np.py) -- the pooling backward against float64 torch autograd of
max_pool2d(relu(z + b), 2, 2, ceil_mode=True), the dropout mask's rule and statistics --, the entry points' refusal rules through the
built library (each returns before any HIP call), header / library / binding agreeing on the symbols, and the Python fronts' and the
constructors' argument errors on CPU tensors."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vgg_grad_np as vg

_ID = lambda c: '%dx%d' % tuple(c) if isinstance(c, tuple) else None


def _torch_pool_backward(z, bias, dpool):
    """float64 torch-CPU autograd of max_pool2d(relu(z + b), 2, 2, ceil_mode=True) -> dz as an NHWC array"""
    zt = torch.tensor(np.ascontiguousarray(z), dtype=torch.float64).permute(0, 3, 1, 2).contiguous().requires_grad_()
    b = torch.tensor(bias, dtype=torch.float64).view(1, -1, 1, 1)
    y = F.max_pool2d(torch.relu(zt + b), 2, 2, ceil_mode=True)
    y.backward(torch.tensor(np.ascontiguousarray(dpool), dtype=torch.float64).permute(0, 3, 1, 2))
    return y.detach().permute(0, 2, 3, 1).numpy(), zt.grad.permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize('kind', ['int', 'normal'])
@pytest.mark.parametrize('hw', vg.SIZES, ids=_ID)
def test_pool_statement_equals_torch_autograd(hw, kind):
    for B, Cc in ((1, 4), (2, 8)):
        z, bias, dpool = vg.pool_case(kind, hw, B, Cc)
        dz = vg.relu_maxpool2_backward(z, bias, dpool)
        y, want = _torch_pool_backward(z, bias, dpool)
        assert dz.dtype == np.float32 and dz.shape == z.shape
        assert np.array_equal(dz.astype(np.float64), want), (hw, kind, B, Cc)
        assert not np.signbit(dz[dz == 0]).any()                                      # +0 wherever nothing passes
        if kind == 'int':                                                             # (exact sums: the forward agrees too)
            assert np.array_equal(vg.relu_maxpool2_forward(z, bias).astype(np.float64), y)
        # every window passes its gradient to at most one position
        H, W = hw
        OH, OW = vg.pooled_shape(H, W)
        pad = np.zeros((B, 2 * OH, 2 * OW, Cc), np.float32)
        pad[:, :H, :W] = dz
        hits = sum((pad[:, dy::2, dx::2] != 0).astype(int) for dy, dx in vg.TAPS)
        assert hits.max() <= 1


def test_integer_data_holds_positive_ties_and_empty_windows():
    """the integer data set does what it is for: windows whose positive maximum appears twice or more (the first one must win) and
    windows with nothing positive (nothing passes), at every size with more than one tap a window"""
    total = [0, 0, 0]
    for hw in vg.SIZES:
        for B, Cc in ((1, 4), (2, 8)):
            z, bias, _ = vg.pool_case('int', hw, B, Cc)
            assert set(np.unique(z)) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
            got = vg.window_census(z, bias)
            total = [a + b for a, b in zip(total, got)]
            if hw[0] * hw[1] >= 20 and Cc == 8:
                assert got[1] > 0 and got[2] > 0, (hw, got)
    print('\nwindows %d, with a repeated positive maximum %d, with nothing positive %d' % tuple(total))
    assert total[1] > 0 and total[2] > 0


def test_pool_statement_by_hand():
    """one window each: the first of two equal maxima wins; a maximum of exactly 0 passes nothing; bias decides the sign; an edge
    window holds only its taps inside the map"""
    z = np.array([[[3, 3], [1, 3]]], np.float32).reshape(1, 2, 2, 1)
    g = np.full((1, 1, 1, 1), 5, np.float32)
    assert np.array_equal(vg.relu_maxpool2_backward(z, [0.0], g).reshape(2, 2), [[5, 0], [0, 0]])
    assert np.array_equal(vg.relu_maxpool2_backward(z, [-3.0], g).reshape(2, 2), [[0, 0], [0, 0]])        # the maximum is 0
    assert np.array_equal(vg.relu_maxpool2_backward(-z, [2.0], g).reshape(2, 2), [[0, 0], [5, 0]])        # a = -1 -1 / 1 -1
    z = np.array([1, 2, 7], np.float32).reshape(1, 1, 3, 1)                                               # windows {1, 2} and {7}
    g = np.array([4, 9], np.float32).reshape(1, 1, 2, 1)
    assert np.array_equal(vg.relu_maxpool2_backward(z, [0.0], g).reshape(3), [0, 4, 9])
    assert vg.pool_backward_bytes(1, 150, 200, 256) == 4 * (2 * 150 * 200 + 75 * 100) * 256


def test_dropout_statement():
    n = 128 * 4096
    x = np.random.default_rng(3).standard_normal(n).astype(np.float32)
    keep = vg.dropout_keep(n, 0.5, 11, 5, 6)
    assert set(np.unique(keep)) == {0.0, 1.0}
    share = float(keep.mean())
    print('\nkept share of %d elements at keep_prob 0.5: %.5f' % (n, share))
    assert abs(share - 0.5) <= 0.005                                # 7 sigma of a fair draw, sigma = 0.00069
    # forward and backward use the same mask
    y, dx = vg.dropout(x, 0.5, 11, 5, 6), vg.dropout_backward(x, 0.5, 11, 5, 6)
    assert np.array_equal(y != 0, keep != 0) and np.array_equal(dx != 0, keep != 0)
    assert np.array_equal(y[keep == 1], x[keep == 1] / np.float32(0.5))
    # another image, stream or seed is another mask
    for other in ((11, 6, 6), (11, 5, 7), (12, 5, 6), (11 + (1 << 32), 5, 6)):
        k2 = vg.dropout_keep(n, 0.5, *other)
        assert 0.45 < float((k2 != keep).mean()) < 0.55, other
    # the words: element e takes word e & 3 of the group's Philox call
    import targets_np as tn
    w = vg.dropout_words(9, 11, 5, 6)
    for e in range(9):
        assert int(w[e]) == int(tn.philox((e >> 2, 5, 6, 0), (11, 0))[e & 3])
    # keep_prob 1 returns the input unchanged
    assert np.array_equal(vg.dropout(x, 1.0, 11, 5, 6).view(np.uint32), x.view(np.uint32))
    assert np.array_equal(vg.dropout_backward(x, 1.0, 11, 5, 6).view(np.uint32), x.view(np.uint32))


def test_dropout_statement_at_keep_prob_0_7():
    """0.7 is no float32: keep = floor(float32(0.7) + u) with the float32 sum, and (x / kp) * keep differs from x * (keep / kp) and
    from the backward's (x * keep) / kp in the last bit for some x"""
    n = 1 << 16
    kp = np.float32(0.7)
    words = vg.dropout_words(n, 1, 0, 7)
    u = ((words & np.uint32(0x7FFFFF)) | np.uint32(0x3F800000)).view(np.float32) - np.float32(1.0)
    assert u.min() >= 0 and u.max() < 1
    keep = vg.dropout_keep(n, 0.7, 1, 0, 7)
    assert np.array_equal(keep, np.floor(kp + u)) and keep.dtype == np.float32
    # the float32 sum decides: where the float64 sum of the same operands stays below 1 and the float32 one rounds up to it
    exact = np.floor(np.float64(kp) + u.astype(np.float64))
    assert (keep >= exact).all()
    assert abs(float(keep.mean()) - 0.7) < 0.01
    x = np.random.default_rng(5).standard_normal(n).astype(np.float32)
    y = vg.dropout(x, 0.7, 1, 0, 7)
    assert np.array_equal(y, (x / kp) * keep)
    other = x * (np.float32(1.0) / kp) * keep
    assert (y != other).any()                                       # the division order is observable
    dx = vg.dropout_backward(x, 0.7, 1, 0, 7)
    assert np.array_equal(dx, (x * keep) / kp)


# ---- the C entry points: every refusal happens before any HIP call ------------------------------------------------------------------
_POOL = dict(z=0x10000, bias=0x20000, dpool=0x30000, dz=0x40000, B=1, H=5, W=4, C=8)
_DROP = dict(x=0x10000, y=0x20000, n=100, keep_prob=0.5, seed=1, image_id=0, stream_id=6)


def _call(L, name, good, **bad):
    a = dict(good, **bad)
    if name == 'odet_relu_maxpool2_backward_f32':
        return L.odet_relu_maxpool2_backward_f32(a['z'], a['bias'], a['dpool'], a['dz'], a['B'], a['H'], a['W'], a['C'], None)
    return getattr(L, name)(a['x'], a['y'], a['n'], a['keep_prob'], a['seed'], a['image_id'], a['stream_id'], None)


def test_entry_points_refuse_bad_arguments_before_any_device_call():
    from tf_eager_object_detection_amd import _lib
    L = _lib.lib()
    rows = [('odet_relu_maxpool2_backward_f32', _POOL, label, bad) for label, bad in [
        ('H 0', dict(H=0)), ('W 0', dict(W=0)), ('H -1', dict(H=-1)), ('B -1', dict(B=-1)), ('C 6', dict(C=6)), ('C 0', dict(C=0)),
        ('C -4', dict(C=-4)), ('null z', dict(z=None)), ('null bias', dict(bias=None)), ('null dpool', dict(dpool=None)),
        ('null dz', dict(dz=None)), ('misaligned z', dict(z=0x10004)), ('misaligned bias', dict(bias=0x20008)),
        ('misaligned dpool', dict(dpool=0x3000c)), ('misaligned dz', dict(dz=0x40004))]]
    for name in ('odet_dropout_f32', 'odet_dropout_backward_f32'):
        rows += [(name, _DROP, label, bad) for label, bad in [
            ('keep_prob 0', dict(keep_prob=0.0)), ('keep_prob -0.5', dict(keep_prob=-0.5)), ('keep_prob 1.5', dict(keep_prob=1.5)),
            ('keep_prob nan', dict(keep_prob=float('nan'))), ('n -1', dict(n=-1)), ('n 2^34 + 1', dict(n=(1 << 34) + 1)),
            ('null x', dict(x=None)), ('null y', dict(y=None)), ('misaligned x', dict(x=0x10004)), ('misaligned y', dict(y=0x20008))]]
    for name, good, label, bad in rows:
        rc = _call(L, name, good, **bad)
        msg = L.odet_last_error()
        print('%s: %s -> %d %r' % (name, label, rc, msg))
        assert rc == -1, '%s: %s returned %d: %r' % (name, label, rc, msg)                            # ODET_E_INVALID
        assert msg.startswith(name.encode()) and b' failed: ' not in msg, msg                         # (no HIP call was made)
    # nothing to do is a no-op that returns OK
    assert _call(L, 'odet_relu_maxpool2_backward_f32', _POOL, B=0) == 0
    for name in ('odet_dropout_f32', 'odet_dropout_backward_f32'):
        assert _call(L, name, _DROP, n=0) == 0 and _call(L, name, _DROP, n=0, x=None, y=None) == 0
        assert _call(L, name, _DROP, keep_prob=1.0, y=_DROP['x']) == 0                 # in place at keep_prob 1: nothing to copy


def test_header_library_and_binding_agree_on_the_symbols():
    from tf_eager_object_detection_amd import _build, _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'odet.h')).read()
    assert ('int odet_relu_maxpool2_backward_f32(const float* z, const float* bias, const float* dpool, float* dz, int B, int H, int W, '
            'int C,') in header
    assert ('int odet_dropout_f32(const float* x, float* y, long long n, float keep_prob, uint64_t seed, uint32_t image_id, '
            'uint32_t stream_id,') in header
    assert ('int odet_dropout_backward_f32(const float* dy, float* dx, long long n, float keep_prob, uint64_t seed, uint32_t image_id,'
            ) in header
    for sym in ('odet_relu_maxpool2_backward_f32', 'odet_dropout_f32', 'odet_dropout_backward_f32'):
        assert sym in header.split('#define ODET_VERSION')[0], sym                                    # the list of additions
        assert hasattr(C.CDLL(_lib.LIB_PATH), sym), sym
    assert 'vgg16_faster_rcnn.py:307, 325' in header and 'vgg16_faster_rcnn.py:250-253' in header
    assert '#define ODET_VERSION 103' in header and _lib.ODET_VERSION == 103
    assert 'vgg_grad.hip' in _build.SOURCES
    res, args = _lib.SIGNATURES['odet_relu_maxpool2_backward_f32']
    assert res is C.c_int and args == [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_void_p]
    for sym in ('odet_dropout_f32', 'odet_dropout_backward_f32'):
        res, args = _lib.SIGNATURES[sym]
        assert res is C.c_int and args == [C.c_void_p, C.c_void_p, C.c_longlong, C.c_float, C.c_uint64, C.c_uint32, C.c_uint32,
                                           C.c_void_p]


# ---- the Python fronts and the constructors, on CPU tensors -----------------------------------------------------------------------
def test_python_fronts_refuse_on_cpu_tensors():
    from tf_eager_object_detection_amd import ops
    z, b, g = torch.zeros(1, 5, 4, 8), torch.zeros(8), torch.zeros(1, 3, 2, 8)
    pool = ops.relu_maxpool2_backward
    for bad, match in (((z.half(), b, g), 'float32'), ((z, b.double(), g), 'float32'), ((z, b, g.half()), 'float32'),
                       ((z.permute(0, 2, 1, 3), b, g), 'contiguous'), ((z, b, g.permute(0, 2, 1, 3)), 'contiguous'),
                       ((z[0], b, g), 'NHWC'), ((torch.zeros(1, 5, 4, 6), torch.zeros(6), torch.zeros(1, 3, 2, 6)), 'multiple of 4'),
                       ((torch.zeros(1, 0, 4, 8), b, g), 'positive'), ((z, torch.zeros(4), g), 'bias'),
                       ((z, b, torch.zeros(1, 2, 2, 8)), 'dpool'), ((z, b, torch.zeros(1, 3, 3, 8)), 'dpool'),
                       ((z, b, torch.zeros(2, 3, 2, 8)), 'dpool')):
        with pytest.raises(ValueError, match=match):
            pool(*bad)
    with pytest.raises(ValueError, match='GPU'):                     # (and no CPU path behind the checks)
        pool(z, b, g)
    x = torch.zeros(5, 13)
    for fn in (ops.dropout, ops.dropout_backward):
        for kp in (0.0, -0.1, 1.5, float('nan')):
            with pytest.raises(ValueError, match='keep_prob'):
                fn(x, kp, 0, 0, 6)
        with pytest.raises(ValueError, match='float32'):
            fn(x.half(), 0.5, 0, 0, 6)
        with pytest.raises(ValueError, match='contiguous'):
            fn(x.t(), 0.5, 0, 0, 6)
        with pytest.raises(ValueError, match='seed'):
            fn(x, 0.5, -1, 0, 6)
        with pytest.raises(ValueError, match='stream_id'):
            fn(x, 0.5, 0, 0, -1)
        with pytest.raises(ValueError, match='GPU'):
            fn(x, 0.5, 0, 0, 6)
    with pytest.raises(ValueError, match='keep_prob'):
        ops.dropout_trainable(x, 1.5, 0, 0, 6)
    assert ops.dropout_trainable(x, 1.0, 0, 0, 6) is x               # tf.nn.dropout returns its input at keep_prob 1
    assert (ops.DROPOUT_STREAM_FC1, ops.DROPOUT_STREAM_FC2) == (vg.STREAM_DROPOUT_FC1, vg.STREAM_DROPOUT_FC2) == (6, 7)
    xc, w, bias = torch.zeros(1, 5, 7, 64), torch.zeros(64, 64, 3, 3), torch.zeros(64)
    conv = ops.conv3x3_relu_pool_trainable
    for bad, match in (((xc.half(), w, bias), 'float32'), ((xc, w.half(), bias), 'float32'), ((xc, w, bias.half()), 'float32'),
                       ((xc.permute(0, 2, 1, 3), w, bias), 'contiguous'), ((xc[0], w, bias), 'NHWC'),
                       ((torch.zeros(1, 5, 7, 48), torch.zeros(64, 48, 3, 3), bias), 'multiple of 32'),
                       ((xc, torch.zeros(32, 64, 3, 3), torch.zeros(32)), 'one of 64'), ((xc, w, torch.zeros(32)), 'bias'),
                       ((xc, torch.zeros(64, 32, 3, 3), bias), 'weight')):
        with pytest.raises(ValueError, match=match):
            conv(*bad)
    with pytest.raises(ValueError, match='GPU'):
        conv(xc, w, bias)
    for form in ('x3', 'x2'):
        with ops.f32_form(form):
            for call in (lambda: pool(z, b, g), lambda: ops.dropout(x, 0.5, 0, 0, 6), lambda: ops.dropout_backward(x, 0.5, 0, 0, 6),
                         lambda: conv(xc, w, bias)):
                with pytest.raises(ValueError, match="only under f32_form 'exact'"):
                    call()


def test_detector_trainable_parts_refuse_other_forms_without_a_gpu():
    from tf_eager_object_detection_amd.model import rpn_trainable, vgg_trainable
    from tf_eager_object_detection_amd.model.frcnn_detector import Vgg16Detector
    det = Vgg16Detector(21, (64, 64), 1, dtype=torch.float32)
    assert [i for i, _ in det._layer_plan()] == list(range(1, 13))
    assert [i for i, pooled in det._layer_plan() if pooled] == [1, 3, 6, 9]           # block1..block4's last convolutions
    for attr, bad in (('f32_form', 'x3'), ('f32_form', 'x2'), ('dtype', torch.float16)):
        good = getattr(det, attr)
        setattr(det, attr, bad)
        try:
            with pytest.raises(ValueError, match='extractor_trainable needs'):
                vgg_trainable.extractor_trainable(det, torch.zeros(1, 64, 64, 3))
            with pytest.raises(ValueError, match='rpn_trainable needs'):
                rpn_trainable.rpn_trainable(det, [torch.zeros(1, 512, 4, 4)])
            with pytest.raises(ValueError, match='roi_head_trainable needs'):
                vgg_trainable.roi_head_trainable(det, torch.zeros(2, 7, 7, 512))
        finally:
            setattr(det, attr, good)


def test_caller_model_keyword_rules():
    import inspect
    from tf_eager_object_detection_amd.model.base_faster_rcnn_model import BaseFasterRcnn, ResNetFasterRcnn, Vgg16FasterRcnn
    sig = inspect.signature(Vgg16FasterRcnn.__init__).parameters
    assert [sig[k].default for k in ('train_roi_head', 'train_rpn_head', 'train_extractor', 'dropout_seed')] == [False, False, False, 0]
    assert (BaseFasterRcnn._train_roi_head, BaseFasterRcnn._train_rpn_head, BaseFasterRcnn._train_extractor) == (False, False, False)
    with pytest.raises(ValueError, match='train_extractor=True needs train_rpn_head=True or train_roi_head=True'):
        Vgg16FasterRcnn(train_extractor=True, device='cpu')
    for name, what in (('train_roi_head', 'Dense backward'), ('train_rpn_head', 'convolution backward'),
                       ('train_extractor', 'convolution and pooling backward')):
        kw = {name: True, 'train_roi_head': True} if name == 'train_extractor' else {name: True}
        with pytest.raises(ValueError, match='%s=True needs dtype=torch.float32 and f32_form=\'exact\' \\(the %s' % (name, what)):
            Vgg16FasterRcnn(dtype=torch.float16, device='cpu', **kw)
        for form in ('x3', 'x2'):
            with pytest.raises(ValueError, match='%s=True needs dtype' % name):
                Vgg16FasterRcnn(f32_form=form, device='cpu', **kw)
    with pytest.raises(ValueError, match='roi_head_keep_dropout_rate'):
        Vgg16FasterRcnn(train_roi_head=True, roi_head_keep_dropout_rate=0.0, device='cpu')
    for name in ('train_roi_head', 'train_rpn_head', 'train_extractor', 'dropout_seed'):
        with pytest.raises(NotImplementedError, match='ResNetFasterRcnn: %s' % name):
            ResNetFasterRcnn(depth=50, device='cpu', **{name: True})
    with pytest.raises(TypeError, match='unexpected keyword'):
        Vgg16FasterRcnn(train_neck=True, device='cpu')
    m = Vgg16FasterRcnn(train_roi_head=True, train_rpn_head=True, train_extractor=True, dropout_seed=9, device='cpu')
    assert (m._train_roi_head, m._train_rpn_head, m._train_extractor, m._dropout_seed, m._next_dropout_image_id) == (True, True, True, 9, 0)
    assert m._roi_pooling._trainable
    plain = Vgg16FasterRcnn(device='cpu')
    assert not (plain._train_roi_head or plain._train_rpn_head or plain._train_extractor or plain._roi_pooling._trainable)
    assert len(list(m.dense.parameters())) == 40                        # 13 convolutions, the RpnHead's 3, fc1, fc2, score, bbox
