"""The ResNet-C4 training graph's new operator without a GPU: the NumPy statements of odet_global_avg_pool_f32 and
odet_global_avg_pool_backward_f32 (tests/c4_grad_np.py) -- their accuracy against float64, the transpose property, the edge
behaviour the order implies --, the entry points' refusal rules through the built library (each returns before any HIP call),
header / library / binding agreeing on the symbols, the Python fronts' argument errors on CPU tensors, the keyword rules of
TrainableResNetFasterRcnn and the trained / frozen parameter lists read off the module tree."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

import c4_grad_np as c4

U24 = 2.0 ** -24


# ---- the statements ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(16, 7, 7, 256), (3, 1, 1, 8), (5, 3, 5, 64)], ids=lambda s: 'x'.join(map(str, s)))
def test_forward_statement_is_within_50_units_of_the_float64_mean(shape):
    """non-negative data: every partial sum is at most the total, so hw - 1 rounded adds and one rounded division stay within
    (hw - 1 + 1) * 2^-24 <= 50 * 2^-24 relative for hw <= 49; a wrong divisor or a dropped pixel is a relative error of 1 / hw"""
    rng = np.random.default_rng(1)
    x = np.abs(rng.standard_normal(shape)).astype(np.float32)
    hw = shape[1] * shape[2]
    assert hw <= 49
    want = x.astype(np.float64).reshape(shape[0], hw, shape[3]).mean(axis=1)
    got = c4.gap_forward(x)
    assert got.dtype == np.float32 and got.shape == (shape[0], shape[3])
    rel = np.abs(got.astype(np.float64) - want) / want
    print('\n%s: worst relative error %.2f units of 2^-24' % (shape, float(rel.max()) / U24))
    assert float(rel.max()) <= 50 * U24
    if hw > 1:                                                      # the bound tells a wrong divisor and a dropped pixel
        wrong = got.astype(np.float64) * hw / (hw - 1)
        assert float((np.abs(wrong - want) / want).min()) > 50 * U24
        dropped = c4.gap_forward(x.reshape(shape[0], hw, shape[3])[:, :-1]).astype(np.float64) * (hw - 1) / hw
        assert float((np.abs(dropped - want) / want).max()) > 50 * U24


def test_forward_statement_adds_in_pixel_order():
    """data on which the order shows: 2^24, then forty-eight 1s -- added first to last every 1 is rounded away; added in any
    order that pairs the 1s first, they are not"""
    x = np.ones((1, 7, 7, 4), dtype=np.float32)
    x[0, 0, 0, :] = 2.0 ** 24
    assert np.array_equal(c4.gap_forward(x), np.full((1, 4), np.float32(2.0 ** 24) / np.float32(49), dtype=np.float32))
    assert float(c4.gap_forward(x[:, ::-1, ::-1])[0, 0]) == float(np.float32(2.0 ** 24 + 48) / np.float32(49))


def test_backward_statement_is_the_transpose_of_the_forward():
    """small integers and hw = 64: every sum, and the division by a power of two, is exact, so the two inner products agree exactly"""
    rng = np.random.default_rng(2)
    x = rng.integers(-8, 9, (5, 8, 8, 12)).astype(np.float32)
    g = rng.integers(-8, 9, (5, 12)).astype(np.float32)
    y = c4.gap_forward(x)
    dx = c4.gap_backward(g, (8, 8))
    assert dx.shape == x.shape and dx.dtype == np.float32
    assert np.array_equal(c4.gap_backward(g, 64).reshape(x.shape), dx)
    lhs = float((y.astype(np.float64) * g).sum())
    rhs = float((x.astype(np.float64) * dx).sum())
    assert lhs == rhs and lhs != 0.0
    assert np.array_equal(y.astype(np.float64), x.astype(np.float64).reshape(5, 64, 12).sum(axis=1) / 64)
    assert np.array_equal(dx, np.broadcast_to((g / np.float32(64))[:, None, None, :], x.shape))
    # not a power of two: still one division per element, the same for every pixel
    d49 = c4.gap_backward(g, (7, 7))
    assert np.array_equal(d49, np.broadcast_to((g / np.float32(49))[:, None, None, :], d49.shape))
    assert (d49 != g[:, None, None, :] * (np.float32(1) / np.float32(49))).any()          # the reciprocal form is observable


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_statement_edges():
    rng = np.random.default_rng(3)
    # hw = 1: the input's bits (x / 1)
    x = rng.standard_normal((4, 1, 1, 8)).astype(np.float32)
    x[0, 0, 0, 0], x[1, 0, 0, 1] = -0.0, np.float32(1e-42)
    assert np.array_equal(_bits(c4.gap_forward(x)), _bits(x.reshape(4, 8)))
    assert np.array_equal(_bits(c4.gap_backward(x.reshape(4, 8), (1, 1))), _bits(x))
    # a NaN / an infinity in one pixel reaches its own (r, c) output and no other
    x = rng.standard_normal((3, 7, 7, 8)).astype(np.float32)
    clean = c4.gap_forward(x)
    bad = x.copy()
    bad[1, 3, 4, 5], bad[2, 6, 6, 0], bad[0, 0, 0, 7] = np.nan, np.inf, -np.inf
    got = c4.gap_forward(bad)
    assert np.isnan(got[1, 5]) and got[2, 0] == np.inf and got[0, 7] == -np.inf
    mask = np.ones(got.shape, bool)
    mask[1, 5] = mask[2, 0] = mask[0, 7] = False
    assert np.array_equal(_bits(got[mask]), _bits(clean[mask]))
    # -0 in every pixel gives -0 (the sum starts from the first element, not from +0); one +0 among them gives +0
    z = np.full((2, 7, 7, 4), -0.0, dtype=np.float32)
    assert np.array_equal(_bits(c4.gap_forward(z)), _bits(np.full((2, 4), -0.0, dtype=np.float32)))
    z[1, 3, 3, 2] = 0.0
    want = np.full((2, 4), -0.0, dtype=np.float32)
    want[1, 2] = 0.0
    assert np.array_equal(_bits(c4.gap_forward(z)), _bits(want))
    assert np.array_equal(_bits(c4.gap_backward(want, (2, 3))), _bits(np.broadcast_to(want[:, None, None, :], (2, 2, 3, 4))))


# ---- the C entry points: every refusal happens before any HIP call ------------------------------------------------------------------
_GOOD = dict(a=0x10000, rows=2, hw=49, channels=8, b=0x20000)
SYMBOLS = ('odet_global_avg_pool_f32', 'odet_global_avg_pool_backward_f32')


def _call(L, name, **bad):
    a = dict(_GOOD, **bad)
    return getattr(L, name)(a['a'], a['rows'], a['hw'], a['channels'], a['b'], None)


def test_entry_points_refuse_bad_arguments_before_any_device_call():
    from tf_eager_object_detection_amd import _lib
    L = _lib.lib()
    for name in SYMBOLS:
        for label, bad in [('rows 0', dict(rows=0)), ('rows -1', dict(rows=-1)), ('hw 0', dict(hw=0)), ('hw -3', dict(hw=-3)),
                           ('channels 6', dict(channels=6)), ('channels 0', dict(channels=0)), ('channels -4', dict(channels=-4)),
                           ('null input', dict(a=None)), ('null output', dict(b=None)), ('misaligned input', dict(a=0x10004)),
                           ('misaligned output', dict(b=0x20008))]:
            rc = _call(L, name, **bad)
            msg = L.odet_last_error()
            print('%s: %s -> %d %r' % (name, label, rc, msg))
            assert rc == -1, '%s: %s returned %d: %r' % (name, label, rc, msg)                            # ODET_E_INVALID
            assert msg.startswith(name.encode()) and b' failed: ' not in msg, msg                         # (no HIP call was made)


def test_header_library_and_binding_agree_on_the_symbols():
    from tf_eager_object_detection_amd import _build, _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'odet.h')).read()
    assert 'int odet_global_avg_pool_f32(const float* x, int rows, int hw, int channels, float* out, odet_stream_t stream);' in header
    assert ('int odet_global_avg_pool_backward_f32(const float* g, int rows, int hw, int channels, float* dx, odet_stream_t stream);'
            in header)
    for sym in SYMBOLS:
        assert sym in header.split('#define ODET_VERSION')[0], sym                                    # the list of additions
        assert hasattr(C.CDLL(_lib.LIB_PATH), sym), sym
        res, args = _lib.SIGNATURES[sym]
        assert res is C.c_int and args == [C.c_void_p] + [C.c_int] * 3 + [C.c_void_p] * 2
    assert 'resnet_faster_rcnn.py:167-168' in header and '_MeanGrad' in header
    assert '#define ODET_VERSION 103' in header and _lib.ODET_VERSION == 103
    assert 'c4_grad.hip' in _build.SOURCES


# ---- the Python fronts, on CPU tensors ----------------------------------------------------------------------------------------------
def test_python_fronts_refuse_before_any_gpu_call():
    from tf_eager_object_detection_amd import ops
    x, g = torch.zeros(2, 3, 5, 8), torch.zeros(2, 8)
    fwd, bwd, tr = ops.global_avg_pool, ops.global_avg_pool_backward, ops.global_avg_pool_trainable
    for call, match in ((lambda: fwd(x.half()), 'float32'), (lambda: fwd(x.double()), 'float32'), (lambda: fwd(x[0]), 'NHWC'),
                        (lambda: fwd(x.reshape(2, 15, 8)), 'NHWC'), (lambda: fwd(x.permute(0, 2, 1, 3)), 'contiguous'),
                        (lambda: fwd(torch.zeros(2, 3, 5, 6)), 'multiple of 4'), (lambda: fwd(torch.zeros(2, 3, 5, 0)), 'multiple of 4'),
                        (lambda: fwd(torch.zeros(0, 3, 5, 8)), 'at least one row'), (lambda: fwd(torch.zeros(2, 0, 5, 8)), 'one pixel'),
                        (lambda: fwd(x, out=torch.zeros(2, 4)), 'out must be'), (lambda: fwd(x, out=torch.zeros(2, 8).half()), 'out must be'),
                        (lambda: fwd(x, out=torch.zeros(8, 2).t()), 'out must be'),
                        (lambda: bwd(g.half(), (3, 5)), 'float32'), (lambda: bwd(g[0], (3, 5)), '2-D'),
                        (lambda: bwd(x, (3, 5)), '2-D'), (lambda: bwd(g.t(), (3, 5)), 'contiguous'),
                        (lambda: bwd(torch.zeros(2, 6), (3, 5)), 'multiple of 4'), (lambda: bwd(torch.zeros(0, 8), (3, 5)), 'at least one row'),
                        (lambda: bwd(g, (0, 5)), 'positive'), (lambda: bwd(g, (3, -1)), 'positive'),
                        (lambda: bwd(g, (3, 5), out=torch.zeros(2, 5, 3, 8)), 'out must be'),
                        (lambda: tr(x.half()), 'float32'), (lambda: tr(x[0]), 'NHWC'), (lambda: tr(torch.zeros(2, 3, 5, 6)), 'multiple of 4')):
        with pytest.raises(ValueError, match=match) as e:
            call()
        assert str(e.value).startswith('global_avg_pool'), e.value
    for call in (lambda: fwd(x), lambda: bwd(g, (3, 5)), lambda: tr(x), lambda: fwd(x, out=torch.zeros(2, 8))):
        with pytest.raises(ValueError, match='must be a GPU tensor'):                 # (and no CPU path behind the checks)
            call()
    for form in ('x3', 'x2'):
        with ops.f32_form(form):
            for call in (lambda: fwd(x), lambda: bwd(g, (3, 5)), lambda: tr(x)):
                with pytest.raises(ValueError, match="only under f32_form 'exact'"):
                    call()
            with pytest.raises(ValueError, match='must be a float32 tensor'):         # dtype before the form, as in every front
                fwd(x.half())


def test_detector_trainable_parts_refuse_other_forms_without_a_gpu():
    from tf_eager_object_detection_amd.model import c4_trainable, rpn_trainable
    from tf_eager_object_detection_amd.model.frcnn_detector import ResNetC4Detector
    det = ResNetC4Detector(50, 21, (64, 64), 1, dtype=torch.float32)
    for attr, bad in (('f32_form', 'x3'), ('f32_form', 'x2'), ('dtype', torch.float16)):
        good = getattr(det, attr)
        setattr(det, attr, bad)
        try:
            with pytest.raises(ValueError, match='extractor_trainable needs'):
                c4_trainable.extractor_trainable(det, torch.zeros(1, 64, 64, 3))
            with pytest.raises(ValueError, match='rpn_trainable needs'):
                rpn_trainable.rpn_trainable(det, [torch.zeros(1, 1024, 4, 4)])
            with pytest.raises(ValueError, match='roi_head_trainable needs'):
                c4_trainable.roi_head_trainable(det, torch.zeros(2, 7, 7, 1024))
        finally:
            setattr(det, attr, good)


# ---- the caller object ------------------------------------------------------------------------------------------------------------------
def test_caller_model_keyword_rules():
    from tf_eager_object_detection_amd.model.base_faster_rcnn_model import ResNetFasterRcnn, TrainableResNetFasterRcnn
    T = TrainableResNetFasterRcnn
    assert issubclass(T, ResNetFasterRcnn)
    sig = inspect.signature(T.__init__).parameters
    assert [sig[k].default for k in ('train_roi_head', 'train_rpn_head', 'train_extractor')] == [False, False, False]
    assert 'dropout_seed' not in sig
    base = inspect.signature(ResNetFasterRcnn.__init__).parameters
    assert [(k, sig[k].default) for k in base if k not in ('self', 'kwargs')] == \
        [(k, base[k].default) for k in base if k not in ('self', 'kwargs')]
    with pytest.raises(ValueError, match='train_extractor=True needs train_rpn_head=True or train_roi_head=True'):
        T(train_extractor=True, device='cpu')
    for name, what in (('train_roi_head', 'bottleneck backward has'), ('train_rpn_head', 'convolution backward has'),
                       ('train_extractor', 'bottleneck backward has')):
        kw = {name: True, 'train_rpn_head': True} if name == 'train_extractor' else {name: True}
        with pytest.raises(ValueError, match='TrainableResNetFasterRcnn: %s=True needs dtype=torch.float32 and f32_form=\'exact\' '
                                             '\\(the %s' % (name, what)):
            T(dtype=torch.float16, device='cpu', **kw)
        for form in ('x3', 'x2'):
            with pytest.raises(ValueError, match='TrainableResNetFasterRcnn: %s=True needs dtype' % name):
                T(f32_form=form, device='cpu', **kw)
    for bad in (dict(train_neck=True), dict(dropout_seed=3), dict(roi_head_keep_dropout_rate=0.5)):
        with pytest.raises(TypeError, match='unexpected keyword'):
            T(device='cpu', **bad)
    with pytest.raises(ValueError, match='unknown resnet layers number'):
        T(depth=34, train_roi_head=True, device='cpu')
    m = T(train_roi_head=True, train_rpn_head=True, train_extractor=True, device='cpu')
    assert (m._train_roi_head, m._train_rpn_head, m._train_extractor) == (True, True, True) and m._roi_pooling._trainable
    assert m._get_trainable_roi_head() == m.dense.roi_head_trainable
    head_only = T(train_roi_head=True, device='cpu')
    assert (head_only._train_roi_head, head_only._train_rpn_head, head_only._train_extractor) == (True, False, False)
    assert head_only._roi_pooling._trainable
    rpn_only = T(train_rpn_head=True, num_classes=5, device='cpu')
    assert not rpn_only._roi_pooling._trainable and rpn_only.num_classes == 5
    off = T(device='cpu')
    assert not (off._train_roi_head or off._train_rpn_head or off._train_extractor or off._roi_pooling._trainable)
    plain = ResNetFasterRcnn(device='cpu')
    assert not (plain._train_roi_head or plain._train_rpn_head or plain._train_extractor or plain._roi_pooling._trainable)
    assert [n for n, _ in off.dense.named_parameters()] == [n for n, _ in plain.dense.named_parameters()]
    # the plain class keeps its refusal and now names the class that trains
    with pytest.raises(NotImplementedError, match='ResNetFasterRcnn: train_roi_head.*TrainableResNetFasterRcnn'):
        ResNetFasterRcnn(train_roi_head=True, device='cpu')


@pytest.mark.parametrize('depth, trained, total', [(50, 94, 116), (101, 196, 218)])
def test_trained_and_frozen_names_from_the_module_tree(depth, trained, total):
    from tf_eager_object_detection_amd.model import c4_trainable
    from tf_eager_object_detection_amd.model.extractor_trainable import block_layers
    from tf_eager_object_detection_amd.model.frcnn_detector import ResNetC4Detector
    det = ResNetC4Detector(depth, 21, (64, 64), 1, dtype=torch.float32)
    names = [n for n, _ in det.named_parameters()]
    got, frozen = c4_trainable.trained_names(det), c4_trainable.frozen_names(det)
    assert len(names) == total and len(got) == trained and len(frozen) == 22
    assert sorted(got + frozen) == sorted(names) and not set(got) & set(frozen)
    # counted from the tree itself: two parameters per convolution of every block, per RpnHead layer, per final layer
    per_stage = {s: 2 * sum(len(block_layers(b)) for b in getattr(det, s)) for s in ('conv2', 'conv3', 'conv4', 'conv5')}
    assert 2 + per_stage['conv2'] == 22
    assert per_stage['conv3'] + per_stage['conv4'] + per_stage['conv5'] + 6 + 4 == trained
    assert all(n.startswith(('conv1.', 'conv2.')) for n in frozen)
    head = c4_trainable.trained_names(det, rpn_head=False, extractor=False)
    assert len(head) == per_stage['conv5'] + 4 == 24 and all(n.startswith(('conv5.', 'score.', 'bbox.')) for n in head)
    assert len(c4_trainable.trained_names(det, roi_head=False, extractor=False)) == 6
    assert len(c4_trainable.trained_names(det, roi_head=False, rpn_head=False)) == per_stage['conv3'] + per_stage['conv4']
