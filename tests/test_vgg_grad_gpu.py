"""The VGG16 training graph on the GPU: odet_relu_maxpool2_backward_f32 and odet_dropout_f32 / odet_dropout_backward_f32
(csrc/vgg_grad.hip) bit-equal to the NumPy statements of tests/vgg_grad_np.py; ops.conv3x3_relu_pool_trainable behind
torch.autograd (forward = the detectors' launches, gradients = the ops by hand, exact on integer data, within the any-order summation
bound of tests/test_conv_grad_gpu.py on random data); Vgg16Detector's three trainable parts bit-equal to features / rpn / roi_head
with 32 trained parameters; and Vgg16FasterRcnn with the three keywords: losses, dropout seeds, a training step."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_grad_np as cg
import vgg_grad_np as vg

pytestmark = pytest.mark.gpu

U = 2.0 ** -23
_ID = lambda c: '%dx%d' % tuple(c) if isinstance(c, tuple) else None


def _ops():
    from tf_eager_object_detection_amd import ops
    return ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _np_bits_equal(got, want):
    got = got.detach().contiguous().cpu().numpy()
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), np.ascontiguousarray(want, np.float32).view(np.uint32))


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.detach().contiguous().view(torch.int32), b.detach().contiguous().view(torch.int32))


# ---- 1. the pooling backward ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [4, 64, 256])
@pytest.mark.parametrize('hw', vg.SIZES, ids=_ID)
def test_relu_maxpool2_backward_is_bit_equal_to_the_statement(hw, C):
    ops = _ops()
    for B in (1, 2):
        for kind in ('int', 'normal'):
            z, bias, dpool = vg.pool_case(kind, hw, B, C)
            want = vg.relu_maxpool2_backward(z, bias, dpool)
            tz, tb, tg = _dev(z), _dev(bias), _dev(dpool)
            out = torch.full(z.shape, float('nan'), device='cuda')                 # every element must be written
            got = ops.relu_maxpool2_backward(tz, tb, tg, out=out)
            assert got is out and _np_bits_equal(out, want), (hw, C, B, kind)
            again = ops.relu_maxpool2_backward(tz, tb, tg)                           # a fresh buffer, whatever it held
            assert _same_bits(again, out)
            # the forward the statement is the backward of: what odet_bias_relu_maxpool writes
            assert _np_bits_equal(ops.bias_relu_maxpool(tz, tb, 2, 2, 0, True), vg.relu_maxpool2_forward(z, bias))


def test_relu_maxpool2_backward_grid_stride_pass():
    """more windows than one pass of the grid holds (256 * 64 workgroups of 256 lanes): the grid-stride loop's second turn"""
    ops = _ops()
    hw, B, C = (262, 258), 1, 1024                               # 131 * 129 windows of 256 lanes each = 4.3 M lanes
    assert B * 131 * 129 * (C // 4) > 256 * 64 * 256
    z, bias, dpool = vg.pool_case('normal', hw, B, C)
    out = torch.full(z.shape, float('nan'), device='cuda')
    ops.relu_maxpool2_backward(_dev(z), _dev(bias), _dev(dpool), out=out)
    assert _np_bits_equal(out, vg.relu_maxpool2_backward(z, bias, dpool))


# ---- 2. dropout ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(1, 64), (3, 4096), (128, 4096), (5, 13)], ids=lambda s: '%dx%d' % s)
def test_dropout_is_bit_equal_to_the_statement(shape):
    ops = _ops()
    rng = np.random.default_rng(shape[0] * 31 + shape[1])
    x, dy = rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
    tx, tdy = _dev(x), _dev(dy)
    seed, image_id = (7 << 32) | 5, 3
    for stream in (vg.STREAM_DROPOUT_FC1, vg.STREAM_DROPOUT_FC2):
        for kp in (0.5, 0.7, 1.0):
            out = torch.full(shape, float('nan'), device='cuda')
            assert ops.dropout(tx, kp, seed, image_id, stream, out=out) is out
            assert _np_bits_equal(out, vg.dropout(x, kp, seed, image_id, stream)), (shape, stream, kp)
            back = torch.full(shape, float('nan'), device='cuda')
            ops.dropout_backward(tdy, kp, seed, image_id, stream, out=back)
            assert _np_bits_equal(back, vg.dropout_backward(dy, kp, seed, image_id, stream)), (shape, stream, kp)
            # behind autograd: the same two launches
            xg = tx.clone().requires_grad_()
            y = ops.dropout_trainable(xg, kp, seed, image_id, stream)
            y.backward(tdy)
            assert _same_bits(y, out) and _same_bits(xg.grad, back)
    # in place, and the image id taken modulo 2^32
    buf = tx.clone()
    ops.dropout(buf, 0.5, seed, image_id + (1 << 32), 6, out=buf)
    assert _np_bits_equal(buf, vg.dropout(x, 0.5, seed, image_id, 6))


# ---- 3. the convolution with its pooling behind autograd ----------------------------------------------------------------------------------
def _conv_pool_by_hand(x, w, b, dpool, with_dx=True):
    ops = _ops()
    z = ops.conv3x3_f32(x, w)
    dz = ops.relu_maxpool2_backward(z, b, dpool)
    dw, db = ops.conv3x3_wgrad_f32_levels([x], [dz])
    dx = ops.conv3x3_dgrad_f32_levels([dz], w)[0] if with_dx else None
    return z, dz, dw, db, dx


def _conv_pool_case(hw, kind, seed):
    H, W = hw
    rng = np.random.default_rng(seed + H * 10 + W)
    OH, OW = vg.pooled_shape(H, W)
    if kind == 'int':
        f = lambda *s: rng.integers(-3, 4, s).astype(np.float32)
    else:
        f = lambda *s: rng.standard_normal(s).astype(np.float32)
    return f(1, H, W, 64), f(64, 3, 3, 64), f(64), f(1, OH, OW, 64)


@pytest.mark.parametrize('hw', [(5, 7), (6, 6)], ids=_ID)
def test_conv3x3_relu_pool_trainable(hw, monkeypatch):
    from tf_eager_object_detection_amd.model.layers import _conv_relu_pool
    ops = _ops()
    dgrads = []
    dgrad = ops.conv3x3_dgrad_f32_levels
    monkeypatch.setattr(ops, 'conv3x3_dgrad_f32_levels', lambda *a, **k: dgrads.append(1) or dgrad(*a, **k))
    x, w, b, dpool = _conv_pool_case(hw, 'normal', 1)
    conv = torch.nn.Conv2d(64, 64, 3, padding=1).cuda().to(memory_format=torch.channels_last)
    with torch.no_grad():
        conv.weight.copy_(_dev(w).permute(0, 3, 1, 2))
        conv.bias.copy_(_dev(b))
    tx, tg = _dev(x), _dev(dpool)
    with torch.no_grad():
        want = _conv_relu_pool(conv, tx.permute(0, 3, 1, 2), 2, 2, ceil_mode=True).permute(0, 2, 3, 1)
    # an input that requires no gradient: no dgrad launch
    y = ops.conv3x3_relu_pool_trainable(tx, conv.weight, conv.bias)
    assert _same_bits(y, want) and y.requires_grad
    y.backward(tg)
    assert dgrads == []
    z, dz, dw, db, dx = _conv_pool_by_hand(tx, conv.weight.detach(), conv.bias.detach(), tg)
    assert len(dgrads) == 1
    assert conv.weight.grad.shape == conv.weight.shape and conv.weight.grad.stride() == conv.weight.stride()
    assert _same_bits(conv.weight.grad.permute(0, 2, 3, 1), dw) and _same_bits(conv.bias.grad, db)
    # one that does: the forward kernel on the flipped weight, the caller's cached one when given
    for flipped in (None, ops.conv3x3_flipped_weight(conv.weight.detach())):
        conv.zero_grad(set_to_none=True)
        xg = tx.clone().requires_grad_()
        y = ops.conv3x3_relu_pool_trainable(xg, conv.weight, conv.bias, flipped=flipped)
        n = len(dgrads)
        y.backward(tg)
        assert len(dgrads) == n + 1
        assert _same_bits(y, want) and _same_bits(xg.grad, dx) and _same_bits(conv.weight.grad.permute(0, 2, 3, 1), dw)


@pytest.mark.parametrize('hw', [(5, 7), (6, 6)], ids=_ID)
def test_conv3x3_relu_pool_trainable_is_exact_on_integer_data(hw):
    """integers in -3..3 (the data of tests/test_conv_grad_host.py's exact cases): every product and partial sum is an integer far
    below 2^24, so the float32 forward is exact, the pooling picks the same first maximum as float64 torch does, and every gradient
    equals float64 autograd of max_pool2d(relu(conv2d(x, w, b)), 2, 2, ceil_mode=True) by bytes"""
    ops = _ops()
    x, w, b, dpool = _conv_pool_case(hw, 'int', 2)
    assert 9 * 64 * 9 + 3 < 2 ** 24 and hw[0] * hw[1] * 9 < 2 ** 24
    tw = _dev(w).permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last).requires_grad_()
    tb = _dev(b).requires_grad_()
    xg = _dev(x).requires_grad_()
    y = ops.conv3x3_relu_pool_trainable(xg, tw, tb)
    y.backward(_dev(dpool))
    d = lambda a: torch.tensor(a, dtype=torch.float64)
    x64 = d(x).permute(0, 3, 1, 2).contiguous().requires_grad_()
    w64 = d(w).permute(0, 3, 1, 2).contiguous().requires_grad_()
    b64 = d(b).requires_grad_()
    y64 = F.max_pool2d(F.relu(F.conv2d(x64, w64, b64, padding=1)), 2, 2, ceil_mode=True)
    y64.backward(d(dpool).permute(0, 3, 1, 2))
    same = lambda g, r: g.detach().cpu().contiguous().numpy().tobytes() == r.float().contiguous().numpy().tobytes()
    assert torch.equal(y.detach().cpu().double(), y64.detach().permute(0, 2, 3, 1))
    for name, g, r in (('dw', tw.grad.permute(0, 2, 3, 1), w64.grad.permute(0, 2, 3, 1)), ('db', tb.grad, b64.grad),
                       ('dx', xg.grad, x64.grad.permute(0, 2, 3, 1))):
        assert float(r.abs().max()) > 0 and torch.equal(r.float().double(), r), name
        assert same(g, r), (name, float((g.detach().cpu().double() - r).abs().max()))


def _fraction(got, want, bound):
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= bound).all(), 'largest excess %g over a bound of %g' % ((err - bound).max(), bound.flat[(err - bound).argmax()])
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


@pytest.mark.parametrize('hw', [(5, 7), (6, 6)], ids=_ID)
def test_conv3x3_relu_pool_trainable_within_the_summation_bound(hw):
    """normal random data.  The gate is a selection, not arithmetic: with the float32 forward's own winners (the statement on the
    kernel's z) dz is exact, and the layer's gradients are sums of rounded products over it -- the any-order bound of
    tests/test_conv_grad_gpu.py (b): |got - want| <= K * 2^-23 * (|a| . |b|), K = B H W for dw and db, 9 * cout for dx"""
    ops = _ops()
    x, w, b, dpool = _conv_pool_case(hw, 'normal', 3)
    tw = _dev(w).permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last).requires_grad_()
    tb = _dev(b).requires_grad_()
    xg = _dev(x).requires_grad_()
    y = ops.conv3x3_relu_pool_trainable(xg, tw, tb)
    y.backward(_dev(dpool))
    z32 = ops.conv3x3_f32(xg.detach(), tw.detach()).cpu().numpy()
    dz = vg.relu_maxpool2_backward(z32, b, dpool)
    assert (dz != 0).any()
    K, cout = hw[0] * hw[1], 64
    wdw, wdb = cg.wgrad([x], [dz])
    adw, adb = cg.wgrad_abs([x], [dz])
    worst = {'dw': _fraction(tw.grad.permute(0, 2, 3, 1).cpu().numpy(), wdw, K * U * adw),
             'db': _fraction(tb.grad.cpu().numpy(), wdb, K * U * adb),
             'dx': _fraction(xg.grad.cpu().numpy(), cg.dgrad([dz], w)[0], 9 * cout * U * cg.dgrad_abs([dz], w)[0])}
    print('\n%dx%d: worst fraction of the bound  dx %.4f  dw %.4f  db %.4f' % (hw + (worst['dx'], worst['dw'], worst['db'])))


# ---- 4. the detector ------------------------------------------------------------------------------------------------------------------------
IMAGE = (64, 96)
EXTRACTOR_NAMES = tuple('convs.%d.%s' % (i, k) for i in range(4, 13) for k in ('weight', 'bias'))
FROZEN_NAMES = tuple('convs.%d.%s' % (i, k) for i in range(4) for k in ('weight', 'bias'))
RPN_NAMES = ('rpn_conv.weight', 'rpn_conv.bias', 'rpn_score.weight', 'rpn_score.bias', 'rpn_bbox.weight', 'rpn_bbox.bias')
ROI_NAMES = ('fc1.weight', 'fc1.bias', 'fc2.weight', 'fc2.bias', 'score.weight', 'score.bias', 'bbox.weight', 'bbox.bias')


def _image(rng, shape=IMAGE):
    return torch.from_numpy((rng.uniform(0, 255, (1,) + shape + (3,)) - 110).astype(np.float32)).cuda()


@pytest.fixture(scope='module')
def detector():
    from tf_eager_object_detection_amd.model.frcnn_detector import Vgg16Detector
    torch.manual_seed(2)
    det = Vgg16Detector(21, IMAGE, 1, dtype=torch.float32)
    return det.to(device='cuda', dtype=torch.float32, memory_format=torch.channels_last).eval()


def test_detector_trainable_parts(detector):
    det = detector
    assert len(EXTRACTOR_NAMES) == 18 and len(RPN_NAMES) == 6 and len(ROI_NAMES) == 8 and len(FROZEN_NAMES) == 8
    rng = np.random.default_rng(4)
    img = _image(rng)
    feats = torch.from_numpy(rng.standard_normal((8, 7, 7, 512)).astype(np.float32)).cuda()
    with torch.no_grad():
        c0 = det.features(img)
        s0, d0 = det.rpn(c0)
        l0, b0 = det.roi_head(feats)
    c = det.extractor_trainable(img)
    assert _same_bits(c, c0) and c.shape == c0.shape and c.stride() == c0.stride() and c.requires_grad
    assert tuple(c.shape) == (1, 512, 4, 6)
    s, d = det.rpn_trainable(c)
    assert s.shape == s0.shape and d.shape == d0.shape and _same_bits(s, s0) and _same_bits(d, d0)
    logits, bbox = det.roi_head_trainable(feats, keep_prob=1.0, seed=5, image_id=9)
    assert _same_bits(logits, l0) and _same_bits(bbox, b0)
    # dropout at 0.5: the two masks of streams 6 and 7, reproducible, another image id another mask
    l1, _ = det.roi_head_trainable(feats, 0.5, 5, 9)
    l2, _ = det.roi_head_trainable(feats, 0.5, 5, 9)
    l3, _ = det.roi_head_trainable(feats, 0.5, 5, 10)
    assert _same_bits(l1, l2) and not torch.equal(l1, l0) and not torch.equal(l1, l3)
    g = lambda t: torch.from_numpy(rng.standard_normal(tuple(t.shape)).astype(np.float32)).cuda()
    torch.autograd.backward([c, s, d, logits, bbox], [g(c), g(s), g(d), g(logits), g(bbox)])
    params = dict(det.named_parameters())
    assert sorted(n for n, p in params.items() if p.grad is not None) == sorted(EXTRACTOR_NAMES + RPN_NAMES + ROI_NAMES)
    for n in EXTRACTOR_NAMES + RPN_NAMES + ROI_NAMES:
        gr = params[n].grad
        assert gr.shape == params[n].shape and gr.stride() == params[n].stride(), n
        assert bool(torch.isfinite(gr).all()) and float(gr.abs().max()) > 0, n
    for n in FROZEN_NAMES:
        assert params[n].grad is None, n
    det.zero_grad(set_to_none=True)


# ---- 5. the caller model ----------------------------------------------------------------------------------------------------------------------
MODEL_IMAGE = (208, 256)          # (the smallest anchors are 128 pixels: a smaller image holds none, and the RPN losses are 0)
GT_BOXES = [[40.0, 30.0, 170.0, 160.0], [60.0, 50.0, 240.0, 150.0]]


def _model(state=None, **kw):
    from tf_eager_object_detection_amd.model.base_faster_rcnn_model import Vgg16FasterRcnn
    m = Vgg16FasterRcnn(training_targets='hip', training_losses='hip', **kw)
    if state is not None:
        m._dense_ref.load_state_dict(state)
    return m


ALL = dict(train_roi_head=True, train_rpn_head=True, train_extractor=True)


def test_caller_model_trains_32_parameters():
    from tf_eager_object_detection_amd import training
    torch.manual_seed(3)
    plain = _model()
    state = plain._dense_ref.state_dict()
    rng = np.random.default_rng(6)
    img = _image(rng, MODEL_IMAGE)
    gt = torch.tensor(GT_BOXES, device='cuda')
    gl = torch.tensor([3, 12], device='cuda')
    inputs = (img, gt, gl)
    want = plain(inputs, training=True)
    assert len(want) == 4 and not any(x.requires_grad for x in want) and all(float(x) > 0 for x in want)
    # keep rate 1: the four losses of the model without the keywords, bit for bit
    m = _model(state, roi_head_keep_dropout_rate=1.0, **ALL)
    losses = m(inputs, training=True)
    assert all(x.requires_grad for x in losses) and all(_same_bits(a, b) for a, b in zip(losses, want))
    assert all(torch.equal(a, b) for a, b in zip(m.im_detect(img, 1.0), plain.im_detect(img, 1.0)))
    sum(losses).backward()
    det = m.dense
    params = dict(det.named_parameters())
    trained = EXTRACTOR_NAMES + RPN_NAMES + ROI_NAMES
    assert len(trained) == 32
    assert sorted(n for n, p in params.items() if p.grad is not None) == sorted(trained)
    for n in trained:
        g = params[n].grad
        assert g.shape == params[n].shape and g.stride() == params[n].stride(), n
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, n
    assert all(params[n].grad is None for n in FROZEN_NAMES)
    # one training step: the 32 move, their version counters go up, the eight of blocks 1-2 stay
    named = training.model_variables(det)
    before = {n: (p.detach().clone(), p._version) for n, p in named}
    training.train_step(named, [p.grad for _, p in named], training.MomentumOptimizer(0.01, 0.9), learning_rate_bias_double=True,
                        weight_decays=training.l2_variables(det, 0.0001))
    for n, p in named:
        assert torch.equal(p.detach(), before[n][0]) == (n in FROZEN_NAMES), n
        assert (p._version > before[n][1]) == (n not in FROZEN_NAMES), n
    # the next pass runs on the stepped weights (packs and flipped weights rebuilt): same samples, other losses
    m._anchor_target._next_image_id = m._proposal_target._next_image_id = 0
    det.zero_grad(set_to_none=True)
    again = m(inputs, training=True)
    assert not any(torch.equal(a.detach(), b) for a, b in zip(again, want))
    with torch.no_grad():
        c0 = det.features(img)
    assert _same_bits(det.extractor_trainable(img), c0)


def _restart(m, **private):
    """the model as freshly built with other dropout settings: the target layers' and the dropout's image ids back at 0 (building a
    VGG16 model costs seconds; the settings are plain attributes)"""
    m._anchor_target._next_image_id = m._proposal_target._next_image_id = m._next_dropout_image_id = 0
    for k, v in private.items():
        assert hasattr(m, k), k
        setattr(m, k, v)
    m.dense.zero_grad(set_to_none=True)
    return m


def test_caller_model_dropout_seeds():
    """keep rate 0.5 (the default): two models with one dropout_seed agree bit for bit in losses and gradients; another seed is
    another mask; the image id advances with the training calls; inference sees no dropout"""
    torch.manual_seed(3)
    a = _model(dropout_seed=3, **ALL)
    b = _model(a._dense_ref.state_dict(), dropout_seed=3, **ALL)
    rng = np.random.default_rng(6)
    img = _image(rng, MODEL_IMAGE)
    gt = torch.tensor(GT_BOXES, device='cuda')
    inputs = (img, gt, torch.tensor([3, 12], device='cuda'))
    la, lb = a(inputs, training=True), b(inputs, training=True)
    assert all(_same_bits(x, y) for x, y in zip(la, lb))
    sum(la).backward()
    sum(lb).backward()
    pb = dict(b.dense.named_parameters())
    for n, p in a.dense.named_parameters():
        assert (p.grad is None) == (pb[n].grad is None) and (p.grad is None or _same_bits(p.grad, pb[n].grad)), n
    assert a._next_dropout_image_id == 1 and b._dropout_seed == 3 and b._roi_head_keep_dropout_rate == 0.5
    la = [x.detach() for x in la]
    other = [x.detach() for x in _restart(b, _dropout_seed=4)(inputs, training=True)]
    assert all(_same_bits(x, y) for x, y in zip(other[:2], la[:2]))                  # the RPN losses see no dropout
    assert not torch.equal(other[2], la[2])                                         # roi_cls_loss does
    full = [x.detach() for x in _restart(b, _roi_head_keep_dropout_rate=1.0)(inputs, training=True)]
    assert not torch.equal(full[2], la[2]) and not torch.equal(full[2], other[2])
    same = [x.detach() for x in _restart(b, _dropout_seed=3, _roi_head_keep_dropout_rate=0.5)(inputs, training=True)]
    assert all(_same_bits(x, y) for x, y in zip(same, la))
    # the second training call draws the next image id's masks (the same samples, by the target layers' ids set back)
    b._anchor_target._next_image_id = b._proposal_target._next_image_id = 0
    second = b(inputs, training=True)
    assert b._next_dropout_image_id == 2 and not torch.equal(second[2].detach(), la[2])
    assert all(_same_bits(x, y) for x, y in zip(second[:2], la[:2]))
    # inference sees no dropout
    _restart(b, _roi_head_keep_dropout_rate=1.0)
    assert all(torch.equal(x, y) for x, y in zip(a.im_detect(img, 1.0), b.im_detect(img, 1.0)))


def test_caller_model_keyword_rules():
    from tf_eager_object_detection_amd.model.base_faster_rcnn_model import ResNetFasterRcnn, Vgg16FasterRcnn
    with pytest.raises(ValueError, match='train_extractor=True needs train_rpn_head=True or train_roi_head=True'):
        Vgg16FasterRcnn(train_extractor=True)
    with pytest.raises(ValueError, match='train_roi_head=True needs dtype=torch.float32'):
        Vgg16FasterRcnn(train_roi_head=True, dtype=torch.float16)
    with pytest.raises(ValueError, match='train_rpn_head=True needs dtype=torch.float32'):
        Vgg16FasterRcnn(train_rpn_head=True, f32_form='x3')
    with pytest.raises(NotImplementedError, match='ResNetFasterRcnn: train_roi_head'):
        ResNetFasterRcnn(depth=50, train_roi_head=True)
