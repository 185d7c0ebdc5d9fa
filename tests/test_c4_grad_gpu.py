"""The ResNet-C4 training graph on the GPU, narrowest first: odet_global_avg_pool_f32 / odet_global_avg_pool_backward_f32
(csrc/c4_grad.hip) bit-equal to the NumPy statements of tests/c4_grad_np.py; ops.global_avg_pool_trainable behind torch.autograd;
block_trainable on conv5-shaped blocks over a batch of 7 x 7 crops; ResNetC4Detector's three trainable parts against features / rpn /
roi_head; the head's backward against the ops composed by hand; its graph capture; and TrainableResNetFasterRcnn with the three
keywords: losses, gradients, a training step."""
import numpy as np
import pytest
import torch

import c4_grad_np as c4

pytestmark = pytest.mark.gpu

U = 2.0 ** -23
_ID = lambda s: 'x'.join(map(str, s)) if isinstance(s, tuple) else None


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


def _nan(*shape):
    return torch.full(shape, float('nan'), dtype=torch.float32, device='cuda')


def _rand(rng, kind, shape):
    if kind == 'int':
        return rng.integers(-8, 9, shape).astype(np.float32)
    return rng.standard_normal(shape).astype(np.float32)


# ---- 1. the pooling kernels -----------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1, 4), (3, 7, 7, 36), (5, 7, 7, 2048), (2, 8, 8, 256), (130, 3, 5, 64)]


@pytest.mark.parametrize('kind', ['int', 'normal'])
@pytest.mark.parametrize('shape', SHAPES, ids=_ID)
def test_pooling_kernels_are_bit_equal_to_the_statements(shape, kind):
    ops = _ops()
    rng = np.random.default_rng([7, shape[0], shape[1], shape[3], kind == 'int'])
    R, H, W, Cc = shape
    x, g = _rand(rng, kind, shape), _rand(rng, kind, (R, Cc))
    tx, tg = _dev(x), _dev(g)
    out = _nan(R, Cc)
    got = ops.global_avg_pool(tx, out=out)
    assert got is out and _np_bits_equal(out, c4.gap_forward(x))                     # every element written
    assert _same_bits(ops.global_avg_pool(tx), out)                                 # a fresh buffer, whatever it held
    dx = _nan(R, H, W, Cc)
    got = ops.global_avg_pool_backward(tg, (H, W), out=dx)
    assert got is dx and _np_bits_equal(dx, c4.gap_backward(g, (H, W)))
    assert _same_bits(ops.global_avg_pool_backward(tg, (H, W)), dx)


def test_pooling_grid_stride_passes_are_bit_equal_to_the_statements():
    """the launches cap their grid at 64 workgroups per CU, 256 x 64 x 256 = 4,194,304 lanes a pass: a shape whose lanes (forward:
    R C / 4; backward: R ceil(H W / 8) C / 4) exceed a pass in both launches, so that some lanes take a second element"""
    ops = _ops()
    cap = 256 * 64 * 256
    rng = np.random.default_rng(8)
    R, H, W, Cc = 4100, 1, 2, 4096
    assert R * Cc // 4 > cap
    x = rng.standard_normal((R, H, W, Cc)).astype(np.float32)
    out = _nan(R, Cc)
    ops.global_avg_pool(_dev(x), out=out)
    assert _np_bits_equal(out, c4.gap_forward(x))
    del x, out
    g = rng.standard_normal((R, Cc)).astype(np.float32)
    dx = _nan(R, H, W, Cc)
    ops.global_avg_pool_backward(_dev(g), (H, W), out=dx)
    assert _np_bits_equal(dx, c4.gap_backward(g, (H, W)))


def test_pooling_kernel_edges():
    """tests/test_c4_grad_host.py::test_statement_edges on the GPU, and every loop of the forward: 16 + 4 + 1 pixels and more"""
    ops = _ops()
    rng = np.random.default_rng(9)
    x = rng.standard_normal((4, 1, 1, 8)).astype(np.float32)
    x[0, 0, 0, 0], x[1, 0, 0, 1] = -0.0, np.float32(1e-42)
    assert _np_bits_equal(ops.global_avg_pool(_dev(x)), x.reshape(4, 8))             # hw = 1: the input's bits, subnormals kept
    assert _np_bits_equal(ops.global_avg_pool_backward(_dev(x.reshape(4, 8)), (1, 1)), x)
    x = rng.standard_normal((3, 7, 7, 8)).astype(np.float32)
    clean = ops.global_avg_pool(_dev(x)).cpu().numpy()
    bad = x.copy()
    bad[1, 3, 4, 5], bad[2, 6, 6, 0], bad[0, 0, 0, 7] = np.nan, np.inf, -np.inf
    got = ops.global_avg_pool(_dev(bad)).cpu().numpy()
    assert np.isnan(got[1, 5]) and got[2, 0] == np.inf and got[0, 7] == -np.inf
    mask = np.ones(got.shape, bool)
    mask[1, 5] = mask[2, 0] = mask[0, 7] = False
    assert np.array_equal(got[mask].view(np.uint32), clean[mask].view(np.uint32))
    assert np.array_equal(got[mask].view(np.uint32), c4.gap_forward(bad)[mask].view(np.uint32))
    gb = ops.global_avg_pool_backward(_dev(got), (2, 3)).cpu().numpy()
    assert np.isnan(gb[1, :, :, 5]).all() and (gb[2, :, :, 0] == np.inf).all() and np.isfinite(gb[:, :, :, 1:5]).all()
    z = np.full((2, 7, 7, 4), -0.0, dtype=np.float32)
    z[1, 3, 3, 2] = 0.0
    want = np.full((2, 4), -0.0, dtype=np.float32)
    want[1, 2] = 0.0
    assert _np_bits_equal(ops.global_avg_pool(_dev(z)), want)
    assert _np_bits_equal(ops.global_avg_pool_backward(_dev(want), (2, 3)), np.broadcast_to(want[:, None, None, :], (2, 2, 3, 4)))
    # the order: 2^24 first, then ones that are each rounded away; and every pixel count around the loops' depths
    o = np.ones((1, 7, 7, 4), dtype=np.float32)
    o[0, 0, 0, :] = 2.0 ** 24
    assert _np_bits_equal(ops.global_avg_pool(_dev(o)), c4.gap_forward(o))
    assert c4.gap_forward(o)[0, 0] == np.float32(2.0 ** 24) / np.float32(49)
    for hw in (2, 3, 4, 5, 7, 8, 15, 16, 17, 19, 20, 23, 24, 25, 31, 32, 33, 40, 47, 48, 49, 64, 100):
        x = rng.standard_normal((3, 1, hw, 12)).astype(np.float32)
        assert _np_bits_equal(ops.global_avg_pool(_dev(x)), c4.gap_forward(x)), hw
        g = rng.standard_normal((3, 12)).astype(np.float32)
        dx = _nan(3, 1, hw, 12)                                  # (the backward's lanes own 8 pixels each: every remainder)
        ops.global_avg_pool_backward(_dev(g), (1, hw), out=dx)
        assert _np_bits_equal(dx, c4.gap_backward(g, (1, hw))), hw
    with pytest.raises(ValueError, match='out must be'):
        ops.global_avg_pool(_dev(z), out=_nan(2, 8))


# ---- 2. behind autograd ------------------------------------------------------------------------------------------------------------------
def test_global_avg_pool_trainable(monkeypatch):
    ops = _ops()
    rng = np.random.default_rng(10)
    x, g = _dev(rng.standard_normal((6, 7, 7, 64))), _dev(rng.standard_normal((6, 64)))
    calls = []
    backward = ops.global_avg_pool_backward
    monkeypatch.setattr(ops, 'global_avg_pool_backward', lambda *a, **k: calls.append(1) or backward(*a, **k))
    xg = x.clone().requires_grad_()
    y = ops.global_avg_pool_trainable(xg)
    assert y.requires_grad and _same_bits(y, ops.global_avg_pool(x))
    y.backward(g)
    assert len(calls) == 1 and xg.grad.shape == x.shape and xg.grad.is_contiguous()
    assert xg.grad.cpu().numpy().tobytes() == backward(g, (7, 7)).cpu().numpy().tobytes()
    # an input that needs no gradient: no graph through the pooling, no backward launch
    del calls[:]
    y = ops.global_avg_pool_trainable(x)
    assert not y.requires_grad and _same_bits(y, ops.global_avg_pool(x))
    w = torch.ones(64, device='cuda', requires_grad=True)
    (y * w).backward(g)
    assert not calls and w.grad is not None
    # integers and hw = 64: exact against float64 autograd of the mean
    xi, gi = rng.integers(-8, 9, (3, 8, 8, 16)).astype(np.float32), rng.integers(-8, 9, (3, 16)).astype(np.float32)
    xg = _dev(xi).requires_grad_()
    y = ops.global_avg_pool_trainable(xg)
    y.backward(_dev(gi))
    x64 = torch.tensor(xi, dtype=torch.float64, requires_grad=True)
    y64 = x64.mean(dim=(1, 2))
    y64.backward(torch.tensor(gi, dtype=torch.float64))
    assert torch.equal(y.detach().cpu().double(), y64.detach()) and torch.equal(x64.grad.float().double(), x64.grad)
    assert xg.grad.cpu().numpy().tobytes() == x64.grad.float().numpy().tobytes() and len(calls) == 1


# ---- 3. conv5-shaped blocks on a batch of crops ---------------------------------------------------------------------------------------
IMAGE = (64, 96)
CROPS = 8


@pytest.fixture(scope='module')
def detector():
    from tf_eager_object_detection_amd.model.frcnn_detector import ResNetC4Detector
    torch.manual_seed(2)
    det = ResNetC4Detector(50, 21, IMAGE, 1, dtype=torch.float32)
    det = det.to(device='cuda', dtype=torch.float32, memory_format=torch.channels_last).eval()
    with torch.no_grad():                                   # (non-zero biases: the reference's folded batch-norm has them)
        for n, p in det.named_parameters():
            if p.dim() == 1 and n.startswith('conv5'):
                p.add_(torch.linspace(-0.3, 0.3, p.numel(), device='cuda'))
    return det


@pytest.mark.parametrize('index', [0, 1])
def test_conv5_blocks_on_a_batch_of_crops(detector, index):
    """conv5[0] (1024 -> 512 -> 2048, stride 1, convolutional shortcut) and conv5[1] (identity) on [5,7,7,C]: the forward
    bit-equal to the block, every gradient bit-equal to the ops composed by hand (tests/test_block_grad_gpu.py's composition)"""
    from test_block_grad_gpu import _manual_block_grads, _run_block
    blk = detector.conv5[index]
    assert (blk.short is not None) == (index == 0) and blk.c1.stride[0] == 1
    assert (blk.c1.in_channels, blk.c2.in_channels, blk.c3.out_channels) == ((1024, 2048)[index], 512, 2048)
    rng = np.random.default_rng([11, index])
    x = _dev(rng.standard_normal((5, 7, 7, blk.c1.in_channels))).permute(0, 3, 1, 2)
    dy = _dev(rng.standard_normal((5, 7, 7, 2048))).permute(0, 3, 1, 2)
    manual, dx, _ = _manual_block_grads(blk, x, dy, True)
    params = dict(blk.named_parameters())
    assert len(params) == len(manual) == (8, 6)[index]
    for with_dx in (True, False):
        xin, _ = _run_block(blk, x, dy, with_dx)
        for n, p in params.items():
            assert p.grad is not None and p.grad.shape == p.shape and p.grad.stride() == p.stride(), n
            assert _same_bits(p.grad, manual[n]) and float(p.grad.abs().max()) > 0, (n, with_dx)
        assert (xin.grad is not None) == with_dx and (not with_dx or _same_bits(xin.grad, dx))
    blk.zero_grad(set_to_none=True)


# ---- 4. the detector's parts ----------------------------------------------------------------------------------------------------------------
def _image(rng, shape=IMAGE):
    return torch.from_numpy((rng.uniform(0, 255, (1,) + shape + (3,)) - 110).astype(np.float32)).cuda()


def _names(det, **parts):
    from tf_eager_object_detection_amd.model import c4_trainable
    return c4_trainable.trained_names(det, **parts), c4_trainable.frozen_names(det)


def _crops(rng, n=CROPS):
    return torch.from_numpy(np.maximum(rng.standard_normal((n, 7, 7, 1024)), 0).astype(np.float32)).cuda()


def test_detector_trainable_parts(detector):
    from tf_eager_object_detection_amd.model import c4_trainable
    det = detector
    det.zero_grad(set_to_none=True)
    trained, frozen = _names(det)
    assert len(trained) == 94 and len(frozen) == 22
    rng = np.random.default_rng(4)
    img = _image(rng)
    feats = _crops(rng)
    with torch.no_grad():
        c0 = det.features(img)
        s0, d0 = det.rpn(c0)
        l0, b0 = det.roi_head(feats)
        map0 = det.conv5(feats.permute(0, 3, 1, 2))
    c = det.extractor_trainable(img)
    assert _same_bits(c, c0) and c.shape == c0.shape and c.stride() == c0.stride() and c.requires_grad
    assert tuple(c.shape) == (1, 1024, 4, 6)
    s, d = det.rpn_trainable(c)
    assert s.shape == s0.shape and d.shape == d0.shape and _same_bits(s, s0) and _same_bits(d, d0)
    # the head: conv5's map by bits, the pooled activation by the statement, the outputs within the pooling's rounding
    hmap = c4_trainable.head_map_trainable(det, feats)
    assert hmap.shape == map0.shape and hmap.stride() == map0.stride() and _same_bits(hmap, map0)
    map_np = map0.permute(0, 2, 3, 1).contiguous().cpu().numpy()
    pooled = c4_trainable.head_activation_trainable(det, feats)
    assert _np_bits_equal(pooled, c4.gap_forward(map_np))
    logits, bbox = det.roi_head_trainable(feats)
    assert logits.shape == l0.shape == (CROPS, 21) and bbox.shape == b0.shape == (CROPS, 84) and logits.requires_grad
    # |difference| <= (K + 64) * 2^-23 * (|W| . a + |b|): two float32 chains of K = 2048 products on two pooled values that are
    # each within 52 units of 2^-24 of a, the float64 mean of the (non-negative) conv5 map
    wpad, bpad = det._final_layer()
    a = map_np.astype(np.float64).reshape(CROPS, 49, 2048).mean(axis=1)
    assert (a >= 0).all() and float(a.max()) > 0
    bound = (2048 + 64) * U * (a @ np.abs(wpad.double().cpu().numpy()).T + np.abs(bpad.double().cpu().numpy()))
    worst = 0.0
    for got, want, lo in ((logits, l0, 0), (bbox, b0, 21)):
        err = np.abs(got.detach().double().cpu().numpy() - want.double().cpu().numpy())
        bnd = bound[:, lo:lo + err.shape[1]]
        worst = max(worst, float((err / bnd).max()))
        assert (err <= bnd).all(), 'largest excess %g' % float((err - bnd).max())
    print('\nroi_head_trainable against roi_head: worst fraction of the bound %.4f' % worst)
    g = lambda t: torch.from_numpy(rng.standard_normal(tuple(t.shape)).astype(np.float32)).cuda()
    torch.autograd.backward([c, s, d, logits, bbox], [g(c), g(s), g(d), g(logits), g(bbox)])
    params = dict(det.named_parameters())
    assert sorted(n for n, p in params.items() if p.grad is not None) == sorted(trained)
    for n in trained:
        gr = params[n].grad
        assert gr.shape == params[n].shape and gr.stride() == params[n].stride(), n
        assert bool(torch.isfinite(gr).all()) and float(gr.abs().max()) > 0, n
    for n in frozen:
        assert params[n].grad is None, n
    det.zero_grad(set_to_none=True)


# ---- 5. the head's backward by hand ---------------------------------------------------------------------------------------------------------
def test_roi_head_backward_is_bit_equal_to_the_ops_by_hand(detector):
    """the final pair's Dense backward on the padded weights, global_avg_pool_backward, then the three blocks in reverse"""
    from test_block_grad_gpu import _manual_block_grads
    from tf_eager_object_detection_amd.model import c4_trainable
    ops = _ops()
    det = detector
    det.zero_grad(set_to_none=True)
    rng = np.random.default_rng(12)
    feats = _crops(rng).requires_grad_()
    logits, bbox = det.roi_head_trainable(feats)
    d_logits = _dev(rng.standard_normal(tuple(logits.shape)))
    d_bbox = _dev(rng.standard_normal(tuple(bbox.shape)))
    torch.autograd.backward([logits, bbox], [d_logits, d_bbox])
    params = dict(det.named_parameters())
    head, _ = _names(det, rpn_head=False, extractor=False)
    assert len(head) == 24 and sorted(n for n, p in params.items() if p.grad is not None) == sorted(head)
    with torch.no_grad():
        x = feats.detach().permute(0, 3, 1, 2)
        inputs = [x]
        for blk in det.conv5:
            inputs.append(blk(inputs[-1]))
        pooled = ops.global_avg_pool(inputs[-1].permute(0, 2, 3, 1).contiguous())
        wpad, _ = det._final_layer()
        dy = torch.zeros((CROPS, int(wpad.shape[0])), device='cuda')
        dy[:, :21] = d_logits
        dy[:, 21:105] = d_bbox
        dw, db = ops.dense_wgrad(dy, pooled)
        want = {'score.weight': dw[:21], 'score.bias': db[:21], 'bbox.weight': dw[21:105], 'bbox.bias': db[21:105]}
        d = ops.global_avg_pool_backward(ops.dense_dgrad(dy, wpad), (7, 7)).permute(0, 3, 1, 2)
        for i in (2, 1, 0):
            manual, d, _ = _manual_block_grads(det.conv5[i], inputs[i], d, True)
            want.update(('conv5.%d.%s' % (i, n), gr) for n, gr in manual.items())
    assert sorted(want) == sorted(head)
    for n in head:
        assert params[n].grad.shape == params[n].shape and _same_bits(params[n].grad, want[n]), n
    assert feats.grad.shape == feats.shape and _same_bits(feats.grad, d.permute(0, 2, 3, 1))
    assert float(feats.grad.abs().max()) > 0
    det.zero_grad(set_to_none=True)


# ---- 6. graph capture -----------------------------------------------------------------------------------------------------------------------
def test_roi_head_graph_capture_replays_bit_equal_to_eager(detector):
    """the head's forward and backward -- three blocks, the pooling, the final pair, and back -- captured on one stream (one chain,
    no parallel branches) and replayed on new contents"""
    det = detector
    det.zero_grad(set_to_none=True)
    rng = np.random.default_rng(13)
    head, _ = _names(det, rpn_head=False, extractor=False)
    params = [dict(det.named_parameters())[n] for n in head]
    feats = _crops(rng).requires_grad_()
    d_out = [_dev(rng.standard_normal((CROPS, 21))), _dev(rng.standard_normal((CROPS, 84)))]
    run = lambda: torch.autograd.grad(det.roi_head_trainable(feats), params + [feats], d_out)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                   # (the kernels' one-time device set-up and the flipped weights: outside)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            got = run()
    torch.cuda.current_stream().wait_stream(side)
    with torch.no_grad():
        feats.copy_(_crops(rng))
        d_out[0].copy_(_dev(rng.standard_normal((CROPS, 21))))
        d_out[1].copy_(_dev(rng.standard_normal((CROPS, 84))))
    graph.replay()
    torch.cuda.synchronize()
    want = run()
    assert len(got) == 25 and all(_same_bits(a, b) for a, b in zip(got, want))
    assert all(float(g.abs().max()) > 0 for g in want)


# ---- 7. the caller object -------------------------------------------------------------------------------------------------------------------
MODEL_IMAGE = (208, 256)          # (the smallest anchors are 128 pixels: a smaller image holds none, and the RPN losses are 0)
GT_BOXES = [[40.0, 30.0, 170.0, 160.0], [60.0, 50.0, 240.0, 150.0]]
ALL = dict(train_roi_head=True, train_rpn_head=True, train_extractor=True)


@pytest.fixture(scope='module')
def models():
    """the plain model, its state, and the trainable models built on that state, each built once"""
    from tf_eager_object_detection_amd.model.base_faster_rcnn_model import ResNetFasterRcnn, TrainableResNetFasterRcnn
    kw = dict(depth=50, roi_pooling_max_pooling_flag=False, training_targets='hip', training_losses='hip')
    torch.manual_seed(3)
    plain = ResNetFasterRcnn(**kw)
    state = {k: v.clone() for k, v in plain._dense_ref.state_dict().items()}
    made = {'plain': plain}

    def get(name, **flags):
        if name not in made:
            m = TrainableResNetFasterRcnn(**dict(kw, **flags))
            m._dense_ref.load_state_dict(state)
            made[name] = m
        return made[name]
    return get


def _inputs():
    rng = np.random.default_rng(6)
    img = _image(rng, MODEL_IMAGE)
    return img, torch.tensor(GT_BOXES, device='cuda'), torch.tensor([3, 12], device='cuda')


def _fresh(m):
    """the model as freshly built: the target layers' image ids back at 0, no gradients"""
    m._anchor_target._next_image_id = m._proposal_target._next_image_id = 0
    m.dense.zero_grad(set_to_none=True)
    return m


def _check_grads(det, trained):
    params = dict(det.named_parameters())
    assert sorted(n for n, p in params.items() if p.grad is not None) == sorted(trained)
    for n in trained:
        g = params[n].grad
        assert g.shape == params[n].shape and g.stride() == params[n].stride(), n
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, n


def test_caller_model_with_the_keywords_off_is_the_plain_model(models):
    inputs = _inputs()
    plain, off = _fresh(models('plain')), _fresh(models('off'))
    want = plain(inputs, training=True)
    got = off(inputs, training=True)
    assert len(want) == 4 and not any(x.requires_grad for x in want + got) and all(float(x) > 0 for x in want)
    assert all(_same_bits(a, b) for a, b in zip(got, want))
    assert all(torch.equal(a, b) for a, b in zip(off.im_detect(inputs[0], 1.0), plain.im_detect(inputs[0], 1.0)))
    assert all(torch.equal(a, b) for a, b in zip(off(inputs[0], training=False), plain(inputs[0], training=False)))


def test_caller_model_trains_94_parameters(models):
    from tf_eager_object_detection_amd import training
    inputs = _inputs()
    img = inputs[0]
    plain = _fresh(models('plain'))
    want = [x.detach() for x in plain(inputs, training=True)]
    m = _fresh(models('all', **ALL))
    det = m.dense
    trained, frozen = _names(det)
    assert len(trained) == 94 and len(frozen) == 22 and len(list(det.parameters())) == 116
    losses = m(inputs, training=True)
    assert all(x.requires_grad for x in losses)
    assert _same_bits(losses[0], want[0]) and _same_bits(losses[1], want[1])               # the RPN losses: the plain model's bits
    # (the RoI losses go through the trainable head's pooling: the plain model's to the pooling's rounding, bounded in part 4)
    assert all(bool(torch.isfinite(x)) and float(x.detach()) > 0 for x in losses[2:])
    print('\nRoI losses: trainable %r, plain %r' % ([float(x.detach()) for x in losses[2:]], [float(x) for x in want[2:]]))
    assert all(torch.equal(a, b) for a, b in zip(m.im_detect(img, 1.0), plain.im_detect(img, 1.0)))
    assert all(torch.equal(a, b) for a, b in zip(m(img, training=False), plain(img, training=False)))
    sum(losses).backward()
    _check_grads(det, trained)
    params = dict(det.named_parameters())
    assert all(params[n].grad is None for n in frozen)
    # a second model on the same state: the same losses and the same 94 gradients, bit for bit
    m2 = _fresh(models('all2', **ALL))
    losses2 = m2(inputs, training=True)
    assert all(_same_bits(a, b) for a, b in zip(losses2, losses))
    sum(losses2).backward()
    p2 = dict(m2.dense.named_parameters())
    for n, p in params.items():
        assert (p.grad is None) == (p2[n].grad is None) and (p.grad is None or _same_bits(p.grad, p2[n].grad)), n
    # one training step on the second model: the 94 move, their version counters go up, the 22 of conv1 and conv2 stay
    det2 = m2.dense
    named = training.model_variables(det2)
    before = {n: (p.detach().clone(), p._version) for n, p in named}
    training.train_step(named, [p.grad for _, p in named], training.MomentumOptimizer(0.01, 0.9), learning_rate_bias_double=True,
                        weight_decays=training.l2_variables(det2, 0.0001))
    assert len(named) == 116
    for n, p in named:
        assert torch.equal(p.detach(), before[n][0]) == (n in frozen), n
        assert (p._version > before[n][1]) == (n not in frozen), n
    # the next pass runs on the stepped weights (packs and flipped weights rebuilt): same samples, other losses
    _fresh(m2)
    again = m2(inputs, training=True)
    assert not any(torch.equal(a.detach(), b.detach()) for a, b in zip(again, losses))
    with torch.no_grad():
        c0 = det2.features(img)
    c = det2.extractor_trainable(img)
    assert _same_bits(c, c0) and c.stride() == c0.stride()
    det.zero_grad(set_to_none=True)
    det2.zero_grad(set_to_none=True)


def test_caller_model_partial_keywords(models):
    inputs = _inputs()
    plain = _fresh(models('plain'))
    want = [x.detach() for x in plain(inputs, training=True)]
    # the RoI head alone: conv5 + score + bbox, 24 parameters, and nothing else
    m = _fresh(models('head', train_roi_head=True))
    head, _ = _names(m.dense, rpn_head=False, extractor=False)
    losses = m(inputs, training=True)
    assert [x.requires_grad for x in losses] == [False, False, True, True]
    assert _same_bits(losses[0], want[0]) and _same_bits(losses[1], want[1])
    sum(losses[2:]).backward()
    assert len(head) == 24
    _check_grads(m.dense, head)
    m.dense.zero_grad(set_to_none=True)
    # extractor + RoI head, no RPN keyword: conv3 is reached through the crop backward alone
    m = _fresh(models('extractor_head', train_roi_head=True, train_extractor=True))
    names, _ = _names(m.dense, rpn_head=False)
    losses = m(inputs, training=True)
    assert [x.requires_grad for x in losses] == [False, False, True, True]
    assert _same_bits(losses[0], want[0]) and _same_bits(losses[1], want[1])
    sum(losses[2:]).backward()
    assert len(names) == 88 and any(n.startswith('conv3.0.') for n in names)
    _check_grads(m.dense, names)
    m.dense.zero_grad(set_to_none=True)
