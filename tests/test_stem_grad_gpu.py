"""The FPN stem's backward on the GPU: odet_relu_maxpool3_backward_f32 (csrc/stem_grad.hip) bit-equal to the serial NumPy statement
of tests/stem_grad_np.py on every shape, data set and edge of its arrangement; ops.stem_trainable behind torch.autograd (forward =
the detectors' float32 stem, gradients exact on integer data and within the project's summation bounds on random data, under both
grad forms); ResnetV1Fpn with train_stem: 134 trained parameters, the other 132 and the losses bit-equal to the model without it, one
training step; and one graph capture of the stem's forward and backward."""
import ctypes as C

import numpy as np
import pytest
import torch

import stem_grad_np as sg

pytestmark = pytest.mark.gpu

U = 2.0 ** -23
_ID = lambda s: 'x'.join(str(v) for v in s)


def _ops():
    from tf_eager_object_detection_amd import ops
    return ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _np_bits_equal(got, want):
    got = got.detach().contiguous().cpu().numpy()
    return got.shape == want.shape and got.tobytes() == np.ascontiguousarray(want, np.float32).tobytes()


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.detach().contiguous().view(torch.int32), b.detach().contiguous().view(torch.int32))


# ---- 1. the pooling backward ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', sg.KINDS)
@pytest.mark.parametrize('shape', sg.SHAPES + sg.EDGE_SHAPES, ids=_ID)
def test_relu_maxpool3_backward_is_bit_equal_to_the_statement(shape, kind):
    """sg.SHAPES: the issue's odd and even sizes; sg.EDGE_SHAPES: one shape across each band (6 window rows), strip (15 / 255 / 3 / 85
    window columns by C) and channel-chunk (64 vectors) edge of the kernel, named there.  'order': a wrong order of a pixel's up to
    four terms changes the float32 bits (tests/test_stem_grad_host.py shows it does)."""
    ops = _ops()
    z, bias, dpool = sg.pool_case(kind, shape)
    want = sg.relu_maxpool3_backward_np(z, bias, dpool)
    tz, tb, tg = _dev(z), _dev(bias), _dev(dpool)
    out = torch.full(shape, float('nan'), device='cuda')                       # every element must be written
    got = ops.relu_maxpool3_backward(tz, tb, tg, out=out)
    assert got is out and _np_bits_equal(out, want), (shape, kind)
    assert _same_bits(ops.relu_maxpool3_backward(tz, tb, tg), out)            # a fresh buffer, whatever it held
    # the forward the statement is the backward of: what odet_bias_relu_maxpool writes
    assert _np_bits_equal(ops.bias_relu_maxpool(tz, tb, 3, 2, 1, False), sg.relu_maxpool3_forward_np(z, bias))


def test_a_nan_takes_no_gradient():
    ops = _ops()
    z, bias, dpool = sg.pool_case('normal', (1, 7, 9, 64))
    z[0, 3, 3, :] = np.nan
    z[0, 0, 0, 5] = np.nan
    want = sg.relu_maxpool3_backward_np(z, bias, dpool)
    got = ops.relu_maxpool3_backward(_dev(z), _dev(bias), _dev(dpool))
    assert _np_bits_equal(got, want)
    assert bool((got[0, 3, 3] == 0).all()) and float(got[0, 0, 0, 5]) == 0 and bool(torch.isfinite(got).all())


def test_ties_and_partial_winners():
    """(a) window (0,0) of a 4 x 4 map holds its maximum at (0,0) and at (1,1), which windows (0,1), (1,0), (1,1) share: the first
    tap in row-major order takes window (0,0)'s gradient, (1,1) the other three in ascending window order.  (b) (1,1) is the maximum
    of windows (0,0) and (0,1) but not of (1,0) and (1,1), where (3,1) beats it.  (c) a single -0 term stays -0."""
    ops = _ops()
    bias = torch.zeros(4, device='cuda')
    dpool = np.zeros((1, 2, 2, 4), np.float32)
    dpool[0, :, :, 0] = [[1.0, 10.0], [100.0, 1000.0]]
    z = np.zeros((1, 4, 4, 4), np.float32)
    z[0, 0, 0, 0] = z[0, 1, 1, 0] = 2.0
    dz = ops.relu_maxpool3_backward(_dev(z), bias, _dev(dpool)).cpu().numpy()
    assert dz[0, 0, 0, 0] == 1.0 and dz[0, 1, 1, 0] == 1110.0 and np.count_nonzero(dz) == 2
    z = np.zeros((1, 4, 4, 4), np.float32)
    z[0, 1, 1, 0], z[0, 3, 1, 0] = 2.0, 3.0
    dz = ops.relu_maxpool3_backward(_dev(z), bias, _dev(dpool)).cpu().numpy()
    assert dz[0, 1, 1, 0] == 11.0 and dz[0, 3, 1, 0] == 1100.0 and np.count_nonzero(dz) == 2
    dz = ops.relu_maxpool3_backward(torch.ones(1, 1, 1, 4, device='cuda'), bias, torch.full((1, 1, 1, 4), -0.0, device='cuda'))
    assert bool(torch.signbit(dz).all())


def test_argument_errors():
    ops = _ops()
    z, b, g = (torch.zeros(s, device='cuda') for s in ((1, 5, 4, 8), (8,), (1, 3, 2, 8)))
    with pytest.raises(ValueError, match=r'dpool \(1, 2, 2, 8\) does not go with z \(1, 5, 4, 8\) \(the pooled map is \(1, 3, 2, 8\)\)'):
        ops.relu_maxpool3_backward(z, b, g[:, :2].contiguous())
    with pytest.raises(ValueError, match='C a positive multiple of 4'):
        ops.relu_maxpool3_backward(z[..., :6].contiguous(), b[:6].contiguous(), g[..., :6].contiguous())
    with pytest.raises(ValueError, match='z must be a float32 tensor'):
        ops.relu_maxpool3_backward(z.half(), b, g)
    with pytest.raises(ValueError, match='dpool must be contiguous'):
        ops.relu_maxpool3_backward(z, b, g.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3))
    with pytest.raises(ValueError, match='bias must be a GPU tensor'):
        ops.relu_maxpool3_backward(z, b.cpu(), g)
    # the C ABI: a null pointer is refused on the host, nothing is launched
    L = ops.L.lib()
    rc = L.odet_relu_maxpool3_backward_f32(C.c_void_p(z.data_ptr()), None, C.c_void_p(g.data_ptr()), C.c_void_p(z.data_ptr()),
                                           1, 5, 4, 8, None)
    assert rc == -1 and L.odet_last_error().startswith(b'odet_relu_maxpool3_backward_f32: null pointer')


# ---- 2. ops.stem_trainable ------------------------------------------------------------------------------------------------------------
def _conv1(w, b):
    """a conv1 layer as the detectors hold it (channels_last) with weight ``w`` [64,7,7,3] and bias ``b``"""
    conv = torch.nn.Conv2d(3, 64, 7, stride=2, padding=3).cuda().to(memory_format=torch.channels_last)
    with torch.no_grad():
        conv.weight.copy_(_dev(w).permute(0, 3, 1, 2))
        conv.bias.copy_(_dev(b))
    return conv


def _stem_case(kind, hw, seed):
    H, W = hw
    rng = np.random.default_rng(seed + 100 * H + W)
    Ho, Wo = sg.pooled_shape(H, W)
    Hp, Wp = sg.pooled_shape(Ho, Wo)
    f = (lambda *s: rng.integers(-3, 4, s).astype(np.float32)) if kind == 'int' else (lambda *s: rng.standard_normal(s).astype(np.float32))
    return f(1, H, W, 3), f(64, 7, 7, 3), f(64), f(1, Hp, Wp, 64)


def _by_hand(img, conv, dpool):
    """the launches of the stem's forward and backward, one by one -> (z, dz, dw [64,7,7,3], db)"""
    ops = _ops()
    patches = ops.stem_patches_f32(img)
    z = ops.pointwise(patches, ops.patch_weight(conv.weight.detach(), 160), None, None, False)
    dz = ops.relu_maxpool3_backward(z, conv.bias.detach(), dpool)
    dw160, db = ops.dense_wgrad(dz.view(-1, 64), patches.view(-1, 160))
    assert float(dw160[:, 147:].abs().max()) == 0
    return z, dz, dw160[:, :147].reshape(64, 7, 7, 3), db


@pytest.mark.parametrize('form', ['exact', 'x3'])
def test_stem_trainable_forward_is_the_stem_and_gradients_are_the_ops_by_hand(form):
    from tf_eager_object_detection_amd.model.layers import _stem
    ops = _ops()
    img, w, b, dpool = _stem_case('normal', (37, 45), 1)
    conv = _conv1(w, b)
    timg, tg = _dev(img), _dev(dpool)
    with torch.no_grad():
        want = _stem(conv, timg, torch.float32)
    with ops.grad_form(form):
        y = ops.stem_trainable(timg, conv.weight, conv.bias).permute(0, 3, 1, 2)
        assert y.requires_grad and y.shape == want.shape and y.stride() == want.stride() and _same_bits(y, want)
        y.backward(tg.permute(0, 3, 1, 2))                                     # (backward re-enters the form the forward recorded)
        z, dz, dw, db = _by_hand(timg, conv, tg)
    gw, gb = conv.weight.grad, conv.bias.grad
    assert gw.shape == conv.weight.shape and gw.stride() == conv.weight.stride() and gb.shape == (64,)
    assert _same_bits(gw.permute(0, 2, 3, 1), dw) and _same_bits(gb, db)       # db: dense_wgrad's own
    assert _np_bits_equal(dz, sg.relu_maxpool3_backward_np(z.cpu().numpy(), b, dpool))
    # a second call, and one on the caller's cached patch weight and a plain-format parameter: the same bits
    conv.zero_grad(set_to_none=True)
    plain_w = conv.weight.detach().contiguous().requires_grad_()
    assert plain_w.stride() != conv.weight.stride()
    with ops.grad_form(form):
        ops.stem_trainable(timg, conv.weight, conv.bias).backward(tg)
        ops.stem_trainable(timg, plain_w, conv.bias, stem_weight=ops.patch_weight(plain_w.detach(), 160)).backward(tg)
    assert _same_bits(conv.weight.grad, gw) and plain_w.grad.stride() == plain_w.stride() and _same_bits(plain_w.grad, gw)
    # no graph under no_grad; the image gets no gradient
    with torch.no_grad():
        assert not ops.stem_trainable(timg, conv.weight, conv.bias).requires_grad
    ximg = timg.clone().requires_grad_()
    ops.stem_trainable(ximg, conv.weight, conv.bias).backward(tg)
    assert ximg.grad is None


@pytest.mark.parametrize('form', ['exact', 'x3'])
def test_stem_trainable_is_exact_on_integer_data(form):
    """integers in -3..3 on a 17 x 21 image: every product and partial sum of the forward and of the gradients is an integer far
    below 2^24 (and every operand is exact in one bfloat16 limb), so dw and db equal the float64 statement by bytes"""
    ops = _ops()
    img, w, b, dpool = _stem_case('int', (17, 21), 2)
    assert 147 * 9 + 3 < 2 ** 24 and 9 * 11 * 12 * 3 < 2 ** 24
    conv = _conv1(w, b)
    with ops.grad_form(form):
        y = ops.stem_trainable(_dev(img), conv.weight, conv.bias)
        y.backward(_dev(dpool))
    z64 = sg.stem_conv_np(img, w)
    assert np.array_equal(y.detach().cpu().numpy().astype(np.float64), sg.relu_maxpool3_forward_np(z64, b))
    dz = sg.relu_maxpool3_backward_np(z64.astype(np.float32), b, dpool)
    dw64, db64 = sg.stem_wgrad_np(img, dz)
    assert np.abs(dw64).max() > 0 and np.abs(db64).max() > 0
    assert conv.weight.grad.permute(0, 2, 3, 1).contiguous().cpu().numpy().tobytes() == dw64.astype(np.float32).tobytes()
    assert conv.bias.grad.cpu().numpy().tobytes() == db64.astype(np.float32).tobytes()


@pytest.mark.parametrize('form', ['exact', 'x3'])
def test_stem_trainable_within_the_summation_bound(form):
    """normal data.  The gate is a selection: with the float32 forward's own winners (the statement on the kernel's z) dz is exact,
    and dw is a sum of K = Ho Wo rounded products over it -- 'exact': DESIGN 3.15 (b)'s any-order bound K 2^-23 (|a| . |b|); 'x3':
    3.21's (6 K + 1) 2^-23 (|a| . |b|)"""
    ops = _ops()
    img, w, b, dpool = _stem_case('normal', (37, 45), 3)
    conv = _conv1(w, b)
    timg = _dev(img)
    with ops.grad_form(form):
        ops.stem_trainable(timg, conv.weight, conv.bias).backward(_dev(dpool))
    z32 = ops.pointwise(ops.stem_patches_f32(timg), ops.patch_weight(conv.weight.detach(), 160), None, None, False).cpu().numpy()
    dz = sg.relu_maxpool3_backward_np(z32, b, dpool)
    assert (dz != 0).any()
    K = dz.shape[1] * dz.shape[2]
    dw64, db64 = sg.stem_wgrad_np(img, dz)
    adw, adb = sg.stem_wgrad_np(img, dz, absolute=True)
    factor = K if form == 'exact' else 6 * K + 1
    err = np.abs(conv.weight.grad.permute(0, 2, 3, 1).cpu().numpy().astype(np.float64) - dw64)
    print('\n%s: dw worst fraction of the bound %.4f' % (form, float((err / (factor * U * adw)).max())))
    assert (err <= factor * U * adw).all()
    assert (np.abs(conv.bias.grad.cpu().numpy().astype(np.float64) - db64) <= K * U * adb).all()


def test_stem_trainable_graph_capture_replays_bit_equal_to_eager():
    """the stem's forward and backward -- patches, GEMM, pooling, then the pooling backward, the patches again, the weight gradient
    with its reduce -- captured on one stream (one chain) and replayed on new contents"""
    ops = _ops()
    img, w, b, dpool = _stem_case('normal', (37, 45), 4)
    conv = _conv1(w, b)
    timg, tg = _dev(img), _dev(dpool)
    run = lambda: torch.autograd.grad(ops.stem_trainable(timg, conv.weight, conv.bias), [conv.weight, conv.bias], tg)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                   # (the kernels' one-time device set-up and the workspace: outside)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            got = run()
    torch.cuda.current_stream().wait_stream(side)
    img2, _, _, dpool2 = _stem_case('normal', (37, 45), 5)
    timg.copy_(_dev(img2))
    tg.copy_(_dev(dpool2))
    graph.replay()
    torch.cuda.synchronize()
    want = run()
    assert len(got) == 2 and all(_same_bits(a, c) for a, c in zip(got, want))
    assert all(float(g.abs().max()) > 0 for g in want)


# ---- 3. the caller model ------------------------------------------------------------------------------------------------------------------
IMAGE = (256, 352)                                                        # (tests/test_block_grad_gpu.py's model tests)
FOUR = dict(train_extractor=True, train_neck=True, train_rpn_head=True, train_roi_head=True)


@pytest.fixture(scope='module')
def models():
    """the model with the five keywords, a twin on the same state, the model without train_stem on the same state, and the image
    and ground truth of tests/test_block_grad_gpu.py's model tests (three of the random model's own proposals)"""
    from tf_eager_object_detection_amd.model.base_fpn_model import ResnetV1Fpn
    kw = dict(depth=50, training_targets='hip', training_losses='hip', roi_training_total_num_samples=32, roi_training_max_pos_samples=8,
              **FOUR)
    torch.manual_seed(1)
    m = ResnetV1Fpn(train_stem=True, **kw)
    with torch.no_grad():                                   # (spreads the fresh RpnHead's proposals over sizes and pyramid levels)
        b = m.dense.rpn_bbox.bias
        b.add_(torch.linspace(0.0, 1.6, b.numel(), device=b.device, dtype=b.dtype))
    twin, plain = ResnetV1Fpn(train_stem=True, **kw), ResnetV1Fpn(**kw)
    for other in (twin, plain):
        other._dense_ref.load_state_dict(m._dense_ref.state_dict())
    rng = np.random.default_rng(1)
    img = torch.from_numpy((rng.uniform(0, 255, (1,) + IMAGE + (3,)) - 110).astype(np.float32)).cuda()
    with torch.no_grad():
        p_list = m._neck(m._extractor(img, training=True), training=True)
        scores, deltas = m._get_fpn_head_results(p_list)
        rois = m._rpn_proposal((deltas, m._get_anchors(list(IMAGE)), m._fg_scores(scores), list(IMAGE)), training=True)
    big = rois[((rois[:, 2] - rois[:, 0]) >= 24) & ((rois[:, 3] - rois[:, 1]) >= 24)]
    assert big.shape[0] >= 3, 'the random model proposes fewer than 3 boxes of 24 pixels'
    gt = big[[0, big.shape[0] // 3, 2 * big.shape[0] // 3]].clone()
    return m, twin, plain, (img, gt, torch.tensor([3, 7, 12], device='cuda'))


def test_caller_model_trains_every_parameter(models, monkeypatch):
    from tf_eager_object_detection_amd import training
    ops = _ops()
    m, twin, plain, inputs = models
    seen = []
    pool_backward = ops.relu_maxpool3_backward
    monkeypatch.setattr(ops, 'relu_maxpool3_backward', lambda z, b, g, **k: seen.append((z, g)) or pool_backward(z, b, g, **k))
    losses, want, again = (x(inputs, training=True) for x in (m, plain, twin))
    assert len(losses) == 4 and all(x.requires_grad for x in losses)
    assert all(_same_bits(a, b) for a, b in zip(losses, want)) and all(_same_bits(a, b) for a, b in zip(losses, again))
    for x in (losses, want, again):
        sum(x).backward()
    params, pparams, tparams = (dict(x.dense.named_parameters()) for x in (m, plain, twin))
    assert len(params) == 134
    for n, p in params.items():                                                # every parameter of the detector, none left at None
        g = p.grad
        assert g is not None and g.shape == p.shape and g.stride() == p.stride(), n
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, n
        assert _same_bits(g, tparams[n].grad), n                               # a second model on the same state: the same bits
    stem = ('conv1.weight', 'conv1.bias')
    assert sorted(n for n, p in pparams.items() if p.grad is None) == sorted(stem)          # train_stem=False: conv1 stays None
    for n in params:
        if n not in stem:
            assert _same_bits(params[n].grad, pparams[n].grad), n              # the other 132: bit-equal to the model without it
    # conv1's gradients are the ops called by hand on the pooled map's gradient the backward pass delivered
    assert len(seen) == 2 and _same_bits(seen[0][1], seen[1][1])               # (m's and twin's backward)
    z, dpool = seen[0]
    conv1 = m.dense.conv1
    _, _, dw, db = _by_hand(inputs[0], conv1, dpool)
    assert _same_bits(conv1.weight.grad.permute(0, 2, 3, 1), dw) and _same_bits(conv1.bias.grad, db)
    # one training step on what .backward() left, as it is: conv1 moves, its version counter with it, and the next pass follows
    named = training.model_variables(m.dense)
    before = {n: (p.detach().clone(), p._version) for n, p in named}
    training.train_step(named, [p.grad for _, p in named], training.MomentumOptimizer(0.01, 0.9), learning_rate_bias_double=True,
                        weight_decays=training.l2_variables(m.dense, 0.0001))
    for n, p in named:
        assert not torch.equal(p.detach(), before[n][0]) and p._version > before[n][1], n
    stepped = m(inputs, training=True)
    assert not any(_same_bits(a, b) for a, b in zip(stepped, losses))


def test_caller_model_constructor_errors():
    from tf_eager_object_detection_amd.model.base_faster_rcnn_model import ResNetFasterRcnn, Vgg16FasterRcnn
    from tf_eager_object_detection_amd.model.base_fpn_model import ResnetV1Fpn
    with pytest.raises(ValueError, match='train_stem=True needs train_extractor=True'):
        ResnetV1Fpn(depth=50, train_stem=True, train_neck=True, train_rpn_head=True, train_roi_head=True)
    with pytest.raises(ValueError, match='train_stem=True needs dtype'):
        ResnetV1Fpn(depth=50, train_stem=True, dtype=torch.float16, **FOUR)
    with pytest.raises(ValueError, match='train_stem=True needs dtype'):
        ResnetV1Fpn(depth=50, train_stem=True, f32_form='x3', **FOUR)
    for cls in (ResNetFasterRcnn, Vgg16FasterRcnn):
        with pytest.raises(TypeError, match='train_stem'):
            cls(train_stem=True)
