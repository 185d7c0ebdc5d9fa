"""The float32 Dense backward on the GPU (csrc/dense_grad.hip: odet_dense_dgrad_f32, odet_dense_wgrad_f32) against the float64
statement of tests/dense_grad_np.py: exact on integer data, within the any-order summation bound on random data, bit-equal
between calls, behind torch.autograd (ops.dense_trainable), in the FPN RoI head and the caller model, and under graph capture.

Worst observed fraction of bound (b) on an MI355X (printed by test_random_data_within_the_summation_bound; the table is in DESIGN
3.13): dx 0.020, dw 0.326 (3 rows: a sum of three products), db 0.188."""
import numpy as np
import pytest
import torch

import dense_grad_np as dg

pytestmark = pytest.mark.gpu

U = 2.0 ** -23                                       # unit roundoff of bound (b): one bit, the matrix instruction's inner rounding is not documented
GRID = [(r, ci, co) for r in (1, 2, 3, 5, 17, 64, 130) for ci in (64, 96, 160) for co in (64, 192)]
# whichever tile and split the launcher picks for the head's real fc2 (dgrad: split in 4) and final layer; and the final layer
# at the sampler's full 256 rows (wgrad: split in 4)
HEAD = [(256, 1024, 1024), (37, 1024, 128), (256, 1024, 128)]
MASKS = [(False, False), (True, False), (False, True), (True, True)]         # (y_relu, x_relu)


def _ops():
    from tf_eager_object_detection_amd import ops
    return ops


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _splits(shape):
    L = _ops().L.lib()
    return [bool(L.odet_dense_grad_workspace_bytes(k, *shape)) for k in (0, 1)]


def _run(dy, w, x, y, xr):
    ops = _ops()
    dx = ops.dense_dgrad(_dev(dy), _dev(w), _dev(y), _dev(xr))
    dw, db = ops.dense_wgrad(_dev(dy), _dev(x), _dev(y))
    return dx.cpu().numpy(), dw.cpu().numpy(), db.cpu().numpy()


@pytest.mark.parametrize('shape', GRID + HEAD, ids=lambda s: '%dx%dx%d' % s)
def test_integer_data_is_exact(shape):
    """(a): every product and partial sum is an integer below 2^24, so any correct order gives the float64 result exactly"""
    rows, cin, cout = shape
    rng = np.random.default_rng(rows * 1000003 + cin * 1009 + cout)
    x = rng.integers(-8, 9, (rows, cin))
    w = rng.integers(-4, 5, (cout, cin))
    dy = rng.integers(-4, 5, (rows, cout))
    y = rng.integers(-2, 3, (rows, cout))                      # zeros, negatives and positives
    xr = rng.integers(-2, 3, (rows, cin))
    assert max(cout * 4 * 4, rows * 4 * 8, rows * 4) < 2 ** 24          # the largest partial sum of dx, dw, db
    for my, mx in MASKS:
        yy, xx = (y if my else None), (xr if mx else None)
        dx, dw, db = _run(dy, w, x, yy, xx)
        wdw, wdb = dg.wgrad(dy, x, yy)
        assert torch.equal(torch.from_numpy(dx).double(), torch.from_numpy(dg.dgrad(dy, w, yy, xx))), ('dx', my, mx)
        assert torch.equal(torch.from_numpy(dw).double(), torch.from_numpy(wdw)), ('dw', my, mx)
        assert torch.equal(torch.from_numpy(db).double(), torch.from_numpy(wdb)), ('db', my, mx)
    if rows >= 2:                                               # without the bias gradient, and into a caller's tensor
        ops = _ops()
        out = torch.full((cout, cin), 7.0, device='cuda')
        dw2, none = ops.dense_wgrad(_dev(dy), _dev(x), None, with_bias=False, out=out)
        assert none is None and dw2 is out and torch.equal(out.cpu().double(), torch.from_numpy(dg.wgrad(dy, x)[0]))


def _fraction(got, want, bound):
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= bound).all(), 'largest excess %g over a bound of %g' % ((err - bound).max(), bound.flat[(err - bound).argmax()])
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


RANDOM = [(3, 96, 64), (130, 160, 192), (17, 64, 192)] + HEAD


@pytest.mark.parametrize('shape', RANDOM, ids=lambda s: '%dx%dx%d' % s)
def test_random_data_within_the_summation_bound(shape):
    """(b): |got - want| <= K * 2^-23 * (|a| . |b|) per element, K the contraction length (cout for dx, rows for dw and db): the
    bound of a float32 sum of K rounded products in ANY order"""
    rows, cin, cout = shape
    rng = np.random.default_rng(cin * 7919 + rows)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    x, w, dy, y, xr = f(rows, cin), f(cout, cin), f(rows, cout), f(rows, cout), f(rows, cin)
    worst = {}
    for my, mx in MASKS:
        yy, xx = (y if my else None), (xr if mx else None)
        dx, dw, db = _run(dy, w, x, yy, xx)
        adw, adb = dg.wgrad_abs(dy, x, yy)
        wdw, wdb = dg.wgrad(dy, x, yy)
        bdx = cout * U * dg.dgrad_abs(dy, w, yy)
        if mx:
            bdx = np.where(xr > 0, bdx, 0.0)                    # (a masked element is an exact zero)
        for name, frac in (('dx', _fraction(dx, dg.dgrad(dy, w, yy, xx), bdx)), ('dw', _fraction(dw, wdw, rows * U * adw)),
                           ('db', _fraction(db, wdb, rows * U * adb))):
            worst[name] = max(worst.get(name, 0.0), frac)
    print('\n%s: worst fraction of the bound  dx %.4f  dw %.4f  db %.4f' % (shape, worst['dx'], worst['dw'], worst['db']))


SPLIT = [(256, 1024, 1024), (256, 1024, 128)]               # the shapes of (a) that split (test_the_head_shapes_that_split_are_under_test)


@pytest.mark.parametrize('shape', SPLIT + [(130, 160, 192)], ids=lambda s: '%dx%dx%d' % s)
def test_two_calls_are_bit_equal(shape):
    """(c): every shape of (a) whose dgrad or wgrad splits its contraction (and one that does not)"""
    rows, cin, cout = shape
    rng = np.random.default_rng(5)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    x, w, dy, y, xr = f(rows, cin), f(cout, cin), f(rows, cout), f(rows, cout), f(rows, cin)
    a = _run(dy, w, x, y, xr)
    junk = torch.full((1 << 22,), float('nan'), device='cuda')          # (whatever the workspace holds does not matter)
    del junk
    b = _run(dy, w, x, y, xr)
    for p, q in zip(a, b):
        assert np.array_equal(p.view(np.uint32), q.view(np.uint32))


def test_the_head_shapes_that_split_are_under_test():
    assert _splits((256, 1024, 1024)) == [True, False] and _splits((256, 1024, 128)) == [False, True]
    assert [s for s in GRID + HEAD if any(_splits(s))] == SPLIT


def test_dense_trainable_forward_and_backward():
    """(d): forward = ops.dense bit for bit; backward fills .grad with the kernels' results; no input gradient is computed (or
    returned) when the input needs none"""
    ops = _ops()
    rng = np.random.default_rng(9)
    rows, cin, cout = 21, 96, 128
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).cuda()
    x, dy = f(rows, cin), f(rows, cout)
    for relu in (True, False):
        w, b = f(cout, cin).requires_grad_(), f(cout).requires_grad_()
        y = ops.dense_trainable(x, w, b, relu=relu)
        assert torch.equal(y, ops.dense(x, w.detach(), b.detach(), relu=relu)) and y.requires_grad
        y.backward(dy)
        dw, db = ops.dense_wgrad(dy, x, y.detach() if relu else None)
        assert x.grad is None
        assert torch.equal(w.grad, dw) and torch.equal(b.grad, db)
        assert w.grad.is_contiguous() and w.grad.shape == w.shape and b.grad.shape == b.shape
        xg = x.clone().requires_grad_()
        y2 = ops.dense_trainable(xg, w, b, relu=relu)
        y2.backward(dy)
        assert torch.equal(xg.grad, ops.dense_dgrad(dy, w.detach(), y2.detach() if relu else None))
    w = f(cout, cin).requires_grad_()                           # a layer without a bias
    ops.dense_trainable(x, w, None, relu=True).backward(dy)
    assert w.grad is not None
    with ops.f32_form('x3'):
        with pytest.raises(ValueError, match="only under f32_form 'exact'"):
            ops.dense_trainable(x, w, None)
    with pytest.raises(ValueError, match='float32'):
        ops.dense_dgrad(dy.half(), w.detach().half())


# ---- (e) the head and the caller model ----------------------------------------------------------------------------------------
def _head_reference(feats, det, dys, dyd):
    """float64 torch autograd of the head on the same features and head-output gradients -> ({name: gradient}, {name: bound}).
    Bound (b) composed over the layers (u = 2^-23; R rows; |.| elementwise; a contraction of length K on operands with error
    bounds Ea, Eb: K u (|a| + Ea)(|b| + Eb) + Ea |b| + |a| Eb, second-order terms kept on the safe side):
      forward   E1 = (K1 + 1) u (|x| |W1|^T + |b1|);  E2 = (K2 + 1) u ((|h1| + E1) |W2|^T + |b2|) + E1 |W2|^T
      a ReLU gate whose float64 pre-activation lies within its forward bound of zero may fall either way in float32: such an
      element of dz carries its whole magnitude as error, Z = |dh| + D; elsewhere Z = D under an open gate, 0 under a closed one
      final     dW3: R u |dy|^T (|h2| + E2) + |dy|^T E2;  db3: R u sum |dy|;  dh2: D2 = K3 u |dy| |W3|
      fc2       dW2: R u (|dz2| + Z2)^T (|h1| + E1) + Z2^T (|h1| + E1) + |dz2|^T E1;  db2: R u sum (|dz2| + Z2) + sum Z2
                dh1: D1 = K2 u (|dz2| + Z2) |W2| + Z2 |W2|
      fc1       dW1: R u (|dz1| + Z1)^T |x| + Z1^T |x|;  db1: R u sum (|dz1| + Z1) + sum Z1"""
    d = lambda t: t.detach().double()
    names = ('fc1.weight', 'fc1.bias', 'fc2.weight', 'fc2.bias', 'score.weight', 'score.bias', 'bbox.weight', 'bbox.bias')
    params = dict(det.named_parameters())
    p = {n: d(params[n]).requires_grad_() for n in names}
    x = d(feats).reshape(feats.shape[0], -1)
    pre1 = x @ p['fc1.weight'].T + p['fc1.bias']
    h1 = torch.relu(pre1)
    pre2 = h1 @ p['fc2.weight'].T + p['fc2.bias']
    h2 = torch.relu(pre2)
    s = h2 @ p['score.weight'].T + p['score.bias']
    b = h2 @ p['bbox.weight'].T + p['bbox.bias']
    torch.autograd.backward([s, b], [d(dys), d(dyd)])
    ref = {n: p[n].grad for n in names}
    with torch.no_grad():
        A = torch.abs
        R, K1, K2 = x.shape[0], x.shape[1], h1.shape[1]
        W1, W2 = A(p['fc1.weight']), A(p['fc2.weight'])
        W3 = torch.cat([A(p['score.weight']), A(p['bbox.weight'])], 0)
        K3 = (W3.shape[0] + 63) // 64 * 64
        dy = torch.cat([A(d(dys)), A(d(dyd))], 1)
        E1 = (K1 + 1) * U * (A(x) @ W1.T + A(p['fc1.bias']))
        E2 = (K2 + 1) * U * ((h1 + E1) @ W2.T + A(p['fc2.bias'])) + E1 @ W2.T
        bw3 = R * U * dy.T @ (h2 + E2) + dy.T @ E2
        bb3 = R * U * dy.sum(0)
        dh2 = torch.cat([d(dys), d(dyd)], 1) @ torch.cat([p['score.weight'], p['bbox.weight']], 0)
        D2 = K3 * U * dy @ W3
        Z2 = torch.where(A(pre2) <= E2, A(dh2) + D2, (pre2 > 0) * D2)
        dz2 = A(dh2 * (pre2 > 0))
        bw2 = R * U * (dz2 + Z2).T @ (h1 + E1) + Z2.T @ (h1 + E1) + dz2.T @ E1
        bb2 = R * U * (dz2 + Z2).sum(0) + Z2.sum(0)
        dh1 = (dh2 * (pre2 > 0)) @ p['fc2.weight']
        D1 = K2 * U * (dz2 + Z2) @ W2 + Z2 @ W2
        Z1 = torch.where(A(pre1) <= E1, A(dh1) + D1, (pre1 > 0) * D1)
        dz1 = A(dh1 * (pre1 > 0))
        bw1 = R * U * (dz1 + Z1).T @ A(x) + Z1.T @ A(x)
        bb1 = R * U * (dz1 + Z1).sum(0) + Z1.sum(0)
        n1 = p['score.weight'].shape[0]
        bound = {'fc1.weight': bw1, 'fc1.bias': bb1, 'fc2.weight': bw2, 'fc2.bias': bb2, 'score.weight': bw3[:n1],
                 'score.bias': bb3[:n1], 'bbox.weight': bw3[n1:], 'bbox.bias': bb3[n1:]}
    return ref, bound


def _check_head_grads(det, feats, dys, dyd):
    ref, bound = _head_reference(feats, det, dys, dyd)
    worst = {}
    for n, p in det.named_parameters():
        if n not in ref:
            assert p.grad is None, n
            continue
        assert p.grad is not None and p.grad.is_contiguous() and p.grad.shape == p.shape, n
        err = (p.grad.double() - ref[n]).abs()
        assert bool((err <= bound[n]).all()), (n, float((err - bound[n]).max()))
        assert float(ref[n].abs().max()) > 0, n
        worst[n] = float((err / bound[n].clamp_min(1e-300)).max())
    print('\nhead gradients, worst fraction of the composed bound: %s' % ', '.join('%s %.2e' % kv for kv in worst.items()))


def _manual_head_grads(det, feats, dys, dyd):
    """the same gradients from the kernels called by hand on the head's own float32 activations: what autograd must deliver, bit
    for bit"""
    ops = _ops()
    with torch.no_grad():
        x = feats.reshape(feats.shape[0], -1).contiguous()
        h1 = ops.dense(x, det.fc1.weight, det.fc1.bias, relu=True)
        h2 = ops.dense(h1, det.fc2.weight, det.fc2.bias, relu=True)
        wpad, _ = det._final_layer()
        n1, n5 = det.score.out_features, det.score.out_features + det.bbox.out_features
        dy = torch.zeros((x.shape[0], wpad.shape[0]), device=x.device)
        dy[:, :n1], dy[:, n1:n5] = dys, dyd
        dw3, db3 = ops.dense_wgrad(dy, h2)
        dh2 = ops.dense_dgrad(dy, wpad)
        dw2, db2 = ops.dense_wgrad(dh2, h1, h2)
        dh1 = ops.dense_dgrad(dh2, det.fc2.weight, h2)
        dw1, db1 = ops.dense_wgrad(dh1, x, h1)
    return {'fc1.weight': dw1, 'fc1.bias': db1, 'fc2.weight': dw2, 'fc2.bias': db2, 'score.weight': dw3[:n1], 'score.bias': db3[:n1],
            'bbox.weight': dw3[n1:n5], 'bbox.bias': db3[n1:n5]}


@pytest.fixture(scope='module')
def detector():
    from tf_eager_object_detection_amd.model.fpn_detector import ResNetFpnDetector
    torch.manual_seed(2)
    det = ResNetFpnDetector(50, 21, (64, 64), 1, dtype=torch.float32)
    return det.to(device='cuda', dtype=torch.float32, memory_format=torch.channels_last).eval()


def test_roi_head_trainable(detector):
    det = detector
    det.zero_grad(set_to_none=True)
    rng = np.random.default_rng(3)
    feats = torch.from_numpy(np.maximum(rng.standard_normal((19, 7, 7, 256)), 0).astype(np.float32)).cuda()
    with torch.no_grad():
        s0, d0 = det.roi_head(feats)
    s, d = det.roi_head_trainable(feats)
    assert torch.equal(s, s0) and torch.equal(d, d0) and s.requires_grad and d.requires_grad
    dys = torch.from_numpy(rng.standard_normal(tuple(s.shape)).astype(np.float32)).cuda()
    dyd = torch.from_numpy(rng.standard_normal(tuple(d.shape)).astype(np.float32)).cuda()
    torch.autograd.backward([s, d], [dys, dyd])
    for n, g in _manual_head_grads(det, feats, dys, dyd).items():
        assert torch.equal(dict(det.named_parameters())[n].grad, g), n
    _check_head_grads(det, feats, dys, dyd)
    with pytest.raises(ValueError, match='roi_head_trainable needs'):
        det.f32_form = 'x3'
        try:
            det.roi_head_trainable(feats)
        finally:
            det.f32_form = 'exact'
    det.zero_grad(set_to_none=True)


@pytest.mark.parametrize('kind', ['torch', 'hip'])
def test_caller_model_trains_its_roi_head(kind):
    """ResnetV1Fpn(train_roi_head=True), both training branches (the torch losses and the fused ones, on the fused targets, whose
    sampling is a function of the seed): the RoI losses carry a graph into fc1, fc2, score, bbox; one MomentumOptimizer step
    moves them and the derived padded final layer follows"""
    from tf_eager_object_detection_amd import training
    from tf_eager_object_detection_amd.model.base_fpn_model import ResnetV1Fpn
    from tf_eager_object_detection_amd.model.fpn_detector import ResNetFpnDetector
    shape = (256, 352)
    kw = dict(depth=50, training_targets='hip', training_losses=kind, roi_training_total_num_samples=32, roi_training_max_pos_samples=8)
    torch.manual_seed(1)
    m = ResnetV1Fpn(train_roi_head=True, **kw)
    with torch.no_grad():                                   # (spreads the fresh RpnHead's proposals over sizes and pyramid levels)
        b = m.dense.rpn_bbox.bias
        b.add_(torch.linspace(0.0, 1.6, b.numel(), device=b.device, dtype=b.dtype))
    plain = ResnetV1Fpn(**kw)
    plain._dense_ref.load_state_dict(m._dense_ref.state_dict())
    rng = np.random.default_rng(1)
    img = torch.from_numpy((rng.uniform(0, 255, (1,) + shape + (3,)) - 110).astype(np.float32)).cuda()
    # the ground truth is three of the model's own proposals: RoIs of IoU 1 exist, so the head has foreground rows and the box
    # layer a gradient
    with torch.no_grad():
        p_list = m._neck(m._extractor(img, training=True), training=True)
        scores, deltas = m._get_fpn_head_results(p_list)
        rois = m._rpn_proposal((deltas, m._get_anchors(list(shape)), m._fg_scores(scores), list(shape)), training=True)
    big = rois[((rois[:, 2] - rois[:, 0]) >= 24) & ((rois[:, 3] - rois[:, 1]) >= 24)]
    assert big.shape[0] >= 3, 'the random model proposes fewer than 3 boxes of 24 pixels'
    gt = big[[0, big.shape[0] // 3, 2 * big.shape[0] // 3]].clone()
    gl = torch.tensor([3, 7, 12], device='cuda')
    seen = {}
    head = m._get_trainable_roi_head()

    def spy(feats):
        s, d = head(feats)
        seen['feats'] = feats
        s.register_hook(lambda g: seen.__setitem__('dys', g.clone()))
        d.register_hook(lambda g: seen.__setitem__('dyd', g.clone()))
        return s, d
    m._get_trainable_roi_head = lambda: spy
    losses = m((img, gt, gl), training=True)
    want = plain((img, gt, gl), training=True)
    assert all(torch.equal(a.detach(), b) for a, b in zip(losses, want))                 # bit-equal to the path without the keyword
    assert not any(x.requires_grad for x in want) and all(p.grad is None for p in plain._dense_ref.parameters())
    assert not losses[0].requires_grad and not losses[1].requires_grad and losses[2].requires_grad and losses[3].requires_grad
    assert not seen['feats'].requires_grad                                                 # pooling stays under no_grad
    (losses[2] + losses[3]).backward()
    det = m.dense
    trained = ('fc1.weight', 'fc1.bias', 'fc2.weight', 'fc2.bias', 'score.weight', 'score.bias', 'bbox.weight', 'bbox.bias')
    assert sorted(n for n, p in det.named_parameters() if p.grad is not None) == sorted(trained)
    assert seen['dys'].abs().max() > 0 and seen['dyd'].abs().max() > 0
    _check_head_grads(det, seen['feats'], seen['dys'], seen['dyd'])
    # one training step on what .backward() left, as it is
    named = [(n, p) for n, p in training.model_variables(det) if n in trained]
    before = {n: p.detach().clone() for n, p in named}
    training.train_step(named, [p.grad for _, p in named], training.MomentumOptimizer(0.01, 0.9), learning_rate_bias_double=True,
                        weight_decays=training.l2_variables(det, 0.0001))
    for n, p in named:
        if n.endswith('weight'):
            assert not torch.equal(p.detach(), before[n]), n
    fresh = ResNetFpnDetector(50, 21, (64, 64), 1, dtype=torch.float32)
    fresh.to(device='cuda', dtype=torch.float32, memory_format=torch.channels_last).eval()
    fresh.load_state_dict(det.state_dict())
    with torch.no_grad():
        s1, d1 = det.roi_head(seen['feats'])
        s2, d2 = fresh.roi_head(seen['feats'])
        s3, d3 = det.roi_head_trainable(seen['feats'])
    assert torch.equal(s1, s2) and torch.equal(d1, d2) and torch.equal(s1, s3) and torch.equal(d1, d3)
    assert not torch.equal(s1, seen_scores(plain, seen['feats']))                       # (and the step did change the outputs)


def seen_scores(model, feats):
    with torch.no_grad():
        return model._dense_ref.roi_head(feats)[0]


def test_graph_capture_replays_bit_equal_to_eager():
    """(f): a dgrad (a shape that splits, so its workspace and second launch are captured too) and a wgrad on one stream, replayed
    on new input contents"""
    ops = _ops()
    rng = np.random.default_rng(11)
    rows, cin, cout = 256, 1024, 1024
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).cuda()
    dy, w, x, y = f(rows, cout), f(cout, cin), f(rows, cin), f(rows, cout)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.dense_dgrad(dy, w, y, x)                            # (the kernels' one-time device set-up happens outside the capture)
        ops.dense_wgrad(dy, x, y)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            dx = ops.dense_dgrad(dy, w, y, x)
            dw, db = ops.dense_wgrad(dy, x, y)
    torch.cuda.current_stream().wait_stream(side)
    for t in (dy, w, x, y):
        t.copy_(f(*t.shape))
    graph.replay()
    torch.cuda.synchronize()
    edx = ops.dense_dgrad(dy, w, y, x)
    edw, edb = ops.dense_wgrad(dy, x, y)
    assert torch.equal(dx, edx) and torch.equal(dw, edw) and torch.equal(db, edb)
