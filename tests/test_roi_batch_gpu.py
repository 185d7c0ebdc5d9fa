"""The RoI pooling over a batch of images on the GPU (ops.roi_pool_images, roi_pool_argmax_images, roi_pool_backward_images,
roi_pool_trainable_images, model.roi_pooling.roi_pooling_images): every output byte for byte against tests/roi_grad_np.py applied
image by image (tests/roi_batch_cases.py) and against the single-image functions on each image, the device counts, the
independence of the images, the autograd wiring, the way through a Dense head and the fused RoI losses, graph capture and the
error returns.  No tolerance anywhere."""

import numpy as np
import pytest
import torch

import roi_batch_cases as bc
import roi_cases as rc
import roi_grad_np as rg

pytestmark = pytest.mark.gpu


def _ops():
    from tf_eager_object_detection_amd import ops
    return ops


def _g(a):
    return torch.from_numpy(np.array(a, order='C')).cuda()            # (a copy: the cases' shared arrays are read-only)


def _same_bits(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    want = want.cpu().numpy() if isinstance(want, torch.Tensor) else want
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = got.view(np.uint32) != want.view(np.uint32) if got.dtype == np.float32 else got != want
    assert not bad.any(), '%s: %d of %d elements differ, first at %s: got %r, want %r' % (
        what, int(bad.sum()), bad.size, np.unravel_index(int(np.argmax(bad)), bad.shape), got[bad][0], want[bad][0])


def _device_args(case, counts='case'):
    cnt = case.counts() if isinstance(counts, str) else counts
    kw = dict(strides=[case.stride] * len(case.maps_hw), image_shape=case.image_shape if case.image_shape[0] else None,
              count_dev=None if cnt is None else _g(np.asarray(cnt, np.int32)))
    return _g(case.rois()), (None if case.level() is None else _g(case.level())), kw


def run_batched(case, maps=None, rois=None, dy=None, counts='case'):
    """-> (out, sel or None, [dx]) GPU tensors of the three batched calls; sel is pre-filled with 255, every dx and out with NaN"""
    ops = _ops()
    r, level, kw = _device_args(case, counts)
    r = r if rois is None else rois
    maps = [_g(m) for m in case.maps()] if maps is None else maps
    dy = _g(case.dy()) if dy is None else dy
    shape = (case.B, case.n, case.P, case.P, case.C)
    out = ops.roi_pool_images(maps, r, level, case.norm, case.P, case.pool, out=rc.nan_filled(shape, torch.float32, 'cuda'), **kw)
    sel = None
    if case.pool == rg.POOL_MAX2:
        sel = torch.full(shape, 255, dtype=torch.uint8, device='cuda')
        assert ops.roi_pool_argmax_images(maps, r, level, case.norm, case.P, out=sel, **kw) is sel
    outs = [rc.nan_filled((case.B, h, w, case.C), torch.float32, 'cuda') for h, w in case.maps_hw]
    dxs = ops.roi_pool_backward_images(dy, None, r, level, case.norm, case.P, case.pool, sel=sel, outs=outs, **kw)
    torch.cuda.synchronize()
    assert all(a is b for a, b in zip(dxs, outs))
    return out, sel, dxs


_RESULTS = {}


def _batched(case):
    """the batched calls on a case's own data, run once and shared (nothing writes to them)"""
    if case.name not in _RESULTS:
        _RESULTS[case.name] = run_batched(case)
    return _RESULTS[case.name]


@pytest.mark.parametrize('case', bc.CASES, ids=lambda c: c.name)
def test_out_sel_and_dx_equal_the_restatement_image_by_image(case):
    out, sel, dxs = _batched(case)
    want_out, want_sel, want_dx = case.restated()
    _same_bits(out, want_out, case.name + ' out')
    if want_sel is not None:
        _same_bits(sel, want_sel, case.name + ' sel')
    for l, (g, w) in enumerate(zip(dxs, want_dx)):
        _same_bits(g, w, '%s dx level %d' % (case.name, l))


@pytest.mark.parametrize('case', bc.CASES, ids=lambda c: c.name)
def test_every_image_equals_the_single_image_calls(case):
    ops = _ops()
    out, sel, dxs = _batched(case)
    rois, level, kw = _device_args(case)
    maps, dy = [_g(m) for m in case.maps()], _g(case.dy())
    for b in range(case.B):
        one = dict(kw, count_dev=None if kw['count_dev'] is None else kw['count_dev'][b:b + 1])
        mb = [m[b:b + 1] for m in maps]
        lb = None if level is None else level[b]
        _same_bits(ops.roi_pool(mb, rois[b], lb, case.norm, case.P, case.pool, **one), out[b], '%s out of image %d' % (case.name, b))
        sb = None
        if sel is not None:
            sb = ops.roi_pool_argmax(mb, rois[b], lb, case.norm, case.P, **one)
            _same_bits(sb, sel[b], '%s sel of image %d' % (case.name, b))
        single = ops.roi_pool_backward(dy[b], mb, rois[b], lb, case.norm, case.P, case.pool, sel=sb, **one)
        for l, (s, g) in enumerate(zip(single, dxs)):
            _same_bits(s[0], g[b], '%s dx level %d of image %d' % (case.name, l, b))


def test_no_count_is_a_full_count_and_a_count_above_n_is_n():
    case = bc.BY_NAME['batch_mode_stride_max2_c8_p7_normal']
    assert case.counts() is None
    want = _batched(case)
    for counts in ([case.n] * case.B, [case.n + 27, case.n]):
        got = run_batched(case, counts=counts)
        for a, b in zip([got[0], got[1]] + got[2], [want[0], want[1]] + want[2]):
            assert torch.equal(a, b)


def test_an_image_does_not_depend_on_its_neighbour():
    """other maps, RoIs and dy in image 1: image 0's bytes stay, image 1's change"""
    case = bc.BY_NAME['batch_mode_image_max2_c8_p7_normal']
    first = _batched(case)
    rng = np.random.default_rng(21)
    maps = [_g(m) for m in case.maps()]
    rois, dy = _g(case.rois()), _g(case.dy())
    for t in maps + [dy]:
        t[1] = _g(rng.standard_normal(tuple(t.shape[1:])).astype(np.float32))
    rois[1] = rois[1].flip(0) * 0.75
    second = run_batched(case, maps=maps, rois=rois, dy=dy)
    for a, b in zip([first[0], first[1]] + first[2], [second[0], second[1]] + second[2]):
        assert torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1])


@pytest.mark.parametrize('name', ['batch3_two_levels_counts_13_0_5', 'batch_mode_tp_avg2_c8_p7_normal', 'batch_mode_stride_none_c8_p7_normal'])
def test_roi_pool_trainable_images_wiring(name):
    """the forward is roi_pool_images by bytes; the gradient arrives on exactly the maps that require one and is
    roi_pool_backward_images of the dy that reached the node; the RoIs get none; the same under no_grad through
    roi_pooling_images(trainable=True)"""
    from tf_eager_object_detection_amd.model import roi_pooling as rp
    ops = _ops()
    case = bc.BY_NAME[name]
    plain, _, _ = _batched(case)
    rois, level, kw = _device_args(case)
    maps = [_g(m) for m in case.maps()]
    skip = 1 if len(maps) > 1 else None
    upstream = _g(case.dy())

    def check(pool):
        leaves = [m.clone().requires_grad_(i != skip) for i, m in enumerate(maps)]
        rois_leaf = rois.clone().requires_grad_(True)
        out = pool(leaves, rois_leaf)
        assert out.requires_grad and torch.equal(out, plain)
        seen = []
        out.register_hook(lambda g: seen.append(g.clone()))
        (out * 2.0).backward(upstream)
        assert len(seen) == 1 and torch.equal(seen[0], upstream * 2.0) and rois_leaf.grad is None
        sel = ops.roi_pool_argmax_images(maps, rois, level, case.norm, case.P, **kw) if case.pool == rg.POOL_MAX2 else None
        want = ops.roi_pool_backward_images(seen[0].contiguous(), maps, rois, level, case.norm, case.P, case.pool, sel=sel, **kw)
        for i, (leaf, w) in enumerate(zip(leaves, want)):
            if i == skip:
                assert leaf.grad is None
            else:
                assert torch.equal(leaf.grad, w) and leaf.grad.abs().max() > 0, i

    check(lambda leaves, r: ops.roi_pool_trainable_images(leaves, r, level, case.norm, case.P, case.pool, **kw))

    def through_the_model_function(leaves, r):
        with torch.no_grad():                                   # (the caller's grad mode does not matter)
            return rp.roi_pooling_images(leaves, r, level, case.norm, case.P, case.pool, trainable=True, **kw)
    check(through_the_model_function)
    leaves = [m.clone().requires_grad_(True) for m in maps]
    o = rp.roi_pooling_images(leaves, rois, level, case.norm, case.P, case.pool, **kw)
    assert torch.equal(o, plain) and not o.requires_grad                                       # the default: the plain path
    o = rp.roi_pooling_images(maps, rois, level, case.norm, case.P, case.pool, trainable=True, **kw)
    assert torch.equal(o, plain) and not o.requires_grad                                       # no map asks for a gradient


def test_roi_pooling_images_is_roi_pooling_fpn_levels_for_a_batch():
    from tf_eager_object_detection_amd.model import roi_pooling as rp
    ops = _ops()
    case = bc.BY_NAME['batch3_two_levels_counts_13_0_5']
    rois, level, kw = _device_args(case)
    maps = [_g(m) for m in case.maps()]
    got = rp.roi_pooling_images(maps, rois, level, ops.ROI_NORM_IMAGE, case.P, ops.ROI_POOL_MAX2, image_shape=case.image_shape,
                                count_dev=kw['count_dev'])
    for b in range(case.B):
        want = rp.roi_pooling_fpn_levels([m[b:b + 1] for m in maps], rois[b], level[b], case.image_shape, case.P,
                                         count_dev=kw['count_dev'][b:b + 1])
        assert torch.equal(got[b], want)


def test_through_the_roi_head_and_the_fused_losses():
    """2 images: proposal targets -> batched trainable pooling of the sampled RoIs over two maps that require a gradient -> two
    ops.dense_trainable layers -> fused_roi_losses on [2,...] -> sum().backward().  The maps' gradient is the restatement applied
    to the dy that reached the pooling.  The wiring only: the head's bits are not compared."""
    from tf_eager_object_detection_amd.model import roi_pooling as rp
    from tf_eager_object_detection_amd.model.losses import fused_roi_losses
    ops = _ops()
    B, S, P, Cm, K, shape, hw = 2, 16, 7, 32, 64, (72, 88), ((9, 11), (5, 6))
    rng = np.random.default_rng(31)
    gt = np.stack([bc._pixel_boxes('head_gt_%d' % b, 2, *shape) for b in range(B)]).clip(0, 71)                 # [B,2,4]
    rois = np.stack([np.concatenate([bc._pixel_boxes('head_rois_%d' % b, 26, *shape).clip(0, 71), gt[b],
                                     gt[b] + rng.normal(0, 1.5, (2, 4)).astype(np.float32),
                                     gt[b] + rng.normal(0, 1.5, (2, 4)).astype(np.float32)]) for b in range(B)]).astype(np.float32)
    pt = ops.proposal_targets(_g(rois), _g(gt.reshape(-1, 4)), _g(rng.integers(1, K, B * 2)), [0, 2, 4], K, 0.5, 0.0, S, S // 4,
                              [0, 0, 0, 0], [0.1, 0.1, 0.2, 0.2], seed=5)
    sampled = pt.final_rois                                                                                       # [B,S,4]
    area = (sampled[..., 2] - sampled[..., 0]) * (sampled[..., 3] - sampled[..., 1])
    level = (area > area.median(dim=1, keepdim=True).values).to(torch.int32)                                    # both levels in each image
    maps_np = [rng.standard_normal((B, h, w, Cm)).astype(np.float32) for h, w in hw]
    leaves = [_g(m).requires_grad_(True) for m in maps_np]
    feats = rp.roi_pooling_images(leaves, sampled, level, ops.ROI_NORM_IMAGE, P, ops.ROI_POOL_MAX2, image_shape=shape, trainable=True)
    assert tuple(feats.shape) == (B, S, P, P, Cm) and feats.requires_grad
    seen = []
    feats.register_hook(lambda g: seen.append(g.clone()))
    w1 = _g((rng.standard_normal((64, P * P * Cm)) * 0.05).astype(np.float32)).requires_grad_(True)
    b1 = _g(np.zeros(64, np.float32)).requires_grad_(True)
    w2 = _g((rng.standard_normal((5 * K, 64)) * 0.2).astype(np.float32)).requires_grad_(True)
    b2 = _g(np.zeros(5 * K, np.float32)).requires_grad_(True)
    hidden = ops.dense_trainable(feats.reshape(B * S, P * P * Cm), w1, b1, relu=True)
    head = ops.dense_trainable(hidden, w2, b2).reshape(B, S, 5 * K)
    cls, reg = fused_roi_losses(head[..., :K].contiguous(), head[..., K:].contiguous(), pt, 1.0)
    assert tuple(cls.shape) == (B,) and tuple(reg.shape) == (B,)
    (cls + reg).sum().backward()
    assert len(seen) == 1 and w1.grad is not None and w2.grad is not None
    dy = seen[0].contiguous().cpu().numpy()
    for b in range(B):
        im = rg.GradCase('head_%d' % b, rg.NORM_IMAGE, rg.POOL_MAX2, Cm, P, sampled[b].cpu().numpy(), level=level[b].cpu().numpy(),
                         maps_hw=hw, image_shape=shape)
        mb = [m[b] for m in maps_np]
        want = rg.backward(im, dy[b], rg.select(im, mb))
        for l, leaf in enumerate(leaves):
            _same_bits(leaf.grad[b], want[l], 'map %d of image %d' % (l, b))
            assert np.abs(want[l]).max() > 0


def test_graph_capture_replays_bit_equal_to_eager():
    """forward + select + backward of a batch captured once, replayed twice on new map, RoI, count and upstream contents"""
    ops = _ops()
    case = bc.BY_NAME['batch3_two_levels_counts_13_0_5']
    rois, level, kw = _device_args(case)
    maps, dy = [_g(m) for m in case.maps()], _g(case.dy())
    shape = (case.B, case.n, case.P, case.P, case.C)
    feats = torch.empty(shape, device='cuda')
    sel = torch.empty(shape, dtype=torch.uint8, device='cuda')
    dxs = [torch.empty_like(m) for m in maps]

    def step():
        ops.roi_pool_images(maps, rois, level, case.norm, case.P, case.pool, out=feats, **kw)
        ops.roi_pool_argmax_images(maps, rois, level, case.norm, case.P, out=sel, **kw)
        ops.roi_pool_backward_images(dy, None, rois, level, case.norm, case.P, case.pool, sel=sel, outs=dxs, **kw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            step()
    torch.cuda.current_stream().wait_stream(side)
    rng = np.random.default_rng(12)
    for turn in range(2):
        for t in maps + [dy]:
            t.copy_(_g(rng.standard_normal(tuple(t.shape)).astype(np.float32)))
        rois.copy_(rois.flip(1))
        kw['count_dev'].copy_(kw['count_dev'].roll(1))
        for t in dxs + [feats]:
            t.fill_(float('nan'))
        sel.fill_(255)
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in [feats, sel] + dxs]
        step()
        torch.cuda.synchronize()
        for a, b in zip(got, [feats, sel] + dxs):
            assert torch.equal(a, b), turn
        assert bool(torch.isfinite(feats).all()) and all(bool(torch.isfinite(t).all()) for t in dxs) and int(sel.max()) <= 4
        assert all(float(t.abs().max()) > 0 for t in dxs)


def test_error_returns():
    """B = 0, batch sizes that do not agree and a misaligned rois: OdetError (ODET_E_INVALID where the library sees it), the
    outputs untouched"""
    ops = _ops()
    OdetError = ops.L.OdetError
    case = bc.BY_NAME['batch_mode_stride_max2_c8_p7_normal']
    rois, level, kw = _device_args(case)
    maps, dy = [_g(m) for m in case.maps()], _g(case.dy())
    shape = (case.B, case.n, case.P, case.P, case.C)
    sel = torch.zeros(shape, dtype=torch.uint8, device='cuda')
    args = (case.norm, case.P)

    def calls(maps, rois, dy, sel):
        return (lambda: ops.roi_pool_images(maps, rois, level, *args, case.pool, **kw),
                lambda: ops.roi_pool_argmax_images(maps, rois, level, *args, **kw),
                lambda: ops.roi_pool_backward_images(dy, maps, rois, level, *args, case.pool, sel=sel, **kw))
    # B = 0
    for call in calls([m[:0] for m in maps], rois[:0], dy[:0], sel[:0]):
        with pytest.raises(OdetError, match=r'odet error -1: odet_roi_pool_\w*images: batch 0'):
            call()
    # three images of maps, two of RoIs; two of maps, one of dy
    for call in calls([torch.cat([m, m[:1]]) for m in maps], rois, dy, sel):
        with pytest.raises(OdetError, match='share the batch size'):
            call()
    with pytest.raises(OdetError, match='share the batch size'):
        ops.roi_pool_backward_images(dy[:1], maps, rois, level, *args, case.pool, sel=sel, **kw)
    # rois 4 bytes off a 16-byte boundary
    off = torch.zeros(rois.numel() + 4, device='cuda')[1:1 + rois.numel()].view(rois.shape)
    off.copy_(rois)
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    out = rc.nan_filled(shape, torch.float32, 'cuda')
    dx = rc.nan_filled(tuple(maps[0].shape), torch.float32, 'cuda')
    with pytest.raises(OdetError, match='odet error -1: odet_roi_pool_images: rois'):
        ops.roi_pool_images(maps, off, level, *args, case.pool, out=out, **kw)
    with pytest.raises(OdetError, match='odet error -1: odet_roi_pool_argmax_images: rois'):
        ops.roi_pool_argmax_images(maps, off, level, *args, **kw)
    with pytest.raises(OdetError, match='odet error -1: odet_roi_pool_backward_images: rois'):
        ops.roi_pool_backward_images(dy, None, off, level, *args, case.pool, sel=sel, outs=[dx], **kw)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(dx).all())                        # nothing was launched
