"""The RoI pooling backward on the GPU (csrc/roi_grad.hip): sel and every dx byte for byte against the NumPy restatement
(tests/roi_grad_np.py) with dx pre-filled with NaN, the device count, RoI levels, reproducibility and the order of the sums, the
autograd wiring (ops.roi_pool_trainable), the caller model, an end-to-end backward into the extractor's weights through the
plain-torch maps, and graph capture."""

import numpy as np
import pytest
import torch

import roi_cases as rc
import roi_grad_np as rg

pytestmark = pytest.mark.gpu


def _ops():
    from tf_eager_object_detection_amd import ops
    return ops


def _g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _device_args(case):
    count = None if case.count is None else torch.tensor([case.count], dtype=torch.int32, device='cuda')
    kw = dict(strides=[case.stride] * len(case.maps_hw), image_shape=case.image_shape if case.image_shape[0] else None, count_dev=count)
    return _g(case.rois), (None if case.level is None else _g(case.level)), kw


def gpu_select(case, maps):
    ops = _ops()
    rois, level, kw = _device_args(case)
    out = torch.full((case.n, case.P, case.P, case.C), 255, dtype=torch.uint8, device='cuda')
    ops.roi_pool_argmax([_g(m)[None] for m in maps], rois, level, case.norm, case.P, out=out, **kw)
    return out


def gpu_backward(case, dy, sel):
    """-> [level] numpy [H,W,C]; every dx is pre-filled with NaN"""
    ops = _ops()
    rois, level, kw = _device_args(case)
    outs = [rc.nan_filled((1, h, w, case.C), torch.float32, 'cuda') for h, w in case.maps_hw]
    dxs = ops.roi_pool_backward(dy if isinstance(dy, torch.Tensor) else _g(dy), None, rois, level, case.norm, case.P, case.pool, sel=sel,
                                outs=outs, **kw)
    torch.cuda.synchronize()
    assert all(a is b for a, b in zip(dxs, outs))
    return [d[0].cpu().numpy() for d in dxs]


def _same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = got.view(np.uint32) != want.view(np.uint32) if got.dtype == np.float32 else got != want
    assert not bad.any(), '%s: %d of %d elements differ, first at %s: got %r, want %r' % (
        what, int(bad.sum()), bad.size, np.unravel_index(int(np.argmax(bad)), bad.shape), got[bad][0], want[bad][0])


def _check_case(case, maps=None, dy=None):
    """sel and dx of every level, byte for byte; -> (gpu sel tensor, [dx numpy])"""
    maps = case.maps() if maps is None else maps
    dy = case.dy() if dy is None else dy
    sel_t, sel = None, None
    if case.pool == rg.POOL_MAX2:
        sel = rg.select(case, maps)
        sel_t = gpu_select(case, maps)
        _same_bits(sel_t.cpu().numpy(), sel, case.name + ' sel')
    want = rg.backward(case, dy, sel)
    got = gpu_backward(case, dy, sel_t)
    for l, (g, w) in enumerate(zip(got, want)):
        _same_bits(g, w, '%s dx level %d' % (case.name, l))
    return sel_t, got


CASES = (
    [rg.mode_case(norm, pool) for norm, pool in rg.MODES]                                     # the five mode pairs, P = 7, 17 x 17
    + [rg.mode_case(rg.NORM_STRIDE, rg.POOL_NONE, C=4, P=1), rg.mode_case(rg.NORM_IMAGE, rg.POOL_MAX2, C=4, P=1),      # `single`; crop 2
       rg.mode_case(rg.NORM_STRIDE, rg.POOL_MAX2, C=4, P=16), rg.mode_case(rg.NORM_NOPAD, rg.POOL_NONE, C=4, P=16),   # 64 / 32 mask bits
       rg.mode_case(rg.NORM_TP, rg.POOL_AVG2, C=4, P=16)]
    + [rg.fpn_case(C) for C in (4, 260, 256, 512)]                                            # channels: smallest, 256 + 4, one / two slices
    + [rg.mode_case(rg.NORM_TP, rg.POOL_AVG2, C=260), rg.mode_case(rg.NORM_STRIDE, rg.POOL_NONE, C=512)]
    + [rg.wide_case(rg.POOL_MAX2), rg.wide_case(rg.POOL_NONE)]                                # a map one cell wider than the x tile
    + [rg.coords_case(w) for w in ('edge_at', 'edge_beyond', 'edge_rev', 'nonfinite', 'small', 'pileup')]
    + [rg.coords_case('edge_rev', rg.NORM_IMAGE, rg.POOL_NONE), rg.coords_case('nonfinite', rg.NORM_TP, rg.POOL_AVG2),
       rg.coords_case('edge_at', rg.NORM_NOPAD, rg.POOL_NONE), rg.coords_case('pileup', rg.NORM_TP, rg.POOL_AVG2)])


@pytest.mark.parametrize('case', CASES, ids=lambda c: c.name)
def test_sel_and_dx_equal_the_restatement_byte_for_byte(case):
    _, got = _check_case(case)
    if not case.name.startswith('coords_nonfinite') and not case.name.startswith('coords_edge_beyond'):
        assert any(np.abs(g).max() > 0 for g in got)


def test_nonfinite_boxes_scatter_nothing():
    for pool, norm in ((rg.POOL_MAX2, rg.NORM_STRIDE), (rg.POOL_AVG2, rg.NORM_TP)):
        _, got = _check_case(rg.coords_case('nonfinite', norm, pool))
        assert all((g.view(np.uint32) == 0).all() for g in got)                                # +0.0f everywhere, written


def test_sel_with_nan_bins_and_rows_beyond_the_count():
    """an all-NaN bin is code 4 and scatters nothing; a NaN upstream under an unselected sample does not enter (the add is not
    performed); dy rows at or beyond the count are ignored"""
    case = rg.mode_case(rg.NORM_STRIDE, rg.POOL_MAX2, C=4, count=9, name='sel_nan')
    maps = [m.copy() for m in case.maps()]
    maps[0][5:9, 4:8, 1] = np.nan
    maps[0][:, :, 2] = -np.abs(maps[0][:, :, 2]) - 1
    dy = case.dy()
    sel = rg.select(case, maps)
    assert (sel[:9, ..., 1] == 4).any() and (sel[9:] == 4).all()
    dy[9:] = np.nan                                             # beyond the count
    dy[:9, ..., 1][sel[:9, ..., 1] == 4] = np.nan              # under bins that select nothing
    sel_t = gpu_select(case, maps)
    _same_bits(sel_t.cpu().numpy(), sel, 'sel')
    want = rg.backward(case, dy, sel)
    assert np.isfinite(want[0]).all()
    _same_bits(gpu_backward(case, dy, sel_t)[0], want[0], 'dx')


@pytest.mark.parametrize('count', [0, 5, 40])
def test_count_dev(count):
    """0 (every dx all zeros, every sel 4), below n, above n (clamped to n)"""
    for case in (rg.mode_case(rg.NORM_STRIDE, rg.POOL_MAX2, count=count, name='count_%d' % count),
                 rg.mode_case(rg.NORM_NOPAD, rg.POOL_NONE, count=count, name='count_none_%d' % count)):
        dy = case.dy()
        dy[case.cnt:] = np.nan
        sel_t, got = _check_case(case, dy=dy)
        if count == 0:
            assert (got[0].view(np.uint32) == 0).all() and (sel_t is None or bool((sel_t == 4).all()))
        else:
            assert np.abs(got[0]).max() > 0


def test_roi_levels_clamped_and_a_level_without_rois():
    base = rg.fpn_case(8)
    lv = base.level.copy()
    lv[0], lv[-1] = -2, 9                                                 # (level-sorted rows: the first is on level 0, the last on 3)
    assert np.clip(base.level, 0, 3)[0] == 0 and np.clip(base.level, 0, 3)[-1] == 3
    low_high = rg.GradCase('fpn_levels_outside', base.norm, base.pool, 8, 7, base.rois, level=lv, count=None, maps_hw=base.maps_hw,
                           image_shape=base.image_shape)
    _, got = _check_case(low_high)                                        # outside the range: clamped, as the forward does
    assert all(np.abs(g).max() > 0 for g in got)
    lv = np.where(np.clip(base.level, 0, 3) == 2, 3, base.level)
    order = np.argsort(np.clip(lv, 0, 3), kind='stable')
    case = rg.GradCase('fpn_level2_empty', base.norm, base.pool, 8, 7, base.rois[order], level=lv[order], count=None,
                       maps_hw=base.maps_hw, image_shape=base.image_shape)
    _, got = _check_case(case)
    assert (got[2].view(np.uint32) == 0).all() and np.abs(got[3]).max() > 0   # all zeros, still written (the NaN fill is gone)


def test_two_calls_agree_and_the_roi_order_shows():
    case = rg.order_case()
    maps, dy = case.maps(), case.dy()
    sel_t, first = _check_case(case)
    again = gpu_backward(case, dy, gpu_select(case, maps))
    _same_bits(again[0], first[0], 'second call')
    # the same RoIs and upstream rows in another row order: another order of sums, other bits -- as the restatement says
    perm = np.arange(case.n)[::-1].copy()
    pc = rg.GradCase('order', case.norm, case.pool, case.C, case.P, case.rois[perm], maps_hw=case.maps_hw)
    _, permuted = _check_case(pc, maps=maps, dy=dy[perm])
    differ = int((permuted[0].view(np.uint32) != first[0].view(np.uint32)).sum())
    print('permuted RoI rows: %d of %d elements differ in bits' % (differ, first[0].size))
    assert differ >= first[0].size // 20
    np.testing.assert_allclose(permuted[0], first[0], rtol=0, atol=1e-4)
    inv = np.argsort(perm)
    back = rg.GradCase('order', case.norm, case.pool, case.C, case.P, pc.rois[inv], maps_hw=case.maps_hw)
    _same_bits(gpu_backward(back, dy[perm][inv], gpu_select(back, maps))[0], first[0], 'order restored')


@pytest.mark.parametrize('case', [rg.fpn_case(256), rg.mode_case(rg.NORM_TP, rg.POOL_AVG2), rg.mode_case(rg.NORM_STRIDE, rg.POOL_NONE)],
                         ids=lambda c: c.name)
def test_roi_pool_trainable_wiring(case):
    """the forward equals roi_pool by bytes, .backward() equals roi_pool_backward by bytes, a map that requires no gradient gets
    None, the RoIs get none"""
    ops = _ops()
    rois, level, kw = _device_args(case)
    maps = [_g(m)[None] for m in case.maps()]
    plain = ops.roi_pool(maps, rois, level, case.norm, case.P, case.pool, **kw)
    leaves = [m.clone().requires_grad_(i != 1) for i, m in enumerate(maps)]
    rois_leaf = rois.clone().requires_grad_(True)
    out = ops.roi_pool_trainable(leaves, rois_leaf, level, case.norm, case.P, case.pool, **kw)
    assert out.requires_grad and torch.equal(out, plain)
    dy = _g(case.dy())
    out.backward(dy)
    sel = ops.roi_pool_argmax(maps, rois, level, case.norm, case.P, **kw) if case.pool == rg.POOL_MAX2 else None
    want = ops.roi_pool_backward(dy, maps, rois, level, case.norm, case.P, case.pool, sel=sel, **kw)
    assert rois_leaf.grad is None
    for i, (leaf, w) in enumerate(zip(leaves, want)):
        if i == 1:
            assert leaf.grad is None
        else:
            assert torch.equal(leaf.grad, w) and leaf.grad.abs().max() > 0, i
    # the same through the functions of model/roi_pooling.py
    from tf_eager_object_detection_amd.model import roi_pooling as rp
    if len(maps) > 1:
        lv2 = [m.clone().requires_grad_(True) for m in maps]
        o2 = rp.roi_pooling_fpn_levels(lv2, rois, level, case.image_shape, case.P, count_dev=kw['count_dev'], trainable=True)
        assert torch.equal(o2, plain) and o2.requires_grad
        o2.backward(dy)
        assert all(torch.equal(a.grad, w) for a, w in zip(lv2, want))
        o3 = rp.roi_pooling_fpn_levels(lv2, rois, level, case.image_shape, case.P, count_dev=kw['count_dev'])
        assert torch.equal(o3, plain) and not o3.requires_grad                                 # (the default path, as ever)
        o4 = rp.roi_pooling_fpn_levels(maps, rois, level, case.image_shape, case.P, count_dev=kw['count_dev'], trainable=True)
        assert torch.equal(o4, plain) and not o4.requires_grad                                 # (no map asks for a gradient)


def test_layers_take_their_trainable_form_under_no_grad():
    from tf_eager_object_detection_amd.model import roi_pooling as rp
    ops = _ops()
    case = rg.mode_case(rg.NORM_STRIDE, rg.POOL_MAX2)
    fm = _g(case.maps()[0])[None]
    rois = _g(case.rois)
    dy = _g(case.dy())
    for layer_of, inputs, norm, pool, kw in (
            (lambda t: rp.RoiPoolingCropAndResize(7, True, trainable=t), lambda m: (m, rois, 16), rg.NORM_STRIDE, rg.POOL_MAX2, dict(strides=[16.0])),
            (lambda t: rp.RoiPoolingCropAndResize(7, False, trainable=t), lambda m: (m, rois, 16), rg.NORM_STRIDE, rg.POOL_NONE, dict(strides=[16.0])),
            (lambda t: rp.RoiPoolingCropAndResize2(7, trainable=t), lambda m: (m, rois, [256, 256]), rg.NORM_IMAGE, rg.POOL_MAX2, dict(image_shape=(256, 256))),
            (lambda t: rp.RoiPoolingRoiAlign(7, trainable=t), lambda m: (m, rois, 16), rg.NORM_TP, rg.POOL_AVG2, dict(strides=[16.0]))):
        leaf = fm.clone().requires_grad_(True)
        plain = layer_of(False)(inputs(leaf))
        assert not plain.requires_grad
        with torch.no_grad():                                   # (the caller's grad mode does not matter)
            out = layer_of(True)(inputs(leaf))
        assert out.requires_grad and torch.equal(out, plain)
        out.backward(dy)
        sel = ops.roi_pool_argmax([fm], rois, None, norm, 7, **kw) if pool == rg.POOL_MAX2 else None
        want = ops.roi_pool_backward(dy, [fm], rois, None, norm, 7, pool, sel=sel, **kw)[0]
        assert torch.equal(leaf.grad, want)
        assert not layer_of(True)(inputs(fm)).requires_grad
    leaf = fm.clone().requires_grad_(True)
    boxes = rois / 16.0
    for fn, pool, P in ((lambda **k: rp.crop_and_resize(leaf, boxes, None, 7, **k), rg.POOL_NONE, 7), (lambda **k: rp.roi_align(leaf, boxes, 7, **k), rg.POOL_AVG2, 7)):
        leaf.grad = None
        out = fn(trainable=True)
        assert out.requires_grad and torch.equal(out, fn()) and not fn().requires_grad
        out.backward(dy)
        want = ops.roi_pool_backward(dy, [fm], boxes, None, rg.NORM_TP, P, pool, strides=[1.0])[0]
        assert torch.equal(leaf.grad, want)


def _level_rois(shape):
    """RoIs for P2 .. P5 of an image, a few per level, some crossing the image border"""
    h, w = shape
    rng = np.random.default_rng(5)
    out = []
    for k, size in enumerate((0.2, 0.35, 0.6, 0.9)):
        n = 4 - (k == 3)
        cx, cy = rng.uniform(0.2, 0.8, n) * w, rng.uniform(0.2, 0.8, n) * h
        bw, bh = size * w * rng.uniform(0.8, 1.2, n), size * h * rng.uniform(0.8, 1.2, n)
        out.append(np.stack([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], axis=1).astype(np.float32))
    return out


def test_caller_model_carries_the_gradient_into_the_maps():
    """ResnetV1Fpn(train_roi_head=True)._training_roi_head with p_list leaves that require a gradient: (cls + reg).backward()
    leaves .grad on every pooled map, equal by bytes to the kernels called by hand on fc1's dense_dgrad output; with plain maps
    the result and the graph are as before"""
    from tf_eager_object_detection_amd.model.base_fpn_model import ResnetV1Fpn
    ops = _ops()
    shape = (128, 128)
    torch.manual_seed(4)
    m = ResnetV1Fpn(depth=50, train_roi_head=True)
    g = torch.Generator().manual_seed(6)
    plain_maps = [torch.randn((1, 256, shape[0] // s, shape[1] // s), generator=g).cuda().contiguous(memory_format=torch.channels_last)
                  for s in (4, 8, 16, 32, 64)]
    rois_list = [_g(r) for r in _level_rois(shape)]
    seen = {}
    head = m._get_trainable_roi_head()

    def spy(feats):
        seen['feats'] = feats
        if feats.requires_grad:
            feats.register_hook(lambda gr: seen.__setitem__('dfeats', gr.clone()))
        return head(feats)
    m._get_trainable_roi_head = lambda: spy
    s0, d0 = m._training_roi_head(rois_list, plain_maps, list(shape), True)
    assert not seen['feats'].requires_grad and s0.requires_grad                  # as today: only the head carries a graph
    (s0.sum() + d0.sum()).backward()
    assert all(p.grad is None for p in plain_maps)
    m.dense.zero_grad(set_to_none=True)
    leaves = [p.clone().requires_grad_(True) for p in plain_maps]
    s1, d1 = m._training_roi_head(rois_list, leaves, list(shape), True)
    assert seen['feats'].requires_grad and torch.equal(s1, s0) and torch.equal(d1, d0)
    rng = np.random.default_rng(7)
    ws, wd = _g(rng.standard_normal(tuple(s1.shape)).astype(np.float32)), _g(rng.standard_normal(tuple(d1.shape)).astype(np.float32))
    ((s1 * ws).sum() + (d1 * wd).sum()).backward()
    assert leaves[4].grad is None                                                # (P6 is not pooled)
    dfeats = seen['dfeats'].contiguous()
    assert tuple(dfeats.shape) == (15, 7, 7, 256) and dfeats.abs().max() > 0
    nhwc = [p.permute(0, 2, 3, 1).contiguous() for p in plain_maps[:4]]
    off = 0
    for l, rois in enumerate(rois_list):
        k = int(rois.shape[0])
        dy = dfeats[off:off + k].contiguous()
        off += k
        sel = ops.roi_pool_argmax([nhwc[l]], rois, None, ops.ROI_NORM_IMAGE, 7, image_shape=shape)
        want = ops.roi_pool_backward(dy, [nhwc[l]], rois, None, ops.ROI_NORM_IMAGE, 7, ops.ROI_POOL_MAX2, image_shape=shape, sel=sel)[0]
        got = leaves[l].grad.permute(0, 2, 3, 1)
        assert torch.equal(got, want) and want.abs().max() > 0, l
    # ... and the same bits from ONE launch over the level-sorted RoIs
    level = torch.cat([torch.full((int(r.shape[0]),), l, dtype=torch.int32, device='cuda') for l, r in enumerate(rois_list)])
    allr = torch.cat(rois_list)
    sel = ops.roi_pool_argmax(nhwc, allr, level, ops.ROI_NORM_IMAGE, 7, image_shape=shape)
    for l, w in enumerate(ops.roi_pool_backward(dfeats, nhwc, allr, level, ops.ROI_NORM_IMAGE, 7, ops.ROI_POOL_MAX2, image_shape=shape, sel=sel)):
        assert torch.equal(leaves[l].grad.permute(0, 2, 3, 1), w), l
    assert m.dense.fc1.weight.grad is not None


def test_end_to_end_backward_into_the_extractor():
    """maps from the plain-torch formulation of the dense part (tests/torch_reference.fpn_features) on a detector whose parameters
    require a gradient -> trainable pooling -> roi_head_trainable -> a scalar loss -> backward(): conv1's and a neck layer's
    weights get finite, non-zero gradients.

    The comparison is made on dx of the maps, which the per-cell bound of test_roi_grad_host covers directly (a bound carried
    through torch's convolution backward was not derived): each element of every map's gradient lies within
    (count + 4) * 2^-24 * sum|contributions| of the float64 autograd of the torch restatement with sel imposed, fed the same
    upstream gradient -- and equals the NumPy restatement by bytes."""
    import torch_reference as tr
    from tf_eager_object_detection_amd.model import roi_pooling as rp
    from tf_eager_object_detection_amd.model.fpn_detector import ResNetFpnDetector
    shape = (64, 64)
    torch.manual_seed(8)
    det = ResNetFpnDetector(50, 21, shape, 1, dtype=torch.float32).to(device='cuda', dtype=torch.float32).eval()
    for p in det.parameters():
        p.requires_grad_(True)
    rng = np.random.default_rng(9)
    img = _g((rng.uniform(0, 255, (1,) + shape + (3,)) - 110).astype(np.float32))
    maps = [p.permute(0, 2, 3, 1).contiguous() for p in tr.fpn_features(det, img)[:4]]
    for mp in maps:
        mp.retain_grad()
    per_level = _level_rois(shape)
    rois = np.concatenate(per_level)
    level = np.concatenate([np.full(len(r), l, np.int32) for l, r in enumerate(per_level)])
    feats = rp.roi_pooling_fpn_levels(maps, _g(rois), _g(level), shape, 7, trainable=True)
    seen = {}
    feats.register_hook(lambda gr: seen.__setitem__('dfeats', gr.clone()))
    s, d = det.roi_head_trainable(feats)
    ws, wd = _g(rng.standard_normal(tuple(s.shape)).astype(np.float32)), _g(rng.standard_normal(tuple(d.shape)).astype(np.float32))
    ((s * ws).sum() + (d * wd).sum()).backward()
    for name in ('conv1.weight', 'l2.weight', 's2.weight', 'p5.weight'):
        gr = dict(det.named_parameters())[name].grad
        assert gr is not None and bool(torch.isfinite(gr).all()) and float(gr.abs().max()) > 0, name
    case = rg.GradCase('e2e', rg.NORM_IMAGE, rg.POOL_MAX2, 256, 7, rois, level=level, maps_hw=[tuple(mp.shape[1:3]) for mp in maps],
                       image_shape=shape)
    np_maps = [mp.detach()[0].cpu().numpy() for mp in maps]
    dy = seen['dfeats'].cpu().numpy()
    sel = rg.select(case, np_maps)
    want32, num, mag = rg.backward(case, dy, sel, stats=True)
    want64 = rg.torch_backward(case, np_maps, dy, sel)
    for l, mp in enumerate(maps):
        got = mp.grad[0].cpu().numpy()
        _same_bits(got, want32[l], 'dx level %d' % l)
        bound = (num[l] + 4) * 2.0 ** -24 * mag[l]
        err = np.abs(got.astype(np.float64) - want64[l])
        assert (err <= bound).all(), (l, float((err - bound).max()))
        assert np.abs(got).max() > 0


def test_graph_capture_replays_bit_equal_to_eager():
    """forward + select + backward captured once, replayed on new map, RoI and upstream contents"""
    ops = _ops()
    case = rg.fpn_case(256)
    rois, level, kw = _device_args(case)
    maps = [_g(m)[None] for m in case.maps()]
    dy = _g(case.dy())
    feats = torch.empty((case.n, 7, 7, 256), device='cuda')
    sel = torch.empty((case.n, 7, 7, 256), dtype=torch.uint8, device='cuda')
    dxs = [torch.empty_like(m) for m in maps]

    def step():
        ops.roi_pool(maps, rois, level, case.norm, 7, case.pool, out=feats, **kw)
        ops.roi_pool_argmax(maps, rois, level, case.norm, 7, out=sel, **kw)
        ops.roi_pool_backward(dy, None, rois, level, case.norm, 7, case.pool, sel=sel, outs=dxs, **kw)
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
    for t in maps + [dy]:
        t.copy_(_g(rng.standard_normal(tuple(t.shape)).astype(np.float32)))
    rois.copy_(rois.flip(0))
    for t in dxs + [feats]:
        t.fill_(float('nan'))
    sel.fill_(255)
    graph.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in [feats, sel] + dxs]
    step()
    torch.cuda.synchronize()
    for a, b in zip(got, [feats, sel] + dxs):
        assert torch.equal(a, b)
    assert bool(torch.isfinite(feats).all()) and all(bool(torch.isfinite(t).all()) for t in dxs) and int(sel.max()) <= 4
