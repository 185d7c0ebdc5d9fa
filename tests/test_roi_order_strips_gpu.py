"""The strip order of the RoIs on the GPU: the stand-alone producer (ops.roi_order) and the fused one (tail of the NMS walk,
FpnStepBatch) against the host restatement of d_roi_order_bucket (tools/roi_order_model.bucket_strips).

Image 128 x 192, two levels (maps 32 x 48 and 16 x 24, C = 256), K = 96 RoIs.  The prescribed RoIs have integer corners whose
centres keep half a pixel from every strip boundary (x = multiples of 24) and every bin boundary (y = multiples of 4); the
host restatement does the device's float32 operations, so the buckets of the proposal stage's own RoIs agree as well."""
import numpy as np
import pytest

from tools import roi_order_model as m

SHAPE = (128, 192)
K = 96
C = 256
NL = 2


def _host_buckets(rois, levels):
    return m.bucket_strips(np.asarray(rois, np.float32), np.asarray(levels, np.int64), SHAPE)


def _off_boundaries(rois):
    cx2 = rois[:, 0] + rois[:, 2]                     # twice the centre: strip boundaries at cx = 24 k, bins at cy = 4 j
    cy2 = rois[:, 1] + rois[:, 3]
    return np.all(cx2 % 48 != 0) and np.all(cy2 % 8 != 0)


def _prescribed(seed=5):
    """K level-sorted RoIs with integer corners, 64 on level 0 and 32 on level 1, centres off every boundary"""
    rng = np.random.default_rng(seed)
    x0 = rng.integers(0, 150, K)
    y0 = rng.integers(0, 90, K)
    x1 = x0 + rng.integers(6, 41, K)
    y1 = y0 + rng.integers(6, 37, K)
    x1 = np.where((x0 + x1) % 48 == 0, x1 + 1, x1)
    y1 = np.where((y0 + y1) % 8 == 0, y1 + 1, y1)
    rois = np.stack([x0, y0, x1, y1], 1).astype(np.float32)
    levels = np.repeat([0, 1], [64, 32]).astype(np.int32)
    assert _off_boundaries(rois) and rois[:, 2].max() <= SHAPE[1] - 1 and rois[:, 3].max() <= SHAPE[0] - 1
    return rois, levels


def _check_order(order, rois, levels, count, what):
    """a permutation, padded rows last (in row order), host buckets non-decreasing along the valid part -> buckets"""
    n = len(rois)
    order = np.asarray(order)[:n]
    np.testing.assert_array_equal(np.sort(order), np.arange(n), err_msg='%s: not a permutation' % what)
    np.testing.assert_array_equal(order[count:], np.arange(count, n), err_msg='%s: padded rows not last' % what)
    b = _host_buckets(rois, levels)
    along = b[order[:count]]
    assert np.all(np.diff(along) >= 0), '%s: buckets decrease along the order: %s' % (what, along.tolist())
    return b


def _rows_per_bucket(order, buckets, count):
    out = {}
    for r in np.asarray(order)[:count].tolist():
        out.setdefault(int(buckets[r]), []).append(r)
    return {k: sorted(v) for k, v in out.items()}


def _standalone(rois, levels, count=None):
    import torch
    from tf_eager_object_detection_amd import ops
    dev = torch.device('cuda')
    cd = torch.tensor([count], dtype=torch.int32, device=dev) if count is not None else None
    lv = torch.from_numpy(np.asarray(levels, np.int32)).to(dev) if levels is not None else None
    o = ops.roi_order(torch.from_numpy(np.ascontiguousarray(rois, np.float32)).to(dev), lv, SHAPE, count_dev=cd)
    torch.cuda.synchronize()
    return o.cpu().numpy()


def _expected_standalone(rois, levels, count):
    """the stand-alone key: (bucket, qy, qx, row), padded rows behind"""
    n = len(rois)
    b = _host_buckets(rois, levels)
    qy, qx = m.quantise(rois, SHAPE)
    valid = np.lexsort((np.arange(count), qx[:count], qy[:count], b[:count]))
    return np.concatenate([valid, np.arange(count, n)])


@pytest.mark.gpu
@pytest.mark.parametrize('count', [K, 80])
def test_standalone_order(count):
    rois, levels = _prescribed()
    got = _standalone(rois, levels, count)
    _check_order(got, rois, levels, count, 'ops.roi_order')
    np.testing.assert_array_equal(got, _expected_standalone(rois, levels, count))


def _fused_inputs(image, rng):
    """image 0: distinct scores, small deltas (K proposals from the first candidates).  image 1: 40 anchors with the top scores
    and zero deltas, every other anchor decodes to the whole image (one survivor): fewer than K proposals, and only once
    every anchor has been visited"""
    from tf_eager_object_detection_amd import synthetic as syn
    n = syn.num_fpn_anchors(SHAPE, (4, 8), 3)
    prob = syn.scores_distinct(n, rng)
    deltas = syn.rpn_deltas(n, rng, 0.1)
    if image == 1:
        top = np.argsort(-prob)[:40]
        special = rng.choice(32 * 48 * 3, 40, replace=False)      # (anchors of the first level)
        other = np.setdiff1d(np.arange(n), special)
        p2 = np.empty_like(prob)
        p2[special] = prob[top]
        p2[other] = np.sort(prob)[:len(other)][rng.permutation(len(other))]
        prob = p2
        deltas[:] = np.float32([0, 0, 5, 5])
        deltas[special] = 0
    return syn.logits_from_prob(prob), deltas


@pytest.fixture(scope='module')
def fused():
    """both plans of the proposal stage, B = 2 -> {plan: [per image dict(rois, levels, count, done, order)]}
    'lds'   : first chunk of the default size (k_nms_scan<true>), one sync-free chunk: image 1 is reported empty
    'chunks': first chunk of 4096 candidates + a second one (k_nms_scan<false>): image 1 completes with count < K"""
    import torch
    from tf_eager_object_detection_amd import synthetic as syn
    from tf_eager_object_detection_amd.pipeline import FpnStepBatch
    dev = torch.device('cuda')
    rng = np.random.default_rng(11)
    inputs = [_fused_inputs(b, rng) for b in range(2)]
    maps = [torch.zeros((1, h, w, C), device=dev) for h, w in syn.fpn_level_shapes(SHAPE, (4, 8))]
    cls_s = torch.zeros((K, 3), device=dev)
    cls_d = torch.zeros((K, 3, 4), device=dev)
    out = {}
    for plan, kw in (('lds', dict(blind_chunks=1)), ('chunks', dict(blind_chunks=2, nms_first_chunk=4096))):
        sb = FpnStepBatch(2, SHAPE, 3, K, C, min_level=2, max_level=3, strides=(4, 8), base_sizes=(32, 128), **kw)
        keep = []
        for b, (lg, dl) in enumerate(inputs):
            t = (torch.from_numpy(lg).to(dev), torch.from_numpy(dl).to(dev))
            keep.append(t)
            sb.bind(b, t[0], t[1], maps, cls_s, cls_d)
        sb.enqueue(FpnStepBatch.STAGE_PROPOSALS, 2)
        torch.cuda.synchronize()
        out[plan] = [dict(rois=h.sorted_rois.cpu().numpy(), levels=h.roi_level.cpu().numpy(), count=int(h.roi_count.item()),
                          done=int(h.nms_done.item()), order=h.roi_order.cpu().numpy()) for h in sb.slots]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('plan', ['lds', 'chunks'])
def test_fused_order_and_its_buckets_match_the_standalone(fused, plan):
    img0, img1 = fused[plan]
    assert img0['done'] == 1 and img0['count'] == K
    if plan == 'lds':
        assert img1['done'] == 0 and img1['count'] == 0          # (incomplete inside its one chunk: reported empty)
    else:
        assert img1['done'] == 1 and 1 < img1['count'] < K
    for b, im in enumerate((img0, img1)):
        what = 'fused order, plan %s, image %d (count %d)' % (plan, b, im['count'])
        cnt = im['count']
        assert set(im['levels'][:cnt].tolist()) <= {0, 1}
        buckets = _check_order(im['order'], im['rois'], im['levels'], cnt, what)
        alone = _standalone(im['rois'], im['levels'], cnt)
        _check_order(alone, im['rois'], im['levels'], cnt, what + ' / ops.roi_order on the same RoIs')
        assert _rows_per_bucket(im['order'], buckets, cnt) == _rows_per_bucket(alone, buckets, cnt), what
    assert len(set(img0['levels'].tolist())) == 2                 # (both levels' tables were used)


@pytest.mark.gpu
def test_pooling_does_not_depend_on_the_order():
    import torch
    from tf_eager_object_detection_amd import ops
    dev = torch.device('cuda')
    rois, levels = _prescribed()
    g = torch.Generator(device='cuda')
    g.manual_seed(3)
    maps = [torch.randn((1, 32, 48, C), device=dev, generator=g), torch.randn((1, 16, 24, C), device=dev, generator=g)]
    r, lv = torch.from_numpy(rois).to(dev), torch.from_numpy(levels).to(dev)
    order = ops.roi_order(r, lv, SHAPE)
    kw = dict(image_shape=SHAPE)
    a = ops.roi_pool(maps, r, lv, ops.ROI_NORM_IMAGE, 7, ops.ROI_POOL_MAX2, order=order, **kw)
    b = ops.roi_pool(maps, r, lv, ops.ROI_NORM_IMAGE, 7, ops.ROI_POOL_MAX2, order=None, **kw)
    torch.cuda.synchronize()
    assert a.abs().sum().item() > 0
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def _edge_cases():
    one_bucket = np.float32([[50 + i, 40, 60 + i, 42] for i in (0, 2, 4, 1, 3)])          # strip 2 (even), bin 10
    assert len(set(_host_buckets(one_bucket, np.zeros(5)).tolist())) == 1
    per_strip = np.float32([[24 * s + 8, 10 + 4 * s, 24 * s + 14, 13 + 4 * s] for s in range(8)][::-1])   # one RoI per strip
    odd_even = np.float32([[30, 100, 40, 105], [30, 10, 40, 15], [4, 100, 14, 105], [4, 10, 14, 15]])      # strip 1 (up), strip 0 (down)
    edge = np.float32([[180, 116, 204, 140], [192, 10, 192, 13], [10, 128, 13, 128], [3, 5, 9, 7]])   # centres on the right / bottom edge
    return [('one_bucket', one_bucket, np.zeros(5, np.int32)), ('n1', np.float32([[3, 5, 9, 7]]), np.zeros(1, np.int32)),
            ('n1_no_levels', np.float32([[3, 5, 9, 7]]), None), ('one_per_strip', per_strip, np.ones(8, np.int32)),
            ('odd_and_even_strip', odd_even, np.zeros(4, np.int32)), ('edge_centres', edge, np.zeros(4, np.int32))]


@pytest.mark.gpu
@pytest.mark.parametrize('name', [c[0] for c in _edge_cases()])
def test_edge_inputs(name):
    _, rois, levels = [c for c in _edge_cases() if c[0] == name][0]
    n = len(rois)
    host_levels = np.zeros(n, np.int32) if levels is None else levels
    got = _standalone(rois, levels)
    b = _check_order(got, rois, host_levels, n, name)
    np.testing.assert_array_equal(got, _expected_standalone(rois, host_levels, n))
    if name == 'one_per_strip':
        np.testing.assert_array_equal(got, np.arange(8)[::-1])    # strips left to right = the rows reversed
    if name == 'odd_and_even_strip':
        np.testing.assert_array_equal(got, [3, 2, 0, 1])          # strip 0 top then bottom, strip 1 bottom then top
    if name == 'edge_centres':
        qy, qx = m.quantise(rois, SHAPE)
        assert qx[0] == 4095 and qy[0] == 4095 and qx[1] == 4095 and qy[2] == 4095
        assert b[0] == 7 * 32 + 0                                # last strip (odd): the bottom bin comes first
