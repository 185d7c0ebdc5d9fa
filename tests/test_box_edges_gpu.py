"""The box primitives of csrc/boxes.hip against the statement of tests/box_edge_cases.py, on its edge-value tables and through
every launch path: 0 ulp, 1 ulp behind exp / log, NaN at the same positions (`ec.same`).  The declared properties (DESIGN.md
"Box primitives: declared behaviour") are asserted again on what the kernels return.  ops.* where it reaches the path; the C ABI
(`_lib`) for delta strides, pre-filled outputs and the error returns."""
import ctypes as C

import numpy as np
import pytest

import box_edge_cases as ec

pytestmark = pytest.mark.gpu

H, W = ec.IMAGE
E_INVALID, E_WORKSPACE, E_LIMIT = -1, -2, -4            # include/odet.h


@pytest.fixture(scope='module')
def gpu():
    import torch
    from tf_eager_object_detection_amd import _lib, ops
    _lib.lib()

    class G:
        pass
    G.torch, G.L, G.ops = torch, _lib, ops
    G.up = staticmethod(lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda())
    G.down = staticmethod(lambda t: t.detach().cpu().numpy())
    return G


def _padded(n):
    """the table as it is, and cycled (or cut) to 255, 256 and 257 rows and to one row below, onto and one row above its own
    next multiple of the 256-thread block"""
    r = 256 * -(-n // 256)
    return sorted({n, 255, 256, 257, r - 1, r, r + 1})


def _cycle(a, n):
    return np.ascontiguousarray(a[np.arange(n) % len(a)])


def _last_error(gpu):
    return gpu.L.lib().odet_last_error().decode()


# ---- decode / encode / clip -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('setting', range(len(ec.DECODE_SETTINGS)))
def test_decode_table(gpu, setting):
    means, stds, clip_shape = ec.DECODE_SETTINGS[setting]
    anchors, deltas = ec.decode_table()
    for n in _padded(len(anchors)):
        a, d = _cycle(anchors, n), _cycle(deltas, n)
        got = gpu.down(gpu.ops.decode(gpu.up(a), gpu.up(d), means, stds, clip_shape=clip_shape))
        ec.same(got, ec.decode(a, d, means, stds, clip_shape), 1, 'decode %s n=%d' % (ec.DECODE_SETTINGS[setting], n))
        if clip_shape is not None:                           # no NaN from decode survives the fused clip
            assert not np.isnan(got).any() and got.min() >= 0
            assert got[:, 0::2].max() <= W - 1 and got[:, 1::2].max() <= H - 1


def _decode_strided(gpu, anchors, deltas, stride, column, means, stds, clip_shape):
    """odet_decode reading `deltas` as columns column .. column + 3 of an [n, stride] array"""
    n = len(anchors)
    rng = np.random.default_rng(41)
    wide = rng.normal(0, 1, (n, stride)).astype(np.float32)
    wide[:, column:column + 4] = deltas
    buf = gpu.up(wide)
    out = gpu.torch.full((n, 4), float('nan'), dtype=gpu.torch.float32, device='cuda')
    ch, cw = (0, 0) if clip_shape is None else clip_shape
    L = gpu.L
    dev_anchors = gpu.up(anchors)
    rc = L.lib().odet_decode(L.dptr(dev_anchors), C.c_void_p(buf.data_ptr() + 4 * column), stride, n, L.host4(means, 'means'),
                             L.host4(stds, 'stds'), ch, cw, L.dptr(out), L.stream())
    assert rc == 0, _last_error(gpu)
    assert (buf.data_ptr() + 4 * column) % 16 == (4 * column) % 16
    return gpu.down(out)


@pytest.mark.parametrize('stride,column,path', [(84, 20, 'float4'), (6, 1, 'scalar'), (5, 0, 'scalar'), (5, 1, 'scalar'),
                                                (8, 1, 'scalar: rows off the 16-byte grid'), (8, 4, 'float4')])
def test_decode_delta_strides(gpu, stride, column, path):
    """k_decode's two load paths: one float4 per row where the stride is a multiple of 4 AND the pointer is 16-byte aligned
    (column block 5 of an [n, 84] class-delta array), four scalar loads otherwise -- a stride of 8 from `deltas + 1` included,
    which has to give what the contiguous call gives"""
    anchors, deltas = ec.decode_table()
    for n in (len(anchors), 257):
        a, d = _cycle(anchors, n), _cycle(deltas, n)
        for means, stds, clip_shape in (ec.DECODE_SETTINGS[1], ec.DECODE_SETTINGS[2]):
            got = _decode_strided(gpu, a, d, stride, column, means, stds, clip_shape)
            ec.same(got, ec.decode(a, d, means, stds, clip_shape), 1, 'decode stride %d column %d (%s)' % (stride, column, path))
            contiguous = gpu.down(gpu.ops.decode(gpu.up(a), gpu.up(d), means, stds, clip_shape=clip_shape))
            nan = np.isnan(contiguous)
            assert np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan], contiguous[~nan])


@pytest.mark.parametrize('setting', range(len(ec.ENCODE_SETTINGS)))
def test_encode_table(gpu, setting):
    means, stds = ec.ENCODE_SETTINGS[setting]
    src, gt = ec.encode_table()
    for n in _padded(len(src)):
        s, g = _cycle(src, n), _cycle(gt, n)
        got = gpu.down(gpu.ops.encode(gpu.up(s), gpu.up(g), means, stds))
        ec.same(got, ec.encode(s, g, means, stds), 1, 'encode %s n=%d' % (ec.ENCODE_SETTINGS[setting], n))


@pytest.mark.parametrize('min_value', ec.CLIP_SETTINGS)
def test_clip_table(gpu, min_value):
    boxes = ec.clip_table()
    for n in _padded(len(boxes)):
        b = _cycle(boxes, n)
        got = gpu.down(gpu.ops.clip(gpu.up(b), min_value, H, W))
        ec.same(got, ec.clip(b, min_value, H, W), 0, 'clip min_value %g n=%d' % (min_value, n))
        assert not np.isnan(got).any()                      # the property: a NaN corner becomes the image border
        assert (got >= np.float32(min_value)).all() and got[:, 0::2].max() <= W - 1 and got[:, 1::2].max() <= H - 1


# ---- the filters and where_greater ------------------------------------------------------------------------------------------
def _kept(gpu, idx, cnt, n):
    k = int(cnt.item())
    assert 0 <= k <= n
    return gpu.down(idx[:k])


@pytest.mark.parametrize('min_value,min_edge', ec.FILTER_SETTINGS)
def test_filters_on_the_clip_table(gpu, min_value, min_edge):
    boxes = ec.clip_table()
    for n in _padded(len(boxes)):
        b = _cycle(boxes, n)
        ob, oi, cnt = gpu.ops.clip_filter(gpu.up(b), min_value, H, W, min_edge)
        wb, wi = ec.clip_filter(b, min_value, H, W, min_edge)
        ec.same(_kept(gpu, oi, cnt, n), wi, 0, 'clip_filter indices n=%d' % n)
        ec.same(gpu.down(ob[:len(wi)]), wb, 0, 'clip_filter boxes n=%d' % n)
        assert not np.isnan(gpu.down(ob[:len(wi)])).any()
        oi, cnt = gpu.ops.range_filter(gpu.up(b), H, W)
        ec.same(_kept(gpu, oi, cnt, n), ec.range_filter(b, H, W), 0, 'range_filter n=%d' % n)


@pytest.mark.parametrize('n,kind', ec.compact_cases(), ids=lambda v: str(v))
def test_compaction_patterns(gpu, n, kind):
    """the three launches of run_compact at every tile count and keep pattern; the large case has 1026 tiles, so each thread
    of k_cp_scan's one workgroup scans two of them"""
    mask = ec.keep_mask(n, kind)
    want = np.nonzero(mask)[0]
    oi, cnt = gpu.ops.where_greater(gpu.up(ec.mask_values(mask)), 0.5)
    ec.same(_kept(gpu, oi, cnt, n), want, 0, 'where_greater')
    b = ec.mask_boxes(mask, 'clip_filter')
    ob, oi, cnt = gpu.ops.clip_filter(gpu.up(b), 0, H, W, ec.MIN_EDGE)
    ec.same(_kept(gpu, oi, cnt, n), want, 0, 'clip_filter indices')
    ec.same(gpu.down(ob[:len(want)]), b[want], 0, 'clip_filter boxes')
    oi, cnt = gpu.ops.range_filter(gpu.up(ec.mask_boxes(mask, 'range_filter')), H, W)
    ec.same(_kept(gpu, oi, cnt, n), want, 0, 'range_filter')


def test_where_greater_strided_column(gpu):
    for n in (1, 1025, 4 * 1024 + 3):
        mask = ec.keep_mask(n, 'alternating') | ec.keep_mask(n, 'last')
        table = np.random.default_rng(42).uniform(0.6, 2.0, (n, 21)).astype(np.float32)     # every other column: all kept
        table[:, 5] = ec.mask_values(mask)
        col = gpu.up(table)[:, 5]
        assert n == 1 or col.stride(0) == 21
        oi, cnt = gpu.ops.where_greater(col, 0.5)
        ec.same(_kept(gpu, oi, cnt, n), np.nonzero(mask)[0], 0, 'where_greater, stride 21, n=%d' % n)


@pytest.mark.parametrize('threshold', ec.WHERE_THRESHOLDS, ids=lambda t: repr(float(t)))
def test_where_greater_values_and_thresholds(gpu, threshold):
    """strict >: a value equal to the threshold is dropped; a NaN value or a NaN threshold keeps nothing; +-inf as a threshold"""
    v = ec.where_values()
    for vals in (v, _cycle(v, 1025)):
        oi, cnt = gpu.ops.where_greater(gpu.up(vals), threshold)
        ec.same(_kept(gpu, oi, cnt, len(vals)), ec.where_greater(vals, threshold), 0, 'where_greater thr %r' % threshold)


# ---- pairwise IoU -----------------------------------------------------------------------------------------------------------
def _iou_property(got, b1, b2):
    nan_in = ec.has_nan(b1)[:, None] | ec.has_nan(b2)[None, :]
    assert (np.isnan(got[nan_in]) | (got[nan_in] == 0)).all(), 'a positive IoU from a box with a NaN corner'


def test_iou_table(gpu):
    t = ec.iou_boxes()
    got = gpu.down(gpu.ops.pairwise_iou(gpu.up(t), gpu.up(t)))
    ec.same(got, ec.pairwise_iou(t, t), 0, 'IoU table')
    _iou_property(got, t, t)


@pytest.mark.parametrize('n,m', ec.IOU_SIZES)
def test_iou_sizes(gpu, n, m):
    b1, b2 = ec.iou_operands(n, m)
    got = gpu.down(gpu.ops.pairwise_iou(gpu.up(b1), gpu.up(b2)))
    ec.same(got, ec.pairwise_iou(b1, b2), 0, 'IoU %d x %d' % (n, m))
    _iou_property(got, b1, b2)


def test_iou_at_the_column_limit(gpu):
    m = ec.IOU_MAX_COLUMNS
    b1, b2 = ec.iou_wide(m)
    got = gpu.down(gpu.ops.pairwise_iou(gpu.up(b1), gpu.up(b2)))
    ec.same(got, ec.pairwise_iou(b1, b2), 0, 'IoU 1 x %d' % m)
    _iou_property(got, b1, b2)


def test_iou_one_column_beyond_the_limit(gpu):
    m = ec.IOU_MAX_COLUMNS + 1
    b1, b2 = ec.iou_wide(m)
    out = gpu.torch.full((1, m), float('nan'), dtype=gpu.torch.float32, device='cuda')
    L = gpu.L
    d1, d2 = gpu.up(b1), gpu.up(b2)
    rc = L.lib().odet_pairwise_iou(L.dptr(d1), 1, L.dptr(d2), m, L.dptr(out), L.stream())
    assert rc == E_INVALID and 'm too large' in _last_error(gpu)
    gpu.torch.cuda.synchronize()
    assert bool(gpu.torch.isnan(out).all())                 # nothing was launched


# ---- assign_levels ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('min_level,max_level', ec.LEVEL_RANGES)
def test_assign_levels_sweep(gpu, min_level, max_level):
    rois, _ = ec.level_sweep()
    for n in (len(rois), 1025, 1):
        r = rois[:n]
        srois, lv, perm, counts = (gpu.down(t) for t in gpu.ops.assign_levels(gpu.up(r), min_level, max_level))
        wr, wl, wp, wc = ec.assign_levels(r, min_level, max_level)
        # every RoI has exactly one level
        assert counts.sum() == n and np.array_equal(np.sort(perm), np.arange(n))
        wrong = np.nonzero(lv[np.argsort(perm)] != ec.roi_levels(r, min_level, max_level))[0]
        assert not len(wrong), '%d RoIs at another level, first: %r' % (len(wrong), r[wrong[0]].tolist())
        ec.same(counts, wc, 0, 'counts')
        ec.same(perm, wp, 0, 'perm')
        ec.same(lv, wl, 0, 'levels')
        assert np.array_equal(srois.view(np.uint32), wr.view(np.uint32))


def test_assign_levels_count_on_device(gpu):
    rois, _ = ec.level_sweep()
    rois = rois[:3000]
    for count in (0, 1, 2999, 3000, 3007):
        k = min(count, len(rois))
        cd = gpu.torch.tensor([count], dtype=gpu.torch.int32, device='cuda')
        srois, lv, perm, counts = (gpu.down(t) for t in gpu.ops.assign_levels(gpu.up(rois), 2, 5, count_dev=cd))
        wr, wl, wp, wc = ec.assign_levels(rois[:k], 2, 5)
        ec.same(counts, wc, 0, 'counts, count %d' % count)
        ec.same(perm[:k], wp, 0, 'perm, count %d' % count)
        ec.same(lv[:k], wl, 0, 'levels, count %d' % count)


# ---- gather_rows ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ec.gather_cases(), ids=lambda c: '%dx%d-n%d-%s-%s-count%s' % (c[0], c[1], c[2], c[3], c[4].__name__, c[5]))
def test_gather_rows(gpu, case):
    """odet_gather_rows into an output pre-filled with NaN: min(count, n) rows are written, every row from there on stays as it
    was.  The index and output buffers hold GATHER_SPARE valid entries / rows beyond n, so that a count above n has somewhere
    to go if the clamp to n were missing."""
    rows, rf, n, kind, dtype, count = case
    L, torch = gpu.L, gpu.torch
    src = np.random.default_rng(43).normal(0, 1, (rows, rf)).astype(np.float32)
    idx = ec.gather_indices(n, rows, kind).astype(dtype)
    out = torch.full((n + ec.GATHER_SPARE, rf), float('nan'), dtype=torch.float32, device='cuda')
    cd = None if count is None else torch.tensor([count], dtype=torch.int32, device='cuda')
    dev_src, dev_idx = gpu.up(src), gpu.up(idx)
    rc = L.lib().odet_gather_rows(L.dptr(dev_src), L.dptr(dev_idx), 1 if dtype == np.int64 else 0, n, L.dptr(cd), rf,
                                  L.dptr(out), L.stream())
    assert rc == 0, _last_error(gpu)
    got = gpu.down(out)
    want = ec.gather_rows(src, idx[:n], count)
    k = len(want)
    assert k == (n if count is None else min(count, n))
    assert np.array_equal(got[:k].view(np.uint32), want.view(np.uint32))
    assert np.isnan(got[k:]).all(), 'rows at or beyond the count were written'
    if count is None and rf == 4:                            # and the front end
        via_ops = gpu.down(gpu.ops.gather_rows(gpu.up(src), gpu.up(idx[:n])))
        assert np.array_equal(via_ops.view(np.uint32), want.view(np.uint32))


# ---- error returns ----------------------------------------------------------------------------------------------------------
def test_error_returns(gpu):
    L, torch = gpu.L, gpu.torch
    lib = L.lib()
    nan4 = lambda n: torch.full((n, 4), float('nan'), dtype=torch.float32, device='cuda')
    boxes = gpu.up(_cycle(ec.clip_table(), 64))
    out = nan4(64)
    for stride in (3, 0, -4):
        rc = lib.odet_decode(L.dptr(boxes), L.dptr(boxes), stride, 64, L.host4(ec.M0, 'm'), L.host4(ec.S1, 's'), 0, 0, L.dptr(out), L.stream())
        assert rc == E_INVALID and 'delta_stride' in _last_error(gpu)
    # a workspace one byte short
    n = 2000
    b = gpu.up(_cycle(ec.clip_table(), n))
    nb = lib.odet_compact_workspace_bytes(n)
    ws = L.workspace(nb, b.device)
    ob, oi = nan4(n), torch.full((n,), -1, dtype=torch.int64, device='cuda')
    cnt = torch.full((1,), -7, dtype=torch.int32, device='cuda')
    rc = lib.odet_clip_filter(L.dptr(b), n, 0.0, H, W, 16.0, L.dptr(ob), L.dptr(oi), L.dptr(cnt), L.dptr(ws), nb - 1, L.stream())
    assert rc == E_WORKSPACE and 'workspace too small' in _last_error(gpu)
    rc = lib.odet_range_filter(L.dptr(b), n, H, W, L.dptr(oi), L.dptr(cnt), L.dptr(ws), nb - 1, L.stream())
    assert rc == E_WORKSPACE
    rc = lib.odet_where_greater(L.dptr(b), 4, n, 0.5, L.dptr(oi), L.dptr(cnt), L.dptr(ws), nb - 1, L.stream())
    assert rc == E_WORKSPACE
    # assign_levels one RoI above its limit
    n = ec.ASSIGN_MAX_ROIS + 1
    r = gpu.up(_cycle(ec.level_sweep()[0], n))
    lv, perm = torch.full((n,), -1, dtype=torch.int32, device='cuda'), torch.full((n,), -1, dtype=torch.int64, device='cuda')
    counts = torch.full((4,), -7, dtype=torch.int32, device='cuda')
    sr = nan4(n)
    rc = lib.odet_assign_levels(L.dptr(r), n, None, 2, 5, L.dptr(sr), L.dptr(lv), L.dptr(perm), L.dptr(counts), L.stream())
    assert rc == E_LIMIT and str(ec.ASSIGN_MAX_ROIS) in _last_error(gpu)
    # an RPN layout that does not exist
    fg = torch.full((64,), float('nan'), dtype=torch.float32, device='cuda')
    rc = lib.odet_rpn_fg_softmax(L.dptr(boxes), 64, 1, 2, L.dptr(fg), L.stream())
    assert rc == E_INVALID and 'unknown layout' in _last_error(gpu)
    torch.cuda.synchronize()                                # none of them launched anything
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(ob).all()) and bool((oi == -1).all()) and int(cnt.item()) == -7
    assert bool(torch.isnan(sr).all()) and bool((lv == -1).all()) and bool((counts == -7).all()) and bool(torch.isnan(fg).all())


# ---- through the fused stage ------------------------------------------------------------------------------------------------
def test_region_proposal_with_overflowed_deltas(gpu):
    """k_rp_prepare's decode + clip with dw / dh beyond the float32 exp's range, some of them under the highest scores: the
    overflowed boxes reach the NMS as image borders, never as NaN; indices equal oracle.c's, boxes within the decode's 1 ulp"""
    from oracle import c_oracle as co
    deltas, anchors, scores, hot = ec.fused_case()
    K = 300
    rois, idx, cnt = gpu.ops.region_proposal(gpu.up(deltas), gpu.up(anchors), gpu.up(scores), ec.IMAGE, K, 0.7, ec.M0, ec.S1)
    want_rois, want_idx = co.region_proposal(deltas, anchors, scores, ec.IMAGE, K, 0.7)
    m = int(cnt.item())
    got_idx, got_rois = gpu.down(idx[:m]), gpu.down(rois[:m])
    np.testing.assert_array_equal(got_idx, want_idx)
    ec.same(got_rois, want_rois, 1, 'region_proposal rois')
    assert not np.isnan(got_rois).any() and len(set(got_idx.tolist()) & set(hot.tolist())) >= 1
    ec.same(got_rois, ec.decode(anchors, deltas, ec.M0, ec.S1, ec.IMAGE)[got_idx], 1, 'region_proposal rois against the statement')
