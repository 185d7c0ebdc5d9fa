"""tests/box_edge_cases.py on the host: the statement is anchored on the two oracles wherever no NaN reaches a min / max, the
rows where one does are counted (a table that loses them fails), every table reaches what it is for, and the declared
properties (DESIGN.md "Box primitives: declared behaviour") hold for the statement.  tests/test_box_edges_gpu.py asserts the
same properties on the kernels' outputs."""
import numpy as np
import pytest

import box_edge_cases as ec
from oracle import c_oracle as co
from oracle import oracle_np as on

H, W = ec.IMAGE


def _np(fn, *a, **k):
    with np.errstate(all='ignore'):
        return fn(*a, **k)


# ---- a NaN that arises on the way (inf - inf, inf * 0) from inputs that hold none ------------------------------------------
def _iou_nan_on_the_way(b1, b2):
    """[n, m]: an operand of the outer max(0, .) is a NaN although neither box holds one"""
    p, q = b1.reshape(-1, 1, 4), b2.reshape(1, -1, 4)
    with np.errstate(all='ignore'):
        dh = ec.minnum(p[..., 3], q[..., 3]) - ec.maxnum(p[..., 1], q[..., 1])
        dw = ec.minnum(p[..., 2], q[..., 2]) - ec.maxnum(p[..., 0], q[..., 0])
    return (np.isnan(dh) | np.isnan(dw)) & ~ec.has_nan(b1)[:, None] & ~ec.has_nan(b2)[None, :]


def _level_nan_on_the_way(r):
    with np.errstate(all='ignore'):
        dh, dw = r[:, 3] - r[:, 1], r[:, 2] - r[:, 0]
        area = ec.maxnum(ec.F(0), dh) * ec.maxnum(ec.F(0), dw)
    return (np.isnan(dh) | np.isnan(dw) | np.isnan(area)) & ~ec.has_nan(r)


# ---- statement == oracle_np == oracle.c -----------------------------------------------------------------------------------
@pytest.mark.parametrize('means,stds,clip_shape', ec.DECODE_SETTINGS[:2])
def test_decode_statement_is_both_oracles(means, stds, clip_shape):
    anchors, deltas = ec.decode_table()
    ok = ~ec.has_nan(anchors, deltas)
    assert ok.sum() > 150 and (~ok).sum() > 20
    want = ec.decode(anchors, deltas, means, stds)
    ec.same(_np(on.decode_bbox_with_mean_and_std, anchors, deltas, means, stds)[ok], want[ok], 1, 'decode: oracle_np')
    ec.same(co.decode(anchors, deltas, means, stds)[ok], want[ok], 1, 'decode: oracle.c')
    # plain arithmetic: a NaN input gives the same NaN positions everywhere too
    ec.same(co.decode(anchors, deltas, means, stds), want, 1, 'decode, NaN rows: oracle.c')
    ec.same(_np(on.decode_bbox_with_mean_and_std, anchors, deltas, means, stds), want, 1, 'decode, NaN rows: oracle_np')


def test_decode_table_overflows_from_finite_deltas():
    anchors, deltas = ec.decode_table()
    finite = np.isfinite(anchors).all(axis=1) & np.isfinite(deltas).all(axis=1)
    for means, stds, clip_shape in ec.DECODE_SETTINGS:
        out = ec.decode(anchors, deltas, means, stds)[finite]
        assert (out == -np.inf).any() and (out == np.inf).any() and np.isnan(out).any(), stds
        # d_decode_box on an exp overflow: x1 = -inf, x2 = NaN
        assert ((out[:, 0] == -np.inf) & np.isnan(out[:, 2])).any() and ((out[:, 1] == -np.inf) & np.isnan(out[:, 3])).any()
        # the fused clip is the clip of the decoded box, and leaves no NaN
        fused = ec.decode(anchors, deltas, means, stds, ec.IMAGE)
        ec.same(fused, ec.clip(ec.decode(anchors, deltas, means, stds), 0, H, W), 0, 'fused clip')
        assert not np.isnan(fused).any()
    row = (deltas[:, 2] == ec.F(88.8)) & (deltas[:, 3] == 0) & (deltas[:, 0] == 0) & finite & (anchors == ec.f32(ec.ANCHOR)).all(axis=1)
    assert row.sum() == 1
    np.testing.assert_array_equal(ec.decode(anchors, deltas, ec.M0, ec.S1, ec.IMAGE)[row][0], [0, 64, W - 1, 192])


@pytest.mark.parametrize('means,stds', ec.ENCODE_SETTINGS)
def test_encode_statement_is_both_oracles(means, stds):
    src, gt = ec.encode_table()
    ok = ~ec.has_nan(src, gt)
    want = ec.encode(src, gt, means, stds)
    ec.same(_np(on.encode_bbox_with_mean_and_std, src, gt, means, stds), want, 1, 'encode: oracle_np')
    ec.same(co.encode(src, gt, means, stds), want, 1, 'encode: oracle.c')
    w = want[ok]
    assert (w == -np.inf).any() and (w == np.inf).any() and np.isnan(w).any()     # log(0), x / 0, log of a negative, 0 / 0
    with np.errstate(all='ignore'):
        ratio = (gt[:, 2] - gt[:, 0] + 1) / (src[:, 2] - src[:, 0] + 1)
    assert ((ratio > 0) & (ratio < np.finfo(np.float32).tiny)).any() and ((ratio == np.inf) & ok).any()
    assert (src == gt).all(axis=1).sum() >= 5


@pytest.mark.parametrize('min_value', ec.CLIP_SETTINGS)
def test_clip_statement_and_the_oracles(min_value):
    boxes = ec.clip_table()
    ok = ~ec.has_nan(boxes)
    want = ec.clip(boxes, min_value, H, W)
    got_np = _np(on.bboxes_clip_filter, boxes, min_value, H, W)[0]
    got_c = co.clip_filter(boxes, min_value, H, W)[0]
    ec.same(got_np[ok], want[ok], 0, 'clip: oracle_np')
    ec.same(got_c[ok], want[ok], 0, 'clip: oracle.c')
    # NaN rows: numpy hands the NaN on, oracle.c's `a < b ? a : b` takes the border as minNum does
    assert ec.count_differences(got_np[~ok], want[~ok]) == 14
    assert ec.count_differences(got_c[~ok], want[~ok]) == 0
    assert (~ok).sum() == 8
    # properties of the statement
    assert not np.isnan(want).any()
    assert (want >= ec.F(min_value)).all() and (want[:, 0::2] <= W - 1).all() and (want[:, 1::2] <= H - 1).all()


def test_clip_table_sits_on_the_borders():
    boxes = ec.clip_table()
    for edge in (0.0, W - 1.0, H - 1.0):
        for v in (ec.F(edge), ec.up(edge, 1), ec.up(edge, -1)):
            assert all((boxes[:, s] == v).any() for s in range(4)), (edge, v)
    assert np.isinf(boxes).any() and np.isnan(boxes).all(axis=1).any() and (np.isnan(boxes).sum(axis=1) == 1).sum() == 4
    assert ((boxes[:, 2] < boxes[:, 0]) & (boxes[:, 3] < boxes[:, 1])).any()
    with np.errstate(all='ignore'):
        c = ec.clip(boxes, 0, H, W)
        e0, e1 = c[:, 2] - c[:, 0] + 1, c[:, 3] - c[:, 1] + 1
    me = ec.F(ec.MIN_EDGE)
    for e, o in ((e0, e1), (e1, e0)):                        # exactly min_edge and one ulp below it, on either axis
        assert ((e == me) & (o >= me)).any() and ((e == ec.up(me, -1)) & (o >= me)).any()


@pytest.mark.parametrize('min_value,min_edge', ec.FILTER_SETTINGS)
def test_filter_statements_and_the_oracles(min_value, min_edge):
    boxes = ec.clip_table()
    ok = ~ec.has_nan(boxes)
    clean = boxes[ok]
    wb, wi = ec.clip_filter(clean, min_value, H, W, min_edge)
    for name, (gb, gi) in (('oracle_np', _np(on.bboxes_clip_filter, clean, min_value, H, W, min_edge)),
                           ('oracle.c', co.clip_filter(clean, min_value, H, W, min_edge))):
        ec.same(gi, wi, 0, 'clip_filter indices: ' + name)
        ec.same(gb, wb, 0, 'clip_filter boxes: ' + name)
    assert 0 < len(wi) < len(clean) or min_edge <= 1
    wr = ec.range_filter(clean, H, W)
    ec.same(_np(on.bboxes_range_filter, clean, H, W), wr, 0, 'range_filter: oracle_np')
    ec.same(co.range_filter(clean, H, W), wr, 0, 'range_filter: oracle.c')
    assert 0 < len(wr) < len(clean)
    # with the NaN rows: a comparison with a NaN is false in all three
    ec.same(co.range_filter(boxes, H, W), ec.range_filter(boxes, H, W), 0, 'range_filter, NaN rows: oracle.c')
    ec.same(_np(on.bboxes_range_filter, boxes, H, W), ec.range_filter(boxes, H, W), 0, 'range_filter, NaN rows: oracle_np')
    ec.same(co.clip_filter(boxes, min_value, H, W, min_edge)[1], ec.clip_filter(boxes, min_value, H, W, min_edge)[1], 0,
            'clip_filter, NaN rows: oracle.c')


# of the 295 pairs of the IoU table with a NaN corner: values that differ between the statement and either oracle, and between the oracles
NAN_IOU_DIFFERENCES = {'oracle_np': 133, 'oracle.c': 79, 'between': 54}
LEVEL_NAN_IN_NUMPY = 8             # RoIs of the level table that oracle_np leaves without a level (5 with a NaN, inf x 0 twice, inf - inf)


def test_iou_statement_and_the_oracles():
    t = ec.iou_boxes()
    want = ec.pairwise_iou(t, t)
    got_np, got_c = _np(on.pairwise_iou, t, t), co.pairwise_iou(t, t)
    nan_in = ec.has_nan(t)[:, None] | ec.has_nan(t)[None, :]
    on_the_way = _iou_nan_on_the_way(t, t)
    clean = ~nan_in & ~on_the_way
    assert clean.sum() > 600
    ec.same(got_np[clean], want[clean], 0, 'IoU: oracle_np')
    ec.same(got_c[clean], want[clean], 0, 'IoU: oracle.c')
    # no NaN in the input: the two oracles agree everywhere, NaN positions included ...
    ec.same(got_np[~nan_in], got_c[~nan_in], 0, 'IoU, NaN-free boxes: oracle_np against oracle.c')
    # ... also where inf - inf makes a NaN on the way to max(0, .): both hand it on, maxNum takes the 0.  These pairs have NaN-free
    # inputs and the statement differs from BOTH oracles on them: the min / max rule is not only about NaN inputs.
    assert on_the_way.sum() == 12
    assert ec.count_differences(got_np[on_the_way], want[on_the_way]) == 12
    assert ec.count_differences(got_c[on_the_way], want[on_the_way]) == 12
    assert (want[on_the_way] == 0).all() and np.isnan(got_c[on_the_way]).all()
    # NaN boxes: three rules, three results
    d_np, d_c, d_oo = (ec.count_differences(a[nan_in], b[nan_in]) for a, b in ((got_np, want), (got_c, want), (got_np, got_c)))
    assert (d_np, d_c, d_oo) == (NAN_IOU_DIFFERENCES['oracle_np'], NAN_IOU_DIFFERENCES['oracle.c'], NAN_IOU_DIFFERENCES['between'])
    assert min(d_np, d_c, d_oo) > 0
    # property: a box with a NaN corner never has a positive IoU with anything
    assert (np.isnan(want[nan_in]) | (want[nan_in] == 0)).all()
    # what the table is for
    inter_zero_touching = want[0, 2] == 0 and want[0, 3] == 0 and want[0, 4] > 0 and want[0, 5] > 0
    assert inter_zero_touching and want[0, 1] == 1.0
    zero_area = [11, 12, 13, 14]
    assert (want[np.ix_(zero_area, zero_area)] == 0).all()                     # uni == 0 and inter == 0: 0, not 0 / 0
    assert np.isinf(t).any() and (np.abs(t) == ec.F(3e38)).any() and (t == ec.F(1e20)).any()
    for s in range(4):
        assert (np.isnan(t[:, s]) & (np.isnan(t).sum(axis=1) == 1)).any()



@pytest.mark.parametrize('n,m', ec.IOU_SIZES)
def test_iou_sizes_keep_the_kinds(n, m):
    b1, b2 = ec.iou_operands(n, m)
    assert b1.shape == (n, 4) and b2.shape == (m, 4)
    if m >= 63:
        assert ec.has_nan(b2).any() and np.isinf(b2).any() and (b2[:, 2] < b2[:, 0]).any()
    want = ec.pairwise_iou(b1, b2)
    nan_in = ec.has_nan(b1)[:, None] | ec.has_nan(b2)[None, :]
    assert (np.isnan(want[nan_in]) | (want[nan_in] == 0)).all()


@pytest.mark.parametrize('min_level,max_level', ec.LEVEL_RANGES)
def test_level_statement_and_the_oracles(min_level, max_level):
    rois, which = ec.level_sweep()
    n = len(rois)
    nan_in, on_the_way = ec.has_nan(rois), _level_nan_on_the_way(rois)
    clean = ~nan_in & ~on_the_way
    srois, lv_sorted, perm, counts = ec.assign_levels(rois, min_level, max_level)
    lv = ec.roi_levels(rois, min_level, max_level)
    # property: every RoI gets exactly one level
    assert counts.sum() == n and np.array_equal(np.sort(perm), np.arange(n)) and np.array_equal(lv[perm], lv_sorted)
    assert lv.min() >= 0 and lv.max() <= max_level - min_level and np.array_equal(srois.view(np.uint32), rois[perm].view(np.uint32))
    c_lv, c_perm, c_counts = co.assign_levels(rois, min_level, max_level)
    np_lists, np_perm, np_lv = _np(on.assign_levels, rois, min_level, max_level)
    np.testing.assert_array_equal(c_lv[clean] - min_level, lv[clean])
    np.testing.assert_array_equal(np_lv[clean].astype(np.int32) - min_level, lv[clean])
    # NaN RoIs (and inf x 0, inf - inf): numpy gives them no level at all, oracle.c and the statement the lowest one
    odd = nan_in | on_the_way
    assert nan_in.sum() == 5 and on_the_way.sum() == 3
    assert np.isnan(np_lv[odd]).sum() == LEVEL_NAN_IN_NUMPY and len(np_perm) == n - LEVEL_NAN_IN_NUMPY
    assert (lv[np.isnan(np_lv)] == 0).all()
    np.testing.assert_array_equal(c_lv - min_level, lv)
    np.testing.assert_array_equal(c_perm, perm)
    np.testing.assert_array_equal(c_counts, counts)



def test_level_sweep_straddles_every_boundary():
    rois, which = ec.level_sweep()
    fin = ~ec.has_nan(rois) & np.isfinite(rois).all(axis=1) & (which >= 0)
    pos = np.full(len(rois), np.nan)
    pos[fin] = ec.level_position(rois[fin])
    lv = ec.roi_levels(rois, 0, 7)
    for bi, b in enumerate(ec.LEVEL_BOUNDARIES):
        k = 2 + bi                                           # the level that begins at this boundary
        rows = fin & (which == bi)
        d = pos[rows] - k
        assert rows.sum() > 2 * ec.LEVEL_NEIGHBOURS and np.abs(d).max() < 2e-3
        assert (d < 0).sum() > ec.LEVEL_NEIGHBOURS and (d > 0).sum() > ec.LEVEL_NEIGHBOURS
        inside, outside = np.abs(d) < 0.5 * ec.LEVEL_BAND, np.abs(d) > 2 * ec.LEVEL_BAND
        for side in (d < 0, d > 0):
            assert (inside & side).sum() >= ec.LEVEL_NEIGHBOURS and (outside & side).sum() >= 8
        # both levels appear, and far enough from the boundary the float64 position decides which
        got = lv[rows]
        assert set(got.tolist()) == {k - 1, k}
        far = np.abs(d) > 1e-6
        np.testing.assert_array_equal(got[far], np.where(d[far] < 0, k - 1, k))
        # the model's range hides the outer boundaries (both sides clamp to the same level); (0, 7) shows all five
        assert len(set(ec.roi_levels(rois[rows], 2, 5).tolist())) == (2 if 0 < bi < 4 else 1)
        # the float32 neighbours themselves: squares whose edge lengths are consecutive floats around b
        sq = rois[rows & (rois[:, 0] == 0) & (rois[:, 2] == rois[:, 3])][:, 2]
        walk = np.unique(sq)
        lo = np.searchsorted(walk, ec.up(b, -ec.LEVEL_NEIGHBOURS))
        run = walk[lo:lo + 2 * ec.LEVEL_NEIGHBOURS + 1]
        assert run[-1] == ec.up(b, ec.LEVEL_NEIGHBOURS) and np.array_equal(run[1:], np.nextafter(run[:-1], ec.INF))
    assert len(rois) <= ec.ASSIGN_MAX_ROIS


def test_compaction_cases_hold_every_pattern():
    cases = ec.compact_cases()
    assert {n for n, _ in cases} == set(ec.COMPACT_SIZES) | {ec.COMPACT_LARGE}
    assert {k for _, k in cases} == set(ec.COMPACT_KINDS) | {'large'}
    for n, kind in cases:
        m = ec.keep_mask(n, kind)
        tiles = -(-n // ec.CP_TILE)
        per_tile = np.add.reduceat(m.astype(np.int64), np.arange(0, n, ec.CP_TILE))
        want = {'all': n, 'none': 0, 'alternating': (n + 1) // 2, 'first': 1, 'last': 1, 'one_per_tile': tiles}.get(kind)
        if kind == 'one_per_tile':
            assert (per_tile == 1).all()
        if kind == 'first':
            assert m[0]
        if kind == 'last':
            assert m[-1]
        if kind == 'large':
            assert tiles == 1026 and -(-tiles // ec.CP_SCAN_THREADS) == 2          # k_cp_scan: per == 2
            assert per_tile[0] == ec.CP_TILE // 2 and per_tile[-1] == 1 and 0 < (per_tile[1:-1] > 0).sum() < tiles - 2
            assert per_tile[1024] + per_tile[1025] > 0                             # the tiles a `per` of 1 never visits
        else:
            assert m.sum() == want
        # the three predicates keep exactly the mask
        if n <= 5000:
            ec.same(ec.where_greater(ec.mask_values(m), 0.5), np.nonzero(m)[0], 0, 'where_greater')
            ec.same(ec.clip_filter(ec.mask_boxes(m, 'clip_filter'), 0, H, W, ec.MIN_EDGE)[1], np.nonzero(m)[0], 0, 'clip_filter')
            ec.same(ec.range_filter(ec.mask_boxes(m, 'range_filter'), H, W), np.nonzero(m)[0], 0, 'range_filter')


def test_where_greater_values_and_thresholds():
    v = ec.where_values()
    thr = ec.F(0.05)
    assert (v == thr).any() and (v == ec.up(thr, 1)).any() and np.isnan(v).any() and np.isinf(v).any()
    assert len(ec.where_greater(v, np.nan)) == 0 and len(ec.where_greater(v, np.inf)) == 0
    kept = ec.where_greater(v, -np.inf)
    assert len(kept) == (~np.isnan(v) & (v != -np.inf)).sum()
    assert not (v[ec.where_greater(v, thr)] == thr).any() and not np.isnan(v[ec.where_greater(v, thr)]).any()
    assert {t for t in ec.WHERE_THRESHOLDS if t in (np.inf, -np.inf)} == {np.inf, -np.inf} and any(t != t for t in ec.WHERE_THRESHOLDS)


def test_gather_cases():
    cases = ec.gather_cases()
    assert {c[1] for c in cases} >= set(ec.GATHER_ROW_FLOATS) and {c[4] for c in cases} == {np.int32, np.int64}
    assert any(c[2] * c[1] > ec.GATHER_GRID * ec.GATHER_BLOCK for c in cases)
    counts = {(None if c[5] is None else ('zero' if c[5] == 0 else ('below' if c[5] < c[2] else 'above'))) for c in cases}
    assert counts == {None, 'zero', 'below', 'above'}
    for rows, rf, n, kind, dt, count in cases:
        idx = ec.gather_indices(n, rows, kind)
        assert len(idx) == n + ec.GATHER_SPARE and idx.min() >= 0 and idx.max() < rows
        assert count is None or count <= n + ec.GATHER_SPARE                      # a count above n stays inside the buffers
        src = np.arange(rows * rf, dtype=np.float32).reshape(rows, rf)
        assert len(ec.gather_rows(src, idx[:n], count)) == (n if count is None else min(count, n))
    assert (np.diff(ec.gather_indices(37, 50, 'descending')[:37]) < 0).all()
    assert len(np.unique(ec.gather_indices(37, 50, 'repeated')[:37])) < 37


def test_fused_case_agrees_with_the_c_oracle():
    deltas, anchors, scores, hot = ec.fused_case()
    assert 1900 <= len(anchors) <= 2100 and len(hot) == 16 and len(np.unique(scores)) == len(scores)
    assert (np.maximum(deltas[hot, 2], deltas[hot, 3]) >= ec.F(88.8)).all()
    assert set(np.argsort(-scores)[:6].tolist()) <= set(hot.tolist())
    raw = ec.decode(anchors, deltas, ec.M0, ec.S1)
    assert np.isnan(raw[hot]).any(axis=1).all() and not np.isnan(np.delete(raw, hot, axis=0)).any()
    want = ec.decode(anchors, deltas, ec.M0, ec.S1, ec.IMAGE)
    got = co.clip_filter(co.decode(anchors, deltas, ec.M0, ec.S1), 0, H, W)[0]
    ec.same(got, want, 1, 'decode + clip: oracle.c')
    assert not np.isnan(want).any()
    rois, idx = co.region_proposal(deltas, anchors, scores, ec.IMAGE, 300, 0.7)
    assert len(idx) > 50 and len(set(idx.tolist()) & set(hot.tolist())) >= 1
