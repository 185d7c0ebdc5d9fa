"""k_postops (csrc/postops.hip) orders a class's rows by score first and decodes, filters and runs the greedy NMS over them a
batch of B = PO_ROUND rows at a time, only as far as the walk gets.  Every case here is built to reach a stated number of
batches -- asserted on the host with tests/postops_depth.py, a case that stays inside the first batch proves nothing -- and is
compared with the C oracle by the rule of test_gpu_parity._check_post: labels exact, scores identical bits, boxes within one
unit in the last place (they went through exp).

 * batch edges: exactly n rows above the score threshold, n around B and 2B, nothing suppressed;
 * the cap reached at a batch's last row and one row later;
 * min-edge rejects inside a batch (they take a place in the batch, not in the result);
 * ties at the B-th best key on both sides of the batch boundary, and every score equal;
 * deep walks (12 tight clusters): a cap reached in the fourth batch, and candidates that run out first;
 * a device-side row count below R, with the best scores past it;
 * R = 1500 and 4096;
 * 8 different images in one launch (the step descriptor's detect stage) against their one-image results;
 * the evaluation loop's entry (mode 1);
 * NaN, +inf and scores at / just above the threshold."""
import re
import os

import numpy as np
import pytest

import postops_depth as pd

B = pd.BATCH
SHAPE = (800, 1333)
M0, S2 = [0, 0, 0, 0], [0.1, 0.1, 0.2, 0.2]
NMS, EDGE = 0.3, 16


def g(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ulp(a, b):
    ia = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, np.int64(-2 ** 31) - ia, ia)
    ib = np.where(ib < 0, np.int64(-2 ** 31) - ib, ib)
    return np.abs(ia - ib)


def _check(got, want, what=''):
    gb, gl, gs = got
    wb, wl, ws = want
    if wb is None:
        assert gb is None, '%s: %d detections, the oracle has none' % (what, len(gl))
        return
    assert gb is not None, '%s: no detections, the oracle has %d' % (what, len(wl))
    np.testing.assert_array_equal(gl, wl, err_msg=what)
    np.testing.assert_array_equal(gs.view(np.uint32), np.ascontiguousarray(ws, np.float32).view(np.uint32), err_msg=what)
    assert int(_ulp(gb, wb).max()) <= 1, what


def _gpu(S, D, rois, mpc, mpi, sthr, ncls, count=None, shape=SHAPE):
    import torch
    from tf_eager_object_detection_amd import ops
    cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device='cuda')
    ob, ol, os_, m = ops.post_ops(g(S), g(D), g(rois), shape, M0, S2, mpc, mpi, NMS, sthr, EDGE, ncls, count_dev=cnt)
    m = int(m.item())
    return (None, None, None) if m == 0 else (ob[:m].cpu().numpy(), ol[:m].cpu().numpy(), os_[:m].cpu().numpy())


def _oracle(S, D, rois, mpc, mpi, sthr, ncls, shape=SHAPE):
    from oracle import c_oracle as co
    return co.post_ops(S, D, rois, shape, M0, S2, mpc, mpi, NMS, sthr, EDGE, ncls)


def _walk(S, D, rois, mpc, sthr, ncls, count=None, shape=SHAPE):
    return pd.walk(S, D, rois, shape, M0, S2, mpc, NMS, sthr, EDGE, ncls, count=count)


def _grid_rois(R, size=20, pitch=30, cols=40):
    """R boxes that do not overlap (nor do their decodes with zero deltas, one pixel larger)"""
    i = np.arange(R)
    x, y = (i % cols) * pitch + 5.0, (i // cols) * pitch + 5.0
    return np.stack([x, y, x + size, y + size], axis=1).astype(np.float32)


def _n_above(R, ncls, n, thr, rng):
    """scores with exactly n rows of every foreground class strictly above thr (distinct values, random rows); the others are
    at the threshold itself or below"""
    S = np.empty((R, ncls), np.float32)
    for c in range(ncls):
        low = rng.uniform(0.0, thr, R).astype(np.float32)
        low[rng.integers(0, R, 5)] = np.float32(thr)
        rows = rng.permutation(R)[:n]
        low[rows] = np.float32(thr) + np.float32(0.4) * (1 + rng.permutation(n)).astype(np.float32) / np.float32(n + 1)
        S[:, c] = low
    return S


def _clusters(R, ncls, rng, shape=SHAPE):
    """the 12-cluster construction of test_gpu_parity.test_post_ops_large_r_dense_suppression_and_record: tight clusters,
    deltas ~0, so one box per cluster survives -> (rois, deltas, cluster id per row)"""
    from tf_eager_object_detection_amd import synthetic as syn
    centers = rng.uniform(150, min(shape) - 200, (12, 2)).astype(np.float32)
    cid = rng.integers(0, 12, R)
    ctr = centers[cid] + rng.uniform(-6, 6, (R, 2)).astype(np.float32)
    half = (60 + rng.uniform(-4, 4, (R, 2))).astype(np.float32)
    rois = np.concatenate([ctr - half, ctr + half], axis=1).astype(np.float32)
    D = (syn.class_deltas(R, ncls, rng) * np.float32(0.02)).astype(np.float32)
    return rois, D, cid


def test_batch_size_is_the_kernels():
    """(host) B of this file = PO_ROUND of the kernel"""
    src = open(os.path.join(pd.ROOT, 'tf_eager_object_detection_amd', 'csrc', 'postops.hip')).read()
    assert int(re.search(r'#define PO_ROUND (\d+)', src).group(1)) == B


@pytest.mark.gpu
@pytest.mark.parametrize('n', [0, 1, B - 1, B, B + 1, 2 * B - 1, 2 * B, 2 * B + 1])
def test_batch_edges_everything_kept(n):
    R, ncls, thr = 300, 3, 0.5
    rng = np.random.default_rng(100 + n)
    S, D, rois = _n_above(R, ncls, n, thr, rng), np.zeros((R, ncls, 4), np.float32), _grid_rois(R)
    w = _walk(S, D, rois, R, thr, ncls)
    assert all(d['score_rows'] == d['passing'] == d['kept'] == n for d in w) and pd.batches(w, B) == [-(-n // B)] * 2
    got = _gpu(S, D, rois, R, 2 * R, thr, ncls)
    _check(got, _oracle(S, D, rois, R, 2 * R, thr, ncls), 'n = %d' % n)
    assert n == 0 or (len(got[1]) == 2 * n and (np.diff(got[2]) <= 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize('cap', [B, B + 1])
def test_cap_reached_at_a_batch_end_and_one_row_later(cap):
    R, ncls, thr = 300, 3, 0.5
    rng = np.random.default_rng(7)
    S, D, rois = _n_above(R, ncls, 2 * B + 5, thr, rng), np.zeros((R, ncls, 4), np.float32), _grid_rois(R)
    w = _walk(S, D, rois, cap, thr, ncls)
    assert all(d['kept'] == cap and d['rows_visited'] == cap for d in w) and pd.batches(w, B) == [1 + (cap > B)] * 2
    _check(_gpu(S, D, rois, cap, 2 * cap, thr, ncls), _oracle(S, D, rois, cap, 2 * cap, thr, ncls), 'cap = %d' % cap)


@pytest.mark.gpu
def test_min_edge_rejects_take_a_place_in_the_batch_only():
    R, ncls, thr, cap = 300, 3, 0.5, 40
    rng = np.random.default_rng(11)
    S, D, rois = _n_above(R, ncls, 2 * B + 5, thr, rng), np.zeros((R, ncls, 4), np.float32), _grid_rois(R)
    best = np.argsort(-S[:, 1], kind='stable')[:B]
    small = best[rng.permutation(B)[:B // 2 + 4]]                 # more than half of class 1's first batch: 11-pixel boxes
    rois[small, 2:] = rois[small, :2] + 9.0
    w = _walk(S, D, rois, cap, thr, ncls)
    first = [r for r in best if r not in set(small)]
    assert len(first) < cap and w[0]['kept'] == cap and B < w[0]['rows_visited'] <= 2 * B
    got = _gpu(S, D, rois, cap, 2 * cap, thr, ncls)
    _check(got, _oracle(S, D, rois, cap, 2 * cap, thr, ncls))
    gb = got[0][got[1] == 1]
    assert len(gb) == cap and (gb[:, 2] - gb[:, 0] + 1 >= EDGE).all()


@pytest.mark.gpu
def test_ties_on_both_sides_of_the_batch_boundary():
    """class 1: 44 distinct best scores, then 40 rows at one score (positions 45 .. 84 of the order: the B-th best key is theirs),
    then the rest; class 2: everything quantised to one decimal.  The boxes overlap, so who is kept depends on the order."""
    from tf_eager_object_detection_amd import synthetic as syn
    R, ncls, cap = 300, 3, 50
    rng = np.random.default_rng(13)
    S = np.round(syn.class_scores(R, ncls, rng), 1).astype(np.float32)
    rows = rng.permutation(R)
    S[rows[:B - 20], 1] = np.float32(0.9) + np.float32(0.001) * np.arange(B - 20, dtype=np.float32)
    S[rows[B - 20:B + 20], 1] = np.float32(0.7)
    S[rows[B + 20:], 1] = np.minimum(S[rows[B + 20:], 1], np.float32(0.6))
    D = (syn.class_deltas(R, ncls, rng) * np.float32(0.3)).astype(np.float32)
    rois = syn.random_boxes(R, SHAPE, rng, 100, 500)
    order = np.sort(S[:, 1])[::-1]
    assert order[B - 21] > order[B - 20] == order[B - 1] == order[B] == order[B + 19] > order[B + 20]
    w = _walk(S, D, rois, cap, 0.0, ncls)
    assert w[0]['rows_visited'] > B + 20 and w[1]['rows_visited'] > B, w
    _check(_gpu(S, D, rois, cap, cap, 0.0, ncls), _oracle(S, D, rois, cap, cap, 0.0, ncls))


@pytest.mark.gpu
def test_every_score_equal():
    """one key for all 1000 rows: the order is the row order, every batch boundary falls inside the tie"""
    from tf_eager_object_detection_amd import synthetic as syn
    R, ncls, cap = 1000, 3, 50
    rng = np.random.default_rng(17)
    S = np.full((R, ncls), 0.25, np.float32)
    D = (syn.class_deltas(R, ncls, rng) * np.float32(0.3)).astype(np.float32)
    rois = syn.random_boxes(R, SHAPE, rng, 100, 500)
    w = _walk(S, D, rois, cap, 0.0, ncls)
    assert all(d['kept'] == cap for d in w) and min(pd.batches(w, B)) >= 2, w
    _check(_gpu(S, D, rois, cap, cap, 0.0, ncls), _oracle(S, D, rois, cap, cap, 0.0, ncls))


@pytest.mark.gpu
@pytest.mark.parametrize('cap,exhausted', [(8, False), (50, True)])
def test_deep_walks(cap, exhausted):
    """12 tight clusters, one survivor each.  cap 8: the rows of half of the clusters come only after the best 3 B + 10 rows, so
    the 8th box is kept in the fourth batch or later; cap 50: never reached, every batch is run until the rows run out."""
    from tf_eager_object_detection_amd import synthetic as syn
    R, ncls = 1000, 3
    rng = np.random.default_rng(2301)
    rois, D, cid = _clusters(R, ncls, rng)
    S = syn.class_scores(R, ncls, rng)
    for c in (1, 2):            # the best 3 B + 10 scores go to rows of clusters 0 .. 5
        order = np.argsort(-S[:, c], kind='stable')
        early = np.flatnonzero(cid < 6)[:3 * B + 10]
        rest = np.setdiff1d(np.arange(R), early)
        S[np.concatenate([early, rest]), c] = S[order, c]
    w = _walk(S, D, rois, cap, 0.0, ncls)
    if exhausted:
        assert all(d['kept'] < cap and d['rows_visited'] == d['score_rows'] == R for d in w), w
    else:
        assert all(d['kept'] == cap and d['rows_visited'] > 3 * B + 10 for d in w), w
    _check(_gpu(S, D, rois, cap, 2 * cap, 0.0, ncls), _oracle(S, D, rois, cap, 2 * cap, 0.0, ncls))


@pytest.mark.gpu
def test_device_side_count_below_r():
    """rows past the device-side count hold the best scores and must not take part"""
    R, n, ncls, thr = 300, 200, 3, 0.5
    rng = np.random.default_rng(19)
    S, D, rois = _n_above(R, ncls, 2 * B + 30, thr, rng), np.zeros((R, ncls, 4), np.float32), _grid_rois(R)
    S[n:] = np.float32(2.0)
    w = _walk(S, D, rois, R, thr, ncls, count=n)
    assert all(B < d['kept'] == d['rows_visited'] < 2 * B + 30 for d in w), w
    got = _gpu(S, D, rois, R, 2 * R, thr, ncls, count=n)
    _check(got, _oracle(S[:n], D[:n], rois[:n], R, 2 * R, thr, ncls))
    assert got[2].max() < 1.0


@pytest.mark.gpu
@pytest.mark.parametrize('R', [1500, 4096])
def test_more_than_1024_rows_with_ties_at_the_boundary(R):
    from tf_eager_object_detection_amd import synthetic as syn
    ncls, cap = 3, 50
    rng = np.random.default_rng(R)
    S = np.round(syn.class_scores(R, ncls, rng), 2).astype(np.float32)
    D = (syn.class_deltas(R, ncls, rng) * np.float32(0.3)).astype(np.float32)
    rois = syn.random_boxes(R, SHAPE, rng, 100, 500)
    for c in (1, 2):            # the B-th and the (B + 1)-th best score are one value
        order = np.argsort(-S[:, c], kind='stable')
        S[order[B - 3:B + 3], c] = S[order[B], c]
        o = np.sort(S[:, c])[::-1]
        assert o[B - 1] == o[B]
    w = _walk(S, D, rois, cap, 0.05, ncls)
    assert all(d['kept'] == cap and d['rows_visited'] > B for d in w), w
    _check(_gpu(S, D, rois, cap, cap, 0.05, ncls), _oracle(S, D, rois, cap, cap, 0.05, ncls))


@pytest.mark.gpu
def test_eight_images_in_one_launch():
    """the detect stage of the step descriptor, 8 images with different inputs in one launch -- one with no row above the
    threshold, one with every score equal, one deep (clusters, candidates exhausted): each equals its own one-image launch bit
    for bit, and the oracle"""
    import torch
    from tf_eager_object_detection_amd import synthetic as syn
    from tf_eager_object_detection_amd.pipeline import FpnStepBatch
    shape, R, ncls, cap, mpi, thr = (480, 640), 300, 3, 50, 60, 0.2
    sb = FpnStepBatch(8, shape, ncls, R, 8, max_per_class=cap, max_per_image=mpi, score_threshold=thr, nms_iou=NMS,
                      roi_means=M0, roi_stds=S2)
    dev = torch.device('cuda')
    N = sb.slots[0].N
    logits, rdeltas = torch.zeros((N, 2), device=dev), torch.zeros((N, 4), device=dev)
    maps = [torch.zeros((1, h, w, 8), device=dev) for h, w in syn.fpn_level_shapes(shape)[:4]]
    cases = []
    for b in range(8):
        rng = np.random.default_rng(500 + b)
        S = syn.class_scores(R, ncls, rng)
        D = (syn.class_deltas(R, ncls, rng) * np.float32(0.3)).astype(np.float32)
        rois = syn.random_boxes(R, shape, rng, 60, 300)
        if b == 2:
            S = np.minimum(S, np.float32(thr))
        elif b == 4:
            S[:] = np.float32(0.25)
        elif b == 6:
            rois, D, _ = _clusters(R, ncls, rng, shape)
        cases.append((S, D, rois))
        keep = (g(S), g(D))
        sb.bind(b, logits, rdeltas, maps, *keep)
        sb.slots[b].sorted_rois.copy_(g(rois))
        sb.slots[b].roi_count.fill_(R)
    depth = [_walk(S, D, rois, cap, thr, ncls, shape=shape) for S, D, rois in cases]
    assert all(d['score_rows'] == 0 for d in depth[2]) and min(pd.batches(depth[4], B)) >= 2
    assert all(d['kept'] < cap and d['rows_visited'] > 2 * B for d in depth[6]), depth[6]
    sb.enqueue(sb.STAGE_DETECT, 8)
    torch.cuda.synchronize()
    for b, (S, D, rois) in enumerate(cases):
        s = sb.slots[b]
        m = int(s.det_count.item())
        got = (None, None, None) if m == 0 else (s.det_boxes[:m].cpu().numpy(), s.det_labels[:m].cpu().numpy(),
                                                 s.det_scores[:m].cpu().numpy())
        one = _gpu(S, D, rois, cap, mpi, thr, ncls, shape=shape)
        assert (got[0] is None) == (one[0] is None), b
        for x, y in zip(got, one):
            if x is not None:
                np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32), err_msg='image %d' % b)
        _check(got, _oracle(S, D, rois, cap, mpi, thr, ncls, shape=shape), 'image %d' % b)


@pytest.mark.gpu
def test_mode_1_across_a_batch_boundary():
    """odet_eval_detect (the evaluation loop's per-image cap in the merge) on tied scores that straddle the batch boundary"""
    from oracle import oracle_np as on
    from tf_eager_object_detection_amd import synthetic as syn
    from tf_eager_object_detection_amd.evaluation import pascal_eval as pe
    R, ncls = 300, 21
    rng = np.random.default_rng(23)
    im = syn.eval_image(rng, raw_shape=(375, 500), num_rois=R)
    sc = np.round(im['scores'], 2).astype(np.float32)
    rows = rng.permutation(R)
    sc[rows[:B + 20], 1] = np.float32(0.5)
    sc[rows[:B - 20], 1] += np.float32(0.001) * (1 + np.arange(B - 20, dtype=np.float32))
    o = np.sort(sc[:, 1])[::-1]
    assert o[B - 21] > o[B - 20] == o[B] == o[B + 19]
    kw = dict(score_threshold=0.05, iou_threshold=0.5, max_objects_per_class=100, max_objects_per_image=40, min_size=10)
    want = on.eval_detect_image(sc, im['deltas'], im['rois'], im['img_scale'], im['raw_h'], im['raw_w'], **kw)
    w = pd.walk(sc, im['deltas'], im['rois'], (int(im['raw_h']), int(im['raw_w'])), M0, S2, 100, 0.5, 0.05, 10, ncls,
                roi_div=im['img_scale'])
    assert w[0]['rows_visited'] >= B + 20 and len(want[1]) > 0, w[0]
    got = pe.detect_image(g(sc), g(im['deltas']), g(im['rois']), im['img_scale'], im['raw_h'], im['raw_w'], **kw)
    for j in range(1, ncls):
        assert got[j].shape == want[j].shape, (j, got[j].shape, want[j].shape)
        if len(want[j]):
            np.testing.assert_array_equal(got[j][:, 4].view(np.uint32), want[j][:, 4].view(np.uint32))
            assert int(_ulp(got[j][:, :4], want[j][:, :4]).max()) <= 1


@pytest.mark.gpu
def test_special_scores():
    """NaN never passes the strict >, +inf is the best score there is, a score AT the threshold does not pass and the next float
    above it does; they sit among 2 B + 5 ordinary rows, so the second batch holds the row just above the threshold"""
    R, ncls, thr = 300, 3, 0.5
    rng = np.random.default_rng(29)
    S, D, rois = _n_above(R, ncls, 2 * B + 5, thr, rng), np.zeros((R, ncls, 4), np.float32), _grid_rois(R)
    low = np.flatnonzero((S[:, 1] < thr) & (S[:, 2] < thr))
    S[low[0:3]] = np.nan
    S[low[3], 1] = np.inf
    S[low[4], 2] = np.inf
    S[low[5:8]] = np.float32(thr)
    S[low[8:10]] = np.nextafter(np.float32(thr), np.float32(1))
    w = _walk(S, D, rois, R, thr, ncls)
    assert all(d['kept'] == d['score_rows'] == 2 * B + 5 + 3 for d in w), w
    got = _gpu(S, D, rois, R, 2 * R, thr, ncls)
    _check(got, _oracle(S, D, rois, R, 2 * R, thr, ncls))
    assert np.isinf(got[2][:2]).all() and not np.isnan(got[2]).any() and got[2].min() == np.nextafter(np.float32(thr), np.float32(1))
