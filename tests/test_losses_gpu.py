"""The fused training losses (odet_rpn_loss / odet_rpn_loss_backward / odet_roi_loss, csrc/losses.hip) on the GPU: every output
against the numpy restatement (tests/losses_np.py) bit for bit -- values behind exp / log are held to one unit in the last
place, the observed distance is printed and expected to be 0 --, the dense gradients' zero surface and layout, batch
independence, graph capture of targets -> losses -> backward (no host read, no allocation), torch autograd through
model/losses.py within the derived bounds of tests/test_losses_host.py, and the caller models' `training_losses='hip'`."""
import numpy as np
import pytest
import torch

import losses_np as ln
from oracle import c_oracle as co
from tf_eager_object_detection_amd import synthetic as syn

pytestmark = pytest.mark.gpu

RPN = dict(pos=0.7, neg=0.3, total=256, max_pos=128, means=[0, 0, 0, 0], stds=[1, 1, 1, 1])
ROI_STDS = [0.1, 0.1, 0.2, 0.2]
QUIRK_GT = np.float32([[100, 100, 300, 300], [2000, 2000, 2100, 2100]])
A_FPN = 3                      # anchors per location of the FPN anchor sets (so both score layouts fit them)


def _ulps(a, b):
    ia = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -2 ** 31 - ia, ia)
    ib = np.where(ib < 0, -2 ** 31 - ib, ib)
    return int(np.abs(ia - ib).max()) if ia.size else 0


def _cases():
    """(name, shape, anchors, gt): the four anchor cases of tests/test_targets_gpu.py"""
    out = []
    small = (320, 480)
    a_small = co.fpn_anchors(small)
    out.append(('320x480-7', small, a_small, syn.random_boxes(7, small, np.random.default_rng(11), 30, 200)))
    big = (800, 1333)
    a_big = co.fpn_anchors(big)
    rng = np.random.default_rng(21)
    g8 = syn.random_boxes(8, big, rng, 16, 600)
    g100 = syn.random_boxes(100, big, rng, 16, 600)
    out.append(('800x1333-8', big, a_big, g8))
    out.append(('800x1333-100', big, a_big, g100))
    out.append(('quirk', small, a_small, QUIRK_GT))
    return out


def _pack(gts):
    off = np.cumsum([0] + [len(g) for g in gts]).astype(np.int32)
    boxes = np.concatenate([np.asarray(g, np.float32).reshape(-1, 4) for g in gts] + [np.zeros((1, 4), np.float32)])
    return torch.from_numpy(boxes).cuda(), torch.from_numpy(off).cuda()


def _anchor_targets(gts, shape, anchors, seed=0, first_image_id=0, dense=False):
    from tf_eager_object_detection_amd import ops
    gb, off = _pack(gts)
    return ops.anchor_targets(torch.from_numpy(anchors).cuda(), gb, off, shape, RPN['pos'], RPN['neg'], RPN['total'],
                              RPN['max_pos'], RPN['means'], RPN['stds'], seed=seed, first_image_id=first_image_id, dense=dense)


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _rpn_head(rng, at, N, sigma):
    """head outputs of the batch in the FPN layout: logits over +-30, deltas that straddle 1 / sigma_2 on the sampled rows"""
    idx, tg, counts = _np(at.sample_idx), _np(at.sample_targets), _np(at.counts)
    B = idx.shape[0]
    scores = rng.uniform(-30, 30, (B, N, 2)).astype(np.float32)
    scores[:, ::3] = rng.normal(0, 2, scores[:, ::3].shape)
    deltas = rng.normal(0, 1, (B, N, 4)).astype(np.float32)
    thr = 1.0 / sigma ** 2
    for b in range(B):
        k = max(int(counts[b, 3]), 0)
        deltas[b, idx[b, :k]] = tg[b, :k] + rng.uniform(-2.5 * thr, 2.5 * thr, (k, 4)).astype(np.float32)
    return scores, deltas


def _frcnn(scores_fpn, A):
    """[B,N,2] rows -> the [A bg | A fg] layout, flat per image"""
    return np.stack([ln.from_fpn_view(s, ln.LAYOUT_FRCNN, A) for s in scores_fpn])


def _run_rpn(scores, deltas, at, sigma, layout, A, upstream):
    from tf_eager_object_detection_amd import ops
    s, d = torch.from_numpy(scores).cuda(), torch.from_numpy(deltas).cuda()
    fwd = ops.rpn_losses(s, d, at.sample_idx, at.sample_targets, at.counts, sigma, layout, A)
    up = torch.from_numpy(np.asarray(upstream, np.float32)).cuda()
    bwd = ops.rpn_losses_backward(at.sample_idx, fwd.row_grad_scores, fwd.row_grad_deltas, up, deltas.shape[1], layout, A)
    torch.cuda.synchronize()
    return {k: _np(v) for k, v in list(fwd._asdict().items()) + list(bwd._asdict().items())}


def _compare_rpn(name, got, b, scores, deltas, at_np, sigma, layout, A, upstream):
    """image b of a GPU result against the restatement -> the observed ulp distance of the values behind exp / log"""
    idx, tg, counts = at_np
    want = ln.rpn_loss(scores[b], deltas[b], idx[b], tg[b], counts[b], sigma, layout, A)
    gs, gd = ln.rpn_loss_backward(idx[b], want['row_grad_scores'], want['row_grad_deltas'], upstream[b], deltas.shape[1],
                                  layout, A)
    np.testing.assert_array_equal(got['row_grad_deltas'][b], want['row_grad_deltas'], err_msg=name)
    np.testing.assert_array_equal(got['grad_deltas'][b], gd, err_msg=name)
    assert got['losses'][b, 1] == want['losses'][1], (name, got['losses'][b], want['losses'])
    u = max(_ulps(got['losses'][b, :1], want['losses'][:1]), _ulps(got['row_grad_scores'][b], want['row_grad_scores']),
            _ulps(got['grad_scores'][b], gs))
    assert u <= 1, (name, u)
    return u, want


def test_rpn_losses_match_the_numpy_restatement():
    print()
    rng = np.random.default_rng(3)
    sigma = 3.0
    for name, shape, anchors, gt in _cases():
        N = anchors.shape[0]
        assert N % A_FPN == 0
        at = _anchor_targets([gt], shape, anchors, seed=5, first_image_id=2)
        at_np = (_np(at.sample_idx), _np(at.sample_targets), _np(at.counts))
        scores, deltas = _rpn_head(rng, at, N, sigma)
        upstream = np.float32([[0.75, -1.5]])
        for layout, A, s in ((ln.LAYOUT_FPN, 1, scores.reshape(1, -1)), (ln.LAYOUT_FRCNN, A_FPN, _frcnn(scores, A_FPN))):
            got = _run_rpn(s, deltas, at, sigma, layout, A, upstream)
            u, want = _compare_rpn(name, got, 0, s, deltas, at_np, sigma, layout, A, upstream)
            kfg = int(at_np[2][0, 3])
            if kfg >= 8:
                assert (want['sign'] == 1).any() and (want['sign'] == 0).any()
            print('%-14s layout %d  counts %s  losses %s  behind exp/log: max %d ulp'
                  % (name, layout, at_np[2][0].tolist(), got['losses'][0].tolist(), u))
            assert u == 0, 'expected 0 ulp against numpy (the rule allows 1): %d' % u


def test_dense_rpn_gradients_are_zero_elsewhere_and_layouts_agree():
    rng = np.random.default_rng(4)
    name, shape, anchors, gt = _cases()[1]
    N = anchors.shape[0]
    at = _anchor_targets([gt], shape, anchors, seed=1)
    idx = _np(at.sample_idx)[0]
    scores, deltas = _rpn_head(rng, at, N, 3.0)
    upstream = np.float32([[2.0, 0.5]])
    fpn = _run_rpn(scores.reshape(1, -1), deltas, at, 3.0, ln.LAYOUT_FPN, 1, upstream)
    frc = _run_rpn(_frcnn(scores, A_FPN), deltas, at, 3.0, ln.LAYOUT_FRCNN, A_FPN, upstream)
    touched = np.zeros(N, bool)
    touched[idx[idx >= 0]] = True
    assert touched.sum() == 256
    gs = fpn['grad_scores'][0].reshape(N, 2)
    assert np.all(gs[~touched] == 0) and np.all(fpn['grad_deltas'][0][~touched] == 0)
    assert np.all(np.abs(gs[touched]).sum(axis=1) > 0)
    np.testing.assert_array_equal(ln.fpn_view(frc['grad_scores'][0], ln.LAYOUT_FRCNN, A_FPN), gs)
    for k in ('losses', 'row_grad_scores', 'row_grad_deltas', 'grad_deltas'):
        np.testing.assert_array_equal(frc[k], fpn[k], err_msg=k)
    # a nullable output stays out
    from tf_eager_object_detection_amd import ops
    up = torch.from_numpy(upstream).cuda()
    only = ops.rpn_losses_backward(at.sample_idx, torch.from_numpy(fpn['row_grad_scores']).cuda(),
                                   torch.from_numpy(fpn['row_grad_deltas']).cuda(), up, N, scores=False)
    assert only.grad_scores is None
    np.testing.assert_array_equal(_np(only.grad_deltas), fpn['grad_deltas'])


def _roi_inputs(R, seed, shape=(800, 1333), G=12):
    rng = np.random.default_rng(seed)
    gt = syn.random_boxes(G, shape, rng, 40, 400)
    gt_labels = rng.integers(1, 21, G).astype(np.int64)
    near = (gt[rng.integers(0, G, R // 4)] + rng.normal(0, 10, (R // 4, 4))).astype(np.float32)
    rois = np.concatenate([syn.random_boxes(R - R // 4 - G, shape, rng, 16, 500), near, gt]).astype(np.float32)
    return rois, gt, gt_labels


def _proposal_targets(rois_list, gts, labels_list, C, S, seed=3, first_image_id=0):
    from tf_eager_object_detection_amd import ops
    gb, off = _pack(gts)
    gl = torch.from_numpy(np.concatenate([np.asarray(l, np.int64) for l in labels_list] + [np.zeros(1, np.int64)])).cuda()
    rois = torch.from_numpy(np.stack(rois_list)).cuda()
    return ops.proposal_targets(rois, gb, gl, off, C, 0.5, 0.0, S, S // 4, [0, 0, 0, 0], ROI_STDS, seed=seed,
                                first_image_id=first_image_id)


def _roi_head(rng, pt, R, C, sigma, row_map):
    tg, ins = _np(pt.targets), _np(pt.inside)
    B, S = tg.shape[:2]
    scores = rng.uniform(-30, 30, (B, R, C)).astype(np.float32)
    scores[:, ::2] = rng.normal(0, 2, scores[:, ::2].shape)
    deltas = rng.normal(0, 1, (B, R, 4 * C)).astype(np.float32)
    thr = 1.0 / sigma ** 2
    for b in range(B):
        m = np.arange(R) if row_map is None else row_map[b]
        ok = (m >= 0) & (m < S)
        near = tg[b][m[ok]] + rng.uniform(-2.5 * thr, 2.5 * thr, (int(ok.sum()), 4 * C))
        deltas[b, ok] = np.where(ins[b][m[ok]] != 0, near, deltas[b, ok]).astype(np.float32)
    return scores, deltas


def _run_roi(scores, deltas, pt, sigma, row_map, upstream):
    from tf_eager_object_detection_amd import ops
    rm = None if row_map is None else torch.from_numpy(np.ascontiguousarray(row_map, np.int32)).cuda()
    up = None if upstream is None else torch.from_numpy(np.asarray(upstream, np.float32)).cuda()
    out = ops.roi_losses(torch.from_numpy(scores).cuda(), torch.from_numpy(deltas).cuda(), pt.final_labels, pt.targets,
                         pt.inside, pt.outside, pt.counts, sigma, row_map=rm, upstream=up)
    torch.cuda.synchronize()
    return {k: _np(v) for k, v in out._asdict().items()}


def _compare_roi(name, got, b, scores, deltas, pt_np, sigma, row_map, upstream):
    labels, tg, ins, outs, counts = pt_np
    want = ln.roi_loss(scores[b], deltas[b], labels[b], tg[b], ins[b], outs[b], counts[b], sigma,
                       None if row_map is None else row_map[b], None if upstream is None else upstream[b])
    np.testing.assert_array_equal(got['grad_deltas'][b], want['grad_deltas'], err_msg=name)
    assert got['losses'][b, 1] == want['losses'][1], (name, got['losses'][b], want['losses'])
    u = max(_ulps(got['losses'][b, :1], want['losses'][:1]), _ulps(got['grad_scores'][b], want['grad_scores']))
    assert u <= 1, (name, u)
    return u, want


@pytest.mark.parametrize('C', [21, 81])
def test_roi_losses_match_the_numpy_restatement(C):
    print()
    rng = np.random.default_rng(50 + C)
    S, sigma = 256, 1.0
    rois, gt, gt_labels = _roi_inputs(2000, 12)
    pt = _proposal_targets([rois], [gt], [gt_labels], C, S)
    pt_np = tuple(_np(t) for t in (pt.final_labels, pt.targets, pt.inside, pt.outside, pt.counts))
    assert pt_np[4][0, 3] == S and pt_np[4][0, 2] > 8
    perm = rng.permutation(S).astype(np.int32)[None]
    holes = perm.copy()
    holes[0, rng.choice(S, 5, replace=False)] = -1
    for name, row_map, upstream in (('identity', None, None), ('permutation', perm, np.float32([[1.25, -0.5]])),
                                    ('with -1 rows', holes, np.float32([[0.3, 7.0]])), ('first 100 rows', perm[:, :100], None)):
        R = S if row_map is None else row_map.shape[1]
        scores, deltas = _roi_head(rng, pt, R, C, sigma, row_map)
        got = _run_roi(scores, deltas, pt, sigma, row_map, upstream)
        u, want = _compare_roi(name, got, 0, scores, deltas, pt_np, sigma, row_map, upstream)
        act = want['active']
        assert (want['sign'][act] == 1).any() and (want['sign'][act] == 0).any()
        if name == 'with -1 rows':
            out = holes[0] < 0
            assert np.all(got['grad_scores'][0][out] == 0) and np.all(got['grad_deltas'][0][out] == 0)
        print('C %2d %-14s counts %s  losses %s  behind exp/log: max %d ulp'
              % (C, name, pt_np[4][0].tolist(), got['losses'][0].tolist(), u))
        assert u == 0, 'expected 0 ulp against numpy (the rule allows 1): %d' % u
    # losses only / gradients only give the same bits
    from tf_eager_object_detection_amd import ops
    s, d = torch.from_numpy(scores).cuda(), torch.from_numpy(deltas).cuda()
    rm = torch.from_numpy(np.ascontiguousarray(row_map)).cuda()
    a = ops.roi_losses(s, d, pt.final_labels, pt.targets, pt.inside, pt.outside, pt.counts, sigma, row_map=rm, grads=False)
    g = ops.roi_losses(s, d, pt.final_labels, pt.targets, pt.inside, pt.outside, pt.counts, sigma, row_map=rm, losses=False)
    assert a.grad_scores is None and g.losses is None
    np.testing.assert_array_equal(_np(a.losses), got['losses'])
    np.testing.assert_array_equal(_np(g.grad_deltas), got['grad_deltas'])


def test_empty_and_over_limit_images_give_zeros():
    """an image without a kept row (counts row -1: more boxes than the target stage takes) and a RoI image that wrote nothing"""
    from tf_eager_object_detection_amd import ops
    shape = (320, 480)
    anchors = co.fpn_anchors(shape)
    N = anchors.shape[0]
    rng = np.random.default_rng(8)
    gts = [syn.random_boxes(5, shape, rng, 30, 200), syn.random_boxes(1025, shape, rng, 30, 200)]
    gb, off = _pack(gts)
    at = ops.anchor_targets(torch.from_numpy(anchors).cuda(), gb, off, shape, 0.7, 0.3, 256, 128, [0, 0, 0, 0], [1, 1, 1, 1])
    assert _np(at.counts)[1].tolist() == [-1] * 5
    scores, deltas = _rpn_head(rng, at, N, 3.0)
    got = _run_rpn(scores.reshape(2, -1), deltas, at, 3.0, ln.LAYOUT_FPN, 1, np.float32([[1, 1], [3, 4]]))
    assert got['losses'][0, 0] > 0 and np.all(got['losses'][1] == 0)
    for k in ('row_grad_scores', 'row_grad_deltas', 'grad_scores', 'grad_deltas'):
        assert np.all(got[k][1] == 0) and np.any(got[k][0] != 0), k
    # RoI: image 1 has no written row
    rois, gt, gt_labels = _roi_inputs(600, 5, shape=(600, 800), G=6)
    pt = _proposal_targets([rois, rois], [gt, gt], [gt_labels, gt_labels], 21, 128)
    counts = pt.counts.clone()
    counts[1] = torch.tensor([0, 0, 0, 0], dtype=torch.int32)
    pt0 = pt._replace(counts=counts)
    scores, deltas = _roi_head(rng, pt, 128, 21, 1.0, None)
    got = _run_roi(scores, deltas, pt0, 1.0, None, None)
    assert got['losses'][0, 0] > 0 and np.all(got['losses'][1] == 0)
    assert np.all(got['grad_scores'][1] == 0) and np.all(got['grad_deltas'][1] == 0)


def test_image_alone_equals_image_in_a_batch_of_eight():
    shape = (320, 480)
    anchors = co.fpn_anchors(shape)
    N = anchors.shape[0]
    rng = np.random.default_rng(33)
    gts = [syn.random_boxes(g, shape, rng, 30, 200) for g in (1, 7, 30, 2, 100, 5, 12, 3)]
    at = _anchor_targets(gts, shape, anchors, seed=9, first_image_id=0)
    scores, deltas = _rpn_head(rng, at, N, 3.0)
    upstream = rng.normal(0, 1, (8, 2)).astype(np.float32)
    batch = _run_rpn(scores.reshape(8, -1), deltas, at, 3.0, ln.LAYOUT_FPN, 1, upstream)
    for b in range(8):
        one_at = _anchor_targets([gts[b]], shape, anchors, seed=9, first_image_id=b)
        one = _run_rpn(scores[b:b + 1].reshape(1, -1), deltas[b:b + 1], one_at, 3.0, ln.LAYOUT_FPN, 1, upstream[b:b + 1])
        for k, v in one.items():
            np.testing.assert_array_equal(batch[k][b], v[0], err_msg='rpn image %d %s' % (b, k))
    C, S = 21, 128
    inputs = [_roi_inputs(600, 60 + b, shape=(600, 800), G=3 + b) for b in range(8)]
    pt = _proposal_targets([i[0] for i in inputs], [i[1] for i in inputs], [i[2] for i in inputs], C, S)
    row_map = np.stack([rng.permutation(S) for _ in range(8)]).astype(np.int32)
    scores, deltas = _roi_head(rng, pt, S, C, 1.0, row_map)
    batch = _run_roi(scores, deltas, pt, 1.0, row_map, upstream)
    for b in range(8):
        one_pt = _proposal_targets([inputs[b][0]], [inputs[b][1]], [inputs[b][2]], C, S, first_image_id=b)
        one = _run_roi(scores[b:b + 1], deltas[b:b + 1], one_pt, 1.0, row_map[b:b + 1], upstream[b:b + 1])
        for k, v in one.items():
            np.testing.assert_array_equal(batch[k][b], v[0], err_msg='roi image %d %s' % (b, k))


def test_targets_losses_and_backward_replay_from_one_captured_graph():
    """targets -> losses -> backward captured once; the ground truth is overwritten in the same buffers and the graph replayed,
    twice: every result equals the eager calls on the new contents (a host read or an allocation between the stages would
    fail the capture or freeze the first contents' decisions)"""
    from tf_eager_object_detection_amd import ops
    shape = (320, 480)
    anchors_np = co.fpn_anchors(shape)
    anchors = torch.from_numpy(anchors_np).cuda()
    N, C, S = anchors_np.shape[0], 21, 128
    rng = np.random.default_rng(44)
    rois_np = np.stack([syn.random_boxes(300, shape, rng, 16, 300) for _ in range(2)])

    def contents(gs, jitter_seed):
        r = np.random.default_rng(jitter_seed)
        gts = [syn.random_boxes(g, shape, r, 30, 200) for g in gs]
        boxes = np.zeros((64, 4), np.float32)
        cat = np.concatenate(gts)
        boxes[:len(cat)] = cat
        labels = np.zeros(64, np.int32)
        labels[:len(cat)] = r.integers(1, 21, len(cat))
        rois = rois_np.copy()
        for b, g in enumerate(gts):
            rois[b, :120] = (g[r.integers(0, len(g), 120)] + r.normal(0, 6, (120, 4))).astype(np.float32)
        return boxes, np.cumsum([0] + list(gs)).astype(np.int32), labels, rois

    sets = [contents((7, 3), 1), contents((2, 30), 2), contents((11, 1), 3)]
    gb, off, gl, rois = (torch.from_numpy(x).cuda() for x in sets[0])
    rpn_s = torch.from_numpy(rng.normal(0, 3, (2, 2 * N)).astype(np.float32)).cuda()
    rpn_d = torch.from_numpy(rng.normal(0, 0.2, (2, N, 4)).astype(np.float32)).cuda()
    roi_s = torch.from_numpy(rng.normal(0, 3, (2, S, C)).astype(np.float32)).cuda()
    roi_d = torch.from_numpy(rng.normal(0, 0.7, (2, S, 4 * C)).astype(np.float32)).cuda()
    row_map = torch.from_numpy(np.stack([rng.permutation(S) for _ in range(2)]).astype(np.int32)).cuda()
    upstream = torch.tensor([[0.5, 2.0], [1.5, -1.0]], device='cuda')

    def run():
        at = ops.anchor_targets(anchors, gb, off, shape, 0.7, 0.3, 256, 128, [0, 0, 0, 0], [1, 1, 1, 1], seed=4,
                                first_image_id=10, dense=False)
        pt = ops.proposal_targets(rois, gb, gl, off, C, 0.5, 0.0, S, 32, [0, 0, 0, 0], ROI_STDS, seed=4, first_image_id=10)
        fwd = ops.rpn_losses(rpn_s, rpn_d, at.sample_idx, at.sample_targets, at.counts, 3.0, ops.RPN_LAYOUT_FRCNN, A_FPN)
        bwd = ops.rpn_losses_backward(at.sample_idx, fwd.row_grad_scores, fwd.row_grad_deltas, upstream, N,
                                      ops.RPN_LAYOUT_FRCNN, A_FPN)
        roi = ops.roi_losses(roi_s, roi_d, pt.final_labels, pt.targets, pt.inside, pt.outside, pt.counts, 1.0,
                             row_map=row_map, upstream=upstream)
        return [at.sample_idx, at.counts, pt.counts] + list(fwd) + list(bwd) + list(roi)
    run()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run()
    seen = []
    for nxt in sets[1:]:
        for dst, src in zip((gb, off, gl, rois), nxt):
            dst.copy_(torch.from_numpy(src))
        graph.replay()
        torch.cuda.synchronize()
        replayed = [t.clone() for t in captured]
        eager = run()
        torch.cuda.synchronize()
        for i, (r, e) in enumerate(zip(replayed, eager)):
            np.testing.assert_array_equal(_np(r), _np(e), err_msg='output %d' % i)
        seen.append(_np(replayed[3]).copy())
        assert np.all(_np(replayed[3]) > 0)
    assert not np.array_equal(seen[0], seen[1])               # the replays really did different work


def _dense_torch_losses(scores, deltas, dense, sigma, layout, A):
    """the callers' _get_rpn_loss on the dense targets of one image (float64 on the device)"""
    from tf_eager_object_detection_amd.model.losses import cls_loss, smooth_l1_loss
    labels, targets, inside, outside = (t.double() for t in dense)
    rows = scores.reshape(-1, 2) if layout == ln.LAYOUT_FPN else scores.reshape(-1, 2, A).permute(0, 2, 1).reshape(-1, 2)
    sel = torch.nonzero(labels >= 0)[:, 0]
    return (cls_loss(rows[sel], labels[sel]), smooth_l1_loss(deltas, targets, inside, outside, sigma, dim=[0, 1]),
            rows[sel], labels[sel])


def _z_label(logits, labels):
    z = logits - logits.max(dim=1, keepdim=True).values
    return _np(z.gather(1, labels.long()[:, None])[:, 0])


@pytest.mark.parametrize('layout,A', [(ln.LAYOUT_FPN, 1), (ln.LAYOUT_FRCNN, A_FPN)])
def test_autograd_matches_torch_autograd_on_the_dense_targets(layout, A):
    from tf_eager_object_detection_amd.model.losses import cls_loss, fused_roi_losses, fused_rpn_losses, smooth_l1_loss
    print()
    rng = np.random.default_rng(70)
    name, shape, anchors, gt = _cases()[0]
    N = anchors.shape[0]
    gts = [gt, syn.random_boxes(40, shape, rng, 30, 200)]
    at = _anchor_targets(gts, shape, anchors, seed=2, dense=True)
    scores_np, deltas_np = _rpn_head(rng, at, N, 3.0)
    if layout == ln.LAYOUT_FRCNN:
        scores_np = _frcnn(scores_np, A)
    w = np.float32([[0.75, -1.5], [2.0, 0.25]])
    wt = torch.from_numpy(w).cuda()
    s = torch.from_numpy(scores_np.reshape(2, -1)).cuda().requires_grad_()
    d = torch.from_numpy(deltas_np).cuda().requires_grad_()
    cls, reg = fused_rpn_losses(s, d, at, 3.0, layout, A)
    assert cls.shape == (2,) and reg.shape == (2,)
    (wt[:, 0] * cls + wt[:, 1] * reg).sum().backward()
    for b in range(2):
        s64 = torch.from_numpy(scores_np[b].astype(np.float64)).cuda().requires_grad_()
        d64 = torch.from_numpy(deltas_np[b].astype(np.float64)).cuda().requires_grad_()
        c64, r64, rows, labels = _dense_torch_losses(s64, d64, (at.labels[b], at.targets[b], at.inside[b], at.outside[b]),
                                                     3.0, layout, A)
        (float(w[b, 0]) * c64 + float(w[b, 1]) * r64).backward()
        got = dict(losses=np.array([cls[b].item(), reg[b].item()]), gs=_np(s.grad[b]).reshape(-1), gd=_np(d.grad[b]))
        want = dict(losses=np.array([c64.item(), r64.item()]), gs=_np(s64.grad).reshape(-1), gd=_np(d64.grad))
        n = int(at.counts[b, 3] + at.counts[b, 4])
        ln.check_bounds(got, want, n, 2, _z_label(rows.detach(), labels), ('losses', 'gs', 'gd'), upstream=w[b],
                        report='rpn autograd layout %d image %d' % (layout, b))
        assert np.count_nonzero(np.abs(got['gd']).sum(axis=1)) == int(at.counts[b, 3])
    if layout == ln.LAYOUT_FRCNN:
        return
    # RoI head: C = 21 with the level-order permutation's stand-in
    C, S = 21, 128
    inputs = [_roi_inputs(600, 80 + b, shape=(600, 800), G=4 + b) for b in range(2)]
    pt = _proposal_targets([i[0] for i in inputs], [i[1] for i in inputs], [i[2] for i in inputs], C, S)
    row_map = np.stack([rng.permutation(S) for _ in range(2)]).astype(np.int32)
    scores_np, deltas_np = _roi_head(rng, pt, S, C, 1.0, row_map)
    s = torch.from_numpy(scores_np).cuda().requires_grad_()
    d = torch.from_numpy(deltas_np).cuda().requires_grad_()
    rm = torch.from_numpy(row_map).cuda()
    cls, reg = fused_roi_losses(s, d, pt, 1.0, row_map=rm)
    (wt[:, 0] * cls + wt[:, 1] * reg).sum().backward()
    # only one of the pair: the other head tensor gets a zero gradient
    s1 = torch.from_numpy(scores_np).cuda().requires_grad_()
    d1 = torch.from_numpy(deltas_np).cuda().requires_grad_()
    fused_roi_losses(s1, d1, pt, 1.0, row_map=rm)[0].sum().backward()
    assert bool((d1.grad == 0).all()) and bool((s1.grad != 0).any())
    for b in range(2):
        sel = rm[b].long()
        s64 = torch.from_numpy(scores_np[b].astype(np.float64)).cuda().requires_grad_()
        d64 = torch.from_numpy(deltas_np[b].astype(np.float64)).cuda().requires_grad_()
        labels = pt.final_labels[b][sel]
        c64 = cls_loss(s64, labels)
        r64 = smooth_l1_loss(d64, pt.targets[b][sel].double(), pt.inside[b][sel].double(), pt.outside[b][sel].double(), 1.0)
        (float(w[b, 0]) * c64 + float(w[b, 1]) * r64).backward()
        got = dict(losses=np.array([cls[b].item(), reg[b].item()]), gs=_np(s.grad[b]), gd=_np(d.grad[b]))
        want = dict(losses=np.array([c64.item(), r64.item()]), gs=_np(s64.grad), gd=_np(d64.grad))
        ln.check_bounds(got, want, S, C, _z_label(s64.detach(), labels), ('losses', 'gs', 'gd'), upstream=w[b],
                        report='roi autograd image %d' % b)


def _own_proposals(m, img, frcnn):
    """the training-mode proposals of the model's own RPN for `img`"""
    with torch.no_grad():
        image = img.float().contiguous()
        if frcnn:
            return m._anchors_and_proposals(image, True)[5]
        shape = [int(image.shape[1]), int(image.shape[2])]
        p_list = m._neck(m._extractor(image, training=True), training=True)
        scores, deltas = m._get_fpn_head_results(p_list)
        return m._rpn_proposal((deltas, m._get_anchors(shape), m._fg_scores(scores), shape), training=True)


def _caller_losses(make, shape, frcnn, calls=2):
    """the four losses of `calls` successive training passes of a 'torch' and a 'hip' model of equal seed, what the torch
    model handed to its own loss functions (for the bounds) and the level-order permutations of both (FPN).  The ground
    truth is three of the model's own proposals (both models have the same weights, so the same proposals): RoIs with
    IoU 1 exist, so the RoI head has foreground rows, targets and inside weights to get right."""
    rng = np.random.default_rng(1)
    img = torch.from_numpy((rng.uniform(0, 255, (1,) + shape + (3,)) - 110).astype(np.float32)).cuda()
    gl = torch.tensor([3, 7, 12], device='cuda')
    out, seen, perms, gts = {}, [], {}, {}
    for kind in ('torch', 'hip'):
        torch.manual_seed(1)
        m = make(kind)
        rois = _own_proposals(m, img, frcnn)
        big = rois[((rois[:, 2] - rois[:, 0]) >= 24) & ((rois[:, 3] - rois[:, 1]) >= 24)]
        assert big.shape[0] >= 3, 'the random model proposes fewer than 3 boxes of 24 pixels'
        gt = big[[0, big.shape[0] // 3, 2 * big.shape[0] // 3]].clone()
        gts[kind] = _np(gt)
        if kind == 'torch':
            rpn_loss, roi_loss = m._get_rpn_loss, m._get_roi_loss

            def spy_rpn(*args):
                seen.append(('rpn', args))
                return rpn_loss(*args)

            def spy_roi(*args):
                seen.append(('roi', args))
                return roi_loss(*args)
            m._get_rpn_loss, m._get_roi_loss = spy_rpn, spy_roi
        if not frcnn:
            perms[kind] = []
            assign = m._assign_levels

            def spy_assign(all_rois, assign=assign, store=perms[kind]):
                r = assign(all_rois)
                store.append(_np(r[1]))
                return r
            m._assign_levels = spy_assign
        out[kind] = [[float(x) for x in m((img, gt, gl), training=True)] for _ in range(calls)]
    np.testing.assert_array_equal(gts['torch'], gts['hip'])
    return out, seen, perms


def _check_caller(out, seen, perms, A, frcnn, C):
    calls = len(out['torch'])
    for i in range(calls):
        (_, rpn), (_, roi) = seen[2 * i], seen[2 * i + 1]
        rows = rpn[0].float().reshape(-1, 2, A).permute(0, 2, 1).reshape(-1, 2) if frcnn else rpn[0].float().reshape(-1, 2)
        sel = torch.nonzero(rpn[2] >= 0)[:, 0]
        z_rpn = _z_label(rows[sel], rpn[2][sel])
        z_roi = _z_label(roi[0].float(), roi[2])
        t, h = out['torch'][i], out['hip'][i]
        n_fg = int((roi[2] > 0).sum())
        print('call %d  torch %s\n        hip   %s   (%d foreground RoI rows)' % (i, t, h, n_fg))
        assert all(np.isfinite(t)) and all(np.isfinite(h))
        assert abs(h[0] - t[0]) <= ln.ce_loss_bound(2, z_rpn), (i, 'rpn cls')
        assert abs(h[1] - t[1]) <= 2.0 ** -21 * abs(t[1]), (i, 'rpn reg')
        assert abs(h[2] - t[2]) <= ln.ce_loss_bound(C, z_roi), (i, 'roi cls')
        assert abs(h[3] - t[3]) <= 2.0 ** -21 * abs(t[3]), (i, 'roi reg')
        # every one of the four is exercised: foreground rows with different classes exist, all losses are non-zero
        assert n_fg >= 3 and len(np.unique(_np(roi[2]))) >= 3
        assert min(t) > 0 and min(h) > 0
        if not frcnn:                                      # the level order is a real permutation, the same in both models
            p = perms['torch'][i]
            assert not np.array_equal(p, np.arange(len(p))) and np.array_equal(np.sort(p), np.arange(len(p)))
            np.testing.assert_array_equal(perms['hip'][i], p)
    assert out['torch'][0] != out['torch'][1]              # the second call drew another sample: the image ids advanced


def test_fpn_caller_with_hip_training_losses():
    from tf_eager_object_detection_amd.model.base_fpn_model import ResnetV1Fpn
    with pytest.raises(ValueError, match="training_losses='hip' needs training_targets='hip'"):
        ResnetV1Fpn(depth=50, training_targets='torch', training_losses='hip', device='cpu')
    with pytest.raises(ValueError, match='training_losses'):
        ResnetV1Fpn(depth=50, training_targets='hip', training_losses='numpy', device='cpu')
    print()
    def make(kind):
        # a freshly initialised RpnHead proposes only small boxes (one pyramid level: the level order would be the identity);
        # a bias on its box layer, the same in both models, spreads the proposals' sizes over several levels
        m = ResnetV1Fpn(depth=50, training_targets='hip', training_losses=kind)
        with torch.no_grad():
            b = m.dense.rpn_bbox.bias
            b.add_(torch.linspace(0.0, 1.6, b.numel(), device=b.device, dtype=b.dtype))
        return m
    out, seen, perms = _caller_losses(make, (256, 352), False)
    _check_caller(out, seen, perms, 3, False, 21)


def test_faster_rcnn_caller_with_hip_training_losses():
    from tf_eager_object_detection_amd.model.base_faster_rcnn_model import ResNetFasterRcnn
    with pytest.raises(ValueError, match="training_losses='hip' needs training_targets='hip'"):
        ResNetFasterRcnn(depth=50, training_losses='hip', device='cpu')
    print()
    out, seen, perms = _caller_losses(lambda kind: ResNetFasterRcnn(depth=50, training_targets='hip', training_losses=kind),
                                      (256, 352), True)
    _check_caller(out, seen, perms, 9, True, 21)
