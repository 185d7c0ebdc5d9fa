"""The fused training targets (csrc/targets.hip) where random float boxes and real Philox keys never take them:
A. the selection under the diagnostic build's key mask (odet_debug_tg_key_mask), which makes keys collide so that
   d_tg_radix_select walks all seven digits, ends in each of its three exit shapes and meets thresholds with equal keys
   (tests/test_targets_edges_host.py proves that the committed masks and cases do that);
B. IoU ties and IoUs exactly on a threshold, from hand-made integer boxes, through the product library;
C. the device-side report of an image above 1024 boxes, in the middle of a batch.
Comparisons are exact on every output of both calls; values behind `log` keep the bar of tests/test_targets_gpu.py: the bits of
`ops.encode`, and at most one unit in the last place against numpy."""
import numpy as np
import pytest
import torch

import targets_edge_cases as ec
import targets_np as tn
from oracle import oracle_np as on

pytestmark = pytest.mark.gpu

ANCHOR_KEYS = ('labels', 'inside', 'outside', 'sample_idx', 'counts', 'labels_before_sampling', 'argmax')
ROI_KEYS = ('keep', 'final_labels', 'final_rois', 'counts', 'inside', 'outside')


def _ulps(a, b):
    ia = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -2 ** 31 - ia, ia)
    ib = np.where(ib < 0, -2 ** 31 - ib, ib)
    return int(np.abs(ia - ib).max()) if ia.size else 0


def _pack(gts):
    """packed boxes that really hold every row of every image (+ one spare row), and the offsets"""
    off = np.cumsum([0] + [len(g) for g in gts]).astype(np.int32)
    boxes = np.concatenate([np.asarray(g, np.float32).reshape(-1, 4) for g in gts] + [np.zeros((1, 4), np.float32)])
    assert len(boxes) == off[-1] + 1
    return torch.from_numpy(boxes).cuda(), torch.from_numpy(off).cuda()


def _anchor_call(gts, shape, anchors, pos, neg, total, max_pos, seed=ec.SEED, first_image_id=ec.IMAGE_ID):
    from tf_eager_object_detection_amd import ops
    gb, off = _pack(gts)
    out = ops.anchor_targets(torch.from_numpy(np.ascontiguousarray(anchors, np.float32)).cuda(), gb, off, shape, pos, neg, total,
                             max_pos, ec.MEANS, ec.STDS, seed=seed, first_image_id=first_image_id, dense=True, parity=True)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out._asdict().items()}


def _encode(boxes, gt):
    from tf_eager_object_detection_amd import ops
    if len(boxes) == 0:
        return np.zeros((0, 4), np.float32)
    return ops.encode(torch.from_numpy(np.ascontiguousarray(boxes, np.float32)).cuda(),
                      torch.from_numpy(np.ascontiguousarray(gt, np.float32)).cuda(), ec.MEANS, ec.STDS).cpu().numpy()


def _check_anchor(got, b, want, anchors, gt, msg):
    """image b of an anchor call against the numpy restatement `want` of that image: every output"""
    for k in ANCHOR_KEYS:
        np.testing.assert_array_equal(got[k][b], want[k], err_msg='%s %s' % (msg, k))
    idx = np.nonzero(want['argmax'] >= 0)[0]
    enc = _encode(anchors[idx], np.asarray(gt, np.float32).reshape(-1, 4)[want['argmax'][idx]])
    np.testing.assert_array_equal(got['targets'][b][idx], enc, err_msg='%s targets' % msg)
    rest = np.setdiff1d(np.arange(len(anchors)), idx)
    assert np.all(got['targets'][b][rest] == 0), msg
    k = int((want['sample_idx'] >= 0).sum())
    np.testing.assert_array_equal(got['sample_targets'][b][:k], got['targets'][b][want['sample_idx'][:k]], err_msg=msg)
    assert np.all(got['sample_targets'][b][k:] == 0), msg
    u = max(_ulps(got['targets'][b], want['targets']), _ulps(got['sample_targets'][b], want['sample_targets']))
    assert u <= 1, '%s: targets %d ulp from numpy' % (msg, u)
    return u


def _proposal_call(rois_list, gts, labels_list, neg, total, max_pos, pos=0.5, quirk=True, seed=ec.SEED,
                   first_image_id=ec.IMAGE_ID, roi_counts=None):
    from tf_eager_object_detection_amd import ops
    gb, off = _pack(gts)
    gl = torch.from_numpy(np.concatenate([np.asarray(l, np.int64) for l in labels_list] + [np.zeros(1, np.int64)])).cuda()
    rmax = max(len(r) for r in rois_list)
    rois = np.zeros((len(rois_list), rmax, 4), np.float32)
    for b, r in enumerate(rois_list):
        rois[b, :len(r)] = r
    rc = None if roi_counts is None else torch.tensor(roi_counts, dtype=torch.int32, device='cuda')
    out = ops.proposal_targets(torch.from_numpy(rois).cuda(), gb, gl, off, 21, pos, neg, total, max_pos, ec.MEANS, ec.STDS,
                               reference_row_labels=quirk, seed=seed, first_image_id=first_image_id, roi_counts=rc)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out._asdict().items()}


def _check_proposal(got, b, want, rois, gt, msg, quirk=True):
    """image b of a proposal call against the numpy restatement `want` of rois / gt: every output"""
    for k in ROI_KEYS:
        np.testing.assert_array_equal(got[k][b], want[k], err_msg='%s %s' % (msg, k))
    r = len(want['gt_assignment'])
    np.testing.assert_array_equal(got['gt_assignment'][b][:r], want['gt_assignment'], err_msg=msg)
    assert np.all(got['gt_assignment'][b][r:] == -1), msg
    nfg, total = int(want['counts'][2]), len(want['keep'])
    tg = got['targets'][b].reshape(total, 21, 4)
    gt = np.asarray(gt, np.float32).reshape(-1, 4)
    if nfg and len(gt):
        kfg, ga = want['keep'][:nfg], want['gt_assignment']
        enc = _encode(rois[kfg], gt[ga[kfg]])
        cols = want['final_labels'][:nfg] if not quirk else np.nonzero(want['inside'].reshape(total, 21, 4)[:nfg, :, 0])[1]
        np.testing.assert_array_equal(tg[np.arange(nfg), cols], enc, err_msg='%s targets' % msg)
        assert np.count_nonzero(tg) == np.count_nonzero(enc), msg
    else:
        assert np.all(tg == 0), msg
    u = _ulps(got['targets'][b], want['targets'])
    assert u <= 1, '%s: targets %d ulp from numpy' % (msg, u)
    return u


def _assert_mask_cleared():
    """a product-library call after the block equals its UNMASKED numpy result"""
    _, rois, gt, gl, neg, total, max_pos = ec.proposal_sampling_cases()[0]
    got = _proposal_call([rois], [gt], [gl], neg, total, max_pos)
    want = tn.proposal_target(rois, gt, gl, 21, 0.5, neg, total, max_pos, ec.MEANS, ec.STDS, True, seed=ec.SEED, image_id=ec.IMAGE_ID)
    _check_proposal(got, 0, want, rois, gt, 'after the diagnostic block')
    masked = tn.proposal_target(rois, gt, gl, 21, 0.5, neg, total, max_pos, ec.MEANS, ec.STDS, True, seed=ec.SEED,
                                image_id=ec.IMAGE_ID, key_mask=0)
    assert not np.array_equal(masked['keep'], want['keep'])


# ------------------------------------------------------------------------------------------ A. selection under masks --
@pytest.mark.parametrize('mask', ec.KEY_MASKS, ids=lambda m: '%016x' % m)
def test_anchor_selection_under_key_mask(mask):
    from tools._diag import diag_library
    with diag_library() as lib:
        assert lib.odet_debug_tg_key_mask(mask) == 0
        for name, shape, anchors, gt, total, max_pos in ec.anchor_sampling_cases():
            got = _anchor_call([gt], shape, anchors, 0.7, 0.3, total, max_pos)
            want = tn.anchor_target(gt, shape, anchors, 0.7, 0.3, total, max_pos, ec.MEANS, ec.STDS, seed=ec.SEED,
                                    image_id=ec.IMAGE_ID, key_mask=mask)
            _check_anchor(got, 0, want, anchors, gt, 'mask %016x %s' % (mask, name))
            print('mask %016x %-16s counts %s' % (mask, name, want['counts'].tolist()))
    _assert_mask_cleared()


@pytest.mark.parametrize('mask', ec.KEY_MASKS, ids=lambda m: '%016x' % m)
def test_proposal_selection_under_key_mask(mask):
    from tools._diag import diag_library
    with diag_library() as lib:
        assert lib.odet_debug_tg_key_mask(mask) == 0
        for name, rois, gt, gl, neg, total, max_pos in ec.proposal_sampling_cases():
            for quirk in (True, False):
                got = _proposal_call([rois], [gt], [gl], neg, total, max_pos, quirk=quirk)
                want = tn.proposal_target(rois, gt, gl, 21, 0.5, neg, total, max_pos, ec.MEANS, ec.STDS, quirk, seed=ec.SEED,
                                          image_id=ec.IMAGE_ID, key_mask=mask)
                _check_proposal(got, 0, want, rois, gt, 'mask %016x %s quirk=%s' % (mask, name, quirk), quirk)
            print('mask %016x %-16s counts %s' % (mask, name, want['counts'].tolist()))
    _assert_mask_cleared()


@pytest.mark.parametrize('mask', [0, 0x0010010010010011], ids=lambda m: '%016x' % m)
def test_batch_of_four_under_key_mask_equals_single_images(mask):
    """thresholds are per image, also when keys collide within and across images"""
    from tools._diag import diag_library
    from tf_eager_object_detection_amd import synthetic as syn
    shape, anchors, gt100, _ = ec._big_anchor_inputs()
    rng = np.random.default_rng(33)
    gts = [syn.random_boxes(7, shape, rng, 16, 600), gt100, gt100[:40], np.zeros((0, 4), np.float32)]
    rois, rgt, rgl = ec._roi_inputs()
    roi_sets = [rois, rois[380:460], rois[200:], rois[:300]]
    with diag_library() as lib:
        assert lib.odet_debug_tg_key_mask(mask) == 0
        batch = _anchor_call(gts, shape, anchors, 0.7, 0.3, 256, 128, first_image_id=0)
        for b, gt in enumerate(gts):
            one = _anchor_call([gt], shape, anchors, 0.7, 0.3, 256, 128, first_image_id=b)
            for k, v in one.items():
                np.testing.assert_array_equal(batch[k][b], v[0], err_msg='image %d %s' % (b, k))
            want = tn.anchor_target(gt, shape, anchors, 0.7, 0.3, 256, 128, ec.MEANS, ec.STDS, seed=ec.SEED, image_id=b, key_mask=mask)
            _check_anchor(batch, b, want, anchors, gt, 'mask %016x batch image %d' % (mask, b))
        pb = _proposal_call(roi_sets, [rgt] * 4, [rgl] * 4, 0.0, 128, 32, first_image_id=0, roi_counts=[len(r) for r in roi_sets])
        for b, r in enumerate(roi_sets):
            one = _proposal_call([r], [rgt], [rgl], 0.0, 128, 32, first_image_id=b)
            for k, v in one.items():
                n = v.shape[1] if k == 'gt_assignment' else None
                np.testing.assert_array_equal(pb[k][b][:n], v[0], err_msg='image %d %s' % (b, k))
            want = tn.proposal_target(r, rgt, rgl, 21, 0.5, 0.0, 128, 32, ec.MEANS, ec.STDS, True, seed=ec.SEED, image_id=b, key_mask=mask)
            _check_proposal(pb, b, want, r, rgt, 'mask %016x batch image %d' % (mask, b))
    # the mask is gone: the product library gives the unmasked sample of the same anchor case
    got = _anchor_call([gts[1]], shape, anchors, 0.7, 0.3, 256, 128)
    want = tn.anchor_target(gts[1], shape, anchors, 0.7, 0.3, 256, 128, ec.MEANS, ec.STDS, seed=ec.SEED, image_id=ec.IMAGE_ID)
    _check_anchor(got, 0, want, anchors, gts[1], 'after the diagnostic block')
    _assert_mask_cleared()


# ------------------------------------------------------------------------------------------ B. ties and thresholds --
@pytest.mark.parametrize('case', ec.anchor_tie_cases(), ids=lambda c: c[0])
def test_anchor_ties_and_thresholds(case):
    name, anchors, gt = case
    got = _anchor_call([gt], ec.TIE_SHAPE, anchors, ec.POS, ec.NEG, 256, 128)
    idx, labels, argmax = on.anchor_target_labels(gt, ec.TIE_SHAPE, anchors, ec.POS, ec.NEG)
    n = len(anchors)
    want_l = -np.ones(n, np.int32); want_l[idx] = labels
    want_a = -np.ones(n, np.int32); want_a[idx] = argmax
    np.testing.assert_array_equal(got['labels_before_sampling'][0], want_l, err_msg=name)
    np.testing.assert_array_equal(got['argmax'][0], want_a, err_msg=name)
    assert got['counts'][0, :3].tolist() == [len(idx), int((labels == 1).sum()), int((labels == 0).sum())], name
    want = tn.anchor_target(gt, ec.TIE_SHAPE, anchors, ec.POS, ec.NEG, 256, 128, ec.MEANS, ec.STDS, seed=ec.SEED, image_id=ec.IMAGE_ID)
    u = _check_anchor(got, 0, want, anchors, gt, name)
    print('%-26s N %4d G %4d counts %s  targets vs numpy: max %d ulp' % (name, n, len(gt), want['counts'].tolist(), u))


def test_anchor_tie_cases_in_one_batch_equal_their_single_calls():
    """the three lattice box sets (G = 1, 257, 1024) over one anchor set, next to each other in a batch"""
    cases = {n: (a, g) for n, a, g in ec.anchor_tie_cases()}
    anchors = cases['lattice-G1024'][0]
    gts = [cases['lattice-G1'][1], cases['lattice-G1024'][1], cases['lattice-G257'][1], cases['lattice-G1024'][1][::-1].copy()]
    batch = _anchor_call(gts, ec.TIE_SHAPE, anchors, ec.POS, ec.NEG, 256, 128, first_image_id=0)
    for b, gt in enumerate(gts):
        want = tn.anchor_target(gt, ec.TIE_SHAPE, anchors, ec.POS, ec.NEG, 256, 128, ec.MEANS, ec.STDS, seed=ec.SEED, image_id=b)
        _check_anchor(batch, b, want, anchors, gt, 'image %d' % b)


def test_proposal_ties_thresholds_and_empty_images():
    """duplicated RoI rows, IoU = pos, IoU = neg (first two images), roi_counts = 0 and G = 0, in one batch and alone"""
    (n1, r1, g1, l1), (n2, r2, g2, l2) = ec.proposal_tie_cases()
    none = np.zeros((0, 4), np.float32)
    for neg in (ec.NEG, 0.0):
        rois_list, gts, labels = [r1, r2, r2, r1], [g1, g2, g2, none], [l1, l2, l2, np.zeros(0, np.int64)]
        counts = [len(r1), len(r2), 0, len(r1)]
        got = _proposal_call(rois_list, gts, labels, neg, 128, 32, pos=ec.POS, first_image_id=0, roi_counts=counts)
        for b in range(4):
            rois = rois_list[b][:counts[b]]
            want = tn.proposal_target(rois, gts[b], labels[b], 21, ec.POS, neg, 128, 32, ec.MEANS, ec.STDS, True, seed=ec.SEED,
                                      image_id=b)
            _check_proposal(got, b, want, rois, gts[b], 'neg %s image %d' % (neg, b))
            if len(gts[b]) and len(rois):
                _, ga, fg, bg = on.proposal_target_assign(rois, gts[b], labels[b], ec.POS, neg)
                np.testing.assert_array_equal(got['gt_assignment'][b][:len(rois)], ga)
                assert got['counts'][b, :2].tolist() == [len(fg), len(bg)]
            one = _proposal_call([rois_list[b]], [gts[b]], [labels[b]], neg, 128, 32, pos=ec.POS, first_image_id=b,
                                 roi_counts=[counts[b]])
            for k, v in one.items():
                n = v.shape[1] if k == 'gt_assignment' else None
                np.testing.assert_array_equal(got[k][b][:n], v[0], err_msg='neg %s image %d %s' % (neg, b, k))
        assert got['counts'][2].tolist() == [0, 0, 0, 0] and np.all(got['keep'][2] == -1)           # roi_counts = 0
        n_bg = len(r1) if neg == 0.0 else 0                                                          # G = 0: row maximum 0
        assert got['counts'][3].tolist() == [0, n_bg, 0, 128 if n_bg else 0] and np.all(got['gt_assignment'][3] == -1)
        print('neg %-4s counts %s' % (neg, got['counts'].tolist()))


# ------------------------------------------------------------------------------------------ C. over-limit images --
def test_image_above_the_box_limit_is_reported_on_the_device_and_leaves_its_neighbours_alone():
    """G = 5, 1025, 5: the middle image gets the header's fill values (a `counts` row of -1, labels -1, no sampled row, the
    index outputs argmax / gt_assignment -1 as on every row without ground truth, everything else 0); images 0 and 2 equal
    their single-image results bit for bit"""
    cases = {n: (a, g) for n, a, g in ec.anchor_tie_cases()}
    anchors, many = cases['lattice-G1024']
    rng = np.random.default_rng(8)
    over = np.concatenate([many, many[:1]])
    gts = [many[:5], over, many[300:305]]
    assert [len(g) for g in gts] == [5, 1025, 5]
    got = _anchor_call(gts, ec.TIE_SHAPE, anchors, ec.POS, ec.NEG, 256, 128, first_image_id=0)
    assert np.all(got['counts'][1] == -1)
    assert np.all(got['labels'][1] == -1) and np.all(got['labels_before_sampling'][1] == -1) and np.all(got['argmax'][1] == -1)
    assert np.all(got['sample_idx'][1] == -1)
    for k in ('targets', 'inside', 'outside', 'sample_targets'):
        assert np.all(got[k][1] == 0) and not np.any(np.signbit(got[k][1])), k
    for b in (0, 2):
        one = _anchor_call([gts[b]], ec.TIE_SHAPE, anchors, ec.POS, ec.NEG, 256, 128, first_image_id=b)
        for k, v in one.items():
            np.testing.assert_array_equal(got[k][b], v[0], err_msg='image %d %s' % (b, k))
        want = tn.anchor_target(gts[b], ec.TIE_SHAPE, anchors, ec.POS, ec.NEG, 256, 128, ec.MEANS, ec.STDS, seed=ec.SEED, image_id=b)
        _check_anchor(got, b, want, anchors, gts[b], 'image %d' % b)
    rois = ec.proposal_tie_cases()[1][1]
    labels = [rng.integers(1, 21, len(g)).astype(np.int64) for g in gts]
    pg = _proposal_call([rois] * 3, gts, labels, ec.NEG, 128, 32, pos=ec.POS, first_image_id=0)
    assert np.all(pg['counts'][1] == -1) and np.all(pg['keep'][1] == -1) and np.all(pg['gt_assignment'][1] == -1)
    for k in ('final_rois', 'final_labels', 'targets', 'inside', 'outside'):
        assert np.all(pg[k][1] == 0), k
    for b in (0, 2):
        one = _proposal_call([rois], [gts[b]], [labels[b]], ec.NEG, 128, 32, pos=ec.POS, first_image_id=b)
        for k, v in one.items():
            np.testing.assert_array_equal(pg[k][b], v[0], err_msg='image %d %s' % (b, k))
        want = tn.proposal_target(rois, gts[b], labels[b], 21, ec.POS, ec.NEG, 128, 32, ec.MEANS, ec.STDS, True, seed=ec.SEED, image_id=b)
        _check_proposal(pg, b, want, rois, gts[b], 'image %d' % b)
