"""COCO evaluation on the GPU (-m gpu): odet_eval_detect_topk against the oracle's composition of the script's loop, the
odet_coco_* launches against the plain-Python restatement of COCOeval (tests/coco_eval_np.py) -- every compared array
exactly equal -- and eval_coco end to end."""
import numpy as np
import pytest
import torch

from coco_eval_np import CocoEvalNp
from oracle import oracle_np as on
from tf_eager_object_detection_amd import _lib as L
from tf_eager_object_detection_amd import preprocess as P
from tf_eager_object_detection_amd import synthetic as syn
from tf_eager_object_detection_amd.evaluation import coco_eval as ce

pytestmark = pytest.mark.gpu

COCO_DET = dict(score_threshold=0.0, iou_threshold=0.3, max_objects_per_class=100, max_objects_per_image=100,
                min_size=10)


def _ulp_le1(a, b):
    ia = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -2 ** 31 - ia, ia)
    ib = np.where(ib < 0, -2 ** 31 - ib, ib)
    return ia.size == 0 or int(np.abs(ia - ib).max()) <= 1


def _oracle_topk(scores, deltas, rois, img_scale, raw_h, raw_w, num_classes=81, **kw):
    """eval_coco.py:117-160 composed from the oracle: the per-class loop without the PASCAL cap, concatenation in class
    order, tf.nn.top_k(min(max_per_image, n), sorted=False) = (score desc, position asc)."""
    mpi = kw.pop('max_objects_per_image')
    per = on.eval_detect_image(scores, deltas, rois, img_scale, raw_h, raw_w, num_classes=num_classes,
                               max_objects_per_image=0, **kw)
    dets = np.concatenate([per[j] for j in range(1, num_classes)], axis=0)
    labels = np.concatenate([np.full(len(per[j]), j, np.int32) for j in range(1, num_classes)])
    _, idx = on.tf_top_k(dets[:, 4], min(mpi, len(dets)), sorted=False)
    return dets[idx, :4], labels[idx], dets[idx, 4]


@pytest.mark.parametrize('R,decimals', [(300, 2), (1500, 2), (1000, 1)])
def test_eval_detect_topk_matches_the_oracle_composition(R, decimals):
    rng = np.random.default_rng(R + decimals)
    im = syn.eval_image(rng, raw_shape=(427, 640), num_rois=R, num_classes=81)
    sc = np.round(im['scores'] * 8, decimals).astype(np.float32)      # (many ties, also at the 100th score)
    g = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    boxes, labels, scores = ce.detect_image_coco(g(sc), g(im['deltas']), g(im['rois']), im['img_scale'], im['raw_h'],
                                                 im['raw_w'], **COCO_DET)
    wb, wl, ws = _oracle_topk(sc, im['deltas'], im['rois'], im['img_scale'], im['raw_h'], im['raw_w'], **COCO_DET)
    assert len(ws) == 100
    assert np.count_nonzero(ws == ws[-1]) > 1                           # a tie at the k-th score is cut
    np.testing.assert_array_equal(scores, ws)
    np.testing.assert_array_equal(labels, wl)
    assert _ulp_le1(boxes, wb)                                           # (decode's exp: smoke()'s rule)


def test_eval_detect_topk_empty_image():
    rng = np.random.default_rng(3)
    im = syn.eval_image(rng, raw_shape=(300, 400), num_rois=200, num_classes=81)
    g = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    zero = np.zeros_like(im['scores'])
    boxes, labels, scores = ce.detect_image_coco(g(zero), g(im['deltas']), g(im['rois']), im['img_scale'],
                                                 im['raw_h'], im['raw_w'], **COCO_DET)
    assert boxes.shape == (0, 4) and labels.shape == (0,) and scores.shape == (0,)
    assert ce.coco_records([(boxes, labels, scores)], [1], list(range(1, 81))) == []


# ---- COCO-like sets -------------------------------------------------------------------------------------------------
def coco_like(seed, n_img, n_cat, gt_per_img=7, det_per_img=100, big_segment=0, no_result_images=0):
    rng = np.random.default_rng(seed)
    img_ids = [int(i) for i in rng.choice(np.arange(1, 20 * n_img + 2), n_img, replace=False)]
    cat_ids = sorted(int(c) for c in rng.choice(np.arange(1, 3 * n_cat + 2), n_cat, replace=False))
    file_cats = [cat_ids[i] for i in rng.permutation(n_cat)]
    anns, res = [], []
    for ii, img in enumerate(img_ids):
        ng = int(rng.poisson(gt_per_img)) if ii % 11 else 0
        gts = []
        for _ in range(ng):
            w, h = float(np.round(rng.uniform(4, 300), 2)), float(np.round(rng.uniform(4, 300), 2))
            x, y = float(np.round(rng.uniform(0, 500), 2)), float(np.round(rng.uniform(0, 400), 2))
            area = w * h * float(rng.uniform(0.55, 1.0))
            u = rng.random()
            if u < 0.04:
                area = 1024.0
            elif u < 0.08:
                area = 9216.0
            c = cat_ids[int(min(rng.zipf(1.6), n_cat)) - 1]
            gts.append((c, [x, y, w, h]))
            anns.append({'id': len(anns) + 1, 'image_id': img, 'category_id': c, 'bbox': [x, y, w, h], 'area': area,
                         'iscrowd': int(rng.random() < 0.01)})
        if ii < no_result_images:
            continue
        for k in range(det_per_img):
            if gts and rng.random() < 0.6:
                c, (x, y, w, h) = gts[int(rng.integers(len(gts)))]
                if rng.random() < 0.15:
                    c = cat_ids[int(rng.integers(n_cat))]
                if rng.random() < 0.1:
                    box = [x, y, w, h]                                          # duplicate of a GT box
                else:
                    j = rng.normal(0, 0.08, 4)
                    box = [float(np.round(x + j[0] * w, 2)), float(np.round(y + j[1] * h, 2)),
                           float(np.round(w * (1 + j[2]), 2)), float(np.round(h * (1 + j[3]), 2))]
            else:
                c = cat_ids[int(rng.integers(n_cat))]
                box = [float(np.round(v, 2)) for v in (rng.uniform(0, 500), rng.uniform(0, 400), rng.uniform(2, 200),
                                                       rng.uniform(2, 200))]
            res.append({'image_id': img, 'category_id': c, 'bbox': box, 'score': float(np.round(rng.random(), 2))})
    for k in range(big_segment):                                                # one segment above maxDets[-1]
        res.append({'image_id': img_ids[1], 'category_id': cat_ids[0],
                    'bbox': [float(np.round(v, 2)) for v in rng.uniform(0, 300, 4)],
                    'score': float(np.round(rng.random(), 2))})
    order = rng.permutation(len(res))
    res = [res[i] for i in order]
    gt = {'images': [{'id': i} for i in img_ids], 'categories': [{'id': c} for c in file_cats], 'annotations': anns}
    return gt, res


def _check_matches(got, ev):
    segs = ev.segment_matches()
    assert len(segs) == len(got['seg_cat'])
    off = got['entry_off']
    for s, (k, i, sc, m, ig, npig) in enumerate(segs):
        assert got['seg_cat'][s] == k and got['seg_img'][s] == i
        e0, e1 = off[s], off[s + 1]
        np.testing.assert_array_equal(got['dt_score'][e0:e1], sc)
        np.testing.assert_array_equal(got['dt_matched'][e0:e1].transpose(1, 2, 0), m)
        np.testing.assert_array_equal(got['dt_ignored'][e0:e1].transpose(1, 2, 0), ig)
        np.testing.assert_array_equal(got['dt_rank'][e0:e1], np.arange(e1 - e0))
        np.testing.assert_array_equal(got['npig'][s], npig)


def _check_all(got, ev):
    for key in ('precision', 'recall', 'scores'):
        assert np.array_equal(got[key], ev.eval[key]), key
    assert np.array_equal(got['stats'], ev.stats)


@pytest.mark.parametrize('seed,n_img,n_cat,big', [(1, 3, 2, 0), (2, 40, 8, 150), (3, 120, 20, 0)])
def test_match_and_accumulate_equal_the_restatement(seed, n_img, n_cat, big):
    gt, res = coco_like(seed, n_img, n_cat, det_per_img=30 if n_img > 3 else 6, big_segment=big, no_result_images=2)
    got = ce.coco_evaluate(gt, res)
    ev = CocoEvalNp(gt, res).run()
    _check_matches(got, ev)
    _check_all(got, ev)
    assert (got['precision'] > 0).any() and (got['precision'] == -1).any() or n_img == 3


def test_val_sized_slice_equals_the_restatement():
    gt, res = coco_like(7, 500, 80, det_per_img=100, big_segment=120, no_result_images=5)
    got = ce.coco_evaluate(gt, res)
    ev = CocoEvalNp(gt, res).run()
    _check_matches(got, ev)
    _check_all(got, ev)
    assert got['stats'][0] > 0


def test_image_subset_and_result_file(tmp_path):
    gt, res = coco_like(11, 30, 6, det_per_img=20, no_result_images=4)
    sub = sorted(im['id'] for im in gt['images'])[3:20]
    p = tmp_path / 'res.json'
    ce.write_coco_results_file(str(p), res)
    got = ce.coco_evaluate(gt, str(p), image_ids=sub)
    ev = CocoEvalNp(gt, res, img_ids=sub).run()
    _check_matches(got, ev)
    _check_all(got, ev)


def test_limits_raise_and_the_next_call_succeeds():
    gt, res = coco_like(5, 4, 2, det_per_img=10)
    img, cat = gt['images'][0]['id'], gt['categories'][0]['id']
    many = res + [{'image_id': img, 'category_id': cat, 'bbox': [1.0, 1.0, 5.0, 5.0], 'score': 0.5}] * 4097
    with pytest.raises(L.OdetError, match='exceed'):
        ce.coco_evaluate(gt, many)
    gt2 = dict(gt, annotations=gt['annotations'] + [
        {'id': 100000 + k, 'image_id': img, 'category_id': cat, 'bbox': [1.0, 1.0, 5.0, 5.0], 'area': 25.0,
         'iscrowd': 0} for k in range(1025)])
    with pytest.raises(L.OdetError, match='exceed'):
        ce.coco_evaluate(gt2, res)
    got = ce.coco_evaluate(gt, res)
    _check_all(got, CocoEvalNp(gt, res).run())


def test_eval_coco_end_to_end_matches_the_manual_chain():
    from tf_eager_object_detection_amd.model.base_fpn_model import ResnetV1Fpn
    torch.manual_seed(3)
    m = ResnetV1Fpn(depth=50, num_classes=81, rpn_proposal_num_post_nms_test=300, prediction_score_threshold=0.0)
    rng = np.random.default_rng(5)
    raws = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((150, 200), (171, 133), (120, 160))]
    ids = [42, 7, 13]
    edges = dict(min_edge=256, max_edge=352)
    cats = list(range(1, 91, 1))[:80]
    # the manual chain: preprocessing -> im_detect -> the oracle loop with the top-k cap -> records
    dets = []
    for r in raws:
        batch, scales, raw = P.preprocess_images([r], 'coco', **edges)
        s, d, rois = m.im_detect(batch, scales[0])
        dets.append(_oracle_topk(s.cpu().numpy(), d.cpu().numpy(), rois.cpu().numpy(), 1.0, raw[0][0], raw[0][1],
                                 **COCO_DET))
    want_records = ce.coco_records(dets, ids, cats)
    assert len(want_records) > 0
    # ground truth: some of the detections (so that there are matches), some misses, one crowd, an image without GT
    anns = []
    for k, rec in enumerate(want_records[::7][:30]):
        x, y, w, h = rec['bbox']
        anns.append({'id': k + 1, 'image_id': rec['image_id'], 'category_id': rec['category_id'],
                     'bbox': [x + 0.5, y, w, h - 1.0], 'area': w * h, 'iscrowd': int(k == 3)})
    anns.append({'id': 999, 'image_id': 7, 'category_id': 5, 'bbox': [3.0, 4.0, 50.0, 60.0], 'area': 3000.0,
                 'iscrowd': 0})
    gt = {'images': [{'id': i} for i in ids + [99]], 'categories': [{'id': c} for c in cats], 'annotations': anns}
    got = ce.eval_coco(m, raws, ids, gt, **edges, **COCO_DET)
    ev = CocoEvalNp(gt, want_records).run()
    assert np.array_equal(got['stats'], ev.stats)
    assert got['stats'][1] > 0
    assert len(got['records']) == len(want_records)
