"""COCO bbox evaluation on the host: hand-computed answers for the restatement (tests/coco_eval_np.py) and the package's
host code (records, packing, summarize, loading)."""
import json

import numpy as np
import pytest

from coco_eval_np import CocoEvalNp, IOU_THRS
from tf_eager_object_detection_amd.evaluation import coco_eval as ce

PR0 = 1.0 / (1.0 + np.spacing(1))


def _gt(images, anns, cats=(1,)):
    out = {'images': [{'id': i} for i in images], 'categories': [{'id': c} for c in cats], 'annotations': []}
    for k, a in enumerate(anns):
        img, cat, box = a[:3]
        rec = {'id': k + 1, 'image_id': img, 'category_id': cat, 'bbox': list(map(float, box)),
               'area': float(a[3]) if len(a) > 3 else float(box[2] * box[3]), 'iscrowd': int(a[4]) if len(a) > 4 else 0}
        out['annotations'].append(rec)
    return out


def _res(*rows):
    return [{'image_id': r[0], 'category_id': r[1], 'bbox': list(map(float, r[2])), 'score': float(r[3])} for r in rows]


def _matches(ev, k=0, i=0):
    for kk, ii, sc, m, ig, npig in ev.segment_matches():
        if kk == k and ii == i:
            return sc, m, ig, npig
    raise AssertionError('no segment')


def test_interpolation_known_answer():
    gt = _gt([1], [(1, 1, [0, 0, 100, 100]), (1, 1, [200, 200, 100, 100])])
    res = _res((1, 1, [0, 0, 100, 100], .9), (1, 1, [500, 500, 50, 50], .8), (1, 1, [200, 200, 100, 100], .7))
    ev = CocoEvalNp(gt, res).run()
    assert PR0 == 0.9999999999999998
    want = np.array([PR0] * 51 + [2.0 / 3.0] * 50)
    for t in range(10):
        np.testing.assert_array_equal(ev.eval['precision'][t, :, 0, 0, 2], want)
        assert ev.eval['recall'][t, 0, 0, 2] == 1.0
    assert ev.stats[0] == np.mean(np.tile(want, 10))
    assert abs(ev.stats[0] - 253.0 / 303.0) < 1e-15
    assert ev.stats[3] == -1 and ev.stats[4] == -1          # small / medium: every GT ignored, npig == 0
    np.testing.assert_array_equal(ce.summarize(ev.eval['precision'], ev.eval['recall']), ev.stats)


def test_iou_exactly_on_threshold():
    gt = _gt([1, 2, 3], [(i, 1, [0, 0, 10, 10]) for i in (1, 2, 3)])
    res = _res((1, 1, [0, 0, 10, 5], .5), (2, 1, [0, 0, 10, 7.5], .5), (3, 1, [0, 0, 10, 9], .5))
    ev = CocoEvalNp(gt, res).run()
    assert IOU_THRS[8] == 0.8999999999999999
    for img, last in ((0, 0), (1, int(np.nonzero(IOU_THRS <= 0.75)[0].max())), (2, 8)):
        _, m, _, _ = _matches(ev, 0, img)
        np.testing.assert_array_equal(m[0, :, 0], np.arange(10) <= last)


def test_crowd_matches_many_and_uses_detection_area():
    gt = _gt([1], [(1, 1, [0, 0, 100, 100], 10000, 1), (1, 1, [300, 300, 50, 50])])
    res = _res((1, 1, [10, 10, 20, 20], .9), (1, 1, [50, 50, 20, 20], .8))
    ev = CocoEvalNp(gt, res).run()
    _, m, ig, npig = _matches(ev)
    assert m[0].all() and ig[0].all()                    # both matched to the crowd (IoU = 400 / 400), both ignored
    assert npig[0] == 1
    assert ev.eval['recall'][0, 0, 0, 2] == 0.0          # no FP, no TP


def test_break_rule_keeps_regular_match():
    gt = _gt([1], [(1, 1, [0, 0, 10, 10]), (1, 1, [0, 0, 10, 10], 100, 1)])
    res = _res((1, 1, [0, 0, 10, 5.2], .9))
    ev = CocoEvalNp(gt, res).run()
    _, m, ig, _ = _matches(ev)
    assert m[0].all()
    np.testing.assert_array_equal(ig[0, :, 0], np.arange(10) >= 1)   # t=0: the regular GT (0.52), then break


def test_equal_iou_later_gt_wins():
    gt = _gt([1], [(1, 1, [0, 0, 10, 10]), (1, 1, [0, 0, 10, 10])])
    res = _res((1, 1, [0, 0, 10, 10], .9))
    ev = CocoEvalNp(gt, res).run()
    e = ev.evalImgs[0]
    assert (e['dtMatches'] == 2).all()


def test_area_boundaries_and_out_of_range_detections():
    gt = _gt([1], [(1, 1, [0, 0, 32, 32], 1024)])
    res = _res((1, 1, [0, 0, 32, 32], .9), (1, 1, [500, 500, 5, 10], .8))
    ev = CocoEvalNp(gt, res).run()
    _, m, ig, npig = _matches(ev)
    np.testing.assert_array_equal(npig, [1, 1, 1, 0])    # 1024 is small and medium
    assert m[:3, :, 0].all() and not ig[:3, :, 0].any()
    # the unmatched detection of area 50: an FP in all / small, ignored in medium / large
    assert not m[:, :, 1].any()
    np.testing.assert_array_equal(ig[:, 0, 1], [False, False, True, True])


def test_max_dets_truncation():
    gt = _gt([1], [(1, 1, [0, 0, 10, 10])])
    res = _res(*[(1, 1, [i, 0, 10, 10], 1.0 - i / 1000.0) for i in range(150)])
    ev = CocoEvalNp(gt, res).run()
    sc, m, _, _ = _matches(ev)
    assert len(sc) == 100 and sc[0] == 1.0
    pk = ce._pack(ce.load_coco_gt(gt), res, None)
    assert pk['num_entries'] == 100 and pk['max_seg_dets'] == 150


def test_minus_one_versus_zero():
    gt = _gt([1], [(1, 1, [0, 0, 100, 100]), (1, 1, [200, 200, 100, 100])], cats=(1, 2))
    res = _res((1, 1, [0, 0, 100, 100], .9), (1, 2, [0, 0, 10, 10], .9))
    ev = CocoEvalNp(gt, res).run()
    assert (ev.eval['precision'][:, :, 1] == -1).all() and (ev.eval['recall'][:, 1] == -1).all()
    p = ev.eval['precision'][0, :, 0, 0, 2]
    assert (p[:51] == PR0).all() and (p[51:] == 0).all()   # recall 0.5: thresholds above it stay 0


def test_score_ties_break_by_image_id():
    gt = _gt([1, 2], [(1, 1, [0, 0, 100, 100])])
    res = _res((2, 1, [0, 0, 100, 100], .5), (1, 1, [0, 0, 100, 100], .5))   # the FP's record first
    ev = CocoEvalNp(gt, res).run()
    assert (ev.eval['precision'][:, :, 0, 0, 2] == PR0).all()


def test_plus_one_width_is_float64():
    boxes = np.array([[0.0, 0.0, 0.1, 0.1]], np.float32)
    rec = ce.coco_records([(boxes, np.array([1]), np.array([.5], np.float32))], [7], [3])
    w = rec[0]['bbox'][2]
    assert w == float(np.float64(np.float32(0.1))) + 1.0
    assert w != float(np.float32(np.float32(0.1) + np.float32(1)))
    assert rec[0]['category_id'] == 3 and rec[0]['image_id'] == 7 and rec[0]['score'] == float(np.float32(.5))


def test_label_mapping_and_round_trip(tmp_path):
    gt = _gt([4], [], cats=(7, 1, 3))
    boxes = np.array([[1.5, 2.25, 30.125, 40.0]] * 3, np.float32)
    rec = ce.coco_records([(boxes, np.array([1, 2, 3]), np.array([.9, .8, .7], np.float32))], [4],
                          ce.load_coco_gt(gt).cat_ids)
    assert [r['category_id'] for r in rec] == [1, 3, 7]
    p = tmp_path / 'res.json'
    ce.write_coco_results_file(str(p), rec)
    assert json.load(open(p)) == rec
    a = ce._results_arrays(str(p))
    np.testing.assert_array_equal(a[2][0], [1.5, 2.25, np.float64(np.float32(30.125) - np.float32(1.5)) + 1.0,
                                          np.float64(np.float32(40.0) - np.float32(2.25)) + 1.0])


def test_packing_orders():
    gt = _gt([5, 2], [(5, 3, [0, 0, 1, 1]), (2, 3, [0, 0, 2, 2]), (5, 1, [0, 0, 3, 3]), (5, 3, [0, 0, 4, 4])],
             cats=(3, 1))
    res = _res((5, 1, [0, 0, 1, 1], .1), (2, 3, [0, 0, 1, 1], .2), (5, 1, [0, 0, 2, 2], .3), (5, 7, [0, 0, 1, 1], .4))
    pk = ce._pack(ce.load_coco_gt(gt), res, None)
    np.testing.assert_array_equal(pk['cats'], [1, 3])
    np.testing.assert_array_equal(pk['imgs'], [2, 5])
    np.testing.assert_array_equal(pk['segs'], [1, 2, 3])                 # (cat 1, img 5), (cat 3, img 2), (cat 3, img 5)
    np.testing.assert_array_equal(pk['gt_off'], [0, 1, 2, 4])
    np.testing.assert_array_equal(pk['gt_box'][:, 2], [3, 2, 1, 4])       # file order inside a segment
    np.testing.assert_array_equal(pk['dt_off'], [0, 2, 3, 3])             # category 7 is not evaluated
    np.testing.assert_array_equal(pk['dt_score'], [.1, .3, .2])           # record order inside a segment
    np.testing.assert_array_equal(pk['cat_seg_off'], [0, 1, 3])
    np.testing.assert_array_equal(pk['cat_entry_off'], [0, 2, 3])


def test_bad_input_raises():
    gt = _gt([1], [(1, 1, [0, 0, 10, 10])])
    bad = json.loads(json.dumps(gt))
    bad['annotations'][0]['id'] = 0
    with pytest.raises(ValueError):
        ce.load_coco_gt(bad)
    bad = json.loads(json.dumps(gt))
    bad['annotations'][0]['area'] = float('nan')
    with pytest.raises(ValueError):
        ce.load_coco_gt(bad)
    bad = json.loads(json.dumps(gt))
    del bad['annotations'][0]['area']
    with pytest.raises(ValueError):
        ce.load_coco_gt(bad)
    with pytest.raises(ValueError):
        ce._pack(ce.load_coco_gt(gt), _res((2, 1, [0, 0, 1, 1], .5)), None)
    with pytest.raises(AssertionError):
        CocoEvalNp(gt, _res((2, 1, [0, 0, 1, 1], .5)))


def test_format_stats():
    txt = ce.format_stats(np.arange(12) / 10.0).splitlines()
    assert len(txt) == 12
    assert txt[0] == ' Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 0.000'
    assert txt[11] == ' Average Recall     (AR) @[ IoU=0.50:0.95 | area= large | maxDets=100 ] = 1.100'
