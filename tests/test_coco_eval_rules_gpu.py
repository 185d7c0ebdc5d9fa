"""COCOeval's tie and boundary rules through the odet_coco_* launches (-m gpu): the hand-built cases of
test_coco_eval_host.py run on the GPU, each with its known bits asserted on the kernel output and every array compared
with the restatement; a segment whose IoU tile does not fit in LDS (the recompute path); NaN scores past the host check."""
import numpy as np
import pytest

from coco_eval_np import CocoEvalNp, IOU_THRS
from test_coco_eval_gpu import _check_all, _check_matches, coco_like
from tf_eager_object_detection_amd.evaluation import coco_eval as ce

pytestmark = pytest.mark.gpu


def _gt(images, anns, cats=(1,)):
    out = {'images': [{'id': i} for i in images], 'categories': [{'id': c} for c in cats], 'annotations': []}
    for k, a in enumerate(anns):
        img, cat, box = a[:3]
        out['annotations'].append({'id': k + 1, 'image_id': img, 'category_id': cat, 'bbox': list(map(float, box)),
                                   'area': float(a[3]) if len(a) > 3 else float(box[2] * box[3]),
                                   'iscrowd': int(a[4]) if len(a) > 4 else 0})
    return out


def _res(*rows):
    return [{'image_id': r[0], 'category_id': r[1], 'bbox': list(map(float, r[2])), 'score': float(r[3])} for r in rows]


def _run(gt, res):
    got = ce.coco_evaluate(gt, res)
    ev = CocoEvalNp(gt, res).run()
    _check_matches(got, ev)
    _check_all(got, ev)
    return got


def test_iou_exactly_on_threshold():
    got = _run(_gt([1, 2, 3], [(i, 1, [0, 0, 10, 10]) for i in (1, 2, 3)]),
               _res((1, 1, [0, 0, 10, 5], .5), (2, 1, [0, 0, 10, 7.5], .5), (3, 1, [0, 0, 10, 9], .5)))
    assert IOU_THRS[8] == 0.8999999999999999
    last75 = int(np.nonzero(IOU_THRS <= 0.75)[0].max())
    for s, last in enumerate((0, last75, 8)):                 # IoU 0.5, 0.75, 0.9 (matches at 0.8999999999999999)
        e = got['entry_off'][s]
        np.testing.assert_array_equal(got['dt_matched'][e, 0], np.arange(10) <= last)


def test_equal_iou_later_gt_wins():
    # d1 has IoU 0.5 with both GT: the later one (G2) wins, so d2 (exactly G1) still finds G1 free at t = 0.5
    got = _run(_gt([1], [(1, 1, [0, 0, 10, 5]), (1, 1, [0, 5, 10, 5])]),
               _res((1, 1, [0, 0, 10, 10], .9), (1, 1, [0, 0, 10, 5], .8)))
    m = got['dt_matched']
    assert m[0, 0, 0] and m[1, 0, 0]
    assert not m[0, 0, 1:].any() and m[1, 0, :].all()


def test_break_into_the_ignored_tail():
    got = _run(_gt([1], [(1, 1, [0, 0, 10, 10]), (1, 1, [0, 0, 10, 10], 100, 1)]), _res((1, 1, [0, 0, 10, 5.2], .9)))
    assert got['dt_matched'][0, 0].all()
    np.testing.assert_array_equal(got['dt_ignored'][0, 0], np.arange(10) >= 1)   # t = 0.5: the regular GT, then break


def test_unmatched_detection_area_bounds_are_inclusive():
    got = _run(_gt([1], [(1, 1, [0, 0, 10, 10])]),
               _res((1, 1, [500, 500, 32, 32], .9), (1, 1, [600, 600, 96, 96], .8)))      # areas 1024 and 9216
    assert not got['dt_matched'].any()
    np.testing.assert_array_equal(got['dt_ignored'][0, :, 0], [False, False, False, True])
    np.testing.assert_array_equal(got['dt_ignored'][1, :, 0], [False, True, False, False])


def test_iou_tile_recompute_path():
    """one segment of 250 GT and 150 detections: its 100 x 250 IoU tile (200 000 B) cannot fit in the 150 KiB of LDS, so
    the match recomputes every IoU it visits; the other segments stage theirs"""
    assert 100 * 250 * 8 > 150 * 1024
    gt, res = coco_like(21, 12, 4, det_per_img=20)
    rng = np.random.default_rng(22)
    img, cat = gt['images'][0]['id'], gt['categories'][0]['id']
    boxes = []
    for k in range(250):
        b = [float(v) for v in np.round([rng.uniform(0, 600), rng.uniform(0, 500), rng.uniform(8, 120),
                                         rng.uniform(8, 120)], 2)]
        boxes.append(b)
        gt['annotations'].append({'id': 50000 + k, 'image_id': img, 'category_id': cat, 'bbox': b,
                                  'area': b[2] * b[3] * float(rng.uniform(0.6, 1.0)), 'iscrowd': int(k % 60 == 7)})
    for k in range(150):
        x, y, w, h = boxes[int(rng.integers(250))]
        j = rng.normal(0, 0.06, 4)
        res.append({'image_id': img, 'category_id': cat, 'score': float(np.round(rng.random(), 2)),
                    'bbox': [float(v) for v in np.round([x + j[0] * w, y + j[1] * h, w * (1 + j[2]), h * (1 + j[3])], 2)]})
    got = _run(gt, res)
    assert got['npig'].max() >= 200 and got['dt_matched'].any()


def test_nan_scores_rank_last_in_input_order():
    """NaN scores that reach the launches (the Python layer rejects them) rank after every number, as numpy's argsort of
    -score puts them, in every per-segment order and in the per-category sort"""
    gt, res = coco_like(31, 30, 5, det_per_img=40, big_segment=150)
    sentinel = 0.123456                                       # (coco_like's scores have two decimals)
    nan_at = [i for i in range(len(res)) if i % 5 == 0]
    for i in nan_at:
        res[i]['score'] = sentinel
    pk = ce._pack(ce.load_coco_gt(gt), res, None)
    pk['dt_score'] = np.where(pk['dt_score'] == sentinel, np.nan, pk['dt_score'])
    assert np.isnan(pk['dt_score']).sum() == len(nan_at)
    out = {k: v.cpu().numpy() for k, v in ce._run_gpu(pk, 'cuda').items()}
    E = pk['num_entries']
    got = dict(seg_cat=pk['seg_cat'], seg_img=pk['seg_img'], entry_off=pk['entry_off'], dt_score=out['dt_score'],
               dt_matched=ce._bits(out['dt_matched'], E), dt_ignored=ce._bits(out['dt_ignored'], E),
               dt_rank=out['dt_rank'], npig=out['npig'])
    assert np.isnan(got['dt_score']).any()
    for i in nan_at:
        res[i]['score'] = float('nan')
    ev = CocoEvalNp(gt, res).run()
    _check_matches(got, ev)                                    # (assert_array_equal: NaN equals NaN)
    for key in ('precision', 'recall', 'scores'):
        np.testing.assert_array_equal(out[key], ev.eval[key])
