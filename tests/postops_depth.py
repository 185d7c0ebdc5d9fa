"""How far the per-class greedy NMS of the post-ops walks (numpy + the C oracle, no GPU): the walk k_postops (csrc/postops.hip)
takes, restated.  A class's rows above the score threshold are visited in (score desc, row asc) order; a row is decoded,
clipped and min-edge tested when it is visited, a survivor is tested against the boxes kept so far, and the walk ends with the
max_per_class-th kept box or with the last row.  The kernel fetches the rows a batch at a time, so `rows_visited` of a class
says how many batches its workgroup runs: ceil(rows_visited / batch).

Run as a script it prints, for the benchmark's slot-0 image (seed 1234), how many candidates each workload consumes."""
import os
import sys

import numpy as np

BATCH = 64      # rows per batch = PO_ROUND of csrc/postops.hip (test_postops_lazy_gpu.py holds the two together)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def walk(S, D, rois, image_shape, means, stds, max_per_class, nms_thr, score_thr, min_edge, num_classes, count=None,
         roi_div=1.0):
    """-> one dict per foreground class: score_rows (rows above the score threshold), passing (of them, past the min edge),
    kept, consumed (candidates popped when the last box was kept, min-edge rejects not counted: the figure of the issue's
    table; all of `passing` when the cap is not reached) and rows_visited (the same with the rejects counted)."""
    from oracle import c_oracle as co
    S = np.ascontiguousarray(S, np.float32)
    R, Ccls = S.shape
    D = np.ascontiguousarray(D, np.float32).reshape(R, Ccls, 4)
    rois = np.ascontiguousarray(rois, np.float32).reshape(-1, 4)
    n = R if count is None else min(int(count), R)
    out = []
    for c in range(1, num_classes):
        with np.errstate(invalid='ignore'):
            rows = np.flatnonzero(S[:n, c] > np.float32(score_thr))
        rows = rows[np.argsort(-S[rows, c].astype(np.float64), kind='stable')]      # (score desc, row asc)
        boxes = co.decode(rois[rows] / np.float32(roi_div) if roi_div != 1.0 else rois[rows], D[rows, c], means, stds)
        boxes, sel = co.clip_filter(boxes, 0, image_shape[0], image_shape[1], min_edge)
        keep = co.nms(boxes, S[rows[sel], c], max_per_class, nms_thr) if len(sel) else np.zeros(0, np.int32)
        capped = len(keep) == max_per_class and len(sel) > 0
        consumed = int(keep[-1]) + 1 if capped else len(sel)       # (the filtered list is in visiting order: index = position)
        visited = int(sel[keep[-1]]) + 1 if capped else len(rows)
        out.append(dict(score_rows=len(rows), passing=len(sel), kept=len(keep), consumed=consumed, rows_visited=visited))
    return out


def batches(w, batch):
    """batches the class workgroups run, per class"""
    return [-(-d['rows_visited'] // batch) for d in w]


def _bench_rows(score_kind, num_classes, caps, image_shape=(800, 1333), K=1000):
    from oracle import c_oracle as co
    from tf_eager_object_detection_amd.pipeline import synthetic_fpn_inputs
    host, _ = synthetic_fpn_inputs(image_shape, num_classes, K, 256, seed=1234, score_kind=score_kind, device='cpu')
    anchors = co.fpn_anchors(image_shape)
    rois, _ = co.region_proposal(host['rpn_deltas'], anchors, co.rpn_fg_fpn(host['rpn_logits']), image_shape, K, 0.7)
    _, perm, _ = co.assign_levels(rois)
    k = len(rois)
    return walk(host['cls_scores'][:k], host['cls_deltas'][:k], rois[perm], image_shape, [0, 0, 0, 0], [.1, .1, .2, .2], caps[0],
                0.3, 0.0, 16, num_classes)


def main():
    print('workload (seed 1234) | rows that pass the filters, per class | kept | candidates consumed (min / median / max)')
    for name, kind, ncls, caps, shape in (('headline: distinct RPN scores, 21 classes, caps 50 / 50', 'distinct', 21, (50, 50), (800, 1333)),
                                          ('clustered RPN scores, 21 classes, caps 50 / 50', 'clustered', 21, (50, 50), (800, 1333)),
                                          ('config-5 classes: 81 classes, cap 100', 'distinct', 81, (100, 100), (1333, 1333))):
        w = _bench_rows(kind, ncls, caps, shape)
        p, c = [d['passing'] for d in w], [d['consumed'] for d in w]
        print('%s | %d-%d | %d | %d / %d / %d' % (name, min(p), max(p), min(d['kept'] for d in w), min(c), int(np.median(c)), max(c)))


if __name__ == '__main__':
    main()
