"""Synthetic detection sets for the VOC evaluation tests (tests/test_voc_eval_host.py, tests/test_voc_eval_gpu.py) in the
list form that pascal_eval.evaluate_detections takes, and the conversion to the flat form of voc_eval_gpu."""
import numpy as np


def random_set(seed, n_img, num_classes=21, gt_per_img=4.0, extra_dets=12, hard_frac=0.15, no_gt_class=None,
               no_det_class=None, decimals=2):
    """-> (all_dets [n_img][num_classes] of float32 [n,5], gt_boxes [n_img] float32 [g,4], gt_labels [n_img] int32 [g],
    gt_difficult [n_img] bool [g]).  Every 7th image has no ground truth, every 5th no detections; detections are
    jittered copies of ground truth (some twice: a second match of a taken box), copies with another label, and
    random boxes; scores rounded so that equal scores occur inside images and across them."""
    rng = np.random.default_rng(seed)
    fg = [c for c in range(1, num_classes)]
    gt_cls = [c for c in fg if c != no_gt_class]
    det_cls = [c for c in fg if c != no_det_class]
    all_dets, gt_boxes, gt_labels, gt_difficult = [], [], [], []
    for i in range(n_img):
        g = 0 if i % 7 == 3 else int(rng.poisson(gt_per_img))
        x1, y1 = rng.uniform(0, 400, g), rng.uniform(0, 300, g)
        w, h = rng.uniform(8, 200, g), rng.uniform(8, 200, g)
        gb = np.round(np.stack([x1, y1, x1 + w, y1 + h], 1), 1).astype(np.float32).reshape(-1, 4)
        gl = rng.choice(gt_cls, g).astype(np.int32)
        gd = rng.uniform(size=g) < hard_frac
        rows = []
        if i % 5 != 2:
            for b, l in zip(gb, gl):
                for _ in range(int(rng.choice([0, 1, 1, 2]))):
                    jit = rng.normal(0, 0.12, 4) * np.array([b[2] - b[0], b[3] - b[1]] * 2)
                    lab = int(l) if rng.uniform() < 0.9 else int(rng.choice(fg))
                    rows.append((lab, *(b + jit), rng.uniform(0.3, 1.0)))
            for _ in range(int(rng.integers(0, extra_dets + 1))):
                x, y = rng.uniform(0, 400), rng.uniform(0, 300)
                rows.append((int(rng.choice(fg)), x, y, x + rng.uniform(8, 200), y + rng.uniform(8, 200),
                             rng.uniform(0.05, 0.8)))
        rows = [r for r in rows if r[0] in det_cls]
        per = [np.zeros((0, 5), np.float32) for _ in range(num_classes)]
        if rows:
            arr = np.array(rows, np.float64)
            arr[:, 5] = np.round(arr[:, 5], decimals)
            for c in np.unique(arr[:, 0]).astype(int):
                per[c] = arr[arr[:, 0] == c][:, 1:].astype(np.float32)
        all_dets.append(per)
        gt_boxes.append(gb)
        gt_labels.append(gl)
        gt_difficult.append(gd)
    return all_dets, gt_boxes, gt_labels, gt_difficult


def to_flat(all_dets, gt_boxes, gt_labels, gt_difficult, num_classes):
    """the list form -> ((image_index, label, boxes, scores), gt_image_index, gt_boxes, gt_labels, gt_difficult) with
    the rows in a different (class-major) order than the list form's image-major walk"""
    di, dl, db, ds = [], [], [], []
    for j in range(1, num_classes):
        for i, d in enumerate(all_dets):
            a = np.asarray(d[j]).reshape(-1, 5)
            di.append(np.full(len(a), i, np.int64))
            dl.append(np.full(len(a), j, np.int64))
            db.append(a[:, :4])
            ds.append(a[:, 4])
    gi = np.concatenate([np.full(len(l), i, np.int64) for i, l in enumerate(gt_labels)])
    return ((np.concatenate(di), np.concatenate(dl), np.concatenate(db), np.concatenate(ds)), gi,
            np.concatenate([np.asarray(b).reshape(-1, 4) for b in gt_boxes]), np.concatenate(gt_labels),
            np.concatenate(gt_difficult))


def host_eval(pe, all_dets, gt_boxes, gt_labels, gt_difficult, num_classes, ovthresh, use_07_metric=True):
    """pascal_eval.voc_eval_arrays per class, as evaluate_detections selects its arguments -> per class (rec, prec, ap,
    npos)"""
    out = []
    n = len(all_dets)
    for j in range(1, num_classes):
        dets = [all_dets[i][j] for i in range(n)]
        gb = [np.asarray(gt_boxes[i], np.float64).reshape(-1, 4)[np.asarray(gt_labels[i]).reshape(-1) == j]
              for i in range(n)]
        gd = [np.asarray(gt_difficult[i], bool).reshape(-1)[np.asarray(gt_labels[i]).reshape(-1) == j]
              for i in range(n)]
        with np.errstate(invalid='ignore', divide='ignore'):
            rec, prec, ap = pe.voc_eval_arrays(dets, gb, gd, ovthresh, use_07_metric)
        out.append((rec, prec, ap, int(sum(int(np.sum(~d)) for d in gd))))
    return out
