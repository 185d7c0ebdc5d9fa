"""COCO bbox evaluation -- counterpart of the reference's scripts/eval_coco.py: the per-image loop that writes COCO
result records (:117-164) and pycocotools' COCOeval (eval_by_cocotools, :65-73) with its default bbox parameters.

* detect_image_coco: the per-image loop, one C-ABI call (odet_eval_detect_topk: the front end of the PASCAL loop, then
  the script's tf.nn.top_k cap, which keeps exactly min(max_objects_per_image, n) detections).
* load_coco_gt / coco_records / write_coco_results_file: host bookkeeping (the records of :157-164).
* coco_evaluate: COCOeval.evaluate + accumulate on the GPU (odet_coco_match, odet_coco_order, odet_coco_accumulate,
  float64 throughout), summarize on the host with pycocotools' own numpy expression.
* eval_coco: the whole script from decoded images.
pycocotools is not a dependency: the semantics are restated (see include/odet.h for the rules the kernels follow).
"""
import ctypes as C
import json
import os

import numpy as np
import torch

from .. import _lib as L
from .. import ops
from .. import preprocess as P
from .raw_images import detect_raw_images

__all__ = ['IOU_THRS', 'REC_THRS', 'MAX_DETS', 'AREA_RNG', 'AREA_LBL', 'CocoGt', 'detect_image_coco', 'load_coco_gt',
           'coco_records', 'write_coco_results_file', 'coco_evaluate', 'summarize', 'format_stats', 'eval_coco']

# Params.setDetParams (the host computes these; the kernels take them as given)
IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
MAX_DETS = [1, 10, 100]
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
AREA_LBL = ['all', 'small', 'medium', 'large']

MAX_SEG_DETS = 4096              # ODET_COCO_MAX_SEG_DETS
MAX_SEG_GT = 1024                # ODET_COCO_MAX_SEG_GT
MAX_ENTRIES = 1 << 24            # ODET_COCO_MAX_ENTRIES
_KEEP = MAX_DETS[-1]


def detect_image_coco(scores, roi_txtytwth, rois, img_scale, raw_h, raw_w, num_classes=81, score_threshold=0.0,
                      iou_threshold=0.3, max_objects_per_class=100, max_objects_per_image=100, target_means=None,
                      target_stds=None, min_size=10, count_dev=None):
    """scripts/eval_coco.py:117-153 for one image (defaults: config/faster_rcnn_config.py:112-115, 137-138).
    scores [R,Ccls] softmax, roi_txtytwth [R,4*Ccls] or [R,Ccls,4], rois [R,4] in resized-image pixels (GPU tensors).
    -> (boxes float32 [n,4] x1y1x2y2 in raw-image pixels, labels int32 [n], scores float32 [n]) with
    n = min(max_objects_per_image, detections after NMS), ordered by (score desc, class asc, NMS order).
    An image where no class survives yields n = 0; the reference would raise at its tf.concat of an empty list."""
    if target_stds is None:
        target_stds = [0.1, 0.1, 0.2, 0.2]
    if target_means is None:
        target_means = [0, 0, 0, 0]
    scores = L.f32c(scores, 'scores')
    if scores.dim() != 2:
        raise ValueError('scores must be [num_rois, num_classes]')
    R, Ccls = scores.shape
    deltas = L.f32c(roi_txtytwth, 'roi_txtytwth')
    if deltas.numel() != R * Ccls * 4:
        raise ValueError('roi_txtytwth must hold [num_rois, num_classes, 4] values')
    rois = ops._boxes(rois, 'rois')
    if rois.shape[0] != R:
        raise ValueError('rois has %d rows for %d score rows' % (rois.shape[0], R))
    if num_classes > Ccls:
        raise ValueError('num_classes %d exceeds the %d score columns' % (num_classes, Ccls))
    cap = max((num_classes - 1) * int(max_objects_per_class), 1)
    dev = scores.device
    ob = torch.empty((cap, 4), dtype=torch.float32, device=dev)
    ol = torch.empty(cap, dtype=torch.int32, device=dev)
    os_ = torch.empty(cap, dtype=torch.float32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    nb = L.lib().odet_post_ops_workspace_bytes(int(num_classes), int(max_objects_per_class))
    ws = L.workspace(nb, dev)
    L.call('odet_eval_detect_topk', L.dptr(scores), L.dptr(deltas), L.dptr(rois), R, L.dptr(count_dev), Ccls,
           int(num_classes), float(img_scale), float(raw_h), float(raw_w), L.host4(target_means, 'target_means'),
           L.host4(target_stds, 'target_stds'), int(max_objects_per_class), int(max_objects_per_image),
           float(iou_threshold), float(score_threshold), float(min_size), L.dptr(ob), L.dptr(ol), L.dptr(os_),
           L.dptr(cnt), L.dptr(ws), nb, L.stream())
    m = int(cnt.item())
    return ob[:m].cpu().numpy(), ol[:m].cpu().numpy(), os_[:m].cpu().numpy()


# ------------------------------------------------------------------------------------------- host bookkeeping --
class CocoGt:
    """What COCOeval reads from an instances_*.json: image ids, category ids, and per annotation its id, image_id,
    category_id, bbox (xywh float64), area (the annotation's field) and iscrowd -- arrays in annotation-file order."""

    def __init__(self, image_ids, cat_ids, ann_id, ann_image, ann_cat, bbox, area, iscrowd):
        self.image_ids = image_ids
        self.cat_ids = cat_ids
        self.ann_id = ann_id
        self.ann_image = ann_image
        self.ann_cat = ann_cat
        self.bbox = bbox
        self.area = area
        self.iscrowd = iscrowd


def load_coco_gt(path_or_dict):
    """instances_*.json (a path or the parsed dict) -> CocoGt.  ValueError for an annotation without `area`, an
    annotation id <= 0 (pycocotools marks a match by the GT id and tests dtm == 0) and NaN values."""
    if isinstance(path_or_dict, CocoGt):
        return path_or_dict
    if isinstance(path_or_dict, (str, os.PathLike)):
        with open(path_or_dict, 'rt') as f:
            d = json.load(f)
    else:
        d = path_or_dict
    image_ids = np.array([im['id'] for im in d['images']], np.int64)
    cat_ids = np.array([c['id'] for c in d['categories']], np.int64)
    anns = d.get('annotations', [])
    for a in anns:
        if 'area' not in a:
            raise ValueError('annotation %r has no area field' % (a.get('id'),))
    n = len(anns)
    ann_id = np.array([a['id'] for a in anns], np.int64).reshape(n)
    ann_image = np.array([a['image_id'] for a in anns], np.int64).reshape(n)
    ann_cat = np.array([a['category_id'] for a in anns], np.int64).reshape(n)
    bbox = np.array([a['bbox'] for a in anns], np.float64).reshape(n, 4)
    area = np.array([a['area'] for a in anns], np.float64).reshape(n)
    iscrowd = np.array([int(a.get('iscrowd', 0)) for a in anns], np.uint8).reshape(n)
    if n and ann_id.min() <= 0:
        raise ValueError('annotation id %d: ids must be >= 1 (COCOeval takes a match to id 0 for no match)'
                         % int(ann_id.min()))
    if np.isnan(bbox).any() or np.isnan(area).any():
        raise ValueError('NaN in a ground-truth bbox or area')
    return CocoGt(image_ids, cat_ids, ann_id, ann_image, ann_cat, bbox, area, iscrowd)


def coco_records(dets_per_image, image_ids, cat_ids):
    """scripts/eval_coco.py:157-164: per image (boxes [n,4] float32 x1y1x2y2, labels [n], scores [n] float32), e.g.
    from detect_image_coco -> the list of result records.  Label j maps to the j-th category id in ascending order
    (what the script's name tables amount to; COCO's getCatIds() order).  bbox = [x1, y1, w, h] with
    w = float64(float32(x2 - x1)) + 1.0 (numpy 1.x promoted the float32 difference before the + 1)."""
    cats = np.unique(np.asarray(cat_ids, np.int64))
    image_ids = list(image_ids)
    if len(image_ids) != len(dets_per_image):
        raise ValueError('%d image ids for %d images' % (len(image_ids), len(dets_per_image)))
    out = []
    for img_id, (boxes, labels, scores) in zip(image_ids, dets_per_image):
        boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
        labels = np.asarray(labels).reshape(-1).astype(np.int64)
        scores = np.asarray(scores, np.float32).reshape(-1)
        if len(labels) and (labels.min() < 1 or labels.max() > len(cats)):
            raise ValueError('labels must lie in 1..%d (the categories of the annotation file)' % len(cats))
        w = (boxes[:, 2] - boxes[:, 0]).astype(np.float64) + 1.0
        h = (boxes[:, 3] - boxes[:, 1]).astype(np.float64) + 1.0
        x1 = boxes[:, 0].astype(np.float64)
        y1 = boxes[:, 1].astype(np.float64)
        cat = cats[labels - 1] if len(labels) else labels
        sc = scores.astype(np.float64)
        for i in range(len(labels)):
            out.append({'image_id': int(img_id), 'category_id': int(cat[i]),
                        'bbox': [float(x1[i]), float(y1[i]), float(w[i]), float(h[i])], 'score': float(sc[i])})
    return out


def write_coco_results_file(path, records):
    """the result file of :166-167 (json.dump of the record list)."""
    with open(path, 'wt') as f:
        json.dump(records, f)


def _results_arrays(results):
    if isinstance(results, (str, os.PathLike)):
        with open(results, 'rt') as f:
            results = json.load(f)
    n = len(results)
    img = np.array([r['image_id'] for r in results], np.int64).reshape(n)
    cat = np.array([r['category_id'] for r in results], np.int64).reshape(n)
    box = np.array([r['bbox'] for r in results], np.float64).reshape(n, 4)
    score = np.array([r['score'] for r in results], np.float64).reshape(n)
    if np.isnan(box).any() or np.isnan(score).any():
        raise ValueError('NaN in a result bbox or score')
    return img, cat, box, score


def _pack(gt, results, image_ids):
    """GT and results -> CSR segments ordered (category asc, image id asc); inside a segment GT keep annotation-file
    order and detections record order (stable sorts: these orders decide ties)."""
    r_img, r_cat, r_box, r_score = _results_arrays(results)
    gt_imgs = np.unique(gt.image_ids)
    bad = ~np.isin(r_img, gt_imgs)
    if bad.any():
        raise ValueError('result image_id %d is not an image of the ground truth (loadRes)' % int(r_img[bad][0]))
    if image_ids is None:
        imgs = gt_imgs
    else:
        imgs = np.unique(np.asarray(image_ids, np.int64))
        if imgs.size == 0:
            raise ValueError('image_ids is empty')
        if not np.isin(imgs, gt_imgs).all():
            raise ValueError('image_ids holds ids that are not images of the ground truth')
    cats = np.unique(gt.cat_ids)
    I, K = len(imgs), len(cats)
    if K == 0:
        raise ValueError('the ground truth has no category')

    def seg_of(img, cat):
        keep = np.isin(img, imgs) & np.isin(cat, cats)
        idx = np.nonzero(keep)[0]
        seg = np.searchsorted(cats, cat[idx]) * I + np.searchsorted(imgs, img[idx])
        o = np.argsort(seg, kind='stable')
        return idx[o], seg[o]

    g_idx, g_seg = seg_of(gt.ann_image, gt.ann_cat)
    d_idx, d_seg = seg_of(r_img, r_cat)
    segs = np.union1d(g_seg, d_seg)
    g_lo = np.searchsorted(g_seg, segs, 'left')
    g_hi = np.searchsorted(g_seg, segs, 'right')
    d_lo = np.searchsorted(d_seg, segs, 'left')
    d_hi = np.searchsorted(d_seg, segs, 'right')
    ng, nd = g_hi - g_lo, d_hi - d_lo
    kept = np.minimum(nd, _KEEP)
    i32 = lambda a: np.ascontiguousarray(a, np.int32)
    seg_cat = segs // I
    cat_seg_off = np.searchsorted(seg_cat, np.arange(K + 1), 'left')
    entry_off = np.concatenate([[0], np.cumsum(kept)])
    return dict(
        imgs=imgs, cats=cats, segs=segs, seg_cat=seg_cat, seg_img=segs % I,
        gt_off=i32(np.append(g_lo, len(g_seg))), dt_off=i32(np.append(d_lo, len(d_seg))), entry_off=i32(entry_off),
        cat_seg_off=i32(cat_seg_off), cat_entry_off=i32(entry_off[cat_seg_off]),
        gt_box=np.ascontiguousarray(gt.bbox[g_idx]), gt_area=np.ascontiguousarray(gt.area[g_idx]),
        gt_crowd=np.ascontiguousarray(gt.iscrowd[g_idx]),
        dt_box=np.ascontiguousarray(r_box[d_idx]), dt_score=np.ascontiguousarray(r_score[d_idx]),
        max_seg_dets=int(nd.max()) if len(nd) else 0, max_seg_gt=int(ng.max()) if len(ng) else 0,
        num_entries=int(entry_off[-1]))


def _host_doubles(values):
    v = [float(x) for x in np.asarray(values, np.float64).reshape(-1)]
    return (C.c_double * len(v))(*v)


def _run_gpu(pk, device, events=None):
    """The three launches on the current stream; events (optional): 4 torch.cuda.Event recorded around them."""
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise L.OdetError('coco_evaluate runs on the GPU: tf_eager_object_detection_amd has no CPU path')

    def up(a):
        t = torch.from_numpy(np.ascontiguousarray(a))
        return t.pin_memory().to(dev, non_blocking=True) if t.numel() else t.to(dev)

    S, K, E = len(pk['segs']), len(pk['cats']), pk['num_entries']
    gt_off, dt_off, e_off = up(pk['gt_off']), up(pk['dt_off']), up(pk['entry_off'])
    cat_seg_off, cat_entry_off = up(pk['cat_seg_off']), up(pk['cat_entry_off'])
    gt_box, gt_area, gt_crowd = up(pk['gt_box']), up(pk['gt_area']), up(pk['gt_crowd'])
    dt_box, dt_score = up(pk['dt_box']), up(pk['dt_score'])
    e_score = torch.empty(E, dtype=torch.float64, device=dev)
    e_matched = torch.empty(E, dtype=torch.int64, device=dev)
    e_ignored = torch.empty(E, dtype=torch.int64, device=dev)
    e_rank = torch.empty(E, dtype=torch.int32, device=dev)
    npig = torch.empty((S, 4), dtype=torch.int32, device=dev)
    order = torch.empty(E, dtype=torch.int32, device=dev)
    T, R, A, M = len(IOU_THRS), len(REC_THRS), len(AREA_RNG), len(MAX_DETS)
    precision = torch.empty((T, R, K, A, M), dtype=torch.float64, device=dev)
    scores = torch.empty((T, R, K, A, M), dtype=torch.float64, device=dev)
    recall = torch.empty((T, K, A, M), dtype=torch.float64, device=dev)
    nb = L.lib().odet_coco_eval_workspace_bytes(E)
    ws = L.workspace(nb, dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t.numel() else None
    st = L.stream()
    if events:
        events[0].record()
    L.call('odet_coco_match', S, p(gt_off), p(dt_off), p(e_off), p(gt_box), p(gt_area), p(gt_crowd), p(dt_box),
           p(dt_score), _host_doubles(IOU_THRS), _host_doubles(AREA_RNG), pk['max_seg_dets'], pk['max_seg_gt'], E,
           p(e_score), p(e_matched), p(e_ignored), p(e_rank), p(npig), st)
    if events:
        events[1].record()
    L.call('odet_coco_order', E, K, p(cat_entry_off), p(e_score), p(order), p(ws), nb, st)
    if events:
        events[2].record()
    L.call('odet_coco_accumulate', K, p(cat_seg_off), p(cat_entry_off), p(npig), p(order), p(e_score), p(e_matched),
           p(e_ignored), p(e_rank), _host_doubles(REC_THRS), (C.c_int * 3)(*MAX_DETS), p(precision), p(recall),
           p(scores), st)
    if events:
        events[3].record()
    return dict(precision=precision, recall=recall, scores=scores, dt_score=e_score, dt_matched=e_matched,
                dt_ignored=e_ignored, dt_rank=e_rank, npig=npig, order=order)


def _bits(v, E):
    """uint64 words [E] (bit a*10 + t) -> bool [E, 4, 10]"""
    u = v.view(np.uint64)
    sh = np.arange(len(AREA_RNG) * len(IOU_THRS), dtype=np.uint64)
    return ((u[:, None] >> sh[None, :]) & np.uint64(1)).astype(bool).reshape(E, len(AREA_RNG), len(IOU_THRS))


def coco_evaluate(gt, results, image_ids=None, device='cuda'):
    """COCOeval(gt, loadRes(results), 'bbox') with params.imgIds = image_ids (default: every GT image, what
    eval_coco.py's coco_dt.getImgIds() amounts to), evaluate(), accumulate(), summarize().
    gt: CocoGt, a path or the parsed dict; results: a record list or a result file.
    -> dict: precision, scores [10,101,K,4,3], recall [10,K,4,3] (numpy float64, -1 where pycocotools leaves -1),
    stats (12 values), and the per-segment match arrays: seg_cat / seg_img (indices into cat_ids / img_ids),
    entry_off [S+1], dt_score [E] (each segment's kept detections, stable score desc), dt_matched / dt_ignored
    bool [E, 4 areas, 10 thresholds], dt_rank [E], npig [S, 4].
    ValueError: a result image_id that is no GT image (loadRes), NaN; OdetError (ODET_E_LIMIT) above the kernel limits."""
    gt = load_coco_gt(gt)
    pk = _pack(gt, results, image_ids)
    out = _run_gpu(pk, device)
    host = {k: v.cpu().numpy() for k, v in out.items()}          # (the one synchronisation)
    E = pk['num_entries']
    res = dict(precision=host['precision'], recall=host['recall'], scores=host['scores'],
               img_ids=pk['imgs'], cat_ids=pk['cats'], seg_cat=pk['seg_cat'], seg_img=pk['seg_img'],
               entry_off=pk['entry_off'], dt_score=host['dt_score'], dt_matched=_bits(host['dt_matched'], E),
               dt_ignored=_bits(host['dt_ignored'], E), dt_rank=host['dt_rank'], npig=host['npig'])
    res['stats'] = summarize(res['precision'], res['recall'])
    return res


def _summarize_one(precision, recall, ap=1, iouThr=None, areaRng='all', maxDets=100):
    aind = [i for i, aRng in enumerate(AREA_LBL) if aRng == areaRng]
    mind = [i for i, mDet in enumerate(MAX_DETS) if mDet == maxDets]
    if ap == 1:
        s = precision
        if iouThr is not None:
            t = np.where(iouThr == IOU_THRS)[0]
            s = s[t]
        s = s[:, :, :, aind, mind]
    else:
        s = recall
        if iouThr is not None:
            t = np.where(iouThr == IOU_THRS)[0]
            s = s[t]
        s = s[:, :, aind, mind]
    if len(s[s > -1]) == 0:
        return -1
    return np.mean(s[s > -1])


_SUMMARY = [(1, None, 'all', 100), (1, .5, 'all', 100), (1, .75, 'all', 100), (1, None, 'small', 100),
            (1, None, 'medium', 100), (1, None, 'large', 100), (0, None, 'all', 1), (0, None, 'all', 10),
            (0, None, 'all', 100), (0, None, 'small', 100), (0, None, 'medium', 100), (0, None, 'large', 100)]


def summarize(precision, recall):
    """COCOeval.summarize's 12 stats (_summarizeDets): np.mean(s[s > -1]) per selection, -1 when nothing is left."""
    stats = np.zeros((12,))
    for i, (ap, thr, area, md) in enumerate(_SUMMARY):
        stats[i] = _summarize_one(precision, recall, ap, thr, area, md)
    return stats


def format_stats(stats):
    """the 12 lines COCOeval.summarize prints (its iStr format)."""
    iStr = ' {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}'
    lines = []
    for (ap, thr, area, md), v in zip(_SUMMARY, stats):
        title = 'Average Precision' if ap == 1 else 'Average Recall'
        typ = '(AP)' if ap == 1 else '(AR)'
        iou = '{:0.2f}:{:0.2f}'.format(IOU_THRS[0], IOU_THRS[-1]) if thr is None else '{:0.2f}'.format(thr)
        lines.append(iStr.format(title, typ, iou, area, md, v))
    return '\n'.join(lines)


def eval_coco(model, images, image_ids, gt, preprocessing_type='caffe', caffe_pixel_means=P.CAFFE_PIXEL_MEANS,
              min_edge=600, max_edge=1000, score_threshold=0.0, iou_threshold=0.3, max_objects_per_class=100,
              max_objects_per_image=100, target_means=None, target_stds=None, min_size=10, result_file=None,
              device='cuda'):
    """scripts/eval_coco.py:76-168 eval_coco from decoded RGB uint8 images: preprocess_images(..., 'coco') ->
    im_detect -> detect_image_coco -> coco_records -> (optional result file) -> coco_evaluate over every GT image (the
    script's params.imgIds = coco_dt.getImgIds(): images without results count their GT as misses).
    model: a caller object or a fast detector, as in raw_images.detect_raw_images.  min_edge / max_edge are explicit:
    the script itself passes them swapped (min_edge=1000, max_edge=600, see preprocess.py).
    -> coco_evaluate's dict plus 'records'."""
    gt = load_coco_gt(gt)
    image_ids = list(image_ids)
    dets = detect_raw_images(model, images, 'coco', preprocessing_type=preprocessing_type,
                             caffe_pixel_means=caffe_pixel_means, min_edge=min_edge, max_edge=max_edge,
                             score_threshold=score_threshold, iou_threshold=iou_threshold,
                             max_objects_per_class=max_objects_per_class, max_objects_per_image=max_objects_per_image,
                             target_means=target_means, target_stds=target_stds, min_size=min_size,
                             detect=detect_image_coco)
    records = coco_records(dets, image_ids, gt.cat_ids)
    if result_file is not None:
        write_coco_results_file(result_file, records)
    res = coco_evaluate(gt, records, device=device)
    res['records'] = records
    return res
