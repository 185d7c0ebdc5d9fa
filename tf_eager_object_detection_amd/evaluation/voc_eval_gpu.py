"""PASCAL VOC evaluation and the accuracy gate's paired bootstrap on the GPU -- the counterpart of pascal_eval's
voc_eval_arrays / evaluate_detections (evaluation/detectron_pascal_evaluation_utils.py:54-222 as
scripts/eval_pascal.py:74-96 runs it) and of precision_gate.paired_map_delta, which stay the host statements these are
checked against.

* voc_evaluate: every class at once -- odet_voc_match (the walk over the detections, one wave per (class, image)),
  odet_coco_order (the stable score order of every class), odet_voc_accumulate (rec, prec, both APs); float64 and the
  reference's operation order throughout, so rec / prec / both APs equal the host's bit for bit (the area AP's np.sum
  is restated with numpy's own order of additions).
* evaluate_detections_gpu: evaluate_detections' signature and meaning.
* paired_map_delta_gpu: paired_map_delta's signature and result; both detection sets are packed as 2 x (classes) against
  the same annotations, odet_voc_bootstrap computes every (resample, class, set) AP in one launch from the counts the
  host draws with the same generator, the means over classes and the percentiles stay numpy.
The host packs with vectorised numpy; there is one host->device copy per array, one device->host copy per result and no
CPU path: without a GPU these functions raise.
"""
import ctypes as C

import numpy as np
import torch

from .. import _lib as L

__all__ = ['REC_THRS_07', 'MAX_SEG_DETS', 'MAX_SEG_GT', 'MAX_ENTRIES', 'voc_evaluate', 'evaluate_detections_gpu',
           'paired_map_delta_gpu']

REC_THRS_07 = np.arange(0., 1.1, 0.1)      # voc_ap's thresholds (:61), computed here and handed to the kernels
MAX_SEG_DETS = 4096                        # ODET_VOC_MAX_SEG_DETS
MAX_SEG_GT = 1024                          # ODET_VOC_MAX_SEG_GT
MAX_ENTRIES = 1 << 24                      # ODET_VOC_MAX_ENTRIES
FLAG_IGNORED, FLAG_TP, FLAG_FP = 0, 1, 2   # ODET_VOC_IGNORED / _TP / _FP
AP_07, AP_AREA = 0, 1                      # ODET_VOC_AP_07 / _AREA


# ------------------------------------------------------------------------------------------------------ packing --
def _concat(rows, width):
    """list of [n, width] arrays (empty ones of any shape) -> one float64 [N, width] array and the row counts"""
    if not rows:
        return np.zeros((0, width), np.float64) if width else np.zeros(0, np.float64), np.zeros(0, np.int64)
    shape = (-1, width) if width else (-1,)
    try:
        flat = np.concatenate(rows)
        if flat.ndim != len(shape) or (width and flat.shape[1] != width):
            raise ValueError
        lens = np.fromiter(map(len, rows), np.int64, len(rows))
    except (ValueError, TypeError):
        rows = [np.asarray(r).reshape(shape) for r in rows]
        flat = np.concatenate(rows)
        lens = np.fromiter(map(len, rows), np.int64, len(rows))
    return flat, lens


def _is_flat(all_dets):
    return isinstance(all_dets, tuple) and len(all_dets) == 4 and all(isinstance(a, np.ndarray) for a in all_dets)


def _flat_dets(all_dets, num_classes):
    """all_dets[i][j] = [n, 5] (detect_image's output) or the tuple (image_index [N], label [N], boxes [N,4], scores
    [N]) -> (image int64 [N], label int64 [N], boxes float64 [N,4], scores float64 [N], images or None).  float32
    values are widened, as voc_eval_arrays' np.asarray(..., float64) does."""
    if _is_flat(all_dets):
        img, lab, box, score = all_dets
        img = np.asarray(img).reshape(-1).astype(np.int64)
        lab = np.asarray(lab).reshape(-1).astype(np.int64)
        box = np.asarray(box, np.float64).reshape(-1, 4)
        score = np.asarray(score, np.float64).reshape(-1)
        if not (len(img) == len(lab) == len(box) == len(score)):
            raise ValueError('image_index, label, boxes and scores differ in length')
        if len(lab) and (lab.min() < 1 or lab.max() >= num_classes):
            raise ValueError('detection labels must lie in 1..%d' % (num_classes - 1))
        return img, lab, box, score, None
    n, K = len(all_dets), num_classes - 1
    rows = [d[j] for d in all_dets for j in range(1, num_classes)]
    flat, lens = _concat(rows, 5)
    flat = flat.astype(np.float64, copy=False)
    img = np.repeat(np.repeat(np.arange(n, dtype=np.int64), K), lens)
    lab = np.repeat(np.tile(np.arange(1, num_classes, dtype=np.int64), n), lens)
    return img, lab, np.ascontiguousarray(flat[:, :4]), np.ascontiguousarray(flat[:, 4]), n


def _flat_gt(gt_boxes, gt_labels, gt_difficult, gt_image_index):
    """per-image lists (gt_boxes[i] [g,4], gt_labels[i] [g], gt_difficult[i] bool [g] or None) or, with gt_image_index,
    flat arrays -> (image int64 [G], label int64 [G], boxes float64 [G,4], difficult uint8 [G], images or None)"""
    if gt_image_index is not None:
        img = np.asarray(gt_image_index).reshape(-1).astype(np.int64)
        box = np.asarray(gt_boxes, np.float64).reshape(-1, 4)
        lab = np.asarray(gt_labels).reshape(-1).astype(np.int64)
        hard = (np.zeros(len(lab), np.uint8) if gt_difficult is None
                else np.asarray(gt_difficult).reshape(-1).astype(bool).astype(np.uint8))
        n = None
    else:
        n = len(gt_boxes)
        if len(gt_labels) != n:
            raise ValueError('%d label arrays for %d box arrays' % (len(gt_labels), n))
        box, lens = _concat(list(gt_boxes), 4)
        box = box.astype(np.float64, copy=False)
        lab, llens = _concat(list(gt_labels), 0)
        lab = lab.astype(np.int64)
        if not np.array_equal(lens, llens):
            raise ValueError('ground-truth boxes and labels differ in length')
        if gt_difficult is None:
            hard = np.zeros(len(lab), np.uint8)
        else:
            hard, hlens = _concat(list(gt_difficult), 0)
            if not np.array_equal(lens, hlens):
                raise ValueError('ground-truth boxes and difficult flags differ in length')
            hard = hard.astype(bool).astype(np.uint8)
        img = np.repeat(np.arange(n, dtype=np.int64), lens)
    if not (len(img) == len(lab) == len(box) == len(hard)):
        raise ValueError('ground-truth arrays differ in length')
    return img, lab, box, hard, n


def _pack(d_img, d_cls, d_box, d_score, g_img, g_cls, g_box, g_hard, num_images, num_classes):
    """Detections and ground truth (class indices 0..num_classes-1, image indices 0..num_images-1) -> CSR segments =
    (class, image) pairs that hold either, ordered (class asc, image asc); inside a segment ground truth keeps
    annotation order and detections the order of the input arrays (stable sorts: these orders decide ties).
    ValueError for non-finite values and for a segment above a limit -- before anything is copied or launched."""
    I, K = int(num_images), int(num_classes)
    if I < 1 or K < 1:
        raise ValueError('need at least one image and one class')
    if not (np.isfinite(d_box).all() and np.isfinite(d_score).all()):
        raise ValueError('non-finite value in a detection box or score')
    if not np.isfinite(g_box).all():
        raise ValueError('non-finite value in a ground-truth box')
    for name, img in (('detection', d_img), ('ground-truth', g_img)):
        if len(img) and (img.min() < 0 or img.max() >= I):
            raise ValueError('%s image index outside 0..%d' % (name, I - 1))
    if len(d_score) > MAX_ENTRIES:
        raise ValueError('%d detections exceed MAX_ENTRIES = %d' % (len(d_score), MAX_ENTRIES))

    def seg_of(cls, img):
        seg = cls * I + img
        o = np.argsort(seg, kind='stable')
        return o, seg[o]

    g_idx, g_seg = seg_of(g_cls, g_img)
    d_idx, d_seg = seg_of(d_cls, d_img)
    segs = np.union1d(g_seg, d_seg)
    g_lo = np.searchsorted(g_seg, segs, 'left')
    d_lo = np.searchsorted(d_seg, segs, 'left')
    gt_off = np.append(g_lo, len(g_seg))
    dt_off = np.append(d_lo, len(d_seg))
    ng, nd = np.diff(gt_off), np.diff(dt_off)
    max_d, max_g = (int(nd.max()), int(ng.max())) if len(segs) else (0, 0)
    if max_d > MAX_SEG_DETS:
        raise ValueError('%d detections of one class in one image exceed MAX_SEG_DETS = %d' % (max_d, MAX_SEG_DETS))
    if max_g > MAX_SEG_GT:
        raise ValueError('%d ground-truth boxes of one class in one image exceed MAX_SEG_GT = %d' % (max_g, MAX_SEG_GT))
    seg_cls, seg_img = segs // I, segs % I
    cls_seg_off = np.searchsorted(seg_cls, np.arange(K + 1), 'left')
    i32 = lambda a: np.ascontiguousarray(a, np.int32)
    return dict(
        num_images=I, num_classes=K, num_segments=len(segs), num_entries=len(d_seg), num_gt=len(g_seg),
        seg_cls=i32(seg_cls), seg_img=i32(seg_img), gt_off=i32(gt_off), dt_off=i32(dt_off),
        cls_seg_off=i32(cls_seg_off), cls_entry_off=i32(dt_off[cls_seg_off]),
        gt_box=np.ascontiguousarray(g_box[g_idx], np.float64), gt_hard=np.ascontiguousarray(g_hard[g_idx], np.uint8),
        dt_box=np.ascontiguousarray(d_box[d_idx], np.float64), dt_score=np.ascontiguousarray(d_score[d_idx], np.float64),
        entry_image=i32(np.repeat(seg_img, nd)), dt_index=d_idx, gt_index=g_idx, max_seg_dets=max_d, max_seg_gt=max_g)


def _pack_eval(all_dets, gt_boxes, gt_labels, gt_difficult, num_classes, gt_image_index=None, num_images=None):
    """voc_evaluate's arguments -> _pack's dict (class index = label - 1; ground truth of other labels is left out, as
    evaluate_detections' `lab == j` selection leaves it out)."""
    if num_classes < 2:
        raise ValueError('num_classes counts the background: at least 2')
    d_img, d_lab, d_box, d_score, nd = _flat_dets(all_dets, num_classes)
    g_img, g_lab, g_box, g_hard, ng = _flat_gt(gt_boxes, gt_labels, gt_difficult, gt_image_index)
    known = [n for n in (nd, ng, num_images) if n is not None]
    if not known:
        raise ValueError('flat detections and flat ground truth need num_images')
    if len(set(known)) != 1:
        raise ValueError('the number of images differs between the arguments: %r' % (known,))
    keep = (g_lab >= 1) & (g_lab < num_classes)
    return _pack(d_img, d_lab - 1, d_box, d_score, g_img[keep], g_lab[keep] - 1, g_box[keep], g_hard[keep], known[0],
                 num_classes - 1)


# ------------------------------------------------------------------------------------------------------ the GPU --
def _host_doubles(values):
    v = [float(x) for x in np.asarray(values, np.float64).reshape(-1)]
    return (C.c_double * len(v))(*v)


def _run_gpu(pk, device, ovthresh=0.5, counts=None, metric=AP_07, events=None):
    """The launches on the current stream: match, order, accumulate and, with counts (int32 [B, num_images]), the
    bootstrap.  events (optional): 6 torch.cuda.Event recorded before the copies in and around every launch."""
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise L.OdetError('voc_evaluate runs on the GPU: tf_eager_object_detection_amd has no CPU path')

    def up(a):
        t = torch.from_numpy(np.ascontiguousarray(a))
        return t.pin_memory().to(dev, non_blocking=True) if t.numel() else t.to(dev)

    S, K, E, I = pk['num_segments'], pk['num_classes'], pk['num_entries'], pk['num_images']
    if events:
        events[0].record()
    gt_off, dt_off = up(pk['gt_off']), up(pk['dt_off'])
    cls_seg_off, cls_entry_off = up(pk['cls_seg_off']), up(pk['cls_entry_off'])
    seg_img, entry_image = up(pk['seg_img']), up(pk['entry_image'])
    gt_box, gt_hard, dt_box, dt_score = up(pk['gt_box']), up(pk['gt_hard']), up(pk['dt_box']), up(pk['dt_score'])
    counts_d = None if counts is None else up(np.ascontiguousarray(counts, np.int32))
    e_score = torch.empty(E, dtype=torch.float64, device=dev)
    e_flag = torch.empty(E, dtype=torch.uint8, device=dev)
    seg_npos = torch.empty(S, dtype=torch.int32, device=dev)
    order = torch.empty(E, dtype=torch.int32, device=dev)
    rec = torch.empty(E, dtype=torch.float64, device=dev)
    prec = torch.empty(E, dtype=torch.float64, device=dev)
    ap07 = torch.empty(K, dtype=torch.float64, device=dev)
    ap_area = torch.empty(K, dtype=torch.float64, device=dev)
    npos = torch.empty(K, dtype=torch.int64, device=dev)
    s_flag = torch.empty(E, dtype=torch.uint8, device=dev)
    s_img = torch.empty(E, dtype=torch.int32, device=dev)
    nb = L.lib().odet_coco_eval_workspace_bytes(E)
    ws = L.workspace(nb, dev)
    nb_acc = L.lib().odet_voc_eval_workspace_bytes(E, K, 1, AP_AREA)
    ws_acc = L.workspace(nb_acc, dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t.numel() else None
    thr = _host_doubles(REC_THRS_07)
    st = L.stream()
    if events:
        events[1].record()
    L.call('odet_voc_match', S, p(gt_off), p(dt_off), p(gt_box), p(gt_hard), p(dt_box), p(dt_score), float(ovthresh),
           pk['max_seg_dets'], pk['max_seg_gt'], pk['num_gt'], E, p(e_score), p(e_flag), p(seg_npos), st)
    if events:
        events[2].record()
    # np.argsort(-confidence, kind='stable') of every class: entries are class-major, image-ascending and sorted inside
    # their segment, so (class asc, score desc, entry index asc) is that order
    L.call('odet_coco_order', E, K, p(cls_entry_off), p(e_score), p(order), p(ws), nb, st)
    if events:
        events[3].record()
    L.call('odet_voc_accumulate', K, S, E, p(cls_seg_off), p(cls_entry_off), p(seg_npos), p(order), p(e_flag),
           p(entry_image), thr, p(rec), p(prec), p(ap07), p(ap_area), p(npos), p(s_flag), p(s_img), p(ws_acc), nb_acc, st)
    if events:
        events[4].record()
    out = dict(rec=rec, prec=prec, ap07=ap07, ap_area=ap_area, npos=npos, flag=s_flag, order=order)
    if counts_d is not None:
        B = int(counts_d.shape[0])
        if counts_d.dim() != 2 or int(counts_d.shape[1]) != I:
            raise ValueError('counts must be [resamples, %d]' % I)
        boot_ap = torch.empty((B, K), dtype=torch.float64, device=dev)
        boot_npos = torch.empty((B, K), dtype=torch.int64, device=dev)
        nb_boot = L.lib().odet_voc_eval_workspace_bytes(E, K, B, int(metric))
        ws_boot = L.workspace(nb_boot, dev)
        L.call('odet_voc_bootstrap', B, K, I, S, E, p(cls_seg_off), p(cls_entry_off), p(seg_img), p(seg_npos),
               p(s_flag), p(s_img), p(counts_d), thr, int(metric), p(boot_ap), p(boot_npos), p(ws_boot), nb_boot, st)
        out.update(boot_ap=boot_ap, boot_npos=boot_npos)
    if events:
        events[5].record()
    return out


def voc_evaluate(all_dets, gt_boxes, gt_labels, gt_difficult=None, num_classes=21, ovthresh=0.5, device='cuda',
                 gt_image_index=None, num_images=None):
    """voc_eval (:86-222) of every class 1..num_classes-1 at once.
    all_dets: all_dets[i][j] = [n, 5] (x1, y1, x2, y2, score) of image i and class j (detect_image's output; what
    evaluate_detections takes) or the tuple of flat numpy arrays (image_index [N], label [N], boxes [N,4], scores [N]).
    gt_boxes / gt_labels / gt_difficult: per-image lists ([g,4], [g], bool [g]) or, with gt_image_index [G], flat arrays
    ([G,4], [G], [G]); num_images is needed when both are flat.
    -> dict: rec, prec (lists, index = class - 1, float64 arrays in descending-score order), ap07, ap_area float64
    [num_classes-1], npos int64 [num_classes-1], flag (list of uint8 arrays: 1 true positive, 2 false positive, 0 matched
    a `difficult` box).  ValueError: non-finite values, a (class, image) above MAX_SEG_DETS / MAX_SEG_GT."""
    pk = _pack_eval(all_dets, gt_boxes, gt_labels, gt_difficult, num_classes, gt_image_index, num_images)
    out = _run_gpu(pk, device, ovthresh)
    host = {k: out[k].cpu().numpy() for k in ('rec', 'prec', 'ap07', 'ap_area', 'npos', 'flag')}    # (the one sync)
    off = pk['cls_entry_off']
    cut = lambda a: [a[off[k]:off[k + 1]] for k in range(pk['num_classes'])]
    return dict(rec=cut(host['rec']), prec=cut(host['prec']), flag=cut(host['flag']), ap07=host['ap07'],
                ap_area=host['ap_area'], npos=host['npos'])


def evaluate_detections_gpu(all_dets, gt_boxes, gt_labels, gt_difficult=None, num_classes=21, ovthresh=0.5,
                            use_07_metric=True, device='cuda'):
    """pascal_eval.evaluate_detections on the GPU: mAP over classes 1..num_classes-1 (scripts/eval_pascal.py:74-96).
    -> (mAP, aps)."""
    res = voc_evaluate(all_dets, gt_boxes, gt_labels, gt_difficult, num_classes, ovthresh, device)
    aps = [float(v) for v in (res['ap07'] if use_07_metric else res['ap_area'])]
    return float(np.mean(aps)), aps


def _pack_pair(dets_a, dets_b, gt_boxes, gt_labels, num_classes):
    """both detection sets against the same annotations as ONE packing: class index k of set a, (num_classes-1) + k of
    set b, the ground truth once per set"""
    K = num_classes - 1
    a_img, a_lab, a_box, a_score, na = _flat_dets(dets_a, num_classes)
    b_img, b_lab, b_box, b_score, nb = _flat_dets(dets_b, num_classes)
    g_img, g_lab, g_box, g_hard, ng = _flat_gt(gt_boxes, gt_labels, None, None)
    if not (na == nb == ng):
        raise ValueError('the number of images differs between the arguments: %r' % ([na, nb, ng],))
    keep = (g_lab >= 1) & (g_lab < num_classes)
    g_img, g_lab, g_box, g_hard = g_img[keep], g_lab[keep], g_box[keep], g_hard[keep]
    cat = np.concatenate
    return _pack(cat([a_img, b_img]), cat([a_lab - 1, b_lab - 1 + K]), cat([a_box, b_box]), cat([a_score, b_score]),
                 cat([g_img, g_img]), cat([g_lab - 1, g_lab - 1 + K]), cat([g_box, g_box]), cat([g_hard, g_hard]),
                 ng, 2 * K)


def _draw_counts(n, resamples, seed):
    """row 0: every image once (the full set); row 1 + r: resample r of paired_map_delta's generator stream"""
    counts = np.ones((resamples + 1, n), np.int32)
    rng = np.random.default_rng(seed)
    for r in range(resamples):
        counts[1 + r] = np.bincount(rng.integers(0, n, n), minlength=n)
    return counts


def _maps_from_boot(ap, npos, K):
    """[B, 2K] per-class APs -> per row the two mAPs over the classes that have ground truth in that resample
    (_map_weighted's `if npos == 0: continue`), numpy's mean as the host takes it"""
    out = np.zeros((ap.shape[0], 2), np.float64)
    for b in range(ap.shape[0]):
        for s in range(2):
            sel = npos[b, s * K:(s + 1) * K] != 0
            v = ap[b, s * K:(s + 1) * K][sel]
            out[b, s] = float(np.mean(v)) if len(v) else 0.0
    return out


def _paired_boot(dets_a, dets_b, gt_boxes, gt_labels, num_classes, resamples, seed, use_07_metric, device):
    """-> (ap float64 [1 + resamples, 2 * (num_classes-1)], npos int64 of the same shape, counts): row 0 the full set,
    columns: the classes of set a, then of set b"""
    pk = _pack_pair(dets_a, dets_b, gt_boxes, gt_labels, num_classes)
    counts = _draw_counts(pk['num_images'], int(resamples), seed)
    out = _run_gpu(pk, device, 0.5, counts, AP_07 if use_07_metric else AP_AREA)
    return out['boot_ap'].cpu().numpy(), out['boot_npos'].cpu().numpy(), counts


def paired_map_delta_gpu(dets_a, dets_b, gt_boxes, gt_labels, num_classes=21, resamples=400, seed=0,
                         use_07_metric=True, device='cuda'):
    """precision_gate.paired_map_delta on the GPU: mAP of two detection sets against the same annotations, their
    difference, and the paired bootstrap over images of that difference (same seed -> same resamples)."""
    ap, npos, _ = _paired_boot(dets_a, dets_b, gt_boxes, gt_labels, num_classes, resamples, seed, use_07_metric, device)
    maps = _maps_from_boot(ap, npos, num_classes - 1)
    a, b = float(maps[0, 0]), float(maps[0, 1])
    ds = maps[1:, 1] - maps[1:, 0] if resamples else np.zeros(1)
    return dict(map_a=a, map_b=b, delta=b - a, delta_boot_mean=float(ds.mean()), delta_boot_std=float(ds.std()),
                delta_ci95=[float(np.percentile(ds, 2.5)), float(np.percentile(ds, 97.5))], resamples=resamples)
