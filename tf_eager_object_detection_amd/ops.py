"""Functional torch-tensor front-end of the C ABI (one function per odet_* entry point).

Inputs and outputs are GPU tensors; shapes that depend on data (NMS survivors, filters) come
back padded together with a device-side count.  The reference-surface modules in
``model/`` and ``utils/`` slice them to the reference's dynamic shapes (one host sync, as the
reference itself does at region_proposal.py:78 / prediction.py:147); ``pipeline.py`` keeps
everything padded and sync-free.
"""
import collections
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from .derived import invalidate
# the float32 layers' arithmetic forms, the gradient GEMMs' form, the limb splitters and the split-precision workspace
from .f32_forms import (  # noqa: F401
    _F32_CTX, current_f32_form, f32_form, _GRAD_CTX, GRAD_FORMS, current_grad_form, check_grad_form, grad_form, carries_grad_form,
    split_bf16x3, f16x2_exponent, split_f16x2, X3Workspace, _X3_WS, _x3_workspace, _F32_FORMS, _f32_sym, _f32_call)

# constants of include/odet.h
RPN_LAYOUT_FPN, RPN_LAYOUT_FRCNN = 0, 1
ROI_NORM_STRIDE, ROI_NORM_IMAGE, ROI_NORM_TP_ALIGN = 0, 1, 2
ROI_POOL_NONE, ROI_POOL_MAX2, ROI_POOL_AVG2 = 0, 1, 2
ASSIGN_MAX_ROIS = 8192
POSTOPS_MAX_ROIS = 4096
POSTOPS_MAX_CANDIDATES = 8192
MAX_LEVELS = 8

# the name DESIGN.md knows derived.invalidate by: after `.data` / set_() writes (no version bump); drops EVERY derived tensor
invalidate_planes = invalidate


def _out(out, shape, dtype, device):
    """the result tensor of a launch: a fresh one, or the caller's `out` when it is a contiguous `dtype` tensor of `shape`"""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if out.dtype != dtype or tuple(out.shape) != tuple(shape) or not out.is_contiguous():
        raise ValueError('out must be a contiguous %s tensor of shape %s, got %s %s'
                         % (dtype, tuple(shape), out.dtype, tuple(out.shape)))
    return out


def _boxes(t, name):
    t = L.f32c(t, name)
    if t.dim() != 2 or t.shape[1] != 4:
        raise ValueError('%s must have shape [N,4], got %s' % (name, tuple(t.shape)))
    return t


def anchors_shift(anchor_base, feat_stride, height, width):
    base = _boxes(anchor_base, 'anchor_base')
    fh, fw = int(height), int(width)
    out = torch.empty((fh * fw * base.shape[0], 4), dtype=torch.float32, device=base.device)
    L.check(L.lib().odet_anchors_shift(L.dptr(base), base.shape[0], int(feat_stride), fh, fw, L.dptr(out), L.stream()))
    return out


def anchors_fpn(fh_list, fw_list, stride_list, wh_table, device):
    """wh_table: float32 numpy [num_levels, A, 2] of (w, h) per level / anchor."""
    nl = len(fh_list)
    wh = np.ascontiguousarray(wh_table, dtype=np.float32)
    A = wh.shape[1]
    fh = (C.c_int * nl)(*[int(v) for v in fh_list])
    fw = (C.c_int * nl)(*[int(v) for v in fw_list])
    st = (C.c_int * nl)(*[int(v) for v in stride_list])
    total = sum(int(a) * int(b) for a, b in zip(fh_list, fw_list)) * A
    out = torch.empty((total, 4), dtype=torch.float32, device=device)
    L.check(L.lib().odet_anchors_fpn(nl, A, fh, fw, st, wh.ctypes.data_as(C.c_void_p), L.dptr(out), L.stream()))
    return out


def decode(anchors, deltas, means, stds, clip_shape=None, out=None):
    anchors = _boxes(anchors, 'anchors')
    deltas = L.f32c(deltas, 'deltas')
    n = anchors.shape[0]
    if deltas.numel() != n * 4:
        raise ValueError('deltas must hold %d x 4 values, got shape %s' % (n, tuple(deltas.shape)))
    if out is None:
        out = torch.empty((n, 4), dtype=torch.float32, device=anchors.device)
    ch, cw = (0, 0) if clip_shape is None else (int(clip_shape[0]), int(clip_shape[1]))
    L.check(L.lib().odet_decode(L.dptr(anchors), L.dptr(deltas), 4, n, L.host4(means, 'target_means'),
                                L.host4(stds, 'target_stds'), ch, cw, L.dptr(out), L.stream()))
    return out


def encode(src, dst, means, stds):
    src = _boxes(src, 'src_bbox')
    dst = _boxes(dst, 'dst_bbox')
    if src.shape != dst.shape:
        raise ValueError('src_bbox and dst_bbox shapes differ: %s vs %s' % (tuple(src.shape), tuple(dst.shape)))
    out = torch.empty_like(src)
    L.check(L.lib().odet_encode(L.dptr(src), L.dptr(dst), src.shape[0], L.host4(means, 'target_means'),
                                L.host4(stds, 'target_stds'), L.dptr(out), L.stream()))
    return out


def clip(boxes, min_value, max_height, max_width):
    boxes = _boxes(boxes, 'boxes')
    out = torch.empty_like(boxes)
    L.check(L.lib().odet_clip(L.dptr(boxes), boxes.shape[0], float(min_value), int(max_height), int(max_width),
                              L.dptr(out), L.stream()))
    return out


def _count_tensor(device):
    return torch.zeros(1, dtype=torch.int32, device=device)


def clip_filter(boxes, min_value, max_height, max_width, min_edge):
    """-> (boxes [n,4] padded, idx int64 [n] padded, count int32[1] on device)"""
    boxes = _boxes(boxes, 'boxes')
    n = boxes.shape[0]
    ob = torch.empty_like(boxes)
    oi = torch.empty(n, dtype=torch.int64, device=boxes.device)
    cnt = _count_tensor(boxes.device)
    nb = L.lib().odet_compact_workspace_bytes(n)
    ws = L.workspace(nb, boxes.device)
    L.check(L.lib().odet_clip_filter(L.dptr(boxes), n, float(min_value), int(max_height), int(max_width),
                                     float(min_edge), L.dptr(ob), L.dptr(oi), L.dptr(cnt), L.dptr(ws), nb, L.stream()))
    return ob, oi, cnt


def range_filter(boxes, max_height, max_width):
    boxes = _boxes(boxes, 'anchors')
    n = boxes.shape[0]
    oi = torch.empty(n, dtype=torch.int64, device=boxes.device)
    cnt = _count_tensor(boxes.device)
    nb = L.lib().odet_compact_workspace_bytes(n)
    ws = L.workspace(nb, boxes.device)
    L.check(L.lib().odet_range_filter(L.dptr(boxes), n, int(max_height), int(max_width), L.dptr(oi), L.dptr(cnt),
                                      L.dptr(ws), nb, L.stream()))
    return oi, cnt


def where_greater(values, threshold):
    """tf.where(values > threshold)[:, 0] for a 1-D (possibly strided) float32 GPU tensor."""
    if values.dim() != 1:
        raise ValueError('values must be 1-D')
    if values.dtype != torch.float32 or not values.is_cuda:
        values = L.f32c(values, 'values')
    n = values.shape[0]
    stride = values.stride(0) if n > 1 else 1
    if stride < 1:
        values = values.contiguous()
        stride = 1
    oi = torch.empty(n, dtype=torch.int64, device=values.device)
    cnt = _count_tensor(values.device)
    nb = L.lib().odet_compact_workspace_bytes(n)
    ws = L.workspace(nb, values.device)
    L.check(L.lib().odet_where_greater(C.c_void_p(values.data_ptr()), stride, n, float(threshold), L.dptr(oi),
                                       L.dptr(cnt), L.dptr(ws), nb, L.stream()))
    return oi, cnt


def pairwise_iou(b1, b2):
    b1 = _boxes(b1, 'boxlist1')
    b2 = _boxes(b2, 'boxlist2')
    out = torch.empty((b1.shape[0], b2.shape[0]), dtype=torch.float32, device=b1.device)
    L.check(L.lib().odet_pairwise_iou(L.dptr(b1), b1.shape[0], L.dptr(b2), b2.shape[0], L.dptr(out), L.stream()))
    return out


def gather_rows(src, idx, count_dev=None):
    src = L.f32c(src, 'src')
    row = int(np.prod(src.shape[1:])) if src.dim() > 1 else 1
    if idx.dtype not in (torch.int32, torch.int64):
        raise TypeError('idx must be int32 or int64')
    idx = idx.contiguous()
    n = idx.shape[0]
    out = torch.empty((n,) + tuple(src.shape[1:]), dtype=torch.float32, device=src.device)
    L.check(L.lib().odet_gather_rows(L.dptr(src), L.dptr(idx), 1 if idx.dtype == torch.int64 else 0, n,
                                     L.dptr(count_dev), row, L.dptr(out), L.stream()))
    return out


def rpn_fg_softmax(logits, num_anchors, layout):
    logits = L.f32c(logits, 'rpn_score')
    if layout == RPN_LAYOUT_FPN:
        if logits.numel() % 2:
            raise ValueError('FPN rpn scores must reshape to [-1, 2]')
        n = logits.numel() // 2
        out = torch.empty(n, dtype=torch.float32, device=logits.device)
        L.check(L.lib().odet_rpn_fg_softmax(L.dptr(logits), n, 1, layout, L.dptr(out), L.stream()))
    else:
        A = int(num_anchors)
        if logits.numel() % (2 * A):
            raise ValueError('rpn scores must reshape to [-1, 2*num_anchors]')
        nloc = logits.numel() // (2 * A)
        out = torch.empty(nloc * A, dtype=torch.float32, device=logits.device)
        L.check(L.lib().odet_rpn_fg_softmax(L.dptr(logits), nloc, A, layout, L.dptr(out), L.stream()))
    return out


def nms(boxes, scores, max_output_size, iou_threshold, with_boxes=False, blind_chunks=1, done=None):
    """-> (idx int32 [K] padded, count int32[1]) (+ gathered boxes [K,4]).  ``done`` (int32[1]
    GPU tensor) switches to the sync-free mode of odet_nms."""
    boxes = _boxes(boxes, 'boxes')
    scores = L.f32c(scores, 'scores').reshape(-1)
    n = boxes.shape[0]
    if scores.shape[0] != n:
        raise ValueError('scores has %d entries for %d boxes' % (scores.shape[0], n))
    K = max(min(int(max_output_size), n), 0)
    idx = torch.empty(max(K, 1), dtype=torch.int32, device=boxes.device)
    ob = torch.empty((max(K, 1), 4), dtype=torch.float32, device=boxes.device) if with_boxes else None
    cnt = _count_tensor(boxes.device)
    nb = L.lib().odet_nms_workspace_bytes(n, K)
    ws = L.workspace(nb, boxes.device)
    L.check(L.lib().odet_nms(L.dptr(boxes), L.dptr(scores), n, K, float(iou_threshold), L.dptr(idx), L.dptr(ob),
                             L.dptr(cnt), int(blind_chunks), L.dptr(done), L.dptr(ws), nb, L.stream()))
    return (idx, cnt, ob) if with_boxes else (idx, cnt)


def region_proposal(deltas, anchors, scores, image_shape, num_post_nms, iou_threshold, means, stds,
                    workspace=None, blind_chunks=1, done=None, out=None):
    """-> (rois [K,4] padded, idx int32 [K] padded, count int32[1]).  ``done`` (int32[1] GPU
    tensor) switches to the sync-free mode of odet_region_proposal."""
    anchors = _boxes(anchors, 'anchors')
    deltas = L.f32c(deltas, 'bboxes_txtytwth')
    scores = L.f32c(scores, 'scores').reshape(-1)
    n = anchors.shape[0]
    if deltas.numel() != n * 4 or scores.shape[0] != n:
        # the reference would raise InvalidArgumentError from TF on mismatched N
        raise ValueError('RegionProposal: %d anchors but deltas %s / scores %s'
                         % (n, tuple(deltas.shape), tuple(scores.shape)))
    K = max(min(int(num_post_nms), n), 0)
    if out is not None:
        rois, idx, cnt = out
    else:
        rois = torch.empty((max(K, 1), 4), dtype=torch.float32, device=anchors.device)
        idx = torch.empty(max(K, 1), dtype=torch.int32, device=anchors.device)
        cnt = _count_tensor(anchors.device)
    nb = L.lib().odet_region_proposal_workspace_bytes(n, K)
    ws = workspace if workspace is not None and workspace.numel() >= nb else L.workspace(nb, anchors.device)
    L.check(L.lib().odet_region_proposal(L.dptr(deltas), L.dptr(anchors), L.dptr(scores), n, int(image_shape[0]),
                                         int(image_shape[1]), L.host4(means, 'target_means'),
                                         L.host4(stds, 'target_stds'), K, float(iou_threshold), L.dptr(rois),
                                         L.dptr(idx), L.dptr(cnt), int(blind_chunks), L.dptr(done), L.dptr(ws),
                                         ws.numel(), L.stream()))
    return rois, idx, cnt


FUSED_ORDER_MAX_ROIS = 1024          # ODET_FUSED_ORDER_MAX_ROIS


def fpn_proposals(rpn_logits, rpn_deltas, fh_list, fw_list, stride_list, wh_table, image_shape, num_post_nms,
                  iou_threshold, means, stds, min_level=None, max_level=None, workspace=None, blind_chunks=1,
                  done=None, out=None, out_levels=None, out_order=None):
    """The whole FPN proposal stage (anchors in registers -> fg softmax -> decode+clip -> NMS over all
    anchors [-> level assignment]) as ONE C-ABI call.  -> (rois [K,4] padded, idx int32 [K], count int32[1])
    and, when min_level is given, (sorted rois [K,4], level int32 [K], perm int64 [K], counts int32 [L]).
    out_order (int32 [K], K <= FUSED_ORDER_MAX_ROIS, needs the level outputs): receives the spatial processing order
    of the level-sorted RoIs (what roi_order computes) from the same launches."""
    logits = L.f32c(rpn_logits, 'rpn_score')
    deltas = L.f32c(rpn_deltas, 'rpn_bbox_txtytwth')
    nl = len(fh_list)
    wh = np.ascontiguousarray(wh_table, dtype=np.float32)
    A = wh.shape[1]
    n = sum(int(a) * int(b) for a, b in zip(fh_list, fw_list)) * A
    if logits.numel() != n * 2 or deltas.numel() != n * 4:
        raise ValueError('fpn_proposals: %d anchors but rpn scores %s / deltas %s'
                         % (n, tuple(logits.shape), tuple(deltas.shape)))
    fh = (C.c_int * nl)(*[int(v) for v in fh_list])
    fw = (C.c_int * nl)(*[int(v) for v in fw_list])
    st = (C.c_int * nl)(*[int(v) for v in stride_list])
    K = max(min(int(num_post_nms), n), 1)
    dev = logits.device
    if out is not None:
        rois, idx, cnt = out
    else:
        rois = torch.empty((K, 4), dtype=torch.float32, device=dev)
        idx = torch.empty(K, dtype=torch.int32, device=dev)
        cnt = _count_tensor(dev)
    lv = None
    if min_level is not None:
        nlv = int(max_level) - int(min_level) + 1
        lv = out_levels if out_levels is not None else (
            torch.empty((K, 4), dtype=torch.float32, device=dev), torch.empty(K, dtype=torch.int32, device=dev),
            torch.empty(K, dtype=torch.int64, device=dev), torch.empty(nlv, dtype=torch.int32, device=dev))
    nb = L.lib().odet_fpn_proposals_workspace_bytes(n, K)
    ws = workspace if workspace is not None and workspace.numel() >= nb else L.workspace(nb, dev)
    L.call(
        'odet_fpn_proposals', L.dptr(logits), L.dptr(deltas), nl, A, fh, fw, st, wh.ctypes.data_as(C.c_void_p), int(image_shape[0]),
        int(image_shape[1]), L.host4(means, 'target_means'), L.host4(stds, 'target_stds'), K, float(iou_threshold),
        int(min_level or 0), int(max_level or 0), L.dptr(rois), L.dptr(idx), L.dptr(cnt),
        L.dptr(lv[0]) if lv else None, L.dptr(lv[1]) if lv else None, L.dptr(lv[2]) if lv else None,
        L.dptr(lv[3]) if lv else None, L.dptr(out_order, torch.int32, 'out_order') if out_order is not None else None,
        int(blind_chunks), L.dptr(done), L.dptr(ws), ws.numel(), L.stream())
    return (rois, idx, cnt) + ((lv,) if lv else ())


def frcnn_proposals(rpn_logits, rpn_deltas, anchor_base, feat_stride, fh, fw, image_shape, num_post_nms,
                    iou_threshold, means, stds, workspace=None, blind_chunks=1, done=None, out=None):
    """The proposal stage of BaseFasterRcnn.call (anchors in registers -> fg softmax of the [A bg | A fg]
    layout -> decode+clip -> NMS over all anchors) as ONE C-ABI call.
    -> (rois [K,4] padded, idx int32 [K], count int32[1])."""
    logits = L.f32c(rpn_logits, 'rpn_score')
    deltas = L.f32c(rpn_deltas, 'rpn_bbox_txtytwth')
    base = np.ascontiguousarray(np.asarray(anchor_base, dtype=np.float32).reshape(-1, 4))
    A = base.shape[0]
    fh, fw = int(fh), int(fw)
    n = fh * fw * A
    if logits.numel() != n * 2 or deltas.numel() != n * 4:
        raise ValueError('frcnn_proposals: %d anchors but rpn scores %s / deltas %s'
                         % (n, tuple(logits.shape), tuple(deltas.shape)))
    K = max(min(int(num_post_nms), n), 1)
    dev = logits.device
    if out is not None:
        rois, idx, cnt = out
    else:
        rois = torch.empty((K, 4), dtype=torch.float32, device=dev)
        idx = torch.empty(K, dtype=torch.int32, device=dev)
        cnt = _count_tensor(dev)
    nb = L.lib().odet_frcnn_proposals_workspace_bytes(n, K)
    ws = workspace if workspace is not None and workspace.numel() >= nb else L.workspace(nb, dev)
    L.call('odet_frcnn_proposals', L.dptr(logits), L.dptr(deltas), base.ctypes.data_as(C.c_void_p), A,
           int(feat_stride), fh, fw, int(image_shape[0]), int(image_shape[1]), L.host4(means, 'target_means'),
           L.host4(stds, 'target_stds'), K, float(iou_threshold), L.dptr(rois), L.dptr(idx), L.dptr(cnt),
           int(blind_chunks), L.dptr(done), L.dptr(ws), ws.numel(), L.stream())
    return rois, idx, cnt


def assign_levels(rois, min_level, max_level, count_dev=None, out=None):
    """-> (sorted rois [n,4], level int32 [n] (0-based), perm int64 [n], counts int32 [L]).
    ``out`` = preallocated (sorted rois, level, perm, counts) to reuse."""
    rois = _boxes(rois, 'all_rois')
    n = rois.shape[0]
    nl = int(max_level) - int(min_level) + 1
    if out is not None:
        out, lvl, perm, counts = out
    else:
        out = torch.empty_like(rois)
        lvl = torch.empty(max(n, 1), dtype=torch.int32, device=rois.device)
        perm = torch.empty(max(n, 1), dtype=torch.int64, device=rois.device)
        counts = torch.empty(nl, dtype=torch.int32, device=rois.device)
    L.check(L.lib().odet_assign_levels(L.dptr(rois), n, L.dptr(count_dev), int(min_level), int(max_level),
                                       L.dptr(out), L.dptr(lvl), L.dptr(perm), L.dptr(counts), L.stream()))
    return out, lvl[:n], perm[:n], counts


ASSIGN_IMAGES_MAX_BATCH = 64   # ODET_ASSIGN_MAX_BATCH (= TARGETS_MAX_BATCH: what one targets call produces)


def assign_levels_images(rois, min_level, max_level, count_dev=None, out=None):
    """assign_levels for B images in ONE launch: rois [B,n,4], count_dev int32 [B] (None: n RoIs in every image)
    -> (sorted rois [B,n,4], level int32 [B,n] (0-based), perm int64 [B,n] (rows inside the image), counts int32 [B,L]).
    Image b's rows below its count and counts[b] are assign_levels' on image b alone, bit for bit; the rows from its count on
    are not written.  ``out`` = preallocated (sorted rois, level, perm, counts) to reuse."""
    rois = L.f32c(rois, 'all_rois')
    if rois.dim() != 3 or rois.shape[2] != 4:
        raise ValueError('all_rois must have shape [B,n,4], got %s' % (tuple(rois.shape),))
    B, n = int(rois.shape[0]), int(rois.shape[1])
    nl = int(max_level) - int(min_level) + 1
    if count_dev is not None and (count_dev.dtype != torch.int32 or count_dev.numel() != B):
        raise ValueError('count_dev must be int32 [%d], got %s %s' % (B, count_dev.dtype, tuple(count_dev.shape)))
    if out is not None:
        out, lvl, perm, counts = out
        if tuple(out.shape) != (B, n, 4) or tuple(lvl.shape) != (B, n) or tuple(perm.shape) != (B, n) or \
                counts.numel() != B * max(nl, 0):
            raise ValueError('out must be (sorted rois [%d,%d,4], level [%d,%d], perm [%d,%d], counts [%d,%d])'
                             % (B, n, B, n, B, n, B, nl))
    else:
        out = torch.empty_like(rois)
        lvl = torch.empty((B, n), dtype=torch.int32, device=rois.device)
        perm = torch.empty((B, n), dtype=torch.int64, device=rois.device)
        counts = torch.empty((B, max(nl, 0)), dtype=torch.int32, device=rois.device)
    L.check(L.lib().odet_assign_levels_images(L.dptr(rois), B, n, L.dptr(count_dev, torch.int32, 'count_dev'), int(min_level),
                                              int(max_level), L.dptr(out, torch.float32, 'out'), L.dptr(lvl, torch.int32, 'level'),
                                              L.dptr(perm, torch.int64, 'perm'), L.dptr(counts, torch.int32, 'counts'),
                                              L.stream()))
    return out, lvl, perm, counts


def fpn_topdown_merge(top, lateral, out=None):
    """P_k = 0.5 * tf.image.resize_bilinear(P_{k+1}, size(lateral)) + 0.5 * lateral (reference
    model/fpn/resnet_fpn.py:385-398, TF 1.x legacy resize) in one launch.  ``top`` [B,h,w,C] and
    ``lateral`` [B,H,W,C]: NHWC GPU tensors of the same dtype (float32 or float16); contiguous NHWC memory."""
    if top.dim() != 4 or lateral.dim() != 4:
        raise ValueError('top and lateral must be [B,h,w,C] tensors')
    if top.dtype != lateral.dtype or top.dtype not in (torch.float32, torch.float16):
        raise TypeError('top and lateral must both be float32 or both float16')
    if top.shape[0] != lateral.shape[0] or top.shape[3] != lateral.shape[3]:
        raise ValueError('top %s and lateral %s must agree in batch and channels' % (tuple(top.shape), tuple(lateral.shape)))
    if not top.is_contiguous():
        top = top.contiguous()
    if not lateral.is_contiguous():
        lateral = lateral.contiguous()
    B, h, w, Cc = (int(v) for v in top.shape)
    H, W = int(lateral.shape[1]), int(lateral.shape[2])
    if out is None:
        out = torch.empty_like(lateral)
    L.call('odet_fpn_topdown_merge', L.dptr(top), h, w, L.dptr(lateral), H, W, B, Cc, L.dptr(out),
           1 if top.dtype == torch.float16 else 0, L.stream())
    return out


def _grad_f32(who, what, named):
    """the first two rules of every backward front, in this order: the named operands are float32 tensors, the current f32 form is
    'exact' (``what``: the backward the messages name)"""
    for name, t in named:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise ValueError('%s: %s must be a float32 tensor (the %s has no float16 form), got %s'
                             % (who, name, what, getattr(t, 'dtype', type(t).__name__)))
    if current_f32_form() != 'exact':
        raise ValueError("%s: the %s runs only under f32_form 'exact' (its split-precision form is ops.grad_form('x3')), not %r"
                         % (who, what, current_f32_form()))


def _grad_operands(who, what, named, ndim=None):
    """the ONE front of the backward ops' operands (``named``: (name, tensor) pairs): _grad_f32, then contiguous and of rank
    ``ndim`` where one is given.  The caller goes on with its own shape rules and ends with _grad_on_gpu: dtype, form, rank and
    contiguity, shapes, device -- the same precedence in every front."""
    _grad_f32(who, what, named)
    how = {None: 'contiguous', 2: 'a contiguous 2-D tensor', 4: 'a contiguous NHWC tensor [B,H,W,C]'}[ndim]
    for name, t in named:
        if (ndim is not None and t.dim() != ndim) or not t.is_contiguous():
            raise ValueError('%s: %s must be %s' % (who, name, how))


def _grad_on_gpu(who, named):
    for name, t in named:
        if not t.is_cuda:
            raise ValueError('%s: %s must be a GPU tensor' % (who, name))


def _grad_symbols(exact, x3):
    """the (entry point, workspace query) pair of the current grad form"""
    return x3 if current_grad_form() == 'x3' else exact


def _grad_workspace(query_symbol, query_args, device):
    """the split-K workspace of a gradient GEMM, sized by the library's own query -> (pointer or None, bytes)"""
    n = int(getattr(L.lib(), query_symbol)(*query_args))
    return (C.c_void_p(L.workspace(n, device).data_ptr()), n) if n else (None, 0)


def fpn_topdown_backward(fine, top_hw, base=None, sub=None, out_scale=1.0, out=None):
    """The backward of the top-down merge's resize with the coarse map's other gradient terms folded in
    (odet_fpn_topdown_backward_f32; resnet_fpn.py:385-398 in reverse): d_top [B,h,w,C] = out_scale * (base + sub placed at the even
    pixels + the transpose of resize_bilinear(top, (H, W)) applied to fine), added in that order, in one launch without atomics.
    ``fine`` [B,H,W,C] (the gradient with respect to the resized map, the merge's 0.5 already applied), ``base`` [B,h,w,C] and
    ``sub`` [B,ceil(h/2),ceil(w/2),C] (the gradient of top[:, ::2, ::2]) are contiguous NHWC float32 GPU tensors; each may be
    None (its term is skipped), not all three.  ``top_hw`` = (h, w).  float32, f32_form 'exact' only."""
    who = 'fpn_topdown_backward'
    named = [(n, t) for n, t in (('fine', fine), ('base', base), ('sub', sub)) if t is not None]
    if not named:
        raise ValueError('%s: at least one of fine, base and sub is needed' % who)
    _grad_operands(who, 'neck backward', named, ndim=4)
    h, w = int(top_hw[0]), int(top_hw[1])
    B, Cc = int(named[0][1].shape[0]), int(named[0][1].shape[3])
    if h < 1 or w < 1 or Cc < 4 or Cc % 4:
        raise ValueError('%s: top_hw %s must be positive and C %d a multiple of 4' % (who, (h, w), Cc))
    want = {'base': (B, h, w, Cc), 'sub': (B, (h + 1) // 2, (w + 1) // 2, Cc)}
    for name, t in named:
        if name == 'fine':
            if int(t.shape[1]) < 1 or int(t.shape[2]) < 1:
                raise ValueError('%s: fine %s must have a positive size' % (who, tuple(t.shape)))
        elif tuple(t.shape) != want[name]:
            raise ValueError('%s: %s %s does not go with top_hw %s and %s %s (expected %s)'
                             % (who, name, tuple(t.shape), (h, w), named[0][0], tuple(named[0][1].shape), want[name]))
    _grad_on_gpu(who, named)
    out = _out(out, (B, h, w, Cc), torch.float32, named[0][1].device)
    H, W = (int(fine.shape[1]), int(fine.shape[2])) if fine is not None else (h, w)
    L.call('odet_fpn_topdown_backward_f32', L.dptr(fine), H, W, L.dptr(base), L.dptr(sub), float(out_scale), L.dptr(out), h, w, B,
           Cc, L.stream())
    return out


def _positive_maps(who, named):
    """the first shape rule of stride_gather / block_input_grad: a positive map size and C a positive multiple of 4"""
    for name, t in named:
        if int(t.shape[1]) < 1 or int(t.shape[2]) < 1 or int(t.shape[3]) < 4 or int(t.shape[3]) % 4:
            raise ValueError('%s: %s %s must have a positive map size and C a positive multiple of 4' % (who, name, tuple(t.shape)))


def _stride_1_or_2(who, stride):
    if stride not in (1, 2):
        raise ValueError('%s: stride must be 1 or 2, got %r' % (who, stride))
    return int(stride)


def stride_gather(x, stride, out=None):
    """x[:, ::stride, ::stride, :] as a contiguous map (odet_stride_gather_f32): the [rows, cin] input that dense_wgrad needs for a
    strided 1x1 convolution (resnet_fpn.py:154-205: the first block of conv3..conv5).  ``x`` [B,H,W,C] contiguous NHWC float32 on
    the GPU, C % 4 == 0, stride 1 or 2 -> [B, ceil(H/stride), ceil(W/stride), C].  float32, f32_form 'exact' only."""
    who = 'stride_gather'
    _grad_operands(who, 'bottleneck backward', [('x', x)], ndim=4)
    _positive_maps(who, [('x', x)])
    stride = _stride_1_or_2(who, stride)
    _grad_on_gpu(who, [('x', x)])
    B, H, W, Cc = (int(v) for v in x.shape)
    out = _out(out, (B, (H - 1) // stride + 1, (W - 1) // stride + 1, Cc), torch.float32, x.device)
    L.call('odet_stride_gather_f32', L.dptr(x), B, H, W, Cc, stride, L.dptr(out), L.stream())
    return out


def block_input_grad(d1, dy=None, y=None, d2=None, stride=1, in_hw=None, out=None):
    """The gradient with respect to a bottleneck block's input in one launch (odet_block_input_grad_f32), in one of two forms.
    Identity shortcut -- ``dy`` and ``y`` given: dx = (y > 0 ? dy : +0) + d1, all [B,H,W,C] (y: the block's output, dy: its
    gradient, d1: the first convolution's input gradient); no d2, stride 1.  Convolutional shortcut -- no dy / y:
    dx[b,Y,X] = d1[b,Y/stride,X/stride] + d2[...] at the pixels both of whose coordinates are multiples of stride, +0 elsewhere;
    ``d1`` and the optional ``d2`` (the shortcut convolution's input gradient) [B,Ho,Wo,C], ``in_hw`` = (H, W) of the block's
    input with ceil(H/stride) == Ho (default: (Ho, Wo) at stride 1; required at stride 2, where two sizes share an Ho).
    Contiguous NHWC float32 GPU tensors, C % 4 == 0.  float32, f32_form 'exact' only."""
    who = 'block_input_grad'
    if (dy is None) != (y is None):
        raise ValueError('%s: dy and y come together (the identity form) or not at all (the convolutional-shortcut form)' % who)
    identity = dy is not None
    named = [(n, t) for n, t in (('d1', d1), ('dy', dy), ('y', y), ('d2', d2)) if t is not None or n == 'd1']
    _grad_operands(who, 'bottleneck backward', named, ndim=4)
    _positive_maps(who, named)
    stride = _stride_1_or_2(who, stride)
    if identity and (d2 is not None or stride != 1):
        raise ValueError('%s: the identity form (dy, y, d1) takes no d2 and stride 1 only' % who)
    B, Ho, Wo, Cc = (int(v) for v in d1.shape)
    for name, t in named[1:]:
        if tuple(t.shape) != (B, Ho, Wo, Cc):
            raise ValueError('%s: %s %s does not go with d1 %s' % (who, name, tuple(t.shape), (B, Ho, Wo, Cc)))
    if in_hw is None:
        if stride != 1:
            raise ValueError('%s: in_hw (the size of the block\'s input) is needed at stride 2' % who)
        in_hw = (Ho, Wo)
    H, W = int(in_hw[0]), int(in_hw[1])
    if H < 1 or W < 1 or ((H - 1) // stride + 1, (W - 1) // stride + 1) != (Ho, Wo):
        raise ValueError('%s: in_hw %s at stride %d does not go with d1 %s' % (who, (H, W), stride, (B, Ho, Wo, Cc)))
    _grad_on_gpu(who, named)
    out = _out(out, (B, H, W, Cc), torch.float32, d1.device)
    L.call('odet_block_input_grad_f32', L.dptr(dy), L.dptr(y), L.dptr(d1), L.dptr(d2), L.dptr(out), B, H, W, Cc, stride, L.stream())
    return out


def relu_maxpool2_backward(z, bias, dpool, out=None):
    """The backward of bias_relu_maxpool(z, bias, 2, 2, 0, ceil_mode=True) in one launch (odet_relu_maxpool2_backward_f32): TF's
    MaxPoolGrad then ReluGrad of MaxPooling2D((2,2), 2, 'same') after a ReLU convolution (vgg16_faster_rcnn.py:307, 325).  ``z``
    [B,H,W,C] (the convolution's raw output, without bias), ``bias`` [C], ``dpool`` [B,ceil(H/2),ceil(W/2),C] -> dz [B,H,W,C]:
    dpool at the first position of each window that holds its maximum of max(z + bias, 0) when that is > 0, +0 elsewhere.
    Contiguous NHWC float32 GPU tensors, C % 4 == 0.  float32, f32_form 'exact' only."""
    who = 'relu_maxpool2_backward'
    named = [('z', z), ('bias', bias), ('dpool', dpool)]
    _grad_operands(who, 'max-pooling backward', named)
    if z.dim() != 4 or int(z.shape[1]) < 1 or int(z.shape[2]) < 1 or int(z.shape[3]) < 4 or int(z.shape[3]) % 4:
        raise ValueError('%s: z %s must be an NHWC tensor [B,H,W,C] with a positive map size and C a positive multiple of 4'
                         % (who, tuple(z.shape)))
    B, H, W, Cc = (int(v) for v in z.shape)
    if tuple(bias.shape) != (Cc,):
        raise ValueError('%s: bias %s does not go with z %s' % (who, tuple(bias.shape), tuple(z.shape)))
    if tuple(dpool.shape) != (B, (H + 1) // 2, (W + 1) // 2, Cc):
        raise ValueError('%s: dpool %s does not go with z %s (the pooled map is %s)'
                         % (who, tuple(dpool.shape), tuple(z.shape), (B, (H + 1) // 2, (W + 1) // 2, Cc)))
    _grad_on_gpu(who, named)
    out = _out(out, (B, H, W, Cc), torch.float32, z.device)
    L.call('odet_relu_maxpool2_backward_f32', L.dptr(z), L.dptr(bias), L.dptr(dpool), L.dptr(out), B, H, W, Cc, L.stream())
    return out


def relu_maxpool3_backward(z, bias, dpool, out=None):
    """The backward of bias_relu_maxpool(z, bias, 3, 2, 1, ceil_mode=False) in one launch (odet_relu_maxpool3_backward_f32): TF's
    MaxPoolGrad through pool1_pad, then ReluGrad, behind the FPN stem's trainable conv1 (resnet_fpn.py:233-242).  ``z`` [B,H,W,C]
    (the convolution's raw output, without bias), ``bias`` [C], ``dpool`` [B,(H-1)//2+1,(W-1)//2+1,C] -> dz [B,H,W,C]: window (p,q)
    covers rows 2p-1..2p+1 and columns 2q-1..2q+1 inside the map and gives dpool[p,q] to the first tap in row-major order that
    holds its maximum of max(z + bias, 0) when that is > 0 (a NaN never wins); a pixel sums the up to four windows it wins in
    ascending (p,q) order, +0 where it wins none.  Elementwise, so the same under both grad forms.  Contiguous NHWC float32 GPU
    tensors, C % 4 == 0.  float32, f32_form 'exact' only."""
    who = 'relu_maxpool3_backward'
    named = [('z', z), ('bias', bias), ('dpool', dpool)]
    _grad_operands(who, 'max-pooling backward', named)
    if z.dim() != 4 or int(z.shape[1]) < 1 or int(z.shape[2]) < 1 or int(z.shape[3]) < 4 or int(z.shape[3]) % 4:
        raise ValueError('%s: z %s must be an NHWC tensor [B,H,W,C] with a positive map size and C a positive multiple of 4'
                         % (who, tuple(z.shape)))
    B, H, W, Cc = (int(v) for v in z.shape)
    if tuple(bias.shape) != (Cc,):
        raise ValueError('%s: bias %s does not go with z %s' % (who, tuple(bias.shape), tuple(z.shape)))
    pooled = (B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cc)
    if tuple(dpool.shape) != pooled:
        raise ValueError('%s: dpool %s does not go with z %s (the pooled map is %s)' % (who, tuple(dpool.shape), tuple(z.shape), pooled))
    _grad_on_gpu(who, named)
    out = _out(out, (B, H, W, Cc), torch.float32, z.device)
    L.call('odet_relu_maxpool3_backward_f32', L.dptr(z), L.dptr(bias), L.dptr(dpool), L.dptr(out), B, H, W, Cc, L.stream())
    return out


DROPOUT_STREAM_FC1, DROPOUT_STREAM_FC2 = 6, 7           # the Philox streams of the RoI head's two dropouts (0-5: include/odet.h)


def _dropout(sym, who, x, keep_prob, seed, image_id, stream_id, out):
    _grad_operands(who, 'dropout', [('x' if sym == 'odet_dropout_f32' else 'dy', x)])
    keep_prob = float(keep_prob)
    if not 0.0 < keep_prob <= 1.0:
        raise ValueError('%s: keep_prob must be in (0, 1], got %r' % (who, keep_prob))
    seed, image_id, stream_id = int(seed), int(image_id), int(stream_id)
    if not 0 <= seed < 1 << 64 or not 0 <= stream_id < 1 << 32:
        raise ValueError('%s: seed must be in [0, 2^64) and stream_id in [0, 2^32), got %d, %d' % (who, seed, stream_id))
    _grad_on_gpu(who, [('x', x)])
    out = _out(out, tuple(x.shape), torch.float32, x.device)
    L.call(sym, L.dptr(x), L.dptr(out), x.numel(), keep_prob, seed, image_id & 0xFFFFFFFF, stream_id, L.stream())
    return out


def dropout(x, keep_prob, seed, image_id, stream_id, out=None):
    """tf.nn.dropout(x, keep_prob) of TF r1.13 with the counter-based rule in place of TF's generator (odet_dropout_f32;
    vgg16_faster_rcnn.py:250-253): y = (x / keep_prob) * keep, keep = floor(keep_prob + u) with u from word e & 3 of
    philox((e >> 2, image_id, stream_id, 0), seed) for the flat element e.  ``x``: a contiguous float32 GPU tensor of any shape;
    keep_prob in (0, 1] (1: a copy); stream 6 is the dropout after fc1, 7 the one after fc2.  float32, f32_form 'exact' only."""
    return _dropout('odet_dropout_f32', 'dropout', x, keep_prob, seed, image_id, stream_id, out)


def dropout_backward(dy, keep_prob, seed, image_id, stream_id, out=None):
    """dropout's backward (odet_dropout_backward_f32): dx = (dy * keep) / keep_prob, the mask recomputed from the same counters"""
    return _dropout('odet_dropout_backward_f32', 'dropout_backward', dy, keep_prob, seed, image_id, stream_id, out)


class _DropoutTrainable(torch.autograd.Function):
    """ops.dropout forward, ops.dropout_backward backward; nothing is saved but the counters"""

    @staticmethod
    def forward(ctx, x, keep_prob, seed, image_id, stream_id):
        ctx.args = (keep_prob, seed, image_id, stream_id)
        return dropout(x, keep_prob, seed, image_id, stream_id)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        return dropout_backward(dy.contiguous(), *ctx.args), None, None, None, None


def dropout_trainable(x, keep_prob, seed, image_id, stream_id):
    """ops.dropout with a backward pass (float32, f32_form 'exact'): the forward is `dropout`, bit for bit.  keep_prob == 1 returns
    ``x`` itself, as tf.nn.dropout does."""
    if float(keep_prob) == 1.0:
        return x
    return _DropoutTrainable.apply(x.contiguous(), float(keep_prob), int(seed), int(image_id),
                                   int(stream_id))


def _gap_out(who, out, shape, name, operand):
    """the last two rules of the pooling fronts: a given ``out`` is one more shape rule (checked before the device, like every
    shape), then operand and ``out`` on the GPU -> the result tensor"""
    if out is not None:
        try:
            _out(out, shape, torch.float32, None)
        except ValueError as e:
            raise ValueError('%s: %s' % (who, e)) from None
    _grad_on_gpu(who, [(name, operand)] + ([('out', out)] if out is not None else []))
    return _out(out, shape, torch.float32, operand.device)


def global_avg_pool(x, out=None):
    """GlobalAveragePooling2D with a stated order (odet_global_avg_pool_f32; resnet_faster_rcnn.py:167-168, between the conv5 stack
    and the two Dense layers): out[r,c] = (x[r,0,0,c] + x[r,0,1,c] + ... ) / (float)(H W), the float32 sum over the pixels in
    row-major order, every add rounded, started from the first pixel itself; then one IEEE division.  ``x`` [R,H,W,C] contiguous
    NHWC float32 on the GPU, R, H, W >= 1, C % 4 == 0 -> [R,C].  float32, f32_form 'exact' only."""
    who = 'global_avg_pool'
    _grad_operands(who, 'pooling backward', [('x', x)], ndim=4)
    if min(int(v) for v in x.shape[:3]) < 1 or int(x.shape[3]) < 4 or int(x.shape[3]) % 4:
        raise ValueError('%s: x %s must have at least one row and one pixel and C a positive multiple of 4' % (who, tuple(x.shape)))
    R, H, W, Cc = (int(v) for v in x.shape)
    out = _gap_out(who, out, (R, Cc), 'x', x)
    L.call('odet_global_avg_pool_f32', L.dptr(x), R, H * W, Cc, L.dptr(out), L.stream())
    return out


def global_avg_pool_backward(g, hw, out=None):
    """global_avg_pool's backward (odet_global_avg_pool_backward_f32), TF's _MeanGrad: dx[r,y,x,c] = g[r,c] / (float)(H W) at every
    pixel.  ``g`` [R,C] contiguous float32 on the GPU, R >= 1, C % 4 == 0; ``hw`` = (H, W) of the pooled map, both >= 1
    -> [R,H,W,C].  float32, f32_form 'exact' only."""
    who = 'global_avg_pool_backward'
    _grad_operands(who, 'pooling backward', [('g', g)], ndim=2)
    if int(g.shape[0]) < 1 or int(g.shape[1]) < 4 or int(g.shape[1]) % 4:
        raise ValueError('%s: g %s must have at least one row and C a positive multiple of 4' % (who, tuple(g.shape)))
    H, W = int(hw[0]), int(hw[1])
    if H < 1 or W < 1:
        raise ValueError('%s: hw %s must be positive' % (who, (H, W)))
    R, Cc = int(g.shape[0]), int(g.shape[1])
    out = _gap_out(who, out, (R, H, W, Cc), 'g', g)
    L.call('odet_global_avg_pool_backward_f32', L.dptr(g), R, H * W, Cc, L.dptr(out), L.stream())
    return out


class _GlobalAvgPoolTrainable(torch.autograd.Function):
    """ops.global_avg_pool forward, ops.global_avg_pool_backward backward; nothing is saved but the map's size"""

    @staticmethod
    def forward(ctx, x):
        ctx.hw = (int(x.shape[1]), int(x.shape[2]))
        return global_avg_pool(x)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return global_avg_pool_backward(g.contiguous(), ctx.hw) if ctx.needs_input_grad[0] else None


def global_avg_pool_trainable(x):
    """ops.global_avg_pool with a backward pass (float32, f32_form 'exact'): the forward is `global_avg_pool`, bit for bit; the
    backward is one global_avg_pool_backward, computed only when ``x`` requires a gradient."""
    return _GlobalAvgPoolTrainable.apply(x)


def bias_act_(x, bias, residual=None, relu=True):
    """In place on an NHWC (or any [..., C] contiguous) activation: x = relu?((x + bias) (+ residual)) -- the
    convolution epilogue of the reference's ResNet blocks / RPN head (resnet_fpn.py:154-205) in one pass."""
    if x.dtype not in (torch.float32, torch.float16) or bias.dtype != x.dtype:
        raise TypeError('x and bias must both be float32 or both float16')
    if residual is not None and (residual.dtype != x.dtype or residual.shape != x.shape):
        raise ValueError('residual must match x in dtype and shape')
    Cc = int(x.shape[-1])
    if bias.numel() != Cc:
        raise ValueError('bias must have %d elements' % Cc)
    L.call('odet_bias_act', L.dptr(x), L.dptr(bias), L.dptr(residual), x.numel() // Cc, Cc, 1 if relu else 0,
           1 if x.dtype == torch.float16 else 0, L.stream())
    return x


def rpn_pack(level_out, bias, out, out_offset):
    """One level of the RPN head's output into the concatenated arrays: ``level_out`` [B,h,w,ch] NHWC (float32 /
    float16, the 1x1 convolution WITHOUT its bias), ``bias`` [ch] of the same dtype, ``out`` float32 [B, N, 2 or 4]
    contiguous; ``out_offset`` = the level's first VALUE (anchor offset x 2 or 4) inside an image."""
    if level_out.dim() != 4 or not level_out.is_contiguous():
        raise ValueError('level_out must be a contiguous NHWC [B,h,w,ch] tensor')
    if level_out.dtype not in (torch.float32, torch.float16) or bias.dtype != level_out.dtype:
        raise TypeError('level_out and bias must both be float32 or both float16')
    B, h, w, ch = (int(v) for v in level_out.shape)
    if out.dtype != torch.float32 or not out.is_contiguous() or out.shape[0] != B:
        raise ValueError('out must be a contiguous float32 [B, N, k] tensor')
    stride = out.numel() // max(B, 1)
    L.call('odet_rpn_pack', L.dptr(level_out), L.dptr(bias), h * w, ch, B, L.dptr(out), stride, int(out_offset),
           1 if level_out.dtype == torch.float16 else 0, L.stream())
    return out


def bias_relu_maxpool(x, bias, kernel, stride, pad=0, ceil_mode=False):
    """maxpool(relu(x + bias)) in one pass: ``x`` NHWC [B,H,W,C] contiguous (float32 / float16; a convolution WITHOUT
    its bias), ``bias`` [C]; window ``kernel`` x ``kernel``, ``stride``, ``pad`` skipped taps on every side;
    ``ceil_mode`` as torch's max_pool2d (TF 'same' pooling for kernel == stride).  Returns NHWC [B,OH,OW,C]."""
    if x.dim() != 4 or not x.is_cuda or not x.is_contiguous() or x.dtype not in (torch.float32, torch.float16):
        raise ValueError('x must be a contiguous NHWC float32 / float16 GPU tensor')
    B, H, W, Cn = (int(v) for v in x.shape)
    if bias.dtype != x.dtype or bias.numel() != Cn or not bias.is_contiguous():
        raise ValueError('bias must be a contiguous [C] tensor of the same dtype')

    def osz(n):
        a = n + 2 * pad - kernel
        o = (-(-a // stride) if ceil_mode else a // stride) + 1
        if ceil_mode and (o - 1) * stride >= n + pad:        # torch: the last window must start inside the map
            o -= 1
        return o
    OH, OW = osz(H), osz(W)
    out = torch.empty((B, OH, OW, Cn), dtype=x.dtype, device=x.device)
    L.call('odet_bias_relu_maxpool', L.dptr(x), L.dptr(bias), L.dptr(out), B, H, W, Cn, OH, OW, int(kernel), int(stride),
           int(pad), 1 if x.dtype == torch.float16 else 0, L.stream())
    return out


def rpn_head_tail(conv_out, conv_bias, weight, bias, num_anchors, scores, deltas, anchor_offset):
    """Everything of the RpnHead after its 3x3 convolution for one level, in one MFMA pass: ``conv_out`` [B,h,w,512]
    float16 NHWC contiguous (the 3x3 convolution WITHOUT its bias), ``conv_bias`` [512], ``weight`` [6A,512(,1,1)]
    (2A score rows then 4A delta rows), ``bias`` [6A]; relu(conv_out + conv_bias) . weight^T + bias -> the level's
    slices of ``scores`` [B,N,2] / ``deltas`` [B,N,4] (float32) starting at anchor ``anchor_offset``."""
    A = int(num_anchors)
    if conv_out.dim() != 4 or conv_out.dtype != torch.float16 or not conv_out.is_contiguous() or conv_out.shape[3] != 512:
        raise ValueError('conv_out must be a contiguous float16 NHWC [B,h,w,512] tensor')
    if weight.dtype != torch.float16 or weight.numel() != 6 * A * 512:
        raise ValueError('weight must be a float16 [6A, 512] tensor')
    w = weight.reshape(6 * A, 512)
    if not w.is_contiguous():
        w = w.contiguous()
    for t, n_ in ((conv_bias, 512), (bias, 6 * A)):
        if t.dtype != torch.float16 or t.numel() != n_ or not t.is_contiguous():
            raise ValueError('conv_bias [512] / bias [6A] must be contiguous float16 tensors')
    B, h, w_ = (int(v) for v in conv_out.shape[:3])
    for t, k in ((scores, 2), (deltas, 4)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 3 or t.shape[0] != B or t.shape[2] != k:
            raise ValueError('scores / deltas must be contiguous float32 [B, N, 2] / [B, N, 4] tensors')
    L.call('odet_rpn_head_tail_f16', L.dptr(conv_out), L.dptr(conv_bias), L.dptr(w), L.dptr(bias), h * w_, A, B,
           L.dptr(scores), scores.numel() // max(B, 1), int(anchor_offset) * 2, L.dptr(deltas),
           deltas.numel() // max(B, 1), int(anchor_offset) * 4, L.stream())
    return scores, deltas


_CONV3X3_FORMS = {torch.float16: ('odet_conv3x3_f16', 'float16', 64), torch.float32: ('odet_conv3x3_f32', 'float32', 32)}


def _conv3x3_weight(weight, cin, cout, dtype, name):
    if weight.dtype != dtype or weight.dim() != 4 or weight.numel() != cout * 9 * cin:
        raise ValueError('weight must be %s [cout,cin,3,3] (channels_last) or [cout,3,3,cin]' % name)
    if tuple(weight.shape[1:]) == (cin, 3, 3):
        w = weight.permute(0, 2, 3, 1)                    # [cout,3,3,cin] view; contiguous iff channels_last memory
    elif tuple(weight.shape[1:]) == (3, 3, cin):
        w = weight
    else:
        raise ValueError('weight shape %s does not match cin = %d' % (tuple(weight.shape), cin))
    return w if w.is_contiguous() else w.contiguous()


def _conv3x3(dtype, x, weight, bias, relu, out):
    sym, name, _ = _CONV3X3_FORMS[dtype]
    if x.dtype != dtype or not x.is_cuda or x.dim() != 4 or not x.is_contiguous():
        raise ValueError('x must be a contiguous NHWC %s GPU tensor [B,H,W,cin]' % name)
    B, H, W, cin = (int(v) for v in x.shape)
    cout = int(weight.shape[0])
    w = _conv3x3_weight(weight, cin, cout, dtype, name)
    if bias is not None and (bias.dtype != dtype or bias.numel() != cout or not bias.is_contiguous()):
        raise ValueError('bias must be a contiguous %s [cout] tensor' % name)
    shape = (B, H, W, cout)
    out = _out(out, shape, dtype, x.device)
    ws, wp, extra = None, L.dptr(w), ()
    if dtype == torch.float32:
        ws, sym, wp, extra = _f32_sym('odet_conv3x3_%s', w, weight)
    _f32_call(ws, sym, L.dptr(x), wp, L.dptr(bias) if bias is not None else None, L.dptr(out), B, H, W,
           cin, cout, 1 if relu else 0, *extra, L.stream())
    return out


def _conv3x3_levels(dtype, xs, weight, bias, relu, outs):
    sym, name, _ = _CONV3X3_FORMS[dtype]
    if not 1 <= len(xs) <= MAX_LEVELS:
        raise ValueError('between 1 and %d maps expected' % MAX_LEVELS)
    B, cin = int(xs[0].shape[0]), int(xs[0].shape[3])
    cout = int(weight.shape[0])
    w = _conv3x3_weight(weight, cin, cout, dtype, name)
    if bias is not None and (bias.dtype != dtype or bias.numel() != cout or not bias.is_contiguous()):
        raise ValueError('bias must be a contiguous %s [cout] tensor' % name)
    lv = (L.OdetConvLevel * len(xs))()
    if outs is None:
        outs = [torch.empty(tuple(x.shape[:3]) + (cout,), dtype=dtype, device=x.device) for x in xs]
    for i, (x, y) in enumerate(zip(xs, outs)):
        if x.dtype != dtype or not x.is_cuda or x.dim() != 4 or not x.is_contiguous() or int(x.shape[0]) != B \
                or int(x.shape[3]) != cin:
            raise ValueError('maps must be contiguous NHWC %s GPU tensors [B,H,W,cin] of one batch size' % name)
        if y.dtype != dtype or tuple(y.shape) != tuple(x.shape[:3]) + (cout,) or not y.is_contiguous():
            raise ValueError('outs must be contiguous %s tensors [B,H,W,cout]' % name)
        lv[i].x, lv[i].y, lv[i].H, lv[i].W = x.data_ptr(), y.data_ptr(), int(x.shape[1]), int(x.shape[2])
    ws, sym, wp, extra = None, sym + '_levels', L.dptr(w), ()
    if dtype == torch.float32:
        ws, sym, wp, extra = _f32_sym('odet_conv3x3_%s_levels', w, weight)
    _f32_call(ws, sym, lv, len(xs), wp, L.dptr(bias) if bias is not None else None, B, cin, cout,
           1 if relu else 0, *extra, L.stream())
    return outs


def conv3x3_f16(x, weight, bias=None, relu=False, out=None):
    """3x3 stride-1 'same' convolution as ONE hand-written implicit-GEMM kernel on the matrix cores (the RpnHead's
    convolution, base_fpn_model.py:401-417): ``x`` NHWC float16 contiguous [B,H,W,cin]; ``weight`` float16
    [cout,cin,3,3] in channels_last memory format (= [cout][3][3][cin]: `w.contiguous(memory_format=channels_last)`)
    or an explicit [cout,3,3,cin] tensor; ``bias`` float16 [cout] or None; -> NHWC float16 [B,H,W,cout].
    cin % 64 == 0, cout % 64 == 0 (256-channel tiles; 128 / 64-channel tiles when cout is not a multiple of 256)."""
    return _conv3x3(torch.float16, x, weight, bias, relu, out)


def conv3x3_relu_pool2_f16(x, weight, bias, out=None):
    """max_pool2x2/2 'same' (relu(conv3x3(x) + bias)) in ONE launch (odet_conv3x3_relu_pool2_f16; a VGG16 stage's last
    convolution with its pooling, vgg16_faster_rcnn.py:260-342): operands as conv3x3_f16, -> NHWC float16
    [B, ceil(H/2), ceil(W/2), cout]; the un-pooled map is never written."""
    if x.dtype != torch.float16 or not x.is_cuda or x.dim() != 4 or not x.is_contiguous():
        raise ValueError('x must be a contiguous NHWC float16 GPU tensor [B,H,W,cin]')
    B, H, W, cin = (int(v) for v in x.shape)
    cout = int(weight.shape[0])
    w = _conv3x3_weight(weight, cin, cout, torch.float16, 'float16')
    if bias is None or bias.dtype != torch.float16 or bias.numel() != cout or not bias.is_contiguous():
        raise ValueError('bias must be a contiguous float16 [cout] tensor')
    shape = (B, (H + 1) // 2, (W + 1) // 2, cout)
    out = _out(out, shape, torch.float16, x.device)
    L.call('odet_conv3x3_relu_pool2_f16', L.dptr(x), L.dptr(w), L.dptr(bias), L.dptr(out), B, H, W, cin, cout, L.stream())
    return out


def conv3x3_f16_levels(xs, weight, bias=None, relu=False, outs=None):
    """conv3x3_f16 with shared weights over a list of NHWC float16 maps [B,H_l,W_l,cin] (the RpnHead over the pyramid
    levels) in ONE launch; -> list of [B,H_l,W_l,cout]."""
    return _conv3x3_levels(torch.float16, xs, weight, bias, relu, outs)


def rpn_head_fused(xs, conv_weight, conv_bias, weight, bias, num_anchors, scores, deltas):
    """The whole RpnHead over the pyramid levels in ONE launch (odet_rpn_head_fused_f16): ``xs`` NHWC float16 maps
    [B,H_l,W_l,cin] in concatenation order, ``conv_weight`` [cout,cin,3,3] (channels_last) / ``conv_bias`` [cout] of the
    3x3 convolution, ``weight`` [6A,cout(,1,1)] / ``bias`` [6A] = the score rows then the delta rows of the two 1x1
    convolutions; relu(conv + conv_bias) . weight^T + bias -> ``scores`` [B,N,2] / ``deltas`` [B,N,4] float32 (a
    workgroup walks the channel tiles of its pixel slab: no workspace, no second launch).  cout in {256, 512}."""
    A = int(num_anchors)
    if not 1 <= len(xs) <= MAX_LEVELS:
        raise ValueError('between 1 and %d maps expected' % MAX_LEVELS)
    B, cin = int(xs[0].shape[0]), int(xs[0].shape[3])
    cout = int(conv_weight.shape[0])
    w3 = _conv3x3_weight(conv_weight, cin, cout, torch.float16, 'float16')
    if weight.dtype != torch.float16 or weight.numel() != 6 * A * cout:
        raise ValueError('weight must be a float16 [6A, cout] tensor')
    w1 = weight.reshape(6 * A, cout)
    if not w1.is_contiguous():
        w1 = w1.contiguous()
    for t, n_ in ((conv_bias, cout), (bias, 6 * A)):
        if t.dtype != torch.float16 or t.numel() != n_ or not t.is_contiguous():
            raise ValueError('conv_bias [cout] / bias [6A] must be contiguous float16 tensors')
    lv = (L.OdetConvLevel * len(xs))()
    n = 0
    for i, x in enumerate(xs):
        if x.dtype != torch.float16 or not x.is_cuda or x.dim() != 4 or not x.is_contiguous() or int(x.shape[0]) != B \
                or int(x.shape[3]) != cin:
            raise ValueError('maps must be contiguous NHWC float16 GPU tensors [B,H,W,cin] of one batch size')
        lv[i].x, lv[i].y, lv[i].H, lv[i].W = x.data_ptr(), None, int(x.shape[1]), int(x.shape[2])
        n += int(x.shape[1]) * int(x.shape[2]) * A
    for t, k in ((scores, 2), (deltas, 4)):
        if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != (B, n, k):
            raise ValueError('scores / deltas must be contiguous float32 [B, N, 2] / [B, N, 4] tensors, N = sum H*W*A')
    L.call('odet_rpn_head_fused_f16', lv, len(xs), L.dptr(w3), L.dptr(conv_bias), L.dptr(w1), L.dptr(bias), A, B, cin, cout,
           L.dptr(scores), n * 2, L.dptr(deltas), n * 4, L.stream())
    return scores, deltas


def conv3x3_conv1x1_f16(x, weight2, bias2, weight3, bias3, residual=None, relu=True, out=None):
    """A bottleneck block's 3x3 convolution and its last 1x1 convolution in ONE launch (odet_conv3x3_conv1x1_f16):
    relu(relu(conv3x3(x, weight2) + bias2) . weight3^T + bias3 + residual).  ``x`` NHWC float16 [B,H,W,cin], ``weight2``
    [cmid,cin,3,3] (channels_last) with cmid = 64, 128 or 256 (ResNet conv2 / conv3 / conv4: one workgroup holds all of them),
    ``weight3`` [n3,cmid(,1,1)], ``residual`` / ``out`` NHWC float16 [B,H,W,n3]."""
    if x.dtype != torch.float16 or not x.is_cuda or x.dim() != 4 or not x.is_contiguous():
        raise ValueError('x must be a contiguous NHWC float16 GPU tensor [B,H,W,cin]')
    B, H, W, cin = (int(v) for v in x.shape)
    cmid = int(weight2.shape[0])
    if cmid not in (64, 128, 256):
        raise ValueError('the 3x3 convolution must have 64, 128 or 256 output channels')
    w2 = _conv3x3_weight(weight2, cin, cmid, torch.float16, 'float16')
    n3 = int(weight3.shape[0])
    if weight3.dtype != torch.float16 or weight3.numel() != n3 * cmid:
        raise ValueError('weight3 must be a float16 [n3, cmid] tensor')
    w3 = weight3.reshape(n3, cmid)
    if not w3.is_contiguous():
        w3 = w3.contiguous()
    for t, n_ in ((bias2, cmid), (bias3, n3)):
        if t.dtype != torch.float16 or t.numel() != n_ or not t.is_contiguous():
            raise ValueError('bias2 [cmid] / bias3 [n3] must be contiguous float16 tensors')
    shape = (B, H, W, n3)
    if residual is not None and (residual.dtype != torch.float16 or tuple(residual.shape) != shape or not residual.is_contiguous()):
        raise ValueError('residual must be a contiguous float16 tensor [B,H,W,n3]')
    out = _out(out, shape, torch.float16, x.device)
    L.call('odet_bottleneck_tail_f16', L.dptr(x), L.dptr(w2), L.dptr(bias2), L.dptr(w3), L.dptr(bias3),
           L.dptr(residual) if residual is not None else None, L.dptr(out), B, H, W, cin, cmid, n3, 1 if relu else 0,
           L.stream())
    return out


def stem_pack_weights(weight):
    """[64,3,7,7] float16 stem weights (any strides) -> the packed [64*7*32] float16 layout of stem_conv7_pool3."""
    if weight.dtype != torch.float16 or tuple(weight.shape) != (64, 3, 7, 7) or not weight.is_cuda:
        raise ValueError('weight must be a float16 [64,3,7,7] GPU tensor')
    packed = torch.empty(64 * 7 * 32, dtype=torch.float16, device=weight.device)
    so, sc, sy, sx = (int(v) for v in weight.stride())
    L.call('odet_stem_pack_weights_f16', C.c_void_p(weight.data_ptr()), so, sc, sy, sx, L.dptr(packed), L.stream())     # (any strides)
    return packed


def stem_conv7_pool3(images_nhwc, packed_weight, bias, out=None):
    """The ResNet stem in ONE launch (odet_stem_conv7_pool3_f16): pad 3 + 7x7/2 convolution + bias + ReLU + pad 1 + 3x3/2
    max-pooling from the NHWC image [B,H,W,3] (float32 or float16) to NHWC float16 [B,PH,PW,64]."""
    x = images_nhwc
    if x.dtype not in (torch.float32, torch.float16) or not x.is_cuda or x.dim() != 4 or int(x.shape[3]) != 3 or not x.is_contiguous():
        raise ValueError('images must be a contiguous NHWC float32 / float16 GPU tensor [B,H,W,3]')
    if packed_weight.dtype != torch.float16 or packed_weight.numel() != 64 * 7 * 32 or not packed_weight.is_contiguous():
        raise ValueError('packed_weight: the result of stem_pack_weights')
    if bias.dtype != torch.float16 or bias.numel() != 64 or not bias.is_contiguous():
        raise ValueError('bias must be a contiguous float16 [64] tensor')
    B, H, W = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
    ch, cw = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    shape = (B, (ch - 1) // 2 + 1, (cw - 1) // 2 + 1, 64)
    out = _out(out, shape, torch.float16, x.device)
    L.call('odet_stem_conv7_pool3_f16', L.dptr(x), 1 if x.dtype == torch.float16 else 0, L.dptr(packed_weight), L.dptr(bias),
           L.dptr(out), B, H, W, L.stream())
    return out


def conv3x3_rgb_pack_weights(weight):
    """[64,3,3,3] float16 weights of a 3-channel 3x3 convolution (any strides) -> the packed [4*2*64*8] float16 layout of
    conv3x3_rgb."""
    if weight.dtype != torch.float16 or tuple(weight.shape) != (64, 3, 3, 3) or not weight.is_cuda:
        raise ValueError('weight must be a float16 [64,3,3,3] GPU tensor')
    packed = torch.empty(4 * 2 * 64 * 8, dtype=torch.float16, device=weight.device)
    so, sc, sy, sx = (int(v) for v in weight.stride())
    L.call('odet_conv3x3_rgb_pack_weights_f16', C.c_void_p(weight.data_ptr()), so, sc, sy, sx, L.dptr(packed), L.stream())
    return packed


def conv3x3_rgb(images_nhwc, packed_weight, bias, relu=True, out=None):
    """VGG16's first convolution in ONE launch (odet_conv3x3_rgb_f16): Conv2D(64, 3x3, 'same') + bias (+ ReLU) from the NHWC
    image [B,H,W,3] (float32 or float16) to NHWC float16 [B,H,W,64]."""
    x = images_nhwc
    if x.dtype not in (torch.float32, torch.float16) or not x.is_cuda or x.dim() != 4 or int(x.shape[3]) != 3 or not x.is_contiguous():
        raise ValueError('images must be a contiguous NHWC float32 / float16 GPU tensor [B,H,W,3]')
    if packed_weight.dtype != torch.float16 or packed_weight.numel() != 4 * 2 * 64 * 8 or not packed_weight.is_contiguous():
        raise ValueError('packed_weight: the result of conv3x3_rgb_pack_weights')
    if bias.dtype != torch.float16 or bias.numel() != 64 or not bias.is_contiguous():
        raise ValueError('bias must be a contiguous float16 [64] tensor')
    B, H, W = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
    shape = (B, H, W, 64)
    out = _out(out, shape, torch.float16, x.device)
    L.call('odet_conv3x3_rgb_f16', L.dptr(x), 1 if x.dtype == torch.float16 else 0, L.dptr(packed_weight), L.dptr(bias),
           L.dptr(out), B, H, W, 1 if relu else 0, L.stream())
    return out


def conv3x3_f32(x, weight, bias=None, relu=False, out=None):
    """conv3x3_f16 in the reference's precision: float32 operands and result, exact-float32 matrix instructions
    (every product and sum rounded to float32 once, as a chain of fmaf).  cin % 32 == 0, cout % 64 == 0."""
    return _conv3x3(torch.float32, x, weight, bias, relu, out)


def conv3x3_f32_levels(xs, weight, bias=None, relu=False, outs=None):
    """conv3x3_f32 with shared weights over a list of NHWC float32 maps in ONE launch."""
    return _conv3x3_levels(torch.float32, xs, weight, bias, relu, outs)


def conv1x1_f16(x, weight, bias, residual=None, relu=True, out=None, in_bias=None):
    """1x1 stride-1 convolution + bias (+ residual) (+ ReLU) in ONE kernel on the matrix cores: ``x`` [..., cin]
    NHWC float16 contiguous (any leading dims), ``weight`` [cout, cin(, 1, 1)], ``bias`` [cout], ``residual`` /
    ``out`` [..., cout] (``out`` may be ``residual``).  cin in {64, 128, 256, 512}, cout % 64 == 0.  ``in_bias`` [cin]:
    ``x`` is the preceding convolution without its bias and ReLU; relu(x + in_bias) is applied on load."""
    if x.dtype != torch.float16 or not x.is_cuda or not x.is_contiguous():
        raise ValueError('x must be a contiguous float16 GPU tensor [..., cin]')
    cin = int(x.shape[-1])
    cout = int(weight.shape[0])
    if weight.dtype != torch.float16 or weight.numel() != cout * cin:
        raise ValueError('weight must be a float16 [cout, cin] (or [cout, cin, 1, 1]) tensor')
    w = weight.reshape(cout, cin)       # (a channels_last [cout, cin, 1, 1] weight is the same memory: a view)
    if not w.is_contiguous():
        w = w.contiguous()
    if bias.dtype != torch.float16 or bias.numel() != cout or not bias.is_contiguous():
        raise ValueError('bias must be a contiguous float16 [cout] tensor')
    shape = tuple(x.shape[:-1]) + (cout,)
    if residual is not None and (residual.dtype != torch.float16 or tuple(residual.shape) != shape
                                 or not residual.is_contiguous()):
        raise ValueError('residual must be a contiguous float16 tensor shaped like the output')
    out = _out(out, shape, torch.float16, x.device)
    if out.data_ptr() == x.data_ptr():
        raise ValueError('out must not alias x')
    if in_bias is not None and (in_bias.dtype != torch.float16 or in_bias.numel() != cin or not in_bias.is_contiguous()):
        raise ValueError('in_bias must be a contiguous float16 [cin] tensor')
    L.call('odet_conv1x1_f16', L.dptr(x), L.dptr(in_bias) if in_bias is not None else None, L.dptr(w), L.dptr(bias),
           L.dptr(residual) if residual is not None else None,
           L.dptr(out), x.numel() // cin, cin, cout, 1 if relu else 0, L.stream())
    return out


_PW_FORMS = {torch.float16: ('f16', 'float16', 64), torch.float32: ('f32', 'float32', 32)}     # suffix, name, K granule


def _pw_args(x, weight, bias, who, min_k=True):
    if x.dtype not in _PW_FORMS:
        raise ValueError('%s: x must be float16 or float32' % who)
    sfx, name, gran = _PW_FORMS[x.dtype]
    if not x.is_cuda or not x.is_contiguous() or x.dim() != 4:
        raise ValueError('%s: x must be a contiguous %s GPU tensor [batch, H, W, cin]' % (who, name))
    cin, cout = int(x.shape[-1]), int(weight.shape[0])
    if weight.dtype != x.dtype or weight.numel() % cout:
        raise ValueError('%s: weight must be a %s [cout, cin(, 1, 1)] tensor' % (who, name))
    w = weight.reshape(cout, -1)
    if w.shape[1] != cin:             # (the kernels read the weight rows with stride cin)
        raise ValueError('%s: weight has %d input channels, x %d' % (who, w.shape[1], cin))
    if not w.is_contiguous():
        w = w.contiguous()
    if bias is not None and (bias.dtype != x.dtype or bias.numel() != cout or not bias.is_contiguous()):
        raise ValueError('%s: bias must be a contiguous %s [cout] tensor' % (who, name))
    if cin % gran or (min_k and cin < 2 * gran) or cout % 64:
        raise ValueError('%s: cin %d must be a multiple of %d (>= %d), cout %d a multiple of 64' % (who, cin, gran, 2 * gran, cout))
    return w, cin, cout, sfx


def pointwise(x, weight, bias=None, residual=None, relu=False, stride=1, out=None):
    """A 1x1 convolution (stride 1 or 2, 'valid') or dense layer as the LDS-staged GEMM on the matrix cores
    (odet_pointwise_f16 / odet_pointwise_f32 by the dtype of ``x``): ``x`` [B,H,W,cin] NHWC contiguous, ``weight``
    [cout, cin(, 1, 1)], ``residual`` / ``out`` [B, ceil(H/stride), ceil(W/stride), cout];
    relu?(x[:, ::stride, ::stride] . w^T + bias + residual).  float32: exact-float32 matrix instructions."""
    w, cin, cout, sfx = _pw_args(x, weight, bias, 'pointwise')
    B, H, W = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
    stride = int(stride)
    shape = (B, (H + stride - 1) // stride, (W + stride - 1) // stride, cout)
    if residual is not None and (residual.dtype != x.dtype or tuple(residual.shape) != shape or not residual.is_contiguous()):
        raise ValueError('residual must be a contiguous tensor of the output\'s dtype and shape %s' % (shape,))
    out = _out(out, shape, x.dtype, x.device)
    ws, sym, wp, extra = _f32_sym('odet_pointwise_%s', w, weight) if sfx == 'f32' else (None, 'odet_pointwise_f16', L.dptr(w), ())
    _f32_call(ws, sym, L.dptr(x), wp, L.dptr(bias) if bias is not None else None,
           L.dptr(residual) if residual is not None else None, L.dptr(out), B, H, W, stride, cin, cout, 1 if relu else 0,
           *extra, L.stream())
    return out


def dense(x, weight, bias=None, relu=False, out=None):
    """keras Dense on the same kernel: ``x`` [rows, cin] contiguous, ``weight`` [cout, cin] -> [rows, cout]."""
    if x.dim() != 2:
        raise ValueError('dense: x must be [rows, cin]')
    y = pointwise(x.view(1, 1, x.shape[0], x.shape[1]), weight, bias, None, relu, 1,
                  None if out is None else out.view(1, 1, out.shape[0], out.shape[1]))
    return y.view(x.shape[0], -1)


def _dense_grad_args(who, dy, other, other_name, other_cols, y_relu):
    """the front dense_dgrad / dense_wgrad share: _grad_operands on 2-D tensors, the kernels' shape rules, _grad_on_gpu ->
    (rows, cin, cout)"""
    named = [('dy', dy), (other_name, other)] + ([('y_relu', y_relu)] if y_relu is not None else [])
    _grad_operands(who, 'Dense backward', named, ndim=2)
    rows, cout = int(dy.shape[0]), int(dy.shape[1])
    if y_relu is not None and tuple(y_relu.shape) != (rows, cout):
        raise ValueError('%s: y_relu must have the shape of dy %s, got %s' % (who, (rows, cout), tuple(y_relu.shape)))
    if int(other.shape[0]) != other_cols(rows, cout):
        raise ValueError('%s: %s %s does not go with dy %s' % (who, other_name, tuple(other.shape), (rows, cout)))
    cin = int(other.shape[1])
    if rows < 1 or cin % 32 or cin < 64 or cout % 64 or cout < 64:
        raise ValueError('%s: rows %d must be positive, cin %d a multiple of 32 (>= 64), cout %d a multiple of 64'
                         % (who, rows, cin, cout))
    _grad_on_gpu(who, named)
    return rows, cin, cout


def dense_dgrad(dy, weight, y_relu=None, x_relu=None, out=None):
    """The input gradient of a float32 Dense layer (odet_dense_dgrad_f32): dy [rows, cout], weight [cout, cin] (the forward's
    own layout) -> dx [rows, cin] = dz . weight, dz = dy where y_relu > 0 else 0 (y_relu: the layer's forward output, when it
    had a ReLU); x_relu (the forward output of the layer below, [rows, cin]) keeps dx only where it is > 0."""
    rows, cin, cout = _dense_grad_args('dense_dgrad', dy, weight, 'weight', lambda r, c: c, y_relu)
    if x_relu is not None and (not isinstance(x_relu, torch.Tensor) or x_relu.dtype != torch.float32 or not x_relu.is_cuda
                               or tuple(x_relu.shape) != (rows, cin) or not x_relu.is_contiguous()):
        raise ValueError('dense_dgrad: x_relu must be a contiguous float32 GPU tensor of shape %s' % ((rows, cin),))
    out = _out(out, (rows, cin), torch.float32, dy.device)
    entry, query = _grad_symbols(('odet_dense_dgrad_f32', 'odet_dense_grad_workspace_bytes'),
                                 ('odet_dense_dgrad_x3', 'odet_dense_grad_x3_workspace_bytes'))
    wsp, wsn = _grad_workspace(query, (0, rows, cin, cout), dy.device)
    L.call(entry, L.dptr(dy), L.dptr(weight), L.dptr(y_relu), L.dptr(x_relu), L.dptr(out), rows, cin, cout,
           wsp, wsn, L.stream())
    return out


def dense_wgrad(dy, x, y_relu=None, with_bias=True, out=None):
    """The parameter gradients of a float32 Dense layer (odet_dense_wgrad_f32): dy [rows, cout], x [rows, cin] (the layer's
    input) -> (dw [cout, cin] = dz^T . x, db [cout] = column sums of dz, or None without with_bias); dz as in dense_dgrad."""
    rows, cin, cout = _dense_grad_args('dense_wgrad', dy, x, 'x', lambda r, c: r, y_relu)
    dw = _out(out, (cout, cin), torch.float32, dy.device)
    db = torch.empty((cout,), dtype=torch.float32, device=dy.device) if with_bias else None
    entry, query = _grad_symbols(('odet_dense_wgrad_f32', 'odet_dense_grad_workspace_bytes'),
                                 ('odet_dense_wgrad_x3', 'odet_dense_grad_x3_workspace_bytes'))
    wsp, wsn = _grad_workspace(query, (1, rows, cin, cout), dy.device)
    L.call(entry, L.dptr(dy), L.dptr(x), L.dptr(y_relu), L.dptr(dw), L.dptr(db), rows, cin, cout, wsp, wsn,
           L.stream())
    return dw, db


@carries_grad_form
class _DenseTrainable(torch.autograd.Function):
    """ops.dense forward; odet_dense_wgrad_f32 (and, only when the input needs a gradient, odet_dense_dgrad_f32) backward"""

    @staticmethod
    def forward(ctx, x, weight, bias, relu):
        y = dense(x, weight, bias, relu)
        ctx.relu = bool(relu)
        ctx.save_for_backward(x, weight, y if relu else None)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, weight, y = ctx.saved_tensors
        dy = dy.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            dw, db = dense_wgrad(dy, x, y, with_bias=ctx.has_bias and ctx.needs_input_grad[2])
            dw = dw if ctx.needs_input_grad[1] else None
        if ctx.needs_input_grad[0]:
            dx = dense_dgrad(dy, weight, y)
        return dx, dw, db, None


def dense_trainable(x, weight, bias, relu=False):
    """ops.dense with a backward pass (float32, f32_form 'exact'): the forward is `dense`, bit for bit; `.backward()` leaves
    weight.grad [cout, cin] and bias.grad [cout] contiguous in the variables' shapes (what training.train_step takes), and
    computes the input gradient only when x requires one."""
    _grad_f32('dense_trainable', 'Dense backward', [('x', x), ('weight', weight)])
    if x.dim() != 2 or weight.dim() != 2 or not weight.is_contiguous():
        raise ValueError('dense_trainable: x must be [rows, cin] and weight a contiguous [cout, cin]')
    return _DenseTrainable.apply(x.contiguous(), weight, bias, bool(relu))


def _conv_grad_maps(who, named_lists):
    """the front the 3x3 convolution's backward ops share: 1..MAX_LEVELS maps, the lists equally long, _grad_operands on every map,
    one batch size and the lists shaped level by level -> (levels, batch, the named tensors for _grad_on_gpu, which the caller
    runs after its shape rules)"""
    lists = [(name, ts) for name, ts in named_lists if ts is not None]
    n = len(lists[0][1])
    if not 1 <= n <= MAX_LEVELS or any(len(ts) != n for _, ts in lists):
        raise ValueError('%s: between 1 and %d maps expected, as many in every list' % (who, MAX_LEVELS))
    every = [('%s[%d]' % (name, i), t) for name, ts in lists for i, t in enumerate(ts) if t is not None]
    _grad_operands(who, 'convolution backward', every, ndim=4)
    B = int(lists[0][1][0].shape[0])
    for i in range(n):
        hw = tuple(lists[0][1][i].shape[:3])
        for name, ts in lists:
            chans = next(int(t.shape[3]) for t in ts if t is not None)
            if ts[i] is not None and (tuple(ts[i].shape[:3]) != hw or int(ts[i].shape[3]) != chans or hw[0] != B):
                raise ValueError('%s: %s[%d] %s does not go with %s[%d] %s (one batch size, one channel count per list)'
                                 % (who, name, i, tuple(ts[i].shape), lists[0][0], i, tuple(lists[0][1][i].shape)))
    return n, B, every


def conv3x3_wgrad_f32_levels(xs, dys, y_relus=None, with_bias=True, out=None):
    """The parameter gradients of conv3x3_f32_levels (odet_conv3x3_wgrad_f32_levels): xs [B,H,W,cin] (the layer's inputs) and dys
    [B,H,W,cout] per level, contiguous NHWC float32 -> (dw [cout,3,3,cin], the forward's weight layout, summed over the levels;
    db [cout], or None without with_bias).  dz = dy where y_relu > 0 else 0 for the levels whose y_relus entry (the forward
    output) is given.  cin % 32 == 0, cout % 64 == 0."""
    who = 'conv3x3_wgrad_f32_levels'
    if y_relus is not None and all(y is None for y in y_relus):
        y_relus = None
    n, B, every = _conv_grad_maps(who, [('xs', xs), ('dys', dys), ('y_relus', y_relus)])
    cin, cout = int(xs[0].shape[3]), int(dys[0].shape[3])
    if y_relus is not None and any(y is not None and int(y.shape[3]) != cout for y in y_relus):
        raise ValueError('%s: y_relus must have the shapes of dys' % who)
    if cin % 32 or cout % 64:
        raise ValueError('%s: cin %d must be a multiple of 32, cout %d a multiple of 64' % (who, cin, cout))
    _grad_on_gpu(who, every)
    lv = (L.OdetConvGradLevel * n)()
    for i in range(n):
        y = y_relus[i] if y_relus is not None else None
        lv[i].x, lv[i].dy, lv[i].y_relu = xs[i].data_ptr(), dys[i].data_ptr(), (y.data_ptr() if y is not None else None)
        lv[i].H, lv[i].W = int(xs[i].shape[1]), int(xs[i].shape[2])
    dev = xs[0].device
    dw = _out(out, (cout, 3, 3, cin), torch.float32, dev)
    db = torch.empty((cout,), dtype=torch.float32, device=dev) if with_bias else None
    entry, query = _grad_symbols(('odet_conv3x3_wgrad_f32_levels', 'odet_conv3x3_wgrad_workspace_bytes'),
                                 ('odet_conv3x3_wgrad_x3_levels', 'odet_conv3x3_wgrad_x3_workspace_bytes'))
    wsp, wsn = _grad_workspace(query, (lv, n, B, cin, cout), dev)
    L.call(entry, lv, n, L.dptr(dw), L.dptr(db), B, cin, cout, wsp, wsn, L.stream())
    return dw, db


def conv3x3_flipped_weight(weight):
    """w'[ci][ky][kx][co] = w[co][2-ky][2-kx][ci]: the weight whose FORWARD convolution is `weight`'s input gradient, as a
    contiguous [cin,3,3,cout] tensor (weight: [cout,cin,3,3] channels_last or contiguous, or [cout,3,3,cin])"""
    if weight.dim() != 4 or weight.dtype != torch.float32:
        raise ValueError('conv3x3_flipped_weight: weight must be float32 [cout,cin,3,3] or [cout,3,3,cin]')
    w = _conv3x3_weight_nhwc(weight, 'conv3x3_flipped_weight')
    with torch.no_grad():
        return w.flip(1, 2).permute(3, 1, 2, 0).contiguous()


def conv3x3_dgrad_f32_levels(dzs, weight, outs=None, flipped=None):
    """The input gradient of conv3x3_f32_levels: dx[b,y,x,ci] = sum over taps and co of dz[b,y-ky+1,x-kx+1,co] * w[co][ky][kx][ci] --
    the FORWARD kernel on dz (cin and cout exchanged) with the flipped, transposed weight (conv3x3_flipped_weight; `flipped`: a
    caller's cached one), no kernel of its own.  dzs [B,H,W,cout] per level must already be gated by the layer's ReLU.  The
    forward's rules with the roles exchanged: cout % 32 == 0, cin % 64 == 0."""
    who = 'conv3x3_dgrad_f32_levels'
    _, _, every = _conv_grad_maps(who, [('dzs', dzs)])
    if not isinstance(weight, torch.Tensor) or weight.dtype != torch.float32 or weight.dim() != 4:
        raise ValueError('%s: weight must be a float32 [cout,cin,3,3] or [cout,3,3,cin] tensor' % who)
    cout = int(dzs[0].shape[3])
    cin = weight.numel() // (9 * cout) if cout else 0
    if int(weight.shape[0]) != cout or cout % 32 or cin % 64 or cin < 64:
        raise ValueError('%s: cout %d must be a multiple of 32 (the weight has %d output channels), cin %d a multiple of 64'
                         % (who, cout, int(weight.shape[0]), cin))
    _grad_on_gpu(who, every + [('weight', weight)])
    wf = conv3x3_flipped_weight(weight) if flipped is None else flipped
    if tuple(wf.shape) != (cin, 3, 3, cout) or not wf.is_contiguous():
        raise ValueError('%s: flipped must be a contiguous [cin,3,3,cout] tensor' % who)
    if current_grad_form() == 'x3':                     # (the flipped tensor's limb planes: derived.py's, keyed on it)
        with f32_form('x3'):
            return _conv3x3_levels(torch.float32, list(dzs), wf, None, False, outs)
    return _conv3x3_levels(torch.float32, list(dzs), wf, None, False, outs)


@carries_grad_form
class _Conv3x3Trainable(torch.autograd.Function):
    """ops.conv3x3_f32_levels forward; one odet_conv3x3_wgrad_f32_levels over all levels (and, only when an input needs a gradient,
    the forward kernel on the flipped weight) backward"""

    @staticmethod
    def forward(ctx, weight, bias, relu, *xs):
        ys = conv3x3_f32_levels(list(xs), weight, bias, relu)
        ctx.relu, ctx.has_bias, ctx.n = bool(relu), bias is not None, len(xs)
        ctx.flipped = None                                   # (conv3x3_trainable_levels hangs a caller's cached one on the node)
        ctx.save_for_backward(weight, *xs, *(ys if relu else ()))
        return tuple(ys)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *dys):
        weight, xs = ctx.saved_tensors[0], list(ctx.saved_tensors[1:1 + ctx.n])
        ys = list(ctx.saved_tensors[1 + ctx.n:]) if ctx.relu else None
        dys = [d.contiguous() for d in dys]
        dw = db = None
        dxs = [None] * ctx.n
        need_b = ctx.has_bias and ctx.needs_input_grad[1]
        if ctx.needs_input_grad[0] or need_b:
            dw, db = conv3x3_wgrad_f32_levels(xs, dys, ys, with_bias=need_b)
            dw = _conv3x3_weight_grad(dw, weight) if ctx.needs_input_grad[0] else None
        if any(ctx.needs_input_grad[3:]):
            dzs = dys if ys is None else [torch.where(y > 0, d, torch.zeros_like(d)) for y, d in zip(ys, dys)]
            got = conv3x3_dgrad_f32_levels(dzs, weight, flipped=ctx.flipped)
            dxs = [g if need else None for g, need in zip(got, ctx.needs_input_grad[3:])]
        return (dw, db, None) + tuple(dxs)


def _conv3x3_weight_nhwc(weight, who):
    """the [cout,3,3,cin] view of a [cout,cin,3,3] or [cout,3,3,cin] weight; a [cout,3,3,3] one reads either way and is refused"""
    a, b = tuple(weight.shape[1:3]) == (3, 3), tuple(weight.shape[2:]) == (3, 3)
    if a == b:
        raise ValueError('%s: weight %s is not [cout,cin,3,3] or [cout,3,3,cin] (or, with 3 channels, reads as both)'
                         % (who, tuple(weight.shape)))
    return weight if a else weight.permute(0, 2, 3, 1)


def _conv3x3_weight_grad(dw, weight):
    """the kernel's dw [cout,3,3,cin] in the parameter's own shape and memory format (what training.train_step takes as it is): a
    [cout,cin,3,3] parameter gets the permuted view -- channels_last memory, the same bytes -- or, when it is contiguous in the
    plain format, a contiguous copy"""
    if tuple(weight.shape[1:3]) == (3, 3):                # an explicit [cout,3,3,cin] parameter (cin % 32 == 0: never 3)
        return dw
    g = dw.permute(0, 3, 1, 2)
    if weight.is_contiguous(memory_format=torch.channels_last):
        return g
    return g.contiguous()


def conv3x3_trainable_levels(xs, weight, bias, relu=False, flipped=None):
    """ops.conv3x3_f32_levels with a backward pass (float32, f32_form 'exact'): the forward is conv3x3_f32_levels, bit for bit;
    `.backward()` leaves weight.grad in the parameter's own shape and memory format and bias.grad [cout], from ONE wgrad launch
    over all levels (plus its reduce and bias launches), and computes input gradients only when a map requires one (``flipped``: a
    caller's cached conv3x3_flipped_weight for them; without it the backward pass flips the weight itself)."""
    _grad_f32('conv3x3_trainable_levels', 'convolution backward',
              [('weight', weight)] + [('xs[%d]' % i, x) for i, x in enumerate(xs)])
    ys = list(_Conv3x3Trainable.apply(weight, bias, bool(relu), *[x.contiguous() for x in xs]))
    if flipped is not None and ys[0].grad_fn is not None:
        ys[0].grad_fn.flipped = flipped                      # (the node IS the ctx that backward receives)
    return ys


@carries_grad_form
class _Conv3x3ReluPoolTrainable(torch.autograd.Function):
    """conv3x3_f32 without its epilogue, then bias_relu_maxpool (2x2 / 2, ceil mode) forward; relu_maxpool2_backward, then one
    odet_conv3x3_wgrad_f32_levels on the gated gradient (and, only when the input needs a gradient, the forward kernel on the
    flipped weight) backward"""

    @staticmethod
    def forward(ctx, x, weight, bias, flipped):
        z = conv3x3_f32(x, weight)
        ctx.save_for_backward(x, z, bias, weight, flipped)
        return bias_relu_maxpool(z, bias, 2, 2, 0, True)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dpool):
        x, z, bias, weight, flipped = ctx.saved_tensors
        dz = relu_maxpool2_backward(z, bias, dpool.contiguous())
        dx = dw = db = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dw, db = conv3x3_wgrad_f32_levels([x], [dz], with_bias=ctx.needs_input_grad[2])      # (dz is gated: no y_relus)
            dw = _conv3x3_weight_grad(dw, weight) if ctx.needs_input_grad[1] else None
        if ctx.needs_input_grad[0]:
            dx = conv3x3_dgrad_f32_levels([dz], weight, flipped=flipped)[0]
        return dx, dw, db, None


def conv3x3_relu_pool_trainable(x, weight, bias, flipped=None):
    """max_pool(relu(conv3x3(x) + bias)) with MaxPooling2D((2,2), 2, 'same') and a backward pass (float32, f32_form 'exact';
    vgg16_faster_rcnn.py:300-325: a stage's last convolution and its pooling): the forward is conv3x3_f32 without its epilogue, then
    bias_relu_maxpool -- the detectors' float32 launches, bit for bit; `.backward()` leaves weight.grad in the parameter's own
    shape and memory format and bias.grad [cout], and computes the input gradient only when ``x`` requires one (``flipped``: a
    caller's cached conv3x3_flipped_weight).  ``x`` [B,H,W,cin] contiguous NHWC -> [B,ceil(H/2),ceil(W/2),cout]."""
    who = 'conv3x3_relu_pool_trainable'
    _grad_operands(who, 'convolution backward', [('x', x), ('bias', bias)])
    _grad_f32(who, 'convolution backward', [('weight', weight)])                    # (channels_last or contiguous: _conv3x3_weight)
    if x.dim() != 4 or weight.dim() != 4:
        raise ValueError('%s: x must be an NHWC tensor [B,H,W,cin] and weight [cout,cin,3,3] or [cout,3,3,cin]' % who)
    cin, cout = int(x.shape[3]), int(weight.shape[0])
    if cin % 32 or cout % 64 or weight.numel() != cout * 9 * cin or tuple(bias.shape) != (cout,):
        raise ValueError('%s: cin %d must be a multiple of 32 and cout %d one of 64, weight %s and bias %s must go with them'
                         % (who, cin, cout, tuple(weight.shape), tuple(bias.shape)))
    _grad_on_gpu(who, [('x', x), ('weight', weight), ('bias', bias)])
    return _Conv3x3ReluPoolTrainable.apply(x, weight, bias, flipped)


def rpn_unpack_pair(d_scores, d_deltas, num_anchors, pixels, anchor_offset, out):
    """The inverse of rpn_pack_pair's index map (odet_rpn_unpack_pair): from ``d_scores`` [B,N,2] and ``d_deltas`` [B,N,4] the
    gradient ``out`` [B * pixels, 64 k] of one level's PADDED pair output (2A score columns, 4A delta columns, then zeros), the
    level starting at anchor ``anchor_offset``."""
    A, B = int(num_anchors), int(d_scores.shape[0])
    for t, k in ((d_scores, 2), (d_deltas, 4)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 3 or t.shape[0] != B or t.shape[2] != k:
            raise ValueError('d_scores / d_deltas must be contiguous float32 [B, N, 2] / [B, N, 4] tensors')
    if out.dtype != torch.float32 or out.dim() != 2 or not out.is_contiguous() or out.shape[0] != B * int(pixels) \
            or out.shape[1] < 6 * A:
        raise ValueError('out must be a contiguous float32 [B * pixels, >= 6A] tensor')
    if not (d_scores.is_cuda and d_deltas.is_cuda and out.is_cuda):
        raise ValueError('rpn_unpack_pair: d_scores, d_deltas and out must be GPU tensors')
    L.call('odet_rpn_unpack_pair', L.dptr(d_scores), d_scores.numel() // max(B, 1), int(anchor_offset) * 2, L.dptr(d_deltas),
           d_deltas.numel() // max(B, 1), int(anchor_offset) * 4, int(pixels), A, B, int(out.shape[1]), L.dptr(out), L.stream())
    return out


def lateral_merge(x, weight, bias, top, out=None):
    """The FPN neck's lateral 1x1 convolution with the top-down merge in its epilogue (odet_lateral_merge_f16 / _f32;
    resnet_fpn.py:385-398): 0.5 * resize_bilinear(top) + 0.5 * (x . w^T + bias); ``x`` [B,H,W,cin], ``top`` [B,h,w,cout]
    NHWC contiguous, float16 or float32."""
    w, cin, cout, sfx = _pw_args(x, weight, bias, 'lateral_merge')
    B, H, W = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
    if top.dtype != x.dtype or not top.is_cuda or not top.is_contiguous() or top.dim() != 4 \
            or top.shape[0] != B or top.shape[3] != cout:
        raise ValueError('top must be a contiguous GPU tensor [batch, h, w, cout] of x\'s dtype')
    shape = (B, H, W, cout)
    out = _out(out, shape, x.dtype, x.device)
    ws, sym, wp, extra = _f32_sym('odet_lateral_merge_%s', w, weight) if sfx == 'f32' \
        else (None, 'odet_lateral_merge_f16', L.dptr(w), ())
    _f32_call(ws, sym, L.dptr(x), wp, L.dptr(bias) if bias is not None else None, L.dptr(top),
           int(top.shape[1]), int(top.shape[2]), L.dptr(out), B, H, W, cin, cout, *extra, L.stream())
    return out


def pointwise_dual(x1, x2, weight, bias=None, stride=1, relu=True, out=None):
    """relu?([x1 | x2[:, ::stride, ::stride]] . weight^T + bias) in one contraction (odet_pointwise_dual_f16 / _f32): the
    last 1x1 convolution of a stage's first bottleneck together with its convolutional shortcut.  ``x1`` [B,Ho,Wo,cin1],
    ``x2`` [B,H,W,cin2] NHWC contiguous of one dtype, ``weight`` [cout, cin1 + cin2] contiguous."""
    if x1.dtype != x2.dtype or x1.dtype not in _PW_FORMS:
        raise ValueError('pointwise_dual: x1 and x2 must both be float16 or float32')
    sfx, name, gran = _PW_FORMS[x1.dtype]
    for t, nm in ((x1, 'x1'), (x2, 'x2')):
        if not t.is_cuda or not t.is_contiguous() or t.dim() != 4:
            raise ValueError('pointwise_dual: %s must be a contiguous GPU tensor [batch, H, W, C]' % nm)
    B, H, W, c2 = (int(v) for v in x2.shape)
    stride = int(stride)
    Ho, Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
    c1 = int(x1.shape[3])
    if tuple(x1.shape[:3]) != (B, Ho, Wo):
        raise ValueError('pointwise_dual: x1 %s does not match the strided x2 map (%d, %d, %d)' % (tuple(x1.shape), B, Ho, Wo))
    cout = int(weight.shape[0])
    if weight.dtype != x1.dtype or tuple(weight.shape) != (cout, c1 + c2) or not weight.is_contiguous():
        raise ValueError('pointwise_dual: weight must be a contiguous %s [cout, cin1 + cin2] tensor' % name)
    if bias is not None and (bias.dtype != x1.dtype or bias.numel() != cout or not bias.is_contiguous()):
        raise ValueError('pointwise_dual: bias must be a contiguous %s [cout] tensor' % name)
    if c1 % gran or c2 % gran or cout % 64:
        raise ValueError('pointwise_dual: cin1 / cin2 must be multiples of %d, cout of 64' % gran)
    shape = (B, Ho, Wo, cout)
    out = _out(out, shape, x1.dtype, x1.device)
    ws, sym, wp, extra = _f32_sym('odet_pointwise_dual_%s', weight) if sfx == 'f32' \
        else (None, 'odet_pointwise_dual_f16', L.dptr(weight), ())
    _f32_call(ws, sym, L.dptr(x1), c1, L.dptr(x2), c2, H, W, stride, wp,
           L.dptr(bias) if bias is not None else None, L.dptr(out), B, cout, 1 if relu else 0, *extra, L.stream())
    return out


# (the float16 names the round-3 callers and tests use)
pointwise_f16, dense_f16, lateral_merge_f16, pointwise_dual_f16 = pointwise, dense, lateral_merge, pointwise_dual


def stem_patches_f32(images_nhwc):
    """The stem's patch matrix for the float32 mode (odet_stem_patches_f32): NHWC float32 [B,H,W,3] -> [B, Ho, Wo, 160] with
    row = the zero-padded 7 x 7 x 3 window of conv1_pad + the 7x7 / 2 'valid' convolution in (dy, dx, channel) order,
    Ho = (H - 1) // 2 + 1.  The convolution is then `pointwise` on it (weights [64, 160] in the same order)."""
    x = images_nhwc
    if x.dtype != torch.float32 or not x.is_cuda or not x.is_contiguous() or x.dim() != 4 or x.shape[3] != 3:
        raise ValueError('stem_patches_f32: images must be a contiguous float32 GPU tensor [B, H, W, 3]')
    B, H, W = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
    out = torch.empty((B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 160), dtype=torch.float32, device=x.device)
    L.call('odet_stem_patches_f32', L.dptr(x), L.dptr(out), B, H, W, L.stream())
    return out


# the float32 mode's patch matrices (stem, VGG16's first convolution) are addressed with 32-bit byte offsets
PATCH_BYTES_MAX = 0xF0000000
STEM_PATCH_K = 160                # floats per row of the stem's patch matrix: 7 x 7 x 3 = 147 used


def patch_weight(weight, kpad):
    """a [cout, cin, kh, kw] convolution weight as the patch-matrix GEMM's float32 [cout, kpad]: rows in (dy, dx, channel) order,
    zero columns from kh * kw * cin on"""
    with torch.no_grad():
        cout = int(weight.shape[0])
        k = weight.numel() // cout
        w = torch.zeros((cout, kpad), dtype=torch.float32, device=weight.device)
        w[:, :k] = weight.permute(0, 2, 3, 1).reshape(cout, k)
    return w


@carries_grad_form
class _StemTrainable(torch.autograd.Function):
    """stem_patches_f32, pointwise, bias_relu_maxpool (3x3 / 2, pad 1) forward -- the float32 stem's launches; backward:
    relu_maxpool3_backward on the saved raw convolution output, the patch matrix built again, then ONE dense_wgrad over the
    pixels.  The image gets no gradient."""

    @staticmethod
    def forward(ctx, images, weight, bias, stem_weight):
        z = pointwise(stem_patches_f32(images), stem_weight, None, None, False)
        ctx.save_for_backward(images, z, weight, bias)
        return bias_relu_maxpool(z, bias, 3, 2, 1, False)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dpool):
        images, z, weight, bias = ctx.saved_tensors
        dw = db = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dz = relu_maxpool3_backward(z, bias, dpool.contiguous())
            patches = stem_patches_f32(images)                            # (171 MB at 800 x 1333: built again, never saved)
            dw, db = dense_wgrad(dz.view(-1, 64), patches.view(-1, STEM_PATCH_K), with_bias=ctx.needs_input_grad[2])
            if ctx.needs_input_grad[1]:
                # [64, 147] in (dy, dx, channel) order -> the parameter's [64, 3, 7, 7], in its own memory format
                dw = dw[:, :147].reshape(64, 7, 7, 3).permute(0, 3, 1, 2)
                if not weight.is_contiguous(memory_format=torch.channels_last):
                    dw = dw.contiguous()
            else:
                dw = None
        return None, dw, db, None


def stem_trainable(images_nhwc, weight, bias, stem_weight=None):
    """The float32 ResNet stem -- conv1_pad + 7x7 / 2 convolution + bias + ReLU + pool1_pad + 3x3 / 2 max-pooling
    (resnet_fpn.py:233-242) -- with a backward pass into conv1's weight and bias (float32, f32_form 'exact'): the forward is the
    launches of the detectors' float32 stem (stem_patches_f32, pointwise, bias_relu_maxpool), bit for bit; `.backward()` leaves
    weight.grad in the parameter's own shape [64,3,7,7] and memory format and bias.grad [64].  The forward keeps the raw convolution
    output (which it writes anyway) and not the patch matrix; the backward builds that again.  ``images_nhwc`` [B,H,W,3] contiguous
    float32 on the GPU, whose patch matrix stays below PATCH_BYTES_MAX (one group: training runs one image a call); the image gets
    no gradient.  ``stem_weight``: a caller's cached patch_weight(weight, STEM_PATCH_K).  -> NHWC [B,Hp,Wp,64]."""
    who = 'stem_trainable'
    _grad_operands(who, 'stem backward', [('images', images_nhwc), ('bias', bias)])
    _grad_f32(who, 'stem backward', [('weight', weight)])                         # (channels_last or contiguous)
    if images_nhwc.dim() != 4 or int(images_nhwc.shape[3]) != 3 or min(int(v) for v in images_nhwc.shape[:3]) < 1:
        raise ValueError('%s: images %s must be an NHWC tensor [B,H,W,3] with a positive size' % (who, tuple(images_nhwc.shape)))
    if tuple(weight.shape) != (64, 3, 7, 7) or tuple(bias.shape) != (64,):
        raise ValueError('%s: weight %s and bias %s must be [64,3,7,7] and [64]' % (who, tuple(weight.shape), tuple(bias.shape)))
    B, H, W = (int(v) for v in images_nhwc.shape[:3])
    patch_bytes = B * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1) * STEM_PATCH_K * 4
    if patch_bytes > PATCH_BYTES_MAX:
        raise ValueError('%s: the patch matrix of images %s takes %d bytes, more than one group of %d (train one image a call)'
                         % (who, tuple(images_nhwc.shape), patch_bytes, PATCH_BYTES_MAX))
    if stem_weight is None:
        stem_weight = patch_weight(weight, STEM_PATCH_K)
    elif not isinstance(stem_weight, torch.Tensor) or stem_weight.dtype != torch.float32 \
            or tuple(stem_weight.shape) != (64, STEM_PATCH_K) or not stem_weight.is_contiguous():
        raise ValueError('%s: stem_weight must be a contiguous float32 [64, %d] tensor' % (who, STEM_PATCH_K))
    _grad_on_gpu(who, [('images', images_nhwc), ('weight', weight), ('bias', bias), ('stem_weight', stem_weight)])
    return _StemTrainable.apply(images_nhwc, weight, bias, stem_weight)


def rgb_patches3x3_f32(images_nhwc):
    """The patch matrix of a 3x3 'same' convolution on a 3-channel image for the float32 mode (odet_rgb_patches3x3_f32): NHWC
    float32 [B,H,W,3] -> [B,H,W,64], row = the zero-padded 3 x 3 x 3 window in (dy, dx, channel) order + zeros.  The
    convolution is then `pointwise` on it (weights [cout, 64] in the same order)."""
    x = images_nhwc
    if x.dtype != torch.float32 or not x.is_cuda or not x.is_contiguous() or x.dim() != 4 or x.shape[3] != 3:
        raise ValueError('rgb_patches3x3_f32: images must be a contiguous float32 GPU tensor [B, H, W, 3]')
    B, H, W = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
    out = torch.empty((B, H, W, 64), dtype=torch.float32, device=x.device)
    L.call('odet_rgb_patches3x3_f32', L.dptr(x), L.dptr(out), B, H, W, L.stream())
    return out


def dense_f16_out_f32(x, weight, bias=None, relu=False, out=None):
    """The last dense layer with float32 results (odet_dense_f16_out_f32): ``x`` [rows, cin] / ``weight`` [cout, cin]
    float16 contiguous, ``bias`` [cout] float32 -> float32 [rows, cout]; cout % 64 == 0 (pad the weight rows with zeros)."""
    if x.dtype != torch.float16 or not x.is_cuda or not x.is_contiguous() or x.dim() != 2:
        raise ValueError('dense_f16_out_f32: x must be a contiguous float16 GPU tensor [rows, cin]')
    w, cin, cout, _ = _pw_args(x.view(1, 1, x.shape[0], x.shape[1]), weight, None, 'dense_f16_out_f32')
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() != cout or not bias.is_contiguous()):
        raise ValueError('dense_f16_out_f32: bias must be a contiguous float32 [cout] tensor')
    rows = int(x.shape[0])
    out = _out(out, (rows, cout), torch.float32, x.device)
    L.call('odet_dense_f16_out_f32', L.dptr(x), L.dptr(w), L.dptr(bias) if bias is not None else None, L.dptr(out), rows,
           cin, cout, 1 if relu else 0, L.stream())
    return out


def rpn_pack_pair(level_out, bias, num_anchors, scores, deltas, anchor_offset):
    """rpn_pack for the RpnHead's two 1x1 convolutions run as one contraction: ``level_out`` [B,h,w,6A] (2A score
    channels then 4A delta channels, no bias), ``bias`` [6A]; writes the level's slices of ``scores`` [B,N,2] and
    ``deltas`` [B,N,4] (float32) starting at anchor ``anchor_offset``."""
    if level_out.dim() != 4 or not level_out.is_contiguous():
        raise ValueError('level_out must be a contiguous NHWC [B,h,w,6A] tensor')
    if level_out.dtype not in (torch.float32, torch.float16) or bias.dtype != level_out.dtype:
        raise TypeError('level_out and bias must both be float32 or both float16')
    B, h, w, ch = (int(v) for v in level_out.shape)
    A = int(num_anchors)
    if ch != 6 * A or bias.numel() != ch:
        raise ValueError('level_out / bias must have 6 * num_anchors channels')
    for t, k in ((scores, 2), (deltas, 4)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 3 or t.shape[0] != B or t.shape[2] != k:
            raise ValueError('scores / deltas must be contiguous float32 [B, N, 2] / [B, N, 4] tensors')
    L.call('odet_rpn_pack_pair', L.dptr(level_out), L.dptr(bias), h * w, A, B, L.dptr(scores),
           scores.numel() // max(B, 1), int(anchor_offset) * 2, L.dptr(deltas), deltas.numel() // max(B, 1),
           int(anchor_offset) * 4, 1 if level_out.dtype == torch.float16 else 0, L.stream())
    return scores, deltas


class ProfEvent:
    """HIP event for odet_roi_pool_timed (the dispatch's own begin / end timestamps)."""

    def __init__(self):
        self.handle = C.c_void_p()
        L.check(L.lib().odet_prof_event_create(C.byref(self.handle)))

    def elapsed_ms(self, stop):
        ms = C.c_float()
        L.check(L.lib().odet_prof_event_elapsed_ms(self.handle, stop.handle, C.byref(ms)))
        return float(ms.value)

    def __del__(self):
        try:
            if self.handle:
                L.lib().odet_prof_event_destroy(self.handle)
        except Exception:
            pass


def roi_order(rois, roi_level, image_shape, count_dev=None, out=None):
    """Spatial processing order (int32 [n]) of the RoIs for roi_pool(order=...): sorted by (level, column strip of 1/8 of the
    image by the box centre's x, bin of 1/32 of the image by its y -- downwards on even strips, upwards on odd ones --, then
    y, x, row); rows >= count_dev[0] follow in row order.  The proposal stage writes the same bucket sequence itself up to
    FUSED_ORDER_MAX_ROIS proposals (arbitrary order inside a bucket there)."""
    rois = _boxes(rois, 'rois')
    n = rois.shape[0]
    if out is None:
        out = torch.empty(max(n, 1), dtype=torch.int32, device=rois.device)
    if roi_level is not None and roi_level.dtype != torch.int32:
        roi_level = roi_level.to(torch.int32)
    L.call('odet_roi_order', L.dptr(rois), L.dptr(roi_level), n, L.dptr(count_dev), int(image_shape[0]),
           int(image_shape[1]), L.dptr(out), L.stream())
    return out


ROI_GRAD_MAX_ROIS = 8192       # odet_roi_pool_argmax / odet_roi_pool_backward: ODET_E_LIMIT above
ROI_GRAD_MAX_POOL = 16
ROI_IMAGES_MAX_BATCH = 64      # ODET_E_LIMIT above (TARGETS_MAX_BATCH: what one targets call produces)

# The two forms of every RoI operation.  One image: maps / dx [1,H,W,C] per level, rois [n,4], roi_level int32 [n], count_dev
# int32 [1], features / dy / sel [n,P,P,C].  A batch of images (odet_roi_pool_*_images), dense and strided, what the batched targets
# and dense parts hand over: the same with a leading B; the images share the level shapes, n, P and the modes, and image b's results
# are the single-image functions' on image b alone, bit for bit; float32 only.  A form names its three C symbols (a function's
# `who` in error texts is its symbol without 'odet_'); everything else that differs hangs on `batched`.
_RoiForm = collections.namedtuple('_RoiForm', 'batched pool argmax backward')
_ROI_ONE = _RoiForm(False, 'odet_roi_pool', 'odet_roi_pool_argmax', 'odet_roi_pool_backward')
_ROI_IMAGES = _RoiForm(True, 'odet_roi_pool_images', 'odet_roi_pool_argmax_images', 'odet_roi_pool_backward_images')


def _roi_image_shape(image_shape):
    return (0, 0) if image_shape is None else (int(image_shape[0]), int(image_shape[1]))


def _roi_f32(who, what, tensors, strict=False):
    """the float32 rule of the gradient forms, asked before anything needs a device; shapes pass unless `strict`"""
    for t in tensors:
        if getattr(t, 'dtype', None if strict else torch.float32) != torch.float32:
            raise ValueError('%s: %s must be float32 tensors (the RoI backward has no float16 form), got %s'
                             % (who, what, getattr(t, 'dtype', type(t).__name__)))


def _roi_rois(form, who, rois, roi_level, pool_size):
    """the RoI front -> (float32 rois [n,4] or [B,n,4], roi_level int32 of the leading shape or None, the leading shape (n,) or
    (B, n), P)"""
    if form.batched:
        rois = L.f32c(rois, 'rois')
        if rois.dim() != 3 or rois.shape[2] != 4:
            raise ValueError('%s: rois must have shape [B,n,4], got %s' % (who, tuple(rois.shape)))
    else:
        rois = _boxes(rois, 'rois')
    lead = tuple(rois.shape[:-1])
    if roi_level is not None:
        if roi_level.dtype != torch.int32:
            roi_level = roi_level.to(torch.int32)
        if form.batched and tuple(roi_level.shape) != lead:
            raise L.OdetError('%s: roi_level must have shape [B,n] = %s, got %s' % (who, lead, tuple(roi_level.shape)))
    return rois, roi_level, lead, int(pool_size)


def _roi_levels(who, maps_or_shapes, strides, device=None, alloc=False, batch=1, forward=False):
    """the level table of every RoI call -> (levels, tensors, C).  `maps_or_shapes` = NHWC GPU tensors [batch,H,W,C], one per
    level.  The gradient forms take contiguous float32 tensors (the maps, or dx buffers to write; _roi_f32 has been asked) or,
    with `alloc`, shapes: buffers are made on `device`.  `forward`: float16 maps stay when every map is float16, anything else is
    cast (L.f32c)."""
    nl = len(maps_or_shapes)
    if nl < 1 or nl > MAX_LEVELS:
        raise ValueError('%s: between 1 and %d feature maps expected' % (who, MAX_LEVELS))
    levels = (L.OdetLevel * nl)()
    keep, Cc = [], None
    f16 = forward and all(isinstance(fm, torch.Tensor) and fm.dtype == torch.float16 for fm in maps_or_shapes)
    for i, fm in enumerate(maps_or_shapes):
        if f16 and fm.is_cuda:
            fm = fm.contiguous()
        elif forward:                                                    # (a float16 map on the CPU is refused here as well)
            fm = L.f32c(fm, 'shared_layers')
        elif not isinstance(fm, torch.Tensor):
            if not alloc:
                raise TypeError('%s: feature maps must be tensors' % who)
            fm = torch.empty(tuple(int(v) for v in fm), dtype=torch.float32, device=device)
        shape = tuple(fm.shape)
        if len(shape) != 4 or (batch == 1 and shape[0] != 1):
            raise ValueError('%s: feature map must be NHWC with batch 1, got %s' % (who, shape))
        if shape[0] != batch:
            raise L.OdetError('%s: the maps, the RoIs and dy of a call must share the batch size (%d), got a map of shape %s'
                              % (who, batch, shape))
        if not fm.is_cuda:
            raise L.OdetError('%s: shared_layers must live on the GPU: tf_eager_object_detection_amd has no CPU path' % who)
        if not fm.is_contiguous():
            raise ValueError('%s: feature maps must be contiguous' % who)
        if Cc is None:
            Cc = shape[3]
        elif shape[3] != Cc:
            raise ValueError('%s: all levels must share the channel count' % who)
        keep.append(fm)
        lv = levels[i]
        lv.data, lv.H, lv.W, lv.stride = fm.data_ptr(), shape[1], shape[2], float(strides[i]) if strides is not None else 0.0
    return levels, keep, Cc


def _roi_images_count(who, count_dev, B):
    if count_dev is not None and (count_dev.dtype != torch.int32 or count_dev.numel() != B):
        raise L.OdetError('%s: count_dev must be int32 [B] = [%d], got %s %s' % (who, B, count_dev.dtype, tuple(count_dev.shape)))


def _roi_rows(who, t, name, dtype, shape):
    """dy or sel: a contiguous `dtype` tensor of `shape` = [n,P,P,C] or [B,n,P,P,C]"""
    if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
        if t.dim() == 5 and tuple(t.shape[1:]) == shape[1:] and t.shape[0] != shape[0]:
            raise L.OdetError('%s: the maps, the RoIs and dy of a call must share the batch size (%d), got %s of shape %s'
                              % (who, shape[0], name, tuple(t.shape)))
        raise ValueError('%s: %s must be contiguous %s %s = %s, got %s %s'
                         % (who, name, dtype, '[B,n,P,P,C]' if len(shape) == 5 else '[n,P,P,C]', shape, t.dtype, tuple(t.shape)))


def roi_pool(feature_maps, rois, roi_level, norm_mode, pool_size, pool_mode, strides=None, image_shape=None,
             count_dev=None, out=None, events=None, order=None):
    """feature_maps: list of NHWC float32 GPU tensors [1,H,W,C] (one per level).  ``events`` = (start, stop)
    ProfEvent pair attached to the dispatch (profiling); ``order`` = int32 processing order (roi_order)."""
    rois, roi_level, (n,), P = _roi_rois(_ROI_ONE, 'roi_pool', rois, roi_level, pool_size)
    levels, keep, Cc = _roi_levels('roi_pool', feature_maps, strides, forward=True)
    f16 = keep[0].dtype == torch.float16
    if out is None:
        out = torch.empty((n, P, P, Cc), dtype=keep[0].dtype, device=rois.device)
    elif f16 and out.dtype != torch.float16:
        raise TypeError('out must be float16 for float16 feature maps')
    ih, iw = _roi_image_shape(image_shape)
    head = (levels, len(keep), Cc, L.dptr(rois), L.dptr(roi_level), n, L.dptr(count_dev))
    tail = (int(norm_mode), ih, iw, P, int(pool_mode), C.c_void_p(out.data_ptr()) if f16 else L.dptr(out), L.stream())
    timed = (events[0].handle, events[1].handle) if events else ()
    if f16 or order is not None:
        head += (L.dptr(order, torch.int32, 'order') if order is not None else None,)
    if f16:
        L.call('odet_roi_pool_f16_timed' if timed else 'odet_roi_pool_f16', *(head + tail + timed))
    elif order is not None:
        L.call('odet_roi_pool_ordered', *(head + tail + (timed or (None, None))))
    else:
        L.call('odet_roi_pool_timed' if timed else 'odet_roi_pool', *(head + tail + timed))
    return out


def _roi_pool_rows(form, pool_mode, select, feature_maps, rois, roi_level, norm_mode, pool_size, strides, image_shape, count_dev,
                   out=None, sel=None):
    """The launches of a form over float32 maps that fill rows, on one level table and one set of pointers -> (out, sel): the
    forward (`pool_mode` not None: form.pool, float32 rows into `out`) and / or the select (`select`: form.argmax, uint8 rows into
    `sel`), in this order."""
    who = (form.argmax if pool_mode is None else form.pool)[5:]
    _roi_f32(who, 'feature maps', feature_maps)
    rois, roi_level, lead, P = _roi_rois(form, who, rois, roi_level, pool_size)
    levels, keep, Cc = _roi_levels(who, list(feature_maps), strides, batch=lead[0] if form.batched else 1)
    if form.batched:
        _roi_images_count(who, count_dev, lead[0])
    ih, iw = _roi_image_shape(image_shape)
    args = (levels, len(keep), Cc) + lead[:-1] + (L.dptr(rois), L.dptr(roi_level), lead[-1], L.dptr(count_dev), int(norm_mode),
                                                   ih, iw, P)
    stream = L.stream()
    if pool_mode is not None:
        out = _out(out, lead + (P, P, Cc), torch.float32, rois.device)
        L.call(form.pool, *args, int(pool_mode), L.dptr(out), stream)
    if select:
        sel = _out(sel, lead + (P, P, Cc), torch.uint8, rois.device)
        L.call(form.argmax, *args, L.dptr(sel), stream)
    return out, sel


def roi_pool_argmax(feature_maps, rois, roi_level, norm_mode, pool_size, strides=None, image_shape=None, count_dev=None,
                    out=None):
    """Which sample of each 2x2 bin roi_pool(..., ROI_POOL_MAX2) took (odet_roi_pool_argmax): uint8 [n,P,P,C], 0..3 = 2*di+dj
    (the first sample equal to the pooled value), 4 = none.  float32 maps only."""
    return _roi_pool_rows(_ROI_ONE, None, True, feature_maps, rois, roi_level, norm_mode, pool_size, strides, image_shape, count_dev,
                          sel=out)[1]


def roi_pool_images(feature_maps, rois, roi_level, norm_mode, pool_size, pool_mode, strides=None, image_shape=None, count_dev=None,
                    out=None):
    """roi_pool over B images (odet_roi_pool_images): feature_maps = one float32 [B,H,W,C] GPU tensor per level, rois [B,n,4] ->
    [B,n,P,P,C]; ceil(B / 8) launches of the forward's own batched form, image b bit-equal to roi_pool on image b."""
    return _roi_pool_rows(_ROI_IMAGES, int(pool_mode), False, feature_maps, rois, roi_level, norm_mode, pool_size, strides,
                          image_shape, count_dev, out=out)[0]


def roi_pool_argmax_images(feature_maps, rois, roi_level, norm_mode, pool_size, strides=None, image_shape=None, count_dev=None,
                           out=None):
    """roi_pool_argmax over B images in one launch (odet_roi_pool_argmax_images): uint8 [B,n,P,P,C], rows at or beyond
    count_dev[b] 4."""
    return _roi_pool_rows(_ROI_IMAGES, None, True, feature_maps, rois, roi_level, norm_mode, pool_size, strides, image_shape,
                          count_dev, sel=out)[1]


def _roi_pool_backward(form, dy, feature_shapes_or_maps, rois, roi_level, norm_mode, pool_size, pool_mode, strides, image_shape,
                       count_dev, outs, sel):
    who = form.backward[5:]
    _roi_f32(who, 'dy', [dy], strict=True)
    _roi_f32(who, 'feature maps', feature_shapes_or_maps if outs is None else outs)
    if (int(pool_mode) == ROI_POOL_MAX2) != (sel is not None):
        raise ValueError('%s: sel (%s) is required for ROI_POOL_MAX2 and goes with no other pool_mode' % (who, form.argmax[5:]))
    rois, roi_level, lead, P = _roi_rois(form, who, rois, roi_level, pool_size)
    if outs is None:
        outs = [tuple(fm.shape) if isinstance(fm, torch.Tensor) else tuple(fm) for fm in feature_shapes_or_maps]
    levels, dxs, Cc = _roi_levels(who, list(outs), strides, rois.device, alloc=True, batch=lead[0] if form.batched else 1)
    if form.batched:
        _roi_images_count(who, count_dev, lead[0])
    rows = lead + (P, P, Cc)
    _roi_rows(who, dy, 'dy', torch.float32, rows)
    if sel is not None:
        _roi_rows(who, sel, 'sel', torch.uint8, rows)
    ih, iw = _roi_image_shape(image_shape)
    L.call(form.backward, levels, len(dxs), Cc, *lead[:-1], L.dptr(rois), L.dptr(roi_level), lead[-1], L.dptr(count_dev),
           int(norm_mode), ih, iw, P, int(pool_mode), L.dptr(dy), L.dptr(sel), L.stream())
    return dxs


def roi_pool_backward(dy, feature_shapes_or_maps, rois, roi_level, norm_mode, pool_size, pool_mode, strides=None,
                      image_shape=None, count_dev=None, outs=None, sel=None):
    """The gradient of roi_pool with respect to its float32 maps (odet_roi_pool_backward): dy [n,P,P,C] -> list of dx, one
    [1,H,W,C] float32 per level, every element written once in an order fixed by the data's indices (bit-reproducible).
    `feature_shapes_or_maps`: the maps (only their shapes are used) or their shapes; `sel`: roi_pool_argmax's output, required
    for ROI_POOL_MAX2 and refused otherwise; `outs`: buffers to write instead of new ones."""
    return _roi_pool_backward(_ROI_ONE, dy, feature_shapes_or_maps, rois, roi_level, norm_mode, pool_size, pool_mode, strides,
                              image_shape, count_dev, outs, sel)


def roi_pool_backward_images(dy, feature_shapes_or_maps, rois, roi_level, norm_mode, pool_size, pool_mode, strides=None,
                             image_shape=None, count_dev=None, outs=None, sel=None):
    """roi_pool_backward over B images in one launch (odet_roi_pool_backward_images): dy [B,n,P,P,C] -> list of dx, one
    [B,H,W,C] float32 per level, every element written once (zeros for an image without RoIs); a workgroup walks the RoIs of its
    own image only.  Arguments as roi_pool_backward, with the batched shapes."""
    return _roi_pool_backward(_ROI_IMAGES, dy, feature_shapes_or_maps, rois, roi_level, norm_mode, pool_size, pool_mode, strides,
                              image_shape, count_dev, outs, sel)


class _RoiPoolTrainable(torch.autograd.Function):
    """cfg[0] = the form.  The form's forward launch (over float32 maps form.pool is what roi_pool / roi_pool_images call) and,
    for ROI_POOL_MAX2, its select launch while the maps are warm, on one level table; one backward launch of the form.  Both go
    straight to the bodies behind the public functions, not through the names ops.roi_pool_argmax* / ops.roi_pool_backward*."""

    @staticmethod
    def forward(ctx, rois, roi_level, count_dev, cfg, *maps):
        form, norm_mode, pool_size, pool_mode, strides, image_shape = cfg
        out, sel = _roi_pool_rows(form, pool_mode, pool_mode == ROI_POOL_MAX2, maps, rois, roi_level, norm_mode, pool_size, strides,
                                  image_shape, count_dev)
        ctx.cfg = cfg
        ctx.shapes = [tuple(m.shape) for m in maps]
        ctx.save_for_backward(rois, roi_level, count_dev, sel)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        rois, roi_level, count_dev, sel = ctx.saved_tensors
        form, norm_mode, pool_size, pool_mode, strides, image_shape = ctx.cfg
        dxs = _roi_pool_backward(form, dy if dy.is_contiguous() else dy.contiguous(), ctx.shapes, rois, roi_level, norm_mode,
                                 pool_size, pool_mode, strides, image_shape, count_dev, None, sel)
        return (None, None, None, None) + tuple(dx if need else None for dx, need in zip(dxs, ctx.needs_input_grad[4:]))


def _roi_pool_trainable(form, feature_maps, rois, roi_level, norm_mode, pool_size, pool_mode, strides, image_shape, count_dev):
    who = 'roi_pool_trainable_images' if form.batched else 'roi_pool_trainable'
    _roi_f32(who, 'feature maps', feature_maps, strict=True)
    maps = [fm if fm.is_contiguous() else fm.contiguous() for fm in feature_maps]
    if form.batched:                                                     # (the limits come before anything asks for a device)
        if rois.dim() != 3 or rois.shape[2] != 4:
            raise ValueError('%s: rois must have shape [B,n,4], got %s' % (who, tuple(rois.shape)))
        if int(rois.shape[0]) > ROI_IMAGES_MAX_BATCH or int(rois.shape[1]) > ROI_GRAD_MAX_ROIS or int(pool_size) > ROI_GRAD_MAX_POOL:
            raise ValueError('%s: at most %d images, %d RoIs per image and pool_size %d'
                             % (who, ROI_IMAGES_MAX_BATCH, ROI_GRAD_MAX_ROIS, ROI_GRAD_MAX_POOL))
    elif int(rois.shape[0]) > ROI_GRAD_MAX_ROIS or int(pool_size) > ROI_GRAD_MAX_POOL:
        raise ValueError('%s: at most %d RoIs and pool_size %d' % (who, ROI_GRAD_MAX_ROIS, ROI_GRAD_MAX_POOL))
    cfg = (form, int(norm_mode), int(pool_size), int(pool_mode), None if strides is None else tuple(float(s) for s in strides),
           None if image_shape is None else _roi_image_shape(image_shape))
    return _RoiPoolTrainable.apply(rois.detach() if rois.requires_grad else rois, roi_level, count_dev, cfg, *maps)


def roi_pool_trainable(feature_maps, rois, roi_level, norm_mode, pool_size, pool_mode, strides=None, image_shape=None,
                       count_dev=None):
    """ops.roi_pool with a backward pass into the float32 maps: the forward is `roi_pool`, bit for bit; `.backward()` is one
    roi_pool_backward and leaves a gradient on every map that requires one (None for the others).  The RoIs get no gradient
    (the reference stops it: roi_pooling.py:78)."""
    return _roi_pool_trainable(_ROI_ONE, feature_maps, rois, roi_level, norm_mode, pool_size, pool_mode, strides, image_shape,
                               count_dev)


def roi_pool_trainable_images(feature_maps, rois, roi_level, norm_mode, pool_size, pool_mode, strides=None, image_shape=None,
                              count_dev=None):
    """roi_pool_images with a backward pass into the float32 maps: the forward is `roi_pool_images`, bit for bit; `.backward()` is
    one roi_pool_backward_images and leaves a gradient on every map that requires one (None for the others).  The RoIs get no
    gradient.  No host read anywhere: graph-capturable."""
    return _roi_pool_trainable(_ROI_IMAGES, feature_maps, rois, roi_level, norm_mode, pool_size, pool_mode, strides, image_shape,
                               count_dev)


def post_ops(scores, deltas, rois, image_shape, means, stds, max_per_class, max_per_image, nms_iou_threshold,
             score_threshold, min_edge, num_classes, count_dev=None, out=None, workspace=None, record=None):
    """-> (boxes [M,4], labels int32 [M], scores [M]) padded to max_per_image, count int32[1].
    ``out`` = preallocated (boxes, labels, scores, count); ``workspace`` = reusable uint8 buffer;
    ``record`` = float32 [max_per_image*6+1] GPU tensor that also receives the detection record."""
    scores = L.f32c(scores, 'roi_scores_softmax')
    if scores.dim() != 2:
        raise ValueError('roi_scores_softmax must be [num_rois, num_classes]')
    R, Ccls = scores.shape
    deltas = L.f32c(deltas, 'roi_txtytwth')
    if deltas.numel() != R * Ccls * 4:
        raise ValueError('roi_txtytwth must hold [num_rois, num_classes, 4] values')
    rois = _boxes(rois, 'rois')
    if rois.shape[0] != R:
        raise ValueError('rois has %d rows for %d score rows' % (rois.shape[0], R))
    M = max(int(max_per_image), 1)
    if out is not None:
        ob, ol, os_, cnt = out
    else:
        ob = torch.empty((M, 4), dtype=torch.float32, device=scores.device)
        ol = torch.empty(M, dtype=torch.int32, device=scores.device)
        os_ = torch.empty(M, dtype=torch.float32, device=scores.device)
        cnt = _count_tensor(scores.device)
    nb = L.lib().odet_post_ops_workspace_bytes(int(num_classes), int(max_per_class))
    ws = workspace if workspace is not None and workspace.numel() >= nb else L.workspace(nb, scores.device)
    head = (L.dptr(scores), L.dptr(deltas), L.dptr(rois), R, L.dptr(count_dev), Ccls, int(num_classes),
            int(image_shape[0]), int(image_shape[1]), L.host4(means, 'target_means'), L.host4(stds, 'target_stds'),
            int(max_per_class), int(max_per_image), float(nms_iou_threshold), float(score_threshold),
            float(min_edge), L.dptr(ob), L.dptr(ol), L.dptr(os_), L.dptr(cnt))
    if record is None:
        L.call('odet_post_ops', *head, L.dptr(ws), nb, L.stream())
    else:
        if record.numel() < M * 6 + 1:
            raise ValueError('record must hold max_per_image*6+1 floats')
        L.call('odet_post_ops_record', *head, L.dptr(record, torch.float32, 'record'), L.dptr(ws), nb, L.stream())
    return ob, ol, os_, cnt


# ---- fused training targets (csrc/targets.hip) ---------------------------------------------------------------------------------
TARGETS_MAX_GT = 1024
TARGETS_MAX_BATCH = 64

AnchorTargets = collections.namedtuple('AnchorTargets', [
    'labels', 'targets', 'inside', 'outside', 'sample_idx', 'sample_targets', 'counts', 'labels_before_sampling', 'argmax'])
ProposalTargets = collections.namedtuple('ProposalTargets', [
    'final_rois', 'final_labels', 'targets', 'inside', 'outside', 'keep', 'gt_assignment', 'counts'])


def _gt_offsets(gt_offsets, device):
    """device int32 [B+1] as it is (never read here); a host sequence is checked against the per-image limit and uploaded"""
    if isinstance(gt_offsets, torch.Tensor) and gt_offsets.is_cuda:
        if gt_offsets.dtype != torch.int32 or gt_offsets.dim() != 1 or gt_offsets.numel() < 2:
            raise TypeError('gt_offsets must be an int32 vector of batch + 1 entries')
        return gt_offsets.contiguous()
    off = [int(v) for v in gt_offsets]
    if len(off) < 2 or off[0] < 0 or any(b < a for a, b in zip(off, off[1:])):
        raise ValueError('gt_offsets must hold batch + 1 non-decreasing offsets')
    if max(b - a for a, b in zip(off, off[1:])) > TARGETS_MAX_GT:
        raise L.OdetError('more than %d ground-truth boxes in one image' % TARGETS_MAX_GT)
    return torch.tensor(off, dtype=torch.int32, device=device)


def anchor_targets(anchors, gt_boxes, gt_offsets, image_shape, pos_iou_threshold, neg_iou_threshold, total_num_samples,
                   max_pos_samples, means, stds, seed=0, first_image_id=0, dense=True, parity=False, workspace=None):
    """odet_anchor_target for the B = len(gt_offsets) - 1 images that share `anchors` [N,4]: -> AnchorTargets of
    labels [B,N], targets / inside / outside [B,N,4] (None with dense=False), sample_idx int32 [B,S], sample_targets [B,S,4],
    counts int32 [B,5], labels_before_sampling / argmax int32 [B,N] (None unless parity=True).  Nothing is read back."""
    anchors = _boxes(anchors, 'all_anchors')
    gt = _boxes(gt_boxes, 'gt_boxes')
    dev = anchors.device
    if gt.shape[0] == 0:                     # (no ground truth anywhere: the kernels still want a valid address)
        gt = gt.new_zeros((1, 4))
    off = _gt_offsets(gt_offsets, dev)
    B, N, S = off.numel() - 1, anchors.shape[0], int(total_num_samples)

    def new(shape, dtype=torch.float32):
        return torch.empty(shape, dtype=dtype, device=dev)
    labels, targets, inside, outside = (new((B, N)), new((B, N, 4)), new((B, N, 4)), new((B, N, 4))) if dense else (None,) * 4
    before, argmax = (new((B, N), torch.int32), new((B, N), torch.int32)) if parity else (None, None)
    sample_idx, sample_targets, counts = new((B, S), torch.int32), new((B, S, 4)), new((B, 5), torch.int32)
    nb = L.lib().odet_anchor_target_workspace_bytes(N, B, S)
    ws = workspace if workspace is not None and workspace.numel() >= nb else L.workspace(nb, dev)
    L.call('odet_anchor_target', L.dptr(anchors), N, L.dptr(gt), L.dptr(off), B, int(image_shape[0]), int(image_shape[1]),
           float(pos_iou_threshold), float(neg_iou_threshold), S, int(max_pos_samples), L.host4(means, 'target_means'),
           L.host4(stds, 'target_stds'), int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_image_id) & 0xFFFFFFFF, L.dptr(labels),
           L.dptr(targets), L.dptr(inside), L.dptr(outside), L.dptr(sample_idx), L.dptr(sample_targets), L.dptr(counts),
           L.dptr(before), L.dptr(argmax), L.dptr(ws), ws.numel(), L.stream())
    return AnchorTargets(labels, targets, inside, outside, sample_idx, sample_targets, counts, before, argmax)


def proposal_targets(rois, gt_boxes, gt_labels, gt_offsets, num_classes, pos_iou_threshold, neg_iou_threshold,
                     total_num_samples, max_pos_samples, means, stds, reference_row_labels=True, seed=0, first_image_id=0,
                     roi_counts=None, workspace=None):
    """odet_proposal_target: rois [B,Rmax,4] (roi_counts: optional device int32 [B]) -> ProposalTargets of final_rois [B,S,4],
    final_labels int32 [B,S], targets / inside / outside [B,S,4*num_classes], keep int32 [B,S], gt_assignment int32 [B,Rmax],
    counts int32 [B,4].  Nothing is read back."""
    rois = L.f32c(rois, 'rois')
    if rois.dim() != 3 or rois.shape[2] != 4:
        raise ValueError('rois must have shape [B,Rmax,4], got %s' % (tuple(rois.shape),))
    gt = _boxes(gt_boxes, 'gt_boxes')
    dev = rois.device
    off = _gt_offsets(gt_offsets, dev)
    B, R, S, W = rois.shape[0], rois.shape[1], int(total_num_samples), 4 * int(num_classes)
    if off.numel() != B + 1:
        raise ValueError('gt_offsets has %d entries for %d images' % (off.numel(), B))
    if not isinstance(gt_labels, torch.Tensor) or not gt_labels.is_cuda:
        raise L.OdetError('gt_labels must live on the GPU: tf_eager_object_detection_amd has no CPU path')
    gl = gt_labels.to(torch.int32).contiguous()
    if gl.numel() != gt.shape[0]:
        raise ValueError('gt_labels has %d entries for %d boxes' % (gl.numel(), gt.shape[0]))
    if gt.shape[0] == 0:
        gt, gl = gt.new_zeros((1, 4)), gl.new_zeros(1)

    def new(shape, dtype=torch.float32):
        return torch.empty(shape, dtype=dtype, device=dev)
    out = ProposalTargets(new((B, S, 4)), new((B, S), torch.int32), new((B, S, W)), new((B, S, W)), new((B, S, W)),
                          new((B, S), torch.int32), new((B, R), torch.int32), new((B, 4), torch.int32))
    nb = L.lib().odet_proposal_target_workspace_bytes(R, B)
    ws = workspace if workspace is not None and workspace.numel() >= nb else L.workspace(nb, dev)
    L.call('odet_proposal_target', L.dptr(rois), L.dptr(roi_counts, torch.int32, 'roi_counts'), R, L.dptr(gt), L.dptr(gl),
           L.dptr(off), B, int(num_classes), float(pos_iou_threshold), float(neg_iou_threshold), S, int(max_pos_samples),
           L.host4(means, 'target_means'), L.host4(stds, 'target_stds'), 1 if reference_row_labels else 0,
           int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_image_id) & 0xFFFFFFFF, *[L.dptr(t) for t in out], L.dptr(ws), ws.numel(),
           L.stream())
    return out


# ---- fused training losses (csrc/losses.hip) ------------------------------------------------------------------------------------
LOSSES_MAX_CLASSES = 1024
LOSSES_MAX_ROWS = 2048

RpnLosses = collections.namedtuple('RpnLosses', ['losses', 'row_grad_scores', 'row_grad_deltas'])
RpnLossGrads = collections.namedtuple('RpnLossGrads', ['grad_scores', 'grad_deltas'])
RoiLosses = collections.namedtuple('RoiLosses', ['losses', 'grad_scores', 'grad_deltas'])


def _rpn_head_outputs(scores, deltas, B):
    """float32 contiguous scores (2N floats per image, any shape) and deltas (4N floats per image) of B images -> (s, d, N)"""
    scores, deltas = L.f32c(scores, 'rpn scores'), L.f32c(deltas, 'rpn deltas')
    if deltas.numel() % (4 * B) or scores.numel() * 2 != deltas.numel():
        raise ValueError('rpn scores / deltas of %d / %d elements do not hold 2N / 4N floats for each of %d images'
                         % (scores.numel(), deltas.numel(), B))
    return scores, deltas, deltas.numel() // (4 * B)


def rpn_losses(scores, deltas, sample_idx, sample_targets, counts, sigma, layout=RPN_LAYOUT_FPN, anchors_per_location=1):
    """odet_rpn_loss: the head outputs of B images (scores in `layout` with A = `anchors_per_location`, deltas [B,N,4]) and the
    compact anchor targets (AnchorTargets.sample_idx / sample_targets / counts) -> RpnLosses(losses [B,2] = (cls, reg), row_grad_scores [B,S,2],
    row_grad_deltas [B,S,4]).  Nothing is read back."""
    B, S = int(sample_idx.shape[0]), int(sample_idx.shape[1])
    scores, deltas, N = _rpn_head_outputs(scores, deltas, B)
    dev = scores.device
    out = RpnLosses(torch.empty((B, 2), dtype=torch.float32, device=dev), torch.empty((B, S, 2), dtype=torch.float32, device=dev),
                    torch.empty((B, S, 4), dtype=torch.float32, device=dev))
    L.call('odet_rpn_loss', L.dptr(scores), L.dptr(deltas), N, B, int(layout), int(anchors_per_location),
           L.dptr(sample_idx, torch.int32, 'sample_idx'), L.dptr(sample_targets, torch.float32, 'sample_targets'),
           L.dptr(counts, torch.int32, 'counts'), S, float(sigma), *[L.dptr(t) for t in out], L.stream())
    return out


def rpn_losses_backward(sample_idx, row_grad_scores, row_grad_deltas, upstream, num_anchors, layout=RPN_LAYOUT_FPN,
                        anchors_per_location=1, scores=True, deltas=True):
    """odet_rpn_loss_backward for N = `num_anchors` anchors per image (the header's name): upstream float32 [B,2] (device) ->
    RpnLossGrads(grad_scores [B, 2N] in the scores' layout, grad_deltas [B,N,4]); `scores` / `deltas` = False leaves that gradient out (None)."""
    B, S, N = int(sample_idx.shape[0]), int(sample_idx.shape[1]), int(num_anchors)
    dev = sample_idx.device
    gs = torch.empty((B, 2 * N), dtype=torch.float32, device=dev) if scores else None
    gd = torch.empty((B, N, 4), dtype=torch.float32, device=dev) if deltas else None
    L.call('odet_rpn_loss_backward', L.dptr(sample_idx, torch.int32, 'sample_idx'),
           L.dptr(row_grad_scores, torch.float32, 'row_grad_scores'), L.dptr(row_grad_deltas, torch.float32, 'row_grad_deltas'),
           L.dptr(upstream, torch.float32, 'upstream'), N, B, int(layout), int(anchors_per_location), S, L.dptr(gs), L.dptr(gd),
           L.stream())
    return RpnLossGrads(gs, gd)


def roi_losses(scores, deltas, final_labels, targets, inside, outside, counts, sigma, row_map=None, upstream=None,
               losses=True, grads=True, grad_scores=True, grad_deltas=True):
    """odet_roi_loss: scores [B,R,C], deltas [B,R,4C] and the outputs of ops.proposal_targets -> RoiLosses(losses [B,2] =
    (cls, reg), grad_scores [B,R,C], grad_deltas [B,R,4C]) (None where not asked for: `losses`, `grads` for both gradients,
    `grad_scores` / `grad_deltas` for one).  row_map: int32 [B,R], head row ->
    target row; upstream: device float32 [B,2].  Nothing is read back."""
    scores, deltas = L.f32c(scores, 'roi scores'), L.f32c(deltas, 'roi deltas')
    if scores.dim() != 3 or deltas.dim() != 3 or deltas.shape[:2] != scores.shape[:2] or deltas.shape[2] != 4 * scores.shape[2]:
        raise ValueError('roi scores / deltas must have shapes [B,R,C] / [B,R,4C], got %s / %s'
                         % (tuple(scores.shape), tuple(deltas.shape)))
    B, R, C = (int(v) for v in scores.shape)
    S = int(final_labels.shape[1])
    for name, t, shape in (('final_labels', final_labels, (B, S)), ('targets', targets, (B, S, 4 * C)),
                           ('inside', inside, (B, S, 4 * C)), ('outside', outside, (B, S, 4 * C)), ('counts', counts, (B, 4))):
        if tuple(t.shape) != shape:
            raise ValueError('%s of shape %s does not match %s (%d images, %d classes)' % (name, tuple(t.shape), shape, B, C))
    if row_map is not None and tuple(row_map.shape) != (B, R):
        raise ValueError('row_map must have shape [%d,%d]' % (B, R))
    dev = scores.device
    out = RoiLosses(torch.empty((B, 2), dtype=torch.float32, device=dev) if losses else None,
                    torch.empty((B, R, C), dtype=torch.float32, device=dev) if grads and grad_scores else None,
                    torch.empty((B, R, 4 * C), dtype=torch.float32, device=dev) if grads and grad_deltas else None)
    L.call('odet_roi_loss', L.dptr(scores), L.dptr(deltas), R, C, B, L.dptr(final_labels, torch.int32, 'final_labels'),
           L.dptr(targets, torch.float32, 'targets'), L.dptr(inside, torch.float32, 'inside'),
           L.dptr(outside, torch.float32, 'outside'), L.dptr(counts, torch.int32, 'counts'), S,
           L.dptr(row_map, torch.int32, 'row_map'), float(sigma), L.dptr(upstream, torch.float32, 'upstream'),
           *[L.dptr(t) for t in out], L.stream())
    return out


# ---- the training step (csrc/optimizer.hip) -------------------------------------------------------------------------------------
OPT_CHUNK = L.OPT_CHUNK
OPT_MAX_TENSORS, OPT_MAX_CHUNKS, OPT_MAX_BOUNDARIES = L.OPT_MAX_TENSORS, L.OPT_MAX_CHUNKS, L.OPT_MAX_BOUNDARIES

OptimizerOutputs = collections.namedtuple('OptimizerOutputs', ['l2_loss', 'tensor_l2_losses'])


def opt_chunk_table(numels):
    """numel per variable -> (first_chunk per variable, [(tensor, offset)]): chunks of OPT_CHUNK elements, none spanning two
    tensors, a tensor's chunks consecutive in ascending offset (host arithmetic only)"""
    first, chunks = [], []
    for t, n in enumerate(numels):
        first.append(len(chunks))
        chunks.extend((t, o) for o in range(0, int(n), OPT_CHUNK))
    return first, chunks


def _bytes_tensor(obj, device):
    return torch.frombuffer(bytearray(bytes(obj)), dtype=torch.uint8).to(device)


class _PointerColumn:
    """A device column of tensor pointers (int64, 0 = absent) with its pinned staging copy: a table of its own, so that tensors
    that moved cost an 8-byte re-upload each and unchanged pointers cost nothing."""

    def __init__(self, n, device):
        self.n = int(n)
        self.device_column = torch.zeros(max(self.n, 1), dtype=torch.int64, device=device)
        self._host = torch.zeros(max(self.n, 1), dtype=torch.int64).pin_memory()
        self._now = None
        self._copied = None

    def set(self, pointers, in_capture):
        """Unchanged -> nothing happens, returns False.  Changed -> re-uploaded from pinned memory on the current stream (nothing
        is read back), returns True; inside a graph capture that raises OdetError(in_capture)."""
        pointers = tuple(int(p) for p in pointers)
        if len(pointers) != self.n:
            raise ValueError('%d pointers for a column of %d' % (len(pointers), self.n))
        if pointers == self._now:
            return False
        if torch.cuda.is_current_stream_capturing():
            raise L.OdetError(in_capture)
        if self._copied is not None:
            self._copied.synchronize()                         # (the previous upload has left the pinned buffer)
        if pointers:
            self._host[:len(pointers)] = torch.tensor(pointers, dtype=torch.int64)
        self.device_column.copy_(self._host, non_blocking=True)
        self._copied = torch.cuda.Event()
        self._copied.record()
        self._now = pointers
        return True


class OptimizerTables:
    """The device tables of one variable list (include/odet.h "training step"), built once: the tensor records, the chunk
    table, the gradient pointer column with its pinned staging copy, the partials buffer and the two L2 outputs.
    records: one dict per variable with var, slot0, slot1, master (tensors or None), weight_decay, grad_scale, grad_f16."""

    def __init__(self, records, device):
        self.device = torch.device(device)
        T = len(records)
        if T > OPT_MAX_TENSORS:
            raise ValueError('%d variables exceed the limit of %d' % (T, OPT_MAX_TENSORS))
        first, chunks = opt_chunk_table([r['var'].numel() for r in records])
        if len(chunks) > OPT_MAX_CHUNKS:
            raise ValueError('%d chunks exceed the limit of %d' % (len(chunks), OPT_MAX_CHUNKS))
        self.num_tensors, self.num_chunks = T, len(chunks)
        self._keep = records                                   # (the tables hold raw pointers into these tensors)
        self._first = first
        ctab = (L.OdetOptChunk * max(len(chunks), 1))()
        for i, (t, o) in enumerate(chunks):
            ctab[i].offset, ctab[i].tensor = o, t
        self.chunks = _bytes_tensor(ctab, self.device)
        self.tensors = torch.empty(max(T, 1) * C.sizeof(L.OdetOptTensor), dtype=torch.uint8, device=self.device)
        self.write_tensors()
        self._column = _PointerColumn(T, self.device)
        self.grads = self._column.device_column
        self.partials = L.workspace(L.lib().odet_opt_partials_bytes(self.num_chunks), self.device)
        self.tensor_l2_losses = torch.zeros(max(T, 1), dtype=torch.float32, device=self.device)[:T]
        self.l2_loss = torch.zeros((), dtype=torch.float32, device=self.device)

    def _ptr(self, t, dtype, name):
        if t is None:
            return None
        if t.device != self.device:
            raise L.OdetError('%s lives on %s, the tables on %s' % (name, t.device, self.device))
        if dtype is not None and t.dtype != dtype:
            raise TypeError('%s must be %s, got %s' % (name, dtype, t.dtype))
        return t.data_ptr()

    def write_tensors(self):
        """(re)writes the tensor records from the record dicts: a copy to the device on the current stream"""
        tab = (L.OdetOptTensor * max(self.num_tensors, 1))()
        for i, r in enumerate(self._keep):
            v = r['var']
            if v.dtype not in (torch.float32, torch.float16):
                raise TypeError('variable %d must be float32 or float16, got %s' % (i, v.dtype))
            if v.dtype == torch.float16 and r.get('master') is None:
                raise ValueError('float16 variable %d has no float32 master' % i)
            e = tab[i]
            e.var = self._ptr(v, None, 'variable %d' % i)
            e.slot0 = self._ptr(r.get('slot0'), torch.float32, 'slot0 of variable %d' % i)
            e.slot1 = self._ptr(r.get('slot1'), torch.float32, 'slot1 of variable %d' % i)
            e.master = self._ptr(r.get('master'), torch.float32, 'master of variable %d' % i) if v.dtype == torch.float16 else None
            e.numel = v.numel()
            e.weight_decay = float(r.get('weight_decay', 0.0))
            e.grad_scale = float(r.get('grad_scale', 1.0))
            e.flags = (L.OPT_VAR_F16 if v.dtype == torch.float16 else 0) | (L.OPT_GRAD_F16 if r.get('grad_f16') else 0)
            e.first_chunk = self._first[i]
        host = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8)
        if torch.cuda.is_current_stream_capturing():
            raise L.OdetError('the tensor table changed inside a graph capture')
        self.tensors.copy_(host)                               # (pageable: the copy has completed on return)

    def set_gradients(self, pointers):
        """pointers: one int per variable (0 = None this step).  Unchanged -> nothing happens.  Changed -> the pointer column is
        re-uploaded from pinned memory on the current stream (nothing is read back); inside a graph capture that is an error."""
        pointers = tuple(pointers)
        if len(pointers) != self.num_tensors:
            raise ValueError('%d gradient pointers for %d variables' % (len(pointers), self.num_tensors))
        return self._column.set(pointers, 'the gradient pointers changed inside a graph capture: bind the gradients the graph will '
                                'use (set_gradients / Optimizer.prepare) before capturing, and write new gradients into them')


def _opt_config(tables, kind=0, num_boundaries=0, momentum=0.0, beta1=0.0, beta2=0.0, epsilon=0.0):
    return L.OdetOptConfig(int(kind), tables.num_tensors, tables.num_chunks, int(num_boundaries), float(momentum),
                           float(beta1), float(beta2), float(epsilon))


def optimizer_step(tables, state, kind, num_boundaries=0, momentum=0.0, beta1=0.9, beta2=0.999, epsilon=1e-8, l2=True):
    """odet_opt_step over `tables` (whose gradient column the caller has set) and the device state block `state` (uint8
    [sizeof odet_opt_state_t]).  l2: also write tables.l2_loss / tables.tensor_l2_losses (of the pre-update values).  Two
    launches, nothing is read back."""
    if state.dtype != torch.uint8 or state.numel() != C.sizeof(L.OdetOptState) or state.device != tables.device:
        raise ValueError('state must be a uint8 tensor of %d bytes on %s' % (C.sizeof(L.OdetOptState), tables.device))
    cfg = _opt_config(tables, kind, num_boundaries, momentum, beta1, beta2, epsilon)
    L.call('odet_opt_step', C.byref(cfg), L.dptr(tables.tensors), L.dptr(tables.grads), L.dptr(tables.chunks), L.dptr(state),
           L.dptr(tables.partials), tables.partials.numel(), L.dptr(tables.tensor_l2_losses) if l2 else None,
           L.dptr(tables.l2_loss) if l2 else None, L.stream())
    return OptimizerOutputs(tables.l2_loss, tables.tensor_l2_losses) if l2 else None


def l2_loss(tables):
    """odet_l2_loss: the regulariser's forward value (total, per tensor) over `tables`, nothing else written"""
    cfg = _opt_config(tables)
    L.call('odet_l2_loss', C.byref(cfg), L.dptr(tables.tensors), L.dptr(tables.chunks), L.dptr(tables.partials),
           tables.partials.numel(), L.dptr(tables.tensor_l2_losses), L.dptr(tables.l2_loss), L.stream())
    return OptimizerOutputs(tables.l2_loss, tables.tensor_l2_losses)


# ---- the gradient exchange (csrc/grad_exchange.hip) -----------------------------------------------------------------------------
RANK_MEAN_MAX_WORLD = L.RANK_MEAN_MAX_WORLD


def memory_dense(t):
    """True when the tensor's elements fill numel consecutive places (contiguous in the default or the channels-last sense)"""
    if t.numel() == 0 or t.is_contiguous():
        return True
    if t.dim() == 4:
        return t.is_contiguous(memory_format=torch.channels_last)
    if t.dim() == 5:
        return t.is_contiguous(memory_format=torch.channels_last_3d)
    return False


class BucketTables:
    """The layout of one tensor list in a float32 bucket (include/odet.h "gradient exchange") and, on a GPU, its device tables.
    numels: one int per tensor, None = absent (no place in the bucket).  The chunk table is the optimizer's (opt_chunk_table)
    over the present tensors, so table chunk c is bucket chunk c; the bucket is world * shard_chunks chunks, the chunks past
    the table being padding.  device None / cpu: host arithmetic only (the layout; nothing is uploaded)."""

    def __init__(self, numels, world=1, device=None):
        self.world = int(world)
        if self.world < 1:
            raise ValueError('world must be at least 1, got %d' % self.world)
        self.numels = [None if n is None else int(n) for n in numels]
        T = len(self.numels)
        if T > OPT_MAX_TENSORS:
            raise ValueError('%d tensors exceed the limit of %d' % (T, OPT_MAX_TENSORS))
        first, self.chunk_list = opt_chunk_table([0 if n is None else n for n in self.numels])
        self.first_chunk = [None if n is None else f for n, f in zip(self.numels, first)]
        self.num_tensors, self.num_chunks = T, len(self.chunk_list)
        self.shard_chunks = -(-self.num_chunks // self.world)
        self.bucket_chunks = self.world * self.shard_chunks
        if self.bucket_chunks > OPT_MAX_CHUNKS:
            raise ValueError('%d chunks exceed the limit of %d' % (self.bucket_chunks, OPT_MAX_CHUNKS))
        self.shard_numel, self.bucket_numel = self.shard_chunks * OPT_CHUNK, self.bucket_chunks * OPT_CHUNK
        self.device = torch.device(device) if device is not None else torch.device('cpu')
        if self.device.type == 'cuda':
            ctab = (L.OdetOptChunk * max(self.num_chunks, 1))()
            for i, (t, o) in enumerate(self.chunk_list):
                ctab[i].offset, ctab[i].tensor = o, t
            self.chunks = _bytes_tensor(ctab, self.device)
            self.numels_dev = torch.tensor([0 if n is None else n for n in self.numels] or [0], dtype=torch.int64).to(self.device)
            self._column = _PointerColumn(T, self.device)
            self.pointers = self._column.device_column

    def offset(self, t):
        """first bucket element of tensor t (a multiple of OPT_CHUNK), None for an absent one"""
        f = self.first_chunk[t]
        return None if f is None else f * OPT_CHUNK

    def new_bucket(self, device=None):
        return torch.empty(self.bucket_numel, dtype=torch.float32, device=device if device is not None else self.device)

    def check(self, tensors):
        """the tensors this layout was built for: float32, dense, present exactly where the layout has a place"""
        tensors = list(tensors)
        if len(tensors) != self.num_tensors:
            raise ValueError('%d tensors for a layout of %d' % (len(tensors), self.num_tensors))
        for i, (t, n) in enumerate(zip(tensors, self.numels)):
            if (t is None) != (n is None):
                raise ValueError('tensor %d is %s, the layout has it %s' % (i, 'absent' if t is None else 'present',
                                                                            'absent' if n is None else 'present'))
            if t is None:
                continue
            if t.dtype != torch.float32:
                raise TypeError('tensor %d must be float32, got %s' % (i, t.dtype))
            if t.numel() != n:
                raise ValueError('tensor %d has %d elements, the layout %d' % (i, t.numel(), n))
            if not memory_dense(t):
                raise ValueError('tensor %d is not dense in memory (shape %s, strides %s)' % (i, tuple(t.shape), t.stride()))
            if t.device != self.device:
                raise L.OdetError('tensor %d lives on %s, the tables on %s' % (i, t.device, self.device))
        return tensors

    def set_pointers(self, tensors):
        """binds the tensor list (None = absent).  Unchanged pointers -> nothing happens, returns False.  Changed -> the pointer
        column is re-uploaded from pinned memory on the current stream; inside a graph capture that is an error."""
        return self._column.set([0 if t is None else t.data_ptr() for t in self.check(tensors)],
                                'the bucket pointers changed inside a graph capture: bind the tensors before capturing')

    def _bucket(self, bucket):
        if bucket.dtype != torch.float32 or bucket.numel() != self.bucket_numel or not bucket.is_contiguous() or bucket.dim() != 1:
            raise ValueError('the bucket must be a contiguous float32 vector of %d elements' % self.bucket_numel)
        if bucket.device != self.device:
            raise L.OdetError('the bucket lives on %s, the tables on %s' % (bucket.device, self.device))
        return bucket


def bucket_pack(tables, tensors, bucket=None):
    """odet_bucket_pack_f32: the list of float32 tensors (None where the layout has none) -> the whole bucket, one launch"""
    bucket = tables._bucket(bucket if bucket is not None else tables.new_bucket())
    tables.set_pointers(tensors)
    L.call('odet_bucket_pack_f32', L.dptr(tables.pointers), L.dptr(tables.numels_dev), tables.num_tensors, L.dptr(tables.chunks),
           tables.num_chunks, L.dptr(bucket), tables.bucket_chunks, L.stream())
    return bucket


def bucket_accumulate(tables, tensors, bucket, first, divisor=1.0):
    """odet_bucket_accumulate_f32: one image of a K-image window, one launch.  first: bucket = tensors, every element of the
    bucket written as bucket_pack writes it; else bucket += tensors (one float32 add) over the present tensors' elements only.
    divisor != 1: the sum then goes through one IEEE float32 division (the window's last call carries float32(K))."""
    tables._bucket(bucket)
    divisor = float(divisor)
    if not (0.0 < divisor < float('inf')):
        raise ValueError('the divisor must be finite and > 0, got %r' % divisor)
    tables.set_pointers(tensors)
    L.call('odet_bucket_accumulate_f32', L.dptr(tables.pointers), L.dptr(tables.numels_dev), tables.num_tensors, L.dptr(tables.chunks),
           tables.num_chunks, L.dptr(bucket), tables.bucket_chunks, 1 if first else 0, divisor, L.stream())
    return bucket


def bucket_unpack(tables, bucket, tensors):
    """odet_bucket_unpack_f32: the bucket -> the tensors' own elements, one launch; nothing else is written"""
    tables._bucket(bucket)
    tables.set_pointers(tensors)
    L.call('odet_bucket_unpack_f32', L.dptr(bucket), tables.bucket_chunks, L.dptr(tables.pointers), L.dptr(tables.numels_dev),
           tables.num_tensors, L.dptr(tables.chunks), tables.num_chunks, L.stream())
    return tensors


def rank_mean(parts, average=True, out=None):
    """odet_rank_mean_f32: parts float32 [world, n] -> [n], the float32 sum over the ranks in ascending rank order, divided by
    float32(world) with `average`"""
    if parts.dim() != 2:
        raise ValueError('parts must have shape [world, n], got %s' % (tuple(parts.shape),))
    world, n = parts.shape
    if world < 1:
        raise ValueError('world must be at least 1')
    if world > RANK_MEAN_MAX_WORLD:
        raise ValueError('world %d exceeds the limit of %d' % (world, RANK_MEAN_MAX_WORLD))
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=parts.device)
    elif tuple(out.shape) != (n,) or out.device != parts.device:
        raise ValueError('out must have shape [%d] on %s' % (n, parts.device))
    L.call('odet_rank_mean_f32', L.dptr(parts, torch.float32, 'parts'), int(world), int(n), 1 if average else 0,
           L.dptr(out, torch.float32, 'out'), L.stream())
    return out
