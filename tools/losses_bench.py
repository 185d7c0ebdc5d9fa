#!/usr/bin/env python3
"""Times targets -> losses -> gradients of the training head two ways on the same inputs; writes profiles/losses_bench.json.

  fused      one batch per call: ops.anchor_targets(dense=False) + ops.rpn_losses + ops.rpn_losses_backward, resp.
             ops.proposal_targets + ops.roi_losses (losses and gradients in one launch).
               us       GPU time: 10 calls captured in one HIP graph, replayed, median of 20 replays / 10;
               wall_us  the same calls eagerly: synchronised wall time, median (launches and output allocation included).
  composed   what `training=True` did before the fused losses existed, one image after the other: the fused target stage with
             its dense outputs (FusedAnchorTarget / FusedProposalTarget single-image calls), the callers' _get_rpn_loss /
             _get_roi_loss through model/losses.py (nonzero, gathers, elementwise torch launches) and torch autograd back to the
             same two head tensors.  It reads the device on the host, so it cannot be captured: synchronised wall time is the
             only clock that applies (composed_wall_us), and `wall_us` is the fused number to hold against it.

Rows: 800 x 1333 FPN anchors (N = 267 069), G in {8, 100} boxes per image, batch in {1, 8}; the RoI head on the 128 rows sampled
from R = 2000 RoIs per image with C in {21, 81} classes.

    python tools/losses_bench.py"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tf_eager_object_detection_amd import ops                                            # noqa: E402
from tf_eager_object_detection_amd import synthetic as syn                               # noqa: E402
from tf_eager_object_detection_amd.model.anchor_target import FusedAnchorTarget          # noqa: E402
from tf_eager_object_detection_amd.model.losses import cls_loss, smooth_l1_loss          # noqa: E402
from tf_eager_object_detection_amd.model.proposal_target import FusedProposalTarget      # noqa: E402
from tools.targets_bench import INNER, SHAPE, fpn_anchors, graph_us, wall_us             # noqa: E402

RPN = (0.7, 0.3, 256, 128, [0, 0, 0, 0], [1, 1, 1, 1])
ROI_TAIL = (0.5, 0.0, 128, 32, [0, 0, 0, 0], [0.1, 0.1, 0.2, 0.2])
RPN_SIGMA, ROI_SIGMA = 3.0, 1.0


def composed_rpn(layer, gt, anchors, scores, deltas):
    """base_fpn_model.py: the dense targets of one image, _get_rpn_loss, autograd to the head tensors"""
    labels, targets, inside, outside = layer((gt, SHAPE, anchors))
    sel = torch.nonzero(labels >= 0)[:, 0]
    cls = cls_loss(logits=scores[sel], labels=labels[sel])
    reg = smooth_l1_loss(deltas, targets, inside, outside, RPN_SIGMA, dim=[0, 1])
    return (cls, reg) + torch.autograd.grad(cls + reg, (scores, deltas))


def composed_roi(layer, rois, gt, gl, scores, deltas):
    """the proposal targets of one image, _get_roi_loss, autograd to the head tensors"""
    _, labels, targets, inside, outside = layer((rois, gt, gl))
    cls = cls_loss(logits=scores, labels=labels)
    reg = smooth_l1_loss(deltas, targets, inside, outside, sigma=ROI_SIGMA)
    return (cls, reg) + torch.autograd.grad(cls + reg, (scores, deltas))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', help='output path (default profiles/losses_bench.json)')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    anchors = fpn_anchors(SHAPE)
    N = int(anchors.shape[0])
    rows = []
    for G in (8, 100):
        for B in (1, 8):
            rng = np.random.default_rng(100 * G + B)
            gts = [syn.random_boxes(G, SHAPE, rng, 16, 600) for _ in range(B)]
            gb = torch.from_numpy(np.concatenate(gts)).cuda()
            off = torch.arange(0, (B + 1) * G, G, dtype=torch.int32, device='cuda')
            per_image = [torch.from_numpy(g).cuda() for g in gts]
            scores = torch.from_numpy(rng.normal(0, 2, (B, N, 2)).astype(np.float32)).cuda()
            deltas = torch.from_numpy(rng.normal(0, 0.3, (B, N, 4)).astype(np.float32)).cuda()
            upstream = torch.ones((B, 2), device='cuda')
            leaf_s, leaf_d = scores.clone().requires_grad_(), deltas.clone().requires_grad_()
            layer = FusedAnchorTarget(*RPN, seed=1)

            def composed():
                return [composed_rpn(layer, per_image[b], anchors, leaf_s[b], leaf_d[b]) for b in range(B)]

            def fused():
                at = ops.anchor_targets(anchors, gb, off, SHAPE, *RPN, seed=1, dense=False)
                fwd = ops.rpn_losses(scores, deltas, at.sample_idx, at.sample_targets, at.counts, RPN_SIGMA)
                return fwd, ops.rpn_losses_backward(at.sample_idx, fwd.row_grad_scores, fwd.row_grad_deltas, upstream, N)
            c_us = wall_us(composed)
            row = dict(op='rpn', N=N, G=G, batch=B, us=round(graph_us(fused), 1), wall_us=round(wall_us(fused), 1),
                       composed_wall_us=round(c_us, 1))
            row['composed_vs_fused_wall'] = round(row['composed_wall_us'] / row['wall_us'], 1)
            print(json.dumps(row), flush=True)
            rows.append(row)
    R = 2000
    for C in (21, 81):
        for G in (8, 100):
            for B in (1, 8):
                rng = np.random.default_rng(7 * G + B + C)
                roi = (C,) + ROI_TAIL
                S = roi[3]
                gts = [syn.random_boxes(G, SHAPE, rng, 16, 600) for _ in range(B)]
                rois = np.stack([np.concatenate([syn.random_boxes(R - 500, SHAPE, rng, 16, 600),
                                                 (g[rng.integers(0, G, 500)] + rng.normal(0, 8, (500, 4))).astype(np.float32)])
                                 for g in gts]).astype(np.float32)
                gb = torch.from_numpy(np.concatenate(gts)).cuda()
                gl = torch.from_numpy(rng.integers(1, min(C, 21), B * G).astype(np.int32)).cuda()
                off = torch.arange(0, (B + 1) * G, G, dtype=torch.int32, device='cuda')
                gr = torch.from_numpy(rois).cuda()
                scores = torch.from_numpy(rng.normal(0, 2, (B, S, C)).astype(np.float32)).cuda()
                deltas = torch.from_numpy(rng.normal(0, 0.7, (B, S, 4 * C)).astype(np.float32)).cuda()
                upstream = torch.ones((B, 2), device='cuda')
                leaf_s, leaf_d = scores.clone().requires_grad_(), deltas.clone().requires_grad_()
                layer = FusedProposalTarget(*roi, seed=1)
                per_image = [(gr[b], gb[b * G:(b + 1) * G], gl[b * G:(b + 1) * G].long()) for b in range(B)]

                def composed():
                    return [composed_roi(layer, *per_image[b], leaf_s[b], leaf_d[b]) for b in range(B)]

                def fused():
                    pt = ops.proposal_targets(gr, gb, gl, off, *roi, seed=1)
                    return ops.roi_losses(scores, deltas, pt.final_labels, pt.targets, pt.inside, pt.outside, pt.counts,
                                          ROI_SIGMA, upstream=upstream)
                c_us = wall_us(composed)
                row = dict(op='roi', R=R, rows=S, C=C, G=G, batch=B, us=round(graph_us(fused), 1),
                           wall_us=round(wall_us(fused), 1), composed_wall_us=round(c_us, 1))
                row['composed_vs_fused_wall'] = round(row['composed_wall_us'] / row['wall_us'], 1)
                print(json.dumps(row), flush=True)
                rows.append(row)
    out = dict(device=torch.cuda.get_device_name(0),
               protocol='us: %d calls per HIP graph, median of 20 replays; wall_us / composed_wall_us: synchronised wall time, '
                        'median of 10 calls' % INNER, rows=rows)
    path = a.out or os.path.join(ROOT, 'profiles', 'losses_bench.json')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
    print('wrote', path)


if __name__ == '__main__':
    main()
