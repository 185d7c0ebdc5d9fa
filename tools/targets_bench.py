#!/usr/bin/env python3
"""Times the fused training targets (odet_anchor_target / odet_proposal_target, one call per batch) next to the torch-composed
classes (model.AnchorTarget / model.ProposalTarget, one call per image) on the same inputs; writes profiles/targets_bench.json.

Rows: 800 x 1333 FPN anchors (N = 267 069), G in {8, 100} boxes per image, batch in {1, 8}, dense outputs and compact-only;
the proposal targets on R = 2000 RoIs per image.
  us            fused call, GPU time: 10 calls captured in one HIP graph, replayed, median of the replays / 10 (the protocol of
                tools/preprocess_bench.py; output allocation happens once, at capture);
  wall_us       the same fused call eagerly: synchronised wall time, median (what a caller outside a graph pays: launches and
                output allocation included);
  torch_wall_us the composed class over the images of the batch, one after the other: synchronised wall time, median.  It reads
                device counts on the host several times per image, so it cannot be captured -- wall time is the only clock that
                applies to it, and `wall_us` is the fused number to hold against it.

    python tools/targets_bench.py"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tf_eager_object_detection_amd import ops                                            # noqa: E402
from tf_eager_object_detection_amd import synthetic as syn                               # noqa: E402
from tf_eager_object_detection_amd.model.anchor_target import AnchorTarget               # noqa: E402
from tf_eager_object_detection_amd.model.proposal_target import ProposalTarget           # noqa: E402
from tf_eager_object_detection_amd.utils.anchor_generator import make_anchors            # noqa: E402

INNER = 10
SHAPE = (800, 1333)
RPN = (0.7, 0.3, 256, 128, [0, 0, 0, 0], [1, 1, 1, 1])
ROI = (21, 0.5, 0.0, 128, 32, [0, 0, 0, 0], [0.1, 0.1, 0.2, 0.2])


def graph_us(fn, replays=20):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s), torch.cuda.graph(g, stream=s):
        for _ in range(INNER):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(replays):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / INNER)
    return float(np.median(ts))


def wall_us(fn, calls=10):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e6)
    return float(np.median(ts))


def fpn_anchors(shape):
    out = []
    for stride, base in zip(syn.FPN_STRIDES, syn.FPN_BASE_SIZES):
        out.append(make_anchors(base_anchor_size=base, anchor_scales=syn.FPN_SCALES, anchor_ratios=syn.FPN_RATIOS,
                                featuremap_height=float(-(-shape[0] // stride)), featuremap_width=float(-(-shape[1] // stride)),
                                stride=stride))
    return torch.cat(out, dim=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', help='output path (default profiles/targets_bench.json)')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    anchors = fpn_anchors(SHAPE)
    rows = []
    for G in (8, 100):
        for B in (1, 8):
            rng = np.random.default_rng(100 * G + B)
            gts = [syn.random_boxes(G, SHAPE, rng, 16, 600) for _ in range(B)]
            gb = torch.from_numpy(np.concatenate(gts)).cuda()
            off = torch.arange(0, (B + 1) * G, G, dtype=torch.int32, device='cuda')
            per_image = [torch.from_numpy(g).cuda() for g in gts]
            composed = AnchorTarget(*RPN)

            def torch_call():
                return [composed((g, SHAPE, anchors)) for g in per_image]
            t_us = wall_us(torch_call)
            for dense in (True, False):
                def fused():
                    return ops.anchor_targets(anchors, gb, off, SHAPE, *RPN, seed=1, dense=dense)
                row = dict(op='anchor_target', N=int(anchors.shape[0]), G=G, batch=B, outputs='dense' if dense else 'compact',
                           us=round(graph_us(fused), 1), wall_us=round(wall_us(fused), 1), torch_wall_us=round(t_us, 1))
                row['torch_vs_fused_wall'] = round(row['torch_wall_us'] / row['wall_us'], 1)
                print(json.dumps(row))
                rows.append(row)
    R = 2000
    for G in (8, 100):
        for B in (1, 8):
            rng = np.random.default_rng(7 * G + B)
            gts = [syn.random_boxes(G, SHAPE, rng, 16, 600) for _ in range(B)]
            rois = np.stack([np.concatenate([syn.random_boxes(R - 500, SHAPE, rng, 16, 600),
                                             (g[rng.integers(0, G, 500)] + rng.normal(0, 8, (500, 4))).astype(np.float32)])
                             for g in gts]).astype(np.float32)
            gb = torch.from_numpy(np.concatenate(gts)).cuda()
            gl = torch.from_numpy(rng.integers(1, 21, B * G).astype(np.int32)).cuda()
            off = torch.arange(0, (B + 1) * G, G, dtype=torch.int32, device='cuda')
            gr = torch.from_numpy(rois).cuda()
            composed = ProposalTarget(*ROI)
            per_image = [(gr[b], gb[b * G:(b + 1) * G], gl[b * G:(b + 1) * G].long()) for b in range(B)]

            def torch_call():
                return [composed(x) for x in per_image]

            def fused():
                return ops.proposal_targets(gr, gb, gl, off, *ROI, seed=1)
            row = dict(op='proposal_target', R=R, G=G, batch=B, us=round(graph_us(fused), 1), wall_us=round(wall_us(fused), 1),
                       torch_wall_us=round(wall_us(torch_call), 1))
            row['torch_vs_fused_wall'] = round(row['torch_wall_us'] / row['wall_us'], 1)
            print(json.dumps(row))
            rows.append(row)
    out = dict(device=torch.cuda.get_device_name(0),
               protocol='us: %d calls per HIP graph, median of 20 replays; wall_us / torch_wall_us: synchronised wall time, '
                        'median of 10 calls' % INNER, rows=rows)
    path = a.out or os.path.join(ROOT, 'profiles', 'targets_bench.json')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
    print('wrote', path)


if __name__ == '__main__':
    main()
