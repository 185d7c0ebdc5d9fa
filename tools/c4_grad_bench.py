#!/usr/bin/env python3
"""Times the ResNet-C4 training graph's new launches (csrc/c4_grad.hip) at the head's own shape, the whole RoI-head backward and one
whole training call of the caller object, batch 1, against the torch composition on the same float32 tensors; writes
profiles/c4_grad_bench.json.

  ours       ops.global_avg_pool / ops.global_avg_pool_backward on 128 x 7 x 7 x 2048; for the head torch.autograd.grad through
             ResNetC4Detector.roi_head_trainable on 128 crops of 7 x 7 x 1024 (depths 50 and 101: 24 parameter gradients and the
             crops' gradient); for the training call TrainableResNetFasterRcnn with the three keywords on an 800 x 1333 image
             (training_targets = training_losses = 'hip'): the four losses and sum(losses).backward().
  yardstick  the pooling: Tensor.mean over the two pixel axes of the same NHWC tensor, and g[:, None, None, :].expand / 49
             materialised; the head: autograd over F.conv2d / mean / F.linear (the library's convolutions and GEMMs) with the same
             shapes, parameters and output gradients.  The training call has no yardstick (torch has no such model): its row is
             wall time around eager calls, synchronised, not a graph.

Clock of the graph rows: GPU time of INNER calls captured in one HIP graph and replayed; per row the two graphs are replayed
alternately, REPLAYS times each, after 3 warm-up replays; median and (min, max) per call in microseconds.  `tbytes_per_s`: the bytes
the algorithm needs (4 R (H W + 1) C on either pooling launch) over the median, next to the 8 TB/s HBM figure.  Every row with a
yardstick says MET or SLOWER.

    python tools/c4_grad_bench.py"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tf_eager_object_detection_amd import ops                                                        # noqa: E402
from tf_eager_object_detection_amd.model.base_faster_rcnn_model import TrainableResNetFasterRcnn    # noqa: E402
from tf_eager_object_detection_amd.model.frcnn_detector import ResNetC4Detector                     # noqa: E402
from tools.vgg_grad_bench import REPLAYS, HBM_BYTES_PER_S                                            # noqa: E402
import tools.vgg_grad_bench as common                                                                # noqa: E402


def pooling_rows(f, R, H, W, C):
    x, g = f(R, H, W, C), f(R, C)
    nbytes = 4 * R * (H * W + 1) * C
    shape = '%dx%dx%dx%d' % (R, H, W, C)
    return [common.row_of('global_avg_pool %s' % shape, lambda: ops.global_avg_pool(x), lambda: x.mean(dim=(1, 2)), nbytes),
            common.row_of('global_avg_pool_backward %s' % shape, lambda: ops.global_avg_pool_backward(g, (H, W)),
                          lambda: (g[:, None, None, :].expand(R, H, W, C) / float(H * W)).contiguous(), nbytes)]


def _plain_block(x, P, prefix, stride, short):
    p = lambda n: P[prefix + n]
    y = F.relu(F.conv2d(x, p('c1.weight'), p('c1.bias'), stride=stride))
    y = F.relu(F.conv2d(y, p('c2.weight'), p('c2.bias'), padding=1))
    y = F.conv2d(y, p('c3.weight'), p('c3.bias'))
    s = F.conv2d(x, p('short.weight'), p('short.bias'), stride=stride) if short else x
    return F.relu(y + s)


def head_row(f, depth, rois):
    """the RoI head's backward: three conv5 blocks, the pooling, score and bbox -- 24 parameter gradients and the crops' gradient"""
    det = ResNetC4Detector(depth, 21, (64, 64), 1, dtype=torch.float32)
    det = det.to(device='cuda', dtype=torch.float32, memory_format=torch.channels_last).eval()
    feats = f(rois, 7, 7, 1024).relu_().requires_grad_()
    outs = list(det.roi_head_trainable(feats))
    gouts = [f(*t.shape) * 1e-3 for t in outs]
    names = [n for n, _ in det.named_parameters() if n.startswith(('conv5.', 'score.', 'bbox.'))]
    params = [dict(det.named_parameters())[n] for n in names]
    assert len(params) == 24
    P = {n: dict(det.named_parameters())[n].detach().clone().requires_grad_() for n in names}
    xt = feats.detach().permute(0, 3, 1, 2).requires_grad_()                              # channels_last, as torch would hold it
    y = xt
    for i, blk in enumerate(det.conv5):
        y = _plain_block(y, P, 'conv5.%d.' % i, int(blk.c1.stride[0]), blk.short is not None)
    a = y.mean(dim=(2, 3))
    youts = [F.linear(a, P['score.weight'], P['score.bias']), F.linear(a, P['bbox.weight'], P['bbox.bias'])]
    return common.row_of('RoI head backward (24 parameter gradients + the crops), depth %d, %d crops' % (depth, rois),
                         lambda: torch.autograd.grad(outs, params + [feats], gouts, retain_graph=True),
                         lambda: torch.autograd.grad(youts, list(P.values()) + [xt], gouts, retain_graph=True), inner=2)


def training_call_row(f, image, depth, calls):
    """one whole training call of the caller object: forward with the fused targets and losses, then backward into 94 parameters"""
    m = TrainableResNetFasterRcnn(depth=depth, roi_pooling_max_pooling_flag=False, training_targets='hip', training_losses='hip',
                                  train_roi_head=True, train_rpn_head=True, train_extractor=True)
    img = f(1, image[0], image[1], 3) * 50.0
    H, W = image
    gt = torch.tensor([[0.1 * W, 0.1 * H, 0.5 * W, 0.6 * H], [0.4 * W, 0.3 * H, 0.9 * W, 0.8 * H]], device='cuda')
    gl = torch.tensor([3, 12], device='cuda')
    ts = []
    for k in range(calls + 2):
        m.dense.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        losses = m((img, gt, gl), training=True)
        sum(losses).backward()
        torch.cuda.synchronize()
        if k >= 2:
            ts.append((time.perf_counter() - t0) * 1e3)
    trained = sum(1 for p in m.dense.parameters() if p.grad is not None)
    row = dict(launch='training call (forward + backward), depth %d, %dx%d image' % (depth, H, W), clock='wall, eager, synchronised',
               calls=calls, ours_ms=round(float(np.median(ts)), 2), ours_range_ms=[round(min(ts), 2), round(max(ts), 2)],
               trained_parameters=trained, losses=[float(x.detach()) for x in losses])
    print(json.dumps(row), flush=True)
    return row


def measure(a):
    rng = np.random.default_rng(0)
    torch.manual_seed(0)                                                                   # (the models' random weights)
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).cuda()
    rows = pooling_rows(f, a.rois, 7, 7, 2048)
    rows += [head_row(f, depth, a.rois) for depth in (50, 101)]
    rows.append(training_call_row(f, tuple(a.image), 50, a.calls))
    slower = [r['launch'] for r in rows if r.get('verdict') == 'SLOWER']
    return dict(device=torch.cuda.get_device_name(0), image=list(a.image), rois=a.rois,
                protocol='calls_per_graph calls per HIP graph; ours / yardstick graphs replayed alternately, %d replays each after 3 '
                         'warm-up replays; median and [min, max] microseconds per call; tensors, autograd graphs and captures all on '
                         'one side stream; the training call: wall milliseconds around eager calls' % REPLAYS,
                hbm_figure_bytes_per_s=HBM_BYTES_PER_S, slower_than_yardstick=slower, rows=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', help='output path (default profiles/c4_grad_bench.json)')
    ap.add_argument('--image', type=int, nargs=2, default=(800, 1333))
    ap.add_argument('--rois', type=int, default=128)
    ap.add_argument('--calls', type=int, default=5)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    common.STREAM = torch.cuda.Stream()
    common.STREAM.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(common.STREAM):
        out = measure(a)
    path = a.out or os.path.join(ROOT, 'profiles', 'c4_grad_bench.json')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as fh:
        json.dump(out, fh, indent=1)
    print('wrote', path)


if __name__ == '__main__':
    main()
