#!/usr/bin/env python3
"""Times the ResNet extractor's backward (csrc/block_grad.hip's two launches, one bottleneck's backward per stage, the whole
conv2..conv5 backward at depths 50 and 101) on the 800 x 1333 image at batch 1 (C2..C5 = 200x334, 100x167, 50x84, 25x42), against
torch on the same float32 tensors; writes profiles/extractor_grad_bench.json.

  ours       ops.stride_gather and ops.block_input_grad (both forms) on each stage's map; one identity block's backward per stage and
             the whole extractor backward: everything .backward() of model/extractor_trainable.py enqueues (the autograd graph of
             block_trainable / extractor_trainable is built once, the captured part is the backward alone).
  yardstick  the torch composition each launch replaces -- x[:, ::2, ::2].contiguous(); torch.where(y > 0, dy, 0) + d1; a zero-filled
             map with d1 + d2 written into its [::2, ::2] pixels -- and, for a block and for the extractor, torch autograd of the plain
             F.conv2d bottleneck on channels_last tensors with the same weights (gradients of the same parameters and the same input).

Clock (the protocol of tools/neck_grad_bench.py): GPU time of INNER calls captured in one HIP graph and replayed; per row the two
graphs are replayed alternately, REPLAYS times each, after 3 warm-up replays; median and (min, max) per call in microseconds.
`bytes_per_s`: a launch's ALGORITHMIC bytes (every operand and the result once) over the median time; `hbm_fraction`: that over
the chip's 8 TB/s.  Every row is marked MET (ours not slower than the yardstick's median) or SLOWER.

    python tools/extractor_grad_bench.py"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tf_eager_object_detection_amd import ops                                                          # noqa: E402
from tf_eager_object_detection_amd.model.extractor_trainable import STAGES, block_layers, block_trainable  # noqa: E402
from tf_eager_object_detection_amd.model.fpn_detector import ResNetFpnDetector                        # noqa: E402
from tf_eager_object_detection_amd.model.layers import _stem                                          # noqa: E402
import neck_grad_bench as nb                                                                           # noqa: E402

HBM_PEAK = 8.0e12
CHANNELS = (256, 512, 1024, 2048)


def row_of(name, ours, yardstick, nbytes=None, **extra):
    row = nb.row_of(name, ours, yardstick, nbytes, **extra)
    if 'yardstick_over_ours' in row:
        row['verdict'] = 'MET' if row['yardstick_over_ours'] >= 1.0 else 'SLOWER'
    if nbytes:
        row['hbm_fraction'] = round(row['bytes_per_s'] / HBM_PEAK, 3)
    return row


def plain_block(blk, P, x):
    """the plain F.conv2d bottleneck on channels_last tensors; P: {parameter: leaf clone}"""
    w = lambda conv: (P[conv.weight], P[conv.bias])
    s = blk.c1.stride[0]
    a = F.relu(F.conv2d(x, *w(blk.c1), stride=s))
    b = F.relu(F.conv2d(a, *w(blk.c2), padding=1))
    y = F.conv2d(b, *w(blk.c3))
    return F.relu(y + (F.conv2d(x, *w(blk.short), stride=s) if blk.short is not None else x))


def leaves_of(blocks):
    params = [p for blk in blocks for conv in block_layers(blk) for p in (conv.weight, conv.bias)]
    return params, {p: p.detach().clone().requires_grad_() for p in params}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', help='output path (default profiles/extractor_grad_bench.json)')
    ap.add_argument('--image', type=int, nargs=2, default=(800, 1333))
    ap.add_argument('--depths', type=int, nargs='*', default=(50, 101))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    nb.STREAM = torch.cuda.Stream()
    nb.STREAM.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(nb.STREAM):
        out = measure(a)
    path = a.out or os.path.join(ROOT, 'profiles', 'extractor_grad_bench.json')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as fh:
        json.dump(out, fh, indent=1)
    print('wrote', path)


def measure(a):
    rng = np.random.default_rng(0)
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).cuda()
    shapes = [(-(-a.image[0] // s), -(-a.image[1] // s)) for s in (4, 8, 16, 32)]
    nchw = lambda t: t.permute(0, 3, 1, 2)
    rows = []
    # ---- the two new launches on each stage's map
    for k, ((H, W), C) in enumerate(zip(shapes, CHANNELS)):
        dy, y, d1 = f(1, H, W, C), f(1, H, W, C), f(1, H, W, C)
        zero = torch.zeros((), device='cuda')
        rows.append(row_of('join, identity form, %s map %dx%dx%d' % (STAGES[k], H, W, C), lambda: ops.block_input_grad(d1, dy=dy, y=y),
                           lambda: torch.where(y > 0, dy, zero) + d1, 4 * 4 * dy.numel()))
        if k == 3:
            continue
        # the first block of the NEXT stage reads this map at stride 2
        Ho, Wo = (H + 1) // 2, (W + 1) // 2
        g1, g2 = f(1, Ho, Wo, C), f(1, Ho, Wo, C)
        rows.append(row_of('stride-2 gather, %s input %dx%dx%d' % (STAGES[k + 1], H, W, C), lambda: ops.stride_gather(dy, 2),
                           lambda: dy[:, ::2, ::2].contiguous(), 4 * 2 * g1.numel()))

        def scatter():
            out = torch.zeros_like(dy)
            out[:, ::2, ::2] = g1 + g2
            return out

        rows.append(row_of('join, convolutional-shortcut form at stride 2, %s input %dx%dx%d' % (STAGES[k + 1], H, W, C),
                           lambda: ops.block_input_grad(g1, d2=g2, stride=2, in_hw=(H, W)), scatter, 4 * (2 * g1.numel() + dy.numel())))
        del dy, y, d1, g1, g2
    # ---- one identity block's backward per stage, and the whole extractor
    for depth in a.depths:
        torch.manual_seed(depth)
        det = ResNetFpnDetector(depth, 21, tuple(a.image), 1, dtype=torch.float32)
        det = det.to(device='cuda', dtype=torch.float32, memory_format=torch.channels_last).eval()
        img = f(1, a.image[0], a.image[1], 3) * 60
        with torch.no_grad():
            x0 = _stem(det.conv1, img, det.dtype)
            ins = [x0] + list(det.extractor(img))[:3]
        if depth == a.depths[0]:
            for k, name in enumerate(STAGES):
                blk = getattr(det, name)[1]
                with torch.no_grad():
                    x = getattr(det, name)[0](ins[k])
                params, P = leaves_of([blk])
                xo, xy = x.clone().requires_grad_(), x.clone().requires_grad_()
                yo, yy = block_trainable(blk, xo), plain_block(blk, P, xy)
                dy = nchw(f(*[yo.shape[i] for i in (0, 2, 3, 1)]))
                rows.append(row_of('one identity block backward (6 parameter gradients + dx), %s %dx%d' % ((name,) + shapes[k]),
                                   lambda: torch.autograd.grad(yo, [xo] + params, dy, retain_graph=True),
                                   lambda: torch.autograd.grad(yy, [xy] + list(P.values()), dy, retain_graph=True)))
                del yo, yy, xo, xy, dy
        blocks = [blk for name in STAGES for blk in getattr(det, name)]
        params, P = leaves_of(blocks)
        outs = det.extractor_trainable(img)
        t, pouts = x0, []
        for name in STAGES:
            for blk in getattr(det, name):
                t = plain_block(blk, P, t)
            pouts.append(t)
        douts = [nchw(f(*[o.shape[i] for i in (0, 2, 3, 1)])) for o in outs]
        rows.append(row_of('whole extractor backward, depth %d (%d parameter gradients)' % (depth, len(params)),
                           lambda: torch.autograd.grad(outs, params, douts, retain_graph=True),
                           lambda: torch.autograd.grad(pouts, list(P.values()), douts, retain_graph=True)))
        del outs, pouts, douts, det, P
        torch.cuda.empty_cache()
    slower = [r['launch'] for r in rows if r.get('verdict') == 'SLOWER']
    return dict(device=torch.cuda.get_device_name(0), image=list(a.image), levels=shapes,
                protocol='%d calls per HIP graph; ours / yardstick graphs replayed alternately, %d replays each after 3 warm-up replays; '
                         'median and [min, max] microseconds per call; tensors, autograd graphs and captures all on one side stream'
                         % (nb.INNER, nb.REPLAYS),
                expectation='ours not slower than the torch composition it replaces: MET or SLOWER per row',
                slower_than_yardstick=slower, rows=rows)


if __name__ == '__main__':
    main()
