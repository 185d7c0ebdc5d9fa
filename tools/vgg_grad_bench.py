#!/usr/bin/env python3
"""Times the VGG16 training graph's two new launches (csrc/vgg_grad.hip) on the 600 x 800 image's shapes and the whole dense backward
of one training call, batch 1, against the torch composition on the same float32 tensors; writes profiles/vgg_grad_bench.json.

  ours       ops.relu_maxpool2_backward on block3_pool's and block4_pool's inputs (150 x 200 x 256, 75 x 100 x 512), ops.dropout /
             ops.dropout_backward on the head's 128 x 4096 activations; for the whole pass torch.autograd.grad through
             Vgg16Detector.extractor_trainable, rpn_trainable and roi_head_trainable(keep_prob 0.5): the 32 parameter gradients.
  yardstick  the pooling: autograd's backward of F.max_pool2d(F.relu(z + b), 2, 2, ceil_mode=True) with respect to z (channels_last
             tensors, the graph built once); dropout: F.dropout(x, 0.5) forward, dy * mask * (1 / keep_prob) on the stored mask
             backward; the whole pass: autograd over F.conv2d / F.max_pool2d / F.linear / the mask multiply (the library's
             convolutions and GEMMs) with the same shapes, parameters and output gradients.
  The RoI pooling and the losses are not part of the whole-pass row: their backward is the same launch on either side (torch has
  no such operator), so the row starts from gradients at the head's outputs, the RpnHead's outputs and the shared map.

Clock: GPU time of INNER calls captured in one HIP graph and replayed; per row the two graphs are replayed alternately, REPLAYS
times each, after 3 warm-up replays; median and (min, max) per call in microseconds.  `bytes_per_s`: the bytes the algorithm needs
(pooling: z read, dz written, dpool read = 4 (2 H W + OH OW) C; dropout: one read, one write) over the median, next to the 8 TB/s HBM
figure.  Every row says MET or SLOWER against its yardstick.

    python tools/vgg_grad_bench.py"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tf_eager_object_detection_amd import ops                                            # noqa: E402
from tf_eager_object_detection_amd.model.frcnn_detector import Vgg16Detector            # noqa: E402

REPLAYS = 30
HBM_BYTES_PER_S = 8.0e12
SEED, IMAGE_ID = 11, 0

STREAM = None        # main(): everything runs on ONE side stream, so that autograd's backward (which runs on the stream of its
                     # forward) is on the capturing stream


def capture(fn, inner):
    fn()
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=STREAM):
        for _ in range(inner):
            fn()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    return g


def alternate(graphs, inner):
    """{name: graph} -> {name: (median, min, max)} microseconds per call, the graphs replayed in turn"""
    ts = {k: [] for k in graphs}
    for _ in range(REPLAYS):
        for k, g in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            torch.cuda.synchronize()
            ts[k].append(a.elapsed_time(b) * 1e3 / inner)
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in ts.items()}


def row_of(name, ours, yardstick, nbytes=None, inner=10, **extra):
    graphs = {'ours': capture(ours, inner)}
    note = None
    try:
        graphs['yardstick'] = capture(yardstick, inner)
    except Exception as e:                                                                # torch refuses the capture
        note = 'yardstick: %s: %s' % (type(e).__name__, str(e).splitlines()[0][:200])
        torch.cuda.synchronize()
    t = alternate(graphs, inner)
    row = dict(launch=name, calls_per_graph=inner, **extra)
    for k, v in t.items():
        row[k + '_us'] = round(v[0], 2)
        row[k + '_range_us'] = [round(v[1], 2), round(v[2], 2)]
    if 'yardstick' in t:
        row['yardstick_over_ours'] = round(t['yardstick'][0] / t['ours'][0], 3)
        row['verdict'] = 'MET' if t['ours'][0] <= t['yardstick'][0] else 'SLOWER'
    if note:
        row['yardstick_note'] = note
    if nbytes:
        row['algorithmic_bytes'] = int(nbytes)
        row['tbytes_per_s'] = round(nbytes / t['ours'][0] / 1e6, 3)
        row['share_of_hbm_figure'] = round(nbytes / t['ours'][0] * 1e6 / HBM_BYTES_PER_S, 4)
    print(json.dumps(row), flush=True)
    return row


def pool_row(f, H, W, C):
    OH, OW = (H + 1) // 2, (W + 1) // 2
    z, bias, dpool = f(1, H, W, C), f(C), f(1, OH, OW, C)
    zt = z.permute(0, 3, 1, 2).detach().requires_grad_()                                  # channels_last, as torch would hold it
    y = F.max_pool2d(F.relu(zt + bias.view(1, -1, 1, 1)), 2, 2, ceil_mode=True)
    g = dpool.permute(0, 3, 1, 2)
    return row_of('relu_maxpool2_backward %dx%dx%d' % (H, W, C), lambda: ops.relu_maxpool2_backward(z, bias, dpool),
                  lambda: torch.autograd.grad(y, zt, g, retain_graph=True), 4 * (2 * H * W + OH * OW) * C)


def dropout_rows(f, rows, cols):
    x, dy = f(rows, cols), f(rows, cols)
    mask = (torch.rand(rows, cols, device='cuda') < 0.5).float()
    nbytes = 4 * 2 * rows * cols
    return [row_of('dropout %dx%d' % (rows, cols), lambda: ops.dropout(x, 0.5, SEED, IMAGE_ID, ops.DROPOUT_STREAM_FC1),
                   lambda: F.dropout(x, 0.5, training=True), nbytes),
            row_of('dropout_backward %dx%d' % (rows, cols), lambda: ops.dropout_backward(dy, 0.5, SEED, IMAGE_ID, ops.DROPOUT_STREAM_FC1),
                   lambda: dy * mask * 2.0, nbytes, yardstick_reads_a_stored_mask=True)]


def whole_pass_row(f, image, rois):
    """the dense backward of one training call: block3_conv1 .. block5_conv3 with the two poolings, the RpnHead, the RoI head with
    its dropouts -- 32 parameter gradients on either side"""
    det = Vgg16Detector(21, image, 1, dtype=torch.float32).to(device='cuda', dtype=torch.float32, memory_format=torch.channels_last).eval()
    img = f(1, image[0], image[1], 3) * 50.0
    feats = f(rois, 7, 7, 512).relu_()
    # ours: the graph through the three trainable parts, built once
    c = det.extractor_trainable(img)
    s, d = det.rpn_trainable(c)
    logits, bbox = det.roi_head_trainable(feats, 0.5, SEED, IMAGE_ID)
    outs = [c, s, d, logits, bbox]
    gouts = [f(*t.shape) * 1e-3 for t in outs]
    gouts[0] = gouts[0].contiguous(memory_format=torch.channels_last)
    params = [p for n, p in det.named_parameters() if not n.startswith(('convs.0.', 'convs.1.', 'convs.2.', 'convs.3.'))]
    assert len(params) == 32
    # the yardstick: the plain torch formulation on copies of the same parameters
    P = {n: p.detach().clone().requires_grad_() for n, p in det.named_parameters()}
    with torch.no_grad():
        x = det._first_conv(img)
        for i, pooled in det._layer_plan():
            if i < 4:
                x = det._layer(i, pooled, x)
    for i, pooled in det._layer_plan():
        if i < 4:
            continue
        x = F.relu(F.conv2d(x, P['convs.%d.weight' % i], P['convs.%d.bias' % i], padding=1))
        if pooled:
            x = F.max_pool2d(x, 2, 2, ceil_mode=True)
    h = F.relu(F.conv2d(x, P['rpn_conv.weight'], P['rpn_conv.bias'], padding=1))
    ys = F.conv2d(h, P['rpn_score.weight'], P['rpn_score.bias']).permute(0, 2, 3, 1).reshape(s.shape)
    yd = F.conv2d(h, P['rpn_bbox.weight'], P['rpn_bbox.bias']).permute(0, 2, 3, 1).reshape(d.shape)
    m1 = (torch.rand(rois, 4096, device='cuda') < 0.5).float() * 2.0
    m2 = (torch.rand(rois, 4096, device='cuda') < 0.5).float() * 2.0
    a = F.relu(F.linear(feats.reshape(rois, -1), P['fc1.weight'], P['fc1.bias'])) * m1
    a = F.relu(F.linear(a, P['fc2.weight'], P['fc2.bias'])) * m2
    youts = [x, ys, yd, F.linear(a, P['score.weight'], P['score.bias']), F.linear(a, P['bbox.weight'], P['bbox.bias'])]
    leaves = [p for n, p in P.items() if not n.startswith(('convs.0.', 'convs.1.', 'convs.2.', 'convs.3.'))]
    return row_of('whole dense backward (32 parameter gradients), %dx%d image, %d RoIs' % (image + (rois,)),
                  lambda: torch.autograd.grad(outs, params, gouts, retain_graph=True),
                  lambda: torch.autograd.grad(youts, leaves, gouts, retain_graph=True), inner=2)


def measure(a):
    rng = np.random.default_rng(0)
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).cuda()
    H, W = a.image
    rows = [pool_row(f, -(-H // 4), -(-W // 4), 256), pool_row(f, -(-H // 8), -(-W // 8), 512)]
    rows += dropout_rows(f, a.rois, 4096)
    rows.append(whole_pass_row(f, tuple(a.image), a.rois))
    slower = [r['launch'] for r in rows if r.get('verdict') == 'SLOWER']
    return dict(device=torch.cuda.get_device_name(0), image=list(a.image), rois=a.rois,
                protocol='calls_per_graph calls per HIP graph; ours / yardstick graphs replayed alternately, %d replays each after 3 '
                         'warm-up replays; median and [min, max] microseconds per call; tensors, autograd graphs and captures all on '
                         'one side stream' % REPLAYS,
                hbm_figure_bytes_per_s=HBM_BYTES_PER_S, slower_than_yardstick=slower, rows=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', help='output path (default profiles/vgg_grad_bench.json)')
    ap.add_argument('--image', type=int, nargs=2, default=(600, 800))
    ap.add_argument('--rois', type=int, default=128)
    a = ap.parse_args()
    global STREAM
    torch.cuda.set_device(0)
    STREAM = torch.cuda.Stream()
    STREAM.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(STREAM):
        out = measure(a)
    path = a.out or os.path.join(ROOT, 'profiles', 'vgg_grad_bench.json')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as fh:
        json.dump(out, fh, indent=1)
    print('wrote', path)


if __name__ == '__main__':
    main()
