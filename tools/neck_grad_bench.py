#!/usr/bin/env python3
"""Times the FPN neck's backward launches (csrc/neck.hip odet_fpn_topdown_backward_f32, csrc/conv_grad.hip, csrc/dense_grad.hip over
pixels) on the 800 x 1333 pyramid at batch 1 (C2..C5 = 200x334, 100x167, 50x84, 25x42), and the whole neck backward, against torch
autograd on the same float32 tensors; writes profiles/neck_grad_bench.json.

  ours       merge backward: ops.fpn_topdown_backward per coarse level (the resize's transpose + base (+ sub) + scale, one launch);
             s_k: ops.conv3x3_wgrad_f32_levels and ops.conv3x3_dgrad_f32_levels on the cached flipped weight (s2's halved); 1x1
             layers: ops.dense_wgrad over pixels; whole neck: everything .backward() of neck_trainable enqueues.
  yardstick  torch autograd: for the merge alone the backward of layers.tf_legacy_resize_bilinear (the gradient with respect
             to the coarse map ONLY: no base, no scale -- less work than ours does in the launch); for the whole neck the backward
             of tf_legacy_resize_bilinear + F.conv2d on channels_last tensors (parameter gradients, no gradient into C2..C5).  The
             autograd graph is built once outside the capture, on the stream that captures (autograd runs a backward on its
             forward's stream); the captured part is the backward alone.

Clock: GPU time of INNER calls captured in one HIP graph and replayed; per row the graphs are replayed alternately, REPLAYS times
each, after 3 warm-up replays; median and (min, max) per call in microseconds.  `bytes_per_s` of the merge backward: its
ALGORITHMIC bytes (fine + base + d_top, each once) over the median time.

    python tools/neck_grad_bench.py"""
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
from tf_eager_object_detection_amd.model.layers import tf_legacy_resize_bilinear   # noqa: E402

INNER, REPLAYS = 3, 30
TOP = 256
CINS = (256, 512, 1024, 2048)


STREAM = None        # main(): everything runs on ONE side stream, so that autograd's backward (which runs on the stream of its
                     # forward) is on the capturing stream


def capture(fn):
    fn()
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=STREAM):
        for _ in range(INNER):
            fn()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    return g


def alternate(graphs):
    """{name: graph} -> {name: (median, min, max)} microseconds per call, the graphs replayed in turn"""
    ts = {k: [] for k in graphs}
    for _ in range(REPLAYS):
        for k, g in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            torch.cuda.synchronize()
            ts[k].append(a.elapsed_time(b) * 1e3 / INNER)
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in ts.items()}


def row_of(name, ours, yardstick, nbytes=None, **extra):
    graphs = {'ours': capture(ours)}
    note = None
    if yardstick is not None:
        try:
            graphs['yardstick'] = capture(yardstick)
        except Exception as e:                                                            # torch refuses the capture
            note = 'yardstick: %s: %s' % (type(e).__name__, str(e).splitlines()[0][:200])
            torch.cuda.synchronize()
    t = alternate(graphs)
    row = dict(launch=name, **extra)
    for k, v in t.items():
        row[k + '_us'] = round(v[0], 2)
        row[k + '_range_us'] = [round(v[1], 2), round(v[2], 2)]
    if 'yardstick' in t:
        row['yardstick_over_ours'] = round(t['yardstick'][0] / t['ours'][0], 3)
    if note:
        row['yardstick_note'] = note
    if nbytes:
        row['algorithmic_bytes'] = int(nbytes)
        row['bytes_per_s'] = round(nbytes / t['ours'][0] * 1e6, 1)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', help='output path (default profiles/neck_grad_bench.json)')
    ap.add_argument('--image', type=int, nargs=2, default=(800, 1333))
    a = ap.parse_args()
    global STREAM
    torch.cuda.set_device(0)
    STREAM = torch.cuda.Stream()
    STREAM.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(STREAM):
        out = measure(a)
    path = a.out or os.path.join(ROOT, 'profiles', 'neck_grad_bench.json')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as fh:
        json.dump(out, fh, indent=1)
    print('wrote', path)


def measure(a):
    rng = np.random.default_rng(0)
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).cuda()
    shapes = [(-(-a.image[0] // s), -(-a.image[1] // s)) for s in (4, 8, 16, 32)]
    h6 = ((shapes[3][0] + 1) // 2, (shapes[3][1] + 1) // 2)
    cs = [f(1, h, w, c) for (h, w), c in zip(shapes, CINS)]                              # NHWC
    ms = [f(1, h, w, TOP) for h, w in shapes[:3]]
    dps = [f(1, h, w, TOP) for h, w in shapes + [h6]]
    w1 = {n: f(TOP, c) * 0.02 for n, c in zip(('l2', 'l3', 'l4', 'p5'), CINS)}
    w3 = {n: (f(TOP, TOP, 3, 3) * 0.02).contiguous(memory_format=torch.channels_last) for n in ('s2', 's3', 's4')}
    flip = {n: ops.conv3x3_flipped_weight(w) for n, w in w3.items()}
    flip['s2'] = flip['s2'] * 0.5
    dm = [ops.conv3x3_dgrad_f32_levels([dps[i]], w3[n], flipped=flip[n])[0] for i, n in enumerate(('s2', 's3', 's4'))]
    hs = [dm[0], ops.fpn_topdown_backward(dm[0], shapes[1], base=dm[1], out_scale=0.5)]
    hs.append(ops.fpn_topdown_backward(hs[1], shapes[2], base=dm[2], out_scale=0.5))
    hs.append(ops.fpn_topdown_backward(hs[2], shapes[3], base=dps[3], sub=dps[4], out_scale=1.0))
    nchw = lambda t: t.permute(0, 3, 1, 2)
    torch.cuda.synchronize()
    print('inputs ready: levels %s' % (shapes,), flush=True)

    def resize_backward(fine, top_hw):
        z = torch.zeros((1, TOP) + tuple(top_hw), device='cuda').contiguous(memory_format=torch.channels_last).requires_grad_()
        y = tf_legacy_resize_bilinear(z, fine.shape[1:3])
        return lambda: torch.autograd.grad(y, z, nchw(fine), retain_graph=True)

    rows = []
    for k, (fine, base, sub, scale) in enumerate(((hs[0], dm[1], None, 0.5), (hs[1], dm[2], None, 0.5), (hs[2], dps[3], dps[4], 1.0))):
        top_hw = shapes[k + 1]
        nbytes = 4 * (fine.numel() + 2 * base.numel())
        rows.append(row_of('merge backward %dx%d -> %dx%d%s' % (tuple(fine.shape[1:3]) + tuple(top_hw) + (' (+ sub)' if sub is not None else '',)),
                           lambda: ops.fpn_topdown_backward(fine, top_hw, base=base, sub=sub, out_scale=scale),
                           resize_backward(fine, top_hw), nbytes))
    for i, n in enumerate(('s2', 's3', 's4')):
        rows.append(row_of('%s wgrad (dw + db) %dx%d' % ((n,) + shapes[i]), lambda: ops.conv3x3_wgrad_f32_levels([ms[i]], [dps[i]]), None))
        rows.append(row_of('%s dgrad %dx%d' % ((n,) + shapes[i]), lambda: ops.conv3x3_dgrad_f32_levels([dps[i]], w3[n], flipped=flip[n]), None))
    for i, n in enumerate(('l2', 'l3', 'l4', 'p5')):
        rows.append(row_of('%s wgrad (dw + db) %dx%d, %d channels' % ((n,) + shapes[i] + (CINS[i],)),
                           lambda: ops.dense_wgrad(hs[i].view(-1, TOP), cs[i].view(-1, CINS[i])), None))

    def ours_neck():
        out, d = [], {}
        for i, n in enumerate(('s2', 's3', 's4')):
            out.append(ops.conv3x3_wgrad_f32_levels([ms[i]], [dps[i]]))
            d[n] = ops.conv3x3_dgrad_f32_levels([dps[i]], w3[n], flipped=flip[n])[0]
        h = [d['s2']]
        h.append(ops.fpn_topdown_backward(h[0], shapes[1], base=d['s3'], out_scale=0.5))
        h.append(ops.fpn_topdown_backward(h[1], shapes[2], base=d['s4'], out_scale=0.5))
        h.append(ops.fpn_topdown_backward(h[2], shapes[3], base=dps[3], sub=dps[4], out_scale=1.0))
        for i in range(4):
            out.append(ops.dense_wgrad(h[i].view(-1, TOP), cs[i].view(-1, CINS[i])))
        return out

    # the yardstick's neck: float32 autograd of the plain formulation, the graph built once
    P = {n: w.view(TOP, -1, 1, 1).clone().requires_grad_() for n, w in w1.items()}
    P.update({n: w.clone().requires_grad_() for n, w in w3.items()})
    Bz = {n: torch.zeros(TOP, device='cuda', requires_grad=True) for n in P}
    xc = [nchw(c) for c in cs]
    p5 = F.conv2d(xc[3], P['p5'], Bz['p5'])
    m4 = 0.5 * tf_legacy_resize_bilinear(p5, shapes[2]) + 0.5 * F.conv2d(xc[2], P['l4'], Bz['l4'])
    m3 = 0.5 * tf_legacy_resize_bilinear(m4, shapes[1]) + 0.5 * F.conv2d(xc[1], P['l3'], Bz['l3'])
    m2 = 0.5 * tf_legacy_resize_bilinear(m3, shapes[0]) + 0.5 * F.conv2d(xc[0], P['l2'], Bz['l2'])
    outs = [F.conv2d(m2, P['s2'], Bz['s2'], padding=1), F.conv2d(m3, P['s3'], Bz['s3'], padding=1),
            F.conv2d(m4, P['s4'], Bz['s4'], padding=1), p5, p5[:, :, ::2, ::2]]
    leaves = list(P.values()) + list(Bz.values())
    gouts = [nchw(d) for d in dps]
    rows.append(row_of('whole neck backward (14 parameter gradients)', ours_neck,
                       lambda: torch.autograd.grad(outs, leaves, gouts, retain_graph=True)))
    slower = [r['launch'] for r in rows if r.get('yardstick_over_ours', 1.0) < 1.0]
    return dict(device=torch.cuda.get_device_name(0), image=list(a.image), levels=shapes,
                protocol='%d calls per HIP graph; ours / yardstick graphs replayed alternately, %d replays each after 3 warm-up replays; '
                         'median and [min, max] microseconds per call; tensors, autograd graphs and captures all on one side stream'
                         % (INNER, REPLAYS),
                slower_than_yardstick=slower, rows=rows)


if __name__ == '__main__':
    main()
