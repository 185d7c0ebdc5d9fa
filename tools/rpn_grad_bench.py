#!/usr/bin/env python3
"""Times the FPN RpnHead's backward launches (csrc/conv_grad.hip, csrc/dense_grad.hip over pixels, odet_rpn_unpack_pair) on the
800 x 1333 pyramid at batch 1, and the whole head backward, against the library's convolution backward on the same float32
tensors; writes profiles/rpn_grad_bench.json.

  ours     conv3x3 wgrad: ops.conv3x3_wgrad_f32_levels (main launch + the parts' reduce + the bias sums, all five levels in one
           call); conv3x3 dgrad: ops.conv3x3_dgrad_f32_levels (the forward kernel on the cached flipped weight); pair wgrad /
           dgrad: ops.dense_wgrad / ops.dense_dgrad(x_relu = h) over all pixels; unpack: five ops.rpn_unpack_pair.
  library  what torch autograd runs for F.conv2d + relu + the two 1x1 convolutions: aten.convolution_backward per level (weight
           and bias gradient, resp. input gradient) on channels_last views of the same memory, the levels' results added; the
           pair as matrix products with the elementwise gate.  When the library refuses the configuration the row says so and
           ours is timed alone.
  head     everything .backward() of rpn_trainable enqueues, with and without the input gradient, against the same chain.

Clock: GPU time of INNER calls captured in one HIP graph and replayed; per row the graphs are replayed alternately, REPLAYS times
each, after 3 warm-up replays; median and (min, max) per call in microseconds.  `tflops` (2 * pixels * 9 cin * cout for the 3x3
launches) stands next to the 157.3 TFLOP/s float32 matrix peak.

    python tools/rpn_grad_bench.py"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tf_eager_object_detection_amd import ops                                            # noqa: E402

INNER, REPLAYS = 3, 30
F32_MATRIX_FLOPS = 157.3e12
A, CIN, CMID, PAD = 3, 256, 512, 64


def capture(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
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


def row_of(name, ours, library, flops=None, **extra):
    graphs = {'ours': capture(ours)}
    note = None
    if library is not None:
        try:
            graphs['library'] = capture(library)
        except Exception as e:                                                            # the library refuses the configuration
            note = 'library: %s: %s' % (type(e).__name__, str(e).splitlines()[0][:200])
            torch.cuda.synchronize()
    t = alternate(graphs)
    row = dict(launch=name, **extra)
    for k, v in t.items():
        row[k + '_us'] = round(v[0], 2)
        row[k + '_range_us'] = [round(v[1], 2), round(v[2], 2)]
    if 'library' in t:
        row['library_over_ours'] = round(t['library'][0] / t['ours'][0], 3)
    if note:
        row['library_note'] = note
    if flops:
        row['tflops'] = round(flops / t['ours'][0] / 1e6, 2)
        row['share_of_f32_matrix_peak'] = round(flops / t['ours'][0] * 1e6 / F32_MATRIX_FLOPS, 4)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', help='output path (default profiles/rpn_grad_bench.json)')
    ap.add_argument('--image', type=int, nargs=2, default=(800, 1333))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    rng = np.random.default_rng(0)
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).cuda()
    shapes = [(-(-a.image[0] // s), -(-a.image[1] // s)) for s in (4, 8, 16, 32, 64)]
    pixels = [h * w for h, w in shapes]
    P, N = sum(pixels), sum(pixels) * A
    xs = [f(1, h, w, CIN) for h, w in shapes]
    hbuf = f(P, CMID).relu_()
    w3 = (f(CMID, CIN, 3, 3) * 0.01).contiguous(memory_format=torch.channels_last)
    wflip = ops.conv3x3_flipped_weight(w3)
    wpad = f(PAD, CMID) * 0.01
    wpad[6 * A:] = 0
    ds, dd = f(1, N, 2), f(1, N, 4)
    dpair = torch.empty((P, PAD), device='cuda')
    dh = f(P, CMID) * (hbuf > 0)

    def views(buf):
        out, off = [], 0
        for (h, w), n in zip(shapes, pixels):
            out.append(buf[off:off + n].view(1, h, w, -1))
            off += n
        return out
    dhs = views(dh)
    nchw = lambda t: t.permute(0, 3, 1, 2)
    cb = torch.ops.aten.convolution_backward

    def unpack():
        off = aoff = 0
        for n in pixels:
            ops.rpn_unpack_pair(ds, dd, A, n, aoff, dpair[off:off + n])
            off += n
            aoff += n * A
    unpack()

    def lib_conv(mask):
        return [cb(nchw(g), nchw(x), w3, [CMID], [1, 1], [1, 1], [1, 1], False, [0, 0], 1, mask) for g, x in zip(dhs, xs)]

    def lib_wgrad():
        got = lib_conv([False, True, True])
        dw, db = got[0][1], got[0][2]
        for g in got[1:]:
            dw, db = dw + g[1], db + g[2]
        return dw, db

    def lib_pair_dgrad(g=None):
        return ((dpair[:, :6 * A] if g is None else g) @ wpad[:6 * A]) * (hbuf > 0)

    def ours_head(with_dx):
        unpack()
        out = [ops.dense_wgrad(dpair, hbuf), ops.conv3x3_wgrad_f32_levels(xs, views(ops.dense_dgrad(dpair, wpad, x_relu=hbuf)))]
        if with_dx:
            out.append(ops.conv3x3_dgrad_f32_levels(dhs, w3, flipped=wflip))
        return out

    def lib_head(with_dx):
        g = dpair[:, :6 * A]
        out = [g.t() @ hbuf, g.sum(0)]
        dz = views(lib_pair_dgrad(g))
        got = [cb(nchw(d), nchw(x), w3, [CMID], [1, 1], [1, 1], [1, 1], False, [0, 0], 1, [with_dx, True, True]) for d, x in zip(dz, xs)]
        dw, db = got[0][1], got[0][2]
        for t in got[1:]:
            dw, db = dw + t[1], db + t[2]
        return out + [dw, db] + [t[0] for t in got]

    conv_flops = 2.0 * P * 9 * CIN * CMID
    lv = (ops.L.OdetConvGradLevel * len(shapes))()
    for i, (h, w) in enumerate(shapes):
        lv[i].H, lv[i].W = h, w
    parts = int(ops.L.lib().odet_conv3x3_wgrad_workspace_bytes(lv, len(shapes), 1, CIN, CMID)) // (CMID * 9 * CIN * 4)
    rows = [
        row_of('conv3x3 wgrad (dw + db, five levels)', lambda: ops.conv3x3_wgrad_f32_levels(xs, dhs), lib_wgrad, conv_flops, parts=parts),
        row_of('conv3x3 wgrad, dw alone', lambda: ops.conv3x3_wgrad_f32_levels(xs, dhs, with_bias=False), None, conv_flops),
        row_of('conv3x3 dgrad (five levels)', lambda: ops.conv3x3_dgrad_f32_levels(dhs, w3, flipped=wflip),
               lambda: lib_conv([True, False, False]), conv_flops),
        row_of('pair wgrad (dw + db)', lambda: ops.dense_wgrad(dpair, hbuf),
               lambda: (dpair[:, :6 * A].t() @ hbuf, dpair[:, :6 * A].sum(0)), 2.0 * P * PAD * CMID),
        row_of('pair dgrad + gate', lambda: ops.dense_dgrad(dpair, wpad, x_relu=hbuf), lib_pair_dgrad, 2.0 * P * PAD * CMID),
        row_of('unpack (five launches)', unpack, None),
        row_of('whole head backward, no input gradient', lambda: ours_head(False), lambda: lib_head(False)),
        row_of('whole head backward, with input gradient', lambda: ours_head(True), lambda: lib_head(True)),
    ]
    slower = [r['launch'] for r in rows if r.get('library_over_ours', 1.0) < 1.0]
    out = dict(device=torch.cuda.get_device_name(0), image=list(a.image), levels=shapes, pixels=P,
               protocol='%d calls per HIP graph; ours / library graphs replayed alternately, %d replays each after 3 warm-up replays; '
                        'median and [min, max] microseconds per call' % (INNER, REPLAYS),
               f32_matrix_peak_flops=F32_MATRIX_FLOPS, slower_than_library=slower, rows=rows)
    path = a.out or os.path.join(ROOT, 'profiles', 'rpn_grad_bench.json')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as fh:
        json.dump(out, fh, indent=1)
    print('wrote', path)


if __name__ == '__main__':
    main()
