#!/usr/bin/env python3
"""Times the split-precision gradient launches (csrc/grad_gemm.h: dg_tile_x3; ops.grad_form('x3')) against the exact-float32 form
of the same entry points and against the library composition tools/dense_grad_bench.py uses, on the same tensors; writes
profiles/grad_x3_bench.json.

  per launch   the FPN RoI head's fc1 / fc2 / final-layer wgrad (dw and db) and dgrad at 256 rows; the RpnHead's 3x3 wgrad and
               dgrad (256 -> 512) on the pyramid of an 800 x 1333 image.
               library: dz = dy * (y > 0), then dz.t() @ x and dz.sum(0), resp. dz @ w; the convolution's
               torch.nn.grad.conv2d_weight / conv2d_input per level.
  extractor    one identity bottleneck's backward per stage (conv2 .. conv5 at 800 x 1333) and the whole conv2..conv5 backward at
               depth 50, what .backward() enqueues captured in a HIP graph (the protocol of tools/extractor_grad_bench.py); library:
               torch autograd of the plain F.conv2d bottleneck with the same weights.
  whole model  ResnetV1Fpn depth 50 with the four train keywords at 800 x 1333: sum(losses).backward(), 'x3' against 'exact' --
               wall time between two device synchronisations, host work included (the losses' backward reads the host, so this
               one is not a graph): a lower bound on the ratio of GPU times.

Clock of the per-launch rows: GPU time of INNER calls captured in one HIP graph and replayed; the graphs of a row are replayed
alternately, REPLAYS times each, after 3 warm-up replays; median and (min, max) per call in microseconds.  A row where 'x3' is
slower than 'exact' or than the library is marked SLOWER.

    python tools/grad_x3_bench.py [--skip-model]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from tf_eager_object_detection_amd import ops                                            # noqa: E402
from dense_grad_bench import REPLAYS, INNER, alternate, capture                          # noqa: E402
import neck_grad_bench as nb                                                             # noqa: E402

PYRAMID = [(200, 334), (100, 167), (50, 84), (25, 42), (13, 21)]                        # 800 x 1333 at strides 4 .. 64


def in_form(form, fn):
    def run():
        with ops.grad_form(form):
            return fn()
    return run


def row(name, graphs, flops=None):
    out = dict(name=name)
    captured = {}
    for k, f in graphs.items():
        try:
            captured[k] = capture(f)
        except RuntimeError as e:                                # (a library call that cannot be captured: the row says so)
            if k != 'library':
                raise
            out['library_error'] = str(e).splitlines()[0][:200]
            torch.cuda.synchronize()
    t = alternate(captured)
    for k, (med, lo, hi) in t.items():
        out[k + '_us'] = round(med, 2)
        out[k + '_min_max_us'] = [round(lo, 2), round(hi, 2)]
    out['x3_over_exact'] = round(t['exact'][0] / t['x3'][0], 3)
    if 'library' in t:
        out['x3_over_library'] = round(t['library'][0] / t['x3'][0], 3)
    if flops:
        out['x3_tflops'] = round(flops / t['x3'][0] * 1e-6, 1)
    out['verdict'] = 'SLOWER' if min(out['x3_over_exact'], out.get('x3_over_library', 1.0)) < 1.0 else 'faster'
    print(json.dumps(out), flush=True)
    return out


def dense_rows(gen, layer, rows, cin, cout, relu):
    f = lambda *s: torch.randn(*s, generator=gen, device='cuda')
    x, w, dy = f(rows, cin), f(cout, cin), f(rows, cout)
    y = f(rows, cout) if relu else None
    gate = (lambda: dy * (y > 0)) if relu else (lambda: dy)

    def lib_wgrad():
        dz = gate()
        return dz.t() @ x, dz.sum(0)
    flops = 2.0 * rows * cin * cout
    return [row('%s wgrad %dx%dx%d' % (layer, rows, cin, cout),
                dict(x3=in_form('x3', lambda: ops.dense_wgrad(dy, x, y)), exact=in_form('exact', lambda: ops.dense_wgrad(dy, x, y)),
                     library=lib_wgrad), flops),
            row('%s dgrad %dx%dx%d' % (layer, rows, cin, cout),
                dict(x3=in_form('x3', lambda: ops.dense_dgrad(dy, w, y)), exact=in_form('exact', lambda: ops.dense_dgrad(dy, w, y)),
                     library=lambda: gate() @ w), flops)]


def rpn_rows(gen, cin=256, cout=512):
    f = lambda c: [torch.randn(1, h, w, c, generator=gen, device='cuda') for h, w in PYRAMID]
    xs, dys, ys = f(cin), f(cout), f(cout)
    w = torch.randn(cout, cin, 3, 3, generator=gen, device='cuda').contiguous(memory_format=torch.channels_last)
    wf = ops.conv3x3_flipped_weight(w)
    nchw = lambda t: t.permute(0, 3, 1, 2)
    dzs = [torch.where(y > 0, d, torch.zeros_like(d)) for y, d in zip(ys, dys)]

    def lib_wgrad():
        dw = None
        for x, d, y in zip(xs, dys, ys):
            dz = d * (y > 0)
            g = torch.nn.grad.conv2d_weight(nchw(x), w.shape, nchw(dz), padding=1)
            dw = g if dw is None else dw + g
        return dw
    pixels = sum(h * w_ for h, w_ in PYRAMID)
    flops = 2.0 * pixels * 9 * cin * cout
    return [row('rpn 3x3 wgrad %d->%d, %d pixels' % (cin, cout, pixels),
                dict(x3=in_form('x3', lambda: ops.conv3x3_wgrad_f32_levels(xs, dys, ys)),
                     exact=in_form('exact', lambda: ops.conv3x3_wgrad_f32_levels(xs, dys, ys)), library=lib_wgrad), flops),
            row('rpn 3x3 dgrad %d->%d, %d pixels' % (cin, cout, pixels),
                dict(x3=in_form('x3', lambda: ops.conv3x3_dgrad_f32_levels(dzs, w, flipped=wf)),
                     exact=in_form('exact', lambda: ops.conv3x3_dgrad_f32_levels(dzs, w, flipped=wf)),
                     library=lambda: [torch.nn.grad.conv2d_input(nchw(x).shape, w, nchw(d), padding=1) for x, d in zip(xs, dzs)]), flops)]


def autograd_row(name, fns):
    """a row whose three sides are autograd backward passes, captured as tools/neck_grad_bench.py captures them (everything on ONE
    side stream, nb.INNER calls per graph)"""
    t = nb.alternate({k: nb.capture(f) for k, f in fns.items()})
    out = dict(name=name)
    for k, (med, lo, hi) in t.items():
        out[k + '_us'] = round(med, 2)
        out[k + '_min_max_us'] = [round(lo, 2), round(hi, 2)]
    out['x3_over_exact'] = round(t['exact'][0] / t['x3'][0], 3)
    out['x3_over_library'] = round(t['library'][0] / t['x3'][0], 3)
    out['verdict'] = 'SLOWER' if min(out['x3_over_exact'], out['x3_over_library']) < 1.0 else 'faster'
    print(json.dumps(out), flush=True)
    return out


def extractor_rows(image=(800, 1333), depth=50):
    """one identity bottleneck's backward per stage (6 parameter gradients + dx: the 1x1 layers' dgrad / wgrad over pixels, the 3x3
    wgrad and input gradient) and the whole conv2..conv5 backward, in a HIP graph: the trainable block under grad_form 'x3' and
    'exact' (the form is recorded on the graph's nodes when it is built) against torch autograd of the plain F.conv2d bottleneck"""
    from extractor_grad_bench import leaves_of, plain_block
    from tf_eager_object_detection_amd.model.extractor_trainable import STAGES, block_trainable
    from tf_eager_object_detection_amd.model.fpn_detector import ResNetFpnDetector
    from tf_eager_object_detection_amd.model.layers import _stem
    rng = np.random.default_rng(0)
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).cuda()
    nchw = lambda t: t.permute(0, 3, 1, 2)
    rows = []
    torch.manual_seed(depth)
    det = ResNetFpnDetector(depth, 21, tuple(image), 1, dtype=torch.float32)
    det = det.to(device='cuda', dtype=torch.float32, memory_format=torch.channels_last).eval()
    img = f(1, image[0], image[1], 3) * 60
    with torch.no_grad():
        x0 = _stem(det.conv1, img, det.dtype)
        ins = [x0] + list(det.extractor(img))[:3]

    def grad_of(outs, leaves, douts):
        return lambda: torch.autograd.grad(outs, leaves, douts, retain_graph=True)
    for k, name in enumerate(STAGES):
        blk = getattr(det, name)[1]
        with torch.no_grad():
            x = getattr(det, name)[0](ins[k])
        params, P = leaves_of([blk])
        fns, keep = {}, []
        for form in ('x3', 'exact'):
            xi = x.clone().requires_grad_()
            with ops.grad_form(form):
                y = block_trainable(blk, xi)
            keep.append((xi, y))
        dy = nchw(f(*[keep[0][1].shape[i] for i in (0, 2, 3, 1)]))
        xl = x.clone().requires_grad_()
        fns = {'x3': grad_of(keep[0][1], [keep[0][0]] + params, dy), 'exact': grad_of(keep[1][1], [keep[1][0]] + params, dy),
               'library': grad_of(plain_block(blk, P, xl), [xl] + list(P.values()), dy)}
        rows.append(autograd_row('one identity block backward, %s %dx%d, %d channels' % (name, x.shape[2], x.shape[3], x.shape[1]), fns))
        del fns, keep, dy, xl
    blocks = [blk for name in STAGES for blk in getattr(det, name)]
    params, P = leaves_of(blocks)
    outs = {}
    for form in ('x3', 'exact'):
        det.grad_form = form
        outs[form] = det.extractor_trainable(img)
    det.grad_form = 'exact'
    t, pouts = x0, []
    for name in STAGES:
        for blk in getattr(det, name):
            t = plain_block(blk, P, t)
        pouts.append(t)
    douts = [nchw(f(*[o.shape[i] for i in (0, 2, 3, 1)])) for o in outs['x3']]
    rows.append(autograd_row('whole extractor backward conv2..conv5, depth %d (%d parameter gradients)' % (depth, len(params)),
                             {'x3': grad_of(outs['x3'], params, douts), 'exact': grad_of(outs['exact'], params, douts),
                              'library': grad_of(pouts, list(P.values()), douts)}))
    return rows


def model_row(steps=5):
    from tf_eager_object_detection_amd.model.base_fpn_model import ResnetV1Fpn
    kw = dict(depth=50, train_roi_head=True, train_rpn_head=True, train_neck=True, train_extractor=True, training_targets='hip',
              training_losses='hip')
    torch.manual_seed(0)
    models = {'exact': ResnetV1Fpn(**kw)}
    models['x3'] = ResnetV1Fpn(grad_form='x3', **kw)
    models['x3']._dense_ref.load_state_dict(models['exact']._dense_ref.state_dict())
    rng = np.random.default_rng(0)
    img = torch.from_numpy((rng.uniform(0, 255, (1, 800, 1333, 3)) - 110).astype(np.float32)).cuda()
    inputs = (img, torch.tensor([[100.0, 120.0, 500.0, 640.0], [300.0, 200.0, 700.0, 1100.0]], device='cuda'),
              torch.tensor([3, 12], device='cuda'))
    ts = {k: [] for k in models}
    for i in range(steps + 2):
        for k, m in models.items():
            m.dense.zero_grad(set_to_none=True)
            loss = sum(m(inputs, training=True))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss.backward()
            torch.cuda.synchronize()
            if i >= 2:
                ts[k].append((time.perf_counter() - t0) * 1e3)
    out = dict(name='ResnetV1Fpn-50 whole backward, 800 x 1333 (wall ms between synchronisations)',
               x3_ms=round(float(np.median(ts['x3'])), 2), exact_ms=round(float(np.median(ts['exact'])), 2))
    out['x3_over_exact'] = round(out['exact_ms'] / out['x3_ms'], 3)
    out['verdict'] = 'SLOWER' if out['x3_over_exact'] < 1.0 else 'faster'
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--skip-model', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'grad_x3_bench.json'))
    a = ap.parse_args()
    gen = torch.Generator(device='cuda').manual_seed(0)
    rows = []
    for layer, shape, relu in (('fc1', (256, 12544, 1024), True), ('fc2', (256, 1024, 1024), True), ('final', (256, 1024, 128), False)):
        rows += dense_rows(gen, layer, *shape, relu)
    rows += rpn_rows(gen)
    nb.STREAM = torch.cuda.Stream()
    nb.STREAM.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(nb.STREAM):
        rows += extractor_rows()
    torch.cuda.current_stream().wait_stream(nb.STREAM)
    torch.cuda.empty_cache()
    if not a.skip_model:
        rows.append(model_row())
    out = dict(device=torch.cuda.get_device_name(0), rows=rows,
               protocol='%d calls per HIP graph; the x3 / exact / library graphs of a row replayed alternately, %d replays each after 3 '
                        'warm-up replays; ratios are medians, other form over x3 (above 1: x3 is faster)' % (INNER, REPLAYS))
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print('wrote', a.out)


if __name__ == '__main__':
    main()
