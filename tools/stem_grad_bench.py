#!/usr/bin/env python3
"""Times the FPN stem's backward (csrc/stem_grad.hip, ops.stem_trainable) at the stem shapes of an 800 x 1333 image, batch 1,
against the torch composition on the same float32 tensors, and the whole ResnetV1Fpn-50 training call with and without train_stem;
writes profiles/stem_grad_bench.json.

  ours       ops.relu_maxpool3_backward on the 400 x 667 x 64 raw convolution output; ops.stem_patches_f32 + ops.dense_wgrad
             (the patch matrix built again, then conv1's weight and bias gradient); the whole stem backward: torch.autograd.grad
             through ops.stem_trainable into conv1's weight and bias.
  yardstick  the pooling: autograd's backward of F.max_pool2d(F.relu(z + b), 3, 2, 1) on the same tensor, channels_last as
             torch would hold it; the whole stem: autograd over F.conv2d(7x7 / 2, pad 3) + relu + max_pool2d (the library's
             convolution) into the same two parameters.  The patch recompute + dense_wgrad row has the convolution's own
             weight-gradient as its yardstick: autograd over F.conv2d alone, with the same dz.
  floor      the pooling backward's algorithmic bytes (z and dpool read once, dz written once) over the 8 TB/s HBM figure.

Clock of the graph rows: tools/vgg_grad_bench.py's -- GPU time of INNER calls captured in one HIP graph, ours and the yardstick
replayed alternately, median and (min, max) per call in microseconds.  Every row with a yardstick says MET or SLOWER.  The training
calls: wall time around eager calls, synchronised; the run with the keyword off is timed TWICE, and the spread between those two
runs stands next to both figures.

    python tools/stem_grad_bench.py"""
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
from tf_eager_object_detection_amd import ops                                            # noqa: E402
from tf_eager_object_detection_amd.model.base_fpn_model import ResnetV1Fpn              # noqa: E402
from tools.vgg_grad_bench import REPLAYS, HBM_BYTES_PER_S                                # noqa: E402
import tools.vgg_grad_bench as common                                                    # noqa: E402


def pool_row(f, H, W, C):
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    z, bias, dpool = f(1, H, W, C), f(C), f(1, OH, OW, C)
    zt = z.permute(0, 3, 1, 2).detach().requires_grad_()                                  # channels_last, as torch would hold it
    y = F.max_pool2d(F.relu(zt + bias.view(1, -1, 1, 1)), 3, 2, 1)
    g = dpool.permute(0, 3, 1, 2)
    nbytes = 4 * (2 * H * W + OH * OW) * C
    row = common.row_of('relu_maxpool3_backward %dx%dx%d' % (H, W, C), lambda: ops.relu_maxpool3_backward(z, bias, dpool),
                        lambda: torch.autograd.grad(y, zt, g, retain_graph=True), nbytes)
    row['byte_floor_us'] = round(nbytes / HBM_BYTES_PER_S * 1e6, 2)
    return row


def stem_rows(f, image):
    H, W = image
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    img = f(1, H, W, 3) * 50.0
    conv = torch.nn.Conv2d(3, 64, 7, stride=2, padding=3).cuda().to(memory_format=torch.channels_last)
    dz = f(1, Ho, Wo, 64)
    dpool = f(1, (Ho - 1) // 2 + 1, (Wo - 1) // 2 + 1, 64)
    xt = img.permute(0, 3, 1, 2)
    wt, bt = conv.weight.detach().clone().requires_grad_(), conv.bias.detach().clone().requires_grad_()
    zt = F.conv2d(xt, wt, bt, stride=2, padding=3)
    yt = F.max_pool2d(F.relu(zt), 3, 2, 1)

    def wgrad():
        patches = ops.stem_patches_f32(img)
        return ops.dense_wgrad(dz.view(-1, 64), patches.view(-1, ops.STEM_PATCH_K))
    y = ops.stem_trainable(img, conv.weight, conv.bias)
    rows = [common.row_of('stem_patches_f32 + dense_wgrad, %dx%d image (%d rows x 160 -> 64)' % (H, W, Ho * Wo), wgrad,
                          lambda: torch.autograd.grad(zt, [wt, bt], dz.permute(0, 3, 1, 2), retain_graph=True), inner=4),
            common.row_of('stem backward (pooling backward + patches + dense_wgrad), %dx%d image' % (H, W),
                          lambda: torch.autograd.grad(y, [conv.weight, conv.bias], dpool, retain_graph=True),
                          lambda: torch.autograd.grad(yt, [wt, bt], dpool.permute(0, 3, 1, 2), retain_graph=True), inner=4)]
    return rows


def training_calls(f, image, train_stem, calls):
    """whole training calls of ResnetV1Fpn-50 (forward with the fused targets and losses, then backward): wall ms per call"""
    torch.manual_seed(0)
    m = ResnetV1Fpn(depth=50, training_targets='hip', training_losses='hip', train_extractor=True, train_neck=True,
                    train_rpn_head=True, train_roi_head=True, train_stem=train_stem)
    H, W = image
    img = f(1, H, W, 3) * 50.0
    gt = torch.tensor([[0.1 * W, 0.1 * H, 0.5 * W, 0.6 * H], [0.4 * W, 0.3 * H, 0.9 * W, 0.8 * H]], device='cuda')
    gl = torch.tensor([3, 12], device='cuda')
    fwd, bwd = [], []
    for k in range(calls + 2):
        m.dense.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        losses = m((img, gt, gl), training=True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        sum(losses).backward()
        torch.cuda.synchronize()
        if k >= 2:
            fwd.append((t1 - t0) * 1e3)
            bwd.append((time.perf_counter() - t1) * 1e3)
    trained = sum(1 for p in m.dense.parameters() if p.grad is not None)
    del m
    torch.cuda.empty_cache()
    return dict(train_stem=train_stem, calls=calls, trained_parameters=trained, backward_ms=round(float(np.median(bwd)), 2),
                backward_range_ms=[round(min(bwd), 2), round(max(bwd), 2)], forward_ms=round(float(np.median(fwd)), 2))


def measure(a):
    rng = np.random.default_rng(0)
    torch.manual_seed(0)
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).cuda()
    H, W = a.image
    rows = [pool_row(f, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 64)] + stem_rows(f, tuple(a.image))
    model = []
    if a.calls:
        for stem in (False, True, False):                                      # the keyword off twice: the run-to-run spread
            model.append(training_calls(f, tuple(a.image), stem, a.calls))
            print(json.dumps(model[-1]), flush=True)
        off = [r['backward_ms'] for r in model if not r['train_stem']]
        on = [r['backward_ms'] for r in model if r['train_stem']][0]
        model_summary = dict(backward_ms_train_stem_off=off, backward_ms_train_stem_on=on,
                             run_to_run_spread_ms=round(abs(off[0] - off[1]), 2),
                             train_stem_adds_ms=round(on - float(np.mean(off)), 2))
    else:
        model_summary = None
    slower = [r['launch'] for r in rows if r.get('verdict') == 'SLOWER']
    return dict(device=torch.cuda.get_device_name(0), image=list(a.image),
                protocol='calls_per_graph calls per HIP graph; ours / yardstick graphs replayed alternately, %d replays each after 3 '
                         'warm-up replays; median and [min, max] microseconds per call; tensors, autograd graphs and captures all on '
                         'one side stream; the training calls: wall milliseconds around eager backward passes, synchronised, the '
                         'model without train_stem timed twice' % REPLAYS,
                hbm_figure_bytes_per_s=HBM_BYTES_PER_S, slower_than_yardstick=slower, rows=rows,
                resnet_v1_fpn_50_training_calls=model, resnet_v1_fpn_50_backward=model_summary)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', help='output path (default profiles/stem_grad_bench.json)')
    ap.add_argument('--image', type=int, nargs=2, default=(800, 1333))
    ap.add_argument('--calls', type=int, default=5, help='timed training calls per model (0: skip the models)')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    common.STREAM = torch.cuda.Stream()
    common.STREAM.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(common.STREAM):
        out = measure(a)
    path = a.out or os.path.join(ROOT, 'profiles', 'stem_grad_bench.json')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as fh:
        json.dump(out, fh, indent=1)
    print('wrote', path)


if __name__ == '__main__':
    main()
