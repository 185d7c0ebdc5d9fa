#!/usr/bin/env python3
"""Times odet_preprocess_train (the training input stage, one launch per batch) against odet_preprocess_images (coco) on the
same batch, in one process, and writes profiles/train_input_bench.json.

The batch: 8 raw 375 x 500 images -> 600 x 800, caffe normalisation, 8 boxes per image for the training call; every buffer
already on the device.  Variants: `eval` (odet_preprocess_images), `train` (no image mirrored), `train_flipped` (every image
mirrored); float32 and float16 output.

Protocol: each variant's launch is captured INNER times in one HIP graph (back-to-back on one stream, no host time inside);
the graphs are replayed in turn, ROUNDS rounds, so every variant sees the same drift of the machine.  Per variant: the median,
the quartiles and the extremes of (replay time / INNER) in microseconds.  ratio = variant median / eval median of the same
dtype; spread = (eval's 75 % quartile - 25 % quartile) / eval median, the run-to-run spread the ratios are to be read against.

    python tools/train_input_bench.py"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tf_eager_object_detection_amd import _lib as L                                     # noqa: E402
from tf_eager_object_detection_amd import preprocess as P                              # noqa: E402

INNER, ROUNDS = 50, 40
B, RAW, G = 8, (375, 500), 8


def capture(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()                                             # (warm-up outside the capture: the kernel attributes)
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


def replay_us(g):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / INNER


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', help='output path (default profiles/train_input_bench.json)')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    rng = np.random.default_rng(0)
    H, W, _ = P.resized_shape(*RAW, pipeline='coco')
    raws = [torch.from_numpy(rng.integers(0, 256, RAW + (3,), dtype=np.uint8)).cuda() for _ in range(B)]
    boxes = torch.from_numpy(np.sort(rng.uniform(0, 1, (B * G, 2, 2)).astype(np.float32), axis=1).reshape(-1, 4)).cuda()
    ptrs = (C.c_void_p * B)(*[t.data_ptr() for t in raws])
    hs, ws = (C.c_int * B)(*([RAW[0]] * B)), (C.c_int * B)(*([RAW[1]] * B))
    pitch = (C.c_longlong * B)(*([3 * RAW[1]] * B))
    means = (C.c_double * 3)(*P.CAFFE_PIXEL_MEANS)
    offsets = (C.c_int * (B + 1))(*[G * i for i in range(B + 1)])
    gt_boxes = torch.empty((B * G, 4), dtype=torch.float32, device='cuda')
    gt_offsets = torch.empty(B + 1, dtype=torch.int32, device='cuda')
    graphs, keep = {}, []
    for dtype in (torch.float32, torch.float16):
        name = str(dtype).replace('torch.', '')
        f16 = int(dtype == torch.float16)
        out = torch.empty((B, H, W, 3), dtype=dtype, device='cuda')
        keep.append(out)

        def ev(out=out, f16=f16):
            L.call('odet_preprocess_images', ptrs, hs, ws, pitch, B, H, W, P.PIPELINES['coco'], 0, 0, means, L.dptr(out), f16,
                   L.stream())

        def train(flag, out=out, f16=f16):
            L.call('odet_preprocess_train', ptrs, hs, ws, pitch, B, H, W, 0, means, L.dptr(boxes), offsets, 1,
                   (C.c_int * B)(*([flag] * B)), 0, 0, L.dptr(out), f16, L.dptr(gt_boxes), L.dptr(gt_offsets), None, L.stream())
        graphs[name, 'eval'] = capture(ev)
        graphs[name, 'train'] = capture(lambda: train(0))
        graphs[name, 'train_flipped'] = capture(lambda: train(1))
    times = {k: [] for k in graphs}
    for _ in range(ROUNDS):
        for k, g in graphs.items():
            times[k].append(replay_us(g))
    rows = []
    for (name, variant), ts in times.items():
        q = np.percentile(ts, [0, 25, 50, 75, 100])
        base = float(np.median(times[name, 'eval']))
        eq = np.percentile(times[name, 'eval'], [25, 75])
        row = dict(dtype=name, variant=variant, us=round(float(q[2]), 2), q25=round(float(q[1]), 2), q75=round(float(q[3]), 2),
                   min=round(float(q[0]), 2), max=round(float(q[4]), 2), ratio_to_eval=round(float(q[2]) / base, 4),
                   eval_spread=round(float(eq[1] - eq[0]) / base, 4))
        print(json.dumps(row))
        rows.append(row)
    res = dict(device=torch.cuda.get_device_name(0), batch=B, raw=list(RAW), out=[H, W], boxes_per_image=G,
               protocol='%d launches per HIP graph; the six graphs replayed in turn, %d rounds' % (INNER, ROUNDS), rows=rows)
    path = a.out or os.path.join(ROOT, 'profiles', 'train_input_bench.json')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', path)


if __name__ == '__main__':
    main()
