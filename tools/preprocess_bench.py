#!/usr/bin/env python3
"""Times odet_preprocess_images (the eval loaders' normalisation + resize, one launch per batch) at the eval shapes and
writes profiles/preprocess_<tag>.json.

Per row: batch 1 / 8 of raw 375x500 (-> 600x800) or 1080x1920 (-> 562x1000 voc, 562x999 coco), pipeline voc / coco
(caffe normalisation), float32 / float16 output:
  us            GPU time per launch: 20 launches captured in one HIP graph, replayed, median of the replays / 20
                (back-to-back launches on one stream, no host time inside);
  bytes         moved per launch: 3*h*w read + 12*H*W (float32) or 6*H*W (float16) written, per image;
  torch_us      the same work composed from torch ops under the same protocol: type conversion, mean subtraction,
                layers.tf_legacy_resize_bilinear (NCHW) and the NHWC layout (+ the float16 cast);
  calib_us      odet_calib_stream_mix moving the same read and write bytes (a kernel that only moves bytes), same protocol:
                rate_vs_calib = (bytes / us) / (calib_bytes / calib_us), the kernel's byte rate over the calibration's.

    python tools/preprocess_bench.py --tag r07"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tf_eager_object_detection_amd import _lib as L                                     # noqa: E402
from tf_eager_object_detection_amd import preprocess as P                              # noqa: E402
from tf_eager_object_detection_amd.model.layers import tf_legacy_resize_bilinear  # noqa: E402

INNER = 20


def graph_us(fn, replays=30):
    """median GPU time of one fn() call: INNER calls captured in one graph, replayed"""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()                                             # (warm-up outside the capture: kernel attributes, allocator)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tag', default='local')
    ap.add_argument('--out', help='output path (default profiles/preprocess_<tag>.json)')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    rows = []
    rng = np.random.default_rng(0)
    means = torch.tensor(P.CAFFE_PIXEL_MEANS, dtype=torch.float32, device='cuda')
    for raw_hw in ((375, 500), (1080, 1920)):
        for B in (1, 8):
            raws = [torch.from_numpy(rng.integers(0, 256, raw_hw + (3,), dtype=np.uint8)).cuda() for _ in range(B)]
            stacked = torch.stack(raws)
            for pipeline in ('voc', 'coco'):
                H, W, _ = P.resized_shape(*raw_hw, pipeline=pipeline)
                for dtype in (torch.float32, torch.float16):
                    es = 4 if dtype == torch.float32 else 2
                    nbytes = B * (3 * raw_hw[0] * raw_hw[1] + 3 * es * H * W)
                    us = graph_us(lambda: P.preprocess_images(raws, pipeline, dtype=dtype))

                    def composed():
                        x = stacked.float() - means
                        y = tf_legacy_resize_bilinear(x.permute(0, 3, 1, 2), (H, W)).permute(0, 2, 3, 1).contiguous()
                        return y.half() if dtype == torch.float16 else y
                    t_us = graph_us(composed)
                    rb = (B * 3 * raw_hw[0] * raw_hw[1] // 8192 + 1) * 8192
                    wb = (B * 3 * es * H * W // 8192 + 1) * 8192
                    src = torch.zeros(rb, dtype=torch.uint8, device='cuda')
                    dst = torch.empty(wb, dtype=torch.uint8, device='cuda')
                    c_us = graph_us(lambda: L.call('odet_calib_stream_mix', src.data_ptr(), rb, dst.data_ptr(), wb,
                                                   L.stream(), None, None))
                    row = dict(pipeline=pipeline, dtype=str(dtype).replace('torch.', ''), batch=B, raw=list(raw_hw),
                               out=[H, W], us=round(us, 2), bytes=nbytes, GBps=round(nbytes / us / 1e3, 1),
                               torch_us=round(t_us, 2), torch_vs_kernel=round(t_us / us, 2), calib_us=round(c_us, 2),
                               calib_bytes=rb + wb, calib_GBps=round((rb + wb) / c_us / 1e3, 1),
                               rate_vs_calib=round(c_us / us * nbytes / (rb + wb), 3))
                    print(json.dumps(row))
                    rows.append(row)
    out = dict(device=torch.cuda.get_device_name(0), protocol='%d launches per HIP graph, median of 30 replays' % INNER,
               rows=rows)
    path = a.out or os.path.join(ROOT, 'profiles', 'preprocess_%s.json' % a.tag)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
    print('wrote', path)


if __name__ == '__main__':
    main()
