#!/usr/bin/env python3
"""Times the accumulate launch of the K-image training step (odet_bucket_accumulate_f32, csrc/grad_exchange.hip) on the gradient
shapes of ResNet-101-FPN, each form against what torch offers on the same tensors; writes profiles/grad_accumulate_bench.json.

  first   ops.bucket_accumulate(first=True): the gradient list -> the bucket            vs  torch._foreach_copy_ into per-tensor sums
  later   ops.bucket_accumulate(first=False): bucket += gradients, one launch           vs  torch._foreach_add_ ; and one add_ per tensor
                                                                                            (autograd's own accumulation into p.grad)
  last    the same with divisor = float32(K): bucket = (bucket + gradients) / K         vs  torch._foreach_add_ then torch._foreach_div_

Protocol (tools/optimizer_bench.py's): GPU time with INNER calls captured in one HIP graph, replayed after 3 warm-up replays,
median / min / max of 20 replays / INNER.  bytes = the floor of the operation: 12 bytes per element (two reads, one write), 8 for
the first form; floor_us = bytes / 8 TB/s, the data-sheet figure this project quotes fractions of.

    python tools/grad_accumulate_bench.py"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tf_eager_object_detection_amd import ops                                             # noqa: E402
from tf_eager_object_detection_amd.model.fpn_detector import ResNetFpnDetector            # noqa: E402
from tools.optimizer_bench import PEAK, graph_us                                          # noqa: E402

K = 4
INNER = 10


def row(name, nbytes, fused, compositions, **extra):
    us, lo, hi = graph_us(fused, INNER)
    r = dict(op=name, bytes=nbytes, floor_us=round(nbytes / PEAK * 1e6, 1), us=round(us, 1), us_min=round(lo, 1), us_max=round(hi, 1),
             gb_per_s=round(nbytes / us / 1e3, 1), hbm_frac=round(nbytes / (us * 1e-6) / PEAK, 3), composed=[], **extra)
    for label, fn in compositions:
        c_us, c_lo, c_hi = graph_us(fn, INNER)
        r['composed'].append(dict(composition=label, us=round(c_us, 1), us_min=round(c_lo, 1), us_max=round(c_hi, 1),
                                  composed_vs_fused=round(c_us / us, 2)))
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', help='output path (default profiles/grad_accumulate_bench.json)')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    model = ResNetFpnDetector(101, 21, (800, 1333), 1000, dtype=torch.float32)
    # every parameter a training step with train_extractor=True gives a gradient: all but the frozen conv1
    shapes = [tuple(p.shape) for n, p in model.named_parameters() if not n.startswith('conv1.')]
    del model
    gen = torch.Generator(device='cuda')
    gen.manual_seed(1)
    grads = [torch.randn(s, device='cuda', generator=gen) * 0.01 for s in shapes]
    elements = sum(g.numel() for g in grads)
    tb = ops.BucketTables([g.numel() for g in grads], 1, 'cuda:0')
    bucket = tb.new_bucket()
    sums = [torch.zeros_like(g) for g in grads]                  # what torch accumulates into: one tensor per gradient
    common = dict(tensors=len(grads), elements=elements, bucket_elements=tb.bucket_numel)
    rows = []

    rows.append(row('first', 8 * elements, lambda: ops.bucket_accumulate(tb, grads, bucket, True),
                    [('torch._foreach_copy_(sums, gradients)', lambda: torch._foreach_copy_(sums, grads))], **common))

    def per_tensor():
        for s, g in zip(sums, grads):
            s.add_(g)
    rows.append(row('later', 12 * elements, lambda: ops.bucket_accumulate(tb, grads, bucket, False),
                    [('torch._foreach_add_(sums, gradients)', lambda: torch._foreach_add_(sums, grads)),
                     ('one add_ per tensor (autograd\'s accumulation into p.grad)', per_tensor)], **common))

    def add_div():
        torch._foreach_add_(sums, grads)
        torch._foreach_div_(sums, float(K))
    rows.append(row('last', 12 * elements, lambda: ops.bucket_accumulate(tb, grads, bucket, False, float(K)),
                    [('torch._foreach_add_ then torch._foreach_div_(sums, %d)' % K, add_div)], images=K, **common))

    # the launch equals the composition by bytes on one window (one add per image is order-free at two images)
    ops.bucket_accumulate(tb, grads, bucket, True)
    ops.bucket_accumulate(tb, grads, bucket, False, 2.0)
    torch._foreach_copy_(sums, grads)
    torch._foreach_add_(sums, grads)
    torch._foreach_div_(sums, 2.0)
    torch.cuda.synchronize()
    assert all(torch.equal(bucket[tb.offset(i):tb.offset(i) + g.numel()].view(torch.int32), s.reshape(-1).view(torch.int32))
               for i, (g, s) in enumerate(zip(grads, sums)))

    out = dict(device=torch.cuda.get_device_name(0),
               protocol='us: %d calls per HIP graph, 3 warm-up replays, median / min / max of 20 replays; bytes: 12 per element '
                        '(8 for the first form), the floor; floor_us and hbm_frac: against 8 TB/s' % INNER,
               rows=rows)
    path = a.out or os.path.join(ROOT, 'profiles', 'grad_accumulate_bench.json')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
    print('wrote', path)


if __name__ == '__main__':
    main()
