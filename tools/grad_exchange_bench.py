#!/usr/bin/env python3
"""Times the three launches of the data-parallel gradient exchange (csrc/grad_exchange.hip) on the gradient shapes of
ResNet-101-FPN at world = 8, each against the torch composition on the same tensors; writes profiles/grad_exchange_bench.json.

  pack       ops.bucket_pack: the whole gradient list -> the bucket, one launch        vs  torch.cat of the flattened gradients
  unpack     ops.bucket_unpack: the bucket -> every tensor, one launch                 vs  one copy_ per tensor from the bucket
  rank_mean  ops.rank_mean: parts [8, shard] -> [shard], ascending rank, one division  vs  parts.sum(0) / 8
             (the eight parts are simulated on one GPU: random data of a shard's size)

Protocol (tools/optimizer_bench.py's): GPU time with INNER calls captured in one HIP graph, replayed after 3 warm-up replays,
median / min / max of 20 replays / INNER.  bytes = what the operation has to move (every element read once and written once;
rank_mean: eight parts read, one shard written); hbm_frac = bytes / us / 8 TB/s, the data-sheet figure this project quotes
fractions of.  The collectives between the launches (all_to_all_single, all_gather_into_tensor over xGMI) need eight GPUs and
are not measured here.

    python tools/grad_exchange_bench.py"""
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

WORLD = 8
INNER = 10


def row(name, nbytes, fused, composed, **extra):
    us, lo, hi = graph_us(fused, INNER)
    c_us, c_lo, c_hi = graph_us(composed, INNER)
    r = dict(op=name, world=WORLD, bytes=nbytes, us=round(us, 1), us_min=round(lo, 1), us_max=round(hi, 1),
             gb_per_s=round(nbytes / us / 1e3, 1), hbm_frac=round(nbytes / (us * 1e-6) / PEAK, 3), composed_us=round(c_us, 1),
             composed_us_min=round(c_lo, 1), composed_us_max=round(c_hi, 1), composed_vs_fused=round(c_us / us, 2), **extra)
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', help='output path (default profiles/grad_exchange_bench.json)')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    model = ResNetFpnDetector(101, 21, (800, 1333), 1000, dtype=torch.float32)
    # every parameter a training step with train_extractor=True gives a gradient: all but the frozen conv1 (234 tensors)
    shapes = [tuple(p.shape) for n, p in model.named_parameters() if not n.startswith('conv1.')]
    del model
    gen = torch.Generator(device='cuda')
    gen.manual_seed(1)
    grads = [torch.randn(s, device='cuda', generator=gen) * 0.01 for s in shapes]
    elements = sum(g.numel() for g in grads)
    tb = ops.BucketTables([g.numel() for g in grads], WORLD, 'cuda:0')
    bucket = tb.new_bucket()
    flat = [g.reshape(-1) for g in grads]
    rows = []

    rows.append(row('pack', 4 * (elements + tb.bucket_numel), lambda: ops.bucket_pack(tb, grads, bucket), lambda: torch.cat(flat),
                    tensors=len(grads), elements=elements, bucket_elements=tb.bucket_numel, composition='torch.cat(flattened gradients)'))

    ops.bucket_pack(tb, grads, bucket)
    dst = [torch.empty_like(g) for g in grads]
    pieces = [bucket[tb.offset(i):tb.offset(i) + g.numel()].view(g.shape) for i, g in enumerate(grads)]

    def copies():
        for d, p in zip(dst, pieces):
            d.copy_(p)
    rows.append(row('unpack', 8 * elements, lambda: ops.bucket_unpack(tb, bucket, dst), copies, tensors=len(grads), elements=elements,
                    bucket_elements=tb.bucket_numel, composition='one copy_ per tensor'))
    assert all(torch.equal(d, g) for d, g in zip(dst, grads))

    parts = torch.randn((WORLD, tb.shard_numel), device='cuda', generator=gen) * 0.01
    out = torch.empty(tb.shard_numel, device='cuda')
    rows.append(row('rank_mean', 4 * (WORLD + 1) * tb.shard_numel, lambda: ops.rank_mean(parts, True, out=out),
                    lambda: parts.sum(0) / WORLD, elements=tb.shard_numel, composition='parts.sum(0) / 8'))

    out = dict(device=torch.cuda.get_device_name(0),
               protocol='us: %d calls per HIP graph, 3 warm-up replays, median / min / max of 20 replays; hbm_frac: bytes / us / '
                        '8 TB/s; the eight ranks\' parts are simulated on one GPU; the collectives over xGMI: not measured' % INNER,
               rows=rows)
    path = a.out or os.path.join(ROOT, 'profiles', 'grad_exchange_bench.json')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
    print('wrote', path)


if __name__ == '__main__':
    main()
