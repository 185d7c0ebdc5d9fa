#!/usr/bin/env python3
"""Times the RoI pooling over a batch of images (odet_roi_pool_images, odet_roi_pool_argmax_images,
odet_roi_pool_backward_images) at the FPN training shapes of an 800 x 1333 image -- maps 200 x 334, 100 x 167, 50 x 84, 25 x 42,
C = 256, P = 7, MAX2, NORM_IMAGE -- for 256 and 512 RoIs per image (synthetic.random_boxes, level-sorted per image by
ops.assign_levels) and B = 2, 4, 8 images.  Writes profiles/roi_grad_batch_bench.json.

Per (RoIs, B), for the backward (select + gather) and for the forward:
  batched    (a) the *_images calls on the dense [B,...] tensors: 2 launches for the backward, ceil(B / 8) for the forward;
  singles    (b) the single-image calls on the B slices of the SAME tensors, one after the other: 2 B and B launches -- what the
             code ran before the batched calls existed, and the comparison that counts;
  torch      (c) the torch restatement the tests use (index gathers of the four taps of every sample, the bilinear weights,
             max_pool2d) over the B images: forward under no_grad, backward as torch.autograd.grad on retained graphs.  Its scatter
             is atomic and not reproducible: a yardstick for time, not for bits.

Clock: GPU time of INNER calls captured in one HIP graph and replayed; the three graphs are replayed alternately, REPLAYS times
each after 3 warm-up replays, and the whole alternation is run ROUNDS times: per row the median of each round, the overall
[min, max] per call in microseconds, and `spread_us` = the largest difference between two rounds' medians of the same graph (the
run-to-run spread).  `verdict`: FASTER when every round's batched median lies below every round's singles median by more than
that spread, else SLOWER.  Before timing, the batched results are compared with the singles' (bit-equal) and with torch's.

    python tools/roi_grad_batch_bench.py"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from tf_eager_object_detection_amd import ops, synthetic as syn                          # noqa: E402
import roi_grad_np as rg                                                                 # noqa: E402
import tools.roi_grad_bench as single                                                    # noqa: E402

ROUNDS = 3
SHAPE, C, P = single.SHAPE, single.C, single.P


def torch_image(case, maps):
    """the vectorised torch restatement of one image: -> fwd(maps of the image, [level] -> [H,W,C]) = pooled features in LEVEL
    order, and the row permutation that order is"""
    taps = [rg.taps(case, r) for r in range(case.n)]
    per_level, rows = [], []
    for l in range(len(maps)):
        idx = [r for r in range(case.n) if taps[r][0] == l]
        if not idx:
            continue
        g = lambda k, ax: torch.from_numpy(np.stack([np.asarray(taps[r][ax][k]) for r in idx])).cuda()
        per_level.append((l, g(2, 1).long(), g(3, 1).long(), g(4, 1)[:, :, None, None], g(1, 1), g(2, 2).long(), g(3, 2).long(),
                          g(4, 2)[:, None, :, None], g(1, 2)))
        rows += idx

    def fwd(ms):
        outs = []
        for l, ylo, yhi, wy, yok, xlo, xhi, wx, xok in per_level:
            m = ms[l]
            tap = lambda yy, xx: m[yy[:, :, None], xx[:, None, :]]
            top = tap(ylo, xlo) + (tap(ylo, xhi) - tap(ylo, xlo)) * wx
            bot = tap(yhi, xlo) + (tap(yhi, xhi) - tap(yhi, xlo)) * wx
            v = (top + (bot - top) * wy) * (yok[:, :, None, None] & xok[:, None, :, None])
            outs.append(torch.nn.functional.max_pool2d(v.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1))
        return torch.cat(outs)
    return fwd, torch.from_numpy(np.asarray(rows)).cuda()


def rounds(graphs):
    """ROUNDS alternations -> {name: (medians per round, min, max)}"""
    per = [single.alternate(graphs) for _ in range(ROUNDS)]
    return {k: ([p[k][0] for p in per], min(p[k][1] for p in per), max(p[k][2] for p in per)) for k in graphs}


def row_of(what, n, B, launches, t):
    row = dict(what=what, rois_per_image=n, images=B, launches=launches)
    for k, (med, lo, hi) in t.items():
        row[k + '_us'] = round(float(np.median(med)), 2)
        row[k + '_round_medians_us'] = [round(m, 2) for m in med]
        row[k + '_range_us'] = [round(lo, 2), round(hi, 2)]
    spread = max(max(m) - min(m) for m in (t['batched'][0], t['singles'][0]))
    row['spread_us'] = round(spread, 2)
    row['singles_over_batched'] = round(row['singles_us'] / row['batched_us'], 3)
    row['torch_over_batched'] = round(row['torch_us'] / row['batched_us'], 3)
    row['verdict'] = 'FASTER' if min(t['singles'][0]) - max(t['batched'][0]) > spread else 'SLOWER'
    print(json.dumps(row), flush=True)
    return row


def bench(n, B):
    rng = np.random.default_rng(100 * B + n)
    hw = syn.fpn_level_shapes(SHAPE)[:4]
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).cuda()
    per = [ops.assign_levels(torch.from_numpy(syn.random_boxes(n, SHAPE, rng, 16, 600).astype(np.float32)).cuda(), 2, 5)[:2]
           for _ in range(B)]
    rois, level = torch.stack([p[0] for p in per]).contiguous(), torch.stack([p[1] for p in per]).to(torch.int32).contiguous()
    maps = [f(B, h, w, C) for h, w in hw]
    dy = f(B, n, P, P, C)
    feats, sel = torch.empty_like(dy), torch.empty(tuple(dy.shape), dtype=torch.uint8, device='cuda')
    dxs = [torch.empty_like(m) for m in maps]
    feats1, sel1, dxs1 = torch.empty_like(feats), torch.empty_like(sel), [torch.empty_like(m) for m in maps]
    kw = dict(image_shape=SHAPE)
    norm, pool = ops.ROI_NORM_IMAGE, ops.ROI_POOL_MAX2

    def fwd_batched():
        ops.roi_pool_images(maps, rois, level, norm, P, pool, out=feats, **kw)

    def bwd_batched():
        ops.roi_pool_argmax_images(maps, rois, level, norm, P, out=sel, **kw)
        ops.roi_pool_backward_images(dy, None, rois, level, norm, P, pool, sel=sel, outs=dxs, **kw)
    slices = [([m[b:b + 1] for m in maps], [d[b:b + 1] for d in dxs1]) for b in range(B)]

    def fwd_singles():
        for b in range(B):
            ops.roi_pool(slices[b][0], rois[b], level[b], norm, P, pool, out=feats1[b], **kw)

    def bwd_singles():
        for b in range(B):
            ops.roi_pool_argmax(slices[b][0], rois[b], level[b], norm, P, out=sel1[b], **kw)
            ops.roi_pool_backward(dy[b], None, rois[b], level[b], norm, P, pool, sel=sel1[b], outs=slices[b][1], **kw)
    # torch: one retained graph per image
    images = []
    for b in range(B):
        case = rg.GradCase('bench', rg.NORM_IMAGE, rg.POOL_MAX2, C, P, rois[b].cpu().numpy(), level=level[b].cpu().numpy(), maps_hw=hw,
                           image_shape=SHAPE)
        fwd, order = torch_image(case, maps)
        leaves = [m[b].clone().requires_grad_(True) for m in maps]
        used = [l for l in range(len(hw)) if int((level[b] == l).sum())]
        images.append((fwd, order, leaves, used, fwd(leaves), dy[b][order].contiguous()))

    def fwd_torch():
        with torch.no_grad():
            return [im[0](im[2]) for im in images]

    def bwd_torch():
        return [torch.autograd.grad(im[4], [im[2][l] for l in im[3]], im[5], retain_graph=True) for im in images]
    # the same results first: batched == singles by bits, torch to rounding
    for fn in (fwd_batched, bwd_batched, fwd_singles, bwd_singles):
        fn()
    torch.cuda.synchronize()
    assert torch.equal(feats, feats1) and torch.equal(sel, sel1) and all(torch.equal(a, c) for a, c in zip(dxs, dxs1))
    worst_f = max(float((feats[b][im[1]] - o).abs().max()) for b, (im, o) in enumerate(zip(images, fwd_torch())))
    worst_b = max(float((dxs[l][b] - g).abs().max()) for b, (im, gs) in enumerate(zip(images, bwd_torch())) for l, g in zip(im[3], gs))
    cap = single.capture
    rows = []
    t = rounds({'batched': cap(bwd_batched), 'singles': cap(bwd_singles), 'torch': cap(bwd_torch)})
    rows.append(dict(row_of('backward (select + gather)', n, B, dict(batched=2, singles=2 * B), t), max_abs_difference_to_torch=worst_b))
    t = rounds({'batched': cap(fwd_batched), 'singles': cap(fwd_singles), 'torch': cap(fwd_torch)})
    rows.append(dict(row_of('forward', n, B, dict(batched=-(-B // 8), singles=B), t), max_abs_difference_to_torch=worst_f))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', help='output path (default profiles/roi_grad_batch_bench.json)')
    ap.add_argument('--rois', type=int, nargs='+', default=[256, 512])
    ap.add_argument('--images', type=int, nargs='+', default=[2, 4, 8])
    a = ap.parse_args()
    torch.cuda.set_device(0)
    single.STREAM = torch.cuda.Stream()
    single.STREAM.wait_stream(torch.cuda.current_stream())
    rows = []
    with torch.cuda.stream(single.STREAM):
        for n in a.rois:
            for B in a.images:
                rows += bench(n, B)
                torch.cuda.empty_cache()
    out = dict(device=torch.cuda.get_device_name(0),
               protocol='%d calls per HIP graph; the three graphs of a row replayed alternately, %d replays each after 3 warm-up replays, '
                        '%d rounds; median of the round medians, every round median, [min, max] microseconds per call; spread_us = the '
                        'largest difference between two round medians of the batched or the singles graph'
                        % (single.INNER, single.REPLAYS, ROUNDS),
               slower_than_singles=['%s, %d RoIs x %d images' % (r['what'], r['rois_per_image'], r['images']) for r in rows
                                    if r['verdict'] == 'SLOWER'], rows=rows)
    path = a.out or os.path.join(ROOT, 'profiles', 'roi_grad_batch_bench.json')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
    print('wrote', path)


if __name__ == '__main__':
    main()
