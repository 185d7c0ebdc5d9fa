#!/usr/bin/env python3
"""Times the RoI pooling backward (csrc/roi_grad.hip: the select launch and the gather) at the FPN training shapes of an
800 x 1333 image -- maps 200 x 334, 100 x 167, 50 x 84, 25 x 42, C = 256, P = 7, MAX2, NORM_IMAGE -- for 256 and 512 RoIs drawn
with synthetic.random_boxes (what the proposal-target benchmarks draw) and for the PILE-UP: 512 RoIs whose sample rows all tap the
same few cell rows of P2, the worst serial depth of a tile.  Writes profiles/roi_grad_bench.json.

  ours       odet_roi_pool_argmax (select) and odet_roi_pool_backward (grad), each in its own graph, and both in one.
  yardstick  the torch restatement the tests use (index gathers of the four taps of every sample, the bilinear weights,
             max_pool2d), vectorised over the RoIs of a level, BACKWARD ONLY (torch.autograd.grad on a retained graph).  Its scatter
             is atomic and not reproducible: a yardstick for time, not for bits.

Clock: GPU time of INNER calls captured in one HIP graph and replayed; the graphs are replayed alternately, REPLAYS times each
after 3 warm-up replays; median and (min, max) per call in microseconds.  `share_of_copy_bandwidth`: the algorithmic bytes (every
dx written once, dy and sel read once) over the median of select + grad, against the bandwidth a device-to-device copy of 256 MB
reaches in the same process, measured the same way.

    python tools/roi_grad_bench.py"""
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

INNER, REPLAYS = 5, 30
SHAPE = (800, 1333)
C, P = 256, 7


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


def stat(row, name, t):
    row[name + '_us'] = round(t[0], 2)
    row[name + '_range_us'] = [round(t[1], 2), round(t[2], 2)]


def copy_bandwidth():
    a = torch.empty(64 * 1024 * 1024, dtype=torch.float32, device='cuda')
    b = torch.empty_like(a)
    t = alternate({'copy': capture(lambda: b.copy_(a))})['copy']
    return 2.0 * a.numel() * 4 / (t[0] * 1e-6)


def yardstick(case, maps):
    """the vectorised torch restatement over leaves of the maps -> (pooled features [n,P,P,C] in the case's row order, leaves)"""
    leaves = [m.clone().requires_grad_(True) for m in maps]
    taps = [rg.taps(case, r) for r in range(case.n)]
    outs, rows = [], []
    for l, leaf in enumerate(leaves):
        idx = [r for r in range(case.n) if taps[r][0] == l]
        if not idx:
            continue
        g = lambda k, ax: torch.from_numpy(np.stack([np.asarray(taps[r][ax][k]) for r in idx])).cuda()
        ylo, yhi, wy, yok = g(2, 1).long(), g(3, 1).long(), g(4, 1), g(1, 1)
        xlo, xhi, wx, xok = g(2, 2).long(), g(3, 2).long(), g(4, 2), g(1, 2)
        m = leaf[0]
        wy, wx = wy[:, :, None, None], wx[:, None, :, None]
        tap = lambda yy, xx: m[yy[:, :, None], xx[:, None, :]]
        top = tap(ylo, xlo) + (tap(ylo, xhi) - tap(ylo, xlo)) * wx
        bot = tap(yhi, xlo) + (tap(yhi, xhi) - tap(yhi, xlo)) * wx
        v = (top + (bot - top) * wy) * (yok[:, :, None, None] & xok[:, None, :, None])
        outs.append(torch.nn.functional.max_pool2d(v.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1))
        rows += idx
    out = torch.cat(outs)
    inv = torch.from_numpy(np.argsort(np.asarray(rows))).cuda()
    return out[inv], leaves


def bench(name, rois, bw):
    rois_t = torch.from_numpy(np.ascontiguousarray(rois, np.float32)).cuda()
    srois, level, perm, counts = ops.assign_levels(rois_t, 2, 5)
    n = int(srois.shape[0])
    hw = syn.fpn_level_shapes(SHAPE)[:4]
    rng = np.random.default_rng(1)
    maps = [torch.from_numpy(rng.standard_normal((1, h, w, C)).astype(np.float32)).cuda() for h, w in hw]
    dy = torch.from_numpy(rng.standard_normal((n, P, P, C)).astype(np.float32)).cuda()
    sel = torch.empty((n, P, P, C), dtype=torch.uint8, device='cuda')
    dxs = [torch.empty_like(m) for m in maps]
    args = (srois, level, ops.ROI_NORM_IMAGE, P)
    select = lambda: ops.roi_pool_argmax(maps, *args, image_shape=SHAPE, out=sel)
    grad = lambda: ops.roi_pool_backward(dy, None, *args, ops.ROI_POOL_MAX2, image_shape=SHAPE, sel=sel, outs=dxs)
    select()
    case = rg.GradCase(name, rg.NORM_IMAGE, rg.POOL_MAX2, C, P, srois.cpu().numpy(), level=level.cpu().numpy(), maps_hw=hw,
                       image_shape=SHAPE)
    out, leaves = yardstick(case, maps)
    used_levels = [l for l in range(len(leaves)) if int((level == l).sum())]
    used = [leaves[l] for l in used_levels]
    ybw = lambda: torch.autograd.grad(out, used, dy, retain_graph=True)
    # the yardstick computes the same gradient (to rounding: its sums come in another order)
    got = grad()
    want = ybw()
    worst = max(float((g - w).abs().max()) for g, w in zip([got[l] for l in used_levels], want))
    t = alternate({'select': capture(select), 'grad': capture(grad), 'both': capture(lambda: (select(), grad())), 'yardstick': capture(ybw)})
    nbytes = sum(m.numel() for m in maps) * 4 + dy.numel() * 4 + sel.numel()
    row = dict(case=name, rois=n, per_level=[int(c) for c in counts.tolist()], max_abs_difference_to_yardstick=worst)
    for k in ('select', 'grad', 'both', 'yardstick'):
        stat(row, k, t[k])
    row['yardstick_over_ours'] = round(t['yardstick'][0] / t['both'][0], 3)
    row['algorithmic_bytes'] = nbytes
    row['share_of_copy_bandwidth'] = round(nbytes / (t['both'][0] * 1e-6) / bw, 4)
    row['expectation_no_slower_than_yardstick'] = 'MET' if t['both'][0] <= t['yardstick'][0] else 'MISSED'
    print(json.dumps(row), flush=True)
    return row


def pileup_rois(n):
    """n RoIs of P2 size whose 14 sample rows all fall into cell rows 100 .. 103 of P2, spread along x"""
    rng = np.random.default_rng(2)
    x0 = rng.uniform(0, SHAPE[1] - 120, n)
    return np.stack([x0, np.full(n, 400.0), x0 + rng.uniform(60, 110, n), np.full(n, 412.0)], axis=1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', help='output path (default profiles/roi_grad_bench.json)')
    a = ap.parse_args()
    global STREAM
    torch.cuda.set_device(0)
    STREAM = torch.cuda.Stream()
    STREAM.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(STREAM):
        bw = copy_bandwidth()
        rng = np.random.default_rng(0)
        rows = [bench('random_256', syn.random_boxes(256, SHAPE, rng, 16, 600), bw),
                bench('random_512', syn.random_boxes(512, SHAPE, rng, 16, 600), bw),
                bench('pileup_512', pileup_rois(512), bw)]
    out = dict(device=torch.cuda.get_device_name(0),
               protocol='%d calls per HIP graph; the graphs replayed alternately, %d replays each after 3 warm-up replays; median and '
                        '[min, max] microseconds per call' % (INNER, REPLAYS),
               copy_bandwidth_bytes_per_s=bw, rows=rows)
    path = a.out or os.path.join(ROOT, 'profiles', 'roi_grad_bench.json')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
    print('wrote', path)


if __name__ == '__main__':
    main()
