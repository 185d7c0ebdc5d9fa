#!/usr/bin/env python3
"""Host model of what the processing order of the RoIs costs in an XCD's L2 (no GPU).

    python tools/roi_order_model.py [--seed 1234] [--order bands strips ...] [--strips 8] [--bins 32]

The RoI kernel's launch reads more map cells than the RoIs tap: cells that fall out of the 4 MB L2 of the
XCD an image is pinned to are fetched again.  This tool prices an order of the RoIs under these assumptions:

  * the L2 is an LRU over map cells (one cell = C channels x 4 B = 1 KB at C = 256); `cells` of them fit;
  * K RoIs are in flight (a 7-wave workgroup is one RoI; 2 workgroups x 32 CUs = 64 when the launch has the XCD to
    itself; two or three launches that share the XCD get K / 2, K / 3 and the same share of the cells);
  * a RoI walks its tapped columns left to right in seven steps, every step over all its tapped rows;
  * the starts of the K slots are staggered by one step each (mod 7), and a slot that finishes takes the next RoI
    of the order.

Inputs: the proposals of the bench's seeded image (oracle.c_oracle, as bench._cpu_leg computes them), the tap footprint of
bench.algorithmic_roi_bytes (first / last in-bounds sample of the 2P x 2P grid).  `bucket_strips` restates
d_roi_order_bucket of csrc/odet_internal.h, `bucket_bands` the order it replaced.

Prints one JSON object: the cells per level, the union of the tapped cells (the floor: every tapped cell fetched once) and
the misses of every requested order at (K, cells) = (64, 4096), (32, 2048), (21, 1365)."""
import argparse
import json
import os
import sys
from collections import OrderedDict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

POOL = 7
STEPS = 7
CONFIGS = ((64, 4096), (32, 2048), (21, 1365))


def quantise(rois, image_shape):
    """(qy, qx): the box centres quantised to 12 bits with the device's float32 operations, clamped"""
    r = np.asarray(rois, np.float32)
    inv_h = np.float32(1.0) / np.float32(image_shape[0])
    inv_w = np.float32(1.0) / np.float32(image_shape[1])
    qy = ((r[:, 1] + r[:, 3]) * np.float32(0.5) * inv_h * np.float32(4096.0)).astype(np.int64)
    qx = ((r[:, 0] + r[:, 2]) * np.float32(0.5) * inv_w * np.float32(4096.0)).astype(np.int64)
    return np.clip(qy, 0, 4095), np.clip(qx, 0, 4095)


def bucket_strips(rois, levels, image_shape, strips=8, bins=32, serpentine=True):
    """d_roi_order_bucket (csrc/odet_internal.h) for strips = 8, bins = 32; other powers of two for the model's table"""
    qy, qx = quantise(rois, image_shape)
    strip = qx // (4096 // strips)
    yb = qy // (4096 // bins)
    if serpentine:
        yb = np.where(strip & 1, bins - 1 - yb, yb)
    return (np.asarray(levels, np.int64) * strips + strip) * bins + yb


def bucket_bands(rois, levels, image_shape):
    """the order before: level, y band of 1/32 of the image"""
    qy, _ = quantise(rois, image_shape)
    return np.asarray(levels, np.int64) * 32 + (qy >> 7)


def bucket_morton(rois, levels, image_shape, tile_px=64):
    """level, then Z-order over tiles of tile_px image pixels"""
    r = np.asarray(rois, np.float32)
    ty = np.clip(((r[:, 1] + r[:, 3]) * np.float32(0.5) / tile_px).astype(np.int64), 0, 1023)
    tx = np.clip(((r[:, 0] + r[:, 2]) * np.float32(0.5) / tile_px).astype(np.int64), 0, 1023)
    code = np.zeros(len(r), np.int64)
    for b in range(10):
        code |= ((tx >> b) & 1) << (2 * b)
        code |= ((ty >> b) & 1) << (2 * b + 1)
    return np.asarray(levels, np.int64) * (1 << 20) + code


def order_of(buckets):
    """counting sort by bucket; inside a bucket the rows keep their order (the device's is arbitrary there)"""
    return np.argsort(np.asarray(buckets), kind='stable')


def footprints(rois, levels, level_shapes, image_shape, pool=POOL):
    """per RoI (row0, row1, col0, col1) inclusive on its level's map, as bench.algorithmic_roi_bytes spans them;
    an empty span is (0, -1)"""
    crop = 2 * pool
    H_img, W_img = np.float32(image_shape[0]), np.float32(image_shape[1])
    out = np.zeros((len(rois), 4), np.int64)
    for i, (r, l) in enumerate(zip(rois, levels)):
        Hk, Wk = level_shapes[int(l)]
        span = []
        for lo, hi, img, dim in ((r[1], r[3], H_img, Hk), (r[0], r[2], W_img, Wk)):
            lo_n, hi_n = np.float32(lo) / img, np.float32(hi) / img
            lim = np.float32(dim - 1)
            scale = (hi_n - lo_n) * lim / np.float32(crop - 1)
            coords = lo_n * lim + np.arange(crop, dtype=np.float32) * scale
            ok = coords[(coords >= 0) & (coords <= lim)]
            if ok.size == 0:
                span += [0, -1]
            else:
                span += [int(max(np.floor(ok.min()), 0)), int(min(np.ceil(ok.max()), dim - 1))]
        out[i] = span
    return out


def cell_steps(fp, levels, level_shapes):
    """per RoI: STEPS lists of cell ids (columns cut into STEPS runs left to right, every run over all rows)"""
    base, off = {}, 0
    for l, (h, w) in enumerate(level_shapes):
        base[l] = off
        off += h * w
    steps = []
    for (r0, r1, c0, c1), l in zip(fp, levels):
        W = level_shapes[int(l)][1]
        cols = np.arange(c0, c1 + 1)
        rows = np.arange(r0, r1 + 1)
        runs = np.array_split(cols, STEPS)
        steps.append([(base[int(l)] + rows[:, None] * W + run[None, :]).ravel().tolist() for run in runs])
    return steps, off


def union_cells(steps, levels, nlevels):
    per = [set() for _ in range(nlevels)]
    for st, l in zip(steps, levels):
        for cells in st:
            per[int(l)].update(cells)
    return [len(s) for s in per]


def misses(steps, order, K, cells):
    """LRU of `cells` cells, K slots; slot k starts k % STEPS ticks late; one step per slot and tick"""
    lru = OrderedDict()
    miss = 0
    nxt = 0
    n = len(order)
    slot_roi = [-1] * K
    slot_step = [0] * K
    delay = [k % STEPS for k in range(K)]
    active = True
    while active:
        active = False
        for k in range(K):
            if delay[k] > 0:
                delay[k] -= 1
                active = active or nxt < n
                continue
            if slot_roi[k] < 0:
                if nxt >= n:
                    continue
                slot_roi[k] = int(order[nxt])
                slot_step[k] = 0
                nxt += 1
            active = True
            for c in steps[slot_roi[k]][slot_step[k]]:
                if c in lru:
                    lru.move_to_end(c)
                else:
                    miss += 1
                    lru[c] = None
                    if len(lru) > cells:
                        lru.popitem(last=False)
            slot_step[k] += 1
            if slot_step[k] == STEPS:
                slot_roi[k] = -1
    return miss


def bench_proposals(seed=1234, image_shape=(800, 1333), num_proposals=1000):
    """the level-sorted proposals of the bench's seeded image: (rois [n, 4], level [n] 0-based, level shapes)"""
    from oracle import c_oracle as co
    from tf_eager_object_detection_amd import synthetic as syn
    from tf_eager_object_detection_amd.pipeline import synthetic_fpn_inputs
    host, _ = synthetic_fpn_inputs(image_shape, 21, num_proposals, 256, seed=seed, device='cpu')
    anchors = co.fpn_anchors(image_shape)
    fg = co.rpn_fg_fpn(host['rpn_logits'])
    rois, _ = co.region_proposal(host['rpn_deltas'], anchors, fg, image_shape, num_proposals, 0.7)
    lv, perm, _ = co.assign_levels(rois)
    return np.ascontiguousarray(rois[perm], np.float32), (lv[perm] - 2).astype(np.int64), list(syn.fpn_level_shapes(image_shape)[:4])


ORDERS = {
    'bands': lambda r, l, s, a: bucket_bands(r, l, s),
    'strips': lambda r, l, s, a: bucket_strips(r, l, s, a.strips, a.bins, True),
    'strips_plain': lambda r, l, s, a: bucket_strips(r, l, s, a.strips, a.bins, False),
    'morton': lambda r, l, s, a: bucket_morton(r, l, s),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seed', type=int, default=1234)
    ap.add_argument('--order', nargs='+', default=['bands', 'strips', 'strips_plain', 'morton'], choices=sorted(ORDERS))
    ap.add_argument('--strips', type=int, default=8)
    ap.add_argument('--bins', type=int, default=32)
    a = ap.parse_args()
    image_shape = (800, 1333)
    rois, levels, shapes = bench_proposals(a.seed, image_shape)
    fp = footprints(rois, levels, shapes, image_shape)
    steps, total = cell_steps(fp, levels, shapes)
    uni = union_cells(steps, levels, len(shapes))
    out = dict(seed=a.seed, rois=len(rois), level_split=[int((levels == l).sum()) for l in range(len(shapes))],
               cells_in_map=[h * w for h, w in shapes], union_cells=uni, union_total=sum(uni),
               union_MB_per_image=round(sum(uni) * 1024 / 1e6, 1), strips=a.strips, bins=a.bins, misses={})
    for name in a.order:
        order = order_of(ORDERS[name](rois, levels, image_shape, a))
        out['misses'][name] = {'K%d_cells%d' % kc: misses(steps, order, *kc) for kc in CONFIGS}
    print(json.dumps(out, indent=1))


if __name__ == '__main__':
    main()
