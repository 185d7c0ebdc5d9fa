#!/usr/bin/env python3
"""Times the batched training call of ResnetV1Fpn (depth 50, all five train keywords, training_targets = training_losses = 'hip')
against what ran before it existed, at 800 x 1333 and at the tests' 256 x 352, for B = 1, 2, 4 images.  Writes
profiles/train_call_bench.json.

Per (image size, B), forward plus backward:
  batched    (a) ONE four-tuple call on the B images and one backward() of the sum of its 4 B losses;
  singles    (b) B three-tuple calls on the same images, each with its own backward() -- the parent commit's K-image step, and the
             comparison that counts.

Clock: wall time with a synchronize on each side of forward plus backward (the proposal calls read counts on the host, so the
calls are not captured).  The two loops are run alternately, CALLS times each after 2 warm-up calls, and the whole alternation is
run ROUNDS times: per row the median of the round medians, every round median, and `spread_ms` = the largest difference between two
round medians of the same loop.  `verdict` (the rule of tools/roi_grad_batch_bench.py): FASTER when every round's batched median
lies below every round's singles median by more than that spread, else SLOWER.

`parity` (--parity, at 256 x 352 on the tests' model and images): the largest relative difference of the losses and of the parameter
gradients between one two-image call and the two one-image calls -- what tests/test_train_batch_gpu.py bounds by 8 x.

    python tools/train_call_bench.py [--parity]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tf_eager_object_detection_amd.model.base_fpn_model import ResnetV1Fpn                 # noqa: E402

ROUNDS, CALLS, WARMUP = 3, 5, 2
MODEL = dict(depth=50, training_targets='hip', training_losses='hip', train_neck=True, train_rpn_head=True, train_roi_head=True,
             train_extractor=True, train_stem=True)
SIZES = {'800x1333': (800, 1333), '256x352': (256, 352)}


def make_model(seed=1, **kw):
    torch.manual_seed(seed)
    m = ResnetV1Fpn(**dict(MODEL, **kw))
    with torch.no_grad():                                   # (spreads the fresh RpnHead's proposals over sizes and pyramid levels)
        b = m.dense.rpn_bbox.bias
        b.add_(torch.linspace(0.0, 1.6, b.numel(), device=b.device, dtype=b.dtype))
    return m


def make_images(B, shape, seed=20):
    h, w = shape
    images, boxes = [], []
    for k in range(B):
        rng = np.random.default_rng(seed + k)
        images.append(torch.from_numpy((rng.uniform(0, 255, (1, h, w, 3)) - 110).astype(np.float32)).cuda())
        x0, y0 = rng.uniform(0, w * 0.5, 3), rng.uniform(0, h * 0.5, 3)
        bw, bh = rng.uniform(w * 0.1, w * 0.45, 3), rng.uniform(h * 0.1, h * 0.45, 3)
        boxes.append(torch.from_numpy(np.stack([x0, y0, x0 + bw, y0 + bh], axis=1).astype(np.float32)).cuda())
    labels = torch.tensor([3, 7, 12], device='cuda')
    return images, boxes, labels


def set_ids(m, k):
    m._anchor_target._next_image_id = m._proposal_target._next_image_id = k


def clear(m):
    for p in m.dense.parameters():
        p.grad = None


def loops(m, B, shape):
    images, boxes, labels = make_images(B, shape)
    four = (torch.cat(images), torch.cat(boxes), labels.repeat(B),
            torch.tensor([3 * b for b in range(B + 1)], dtype=torch.int32, device='cuda'))

    def batched():
        set_ids(m, 0)
        sum(x.sum() for x in m(four, True)).backward()
        clear(m)

    def singles():
        set_ids(m, 0)
        for b in range(B):
            sum(m((images[b], boxes[b], labels), True)).backward()
        clear(m)
    return {'batched': batched, 'singles': singles}


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def alternate(fns):
    for _ in range(WARMUP):
        for fn in fns.values():
            fn()
    ts = {k: [] for k in fns}
    for _ in range(CALLS):
        for k, fn in fns.items():
            ts[k].append(timed(fn))
    return {k: float(np.median(v)) for k, v in ts.items()}


def bench(m, name, B):
    fns = loops(m, B, SIZES[name])
    per = [alternate(fns) for _ in range(ROUNDS)]
    med = {k: [p[k] for p in per] for k in fns}
    spread = max(max(v) - min(v) for v in med.values())
    row = dict(image=name, images=B, spread_ms=round(spread, 3))
    for k, v in med.items():
        row[k + '_ms'] = round(float(np.median(v)), 3)
        row[k + '_round_medians_ms'] = [round(x, 3) for x in v]
    row['batched_ms_per_image'] = round(row['batched_ms'] / B, 3)
    row['singles_over_batched'] = round(row['singles_ms'] / row['batched_ms'], 3)
    row['verdict'] = 'FASTER' if min(med['singles']) - max(med['batched']) > spread else 'SLOWER'
    print(json.dumps(row), flush=True)
    return row


def parity():
    """one two-image call against the two one-image calls on the tests' model (train_neck / train_rpn_head / train_roi_head, 32 RoI
    samples) and images: the front's byte equality, the largest relative loss difference and, per parameter, max|g2 - (g1_0 + g1_1)|
    / max|g1_0 + g1_1|"""
    m = make_model(train_extractor=False, train_stem=False, roi_training_total_num_samples=32, roi_training_max_pos_samples=8)
    m.keep_training_pass = True
    shape = list(SIZES['256x352'])
    images, boxes, labels = make_images(2, shape)
    for k, img in enumerate(images):                         # the tests' ground truth: three of the model's own proposals per image
        with torch.no_grad():
            scores, deltas = m._get_fpn_head_results(m._neck(m._extractor(img, training=True), training=True))
            rois = m._rpn_proposal((deltas, m._get_anchors(shape), m._fg_scores(scores), shape), training=True)
        big = rois[((rois[:, 2] - rois[:, 0]) >= 24) & ((rois[:, 3] - rois[:, 1]) >= 24)]
        boxes[k] = big[[0, big.shape[0] // 3, 2 * big.shape[0] // 3]].clone()
    named = list(m.dense.named_parameters())

    def call(ks, first_id):
        set_ids(m, first_id)
        four = (torch.cat([images[k] for k in ks]), torch.cat([boxes[k] for k in ks]), labels.repeat(len(ks)),
                torch.tensor([3 * b for b in range(len(ks) + 1)], dtype=torch.int32, device='cuda'))
        losses = m(four, True)
        sum(x.sum() for x in losses).backward()
        grads = {n: None if p.grad is None else p.grad.detach().double().cpu().numpy().copy() for n, p in named}
        clear(m)
        return torch.stack([x.detach() for x in losses]).double().cpu().numpy(), grads, m.last_training_pass
    l2, g2, r2 = call([0, 1], 5)
    ones = [call([k], 5 + k) for k in range(2)]
    front = all(torch.equal(r2[name][b], ones[b][2][name][0]) for b in range(2) for name in ('rpn_score', 'rpn_deltas')) and \
        all(torch.equal(p2[b], p1[0]) for b in range(2) for p2, p1 in zip(r2['maps'], ones[b][2]['maps']))
    loss = max(abs(l2[i, b] - ones[b][0][i, 0]) / abs(ones[b][0][i, 0]) for i in range(4) for b in range(2))
    grad = {}
    for n, g in g2.items():
        if g is not None:
            both = ones[0][1][n] + ones[1][1][n]
            grad[n] = float(np.abs(g - both).max() / np.abs(both).max())
    worst = max(grad, key=grad.get)
    return dict(front_bytes_equal=bool(front), largest_relative_loss_difference=float(loss),
                largest_relative_gradient_difference=grad[worst], parameter=worst, parameters=len(grad))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', help='output path (default profiles/train_call_bench.json)')
    ap.add_argument('--sizes', nargs='+', default=list(SIZES), choices=list(SIZES))
    ap.add_argument('--images', type=int, nargs='+', default=[1, 2, 4])
    ap.add_argument('--parity', action='store_true', help='also measure the two-image call against the two one-image calls')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    out = dict(device=torch.cuda.get_device_name(0),
               protocol='wall time, a synchronize on each side of forward plus backward; the two loops alternately, %d calls each after '
                        '%d warm-up calls, %d rounds; median of the round medians in milliseconds; spread_ms = the largest difference '
                        'between two round medians of one loop' % (CALLS, WARMUP, ROUNDS))
    if a.parity:
        out['parity'] = parity()
        print(json.dumps(out['parity']), flush=True)
    m = make_model()
    rows = []
    for name in a.sizes:
        for B in a.images:
            rows.append(bench(m, name, B))
            torch.cuda.empty_cache()
    out['slower_than_singles'] = ['%s x %d images' % (r['image'], r['images']) for r in rows if r['verdict'] == 'SLOWER']
    out['rows'] = rows
    path = a.out or os.path.join(ROOT, 'profiles', 'train_call_bench.json')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
    print('wrote', path)


if __name__ == '__main__':
    main()
