#!/usr/bin/env python3
"""Times one training step (L2 regulariser + bias doubling + schedule + Momentum / Adam update) on the parameter shapes of
ResNet-101-FPN two ways; writes profiles/optimizer_bench.json.

  fused      training.MomentumOptimizer / AdamOptimizer.apply_gradients: one update launch over all chunks + one finish launch
             (csrc/optimizer.hip).
               us       GPU time: INNER steps captured in one HIP graph, replayed after 3 warm-up replays, median of 20 replays /
                        INNER (us_min / us_max: the spread over the replays);
               wall_us  the same call eagerly: synchronised wall time, median of 10 calls (table look-up and launches included).
  composed   the same update written with torch tensor operations, one tensor after the other: what a caller had to write
             before the fused step existed (same formulas; its sums are torch's, not the ordered float64 sum).  Timed the same
             two ways (one step per graph: it is more than a thousand launches).

Rows: float32 parameters, and float16 parameters with float32 masters and float16 gradients; momentum and adam; each with and
without the L2 output.  The shapes are ResNetFpnDetector(101).named_parameters(), weight decay on every kernel (dim >= 2),
scale 2 on every bias.  bytes = what one step has to move (every array read once, every updated array written once);
hbm_frac = bytes / us / 8 TB/s, the data-sheet figure this project quotes fractions of.

    python tools/optimizer_bench.py"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tf_eager_object_detection_amd import training                                        # noqa: E402
from tf_eager_object_detection_amd.model.fpn_detector import ResNetFpnDetector            # noqa: E402

PEAK = 8e12
INNER = 10
LR, MU, B1, B2, EPS, WD = 0.01, 0.9, 0.9, 0.999, 1e-8, 1e-4


def graph_us(fn, inner, replays=20):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s), torch.cuda.graph(g, stream=s):
        for _ in range(inner):
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
        ts.append(a.elapsed_time(b) * 1e3 / inner)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def wall_us(fn, calls=10):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e6)
    return float(np.median(ts))


class Composed:
    """the step as per-tensor torch operations (float32 arithmetic in the fused step's order; masters for float16 variables)"""

    def __init__(self, kind, variables, grads, wds, scales, l2):
        self.kind, self.vars, self.grads, self.wds, self.scales, self.l2 = kind, variables, grads, wds, scales, l2
        self.w32 = [v.float() if v.dtype == torch.float16 else v for v in variables]
        self.s0 = [torch.zeros_like(w) for w in self.w32]
        self.s1 = [torch.zeros_like(w) for w in self.w32] if kind == 'adam' else None
        self.b1p, self.b2p = B1, B2

    def __call__(self):
        total = None
        alpha = LR * (1.0 - self.b2p) ** 0.5 / (1.0 - self.b1p)
        for i, (v, w, g) in enumerate(zip(self.vars, self.w32, self.grads)):
            wd = self.wds[i]
            if self.l2 and wd:
                loss = wd * (w * w).sum(dtype=torch.float64).float()
                total = loss if total is None else total + loss
            g = g.float() if g.dtype == torch.float16 else g
            if wd:
                g = g + wd * (2.0 * w)
            if self.scales[i] != 1.0:
                g = g * self.scales[i]
            if self.kind == 'momentum':
                self.s0[i].mul_(MU).add_(g)
                w.sub_(self.s0[i] * LR)
            else:
                self.s0[i].add_((g - self.s0[i]) * (1.0 - B1))
                self.s1[i].add_((g * g - self.s1[i]) * (1.0 - B2))
                w.sub_((self.s0[i] * alpha) / (self.s1[i].sqrt() + EPS))
            if v is not w:
                v.copy_(w)
        return total


def step_bytes(kind, variables, f16):
    n = sum(v.numel() for v in variables)
    slots = 1 if kind == 'momentum' else 2
    per = 8 + 8 * slots + (2 + 2 if f16 else 4)       # w (or master) r+w, slots r+w, float16: variable write + float16 gradient
    return n * per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', help='output path (default profiles/optimizer_bench.json)')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    model = ResNetFpnDetector(101, 21, (800, 1333), 1000, dtype=torch.float32)
    named = [(n, tuple(p.shape)) for n, p in model.named_parameters()]
    del model
    names = [n for n, _ in named]
    wds = [WD if len(s) >= 2 else 0.0 for _, s in named]
    scales = training.grad_scales(names, True)
    gen = torch.Generator(device='cuda')
    gen.manual_seed(1)
    rows = []
    for f16 in (False, True):
        dt = torch.float16 if f16 else torch.float32
        for kind in ('momentum', 'adam'):
            for l2 in (False, True):
                variables = [(torch.randn(s, device='cuda', generator=gen) * 0.05).to(dt) for _, s in named]
                grads = [(torch.randn(s, device='cuda', generator=gen) * 0.01).to(dt) for _, s in named]
                opt = training.MomentumOptimizer(LR, MU) if kind == 'momentum' else training.AdamOptimizer(LR, B1, B2, EPS)
                gv = list(zip(grads, variables))

                def fused():
                    return opt.apply_gradients(gv, grad_scales=scales, weight_decays=wds, l2=l2)
                opt.prepare(gv, grad_scales=scales, weight_decays=wds)
                us, lo, hi = graph_us(fused, INNER)
                w_us = wall_us(fused)
                cvars = [v.clone() for v in variables]
                composed = Composed(kind, cvars, grads, wds, scales, l2)
                c_us, c_lo, c_hi = graph_us(composed, 1, replays=10)
                c_wall = wall_us(composed, calls=5)
                nbytes = step_bytes(kind, variables, f16)
                row = dict(kind=kind, dtype='float16+master' if f16 else 'float32', l2=l2, tensors=len(named),
                           elements=sum(v.numel() for v in variables), bytes=nbytes, us=round(us, 1), us_min=round(lo, 1),
                           us_max=round(hi, 1), wall_us=round(w_us, 1), gb_per_s=round(nbytes / us / 1e3, 1),
                           hbm_frac=round(nbytes / (us * 1e-6) / PEAK, 3), composed_us=round(c_us, 1),
                           composed_us_min=round(c_lo, 1), composed_us_max=round(c_hi, 1), composed_wall_us=round(c_wall, 1))
                row['composed_vs_fused'] = round(c_us / us, 1)
                row['composed_vs_fused_wall'] = round(c_wall / w_us, 1)
                print(json.dumps(row), flush=True)
                rows.append(row)
                del variables, grads, cvars, composed, opt, gv
                torch.cuda.empty_cache()
    out = dict(device=torch.cuda.get_device_name(0),
               protocol='us: %d fused steps (composed: 1 step) per HIP graph, 3 warm-up replays, median / min / max of 20 (10) '
                        'replays; wall_us: synchronised wall time, median of 10 (5) calls after 2; hbm_frac: bytes / us / 8 TB/s'
                        % INNER, rows=rows)
    path = a.out or os.path.join(ROOT, 'profiles', 'optimizer_bench.json')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
    print('wrote', path)


if __name__ == '__main__':
    main()
