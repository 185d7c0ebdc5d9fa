#!/usr/bin/env python3
"""Times the FPN RoI head's backward launches (csrc/dense_grad.hip) at rows = 256, C = 21 and C = 81, and the whole head
backward, against torch's own composition on the same tensors; writes profiles/dense_grad_bench.json.

  ours     ops.dense_wgrad (dw and db, the ReLU gate applied while staging) / ops.dense_dgrad.
  library  what autograd of F.linear + relu runs: dz = dy * (y > 0) (one elementwise launch, where the layer has a ReLU), then
           dz.t() @ x and dz.sum(0), resp. dz @ w -- the library GEMM.  `library_gemm_us` is the GEMM alone on a ready dz.
  head     the seven launches .backward() of roi_head_trainable enqueues (final wgrad + dgrad, fc2 wgrad + dgrad, fc1 wgrad; no
           input gradient for fc1) against the same chain of torch operations.

Clock: GPU time of INNER calls captured in one HIP graph and replayed; per row the two graphs are replayed alternately, REPLAYS
times each, after 3 warm-up replays; median and (min, max) per call in microseconds.  `gbytes_per_s` of the fc1 wgrad: the bytes
the algorithm needs (x and dy read once, y read once, dw written once) over the median, next to the 8 TB/s HBM roofline; its
`tflops` (2 rows cin cout) stands next to the 157.3 TFLOP/s float32 matrix peak, which is what bounds it at rows = 256.

    python tools/dense_grad_bench.py"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tf_eager_object_detection_amd import ops                                            # noqa: E402

INNER, REPLAYS = 10, 30
HBM_BYTES_PER_S, F32_MATRIX_FLOPS = 8.0e12, 157.3e12


def capture(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
        fn()
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


def alternate(graphs):
    """{name: graph} -> {name: (median, min, max)} microseconds per call, the graphs replayed in turn"""
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


def launch_rows(rng, layer, rows, cin, cout, relu, need_dx):
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).cuda()
    x, w, dy = f(rows, cin), f(cout, cin), f(rows, cout)
    y = f(rows, cout) if relu else None
    dz = dy * (y > 0) if relu else dy
    out = []

    def lib_wgrad():
        g = dy * (y > 0) if relu else dy
        return g.t() @ x, g.sum(0)

    kinds = [('wgrad', lambda: ops.dense_wgrad(dy, x, y), lib_wgrad, lambda: dz.t() @ x)]
    if need_dx:
        kinds.append(('dgrad', lambda: ops.dense_dgrad(dy, w, y), lambda: (dy * (y > 0) if relu else dy) @ w, lambda: dz @ w))
    for kind, ours, lib, gemm in kinds:
        t = alternate({'ours': capture(ours), 'library': capture(lib), 'library_gemm': capture(gemm)})
        row = dict(layer=layer, launch=kind, rows=rows, cin=cin, cout=cout, relu_gate=bool(relu),
                   split=bool(ops.L.lib().odet_dense_grad_workspace_bytes(1 if kind == 'wgrad' else 0, rows, cin, cout)))
        for k in ('ours', 'library', 'library_gemm'):
            stat(row, k, t[k])
        row['library_over_ours'] = round(t['library'][0] / t['ours'][0], 3)
        row['tflops'] = round(2.0 * rows * cin * cout / t['ours'][0] / 1e6, 2)
        if kind == 'wgrad':
            nbytes = 4 * (rows * cin + rows * cout * (2 if relu else 1) + cout * cin)
            row['bytes'] = nbytes
            row['gbytes_per_s'] = round(nbytes / t['ours'][0] / 1e3, 1)
            row['share_of_hbm_roofline'] = round(nbytes / t['ours'][0] * 1e6 / HBM_BYTES_PER_S, 4)
        row['share_of_f32_matrix_peak'] = round(row['tflops'] * 1e12 / F32_MATRIX_FLOPS, 4)
        print(json.dumps(row), flush=True)
        out.append(row)
    return out


def head_rows(rng, C, rows):
    """the head's seven backward launches in order (what .backward() of roi_head_trainable enqueues), against the same chain of
    torch operations; both without autograd's host work, which a graph replay does not have either"""
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).cuda()
    n5 = 5 * C
    pad = (n5 + 63) // 64 * 64
    x, h1, h2 = f(rows, 7 * 7 * 256).relu_(), f(rows, 1024).relu_(), f(rows, 1024).relu_()
    w2, w3 = f(1024, 1024), f(pad, 1024)
    w3[n5:] = 0
    dy = f(rows, pad)
    dy[:, n5:] = 0

    def ours():
        dw3, db3 = ops.dense_wgrad(dy, h2)
        dh2 = ops.dense_dgrad(dy, w3)
        dw2, db2 = ops.dense_wgrad(dh2, h1, h2)
        dh1 = ops.dense_dgrad(dh2, w2, h2)
        return dw3, db3, dw2, db2, ops.dense_wgrad(dh1, x, h1)

    def library():
        dyc = dy[:, :n5]
        dw3, db3 = dyc.t() @ h2, dyc.sum(0)
        dz2 = (dyc @ w3[:n5]) * (h2 > 0)
        dw2, db2 = dz2.t() @ h1, dz2.sum(0)
        dz1 = (dz2 @ w2) * (h1 > 0)
        return dw3, db3, dw2, db2, dz1.t() @ x, dz1.sum(0)
    t = alternate({'ours': capture(ours), 'library': capture(library)})
    row = dict(layer='whole head backward', rows=rows, C=C)
    stat(row, 'ours', t['ours'])
    stat(row, 'library', t['library'])
    row['library_over_ours'] = round(t['library'][0] / t['ours'][0], 3)
    print(json.dumps(row), flush=True)
    return [row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', help='output path (default profiles/dense_grad_bench.json)')
    ap.add_argument('--rows', type=int, default=256)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    rng = np.random.default_rng(0)
    R = a.rows
    rows = launch_rows(rng, 'fc1', R, 7 * 7 * 256, 1024, True, False)
    rows += launch_rows(rng, 'fc2', R, 1024, 1024, True, True)
    for C in (21, 81):
        rows += launch_rows(rng, 'final (C = %d)' % C, R, 1024, (5 * C + 63) // 64 * 64, False, True)
    for C in (21, 81):
        rows += head_rows(rng, C, R)
    slower = [(r['layer'], r.get('launch', '')) for r in rows if r['library_over_ours'] < 1.0]
    out = dict(device=torch.cuda.get_device_name(0),
               protocol='%d calls per HIP graph; ours / library / library_gemm graphs replayed alternately, %d replays each after 3 '
                        'warm-up replays; median and [min, max] microseconds per call' % (INNER, REPLAYS),
               hbm_roofline_bytes_per_s=HBM_BYTES_PER_S, f32_matrix_peak_flops=F32_MATRIX_FLOPS, slower_than_library=slower, rows=rows)
    path = a.out or os.path.join(ROOT, 'profiles', 'dense_grad_bench.json')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
    print('wrote', path)


if __name__ == '__main__':
    main()
