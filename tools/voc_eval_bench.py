"""The accuracy gate's evaluation, host against GPU, on a seeded synthetic set: precision_gate.paired_map_delta (numpy,
Python loops) and voc_eval_gpu.paired_map_delta_gpu (odet_voc_match / odet_coco_order / odet_voc_accumulate /
odet_voc_bootstrap) on the same detections in the same process.  Checks that the two results are equal and writes the
record: host seconds, GPU-path seconds end to end (packing, copies, launches, host reductions) and the split of the GPU
path (kernel times from HIP events).  One warm-up, then the median of --reps runs with min and max.

    python tools/voc_eval_bench.py [--scenes 4096] [--dets 50] [--classes 20] [--resamples 400] [--reps 5]
                                   [--host-reps 5] [--out profiles/voc_eval_r08.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic_sets(scenes, dets_per_image, classes, seed=8):
    """-> (dets_a, dets_b, gt_boxes, gt_labels) in the list form the gate holds: dets[i][j] float32 [n,5] (index 0
    unused), gt_boxes[i] float32 [g,4], gt_labels[i] int32 [g].  3-8 boxes per scene; 60 % of the detections are
    jittered ground truth (mostly the right class), the rest clutter; scores rounded to two decimals; set b is set a
    with every fifth detection moved and re-scored (two modes of one detector)."""
    rng = np.random.default_rng(seed)
    nc = classes + 1
    ng = rng.integers(3, 9, scenes)
    G = int(ng.sum())
    g_img = np.repeat(np.arange(scenes), ng)
    xy = rng.uniform(0, 900, (G, 2))
    wh = np.exp(rng.uniform(np.log(40), np.log(400), (G, 2)))
    g_box = np.floor(np.concatenate([xy, xy + wh], 1)).astype(np.float32)
    g_lab = rng.integers(1, nc, G).astype(np.int32)
    g_start = np.concatenate([[0], np.cumsum(ng)])
    D = scenes * dets_per_image
    d_img = np.repeat(np.arange(scenes), dets_per_image)
    own = rng.random(D) < 0.6
    pick = g_start[d_img] + (rng.random(D) * ng[d_img]).astype(np.int64)
    gb = g_box[pick].astype(np.float64)
    size = np.stack([gb[:, 2] - gb[:, 0], gb[:, 3] - gb[:, 1]] * 2, 1)
    jb = gb + rng.normal(0, 0.1, (D, 4)) * size
    cxy = rng.uniform(0, 900, (D, 2))
    clutter = np.concatenate([cxy, cxy + np.exp(rng.uniform(np.log(30), np.log(400), (D, 2)))], 1)
    box = np.where(own[:, None], jb, clutter)
    lab = np.where(own & (rng.random(D) < 0.85), g_lab[pick], rng.integers(1, nc, D))
    score = np.round(np.where(own, rng.uniform(0.2, 1.0, D), rng.uniform(0.05, 0.7, D)), 2)
    a = np.concatenate([box, score[:, None]], 1).astype(np.float32)
    move = rng.random(D) < 0.2
    b = a.copy()
    b[move, :4] += (rng.normal(0, 0.04, (D, 4)) * size)[move].astype(np.float32)
    b[move, 4] = np.round(np.clip(b[move, 4] + rng.normal(0, 0.03, int(move.sum())), 0.05, 1.0), 2)

    def lists(rows):
        key = d_img * nc + lab
        o = np.argsort(key, kind='stable')
        cut = np.searchsorted(key[o], np.arange(scenes * nc + 1), 'left')
        rows = rows[o]
        return [[rows[cut[i * nc + j]:cut[i * nc + j + 1]] for j in range(nc)] for i in range(scenes)]

    gt_boxes = [g_box[g_start[i]:g_start[i + 1]] for i in range(scenes)]
    gt_labels = [g_lab[g_start[i]:g_start[i + 1]] for i in range(scenes)]
    return lists(a), lists(b), gt_boxes, gt_labels


def _stats(v):
    return {'median': float(np.median(v)), 'min': float(np.min(v)), 'max': float(np.max(v)), 'runs': len(v)}


def gpu_split(dets_a, dets_b, gt_boxes, gt_labels, nc, resamples, seed):
    """paired_map_delta_gpu's own steps with a clock around each: -> (result, seconds per stage)"""
    import torch
    from tf_eager_object_detection_amd.evaluation import voc_eval_gpu as vg
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pk = vg._pack_pair(dets_a, dets_b, gt_boxes, gt_labels, nc)
    t1 = time.perf_counter()
    counts = vg._draw_counts(pk['num_images'], resamples, seed)
    t2 = time.perf_counter()
    out = vg._run_gpu(pk, 'cuda', 0.5, counts, vg.AP_07, events=ev)
    t3 = time.perf_counter()
    ap, npos = out['boot_ap'].cpu().numpy(), out['boot_npos'].cpu().numpy()
    t4 = time.perf_counter()
    maps = vg._maps_from_boot(ap, npos, nc - 1)
    ds = maps[1:, 1] - maps[1:, 0]
    res = dict(map_a=float(maps[0, 0]), map_b=float(maps[0, 1]), delta=float(maps[0, 1]) - float(maps[0, 0]),
               delta_boot_mean=float(ds.mean()), delta_boot_std=float(ds.std()),
               delta_ci95=[float(np.percentile(ds, 2.5)), float(np.percentile(ds, 97.5))], resamples=resamples)
    t5 = time.perf_counter()
    ms = lambda i: ev[i].elapsed_time(ev[i + 1]) / 1e3
    return res, {'pack': t1 - t0, 'draw_counts': t2 - t1, 'copy_in': ms(0), 'match': ms(1), 'order': ms(2),
                 'accumulate': ms(3), 'bootstrap': ms(4), 'enqueue_wall': t3 - t2, 'wait_and_copy_out': t4 - t3,
                 'host_reductions': t5 - t4, 'total': t5 - t0,
                 'segments': pk['num_segments'], 'entries': pk['num_entries']}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scenes', type=int, default=4096)
    ap.add_argument('--dets', type=int, default=50, help='detections per image and set')
    ap.add_argument('--classes', type=int, default=20)
    ap.add_argument('--resamples', type=int, default=400)
    ap.add_argument('--reps', type=int, default=5, help='timed runs of the GPU path (after one warm-up)')
    ap.add_argument('--host-reps', type=int, default=5, help='timed runs of the host path (after one warm-up)')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'voc_eval_r08.json'))
    a = ap.parse_args()
    if a.reps < 1 or a.host_reps < 1:
        ap.error('--reps and --host-reps must be at least 1')
    import torch
    from tf_eager_object_detection_amd.evaluation import precision_gate as pg
    from tf_eager_object_detection_amd.evaluation import voc_eval_gpu as vg
    nc = a.classes + 1
    t0 = time.perf_counter()
    da, db, gb, gl = synthetic_sets(a.scenes, a.dets, a.classes)
    build_s = time.perf_counter() - t0
    args = (da, db, gb, gl, nc)
    kw = dict(resamples=a.resamples, seed=a.seed)

    gpu_s, split, got = [], [], None
    for r in range(a.reps + 1):                                    # (run 0: warm-up)
        torch.cuda.synchronize()
        t = time.perf_counter()
        got = vg.paired_map_delta_gpu(*args, **kw)
        gpu_s.append(time.perf_counter() - t)
        res, sp = gpu_split(*args, a.resamples, a.seed)
        assert res == got
        split.append(sp)
    got_area = vg.paired_map_delta_gpu(*args, resamples=0, seed=a.seed, use_07_metric=False)
    host_s, want = [], None
    for r in range(a.host_reps + 1):
        t = time.perf_counter()
        want = pg.paired_map_delta(*args, **kw)
        host_s.append(time.perf_counter() - t)
        print('host run %d: %.2f s' % (r, host_s[-1]), flush=True)
    want_area = pg.paired_map_delta(*args, resamples=0, seed=a.seed, use_07_metric=False)
    equal = got == want and got_area == want_area
    gpu, host = _stats(gpu_s[1:]), _stats(host_s[1:])
    keys = [k for k in split[0] if k not in ('segments', 'entries')]
    rec = {
        'what': 'precision_gate.paired_map_delta (host) against voc_eval_gpu.paired_map_delta_gpu (GPU path end to end: '
                'packing, copies, launches, host reductions) on the same seeded synthetic detections, same process',
        'how_built': 'python tools/voc_eval_bench.py (one warm-up of each path, then the timed runs)',
        'set': {'scenes': a.scenes, 'sets': 2, 'detections_per_image_and_set': a.dets, 'classes': a.classes,
                'resamples': a.resamples, 'scores': 'rounded to two decimals', 'seed': a.seed,
                'segments': split[0]['segments'], 'entries': split[0]['entries'], 'build_set_s': build_s},
        'results_equal': bool(equal), 'result': got, 'result_area_metric_resamples_0': got_area,
        'host_s': host, 'gpu_path_s': gpu, 'ratio_host_over_gpu_path_medians': host['median'] / gpu['median'],
        'host_ms_per_scene': 1e3 * host['median'] / a.scenes, 'gpu_path_ms_per_scene': 1e3 * gpu['median'] / a.scenes,
        'gpu_path_split_s_median': {k: float(np.median([s[k] for s in split[1:]])) for k in keys},
        'gpu_path_split_s_min': {k: float(np.min([s[k] for s in split[1:]])) for k in keys},
        'gpu_path_split_s_max': {k: float(np.max([s[k] for s in split[1:]])) for k in keys},
        'split_note': 'copy_in, match, order, accumulate, bootstrap: HIP events on the stream (copy_in includes pinning the '
                      'host arrays); pack, draw_counts, enqueue_wall, wait_and_copy_out, host_reductions: host clock; '
                      'the events overlap enqueue_wall and wait_and_copy_out',
        'device': torch.cuda.get_device_name(0),
    }
    print(json.dumps({k: rec[k] for k in ('results_equal', 'host_s', 'gpu_path_s', 'ratio_host_over_gpu_path_medians',
                                          'gpu_path_split_s_median')}))
    if a.out:
        with open(a.out, 'w') as f:
            f.write(json.dumps(rec, indent=1) + '\n')
    if not equal:
        print('host:', want, want_area, '\ngpu: ', got, got_area)
        sys.exit(1)


if __name__ == '__main__':
    main()
