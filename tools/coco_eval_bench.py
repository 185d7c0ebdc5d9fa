"""COCO bbox evaluation timing on a seeded val2017-sized set (5000 images, 80 categories, ~7 GT and 100 detections per
image): host packing, the three launches (odet_coco_match / odet_coco_order / odet_coco_accumulate, HIP events), and --
with --restatement, which needs no GPU -- one run of the plain-Python COCOeval restatement of tests/coco_eval_np.py.

    python tools/coco_eval_bench.py [--reps 20] [--out FILE]          # GPU part
    python tools/coco_eval_bench.py --restatement [--out FILE]        # CPU restatement (minutes)
    rocprofv3 --kernel-trace --stats -d DIR -o coco -- python tools/coco_eval_bench.py --reps 3
    python tools/coco_eval_bench.py --merge GPU.json RESTATEMENT.json DIR/.../coco_results.db --out FILE

--merge builds the committed record (profiles/coco_eval_<tag>.json) from the three runs: the GPU part, the restatement
part, and the per-kernel durations of the rocprofv3 trace (its `kernels` table, summed per kernel name and divided by
the --reps + 3 calls of that run: the warm-up calls, the timed ones and the checking coco_evaluate).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def val_sized_set(seed=2017, n_img=5000, n_cat=80, gt_per_img=7, det_per_img=100):
    """vectorised: GT boxes with an area field below the box area (1 % crowd, some areas on the range bounds), 60 % of
    the detections jittered GT boxes (mostly the right category), the rest clutter; two-decimal scores."""
    rng = np.random.default_rng(seed)
    img_ids = np.sort(rng.choice(np.arange(1, 600000), n_img, replace=False))
    cat_ids = np.sort(rng.choice(np.arange(1, 91), n_cat, replace=False))
    ng = rng.poisson(gt_per_img, n_img)
    g_img = np.repeat(img_ids, ng)
    G = len(g_img)
    g_cat = cat_ids[np.minimum(rng.zipf(1.3, G), n_cat) - 1]
    wh = np.round(np.exp(rng.uniform(np.log(4), np.log(400), (G, 2))), 2)
    xy = np.round(rng.uniform(0, 500, (G, 2)), 2)
    area = wh[:, 0] * wh[:, 1] * rng.uniform(0.55, 1.0, G)
    u = rng.random(G)
    area[u < 0.02] = 1024.0
    area[(u >= 0.02) & (u < 0.04)] = 9216.0
    crowd = (rng.random(G) < 0.01).astype(int)
    anns = [{'id': i + 1, 'image_id': int(g_img[i]), 'category_id': int(g_cat[i]),
             'bbox': [float(xy[i, 0]), float(xy[i, 1]), float(wh[i, 0]), float(wh[i, 1])], 'area': float(area[i]),
             'iscrowd': int(crowd[i])} for i in range(G)]
    D = n_img * det_per_img
    d_img_idx = np.repeat(np.arange(n_img), det_per_img)
    g_start = np.concatenate([[0], np.cumsum(ng)])
    has = ng[d_img_idx] > 0
    own = has & (rng.random(D) < 0.6)
    pick = g_start[d_img_idx] + (rng.random(D) * np.maximum(ng[d_img_idx], 1)).astype(np.int64)
    pick = np.minimum(pick, max(G - 1, 0))
    jit = rng.normal(0, 0.08, (D, 4))
    box = np.round(np.concatenate([rng.uniform(0, 500, (D, 2)), rng.uniform(2, 200, (D, 2))], 1), 2)
    gb = np.concatenate([xy, wh], 1)[pick]
    jb = np.round(np.stack([gb[:, 0] + jit[:, 0] * gb[:, 2], gb[:, 1] + jit[:, 1] * gb[:, 3],
                            gb[:, 2] * (1 + jit[:, 2]), gb[:, 3] * (1 + jit[:, 3])], 1), 2)
    box = np.where(own[:, None], jb, box)
    cat = np.where(own & (rng.random(D) < 0.85), g_cat[pick], cat_ids[rng.integers(0, n_cat, D)])
    score = np.round(rng.random(D), 2)
    res = [{'image_id': int(img_ids[d_img_idx[i]]), 'category_id': int(cat[i]), 'bbox': box[i].tolist(),
            'score': float(score[i])} for i in range(D)]
    gt = {'images': [{'id': int(i)} for i in img_ids], 'categories': [{'id': int(c)} for c in cat_ids],
          'annotations': anns}
    return gt, res


def gpu_part(gt, res, reps):
    import torch
    from tf_eager_object_detection_amd.evaluation import coco_eval as ce
    g = ce.load_coco_gt(gt)
    t0 = time.perf_counter()
    pk = ce._pack(g, res, None)
    pack_s = time.perf_counter() - t0
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    stages = {'match': [], 'order': [], 'accumulate': []}
    walls = []
    for r in range(reps + 2):
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        out = ce._run_gpu(pk, 'cuda', events=ev)
        prec = out['precision'].cpu()
        walls.append(time.perf_counter() - w0)
        if r >= 2:
            stages['match'].append(ev[0].elapsed_time(ev[1]))
            stages['order'].append(ev[1].elapsed_time(ev[2]))
            stages['accumulate'].append(ev[2].elapsed_time(ev[3]))
    full = ce.coco_evaluate(g, res)
    assert np.array_equal(full['precision'], prec.numpy())
    med = {k: float(np.median(v)) for k, v in stages.items()}
    return {
        'segments': int(len(pk['segs'])), 'entries': pk['num_entries'], 'gt': int(len(pk['gt_area'])),
        'detections': int(len(pk['dt_score'])), 'max_seg_dets': pk['max_seg_dets'], 'max_seg_gt': pk['max_seg_gt'],
        'host_pack_s': pack_s,
        'kernel_ms_median': med, 'kernel_ms_all': stages, 'kernel_ms_total_median': float(sum(med.values())),
        'dominant_stage': max(med, key=med.get),
        'wall_s_run_gpu_plus_copy_median': float(np.median(walls[2:])),
        'stats': [float(v) for v in full['stats']], 'reps': reps,
        'device': torch.cuda.get_device_name(0),
    }


def restatement_part(gt, res):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from coco_eval_np import CocoEvalNp
    t0 = time.perf_counter()
    ev = CocoEvalNp(gt, res)
    ev.evaluate()
    t1 = time.perf_counter()
    ev.accumulate()
    t2 = time.perf_counter()
    ev.summarize()
    return {'restatement_evaluate_s': t1 - t0, 'restatement_accumulate_s': t2 - t1,
            'restatement_total_s': time.perf_counter() - t0, 'stats': [float(v) for v in ev.stats]}


def merge(gpu_json, restatement_json, rocprof_db, calls):
    import sqlite3
    g = json.load(open(gpu_json))
    r = json.load(open(restatement_json))
    con = sqlite3.connect(rocprof_db)
    kern = [dict(kernel=n, calls=c, total_ns=t, avg_ns=a, min_ns=lo, max_ns=hi) for n, c, t, a, lo, hi in con.execute(
        "select name, count(*), sum(duration), avg(duration), min(duration), max(duration) from kernels "
        "where name like '%coco%' or name like '%k_rs_%' group by name order by sum(duration) desc")]
    stage = lambda f: round(sum(k['total_ns'] for k in kern if f(k['kernel'])) / calls / 1000.0, 1)
    return {
        'what': 'COCO bbox evaluation (odet_coco_match / odet_coco_order / odet_coco_accumulate) on the seeded '
                'val2017-sized set of tools/coco_eval_bench.py',
        'how_built': 'tools/coco_eval_bench.py --merge of three runs: the GPU part (--reps %d), the --restatement part '
                     '(CPU only) and a rocprofv3 --kernel-trace run of the GPU part' % g['reps'],
        'gpu': {k: v for k, v in g.items() if k != 'stats'},
        'rocprofv3_kernel_trace': {
            'calls': calls, 'kernels': kern,
            'note': 'order = k_coco_key_* + k_coco_compose + 3 x (k_rs_init + 3 k_rs_hist + 4 k_rs_scatter)',
            'per_call_us': {'match': stage(lambda n: 'k_coco_match' in n),
                            'order': stage(lambda n: 'k_coco_match' not in n and 'k_coco_accumulate' not in n),
                            'accumulate': stage(lambda n: 'k_coco_accumulate' in n)}},
        'restatement_cpu': {k: v for k, v in r.items() if k not in ('set', 'stats', 'build_set_s')},
        'stats_equal_gpu_vs_restatement': g['stats'] == r['stats'], 'stats': g['stats'], 'set': g['set']}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--restatement', action='store_true')
    ap.add_argument('--out', default=None)
    ap.add_argument('--merge', nargs=3, metavar=('GPU_JSON', 'RESTATEMENT_JSON', 'ROCPROF_DB'), default=None)
    ap.add_argument('--merge-calls', type=int, default=6, help='calls in the traced run (its --reps + 3)')
    a = ap.parse_args()
    if a.merge:
        rec = merge(*a.merge, calls=a.merge_calls)
        print(json.dumps(rec['rocprofv3_kernel_trace']['per_call_us']))
        if a.out:
            with open(a.out, 'w') as f:
                f.write(json.dumps(rec, indent=1) + '\n')
        return
    t0 = time.perf_counter()
    gt, res = val_sized_set()
    rec = {'set': {'images': 5000, 'categories': 80, 'gt_per_image': 7, 'detections_per_image': 100, 'seed': 2017},
           'build_set_s': time.perf_counter() - t0}
    rec.update(restatement_part(gt, res) if a.restatement else gpu_part(gt, res, a.reps))
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(json.dumps(rec, indent=1) + '\n')


if __name__ == '__main__':
    main()
