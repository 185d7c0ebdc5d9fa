"""Independent restatement of pycocotools' COCOeval for iouType 'bbox' (test infrastructure, not a dependency):
COCO.loadRes, COCOeval._prepare / computeIoU / evaluateImg / accumulate / summarize and maskApi.c bbIou, written with
dicts and loops shaped like pycocotools'.  It shares no code with the package's packing."""
import json
from collections import defaultdict

import numpy as np

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
MAX_DETS = [1, 10, 100]
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
AREA_LBL = ['all', 'small', 'medium', 'large']


def bb_iou(dt, gt, iscrowd):
    """maskApi.c bbIou: dt [m] and gt [n] xywh lists -> [m, n] (float64)."""
    m, n = len(dt), len(gt)
    o = np.zeros((m, n))
    for g in range(n):
        G = gt[g]
        ga = G[2] * G[3]
        crowd = iscrowd[g]
        for d in range(m):
            D = dt[d]
            da = D[2] * D[3]
            w = min(D[2] + D[0], G[2] + G[0]) - max(D[0], G[0])
            if w <= 0:
                continue
            h = min(D[3] + D[1], G[3] + G[1]) - max(D[1], G[1])
            if h <= 0:
                continue
            i = w * h
            u = da if crowd else da + ga - i
            o[d, g] = i / u
    return o


class CocoEvalNp:
    def __init__(self, gt_dict, results, img_ids=None):
        if isinstance(results, str):
            with open(results) as f:
                results = json.load(f)
        self.gt_imgs = [im['id'] for im in gt_dict['images']]
        self.cat_ids = sorted(c['id'] for c in gt_dict['categories'])
        self.gt_anns = [dict(a) for a in gt_dict.get('annotations', [])]
        # loadRes (bbox)
        assert set(r['image_id'] for r in results) <= set(self.gt_imgs), 'Results do not correspond to current coco set'
        self.dt_anns = []
        for i, r in enumerate(results):
            a = dict(r)
            bb = a['bbox']
            a['area'] = bb[2] * bb[3]
            a['id'] = i + 1
            a['iscrowd'] = 0
            self.dt_anns.append(a)
        self.img_ids = sorted(set(self.gt_imgs if img_ids is None else img_ids))

    def _anns(self, anns):
        by_img = defaultdict(list)
        for a in anns:
            by_img[a['image_id']].append(a)
        out = []
        cats = set(self.cat_ids)
        for i in self.img_ids:
            out.extend(a for a in by_img.get(i, []) if a['category_id'] in cats)
        return out

    def _prepare(self):
        gts = self._anns(self.gt_anns)
        dts = self._anns(self.dt_anns)
        for gt in gts:
            gt['ignore'] = gt['ignore'] if 'ignore' in gt else 0
            gt['ignore'] = 'iscrowd' in gt and gt['iscrowd']
        self._gts = defaultdict(list)
        self._dts = defaultdict(list)
        for gt in gts:
            self._gts[gt['image_id'], gt['category_id']].append(gt)
        for dt in dts:
            self._dts[dt['image_id'], dt['category_id']].append(dt)

    def computeIoU(self, imgId, catId):
        gt = self._gts[imgId, catId]
        dt = self._dts[imgId, catId]
        if len(gt) == 0 and len(dt) == 0:
            return []
        inds = np.argsort([-d['score'] for d in dt], kind='mergesort')
        dt = [dt[i] for i in inds]
        if len(dt) > MAX_DETS[-1]:
            dt = dt[0:MAX_DETS[-1]]
        if len(dt) == 0 or len(gt) == 0:
            return []
        g = [g['bbox'] for g in gt]
        d = [d['bbox'] for d in dt]
        iscrowd = [int(o['iscrowd']) for o in gt]
        return bb_iou(d, g, iscrowd)

    def evaluateImg(self, imgId, catId, aRng, maxDet):
        gt = self._gts[imgId, catId]
        dt = self._dts[imgId, catId]
        if len(gt) == 0 and len(dt) == 0:
            return None
        for g in gt:
            if g['ignore'] or (g['area'] < aRng[0] or g['area'] > aRng[1]):
                g['_ignore'] = 1
            else:
                g['_ignore'] = 0
        gtind = np.argsort([g['_ignore'] for g in gt], kind='mergesort')
        gt = [gt[i] for i in gtind]
        dtind = np.argsort([-d['score'] for d in dt], kind='mergesort')
        dt = [dt[i] for i in dtind[0:maxDet]]
        iscrowd = [int(o['iscrowd']) for o in gt]
        ious = self.ious[imgId, catId][:, gtind] if len(self.ious[imgId, catId]) > 0 else self.ious[imgId, catId]
        T = len(IOU_THRS)
        G = len(gt)
        D = len(dt)
        gtm = np.zeros((T, G))
        dtm = np.zeros((T, D))
        gtIg = np.array([g['_ignore'] for g in gt])
        dtIg = np.zeros((T, D))
        if not len(ious) == 0:
            for tind, t in enumerate(IOU_THRS):
                for dind, d in enumerate(dt):
                    iou = min([t, 1 - 1e-10])
                    m = -1
                    for gind, g in enumerate(gt):
                        if gtm[tind, gind] > 0 and not iscrowd[gind]:
                            continue
                        if m > -1 and gtIg[m] == 0 and gtIg[gind] == 1:
                            break
                        if ious[dind, gind] < iou:
                            continue
                        iou = ious[dind, gind]
                        m = gind
                    if m == -1:
                        continue
                    dtIg[tind, dind] = gtIg[m]
                    dtm[tind, dind] = gt[m]['id']
                    gtm[tind, m] = d['id']
        a = np.array([d['area'] < aRng[0] or d['area'] > aRng[1] for d in dt]).reshape((1, len(dt)))
        dtIg = np.logical_or(dtIg, np.logical_and(dtm == 0, np.repeat(a, T, 0)))
        return {'image_id': imgId, 'category_id': catId, 'aRng': aRng, 'maxDet': maxDet,
                'dtScores': [d['score'] for d in dt], 'dtMatches': dtm, 'gtIgnore': gtIg, 'dtIgnore': dtIg}

    def evaluate(self):
        self._prepare()
        self.ious = {(imgId, catId): self.computeIoU(imgId, catId) for imgId in self.img_ids for catId in self.cat_ids}
        maxDet = MAX_DETS[-1]
        self.evalImgs = [self.evaluateImg(imgId, catId, areaRng, maxDet)
                         for catId in self.cat_ids for areaRng in AREA_RNG for imgId in self.img_ids]

    def accumulate(self):
        T, R, K, A, M = len(IOU_THRS), len(REC_THRS), len(self.cat_ids), len(AREA_RNG), len(MAX_DETS)
        precision = -np.ones((T, R, K, A, M))
        recall = -np.ones((T, K, A, M))
        scores = -np.ones((T, R, K, A, M))
        I0, A0 = len(self.img_ids), len(AREA_RNG)
        for k in range(K):
            Nk = k * A0 * I0
            for a in range(A):
                Na = a * I0
                for m, maxDet in enumerate(MAX_DETS):
                    E = [self.evalImgs[Nk + Na + i] for i in range(I0)]
                    E = [e for e in E if e is not None]
                    if len(E) == 0:
                        continue
                    dtScores = np.concatenate([e['dtScores'][0:maxDet] for e in E])
                    inds = np.argsort(-dtScores, kind='mergesort')
                    dtScoresSorted = dtScores[inds]
                    dtm = np.concatenate([e['dtMatches'][:, 0:maxDet] for e in E], axis=1)[:, inds]
                    dtIg = np.concatenate([e['dtIgnore'][:, 0:maxDet] for e in E], axis=1)[:, inds]
                    gtIg = np.concatenate([e['gtIgnore'] for e in E])
                    npig = np.count_nonzero(gtIg == 0)
                    if npig == 0:
                        continue
                    tps = np.logical_and(dtm, np.logical_not(dtIg))
                    fps = np.logical_and(np.logical_not(dtm), np.logical_not(dtIg))
                    tp_sum = np.cumsum(tps, axis=1).astype(dtype=np.float64)
                    fp_sum = np.cumsum(fps, axis=1).astype(dtype=np.float64)
                    for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                        tp = np.array(tp)
                        fp = np.array(fp)
                        nd = len(tp)
                        rc = tp / npig
                        pr = tp / (fp + tp + np.spacing(1))
                        q = np.zeros((R,))
                        ss = np.zeros((R,))
                        if nd:
                            recall[t, k, a, m] = rc[-1]
                        else:
                            recall[t, k, a, m] = 0
                        pr = pr.tolist()
                        q = q.tolist()
                        for i in range(nd - 1, 0, -1):
                            if pr[i] > pr[i - 1]:
                                pr[i - 1] = pr[i]
                        inds = np.searchsorted(rc, REC_THRS, side='left')
                        try:
                            for ri, pi in enumerate(inds):
                                q[ri] = pr[pi]
                                ss[ri] = dtScoresSorted[pi]
                        except IndexError:
                            pass
                        precision[t, :, k, a, m] = np.array(q)
                        scores[t, :, k, a, m] = np.array(ss)
        self.eval = {'precision': precision, 'recall': recall, 'scores': scores}

    def summarize(self):
        def _summarize(ap=1, iouThr=None, areaRng='all', maxDets=100):
            aind = [i for i, aRng in enumerate(AREA_LBL) if aRng == areaRng]
            mind = [i for i, mDet in enumerate(MAX_DETS) if mDet == maxDets]
            if ap == 1:
                s = self.eval['precision']
                if iouThr is not None:
                    t = np.where(iouThr == IOU_THRS)[0]
                    s = s[t]
                s = s[:, :, :, aind, mind]
            else:
                s = self.eval['recall']
                if iouThr is not None:
                    t = np.where(iouThr == IOU_THRS)[0]
                    s = s[t]
                s = s[:, :, aind, mind]
            if len(s[s > -1]) == 0:
                mean_s = -1
            else:
                mean_s = np.mean(s[s > -1])
            return mean_s
        stats = np.zeros((12,))
        stats[0] = _summarize(1)
        stats[1] = _summarize(1, iouThr=.5, maxDets=MAX_DETS[2])
        stats[2] = _summarize(1, iouThr=.75, maxDets=MAX_DETS[2])
        stats[3] = _summarize(1, areaRng='small', maxDets=MAX_DETS[2])
        stats[4] = _summarize(1, areaRng='medium', maxDets=MAX_DETS[2])
        stats[5] = _summarize(1, areaRng='large', maxDets=MAX_DETS[2])
        stats[6] = _summarize(0, maxDets=MAX_DETS[0])
        stats[7] = _summarize(0, maxDets=MAX_DETS[1])
        stats[8] = _summarize(0, maxDets=MAX_DETS[2])
        stats[9] = _summarize(0, areaRng='small', maxDets=MAX_DETS[2])
        stats[10] = _summarize(0, areaRng='medium', maxDets=MAX_DETS[2])
        stats[11] = _summarize(0, areaRng='large', maxDets=MAX_DETS[2])
        self.stats = stats
        return stats

    def run(self):
        self.evaluate()
        self.accumulate()
        self.summarize()
        return self

    def segment_matches(self):
        """per (category, image) with an evalImg, in (category, image) order: (cat index, img index, dtScores,
        dtMatches != 0 [4, 10, D], dtIgnore [4, 10, D], npig per area [4]) -- the per-segment outputs of the match."""
        out = []
        I0, A0 = len(self.img_ids), len(AREA_RNG)
        for k in range(len(self.cat_ids)):
            for i in range(I0):
                es = [self.evalImgs[k * A0 * I0 + a * I0 + i] for a in range(A0)]
                if es[0] is None:
                    continue
                out.append((k, i, np.array(es[0]['dtScores'], np.float64),
                            np.stack([e['dtMatches'] != 0 for e in es]), np.stack([e['dtIgnore'] for e in es]),
                            np.array([np.count_nonzero(e['gtIgnore'] == 0) for e in es])))
        return out
