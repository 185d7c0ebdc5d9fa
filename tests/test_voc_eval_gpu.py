"""VOC evaluation and the gate's paired bootstrap on the GPU (-m gpu): the odet_voc_* launches against the reference's own
voc_eval results (tests/golden/ref_numpy_vectors.npz), against pascal_eval.voc_eval_arrays / evaluate_detections and
against precision_gate.paired_map_delta -- rec, prec, npos, the 11-point AP and everything derived from it exactly equal.
The area AP is checked against the bound of summing the same non-negative terms in any order, and -- because the kernel
restates np.sum's order of additions -- for equality as well."""
import os

import numpy as np
import pytest
import torch

from tf_eager_object_detection_amd import _lib as L
from tf_eager_object_detection_amd.evaluation import pascal_eval as pe
from tf_eager_object_detection_amd.evaluation import precision_gate as pg
from tf_eager_object_detection_amd.evaluation import voc_eval_gpu as vg
from voc_eval_sets import host_eval, random_set, to_flat

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def _area_close(got, want, m):
    """both sum the same m non-negative terms, each within (m-1) * 2^-53 relative of the true sum whatever the order:
    2 * (m-1) * 2^-53 relative between the two.  The kernel adds in numpy's order, so the two are equal as well."""
    tol = 2.0 * max(m - 1, 0) * U * abs(want)
    print('area AP: gpu %.17g host %.17g |diff| %.3g bound %.3g (m = %d)%s'
          % (got, want, abs(got - want), tol, m, '' if got == want else '  NOT EQUAL'))
    return abs(got - want) <= tol and got == want


def _check_against_host(dets, gb, gl, gd, nc, ovthresh, res=None):
    res = vg.voc_evaluate(dets, gb, gl, gd, nc, ovthresh) if res is None else res
    want = host_eval(pe, dets, gb, gl, gd, nc, ovthresh, True)
    want_area = host_eval(pe, dets, gb, gl, gd, nc, ovthresh, False)
    for k in range(nc - 1):
        rec, prec, ap07, npos = want[k]
        np.testing.assert_array_equal(res['rec'][k], rec, err_msg='rec of class %d' % (k + 1))
        np.testing.assert_array_equal(res['prec'][k], prec, err_msg='prec of class %d' % (k + 1))
        assert int(res['npos'][k]) == npos
        assert res['ap07'][k] == ap07, (k, res['ap07'][k], ap07)
        assert _area_close(float(res['ap_area'][k]), float(want_area[k][2]), len(rec) + 1), k
    return res, want


# 1 ---------------------------------------------------------------------------------------------------------------
def _ve_flat(golden):
    """the dataset the reference's own voc_eval ran on (tests/test_evaluation.py:_ve_case shows the layout) in the flat
    form: classes 0..2 of the file are labels 1..3"""
    nc = int(golden['ve_num_classes'])
    d = [golden['ve_dets_%d' % c] for c in range(nc)]             # rows (image, x1, y1, x2, y2, score) in file order
    g = golden['ve_gts']                                          # rows (image, class, x1, y1, x2, y2, difficult)
    dets = (np.concatenate([a[:, 0] for a in d]).astype(np.int64),
            np.concatenate([np.full(len(a), c + 1, np.int64) for c, a in enumerate(d)]),
            np.concatenate([a[:, 1:5] for a in d]), np.concatenate([a[:, 5] for a in d]))
    return dets, g[:, 0].astype(np.int64), g[:, 2:6], g[:, 1].astype(np.int64) + 1, g[:, 6].astype(bool), nc


def test_the_references_own_results():
    golden = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'ref_numpy_vectors.npz'))
    dets, gi, gbox, glab, ghard, nc = _ve_flat(golden)
    assert nc == 3 and ghard.any()
    res = vg.voc_evaluate(dets, gbox, glab, ghard, nc + 1, 0.5, gt_image_index=gi,
                          num_images=int(golden['ve_num_images']))
    for c in range(nc):
        np.testing.assert_array_equal(res['rec'][c], golden['ve_rec_%d' % c])
        np.testing.assert_array_equal(res['prec'][c], golden['ve_prec_%d' % c])
        assert res['ap07'][c] == float(golden['ve_ap07_%d' % c])
        assert _area_close(float(res['ap_area'][c]), float(golden['ve_aparea_%d' % c]), len(res['rec'][c]) + 1)


# 2, 3 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed,n_img,ovthresh', [(0, 40, 0.5), (1, 300, 0.3), (2, 2000, 0.5), (3, 700, 0.3)])
def test_random_sets_against_the_host_evaluation(seed, n_img, ovthresh):
    nc = 21
    dets, gb, gl, gd = random_set(seed, n_img, nc, extra_dets=60 if n_img >= 2000 else 12, no_gt_class=5, no_det_class=9)
    # equal scores inside an image's class and across images
    assert any(len(np.unique(d[j][:, 4])) < len(d[j]) for d in dets for j in range(1, nc))
    per_image = lambda j: [np.unique(d[j][:, 4]) for d in dets if len(d[j])]
    assert any(len(np.unique(np.concatenate(s))) < sum(len(x) for x in s) for s in map(per_image, range(1, nc)) if s)
    hard = np.concatenate(gd)
    assert 0.08 < hard.mean() < 0.25
    assert any(len(l) == 0 for l in gl) and any(all(len(a) == 0 for a in d) for d in dets)
    res, want = _check_against_host(dets, gb, gl, gd, nc, ovthresh)
    assert res['npos'][5 - 1] == 0 and len(res['rec'][5 - 1]) > 0 and not res['rec'][5 - 1].any()
    assert len(res['rec'][9 - 1]) == 0 and res['npos'][9 - 1] > 0 and res['ap07'][9 - 1] == 0.0
    for metric in (True, False):
        m_host, aps_host = pe.evaluate_detections(dets, gb, gl, gd, nc, ovthresh, metric)
        m_gpu, aps_gpu = vg.evaluate_detections_gpu(dets, gb, gl, gd, nc, ovthresh, metric)
        if metric:
            assert aps_gpu == [float(a) for a in aps_host] and m_gpu == m_host
        else:
            assert _area_close(m_gpu, m_host, max(len(r) for r in res['rec']) + 1)
    # the flat form gives the same results
    fd, gi, fgb, fgl, fgd = to_flat(dets, gb, gl, gd, nc)
    flat = vg.voc_evaluate(fd, fgb, fgl, fgd, nc, ovthresh, gt_image_index=gi, num_images=n_img)
    for k in range(nc - 1):
        np.testing.assert_array_equal(flat['rec'][k], res['rec'][k])
        np.testing.assert_array_equal(flat['prec'][k], res['prec'][k])
    np.testing.assert_array_equal(flat['ap07'], res['ap07'])
    np.testing.assert_array_equal(flat['ap_area'], res['ap_area'])


def test_long_classes_cross_the_chunk_and_the_summation_piece_boundaries():
    """two classes over 6000 images: several chunks of the block scans (carries forwards and backwards) and more than
    8192 terms in the area sum (np.sum adds pieces of 8192 elements)"""
    nc = 3
    dets, gb, gl, gd = random_set(4, 6000, nc, gt_per_img=8.0, extra_dets=20)
    res, _ = _check_against_host(dets, gb, gl, gd, nc, 0.5)
    assert all(len(f) > 3 * 2048 for f in res['flag']) and all((f == vg.FLAG_TP).sum() > 8192 for f in res['flag'])
    for k in range(nc - 1):
        assert len(np.unique(res['rec'][k])) > 8192


# 4 ---------------------------------------------------------------------------------------------------------------
def _one_class(dets_per_image, gts_per_image, hard_per_image, ovthresh=0.5):
    """one foreground class; -> (GPU result of that class, host (rec, prec, ap07))"""
    dets = [[np.zeros((0, 5)), np.asarray(d, np.float64).reshape(-1, 5)] for d in dets_per_image]
    gb = [np.asarray(g, np.float64).reshape(-1, 4) for g in gts_per_image]
    gl = [np.ones(len(g), np.int32) for g in gb]
    gd = [np.asarray(h, bool).reshape(-1) for h in hard_per_image]
    res, want = _check_against_host(dets, gb, gl, gd, 2, ovthresh)
    return {k: res[k][0] for k in res}, want[0]


def test_rule_iou_exactly_at_the_threshold_is_no_match():
    got, (rec, prec, ap, npos) = _one_class([[[0, 0, 9, 9, 0.9]]], [[[0, 0, 9, 19]]], [[False]])      # 100 / 200
    assert got['flag'].tolist() == [vg.FLAG_FP] and rec.tolist() == [0.0] and prec.tolist() == [0.0]
    got, _ = _one_class([[[0, 0, 9, 9, 0.9]]], [[[0, 0, 9, 19]]], [[False]], ovthresh=0.49)
    assert got['flag'].tolist() == [vg.FLAG_TP]


def test_rule_second_detection_on_a_taken_box_is_fp():
    got, (rec, prec, ap, npos) = _one_class([[[0, 0, 9, 9, 0.9], [0, 0, 9, 10, 0.8], [1, 0, 9, 9, 0.7]]],
                                            [[[0, 0, 9, 9]]], [[False]])
    assert got['flag'].tolist() == [vg.FLAG_TP, vg.FLAG_FP, vg.FLAG_FP] and rec.tolist() == [1.0, 1.0, 1.0]


def test_rule_difficult_match_is_neither_and_leaves_the_box_free():
    got, (rec, prec, ap, npos) = _one_class([[[0, 0, 9, 9, 0.9], [0, 0, 9, 9, 0.8]]], [[[0, 0, 9, 9]]], [[True]])
    assert got['flag'].tolist() == [vg.FLAG_IGNORED, vg.FLAG_IGNORED] and npos == 0 and got['npos'] == 0
    assert not rec.any() and not prec.any() and not got['rec'].any() and not got['prec'].any()
    # next to a regular box: the difficult match does not count, the regular one does
    got, (rec, prec, ap, npos) = _one_class([[[0, 0, 9, 9, 0.9], [50, 50, 59, 59, 0.8]]],
                                            [[[0, 0, 9, 9], [50, 50, 59, 59]]], [[True, False]])
    assert got['flag'].tolist() == [vg.FLAG_IGNORED, vg.FLAG_TP] and rec.tolist() == [0.0, 1.0]


def test_rule_equal_overlap_takes_the_first_box():
    # the same box twice, the first copy difficult: argmax takes the first, so the detection is ignored (the second copy
    # would have made it a true positive) -- and the other way round
    got, _ = _one_class([[[0, 0, 9, 9, 0.9]]], [[[0, 0, 9, 9], [0, 0, 9, 9]]], [[True, False]])
    assert got['flag'].tolist() == [vg.FLAG_IGNORED]
    got, _ = _one_class([[[0, 0, 9, 9, 0.9], [0, 0, 9, 9, 0.8]]], [[[0, 0, 9, 9], [0, 0, 9, 9]]], [[False, True]])
    assert got['flag'].tolist() == [vg.FLAG_TP, vg.FLAG_FP]
    # 70 copies: the first maximum lies in another lane's share than the last
    g = [[0, 0, 9, 9]] * 70
    got, _ = _one_class([[[0, 0, 9, 9, 0.9], [0, 0, 9, 9, 0.8]]], [g], [[False] + [True] * 69])
    assert got['flag'].tolist() == [vg.FLAG_TP, vg.FLAG_FP]
    got, _ = _one_class([[[0, 0, 9, 9, 0.9]]], [g], [[True] * 69 + [False]])
    assert got['flag'].tolist() == [vg.FLAG_IGNORED]


def test_rule_nan_overlap_is_fp():
    # finite boxes of zero area: iw = ih = 0, uni = 0 + 0 - 0, 0 / 0 -> NaN; np.max is NaN, NaN > ovthresh is False
    got, (rec, prec, ap, npos) = _one_class([[[5, 5, 4, 4, 0.9]]], [[[5, 5, 4, 4]]], [[False]])
    assert got['flag'].tolist() == [vg.FLAG_FP] and rec.tolist() == [0.0]
    # a NaN among regular overlaps still makes the detection a false positive
    got, (rec, prec, ap, npos) = _one_class([[[5, 5, 4, 4, 0.9]]], [[[5, 5, 4, 4], [0, 0, 9, 9]]], [[False, False]])
    assert got['flag'].tolist() == [vg.FLAG_FP]


def test_rule_equal_scores_keep_input_order():
    hit, miss = [0, 0, 9, 9, 0.5], [100, 100, 120, 120, 0.5]
    a, (rec_a, _, _, _) = _one_class([[miss, hit]], [[[0, 0, 9, 9]]], [[False]])
    b, (rec_b, _, _, _) = _one_class([[hit, miss]], [[[0, 0, 9, 9]]], [[False]])
    assert a['flag'].tolist() == [vg.FLAG_FP, vg.FLAG_TP] and b['flag'].tolist() == [vg.FLAG_TP, vg.FLAG_FP]
    assert rec_a.tolist() == [0.0, 1.0] and rec_b.tolist() == [1.0, 1.0]
    # across images: equal scores in image order
    c, (rec_c, _, _, _) = _one_class([[miss], [hit], [miss]], [[], [[0, 0, 9, 9]], []], [[], [False], []])
    assert c['flag'].tolist() == [vg.FLAG_FP, vg.FLAG_TP, vg.FLAG_FP]


def test_rule_segment_without_ground_truth():
    got, (rec, prec, ap, npos) = _one_class([[[0, 0, 9, 9, 0.9]], [[0, 0, 9, 9, 0.8]]], [[], [[0, 0, 9, 9]]], [[], [False]])
    assert got['flag'].tolist() == [vg.FLAG_FP, vg.FLAG_TP] and prec.tolist() == [0.0, 0.5]


def test_nothing_to_match():
    """no detections at all, no ground truth at all, neither: every output is defined and equals the host's"""
    nc = 4
    dets, gb, gl, gd = random_set(41, 12, nc)
    none = [[np.zeros((0, 5), np.float32)] * nc for _ in dets]
    nogt = ([np.zeros((0, 4), np.float32)] * len(dets), [np.zeros(0, np.int32)] * len(dets), [np.zeros(0, bool)] * len(dets))
    res, _ = _check_against_host(none, gb, gl, gd, nc, 0.5)
    assert all(len(r) == 0 for r in res['rec']) and res['npos'].sum() > 0 and not res['ap07'].any()
    res, _ = _check_against_host(dets, *nogt, nc, 0.5)
    assert res['npos'].sum() == 0 and all((f == vg.FLAG_FP).all() for f in res['flag'])
    res, _ = _check_against_host(none, *nogt, nc, 0.5)
    assert not res['ap07'].any() and not res['ap_area'].any()
    got = vg.paired_map_delta_gpu(none, none, *nogt[:2], nc, resamples=4)
    assert got == pg.paired_map_delta(none, none, *nogt[:2], nc, resamples=4)


# 5 ---------------------------------------------------------------------------------------------------------------
def test_a_large_segment():
    nc = 4
    dets, gb, gl, gd = random_set(21, 30, nc)
    rng = np.random.default_rng(22)
    G, D = 700, 3000
    x, y = rng.uniform(0, 3000, G), rng.uniform(0, 3000, G)
    big_g = np.round(np.stack([x, y, x + rng.uniform(20, 60, G), y + rng.uniform(20, 60, G)], 1)).astype(np.float32)
    src = rng.integers(0, G, D)
    big_d = big_g[src].astype(np.float64) + rng.normal(0, 6, (D, 4))
    big_d = np.concatenate([big_d, np.round(rng.uniform(0.05, 1, (D, 1)), 2)], 1).astype(np.float32)
    dets[11][2] = big_d
    gb[11] = np.concatenate([gb[11], big_g])
    gl[11] = np.concatenate([gl[11], np.full(G, 2, np.int32)])
    gd[11] = np.concatenate([gd[11], rng.uniform(size=G) < 0.15])
    res, _ = _check_against_host(dets, gb, gl, gd, nc, 0.5)
    f = res['flag'][1]
    assert (f == vg.FLAG_TP).sum() > 100 and (f == vg.FLAG_FP).sum() > 100 and (f == vg.FLAG_IGNORED).sum() > 10


def test_above_a_limit_nothing_is_launched(monkeypatch):
    dets, gb, gl, gd = random_set(23, 5, 3)
    calls = []
    real = L.call
    monkeypatch.setattr(L, 'call', lambda name, *a: (calls.append(name), real(name, *a)))
    d2 = [list(d) for d in dets]
    d2[2][1] = np.tile(np.float32([[0, 0, 10, 10, 0.5]]), (vg.MAX_SEG_DETS + 1, 1))
    with pytest.raises(ValueError, match='MAX_SEG_DETS'):
        vg.voc_evaluate(d2, gb, gl, gd, 3)
    gb2, gl2, gd2 = list(gb), list(gl), list(gd)
    gb2[1] = np.tile(np.float32([[0, 0, 10, 10]]), (vg.MAX_SEG_GT + 1, 1))
    gl2[1] = np.full(vg.MAX_SEG_GT + 1, 2, np.int32)
    gd2[1] = np.zeros(vg.MAX_SEG_GT + 1, bool)
    with pytest.raises(ValueError, match='MAX_SEG_GT'):
        vg.voc_evaluate(dets, gb2, gl2, gd2, 3)
    assert calls == []
    # the library itself refuses the same sizes before any launch (ODET_E_LIMIT)
    rc = L.lib().odet_voc_match(1, None, None, None, None, None, None, 0.5, vg.MAX_SEG_DETS + 1, 1, 1, 1, None, None,
                                None, None)
    assert rc == -4 and b'exceed' in L.lib().odet_last_error()
    rc = L.lib().odet_voc_match(1, None, None, None, None, None, None, 0.5, 1, vg.MAX_SEG_GT + 1, 1, 1, None, None, None,
                                None)
    assert rc == -4 and b'exceed' in L.lib().odet_last_error()
    # at the limits it runs and equals the host
    d2[2][1] = np.concatenate([np.tile(np.float32([[0, 0, 10, 10]]), (vg.MAX_SEG_DETS, 1)),
                               np.round(np.random.default_rng(1).uniform(0, 1, (vg.MAX_SEG_DETS, 1)), 2)], 1)
    _check_against_host(d2, gb, gl, gd, 3, 0.5)


# 6 ---------------------------------------------------------------------------------------------------------------
def _gate_sets(seed, n_img=300, nc=21):
    """two detection sets on the same annotations (no difficult boxes, as in the gate's scenes); the ground truth of
    the last class lies in image 0 alone"""
    da, gb, gl, _ = random_set(seed, n_img, nc, no_gt_class=nc - 1, hard_frac=0.0)
    db, _, _, _ = random_set(seed + 1000, n_img, nc, hard_frac=0.0)
    # set b: the same scenes' detections, perturbed -- take a's and replace a third of the images by b's own
    db = [da[i] if i % 3 else db[i] for i in range(n_img)]
    gb[0] = np.concatenate([gb[0], np.float32([[10, 10, 60, 60], [200, 100, 280, 190]])])
    gl[0] = np.concatenate([gl[0], np.int32([nc - 1, nc - 1])])
    for d in (da, db):
        d[0] = list(d[0])
        d[0][nc - 1] = np.float32([[11, 10, 60, 61, 0.9], [150, 100, 260, 190, 0.4]])
    return da, db, gb, gl


def _host_boot_table(dets, gb, gl, nc, counts, use_07_metric):
    """precision_gate._map_weighted's loop, per class: AP and npos of every row of counts"""
    flat = pg._flat_matches(pg._image_matches(dets, gb, gl, nc))
    ap = np.zeros((len(counts), nc - 1))
    npos_t = np.zeros((len(counts), nc - 1), np.int64)
    for b, c in enumerate(counts):
        for k, (tp, im, npos_img) in enumerate(flat):
            npos = float(np.dot(c, npos_img))
            npos_t[b, k] = int(npos)
            if npos == 0:
                continue
            w = c[im].astype(np.float64)
            ctp, cfp = np.cumsum(tp * w), np.cumsum((~tp) * w)
            rec = ctp / npos
            prec = ctp / np.maximum(ctp + cfp, np.finfo(np.float64).eps)
            ap[b, k] = pe.voc_ap(rec, prec, use_07_metric)
    return ap, npos_t, [len(f[0]) for f in flat]


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_bootstrap_equals_the_host_loop(seed):
    nc, n_img, R = 21, 300, 50
    da, db, gb, gl = _gate_sets(seed, n_img, nc)
    K = nc - 1
    ap, npos, counts = vg._paired_boot(da, db, gb, gl, nc, R, seed, True, 'cuda')
    assert ap.shape == npos.shape == (R + 1, 2 * K)
    for s, d in enumerate((da, db)):
        want_ap, want_npos, _ = _host_boot_table(d, gb, gl, nc, counts, True)
        # some resamples leave image 0 out, and with it the last class's ground truth (asserted on the HOST's table)
        assert (want_npos[1:, K - 1] == 0).sum() >= 1 and (want_npos[1:, K - 1] > 0).sum() >= 1
        np.testing.assert_array_equal(npos[:, s * K:(s + 1) * K], want_npos)
        np.testing.assert_array_equal(ap[:, s * K:(s + 1) * K], want_ap)
    want = pg.paired_map_delta(da, db, gb, gl, nc, resamples=R, seed=seed)
    got = vg.paired_map_delta_gpu(da, db, gb, gl, nc, resamples=R, seed=seed)
    assert sorted(got) == sorted(want)
    for k in ('map_a', 'map_b', 'delta', 'delta_boot_mean', 'delta_boot_std', 'delta_ci95', 'resamples'):
        assert got[k] == want[k], (k, got[k], want[k])
    assert want['delta'] != 0.0 and want['delta_boot_std'] > 0.0


def test_bootstrap_area_metric():
    nc, n_img, seed = 21, 300, 0
    da, db, gb, gl = _gate_sets(seed, n_img, nc)
    K = nc - 1
    # per-class APs of the full set and of a few resamples
    ap, npos, counts = vg._paired_boot(da, db, gb, gl, nc, 5, seed, False, 'cuda')
    m_max = 0
    for s, d in enumerate((da, db)):
        want_ap, want_npos, n_entries = _host_boot_table(d, gb, gl, nc, counts, False)
        np.testing.assert_array_equal(npos[:, s * K:(s + 1) * K], want_npos)
        for b in range(len(counts)):
            for k in range(K):
                assert _area_close(float(ap[b, s * K + k]), float(want_ap[b, k]), n_entries[k] + 1), (s, b, k)
        m_max = max(m_max, max(n_entries) + 1)
    # resamples=0 is how the gate uses this metric
    want = pg.paired_map_delta(da, db, gb, gl, nc, resamples=0, seed=seed, use_07_metric=False)
    got = vg.paired_map_delta_gpu(da, db, gb, gl, nc, resamples=0, seed=seed, use_07_metric=False)
    assert sorted(got) == sorted(want)
    assert _area_close(got['map_a'], want['map_a'], m_max) and _area_close(got['map_b'], want['map_b'], m_max)
    assert got['delta'] == got['map_b'] - got['map_a']
    for k in ('delta_boot_mean', 'delta_boot_std', 'delta_ci95', 'resamples'):
        assert got[k] == want[k], k


# 7 ---------------------------------------------------------------------------------------------------------------
def test_the_gate_end_to_end_with_both_evaluators():
    kw = dict(num_images=32, image_shape=(256, 352), depth=50, num_proposals=300, batch32=4, batch16=8, train_images=16,
              resamples=50)
    host = pg.fp16_vs_fp32(evaluator='host', **kw)
    gpu = pg.fp16_vs_fp32(evaluator='gpu', **kw)
    keys = [k for k in host if k.startswith('map_')]
    assert {'map_fp32', 'map_fp16', 'map_delta', 'map_delta_ci95_paired_bootstrap', 'map_delta_bootstrap_std',
            'map_delta_area_metric'} <= set(keys)
    assert sorted(host) == sorted(gpu)
    for k in keys:
        print(k, host[k], gpu[k])
    for k in keys:                                                # (the area figure too: np.sum's order is restated)
        assert gpu[k] == host[k], (k, gpu[k], host[k])
    assert host['gt_boxes'] > 0 and host['detections_fp32'] > 0


# 8 ---------------------------------------------------------------------------------------------------------------
def test_runs_on_the_current_stream_and_leaves_no_state():
    nc = 8
    dets, gb, gl, gd = random_set(31, 120, nc)
    first = vg.voc_evaluate(dets, gb, gl, gd, nc, 0.5)
    _check_against_host(dets, gb, gl, gd, nc, 0.5, res=first)
    other = random_set(32, 90, nc)
    vg.voc_evaluate(*other, nc, 0.3)                               # another problem in between
    again = vg.voc_evaluate(dets, gb, gl, gd, nc, 0.5)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        on_side = vg.voc_evaluate(dets, gb, gl, gd, nc, 0.5)
    for res in (again, on_side):
        for key in ('rec', 'prec', 'flag'):
            for k in range(nc - 1):
                np.testing.assert_array_equal(res[key][k], first[key][k])
        for key in ('ap07', 'ap_area', 'npos'):
            np.testing.assert_array_equal(res[key], first[key])     # (the area AP too: a fixed summation tree)
    da, db, gb2, gl2 = _gate_sets(5, 100, nc)
    a = vg._paired_boot(da, db, gb2, gl2, nc, 20, 1, True, 'cuda')
    with torch.cuda.stream(side):
        b = vg._paired_boot(da, db, gb2, gl2, nc, 20, 1, True, 'cuda')
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
