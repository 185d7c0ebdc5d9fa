"""Host side of the GPU VOC evaluation (no GPU): packing into (class, image) segments, the input checks that must fire
before the library is called, and the public surface (evaluation/voc_eval_gpu.py, precision_gate.fp16_vs_fp32's
`evaluator` keyword)."""
import inspect

import numpy as np
import pytest

from tf_eager_object_detection_amd import _lib as L
from tf_eager_object_detection_amd.evaluation import precision_gate as pg
from tf_eager_object_detection_amd.evaluation import voc_eval_gpu as vg
from voc_eval_sets import random_set, to_flat

NC = 6


@pytest.fixture
def no_library(monkeypatch):
    """any use of the library (a launch, a workspace query, a copy to the device) fails the test"""
    def boom(*a, **k):
        raise AssertionError('the library was called')
    monkeypatch.setattr(L, 'call', boom)
    monkeypatch.setattr(L, 'lib', boom)
    monkeypatch.setattr(vg, '_run_gpu', boom)


def test_header_limits_match_the_module():
    import os
    import re
    text = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'odet.h')).read()
    val = lambda n: eval(re.search(r'#define %s\s+(\([^)]*\)|\S+)' % n, text).group(1))
    assert val('ODET_VOC_MAX_SEG_DETS') == vg.MAX_SEG_DETS and val('ODET_VOC_MAX_SEG_GT') == vg.MAX_SEG_GT
    assert val('ODET_VOC_MAX_ENTRIES') == vg.MAX_ENTRIES and val('ODET_VOC_R') == len(vg.REC_THRS_07) == 11
    assert (val('ODET_VOC_IGNORED'), val('ODET_VOC_TP'), val('ODET_VOC_FP')) == (vg.FLAG_IGNORED, vg.FLAG_TP, vg.FLAG_FP)
    assert (val('ODET_VOC_AP_07'), val('ODET_VOC_AP_AREA')) == (vg.AP_07, vg.AP_AREA)
    np.testing.assert_array_equal(vg.REC_THRS_07, np.arange(0., 1.1, 0.1))


def test_list_and_flat_forms_pack_to_the_same_segments():
    dets, gb, gl, gd = random_set(5, 23, NC, no_gt_class=2, no_det_class=4)
    a = vg._pack_eval(dets, gb, gl, gd, NC)
    fd, gi, fgb, fgl, fgd = to_flat(dets, gb, gl, gd, NC)
    b = vg._pack_eval(fd, fgb, fgl, fgd, NC, gt_image_index=gi, num_images=len(dets))
    for k in a:
        if k not in ('dt_index', 'gt_index'):                    # (positions in the callers' differently ordered arrays)
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    # flat ground truth with list detections, and the number of images taken from the lists
    c = vg._pack_eval(dets, fgb, fgl, fgd, NC, gt_image_index=gi)
    np.testing.assert_array_equal(a['gt_box'], c['gt_box'])
    np.testing.assert_array_equal(a['gt_off'], c['gt_off'])


def test_segments_order_offsets_and_dtypes():
    dets, gb, gl, gd = random_set(6, 17, NC, no_gt_class=2, no_det_class=4)
    n, K = len(dets), NC - 1
    pk = vg._pack_eval(dets, gb, gl, gd, NC)
    seg = pk['seg_cls'].astype(np.int64) * n + pk['seg_img']
    assert (np.diff(seg) > 0).all()                               # (class asc, image asc), every pair once
    assert pk['num_images'] == n and pk['num_classes'] == K and pk['num_segments'] == len(seg)
    for k in ('seg_cls', 'seg_img', 'gt_off', 'dt_off', 'cls_seg_off', 'cls_entry_off', 'entry_image'):
        assert pk[k].dtype == np.int32 and pk[k].flags.c_contiguous, k
    assert pk['gt_box'].dtype == pk['dt_box'].dtype == pk['dt_score'].dtype == np.float64
    assert pk['gt_hard'].dtype == np.uint8
    assert pk['gt_off'][0] == 0 and pk['gt_off'][-1] == pk['num_gt'] == sum(len(l) for l in gl)
    assert pk['dt_off'][0] == 0 and pk['dt_off'][-1] == pk['num_entries'] == sum(len(a) for d in dets for a in d)
    assert len(pk['cls_seg_off']) == K + 1 and pk['cls_seg_off'][-1] == len(seg)
    seen = set()
    for s in range(len(seg)):
        c, i = int(pk['seg_cls'][s]), int(pk['seg_img'][s])
        seen.add((c, i))
        sel = gl[i] == c + 1
        g0, g1 = pk['gt_off'][s], pk['gt_off'][s + 1]
        np.testing.assert_array_equal(pk['gt_box'][g0:g1], gb[i][sel].astype(np.float64))       # annotation order, widened
        np.testing.assert_array_equal(pk['gt_hard'][g0:g1], gd[i][sel].astype(np.uint8))
        d0, d1 = pk['dt_off'][s], pk['dt_off'][s + 1]
        np.testing.assert_array_equal(pk['dt_box'][d0:d1], dets[i][c + 1][:, :4].astype(np.float64))   # input order
        np.testing.assert_array_equal(pk['dt_score'][d0:d1], dets[i][c + 1][:, 4].astype(np.float64))
        assert (pk['entry_image'][d0:d1] == i).all()
        assert g1 > g0 or d1 > d0
        assert pk['cls_seg_off'][c] <= s < pk['cls_seg_off'][c + 1]
    # every (class, image) that holds ground truth or detections is a segment; nothing else is
    want = {(int(l) - 1, i) for i in range(n) for l in gl[i]} | {(j - 1, i) for i in range(n) for j in range(1, NC)
                                                                if len(dets[i][j])}
    assert seen == want
    assert pk['max_seg_dets'] == max(len(a) for d in dets for a in d)
    # the class without ground truth has segments with detections only, the one without detections ground truth only,
    # images without detections / without ground truth occur
    c = 2 - 1
    s0, s1 = pk['cls_seg_off'][c], pk['cls_seg_off'][c + 1]
    assert s1 > s0 and pk['gt_off'][s0] == pk['gt_off'][s1] and pk['dt_off'][s1] > pk['dt_off'][s0]
    c = 4 - 1
    s0, s1 = pk['cls_seg_off'][c], pk['cls_seg_off'][c + 1]
    assert s1 > s0 and pk['dt_off'][s0] == pk['dt_off'][s1] and pk['gt_off'][s1] > pk['gt_off'][s0]
    assert pk['cls_entry_off'][c] == pk['cls_entry_off'][c + 1]
    assert any(all(len(a) == 0 for a in d) for d in dets) and any(len(l) == 0 for l in gl)


def test_empty_inputs_pack():
    dets = [[np.zeros((0, 5), np.float32)] * 3 for _ in range(4)]
    pk = vg._pack_eval(dets, [np.zeros((0, 4))] * 4, [np.zeros(0, np.int32)] * 4, None, 3)
    assert pk['num_segments'] == 0 and pk['num_entries'] == 0 and pk['max_seg_dets'] == 0 and pk['max_seg_gt'] == 0
    np.testing.assert_array_equal(pk['cls_seg_off'], [0, 0, 0])
    # ground truth given as plain lists, labels outside 1..num_classes-1 are left out (evaluate_detections' selection)
    pk = vg._pack_eval(dets, [[[0, 0, 5, 5], [1, 1, 8, 8]], [], [], []], [[2, 7], [], [], []], None, 3)
    assert pk['num_gt'] == 1 and pk['seg_cls'].tolist() == [1] and pk['seg_img'].tolist() == [0]


@pytest.mark.parametrize('what', ['score_nan', 'score_inf', 'box_nan', 'box_inf', 'gt_nan', 'gt_inf'])
def test_non_finite_values_raise_before_the_library(what, no_library):
    dets, gb, gl, gd = random_set(7, 9, NC)
    i = next(k for k in range(9) if len(dets[k][1]) and len(gb[k]))
    bad = np.nan if what.endswith('nan') else np.inf
    if what.startswith('score'):
        dets[i][1][0, 4] = bad
    elif what.startswith('box'):
        dets[i][1][0, 1] = -bad
    else:
        gb[i][0, 2] = bad
    with pytest.raises(ValueError, match='non-finite'):
        vg.voc_evaluate(dets, gb, gl, gd, NC)
    with pytest.raises(ValueError, match='non-finite'):
        vg.paired_map_delta_gpu(dets, dets, gb, gl, NC, resamples=3)


def test_a_segment_above_a_limit_raises_before_the_library(no_library):
    dets, gb, gl, gd = random_set(8, 5, 3)
    big = np.tile(np.float32([[0, 0, 10, 10, 0.5]]), (vg.MAX_SEG_DETS + 1, 1))
    d2 = [list(d) for d in dets]
    d2[2][1] = big
    with pytest.raises(ValueError, match='MAX_SEG_DETS'):
        vg.voc_evaluate(d2, gb, gl, gd, 3)
    d2[2][1] = big[:-1]                                           # at the limit: packs
    assert vg._pack_eval(d2, gb, gl, gd, 3)['max_seg_dets'] == vg.MAX_SEG_DETS
    gb2, gl2, gd2 = list(gb), list(gl), list(gd)
    gb2[1] = np.tile(np.float32([[0, 0, 10, 10]]), (vg.MAX_SEG_GT + 1, 1))
    gl2[1] = np.full(vg.MAX_SEG_GT + 1, 2, np.int32)
    gd2[1] = np.zeros(vg.MAX_SEG_GT + 1, bool)
    with pytest.raises(ValueError, match='MAX_SEG_GT'):
        vg.voc_evaluate(dets, gb2, gl2, gd2, 3)
    with pytest.raises(ValueError, match='MAX_SEG_GT'):
        vg.paired_map_delta_gpu(dets, dets, gb2, gl2, 3, resamples=2)


def test_inconsistent_arguments_raise(no_library):
    dets, gb, gl, gd = random_set(9, 6, 3)
    with pytest.raises(ValueError):
        vg.voc_evaluate(dets, gb[:-1], gl[:-1], gd[:-1], 3)        # another number of images
    fd, gi, fgb, fgl, fgd = to_flat(dets, gb, gl, gd, 3)
    with pytest.raises(ValueError, match='num_images'):
        vg.voc_evaluate(fd, fgb, fgl, fgd, 3, gt_image_index=gi)
    with pytest.raises(ValueError, match='labels'):
        vg.voc_evaluate((fd[0], fd[1] + 5, fd[2], fd[3]), gb, gl, gd, 3)
    with pytest.raises(ValueError, match='image index'):
        vg.voc_evaluate((fd[0] + 100, fd[1], fd[2], fd[3]), gb, gl, gd, 3)


def test_no_cpu_path():
    dets, gb, gl, gd = random_set(10, 4, 3)
    with pytest.raises(L.OdetError, match='no CPU path'):
        vg.voc_evaluate(dets, gb, gl, gd, 3, device='cpu')
    with pytest.raises(L.OdetError, match='no CPU path'):
        vg.paired_map_delta_gpu(dets, dets, gb, gl, 3, resamples=2, device='cpu')


def test_pair_packing_puts_set_b_behind_set_a():
    da, gb, gl, _ = random_set(11, 12, NC)
    db, _, _, _ = random_set(12, 12, NC)
    K = NC - 1
    pk = vg._pack_pair(da, db, gb, gl, NC)
    a = vg._pack_eval(da, gb, gl, None, NC)
    b = vg._pack_eval(db, gb, gl, None, NC)
    assert pk['num_classes'] == 2 * K and pk['num_entries'] == a['num_entries'] + b['num_entries']
    np.testing.assert_array_equal(pk['dt_score'], np.concatenate([a['dt_score'], b['dt_score']]))
    np.testing.assert_array_equal(pk['gt_box'], np.concatenate([a['gt_box'], b['gt_box']]))
    np.testing.assert_array_equal(pk['seg_cls'], np.concatenate([a['seg_cls'], b['seg_cls'] + K]))
    np.testing.assert_array_equal(pk['cls_entry_off'][:K + 1], a['cls_entry_off'])
    np.testing.assert_array_equal(pk['cls_entry_off'][K:], b['cls_entry_off'] + a['num_entries'])


def test_counts_follow_the_host_generator_stream():
    n, r, seed = 37, 6, 4
    counts = vg._draw_counts(n, r, seed)
    assert counts.dtype == np.int32 and counts.shape == (r + 1, n) and (counts[0] == 1).all()
    rng = np.random.default_rng(seed)
    for k in range(r):                                             # paired_map_delta's loop
        np.testing.assert_array_equal(counts[1 + k], np.bincount(rng.integers(0, n, n), minlength=n))


def test_maps_leave_out_classes_without_ground_truth():
    ap = np.array([[0.5, 0.25, 0.0, 1.0, 0.0, 0.5]])
    npos = np.array([[3, 2, 0, 1, 0, 4]])
    np.testing.assert_array_equal(vg._maps_from_boot(ap, npos, 3), [[np.mean([0.5, 0.25]), np.mean([1.0, 0.5])]])
    np.testing.assert_array_equal(vg._maps_from_boot(ap, npos * 0, 3), [[0.0, 0.0]])


def test_public_surface():
    assert inspect.signature(pg.fp16_vs_fp32).parameters['evaluator'].default == 'host'
    with pytest.raises(ValueError, match='evaluator'):
        pg.fp16_vs_fp32(evaluator='numpy')
    host, gpu = inspect.signature(pg.paired_map_delta).parameters, inspect.signature(vg.paired_map_delta_gpu).parameters
    assert list(gpu)[:len(host)] == list(host)
    assert all(gpu[k].default == host[k].default for k in host)
    from tf_eager_object_detection_amd.evaluation import pascal_eval as pe
    host, gpu = inspect.signature(pe.evaluate_detections).parameters, inspect.signature(vg.evaluate_detections_gpu).parameters
    assert list(gpu)[:len(host)] == list(host) and all(gpu[k].default == host[k].default for k in host)


def test_result_keys_equal_the_host_ones(monkeypatch):
    """paired_map_delta_gpu builds its record from the bootstrap's [1 + resamples, 2K] table exactly as paired_map_delta
    does from its loop: here with the table the HOST computes (no GPU), every value must come out equal"""
    da, gb, gl, _ = random_set(13, 40, NC, no_gt_class=3)
    db, _, _, _ = random_set(14, 40, NC)
    K, R, seed = NC - 1, 12, 3
    want = pg.paired_map_delta(da, db, gb, gl, NC, resamples=R, seed=seed)

    def host_table(dets_a, dets_b, gt_boxes, gt_labels, num_classes, resamples, seed, use_07_metric, device):
        counts = vg._draw_counts(len(dets_a), resamples, seed)
        ap = np.zeros((resamples + 1, 2 * K))
        npos = np.zeros((resamples + 1, 2 * K), np.int64)
        for s, d in enumerate((dets_a, dets_b)):
            flat = pg._flat_matches(pg._image_matches(d, gt_boxes, gt_labels, num_classes))
            for b in range(resamples + 1):
                for k, (tp, im, npos_img) in enumerate(flat):
                    npos[b, s * K + k] = int(np.dot(counts[b], npos_img))
                    ap[b, s * K + k] = pg._map_weighted([(tp, im, npos_img)], counts[b], use_07_metric)
        return ap, npos, counts
    monkeypatch.setattr(vg, '_paired_boot', host_table)
    got = vg.paired_map_delta_gpu(da, db, gb, gl, NC, resamples=R, seed=seed)
    assert sorted(got) == sorted(want)
    assert got == want
    got0 = vg.paired_map_delta_gpu(da, db, gb, gl, NC, resamples=0, seed=seed, use_07_metric=False)
    want0 = pg.paired_map_delta(da, db, gb, gl, NC, resamples=0, seed=seed, use_07_metric=False)
    assert sorted(got0) == sorted(want0) and got0 == want0
