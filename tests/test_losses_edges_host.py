"""tests/losses_edge_cases.py on the host: every case reaches the path it names (recomputed from the kernel's constants), its
restated outputs exist, the clamps and stray indices follow the header's rule, the documented limits answer ODET_E_LIMIT
before any GPU work, and the count of switch elements on which `<=` instead of `<` would change a bit."""
import numpy as np
import pytest

import losses_edge_cases as ec
import losses_np as ln

ROI, RPN, BWD = ec.roi_cases(), ec.rpn_cases(), ec.backward_cases()


def _id(c):
    return c['name']


def _reaches(c, path):
    assert c['reaches'] or c['B'] == 0, 'the case names no path'
    for k, v in c['reaches'].items():
        assert path[k] == v, (c['name'], k, path[k], v)


@pytest.mark.parametrize('c', ROI, ids=_id)
def test_roi_case_reaches_its_path(c):
    _reaches(c, ec.roi_path(c))
    for up in (None,) + ec.UPSTREAMS:
        want = ec.roi_expected(c, up)
        assert len(want) == c['B']
        for w in want:
            assert w['grad_scores'].shape == (c['R'], c['C']) and w['grad_deltas'].shape == (c['R'], 4 * c['C'])
            assert not np.isnan(w['grad_scores']).any() and not np.isnan(w['grad_deltas']).any()


def test_the_roi_table_covers_the_issues_sizes():
    assert {c['C'] for c in ROI} >= {1, 2, 16, 63, 64, 65, 128, 129, 1024}
    assert {c['R'] for c in ROI} >= {0, 1, 7, 8, 9, 2048}
    assert {c['S'] for c in ROI} >= {1, 1024} and {c['B'] for c in ROI} >= {0, 64}
    assert [o[1:] for o in ec.ROI_OVER_LIMIT] == [(ec.LS_MAX_CLASSES + 1, 2, 2, 1), (2, ec.LS_MAX_ROWS + 1, 2, 1),
                                                  (2, 2, ec.LS_MAX_SAMPLES + 1, 1), (2, 2, 2, ec.MAX_BATCH + 1)]
    assert {c['S'] for c in RPN} >= {1, 63, 64, 65, 1024}
    assert {(c['layout'], c['A']) for c in RPN} >= {(0, 1), (1, 1), (1, 9), (1, 15)}


@pytest.mark.parametrize('c', RPN, ids=_id)
def test_rpn_case_reaches_its_path(c):
    _reaches(c, ec.rpn_path(c))
    for up in ec.UPSTREAMS:
        want = ec.rpn_expected(c, np.tile(up, (c['B'], 1)))
        for b, w in enumerate(want):
            n = ec.rpn_path(c)['n'][b]
            assert np.all(w['row_grad_scores'][n:] == 0) and np.all(w['row_grad_deltas'][n:] == 0)
            assert not np.isnan(w['grad_scores']).any() and not np.isnan(w['losses']).any()


@pytest.mark.parametrize('c', BWD, ids=_id)
def test_backward_case_reaches_its_fill_path(c):
    _reaches(c, ec.fill_path(c['N'], c['B'], c['want_scores'], c['want_deltas']))


def test_the_big_fill_takes_a_fifth_trip():
    p = ec.fill_path(**ec.BIG_FILL)
    assert p['vectors'] > ec.FILL_MAX_BLOCKS * ec.FILL_THREADS * ec.FILL_STORES and p['blocks'] == ec.FILL_MAX_BLOCKS
    assert p['trips'] == 5 and p['tail_scores'] == 0 and p['tail_deltas'] == 0


def test_clamps_and_stray_indices_follow_the_headers_rule():
    c = next(c for c in RPN if c['name'] == 'counts')
    want = ec.rpn_expected(c, np.ones((c['B'], 2), np.float32))
    # kfg = 0: reg is exactly +0 and no row has a delta gradient; kbg = 0 and kfg = S: every row is foreground
    assert want[0]['losses'][1].tobytes() == np.float32(0).tobytes() and not want[0]['row_grad_deltas'].any()
    assert np.all(np.abs(want[2]['row_grad_deltas']).sum(axis=1) > 0)
    # kfg + kbg > S: n = S = 64, so the gradients are over 64; kfg > S: kfg = S
    for b, kfg in ((3, 40), (4, 64)):
        assert want[b]['n'] == 64 and np.count_nonzero(np.abs(want[b]['row_grad_deltas']).sum(axis=1)) == kfg
        assert np.all(np.abs(want[b]['row_grad_scores']).sum(axis=1) > 0)
    for b in (5, 6, 7):
        assert not want[b]['losses'].any() and not want[b]['row_grad_scores'].any() and not want[b]['grad_scores'].any()
    # a stray index adds nothing and gets zero row gradients but counts in n: the same image without the stray rows, at the
    # same n, has the same row gradients elsewhere
    c = next(c for c in RPN if 'stray' in c['name'] and c['layout'] == 0)
    w = ec.rpn_expected(c, np.ones((c['B'], 2), np.float32))[0]
    assert w['n'] == 26 and not w['row_grad_scores'][[3, 13, 20]].any() and not w['row_grad_deltas'][3].any()
    assert np.all(w['ce_rows'][[3, 13, 20]] == 0) and np.count_nonzero(w['ce_rows']) > 10
    assert np.count_nonzero(np.abs(w['grad_deltas']).sum(axis=1)) == 11          # 12 foreground rows, one of them stray
    other = w['row_grad_scores'][0] * np.float32(26)                             # p - onehot: the gradient is over n = 26
    assert np.abs(other).max() <= 1


def test_the_documented_limits_answer_before_any_gpu_work():
    from tf_eager_object_detection_amd import _lib
    L = _lib.lib()
    for what, C, R, S, B in ec.ROI_OVER_LIMIT:
        assert L.odet_roi_loss(None, None, R, C, B, None, None, None, None, None, S, None, 1.0, None, None, None, None,
                               None) == -4, what
    for what, S, B in ec.RPN_OVER_LIMIT:
        assert L.odet_rpn_loss(None, None, 90, B, 0, 1, None, None, None, S, 3.0, None, None, None, None) == -4, what
        assert L.odet_rpn_loss_backward(None, None, None, None, 90, B, 0, 1, S, None, None, None) == -4, what
    # at the limits the size checks pass (the null pointers are what is refused)
    assert L.odet_roi_loss(None, None, 2048, 1024, 64, None, None, None, None, None, 1024, None, 1.0, None, None, None, None,
                           None) == -1
    assert L.odet_rpn_loss(None, None, 90, 64, 0, 1, None, None, None, 1024, 3.0, None, None, None, None) == -1


@pytest.mark.parametrize('sigma', [1.0, 2.0, 3.0])
def test_count_of_switch_elements_where_the_comparison_shows(sigma):
    """the function is continuous at |d| = 1 / sigma_2, so `<=` for `<` changes few bits; the count is printed, not bounded"""
    v = ec.switch_values(sigma)
    thr = ln.sl_const(sigma)[1]
    assert np.abs(v[1]) == thr and np.abs(v[0]) < thr < np.abs(v[2]) and len(set(v.tolist())) == 6
    lt = ln.smooth_l1(v, 0, 1, 1, sigma)
    le = ec.smooth_l1_le(v, 0, 1, 1, sigma)
    assert lt[2].tolist() == [1, 0, 0, 1, 0, 0]
    loss = int(np.sum(lt[0].view(np.uint32) != le[0].view(np.uint32)))
    grad = int(np.sum(lt[1].view(np.uint32) != le[1].view(np.uint32)))
    print('\nsigma %g: `<=` would change %d of 6 loss terms and %d of 6 gradients' % (sigma, loss, grad))
    for make in (ec.roi_switch_case, ec.rpn_switch_case):
        c = make(sigma)
        d = c['deltas'][0]
        assert np.isin(v, d).all()
