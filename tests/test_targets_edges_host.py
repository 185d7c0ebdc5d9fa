"""CPU proof of what tests/test_targets_edges_gpu.py covers (no GPU): the committed key masks and sampling cases of
tests/targets_edge_cases.py walk d_tg_radix_select through every one of its seven levels and all three of its exit shapes on
each of the four selection streams, with keys that tie on the threshold; and every hand-made tie / threshold case changes under
at least one wrong reading of the label rules.  selection_trace only ACCOUNTS for coverage here; the k-th pair itself always
comes from the lexsort of tests/targets_np.select."""
import numpy as np
import pytest

import targets_edge_cases as ec
import targets_np as tn
from oracle import oracle_np as on

F32 = np.float32


def _kth_pair(keys, idx, k):
    order = np.lexsort((idx, keys))
    return int(keys[order[k - 1]]), int(idx[order[k - 1]])


@pytest.mark.parametrize('mask', [None, 0, 0xF, 0xFFF << 28, 0xFFF << 4, 0x0030030030030033])
def test_trace_reconstructs_the_kth_pair_of_the_lexsort(mask):
    cand = np.sort(np.random.default_rng(3).choice(200000, 5000, replace=False)).astype(np.int64)
    keys = tn.key64(1, 7, cand, 5, mask)
    n = len(cand)
    top = np.bincount((keys >> np.uint64(52)).astype(np.int64), minlength=4096)
    exact = int(np.cumsum(top)[np.nonzero(top >= 2)[0][0]])        # a level-0 bin of >= 2 candidates holds exactly the rows needed
    ks = [1, n - 1, 256] + ([exact] if exact < n else [])
    for k in ks:
        tr = tn.selection_trace(keys, cand, k)
        assert tr['kth'] == _kth_pair(keys, cand, k), (mask, k)
        assert tr['kept'] == k
        sel = tn.select(cand, k, 1, 7, 5, mask)
        assert (int(tn.key64(1, 7, sel[-1:], 5, mask)[0]), int(sel[-1])) == tr['kth']
        last = tr['levels'][-1]
        assert last['level'] == tr['end'] and last['count'] == last['need']
        assert all(lv['count'] > lv['need'] for lv in tr['levels'][:-1])
    if exact < n:
        tr = tn.selection_trace(keys, cand, exact)
        assert tr['end'] == 0 and tr['threshold'][1] == 0xFFFFFFFF and tr['threshold'][0] & ((1 << 52) - 1) == (1 << 52) - 1
    # nothing to walk: the kernel returns before the first level
    assert tn.selection_trace(keys, cand, 0)['end'] is None and tn.selection_trace(keys, cand, n)['end'] is None


def test_mask_none_is_all_ones_and_leaves_existing_callers_unchanged():
    i = np.arange(1000)
    np.testing.assert_array_equal(tn.key64(2, 1, i, 9), tn.key64(2, 1, i, 9, ec.ALL_ONES))
    np.testing.assert_array_equal(tn.key64(2, 1, i, 9, 0xFFF << 28), tn.key64(2, 1, i, 9) & np.uint64(0xFFF << 28))
    np.testing.assert_array_equal(tn.select(i, 10, 0, 0, 1, 0), np.arange(10))          # equal keys: the index orders


def _all_traces():
    """[(stream, mask, case name, trace, keys, candidates, k)] of every selection the GPU test makes"""
    out = []
    sels = [(c[0], ec.anchor_selections(c)) for c in ec.anchor_sampling_cases()] + \
           [(c[0], ec.proposal_selections(c)) for c in ec.proposal_sampling_cases()]
    for mask in ec.KEY_MASKS:
        for name, pairs in sels:
            for stream, cand, k in pairs:
                keys = tn.key64(stream, ec.IMAGE_ID, cand, ec.SEED, mask)
                out.append((stream, mask, name, tn.selection_trace(keys, cand, k), keys, np.asarray(cand, np.int64), k))
    return out


def test_masks_and_cases_cover_every_level_exit_and_key_tie_on_each_stream():
    traces = _all_traces()
    print()
    print('stream | discriminating walks per level 0..6 | walks ending on level 0..6 | walks with >= 2 kept rows on the threshold key')
    for stream in (tn.STREAM_ANCHOR_FG, tn.STREAM_ANCHOR_BG, tn.STREAM_ROI_FG, tn.STREAM_ROI_BG):
        disc, ends, ties = [0] * 7, [0] * 7, 0
        for s, mask, name, tr, keys, cand, k in traces:
            if s != stream or tr['end'] is None:
                continue
            assert tr['kth'] == _kth_pair(keys, cand, k), (stream, hex(mask), name)
            for lv in tr['levels']:
                if lv['occupied'] >= 2 and lv['below'] > 0:
                    disc[lv['level']] += 1
            ends[tr['end']] += 1
            kept_on_key = int(np.count_nonzero((keys == np.uint64(tr['kth'][0])) & (cand <= tr['kth'][1])))
            ties += kept_on_key >= 2
        print('%6d | %-35s | %-26s | %d' % (stream, disc, ends, ties))
        assert all(d > 0 for d in disc), 'stream %d: no discriminating walk at some level: %s' % (stream, disc)
        assert sum(ends[:5]) > 0 and ends[5] > 0 and ends[6] > 0, 'stream %d: an exit shape is missing: %s' % (stream, ends)
        assert ties > 0, 'stream %d: no threshold with equal keys' % stream


def test_production_keys_never_pass_level_one():
    """why the diagnostic hook exists: with the real Philox keys no committed case walks deeper than the second digit, and neither
    do 200 000 contiguous candidates at k = 256, 1 and n - 1"""
    for s, mask, name, tr, *_ in _all_traces():
        if mask == ec.ALL_ONES and tr['end'] is not None:
            assert tr['end'] <= 1, (s, name, tr['end'])
    cand = np.arange(200000)
    keys = tn.key64(1, 0, cand, 5)
    for k in (256, 1, 199999):
        assert tn.selection_trace(keys, cand, k)['end'] <= 1


def test_sampling_cases_are_the_ones_asked_for():
    n_fg = ec._big_anchor_inputs()[3]
    by = {c[0]: dict((s, (len(cand), k)) for s, cand, k in ec.anchor_selections(c)) for c in ec.anchor_sampling_cases()}
    assert by['both-sampled'][0] == (n_fg, 128) and by['both-sampled'][1][1] == 128 and by['both-sampled'][1][0] > 128
    assert by['sample-limit'][0] == (n_fg, n_fg) and by['sample-limit'][1][1] == 1024 - n_fg
    assert by['one-row'][0] == (n_fg, 1) and by['one-row'][1][1] == 0
    assert by['all-but-one-fg'][0] == (n_fg, n_fg - 1) and by['every-fg'][0] == (n_fg, n_fg)
    by = {c[0]: dict((s, (len(cand), k)) for s, cand, k in ec.proposal_selections(c)) for c in ec.proposal_sampling_cases()}
    n_bg = by['few-sampled'][3][0]
    assert [by[n][3][1] - n_bg for n in ('few-sampled', 'few-all-kept', 'few-replace')] == [-1, 0, 1]
    assert by['few-sampled'][2][0] > by['few-sampled'][2][1]                                  # foreground sampled as well
    assert by['600-sampled'][3][0] > by['600-sampled'][3][1] and by['600-replace'][3][0] < by['600-replace'][3][1]


# ---------------------------------------------------------------------------------------------- sharpness of part B --
ANCHOR_FLIPS = ('last-argmax', 'pos-strict', 'neg-inclusive', 'first-tying-anchor-only')
ROI_FLIPS = ('last-argmax', 'pos-strict', 'neg-strict')


def _argmax(iou, flip):
    return iou.shape[1] - 1 - np.argmax(iou[:, ::-1], axis=1) if flip == 'last-argmax' else np.argmax(iou, axis=1)


def _anchor_labels(gt, shape, anchors, pos, neg, flip=None):
    """oracle_np.anchor_target_labels with ONE rule read wrongly"""
    idx = on.bboxes_range_filter(anchors, shape[0], shape[1])
    iou = on.pairwise_iou(F32(anchors)[idx], gt)
    mx, col = iou.max(axis=1), iou.max(axis=0)
    labels = -np.ones(len(idx), np.int32)
    labels[(mx <= F32(neg)) if flip == 'neg-inclusive' else (mx < F32(neg))] = 0
    labels[np.argmax(iou, axis=0) if flip == 'first-tying-anchor-only' else np.nonzero(iou == col[None, :])[0]] = 1
    labels[(mx > F32(pos)) if flip == 'pos-strict' else (mx >= F32(pos))] = 1
    return idx, labels, _argmax(iou, flip)


def _roi_assign(rois, gt, pos, neg, flip=None):
    iou = on.pairwise_iou(rois, gt)
    mx = iou.max(axis=1)
    is_fg = (mx > F32(pos)) if flip == 'pos-strict' else (mx >= F32(pos))
    is_bg = ~is_fg & ((mx > F32(neg)) if flip == 'neg-strict' else (mx >= F32(neg)))
    return _argmax(iou, flip), np.nonzero(is_fg)[0], np.nonzero(is_bg)[0]


def test_every_tie_case_changes_under_a_flipped_rule_and_every_flip_is_caught():
    caught = dict.fromkeys(ANCHOR_FLIPS, 0)
    print()
    for name, anchors, gt in ec.anchor_tie_cases():
        idx, labels, argmax = on.anchor_target_labels(gt, ec.TIE_SHAPE, anchors, ec.POS, ec.NEG)
        mine = _anchor_labels(gt, ec.TIE_SHAPE, anchors, ec.POS, ec.NEG)
        for a, b in zip((idx, labels, argmax), mine):
            np.testing.assert_array_equal(a, b, err_msg=name)
        changed = []
        for flip in ANCHOR_FLIPS:
            _, l2, a2 = _anchor_labels(gt, ec.TIE_SHAPE, anchors, ec.POS, ec.NEG, flip)
            if not (np.array_equal(l2, labels) and np.array_equal(a2, argmax)):
                changed.append(flip)
                caught[flip] += 1
        print('%-26s N %4d G %4d  labels 1/0/-1: %d/%d/%d  changes under: %s' % (
            name, len(anchors), len(gt), (labels == 1).sum(), (labels == 0).sum(), (labels == -1).sum(), ', '.join(changed)))
        assert changed, '%s: no flipped rule changes it' % name
    assert all(caught.values()), caught
    caught = dict.fromkeys(ROI_FLIPS, 0)
    for name, rois, gt, gl in ec.proposal_tie_cases():
        _, ga, fg, bg = on.proposal_target_assign(rois, gt, gl, ec.POS, ec.NEG)
        mine = _roi_assign(rois, gt, ec.POS, ec.NEG)
        for a, b in zip((ga, fg, bg), mine):
            np.testing.assert_array_equal(a, b, err_msg=name)
        changed = []
        for flip in ROI_FLIPS:
            got = _roi_assign(rois, gt, ec.POS, ec.NEG, flip)
            if not all(np.array_equal(a, b) for a, b in zip((ga, fg, bg), got)):
                changed.append(flip)
                caught[flip] += 1
        print('%-26s R %4d G %4d  fg %d bg %d  changes under: %s' % (name, len(rois), len(gt), len(fg), len(bg), ', '.join(changed)))
        assert changed, '%s: no flipped rule changes it' % name
        assert len(np.unique(rois, axis=0)) < len(rois), '%s: no duplicated RoI row' % name
    assert all(caught.values()), caught


def test_tie_cases_hold_what_their_names_say():
    cases = {n: (a, g) for n, a, g in ec.anchor_tie_cases()}

    def run(name):
        a, g = cases[name]
        idx, labels, argmax = on.anchor_target_labels(g, ec.TIE_SHAPE, a, ec.POS, ec.NEG)
        full = -2 * np.ones(len(a), np.int32); full[idx] = labels
        am = -np.ones(len(a), np.int64); am[idx] = argmax
        return a, g, full, am, on.pairwise_iou(a, g)
    a, g, lab, am, iou = run('duplicate-box')
    assert np.array_equal(g[0], g[1]) and am[0] == 0 and am[2] == 2
    a, g, lab, am, iou = run('box-equals-anchor')
    assert (iou == 1).sum() >= 2
    for name in ('between-two-anchors', 'between-two-workgroups'):
        a, g, lab, am, iou = run(name)
        tie = np.nonzero(iou[:, 0] == iou[:, 0].max())[0]
        assert len(tie) == 2 and np.all(lab[tie] == 1) and ec.NEG < iou[tie[0], 0] < ec.POS
        assert (tie[1] - tie[0] > 256) == (name == 'between-two-workgroups')
    a, g, lab, am, iou = run('iou-equals-pos')
    on_pos = np.nonzero((iou.max(axis=1) == F32(ec.POS)) & (iou < iou.max(axis=0)[None, :]).all(axis=1))[0]
    assert len(on_pos) and np.all(lab[on_pos] == 1)                     # `>=` alone makes them foreground
    a, g, lab, am, iou = run('iou-equals-neg')
    on_neg = np.nonzero(iou.max(axis=1) == F32(ec.NEG))[0]
    assert len(on_neg) and np.all(lab[on_neg] == -1)
    a, g, lab, am, iou = run('column-maximum-below-neg')
    assert iou[0].max() == F32(1 / 64) and iou[0, 0] == iou[:, 0].max() and lab[0] == 1
    a, g, lab, am, iou = run('zero-area-box')
    assert on.area(g)[1] == 0 and np.all(iou[:, 1] == 0) and np.all(lab == 1)
    assert len(cases['one-anchor'][0]) == 1
    assert sorted(len(g) for n, (a, g) in cases.items() if n.startswith('lattice')) == [1, 257, 1024]
    assert all(len(a) % 256 for n, (a, g) in cases.items())
    # the lattice cases really hold ties: equal non-zero maxima in a column, duplicated boxes, IoUs on both thresholds
    a, g, lab, am, iou = run('lattice-G1024')
    assert len(np.unique(g, axis=0)) < len(g)
    assert ((iou == iou.max(axis=0)[None, :]) & (iou > 0)).sum(axis=0).max() >= 2
    assert (iou == F32(ec.POS)).any() and (iou == F32(ec.NEG)).any() and (iou == 1).any()
    assert (lab == -2).any()                                            # anchors outside the image
