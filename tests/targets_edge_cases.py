"""The inputs of tests/test_targets_edges_host.py (which proves on the CPU what they cover) and tests/test_targets_edges_gpu.py
(which runs them): the key masks and sampling cases that walk d_tg_radix_select through all seven digits, and hand-made
integer boxes whose IoUs tie or sit exactly on a threshold.  ONE list of each, imported by both files."""
import functools

import numpy as np

import targets_np as tn
from oracle import oracle_np as on

ALL_ONES = 0xFFFFFFFFFFFFFFFF
# Digit l of V = key64 * 2^20 + i covers key bits 63-12l .. 52-12l for l = 0 .. 4, key bits 3 .. 0 + index bits 19 .. 12 for
# l = 5 and index bits 11 .. 0 for l = 6.  What each mask is for (tests/test_targets_edges_host.py checks the sum of it):
KEY_MASKS = [
    ALL_ONES,                  # the product's keys through the diagnostic build: the walk ends on level 0 or 1
    0x0000000000000000,        # every key equal: the index alone orders (levels 5 and 6; `i <= t.idx` decides every row)
    0x000000000000000F,        # four key bits: the mixed digit of level 5 really mixes
    0x000000FFF0000000,        # one full digit at level 2 (the first that recomputes the low key word)
    0x000000000FFF0000,        # one full digit at level 3
    0x000000000000FFF0,        # one full digit at level 4
    0x0030030030030033,        # two bits in every key digit: large candidate sets branch at every level
    0x0010010010010011,        # one bit in every key digit: the small sets (a few hundred candidates) do
    0x0010010010010010,        # the same without key bit 0: small sets meet again at level 5 and part at level 6
]

MEANS, STDS = [0.0, 0.0, 0.0, 0.0], [0.1, 0.1, 0.2, 0.2]
SEED, IMAGE_ID = 5, 2


# ---------------------------------------------------------------------------------------------- part A: sampling cases --
@functools.lru_cache(maxsize=None)
def _big_anchor_inputs():
    """the 800 x 1333 anchors with 100 boxes of tests/test_targets_gpu.py (447 foreground, both kinds sampled at 256 / 128)"""
    from oracle import c_oracle as co
    from tf_eager_object_detection_amd import synthetic as syn
    shape = (800, 1333)
    anchors = co.fpn_anchors(shape)
    rng = np.random.default_rng(21)
    syn.random_boxes(8, shape, rng, 16, 600)
    gt = syn.random_boxes(100, shape, rng, 16, 600)
    _, labels, _ = on.anchor_target_labels(gt, shape, anchors, 0.7, 0.3)
    return shape, anchors, gt, int((labels == 1).sum())


@functools.lru_cache(maxsize=None)
def anchor_sampling_cases():
    """[(name, shape, anchors, gt, total, max_pos)]; pos 0.7, neg 0.3"""
    shape, anchors, gt, n_fg = _big_anchor_inputs()
    return [('both-sampled', shape, anchors, gt, 256, 128),
            ('sample-limit', shape, anchors, gt, 1024, 512),            # TG_MAX_SAMPLES
            ('one-row', shape, anchors, gt, 1, 1),
            ('all-but-one-fg', shape, anchors, gt, 512, n_fg - 1),
            ('every-fg', shape, anchors, gt, 512, n_fg)]                # the foreground selection returns before the walk


@functools.lru_cache(maxsize=None)
def _roi_inputs():
    """the 600-RoI input of tests/test_targets_gpu.py (seed 12 at 600 x 800)"""
    from tf_eager_object_detection_amd import synthetic as syn
    rng = np.random.default_rng(12)
    shape = (600, 800)
    gt = syn.random_boxes(6, shape, rng, 60, 300)
    gt_labels = rng.integers(1, 21, 6).astype(np.int64)
    rois = np.concatenate([syn.random_boxes(400, shape, rng, 20, 300),
                           (gt[rng.integers(0, 6, 200)] + rng.normal(0, 8, (200, 4))).astype(np.float32), gt]).astype(np.float32)
    return rois, gt, gt_labels


@functools.lru_cache(maxsize=None)
def proposal_sampling_cases():
    """[(name, rois, gt, gt_labels, neg, total, max_pos)]; pos 0.5, 21 classes.  `few`: rows 380 .. 459 of the 600 (random and
    near-box RoIs), neg 0 so that every other row is background; total puts want at n_bg - 1 / n_bg / n_bg + 1."""
    rois, gt, gt_labels = _roi_inputs()
    few = rois[380:460]
    _, _, fg, bg = on.proposal_target_assign(few, gt, gt_labels, 0.5, 0.0)
    max_pos = 8
    assert len(fg) > max_pos and len(bg) > 8 and len(fg) + len(bg) == len(few)
    out = [('600-sampled', rois, gt, gt_labels, 0.0, 128, 32),
           ('600-replace', rois, gt, gt_labels, 0.1, 128, 32)]
    for name, extra in (('few-sampled', -1), ('few-all-kept', 0), ('few-replace', 1)):
        out.append((name, few, gt, gt_labels, 0.0, max_pos + len(bg) + extra, max_pos))
    # RoI rows stay below 2^12, so the mixed digit of level 5 is the keys' low four bits alone there, and a walk ends on it only
    # when k is the size of a group of them: as many rows of each kind as have the low key bits 0000 (under the mask 0xF)
    _, _, fg, bg = on.proposal_target_assign(rois, gt, gt_labels, 0.5, 0.0)
    k_fg = int((tn.key64(tn.STREAM_ROI_FG, IMAGE_ID, fg, SEED, 0xF) == 0).sum())
    k_bg = int((tn.key64(tn.STREAM_ROI_BG, IMAGE_ID, bg, SEED, 0xF) == 0).sum())
    assert 1 < k_fg < len(fg) and 1 < k_bg < len(bg)
    out.append(('600-whole-nibble', rois, gt, gt_labels, 0.0, k_fg + k_bg, k_fg))
    return out


def anchor_selections(case):
    """the two selections an anchor case makes: [(stream, candidate indices, k)]"""
    _, shape, anchors, gt, total, max_pos = case
    _, labels, _ = _labels_cached(case[0])
    idx = on.bboxes_range_filter(anchors, shape[0], shape[1])
    fg, bg = idx[labels == 1], idx[labels == 0]
    k_fg = min(len(fg), max_pos)
    return [(tn.STREAM_ANCHOR_FG, fg, k_fg), (tn.STREAM_ANCHOR_BG, bg, min(len(bg), max(total - k_fg, 0)))]


@functools.lru_cache(maxsize=None)
def _labels_cached(name):
    case = [c for c in anchor_sampling_cases() if c[0] == name][0]
    return on.anchor_target_labels(case[3], case[1], case[2], 0.7, 0.3)


def proposal_selections(case):
    """the two selections a proposal case makes: [(stream, candidate rows, k)] (k >= n: everything kept / with replacement)"""
    _, rois, gt, gt_labels, neg, total, max_pos = case
    _, _, fg, bg = on.proposal_target_assign(rois, gt, gt_labels, 0.5, neg)
    k_fg = min(len(fg), max_pos)
    return [(tn.STREAM_ROI_FG, fg, k_fg), (tn.STREAM_ROI_BG, bg, total - k_fg)]


# ------------------------------------------------------------------------------------ part B: ties and thresholds --
# Integer coordinates and the dyadic thresholds pos = 1/2, neg = 1/4: areas, intersections and unions are small integers and the
# quotients that matter (1, 1/2, 1/4, 1/64) are exact.  IoU uses the +1 convention: [x0, y0, x1, y1] covers (x1 - x0 + 1) x
# (y1 - y0 + 1) pixels.
POS, NEG = 0.5, 0.25
TIE_SHAPE = (256, 512)


def _far_fillers(n, x0=200):
    """n inside anchors 2 x 2 away from every box of the hand-made cases (IoU 0 with all of them)"""
    k = np.arange(n)
    x, y = x0 + 4 * (k % 64), 128 + 4 * (k // 64)
    return np.stack([x, y, x + 1, y + 1], axis=1).astype(np.float32)


def _grid_case(g, n, seed):
    """n anchors on a 4-pixel lattice (sizes 4 / 8 / 16, a few of them outside the image) and g lattice boxes: ties, duplicates,
    IoU = 1, 1/2 and 1/4 all occur by themselves"""
    rng = np.random.default_rng(seed)

    def boxes(m, lo):
        w, h = 4 * 2 ** rng.integers(0, 3, m), 4 * 2 ** rng.integers(0, 3, m)
        x, y = 4 * rng.integers(lo, 16, m), 4 * rng.integers(lo, 12, m)
        return np.stack([x, y, x + w - 1, y + h - 1], axis=1).astype(np.float32)
    return boxes(n, -1), boxes(g, 0)


@functools.lru_cache(maxsize=None)
def anchor_tie_cases():
    """[(name, anchors [N,4], gt [G,4])] for image TIE_SHAPE with POS / NEG"""
    f = np.float32
    A, A2 = [0, 0, 3, 3], [4, 0, 7, 3]                       # two 4 x 4 anchors side by side
    between = [2, 0, 5, 3]                                   # 8 pixels in each: IoU 8 / 24 with both, the column maximum twice
    tall = [0, 16, 3, 23]                                    # 4 x 8 box
    tall_anchors = [[0, 16, 3, 23],                          # equal to the box: IoU 1 (its column maximum)
                    [0, 16, 3, 19],                          # its upper half: 16 / 32 = pos exactly, not a column maximum
                    [0, 22, 3, 23]]                          # its last two rows: 8 / 32 = neg exactly
    big, corner = [64, 64, 95, 95], [64, 64, 67, 67]         # 16 / 1024 < neg, and the only anchor the big box meets
    out = []
    out.append(('duplicate-box', f([A, A2, [0, 8, 3, 11]]), f([[0, 0, 3, 5], [0, 0, 3, 5], [0, 8, 3, 11], [0, 8, 3, 11]])))
    out.append(('box-equals-anchor', f([A, A2] + tall_anchors), f([A, tall, A])))
    out.append(('between-two-anchors', f([A, A2, [8, 0, 11, 3]]), f([between])))
    far = np.concatenate([f([A]), _far_fillers(299), f([A2]), _far_fillers(3, 100)])
    out.append(('between-two-workgroups', far, f([between])))                  # the tying anchors are rows 0 and 300
    out.append(('iou-equals-pos', f(tall_anchors + [A]), f([tall, [0, 0, 3, 5]])))
    out.append(('iou-equals-neg', f(tall_anchors[::-1] + [A]), f([tall, [0, 0, 3, 5]])))
    out.append(('column-maximum-below-neg', f([corner, A, A2]), f([big, between])))
    out.append(('zero-area-box', f([A, A2, corner]), f([[0, 0, 3, 5], [40, 40, 39, 39]])))       # 0 x 0 pixels: IoU 0 everywhere
    out.append(('one-anchor', f([A]), f([[0, 0, 3, 5], [0, 0, 3, 5]])))
    for g, n, seed in ((1, 300, 1), (257, 1000, 2), (1024, 1000, 3)):
        a, b = _grid_case(g, n, seed)
        if g == 1:                                            # one box between two lattice anchors (rows 0 and 299)
            b = f([[6, 8, 9, 11]])
            a[0], a[-1] = [4, 8, 7, 11], [8, 8, 11, 11]
        out.append(('lattice-G%d' % g, a, b))
    return out


@functools.lru_cache(maxsize=None)
def proposal_tie_cases():
    """[(name, rois [R,4], gt [G,4], gt_labels [G])] with POS / NEG: every case has duplicated RoI rows; the RoIs of the first
    reach pos, neg and 1 exactly and both cases meet duplicated boxes"""
    f = np.float32
    tall = [0, 16, 3, 23]
    rois = f([[0, 16, 3, 19], [0, 22, 3, 23], [0, 16, 3, 19], tall, [0, 22, 3, 23], [100, 100, 120, 120], tall,
              [0, 16, 3, 20], [0, 21, 3, 23]])
    out = [('pos-neg-duplicates', rois, f([tall, tall, [40, 40, 47, 47]]), np.int64([3, 7, 5]))]
    a, b = _grid_case(40, 200, 4)
    a = np.concatenate([a[a.min(axis=1) >= 0], a[:20]])
    out.append(('lattice', a.astype(f), b, np.random.default_rng(5).integers(1, 21, 40).astype(np.int64)))
    return out
