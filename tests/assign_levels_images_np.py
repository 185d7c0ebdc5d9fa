"""NumPy restatement of odet_assign_levels_images from the header's text alone -- image b of dense [B,n,...] tensors is what
odet_assign_levels writes for image b alone (the oracle's level rule and stable partition: tests/box_edge_cases.py), rows at or
beyond cnt_b = min(count[b], n) are NOT written, counts[b, :] always is -- and the case table: the smallest shapes at which the
batched kernel can go wrong.  It shares no code with ops.py."""
import numpy as np

import box_edge_cases as ec

ROI_FILL, LEVEL_FILL, PERM_FILL, COUNT_FILL = np.float32(-7.0), np.int32(-9), np.int64(-5), np.int32(-3)
MAX_ROIS = 8192          # ODET_ASSIGN_MAX_ROIS: 1024 threads x 8 items


def effective_counts(counts, B, n):
    """cnt_b = min(count[b], n), or n without counts"""
    if counts is None:
        return [n] * B
    return [max(min(int(c), n), 0) for c in counts]


def restate(rois, counts, min_level, max_level):
    """-> (sorted rois [B,n,4], level int32 [B,n], perm int64 [B,n], level counts int32 [B,L]) with the *_FILL values wherever the
    kernel writes nothing"""
    rois = np.asarray(rois, np.float32)
    B, n = rois.shape[:2]
    L = max_level - min_level + 1
    out = np.full((B, n, 4), ROI_FILL, np.float32)
    level = np.full((B, n), LEVEL_FILL, np.int32)
    perm = np.full((B, n), PERM_FILL, np.int64)
    lcounts = np.zeros((B, L), np.int32)
    for b, c in enumerate(effective_counts(counts, B, n)):
        if c:
            out[b, :c], level[b, :c], perm[b, :c], lcounts[b] = ec.assign_levels(rois[b, :c], min_level, max_level)
    return out, level, perm, lcounts


def _random_rois(rng, n):
    """upright boxes whose sqrt(area) is log-uniform over 30 .. 900: all four of the levels 2 .. 5, interleaved"""
    edge = np.exp(rng.uniform(np.log(30.0), np.log(900.0), n))
    aspect = np.exp(rng.uniform(-0.7, 0.7, n))
    w, h = edge * aspect, edge / aspect
    x0, y0 = rng.uniform(0, 300, n), rng.uniform(0, 300, n)
    return np.stack([x0, y0, x0 + w, y0 + h], axis=1).astype(np.float32)


class Case:
    def __init__(self, name, rois, counts, min_level=2, max_level=5):
        self.name, self.rois, self.counts = name, np.ascontiguousarray(rois, np.float32), counts
        self.min_level, self.max_level = min_level, max_level
        self.B, self.n = self.rois.shape[:2]
        assert self.n <= MAX_ROIS

    def cnt(self):
        return effective_counts(self.counts, self.B, self.n)

    def restated(self):
        return restate(self.rois, self.counts, self.min_level, self.max_level)


def _random_case(name, B, n, counts, seed):
    rng = np.random.default_rng(seed)
    return Case(name, np.stack([_random_rois(rng, n) for _ in range(B)]), counts)


def _boundary_case(min_level, max_level):
    """image 0: the float32 neighbours of every level boundary (box_edge_cases.level_sweep, its odd rows included); image 1: the
    same rows in another order with every third one replaced by a random box, so that its levels (another count per level) and
    its permutation are other bytes"""
    sweep, _ = ec.level_sweep()
    rng = np.random.default_rng(77)
    other = sweep[rng.permutation(len(sweep))]
    other[::3] = _random_rois(rng, len(other[::3]))
    return Case('b2_level_boundaries_%d_%d' % (min_level, max_level), np.stack([sweep, other]), None, min_level, max_level)


CASES = [
    _random_case('b3_n13_counts_13_0_5', 3, 13, [13, 0, 5], 1),
    _random_case('b2_n8192_all_items', 2, MAX_ROIS, [MAX_ROIS, MAX_ROIS], 2),          # every thread's 8 items
    _boundary_case(2, 5),
    _boundary_case(0, 7),
    _random_case('b2_n13_count_above_n', 2, 13, [20, 7], 3),
]
BY_NAME = {c.name: c for c in CASES}
