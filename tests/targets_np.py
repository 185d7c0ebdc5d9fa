"""numpy restatement of the fused training targets (include/odet.h "training targets"): Philox4x32-10, key64, the
selection rule and both target functions end to end, on top of the oracle's deterministic halves
(oracle_np.anchor_target_labels, proposal_target_assign, encode_bbox_with_mean_and_std).  The checker of
tests/test_targets_host.py and tests/test_targets_gpu.py; the product never imports it."""
import numpy as np

from oracle import oracle_np as on

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF

STREAM_ANCHOR_FG, STREAM_ANCHOR_BG, STREAM_ROI_FG, STREAM_ROI_BG, STREAM_ROI_REPLACE = 0, 1, 2, 3, 4


def philox(ctr, key):
    """Philox4x32 with 10 rounds.  ctr: four uint32 (scalars or equal-shape arrays), key: two uint32 -> four uint64 arrays
    holding the 32-bit output words."""
    c = [np.asarray(v, np.uint64) & np.uint64(MASK) for v in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def _seed_words(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & MASK, seed >> 32


def key64(stream, image_id, i, seed, key_mask=None):
    """(w0 << 32) | w1 of philox((i, image_id, stream, 0), seed words) for an array of candidate indices i.  key_mask (None =
    all ones) is ANDed onto the key: the diagnostic build's odet_debug_tg_key_mask, which makes keys collide."""
    w = philox((np.asarray(i, np.uint64), image_id, stream, 0), _seed_words(seed))
    return _masked((w[0] << np.uint64(32)) | w[1], key_mask)


def _masked(keys, key_mask):
    return keys if key_mask is None else keys & np.uint64(int(key_mask) & 0xFFFFFFFFFFFFFFFF)


def select(candidates, k, stream, image_id, seed, key_mask=None):
    """The k candidates (int array of indices) with the smallest (key64, index) pairs, in ascending pair order."""
    cand = np.asarray(candidates, np.int64)
    if k <= 0:
        return cand[:0]
    keys = _masked(key64(stream, image_id, cand, seed), key_mask)          # the mask goes onto the 64-bit key before the sort
    order = np.lexsort((cand, keys))              # last key is the primary one
    return cand[order[:k]]


def selection_trace(keys, indices, k):
    """COVERAGE ACCOUNTING ONLY (never decides whether a kernel output is right: that is select()'s lexsort).  Mirrors the digit
    walk of d_tg_radix_select over V = key64 * 2^20 + i in seven 12-bit digits, most significant first, for the k-th smallest
    (key, index) pair of the candidates.  -> dict(levels=[dict(level, occupied, below, count, need)], end, threshold, kth):
    per level visited the number of occupied bins among the candidates still in play, the candidates in bins below the chosen
    one, the chosen bin's count and the rows still needed from it (the walk ends where count == need); `end` the level the
    walk ended on (None: k <= 0 or k >= n, the kernel returns before the walk); `threshold` the (key, index) pair the walk
    leaves (remaining low bits all ones, the index 0xFFFFFFFF when it ended above the index digits) and `kth` the largest
    candidate pair not above it."""
    keys = np.asarray(keys, np.uint64)
    idx = np.asarray(indices, np.int64)
    out = dict(levels=[], end=None, threshold=None, kth=None)
    if k <= 0 or len(keys) <= k:
        return out
    play = np.ones(len(keys), bool)
    pk, pi, need = 0, 0, int(k)
    for l in range(7):
        shift = 72 - 12 * l
        if shift >= 20:
            d = ((keys >> np.uint64(shift - 20)) & np.uint64(0xFFF)).astype(np.int64)
        elif l == 5:
            d = ((keys & np.uint64(0xF)).astype(np.int64) << 8) | ((idx >> 12) & 0xFF)
        else:
            d = idx & 0xFFF
        hist = np.bincount(d[play], minlength=4096)
        run = np.cumsum(hist)
        digit = int(np.searchsorted(run, need))                   # the first bin whose inclusive count reaches `need`
        below, count = int(run[digit] - hist[digit]), int(hist[digit])
        need -= below
        out['levels'].append(dict(level=l, occupied=int(np.count_nonzero(hist)), below=below, count=count, need=need))
        play &= d == digit
        if shift >= 20:
            pk |= digit << (shift - 20)
        elif l == 5:
            pk |= digit >> 8
            pi |= (digit & 0xFF) << 12
        else:
            pi |= digit
        if count == need:
            if shift >= 20:
                pk |= (1 << (shift - 20)) - 1
                pi = 0xFFFFFFFF
            else:
                pi |= (1 << shift) - 1
            out['end'] = l
            break
    out['threshold'] = (pk, pi)
    kept = (keys < np.uint64(pk)) | ((keys == np.uint64(pk)) & (idx <= pi))
    order = np.lexsort((idx[kept], keys[kept]))
    out['kept'] = int(kept.sum())
    out['kth'] = (int(keys[kept][order[-1]]), int(idx[kept][order[-1]]))
    return out


def replacement_pick(j, n_bg, image_id, seed):
    """index into bg_ascending of with-replacement draw j (array)"""
    w0 = philox((np.asarray(j, np.uint64), image_id, STREAM_ROI_REPLACE, 0), _seed_words(seed))[0]
    return ((w0 * np.uint64(n_bg)) >> np.uint64(32)).astype(np.int64)


def anchor_target(gt, image_shape, anchors, pos, neg, total, max_pos, means, stds, seed=0, image_id=0, key_mask=None):
    """One image -> dict of every output of odet_anchor_target (dense surface, compact form, parity outputs)."""
    anchors = np.asarray(anchors, np.float32)
    gt = np.asarray(gt, np.float32).reshape(-1, 4)
    n = anchors.shape[0]
    if gt.shape[0] > 0:
        idx, lab, am = on.anchor_target_labels(gt, image_shape, anchors, pos, neg)
    else:                                          # defined here, not by the reference: background only
        idx = on.bboxes_range_filter(anchors, image_shape[0], image_shape[1])
        lab = np.zeros(len(idx), np.int32) if np.float32(0) < np.float32(neg) else -np.ones(len(idx), np.int32)
        if np.float32(0) >= np.float32(pos):
            lab[:] = 1
        am = -np.ones(len(idx), np.int64)
    before = -np.ones(n, np.int32); before[idx] = lab
    argmax = -np.ones(n, np.int32); argmax[idx] = am
    fg, bg = np.nonzero(before == 1)[0], np.nonzero(before == 0)[0]
    kept_fg = np.sort(select(fg, min(len(fg), max_pos), STREAM_ANCHOR_FG, image_id, seed, key_mask))
    kept_bg = np.sort(select(bg, min(len(bg), max(total - len(kept_fg), 0)), STREAM_ANCHOR_BG, image_id, seed, key_mask))
    labels = -np.ones(n, np.float32)
    labels[kept_fg] = 1
    labels[kept_bg] = 0
    targets = np.zeros((n, 4), np.float32)
    if gt.shape[0] > 0:
        targets[idx] = on.encode_bbox_with_mean_and_std(anchors[idx], gt[am], means, stds)
    inside = np.zeros((n, 4), np.float32); inside[labels == 1] = 1
    outside = np.zeros((n, 4), np.float32)
    if len(kept_fg) + len(kept_bg):
        outside[labels >= 0] = np.float32(1) / np.float32(len(kept_fg) + len(kept_bg))
    sample_idx = -np.ones(total, np.int32)
    both = np.concatenate([kept_fg, kept_bg])
    sample_idx[:len(both)] = both
    sample_targets = np.zeros((total, 4), np.float32)
    sample_targets[:len(both)] = targets[both]
    counts = np.array([len(idx), len(fg), len(bg), len(kept_fg), len(kept_bg)], np.int32)
    return dict(labels=labels, targets=targets, inside=inside, outside=outside, sample_idx=sample_idx,
                sample_targets=sample_targets, counts=counts, labels_before_sampling=before, argmax=argmax)


def proposal_target(rois, gt, gt_labels, num_classes, pos, neg, total, max_pos, means, stds, reference_row_labels=True,
                    seed=0, image_id=0, key_mask=None):
    """One image -> dict of every output of odet_proposal_target (key_mask: the selection keys only, not the with-replacement
    draw)."""
    rois = np.asarray(rois, np.float32).reshape(-1, 4)
    gt = np.asarray(gt, np.float32).reshape(-1, 4)
    gt_labels = np.asarray(gt_labels, np.int64)
    r = rois.shape[0]
    if gt.shape[0] > 0:
        labels, ga, fg, bg = on.proposal_target_assign(rois, gt, gt_labels, pos, neg)
    else:
        labels, ga = np.zeros(r, np.int64), -np.ones(r, np.int64)
        fg = np.arange(r) if np.float32(0) >= np.float32(pos) else np.arange(0)
        bg = np.arange(r) if np.float32(neg) <= np.float32(0) < np.float32(pos) else np.arange(0)
    if len(fg) > max_pos:
        kfg = select(fg, max_pos, STREAM_ROI_FG, image_id, seed, key_mask)         # ascending (key64, i)
    else:
        kfg = np.sort(fg)
    want = total - len(kfg)
    if len(bg) > want:
        kbg = select(bg, want, STREAM_ROI_BG, image_id, seed, key_mask)
    elif len(bg) == want or len(bg) == 0:
        kbg = np.sort(bg)
    else:
        kbg = np.sort(bg)[replacement_pick(np.arange(want), len(bg), image_id, seed)]
    keep_rows = np.concatenate([kfg, kbg]).astype(np.int64)
    rows, nfg = len(keep_rows), len(kfg)
    w = 4 * num_classes
    out = dict(final_rois=np.zeros((total, 4), np.float32), final_labels=np.zeros(total, np.int32),
               targets=np.zeros((total, w), np.float32), inside=np.zeros((total, w), np.float32),
               outside=np.zeros((total, w), np.float32), keep=-np.ones(total, np.int32),
               gt_assignment=ga.astype(np.int32), counts=np.array([len(fg), len(bg), nfg, rows], np.int32))
    out['final_rois'][:rows] = rois[keep_rows]
    out['final_labels'][:nfg] = labels[kfg]
    out['keep'][:rows] = keep_rows
    out['outside'][:rows] = 1
    if nfg and gt.shape[0] > 0:
        enc = on.encode_bbox_with_mean_and_std(rois[kfg], gt[ga[kfg]], means, stds)
        cols = labels[:nfg] if reference_row_labels else labels[kfg]
        for row in range(nfg):
            c = int(cols[row])
            out['targets'][row, 4 * c:4 * c + 4] = enc[row]
            out['inside'][row, 4 * c:4 * c + 4] = 1
    return out
