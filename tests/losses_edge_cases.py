"""The edge-case table of the fused training losses (csrc/losses.hip): hand-made compact targets at the sizes where the kernels
take another path -- class chunks of a wave, 4C against 64 columns, rows against the 8 waves, the limits, head rows against
target rows, the clamps on the counts, stray indices and labels, the exponential's subnormal range and the smooth-L1 switch.
Every case is ONE call (a batch); `reaches` names the path facts the case is there for, and `path(case)` recomputes them from
the kernel's constants, so tests/test_losses_edges_host.py can assert that the case gets where it says.  The expected outputs
come from tests/losses_np.py image by image (`expected`); tests/test_losses_edges_gpu.py compares bytes."""
import numpy as np

import losses_np as ln

F32 = np.float32
WAVE = 64                      # ODET_WAVE
LS_MAX_SAMPLES = 1024
LS_MAX_CLASSES = 1024
LS_MAX_ROWS = 2048
LS_ROI_WAVES = 8               # LS_ROI_THREADS / ODET_WAVE
MAX_BATCH = 64
FILL_THREADS, FILL_MAX_BLOCKS, FILL_STORES = 256, 8192, 4

UPSTREAMS = (np.float32([1.25, 0.5]), np.float32([-0.75, -2.0]))     # positive and negative: a -0 must be a -0

# gaps x_j - max: e = 1; e a float32 subnormal (-87.4 .. -103.9); e = 0 just below -103.98 and at -200
GAPS = [0.0, -87.5, -95.25, -103.5, -103.9, -103.99, -200.0]


# ---- RoI ------------------------------------------------------------------------------------------------------------------
def roi_case(name, C, R, S, B=1, counts3=None, row_map=None, sigma=1.0, seed=0, reaches=None):
    """random head outputs and targets of the shape odet_proposal_target writes; counts3: counts[3] per image (default S)"""
    rng = np.random.default_rng(1000 + seed)
    W = 4 * C
    labels = rng.integers(0, C, (B, S)).astype(np.int32)
    targets, inside, outside = (np.zeros((B, S, W), F32) for _ in range(3))
    cls = rng.integers(0, C, (B, S))
    for k in range(4):
        col = (4 * cls + k)[..., None]
        np.put_along_axis(targets, col, rng.normal(0, 1, (B, S, 1)).astype(F32), axis=2)
        np.put_along_axis(inside, col, F32(1), axis=2)
    outside[:] = (inside != 0) * rng.choice(np.float32([1.0, 0.5]), (B, S, 1))
    counts3 = [S] * B if counts3 is None else list(counts3)
    counts = np.array([[max(c, 0), 0, 0, c] for c in counts3], np.int32).reshape(B, 4)
    scores = rng.uniform(-30, 30, (B, R, C)).astype(F32)
    scores[:, ::2] = rng.normal(0, 2, scores[:, ::2].shape)
    deltas = rng.normal(0, 1, (B, R, W)).astype(F32)
    rm = None if row_map is None else np.broadcast_to(np.asarray(row_map, np.int32), (B, R)).copy()
    thr = 1.0 / sigma ** 2
    for b in range(B):                                               # differences on both sides of 1 / sigma_2
        m = np.arange(R) if rm is None else rm[b]
        ok = (m >= 0) & (m < S)
        near = targets[b][m[ok]] + rng.uniform(-2.5 * thr, 2.5 * thr, (int(ok.sum()), W))
        deltas[b, ok] = np.where(inside[b][m[ok]] != 0, near, deltas[b, ok]).astype(F32)
    return dict(kind='roi', name=name, C=C, R=R, S=S, B=B, scores=scores, deltas=deltas, labels=labels, targets=targets,
                inside=inside, outside=outside, counts=counts, row_map=rm, sigma=sigma, reaches=reaches or {})


def roi_path(c):
    """what the kernel does with the case, from its constants"""
    C, R, S = c['C'], c['R'], c['S']
    chunks = -(-C // WAVE)
    out = dict(class_chunks=chunks, last_chunk=C - WAVE * (chunks - 1),
               columns='below' if 4 * C < WAVE else ('equal' if 4 * C == WAVE else 'above'),
               row_trips=-(-R // LS_ROI_WAVES), idle_waves=(-R) % LS_ROI_WAVES if R else LS_ROI_WAVES,
               at_class_limit=C == LS_MAX_CLASSES, at_row_limit=R == LS_MAX_ROWS, at_sample_limit=S == LS_MAX_SAMPLES,
               at_batch_limit=c['B'] == MAX_BATCH)
    rows = [min(max(int(k), 0), S) for k in c['counts'][:, 3]]
    out['rows'] = rows
    out['clamped_high'] = [int(k) > S for k in c['counts'][:, 3]]
    out['clamped_low'] = [int(k) < 0 for k in c['counts'][:, 3]]
    took, bad_label, unmapped, dup = [], [], [], []
    for b in range(c['B']):
        m = np.arange(R) if c['row_map'] is None else c['row_map'][b]
        ok = (m >= 0) & (m < rows[b])
        lab = np.where(ok, c['labels'][b][np.where(ok, m, 0)], 0)
        good = ok & (lab >= 0) & (lab < C)
        took.append(int(good.sum()))
        bad_label.append(int((ok & ~good).sum()))
        unmapped.append(int((~ok).sum()))
        dup.append(int(ok.sum() - len(np.unique(m[ok]))))
    out.update(rows_taking_part=took, rows_with_a_stray_label=bad_label, rows_without_a_target=unmapped, duplicate_targets=dup)
    return out


def _exp_rows(C=8):
    """[rows, C] logits and a label per row around the exponential's range"""
    rows, labels = [], []
    for shift in (0.0, 17.5):                                        # the maximum need not be 0
        x = np.full(C, -200.0, F32)
        x[:len(GAPS)] = GAPS
        rows += [x + F32(shift), (x + F32(shift))[::-1].copy()]
        labels += [0, 3]                                             # the maximum; a subnormal / zero exponential
    rows.append(np.float32([0, -200] + [-200] * (C - 2)))            # probability 1 on the label: CE = 0
    labels.append(0)
    rows.append(np.float32([0, -200] + [-150] * (C - 2)))            # probability 0 on the label: CE = 200
    labels.append(1)
    for v in (0.0, -7.25, 3e38, -3e38):                              # all classes equal
        rows.append(np.full(C, v, F32))
        labels.append(C - 1)
    x = np.full(C, -3e38, F32)
    x[2] = 3e38
    rows.append(x)                                                   # gaps of -inf
    labels.append(2)
    x = np.float32([3e38, 3e38, -3e38, 0, 1, -1, 88, -104][:C])
    rows.append(x)
    labels.append(1)
    return np.stack(rows), np.array(labels, np.int32)


def roi_exp_case():
    x, lab = _exp_rows()
    R, C = x.shape
    c = roi_case('the exponential\'s range', C, R, R, seed=41, reaches=dict(class_chunks=1))
    c['scores'][0] = x
    c['labels'][0] = lab
    return c


def switch_values(sigma):
    """|d| at float32(1 / sigma_2) and its two float32 neighbours, both signs"""
    thr = ln.sl_const(sigma)[1]
    v = [np.nextafter(thr, F32(0)), thr, np.nextafter(thr, F32(2))]
    return np.float32(v + [-x for x in v])


def roi_switch_case(sigma):
    c = roi_case('smooth-L1 switch, sigma %g' % sigma, 2, 3, 3, sigma=sigma, seed=50, reaches=dict(columns='below'))
    v = switch_values(sigma)
    c['targets'][:] = 0
    c['inside'][:] = 1
    c['outside'][:] = 1
    c['deltas'][0] = 0
    c['deltas'][0, 0, :6] = v
    c['deltas'][0, 1, 2:8] = v[::-1]
    return c


def roi_cases():
    out = []
    for C, facts in ((1, dict(class_chunks=1, last_chunk=1, columns='below')), (2, dict(columns='below')),
                     (16, dict(columns='equal')), (63, dict(class_chunks=1, last_chunk=63, columns='above')),
                     (64, dict(class_chunks=1, last_chunk=64)), (65, dict(class_chunks=2, last_chunk=1)),
                     (128, dict(class_chunks=2, last_chunk=64)), (129, dict(class_chunks=3, last_chunk=1)),
                     (1024, dict(class_chunks=16, last_chunk=64, at_class_limit=True))):
        R = 8 if C == 1024 else 9
        out.append(roi_case('C = %d' % C, C, R, 8, seed=C, reaches=facts))
    for R, facts in ((0, dict(row_trips=0)), (1, dict(row_trips=1, idle_waves=7)), (7, dict(row_trips=1, idle_waves=1)),
                     (8, dict(row_trips=1, idle_waves=0)), (9, dict(row_trips=2, idle_waves=7))):
        out.append(roi_case('R = %d' % R, 5, R, 16, counts3=[12], seed=100 + R, reaches=facts))
    # R above S: every target row twice, some head rows without one; at the row and the sample limit
    rng = np.random.default_rng(7)
    rm = np.concatenate([rng.permutation(1024), rng.permutation(1024)]).astype(np.int32)
    rm[rng.choice(2048, 40, replace=False)] = -1
    out.append(roi_case('R = 2048, S = 1024', 3, 2048, 1024, row_map=rm, seed=2048,
                        reaches=dict(row_trips=256, at_row_limit=True, at_sample_limit=True, rows_without_a_target=[40],
                                     duplicate_targets=[2048 - 40 - len(np.unique(rm[rm >= 0]))])))
    rm = np.int32([3, 3, -1, 0, 7, 7, 7, 1, 2, -1, 5, 6, 4])
    out.append(roi_case('R above S with duplicates and -1', 5, 13, 8, row_map=rm, seed=13,
                        reaches=dict(rows_without_a_target=[2], duplicate_targets=[3], rows_taking_part=[11])))
    out.append(roi_case('R below rows', 5, 5, 8, seed=14, reaches=dict(rows=[8], rows_taking_part=[5])))
    out.append(roi_case('counts[3] in -1, 0, 1, S, S + 5', 4, 6, 6, B=5, counts3=[-1, 0, 1, 6, 11], seed=15,
                        reaches=dict(rows=[0, 0, 1, 6, 6], clamped_low=[True, False, False, False, False],
                                     clamped_high=[False, False, False, False, True], rows_taking_part=[0, 0, 1, 6, 6])))
    c = roi_case('labels of -1 and C on rows that would take part', 4, 8, 8, seed=16,
                 reaches=dict(rows=[8], rows_with_a_stray_label=[3], rows_taking_part=[5]))
    c['labels'][0, [1, 4, 6]] = [-1, 4, -1]
    out.append(c)
    out.append(roi_case('S = 1', 4, 3, 1, seed=17, reaches=dict(rows=[1], rows_taking_part=[1])))
    out.append(roi_case('batch 64', 3, 4, 4, B=64, seed=18, reaches=dict(at_batch_limit=True)))
    out.append(roi_case('batch 0', 3, 4, 4, B=0, seed=19))
    out.append(roi_exp_case())
    out += [roi_switch_case(s) for s in (1.0, 2.0, 3.0)]
    return out


# (what, C, R, S, B) of the calls that must return ODET_E_LIMIT
ROI_OVER_LIMIT = [('C = 1025', 1025, 2, 2, 1), ('R = 2049', 2, 2049, 2, 1), ('S = 1025', 2, 2, 1025, 1), ('batch 65', 2, 2, 2, 65)]


def roi_expected(c, upstream=None):
    """per image: dict(losses, grad_scores, grad_deltas)"""
    return [ln.roi_loss(c['scores'][b], c['deltas'][b], c['labels'][b], c['targets'][b], c['inside'][b], c['outside'][b],
                        c['counts'][b], c['sigma'], None if c['row_map'] is None else c['row_map'][b], upstream)
            for b in range(c['B'])]


# ---- RPN ------------------------------------------------------------------------------------------------------------------
RPN_N = 1080                   # a multiple of A = 1, 9 and 15, above the sample limit


def rpn_case(name, S, images, layout=ln.LAYOUT_FPN, A=1, N=RPN_N, sigma=3.0, seed=0, reaches=None):
    """images: [(kfg, kbg)] as the counts say them (unclamped; (-1, -1) = an image over the box limit).  The first sampled
    rows of every image hold the indices 0 and N - 1."""
    rng = np.random.default_rng(2000 + seed)
    B = len(images)
    assert N % A == 0
    idx = -np.ones((B, S), np.int32)
    tg = np.zeros((B, S, 4), F32)
    counts = np.zeros((B, 5), np.int32)
    scores = rng.uniform(-30, 30, (B, N, 2)).astype(F32)
    scores[:, ::3] = rng.normal(0, 2, scores[:, ::3].shape)
    deltas = rng.normal(0, 1, (B, N, 4)).astype(F32)
    thr = 1.0 / sigma ** 2
    for b, (kfg, kbg) in enumerate(images):
        counts[b] = [N, max(kfg, 0), max(kbg, 0), kfg, kbg] if kfg >= 0 and kbg >= 0 else [-1] * 5
        pick = rng.permutation(np.arange(1, N - 1))[:S]
        pick[:2] = [N - 1, 0][:min(S, 2)]
        idx[b] = pick                                                # (every one of the S entries is a real index: the clamps
        tg[b] = rng.normal(0, 1, (S, 4))                             #  decide which of them count)
        deltas[b, pick] = tg[b] + rng.uniform(-2.5 * thr, 2.5 * thr, (S, 4)).astype(F32)
    flat = np.stack([ln.from_fpn_view(s, layout, A) for s in scores]) if B else scores.reshape(0, 2 * N)
    return dict(kind='rpn', name=name, S=S, N=N, B=B, layout=layout, A=A, sigma=sigma, scores=flat, deltas=deltas,
                sample_idx=idx, sample_targets=tg, counts=counts, reaches=reaches or {})


def rpn_path(c):
    S = c['S']
    out = dict(n=[], kfg=[], waves=[], clamped_sum=[], clamped_kfg=[], emptied=[], stray=[])
    for b in range(c['B']):
        kfg, kbg = int(c['counts'][b, 3]), int(c['counts'][b, 4])
        neg = kfg < 0 or kbg < 0
        if neg:
            kfg = kbg = 0
        out['emptied'].append(neg)
        out['clamped_kfg'].append(kfg > S)
        out['clamped_sum'].append(kfg + kbg > S)
        kfg = min(kfg, S)
        n = min(kfg + kbg, S)
        out['n'].append(n)
        out['kfg'].append(kfg)
        out['waves'].append(-(-n // WAVE))
        i = c['sample_idx'][b, :n]
        out['stray'].append(int(((i < 0) | (i >= c['N'])).sum()))
    out['at_sample_limit'] = S == LS_MAX_SAMPLES
    return out


def rpn_exp_case():
    """two-class rows over the gaps, as foreground and as background rows"""
    gaps = GAPS + [-np.inf]
    S = 4 * len(gaps)
    c = rpn_case('the exponential\'s range', S, [(S // 2, S // 2)], seed=60, reaches=dict(n=[S]))
    x = ln.fpn_view(c['scores'][0], c['layout'], c['A'])
    for r in range(S):
        g, swap = gaps[r % len(gaps)], (r // len(gaps)) % 2
        if np.isinf(g):                                              # (the label on the maximum: the loss stays finite)
            x[c['sample_idx'][0, r]] = [-3e38, 3e38] if r < S // 2 else [3e38, -3e38]
            continue
        pair = np.float32([5.5, 5.5 + g])
        x[c['sample_idx'][0, r]] = pair[::-1] if swap else pair
    x[c['sample_idx'][0, 0]] = [2.5, 2.5]                            # both classes equal
    return c


def rpn_switch_case(sigma):
    c = rpn_case('smooth-L1 switch, sigma %g' % sigma, 4, [(3, 1)], sigma=sigma, seed=70, reaches=dict(kfg=[3]))
    v = switch_values(sigma)
    c['sample_targets'][:] = 0
    i = c['sample_idx'][0]
    c['deltas'][0, i[0]] = v[:4]
    c['deltas'][0, i[1]] = v[2:]
    c['deltas'][0, i[2]] = v[[5, 0, 4, 1]]
    return c


def rpn_cases():
    out = []
    for S in (1, 63, 64, 65, 1024):
        out.append(rpn_case('S = %d' % S, S, [(S // 2, S - S // 2)], seed=S,
                            reaches=dict(n=[S], waves=[-(-S // WAVE)], at_sample_limit=S == 1024)))
    out.append(rpn_case('counts', 64, [(0, 64), (10, 0), (64, 0), (40, 40), (70, 5), (-1, -1), (0, 0), (3, -1)], seed=80,
                        reaches=dict(n=[64, 10, 64, 64, 64, 0, 0, 0], kfg=[0, 10, 64, 40, 64, 0, 0, 0],
                                     clamped_sum=[False, False, False, True, True, False, False, False],
                                     clamped_kfg=[False, False, False, False, True, False, False, False],
                                     emptied=[False, False, False, False, False, True, False, True])))
    for layout, A in ((ln.LAYOUT_FPN, 1), (ln.LAYOUT_FRCNN, 1), (ln.LAYOUT_FRCNN, 9), (ln.LAYOUT_FRCNN, 15)):
        c = rpn_case('layout %d, A = %d, stray indices' % (layout, A), 32, [(12, 14), (5, 3)], layout, A, seed=90 + A,
                     reaches=dict(n=[26, 8], stray=[3, 1]))
        c['sample_idx'][0, [3, 13, 20]] = [-1, RPN_N, -7]            # a foreground row, background rows: inside the first n
        c['sample_idx'][1, 2] = RPN_N + 5
        c['sample_idx'][1, 20] = -1                                  # (past n: not a row at all)
        out.append(c)
    out.append(rpn_exp_case())
    out += [rpn_switch_case(s) for s in (1.0, 2.0, 3.0)]
    return out


RPN_OVER_LIMIT = [('S = 1025', 1025, 1), ('batch 65', 8, 65)]


def rpn_expected(c, upstream):
    """per image: dict(losses, row_grad_scores, row_grad_deltas, grad_scores, grad_deltas) at upstream [B,2]"""
    out = []
    for b in range(c['B']):
        r = ln.rpn_loss(c['scores'][b], c['deltas'][b], c['sample_idx'][b], c['sample_targets'][b], c['counts'][b], c['sigma'],
                        c['layout'], c['A'])
        r['grad_scores'], r['grad_deltas'] = ln.rpn_loss_backward(c['sample_idx'][b], r['row_grad_scores'], r['row_grad_deltas'],
                                                                  upstream[b], c['N'], c['layout'], c['A'])
        out.append(r)
    return out


# ---- the dense gradients' zero fill -------------------------------------------------------------------------------------------
def fill_path(N, B, scores=True, deltas=True):
    """k_zero_fill2 as odet_rpn_loss_backward launches it"""
    n0, n1 = (2 * N * B if scores else 0), (4 * N * B if deltas else 0)
    vec = n0 // 4 + n1 // 4
    blocks = min(max(-(-vec // (FILL_THREADS * FILL_STORES)), 1), FILL_MAX_BLOCKS)
    return dict(tail_scores=n0 % 4, tail_deltas=n1 % 4, vectors=vec, blocks=blocks, trips=-(-vec // (blocks * FILL_THREADS)))


def backward_case(name, N, B, S=16, scores=True, deltas=True, seed=0, reaches=None):
    """row gradients of any value scattered into N anchors: indices 0 and N - 1, one stray each side, distinct otherwise"""
    rng = np.random.default_rng(3000 + seed)
    idx = -np.ones((B, S), np.int32)
    k = min(S - 4, N - 2)
    for b in range(B):
        idx[b, :4] = [0, N - 1, -1, N]
        idx[b, 4:4 + k] = rng.permutation(np.arange(1, N - 1))[:k]
    return dict(kind='rpn_bwd', name=name, N=N, B=B, S=S, want_scores=scores, want_deltas=deltas, sample_idx=idx,
                row_gs=rng.normal(0, 1, (B, S, 2)).astype(F32), row_gd=rng.normal(0, 1, (B, S, 4)).astype(F32),
                upstream=rng.normal(0, 1, (B, 2)).astype(F32), reaches=reaches or {})


BIG_FILL = dict(N=100003, B=64)    # 2NB + 4NB floats = 154 MB: more vectors than 8192 blocks x 256 lanes x 4 stores


def backward_cases():
    out = []
    for B in (1, 3):
        out.append(backward_case('N odd, B = %d' % B, 1001, B, seed=B, reaches=dict(tail_scores=2, tail_deltas=0)))
    out.append(backward_case('grad_scores alone', 1001, 3, deltas=False, seed=5, reaches=dict(tail_scores=2)))
    out.append(backward_case('grad_deltas alone', 1001, 3, scores=False, seed=6, reaches=dict(tail_scores=0, tail_deltas=0)))
    out.append(backward_case('N = 3', 3, 1, S=6, seed=7, reaches=dict(vectors=4, tail_scores=2, blocks=1, trips=1)))
    return out


def backward_expected(c):
    return [ln.rpn_loss_backward(c['sample_idx'][b], c['row_gs'][b], c['row_gd'][b], c['upstream'][b], c['N'])
            for b in range(c['B'])]


def smooth_l1_le(pred, tgt, inside, outside, sigma):
    """losses_np.smooth_l1 with `<=` at the switch (for counting where the comparison's strictness shows)"""
    s2, thr, half_s2, half_inv = ln.sl_const(sigma)
    pred, tgt, inside, outside = (np.asarray(v, F32) for v in (pred, tgt, inside, outside))
    d = inside * (pred - tgt)
    ad = np.abs(d)
    sign = (ad <= thr).astype(F32)
    in_loss = d * d * half_s2 * sign + (ad - half_inv) * (F32(1) - sign)
    slope = np.where(sign != 0, s2 * d, np.where(d > 0, F32(1), F32(-1))).astype(F32)
    return outside * in_loss, outside * inside * slope
