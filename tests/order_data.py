"""Data on which the ORDER of a float64 sum shows in the float32 result, for every ordered sum of the training kernels
(include/odet.h "training losses" and the L2 sum of "training step"), with the wrong orders each data set tells apart from the
header's.  On random data a float64 sum of a few hundred float32 terms rounds to the same float32 in any order; here the sum
sits exactly on a float32 tie and carries terms that a float64 accumulator loses one at a time but keeps when they are added
together first.

Construction A (non-negative terms): BIG + TIE = 2^p + 2^(p-24) is exactly half way between two float32 values and rounds to
the even one, 2^p.  A SMALL term is at most half a float64 unit there (2^(p-53)): added to the running sum it is lost, added
to another SMALL first it is kept and lifts the sum over the tie, to 2^p + 2^(p-23).  NORMAL = 2^(p-40) is kept by a float64
accumulator (over the tie: up) and lost by a float32 one.  Smooth-L1 terms of these sizes come from the linear branch with
target 0, cross-entropy terms from a label logit of -v against a maximum of 0 (e_label = 0, s = 1, log = 0: CE = v exactly).

Construction B (the class sum of a softmax row): e_0 = 1, e_1 = exp(z1) an odd multiple of 2^-24 in [0.5, 1) whose tie 1 + e_1
rounds DOWN, and classes with e < 2^-53.  Every z of such a row has its float64 exponential (and log s its float64 value) at
least 1000 float64 units from a float32 rounding boundary, so a last-bit difference between two libraries' exp / log cannot
move the float32 bits.

A data set is a dict: `kind` ('rpn' | 'roi' | 'l2' | 'add_n'), `sum` (its row of TABLE), `name`, `wrong` (the names of the
wrong orders it separates), `watch` (the outputs the order shows in) and the inputs of ONE image / tensor list for the real
entry point.  `expected(ds)` is the header's result, `expected(ds, wrong)` the result under a wrong order; both come from the
restatements (tests/losses_np.py, tests/optimizer_np.py) alone.  Shared by tests/test_sum_orders_host.py (which proves the
separation) and tests/test_sum_orders_gpu.py (which asks the GPU for the header's bytes)."""
import functools

import numpy as np

import losses_np as ln
import optimizer_np as onp

F32, F64 = np.float32, np.float64
CH = onp.CH

# the sums of the header and the wrong orders at least one data set of each must separate
TABLE = {
    'rpn reg': ['rows reversed', 'tree over rows', 'float32 accumulator', 'flat sum of the 4n terms', 'coordinates reversed'],
    'rpn ce': ['rows reversed', 'tree over rows', 'float32 accumulator', 'mean in float64 before the rounding'],
    'roi classes C=21': ['classes reversed', 'tree over classes', 'float32 accumulator'],
    'roi classes C=81': ['classes reversed', 'tree over classes', 'float32 accumulator'],
    'roi columns C=21': ['ascending columns', 'partials in descending l', 'tree over the partials', 'float32 accumulator'],
    'roi columns C=81': ['ascending columns', 'partials in descending l', 'tree over the partials', 'float32 accumulator'],
    'roi rows': ['rows reversed', 'tree over rows', 'float32 accumulator', 'target-row order'],
    'l2 tensor': ['lane squares reversed', 'lanes sequential', 'chunks sequential', 'float32 accumulator',
                  'lane of element j is j % 256', 'lane of element j is j / 16'],
    'l2 add_n': ['tensors reversed', 'float64 accumulator'],
}


# ---- the wrong orders: each mirrors ordered_sum / roi_row_sum / l2_sum / add_n with the one change it is named after ----------
def sum_reversed(x, axis=-1):
    return ln.ordered_sum(np.flip(np.asarray(x), axis), axis)


def sum_tree(x, axis=-1):
    """pairwise: neighbours first, then neighbours of the pair sums, ... (zeros pad to a power of two)"""
    x = np.moveaxis(np.asarray(x).astype(F64), axis, -1)
    n = 1
    while n < x.shape[-1]:
        n *= 2
    pad = np.zeros(x.shape[:-1] + (n,), F64)
    pad[..., :x.shape[-1]] = x
    while pad.shape[-1] > 1:
        pad = pad[..., 0::2] + pad[..., 1::2]
    return pad[..., 0]


def sum_f32(x, axis=-1):
    """sequential in ascending order, the accumulator a float32"""
    x = np.asarray(x).astype(F32)
    if x.shape[axis] == 0:
        return np.zeros(np.delete(x.shape, axis), F32)
    return np.take(np.cumsum(x, axis=axis, dtype=F32), -1, axis=axis)


def _partials(terms, dtype=F64):
    r, w = terms.shape
    pad = np.zeros((r, -(-w // 64) * 64), dtype)
    pad[:, :w] = terms
    return pad.reshape(r, -1, 64)


def columns_ascending(terms, axis=1):
    return ln.ordered_sum(terms, axis=1)


def columns_partials_descending(terms, axis=1):
    return sum_reversed(ln.ordered_sum(_partials(terms), axis=1), axis=1)


def columns_partials_tree(terms, axis=1):
    return sum_tree(ln.ordered_sum(_partials(terms), axis=1), axis=1)


def columns_f32(terms, axis=1):
    return sum_f32(sum_f32(_partials(terms, F32), axis=1), axis=1)


def _fold(v):
    n = v.shape[-1]
    while n > 1:
        v = v[..., :n // 2] + v[..., n // 2:n]
        n //= 2
    return v[..., 0]


def l2_sum_mirror(w, lane_map='j/4 % 256', squares_reversed=False, lanes_sequential=False, chunks_sequential=False, acc=F64):
    """optimizer_np.l2_sum with one step replaced"""
    w = np.ascontiguousarray(w, dtype=F32).reshape(-1)
    nc = -(-w.size // CH)
    sq = np.zeros(nc * CH, F32)
    sq[:w.size] = w * w
    if lane_map == 'j/4 % 256':
        lanes = sq.reshape(nc, 4, 256, 4).transpose(0, 2, 1, 3).reshape(nc, 256, 16)
    elif lane_map == 'j % 256':
        lanes = sq.reshape(nc, 16, 256).transpose(0, 2, 1)
    else:
        assert lane_map == 'j / 16'
        lanes = sq.reshape(nc, 256, 16)
    lanes = lanes.astype(acc)
    if squares_reversed:
        lanes = lanes[:, :, ::-1]
    lane_sum = np.cumsum(lanes, axis=2, dtype=acc)[:, :, -1].reshape(nc, 4, 64)
    waves = np.cumsum(lane_sum, axis=2, dtype=acc)[:, :, -1] if lanes_sequential else _fold(lane_sum)
    chunk = np.cumsum(waves, axis=1, dtype=acc)[:, -1]
    if chunks_sequential:
        return F64(np.cumsum(chunk, dtype=acc)[-1])
    p = np.zeros(-(-nc // 64) * 64, acc)
    p[:nc] = chunk
    return F64(_fold(np.cumsum(p.reshape(-1, 64), axis=0, dtype=acc)[-1]))


L2_WRONG = {
    'lane squares reversed': dict(squares_reversed=True),
    'lanes sequential': dict(lanes_sequential=True),
    'chunks sequential': dict(chunks_sequential=True),
    'float32 accumulator': dict(acc=F32),
    'lane of element j is j % 256': dict(lane_map='j % 256'),
    'lane of element j is j / 16': dict(lane_map='j / 16'),
}


def add_n_reversed(losses):
    return onp.add_n(list(losses)[::-1])


def add_n_f64(losses):
    return F32(ln.ordered_sum(np.asarray(losses, F32)))


# the losses' wrong orders as replacements of the restatement's sums by role (losses_np._header_sums)
LOSS_WRONG = {
    ('rpn reg', 'rows reversed'): dict(rows_reg=sum_reversed),
    ('rpn reg', 'tree over rows'): dict(rows_reg=sum_tree),
    ('rpn reg', 'float32 accumulator'): dict(rows_reg=sum_f32, coords=sum_f32),
    ('rpn reg', 'flat sum of the 4n terms'): dict(coords=lambda t, axis: np.asarray(t), rows_reg=lambda t: ln.ordered_sum(t.reshape(-1))),
    ('rpn reg', 'coordinates reversed'): dict(coords=sum_reversed),
    ('rpn ce', 'rows reversed'): dict(rows_ce=sum_reversed),
    ('rpn ce', 'tree over rows'): dict(rows_ce=sum_tree),
    ('rpn ce', 'float32 accumulator'): dict(rows_ce=sum_f32),
    ('roi classes', 'classes reversed'): dict(classes=sum_reversed),
    ('roi classes', 'tree over classes'): dict(classes=sum_tree),
    ('roi classes', 'float32 accumulator'): dict(classes=sum_f32),
    ('roi columns', 'ascending columns'): dict(columns=columns_ascending),
    ('roi columns', 'partials in descending l'): dict(columns=columns_partials_descending),
    ('roi columns', 'tree over the partials'): dict(columns=columns_partials_tree),
    ('roi columns', 'float32 accumulator'): dict(columns=columns_f32),
    ('roi rows', 'rows reversed'): dict(rows_ce=sum_reversed, rows_reg=sum_reversed),
    ('roi rows', 'tree over rows'): dict(rows_ce=sum_tree, rows_reg=sum_tree),
    ('roi rows', 'float32 accumulator'): dict(rows_ce=sum_f32, rows_reg=sum_f32),
}


def rpn_mean_in_float64(res):
    """cls = float32(sum / n) instead of float32(sum) / float32(n)"""
    losses = res['losses'].copy()
    losses[0] = F32(ln.ordered_sum(res['ce_rows']) / F64(max(res['n'], 1)))
    return losses


def roi_target_row_order(res):
    """the row terms added in the order of their TARGET rows instead of their head rows"""
    order = np.argsort(res['target_row'], kind='stable')
    nf = F32(max(res['rows'], 1))
    return np.array([F32(ln.ordered_sum(res['ce_rows'][order])) / nf, F32(ln.ordered_sum(res['reg_rows'][order])) / nf], F32)


# ---- construction A -------------------------------------------------------------------------------------------------------
def _same_bits_in_any_libm(v64):
    """v64 (float64, positive) lies at least 1000 float64 units from the nearest float32 rounding boundary"""
    v64 = F64(v64)
    f = F32(v64)
    lo = (F64(f) + F64(np.nextafter(f, F32(-np.inf)))) / 2
    hi = (F64(f) + F64(np.nextafter(f, F32(np.inf)))) / 2
    return min(v64 - lo, hi - v64) >= 1000 * np.spacing(v64)


# RPN (sigma 3, n = 8, outside = 1/8 exact): |d| of the linear branch; 512 - 0.5/9 stays just under half a float64 unit of BIG
RPN_SIGMA, RPN_N = 3.0, 8
D_BIG, D_TIE, D_SMALL, D_NORMAL = 2.0 ** 62, 2.0 ** 38, 512.0, 2.0 ** 22
# cross-entropy terms and RoI smooth-L1 terms (sigma 1, outside an input: |d| = 2^k, k >= 25, scaled by outside = 2^-j)
BIG, TIE, SMALL, NORMAL = 2.0 ** 60, 2.0 ** 36, 2.0 ** 7, 2.0 ** 20
ROI_SIGMA = 1.0


def _rpn_image(ce_terms, reg_rows, kfg, N=32, S=16):
    """one image whose row r has the CE term ce_terms[r] (0: both logits equal, CE = log 2) and, for r < kfg, the smooth-L1
    differences reg_rows[r] (targets 0).  n = len(ce_terms)."""
    n = len(ce_terms)
    assert kfg <= n <= S and len(reg_rows) == kfg
    idx = -np.ones(S, np.int32)
    idx[:n] = (5 * np.arange(n) + 3) % N                             # distinct, not ascending
    scores = np.zeros((N, 2), F32)
    deltas = np.zeros((N, 4), F32)
    for r in range(n):
        label = 1 if r < kfg else 0
        scores[idx[r], label] = -F32(ce_terms[r])
        if r < kfg:
            deltas[idx[r]] = np.asarray(reg_rows[r], F32)
    counts = np.array([N, kfg, n - kfg, kfg, n - kfg], np.int32)
    return dict(kind='rpn', scores=scores.reshape(-1), deltas=deltas, sample_idx=idx, sample_targets=np.zeros((S, 4), F32),
                counts=counts, sigma=RPN_SIGMA, layout=ln.LAYOUT_FPN, A=1, N=N)


def _rpn_reg(name, rows, wrong):
    n = RPN_N
    rows = [list(r) for r in rows] + [[0, 0, 0, 0]] * (n - len(rows))
    ds = _rpn_image([0.0] * n, rows, n)
    ds.update(sum='rpn reg', name=name, wrong=wrong, watch=('losses',))
    return ds


def _rpn_ce(name, terms, wrong, kfg=4):
    ds = _rpn_image(list(terms), [[0, 0, 0, 0]] * kfg, kfg)
    ds.update(sum='rpn ce', name=name, wrong=wrong, watch=('losses',))
    return ds


def rpn_sets():
    z = [0, 0, 0, 0]
    out = [
        _rpn_reg('tie row, then four small rows', [[D_BIG, D_TIE, 0, 0]] + [[D_SMALL, 0, 0, 0]] * 4,
                 ['rows reversed', 'tree over rows']),
        _rpn_reg('big, tie, normal rows', [[D_BIG, 0, 0, 0], [D_TIE, 0, 0, 0], [D_NORMAL, 0, 0, 0]], ['float32 accumulator']),
        _rpn_reg('tie row, then a row of four smalls', [[D_BIG, D_TIE, 0, 0], [D_SMALL] * 4], ['flat sum of the 4n terms']),
        _rpn_reg('big, small, small, tie in one row', [[D_BIG, D_SMALL, D_SMALL, D_TIE], z], ['coordinates reversed']),
        _rpn_ce('big, tie, six smalls', [BIG, TIE] + [SMALL] * 6, ['rows reversed', 'tree over rows']),
        _rpn_ce('big, tie, six normals', [BIG, TIE] + [NORMAL] * 6, ['float32 accumulator']),
        # n = 3: float32(2^24 + 5) = 2^24 + 4, a third of which is 5592406.67 -> 5592406.5; (2^24 + 5) / 3 is 5592407 exactly
        _rpn_ce('n = 3', MEAN_TERMS, ['mean in float64 before the rounding'], kfg=1),
    ]
    return out


MEAN_TERMS = [2.0 ** 24 - 300, 150.0, 155.0]


# ---- RoI --------------------------------------------------------------------------------------------------------------------
def _roi_image(C, R, S, rows, scores, deltas, labels, cols, row_map=None):
    """cols: [(target row, column, |d|, outside)] -> targets 0, inside 1 and `outside` there, everything else 0"""
    W = 4 * C
    targets, inside, outside = np.zeros((S, W), F32), np.zeros((S, W), F32), np.zeros((S, W), F32)
    for m, c, d, o in cols:
        inside[m, c], outside[m, c] = 1, o
    return dict(kind='roi', scores=np.asarray(scores, F32).reshape(R, C), deltas=np.asarray(deltas, F32).reshape(R, W),
                labels=np.asarray(labels, np.int32), targets=targets, inside=inside, outside=outside,
                counts=np.array([rows, 0, 0, rows], np.int32), sigma=ROI_SIGMA,
                row_map=None if row_map is None else np.asarray(row_map, np.int32), upstream=None)


# a smooth-L1 term of the linear branch at sigma 1: (|d|, outside) with |d| = 2^k, k >= 25
_TERM = {BIG: (2.0 ** 60, 1.0), TIE: (2.0 ** 36, 1.0), SMALL: (2.0 ** 25, 2.0 ** -18), NORMAL: (2.0 ** 25, 2.0 ** -5)}


@functools.lru_cache(None)
def softmax_tie():
    """(z1, z_small, z_normal) of construction B"""
    z = np.linspace(-0.6, -0.1, 200001).astype(F32)
    e64 = np.exp(z.astype(F64))
    e = e64.astype(F32)
    k = np.round(e.astype(F64) * 2.0 ** 24).astype(np.int64)
    tie = (k % 2 == 1) & (e >= 0.5) & (e < 1)
    s = 1.0 + e.astype(F64)                                          # exact
    down, up = s.astype(F32), np.nextafter(s.astype(F32), F32(2))
    tie &= down.astype(F64) < s                                      # the even neighbour is the one below
    z_small, z_normal = F32(-37.6), F32(-21.0)
    assert np.exp(F64(z_small)) < 2.0 ** -53 and 4 * np.exp(F64(z_small)) > 2.0 ** -53
    assert _same_bits_in_any_libm(np.exp(F64(z_small))) and _same_bits_in_any_libm(np.exp(F64(z_normal)))
    for i in np.nonzero(tie)[0]:
        if not (_same_bits_in_any_libm(e64[i]) and _same_bits_in_any_libm(np.log(F64(down[i])))
                and _same_bits_in_any_libm(np.log(F64(up[i])))):
            continue
        p_down, p_up = np.array([1, e[i]], F32) / down[i], np.array([1, e[i]], F32) / up[i]
        if np.all(p_down != p_up):                                   # the order shows in both gradients too
            return z[i], z_small, z_normal
    raise AssertionError('no z1 found')


def _roi_classes(C, name, row, wrong):
    ds = _roi_image(C, 1, 1, 1, row, np.zeros(4 * C), [0], [])
    ds.update(sum='roi classes C=%d' % C, name='C=%d %s' % (C, name), wrong=wrong, watch=('losses', 'grad_scores'))
    return ds


def _roi_columns(C, name, cols, wrong):
    deltas = np.zeros(4 * C, F32)
    spec = []
    for c, term in cols:
        d, o = _TERM[term]
        deltas[c] = d
        spec.append((0, c, d, o))
    ds = _roi_image(C, 1, 1, 1, np.zeros(C), deltas, [0], spec)
    ds.update(sum='roi columns C=%d' % C, name='C=%d %s' % (C, name), wrong=wrong, watch=('losses',))
    return ds


def _roi_rows(name, terms, wrong, row_map=None, C=21):
    """head row r: CE term terms[r] and a smooth-L1 row sum of terms[r] (one column)"""
    R = S = len(terms)
    m = np.arange(R) if row_map is None else np.asarray(row_map)
    labels = np.zeros(S, np.int32)
    labels[m] = 1 + np.arange(R) % 5
    scores = np.full((R, C), -200, F32)
    scores[:, 0] = 0                                                 # s = 1 exactly: CE = -z_label
    deltas = np.zeros((R, 4 * C), F32)
    spec = []
    for r, term in enumerate(terms):
        scores[r, labels[m[r]]] = -F32(term)
        d, o = _TERM[term]
        c = 4 * labels[m[r]] + r % 4
        deltas[r, c] = d
        spec.append((m[r], c, d, o))
    ds = _roi_image(C, R, S, S, scores, deltas, labels, spec, row_map)
    ds.update(sum='roi rows', name=name, wrong=wrong, watch=('losses',))
    return ds


def roi_sets():
    z1, zs, zn = softmax_tie()
    out = []
    for C in (21, 81):
        row = np.full(C, zs, F32)
        row[0], row[1] = 0, z1
        out.append(_roi_classes(C, 'tie partner in column 1', row, ['classes reversed', 'tree over classes']))
        f = row.copy()
        f[2] = zn
        out.append(_roi_classes(C, 'tie partner in column 1, a normal term in column 2', f, ['float32 accumulator']))
        if C > 64:                                                   # either side of the wave's second trip over the classes
            late = np.full(C, zs, F32)
            late[0], late[70] = 0, z1
            out.append(_roi_classes(C, 'tie partner in column 70', late, ['classes reversed', 'tree over classes']))
            f = row.copy()
            f[70] = zn
            out.append(_roi_classes(C, 'tie partner in column 1, a normal term in column 70', f, ['float32 accumulator']))
        far = 2 + 64 * ((4 * C - 3) // 64)                           # the last column of partial 2
        out.append(_roi_columns(C, 'two smalls in partial 2', [(0, BIG), (1, TIE), (2, SMALL), (far, SMALL)],
                                ['ascending columns']))
        out.append(_roi_columns(C, 'smalls in partials 2..5', [(0, BIG), (1, TIE)] + [(c, SMALL) for c in (2, 3, 4, 5)],
                                ['partials in descending l', 'tree over the partials']))
        out.append(_roi_columns(C, 'a normal term in partial 2', [(0, BIG), (1, TIE), (far, NORMAL)], ['float32 accumulator']))
    out.append(_roi_rows('big, tie, six small rows', [BIG, TIE] + [SMALL] * 6, ['rows reversed', 'tree over rows']))
    out.append(_roi_rows('big, tie, six normal rows', [BIG, TIE] + [NORMAL] * 6, ['float32 accumulator']))
    out.append(_roi_rows('the small rows have the first target rows', [BIG, TIE] + [SMALL] * 6, ['target-row order'],
                         row_map=[6, 7, 0, 1, 2, 3, 4, 5]))
    return out


# ---- L2 ---------------------------------------------------------------------------------------------------------------------
# squares: (2^30)^2 = BIG, (2^18)^2 = TIE; 11^2 = 121 is under half a float64 unit of BIG (128), two of them are over it;
# (2^10)^2 = NORMAL
W_BIG, W_TIE, W_SMALL, W_NORMAL = 2.0 ** 30, 2.0 ** 18, 11.0, 2.0 ** 10
L2_WD = 0.5


def _l2(name, numel, at, wrong):
    w = np.zeros(numel, F32)
    for j, v in at.items():
        w[j] = v
    return dict(kind='l2', sum='l2 tensor', name=name, wrong=wrong, watch=('tensor_loss',), w=w, wd=L2_WD)


def l2_sets():
    lane = lambda l, k=0, e=0: k * 1024 + 4 * l + e                  # element of lane l, group k, position e of a chunk
    return [
        _l2('small, small, tie, big in lane 0', 300, {0: W_SMALL, 1: W_SMALL, 2: W_TIE, 3: W_BIG},
            ['lane of element j is j % 256']),
        _l2('big, tie, small, small over the four groups of lane 5', 4096,
            {lane(5, 0, 1): W_BIG, lane(5, 1, 0): W_TIE, lane(5, 2, 3): W_SMALL, lane(5, 3, 2): W_SMALL}, ['lane squares reversed']),
        _l2('big and tie in lanes 0 and 32, smalls in lanes 16 and 48', 200,
            {lane(0): W_BIG, lane(32): W_TIE, lane(16): W_SMALL, lane(48): W_SMALL}, ['lanes sequential']),
        _l2('big and tie in lane 0, two smalls in lane 1', 300, {0: W_BIG, 1: W_TIE, 4: W_SMALL, 5: W_SMALL},
            ['lane of element j is j / 16']),
        _l2('big, tie, normal in lane 3', 65, {12: W_BIG, 13: W_TIE, 14: W_NORMAL}, ['float32 accumulator']),
        _l2('big and tie in chunks 0 and 32, smalls in chunks 1 and 65', 65 * CH + 9,
            {0: W_BIG, 32 * CH + 77: W_TIE, CH + 5: W_SMALL, 65 * CH + 8: W_SMALL}, ['chunks sequential']),
    ]


def l2_many_chunks():
    """more than 512 chunks: lane 1 of the finish takes chunk 513 on its second trip"""
    return _l2('chunks 0, 512 (tie), 1 and 513 (smalls)', 513 * CH + 5,
               {3: W_BIG, 512 * CH + 100: W_TIE, CH + 5: W_SMALL, 513 * CH + 4: W_SMALL}, ['chunks sequential'])


def add_n_sets():
    """per-tensor losses 2^24, 1, 1 (weight decay 1): left to right both 1s are lost on the tie"""
    tensors = [np.array([2.0 ** 12], F32), np.array([1.0], F32), np.array([0.0, 1.0, 0.0], F32)]
    return [dict(kind='add_n', sum='l2 add_n', name='2^24 + 1 + 1', wrong=['tensors reversed', 'float64 accumulator'],
                 watch=('total',), tensors=tensors, wds=[1.0, 1.0, 1.0])]


def add_n_many_tensors():
    """1100 tiny tensors, every third regularised (weight decay 1): losses 2^24, then 1s that are lost one at a time, and 3s
    past tensor 1024, each of which moves the total"""
    tensors, wds = [], []
    for t in range(1100):
        w = np.zeros(1 + t % 5, F32)
        w[t % w.size] = 2.0 ** 12 if t == 0 else (np.sqrt(F32(3.0)) if t >= 1024 else 1.0)
        tensors.append(w)
        wds.append(1.0 if t % 3 == 0 else 0.0)
    return dict(kind='add_n', sum='l2 add_n', name='1100 tensors', wrong=['tensors reversed', 'float64 accumulator'],
                watch=('total',), tensors=tensors, wds=wds)


def all_sets():
    return rpn_sets() + roi_sets() + l2_sets() + [l2_many_chunks()] + add_n_sets() + [add_n_many_tensors()]


# ---- expected outputs -----------------------------------------------------------------------------------------------------
def _loss_key(ds):
    return ' '.join(ds['sum'].split(' ')[:2])                        # 'roi classes C=21' -> 'roi classes'


def expected(ds, wrong=None):
    """the float32 outputs of the entry point on `ds` in the header's order, or with one sum in the order `wrong`"""
    if ds['kind'] == 'l2':
        s = onp.l2_sum(ds['w']) if wrong is None else l2_sum_mirror(ds['w'], **L2_WRONG[wrong])
        return dict(tensor_loss=np.array([F32(F32(ds['wd']) * F32(s))], F32))
    if ds['kind'] == 'add_n':
        per = np.array([onp.l2_loss(w, wd) for w, wd in zip(ds['tensors'], ds['wds'])], F32)
        total = {None: onp.add_n, 'tensors reversed': add_n_reversed, 'float64 accumulator': add_n_f64}[wrong](per)
        return dict(tensor_losses=per, total=np.array([total], F32))
    post = {'mean in float64 before the rounding': rpn_mean_in_float64, 'target-row order': roi_target_row_order}.get(wrong)
    sums = None if wrong is None or post else LOSS_WRONG[(_loss_key(ds), wrong)]
    if ds['kind'] == 'rpn':
        res = ln.rpn_loss(ds['scores'], ds['deltas'], ds['sample_idx'], ds['sample_targets'], ds['counts'], ds['sigma'],
                          ds['layout'], ds['A'], sums=sums)
        out = dict(losses=res['losses'], row_grad_scores=res['row_grad_scores'], row_grad_deltas=res['row_grad_deltas'])
    else:
        res = ln.roi_loss(ds['scores'], ds['deltas'], ds['labels'], ds['targets'], ds['inside'], ds['outside'], ds['counts'],
                          ds['sigma'], ds['row_map'], ds['upstream'], sums=sums)
        out = dict(losses=res['losses'], grad_scores=res['grad_scores'], grad_deltas=res['grad_deltas'])
    if post:
        out['losses'] = post(res)
    return out


def inputs_of(ds):
    """every input array of a data set (for the finiteness check)"""
    if ds['kind'] == 'l2':
        return [ds['w']]
    if ds['kind'] == 'add_n':
        return list(ds['tensors'])
    keys = ('scores', 'deltas', 'sample_targets') if ds['kind'] == 'rpn' else ('scores', 'deltas', 'targets', 'inside', 'outside')
    return [ds[k] for k in keys]
