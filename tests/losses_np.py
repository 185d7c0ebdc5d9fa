"""numpy restatement of the fused training losses (include/odet.h "training losses": odet_rpn_loss, odet_rpn_loss_backward,
odet_roi_loss), one image per call, in the arithmetic the header defines: float32 element operations in the order of the
reference's model/losses.py:16-28 and of a max-shifted softmax cross entropy (:12), exp / log rounded once from float64, and
every sum a float64 `cumsum` in the header's order, rounded to float32 once.  `*_f64` evaluate the same formulas and their
analytic gradients in float64 (the yardstick of the derived bounds).  The checker of tests/test_losses_host.py and
tests/test_losses_gpu.py; the product never imports it."""
import numpy as np

F32, F64 = np.float32, np.float64
LAYOUT_FPN, LAYOUT_FRCNN = 0, 1


def exp32(x):
    return np.exp(np.asarray(x, F32).astype(F64)).astype(F32)


def log32(x):
    return np.log(np.asarray(x, F32).astype(F64)).astype(F32)


def ordered_sum(x, axis=-1):
    """sequential float64 sum in ascending index order along `axis` (0 for an empty axis)"""
    x = np.asarray(x).astype(F64)
    if x.shape[axis] == 0:
        return np.zeros(np.delete(x.shape, axis), F64)
    return np.take(np.cumsum(x, axis=axis), -1, axis=axis)


def sl_const(sigma):
    """losses.py:17-22: sigma_2, 1/sigma_2, sigma_2/2, 0.5/sigma_2 as float32 operations"""
    s2 = F32(sigma) * F32(sigma)
    return s2, F32(1) / s2, s2 / F32(2), F32(0.5) / s2


def smooth_l1(pred, tgt, inside, outside, sigma):
    """losses.py:18-23 per element -> (loss terms, gradient outside * inside * (sigma_2 * d | sign(d)), sign mask)"""
    s2, thr, half_s2, half_inv = sl_const(sigma)
    pred, tgt, inside, outside = (np.asarray(v, F32) for v in (pred, tgt, inside, outside))
    d = inside * (pred - tgt)
    ad = np.abs(d)
    sign = (ad < thr).astype(F32)
    in_loss = d * d * half_s2 * sign + (ad - half_inv) * (F32(1) - sign)
    slope = np.where(sign != 0, s2 * d, np.where(d > 0, F32(1), F32(-1))).astype(F32)
    return outside * in_loss, outside * inside * slope, sign


def softmax_rows(x, label, class_sum=ordered_sum):
    """x float32 [n,C], label int [n] -> (CE [n], p [n,C], z_label [n]) with s summed over the classes in ascending order"""
    x = np.asarray(x, F32)
    n = x.shape[0]
    if n == 0:
        return np.zeros(0, F32), np.zeros(x.shape, F32), np.zeros(0, F32)
    with np.errstate(over='ignore'):                                 # (logits of +-3e38: the gap is -inf, e is 0)
        z = x - x.max(axis=1, keepdims=True)
    e = exp32(z)
    sf = np.asarray(class_sum(e, axis=1)).astype(F32)
    zl = z[np.arange(n), label]
    return log32(sf) - zl, e / sf[:, None], zl


# the sums of a loss by role, in the header's orders.  tests/order_data.py swaps one for a wrong order to prove that its data
# tells the two apart; nothing else passes `sums`.
def _header_sums(sums):
    out = dict(classes=ordered_sum, coords=ordered_sum, columns=roi_row_sum, rows_ce=ordered_sum, rows_reg=ordered_sum)
    out.update(sums or {})
    return out


def fpn_view(scores, layout, A):
    """the [N,2] (bg, fg) rows of one image's scores in either layout (base_faster_rcnn_model.py:203)"""
    scores = np.asarray(scores)
    if layout == LAYOUT_FPN:
        return scores.reshape(-1, 2)
    return scores.reshape(-1, 2, A).transpose(0, 2, 1).reshape(-1, 2)


def from_fpn_view(rows, layout, A):
    """the inverse re-layout, flat"""
    if layout == LAYOUT_FPN:
        return rows.reshape(-1)
    return rows.reshape(-1, A, 2).transpose(0, 2, 1).reshape(-1)


def rpn_loss(scores, deltas, sample_idx, sample_targets, counts, sigma, layout=LAYOUT_FPN, A=1, sums=None):
    """one image of odet_rpn_loss -> dict(losses [2], row_grad_scores [S,2], row_grad_deltas [S,4], z_label, sign, and the
    terms of the sums: ce_rows [n] float32, reg_terms [n,4] float32).  The header's clamps: a negative count empties the
    image, kfg = min(kfg, S), n = min(kfg + kbg, S); a row r < n whose index lies outside 0..N-1 adds nothing and has zero row
    gradients, but counts in n."""
    sm = _header_sums(sums)
    x = fpn_view(np.asarray(scores, F32), layout, A)
    deltas = np.asarray(deltas, F32).reshape(-1, 4)
    N, S = deltas.shape[0], len(sample_idx)
    kfg, kbg = int(counts[3]), int(counts[4])
    if kfg < 0 or kbg < 0:
        kfg = kbg = 0
    kfg = min(kfg, S)
    n = min(kfg + kbg, S)
    nf = F32(max(n, 1))
    row_gs, row_gd = np.zeros((S, 2), F32), np.zeros((S, 4), F32)
    idx = np.asarray(sample_idx[:n], np.int64)
    v = np.nonzero((idx >= 0) & (idx < N))[0]                        # the rows that take part
    label = (v < kfg).astype(np.int64)
    ce, p, zl = softmax_rows(x[idx[v]], label, sm['classes'])
    onehot = np.zeros((len(v), 2), F32)
    onehot[np.arange(len(v)), label] = 1
    row_gs[v] = (p - onehot) / nf
    outside = F32(1) / nf
    f = v[v < kfg]
    terms, grad, sign = smooth_l1(deltas[idx[f]], np.asarray(sample_targets, F32).reshape(-1, 4)[f], F32(1), outside, sigma)
    row_gd[f] = grad
    ce_rows, reg_terms = np.zeros(n, F32), np.zeros((n, 4), F32)
    ce_rows[v] = ce
    reg_terms[f] = terms
    cls = F32(sm['rows_ce'](ce_rows)) / nf
    reg = F32(sm['rows_reg'](sm['coords'](reg_terms, axis=1)))       # the 4 coordinates of a row, then the rows
    return dict(losses=np.array([cls, reg], F32), row_grad_scores=row_gs, row_grad_deltas=row_gd, z_label=zl, sign=sign,
                ce_rows=ce_rows, reg_terms=reg_terms, n=n)


def rpn_loss_backward(sample_idx, row_grad_scores, row_grad_deltas, upstream, N, layout=LAYOUT_FPN, A=1):
    """one image of odet_rpn_loss_backward -> (grad_scores flat [2N] in `layout`, grad_deltas [N,4]): every one of the S rows
    whose index lies in 0..N-1 is written (a row >= n with upstream * 0, which is -0 under a negative upstream), an index
    outside is skipped"""
    rows, gd = np.zeros((N, 2), F32), np.zeros((N, 4), F32)
    k = (np.asarray(sample_idx) >= 0) & (np.asarray(sample_idx) < N)
    idx = np.asarray(sample_idx)[k]
    rows[idx] = F32(upstream[0]) * np.asarray(row_grad_scores, F32)[k]
    gd[idx] = F32(upstream[1]) * np.asarray(row_grad_deltas, F32)[k]
    return from_fpn_view(rows, layout, A), gd


def roi_row_sum(terms, axis=1):
    """the 4C columns of every row as 64 partial sums (partial l: columns l, l + 64, ... ascending), added in ascending l"""
    assert axis == 1
    r, w = terms.shape
    pad = np.zeros((r, -(-w // 64) * 64), F64)
    pad[:, :w] = terms
    return ordered_sum(ordered_sum(pad.reshape(r, -1, 64), axis=1), axis=1)


def _roi_rows(R, labels, counts, row_map, C):
    rows = min(max(int(counts[3]), 0), len(labels))
    m = np.arange(R) if row_map is None else np.asarray(row_map, np.int64)
    ok = (m >= 0) & (m < rows)
    lab = np.where(ok, np.asarray(labels, np.int64)[np.where(ok, m, 0)], -1)
    ok = ok & (lab >= 0) & (lab < C)
    return rows, m, ok, lab


def roi_loss(scores, deltas, labels, targets, inside, outside, counts, sigma, row_map=None, upstream=None, sums=None):
    """one image of odet_roi_loss -> dict(losses [2], grad_scores [R,C], grad_deltas [R,4C], z_label, sign, and the terms of
    the row sums: ce_rows [R] float32, reg_rows [R] float64, target_row [R]).  rows = min(max(counts[3], 0), S)."""
    sm = _header_sums(sums)
    scores, deltas = np.asarray(scores, F32), np.asarray(deltas, F32)
    R, C = scores.shape
    rows, m, ok, lab = _roi_rows(R, labels, counts, row_map, C)
    nf = F32(max(rows, 1))
    up = (F32(1), F32(1)) if upstream is None else (F32(upstream[0]), F32(upstream[1]))
    v = np.nonzero(ok)[0]
    ce_all, reg_all = np.zeros(R, F32), np.zeros(R, F64)
    gs, gd = np.zeros((R, C), F32), np.zeros((R, 4 * C), F32)
    ce, p, zl = softmax_rows(scores[v], lab[v], sm['classes'])
    onehot = np.zeros((len(v), C), F32)
    onehot[np.arange(len(v)), lab[v]] = 1
    gs[v] = up[0] * ((p - onehot) / nf)
    mv = m[v]
    terms, grad, sign = smooth_l1(deltas[v], np.asarray(targets, F32)[mv], np.asarray(inside, F32)[mv],
                                  np.asarray(outside, F32)[mv], sigma)
    gd[v] = up[1] * (grad / nf)
    ce_all[v] = ce
    if len(v):
        reg_all[v] = sm['columns'](terms, axis=1)
    cls = F32(sm['rows_ce'](ce_all)) / nf
    reg = F32(sm['rows_reg'](reg_all)) / nf
    return dict(losses=np.array([cls, reg], F32), grad_scores=gs, grad_deltas=gd, z_label=zl, sign=sign,
                active=np.asarray(inside, F32)[mv] != 0, ce_rows=ce_all, reg_rows=reg_all, target_row=np.where(ok, m, -1),
                rows=rows)


# ---- the same formulas in float64 ----------------------------------------------------------------------------------------
def _softmax_f64(x, label):
    x = np.asarray(x, F64)
    z = x - x.max(axis=1, keepdims=True)
    e = np.exp(z)
    s = e.sum(axis=1)
    n = x.shape[0]
    onehot = np.zeros(x.shape, F64)
    onehot[np.arange(n), label] = 1
    return np.log(s) - z[np.arange(n), label], e / s[:, None] - onehot


def _smooth_l1_f64(pred, tgt, inside, outside, sigma):
    s2 = F64(sigma) ** 2
    inside, outside = np.asarray(inside, F64), np.asarray(outside, F64)
    d = inside * (np.asarray(pred, F64) - np.asarray(tgt, F64))
    ad = np.abs(d)
    quad = ad < 1.0 / s2
    loss = np.where(quad, d * d * (s2 / 2.0), ad - 0.5 / s2)
    return outside * loss, outside * inside * np.where(quad, s2 * d, np.sign(d))


def rpn_loss_f64(scores, deltas, sample_idx, sample_targets, counts, sigma, layout=LAYOUT_FPN, A=1):
    x = fpn_view(np.asarray(scores, F64), layout, A)
    deltas = np.asarray(deltas, F64).reshape(-1, 4)
    S = len(sample_idx)
    kfg, kbg = max(int(counts[3]), 0), max(int(counts[4]), 0)
    n = kfg + kbg
    row_gs, row_gd = np.zeros((S, 2)), np.zeros((S, 4))
    if n == 0:
        return dict(losses=np.zeros(2), row_grad_scores=row_gs, row_grad_deltas=row_gd)
    idx = np.asarray(sample_idx[:n], np.int64)
    ce, g = _softmax_f64(x[idx], (np.arange(n) < kfg).astype(np.int64))
    row_gs[:n] = g / n
    terms, grad = _smooth_l1_f64(deltas[idx[:kfg]], np.asarray(sample_targets, F64)[:kfg], 1.0, 1.0 / n, sigma)
    row_gd[:kfg] = grad
    return dict(losses=np.array([ce.sum() / n, terms.sum()]), row_grad_scores=row_gs, row_grad_deltas=row_gd)


def roi_loss_f64(scores, deltas, labels, targets, inside, outside, counts, sigma, row_map=None, upstream=None):
    scores, deltas = np.asarray(scores, F64), np.asarray(deltas, F64)
    R, C = scores.shape
    rows, m, ok, lab = _roi_rows(R, labels, counts, row_map, C)
    up = (1.0, 1.0) if upstream is None else (F64(upstream[0]), F64(upstream[1]))
    gs, gd = np.zeros((R, C)), np.zeros((R, 4 * C))
    v = np.nonzero(ok)[0]
    if len(v) == 0:
        return dict(losses=np.zeros(2), grad_scores=gs, grad_deltas=gd)
    ce, g = _softmax_f64(scores[v], lab[v])
    gs[v] = up[0] * g / rows
    mv = m[v]
    terms, grad = _smooth_l1_f64(deltas[v], np.asarray(targets)[mv], np.asarray(inside)[mv], np.asarray(outside)[mv], sigma)
    gd[v] = up[1] * grad / rows
    return dict(losses=np.array([ce.sum() / rows, terms.sum() / rows]), grad_scores=gs, grad_deltas=gd)


# ---- the issue's bounds against the float64 value ------------------------------------------------------------------------
def ce_loss_bound(C, z_label):
    zmax = float(np.abs(z_label).max()) if len(z_label) else 0.0
    return 2.0 ** -22 * (1.0 + 2.0 * np.log(C) + zmax)


def check_bounds(got, want, n, C, z_label, names, report=None, upstream=(1.0, 1.0)):
    """got / want: dicts of float32 results and float64 values; names = (losses, score gradient, delta gradient) keys.
    Asserts the four bounds (the absolute gradient bounds scale with the upstream gradient the results were taken at) and
    returns the observed maxima as fractions of their bounds."""
    n = max(int(n), 1)
    u_cls, u_reg = max(abs(float(upstream[0])), 1e-300), max(abs(float(upstream[1])), 1e-300)
    gl, wl = np.asarray(got[names[0]], F64), np.asarray(want[names[0]], F64)
    out = {}
    out['ce'] = abs(gl[0] - wl[0]) / ce_loss_bound(C, z_label)
    out['sl1'] = abs(gl[1] - wl[1]) / (2.0 ** -21 * wl[1]) if wl[1] != 0 else (0.0 if gl[1] == 0 else np.inf)
    gs, ws = np.asarray(got[names[1]], F64), np.asarray(want[names[1]], F64)
    out['ce_grad'] = float(np.abs(gs - ws).max() / (2.0 ** -20 / n * u_cls)) if gs.size else 0.0
    gd, wd = np.asarray(got[names[2]], F64), np.asarray(want[names[2]], F64)
    bound = np.where(wd != 0, 2.0 ** -21 * np.abs(wd), 2.0 ** -21 / n * u_reg)
    out['sl1_grad'] = float((np.abs(gd - wd) / bound).max()) if gd.size else 0.0
    if report is not None:
        print('%s: error / bound  CE loss %.3f  smooth-L1 loss %.3f  CE gradient %.3f  smooth-L1 gradient %.3f'
              % (report, out['ce'], out['sl1'], out['ce_grad'], out['sl1_grad']))
    for k, v in out.items():
        assert v <= 1.0, (report, k, v)
    return out
