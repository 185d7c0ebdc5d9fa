"""The statement of the FPN neck's backward (csrc/neck.hip odet_fpn_topdown_backward_f32, model/neck_trainable.py).

`topdown_backward` is the float32 statement of the kernel, bit for bit: the SERIAL loop over the fine pixels in ascending (y, x)
that accumulates the four taps TL, TR, BL, BR of each into the coarse map -- every product and every sum rounded to float32, the
accumulator starting at +0 -- then base + sub + S left to right (absent terms skipped) and one multiply by out_scale.  The
coordinates are the forward's own float32 expressions (oracle_np.tf_resize_bilinear_legacy).  No tap is skipped here: the
kernel may skip taps of weight zero because that leaves finite data's bits alone.

`neck_forward` / `neck_backward` are the whole neck in float64 (NHWC maps, 1x1 weights [cout,cin], 3x3 weights [cout,3,3,cin]),
with the resize's weights taken from the same float32 coordinates."""
import numpy as np

import conv_grad_np as cg

F32 = np.float32
LAYERS = ('p5', 'l4', 'l3', 'l2', 's4', 's3', 's2')
# (h, w) -> (H, W): the shapes the host and the GPU tests share.  (1,1)->(2,3): every tap clamped onto one pixel; (3,5)->(6,10) exact
# 2x; (5,4)->(5,4) scale 1; (6,5)->(3,4) a downscale whose odd coarse rows only taps of weight zero reach; (7,5)->(2,4) a downscale
# with coarse rows and columns NO tap reaches; (2,84)->(3,167) the full-size pyramid's non-dyadic ratio
CASES = [((1, 1), (1, 1)), ((1, 1), (2, 3)), ((2, 3), (3, 5)), ((3, 5), (6, 10)), ((4, 6), (7, 11)), ((5, 4), (5, 4)),
         ((6, 5), (3, 4)), ((2, 42), (3, 84)), ((2, 84), (3, 167)), ((7, 5), (2, 4))]


def axis_taps(n_in, n_out):
    """per output index: (lo, hi, lerp) of the TF1 legacy resize along one axis, in float32"""
    s = F32(n_in) / F32(n_out)
    f = (np.arange(n_out, dtype=np.float32) * s).astype(np.float32)
    lo = np.floor(f).astype(np.int64)
    hi = np.minimum(lo + 1, n_in - 1)
    return lo, hi, (f - lo.astype(np.float32)).astype(np.float32)


def tap_counts(top_hw, fine_hw):
    """[h,w] number of taps (of any weight) that land on each coarse pixel"""
    h, w = top_hw
    y0, y1, _ = axis_taps(h, fine_hw[0])
    x0, x1, _ = axis_taps(w, fine_hw[1])
    ny, nx = np.zeros(h, np.int64), np.zeros(w, np.int64)
    np.add.at(ny, y0, 1), np.add.at(ny, y1, 1), np.add.at(nx, x0, 1), np.add.at(nx, x1, 1)
    return ny[:, None] * nx[None, :]


def tap_sum(fine, top_hw):
    """S [B,h,w,C] float32: the serial loop"""
    h, w = int(top_hw[0]), int(top_hw[1])
    fine = np.asarray(fine, dtype=np.float32)
    B, H, W, C = fine.shape
    y0, y1, yl = axis_taps(h, H)
    x0, x1, xl = axis_taps(w, W)
    S = np.zeros((B, h, w, C), np.float32)                      # +0
    one = F32(1)
    for y in range(H):
        wt, wb = one - yl[y], yl[y]
        for x in range(W):
            wl, wr = one - xl[x], xl[x]
            g = fine[:, y, x, :]
            gt, gb = (g * wt).astype(np.float32), (g * wb).astype(np.float32)
            for yy, xx, v in ((y0[y], x0[x], gt * wl), (y0[y], x1[x], gt * wr), (y1[y], x0[x], gb * wl), (y1[y], x1[x], gb * wr)):
                S[:, yy, xx, :] = (S[:, yy, xx, :] + v.astype(np.float32)).astype(np.float32)
    return S


def topdown_backward(fine, top_hw, base=None, sub=None, out_scale=1.0, S=None):
    """d_top [B,h,w,C] float32 (module docstring); fine [B,H,W,C] / base [B,h,w,C] / sub [B,ceil(h/2),ceil(w/2),C] or None; `S`: a
    tap_sum(fine, top_hw) the caller already has"""
    h, w = int(top_hw[0]), int(top_hw[1])
    first = next(t for t in (fine, base, sub) if t is not None)
    B, C = first.shape[0], first.shape[3]
    t, have = None, np.zeros((h, w), bool)
    if base is not None:
        t, have = np.array(base, dtype=np.float32), np.ones((h, w), bool)
    if sub is not None:
        sub = np.asarray(sub, dtype=np.float32)
        if t is None:
            t = np.zeros((B, h, w, C), np.float32)
            t[:, ::2, ::2] = sub
        else:
            t[:, ::2, ::2] = (t[:, ::2, ::2] + sub).astype(np.float32)
        have[::2, ::2] = True
    if fine is not None:
        S = tap_sum(fine, top_hw) if S is None else S
        if t is None:
            t = S
        else:
            t = np.where(have[None, :, :, None], (t + S).astype(np.float32), S)
    return (F32(out_scale) * t).astype(np.float32)


# ---- the whole neck, float64 ----------------------------------------------------------------------------------------------
def resize(x, out_hw):
    """the TF1 legacy resize in float64 with the float32 coordinates: [B,h,w,C] -> [B,H,W,C]"""
    x = np.asarray(x, np.float64)
    y0, y1, yl = axis_taps(x.shape[1], out_hw[0])
    x0, x1, xl = axis_taps(x.shape[2], out_hw[1])
    yl, xl = yl.astype(np.float64)[None, :, None, None], xl.astype(np.float64)[None, None, :, None]
    rows = x[:, y0] * (1 - yl) + x[:, y1] * yl
    return rows[:, :, x0] * (1 - xl) + rows[:, :, x1] * xl


def resize_t(g, top_hw, absolute=False):
    """the transpose of `resize`: [B,H,W,C] -> [B,h,w,C]"""
    g = np.asarray(g, np.float64)
    g = np.abs(g) if absolute else g
    h, w = top_hw
    y0, y1, yl = axis_taps(h, g.shape[1])
    x0, x1, xl = axis_taps(w, g.shape[2])
    yl, xl = yl.astype(np.float64)[None, :, None, None], xl.astype(np.float64)[None, None, :, None]
    cols = np.zeros(g.shape[:2] + (w, g.shape[3]))
    np.add.at(cols, (slice(None), slice(None), x0), g * (1 - xl))
    np.add.at(cols, (slice(None), slice(None), x1), g * xl)
    out = np.zeros((g.shape[0], h, w, g.shape[3]))
    np.add.at(out, (slice(None), y0), cols * (1 - yl))
    np.add.at(out, (slice(None), y1), cols * yl)
    return out


def neck_forward(cs, params):
    """cs = (C2, C3, C4, C5) NHWC; params[name] = (weight, bias) -> ((m2, m3, m4), (P2, P3, P4, P5, P6))"""
    c2, c3, c4, c5 = [np.asarray(c, np.float64) for c in cs]
    lin = lambda x, name: x @ np.asarray(params[name][0], np.float64).T + np.asarray(params[name][1], np.float64)
    p5 = lin(c5, 'p5')
    m4 = 0.5 * resize(p5, c4.shape[1:3]) + 0.5 * lin(c4, 'l4')
    m3 = 0.5 * resize(m4, c3.shape[1:3]) + 0.5 * lin(c3, 'l3')
    m2 = 0.5 * resize(m3, c2.shape[1:3]) + 0.5 * lin(c2, 'l2')

    def conv(m, name):
        w, b = np.asarray(params[name][0], np.float64), np.asarray(params[name][1], np.float64)
        return sum(cg.shifted(m, ky - 1, kx - 1) @ w[:, ky, kx, :].T for ky in range(3) for kx in range(3)) + b
    return (m2, m3, m4), (conv(m2, 's2'), conv(m3, 's3'), conv(m4, 's4'), p5, p5[:, ::2, ::2])


def neck_backward(cs, params, d_ps):
    """d_ps = (dP2..dP6), entries may be None -> (grads[name] = (dw, db) or absent, [dC2, dC3, dC4, dC5] (None where nothing
    arrives))"""
    cs = [np.asarray(c, np.float64) for c in cs]
    ms, _ = neck_forward(cs, params)
    grads, dm = {}, {}
    for name, m, dp in zip(('s2', 's3', 's4'), ms, d_ps[:3]):
        if dp is not None:
            grads[name] = cg.wgrad([m], [dp])
            dm[name] = cg.dgrad([np.asarray(dp, np.float64)], params[name][0])[0]
    h = None if 's2' not in dm else 0.5 * dm['s2']
    hs = {'l2': h}
    for lat, name, c in (('l3', 's3', cs[1]), ('l4', 's4', cs[2])):
        if h is not None or name in dm:
            h = 0.5 * ((dm[name] if name in dm else 0.0) + (resize_t(h, c.shape[1:3]) if h is not None else 0.0))
        hs[lat] = h
    dp5, dp6 = d_ps[3], d_ps[4]
    if h is not None or dp5 is not None or dp6 is not None:
        g = np.zeros(cs[3].shape[:3] + (np.asarray(params['p5'][0]).shape[0],))
        if dp5 is not None:
            g += np.asarray(dp5, np.float64)
        if dp6 is not None:
            g[:, ::2, ::2] += np.asarray(dp6, np.float64)
        if h is not None:
            g += resize_t(h, cs[3].shape[1:3])
        h = g
    hs['p5'] = h
    d_cs = []
    for name, c in zip(('l2', 'l3', 'l4', 'p5'), cs):
        g = hs[name]
        if g is None:
            d_cs.append(None)
            continue
        grads[name] = (np.einsum('bhwo,bhwi->oi', g, c), g.sum(axis=(0, 1, 2)))
        d_cs.append(g @ np.asarray(params[name][0], np.float64))
    return grads, d_cs
