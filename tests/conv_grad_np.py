"""The float64 statement of the 3x3 'same' convolution's backward over a list of levels (csrc/conv_grad.hip, and the input
gradient ops.conv3x3_dgrad_f32_levels runs on the forward kernel): x [B,H,W,cin], dy / y_relu [B,H,W,cout] per level (NHWC),
w [cout,3,3,cin] shared by the levels.  dz = dy where y_relu > 0 else 0 (a select, strict '>');

    dw[co,ky,kx,ci] = sum_level sum_b,y,x dz[b,y,x,co] * x[b,y+ky-1,x+kx-1,ci]        (taps outside the map are zero)
    db[co]          = sum_level sum_b,y,x dz[b,y,x,co]
    dx[b,y,x,ci]    = sum_ky,kx,co dz[b,y-ky+1,x-kx+1,co] * w[co,ky,kx,ci]

The *_abs functions give the same sums over absolute values, which the error bounds of tests/test_conv_grad_gpu.py are built
on.  `plan` restates the launch plan (cg_plan: tile and number of parts, a function of the shapes alone); `pack_index` is the
index map of odet_rpn_pack_pair, `pack` / `unpack` the two directions over it."""
import numpy as np


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def masked_dy(dy, y_relu=None):
    dy = _f64(dy)
    return dy if y_relu is None else np.where(_f64(y_relu) > 0, dy, 0.0)


def shifted(x, oy, ox):
    """out[b,y,x,:] = x[b,y+oy,x+ox,:], zero outside the map"""
    B, H, W, C = x.shape
    out = np.zeros_like(x)
    ys, ye = max(0, -oy), min(H, H - oy)
    xs, xe = max(0, -ox), min(W, W - ox)
    if ys < ye and xs < xe:
        out[:, ys:ye, xs:xe] = x[:, ys + oy:ye + oy, xs + ox:xe + ox]
    return out


def _ys(xs, y_relus):
    return [None] * len(xs) if y_relus is None else list(y_relus)


def wgrad(xs, dys, y_relus=None, absolute=False):
    """(dw [cout,3,3,cin], db [cout]) summed over the levels"""
    f = np.abs if absolute else (lambda a: a)
    cin, cout = xs[0].shape[3], dys[0].shape[3]
    dw, db = np.zeros((cout, 3, 3, cin)), np.zeros((cout,))
    for x, dy, y in zip(xs, dys, _ys(xs, y_relus)):
        x, dz = f(_f64(x)), f(masked_dy(dy, y))
        for ky in range(3):
            for kx in range(3):
                dw[:, ky, kx, :] += np.einsum('bhwo,bhwi->oi', dz, shifted(x, ky - 1, kx - 1))
        db += dz.sum(axis=(0, 1, 2))
    return dw, db


def wgrad_abs(xs, dys, y_relus=None):
    return wgrad(xs, dys, y_relus, absolute=True)


def dgrad(dzs, w, absolute=False):
    """[dx [B,H,W,cin] per level]; dzs are already gated"""
    f = np.abs if absolute else (lambda a: a)
    w = f(_f64(w))
    out = []
    for dz in dzs:
        dz = f(_f64(dz))
        dx = np.zeros(dz.shape[:3] + (w.shape[3],))
        for ky in range(3):
            for kx in range(3):
                dx += shifted(dz, 1 - ky, 1 - kx) @ w[:, ky, kx, :]
        out.append(dx)
    return out


def dgrad_abs(dzs, w):
    return dgrad(dzs, w, absolute=True)


def plan(shapes, batch, cin, cout):
    """cg_plan: (tile edge, parts, pixels per part) of the wgrad launch over levels of `shapes` [(H, W), ...]"""
    K = batch * sum(h * w for h, w in shapes)
    T = 128 if cin % 128 == 0 and cout % 128 == 0 else 64
    tiles = -(-9 * cin // T) * -(-cout // T)
    parts = 1
    if K >= 256:
        parts = max(1, min(512 // tiles, K // 64, 16))
    kper = -(-(-(-K // parts)) // 32) * 32
    return T, -(-K // kper), kper


def workspace_bytes(shapes, batch, cin, cout):
    parts = plan(shapes, batch, cin, cout)[1]
    return parts * cout * 9 * cin * 4 if parts > 1 else 0


def pack_index(pixels, A, anchor_offset):
    """the index map of odet_rpn_pack_pair for one level: (into scores[b].ravel() for channels 0 .. 2A - 1, into
    deltas[b].ravel() for channels 2A .. 6A - 1), each [pixels, channels]"""
    px = np.arange(pixels)[:, None]
    return (anchor_offset * 2 + px * 2 * A + np.arange(2 * A)[None, :],
            anchor_offset * 4 + px * 4 * A + np.arange(4 * A)[None, :])


def pack(level_out, bias, A, scores, deltas, anchor_offset):
    """level_out [B,pixels,6A] + bias -> the level's slices of scores [B,N,2] / deltas [B,N,4] (in place)"""
    B, pixels = level_out.shape[:2]
    si, di = pack_index(pixels, A, anchor_offset)
    v = level_out + bias
    for b in range(B):
        scores[b].reshape(-1)[si] = v[b, :, :2 * A]
        deltas[b].reshape(-1)[di] = v[b, :, 2 * A:6 * A]
    return scores, deltas


def unpack(d_scores, d_deltas, A, pixels, anchor_offset, channels):
    """-> [B * pixels, channels]: the gradient of the level's padded pair output, zeros from column 6A on"""
    B = d_scores.shape[0]
    si, di = pack_index(pixels, A, anchor_offset)
    out = np.zeros((B, pixels, channels), dtype=d_scores.dtype)
    for b in range(B):
        out[b, :, :2 * A] = d_scores[b].reshape(-1)[si]
        out[b, :, 2 * A:6 * A] = d_deltas[b].reshape(-1)[di]
    return out.reshape(B * pixels, channels)
