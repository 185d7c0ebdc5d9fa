"""NumPy statements of the FPN stem's backward (csrc/stem_grad.hip, ops.stem_trainable; include/odet.h "FPN stem training graph"):

    relu_maxpool3_backward_np(z, bias, dpool)   TF's MaxPoolGrad through pool1_pad, then ReluGrad, of the 3x3 / stride 2 / pad 1
                                                max-pooling after a ReLU convolution: a SERIAL loop over the windows in row-major
                                                order that adds into dz in float32 -- the declared order of a pixel's up to four
                                                terms by construction, so the kernel can be held to it bit for bit
    stem_patches_np / stem_wgrad_np             conv1's weight and bias gradient in float64: dz^T . patches over the zero-padded
                                                7 x 7 x 3 windows of the 7x7 / 2 convolution, and the column sums of dz

The checker of tests/test_stem_grad_host.py and tests/test_stem_grad_gpu.py; the product never imports it."""
import numpy as np

TAPS = tuple((dy, dx) for dy in range(3) for dx in range(3))          # the window's row-major order


def pooled_shape(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def relu_maxpool3_forward_np(z, bias):
    """max_pool(relu(z + bias)) with the 3x3 / 2 window on one skipped tap a side, float32 [B,OH,OW,C] (NaN-free data)"""
    a = np.maximum(np.asarray(z, np.float32) + np.asarray(bias, np.float32), np.float32(0))
    B, H, W, C = a.shape
    OH, OW = pooled_shape(H, W)
    pad = np.zeros((B, 2 * OH + 1, 2 * OW + 1, C), np.float32)          # (a >= 0: the padding never changes a maximum)
    pad[:, 1:H + 1, 1:W + 1] = a
    out = np.zeros((B, OH, OW, C), np.float32)
    for dy, dx in TAPS:
        out = np.maximum(out, pad[:, dy:dy + 2 * OH:2, dx:dx + 2 * OW:2])
    return out


def relu_maxpool3_backward_np(z, bias, dpool, descending=False):
    """dz [B,H,W,C] float32.  v = z + bias (one float32 add).  For every window (p,q) in ascending row-major order: its taps inside
    the map are scanned in row-major order from +0 and a tap takes over only when strictly greater, so the winner is the FIRST tap
    that holds the window's maximum and a window with nothing positive (or only NaN) has none; the winner's dz takes dpool[p,q] --
    as it is when it is the pixel's first term, added in float32 otherwise.  Every other element is +0.  ``descending``: the windows
    in the opposite order -- NOT the declared function; what the host test shows the 'order' data set tells apart."""
    z = np.asarray(z, np.float32)
    dpool = np.asarray(dpool, np.float32)
    v = z + np.asarray(bias, np.float32)
    assert v.dtype == np.float32
    B, H, W, C = v.shape
    OH, OW = pooled_shape(H, W)
    assert dpool.shape == (B, OH, OW, C), (dpool.shape, (B, OH, OW, C))
    dz = np.zeros((B, H, W, C), np.float32)
    has = np.zeros((B, H, W, C), bool)
    windows = [(p, q) for p in range(OH) for q in range(OW)]
    with np.errstate(invalid='ignore'):
        for p, q in (reversed(windows) if descending else windows):
            best = np.zeros((B, C), np.float32)
            win = np.full((B, C), -1, np.int64)
            inside = []
            for k, (dy, dx) in enumerate(TAPS):
                i, j = 2 * p - 1 + dy, 2 * q - 1 + dx
                if 0 <= i < H and 0 <= j < W:
                    take = v[:, i, j] > best                              # (False for a NaN)
                    best = np.where(take, v[:, i, j], best)
                    win = np.where(take, k, win)
                    inside.append((k, i, j))
            g = dpool[:, p, q]
            for k, i, j in inside:
                m = win == k
                dz[:, i, j] = np.where(m, np.where(has[:, i, j], dz[:, i, j] + g, g), dz[:, i, j])
                has[:, i, j] |= m
    assert dz.dtype == np.float32
    return dz


def pool_backward_bytes(B, H, W, C):
    """the algorithmic bytes of the pooling backward: z read, dz written, dpool read"""
    OH, OW = pooled_shape(H, W)
    return 4 * (2 * H * W + OH * OW) * C * B


# ---- conv1's gradients, float64 --------------------------------------------------------------------------------------------------
def stem_patches_np(images):
    """[B,H,W,3] -> float64 [B,Ho,Wo,7,7,3]: the zero-padded (3 a side) window of the 7x7 / 2 'valid' convolution at every output
    pixel, in (dy, dx, channel) order"""
    x = np.asarray(images, np.float64)
    B, H, W, _ = x.shape
    Ho, Wo = pooled_shape(H, W)
    pad = np.zeros((B, 2 * Ho + 6, 2 * Wo + 6, 3), np.float64)
    pad[:, 3:H + 3, 3:W + 3] = x
    out = np.empty((B, Ho, Wo, 7, 7, 3), np.float64)
    for dy in range(7):
        for dx in range(7):
            out[:, :, :, dy, dx] = pad[:, dy:dy + 2 * Ho:2, dx:dx + 2 * Wo:2]
    return out


def stem_conv_np(images, weight):
    """the raw convolution output z [B,Ho,Wo,64] in float64; ``weight`` [64,7,7,3] in (dy, dx, channel) order"""
    return np.einsum('bhwk,ok->bhwo', stem_patches_np(images).reshape(images.shape[0], *pooled_shape(*images.shape[1:3]), 147),
                     np.asarray(weight, np.float64).reshape(-1, 147))


def stem_wgrad_np(images, dz, absolute=False):
    """(dw [64,7,7,3], db [64]) in float64: dw = dz^T . patches over the pixels, db = the column sums of dz.  ``absolute``: the same
    products of absolute values, what the summation bounds are built on"""
    pt = stem_patches_np(images).reshape(-1, 147)
    g = np.asarray(dz, np.float64).reshape(-1, dz.shape[-1])
    if absolute:
        pt, g = np.abs(pt), np.abs(g)
    return (g.T @ pt).reshape(-1, 7, 7, 3), g.sum(axis=0)


# ---- the data sets both test files run the pooling backward on -------------------------------------------------------------------
# the issue's shapes [B,H,W,C]: odd and even sizes in both directions (first and last windows of one, two and three rows or
# columns), B > 1
SHAPES = [(1, 1, 1, 4), (1, 1, 2, 4), (1, 2, 1, 8), (1, 2, 3, 4), (1, 3, 3, 4), (1, 4, 4, 8), (2, 5, 4, 64), (1, 7, 9, 64),
          (2, 8, 6, 64)]
# one shape across each edge of the kernel's arrangement (csrc/stem_grad.hip: a workgroup takes SG_BAND = 6 window rows of a strip of
# 256 / min(C/4, 64) - 1 window columns, and 64 channel vectors), in each direction:
EDGE_SHAPES = [
    (1, 12, 30, 64),     # exactly ONE band (6 window rows) and ONE strip (15 window columns at C = 64): the last row 11 and column 29
                         # are written from the step behind the last window row / beside the last window column
    (1, 13, 31, 64),     # one window row into the second band and one window column into the second strip
    (2, 35, 63, 64),     # three whole bands, three strips, two images: inner band and strip edges, halos on both sides
    (1, 3, 513, 4),      # C = 4: 255 window columns a strip; 257 window columns cross it
    (1, 5, 7, 260),      # 65 channel vectors: one past the 64 of a chunk (3 window columns a strip: 4 cross it)
    (1, 19, 5, 12),      # 3 channel vectors: 85 window columns a strip and one idle lane in the workgroup
]
KINDS = ('int', 'normal', 'order')
BIG, ORDER_TERMS = float(2 ** 24), (float(2 ** 24), 1.0, -float(2 ** 24), 1.0)


def pool_case(kind, shape, seed=0):
    """(z, bias, dpool) float32.
    'int'     z and bias integers in -3..3, dpool integers in -3..3: ties everywhere, whole windows <= 0, z + bias == 0 exactly
    'normal'  standard normal data
    'order'   normal data below 1 in magnitude, bias 0, and peaks of 5 at the pixels whose row and column are 1 modulo 4: a window
              holds at most one peak, and a peak wins all (up to four) of its windows; their dpool is (2^24, 1, -2^24, 1) rotated
              by the channel, so the float32 sum depends on the order of the terms"""
    B, H, W, C = shape
    OH, OW = pooled_shape(H, W)
    rng = np.random.default_rng(seed * 7919 + H * 131 + W * 17 + B * 5 + C)
    if kind == 'int':
        z, bias, dpool = rng.integers(-3, 4, shape), rng.integers(-3, 4, (C,)), rng.integers(-3, 4, (B, OH, OW, C))
    elif kind == 'normal':
        z, bias, dpool = rng.standard_normal(shape), rng.standard_normal((C,)), rng.standard_normal((B, OH, OW, C))
    else:
        z, bias, dpool = np.tanh(rng.standard_normal(shape)), np.zeros((C,)), rng.standard_normal((B, OH, OW, C))
        z[:, 1::4, 1::4] = 5.0
        for i in range(1, H, 4):
            for j in range(1, W, 4):
                ws = [(p, q) for p in ((i - 1) // 2, (i + 1) // 2) for q in ((j - 1) // 2, (j + 1) // 2) if p < OH and q < OW]
                for n, (p, q) in enumerate(ws):
                    dpool[:, p, q] = np.array([ORDER_TERMS[(n + c) % 4] for c in range(C)])
    return z.astype(np.float32), bias.astype(np.float32), dpool.astype(np.float32)


def window_census(z, bias):
    """(windows, windows whose positive maximum appears more than once, windows with nothing positive) over all channels"""
    v = np.asarray(z, np.float32) + np.asarray(bias, np.float32)
    B, H, W, C = v.shape
    OH, OW = pooled_shape(H, W)
    pad = np.full((B, 2 * OH + 1, 2 * OW + 1, C), -np.inf, np.float32)
    pad[:, 1:H + 1, 1:W + 1] = v
    taps = np.stack([pad[:, dy:dy + 2 * OH:2, dx:dx + 2 * OW:2] for dy, dx in TAPS])
    mx = taps.max(axis=0)
    ties = ((taps == mx).sum(axis=0) > 1) & (mx > 0)
    return mx.size, int(ties.sum()), int((mx <= 0).sum())
