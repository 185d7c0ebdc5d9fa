"""NumPy statements of the two operators of csrc/vgg_grad.hip (include/odet.h "VGG16 training graph"), in float32 operation by
operation so that the kernels can be held to them bit for bit:

    relu_maxpool2_backward(z, bias, dpool)      TF's MaxPoolGrad then ReluGrad of MaxPooling2D((2,2), 2, 'same') after a ReLU convolution
    dropout / dropout_backward / dropout_keep   tf.nn.dropout of TF r1.13 on the counter-based rule (Philox: tests/targets_np.py)

The checker of tests/test_vgg_grad_host.py and tests/test_vgg_grad_gpu.py; the product never imports it."""
import functools

import numpy as np

import targets_np as tn

STREAM_DROPOUT_FC1, STREAM_DROPOUT_FC2 = 6, 7
TAPS = ((0, 0), (0, 1), (1, 0), (1, 1))                      # the window's row-major order


def pooled_shape(H, W):
    return (H + 1) // 2, (W + 1) // 2


def relu_maxpool2_forward(z, bias):
    """max_pool(relu(z + bias)) with the 2x2 / 2 ceil-mode window, float32 [B,OH,OW,C] (what odet_bias_relu_maxpool writes)"""
    z = np.asarray(z, np.float32)
    a = np.maximum(z + np.asarray(bias, np.float32), np.float32(0))
    B, H, W, C = a.shape
    OH, OW = pooled_shape(H, W)
    out = np.zeros((B, OH, OW, C), np.float32)               # (a >= 0: taps outside the map never win)
    for dy, dx in TAPS:
        t = a[:, dy::2, dx::2]
        out[:, :t.shape[1], :t.shape[2]] = np.maximum(out[:, :t.shape[1], :t.shape[2]], t)
    return out


def relu_maxpool2_backward(z, bias, dpool):
    """dz [B,H,W,C] float32: with a = z + bias (one float32 add), the window's taps inside the map are scanned in row-major order
    and a tap takes over only when strictly greater, so the FIRST maximum wins; the winner receives dpool when its a is > 0; every
    other element is +0"""
    z = np.asarray(z, np.float32)
    dpool = np.asarray(dpool, np.float32)
    a = z + np.asarray(bias, np.float32)
    assert a.dtype == np.float32
    B, H, W, C = a.shape
    OH, OW = pooled_shape(H, W)
    assert dpool.shape == (B, OH, OW, C), (dpool.shape, (B, OH, OW, C))
    best = np.full((B, OH, OW, C), -np.inf, np.float32)
    win = np.full((B, OH, OW, C), -1, np.int64)
    for k, (dy, dx) in enumerate(TAPS):
        t = a[:, dy::2, dx::2]
        h, w = t.shape[1], t.shape[2]
        take = t > best[:, :h, :w]
        if k == 0:
            take = np.ones_like(take)                        # the first tap is always inside the map and starts the scan
        best[:, :h, :w] = np.where(take, t, best[:, :h, :w])
        win[:, :h, :w] = np.where(take, k, win[:, :h, :w])
    dz = np.zeros((B, H, W, C), np.float32)
    for k, (dy, dx) in enumerate(TAPS):
        h, w = dz[:, dy::2, dx::2].shape[1:3]
        dz[:, dy::2, dx::2] = np.where((win[:, :h, :w] == k) & (best[:, :h, :w] > 0), dpool[:, :h, :w], np.float32(0))
    return dz


def pool_backward_bytes(B, H, W, C):
    """the algorithmic bytes of the pooling backward: z read, dz written, dpool read"""
    OH, OW = pooled_shape(H, W)
    return 4 * (2 * H * W + OH * OW) * C * B


@functools.lru_cache(maxsize=16)
def dropout_words(n, seed, image_id, stream_id):
    """the uint32 word of each of n flat elements: word e & 3 of philox((e >> 2, image_id, stream_id, 0), seed words) (cached: the
    tests ask for the same mask several times; read-only)"""
    e = np.arange(n, dtype=np.uint64)
    w = tn.philox((e >> np.uint64(2), int(image_id) & tn.MASK, int(stream_id), 0), tn._seed_words(seed))
    words = np.stack([np.asarray(x, np.uint64) for x in w], axis=-1)                   # [n, 4]
    out = words[np.arange(n), (e & np.uint64(3)).astype(np.int64)].astype(np.uint32)
    out.setflags(write=False)
    return out


def dropout_keep(n, keep_prob, seed, image_id, stream_id):
    """keep [n] float32 in {0, 1}: floor(keep_prob + u) in float32, u = bitcast((word & 0x7fffff) | 0x3f800000) - 1"""
    words = dropout_words(n, seed, image_id, stream_id)
    u = ((words & np.uint32(0x7FFFFF)) | np.uint32(0x3F800000)).view(np.float32) - np.float32(1.0)
    keep = np.floor(np.float32(keep_prob) + u)
    assert keep.dtype == np.float32 and u.dtype == np.float32
    return keep


def dropout(x, keep_prob, seed, image_id, stream_id):
    """y = (x / keep_prob) * keep: a float32 division, then the multiplication; keep_prob == 1 returns x unchanged"""
    x = np.asarray(x, np.float32)
    if np.float32(keep_prob) == np.float32(1.0):
        return x.copy()
    keep = dropout_keep(x.size, keep_prob, seed, image_id, stream_id).reshape(x.shape)
    with np.errstate(invalid='ignore'):
        y = (x / np.float32(keep_prob)) * keep
    assert y.dtype == np.float32
    return y


def dropout_backward(dy, keep_prob, seed, image_id, stream_id):
    """dx = (dy * keep) / keep_prob, the same mask"""
    dy = np.asarray(dy, np.float32)
    if np.float32(keep_prob) == np.float32(1.0):
        return dy.copy()
    keep = dropout_keep(dy.size, keep_prob, seed, image_id, stream_id).reshape(dy.shape)
    with np.errstate(invalid='ignore'):
        dx = (dy * keep) / np.float32(keep_prob)
    assert dx.dtype == np.float32
    return dx


# ---- the data sets both test files run the pooling backward on ------------------------------------------------------------------
SIZES = [(1, 1), (1, 2), (2, 3), (5, 4), (6, 6), (7, 11)]


def pool_case(kind, hw, B, C, seed=0):
    """(z, bias, dpool) float32.  'int': integers in -2..2 (z and bias; dpool in -3..3 without zeros): many windows hold their
    positive maximum more than once and some hold nothing positive (window_census counts them).  'normal': standard normal data"""
    H, W = hw
    OH, OW = pooled_shape(H, W)
    rng = np.random.default_rng(seed * 7919 + H * 131 + W * 17 + B * 5 + C)
    if kind == 'int':
        z = rng.choice([-2, -1, 0, 1, 2], (B, H, W, C), p=[0.1, 0.1, 0.2, 0.2, 0.4])      # (2 is frequent: it ties often)
        bias = rng.integers(-1, 2, (C,))
        dpool = rng.integers(1, 4, (B, OH, OW, C)) * rng.choice([-1, 1], (B, OH, OW, C))
    else:
        z, bias, dpool = rng.standard_normal((B, H, W, C)), rng.standard_normal((C,)), rng.standard_normal((B, OH, OW, C))
    return z.astype(np.float32), bias.astype(np.float32), dpool.astype(np.float32)


def window_census(z, bias):
    """(windows, windows whose positive maximum appears more than once, windows with nothing positive) over all channels"""
    a = np.asarray(z, np.float32) + np.asarray(bias, np.float32)
    B, H, W, C = a.shape
    OH, OW = pooled_shape(H, W)
    pad = np.full((B, 2 * OH, 2 * OW, C), -np.inf, np.float32)
    pad[:, :H, :W] = a
    taps = np.stack([pad[:, dy::2, dx::2] for dy, dx in TAPS])                          # [4,B,OH,OW,C]
    mx = taps.max(axis=0)
    ties = ((taps == mx).sum(axis=0) > 1) & (mx > 0)
    return mx.size, int(ties.sum()), int((mx <= 0).sum())
