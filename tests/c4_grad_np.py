"""NumPy statements of the ResNet-C4 head's global average pooling (csrc/c4_grad.hip), one float32 operation per kernel operation:

    gap_forward(x)        odet_global_avg_pool_f32: x [R,H,W,C] or [R,hw,C] -> [R,C];  s = x[r,0,c], then s = s + x[r,p,c] for
                          p = 1 .. hw-1 in that order (row-major pixels), every add rounded to float32; s / float32(hw)
    gap_backward(g, hw)   odet_global_avg_pool_backward_f32, TF's _MeanGrad: g [R,C] -> [R,hw,C] (hw an int) or [R,H,W,C] (hw a
                          pair);  g[r,c] / float32(hw) at every pixel

The kernels must be bit-equal to them."""
import numpy as np


def gap_forward(x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    x = x.reshape(x.shape[0], -1, x.shape[-1])
    s = x[:, 0, :].copy()                                  # the first pixel itself, not 0 + it
    with np.errstate(all='ignore'):
        for p in range(1, x.shape[1]):
            s = s + x[:, p, :]                             # float32 + float32: one rounding
        return s / np.float32(x.shape[1])


def gap_backward(g, hw):
    g = np.ascontiguousarray(g, dtype=np.float32)
    shape = (int(hw),) if np.ndim(hw) == 0 else tuple(int(v) for v in hw)
    n = int(np.prod(shape))
    with np.errstate(all='ignore'):
        one = g / np.float32(n)
    out = np.empty((g.shape[0], n, g.shape[1]), dtype=np.float32)
    for p in range(n):
        out[:, p, :] = one
    return out.reshape((g.shape[0],) + shape + (g.shape[1],))
