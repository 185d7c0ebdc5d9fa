"""NumPy statements of the ResNet bottleneck's backward (csrc/block_grad.hip, model/extractor_trainable.py; reference
model/fpn/resnet_fpn.py:154-205 in reverse): the two elementwise launches in the dtype of their arguments (float32: the kernels' own
bits), the float64 statement of a whole block's forward and backward over NHWC arrays, and the integer data set on which every
float32 sum of the block's backward is exact.

A block's parameters are a dict P: w1 [f, cin], b1 [f], w2 [f, 3, 3, f], b2 [f], w3 [4f, f], b3 [4f] and, with a convolutional
shortcut, ws [4f, cin], bs [4f]; the stride sits on the first 1x1 convolution and on the shortcut."""
import numpy as np

# the smallest channels the kernels' rules allow: (cin, f, stride, convolutional shortcut)
KINDS = {'identity': (256, 64, 1, False), 'conv_s1': (64, 64, 1, True), 'conv_s2': (256, 64, 2, True)}
MAPS = [(2, 3), (5, 4), (7, 11)]
LAYERS = ('c1', 'c2', 'c3', 'short')


def stride_gather(x, stride):
    """odet_stride_gather_f32: out[b,i,j,:] = x[b, i*stride, j*stride, :]"""
    return np.ascontiguousarray(x[:, ::stride, ::stride])


def input_grad_identity(dy, y, d1):
    """odet_block_input_grad_f32, identity form: (y > 0 ? dy : +0) + d1 -- one add in the arguments' dtype"""
    return np.where(y > 0, dy, np.zeros_like(dy)) + d1


def input_grad_conv(d1, d2, stride, in_hw):
    """odet_block_input_grad_f32, convolutional-shortcut form: d1 + d2 (d2 may be None) placed at the pixels whose coordinates are
    multiples of stride, +0 elsewhere"""
    B, Ho, Wo, C = d1.shape
    H, W = in_hw
    assert ((H - 1) // stride + 1, (W - 1) // stride + 1) == (Ho, Wo)
    out = np.zeros((B, H, W, C), d1.dtype)
    out[:, ::stride, ::stride] = d1 if d2 is None else d1 + d2
    return out


# ---- float64 contractions over NHWC arrays -------------------------------------------------------------------------------------
def lin(x, w):
    return x @ w.T


def lin_wgrad(dz, x):
    return np.einsum('bhwo,bhwi->oi', dz, x)


def lin_dgrad(dz, w):
    return dz @ w


def conv3(x, w):
    """3x3 'same' convolution: x [B,H,W,ci], w [co,3,3,ci]"""
    H, W = x.shape[1:3]
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    return sum(xp[:, ky:ky + H, kx:kx + W] @ w[:, ky, kx].T for ky in range(3) for kx in range(3))


def conv3_wgrad(dz, x):
    H, W = x.shape[1:3]
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    dw = np.zeros((dz.shape[3], 3, 3, x.shape[3]), dz.dtype)
    for ky in range(3):
        for kx in range(3):
            dw[:, ky, kx] = np.einsum('bhwo,bhwi->oi', dz, xp[:, ky:ky + H, kx:kx + W])
    return dw


def conv3_dgrad(dz, w):
    H, W = dz.shape[1:3]
    zp = np.pad(dz, ((0, 0), (1, 1), (1, 1), (0, 0)))
    return sum(zp[:, 2 - ky:2 - ky + H, 2 - kx:2 - kx + W] @ w[:, ky, kx] for ky in range(3) for kx in range(3))


class Record(dict):
    """every intermediate of a block's forward and backward by name; `mag[name]`: the same contraction on the operands' magnitudes
    -- an upper bound of every partial sum of it, in any order"""

    def __init__(self):
        super().__init__()
        self.mag = {}

    def contract(self, name, fn, *operands):
        self[name] = fn(*operands)
        self.mag[name] = fn(*[np.abs(o) for o in operands])
        return self[name]


def block_backward(x, P, stride, dy, gates=None):
    """The float64 statement of one bottleneck, forward and backward: x [B,H,W,cin], dy [B,Ho,Wo,4f] -> (y, {layer: (dw, db)}, dx,
    the Record of every intermediate).  `gates`: (a > 0, b > 0, y > 0) as boolean arrays taken from elsewhere (a float32 forward's
    own: then no gate can fall the other way); default: the statement's own."""
    r = Record()
    short = 'ws' in P
    xs = r['xs'] = stride_gather(x, stride)
    pre_a = r.contract('a_sum', lin, xs, P['w1']) + P['b1']
    ga = pre_a > 0 if gates is None else gates[0]
    a = r['a'] = np.where(ga, pre_a, 0.0)
    pre_b = r.contract('b_sum', conv3, a, P['w2']) + P['b2']
    gb = pre_b > 0 if gates is None else gates[1]
    b = r['b'] = np.where(gb, pre_b, 0.0)
    pre_y = r.contract('y_sum', lin, b, P['w3']) + P['b3']
    pre_y = pre_y + ((r.contract('s_sum', lin, xs, P['ws']) + P['bs']) if short else x)
    gy = pre_y > 0 if gates is None else gates[2]
    y = r['y'] = np.where(gy, pre_y, 0.0)
    r.gates = {'a': ga, 'b': gb, 'y': gy}
    # backward
    dz3 = r['dz3'] = np.where(gy, dy, 0.0)
    grads = {'c3': (r.contract('dw3', lin_wgrad, dz3, b), dz3.sum((0, 1, 2)))}
    db_gated = r['db_gated'] = np.where(gb, r.contract('db_sum', lin_dgrad, dz3, P['w3']), 0.0)
    grads['c2'] = (r.contract('dw2', conv3_wgrad, db_gated, a), db_gated.sum((0, 1, 2)))
    dz1 = r['dz1'] = np.where(ga, r.contract('da', conv3_dgrad, db_gated, P['w2']), 0.0)
    grads['c1'] = (r.contract('dw1', lin_wgrad, dz1, xs), dz1.sum((0, 1, 2)))
    d1 = r.contract('d1', lin_dgrad, dz1, P['w1'])
    if short:
        grads['short'] = (r.contract('dws', lin_wgrad, dz3, xs), dz3.sum((0, 1, 2)))
        d2 = r.contract('d2', lin_dgrad, dz3, P['ws'])
        dx = input_grad_conv(d1, d2, stride, x.shape[1:3])
    else:
        dx = input_grad_identity(dy, y, d1)
    r['dx'] = dx
    for name, (dw, db) in grads.items():
        r['db_' + name] = db
    return y, grads, dx, r


# ---- the integer data set ------------------------------------------------------------------------------------------------------
def integer_case(kind, hw, B, seed=0):
    """(x, P, dy) as float64 arrays of small integers: maps and output gradients in [-3, 3] at density 1/2, weights and biases in
    {-1, 0, 1} (1x1 weights at density 1/8, the 3x3 weight at 1/16, c3's at 1/4) -- every value of the block's forward and backward is
    then an integer far below 2^24 (assert_exact_in_float32), so float32 sums are exact in any order"""
    cin, f, stride, short = KINDS[kind]
    rng = np.random.default_rng([seed, cin, stride, hw[0], hw[1], B])
    sparse = lambda shape, lo, hi, dens: (rng.integers(lo, hi + 1, shape) * (rng.random(shape) < dens)).astype(np.float64)
    P = {'w1': sparse((f, cin), -1, 1, 1 / 8), 'b1': sparse((f,), -1, 1, 1.0),
         'w2': sparse((f, 3, 3, f), -1, 1, 1 / 16), 'b2': sparse((f,), -1, 1, 1.0),
         'w3': sparse((4 * f, f), -1, 1, 1 / 4), 'b3': sparse((4 * f,), -1, 1, 1.0)}
    if short:
        P['ws'], P['bs'] = sparse((4 * f, cin), -1, 1, 1 / 8), sparse((4 * f,), -1, 1, 1.0)
    H, W = hw
    x = sparse((B, H, W, cin), -3, 3, 1 / 2)
    dy = sparse((B, (H - 1) // stride + 1, (W - 1) // stride + 1, 4 * f), -3, 3, 1 / 2)
    return x, P, dy


def assert_exact_in_float32(record):
    """every intermediate is an integer of magnitude < 2^24, so is every contraction on the operands' magnitudes (hence every
    partial sum in any order), and every ReLU gate has open and closed elements"""
    worst = 0.0
    for name, v in list(record.items()) + [('|%s|' % k, m) for k, m in record.mag.items()]:
        v = np.asarray(v, dtype=np.float64)
        assert np.array_equal(v, np.rint(v)), name
        worst = max(worst, float(np.abs(v).max()))
        assert np.abs(v).max() < 2 ** 24, (name, float(np.abs(v).max()))
    for name, g in record.gates.items():
        assert g.any() and not g.all(), 'gate %s is %s everywhere' % (name, 'open' if g.all() else 'closed')
    return worst
