"""The ResNet bottleneck's backward on the GPU: odet_stride_gather_f32 and odet_block_input_grad_f32 (csrc/block_grad.hip) bit-equal
to the statements of tests/block_grad_np.py and bit-equal between calls; one trainable block (model/extractor_trainable.py: output
bit-equal to _Block.forward; gradients bit-equal to the ops called by hand, exact by bytes against float64 autograd of the plain
F.conv2d block on the integer data set that tests/test_block_grad_host.py proves exact, within the composed any-order summation bound
on normal random data, no input-gradient launch for an input that requires none); ResNetFpnDetector.extractor_trainable at depth 50
with its backward under graph capture; and the caller model with train_extractor.

Worst observed fractions of the composed bound are printed by test_block_trainable_within_the_composed_bound; the table is in DESIGN
3.17."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import block_grad_np as bg

pytestmark = pytest.mark.gpu

U = 2.0 ** -23
SIZES = [(1, 1), (1, 2), (2, 3), (5, 4), (6, 6), (7, 11)]
STAGES = ('conv2', 'conv3', 'conv4', 'conv5')
NECK_NAMES = tuple('%s.%s' % (layer, part) for layer in ('p5', 'l4', 'l3', 'l2', 's4', 's3', 's2') for part in ('weight', 'bias'))
HEAD_NAMES = ('rpn_conv.weight', 'rpn_conv.bias', 'rpn_score.weight', 'rpn_score.bias', 'rpn_bbox.weight', 'rpn_bbox.bias')
ROI_NAMES = ('fc1.weight', 'fc1.bias', 'fc2.weight', 'fc2.bias', 'score.weight', 'score.bias', 'bbox.weight', 'bbox.bias')
_ID = lambda c: '%dx%d' % tuple(c) if isinstance(c, tuple) else None


def _ops():
    from tf_eager_object_detection_amd import ops
    return ops


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _np_bits_equal(got, want):
    got = got.cpu().numpy()
    return got.shape == want.shape and np.array_equal(got.view(np.int32), np.ascontiguousarray(want, dtype=np.float32).view(np.int32))


def _nan(*shape):
    return torch.full(shape, float('nan'), device='cuda')


# ---- (1) the kernels against their statements ----------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [4, 64, 256])
@pytest.mark.parametrize('hw', SIZES, ids=_ID)
def test_kernels_are_bit_equal_to_the_statements(hw, C):
    """normal random data, B in {1, 2}, stride 1 and 2, both forms of the join, d2 present and absent; every output buffer starts as
    NaN: every element is written"""
    ops = _ops()
    H, W = hw
    rng = np.random.default_rng(H * 1009 + W * 31 + C)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    for B in (1, 2):
        x = f(B, H, W, C)
        dy, y, d1 = f(B, H, W, C), f(B, H, W, C), f(B, H, W, C)
        out = _nan(B, H, W, C)
        got = ops.block_input_grad(_dev(d1), dy=_dev(dy), y=_dev(y), out=out)
        assert got is out and _np_bits_equal(got, bg.input_grad_identity(dy, y, d1)), ('identity', B)
        for stride in (1, 2):
            Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
            out = _nan(B, Ho, Wo, C)
            got = ops.stride_gather(_dev(x), stride, out=out)
            assert got is out and _np_bits_equal(got, bg.stride_gather(x, stride)), ('gather', B, stride)
            g1, g2 = f(B, Ho, Wo, C), f(B, Ho, Wo, C)
            for d2 in (g2, None):
                out = _nan(B, H, W, C)
                got = ops.block_input_grad(_dev(g1), d2=_dev(d2), stride=stride, in_hw=hw, out=out)
                assert got is out and _np_bits_equal(got, bg.input_grad_conv(g1, d2, stride, hw)), ('conv', B, stride, d2 is None)
        if H % 2 == 0:                      # the other input size with the same Ho: the last row is one the stride does not reach
            assert ops.block_input_grad(_dev(g1), stride=2, in_hw=(H - 1, W)).shape == (B, H - 1, W, C)


def test_grid_stride_pass_is_bit_equal_to_the_statements():
    """more lanes (130 * 130 * 256 = 4.3 M) than the launch's 16384 workgroups of 256 hold: the lanes of the second pass"""
    ops = _ops()
    rng = np.random.default_rng(9)
    B, H, W, C = 1, 130, 130, 1024
    assert B * H * W * (C // 4) > 16384 * 256
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    x, y, d1 = f(B, H, W, C), f(B, H, W, C), f(B, H, W, C)
    assert _np_bits_equal(ops.stride_gather(_dev(x), 1, out=_nan(B, H, W, C)), x)
    assert _np_bits_equal(ops.block_input_grad(_dev(d1), dy=_dev(x), y=_dev(y), out=_nan(B, H, W, C)), bg.input_grad_identity(x, y, d1))
    g1, g2 = x[:, :65, :65].copy(), y[:, :65, :65].copy()
    assert _np_bits_equal(ops.block_input_grad(_dev(g1), d2=_dev(g2), stride=2, in_hw=(H, W), out=_nan(B, H, W, C)),
                          bg.input_grad_conv(g1, g2, 2, (H, W)))


def test_identity_gate_is_strict():
    """y exactly +0 and -0 close the gate (the shortcut's gradient is dropped: dx = +0 + d1); the smallest positive float opens it"""
    ops = _ops()
    rng = np.random.default_rng(3)
    shape = (2, 5, 4, 64)
    y = rng.standard_normal(shape).astype(np.float32)
    flat = y.reshape(-1)
    flat[::3], flat[1::7], flat[2::11] = 0.0, -0.0, 1e-45
    assert (flat == 0).sum() > 100 and np.signbit(flat[flat == 0]).any() and not np.signbit(flat[flat == 0]).all()
    dy = (rng.standard_normal(shape) + 3).astype(np.float32)
    d1 = rng.standard_normal(shape).astype(np.float32)
    d1.reshape(-1)[::6] = -0.0
    want = bg.input_grad_identity(dy, y, d1)
    closed = y == 0
    assert np.array_equal(want[closed].view(np.int32), (np.float32(0) + d1[closed]).view(np.int32))
    assert np.array_equal(want[y == np.float32(1e-45)], (dy + d1)[y == np.float32(1e-45)])
    assert _np_bits_equal(ops.block_input_grad(_dev(d1), dy=_dev(dy), y=_dev(y), out=_nan(*shape)), want)


def test_two_calls_are_bit_equal():
    """hundreds of workgroups, whose order of execution is free; fresh outputs"""
    ops = _ops()
    rng = np.random.default_rng(5)
    B, H, W, C = 2, 50, 84, 256
    t = lambda *s: _dev(rng.standard_normal(s))
    x, dy, y, d1 = t(B, H, W, C), t(B, H, W, C), t(B, H, W, C), t(B, H, W, C)
    g1, g2 = t(B, 25, 42, C), t(B, 25, 42, C)
    first = (ops.stride_gather(x, 2), ops.block_input_grad(d1, dy=dy, y=y), ops.block_input_grad(g1, d2=g2, stride=2, in_hw=(H, W)))
    junk = torch.full((B, H, W, C), 7.0, device='cuda')                           # (the allocator hands out other memory)
    again = (ops.stride_gather(x, 2), ops.block_input_grad(d1, dy=dy, y=y), ops.block_input_grad(g1, d2=g2, stride=2, in_hw=(H, W)))
    assert all(_same_bits(a, b) and bool(torch.isfinite(a).all()) for a, b in zip(first, again)) and junk is not None


def test_python_fronts_argument_errors():
    ops = _ops()
    z = lambda *s: torch.zeros(*s, device='cuda')
    x, d = z(1, 5, 4, 8), z(1, 3, 2, 8)
    assert tuple(ops.stride_gather(x, 2).shape) == (1, 3, 2, 8) and tuple(ops.stride_gather(x, 1).shape) == (1, 5, 4, 8)
    assert tuple(ops.block_input_grad(d, d2=d, stride=2, in_hw=(5, 4)).shape) == (1, 5, 4, 8)
    assert tuple(ops.block_input_grad(d, stride=2, in_hw=(6, 3)).shape) == (1, 6, 3, 8)
    assert tuple(ops.block_input_grad(x, dy=x, y=x).shape) == (1, 5, 4, 8)
    for bad, match in ((x.half(), 'float32'), (x.cpu(), 'GPU'), (z(1, 4, 5, 8).permute(0, 2, 1, 3), 'contiguous'),
                       (z(1, 8, 5, 4).permute(0, 2, 3, 1), 'contiguous'), (z(1, 5, 4, 6), 'multiple of 4')):
        with pytest.raises(ValueError, match=match):
            ops.stride_gather(bad, 2)
        with pytest.raises(ValueError, match=match):
            ops.block_input_grad(bad, dy=bad, y=bad)
    for name in ('dy', 'y', 'd1'):
        for bad, match in ((x.cpu(), 'GPU'), (x.double(), 'float32'), (z(1, 5, 4, 4), 'does not go with'), (z(2, 5, 4, 8), 'does not go with')):
            args = dict(dict(dy=x, y=x, d1=x), **{name: bad})
            if name == 'd1' and match == 'does not go with':
                continue                                                           # (d1 is what the others are compared with)
            with pytest.raises(ValueError, match=match):
                ops.block_input_grad(args['d1'], dy=args['dy'], y=args['y'])
    with pytest.raises(ValueError, match='GPU'):
        ops.block_input_grad(d, d2=d.cpu(), stride=2, in_hw=(5, 4))
    for form in ('x3', 'x2'):
        with ops.f32_form(form):
            with pytest.raises(ValueError, match="only under f32_form 'exact'"):
                ops.stride_gather(x, 2)
            with pytest.raises(ValueError, match="only under f32_form 'exact'"):
                ops.block_input_grad(d, d2=d, stride=2, in_hw=(5, 4))
    for out in (z(1, 5, 4, 4), z(1, 4, 5, 8), z(1, 5, 4, 8).half(), z(1, 5, 8, 4).permute(0, 1, 3, 2)):
        with pytest.raises(ValueError, match='out must be'):
            ops.block_input_grad(d, d2=d, stride=2, in_hw=(5, 4), out=out)
        with pytest.raises(ValueError, match='out must be'):
            ops.stride_gather(x, 1, out=out)


# ---- (2) one trainable block -------------------------------------------------------------------------------------------------------
PARAM_KEYS = (('c1.weight', 'w1'), ('c1.bias', 'b1'), ('c2.weight', 'w2'), ('c2.bias', 'b2'), ('c3.weight', 'w3'), ('c3.bias', 'b3'),
              ('short.weight', 'ws'), ('short.bias', 'bs'))


@pytest.fixture(scope='module')
def blocks():
    """one _Block per kind at the smallest channels the kernels' rules allow, with non-zero biases"""
    from tf_eager_object_detection_amd.model.layers import _Block
    torch.manual_seed(6)
    made = {}
    for kind, (cin, f, stride, short) in bg.KINDS.items():
        blk = _Block(cin, f, stride, short).to(device='cuda', dtype=torch.float32, memory_format=torch.channels_last).eval()
        with torch.no_grad():
            for p in blk.parameters():
                if p.dim() == 1:
                    p.add_(torch.linspace(-0.3, 0.3, p.numel(), device='cuda'))
        made[kind] = blk
    return made


def _map(a):
    """an NHWC array as a channels_last [B,C,H,W] float32 GPU tensor"""
    return _dev(a).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _random_case(kind, hw, B, seed):
    cin, f, stride, _ = bg.KINDS[kind]
    rng = np.random.default_rng([seed, cin, stride, hw[0], hw[1], B])
    H, W = hw
    x = rng.standard_normal((B, H, W, cin)).astype(np.float32)
    dy = rng.standard_normal((B, (H - 1) // stride + 1, (W - 1) // stride + 1, 4 * f)).astype(np.float32)
    return _map(x), _map(dy)


def _manual_block_grads(blk, x, dy, with_dx):
    """the block's gradients from the ops called by hand, with a freshly flipped weight: what autograd must deliver, bit for bit ->
    ({parameter name: gradient in the parameter's shape}, dx or None, (a, b, y))"""
    from tf_eager_object_detection_amd.model.layers import _conv_epi
    ops = _ops()
    with torch.no_grad():
        stride = blk.c1.stride[0]
        a4 = _conv_epi(blk.c1, x, relu=True)
        b4 = _conv_epi(blk.c2, a4, relu=True)
        y4 = blk(x)
        a, b, y, g, xn = _nhwc(a4), _nhwc(b4), _nhwc(y4), _nhwc(dy), _nhwc(x)
        xs = xn[:, ::stride, ::stride].contiguous()
        f, cin, cout = a.shape[3], xn.shape[3], y.shape[3]
        rows = lambda t: t.view(-1, t.shape[3])
        w2d = lambda conv: conv.weight.reshape(conv.weight.shape[0], -1).contiguous()
        out = {}
        dw, out['c3.bias'] = ops.dense_wgrad(rows(g), rows(b), y_relu=rows(y))
        out['c3.weight'] = dw.view(cout, f, 1, 1)
        dbg = ops.dense_dgrad(rows(g), w2d(blk.c3), y_relu=rows(y), x_relu=rows(b)).view(b.shape)
        dw, out['c2.bias'] = ops.conv3x3_wgrad_f32_levels([a], [dbg])
        out['c2.weight'] = dw.permute(0, 3, 1, 2)
        da = ops.conv3x3_dgrad_f32_levels([dbg], blk.c2.weight, flipped=ops.conv3x3_flipped_weight(blk.c2.weight))[0]
        dw, out['c1.bias'] = ops.dense_wgrad(rows(da), rows(xs), y_relu=rows(a))
        out['c1.weight'] = dw.view(f, cin, 1, 1)
        d1 = ops.dense_dgrad(rows(da), w2d(blk.c1), y_relu=rows(a)).view(xs.shape) if with_dx else None
        dx = None
        if blk.short is not None:
            dw, out['short.bias'] = ops.dense_wgrad(rows(g), rows(xs), y_relu=rows(y))
            out['short.weight'] = dw.view(cout, cin, 1, 1)
            if with_dx:
                d2 = ops.dense_dgrad(rows(g), w2d(blk.short), y_relu=rows(y)).view(xs.shape)
                dx = ops.block_input_grad(d1, d2=d2, stride=stride, in_hw=tuple(xn.shape[1:3]))
        elif with_dx:
            dx = ops.block_input_grad(d1, dy=g, y=y)
    return out, None if dx is None else dx.permute(0, 3, 1, 2), (a4, b4, y4)


def _run_block(blk, x, dy, with_dx=True):
    """block_trainable forward (asserted bit-equal to _Block.forward, same shape and strides) and backward -> (the input, y)"""
    from tf_eager_object_detection_amd.model.extractor_trainable import block_trainable
    blk.zero_grad(set_to_none=True)
    with torch.no_grad():
        want = blk(x)
    xin = x.clone().requires_grad_() if with_dx else x
    y = block_trainable(blk, xin)
    assert y.requires_grad and y.shape == want.shape and y.stride() == want.stride() and _same_bits(y, want)
    y.backward(dy)
    return xin, y


CASES = [(kind, hw, B) for kind in bg.KINDS for hw in bg.MAPS for B in (1, 2)]
_CASE_ID = lambda c: '%s-%dx%d-b%d' % (c[0], c[1][0], c[1][1], c[2])


@pytest.mark.parametrize('case', CASES, ids=_CASE_ID)
def test_block_trainable_is_bit_equal_to_block_forward_and_to_the_ops_by_hand(blocks, case, monkeypatch):
    """(a), (b) and (e): with an input that requires a gradient every gradient is the hand-called ops', bit for bit, in its parameter's
    layout; with one that does not, the backward makes c3's one dgrad launch and no join launch, and leaves the same parameter
    gradients"""
    kind, hw, B = case
    blk = blocks[kind]
    ops = _ops()
    x, dy = _random_case(kind, hw, B, 1)
    manual, dx, _ = _manual_block_grads(blk, x, dy, True)
    calls = {'dgrad': 0, 'join': 0}
    dgrad, join = ops.dense_dgrad, ops.block_input_grad

    def spy_dgrad(*a, **k):
        calls['dgrad'] += 1
        return dgrad(*a, **k)

    def spy_join(*a, **k):
        calls['join'] += 1
        return join(*a, **k)

    monkeypatch.setattr(ops, 'dense_dgrad', spy_dgrad)
    monkeypatch.setattr(ops, 'block_input_grad', spy_join)
    params = dict(blk.named_parameters())
    assert len(params) == len(manual) == (8 if blk.short is not None else 6)
    for with_dx in (True, False):
        calls.update(dgrad=0, join=0)
        xin, _ = _run_block(blk, x, dy, with_dx)
        for n, p in params.items():
            assert p.grad is not None and p.grad.shape == p.shape and p.grad.stride() == p.stride(), n
            assert _same_bits(p.grad, manual[n]), (n, with_dx)
        if with_dx:
            assert xin.grad is not None and xin.grad.shape == x.shape and _same_bits(xin.grad, dx)
            assert calls == {'dgrad': 3 if blk.short is not None else 2, 'join': 1}, calls
        else:
            assert xin.grad is None and calls == {'dgrad': 1, 'join': 0}, calls
    blk.zero_grad(set_to_none=True)


def _plain_block(x, P, stride, gates=None):
    """the plain F.conv2d bottleneck on NCHW tensors; gates: (a > 0, b > 0, y > 0) as 0 / 1 tensors in place of the ReLUs"""
    act = (lambda t, i: F.relu(t)) if gates is None else (lambda t, i: t * gates[i])
    a = act(F.conv2d(x, P['c1.weight'], P['c1.bias'], stride=stride), 0)
    b = act(F.conv2d(a, P['c2.weight'], P['c2.bias'], padding=1), 1)
    y = F.conv2d(b, P['c3.weight'], P['c3.bias'])
    y = y + (F.conv2d(x, P['short.weight'], P['short.bias'], stride=stride) if 'short.weight' in P else x)
    return a, b, act(y, 2)


def _set_params(blk, P):
    """P of block_grad_np (w2 [f,3,3,f]) into the block's parameters"""
    params = dict(blk.named_parameters())
    with torch.no_grad():
        for name, key in PARAM_KEYS:
            if name in params:
                v = torch.from_numpy(P[key].astype(np.float32)).cuda()
                params[name].copy_(v.permute(0, 3, 1, 2) if key == 'w2' else v.view(params[name].shape))


@pytest.mark.parametrize('case', CASES, ids=_CASE_ID)
def test_block_trainable_is_exact_on_the_integer_data_set(blocks, case):
    """(c): on block_grad_np.integer_case (proved exact in float32 by tests/test_block_grad_host.py for these very cases) every
    gradient equals float64 torch autograd of the plain F.conv2d block, by bytes"""
    kind, hw, B = case
    blk = blocks[kind]
    params = dict(blk.named_parameters())
    saved = {n: p.detach().clone() for n, p in params.items()}
    try:
        x, P, dy = bg.integer_case(kind, hw, B)
        _set_params(blk, P)
        xin, y = _run_block(blk, _map(x), _map(dy))
        d = lambda t: t.detach().double().contiguous()
        P64 = {n: d(p).requires_grad_() for n, p in params.items()}
        x64 = d(_map(x)).requires_grad_()
        y64 = _plain_block(x64, P64, bg.KINDS[kind][2])[2]
        y64.backward(d(_map(dy)))
        same_bytes = lambda g, r: g.shape == r.shape and g.detach().contiguous().cpu().numpy().tobytes() == r.float().contiguous().cpu().numpy().tobytes()
        assert torch.equal(y.double(), y64)
        for n, p in params.items():
            r = P64[n].grad
            assert float(r.abs().max()) > 0 and torch.equal(r.float().double(), r), n
            assert same_bytes(p.grad, r), (n, float((p.grad.double() - r).abs().max()))
        assert float(x64.grad.abs().max()) > 0 and same_bytes(xin.grad, x64.grad), float((xin.grad.double() - x64.grad).abs().max())
    finally:
        with torch.no_grad():
            for n, p in params.items():
                p.copy_(saved[n])
        blk.zero_grad(set_to_none=True)


def _block_reference(blk, x, dy, forward32):
    """float64 torch autograd of the plain F.conv2d block on the same float32 input, parameters and output gradient -> ({name:
    gradient, 'dx': ...}, the same keys' bounds).  The ReLU gates are the float32 forward's own a > 0, b > 0, y > 0 (so no gate can
    fall the other way in the reference).  The any-order summation bound of DESIGN 3.15(b) composed over the block (u = 2^-23; |.|
    elementwise; a contraction of length K on operands with error bounds Ea, Eb: K u (|a| + Ea)(|b| + Eb) + Ea (|b| + Eb) + |a| Eb;
    R = B Ho Wo output pixels, the contraction length of every parameter gradient; g_a, g_b, g_y the 0 / 1 gates; xs the block's
    input at the stride's pixels; (*) the 3x3 weight gradient's sum over pixels per tap):
      forward   Ea = g_a (cin + 1) u (|xs| |W1|^T + |b1|)
                Eb = g_b ((9 f + 1) u (conv(|a| + Ea, |W2|) + |b2|) + conv(Ea, |W2|))
      c3        dz3 = g_y dy, exact.   dW3: R u |dz3|^T (|b| + Eb) + |dz3|^T Eb;   db3: R u sum |dz3|
                db_gated = g_b (dz3 W3): Dg = g_b 4f u |dz3| |W3|
      c2        dW2: R u (|db_gated| + Dg) (*) (|a| + Ea) + Dg (*) (|a| + Ea) + |db_gated| (*) Ea;   db2: R u sum (|db_gated| + Dg) + sum Dg
                da = conv(db_gated, W2 flipped): Eda = 9 f u conv(|db_gated| + Dg, |W2f|) + conv(Dg, |W2f|)
      c1        dz1 = g_a da: Ez = g_a Eda.   dW1: R u (|dz1| + Ez)^T |xs| + Ez^T |xs|;   db1: R u sum (|dz1| + Ez) + sum Ez
                d1 = dz1 W1: M1 = (|dz1| + Ez) |W1| bounds |d1| + its error;   Ed1 = f u M1 + Ez |W1|
      shortcut  dWs: R u |dz3|^T |xs|;   dbs: R u sum |dz3|;   d2 = dz3 Ws: M2 = |dz3| |Ws|, Ed2 = 4f u M2
      join      identity: Ed1 + u (|dz3| + M1) (one add);   convolutional: Ed1 + Ed2 + u (M1 + M2) at the stride's pixels, 0 elsewhere"""
    a32, b32, y32 = forward32
    d = lambda t: t.detach().double().contiguous()
    Ab = torch.abs
    params = dict(blk.named_parameters())
    P = {n: d(p).requires_grad_() for n, p in params.items()}
    X = d(x).requires_grad_()
    s = blk.c1.stride[0]
    short = blk.short is not None
    ga, gb, gy = d(a32 > 0), d(b32 > 0), d(y32 > 0)
    a, b, y = _plain_block(X, P, s, (ga, gb, gy))
    a.retain_grad()
    b.retain_grad()
    y.backward(d(dy))
    ref = {n: P[n].grad for n in P}
    ref['dx'] = X.grad
    with torch.no_grad():
        xs = Ab(X[:, :, ::s, ::s])
        B, f, cin, cout = X.shape[0], a.shape[1], X.shape[1], y.shape[1]
        R = B * y.shape[2] * y.shape[3]
        W1, W2, W3 = Ab(P['c1.weight']), Ab(P['c2.weight']), Ab(P['c3.weight'])
        mm = lambda g, v: torch.einsum('bohw,bihw->oi', g, v)[:, :, None, None]
        back = lambda g, w: torch.einsum('bohw,oi->bihw', g, w.reshape(w.shape[0], -1))
        sums = lambda g: g.sum((0, 2, 3))

        def wg(g, v):
            unf = F.unfold(v, 3, padding=1)                                            # [B, C * 9, pixels]
            return torch.einsum('bol,bkl->ok', g.reshape(B, g.shape[1], -1), unf).reshape(g.shape[1], v.shape[1], 3, 3)

        Ea = ga * (cin + 1) * U * F.conv2d(xs, W1, Ab(P['c1.bias']))
        Eb = gb * ((9 * f + 1) * U * F.conv2d(Ab(a) + Ea, W2, Ab(P['c2.bias']), padding=1) + F.conv2d(Ea, W2, padding=1))
        dz3 = gy * Ab(d(dy))
        bound = {'c3.weight': R * U * mm(dz3, Ab(b) + Eb) + mm(dz3, Eb), 'c3.bias': R * U * sums(dz3)}
        dbg, Dg = gb * Ab(b.grad), gb * cout * U * back(dz3, W3)
        bound['c2.weight'] = R * U * wg(dbg + Dg, Ab(a) + Ea) + wg(Dg, Ab(a) + Ea) + wg(dbg, Ea)
        bound['c2.bias'] = R * U * sums(dbg + Dg) + sums(Dg)
        W2f = W2.flip(2, 3).transpose(0, 1)
        Ez = ga * (9 * f * U * F.conv2d(dbg + Dg, W2f, padding=1) + F.conv2d(Dg, W2f, padding=1))
        dz1 = ga * Ab(a.grad)
        bound['c1.weight'] = R * U * mm(dz1 + Ez, xs) + mm(Ez, xs)
        bound['c1.bias'] = R * U * sums(dz1 + Ez) + sums(Ez)
        M1 = back(dz1 + Ez, W1)
        Ed1 = f * U * M1 + back(Ez, W1)
        if short:
            Ws = Ab(P['short.weight'])
            bound['short.weight'], bound['short.bias'] = R * U * mm(dz3, xs), R * U * sums(dz3)
            M2 = back(dz3, Ws)
            bdx = torch.zeros_like(X)
            bdx[:, :, ::s, ::s] = Ed1 + cout * U * M2 + U * (M1 + M2)
        else:
            bdx = Ed1 + U * (dz3 + M1)
        bound['dx'] = bdx
    return ref, bound


@pytest.mark.parametrize('case', CASES, ids=_CASE_ID)
def test_block_trainable_within_the_composed_bound(blocks, case):
    """(d): normal random data, every product rounds"""
    kind, hw, B = case
    blk = blocks[kind]
    x, dy = _random_case(kind, hw, B, 2)
    xin, _ = _run_block(blk, x, dy)
    forward32 = _manual_block_grads(blk, x, dy, False)[2]
    ref, bound = _block_reference(blk, x, dy, forward32)
    got = {n: p.grad for n, p in blk.named_parameters()}
    got['dx'] = xin.grad
    worst = {}
    for n in ref:
        err = (got[n].double() - ref[n]).abs()
        assert bool((err <= bound[n]).all()), (n, float((err - bound[n]).max()))
        assert float(ref[n].abs().max()) > 0, n
        worst[n] = float((err / bound[n].clamp_min(1e-300)).max())
    if bg.KINDS[kind][2] == 2:
        off = torch.ones(x.shape[2:], dtype=torch.bool, device='cuda')
        off[::2, ::2] = False
        assert bool((xin.grad[:, :, off] == 0).all()) and bool((ref['dx'][:, :, off] == 0).all())
    print('\n%s gradients, worst fraction of the composed bound: %s' % (_CASE_ID(case), ', '.join('%s %.2e' % kv for kv in worst.items())))
    blk.zero_grad(set_to_none=True)


def test_block_backward_without_an_output_gradient_returns_none():
    """(f): set_materialize_grads(False) -- an output nothing reads arrives as None and every gradient is None, with no launch"""
    from tf_eager_object_detection_amd.model.extractor_trainable import _BlockTrainable

    class Ctx:
        layouts = [None] * 8

    assert _BlockTrainable.backward(Ctx(), None) == (None,) * 11
    Ctx.layouts = [None] * 6
    assert _BlockTrainable.backward(Ctx(), None) == (None,) * 9


# ---- (3) extractor_trainable, depth 50 ---------------------------------------------------------------------------------------------
IMAGE = (256, 352)                                                        # (test_neck_grad_gpu.test_caller_model_trains_its_neck's)


@pytest.fixture(scope='module')
def detector():
    from tf_eager_object_detection_amd.model.fpn_detector import ResNetFpnDetector
    torch.manual_seed(4)
    det = ResNetFpnDetector(50, 21, IMAGE, 1, dtype=torch.float32)
    return det.to(device='cuda', dtype=torch.float32, memory_format=torch.channels_last).eval()


def _image(rng):
    return torch.from_numpy((rng.uniform(0, 255, (1,) + IMAGE + (3,)) - 110).astype(np.float32)).cuda()


def _extractor_names(det):
    return [n for n, _ in det.named_parameters() if n.startswith(STAGES)]


def test_extractor_trainable_depth_50(detector):
    det = detector
    det.zero_grad(set_to_none=True)
    rng = np.random.default_rng(21)
    img = _image(rng)
    with torch.no_grad():
        want = det.extractor(img)
    outs = det.extractor_trainable(img)
    assert len(outs) == 4
    for o, o0 in zip(outs, want):
        assert o.requires_grad and o.shape == o0.shape and o.stride() == o0.stride() and _same_bits(o, o0)
    with torch.no_grad():                                                  # (no graph is recorded under no_grad, same bits)
        quiet = det.extractor_trainable(img)
    assert all(not q.requires_grad and _same_bits(q, o0) for q, o0 in zip(quiet, want))
    d_outs = [torch.from_numpy(rng.standard_normal(tuple(_nhwc(o).shape)).astype(np.float32)).cuda().permute(0, 3, 1, 2) for o in outs]
    torch.autograd.backward(outs, d_outs)
    names = _extractor_names(det)
    assert len(names) == 2 * (3 * 16 + 4) == 104
    params = dict(det.named_parameters())
    for n in names:
        g = params[n].grad
        assert g is not None and g.shape == params[n].shape and g.stride() == params[n].stride(), n
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, n
    assert sorted(n for n, p in params.items() if p.grad is not None) == sorted(names)
    assert params['conv1.weight'].grad is None and params['conv1.bias'].grad is None
    for attr, bad in (('f32_form', 'x3'), ('f32_form', 'x2'), ('dtype', torch.float16)):
        good = getattr(det, attr)
        setattr(det, attr, bad)
        try:
            with pytest.raises(ValueError, match='extractor_trainable needs'):
                det.extractor_trainable(img)
        finally:
            setattr(det, attr, good)
    det.zero_grad(set_to_none=True)


def test_extractor_backward_graph_capture_replays_bit_equal_to_eager(detector):
    """the whole pass -- sixteen blocks forward, then backward: 52 Dense weight gradients, 16 3x3 weight gradients with their reduce
    launches, the input gradients, 3 stride gathers and 15 joins -- captured on one stream and replayed on new contents"""
    det = detector
    det.zero_grad(set_to_none=True)
    rng = np.random.default_rng(22)
    img = _image(rng)
    names = _extractor_names(det)
    params = [dict(det.named_parameters())[n] for n in names]
    with torch.no_grad():
        shapes = [tuple(o.shape) for o in det.extractor(img)]
    draw = lambda: [torch.from_numpy(rng.standard_normal((s[0], s[2], s[3], s[1])).astype(np.float32)).cuda().permute(0, 3, 1, 2) for s in shapes]
    d_outs = draw()
    run = lambda: torch.autograd.grad(det.extractor_trainable(img), params, d_outs)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                   # (the kernels' one-time device set-up and the flipped weights: outside)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            got = run()
    torch.cuda.current_stream().wait_stream(side)
    img.copy_(_image(rng))
    for t, new in zip(d_outs, draw()):
        t.copy_(new)
    graph.replay()
    torch.cuda.synchronize()
    want = run()
    assert len(got) == 104 and all(_same_bits(a, b) for a, b in zip(got, want))
    assert all(float(g.abs().max()) > 0 for g in want)


# ---- (4) the caller model ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['torch', 'hip'])
def test_caller_model_trains_its_extractor(kind):
    """ResnetV1Fpn(train_extractor=True, train_neck=True, train_rpn_head=True, train_roi_head=True), both training branches: the four
    losses are bit-equal to the model without train_extractor, backward() leaves finite non-zero gradients on 132 parameters (28
    downstream of the extractor, bit-equal to that model's; 104 in conv2..conv5), conv1 has none, and one MomentumOptimizer step moves
    every conv2..conv5 parameter and leaves conv1 alone"""
    from tf_eager_object_detection_amd import training
    from tf_eager_object_detection_amd.model.base_fpn_model import ResnetV1Fpn
    kw = dict(depth=50, training_targets='hip', training_losses=kind, roi_training_total_num_samples=32, roi_training_max_pos_samples=8,
              train_neck=True, train_rpn_head=True, train_roi_head=True)
    torch.manual_seed(1)
    m = ResnetV1Fpn(train_extractor=True, **kw)
    with torch.no_grad():                                   # (spreads the fresh RpnHead's proposals over sizes and pyramid levels)
        b = m.dense.rpn_bbox.bias
        b.add_(torch.linspace(0.0, 1.6, b.numel(), device=b.device, dtype=b.dtype))
    plain = ResnetV1Fpn(**kw)
    plain._dense_ref.load_state_dict(m._dense_ref.state_dict())
    rng = np.random.default_rng(1)
    img = _image(rng)
    with torch.no_grad():
        p_list = m._neck(m._extractor(img, training=True), training=True)
        scores, deltas = m._get_fpn_head_results(p_list)
        rois = m._rpn_proposal((deltas, m._get_anchors(list(IMAGE)), m._fg_scores(scores), list(IMAGE)), training=True)
    big = rois[((rois[:, 2] - rois[:, 0]) >= 24) & ((rois[:, 3] - rois[:, 1]) >= 24)]
    assert big.shape[0] >= 3, 'the random model proposes fewer than 3 boxes of 24 pixels'
    gt = big[[0, big.shape[0] // 3, 2 * big.shape[0] // 3]].clone()
    gl = torch.tensor([3, 7, 12], device='cuda')
    losses = m((img, gt, gl), training=True)
    want = plain((img, gt, gl), training=True)
    assert len(losses) == 4 and all(x.requires_grad for x in losses)
    assert all(_same_bits(a, b) for a, b in zip(losses, want))                             # bit-equal to train_extractor=False
    assert all(torch.equal(a, b) for a, b in zip(m.im_detect(img, 1.0), plain.im_detect(img, 1.0)))
    sum(losses).backward()
    sum(want).backward()
    det = m.dense
    params, pparams = dict(det.named_parameters()), dict(plain.dense.named_parameters())
    ext = tuple(_extractor_names(det))
    down = NECK_NAMES + HEAD_NAMES + ROI_NAMES
    assert len(ext) == 104 and len(down) == 28
    assert sorted(n for n, p in params.items() if p.grad is not None) == sorted(ext + down)
    assert sorted(n for n, p in pparams.items() if p.grad is not None) == sorted(down)
    for n in ext + down:
        g = params[n].grad
        assert g.shape == params[n].shape and g.stride() == params[n].stride(), n
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, n
    for n in down:
        assert _same_bits(params[n].grad, pparams[n].grad), n
    assert params['conv1.weight'].grad is None and params['conv1.bias'].grad is None
    # one training step on what .backward() left, as it is
    named = training.model_variables(det)
    before = {n: p.detach().clone() for n, p in named}
    training.train_step(named, [p.grad for _, p in named], training.MomentumOptimizer(0.01, 0.9), learning_rate_bias_double=True,
                        weight_decays=training.l2_variables(det, 0.0001))
    for n, p in named:
        assert torch.equal(p.detach(), before[n]) == n.startswith('conv1.'), n
    with torch.no_grad():                                   # the next pass follows the stepped weights (derived tensors rebuilt)
        again = det.extractor(img)
    after = det.extractor_trainable(img)
    assert all(_same_bits(a, b) for a, b in zip(after, again))


def test_caller_model_constructor_errors():
    from tf_eager_object_detection_amd.model.base_fpn_model import ResnetV1Fpn
    with pytest.raises(ValueError, match='train_extractor=True needs train_neck=True'):
        ResnetV1Fpn(depth=50, train_extractor=True, train_rpn_head=True, train_roi_head=True)
    with pytest.raises(ValueError, match='train_extractor=True needs dtype'):
        ResnetV1Fpn(depth=50, train_extractor=True, train_neck=True, train_rpn_head=True, dtype=torch.float16)
    for form in ('x3', 'x2'):
        with pytest.raises(ValueError, match='train_extractor=True needs dtype'):
            ResnetV1Fpn(depth=50, train_extractor=True, train_neck=True, train_roi_head=True, f32_form=form)
