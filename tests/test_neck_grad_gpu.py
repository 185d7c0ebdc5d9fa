"""The FPN neck's backward on the GPU: odet_fpn_topdown_backward_f32 (csrc/neck.hip) bit-equal to the float32 statement of
tests/neck_grad_np.py and bit-equal between calls, ops.fpn_topdown_backward's argument errors, ResNetFpnDetector.neck_trainable
(outputs bit-equal to neck(); gradients bit-equal to the ops called by hand, within the composed any-order summation bound of float64
torch autograd of the plain neck, exact on small integer data, with output gradients absent), the caller model with train_neck, and
the neck backward under graph capture.

Worst observed fractions of the composed bound are printed by test_neck_trainable_within_the_composed_bound; the table is in
DESIGN 3.16."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import neck_grad_np as ng

pytestmark = pytest.mark.gpu

U = 2.0 ** -23
NECK_NAMES = tuple('%s.%s' % (layer, part) for layer in ng.LAYERS for part in ('weight', 'bias'))
HEAD_NAMES = ('rpn_conv.weight', 'rpn_conv.bias', 'rpn_score.weight', 'rpn_score.bias', 'rpn_bbox.weight', 'rpn_bbox.bias')
ROI_NAMES = ('fc1.weight', 'fc1.bias', 'fc2.weight', 'fc2.bias', 'score.weight', 'score.bias', 'bbox.weight', 'bbox.bias')
EVEN_PYRAMID = [(16, 24), (8, 12), (4, 6), (2, 3)]                # the pyramid of a 64 x 96 image: every ratio exactly 2
ODD_PYRAMID = [(13, 21), (7, 11), (4, 6), (2, 3)]
CINS = (256, 512, 1024, 2048)


def _ops():
    from tf_eager_object_detection_amd import ops
    return ops


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ---- (a) the kernel against its statement ------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [4, 64, 256])
@pytest.mark.parametrize('top_hw,fine_hw', ng.CASES, ids=lambda c: '%dx%d' % tuple(c))
def test_kernel_is_bit_equal_to_the_statement(top_hw, fine_hw, C):
    """normal random data (every product rounds), B in {1, 2}, every combination of fine / base / sub, out_scale in {0.5, 1}; the
    output buffer starts as NaN: every element is written"""
    ops = _ops()
    h, w = top_hw
    H, W = fine_hw
    rng = np.random.default_rng(h * 1009 + W * 31 + C)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    for B in (1, 2):
        fine, base, sub = f(B, H, W, C), f(B, h, w, C), f(B, (h + 1) // 2, (w + 1) // 2, C)
        S = ng.tap_sum(fine, top_hw)
        dfine, dbase, dsub = _dev(fine), _dev(base), _dev(sub)
        for use in itertools.product((True, False), repeat=3):
            if not any(use):
                continue
            for scale in (0.5, 1.0):
                want = ng.topdown_backward(fine if use[0] else None, top_hw, base if use[1] else None, sub if use[2] else None,
                                           scale, S=S)
                out = torch.full((B, h, w, C), float('nan'), device='cuda')
                got = ops.fpn_topdown_backward(dfine if use[0] else None, top_hw, dbase if use[1] else None,
                                               dsub if use[2] else None, scale, out=out)
                assert got is out
                got = got.cpu().numpy()
                assert np.array_equal(got.view(np.int32), want.view(np.int32)), \
                    ('B %d fine/base/sub %s scale %s' % (B, use, scale), int((got.view(np.int32) != want.view(np.int32)).sum()))


# ---- (b) two calls, same bits ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('top_hw,fine_hw', [((25, 42), (50, 84)), ((13, 21), (25, 42)), ((9, 7), (4, 5))], ids=lambda c: '%dx%d' % tuple(c))
def test_two_calls_are_bit_equal(top_hw, fine_hw):
    """hundreds of workgroups, whose order of execution is free; fresh outputs"""
    ops = _ops()
    rng = np.random.default_rng(5)
    h, w = top_hw
    B, C = 2, 256
    fine = _dev(rng.standard_normal((B,) + fine_hw + (C,)))
    base = _dev(rng.standard_normal((B, h, w, C)))
    sub = _dev(rng.standard_normal((B, (h + 1) // 2, (w + 1) // 2, C)))
    a = ops.fpn_topdown_backward(fine, top_hw, base, sub, 0.5)
    junk = torch.full((B, h, w, C), 7.0, device='cuda')                         # (the allocator hands out other memory)
    b = ops.fpn_topdown_backward(fine, top_hw, base, sub, 0.5)
    assert _same_bits(a, b) and bool(torch.isfinite(a).all()) and junk is not None
    # and against the float64 transpose within (n + 4) u sum |terms|
    want = ng.resize_t(fine.cpu().numpy(), top_hw) + base.cpu().numpy().astype(np.float64)
    want[:, ::2, ::2] += sub.cpu().numpy()
    mag = ng.resize_t(fine.cpu().numpy(), top_hw, absolute=True) + np.abs(base.cpu().numpy())
    mag[:, ::2, ::2] += np.abs(sub.cpu().numpy())
    n = ng.tap_counts(top_hw, fine_hw)[None, :, :, None]
    assert (np.abs(a.cpu().numpy().astype(np.float64) - 0.5 * want) <= (n + 4) * U * 0.5 * mag).all()


def test_grid_stride_pass_is_bit_equal_to_the_statement():
    """more lanes (130 * 130 * 256 = 4.3 M) than the launch's 16384 workgroups of 256 hold, as the full-size P2 level has: the lanes
    of the second pass; a downscale from a tiny fine map keeps the statement's serial loop short"""
    ops = _ops()
    rng = np.random.default_rng(9)
    top_hw, B, C = (130, 130), 1, 1024
    assert B * top_hw[0] * top_hw[1] * (C // 4) > 16384 * 256
    fine = rng.standard_normal((B, 3, 4, C)).astype(np.float32)
    base = rng.standard_normal((B,) + top_hw + (C,)).astype(np.float32)
    want = ng.topdown_backward(fine, top_hw, base, None, 0.5)
    out = torch.full((B,) + top_hw + (C,), float('nan'), device='cuda')
    got = ops.fpn_topdown_backward(_dev(fine), top_hw, _dev(base), None, 0.5, out=out).cpu().numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


# ---- (c) the Python front's argument errors ---------------------------------------------------------------------------------------
def test_python_front_argument_errors():
    ops = _ops()
    z = lambda *s: torch.zeros(*s, device='cuda')
    fine, base, sub = z(1, 6, 10, 8), z(1, 3, 5, 8), z(1, 2, 3, 8)
    call = lambda **k: ops.fpn_topdown_backward(k.get('fine', fine), k.get('hw', (3, 5)), base=k.get('base', base), sub=k.get('sub', sub),
                                                out=k.get('out'))
    assert tuple(call().shape) == (1, 3, 5, 8)
    with pytest.raises(ValueError, match='at least one'):
        call(fine=None, base=None, sub=None)
    for name, t in (('fine', fine), ('base', base), ('sub', sub)):
        with pytest.raises(ValueError, match='float32'):
            call(**{name: t.half()})
        with pytest.raises(ValueError, match='float32'):
            call(**{name: t.double()})
        with pytest.raises(ValueError, match='GPU'):
            call(**{name: t.cpu()})
    for form in ('x3', 'x2'):
        with ops.f32_form(form):
            with pytest.raises(ValueError, match="only under f32_form 'exact'"):
                call()
    with pytest.raises(ValueError, match='contiguous'):
        call(fine=z(1, 6, 8, 10).permute(0, 1, 3, 2))
    with pytest.raises(ValueError, match='contiguous'):
        call(base=z(1, 8, 3, 5).permute(0, 2, 3, 1))                             # a channels-first map viewed as NHWC
    with pytest.raises(ValueError, match='contiguous'):
        call(sub=z(2, 3, 8))
    with pytest.raises(ValueError, match='multiple of 4'):
        call(fine=z(1, 6, 10, 6), base=None, sub=None)
    with pytest.raises(ValueError, match='positive'):
        call(hw=(3, 0))
    for bad in (dict(base=z(2, 3, 5, 8)), dict(base=z(1, 3, 5, 4)), dict(base=z(1, 4, 5, 8)), dict(sub=z(1, 1, 3, 8)),
                dict(sub=z(1, 2, 2, 8)), dict(sub=z(1, 2, 3, 4)), dict(fine=None, sub=z(2, 2, 3, 8))):
        with pytest.raises(ValueError, match='does not go with'):
            call(**bad)
    for out in (z(1, 3, 5, 4), z(1, 5, 3, 8), z(1, 3, 5, 8).half(), z(1, 3, 8, 5).permute(0, 1, 3, 2)):
        with pytest.raises(ValueError, match='out must be'):
            call(out=out)


# ---- (d) neck_trainable ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def detector():
    from tf_eager_object_detection_amd.model.fpn_detector import ResNetFpnDetector
    torch.manual_seed(4)
    det = ResNetFpnDetector(50, 21, (64, 96), 1, dtype=torch.float32)
    det = det.to(device='cuda', dtype=torch.float32, memory_format=torch.channels_last).eval()
    with torch.no_grad():                                       # (the fresh layers' biases are zero)
        for name in ng.LAYERS:
            b = getattr(det, name).bias
            b.add_(torch.linspace(-0.3, 0.3, b.numel(), device='cuda'))
    return det


def _c_maps(rng, B, shapes, integer=False):
    draw = (lambda s: (rng.random(s) < 1 / 16).astype(np.float32)) if integer else (lambda s: rng.standard_normal(s).astype(np.float32))
    return [torch.from_numpy(draw((B, c, h, w))).cuda().contiguous(memory_format=torch.channels_last) for (h, w), c in zip(shapes, CINS)]


def _out_shapes(shapes):
    h5, w5 = shapes[3]
    return list(shapes) + [((h5 + 1) // 2, (w5 + 1) // 2)]


def _d_outs(rng, B, shapes, integer=False):
    """gradients for P2..P6 as [B,256,h,w] tensors in NHWC memory"""
    draw = (lambda s: rng.integers(-1, 2, s) * (rng.random(s) < 1 / 16)) if integer else (lambda s: rng.standard_normal(s))
    return [_dev(draw((B, h, w, 256))).permute(0, 3, 1, 2) for h, w in _out_shapes(shapes)]


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _manual_neck_grads(det, cs, dps, with_dc=False):
    """the neck's gradients from the kernels called by hand, with freshly flipped weights: what autograd must deliver, bit for bit.
    dps: dP2..dP6 ([B,256,h,w]) or None -> {parameter name: gradient in the parameter's shape}, 'dc': [dC2..dC5 or None]"""
    from tf_eager_object_detection_amd.model.layers import _conv_epi
    ops = _ops()
    with torch.no_grad():
        c2, c3, c4, c5 = cs
        p5 = _conv_epi(det.p5, c5)
        m4 = det._lateral_merge(p5, det.l4, c4)
        m3 = det._lateral_merge(m4, det.l3, c3)
        m2 = det._lateral_merge(m3, det.l2, c2)
        out, dm = {}, {}
        for name, m, dp, half in (('s4', m4, dps[2], False), ('s3', m3, dps[1], False), ('s2', m2, dps[0], True)):
            if dp is None:
                continue
            conv = getattr(det, name)
            dw, db = ops.conv3x3_wgrad_f32_levels([_nhwc(m)], [_nhwc(dp)])
            out[name + '.weight'], out[name + '.bias'] = dw.permute(0, 3, 1, 2), db
            wf = ops.conv3x3_flipped_weight(conv.weight)
            dm[name] = ops.conv3x3_dgrad_f32_levels([_nhwc(dp)], conv.weight, flipped=wf * 0.5 if half else wf)[0]
        h = dm.get('s2')
        hs = {'l2': h}
        for lat, name, c in (('l3', 's3', c3), ('l4', 's4', c4)):
            if h is not None or name in dm:
                h = ops.fpn_topdown_backward(h, c.shape[2:], base=dm.get(name), out_scale=0.5)
            hs[lat] = h
        if h is not None or dps[3] is not None or dps[4] is not None:
            h = ops.fpn_topdown_backward(h, c5.shape[2:], base=None if dps[3] is None else _nhwc(dps[3]),
                                         sub=None if dps[4] is None else _nhwc(dps[4]), out_scale=1.0)
        hs['p5'] = h
        out['dc'] = []
        for name, c in (('l2', c2), ('l3', c3), ('l4', c4), ('p5', c5)):
            g, conv = hs[name], getattr(det, name)
            if g is None:
                out['dc'].append(None)
                continue
            dw, db = ops.dense_wgrad(g.view(-1, 256), _nhwc(c).view(-1, c.shape[1]))
            out[name + '.weight'], out[name + '.bias'] = dw.view(256, -1, 1, 1), db
            dx = ops.dense_dgrad(g.view(-1, 256), conv.weight.reshape(256, -1).contiguous()) if with_dc else None
            out['dc'].append(None if dx is None else dx.view(c.shape[0], c.shape[2], c.shape[3], -1).permute(0, 3, 1, 2))
        out['h'] = hs
    return out


def _backward(outs, dps):
    keep = [i for i, d in enumerate(dps) if d is not None]
    torch.autograd.backward([outs[i] for i in keep], [dps[i] for i in keep])


def _check_against_manual(det, cs, dps, with_dc):
    """forward bit-equal to neck() with its shapes and strides; backward bit-equal to the ops called by hand"""
    det.zero_grad(set_to_none=True)
    with torch.no_grad():
        want = det.neck(cs)
    xs = [c.clone().requires_grad_() for c in cs] if with_dc else cs
    outs = det.neck_trainable(xs)
    assert len(outs) == 5
    for o, o0 in zip(outs, want):
        assert o.requires_grad and o.shape == o0.shape and o.stride() == o0.stride() and _same_bits(o, o0)
    _backward(outs, dps)
    manual = _manual_neck_grads(det, cs, dps, with_dc)
    params = dict(det.named_parameters())
    for n in NECK_NAMES:
        g = params[n].grad
        if n not in manual:
            assert g is None, n
            continue
        assert g is not None and g.shape == params[n].shape and g.stride() == params[n].stride(), n
        assert _same_bits(g, manual[n]), n
    assert all(p.grad is None for n, p in params.items() if n not in NECK_NAMES)
    for x, dc in zip(xs, manual['dc']):
        if with_dc and dc is not None:
            assert x.grad is not None and _same_bits(x.grad, dc)
        else:
            assert x.grad is None
    return xs, manual


@pytest.mark.parametrize('with_dc', [False, True], ids=['params', 'params+dC'])
@pytest.mark.parametrize('batch', [1, 2])
@pytest.mark.parametrize('shapes', [EVEN_PYRAMID, ODD_PYRAMID], ids=['even', 'odd'])
def test_neck_trainable_is_bit_equal_to_the_ops_by_hand(detector, shapes, batch, with_dc):
    rng = np.random.default_rng(batch * 10 + len(shapes) + shapes[0][0])
    cs = _c_maps(rng, batch, shapes)
    _check_against_manual(detector, cs, _d_outs(rng, batch, shapes), with_dc)
    detector.zero_grad(set_to_none=True)


ABSENT = [(4,), (0, 1, 2, 3), (0,), (1, 2, 3, 4), (0, 1, 2), (3, 4), (1, 3)]


@pytest.mark.parametrize('absent', ABSENT, ids=lambda a: 'without_' + '_'.join('P%d' % (i + 2) for i in a))
def test_neck_trainable_with_output_gradients_absent(detector, absent):
    """an output nothing reads drops its terms: only dP6 (p5 alone trains), no dP2 (the finest merge backward has no `fine`), only
    dP2, ..."""
    rng = np.random.default_rng(sum(absent) + 40)
    cs = _c_maps(rng, 1, ODD_PYRAMID)
    dps = [None if i in absent else d for i, d in enumerate(_d_outs(rng, 1, ODD_PYRAMID))]
    _, manual = _check_against_manual(detector, cs, dps, True)
    got = sorted(n for n in NECK_NAMES if n in manual)
    if absent == (0, 1, 2, 3):
        assert got == ['p5.bias', 'p5.weight']
    if absent == (3, 4):
        assert len(got) == 14
    detector.zero_grad(set_to_none=True)


def _plain_neck(cs, P):
    from tf_eager_object_detection_amd.model.layers import tf_legacy_resize_bilinear as resize
    c2, c3, c4, c5 = cs
    lin = lambda x, n: F.conv2d(x, P[n + '.weight'], P[n + '.bias'])
    p5 = lin(c5, 'p5')
    m4 = 0.5 * resize(p5, c4.shape[2:]) + 0.5 * lin(c4, 'l4')
    m3 = 0.5 * resize(m4, c3.shape[2:]) + 0.5 * lin(c3, 'l3')
    m2 = 0.5 * resize(m3, c2.shape[2:]) + 0.5 * lin(c2, 'l2')
    conv = lambda m, n: F.conv2d(m, P[n + '.weight'], P[n + '.bias'], padding=1)
    return (conv(m2, 's2'), conv(m3, 's3'), conv(m4, 's4'), p5, p5[:, :, ::2, ::2]), (m2, m3, m4, p5)


def _neck_reference(det, cs, dps, with_bound=True):
    """float64 torch autograd of the plain neck (tf_legacy_resize_bilinear + F.conv2d) on the same float32 maps, parameters and output
    gradients -> ({name: gradient, 'dc': [...]}, the same keys' bounds).  The any-order summation bound of DESIGN 3.15(b) composed
    over the layers (u = 2^-23; |.| elementwise; a contraction of length K on operands with error bounds Ea, Eb:
    K u (|a| + Ea)(|b| + Eb) + Ea |b| + |a| Eb; R(.) the resize and Rt(.) its transpose, both with non-negative weights, so they
    carry bounds; T4(.) the SUM of a fine pixel's four tapped values):
      forward   p5: E5 = (K + 1) u (|C5| |W|^T + |b|), K = 2048; a lateral l_k alike with K = C_k's channels: El_k
                m_k = 0.5 up + 0.5 lat: Em_k = 0.5 R(E_top) + 0.5 El_k + 8 u (0.5 T4(|top|) + 0.5 (|C_k| |W|^T + |b|))
                (the lerps' six roundings and the two halves' add, on magnitudes no larger than the taps' sum)
      s_k       dW: R_k u |dP_k| (*) (|m_k| + Em_k) + |dP_k| (*) Em_k, R_k = B H_k W_k pixels ((*): the weight gradient's sum over
                pixels and taps); db: R_k u sum |dP_k|; input gradient: Ds_k = 9 * 256 u |dP_k| (conv) |W_flipped|
      cascade   h2 = 0.5 dgrad_s2 (exact halving): Eh_2 = 0.5 Ds_2
                h_k = 0.5 (dgrad_sk + Rt(h_k-1)): Eh_k = 0.5 (Ds_k + Rt(Eh_k-1)) + (n + 4) u 0.5 (|dgrad_sk| + Rt(|h_k-1| + Eh_k-1)),
                n = the taps that land on the coarse pixel (each adds one rounded sum; + 4: the two weights' 1 - l, the two
                products, the other terms' adds and the scale)
                g5 = dP5 + dP6 placed + Rt(h4): Eg = Rt(Eh_4) + (n + 4) u (|dP5| + |dP6 placed| + Rt(|h4| + Eh_4))
      1x1       dW: R_k u (|h| + Eh)^T |C| + Eh^T |C|; db: R_k u sum (|h| + Eh) + sum Eh; dC: 256 u (|h| + Eh) |W| + Eh |W|"""
    from tf_eager_object_detection_amd.model.layers import tf_legacy_resize_bilinear as resize
    d = lambda t: t.detach().double()
    params = dict(det.named_parameters())
    P = {n: d(params[n]).contiguous().requires_grad_() for n in NECK_NAMES}
    xs = [d(c).contiguous().requires_grad_() for c in cs]
    outs, (m2, m3, m4, p5) = _plain_neck(xs, P)
    keep = [i for i, g in enumerate(dps) if g is not None]
    torch.autograd.backward([outs[i] for i in keep], [d(dps[i]).contiguous() for i in keep])
    ref = {n: P[n].grad for n in NECK_NAMES}
    ref['dc'] = [x.grad for x in xs]
    if not with_bound:
        return ref, None
    with torch.no_grad():
        Ab = torch.abs
        B = xs[0].shape[0]
        zeros = lambda i: torch.zeros((B, 256) + tuple(_out_shapes([tuple(c.shape[2:]) for c in cs])[i]), dtype=torch.float64, device='cuda')
        dP = [zeros(i) if g is None else d(g) for i, g in enumerate(dps)]
        lin_abs = lambda x, n: F.conv2d(Ab(x), Ab(P[n + '.weight']), Ab(P[n + '.bias']))

        def rt(x, top_hw):
            with torch.enable_grad():
                z = torch.zeros(x.shape[:2] + tuple(top_hw), dtype=torch.float64, device='cuda', requires_grad=True)
                return torch.autograd.grad(resize(z, x.shape[2:]), z, x)[0]

        def t4(x, out_hw):
            y0, y1, x0, x1 = [torch.from_numpy(i).cuda() for i in ng.axis_taps(x.shape[2], out_hw[0])[:2] + ng.axis_taps(x.shape[3], out_hw[1])[:2]]
            rows = x[:, :, y0] + x[:, :, y1]
            return rows[:, :, :, x0] + rows[:, :, :, x1]

        def wg_abs(dy, x):
            unf = F.unfold(x, 3, padding=1)                                           # [B, C * 9, pixels]
            return torch.einsum('bol,bkl->ok', dy.reshape(B, dy.shape[1], -1), unf).reshape(dy.shape[1], x.shape[1], 3, 3)

        bound = {}
        Etop, top = (2048 + 1) * U * lin_abs(xs[3], 'p5'), p5
        Em = {}
        for k, (lat, c, m) in enumerate((('l4', xs[2], m4), ('l3', xs[1], m3), ('l2', xs[0], m2))):
            la = lin_abs(c, lat)
            hw = c.shape[2:]
            Em[lat] = 0.5 * resize(Etop, hw) + 0.5 * (c.shape[1] + 1) * U * la + 8 * U * (0.5 * t4(Ab(top), hw) + 0.5 * la)
            Etop, top = Em[lat], m
        Ds, dg = {}, {}
        for name, lat, m, g in (('s2', 'l2', m2, dP[0]), ('s3', 'l3', m3, dP[1]), ('s4', 'l4', m4, dP[2])):
            Rk = B * m.shape[2] * m.shape[3]
            bound[name + '.weight'] = Rk * U * wg_abs(Ab(g), Ab(m) + Em[lat]) + wg_abs(Ab(g), Em[lat])
            bound[name + '.bias'] = Rk * U * Ab(g).sum((0, 2, 3))
            wf = P[name + '.weight'].flip(2, 3).transpose(0, 1)
            dg[name] = F.conv2d(g, wf, padding=1)
            Ds[name] = 9 * 256 * U * F.conv2d(Ab(g), Ab(wf), padding=1)
        h, Eh = 0.5 * dg['s2'], 0.5 * Ds['s2']
        hs = {'l2': (h, Eh)}
        for lat, name, c, cf in (('l3', 's3', xs[1], xs[0]), ('l4', 's4', xs[2], xs[1])):
            hw = tuple(c.shape[2:])
            n = torch.from_numpy(ng.tap_counts(hw, tuple(cf.shape[2:]))).cuda().double()[None, None]
            Eh = 0.5 * (Ds[name] + rt(Eh, hw)) + (n + 4) * U * 0.5 * (Ab(dg[name]) + rt(Ab(h) + Eh, hw))
            h = 0.5 * (dg[name] + rt(h, hw))
            hs[lat] = (h, Eh)
        hw = tuple(xs[3].shape[2:])
        n = torch.from_numpy(ng.tap_counts(hw, tuple(xs[2].shape[2:]))).cuda().double()[None, None]
        placed = torch.zeros_like(dP[3])
        placed[:, :, ::2, ::2] = dP[4]
        Eh = rt(Eh, hw) + (n + 4) * U * (Ab(dP[3]) + Ab(placed) + rt(Ab(h) + Eh, hw))
        h = dP[3] + placed + rt(h, hw)
        hs['p5'] = (h, Eh)
        bound['dc'] = []
        for name, c in (('l2', xs[0]), ('l3', xs[1]), ('l4', xs[2]), ('p5', xs[3])):
            h, Eh = hs[name]
            Rk = B * c.shape[2] * c.shape[3]
            W = Ab(P[name + '.weight']).reshape(256, -1)
            bw = Rk * U * torch.einsum('bohw,bihw->oi', Ab(h) + Eh, Ab(c)) + torch.einsum('bohw,bihw->oi', Eh, Ab(c))
            bound[name + '.weight'] = bw.reshape(256, -1, 1, 1)
            bound[name + '.bias'] = Rk * U * (Ab(h) + Eh).sum((0, 2, 3)) + Eh.sum((0, 2, 3))
            bound['dc'].append(256 * U * torch.einsum('bohw,oi->bihw', Ab(h) + Eh, W) + torch.einsum('bohw,oi->bihw', Eh, W))
    return ref, bound


@pytest.mark.parametrize('batch', [1, 2])
@pytest.mark.parametrize('shapes', [EVEN_PYRAMID, ODD_PYRAMID], ids=['even', 'odd'])
def test_neck_trainable_within_the_composed_bound(detector, shapes, batch):
    det = detector
    det.zero_grad(set_to_none=True)
    rng = np.random.default_rng(batch * 100 + shapes[0][0])
    cs = [c.requires_grad_() for c in _c_maps(rng, batch, shapes)]
    dps = _d_outs(rng, batch, shapes)
    _backward(det.neck_trainable(cs), dps)
    ref, bound = _neck_reference(det, cs, dps)
    params = dict(det.named_parameters())
    worst = {}
    for n in NECK_NAMES:
        err = (params[n].grad.double() - ref[n]).abs()
        assert bool((err <= bound[n]).all()), (n, float((err - bound[n]).max()))
        assert float(ref[n].abs().max()) > 0, n
        worst[n] = float((err / bound[n].clamp_min(1e-300)).max())
    for i, (c, r, b) in enumerate(zip(cs, ref['dc'], bound['dc'])):
        err = (c.grad.double() - r).abs()
        assert bool((err <= b).all()), ('dC%d' % (i + 2), float((err - b).max()))
        worst['dC%d' % (i + 2)] = float((err / b.clamp_min(1e-300)).max())
    print('\nneck gradients, worst fraction of the composed bound: %s' % ', '.join('%s %.2e' % kv for kv in worst.items()))
    det.zero_grad(set_to_none=True)


@pytest.mark.parametrize('batch', [1, 2])
def test_neck_trainable_is_exact_on_small_integer_data(detector, batch):
    """sparse data in {-1, 0, 1} on the pyramid whose ratios are exactly 2 (resize weights in {0, 1/4, 1/2, 3/4, 1}): every value is
    a dyadic rational with at most 15 fractional bits (three merges of 1/2 * 1/16) and a magnitude far below 2^9, so every partial
    sum has fewer than 24 significant bits and the float32 gradients equal the float64 reference's exactly"""
    det = detector
    rng = np.random.default_rng(batch + 70)
    params = dict(det.named_parameters())
    saved = {n: params[n].detach().clone() for n in NECK_NAMES}
    try:
        with torch.no_grad():
            for n in NECK_NAMES:
                p = params[n]
                dens = 1 / 8 if n.endswith('bias') else (1 / 128 if p.shape[2] == 3 else 1 / 32)
                p.copy_(torch.from_numpy((rng.integers(-1, 2, tuple(p.shape)) * (rng.random(tuple(p.shape)) < dens)).astype(np.float32)).cuda())
        det.zero_grad(set_to_none=True)
        cs = [c.requires_grad_() for c in _c_maps(rng, batch, EVEN_PYRAMID, integer=True)]
        dps = _d_outs(rng, batch, EVEN_PYRAMID, integer=True)
        _backward(det.neck_trainable(cs), dps)
        ref, _ = _neck_reference(det, cs, dps, with_bound=False)
        for n in NECK_NAMES:
            assert float(ref[n].abs().max()) > 0, n
            assert torch.equal(params[n].grad.double(), ref[n]), (n, float((params[n].grad.double() - ref[n]).abs().max()))
        for i, (c, r) in enumerate(zip(cs, ref['dc'])):
            assert float(r.abs().max()) > 0 and torch.equal(c.grad.double(), r), 'dC%d' % (i + 2)
    finally:
        with torch.no_grad():
            for n in NECK_NAMES:
                params[n].copy_(saved[n])
        det.zero_grad(set_to_none=True)


def test_neck_trainable_refuses_other_forms(detector):
    det = detector
    cs = _c_maps(np.random.default_rng(0), 1, EVEN_PYRAMID)
    for attr, bad in (('f32_form', 'x3'), ('f32_form', 'x2'), ('dtype', torch.float16)):
        good = getattr(det, attr)
        setattr(det, attr, bad)
        try:
            with pytest.raises(ValueError, match='neck_trainable needs'):
                det.neck_trainable(cs)
        finally:
            setattr(det, attr, good)


# ---- (e) the caller model -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['torch', 'hip'])
def test_caller_model_trains_its_neck(kind):
    """ResnetV1Fpn(train_neck=True, train_rpn_head=True, train_roi_head=True), both training branches: the four losses are bit-equal
    to the model without train_neck, backward() leaves finite non-zero gradients on 28 parameters (14 in the heads, 14 in the neck), one
    MomentumOptimizer step moves the neck's parameters and the next pass follows (the derived flipped weights are rebuilt)"""
    from tf_eager_object_detection_amd import training
    from tf_eager_object_detection_amd.model.base_fpn_model import ResnetV1Fpn
    shape = (256, 352)
    kw = dict(depth=50, training_targets='hip', training_losses=kind, roi_training_total_num_samples=32, roi_training_max_pos_samples=8,
              train_rpn_head=True, train_roi_head=True)
    torch.manual_seed(1)
    m = ResnetV1Fpn(train_neck=True, **kw)
    with torch.no_grad():                                   # (spreads the fresh RpnHead's proposals over sizes and pyramid levels)
        b = m.dense.rpn_bbox.bias
        b.add_(torch.linspace(0.0, 1.6, b.numel(), device=b.device, dtype=b.dtype))
    plain = ResnetV1Fpn(**kw)
    plain._dense_ref.load_state_dict(m._dense_ref.state_dict())
    rng = np.random.default_rng(1)
    img = torch.from_numpy((rng.uniform(0, 255, (1,) + shape + (3,)) - 110).astype(np.float32)).cuda()
    with torch.no_grad():
        c_list = m._extractor(img, training=True)
        p_list = m._neck(c_list, training=True)
        scores, deltas = m._get_fpn_head_results(p_list)
        rois = m._rpn_proposal((deltas, m._get_anchors(list(shape)), m._fg_scores(scores), list(shape)), training=True)
    big = rois[((rois[:, 2] - rois[:, 0]) >= 24) & ((rois[:, 3] - rois[:, 1]) >= 24)]
    assert big.shape[0] >= 3, 'the random model proposes fewer than 3 boxes of 24 pixels'
    gt = big[[0, big.shape[0] // 3, 2 * big.shape[0] // 3]].clone()
    gl = torch.tensor([3, 7, 12], device='cuda')
    losses = m((img, gt, gl), training=True)
    want = plain((img, gt, gl), training=True)
    assert len(losses) == 4 and all(x.requires_grad for x in losses)
    assert all(_same_bits(a, b) for a, b in zip(losses, want))                             # bit-equal to train_neck=False
    # inference and the no-training paths do not change either
    assert all(torch.equal(a, b) for a, b in zip(m.im_detect(img, 1.0), plain.im_detect(img, 1.0)))
    sum(losses).backward()
    det = m.dense
    params = dict(det.named_parameters())
    assert sorted(n for n, p in params.items() if p.grad is not None) == sorted(NECK_NAMES + HEAD_NAMES + ROI_NAMES)
    for n in NECK_NAMES + HEAD_NAMES + ROI_NAMES:
        g = params[n].grad
        assert g.shape == params[n].shape and g.stride() == params[n].stride(), n
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, n
    # the plain model's 14 head gradients come from the same losses without the neck's graph: the heads' own gradients agree
    sum(want).backward()
    pparams = dict(plain.dense.named_parameters())
    assert sorted(n for n, p in pparams.items() if p.grad is not None) == sorted(HEAD_NAMES + ROI_NAMES)
    for n in HEAD_NAMES + ROI_NAMES:
        assert _same_bits(params[n].grad, pparams[n].grad), n
    # one training step on what .backward() left in the neck, as it is
    cs = [c.detach() for c in c_list]
    dps = _d_outs(np.random.default_rng(2), 1, [tuple(c.shape[2:]) for c in cs])
    before_out = [o.detach().clone() for o in det.neck_trainable(cs)]
    named = [(n, p) for n, p in training.model_variables(det) if n in NECK_NAMES]
    assert len(named) == 14
    before = {n: p.detach().clone() for n, p in named}
    training.train_step(named, [p.grad for _, p in named], training.MomentumOptimizer(0.01, 0.9), learning_rate_bias_double=True,
                        weight_decays=training.l2_variables(det, 0.0001))
    for n, p in named:
        assert not torch.equal(p.detach(), before[n]), n
    after_out = det.neck_trainable(cs)
    with torch.no_grad():
        again = det.neck(cs)
    assert all(_same_bits(a, b) for a, b in zip(after_out, again))
    assert not any(torch.equal(a, b) for a, b in zip(after_out[:4], before_out[:4]))        # (the step did change every level)
    det.zero_grad(set_to_none=True)
    _backward(after_out, dps)
    manual = _manual_neck_grads(det, cs, dps)                                              # (flips the stepped weights afresh)
    for n in NECK_NAMES:
        assert _same_bits(params[n].grad, manual[n]), n


def test_caller_model_constructor_errors():
    from tf_eager_object_detection_amd.model.base_fpn_model import ResnetV1Fpn
    with pytest.raises(ValueError, match='train_neck'):
        ResnetV1Fpn(depth=50, train_neck=True)
    with pytest.raises(ValueError, match='train_neck'):
        ResnetV1Fpn(depth=50, train_neck=True, train_rpn_head=True, dtype=torch.float16)
    for form in ('x3', 'x2'):
        with pytest.raises(ValueError, match='train_neck'):
            ResnetV1Fpn(depth=50, train_neck=True, train_roi_head=True, f32_form=form)


# ---- (f) graph capture ----------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_bit_equal_to_eager(detector):
    """the neck backward -- three 3x3 weight gradients with their reduce launches, three input gradients, three merge backwards, four
    Dense weight gradients and input gradients -- captured on one stream and replayed on new contents"""
    det = detector
    rng = np.random.default_rng(13)
    cs = _c_maps(rng, 1, ODD_PYRAMID)
    dps = _d_outs(rng, 1, ODD_PYRAMID)
    flat = lambda out: [out[n] for n in NECK_NAMES] + out['dc']
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _manual_neck_grads(det, cs, dps, with_dc=True)              # (the kernels' one-time device set-up happens outside the capture)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            got = flat(_manual_neck_grads(det, cs, dps, with_dc=True))
    torch.cuda.current_stream().wait_stream(side)
    for t, new in zip(cs + dps, _c_maps(rng, 1, ODD_PYRAMID) + _d_outs(rng, 1, ODD_PYRAMID)):
        t.copy_(new)
    graph.replay()
    torch.cuda.synchronize()
    want = flat(_manual_neck_grads(det, cs, dps, with_dc=True))
    assert all(_same_bits(a, b) for a, b in zip(got, want))
