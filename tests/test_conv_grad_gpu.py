"""The float32 3x3 convolution backward on the GPU (csrc/conv_grad.hip: odet_conv3x3_wgrad_f32_levels; the input gradient on the
forward kernel; odet_rpn_unpack_pair) against the float64 statement of tests/conv_grad_np.py: exact on integer data, within the
any-order summation bound on random data, bit-equal between calls, behind torch.autograd (ops.conv3x3_trainable_levels), in the
FPN RpnHead (rpn_trainable) and the caller model (train_rpn_head), and under graph capture.

Worst observed fractions of bound (b) are printed by test_random_data_within_the_summation_bound and test_rpn_trainable; the table
is in DESIGN 3.15."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_grad_np as cg

pytestmark = pytest.mark.gpu

U = 2.0 ** -23
SINGLE = [(1, 1), (1, 5), (5, 1), (2, 2), (3, 7), (9, 33), (17, 40)]
PYRAMID = [(12, 20), (6, 10), (3, 5), (2, 3), (1, 2)]
HEAD_PYRAMID = [(16, 24), (8, 12), (4, 6), (2, 3), (1, 2)]              # the pyramid of a 64 x 96 image
CHANNELS = [(ci, co) for ci in (64, 96) for co in (64, 192)]
# (levels, batch, [(cin, cout), ...]): the grid of (a); the last two are the head's channels and one level the plan cuts
CASES = [([s], b, CHANNELS) for s in SINGLE for b in (1, 2)] + [(PYRAMID, b, CHANNELS) for b in (1, 2)] \
    + [(HEAD_PYRAMID, 1, [(256, 512)]), ([(23, 31)], 1, [(128, 128)])] \
    + [([(64, 65)], 1, [(64, 64)]), ([(50, 50), (41, 41)], 1, [(64, 64)])]       # from 4096 pixels on db takes its 256-phase form


def _ops():
    from tf_eager_object_detection_amd import ops
    return ops


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _id(case):
    shapes, b, chans = case
    return '%s-b%d%s' % ('+'.join('%dx%d' % s for s in shapes), b, '' if len(chans) > 1 else '-%dx%d' % chans[0])


def _run(xs, dys, ys, w):
    """(dw, db, [dx] or the ValueError of a dgrad the forward kernel does not take) as numpy"""
    ops = _ops()
    dxs, dds, dyy = [_dev(x) for x in xs], [_dev(d) for d in dys], None if ys is None else [_dev(y) for y in ys]
    dw, db = ops.conv3x3_wgrad_f32_levels(dxs, dds, dyy)
    dzs = [_dev(cg.masked_dy(d, y)) for d, y in zip(dys, ys or [None] * len(dys))]
    try:
        dx = [t.cpu().numpy() for t in ops.conv3x3_dgrad_f32_levels(dzs, _dev(w))]
    except ValueError as e:
        dx = e
    return dw.cpu().numpy(), db.cpu().numpy(), dx


def _equal64(got, want):
    return torch.equal(torch.from_numpy(np.ascontiguousarray(got)).double(), torch.from_numpy(np.ascontiguousarray(want)))


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_integer_data_is_exact(case):
    """(a): every product and partial sum is an integer far below 2^24, so any correct order gives the float64 result exactly"""
    shapes, B, chans = case
    K = B * sum(h * w for h, w in shapes)
    for cin, cout in chans:
        rng = np.random.default_rng(K * 1009 + cin * 7 + cout)
        xs = [rng.integers(-3, 4, (B, h, w, cin)) for h, w in shapes]
        dys = [rng.integers(-3, 4, (B, h, w, cout)) for h, w in shapes]
        ys = [rng.integers(-2, 3, (B, h, w, cout)) for h, w in shapes]        # zeros, negatives and positives
        w = rng.integers(-3, 4, (cout, 3, 3, cin))
        assert max(K * 9, 9 * cout * 9) < 2 ** 24
        for gated in (False, True):
            yy = ys if gated else None
            dw, db, dx = _run(xs, dys, yy, w)
            wdw, wdb = cg.wgrad(xs, dys, yy)
            assert _equal64(dw, wdw), ('dw', cin, cout, gated)
            assert _equal64(db, wdb), ('db', cin, cout, gated)
            if cin % 64:                                            # the forward's rules with the roles exchanged
                assert isinstance(dx, ValueError) and 'multiple of 64' in str(dx)
                continue
            want = cg.dgrad([cg.masked_dy(d, y) for d, y in zip(dys, yy or [None] * len(dys))], w)
            for g, t in zip(dx, want):
                assert _equal64(g, t), ('dx', cin, cout, gated)
    if len(shapes) > 1:                                             # a y_relu for SOME levels only, no bias gradient, a caller's tensor
        ops = _ops()
        mixed = [y if i % 2 else None for i, y in enumerate(ys)]
        out = torch.full((cout, 3, 3, cin), 7.0, device='cuda')
        dw2, none = ops.conv3x3_wgrad_f32_levels([_dev(x) for x in xs], [_dev(d) for d in dys], [_dev(y) for y in mixed],
                                                 with_bias=False, out=out)
        assert none is None and dw2 is out and _equal64(out.cpu().numpy(), cg.wgrad(xs, dys, mixed)[0])


def test_cut_and_whole_launches_are_under_test():
    """at least one case of (a) is cut into parts and one is not; a multi-part case with two images exists; the single level
    chosen from the plan is cut, and so is the case at the head's channels"""
    L = _ops().L
    cut = {}
    for shapes, B, chans in CASES:
        for cin, cout in chans:
            lv = (L.OdetConvGradLevel * len(shapes))()
            for i, (h, w) in enumerate(shapes):
                lv[i].H, lv[i].W = h, w
            got = int(L.lib().odet_conv3x3_wgrad_workspace_bytes(lv, len(shapes), B, cin, cout))
            parts = cg.plan(shapes, B, cin, cout)[1]
            assert got == (parts * cout * 9 * cin * 4 if parts > 1 else 0)
            cut[(tuple(shapes), B, cin, cout)] = parts
    assert any(p == 1 for p in cut.values()) and any(p > 1 for p in cut.values())
    assert any(p > 1 and k[1] == 2 for k, p in cut.items())
    assert any(p > 1 and k[1] == 2 and len(k[0]) > 1 for k, p in cut.items())          # the pyramid with two images
    assert cut[(((23, 31),), 1, 128, 128)] > 1 and cut[(tuple(HEAD_PYRAMID), 1, 256, 512)] > 1
    # 9 x 33 and 17 x 40: rows that straddle a K-step (32 pixels) and a part boundary
    for h, w in ((9, 33), (17, 40)):
        kper = cg.plan([(h, w)], 1, 64, 64)[2]
        assert cut[(((h, w),), 1, 64, 64)] > 1 and kper % w and 32 % w


def test_dense_wgrad_over_many_rows_is_exact():
    """the pair of 1x1 convolutions runs ops.dense_wgrad over all pixels: from 4096 rows on its bias sums take the 256-phase form
    (a row count no multiple of 256, gated and not)"""
    import dense_grad_np as dg
    ops = _ops()
    rng = np.random.default_rng(8)
    rows, cin, cout = 4100 + 37, 64, 64
    x, dy, y = rng.integers(-3, 4, (rows, cin)), rng.integers(-3, 4, (rows, cout)), rng.integers(-2, 3, (rows, cout))
    for yy in (None, y):
        dw, db = ops.dense_wgrad(_dev(dy), _dev(x), _dev(yy))
        wdw, wdb = dg.wgrad(dy, x, yy)
        assert _equal64(dw.cpu().numpy(), wdw) and _equal64(db.cpu().numpy(), wdb)


def _fraction(got, want, bound):
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= bound).all(), 'largest excess %g over a bound of %g' % ((err - bound).max(), bound.flat[(err - bound).argmax()])
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


RANDOM = [([(3, 7)], 2, 96, 64), ([(17, 40)], 2, 64, 192), (PYRAMID, 2, 64, 64), (HEAD_PYRAMID, 1, 256, 512)]


@pytest.mark.parametrize('case', RANDOM, ids=lambda c: _id((c[0], c[1], [c[2:]])))
def test_random_data_within_the_summation_bound(case):
    """(b): |got - want| <= K * 2^-23 * (|a| . |b|) per element, K the contraction length (B * sum H W for dw and db, 9 * cout for
    dx): the bound of a float32 sum of K rounded products in ANY order"""
    shapes, B, cin, cout = case
    K = B * sum(h * w for h, w in shapes)
    rng = np.random.default_rng(cin * 7919 + K)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    xs, dys, ys = [f(B, h, w, cin) for h, w in shapes], [f(B, h, w, cout) for h, w in shapes], [f(B, h, w, cout) for h, w in shapes]
    w = f(cout, 3, 3, cin)
    worst = {'dx': 0.0}
    for gated in (False, True):
        yy = ys if gated else None
        dw, db, dx = _run(xs, dys, yy, w)
        wdw, wdb = cg.wgrad(xs, dys, yy)
        adw, adb = cg.wgrad_abs(xs, dys, yy)
        worst['dw'] = max(worst.get('dw', 0.0), _fraction(dw, wdw, K * U * adw))
        worst['db'] = max(worst.get('db', 0.0), _fraction(db, wdb, K * U * adb))
        if cin % 64 == 0:
            dzs = [cg.masked_dy(d, y) for d, y in zip(dys, yy or [None] * len(dys))]
            for g, t, a in zip(dx, cg.dgrad(dzs, w), cg.dgrad_abs(dzs, w)):
                worst['dx'] = max(worst['dx'], _fraction(g, t, 9 * cout * U * a))
    print('\n%s: worst fraction of the bound  dx %.4f  dw %.4f  db %.4f' % (_id((shapes, B, [(cin, cout)])), worst['dx'], worst['dw'], worst['db']))


@pytest.mark.parametrize('case', [([(23, 31)], 1, 128, 128), (PYRAMID, 2, 64, 64)], ids=lambda c: _id((c[0], c[1], [c[2:]])))
def test_two_calls_are_bit_equal(case):
    """(c): a shape that is cut (its workspace holds whatever the allocator hands out) and the pyramid"""
    shapes, B, cin, cout = case
    rng = np.random.default_rng(5)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    xs, dys, ys = [f(B, h, w, cin) for h, w in shapes], [f(B, h, w, cout) for h, w in shapes], [f(B, h, w, cout) for h, w in shapes]
    w = f(cout, 3, 3, cin)
    a = _run(xs, dys, ys, w)
    junk = torch.full((1 << 22,), float('nan'), device='cuda')
    del junk
    b = _run(xs, dys, ys, w)
    for p, q in zip(a[:2] + tuple(a[2]), b[:2] + tuple(b[2])):
        assert np.array_equal(p.view(np.uint32), q.view(np.uint32))


def test_rpn_unpack_pair_is_the_index_map():
    """(d): by bytes; padding columns zero; A = 3, two levels, B = 2; and pack(unpack(g)) with a zero bias returns g"""
    ops = _ops()
    A, B, chp = 3, 2, 64
    pix = [(4, 5), (2, 3)]
    N = sum(h * w for h, w in pix) * A
    rng = np.random.default_rng(4)
    ds, dd = rng.standard_normal((B, N, 2)).astype(np.float32), rng.standard_normal((B, N, 4)).astype(np.float32)
    tds, tdd = _dev(ds), _dev(dd)
    s2, d2 = torch.full_like(tds, float('nan')), torch.full_like(tdd, float('nan'))
    off = 0
    for h, w in pix:
        out = torch.full((B * h * w, chp), float('nan'), device='cuda')
        ops.rpn_unpack_pair(tds, tdd, A, h * w, off, out)
        want = cg.unpack(ds, dd, A, h * w, off, chp)
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))
        assert (want[:, 6 * A:] == 0).all()
        ops.rpn_pack_pair(out[:, :6 * A].contiguous().view(B, h, w, 6 * A), torch.zeros(6 * A, device='cuda'), A, s2, d2, off)
        off += h * w * A
    assert torch.equal(s2, tds) and torch.equal(d2, tdd)


def _count_dgrad(monkeypatch):
    """counts the calls that an input gradient costs: the dgrad front (a launch of the forward kernel) and the flipped weight.
    The probe sees them because both backward passes resolve the two names through the ops MODULE at call time (module globals in
    ops.py, `ops.` attributes in model/rpn_trainable.py): a `from ..ops import ...` there would blind it -- the asserts on what
    backward returns (_spy_backward) would still hold"""
    ops = _ops()
    calls = {'dgrad': 0, 'flip': 0}
    dgrad, flip = ops.conv3x3_dgrad_f32_levels, ops.conv3x3_flipped_weight

    def spy_dgrad(*a, **k):
        calls['dgrad'] += 1
        return dgrad(*a, **k)

    def spy_flip(*a, **k):
        calls['flip'] += 1
        return flip(*a, **k)
    monkeypatch.setattr(ops, 'conv3x3_dgrad_f32_levels', spy_dgrad)
    monkeypatch.setattr(ops, 'conv3x3_flipped_weight', spy_flip)
    return calls


def _spy_backward(monkeypatch, cls):
    """records what every call of an autograd Function's backward RETURNS (the engine looks the method up on the class per call)"""
    seen, orig = [], cls.backward

    def spy(ctx, *grads):
        out = orig(ctx, *grads)
        seen.append(out)
        return out
    monkeypatch.setattr(cls, 'backward', staticmethod(spy))
    return seen


def test_conv3x3_trainable_levels_forward_and_backward(monkeypatch):
    """(e): forward = ops.conv3x3_f32_levels bit for bit; backward = the ops called by hand; no input gradient is computed (or
    returned) when no map needs one; the weight's gradient has the parameter's shape and memory format"""
    ops = _ops()
    rng = np.random.default_rng(9)
    cin, cout, B = 64, 128, 2
    shapes = [(6, 10), (3, 5)]
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).cuda()
    xs, dys = [f(B, h, w, cin) for h, w in shapes], [f(B, h, w, cout) for h, w in shapes]
    calls = _count_dgrad(monkeypatch)
    returned = _spy_backward(monkeypatch, ops._Conv3x3Trainable)
    for relu in (True, False):
        w = f(cout, cin, 3, 3).contiguous(memory_format=torch.channels_last).requires_grad_()
        b = f(cout).requires_grad_()
        ys = ops.conv3x3_trainable_levels(xs, w, b, relu=relu)
        want = ops.conv3x3_f32_levels(xs, w.detach(), b.detach(), relu=relu)
        assert all(torch.equal(y, t) and y.requires_grad for y, t in zip(ys, want))
        # what backward RETURNS for (weight, bias, relu, *maps) when no map needs a gradient: None in every map slot, and neither a
        # dgrad launch nor a flipped weight on the way
        before = dict(calls)
        torch.autograd.backward(ys, dys)
        got = returned[-1]
        assert len(got) == 3 + len(xs) and got[0] is not None and got[1] is not None and all(g is None for g in got[2:])
        assert calls == before, (calls, before)
        dw, db = ops.conv3x3_wgrad_f32_levels(xs, dys, [y.detach() for y in ys] if relu else None)
        assert torch.equal(got[0], w.grad) and torch.equal(got[1], b.grad)
        assert w.grad.shape == w.shape and w.grad.stride() == w.stride() and b.grad.shape == b.shape
        assert torch.equal(w.grad.permute(0, 2, 3, 1), dw) and torch.equal(b.grad, db)
        xg = [x.clone().requires_grad_() for x in xs[:1]] + xs[1:]                    # only the first map wants a gradient
        ys2 = ops.conv3x3_trainable_levels(xg, w, b, relu=relu)
        torch.autograd.backward(ys2, dys)
        got = returned[-1]
        assert got[3] is not None and got[4] is None            # one dgrad call; only the map that asked gets its result
        assert calls['dgrad'] == before['dgrad'] + 1
        dzs = [torch.where(y.detach() > 0, d, torch.zeros_like(d)) if relu else d for y, d in zip(ys2, dys)]
        assert torch.equal(xg[0].grad, ops.conv3x3_dgrad_f32_levels(dzs, w.detach())[0]) and xs[1].grad is None
    # an explicit [cout,3,3,cin] weight, a plain-contiguous [cout,cin,3,3] one, and a layer without a bias
    w2 = f(cout, 3, 3, cin).requires_grad_()
    torch.autograd.backward(ops.conv3x3_trainable_levels(xs, w2, None, relu=True), dys)
    assert w2.grad.shape == w2.shape and w2.grad.is_contiguous()
    w3 = w2.detach().permute(0, 3, 1, 2).contiguous().requires_grad_()
    torch.autograd.backward(ops.conv3x3_trainable_levels(xs, w3, None, relu=True), dys)
    assert w3.grad.is_contiguous() and torch.equal(w3.grad.permute(0, 2, 3, 1), w2.grad)
    with ops.f32_form('x3'):
        with pytest.raises(ValueError, match="only under f32_form 'exact'"):
            ops.conv3x3_trainable_levels(xs, w2, None)


# ---- (f) the head ----------------------------------------------------------------------------------------------------------------
HEAD_NAMES = ('rpn_conv.weight', 'rpn_conv.bias', 'rpn_score.weight', 'rpn_score.bias', 'rpn_bbox.weight', 'rpn_bbox.bias')


@pytest.fixture(scope='module')
def detector():
    from tf_eager_object_detection_amd.model.fpn_detector import ResNetFpnDetector
    torch.manual_seed(2)
    det = ResNetFpnDetector(50, 21, (64, 96), 1, dtype=torch.float32)
    det = det.to(device='cuda', dtype=torch.float32, memory_format=torch.channels_last).eval()
    with torch.no_grad():                                       # (the fresh head's weights of 0.01 / 0.001 would leave gradients near zero)
        for m in (det.rpn_conv, det.rpn_score, det.rpn_bbox):
            m.weight.mul_(5.0)
            m.bias.add_(torch.linspace(-0.2, 0.2, m.bias.numel(), device='cuda'))
    return det


def _maps(rng, B=1, shapes=HEAD_PYRAMID):
    return [torch.from_numpy(rng.standard_normal((B, 256, h, w)).astype(np.float32)).cuda().contiguous(memory_format=torch.channels_last)
            for h, w in shapes]


def _manual_rpn_grads(det, p_list, d_scores, d_deltas, with_dx=False):
    """the head's gradients from the kernels called by hand on the head's own float32 activations: what autograd must deliver,
    bit for bit"""
    from tf_eager_object_detection_amd.model.layers import rpn_pair_padded, rpn_pair_weights
    ops = _ops()
    A = det.A
    with torch.no_grad():
        xs = [p.permute(0, 2, 3, 1).contiguous() for p in p_list]
        B = xs[0].shape[0]
        hs = ops.conv3x3_f32_levels(xs, det.rpn_conv.weight, det.rpn_conv.bias, relu=True)
        h = torch.cat([t.reshape(-1, t.shape[3]) for t in hs], 0)
        wpad = rpn_pair_padded(det, rpn_pair_weights(det)[0])
        dpair, off = [], 0
        for t in hs:
            pix = t.shape[1] * t.shape[2]
            dpair.append(ops.rpn_unpack_pair(d_scores, d_deltas, A, pix, off, torch.empty((B * pix, 64), device='cuda')))
            off += pix * A
        dpair = torch.cat(dpair, 0)
        dwp, dbp = ops.dense_wgrad(dpair, h)
        dh = ops.dense_dgrad(dpair, wpad, x_relu=h)
        dhs, off = [], 0
        for t in hs:
            n = t.shape[0] * t.shape[1] * t.shape[2]
            dhs.append(dh[off:off + n].view(t.shape).contiguous())
            off += n
        dw3, db3 = ops.conv3x3_wgrad_f32_levels(xs, dhs)
        out = {'rpn_conv.weight': dw3.permute(0, 3, 1, 2), 'rpn_conv.bias': db3, 'rpn_score.weight': dwp[:2 * A].view(2 * A, -1, 1, 1),
               'rpn_score.bias': dbp[:2 * A], 'rpn_bbox.weight': dwp[2 * A:6 * A].view(4 * A, -1, 1, 1), 'rpn_bbox.bias': dbp[2 * A:6 * A]}
        if with_dx:
            out['dx'] = [g.permute(0, 3, 1, 2) for g in ops.conv3x3_dgrad_f32_levels(dhs, det.rpn_conv.weight)]
        out['h'] = hs
    return out


def _rpn_reference(det, p_list, hs, d_scores, d_deltas):
    """float64 torch autograd of the head on the same maps and output gradients -> ({name: gradient}, {name: bound}).  The ReLU
    gate is the float32 forward's own h > 0 (so no gate can fall the other way in the reference).  Bound (b) composed over the two
    layers (u = 2^-23; R = all pixels of all levels, the contraction length of every parameter gradient; |.| elementwise; a
    contraction of length K on operands with error bounds Ea, Eb: K u (|a| + Ea)(|b| + Eb) + Ea |b| + |a| Eb):
      forward   E1 = (K1 + 1) u (|x| * |W1| + |b1|), K1 = 9 cin: the float32 h is within E1 of the reference's
      pair      dW2: R u |dy|^T (|h| + E1) + |dy|^T E1;   db2: R u sum |dy|;   dh: D = K2 u |dy| |W2|, K2 = 64 (the padded rows)
      gate      dz = dh where h > 0: error Z = D under an open gate, 0 under a closed one
      3x3       dW1: R u (|dz| + Z) (*) |x| + Z (*) |x|  ((*): the weight gradient's sum over pixels and taps);
                db1: R u sum (|dz| + Z) + sum Z"""
    d = lambda t: t.detach().double()
    A = det.A
    params = dict(det.named_parameters())
    p = {n: d(params[n]).requires_grad_() for n in HEAD_NAMES}
    gates = [d(h > 0).permute(0, 3, 1, 2) for h in hs]
    xs = [d(x) for x in p_list]
    pres = [F.conv2d(x, p['rpn_conv.weight'], p['rpn_conv.bias'], padding=1) for x in xs]
    h64 = [pre * g for pre, g in zip(pres, gates)]
    B = xs[0].shape[0]
    s = torch.cat([F.conv2d(h, p['rpn_score.weight'], p['rpn_score.bias']).permute(0, 2, 3, 1).reshape(B, -1, 2) for h in h64], 1)
    t = torch.cat([F.conv2d(h, p['rpn_bbox.weight'], p['rpn_bbox.bias']).permute(0, 2, 3, 1).reshape(B, -1, 4) for h in h64], 1)
    for h in h64:
        h.retain_grad()
    torch.autograd.backward([s, t], [d(d_scores), d(d_deltas)])
    ref = {n: p[n].grad for n in HEAD_NAMES}
    with torch.no_grad():
        Ab = torch.abs
        W1, b1 = Ab(p['rpn_conv.weight']), Ab(p['rpn_conv.bias'])
        W2 = torch.cat([Ab(p['rpn_score.weight']), Ab(p['rpn_bbox.weight'])], 0).reshape(6 * A, -1)
        K1 = 9 * W1.shape[1]
        R = sum(x.shape[0] * x.shape[2] * x.shape[3] for x in xs)
        rows = lambda m: m.permute(0, 2, 3, 1).reshape(-1, m.shape[1])                       # [B,C,h,w] -> [pixels, C]
        off = 0
        bw2, bb2 = torch.zeros_like(W2), torch.zeros(6 * A, dtype=torch.float64, device=W2.device)
        ax, zsum, z = [], [], []
        for x, h, g in zip(xs, h64, gates):
            pix = x.shape[2] * x.shape[3]
            # the level's rows of the pair's output gradient: [B, pix A, 2] is [(image, pixel), (anchor, class)] = 2A pair channels
            dy = torch.cat([Ab(d(d_scores))[:, off:off + pix * A].reshape(-1, 2 * A),
                            Ab(d(d_deltas))[:, off:off + pix * A].reshape(-1, 4 * A)], 1)
            off += pix * A
            E1 = rows((K1 + 1) * U * F.conv2d(Ab(x), W1, b1, padding=1))
            hA = rows(Ab(h))
            bw2 += R * U * dy.T @ (hA + E1) + dy.T @ E1
            bb2 += R * U * dy.sum(0)
            D = 64 * U * dy @ W2
            Z = rows(g) * D
            ax.append(Ab(x).permute(0, 2, 3, 1).cpu().numpy())
            zsum.append((rows(Ab(h.grad * g)) + Z).reshape(x.shape[0], x.shape[2], x.shape[3], -1).cpu().numpy())
            z.append(Z.reshape(x.shape[0], x.shape[2], x.shape[3], -1).cpu().numpy())
        w_zs, b_zs = cg.wgrad(ax, zsum)
        w_z, b_z = cg.wgrad(ax, z)
        to = lambda a: torch.from_numpy(a).cuda()
        bw1 = (R * U * to(w_zs) + to(w_z)).permute(0, 3, 1, 2)
        bb1 = R * U * to(b_zs) + to(b_z)
        shape = p['rpn_score.weight'].shape[1:]
        bound = {'rpn_conv.weight': bw1, 'rpn_conv.bias': bb1, 'rpn_score.weight': bw2[:2 * A].reshape(2 * A, *shape),
                 'rpn_score.bias': bb2[:2 * A], 'rpn_bbox.weight': bw2[2 * A:].reshape(4 * A, *shape), 'rpn_bbox.bias': bb2[2 * A:]}
    return ref, bound


def _check_rpn_grads(det, p_list, hs, d_scores, d_deltas):
    ref, bound = _rpn_reference(det, p_list, hs, d_scores, d_deltas)
    worst = {}
    for n, p in det.named_parameters():
        if n not in ref:
            assert p.grad is None, n
            continue
        assert p.grad is not None and p.grad.shape == p.shape and p.grad.stride() == p.stride(), n
        err = (p.grad.double() - ref[n]).abs()
        assert bool((err <= bound[n]).all()), (n, float((err - bound[n]).max()))
        assert float(ref[n].abs().max()) > 0, n
        worst[n] = float((err / bound[n].clamp_min(1e-300)).max())
    print('\nRPN head gradients, worst fraction of the composed bound: %s' % ', '.join('%s %.2e' % kv for kv in worst.items()))


@pytest.mark.parametrize('batch', [1, 2])
def test_rpn_trainable(detector, batch, monkeypatch):
    det = detector
    calls = _count_dgrad(monkeypatch)
    from tf_eager_object_detection_amd.model.rpn_trainable import _RpnHeadTrainable
    returned = _spy_backward(monkeypatch, _RpnHeadTrainable)
    det.zero_grad(set_to_none=True)
    rng = np.random.default_rng(3 + batch)
    p_list = _maps(rng, batch)
    with torch.no_grad():
        s0, d0 = det.rpn(p_list)
    s, d = det.rpn_trainable(p_list)
    assert torch.equal(s, s0) and torch.equal(d, d0) and s.requires_grad and d.requires_grad
    ds = torch.from_numpy(rng.standard_normal(tuple(s.shape)).astype(np.float32)).cuda()
    dd = torch.from_numpy(rng.standard_normal(tuple(d.shape)).astype(np.float32)).cuda()
    # no map requires a gradient: backward returns None in every map slot (after the six parameters and the four constants)
    # and neither launches a dgrad nor builds the flipped weight -- in the forward or in the backward
    torch.autograd.backward([s, d], [ds, dd])
    got = returned[-1]
    assert len(got) == 10 + len(p_list) and all(g is not None for g in got[:6]) and all(g is None for g in got[6:])
    assert calls == {'dgrad': 0, 'flip': 0}, calls
    manual = _manual_rpn_grads(det, p_list, ds, dd)
    params = dict(det.named_parameters())
    for n in HEAD_NAMES:
        assert torch.equal(params[n].grad, manual[n]) and torch.equal(got[HEAD_NAMES.index(n)], manual[n]), n
    _check_rpn_grads(det, p_list, manual['h'], ds, dd)
    # maps that require a gradient get one: the forward kernel on the flipped weight, which the detector derives and caches
    det.zero_grad(set_to_none=True)
    pg = [p.clone().requires_grad_() if i in (0, 3) else p for i, p in enumerate(p_list)]
    s2, d2 = det.rpn_trainable(pg)
    assert torch.equal(s2, s0)
    n_dgrad = calls['dgrad']
    torch.autograd.backward([s2, d2], [ds, dd])
    assert [g is not None for g in returned[-1][10:]] == [True, False, False, True, False]
    assert calls['dgrad'] == n_dgrad + 1 and calls['flip'] <= 1                        # (the flipped weight is derived once, then cached)
    dx = _manual_rpn_grads(det, p_list, ds, dd, with_dx=True)['dx']
    assert torch.equal(pg[0].grad, dx[0]) and torch.equal(pg[3].grad, dx[3]) and pg[1].grad is None
    for n in HEAD_NAMES:
        assert torch.equal(params[n].grad, manual[n]), n
    with pytest.raises(ValueError, match='rpn_trainable needs'):
        det.f32_form = 'x3'
        try:
            det.rpn_trainable(p_list)
        finally:
            det.f32_form = 'exact'
    det.zero_grad(set_to_none=True)


# ---- (g) the caller model -----------------------------------------------------------------------------------------------------
ROI_NAMES = ('fc1.weight', 'fc1.bias', 'fc2.weight', 'fc2.bias', 'score.weight', 'score.bias', 'bbox.weight', 'bbox.bias')


@pytest.mark.parametrize('kind', ['torch', 'hip'])
def test_caller_model_trains_its_rpn_head(kind):
    """ResnetV1Fpn(train_rpn_head=True), both training branches, set up as tests/test_dense_grad_gpu.py sets up the RoI head's: the
    four losses are bit-equal to the model without the keyword, the RPN losses carry a graph into rpn_conv, rpn_score and rpn_bbox,
    one MomentumOptimizer step moves them and the derived tensors (the pair, its padded form) follow; with both keywords fourteen
    parameters get gradients"""
    from tf_eager_object_detection_amd import training
    from tf_eager_object_detection_amd.model.base_fpn_model import ResnetV1Fpn
    from tf_eager_object_detection_amd.model.fpn_detector import ResNetFpnDetector
    shape = (256, 352)
    kw = dict(depth=50, training_targets='hip', training_losses=kind, roi_training_total_num_samples=32, roi_training_max_pos_samples=8)
    torch.manual_seed(1)
    m = ResnetV1Fpn(train_rpn_head=True, **kw)
    with torch.no_grad():                                   # (spreads the fresh RpnHead's proposals over sizes and pyramid levels)
        b = m.dense.rpn_bbox.bias
        b.add_(torch.linspace(0.0, 1.6, b.numel(), device=b.device, dtype=b.dtype))
    plain = ResnetV1Fpn(**kw)
    plain._dense_ref.load_state_dict(m._dense_ref.state_dict())
    both = ResnetV1Fpn(train_rpn_head=True, train_roi_head=True, **kw)
    both._dense_ref.load_state_dict(m._dense_ref.state_dict())
    rng = np.random.default_rng(1)
    img = torch.from_numpy((rng.uniform(0, 255, (1,) + shape + (3,)) - 110).astype(np.float32)).cuda()
    with torch.no_grad():
        p_list = m._neck(m._extractor(img, training=True), training=True)
        scores, deltas = m._get_fpn_head_results(p_list)
        rois = m._rpn_proposal((deltas, m._get_anchors(list(shape)), m._fg_scores(scores), list(shape)), training=True)
    big = rois[((rois[:, 2] - rois[:, 0]) >= 24) & ((rois[:, 3] - rois[:, 1]) >= 24)]
    assert big.shape[0] >= 3, 'the random model proposes fewer than 3 boxes of 24 pixels'
    gt = big[[0, big.shape[0] // 3, 2 * big.shape[0] // 3]].clone()
    gl = torch.tensor([3, 7, 12], device='cuda')
    losses = m((img, gt, gl), training=True)
    want = plain((img, gt, gl), training=True)
    assert all(torch.equal(a.detach(), b) for a, b in zip(losses, want))                 # bit-equal to the path without the keyword
    assert not any(x.requires_grad for x in want)
    assert losses[0].requires_grad and losses[1].requires_grad and not losses[2].requires_grad and not losses[3].requires_grad
    (losses[0] + losses[1]).backward()
    det = m.dense
    assert sorted(n for n, p in det.named_parameters() if p.grad is not None) == sorted(HEAD_NAMES)
    params = dict(det.named_parameters())
    for n in HEAD_NAMES:
        g = params[n].grad
        assert g.shape == params[n].shape and g.stride() == params[n].stride() and float(g.abs().max()) > 0, n
    # one training step on what .backward() left, as it is
    named = [(n, p) for n, p in training.model_variables(det) if n in HEAD_NAMES]
    assert len(named) == 6
    before = {n: p.detach().clone() for n, p in named}
    training.train_step(named, [p.grad for _, p in named], training.MomentumOptimizer(0.01, 0.9), learning_rate_bias_double=True,
                        weight_decays=training.l2_variables(det, 0.0001))
    for n, p in named:
        assert not torch.equal(p.detach(), before[n]), n
    fresh = ResNetFpnDetector(50, 21, (64, 64), 1, dtype=torch.float32)
    fresh.to(device='cuda', dtype=torch.float32, memory_format=torch.channels_last).eval()
    fresh.load_state_dict(det.state_dict())
    pg = [p.clone().requires_grad_() for p in p_list]
    with torch.no_grad():
        s1, d1 = det.rpn(p_list)
        s2, d2 = fresh.rpn(p_list)
        s0, _ = plain._dense_ref.rpn(p_list)
    s3, d3 = det.rpn_trainable(pg)
    assert torch.equal(s1, s2) and torch.equal(d1, d2) and torch.equal(s1, s3) and torch.equal(d1, d3)
    assert not torch.equal(s1, s0)                                                         # (and the step did change the outputs)
    # the flipped weight: derived at the first pass whose maps want a gradient, kept, and rebuilt after a write to rpn_conv.weight
    ds, dd = torch.ones_like(s3), torch.ones_like(d3)
    g3 = torch.autograd.grad([s3, d3], pg, [ds, dd])
    s5, d5 = det.rpn_trainable(pg)
    g5 = torch.autograd.grad([s5, d5], pg, [ds, dd])
    manual = _manual_rpn_grads(det, p_list, ds, dd, with_dx=True)['dx']
    assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(g3, g5, manual))
    with torch.no_grad():
        det.rpn_conv.weight.mul_(2.0)
    s6, d6 = det.rpn_trainable(pg)
    g6 = torch.autograd.grad([s6, d6], pg, [ds, dd])
    manual = _manual_rpn_grads(det, p_list, ds, dd, with_dx=True)['dx']
    assert all(torch.equal(a, b) for a, b in zip(g6, manual)) and not torch.equal(g6[0], g3[0])
    # both heads together: fourteen parameters
    l4 = both((img, gt, gl), training=True)
    assert all(x.requires_grad for x in l4) and all(torch.equal(a.detach(), b) for a, b in zip(l4, want))
    sum(l4).backward()
    assert sorted(n for n, p in both.dense.named_parameters() if p.grad is not None) == sorted(HEAD_NAMES + ROI_NAMES)


def test_graph_capture_replays_bit_equal_to_eager(detector):
    """(h): the head's backward -- unpack, the pair's wgrad and dgrad, the 3x3 wgrad (cut: workspace and reduce launch captured
    too), its bias sums and the input gradient -- captured on one stream and replayed on new contents"""
    det = detector
    rng = np.random.default_rng(11)
    p_list = _maps(rng)
    n = sum(h * w for h, w in HEAD_PYRAMID) * det.A
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).cuda()
    ds, dd = f(1, n, 2), f(1, n, 4)
    keys = HEAD_NAMES + ('dx',)
    flat = lambda out: [t for k in keys for t in (out[k] if k == 'dx' else [out[k]])]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _manual_rpn_grads(det, p_list, ds, dd, with_dx=True)        # (the kernels' one-time device set-up happens outside the capture)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            got = flat(_manual_rpn_grads(det, p_list, ds, dd, with_dx=True))
    torch.cuda.current_stream().wait_stream(side)
    for t, new in zip(p_list + [ds, dd], _maps(rng) + [f(1, n, 2), f(1, n, 4)]):
        t.copy_(new)
    graph.replay()
    torch.cuda.synchronize()
    want = flat(_manual_rpn_grads(det, p_list, ds, dd, with_dx=True))
    assert all(torch.equal(a, b) for a, b in zip(got, want))
