"""The split-precision backward on the GPU (csrc/grad_gemm.h: dg_tile_x3 behind odet_dense_dgrad_x3, odet_dense_wgrad_x3 and
odet_conv3x3_wgrad_x3_levels; ops.grad_form('x3')): exact by bytes on data whose six kept limb products sum exactly in any order,
the dropped-product witness through the bare ops and through autograd's own thread, random data against float64 within
(6 K + 1) * 2^-23 * (|a| . |b|) and against the exact form's error, bit-equal repeats, short workspaces, graph capture, the 3x3
input gradient on the forward's split-precision kernel, and the three caller models.

Worst observed on an MI355X (printed by the random-data tests; the table is in DESIGN 3.21): fraction of the bound dx 0.0042,
dw 0.1005 (3 rows), conv dw 0.0153; max error / rms at most 3.03e-06 (x3) beside 2.82e-06 (exact).  The parts against 7 x the exact
form's composed bounds: RoI head at most 4.2e-03 of it (bbox.bias), RpnHead 3.2e-04, neck 3.0e-03 (s4.bias).

The data and its proofs: tests/grad_x3_cases.py, tests/test_grad_x3_host.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import conv_grad_np as cg
import dense_grad_np as dg
import exact_data as ed
import grad_x3_cases as gx

pytestmark = pytest.mark.gpu
U = gx.U


def _ops():
    from tf_eager_object_detection_amd import ops
    return ops


def _gpu(t):
    return None if t is None else gx.f32(t).cuda()


def _np(t):
    return None if t is None else t.numpy()


def _bits_equal(got, want64):
    """a float32 GPU result equals a float64 statement by bytes (the statement is a float32 value; -0.0 and +0.0 both stand for 0)"""
    return torch.equal(got.detach().cpu().double(), torch.as_tensor(want64))


def _dense_both(ops, form, a_w, b_w, a_d, b_d, y, xr):
    """wgrad on (x = a_w [rows][cin], dy = b_w [rows][cout]) and dgrad on (w = a_d [cout][cin], dy = b_d^T), gated by y / xr"""
    with ops.grad_form(form):
        dw, db = ops.dense_wgrad(_gpu(b_w), _gpu(a_w), _gpu(y))
        dx = ops.dense_dgrad(_gpu(b_d.t().contiguous()), _gpu(a_d), _gpu(y), _gpu(xr))
    return dw, db, dx


# ---- 1. exact by bytes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', gx.DENSE_SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_dense_is_exact_by_bytes(shape):
    """integer data and the three limb-sensitive kinds, each with gates of +0.0, -0.0, negative, tiny and plain positive values
    on dy (both ops) and on dgrad's epilogue; split launches included (HEAD)"""
    ops = _ops()
    rows, cin, cout = shape
    g = ed.Gen(rows * 1000003 + cin * 1009 + cout)
    y, xr = gx.gates(g, (rows, cout)), gx.gates(g, (rows, cin))
    for kind in ('integers',) + gx.LIMB_KINDS:
        make = gx.integer_operands if kind == 'integers' else (lambda g_, K, M, N: gx.limb_operands(g_, kind, K, M, N))
        a_w, b_w, _ = make(g, rows, cin, cout)                  # wgrad: K = rows
        a_d, b_d, _ = make(g, cout, cin, rows)                  # dgrad: K = cout
        for gated in (True, False):
            yy, xx = (y, xr) if gated else (None, None)
            dw, db, dx = _dense_both(ops, 'x3', a_w, b_w, a_d, b_d, yy, xx)
            wdw, wdb = dg.wgrad(_np(b_w), _np(a_w), _np(yy))
            assert _bits_equal(dw, wdw), (kind, gated, 'dw')
            assert _bits_equal(dx, dg.dgrad(_np(b_d.t().contiguous()), _np(a_d), _np(yy), _np(xx))), (kind, gated, 'dx')
            if kind == 'integers':
                assert _bits_equal(db, wdb), (kind, gated, 'db')


def _conv_case_data(g, kind, case):
    maps, batch, cin, cout = case
    K = gx.conv_pixels(maps, batch)
    if kind == 'integers':
        a, b = g.ints((K, cin), 8), g.ints((K, cout), 4)
        assert 9 * K * 32 < 2 ** 24
    else:                                                        # (a tap's sum has at most the four non-zero dz of its channel: the
        a, b, _ = gx.limb_operands(g, kind, K, cin, cout)        # proof of the centre tap holds for every tap)
    return gx.conv_maps(a, maps, batch), gx.conv_maps(b, maps, batch)


@pytest.mark.parametrize('case', gx.CONV_CASES, ids=lambda c: '%s-b%d-%dto%d' % ('x'.join('%d.%d' % s for s in c[0]), c[1], c[2], c[3]))
def test_conv_wgrad_is_exact_by_bytes(case):
    ops = _ops()
    maps, batch, cin, cout = case
    g = ed.Gen(7 + cin * 31 + cout + batch * 1013 + sum(h * 131 + w for h, w in maps))
    ys = [gx.gates(g, (batch, h, w, cout)) for h, w in maps]
    for kind in ('integers',) + gx.LIMB_KINDS:
        xs, dys = _conv_case_data(g, kind, case)
        for gated in (True, False):
            dzs = [torch.where(y > 0, d, torch.zeros_like(d)) for y, d in zip(ys, dys)] if gated else dys
            with ops.grad_form('x3'):
                dw, db = ops.conv3x3_wgrad_f32_levels([_gpu(x) for x in xs], [_gpu(d) for d in dys],
                                                      [_gpu(y) for y in ys] if gated else None)
            assert _bits_equal(dw, gx.conv_wgrad_f64(xs, dzs)), (kind, gated)
            if kind == 'integers':
                assert _bits_equal(db, sum(d.sum((0, 1, 2)) for d in dzs)), (kind, gated)


# ---- 2. the dropped-product witness -----------------------------------------------------------------------------------------------
def _witness_dense():
    rows, cin, cout = 17, 96, 64
    a_w, b_w, kept, exact = gx.witness_operands(rows, cin, cout)             # wgrad: K = rows
    a_d, b_d, _, _ = gx.witness_operands(cout, cin, rows)                     # dgrad: K = cout
    return a_w, b_w, a_d, b_d, kept, exact


def _witness_conv():
    """one 3 x 7 map, two images: the two k are pixels (0, 0) and (2, 4) of image 0 -- no tap apart, so only the centre tap's
    products meet; every other tap and channel pair is 0"""
    maps, batch, cin, cout = [(3, 7)], 2, 64, 64
    a, b, kept, exact = gx.witness_operands(gx.conv_pixels(maps, batch), cin, cout, k0=0, k1=2 * 7 + 4)
    return gx.conv_maps(a, maps, batch), gx.conv_maps(b, maps, batch), kept, exact


def _centre_only(dw, value):
    want = torch.zeros(dw.shape, dtype=torch.float64)
    want[:, 1, 1, :] = value
    return _bits_equal(dw, want)


def test_witness_through_the_bare_ops():
    ops = _ops()
    a_w, b_w, a_d, b_d, kept, exact = _witness_dense()
    for form, want in (('x3', kept), ('exact', exact)):
        dw, _, dx = _dense_both(ops, form, a_w, b_w, a_d, b_d, None, None)
        print('\n%s: dw[0][0] = %r, dx[0][0] = %r (want %r)' % (form, float(dw[0, 0]), float(dx[0, 0]), want))
        assert _bits_equal(dw, torch.full(dw.shape, want, dtype=torch.float64)), form
        assert _bits_equal(dx, torch.full(dx.shape, want, dtype=torch.float64)), form
    xs, dys, kept, exact = _witness_conv()
    for form, want in (('x3', kept), ('exact', exact)):
        with ops.grad_form(form):
            dw, _ = ops.conv3x3_wgrad_f32_levels([_gpu(x) for x in xs], [_gpu(d) for d in dys])
        print('%s: conv dw[0][1][1][0] = %r (want %r)' % (form, float(dw[0, 1, 1, 0]), want))
        assert _centre_only(dw, want), form


def test_witness_through_autograd_backward():
    """.backward() runs on autograd's thread, where the ContextVar shows 'exact': the form must come from the graph node.  The
    bare ops under 'exact' return 2^-27 on these tensors (above), so a backward that lost the form fails here."""
    ops = _ops()
    a_w, b_w, a_d, b_d, kept, exact = _witness_dense()
    for form, want in (('x3', kept), ('exact', exact)):
        # wgrad: x = a_w, upstream gradient b_w;  dgrad: weight = a_d, upstream gradient b_d^T
        w = torch.zeros(b_w.shape[1], a_w.shape[1], device='cuda', requires_grad=True)
        with ops.grad_form(form):
            y = ops.dense_trainable(_gpu(a_w), w, None)
        y.backward(_gpu(b_w))                                    # (outside the block, as a training loop calls it)
        assert _bits_equal(w.grad, torch.full(w.shape, want, dtype=torch.float64)), (form, 'dw')
        x = torch.zeros(b_d.shape[1], a_d.shape[1], device='cuda', requires_grad=True)
        wd = _gpu(a_d).requires_grad_()
        with ops.grad_form(form):
            y = ops.dense_trainable(x, wd, None)
            y.backward(_gpu(b_d.t().contiguous()))               # (and inside it)
        assert _bits_equal(x.grad, torch.full(x.shape, want, dtype=torch.float64)), (form, 'dx')
    xs, dys, kept, exact = _witness_conv()
    for form, want in (('x3', kept), ('exact', exact)):
        w = torch.zeros(64, 3, 3, 64, device='cuda', requires_grad=True)
        with ops.grad_form(form):
            ys = ops.conv3x3_trainable_levels([_gpu(x) for x in xs], w, None)
            torch.autograd.backward(ys, [_gpu(d) for d in dys])
        assert _centre_only(w.grad, want), form
    assert ops.current_grad_form() == 'exact'


# ---- 3. random data ---------------------------------------------------------------------------------------------------------------
def _fraction(got, want, bound):
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= bound).all(), 'largest excess %g over a bound of %g' % ((err - bound).max(), bound.flat[(err - bound).argmax()])
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


def _rel(got, want):
    return float(np.abs(got.astype(np.float64) - want).max() / max(np.sqrt((want ** 2).mean()), 1e-300))


@pytest.mark.parametrize('shape', gx.DENSE_RANDOM, ids=lambda s: '%dx%dx%d' % s)
def test_dense_random_data_within_the_bound_and_the_exact_forms_error(shape):
    """|got - want| <= (6 K + 1) * 2^-23 * (|a| . |b|): six float32 accumulations per k in any order, plus the dropped products'
    2^-23 |a b| per product; and max error / rms(want) <= max(2 x the exact form's, 2e-6); db bit-equal between the forms"""
    ops = _ops()
    rows, cin, cout = shape
    rng = np.random.default_rng(cin * 7919 + rows)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    x, w, dy, y, xr = f(rows, cin), f(cout, cin), f(rows, cout), f(rows, cout), f(rows, cin)
    t = lambda a: torch.from_numpy(a).cuda()
    got = {}
    for form in ('exact', 'x3'):
        with ops.grad_form(form):
            dw, db = ops.dense_wgrad(t(dy), t(x), t(y))
            dx = ops.dense_dgrad(t(dy), t(w), t(y), t(xr))
        got[form] = [v.cpu().numpy() for v in (dx, dw, db)]
    wdx, (wdw, wdb) = dg.dgrad(dy, w, y, xr), dg.wgrad(dy, x, y)
    adw, _ = dg.wgrad_abs(dy, x, y)
    bdx = np.where(xr > 0, (6 * cout + 1) * U * dg.dgrad_abs(dy, w, y), 0.0)
    fdx, fdw = _fraction(got['x3'][0], wdx, bdx), _fraction(got['x3'][1], wdw, (6 * rows + 1) * U * adw)
    e = {form: (_rel(got[form][0], wdx), _rel(got[form][1], wdw)) for form in ('exact', 'x3')}
    print('\n%s: fraction of the bound  dx %.4f  dw %.4f;  max error / rms  dx x3 %.3g exact %.3g  dw x3 %.3g exact %.3g'
          % (shape, fdx, fdw, e['x3'][0], e['exact'][0], e['x3'][1], e['exact'][1]))
    for i in (0, 1):
        assert e['x3'][i] <= max(2.0 * e['exact'][i], 2e-6), (i, e)
    assert np.array_equal(got['x3'][2].view(np.uint32), got['exact'][2].view(np.uint32))


@pytest.mark.parametrize('case', gx.CONV_RANDOM, ids=lambda c: '%dmaps-b%d-%dto%d' % (len(c[0]), c[1], c[2], c[3]))
def test_conv_random_data_within_the_bound_and_the_exact_forms_error(case):
    ops = _ops()
    maps, batch, cin, cout = case
    K = gx.conv_pixels(maps, batch)
    rng = np.random.default_rng(K * 31 + cin)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    xs, dys, ys = [[f(batch, h, w, c) for h, w in maps] for c in (cin, cout, cout)]
    t = lambda a: torch.from_numpy(a).cuda()
    got = {}
    for form in ('exact', 'x3'):
        with ops.grad_form(form):
            dw, db = ops.conv3x3_wgrad_f32_levels([t(a) for a in xs], [t(a) for a in dys], [t(a) for a in ys])
        got[form] = (dw.cpu().numpy(), db.cpu().numpy())
    want, _ = cg.wgrad(xs, dys, ys)
    absw, _ = cg.wgrad_abs(xs, dys, ys)
    frac = _fraction(got['x3'][0], want, (6 * K + 1) * U * absw)
    e = {form: _rel(got[form][0], want) for form in got}
    print('\n%s: K %d  fraction of the bound  dw %.4f;  max error / rms  x3 %.3g exact %.3g' % (case[1:], K, frac, e['x3'], e['exact']))
    assert e['x3'] <= max(2.0 * e['exact'], 2e-6), e
    assert np.array_equal(got['x3'][1].view(np.uint32), got['exact'][1].view(np.uint32))


# ---- 4. repeatability ---------------------------------------------------------------------------------------------------------------
REPEAT_DENSE = [(256, 1024, 1024), (256, 1024, 128), (130, 160, 192)]          # dgrad splits; wgrad splits; neither does


def _random_dense(shape, seed=5):
    rows, cin, cout = shape
    gen = torch.Generator().manual_seed(seed)
    f = lambda *s: torch.randn(*s, generator=gen).cuda()
    return dict(x=f(rows, cin), w=f(cout, cin), dy=f(rows, cout), y=f(rows, cout), xr=f(rows, cin))


def _dense_x3(ops, d):
    with ops.grad_form('x3'):
        dw, db = ops.dense_wgrad(d['dy'], d['x'], d['y'])
        return [ops.dense_dgrad(d['dy'], d['w'], d['y'], d['xr']), dw, db]


@pytest.mark.parametrize('shape', REPEAT_DENSE, ids=lambda s: '%dx%dx%d' % s)
def test_dense_two_calls_are_bit_equal(shape):
    ops = _ops()
    assert [gx.dense_plan(k, shape)[1] > 1 for k in ('dgrad', 'wgrad')] == {REPEAT_DENSE[0]: [True, False], REPEAT_DENSE[1]: [False, True],
                                                                           REPEAT_DENSE[2]: [False, False]}[shape]
    d = _random_dense(shape)
    a = _dense_x3(ops, d)
    junk = torch.full((1 << 22,), float('nan'), device='cuda')                   # (whatever the workspace holds does not matter)
    del junk
    b = _dense_x3(ops, d)
    assert all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(a, b))


@pytest.mark.parametrize('case', [gx.CONV_REACH[(64, True)], gx.CONV_REACH[(128, True)], gx.CONV_REACH[(64, False)]],
                         ids=['64-cut', '128-cut', '64-whole'])
def test_conv_two_calls_are_bit_equal(case):
    ops = _ops()
    maps, batch, cin, cout = case
    gen = torch.Generator().manual_seed(3)
    f = lambda c: [torch.randn(batch, h, w, c, generator=gen).cuda() for h, w in maps]
    xs, dys, ys = f(cin), f(cout), f(cout)
    with ops.grad_form('x3'):
        a = ops.conv3x3_wgrad_f32_levels(xs, dys, ys)
        b = ops.conv3x3_wgrad_f32_levels(xs, dys, ys)
    assert all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(a, b))


def test_a_workspace_one_byte_short_is_refused():
    from tf_eager_object_detection_amd import _lib as L
    lib = L.lib()
    d = _random_dense(REPEAT_DENSE[0])
    rows, cin, cout = REPEAT_DENSE[0]
    need = lib.odet_dense_grad_x3_workspace_bytes(0, rows, cin, cout)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    dx = torch.full((rows, cin), 7.0, device='cuda')
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = lib.odet_dense_dgrad_x3(p(d['dy']), p(d['w']), None, None, p(dx), rows, cin, cout, p(ws), need - 1, None)
    assert rc == -2 and b'odet_dense_grad_x3_workspace_bytes' in lib.odet_last_error()
    torch.cuda.synchronize()
    assert bool((dx == 7.0).all())                               # nothing ran
    maps, batch, ci, co = gx.CONV_REACH[(64, True)]
    lv = gx.levels(maps, ptrs=(d['x'].data_ptr(), d['dy'].data_ptr(), None))    # (refused before anything is read)
    need = lib.odet_conv3x3_wgrad_x3_workspace_bytes(lv, len(maps), batch, ci, co)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    rc = lib.odet_conv3x3_wgrad_x3_levels(lv, len(maps), p(dx), None, batch, ci, co, p(ws), need - 1, None)
    assert rc == -2 and b'odet_conv3x3_wgrad_x3_workspace_bytes' in lib.odet_last_error()


def test_graph_capture_replays_bit_equal_to_eager():
    """dense dgrad (split: workspace and reduce launch captured too), wgrad, and the cut conv wgrad, on one stream"""
    ops = _ops()
    d = _random_dense(REPEAT_DENSE[0], seed=1)
    maps, batch, cin, cout = gx.CONV_REACH[(64, True)]
    gen = torch.Generator().manual_seed(2)
    f = lambda c: [torch.randn(batch, h, w, c, generator=gen).cuda() for h, w in maps]
    xs, dys = f(cin), f(cout)

    def run():
        with ops.grad_form('x3'):
            return _dense_x3(ops, d) + list(ops.conv3x3_wgrad_f32_levels(xs, dys))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                    # (the kernels' one-time device set-up happens outside the capture)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            got = run()
    torch.cuda.current_stream().wait_stream(side)
    for t in list(d.values()) + xs + dys:
        t.copy_(torch.randn(t.shape, generator=gen).cuda())
    graph.replay()
    torch.cuda.synchronize()
    want = run()
    assert all(torch.equal(a, b) for a, b in zip(got, want))


# ---- 5. the 3x3 input gradient ----------------------------------------------------------------------------------------------------
def test_conv3x3_dgrad_is_the_split_precision_forward_on_the_flipped_weight():
    from tf_eager_object_detection_amd.model.trainable_common import flipped_weight
    ops = _ops()
    gen = torch.Generator().manual_seed(8)
    conv = torch.nn.Conv2d(64, 128, 3, padding=1).cuda().to(memory_format=torch.channels_last)
    dzs = [torch.randn(2, h, w, 128, generator=gen).cuda() for h, w in gx.PYRAMID[:3]]

    def both():
        wf = flipped_weight(conv)
        with ops.grad_form('x3'):
            got = ops.conv3x3_dgrad_f32_levels(dzs, conv.weight.detach(), flipped=wf)
        with ops.f32_form('x3'):
            want = ops.conv3x3_f32_levels(dzs, wf)
        with ops.grad_form('exact'):
            exact = ops.conv3x3_dgrad_f32_levels(dzs, conv.weight.detach(), flipped=wf)
        return wf, got, want, exact
    wf, got, want, exact = both()
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert not all(torch.equal(a, b) for a, b in zip(got, exact))               # (the exact form rounds differently on random data)
    with torch.no_grad():                                        # an optimiser step: in place, the version counter moves
        conv.weight.mul_(-0.5)
    wf2, got2, want2, _ = both()
    assert wf2 is not wf and torch.equal(wf2, ops.conv3x3_flipped_weight(conv.weight.detach()))
    assert all(torch.equal(a, b) for a, b in zip(got2, want2))
    # the new planes, not the old ones: what a flipped tensor made now, which has no planes yet, gives
    with ops.f32_form('x3'):
        fresh = ops.conv3x3_f32_levels(dzs, ops.conv3x3_flipped_weight(conv.weight.detach()))
    assert all(torch.equal(a, b) for a, b in zip(got2, fresh)) and not any(torch.equal(a, b) for a, b in zip(got2, got))


# ---- 6. the parts and the caller models --------------------------------------------------------------------------------------------
# The exact form's reference-and-bound helpers compose K u (|a| . |b|) per backward contraction with the forward's errors, which
# this form leaves alone.  With K replaced by 6 K + 1 every backward term grows by (6 K + 1) / K <= 7 and the forward terms not at
# all, so 7 x the helpers' bound holds for the split-precision gradients (and is at most 7 / 6 of what the replacement gives on
# the backward terms).
X3_OVER_EXACT_BOUND = 7.0


def _part_detector(seed):
    from tf_eager_object_detection_amd.model.fpn_detector import ResNetFpnDetector
    torch.manual_seed(seed)
    det = ResNetFpnDetector(50, 21, (64, 96), 1, dtype=torch.float32, grad_form='x3')
    return det.to(device='cuda', dtype=torch.float32, memory_format=torch.channels_last).eval()


def _within(name, got, ref, bound, worst):
    err = (got.double() - ref).abs()
    lim = X3_OVER_EXACT_BOUND * bound
    assert bool((err <= lim).all()), (name, float((err - lim).max()))
    assert float(ref.abs().max()) > 0, name
    worst[name] = float((err / lim.clamp_min(1e-300)).max())


def _exact_grads(det, run):
    """the same part under grad_form 'exact' on the same tensors: {name: gradient} (the witness that x3 ran is that weights differ)"""
    det.zero_grad(set_to_none=True)
    det.grad_form = 'exact'
    try:
        run()
    finally:
        det.grad_form = 'x3'
    return {n: p.grad for n, p in det.named_parameters() if p.grad is not None}


def test_roi_head_gradients_within_the_composed_bound():
    import test_dense_grad_gpu as dgt
    det = _part_detector(2)
    rng = np.random.default_rng(3)
    feats = torch.from_numpy(np.maximum(rng.standard_normal((19, 7, 7, 256)), 0).astype(np.float32)).cuda()
    f = lambda shape: torch.from_numpy(rng.standard_normal(tuple(shape)).astype(np.float32)).cuda()
    s, d = det.roi_head_trainable(feats)
    dys, dyd = f(s.shape), f(d.shape)

    def run():
        torch.autograd.backward(det.roi_head_trainable(feats), [dys, dyd])
    exact = _exact_grads(det, run)
    det.zero_grad(set_to_none=True)
    torch.autograd.backward([s, d], [dys, dyd])
    ref, bound = dgt._head_reference(feats, det, dys, dyd)
    worst = {}
    params = dict(det.named_parameters())
    for n in ref:
        _within(n, params[n].grad, ref[n], bound[n], worst)
        assert n.endswith('bias') or not torch.equal(params[n].grad, exact[n]), n
    assert sorted(n for n, p in params.items() if p.grad is not None) == sorted(ref)
    print('\nx3 head gradients, worst fraction of 7 x the composed bound: %s' % ', '.join('%s %.2e' % kv for kv in worst.items()))


def test_rpn_head_gradients_within_the_composed_bound():
    import test_conv_grad_gpu as cgt
    ops = _ops()
    det = _part_detector(2)
    with torch.no_grad():                                       # (as the exact form's test sets the fresh head up)
        for m in (det.rpn_conv, det.rpn_score, det.rpn_bbox):
            m.weight.mul_(5.0)
            m.bias.add_(torch.linspace(-0.2, 0.2, m.bias.numel(), device='cuda'))
    rng = np.random.default_rng(4)
    p_list = cgt._maps(rng, 1)
    f = lambda shape: torch.from_numpy(rng.standard_normal(tuple(shape)).astype(np.float32)).cuda()
    s, d = det.rpn_trainable(p_list)
    ds, dd = f(s.shape), f(d.shape)

    def run():
        torch.autograd.backward(det.rpn_trainable(p_list), [ds, dd])
    exact = _exact_grads(det, run)
    det.zero_grad(set_to_none=True)
    torch.autograd.backward([s, d], [ds, dd])
    with torch.no_grad():
        hs = ops.conv3x3_f32_levels([p.permute(0, 2, 3, 1).contiguous() for p in p_list], det.rpn_conv.weight, det.rpn_conv.bias, relu=True)
    ref, bound = cgt._rpn_reference(det, p_list, hs, ds, dd)
    worst = {}
    params = dict(det.named_parameters())
    for n in cgt.HEAD_NAMES:
        _within(n, params[n].grad, ref[n], bound[n], worst)
        assert n.endswith('bias') or not torch.equal(params[n].grad, exact[n]), n
    print('\nx3 RPN head gradients, worst fraction of 7 x the composed bound: %s' % ', '.join('%s %.2e' % kv for kv in worst.items()))


@pytest.mark.parametrize('shapes', ['even', 'odd'])
def test_neck_gradients_within_the_composed_bound(shapes):
    import neck_grad_np as ng
    import test_neck_grad_gpu as ngt
    shapes = ngt.EVEN_PYRAMID if shapes == 'even' else ngt.ODD_PYRAMID
    det = _part_detector(4)
    with torch.no_grad():                                       # (the fresh layers' biases are zero)
        for name in ng.LAYERS:
            b = getattr(det, name).bias
            b.add_(torch.linspace(-0.3, 0.3, b.numel(), device='cuda'))
    rng = np.random.default_rng(100 + shapes[0][0])
    cs = [c.requires_grad_() for c in ngt._c_maps(rng, 1, shapes)]
    dps = ngt._d_outs(rng, 1, shapes)
    exact = _exact_grads(det, lambda: ngt._backward(det.neck_trainable(cs), dps))
    det.zero_grad(set_to_none=True)
    for c in cs:
        c.grad = None
    ngt._backward(det.neck_trainable(cs), dps)
    ref, bound = ngt._neck_reference(det, cs, dps)
    worst = {}
    params = dict(det.named_parameters())
    for n in ngt.NECK_NAMES:
        _within(n, params[n].grad, ref[n], bound[n], worst)
        assert n.endswith('bias') or not torch.equal(params[n].grad, exact[n]), n
    for i, (c, r, b) in enumerate(zip(cs, ref['dc'], bound['dc'])):
        _within('dC%d' % (i + 2), c.grad, r, b, worst)
    print('\nx3 neck gradients, worst fraction of 7 x the composed bound: %s' % ', '.join('%s %.2e' % kv for kv in worst.items()))


GT_BOXES = [[40.0, 30.0, 170.0, 160.0], [60.0, 50.0, 240.0, 150.0]]


def _model_pair(which):
    from tf_eager_object_detection_amd.model.base_faster_rcnn_model import TrainableResNetFasterRcnn, Vgg16FasterRcnn
    from tf_eager_object_detection_amd.model.base_fpn_model import ResnetV1Fpn
    heads = dict(train_roi_head=True, train_rpn_head=True, train_extractor=True, training_targets='hip', training_losses='hip')
    cls, kw, count, shape = {
        'fpn': (ResnetV1Fpn, dict(heads, depth=50, train_neck=True, roi_training_total_num_samples=32, roi_training_max_pos_samples=8),
                132, (256, 352)),
        'vgg16': (Vgg16FasterRcnn, dict(heads, roi_head_keep_dropout_rate=1.0), 32, (208, 256)),
        'c4': (TrainableResNetFasterRcnn, dict(heads, depth=50, roi_pooling_max_pooling_flag=False), 94, (208, 256)),
    }[which]
    torch.manual_seed(3)
    exact = cls(**kw)
    x3 = cls(grad_form='x3', **kw)
    x3._dense_ref.load_state_dict(exact._dense_ref.state_dict())
    return exact, x3, count, shape


def _fpn_ground_truth(exact, x3, img, shape):
    """as tests/test_conv_grad_gpu.py sets the FPN model up: the fresh RpnHead's proposals spread over sizes and levels, three of
    the larger ones as ground truth -- so that positive RoIs exist and no gradient is an exact zero"""
    with torch.no_grad():
        b = exact.dense.rpn_bbox.bias
        b.add_(torch.linspace(0.0, 1.6, b.numel(), device=b.device, dtype=b.dtype))
        x3._dense_ref.load_state_dict(exact._dense_ref.state_dict())
        p_list = exact._neck(exact._extractor(img, training=True), training=True)
        scores, deltas = exact._get_fpn_head_results(p_list)
        rois = exact._rpn_proposal((deltas, exact._get_anchors(list(shape)), exact._fg_scores(scores), list(shape)), training=True)
    big = rois[((rois[:, 2] - rois[:, 0]) >= 24) & ((rois[:, 3] - rois[:, 1]) >= 24)]
    assert big.shape[0] >= 3, 'the random model proposes fewer than 3 boxes of 24 pixels'
    return big[[0, big.shape[0] // 3, 2 * big.shape[0] // 3]].clone(), torch.tensor([3, 7, 12], device='cuda')


@pytest.mark.parametrize('which', ['fpn', 'vgg16', 'c4'])
def test_caller_model_trains_on_split_precision_gradients(which):
    """grad_form='x3' against 'exact' on identical weights and inputs: the four losses by bytes (the forward is untouched), the
    same parameters hold a gradient, every weight gradient finite and NOT the exact model's bits (x3 ran -- also on autograd's
    thread), and one train_step moves all of them.  No derived bound exists for the deep chains: max |g_x3 - g_exact| / rms(g_exact)
    per parameter is printed."""
    from tf_eager_object_detection_amd import training
    exact, x3, count, shape = _model_pair(which)
    assert (exact.grad_form, x3.grad_form, x3.dense.grad_form) == ('exact', 'x3', 'x3')
    rng = np.random.default_rng(6)
    img = torch.from_numpy((rng.uniform(0, 255, (1,) + shape + (3,)) - 110).astype(np.float32)).cuda()
    inputs = (img, torch.tensor(GT_BOXES, device='cuda'), torch.tensor([3, 12], device='cuda'))
    if which == 'fpn':
        inputs = (img,) + _fpn_ground_truth(exact, x3, img, shape)
    grads = {}
    losses = {}
    for name, m in (('exact', exact), ('x3', x3)):
        out = m(inputs, training=True)
        losses[name] = [v.detach().clone() for v in out]
        sum(out).backward()                                      # (outside any grad_form block)
        grads[name] = {n: p.grad for n, p in m.dense.named_parameters()}
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(losses['exact'], losses['x3']))
    held = sorted(n for n, g in grads['x3'].items() if g is not None)
    assert held == sorted(n for n, g in grads['exact'].items() if g is not None) and len(held) == count
    # the bias gradients whose incoming gradient passed through no x3 launch: those of the heads' last layers, a pure function of
    # the bit-equal forward and of dg_bias_grad's ordered sums
    last_biases = [n for n in held if n.endswith('.bias') and n.split('.')[-2] in ('score', 'bbox', 'rpn_score', 'rpn_bbox')]
    assert len(last_biases) == 4, last_biases
    worst = []
    for n in held:
        gx3, ge = grads['x3'][n], grads['exact'][n]
        assert bool(torch.isfinite(gx3).all()) and gx3.shape == ge.shape and gx3.stride() == ge.stride(), n
        if gx3.dim() >= 2:
            assert not torch.equal(gx3, ge), '%s: the exact form\'s bits -- the split-precision backward did not run' % n
        elif n in last_biases:                                   # db is outside the form, and nothing upstream of it moved
            assert torch.equal(gx3.view(torch.int32), ge.view(torch.int32)), '%s: a last layer\'s bias gradient moved' % n
        rms = float(ge.double().pow(2).mean().sqrt())
        worst.append((float((gx3.double() - ge.double()).abs().max()) / max(rms, 1e-300), n))
    print('\n%s: max |g_x3 - g_exact| / rms(g_exact): worst %s; median %.3g over %d parameters'
          % (which, ', '.join('%s %.3g' % (n, v) for v, n in sorted(worst, reverse=True)[:4]), sorted(worst)[len(worst) // 2][0], count))
    named = [(n, p) for n, p in training.model_variables(x3.dense) if n in held]
    before = {n: p.detach().clone() for n, p in named}
    training.train_step(named, [p.grad for _, p in named], training.MomentumOptimizer(0.01, 0.9), learning_rate_bias_double=True)
    assert all(not torch.equal(p.detach(), before[n]) for n, p in named)
    out = x3(inputs[0], training=False)                          # the weight packs rebuild from the moved parameters
    assert all(bool(torch.isfinite(t.float()).all()) for t in out if isinstance(t, torch.Tensor))
