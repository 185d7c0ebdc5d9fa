"""The training step on the GPU (csrc/optimizer.hip through training.py / ops.py) against tests/optimizer_np.py: BIT equality
everywhere (nothing here passes through exp or log; divide and sqrt are correctly rounded on both sides), so every comparison
prints the largest distance in units of the last place it saw and asserts that it is 0."""
import numpy as np
import pytest
import torch

import optimizer_np as onp

pytestmark = pytest.mark.gpu
CH = onp.CH
f32 = np.float32
WDS = (0.0, 1e-4, 5e-4)


def _ulps(got, want):
    """largest distance in units of the last place (float32 / float16 bit patterns on a monotone integer scale)"""
    got, want = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(want).reshape(-1)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    if got.size == 0:
        return 0
    if got.dtype.kind != 'f':
        return int(np.max(np.abs(got.astype(np.int64) - want.astype(np.int64))))
    it = {2: np.int16, 4: np.int32}[got.dtype.itemsize]
    sign = np.int64(1) << (8 * got.dtype.itemsize - 1)

    def key(a):
        i = a.view(it).astype(np.int64)
        mag = i & (sign - 1)
        return np.where(i < 0, -mag, mag)                            # (a zero of the other sign: caught by the byte comparison)
    if not (np.isfinite(got).all() and np.isfinite(want).all()):
        return 0 if got.tobytes() == want.tobytes() else 1 << 30
    return int(np.max(np.abs(key(got) - key(want))))


class _Report:
    def __init__(self, what):
        self.what, self.worst, self.count = what, 0, 0

    def same(self, name, got, want):
        if isinstance(got, torch.Tensor):
            got = got.detach().cpu().numpy()
        want = np.asarray(want)
        d = _ulps(got, want)
        self.worst, self.count = max(self.worst, d), self.count + 1
        assert d == 0 and got.tobytes() == want.tobytes(), '%s: %s is %d ulp from the restatement' % (self.what, name, d)

    def done(self):
        print('%s: %d arrays compared, largest distance %d ulp' % (self.what, self.count, self.worst))


def _cuda(a, offset=0):
    """numpy 1-D array -> CUDA tensor; offset = elements in front of it inside a larger buffer (offset 1: 4-byte (2-byte) aligned)"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not offset:
        return t.cuda()
    buf = torch.zeros(a.size + offset + 3, dtype=t.dtype, device='cuda')
    v = buf[offset:offset + a.size]
    v.copy_(t)
    assert a.size == 0 or v.data_ptr() % 16 != 0
    return v


def _mixed_list(seed):
    """(values, offsets): the numel set around every path's edge, a view at a one-element offset, ~300 tiny tensors and one
    tensor of several chunks; about 60 k elements"""
    rng = np.random.default_rng(seed)
    numels = [0, 1, 3, 4, 5, 63, 64, 65, CH - 1, CH, CH + 1, 2 * CH + 7]
    offsets = [0] * len(numels)
    numels += [777, CH + 1]                                          # variable at an odd element offset (scalar path)
    offsets += [1, 1]
    numels += [int(n) for n in rng.integers(1, 18, 300)]
    offsets += [0] * 300
    numels += [5 * CH + 123]
    offsets += [0]
    vals = [rng.normal(0, 0.05, n).astype(f32) for n in numels]
    return vals, offsets


def _grads(rng, vals, step, dtype=f32):
    """per variable a gradient or None (about one in seven, a different set every step)"""
    return [None if (i + 2 * step) % 7 == 3 else rng.normal(0, 0.1, v.size).astype(dtype) for i, v in enumerate(vals)]


def _make(kind, training, **kw):
    if kind == 'momentum':
        return training.MomentumOptimizer(kw.get('lr', 0.01), 0.9)
    return training.AdamOptimizer(kw.get('lr', 1e-3), 0.9, 0.999, 1e-8)


def _slot_names(kind):
    return ('momentum',) if kind == 'momentum' else ('m', 'v')


def _compare_state(rep, opt, r, tvars, kind):
    for i, tv in enumerate(tvars):
        rep.same('variable %d' % i, tv, r.vars[i])
        for k, name in enumerate(_slot_names(kind)):
            rep.same('%s of %d' % (name, i), opt.get_slot(tv, name), (r.slot0, r.slot1)[k][i].reshape(-1))
        if r.masters[i] is not None:
            rep.same('master of %d' % i, opt.get_slot(tv, 'master'), r.masters[i].reshape(-1))
    assert int(opt.global_step.item()) == r.step
    if kind == 'adam':
        rep.same('beta powers', opt.beta_powers, np.array([r.b1p, r.b2p], f32))


@pytest.mark.parametrize('kind', ['momentum', 'adam'])
def test_three_steps_bit_equal_on_a_mixed_list(kind):
    from tf_eager_object_detection_amd import training
    vals, offsets = _mixed_list(11)
    n = len(vals)
    wds = [WDS[i % 3] for i in range(n)]
    scales = [2.0 if i % 5 == 1 else 1.0 for i in range(n)]
    sched = training.piecewise_constant([0, 1], [0.05, 0.01, 0.002]) if kind == 'momentum' else \
        training.piecewise_constant([1], [1e-3, 3e-4])
    opt = _make(kind, training, lr=sched)
    r = onp.Restated(kind, vals, wds, sched.boundaries, sched.values)
    tvars = [_cuda(v, o) for v, o in zip(vals, offsets)]
    rng = np.random.default_rng(12)
    rep = _Report('%s, mixed list of %d variables / %d elements' % (kind, n, sum(v.size for v in vals)))
    for step in range(3):
        gs = _grads(rng, vals, step)
        # gradients: every third at an odd element offset too (an aligned variable with a misaligned gradient)
        tg = [None if g is None else _cuda(g, 1 if i % 3 == 0 else 0) for i, g in enumerate(gs)]
        before = [(tv.clone(), tv._version) for tv in tvars]
        out = opt.apply_gradients(zip(tg, tvars), grad_scales=scales, weight_decays=wds, l2=True)
        per, total = r.apply(gs, scales)
        rep.same('per-tensor L2 losses', out.tensor_l2_losses, per)
        rep.same('total L2 loss', out.l2_loss.reshape(1), np.array([total], f32))
        _compare_state(rep, opt, r, tvars, kind)
        for (b, ver), g, tv in zip(before, gs, tvars):
            if g is None:
                assert torch.equal(b, tv) and tv._version == ver      # skipped: untouched, version not bumped
            else:
                assert tv._version > ver
    rep.done()
    assert float(total) > 0


def test_l2_loss_of_a_tensor_does_not_depend_on_the_list():
    from tf_eager_object_detection_amd import training
    rng = np.random.default_rng(21)
    target = rng.normal(0, 1, 70 * CH + 5).astype(f32)                # more than 64 chunks: both levels of the order
    others = [rng.normal(0, 1, n).astype(f32) for n in (3, CH + 1, 65)]
    want = onp.l2_loss(target, 5e-4)
    tt, to = _cuda(target), [_cuda(o) for o in others]
    t_odd = _cuda(target, 1)                                          # the same values on the scalar path
    rep = _Report('L2 loss alone / inside a list / at two positions / misaligned')
    for variables, pos in (([tt], 0), ([to[0], tt, to[1]], 1), ([to[2], to[1], to[0], tt], 3), ([to[1], t_odd], 1)):
        opt = training.MomentumOptimizer(0.01, 0.9)
        out = opt.l2_loss(variables, [5e-4] * len(variables))
        rep.same('loss at position %d of %d' % (pos, len(variables)), out.tensor_l2_losses[pos].reshape(1), np.array([want], f32))
        per = [onp.l2_loss(v.cpu().numpy(), 5e-4) for v in variables]
        rep.same('total', out.l2_loss.reshape(1), np.array([onp.add_n(per)], f32))
    rep.done()


@pytest.mark.parametrize('kind', ['momentum', 'adam'])
def test_l2_loss_alone_equals_the_fused_output_and_writes_nothing_else(kind):
    from tf_eager_object_detection_amd import training
    vals, offsets = _mixed_list(31)
    wds = [WDS[(i + 1) % 3] for i in range(len(vals))]
    opt = _make(kind, training)
    tvars = [_cuda(v, o) for v, o in zip(vals, offsets)]
    rng = np.random.default_rng(32)
    tg = [None if g is None else _cuda(g) for g in _grads(rng, vals, 0)]
    opt.apply_gradients(zip(tg, tvars), weight_decays=wds)            # (one step, so that the slots are not all zero)
    opt.prepare(zip(tg, tvars), weight_decays=wds)

    def snapshot():
        s = [tv.clone() for tv in tvars] + [opt.get_slot(tv, k).clone() for tv in tvars for k in _slot_names(kind)]
        return s + [opt.global_step.clone(), opt.beta_powers.clone()] + [g.clone() for g in tg if g is not None]
    before = snapshot()
    alone = opt.l2_loss()
    alone = (alone.l2_loss.clone(), alone.tensor_l2_losses.clone())
    for a, b in zip(before, snapshot()):
        assert torch.equal(a, b)
    fused = opt.apply_gradients(zip(tg, tvars), weight_decays=wds, l2=True)
    assert torch.equal(alone[0], fused.l2_loss) and torch.equal(alone[1], fused.tensor_l2_losses)
    assert float(alone[0]) > 0


@pytest.mark.parametrize('kind', ['momentum', 'adam'])
def test_float16_variables_masters_and_slots_bit_equal(kind):
    """float16 variables with float32 masters, on data that ROUNDS: with momentum at lr = 0.5 the first tensor's masters land
    exactly between two float16 values (1 + 2^-11: the tie goes to the even neighbour 1, and 1 + 2^-10 + 2^-11 goes up to
    1 + 2^-9); the random tensors round up and down."""
    from tf_eager_object_detection_amd import training
    rng = np.random.default_rng(41)
    h = 2.0 ** -10
    tie_w = np.array([1.0, 1.0 + h, -1.0, -(1.0 + h), 2.0, 0.5], np.float16)
    tie_g = np.array([-h, -h, h, h, -2 * h, -h / 2], f32)             # w - g * 0.5 = w + half a float16 step
    vals = [tie_w] + [rng.normal(0, 0.5, n).astype(np.float16) for n in (5, 65, 777, CH + 1, 2 * CH + 7)]
    offsets = [0, 0, 0, 1, 0, 0]                                      # (one float16 view at a one-element offset: 2-byte aligned)
    wds = [0.0, 1e-4, 5e-4, 0.0, 1e-4, 5e-4]
    lr = 0.5 if kind == 'momentum' else 1e-3
    opt = _make(kind, training, lr=lr)
    r = onp.Restated(kind, vals, wds, (), (lr,))
    tvars = [_cuda(v, o) for v, o in zip(vals, offsets)]
    rep = _Report('%s, float16 variables' % kind)
    ties = ups = downs = 0
    for step in range(3):
        gs = [tie_g if step == 0 else None] + [rng.normal(0, 0.1, v.size).astype(np.float16 if i % 2 else f32)
                                               for i, v in enumerate(vals[1:])]
        if step == 1:
            gs[2] = None
        tg = [None if g is None else _cuda(g) for g in gs]
        opt.apply_gradients(zip(tg, tvars), weight_decays=wds)
        r.apply(gs)
        for m, v in zip(r.masters, r.vars):                           # on the CPU: the restated masters really round
            ties += int(np.sum((m.view(np.uint32) & 0x1FFF) == 0x1000))
            ups += int(np.sum(np.abs(v.astype(f32)) > np.abs(m)))
            downs += int(np.sum(np.abs(v.astype(f32)) < np.abs(m)))
        _compare_state(rep, opt, r, tvars, kind)
    rep.done()
    print('masters: %d ties, %d rounded up, %d rounded down (in magnitude)' % (ties, ups, downs))
    assert ups >= 1 and downs >= 1
    if kind == 'momentum':
        assert ties >= 4
        assert r.vars[0][0] == np.float16(1.0) and r.vars[0][1] == np.float16(1.0 + 2 * h)    # ties to even


@pytest.mark.parametrize('kind', ['momentum', 'adam'])
def test_captured_step_replays_across_the_schedule(kind):
    """the step, the powers and the schedule live on the device: ONE captured step, replayed three times, walks over both
    boundaries of the schedule; a capture that meets another gradient pointer raises"""
    from tf_eager_object_detection_amd import _lib, training
    rng = np.random.default_rng(51)
    vals = [rng.normal(0, 0.05, n).astype(f32) for n in (5, 65, CH + 1, 2 * CH + 7)]
    gs = [rng.normal(0, 0.1, v.size).astype(f32) for v in vals]
    gs[1] = None
    wds = [1e-4, 0.0, 5e-4, 1e-4]
    scales = [1.0, 2.0, 2.0, 1.0]
    sched = training.piecewise_constant([1, 2], [0.1, 0.01, 0.001])
    opt = _make(kind, training, lr=sched)
    r = onp.Restated(kind, vals, wds, sched.boundaries, sched.values)
    tvars = [_cuda(v) for v in vals]
    tg = [None if g is None else _cuda(g) for g in gs]
    opt.prepare(zip(tg, tvars), grad_scales=scales, weight_decays=wds)           # tables and pointers on the device: no step
    assert int(opt.global_step.item()) == 0
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = opt.apply_gradients(zip(tg, tvars), grad_scales=scales, weight_decays=wds, l2=True)
    assert int(opt.global_step.item()) == 0                                      # (capturing runs nothing)
    rep = _Report('%s, one captured step replayed three times' % kind)
    for _ in range(3):
        graph.replay()
        per, total = r.apply(gs, scales)
        rep.same('per-tensor L2 losses', out.tensor_l2_losses, per)
        rep.same('total L2 loss', out.l2_loss.reshape(1), np.array([total], f32))
        _compare_state(rep, opt, r, tvars, kind)
    rep.done()
    assert r.step == 3
    moved = list(tg)
    moved[0] = tg[0].clone()
    graph2 = torch.cuda.CUDAGraph()
    with pytest.raises(_lib.OdetError, match='graph capture'):
        with torch.cuda.graph(graph2):
            opt.apply_gradients(zip(moved, tvars), grad_scales=scales, weight_decays=wds, l2=True)
    torch.cuda.synchronize()
    assert int(opt.global_step.item()) == 3
    # outside a capture the same call re-uploads the pointer column and steps
    opt.apply_gradients(zip(moved, tvars), grad_scales=scales, weight_decays=wds, l2=True)
    r.apply(gs, scales)
    _compare_state(_Report('after the re-upload'), opt, r, tvars, kind)


def test_state_dict_round_trip():
    from tf_eager_object_detection_amd import training
    rng = np.random.default_rng(61)
    vals = [rng.normal(0, 0.05, n).astype(f32) for n in (5, CH + 1)] + [rng.normal(0, 0.5, 65).astype(np.float16)]
    gs = [rng.normal(0, 0.1, v.size).astype(f32) for v in vals]
    a = training.AdamOptimizer(1e-3)
    va = [_cuda(v) for v in vals]
    tg = [_cuda(g) for g in gs]
    a.apply_gradients(zip(tg, va))
    state = a.state_dict()
    assert state['global_step'] == 1 and len(state['slots']) == 3 and state['slots'][2]['master'] is not None
    b = training.AdamOptimizer(1e-3)
    vb = [v.clone() for v in va]
    b.load_state_dict(state)                                                     # (before the variable list is known)
    a.apply_gradients(zip(tg, va))
    b.apply_gradients(zip(tg, vb))
    for x, y in zip(va, vb):
        assert torch.equal(x, y)
    assert int(b.global_step.item()) == 2 and torch.equal(a.beta_powers, b.beta_powers)
    for x, y in zip(va, vb):
        for k in ('m', 'v'):
            assert torch.equal(a.get_slot(x, k), b.get_slot(y, k))


def _flat(out):
    if isinstance(out, torch.Tensor):
        return [out]
    if isinstance(out, (list, tuple)):
        return [t for o in out for t in _flat(o)]
    return []


def test_train_step_on_a_detector_rebuilds_the_weight_packs():
    """one train_step on the smallest ResNet-FPN configuration of the suite: the next forward differs from the previous one
    and equals the forward of a FRESH detector loaded with the restated weights (so every cached weight pack was rebuilt from
    the updated parameters); parameters without a gradient keep their version counter"""
    from tf_eager_object_detection_amd import training
    from tf_eager_object_detection_amd.model.fpn_detector import ResNetFpnDetector
    torch.manual_seed(10)
    shape = (128, 160)
    m = ResNetFpnDetector(50, 21, shape, 50, dtype=torch.float32).prepare()
    rng = np.random.default_rng(71)
    img = torch.from_numpy((rng.uniform(0, 255, (1,) + shape + (3,)) - 110).astype(f32)).cuda()
    feat = torch.from_numpy(rng.normal(0, 1, (8, 7, 7, 256)).astype(f32)).cuda()

    def forward(model):
        with torch.no_grad():
            ps = model.features(img)
            return [t.clone() for t in _flat([ps, model.rpn(ps), model.roi_head(feat), model(img)])]
    first = forward(m)
    named = training.model_variables(m)
    wds = training.l2_variables(m, 1e-4)
    assert wds and all(p.dim() >= 2 for n, p in named if n in wds) and not any('bias' in n for n in wds)
    lr, mu = 0.05, 0.9
    grads, restated = [], {}
    for i, (name, p) in enumerate(named):
        w = p.detach().cpu().numpy()
        if i % 6 == 2:
            grads.append(None)
            restated[name] = w
            continue
        g = (rng.normal(0, 1, w.shape) * max(float(np.abs(w).max()), 1e-2)).astype(f32)
        grads.append(torch.empty_like(p).copy_(torch.from_numpy(g)))              # (the parameter's own memory layout)
        ge = onp.effective_gradient(g, w, wds.get(name, 0.0), 2.0 if 'bias' in name else 1.0)
        restated[name] = onp.momentum_update(w, np.zeros_like(w), ge, lr, mu)[0]
    versions = [p._version for _, p in named]
    opt = training.MomentumOptimizer(lr, mu)
    out = training.train_step(named, grads, opt, learning_rate_bias_double=True, weight_decays=wds, l2=True)
    assert float(out.l2_loss) > 0 and int(opt.global_step.item()) == 1
    rep = _Report('detector parameters after one train_step')
    for (name, p), g, ver in zip(named, grads, versions):
        rep.same(name, p, restated[name])
        assert (p._version == ver) if g is None else (p._version > ver), name
    rep.done()
    second = forward(m)
    assert len(first) == len(second) and any(not torch.equal(a, b) for a, b in zip(first, second))
    fresh = ResNetFpnDetector(50, 21, shape, 50, dtype=torch.float32)
    state = {k: v.clone() for k, v in fresh.state_dict().items()}
    state.update({k: torch.from_numpy(v) for k, v in restated.items()})
    fresh.load_state_dict(state)
    fresh.prepare()
    for a, b in zip(second, forward(fresh)):
        assert torch.equal(a, b)
