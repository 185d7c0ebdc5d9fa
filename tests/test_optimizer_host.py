"""The training step without a GPU: tests/optimizer_np.py (the float32 restatement the GPU tests compare BITS against) is held
against independent float64 recurrences written here straight from the formulas of include/odet.h "training step", the float64
recurrence against torch.optim.SGD, and the host side of the feature (schedule, bias doubling, chunk tables, the C ABI's
argument checks) is exercised directly.

Error bounds.  u = 2^-24 (float32 unit roundoff).  The float64 recurrence starts from the same float32 data and uses the same
float32-rounded constants, so the only difference is the float32 rounding of every operation.  The test carries a first-order
bound E on |float32 - float64| per element from step to step, adding u * |result| for every ROUNDING and propagating the
incoming bounds through the operation (2 * w and * scale are exact):
  gradient   g' = (g + wd * (2 w)) * s         2 roundings:  Eg = s * (2 wd Ew + u |wd 2 w| + u |g + wd 2 w|)
  momentum   a' = a mu + g'                    2 roundings:  Ea' = mu Ea + u |a mu| + Eg + u |a'|
             w' = w - a' lr                    2 roundings:  Ew' = Ew + lr Ea' + u |a' lr| + u |w'|
  adam       alpha = lr sqrt(1 - b2p) / (1 - b1p)   5 roundings + the powers' t roundings after t steps, amplified by
                                                    b / (1 - b):  Ra = 5 u + t u (b2p / (1 - b2p) / 2 + b1p / (1 - b1p))  (relative)
             m' = m + (g' - m) c1, c1 = 1 - beta1   4 roundings:  Em' = Em + c1 (Eg + Em) + 3 u |g' - m| c1 + u |m'|
             v' = v + (g' g' - v) c2                5 roundings:  Eq = 2 |g'| Eg + u g'^2;  Ev' = Ev + c2 (Eq + Ev) + 3 u |g'^2 - v| c2 + u |v'|
             d = sqrt(v') + eps                     2 roundings:  Ed = Ev' / (2 sqrt v') + u sqrt v' + u d
             r = (m' alpha) / d                     2 roundings:  Er = (Em' alpha + |m' alpha| (Ra + u)) / d + |r| Ed / d + u |r|
             w' = w - r                             1 rounding:   Ew' = Ew + Er + u |w'|
The magnitudes are those of the float64 recurrence; the second-order terms (a rounding of an already perturbed value) are
covered by a factor 1.01 on the whole bound.  Each test prints the observed fraction of its bound."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import optimizer_np as onp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
SLACK = 1.01
f32 = np.float32


def _data(seed, n, steps):
    rng = np.random.default_rng(seed)
    w = rng.normal(0, 0.05, n).astype(f32)
    gs = [rng.normal(0, 0.1, n).astype(f32) for _ in range(steps)]
    return w, gs


def _d(x):
    return np.float64(f32(x))


@pytest.mark.parametrize('wd,scale', [(0.0, 1.0), (5e-4, 1.0), (1e-4, 2.0)])
def test_momentum_restatement_against_float64_recurrence(wd, scale):
    steps, n = 6, 5000
    w0, gs = _data(3, n, steps)
    boundaries, values, mu = [2, 4], [0.02, 0.01, 0.001], 0.9
    r = onp.Restated('momentum', [w0], [wd], boundaries, values, momentum=mu)
    w, a = w0.astype(np.float64), np.zeros(n)
    Ew, Ea = np.zeros(n), np.zeros(n)
    worst = 0.0
    for t in range(steps):
        r.apply([gs[t]], [scale])
        lr = _d(values[sum(1 for b in boundaries if b < t)])
        g = gs[t].astype(np.float64)
        if wd != 0:
            reg = _d(wd) * (2.0 * w)
            Eg = 2 * _d(wd) * Ew + U * np.abs(reg) + U * np.abs(g + reg)
            g = g + reg
        else:
            Eg = np.zeros(n)
        g, Eg = g * scale, Eg * scale
        a2 = a * _d(mu) + g
        Ea = _d(mu) * Ea + U * np.abs(a * _d(mu)) + Eg + U * np.abs(a2)
        w2 = w - a2 * lr
        Ew = Ew + lr * Ea + U * np.abs(a2 * lr) + U * np.abs(w2)
        w, a = w2, a2
        for name, got, ref, E in (('w', r.vars[0], w, Ew), ('accum', r.slot0[0], a, Ea)):
            frac = float(np.max(np.abs(got.astype(np.float64) - ref) / (SLACK * E)))
            print('momentum wd=%g scale=%g step %d %s: %.3f of the bound' % (wd, scale, t, name, frac))
            worst = max(worst, frac)
    assert worst <= 1.0
    assert r.step == steps


@pytest.mark.parametrize('wd,scale', [(0.0, 1.0), (5e-4, 2.0)])
def test_adam_restatement_against_float64_recurrence(wd, scale):
    steps, n = 6, 5000
    w0, gs = _data(4, n, steps)
    boundaries, values = [3], [1e-3, 1e-4]
    b1, b2, eps = 0.9, 0.999, 1e-8
    r = onp.Restated('adam', [w0], [wd], boundaries, values, beta1=b1, beta2=b2, epsilon=eps)
    w, m, v = w0.astype(np.float64), np.zeros(n), np.zeros(n)
    Ew, Em, Ev = np.zeros(n), np.zeros(n), np.zeros(n)
    c1, c2 = 1.0 - _d(b1), 1.0 - _d(b2)
    worst = 0.0
    for t in range(steps):
        r.apply([gs[t]], [scale])
        lr = _d(values[sum(1 for b in boundaries if b < t)])
        b1p, b2p = _d(b1) ** (t + 1), _d(b2) ** (t + 1)
        alpha = lr * np.sqrt(1.0 - b2p) / (1.0 - b1p)
        Ra = 5 * U + t * U * (b2p / (1.0 - b2p) / 2.0 + b1p / (1.0 - b1p))
        g = gs[t].astype(np.float64)
        if wd != 0:
            reg = _d(wd) * (2.0 * w)
            Eg = 2 * _d(wd) * Ew + U * np.abs(reg) + U * np.abs(g + reg)
            g = g + reg
        else:
            Eg = np.zeros(n)
        g, Eg = g * scale, Eg * scale
        m2 = m + (g - m) * c1
        Em = Em + c1 * (Eg + Em) + 3 * U * np.abs(g - m) * c1 + U * np.abs(m2)
        Eq = 2 * np.abs(g) * Eg + U * g * g
        v2 = v + (g * g - v) * c2
        Ev = Ev + c2 * (Eq + Ev) + 3 * U * np.abs(g * g - v) * c2 + U * np.abs(v2)
        sv = np.sqrt(v2)
        d = sv + _d(eps)
        Ed = Ev / (2 * np.maximum(sv, 1e-300)) + U * sv + U * d
        q = (m2 * alpha) / d
        Er = (Em * alpha + np.abs(m2 * alpha) * (Ra + U)) / d + np.abs(q) * Ed / d + U * np.abs(q)
        w2 = w - q
        Ew = Ew + Er + U * np.abs(w2)
        w, m, v = w2, m2, v2
        for name, got, ref, E in (('w', r.vars[0], w, Ew), ('m', r.slot0[0], m, Em), ('v', r.slot1[0], v, Ev)):
            frac = float(np.max(np.abs(got.astype(np.float64) - ref) / (SLACK * E)))
            print('adam wd=%g scale=%g step %d %s: %.3f of the bound' % (wd, scale, t, name, frac))
            worst = max(worst, frac)
        # the powers after the step (those of step t + 1): t + 1 rounded multiplications
        for got, ref in ((r.b1p, b1p * _d(b1)), (r.b2p, b2p * _d(b2))):
            assert abs(float(got) - ref) <= SLACK * (t + 1) * U * ref
    assert worst <= 1.0


def test_float64_momentum_recurrence_is_torch_sgd():
    """the float64 recurrence the restatement is held against IS momentum SGD: torch.optim.SGD(dampening=0) in float64 with
    weight_decay = 2 wd (its term is wd_t * w, the L2 regulariser's gradient is wd * 2 w)"""
    steps, n, lr, mu, wd = 5, 1000, 0.01, 0.9, 5e-4
    w0, gs = _data(5, n, steps)
    p = torch.nn.Parameter(torch.from_numpy(w0.astype(np.float64)))
    opt = torch.optim.SGD([p], lr=lr, momentum=mu, dampening=0, weight_decay=2 * wd, nesterov=False)
    w, a = w0.astype(np.float64), np.zeros(n)
    for t in range(steps):
        p.grad = torch.from_numpy(gs[t].astype(np.float64))
        opt.step()
        g = gs[t].astype(np.float64) + wd * (2.0 * w)
        a = a * mu + g
        w = w - a * lr
        rel = float(np.max(np.abs(p.detach().numpy() - w)) / np.max(np.abs(w)))
        print('step %d: %.3e relative' % (t, rel))
        assert rel <= 1e-12


def test_schedule_around_the_boundaries():
    b0, b1 = 5, 9
    vals = [0.1, 0.01, 0.001]
    expect = {0: 0.1, b0 - 1: 0.1, b0: 0.1, b0 + 1: 0.01, b1: 0.01, b1 + 1: 0.001}
    from tf_eager_object_detection_amd import training
    sched = training.piecewise_constant([b0, b1], vals)
    for step, v in expect.items():
        assert onp.piecewise_constant(step, [b0, b1], vals) == f32(v), step
        assert training.learning_rate_at(sched, step) == v, step
    assert onp.piecewise_constant(3, [], [0.5]) == f32(0.5)
    with pytest.raises(ValueError):
        training.piecewise_constant([1, 2], [0.1, 0.2])
    with pytest.raises(ValueError):
        training.piecewise_constant([2, 2], [0.1, 0.2, 0.3])
    with pytest.raises(ValueError):
        training.piecewise_constant(list(range(17)), [0.1] * 18)


def test_bias_doubling_by_name():
    from tf_eager_object_detection_amd import training
    names = ['conv1.weight', 'conv1.bias', 'rpn_score.bias', 'fc1.weight', 'bias_free.kernel']
    assert training.grad_scales(names, True) == [1.0, 2.0, 2.0, 1.0, 2.0]        # ('bias' anywhere in the name, as train.py:36)
    assert training.grad_scales(names, False) == [1.0] * 5
    w0, gs = _data(6, 100, 1)
    a = onp.Restated('momentum', [w0], [1e-4])
    b = onp.Restated('momentum', [w0], [1e-4])
    a.apply([gs[0]], [2.0])
    # scale 2 doubles the gradient AFTER the L2 term: the same bits as doubling both by hand (a power of two is exact)
    g2 = (gs[0] + f32(1e-4) * (f32(2) * w0)) * f32(2)
    w2, acc = onp.momentum_update(w0, np.zeros(100, f32), g2, f32(0.01), f32(0.9))
    assert a.vars[0].tobytes() == w2.tobytes() and a.slot0[0].tobytes() == acc.tobytes()
    b.apply([gs[0]], [1.0])
    assert a.vars[0].tobytes() != b.vars[0].tobytes()


@pytest.mark.parametrize('kind', ['momentum', 'adam'])
def test_none_gradient_leaves_variable_and_slots_bit_identical(kind):
    w0, gs = _data(7, 300, 2)
    w1 = (w0 * 3).astype(np.float16)
    r = onp.Restated(kind, [w0, w1, w0], [1e-4, 5e-4, 0.0])
    r.apply([gs[0], gs[0], gs[0]])
    before = [(r.vars[i].tobytes(), r.slot0[i].tobytes(), None if r.slot1[i] is None else r.slot1[i].tobytes(),
               None if r.masters[i] is None else r.masters[i].tobytes()) for i in range(3)]
    per, total = r.apply([None, None, gs[1]])
    after = [(r.vars[i].tobytes(), r.slot0[i].tobytes(), None if r.slot1[i] is None else r.slot1[i].tobytes(),
              None if r.masters[i] is None else r.masters[i].tobytes()) for i in range(3)]
    assert before[0] == after[0] and before[1] == after[1] and before[2] != after[2]
    assert r.step == 2                                               # (the step still counts)
    assert per[0] > 0 and per[1] > 0 and per[2] == 0                 # (a skipped variable's L2 loss is still part of add_n)


def test_zero_weight_decay_adds_no_term():
    """wd == 0 means NO term, not a term of 0: with w = inf the term 0 * (2 w) would be NaN, and g = -0.0 would become +0.0"""
    w = np.array([np.inf, 1.0, -np.inf], f32)
    g = np.array([0.5, -0.0, 0.25], f32)
    out = onp.effective_gradient(g, w, 0.0, 1.0)
    assert out.tobytes() == g.tobytes()
    with np.errstate(all='ignore'):
        assert np.isnan((g + f32(0.0) * (f32(2.0) * w))[0])           # (what a term of 0 would have given)
        assert onp.effective_gradient(g, w, 1e-4, 1.0)[0] == np.inf
    assert onp.l2_loss(w, 0.0) == 0 and onp.l2_loss(w, 0.0).dtype == f32


def _header_chunk():
    text = open(os.path.join(ROOT, 'include', 'odet.h')).read()
    return int(re.search(r'#define ODET_OPT_CHUNK (\d+)', text).group(1))


def test_chunk_tables_cover_every_element_once():
    from tf_eager_object_detection_amd import ops
    CH = _header_chunk()
    assert CH == ops.OPT_CHUNK == onp.CH
    numels = [0, 1, 3, 4, 5, 63, 64, 65, CH - 1, CH, CH + 1, 2 * CH + 7]
    first, chunks = ops.opt_chunk_table(numels)
    assert (first, chunks) == onp.chunk_table(numels)
    seen = [np.zeros(n, np.int32) for n in numels]
    for c, (t, o) in enumerate(chunks):
        assert o % CH == 0 and 0 <= o < numels[t]
        assert c == first[t] + o // CH                               # a tensor's chunks: consecutive, ascending offset
        seen[t][o:min(o + CH, numels[t])] += 1                       # (a chunk never spans two tensors: it ends at numel)
    for t, s in enumerate(seen):
        assert (s == 1).all(), numels[t]
    assert len(chunks) == sum(-(-n // CH) for n in numels)
    assert first[0] == first[1] == 0                                 # (a tensor of 0 elements has no chunk)


def _l2_sum_loops(w):
    """the header's order once more, with explicit loops (independent of the reshapes of optimizer_np.l2_sum)"""
    CH = _header_chunk()
    sq = (w * w).astype(f32)
    n = len(sq)
    nc = -(-n // CH)

    def fold(v):
        v = list(v)
        h = 32
        while h >= 1:
            v = [v[i] + v[i + h] for i in range(h)]
            h //= 2
        return v[0]

    partial = []
    for c in range(nc):
        lane = [0.0] * 256
        for j in range(c * CH, min((c + 1) * CH, n)):
            lane[((j - c * CH) // 4) % 256] += float(sq[j])
        waves = [fold(lane[64 * k:64 * k + 64]) for k in range(4)]
        partial.append(((waves[0] + waves[1]) + waves[2]) + waves[3])
    sums = [0.0] * 64
    for c, p in enumerate(partial):
        sums[c % 64] += p
    return fold(sums)


@pytest.mark.parametrize('n', [0, 1, 5, 4095, 4097, 2 * 4096 + 7, 66 * 4096 + 3])
def test_l2_sum_is_the_headers_order(n):
    import math
    rng = np.random.default_rng(n)
    w = rng.normal(0, 1, n).astype(f32)
    s = onp.l2_sum(w)
    assert float(s) == _l2_sum_loops(w)                              # the same float64 bits
    exact = math.fsum(float(x) for x in (w * w).astype(f32))
    assert abs(float(s) - exact) <= max(n, 1) * 2.0 ** -53 * exact   # and an honest sum: n float64 roundings at the most
    assert onp.l2_loss(w, 5e-4) == f32(f32(5e-4) * f32(s))


def test_abi_exports_argument_and_limit_returns():
    from tf_eager_object_detection_amd import _lib
    Lb = _lib.lib()
    assert Lb.odet_version() == 103
    for name in ('odet_opt_step', 'odet_l2_loss', 'odet_opt_partials_bytes'):
        assert hasattr(Lb, name) and name in _lib.SIGNATURES
    assert (C.sizeof(_lib.OdetOptTensor), C.sizeof(_lib.OdetOptChunk), C.sizeof(_lib.OdetOptState)) == (64, 16, 216)
    assert C.sizeof(_lib.OdetOptConfig) == 32
    assert Lb.odet_opt_partials_bytes(10) == 80 and Lb.odet_opt_partials_bytes(0) == 8
    P = 0x10000                                                      # pointer-valued integers nothing dereferences

    def cfg(kind=1, T=2, K=2, nb=0, b1=0.9, b2=0.999, eps=1e-8):
        return _lib.OdetOptConfig(kind, T, K, nb, 0.9, b1, b2, eps)

    def step(c, tensors=P, grads=P, chunks=P, state=P, partials=None, pbytes=0, tl=None, total=None):
        rc = Lb.odet_opt_step(C.byref(c) if c is not None else None, tensors, grads, chunks, state, partials, pbytes, tl, total, None)
        return rc, Lb.odet_last_error()

    INVALID, WORKSPACE, LIMIT = -1, -2, -4
    rows = [('null cfg', step(None), INVALID), ('null state', step(cfg(), state=None), INVALID),
            ('null tensors', step(cfg(), tensors=None), INVALID), ('null grads', step(cfg(), grads=None), INVALID),
            ('null chunks', step(cfg(), chunks=None), INVALID), ('kind 0', step(cfg(kind=0)), INVALID),
            ('kind 3', step(cfg(kind=3)), INVALID), ('negative T', step(cfg(T=-1)), INVALID),
            ('beta1 1', step(cfg(kind=2, b1=1.0)), INVALID), ('beta2 < 0', step(cfg(kind=2, b2=-0.1)), INVALID),
            ('epsilon < 0', step(cfg(kind=2, eps=-1.0)), INVALID),
            ('l2 without partials', step(cfg(), tl=P), INVALID), ('misaligned partials', step(cfg(), partials=P + 4, pbytes=64, total=P), INVALID),
            ('small partials', step(cfg(), partials=P, pbytes=8, total=P), WORKSPACE),
            ('T over the limit', step(cfg(T=_lib.OPT_MAX_TENSORS + 1), tensors=None), LIMIT),
            ('K over the limit', step(cfg(K=_lib.OPT_MAX_CHUNKS + 1)), LIMIT),
            ('boundaries over the limit', step(cfg(nb=_lib.OPT_MAX_BOUNDARIES + 1)), LIMIT)]
    c = cfg()
    rows += [('l2: null cfg', (Lb.odet_l2_loss(None, P, P, P, 64, P, P, None), Lb.odet_last_error()), INVALID),
             ('l2: no output', (Lb.odet_l2_loss(C.byref(c), P, P, P, 64, None, None, None), Lb.odet_last_error()), INVALID),
             ('l2: null tensors', (Lb.odet_l2_loss(C.byref(c), None, P, P, 64, P, P, None), Lb.odet_last_error()), INVALID),
             ('l2: null partials', (Lb.odet_l2_loss(C.byref(c), P, P, None, 0, P, P, None), Lb.odet_last_error()), INVALID),
             ('l2: small partials', (Lb.odet_l2_loss(C.byref(c), P, P, P, 8, P, P, None), Lb.odet_last_error()), WORKSPACE)]
    c = cfg(T=_lib.OPT_MAX_TENSORS + 1)
    rows += [('l2: T over the limit', (Lb.odet_l2_loss(C.byref(c), P, P, P, 64, P, P, None), Lb.odet_last_error()), LIMIT)]
    for label, (rc, msg), want in rows:
        print('%s -> %d %r' % (label, rc, msg))
        assert rc == want, (label, rc, msg)
        assert msg.startswith(b'odet_') and b' failed: ' not in msg, msg   # (refused before any HIP call)


def test_python_front_refuses_cpu_tensors_and_bad_layouts():
    from tf_eager_object_detection_amd import _lib, training
    opt = training.MomentumOptimizer(0.01, 0.9)
    w = torch.zeros(8)
    with pytest.raises(_lib.OdetError, match='no CPU path'):
        opt.apply_gradients([(torch.zeros(8), w)])
    with pytest.raises(ValueError):
        training.AdamOptimizer(0.001, beta1=1.0)
    with pytest.raises(ValueError):
        training.train_step([('a', w)], [], opt)
    m = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.Linear(4, 2))
    assert [n for n, _ in training.model_variables(m)] == ['0.weight', '0.bias', '1.weight', '1.bias']
    assert training.l2_variables(m, 1e-4) == {'0.weight': 1e-4, '1.weight': 1e-4}    # kernels (dim >= 2), never a bias
