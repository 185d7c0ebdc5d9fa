"""Dyadic test data for the float16 kernels: operands that are exact in float32 and results that are NOT exact in float16.

Every operand is an integer times a power of two (activations / weights integers, bias / residual multiples of a quantum
2^-s), so every product and every partial sum, in ANY summation order and any K split, is a multiple of the quantum; it is
exact in float32 as long as  (sum |x||w| + |bias| + |residual|) / quantum < 2^24  per output.  `prove_f32_exact` asserts that
from the float64 absolute-value contraction of the actual data -- per case, nothing is assumed.  The expected output of a
float16-storing kernel is then unambiguous: the float64 result rounded ONCE to float16, to nearest even (`rn16`), compared
bit for bit.  The magnitudes are chosen so that most accumulated sums lie above 2048, where float16 has no odd integers any
more: the store really rounds, exact ties are frequent, and a bias / residual added AFTER a first rounding gives another
answer.  `sharpness` measures that from the reference alone, `assert_sharp` holds it to the floors below, and restates the
wrong contracts (truncation, ties away from zero, a late float16 add) -- tests/test_f16_rounding_gpu.py runs the kernels on
exactly the cases of `CASES`, and its CPU half asserts the floors for every one of them, so no GPU case can be vacuous.

Plain module (CPU only: torch on the CPU + numpy); a case's `call` is the only thing that touches the GPU."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

F32_EXACT = float(2 ** 24)
F16_MAX = 65504.0
# floors over the NON-ZERO expected outputs (a ReLU zeroes half)
FLOOR_INEXACT = 1 / 4          # not representable in float16: the store rounds
FLOOR_TIES = 1 / 10            # exactly halfway between two float16 neighbours ...
FLOOR_TIES_EACH = 1 / 20       # ... of which nearest-even sends this share toward zero and this share away from it
FLOOR_TRUNC = 1 / 10           # changed by truncation toward zero
FLOOR_AWAY = 1 / 20            # changed by ties-away-from-zero (the ties that nearest-even sends toward zero)
FLOOR_LATE = 1 / 20            # changed by rounding the accumulated sum first and adding bias / residual in float16


# ---- single roundings and the proof ----------------------------------------------------------------------------------------

def rn16(v64):
    """float64 -> float16, ONE rounding to nearest even: the value must be a float32 already, so that torch's
    double -> float -> half is a single rounding"""
    f = v64.float()
    assert torch.equal(f.double(), v64), 'value is not exact in float32: the expected float16 would be rounded twice'
    return f.half()


def as_f16(v64):
    """an OPERAND: must be exactly representable in float16"""
    h = v64.float().half()
    assert torch.equal(h.double(), v64), 'operand is not exactly representable in float16'
    return h


def prove_f32_exact(abs_total, quantum, integers=(), quanta=()):
    """Asserts the premise of the module: `integers` are integer-valued, `quanta` multiples of `quantum` (a power of two),
    and the absolute-value contraction plus |bias| + |residual| (`abs_total`, float64) stays below 2^24 quanta -- then every
    partial sum of every summation order is a float32.  Returns the worst count of quanta."""
    m, e = np.frexp(quantum)
    assert m == 0.5 and quantum >= 2.0 ** -100, 'the quantum must be a power of two well inside float32\'s normal range'
    for t in integers:
        assert torch.equal(t, t.round())
    for t in quanta:
        q = t / quantum
        assert torch.equal(q, q.round())
    worst = float(abs_total.max()) / quantum
    assert worst < F32_EXACT, 'not exact in float32: %.3g quanta >= 2^24 -- shrink magnitudes or density' % worst
    assert float(abs_total.max()) < 2.0 ** 100
    return worst


# ---- what the reference alone says about a case ----------------------------------------------------------------------------

def _neighbours(v):
    """v float64 numpy, finite, |v| < 65504 -> (h, lo, hi) float64: the nearest-even float16 and the adjacent pair around v"""
    f = v.astype(np.float32)
    assert np.array_equal(f.astype(np.float64), v)
    h16 = f.astype(np.float16)                                        # (numpy: round to nearest even)
    h = h16.astype(np.float64)
    with np.errstate(over='ignore'):                                  # (the neighbour of 65504 is inf)
        up = np.nextafter(h16, np.float16(np.inf)).astype(np.float64)
        dn = np.nextafter(h16, np.float16(-np.inf)).astype(np.float64)
    return h, np.where(h > v, dn, h), np.where(h < v, up, h)


def trunc16(v):
    """the WRONG contract 'round toward zero' (v_cvt_pkrtz): float64 numpy -> float64 values of the float16 results"""
    h, lo, hi = _neighbours(v)
    return np.where(v >= 0, lo, hi)


def away16(v):
    """the WRONG contract 'nearest, ties away from zero'"""
    h, lo, hi = _neighbours(v)
    tie = (h != v) & ((v - lo) == (hi - v))
    return np.where(tie, np.where(v > 0, hi, lo), h)


def sharpness(pre64, late16=None):
    """shares over the non-zero expected outputs; `pre64` the exact result before the store (float64 tensor), `late16` the
    float16 tensor a late float16 add would have stored (None: the form has no bias / residual)"""
    pre = pre64.detach().reshape(-1).numpy()
    keep = pre != 0
    v = pre[keep]
    assert v.size > 0 and float(np.abs(v).max()) < F16_MAX
    h, lo, hi = _neighbours(v)
    inexact = h != v
    tie = inexact & ((v - lo) == (hi - v))
    to_zero = np.abs(h) < np.abs(v)
    s = {'n': int(v.size), 'inexact': inexact.mean(), 'ties': tie.mean(), 'ties_to_zero': (tie & to_zero).mean(),
         'ties_away': (tie & ~to_zero).mean(), 'trunc': (trunc16(v) != h).mean(), 'away': (away16(v) != h).mean()}
    if late16 is not None:
        s['late'] = (late16.detach().reshape(-1).double().numpy()[keep] != h).mean()
    return {k: float(x) for k, x in s.items()}


def assert_sharp(pre64, late16=None, what=''):
    s = sharpness(pre64, late16)
    msg = '%s: %s' % (what, ', '.join('%s %.3f' % kv if kv[0] != 'n' else 'n %d' % kv[1] for kv in s.items()))
    assert s['inexact'] >= FLOOR_INEXACT, msg
    assert s['ties'] >= FLOOR_TIES and s['ties_to_zero'] >= FLOOR_TIES_EACH and s['ties_away'] >= FLOOR_TIES_EACH, msg
    assert s['trunc'] >= FLOOR_TRUNC and s['away'] >= FLOOR_AWAY, msg
    if late16 is not None:
        assert s['late'] >= FLOOR_LATE, msg
    return s


def share_inexact(t64):
    """share of the non-zero values of an INTERMEDIATE that a float16 store has to round"""
    v = t64[t64 != 0]
    return float((v.float().half().double() != v).double().mean())


# ---- generators ------------------------------------------------------------------------------------------------------------

class Gen:
    def __init__(self, seed):
        self.g = torch.Generator()
        self.g.manual_seed(seed)

    def ints(self, shape, amax, density=1.0):
        t = torch.randint(-amax, amax + 1, tuple(shape), generator=self.g).double()
        if density < 1.0:
            t = t * (torch.rand(tuple(shape), generator=self.g) < density).double()
        return t

    def quanta(self, shape, kmax, s):
        """multiples of 2^-s in [-kmax, kmax] * 2^-s"""
        return torch.randint(-kmax, kmax + 1, tuple(shape), generator=self.g).double() * 2.0 ** -s

    def odd_quanta(self, shape, kmax, s):
        """ODD multiples of 2^-s (a value that never vanishes from the rounding decision)"""
        return (2 * torch.randint(-kmax, kmax, tuple(shape), generator=self.g).double() + 1) * 2.0 ** -s

    def f16_ints(self, shape, amax):
        """float16 VALUES of random integers in [-amax, amax] (above 2048 they are already rounded: the output of an earlier
        float16 layer)"""
        return torch.randint(-amax, amax + 1, tuple(shape), generator=self.g).float().half().double()

    def weights(self, shape, k_eff, x_meansq, target=3800.0):
        """integer weights sized so that a k_eff-term sum with activations of mean square `x_meansq` has a standard
        deviation near `target`: far above 2048 (the sum itself needs rounding) and far below 65504 (17 standard deviations)"""
        var = target * target / (k_eff * x_meansq)
        if var >= 2.0 / 3.0:
            amax = max(1, min(63, int((3.0 * var) ** 0.5)))
            return self.ints(shape, amax)
        return self.ints(shape, 1, density=var * 1.5)                # (+-1 or 0: variance 2/3 of the density)


X_MAX = 63
X_MEANSQ = X_MAX * (X_MAX + 1) / 3.0


def conv3x3_acc(x, w):
    """x [B,H,W,C], w [O,C,3,3] float64 -> the 'same' convolution and its absolute-value contraction, NHWC"""
    xn = x.permute(0, 3, 1, 2)
    return (F.conv2d(xn, w, None, 1, 1).permute(0, 2, 3, 1).contiguous(),
            F.conv2d(xn.abs(), w.abs(), None, 1, 1).permute(0, 2, 3, 1).contiguous())


def gemm_acc(x, w):
    return x @ w.t(), x.abs() @ w.abs().t()


def epilogue(acc, bias=None, res=None, relu=False):
    """the CONTRACT of every float16 epilogue: everything in exact arithmetic (float32 on the GPU, exact on this data), then
    ReLU; the caller rounds once"""
    v = acc if bias is None else acc + bias
    if res is not None:
        v = v + res
    return torch.relu(v) if relu else v


def late_epilogue(acc, bias=None, res=None, relu=False):
    """the WRONG contract: the accumulated sum rounded to float16 first, bias / residual added in float16 afterwards"""
    t = rn16(acc)
    if bias is not None:
        t = rn16(t.double() + bias)
    if res is not None:
        t = rn16(t.double() + res)
    return torch.relu(t) if relu else t


def cl(w):
    return w.contiguous(memory_format=torch.channels_last)


# ---- cases -----------------------------------------------------------------------------------------------------------------

class Variant:
    """one launch (or a few) and what it must store: `call(ops, d)` -> tensor or sequence of tensors, d the case's tensors on
    the GPU; `want` the expected tensors (float16 / float32, compared bit for bit); `pre` the exact float64 values before the
    store (None for an output that is not a float16 store), `late` what the late-add contract would store"""

    def __init__(self, name, call, want, pre=None, late=None):
        seq = lambda v: list(v) if isinstance(v, (list, tuple)) else [v]
        self.name, self.call, self.want = name, call, seq(want)
        self.pre = None if pre is None else seq(pre)
        self.late = None if late is None else seq(late)


class Case:
    def __init__(self, name, tensors, variants, worst_quanta, checks=()):
        self.name, self.tensors, self.variants, self.worst_quanta = name, tensors, variants, worst_quanta
        self.checks = list(checks)               # [(what, value, floor)]: further shares the reference must reach

    def assert_not_vacuous(self):
        assert self.worst_quanta < F32_EXACT
        for what, value, floor in self.checks:
            assert value >= floor, '%s %s: %.3f < %.3f' % (self.name, what, value, floor)
        stats, small = {}, []
        for v in self.variants:
            if v.pre is None:
                continue
            pre = torch.cat([p.reshape(-1) for p in v.pre])
            late = None if v.late is None else torch.cat([t.reshape(-1) for t in v.late])
            if int((pre != 0).sum()) < SMALL_SAMPLE:
                small.append((pre, late))
                continue
            stats[v.name] = assert_sharp(pre, late, '%s / %s' % (self.name, v.name))
        if small:
            # a share is a statement about a sample: variants with fewer non-zero outputs than SMALL_SAMPLE (one-pixel maps) are
            # judged together; the late-add share over those of them that have a bias / residual
            stats['small variants'] = assert_sharp(torch.cat([p for p, _ in small]), None, '%s / small variants' % self.name)
            with_late = [(p, l) for p, l in small if l is not None]
            if with_late:
                s_ = sharpness(torch.cat([p for p, _ in with_late]), torch.cat([l for _, l in with_late]))
                assert s_['late'] >= FLOOR_LATE, (self.name, s_)
        return stats


def draws_case(fn, n, *args, **kw):
    """n independent draws of one small case (a one-pixel map has 64 outputs: too few for a share to mean anything) as ONE
    case: every draw's launches run, the floors are judged over all of them together"""
    subs = [fn(*args, seed=50 + i, **kw) for i in range(n)]
    tensors, variants = {}, []
    for i, c in enumerate(subs):
        pre = 'draw%d.' % i
        tensors.update({pre + k: t for k, t in c.tensors.items()})
        for v in c.variants:
            variants.append(Variant('draw %d / %s' % (i, v.name),
                                    lambda ops, d, v=v, pre=pre: v.call(ops, {k[len(pre):]: t for k, t in d.items() if k.startswith(pre)}),
                                    v.want, v.pre, v.late))
    return Case('%s x %d draws' % (subs[0].name, n), tensors, variants, max(c.worst_quanta for c in subs))


def _bias(g, n):
    return g.quanta((n,), 12, 2)                 # k / 4 in [-3, 3]


def conv3x3_case(B, H, W, cin, cout, seed=1, full=True, k_eff=None):
    """ops.conv3x3_f16: bias on / off, ReLU on / off, the [cout,3,3,cin] weight form with `out=`"""
    g = Gen(seed * 7919 + B * 131 + H * 17 + W + cin + cout)
    x = g.ints((B, H, W, cin), X_MAX)
    w = g.weights((cout, cin, 3, 3), k_eff or 9 * cin, X_MEANSQ)
    b = _bias(g, cout)
    acc, ab = conv3x3_acc(x, w)
    worst = prove_f32_exact(ab + b.abs(), 0.25, integers=(x, w), quanta=(b,))
    variants = []
    for use_b, relu in (((True, True), (True, False), (False, True), (False, False)) if full else ((True, True),)):
        pre = epilogue(acc, b if use_b else None, None, relu)
        variants.append(Variant(
            'bias %d relu %d' % (use_b, relu),
            lambda ops, d, use_b=use_b, relu=relu: ops.conv3x3_f16(d['x'], d['w'], d['b'] if use_b else None, relu=relu),
            rn16(pre), pre, late_epilogue(acc, b, None, relu) if use_b else None))
    if full:
        pre = epilogue(acc, b, None, True)

        def with_out(ops, d):
            out = torch.full((B, H, W, cout), float('nan'), dtype=torch.float16, device=d['x'].device)
            ops.conv3x3_f16(d['x'], d['w'].permute(0, 2, 3, 1).contiguous(), d['b'], relu=True, out=out)
            return out
        variants.append(Variant('out= and [cout,3,3,cin] weights', with_out, rn16(pre), pre, late_epilogue(acc, b, None, True)))
    return Case('conv3x3_f16 %s' % ((B, H, W, cin, cout),), {'x': as_f16(x), 'w': cl(as_f16(w)), 'b': as_f16(b)}, variants, worst)


def conv3x3_levels_case(B, shapes, cin, cout, seed=2):
    """ops.conv3x3_f16_levels: several maps, shared weights, one launch"""
    g = Gen(seed * 7919 + cin + cout)
    xs = [g.ints((B, h, w, cin), X_MAX) for h, w in shapes]
    w = g.weights((cout, cin, 3, 3), 9 * cin, X_MEANSQ)
    b = _bias(g, cout)
    accs = [conv3x3_acc(x, w) for x in xs]
    worst = max(prove_f32_exact(ab + b.abs(), 0.25, integers=(x, w), quanta=(b,)) for x, (a, ab) in zip(xs, accs))
    variants = []
    for use_b, relu in ((True, True), (False, False)):
        pre = [epilogue(a, b if use_b else None, None, relu) for a, _ in accs]
        variants.append(Variant(
            'bias %d relu %d' % (use_b, relu),
            lambda ops, d, use_b=use_b, relu=relu: ops.conv3x3_f16_levels([d['x%d' % i] for i in range(len(shapes))], d['w'],
                                                                          d['b'] if use_b else None, relu=relu),
            [rn16(p) for p in pre], pre, [late_epilogue(a, b, None, relu) for a, _ in accs] if use_b else None))
    tensors = {'w': cl(as_f16(w)), 'b': as_f16(b)}
    tensors.update({'x%d' % i: as_f16(x) for i, x in enumerate(xs)})
    return Case('conv3x3_f16_levels %s' % ((B, shapes, cin, cout),), tensors, variants, worst)


def conv3x3_pool_case(B, H, W, cin, cout, seed=3, k_eff=None):
    """ops.conv3x3_relu_pool2_f16: max-pooling 2x2 / 2 'same' of relu(conv + bias); rounding is monotone, so the pooled map of
    the rounded values is the rounding of the pooled exact values"""
    g = Gen(seed * 7919 + B * 131 + H * 17 + W + cin + cout)
    x = g.ints((B, H, W, cin), X_MAX)
    w = g.weights((cout, cin, 3, 3), k_eff or 9 * cin, X_MEANSQ)
    b = _bias(g, cout)
    acc, ab = conv3x3_acc(x, w)
    worst = prove_f32_exact(ab + b.abs(), 0.25, integers=(x, w), quanta=(b,))
    pool = lambda t: F.max_pool2d(t.permute(0, 3, 1, 2), 2, 2, ceil_mode=True).permute(0, 2, 3, 1).contiguous()
    pre = pool(epilogue(acc, b, None, True))
    late = pool(late_epilogue(acc, b, None, True).float()).half()
    v = Variant('pooled', lambda ops, d: ops.conv3x3_relu_pool2_f16(d['x'], d['w'], d['b']), rn16(pre), pre, late)
    return Case('conv3x3_relu_pool2_f16 %s' % ((B, H, W, cin, cout),), {'x': as_f16(x), 'w': cl(as_f16(w)), 'b': as_f16(b)}, [v], worst)


def conv1x1_case(M, K, N, seed=4):
    """ops.conv1x1_f16: residual on / off, ReLU on / off; and `in_bias` (x is a convolution WITHOUT bias and ReLU:
    relu(x + in_bias) is rounded to float16 on load, ONCE, before the contraction)"""
    g = Gen(seed * 7919 + M + K + N)
    x = g.ints((M, K), X_MAX)
    w = g.weights((N, K), K, X_MEANSQ)
    b = _bias(g, N)
    r = g.quanta((M, N), 64, 2)                  # k / 4 in [-16, 16]
    acc, ab = gemm_acc(x, w)
    worst = prove_f32_exact(ab + b.abs() + r.abs(), 0.25, integers=(x, w), quanta=(b, r))
    variants = []
    for use_r, relu in ((True, True), (False, True), (True, False), (False, False)):
        rr = r if use_r else None
        pre = epilogue(acc, b, rr, relu)
        variants.append(Variant('residual %d relu %d' % (use_r, relu),
                                lambda ops, d, use_r=use_r, relu=relu: ops.conv1x1_f16(d['x'], d['w'].view(N, K, 1, 1), d['b'],
                                                                                       d['r'] if use_r else None, relu),
                                rn16(pre), pre, late_epilogue(acc, b, rr, relu)))
    # in_bias: integers up to 1023 plus an odd multiple of 1/4 -> above 512 the sum is not a float16
    x2 = g.ints((M, K), 1023)
    ib = g.odd_quanta((K,), 6, 2)
    t64 = torch.relu(x2 + ib)
    t = rn16(t64).double()
    w2 = g.weights((N, K), K, float((t * t).mean()))
    acc2, ab2 = gemm_acc(t, w2)
    worst = max(worst, prove_f32_exact(ab2 + b.abs() + r.abs(), 0.25, integers=(x2, w2), quanta=(ib, t, b, r)))
    pre = epilogue(acc2, b, r, True)
    variants.append(Variant('in_bias', lambda ops, d: ops.conv1x1_f16(d['x2'], d['w2'], d['b'], d['r'], True, in_bias=d['ib']),
                            rn16(pre), pre, late_epilogue(acc2, b, r, True)))
    tensors = {'x': as_f16(x), 'w': as_f16(w), 'b': as_f16(b), 'r': as_f16(r), 'x2': as_f16(x2), 'w2': as_f16(w2), 'ib': as_f16(ib)}
    return Case('conv1x1_f16 %s' % ((M, K, N),), tensors, variants, worst,
                checks=[('in_bias: loaded activations that round', share_inexact(t64), FLOOR_INEXACT)])


def pointwise_case(B, H, W, K, N, stride, seed=5):
    """ops.pointwise (float16): the epilogue combinations of the existing test, stride 1 and 2"""
    g = Gen(seed * 7919 + B * 7 + H + K + N + stride)
    Ho, Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
    x = g.ints((B, H, W, K), X_MAX)
    w = g.weights((N, K), K, X_MEANSQ)
    b = _bias(g, N)
    r = g.quanta((B, Ho, Wo, N), 64, 2)
    acc, ab = gemm_acc(x[:, ::stride, ::stride], w)
    worst = prove_f32_exact(ab + b.abs() + r.abs(), 0.25, integers=(x, w), quanta=(b, r))
    variants = []
    for use_r, relu, use_b in ((True, True, True), (False, True, True), (True, False, True), (False, False, False)):
        bb, rr = (b if use_b else None), (r if use_r else None)
        pre = epilogue(acc, bb, rr, relu)
        variants.append(Variant('bias %d residual %d relu %d' % (use_b, use_r, relu),
                                lambda ops, d, use_r=use_r, relu=relu, use_b=use_b: ops.pointwise(
                                    d['x'], d['w'].view(N, K, 1, 1), d['b'] if use_b else None, d['r'] if use_r else None, relu, stride),
                                rn16(pre), pre, late_epilogue(acc, bb, rr, relu) if (use_b or use_r) else None))
    return Case('pointwise f16 %s' % ((B, H, W, K, N, stride),), {'x': as_f16(x), 'w': as_f16(w), 'b': as_f16(b), 'r': as_f16(r)},
                variants, worst)


def pointwise_dual_case(B, H, W, K1, K2, N, stride, seed=6):
    """ops.pointwise_dual (float16): one contraction over [x1 | x2(::stride)]"""
    g = Gen(seed * 7919 + K1 + K2 + N + H)
    Ho, Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
    a = g.ints((B, Ho, Wo, K1), X_MAX)
    c = g.ints((B, H, W, K2), X_MAX)
    w = g.weights((N, K1 + K2), K1 + K2, X_MEANSQ)
    b = _bias(g, N)
    acc, ab = gemm_acc(torch.cat([a, c[:, ::stride, ::stride]], -1), w)
    worst = prove_f32_exact(ab + b.abs(), 0.25, integers=(a, c, w), quanta=(b,))
    p1, p2 = epilogue(acc, b, None, True), acc
    variants = [
        Variant('bias relu', lambda ops, d: ops.pointwise_dual(d['a'], d['c'], d['w'], d['b'], stride, relu=True), rn16(p1), p1,
                late_epilogue(acc, b, None, True)),
        Variant('plain', lambda ops, d: ops.pointwise_dual(d['a'], d['c'], d['w'], None, stride, relu=False), rn16(p2), p2)]
    return Case('pointwise_dual f16 %s' % ((B, H, W, K1, K2, N, stride),),
                {'a': as_f16(a), 'c': as_f16(c), 'w': as_f16(w), 'b': as_f16(b)}, variants, worst)


def upsample2_exact(top):
    """TF 1.x legacy bilinear resize (align_corners = False) of [B,h,w,C] to exactly (2h, 2w): the source coordinate of output
    y is y / 2, so every weight is 0 or 1/2 and the three lerps  a + (b - a) * t  are exact on dyadic data"""
    B, h, w, C = top.shape
    iy = torch.arange(2 * h)
    y0, y1, wy = iy // 2, torch.clamp(iy // 2 + 1, max=h - 1), (iy % 2).double() * 0.5
    ix = torch.arange(2 * w)
    x0, x1, wx = ix // 2, torch.clamp(ix // 2 + 1, max=w - 1), (ix % 2).double() * 0.5
    rows0, rows1 = top[:, y0], top[:, y1]
    lerp_x = lambda t: t[:, :, x0] + (t[:, :, x1] - t[:, :, x0]) * wx.view(1, 1, -1, 1)
    t0, t1 = lerp_x(rows0), lerp_x(rows1)
    return t0 + (t1 - t0) * wy.view(1, -1, 1, 1)


def merge_case(B, h, w, C, seed=7):
    """ops.fpn_topdown_merge on float16 maps (csrc/neck.hip): float32 arithmetic on the float16 inputs -- up = the three
    lerps, out = up * 0.5 + lateral * 0.5 -- and ONE rounding, at the store"""
    g = Gen(seed * 7919 + h * 31 + w + C)
    top = g.f16_ints((B, h, w, C), 8191)
    lat = g.f16_ints((B, 2 * h, 2 * w, C), 8191)
    up = upsample2_exact(top)
    pre = up * 0.5 + lat * 0.5
    worst = prove_f32_exact(top.abs().max() * 2 + lat.abs().max(), 0.125, quanta=(top, lat, up, pre))
    # the wrong placement: the resized map rounded to float16 before the merge
    late = rn16(rn16(up).double() * 0.5 + lat * 0.5)
    v = Variant('merge', lambda ops, d: ops.fpn_topdown_merge(d['top'], d['lat']), rn16(pre), pre, late)
    return Case('fpn_topdown_merge f16 %s' % ((B, h, w, C),), {'top': as_f16(top), 'lat': as_f16(lat)}, [v], worst)


def lateral_case(B, H, W, h, w_, K, seed=8):
    """ops.lateral_merge (float16; the pointwise kernel with the merge in its epilogue, csrc/conv3x3.hip): the lateral
    convolution + bias stays in float32, out = up * 0.5 + lateral * 0.5 is rounded ONCE.  The two-launch form
    fpn_topdown_merge(top, pointwise(x, w, b)) rounds the lateral map in between: it is the same function exactly where that
    map is a float16 already -- variant 'exact lateral' (small sums, the result still rounds) asserts the equality of the two
    forms on the GPU, variant 'rounding lateral' the placement of the single rounding."""
    assert H == 2 * h and W == 2 * w_
    N = 256
    g = Gen(seed * 7919 + H * W + K)
    b = _bias(g, N)
    top = g.f16_ints((B, h, w_, N), 8191)
    up = upsample2_exact(top)
    bi = g.ints((N,), 8)                         # (an integer bias where the lateral map has to be a float16 as it stands)
    tensors = {'b': as_f16(b), 'bi': as_f16(bi), 'top': as_f16(top)}
    variants, worst, checks = [], 0.0, []
    for name, target, b in (('rounding lateral', 3800.0, b), ('exact lateral', 300.0, bi)):
        x = g.ints((B, H, W, K), X_MAX)
        w = g.weights((N, K), K, X_MEANSQ, target=target)
        acc, ab = gemm_acc(x, w)
        lat = acc + b
        pre = up * 0.5 + lat * 0.5
        worst = max(worst, prove_f32_exact(ab + b.abs() + top.abs().max() * 2, 0.125, integers=(x, w), quanta=(b, top, up, pre)))
        two = rn16(up * 0.5 + rn16(lat).double() * 0.5)          # the two-launch contract
        key = name.split()[0]
        tensors['x_' + key], tensors['w_' + key] = as_f16(x), as_f16(w)
        if key == 'exact':
            assert float(lat.abs().max()) < 2048 and torch.equal(lat, lat.round())     # integers below 2048
            assert torch.equal(two, rn16(pre))

            def both(ops, d):
                fused = ops.lateral_merge(d['x_exact'], d['w_exact'], d['bi'], d['top'])
                return fused, ops.fpn_topdown_merge(d['top'], ops.pointwise(d['x_exact'], d['w_exact'], d['bi']))
            variants.append(Variant(name, both, [rn16(pre), rn16(pre)], [pre], None))
        else:
            variants.append(Variant(name, lambda ops, d: ops.lateral_merge(d['x_rounding'], d['w_rounding'], d['b'], d['top']),
                                    rn16(pre), pre, two))
            checks.append(('lateral values that a float16 store would round', share_inexact(lat), FLOOR_INEXACT))
    return Case('lateral_merge f16 %s' % ((B, H, W, h, w_, K),), tensors, variants, worst, checks)


def tail_case(B, H, W, cin, n3, cmid, seed=9):
    """ops.conv3x3_conv1x1_f16, with and without the shortcut.  Contract (the existing test's reference()):
    t = float16(relu(conv3x3(x, w2) + b2)); out = float16(relu(t . w3 + b3 (+ r))).  The intermediate t must itself need
    rounding, and the second stage is proved exact on the ROUNDED t.  Two-launch forms: with the first launch's own epilogue
    (conv3x3_f16(x, w2, b2, relu=True)) the contract is the same for any b2; with `in_bias=b2` the first launch stores
    float16(conv) and the load rounds relu(. + b2) again -- a different function where the convolution rounds, so that form
    is held to ITS contract here (and to the fused one in tests/test_detector.py on data where nothing rounds)."""
    g = Gen(seed * 7919 + B * 100 + H + cin + n3 + cmid)
    x = g.ints((B, H, W, cin), X_MAX)
    # (a first stage around 1200: above 512 its sums + k/4 already round, and the second stage then adds MANY middling terms --
    # with intermediates in the thousands it would add two or three, and such a sum is a float16 more often than not)
    w2 = g.weights((cmid, cin, 3, 3), 9 * cin, X_MEANSQ, target=1200.0)
    b2 = _bias(g, cmid)
    acc2, ab2 = conv3x3_acc(x, w2)
    worst = prove_f32_exact(ab2 + b2.abs(), 0.25, integers=(x, w2), quanta=(b2,))
    t64 = epilogue(acc2, b2, None, True)
    t = rn16(t64).double()
    t_two = rn16(torch.relu(rn16(acc2).double() + b2)).double()          # conv3x3_f16(x, w2) then in_bias on load
    w3 = g.weights((n3, cmid), cmid, float((t * t).mean()))
    b3 = g.quanta((n3,), 24, 1)                  # k / 2 in [-12, 12]
    r = g.quanta((B, H, W, n3), 32, 1)           # (halves, as b3: the intermediate's own fractions already spread the sums)
    acc3, ab3 = gemm_acc(t, w3)
    acc3_two, ab3_two = gemm_acc(t_two, w3)
    for a_ in (ab3, ab3_two):
        worst = max(worst, prove_f32_exact(a_ + b3.abs() + r.abs(), 0.25, integers=(w3,), quanta=(t, t_two, b3, r)))
    variants = []
    for use_r in (True, False):
        rr = r if use_r else None
        pre = epilogue(acc3, b3, rr, True)
        pre_two = epilogue(acc3_two, b3, rr, True)

        def forms(ops, d, use_r=use_r):
            res = d['r'] if use_r else None
            fused = ops.conv3x3_conv1x1_f16(d['x'], d['w2'], d['b2'], d['w3'], d['b3'], residual=res, relu=True)
            two = ops.conv1x1_f16(ops.conv3x3_f16(d['x'], d['w2'], d['b2'], relu=True), d['w3'], d['b3'], residual=res, relu=True)
            inb = ops.conv1x1_f16(ops.conv3x3_f16(d['x'], d['w2']), d['w3'], d['b3'], residual=res, relu=True, in_bias=d['b2'])
            return fused, two, inb
        variants.append(Variant('shortcut %d' % use_r, forms, [rn16(pre), rn16(pre), rn16(pre_two)], [pre],
                                [late_epilogue(acc3, b3, rr, True)]))
    tensors = {'x': as_f16(x), 'w2': cl(as_f16(w2)), 'b2': as_f16(b2), 'w3': as_f16(w3), 'b3': as_f16(b3), 'r': as_f16(r)}
    return Case('conv3x3_conv1x1_f16 %s' % ((B, H, W, cin, n3, cmid),), tensors, variants, worst,
                checks=[('intermediate values that round', share_inexact(t64), FLOOR_INEXACT),
                        ('intermediate values the in_bias form rounds differently', float((t != t_two)[t64 != 0].double().mean()), 0.002)])


def bias_relu_maxpool_case(B, H, W, C, k, s, pad, ceil, seed=10):
    """ops.bias_relu_maxpool (float16): max_pool(float16(relu(x + bias))), x a float16 convolution output without its bias"""
    g = Gen(seed * 7919 + H + W + C)
    x = g.f16_ints((B, H, W, C), 4095)
    b = _bias(g, C)
    worst = prove_f32_exact(x.abs().max() + b.abs().max(), 0.25, quanta=(x, b))
    pool = lambda t: F.max_pool2d(t.permute(0, 3, 1, 2), k, s, padding=pad, ceil_mode=ceil).permute(0, 2, 3, 1).contiguous()
    pre = pool(torch.relu(x + b))
    v = Variant('pooled', lambda ops, d: ops.bias_relu_maxpool(d['x'], d['b'], k, s, pad, ceil), rn16(pre), pre)
    return Case('bias_relu_maxpool f16 %s' % ((B, H, W, C, k, s, pad, ceil),), {'x': as_f16(x), 'b': as_f16(b)}, [v], worst)


def bias_act_case(C, seed=11):
    """ops.bias_act_ (float16): float32 arithmetic in the documented order (x + b) + r, ReLU, one rounding.  On the dyadic
    block every float32 operation is exact and the float64 value is the expectation; the late contract rounds x + b to
    float16 before the residual goes in.  The ORDER of the two additions shows only where float32 itself rounds: the
    second block (x and -r neighbouring float16 values, b 2^-11 of their difference) is held to the float32 restatement of the
    documented order on the CPU, and the other order would store other bits for half of it"""
    g = Gen(seed * 7919 + C)
    shape = (3, 17, 19, C)
    x = g.f16_ints(shape, 4095)
    # (k / 4 in [-3, 3] from a fixed table: with 8 channels a random draw of 8 biases decides every share by itself)
    b = torch.tensor([1, -1, 3, -3, 0.5, -0.5, 0.25, -2, 1.5, -0.75, 2.25, -1.25, 0, 2, -2.5, 2.75], dtype=torch.float64)[torch.arange(C) % 16]
    r = g.quanta(shape, 64, 2)
    worst = prove_f32_exact(x.abs().max() + b.abs().max() + r.abs().max(), 0.25, quanta=(x, b, r))
    variants = []
    for use_r, relu in ((True, True), (False, True), (True, False), (False, False)):
        rr = r if use_r else None
        pre = epilogue(x, b, rr, relu)
        late = None
        if use_r:                                                     # x + b rounded to float16 before the residual goes in
            late = rn16(rn16(x + b).double() + r)
            late = torch.relu(late) if relu else late
        variants.append(Variant('residual %d relu %d' % (use_r, relu),
                                lambda ops, d, use_r=use_r, relu=relu: ops.bias_act_(d['x'].clone(), d['b'], d['r'] if use_r else None, relu),
                                rn16(pre), pre, late))
    # the order of the additions: float32 restatement
    # per channel x = 2^e, r = -(x's float16 predecessor) = -(2^e - 2^(e-11)), b = 2^(e-22) + j 2^(e-26): the exact result lies
    # just above the float16 tie 2^(e-11) + 2^(e-22); x + b rounds b to float32's 2^(e-23) at x, b + r to 2^(e-24) at r -- for
    # j = 3, 4 the documented order lands ON the tie (and goes to even), the other order above it
    e = 8 + torch.arange(C) % 8
    j = 2 + (torch.arange(C) // 8 + torch.arange(C)) % 4
    xo = (2.0 ** e).float().expand(shape).contiguous()
    ro = -(2.0 ** e - 2.0 ** (e - 11)).float().expand(shape).contiguous()
    bo = (2.0 ** (e - 22) + j * 2.0 ** (e - 26)).float()
    assert torch.equal(bo.half().float(), bo) and torch.equal(xo.half().float(), xo) and torch.equal(ro.half().float(), ro)
    want = ((xo + bo) + ro).half()
    other = (xo + (bo + ro)).half()
    order_share = float((want != other).double().mean())
    variants.append(Variant('order of the additions', lambda ops, d: ops.bias_act_(d['xo'].clone(), d['bo'], d['ro'], False), want))
    tensors = {'x': as_f16(x), 'b': as_f16(b), 'r': as_f16(r), 'xo': xo.half(), 'bo': bo.half(), 'ro': ro.half()}
    return Case('bias_act_ f16 C=%d' % C, tensors, variants, worst,
                checks=[('outputs that x + (b + r) would change', order_share, FLOOR_INEXACT)])


def _image_conv(img, w, stride, pad):
    xn = F.pad(img.permute(0, 3, 1, 2), (pad,) * 4)
    return (F.conv2d(xn, w, None, stride, 0).permute(0, 2, 3, 1).contiguous(),
            F.conv2d(xn.abs(), w.abs(), None, stride, 0).permute(0, 2, 3, 1).contiguous())


PIX_MAX = 255


def rgb_case(B, H, W, f32_image, seed=12):
    """ops.conv3x3_rgb: float16(relu?(conv3x3(float16(image)) + bias)); integer pixels are the same float16 and float32"""
    g = Gen(seed * 7919 + H * 11 + W + f32_image)
    img = g.ints((B, H, W, 3), PIX_MAX)
    k_eff = 27 if min(H, W) > 2 else 3 * min(H, 3) * min(W, 3)
    w = g.weights((64, 3, 3, 3), k_eff, PIX_MAX * (PIX_MAX + 1) / 3.0)
    b = _bias(g, 64)
    acc, ab = _image_conv(img, w, 1, 1)
    worst = prove_f32_exact(ab + b.abs(), 0.25, integers=(img, w), quanta=(b,))
    variants = []
    for relu in (True, False):
        pre = epilogue(acc, b, None, relu)
        variants.append(Variant('relu %d' % relu, lambda ops, d, relu=relu: ops.conv3x3_rgb(d['img'], ops.conv3x3_rgb_pack_weights(d['w']), d['b'], relu=relu),
                                rn16(pre), pre, late_epilogue(acc, b, None, relu)))
    image = as_f16(img).float() if f32_image else as_f16(img)
    return Case('conv3x3_rgb %s' % ((B, H, W, 'float32' if f32_image else 'float16'),), {'img': image, 'w': as_f16(w), 'b': as_f16(b)},
                variants, worst)


def stem_case(B, H, W, f32_image, seed=13):
    """ops.stem_conv7_pool3: max_pool3x3/2(pad 1)(float16(relu(conv7x7/2(pad 3)(float16(image)) + bias)))"""
    g = Gen(seed * 7919 + H * 7 + W + f32_image)
    img = g.ints((B, H, W, 3), PIX_MAX)
    # (the pooled value is the largest of nine: a smaller target keeps it in the binades where ties are frequent)
    w = g.weights((64, 3, 7, 7), 147 if min(H, W) >= 14 else 75, PIX_MAX * (PIX_MAX + 1) / 3.0, target=1800.0)
    b = _bias(g, 64)
    acc, ab = _image_conv(img, w, 2, 3)
    worst = prove_f32_exact(ab + b.abs(), 0.25, integers=(img, w), quanta=(b,))
    pool = lambda t: F.max_pool2d(F.pad(t.permute(0, 3, 1, 2), (1, 1, 1, 1)), 3, 2).permute(0, 2, 3, 1).contiguous()   # (values >= 0)
    pre = pool(epilogue(acc, b, None, True))
    late = pool(late_epilogue(acc, b, None, True).float()).half()
    v = Variant('stem', lambda ops, d: ops.stem_conv7_pool3(d['img'], ops.stem_pack_weights(d['w']), d['b']), rn16(pre), pre, late)
    image = as_f16(img).float() if f32_image else as_f16(img)
    return Case('stem_conv7_pool3 %s' % ((B, H, W, 'float32' if f32_image else 'float16'),), {'img': image, 'w': as_f16(w), 'b': as_f16(b)},
                [v], worst)


def rpn_tail_case(A, seed=14):
    """ops.rpn_head_tail: t = float16(relu(conv_out + conv_bias)) -- ONE rounding --, then t . w^T + b in float32: on this data
    the float32 scores / deltas are EXACTLY the float64 values"""
    g = Gen(seed * 7919 + A)
    B, shapes = 2, [(13, 17), (7, 9), (3, 5)]
    b1 = g.odd_quanta((512,), 6, 2)
    w = g.ints((6 * A, 512), 3)
    b2 = _bias(g, 6 * A)
    tensors = {'b1': as_f16(b1), 'w': as_f16(w), 'b2': as_f16(b2)}
    n = sum(h * w_ for h, w_ in shapes) * A
    sc, dl, worst, t_all = [], [], 0.0, []
    for i, (h, w_) in enumerate(shapes):
        c = g.f16_ints((B, h, w_, 512), 4095)
        t64 = torch.relu(c + b1)
        t = rn16(t64).double()
        t_all.append(t64.reshape(-1))
        acc, ab = gemm_acc(t.reshape(B, -1, 512), w)
        worst = max(worst, prove_f32_exact(ab + b2.abs(), 0.25, integers=(w,), quanta=(c, b1, t, b2)))
        o = acc + b2
        assert torch.equal(o.float().double(), o)
        sc.append(o[..., :2 * A].reshape(B, -1, 2)); dl.append(o[..., 2 * A:].reshape(B, -1, 4))
        tensors['c%d' % i] = as_f16(c)

    def call(ops, d):
        scores = torch.full((B, n, 2), -7.0, dtype=torch.float32, device=d['w'].device)
        deltas = torch.full((B, n, 4), -7.0, dtype=torch.float32, device=d['w'].device)
        off = 0
        for i, (h, w_) in enumerate(shapes):
            ops.rpn_head_tail(d['c%d' % i], d['b1'], d['w'].view(6 * A, 512, 1, 1), d['b2'], A, scores, deltas, off)
            off += h * w_ * A
        return scores, deltas
    v = Variant('tail', call, [torch.cat(sc, 1).float().contiguous(), torch.cat(dl, 1).float().contiguous()])
    t_all = torch.cat(t_all)
    return Case('rpn_head_tail A=%d' % A, tensors, [v], worst, checks=[('activations that round', share_inexact(t_all), FLOOR_INEXACT)])


def rpn_fused_case(B, A, cin, cout, shapes, seed=15):
    """ops.rpn_head_fused: t = float16(relu(conv3x3(x) + conv_bias)) rounds once (never written), the two 1x1 convolutions
    accumulate it in float32: exact float32 logits / deltas.  With cout = 512 the two-pass form (conv3x3_f16_levels with the
    bias and ReLU in its own epilogue + rpn_head_tail with a zero bias) has the same contract and must give the same bits."""
    g = Gen(seed * 7919 + B * 100 + A + cin + cout)
    xs = [g.ints((B, h, w, cin), X_MAX) for h, w in shapes]
    w3 = g.weights((cout, cin, 3, 3), 9 * cin, X_MEANSQ)
    b3 = _bias(g, cout)
    w1 = g.ints((6 * A, cout), 1)
    b1 = _bias(g, 6 * A)
    n = sum(h * w for h, w in shapes) * A
    sc, dl, worst, t_all, changed = [], [], 0.0, [], []
    for x in xs:
        acc, ab = conv3x3_acc(x, w3)
        worst = max(worst, prove_f32_exact(ab + b3.abs(), 0.25, integers=(x, w3), quanta=(b3,)))
        t64 = epilogue(acc, b3, None, True)
        t = rn16(t64).double()
        t_late = late_epilogue(acc, b3, None, True).double()
        t_all.append(t64.reshape(-1))
        o, ab1 = gemm_acc(t.reshape(B, -1, cout), w1)
        worst = max(worst, prove_f32_exact(ab1 + b1.abs(), 0.25, integers=(w1,), quanta=(t, b1)))
        o = o + b1
        assert torch.equal(o.float().double(), o)
        changed.append(((t_late.reshape(B, -1, cout) @ w1.t() + b1) != o).reshape(-1))
        sc.append(o[..., :2 * A].reshape(B, -1, 2)); dl.append(o[..., 2 * A:].reshape(B, -1, 4))
    want = [torch.cat(sc, 1).float().contiguous(), torch.cat(dl, 1).float().contiguous()]
    L = len(shapes)

    def fused(ops, d):
        scores = torch.full((B, n, 2), 7.0, device=d['w3'].device)
        deltas = torch.full((B, n, 4), 7.0, device=d['w3'].device)
        ops.rpn_head_fused([d['x%d' % i] for i in range(L)], d['w3'], d['b3'], d['w1'], d['b1'], A, scores, deltas)
        return scores, deltas
    variants = [Variant('fused', fused, want)]
    if cout == 512:
        def two_pass(ops, d):
            convs = ops.conv3x3_f16_levels([d['x%d' % i] for i in range(L)], d['w3'], d['b3'], relu=True)
            scores = torch.full((B, n, 2), 7.0, device=d['w3'].device)
            deltas = torch.full((B, n, 4), 7.0, device=d['w3'].device)
            off = 0
            for (h, w), c in zip(shapes, convs):
                ops.rpn_head_tail(c, torch.zeros_like(d['b3']), d['w1'], d['b1'], A, scores, deltas, off)
                off += h * w * A
            return scores, deltas
        variants.append(Variant('two-pass', two_pass, want))
    tensors = {'w3': cl(as_f16(w3)), 'b3': as_f16(b3), 'w1': as_f16(w1), 'b1': as_f16(b1)}
    tensors.update({'x%d' % i: as_f16(x) for i, x in enumerate(xs)})
    return Case('rpn_head_fused %s' % ((B, A, cin, cout, shapes),), tensors, variants, worst,
                checks=[('activations that round', share_inexact(torch.cat(t_all)), FLOOR_INEXACT),
                        ('logits / deltas that a late float16 bias add in the activation changes',
                         float(torch.cat(changed).double().mean()), FLOOR_LATE)])


def dense_out_f32_case(seed=16):
    """ops.dense_f16_out_f32: float16 operands, float32 bias and result -- exactly the float64 value"""
    g = Gen(seed * 7919)
    M, K, N = 1037, 1024, 128
    x = g.ints((M, K), X_MAX)
    w = g.ints((N, K), 31)
    w[105:] = 0
    b = g.quanta((N,), 50, 2)
    acc, ab = gemm_acc(x, w)
    worst = prove_f32_exact(ab + b.abs(), 0.25, integers=(x, w), quanta=(b,))
    o = acc + b
    assert torch.equal(o.float().double(), o) and float(o.abs().max()) > 65520.0       # beyond float16's range
    variants = [Variant('plain', lambda ops, d: ops.dense_f16_out_f32(d['x'], d['w'], d['b']), o.float()),
                Variant('relu', lambda ops, d: ops.dense_f16_out_f32(d['x'], d['w'], d['b'], relu=True), torch.relu(o).float())]
    return Case('dense_f16_out_f32', {'x': as_f16(x), 'w': as_f16(w), 'b': b.float()}, variants, worst)


# ---- the ends of float16's range through a real layer ----------------------------------------------------------------------

SMALL_SAMPLE = 1000
BAND_FLOOR = 300            # outputs per band ("a few hundred")


def _bands(pre):
    a = pre.abs()
    return {'subnormal': int(((a > 0) & (a < 2.0 ** -14)).sum()), 'below_smallest_tie': int(((a > 0) & (a <= 2.0 ** -25)).sum()),
            'clamp_to_65504': int(((a >= 65504) & (a < 65520)).sum()), 'plus_inf': int((pre >= 65520).sum()),
            'minus_inf': int((pre <= -65520).sum())}


def range_case(kind, seed=17):
    """Power-of-two scaling keeps the data dyadic.  'subnormal': float16-SUBNORMAL activations (integers times 2^-24) and
    weights scaled so that the results spread over |v| < 2^-14 and below the smallest tie 2^-25 -- gradual underflow on the way
    in and on the way out, nothing flushed.  'top': results around 65504: [65504, 65520) stores 65504, >= 65520 stores inf,
    -inf becomes 0 under a ReLU."""
    g = Gen(seed * 7919 + len(kind))
    B, H, W, cin, cout = 2, 25, 42, 128, 256
    variants, tensors, worst, bands = [], {}, 0.0, {}
    for form in ('pointwise', 'conv3x3'):
        K = cin if form == 'pointwise' else 9 * cin
        if kind == 'subnormal':
            xs, ws = 2.0 ** -24, 2.0 ** -8                            # products from 2^-32
            x = g.ints((B, H, W, cin), X_MAX) * xs                   # |x| <= 63 * 2^-24 < 2^-18: every one a SUBNORMAL float16
            wi = g.weights((cout, cin, 3, 3) if form == 'conv3x3' else (cout, cin), K, X_MEANSQ, target=400.0)
            b = g.quanta((cout,), 12, 0) * 2.0 ** -24                # multiples of the smallest float16 subnormal
        else:
            xs, ws = 1.0, 1.0
            x = g.ints((B, H, W, cin), X_MAX)
            wi = g.weights((cout, cin, 3, 3) if form == 'conv3x3' else (cout, cin), K, X_MEANSQ, target=60.0)
            # the bias puts every sum next to the end of the range: +-65504 / +-65472 (float16 neighbours), sums ~ +-60 around it
            b = torch.tensor([65504.0, 65472.0])[torch.randint(0, 2, (cout,), generator=g.g)].double() \
                * (2 * torch.randint(0, 2, (cout,), generator=g.g).double() - 1)
        w = wi * ws
        quantum = xs * ws if kind == 'subnormal' else 1.0
        acc, ab = conv3x3_acc(x, w) if form == 'conv3x3' else gemm_acc(x, w)
        worst = max(worst, prove_f32_exact(ab + b.abs(), quantum, quanta=(x, w, b, acc)))
        tensors.update({'x_' + form: as_f16(x), 'w_' + form: cl(as_f16(w)) if form == 'conv3x3' else as_f16(w), 'b_' + form: as_f16(b)})
        for relu in (False, True):
            pre = epilogue(acc, b, None, relu)
            bands['%s relu %d' % (form, relu)] = _bands(pre)
            if form == 'conv3x3':
                call = lambda ops, d, relu=relu: ops.conv3x3_f16(d['x_conv3x3'], d['w_conv3x3'], d['b_conv3x3'], relu=relu)
            else:
                call = lambda ops, d, relu=relu: ops.pointwise(d['x_pointwise'], d['w_pointwise'], d['b_pointwise'], None, relu)
            variants.append(Variant('%s relu %d' % (form, relu), call, rn16(pre)))
    case = Case('range %s' % kind, tensors, variants, worst)
    case.bands = bands
    return case


def assert_bands(case, kind):
    for name, b in case.bands.items():
        if kind == 'subnormal':
            assert b['subnormal'] >= BAND_FLOOR and b['below_smallest_tie'] >= BAND_FLOOR, (name, b)
        else:
            assert b['clamp_to_65504'] >= BAND_FLOOR and b['plus_inf'] >= BAND_FLOOR, (name, b)
            if name.endswith('relu 0'):
                assert b['minus_inf'] >= BAND_FLOOR, (name, b)
            else:
                assert b['minus_inf'] == 0


# ---- the conversion itself: every decision boundary of float16 -------------------------------------------------------------

def f16_decision_boundaries():
    """float32 numpy array: for every finite float16 h >= 0 and its successor the midpoint m (exact in float32) and
    nextafter(m, +-inf), h itself, both signs; +-0, the float32 subnormals around 0, 2^-25 (the smallest tie) and its neighbours,
    65504, the last float32 below 65520, 65520 and its neighbours, +-inf, a few NaN payloads.  Under a million values."""
    h = np.arange(0, 0x7C00, dtype=np.uint16).view(np.float16).astype(np.float32)            # every finite float16 >= 0
    nxt = np.append(h[1:], np.float32(65536.0))                                             # (the successor of 65504 in an unbounded format)
    mid = ((h.astype(np.float64) + nxt.astype(np.float64)) / 2).astype(np.float32)
    assert np.array_equal(mid.astype(np.float64) * 2, h.astype(np.float64) + nxt.astype(np.float64))
    pos = np.concatenate([h, mid, np.nextafter(mid, np.float32(np.inf)), np.nextafter(mid, np.float32(-np.inf)),
                          np.nextafter(h, np.float32(np.inf)), np.nextafter(h[1:], np.float32(-np.inf))])
    tiny = np.array([0, 1, 2, 0x007FFFFF, 0x00800000, 0x00800001], dtype=np.uint32).view(np.float32)      # float32 subnormals, FLT_MIN
    special = np.array([65504.0, 65519.996, 65520.0, 65520.004, 65536.0, 1e30, 3.4028235e38, 2.0 ** -25, 2.0 ** -24, 2.0 ** -14],
                       dtype=np.float32)
    with np.errstate(over='ignore'):
        special = np.concatenate([special, np.nextafter(special, np.float32(np.inf)), np.nextafter(special, np.float32(-np.inf))])
    pos = np.concatenate([pos, tiny, special, np.array([np.inf], np.float32)])
    nans = np.array([0x7FC00000, 0x7F800001, 0xFFC00000, 0x7FFFFFFF, 0xFF800001, 0x7FC12345], dtype=np.uint32).view(np.float32)
    v = np.concatenate([pos, -pos, nans])
    assert v.size < 1_000_000
    return v


def f16_bits_nan_as_one(h_bits):
    """uint16 bits with every NaN mapped to one pattern (NaN compares as NaN, not by payload)"""
    b = np.asarray(h_bits).astype(np.uint16).copy()
    b[(b & 0x7C00 == 0x7C00) & (b & 0x03FF != 0)] = 0x7E00
    return b


def input_conversion_pixels(n, seed=18):
    """float32 pixels for the kernels that convert a float32 image: float16 ties and their float32 neighbours, in the range an
    image has (|v| < 256: float16 ulp 1/8 at the top) -- n values, both signs"""
    g = np.random.default_rng(seed)
    h = g.integers(0x3000, 0x5BFF, size=n).astype(np.uint16).view(np.float16).astype(np.float32)          # [0.125, 255.9)
    nxt = np.nextafter(h.astype(np.float16), np.float16(np.inf)).astype(np.float32)
    mid = (h + nxt) / 2                                                                                    # exact in float32
    pick = g.integers(0, 3, size=n)
    v = np.where(pick == 0, mid, np.where(pick == 1, np.nextafter(mid, np.float32(np.inf)), np.nextafter(mid, np.float32(-np.inf))))
    return (v * g.choice(np.float32([-1, 1]), size=n)).astype(np.float32)


# ---- the registry: every case the GPU tests run ----------------------------------------------------------------------------

CASES = {}


def _add(fn, *args, **kw):
    name = '%s%s' % (fn.__name__.replace('_case', ''), ''.join('-%s' % (a,) for a in args).replace(' ', ''))
    CASES[name] = functools.partial(fn, *args, **kw)


# shapes: subsets of the lists of tests/test_detector.py (partial last tiles, one-pixel maps, every channel-tile width)
for shape in ((1, 13, 21, 256, 512), (3, 7, 5, 128, 256), (2, 31, 45, 64, 192), (2, 50, 84, 64, 64), (1, 100, 167, 128, 128)):
    _add(conv3x3_case, *shape)
CASES['conv3x3-1-1-1-64-64'] = functools.partial(draws_case, conv3x3_case, 12, 1, 1, 1, 64, 64, k_eff=64)
CASES['conv3x3_pool-1-1-1-64-64'] = functools.partial(draws_case, conv3x3_pool_case, 24, 1, 1, 1, 64, 64, k_eff=64)
CASES['rgb-3-1-1-True'] = functools.partial(draws_case, rgb_case, 8, 3, 1, 1, True)                                                # (one pixel: the centre tap only)
# test_conv3x3_f16_every_tile_height: shapes that pick the 256-channel tiles of 4 .. 8 pixel tiles per wave themselves (asserted
# from the launcher's recorded plan: tests/conv_tile_cases.py EVERY_TILE_HEIGHT), then the shapes that test ran before
for H, W in ((128, 250), (100, 334), (191, 250), (170, 334), (191, 334), (20, 84), (328, 100), (209, 200), (300, 167), (349, 167)):
    _add(conv3x3_case, 1, H, W, 64, 256, full=False)
_add(conv3x3_levels_case, 2, ((25, 42), (13, 21), (7, 11), (4, 6)), 128, 256)
for shape in ((2, 37, 45, 64, 64), (1, 64, 96, 64, 128), (3, 9, 7, 128, 256)):
    _add(conv3x3_pool_case, *shape)
for shape in ((1007, 64, 256), (96, 128, 512), (33, 256, 1024), (64, 64, 320), (130, 512, 64), (300, 512, 192)):
    _add(conv1x1_case, *shape)
for shape in ((2, 25, 42, 1024, 256, 1), (2, 50, 84, 256, 512, 2), (1, 33, 47, 512, 1024, 2), (2, 31, 17, 128, 64, 1),
              (1, 9, 11, 1024, 2048, 2), (3, 13, 21, 2048, 512, 1), (1, 1, 1000, 12544, 1024, 1)):
    _add(pointwise_case, *shape)
for shape in ((2, 20, 33, 64, 64, 256, 1), (1, 50, 84, 128, 256, 512, 2)):
    _add(pointwise_dual_case, *shape)
for shape in ((3, 25, 42, 256), (3, 7, 5, 8)):
    _add(merge_case, *shape)
for shape in ((2, 50, 84, 25, 42, 1024), (2, 20, 20, 10, 10, 128)):
    _add(lateral_case, *shape)
for shape in ((1, 13, 21, 256, 1024, 256), (3, 7, 5, 128, 64, 256), (2, 25, 42, 128, 512, 128), (1, 9, 70, 128, 192, 128),
              (1, 33, 47, 64, 256, 64), (3, 6, 5, 64, 64, 64)):
    _add(tail_case, *shape)
for shape in ((2, 41, 67, 64, 3, 2, 1, False), (2, 75, 100, 128, 2, 2, 0, True)):
    _add(bias_relu_maxpool_case, *shape)
for C in (8, 64, 256):
    _add(bias_act_case, C)
for B, H, W, f32 in ((1, 64, 96, True), (2, 61, 75, False), (2, 9, 33, False), (1, 8, 32, True)):
    _add(rgb_case, B, H, W, f32)
for B, H, W, f32 in ((1, 64, 96, True), (2, 61, 75, False), (1, 33, 17, False), (3, 7, 9, True)):
    _add(stem_case, B, H, W, f32)
for A in (3, 4, 1):
    _add(rpn_tail_case, A)
for shape in ((2, 3, 256, 512, ((25, 42), (13, 21), (7, 11), (4, 6))), (3, 4, 128, 256, ((20, 31), (9, 9))), (1, 1, 64, 512, ((37, 53),))):
    _add(rpn_fused_case, *shape)
_add(dense_out_f32_case)


# ---- a seeded slice of tools/fuzz_conv.py's float16 kinds on this generator: odd random shapes on data that rounds ----------

FUZZ_CASES = 27


def fuzz_case(i, seed=0):
    rng = np.random.default_rng(1000 * seed + i)
    ri = lambda lo, hi: int(rng.integers(lo, hi + 1))
    kind = i % 9
    B, H, W = ri(1, 2), ri(2, 40), ri(2, 50)
    if kind == 0:
        return conv3x3_case(B, H, W, 64 * ri(1, 4), 64 * ri(1, 10), seed=100 + i, full=False)
    if kind == 1:
        A, cin, cout = ri(1, 5), 64 * ri(1, 3), 256 * ri(1, 2)
        shapes = tuple((max(2, H >> l), max(2, W >> l)) for l in range(ri(1, 4)))
        return rpn_fused_case(B, A, cin, cout, shapes, seed=100 + i)
    if kind == 2:
        return tail_case(B, H, W, 64 * ri(1, 4), 64 * ri(1, 16), (64, 128, 256)[ri(0, 2)], seed=100 + i)
    if kind == 3:
        return stem_case(B, ri(14, 140), ri(14, 180), bool(i & 1), seed=100 + i)
    if kind == 4:
        return pointwise_case(B, H, W, 64 * ri(2, 12), 64 * ri(1, 9), ri(1, 2), seed=100 + i)
    if kind == 5:
        h, w = max(1, H // 2), max(1, W // 2)
        return lateral_case(B, 2 * h, 2 * w, h, w, 64 * ri(2, 12), seed=100 + i)
    if kind == 6:
        return pointwise_dual_case(B, H, W, 64 * ri(1, 6), 64 * ri(2, 12), 64 * ri(1, 9), ri(1, 2), seed=100 + i)
    if kind == 7:
        return rgb_case(B, ri(3, 70), ri(3, 90), bool(i & 1), seed=100 + i)
    return conv3x3_pool_case(B, H, W, 64 * ri(1, 4), 64 * ri(1, 8), seed=100 + i)


# ---- the INPUT conversion of the kernels that take float32 images ----------------------------------------------------------

def input_conversion_case(kind, convert=None):
    """float32 pixels that are float16 ties or their float32 neighbours, weights that select ONE tap of ONE channel per output
    channel, zero bias: the output IS the converted pixel.  conv3x3_rgb runs without its ReLU; the stem always applies ReLU and
    max-pooling, so it runs twice, the second time with the selector negated (the negative pixels).  `convert`: the float32 ->
    float16 conversion of the image (default: torch's, round to nearest even; the CPU tests pass the wrong ones)."""
    B, H, W = 2, 37, 53
    img = torch.from_numpy(input_conversion_pixels(B * H * W * 3)).view(B, H, W, 3)
    img16 = img.half().double() if convert is None else convert(img)
    k = 3 if kind == 'rgb' else 7
    w = torch.zeros(64, 3, k, k, dtype=torch.float64)
    o = torch.arange(64)
    tap = (o // 3 * 5) % (k * k)                                     # (spread over the window, the centre and the corners included)
    w[o, o % 3, tap // k, tap % k] = 1.0
    tensors = {'img': img, 'w': as_f16(w), 'wneg': as_f16(-w), 'b': torch.zeros(64, dtype=torch.float16)}
    if kind == 'rgb':
        acc, _ = _image_conv(img16, w, 1, 1)
        v = Variant('selected pixel', lambda ops, d: ops.conv3x3_rgb(d['img'], ops.conv3x3_rgb_pack_weights(d['w']), d['b'], relu=False),
                    rn16(acc), acc)
        return Case('conv3x3_rgb input conversion', tensors, [v], 0.0)
    pool = lambda t: F.max_pool2d(F.pad(t.permute(0, 3, 1, 2), (1, 1, 1, 1)), 3, 2).permute(0, 2, 3, 1).contiguous()
    acc, _ = _image_conv(img16, w, 2, 3)
    pos, neg = pool(torch.relu(acc)), pool(torch.relu(-acc) + 0.0)          # (+ 0.0: relu(-0.0) is -0.0 here, the sum of the kernel +0)
    v = Variant('selected pixel, both signs',
                lambda ops, d: (ops.stem_conv7_pool3(d['img'], ops.stem_pack_weights(d['w']), d['b']),
                                ops.stem_conv7_pool3(d['img'], ops.stem_pack_weights(d['wneg']), d['b'])),
                [rn16(pos), rn16(neg)], [pos, neg])
    return Case('stem_conv7_pool3 input conversion', tensors, [v], 0.0)
