"""numpy float32 restatement of the training step (include/odet.h "training step", csrc/optimizer.hip): the piecewise-constant
schedule, the gradient rule (L2 term, bias doubling), the Momentum and Adam updates, the ordered float64 L2 sum and the float32
masters of float16 variables.  Every line is one float32 operation in the header's order; the L2 sum is the header's order
restated with reshapes, cumsum (sequential in numpy) and the fold in halves.  Shared by tests/test_optimizer_host.py and
tests/test_optimizer_gpu.py (which asks the GPU for the same BITS)."""
import numpy as np

CH = 4096                    # ODET_OPT_CHUNK
f32 = np.float32


def piecewise_constant(step, boundaries, values):
    """values[i], i = the number of boundaries strictly below step (learning_rate_decay_v2.piecewise_constant)"""
    assert len(values) == len(boundaries) + 1
    return f32(values[sum(1 for b in boundaries if b < step)])


def fold64(v):
    """[..., 64] float64 -> [...]: v[:32] + v[32:], then [:16] + [16:], ... (the butterfly of a 64-lane wave)"""
    assert v.shape[-1] == 64 and v.dtype == np.float64
    n = 64
    while n > 1:
        v = v[..., :n // 2] + v[..., n // 2:n]
        n //= 2
    return v[..., 0]


def l2_sum(w):
    """float64 S of a float32 tensor in the header's order"""
    w = np.ascontiguousarray(w, dtype=f32).reshape(-1)
    nc = -(-w.size // CH)
    if nc == 0:
        return np.float64(0.0)
    sq = np.zeros(nc * CH, f32)
    sq[:w.size] = w * w                                                              # the float32 squares
    lanes = sq.reshape(nc, 4, 256, 4).transpose(0, 2, 1, 3).reshape(nc, 256, 16).astype(np.float64)
    lane_sum = np.cumsum(lanes, axis=2)[:, :, -1]                                    # a lane's 16 squares in ascending index
    waves = fold64(lane_sum.reshape(nc, 4, 64))
    chunk = np.cumsum(waves, axis=1)[:, -1]                                          # wave 0 + 1 + 2 + 3
    p = np.zeros(-(-nc // 64) * 64, np.float64)
    p[:nc] = chunk
    return fold64(np.cumsum(p.reshape(-1, 64), axis=0)[-1])                          # sum l: chunks l, l + 64, ...


def l2_loss(w, wd):
    """float32(wd * float32(S)); exactly 0 for an unregularised tensor"""
    wd = f32(wd)
    if wd == 0:
        return f32(0.0)
    return f32(wd * f32(l2_sum(w)))


def add_n(losses):
    total = f32(0.0)
    for v in losses:
        total = f32(total + f32(v))
    return total


def effective_gradient(g, w, wd, scale):
    g = np.asarray(g).astype(f32)                       # (a float16 gradient widens exactly)
    wd = f32(wd)
    if wd != 0:
        g = g + wd * (f32(2.0) * w)
    return g * f32(scale)


def momentum_update(w, a, g, lr, mu):
    a2 = a * f32(mu) + g
    return w - a2 * f32(lr), a2


def adam_alpha(lr, b1p, b2p):
    return f32(f32(f32(lr) * np.sqrt(f32(f32(1.0) - f32(b2p)))) / f32(f32(1.0) - f32(b1p)))


def adam_update(w, m, v, g, alpha, beta1, beta2, eps):
    omb1, omb2 = f32(f32(1.0) - f32(beta1)), f32(f32(1.0) - f32(beta2))
    m2 = m + (g - m) * omb1
    v2 = v + (g * g - v) * omb2
    return w - (m2 * f32(alpha)) / (np.sqrt(v2) + f32(eps)), m2, v2


class Restated:
    """The optimizer's whole state over a variable list.  variables: float32 or float16 arrays (copied); a float16 variable
    gets a float32 master created from its value."""

    def __init__(self, kind, variables, weight_decays, boundaries=(), values=(0.01,), momentum=0.9, beta1=0.9, beta2=0.999,
                 epsilon=1e-8):
        assert kind in ('momentum', 'adam')
        self.kind = kind
        self.vars = [np.array(v, copy=True) for v in variables]
        self.masters = [v.astype(f32) if v.dtype == np.float16 else None for v in self.vars]
        self.wds = [f32(w) for w in weight_decays]
        self.boundaries, self.values = list(boundaries), [f32(v) for v in values]
        self.momentum, self.beta1, self.beta2, self.epsilon = f32(momentum), f32(beta1), f32(beta2), f32(epsilon)
        self.step = 0
        self.b1p, self.b2p = f32(beta1), f32(beta2)
        self.slot0 = [np.zeros(v.shape, f32) for v in self.vars]
        self.slot1 = [np.zeros(v.shape, f32) for v in self.vars] if kind == 'adam' else [None] * len(self.vars)

    def w32(self, i):
        return self.masters[i] if self.masters[i] is not None else self.vars[i]

    def l2(self):
        per = np.array([l2_loss(self.w32(i), self.wds[i]) for i in range(len(self.vars))], f32)
        return per, add_n(per)

    def apply(self, grads, scales=None):
        """one step; grads[i] None = skipped.  Returns the L2 losses of the PRE-update values (per tensor, total)."""
        scales = scales if scales is not None else [1.0] * len(self.vars)
        out = self.l2()
        lr = piecewise_constant(self.step, self.boundaries, self.values)
        alpha = adam_alpha(lr, self.b1p, self.b2p) if self.kind == 'adam' else None
        with np.errstate(all='ignore'):
            for i, g in enumerate(grads):
                if g is None:
                    continue
                w = self.w32(i)
                g = effective_gradient(g, w, self.wds[i], scales[i])
                if self.kind == 'momentum':
                    w2, self.slot0[i] = momentum_update(w, self.slot0[i], g, lr, self.momentum)
                else:
                    w2, self.slot0[i], self.slot1[i] = adam_update(w, self.slot0[i], self.slot1[i], g, alpha, self.beta1,
                                                                   self.beta2, self.epsilon)
                assert w2.dtype == f32
                if self.masters[i] is not None:
                    self.masters[i] = w2
                    self.vars[i] = w2.astype(np.float16)            # nearest-even, once
                else:
                    self.vars[i] = w2
        self.step += 1
        if self.kind == 'adam':
            self.b1p, self.b2p = f32(self.b1p * self.beta1), f32(self.b2p * self.beta2)
        return out


def chunk_table(numels):
    """(first_chunk per tensor, [(tensor, offset)]) as training.py builds them"""
    first, chunks = [], []
    for t, n in enumerate(numels):
        first.append(len(chunks))
        chunks.extend((t, o) for o in range(0, n, CH))
    return first, chunks
