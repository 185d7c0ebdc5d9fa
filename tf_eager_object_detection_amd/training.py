"""The training step: the counterpart of the reference's scripts/train.py:22-50 (train_step, the L2 regulariser, the
piecewise-constant learning rate, MomentumOptimizer / AdamOptimizer.apply_gradients) on csrc/optimizer.hip.

The whole variable list is updated by ONE update launch and one finish launch (ops.optimizer_step); the global step, the Adam
beta powers and the schedule live in a small state block on the device, so a step reads nothing back and can be captured in
a graph.  Arithmetic: include/odet.h "training step" (TF r1.13's ApplyMomentum / ApplyAdam, float32, bit for bit;
tests/optimizer_np.py restates it).

Deviations from the reference, both forced by how this package holds its parameters:
  * frozen batch normalisation is folded into the convolution kernels here (model/layers.py _fold_frozen_bn), so
    the L2 regulariser acts on the FOLDED tensors, not on the raw kernels keras regularises;
  * the float16 detector modes hold float16 parameters: the optimizer keeps a float32 master per float16 variable (created
    from its value); the update and the L2 term use the master and the variable is the master rounded to nearest-even once.
A variable is updated in its MEMORY order, so it has to be dense (contiguous in the default or the channels-last sense) and
its gradient has to have the same shape and strides.

Graph capture: bind the gradient tensors first (`prepare(grads_and_vars)` uploads the tables), capture `apply_gradients`
with the same tensors, and write later gradients INTO them.  A capture that meets other gradient pointers raises.  The
version counters of the updated parameters are bumped when `apply_gradients` is called, not when a graph replays: after a
replay call `mark_updated()` so that the tensors the detectors derive from their weights rebuild.  The one rule (derived.py):
a derived tensor is valid while every source is the same object with the same (data_ptr, version, dtype, device, shape,
stride) -- in-place ops through the tensor, load_state_dict and this step rebuild by themselves; `.data` / set_() writes need
derived.invalidate (ops.invalidate_planes, the detectors' prepare()); a captured graph keeps the derived tensors it was captured with.
"""
import collections
import ctypes as C

import torch

from . import _lib as L
from . import ops

PiecewiseConstant = collections.namedtuple('PiecewiseConstant', ['boundaries', 'values'])


def piecewise_constant(boundaries, values):
    """tf.train.piecewise_constant on the global step: values[i] with i = the number of boundaries strictly below the step.
    Returns the schedule (a host description; the optimizer evaluates it on the device)."""
    boundaries, values = [int(b) for b in boundaries], [float(v) for v in values]
    if len(values) != len(boundaries) + 1:
        raise ValueError('The length of boundaries should be 1 less than the length of values')
    if any(b1 <= b0 for b0, b1 in zip(boundaries, boundaries[1:])):
        raise ValueError('boundaries must be strictly increasing')
    if len(boundaries) > ops.OPT_MAX_BOUNDARIES:
        raise ValueError('%d boundaries exceed the limit of %d' % (len(boundaries), ops.OPT_MAX_BOUNDARIES))
    return PiecewiseConstant(tuple(boundaries), tuple(values))


def learning_rate_at(schedule, step):
    """host evaluation of a schedule (float32 value as a Python float), for logging"""
    return schedule.values[sum(1 for b in schedule.boundaries if b < int(step))]


_dense = ops.memory_dense


class _Optimizer:
    _KIND = None
    _SLOTS = ()

    def __init__(self, learning_rate, device=None):
        self._schedule = learning_rate if isinstance(learning_rate, PiecewiseConstant) \
            else piecewise_constant([], [float(learning_rate)])
        self._device = torch.device(device) if device is not None else None
        self._state = None
        self._store = {}              # id(variable) -> {'var', 'slot0', 'slot1', 'master'}
        self._key = None
        self._tables = None
        self._variables = []
        self._pending = None

    # ---- the device state block -------------------------------------------------------------------------------------------
    def _hyper(self):
        return {}

    def _initial_state(self):
        st = L.OdetOptState()
        st.global_step = 0
        h = self._hyper()
        st.beta1_power, st.beta2_power = h.get('beta1', 0.0), h.get('beta2', 0.0)
        for i, b in enumerate(self._schedule.boundaries):
            st.boundaries[i] = b
        for i, v in enumerate(self._schedule.values):
            st.values[i] = v
        return st

    def _state_block(self, device=None):
        if self._state is None:
            dev = self._device or (torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device()))
            if dev.type != 'cuda':
                raise L.OdetError('the optimizer state must live on the GPU: tf_eager_object_detection_amd has no CPU path')
            self._device = dev
            self._state = torch.frombuffer(bytearray(bytes(self._initial_state())), dtype=torch.uint8).to(dev)
        return self._state

    @property
    def global_step(self):
        """the global step as a DEVICE tensor (int64, 0-dim view of the state block): 0 before the first step"""
        return self._state_block()[0:8].view(torch.int64)[0]

    @property
    def beta_powers(self):
        """(beta1_power, beta2_power) as a device float32 [2] view of the state block (Adam)"""
        return self._state_block()[8:16].view(torch.float32)

    # ---- tables -----------------------------------------------------------------------------------------------------------
    def _entry(self, v):
        e = self._store.get(id(v))
        if e is None or e['var'] is not v:
            e = {'var': v}
            for s in self._SLOTS:
                e[s] = torch.zeros(v.numel(), dtype=torch.float32, device=v.device)
            # the float32 master of a float16 variable, created from its value (memory order, like the slots)
            e['master'] = torch.as_strided(v.detach(), (v.numel(),), (1,)).float() if v.dtype == torch.float16 else None
            self._store[id(v)] = e
        return e

    def prepare(self, grads_and_vars, grad_scales=None, weight_decays=None):
        """Builds (or reuses) the device tables of this variable list and binds the gradient tensors: everything a following
        `apply_gradients` with the same tensors needs is then on the device (what a graph capture requires).  No step is taken."""
        gv = [(g, v) for g, v in grads_and_vars]
        n = len(gv)
        scales = [1.0] * n if grad_scales is None else [float(s) for s in grad_scales]
        wds = [0.0] * n if weight_decays is None else [float(w) for w in weight_decays]
        if len(scales) != n or len(wds) != n:
            raise ValueError('grad_scales / weight_decays must have one entry per variable')
        ptrs, gf16 = [], []
        for i, (g, v) in enumerate(gv):
            if not isinstance(v, torch.Tensor) or not v.is_cuda:
                raise L.OdetError('variable %d must live on the GPU: tf_eager_object_detection_amd has no CPU path' % i)
            if v.dtype not in (torch.float32, torch.float16):
                raise TypeError('variable %d must be float32 or float16, got %s' % (i, v.dtype))
            if not _dense(v):
                raise ValueError('variable %d is not dense in memory (shape %s, strides %s)' % (i, tuple(v.shape), v.stride()))
            if g is None:
                ptrs.append(0)
                gf16.append(None)
                continue
            if not g.is_cuda or g.device != v.device:
                raise L.OdetError('gradient %d must live on the GPU of its variable' % i)
            if g.dtype not in (torch.float32, torch.float16):
                raise TypeError('gradient %d must be float32 or float16, got %s' % (i, g.dtype))
            if g.shape != v.shape or (g.numel() > 1 and g.stride() != v.stride() and not (g.is_contiguous() and v.is_contiguous())):
                raise ValueError('gradient %d (shape %s, strides %s) does not have the layout of its variable (shape %s, strides %s)'
                                 % (i, tuple(g.shape), g.stride(), tuple(v.shape), v.stride()))
            ptrs.append(g.data_ptr())
            gf16.append(g.dtype == torch.float16)
        key = tuple((id(v), v.data_ptr(), v.numel(), v.dtype, s, w) for (_, v), s, w in zip(gv, scales, wds))
        if key != self._key:
            dev = gv[0][1].device if gv else (self._device or torch.device('cuda', torch.cuda.current_device()))
            self._state_block(dev)
            if gv and dev != self._device:
                raise L.OdetError('the variables live on %s, the optimizer state on %s' % (dev, self._device))
            if torch.cuda.is_current_stream_capturing():
                raise L.OdetError('the variable list changed inside a graph capture: call prepare() before capturing')
            records = []
            for (g, v), s, w, h in zip(gv, scales, wds, gf16):
                r = dict(self._entry(v))
                r.update(weight_decay=w, grad_scale=s, grad_f16=bool(h))
                records.append(r)
            self._tables = ops.OptimizerTables(records, self._device)
            self._variables = [v for _, v in gv]
            self._key = key
            if self._pending is not None:
                pending, self._pending = self._pending, None
                self._load_slots(pending)
        else:
            # a gradient that changed its dtype changes its variable's record
            changed = False
            for r, h in zip(self._tables._keep, gf16):
                if h is not None and h != r['grad_f16']:
                    r['grad_f16'] = h
                    changed = True
            if changed:
                self._tables.write_tensors()
        self._tables.set_gradients(ptrs)
        self._bound = [g for g, _ in gv]                       # (the pointer column refers to these)
        return self._tables

    def apply_gradients(self, grads_and_vars, grad_scales=None, weight_decays=None, l2=False):
        """One step over the list of (gradient, variable) pairs; a gradient of None skips its variable (variable, slots and
        master untouched, version counter not bumped).  grad_scales: per variable 1 or 2; weight_decays: per variable, 0 =
        unregularised.  l2=True returns ops.OptimizerOutputs (the total L2 loss and the per-variable losses of the PRE-update
        values, device tensors that the next step overwrites), else None."""
        gv = [(g, v) for g, v in grads_and_vars]
        tables = self.prepare(gv, grad_scales, weight_decays)
        out = ops.optimizer_step(tables, self._state_block(), self._KIND, len(self._schedule.boundaries), l2=l2, **self._hyper())
        self._updated = [v for g, v in gv if g is not None]
        self.mark_updated()
        return out

    def get_slot(self, var, name):
        """The slot tensor of a variable this optimizer has seen: 'momentum' (MomentumOptimizer), 'm' / 'v' (AdamOptimizer) or
        'master' (the float32 master of a float16 variable, else None); flat float32 in the variable's memory order."""
        e = self._store.get(id(var))
        if e is None or e['var'] is not var:
            raise KeyError('the optimizer holds no slots for this variable')
        if name == 'master':
            return e['master']
        if name not in self._SLOT_NAMES:
            raise KeyError('%s has no slot %r' % (type(self).__name__, name))
        return e[self._SLOT_NAMES[name]]

    def mark_updated(self):
        """bumps the version counter of every variable the last `apply_gradients` updated (call it after a graph replay)"""
        if getattr(self, '_updated', None):
            torch.autograd.graph.increment_version(self._updated)

    def l2_loss(self, variables=None, weight_decays=None):
        """The regulariser's forward value over the prepared variable list (or over `variables` with `weight_decays`):
        ops.OptimizerOutputs(total, per variable), nothing updated."""
        if variables is not None:
            self.prepare([(None, v) for v in variables], None, weight_decays)
        if self._tables is None:
            raise ValueError('no variable list: pass variables and weight_decays')
        return ops.l2_loss(self._tables)

    # ---- checkpoint state -------------------------------------------------------------------------------------------------
    def state_dict(self):
        """step, beta powers, and the slots / masters of the prepared variable list in its order (host copies)"""
        st = L.OdetOptState.from_buffer_copy(bytes(self._state_block().cpu().numpy().tobytes()))
        slots = []
        for v in self._variables:
            e = self._store[id(v)]
            slots.append({k: (None if e.get(k) is None else e[k].detach().cpu().clone()) for k in self._SLOTS + ('master',)})
        return {'kind': self._KIND, 'global_step': int(st.global_step), 'beta1_power': float(st.beta1_power),
                'beta2_power': float(st.beta2_power), 'slots': slots}

    def _load_slots(self, slots):
        if len(slots) != len(self._variables):
            raise ValueError('state of %d variables, the prepared list has %d' % (len(slots), len(self._variables)))
        for v, s in zip(self._variables, slots):
            e = self._store[id(v)]
            for k in self._SLOTS + ('master',):
                if (e.get(k) is None) != (s.get(k) is None):
                    raise ValueError('slot %r does not match the variable list' % k)
                if e.get(k) is not None:
                    e[k].copy_(s[k].reshape(e[k].shape))

    def load_state_dict(self, state):
        """restores what state_dict() returned; the slots are applied at once when a variable list is prepared, else at the
        next prepare()"""
        if state['kind'] != self._KIND:
            raise ValueError('state of another optimizer kind')
        st = self._initial_state()
        st.global_step = int(state['global_step'])
        st.beta1_power, st.beta2_power = float(state['beta1_power']), float(state['beta2_power'])
        self._state_block().copy_(torch.frombuffer(bytearray(bytes(st)), dtype=torch.uint8))
        if self._variables:
            self._load_slots(state['slots'])
        else:
            self._pending = state['slots']


class MomentumOptimizer(_Optimizer):
    """tf.train.MomentumOptimizer(learning_rate, momentum) without Nesterov: accum = accum * momentum + grad;
    var -= accum * lr.  learning_rate: a float or a piecewise_constant schedule."""
    _KIND = L.OPT_MOMENTUM
    _SLOTS = ('slot0',)
    _SLOT_NAMES = {'momentum': 'slot0'}

    def __init__(self, learning_rate, momentum, device=None):
        super().__init__(learning_rate, device)
        self.momentum = float(momentum)

    def _hyper(self):
        return {'momentum': self.momentum}


class AdamOptimizer(_Optimizer):
    """tf.train.AdamOptimizer: m, v slots and the two beta powers (which start at beta1, beta2)."""
    _KIND = L.OPT_ADAM
    _SLOTS = ('slot0', 'slot1')
    _SLOT_NAMES = {'m': 'slot0', 'v': 'slot1'}

    def __init__(self, learning_rate, beta1=0.9, beta2=0.999, epsilon=1e-8, device=None):
        if not (0.0 <= beta1 < 1.0 and 0.0 <= beta2 < 1.0 and epsilon >= 0.0):
            raise ValueError('beta1, beta2 must lie in [0, 1) and epsilon must not be negative')
        self.beta1, self.beta2, self.epsilon = float(beta1), float(beta2), float(epsilon)
        super().__init__(learning_rate, device)

    def _hyper(self):
        return {'beta1': self.beta1, 'beta2': self.beta2, 'epsilon': self.epsilon}


def model_variables(model):
    """[(name, parameter)] of a detector in named_parameters() order: the reference's base_model.variables"""
    return [(n, p) for n, p in model.named_parameters()]


def l2_variables(model, weight_decay):
    """{name: weight_decay} of the regularised parameters.  The reference gives kernel_regularizer=l2(weight_decay) to every
    convolution and dense KERNEL and none to a bias; here that is every parameter with dim >= 2.  Frozen batch normalisation is
    folded into the kernels of this package's detectors, so the regulariser acts on the folded tensors."""
    return {n: float(weight_decay) for n, p in model.named_parameters() if p.dim() >= 2}


def grad_scales(names, learning_rate_bias_double):
    """train.py:33-40: 2 for every variable with 'bias' in its name when learning_rate_bias_double, else 1"""
    return [2.0 if learning_rate_bias_double and 'bias' in n else 1.0 for n in names]


def train_step(named_variables, gradients, optimizer, learning_rate_bias_double=False, weight_decays=None, l2=False):
    """train.py:22-50 after the tape: named_variables [(name, variable)], gradients one per variable (None = no gradient this
    step: skipped, as train_step drops it).  weight_decays: {name: weight_decay} (l2_variables) or None.  Returns what
    optimizer.apply_gradients returns."""
    named_variables = list(named_variables)
    gradients = list(gradients)
    if len(gradients) != len(named_variables):
        raise ValueError('%d gradients for %d variables' % (len(gradients), len(named_variables)))
    names = [n for n, _ in named_variables]
    wds = None if weight_decays is None else [float(weight_decays.get(n, 0.0)) for n in names]
    return optimizer.apply_gradients(zip(gradients, (v for _, v in named_variables)),
                                     grad_scales=grad_scales(names, learning_rate_bias_double), weight_decays=wds, l2=l2)
