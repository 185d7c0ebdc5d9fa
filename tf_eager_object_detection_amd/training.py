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

The loop around the step (second half of this file): GradientAccumulator forms the mean gradient of K images with one
odet_bucket_accumulate_f32 launch per image, in ascending image order; Trainer is train_one_epoch / train of
scripts/train.py:77-202 with checkpoints (model.ckpt-<global_step>) from which a run resumes with the same bits.
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
        if not state['slots'] and not self._variables:
            self._pending = None      # (a state saved before the first step: no variable list, every slot still zero)
        elif self._variables:
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


# ---- steps over K images, and the loop around them (scripts/train.py:77-202) ------------------------------------------------------
def _accumulate_torch(tables, tensors, bucket, first, divisor):
    """ops.bucket_accumulate in torch ops (CPU tensors): one float32 add per element, one float32 division by a TENSOR divisor,
    +0.0 wherever no tensor lives on a first call"""
    if first:
        bucket.zero_()
    for i, t in enumerate(tables.check(tensors)):
        if t is not None and t.numel():
            o, n = tables.offset(i), t.numel()
            g = torch.as_strided(t, (n,), (1,), t.storage_offset())
            s = g.clone() if first else bucket[o:o + n] + g
            if divisor != 1.0:
                s = s / torch.full_like(s, divisor)
            bucket[o:o + n] = s
    return bucket


class _WindowLayout:
    """the bucket of one set of present gradients and the views the window's last image returns"""

    def __init__(self, numels, variables, device):
        self.tables = ops.BucketTables(numels, 1, device)
        self.bucket = torch.zeros(self.tables.bucket_numel, dtype=torch.float32, device=device)
        self.views = [None if n is None else torch.as_strided(self.bucket, tuple(v.shape), v.stride(), self.tables.offset(i))
                      for i, (n, v) in enumerate(zip(numels, variables))]


class GradientAccumulator:
    """One optimizer step over K images (a WINDOW) with ONE launch per image over the whole gradient list
    (odet_bucket_accumulate_f32): the step's gradient is the float32 sum of the images' gradients in ASCENDING IMAGE order,
    starting from the first image's bits, divided by float32(K) once at the end with `average` -- the statement of
    odet_rank_mean_f32, restated by tests/grad_accumulate_np.py.

    add(gradients) takes one float32 gradient or None per variable (GradientExchange's rules) and returns None for images
    1 .. K - 1 of a window; on the K-th it returns a list of VIEWS into the accumulator's own bucket with the variables' shapes
    and strides (None where the gradient is absent): the same tensors in every window, so the optimizer's pointer column is
    uploaded once (and the next window overwrites them).  The set of present gradients is fixed by a window's first image; a
    later image with another set raises ValueError and leaves the window as it was.  images == 1 returns the gradients as given,
    with no launch.  CPU tensors run the same steps in torch ops.

    `divisor` (default: `images`) is what the window's sum is divided by.  A caller whose add() brings the SUM of several images'
    gradients (Trainer with images_per_call = B: a window of W = K / B calls) passes divisor = K.  With images == 1 and a
    divisor above 1 the one call is a window's first and last at once: ONE launch with first = 1 and that divisor."""

    def __init__(self, variables, images, average=True, divisor=None):
        self.variables = list(variables)
        self.images = int(images)
        if self.images < 1:
            raise ValueError('images must be at least 1, got %d' % self.images)
        self.divisor = self.images if divisor is None else int(divisor)
        if self.divisor < 1 or self.divisor >= 1 << 24:
            raise ValueError('divisor must lie in 1 .. 2^24 - 1, got %d' % self.divisor)
        for i, v in enumerate(self.variables):
            if v.dtype != torch.float32:
                raise TypeError('variable %d must be float32, got %s' % (i, v.dtype))
            if not _dense(v):
                raise ValueError('variable %d is not dense in memory (shape %s, strides %s)' % (i, tuple(v.shape), v.stride()))
        self.average = bool(average)
        self._layouts = {}
        self._key = None              # the open window's set of present gradients
        self._count = 0

    @property
    def pending(self):
        """images in the open window (0 = none open)"""
        return self._count

    def reset(self):
        """drops the open window"""
        self._key, self._count = None, 0

    def _layout(self, numels):
        lay = self._layouts.get(numels)
        if lay is None:
            device = self.variables[0].device if self.variables else torch.device('cpu')
            lay = self._layouts[numels] = _WindowLayout(list(numels), self.variables, device)
        return lay

    def add(self, gradients):
        from . import parallel
        gradients = list(gradients)
        parallel.check_gradients(self.variables, gradients)
        if self.images == 1 and (self.divisor == 1 or not self.average):
            return gradients
        numels = tuple(None if g is None else g.numel() for g in gradients)
        if self._count and numels != self._key:
            raise ValueError('image %d of the window has another set of present gradients than its first image' % (self._count + 1))
        lay = self._layout(numels)
        first, last = self._count == 0, self._count + 1 == self.images
        divisor = float(self.divisor) if (last and self.average) else 1.0       # (float32(K) exactly: K < 2^24)
        if lay.tables.bucket_numel:
            if lay.bucket.is_cuda:
                ops.bucket_accumulate(lay.tables, gradients, lay.bucket, first, divisor)
            else:
                _accumulate_torch(lay.tables, gradients, lay.bucket, first, divisor)
        else:
            lay.tables.check(gradients)
        self._key, self._count = numels, self._count + 1
        if not last:
            return None
        self._count = 0
        return list(lay.views)

    def state_dict(self):
        """the open window: its count, its set of present gradients and a host copy of its bucket"""
        open_ = self._count > 0
        return {'images': self.images, 'average': self.average, 'divisor': self.divisor, 'count': self._count,
                'numels': list(self._key) if open_ else None,
                'bucket': self._layouts[self._key].bucket.detach().cpu().clone() if open_ else None}

    def load_state_dict(self, state):
        if int(state['images']) != self.images or bool(state['average']) != self.average:
            raise ValueError('state of an accumulator over %d images (average=%s), this one has %d (average=%s)'
                             % (state['images'], state['average'], self.images, self.average))
        if int(state.get('divisor', state['images'])) != self.divisor:       # (a state from before the key: divisor = images)
            raise ValueError('state of an accumulator that divides by %d, this one divides by %d'
                             % (int(state.get('divisor', state['images'])), self.divisor))
        count = int(state['count'])
        if not 0 <= count < self.images:
            raise ValueError('an open window holds 0 .. %d images, got %d' % (self.images - 1, count))
        if count == 0:
            self.reset()
            return
        numels = tuple(None if n is None else int(n) for n in state['numels'])
        if len(numels) != len(self.variables) or any(n is not None and n != v.numel() for n, v in zip(numels, self.variables)):
            raise ValueError('the state does not match the variable list')
        lay = self._layout(numels)
        if state['bucket'].numel() != lay.bucket.numel():
            raise ValueError('a bucket of %d elements, the layout has %d' % (state['bucket'].numel(), lay.bucket.numel()))
        lay.bucket.copy_(state['bucket'])
        self._key, self._count = numels, count


CHECKPOINT_PREFIX = 'model.ckpt'


def checkpoint_path(directory, global_step):
    """train.py:157: <directory>/model.ckpt-<global_step>"""
    import os
    return os.path.join(directory, '%s-%d' % (CHECKPOINT_PREFIX, int(global_step)))


def latest_checkpoint(directory):
    """tf.train.latest_checkpoint for the files Trainer.save writes: the model.ckpt-<step> of the HIGHEST step (as a number: 100
    after 10 after 9), None when the directory holds none"""
    import os
    import re
    if directory is None or not os.path.isdir(directory):
        return None
    best = None
    for name in os.listdir(directory):
        m = re.fullmatch(re.escape(CHECKPOINT_PREFIX) + r'-(\d+)', name)
        if m and (best is None or int(m.group(1)) > best[0]):
            best = (int(m.group(1)), os.path.join(directory, name))
    return None if best is None else best[1]


class Trainer:
    """The single-process counterpart of scripts/train.py:77-202: train_one_epoch and train around a caller model (model.dense
    holds the parameters), with an optimizer step every `images_per_step` images on the images' mean gradient
    (GradientAccumulator) and a state that resumes a run exactly: the parameters, the optimizer's slots and step, the number of
    images seen -- which is the Philox image id of the target samplers and the dropout -- and the open window.
    weight_decay: None, or the L2 coefficient of l2_variables.  The image summaries and TensorBoard are not built.
    images_per_call=B (the FPN family's batched training call; images_per_step must be a multiple): a step is K / B calls of B
    images each, one backward() per call."""

    LOG_FORMAT = 'steps %d, lr is %.5f, loss: %.4f, %.4f, %.4f, %.4f, %.4f, %.4f'           # train.py:150

    def __init__(self, model, optimizer, images_per_step=1, learning_rate_bias_double=False, weight_decay=None, images_per_call=1):
        self.model, self.optimizer = model, optimizer
        self.learning_rate_bias_double = bool(learning_rate_bias_double)
        self.images_per_step, self.images_per_call = int(images_per_step), int(images_per_call)
        if self.images_per_call < 1 or self.images_per_step < 1 or self.images_per_step % self.images_per_call:
            raise ValueError('images_per_step (%d) must be a positive multiple of images_per_call (%d)'
                             % (self.images_per_step, self.images_per_call))
        self.named = model_variables(model.dense)
        self.weight_decays = None if weight_decay is None else l2_variables(model.dense, weight_decay)
        # a window of W = K / B calls: a call brings the SUM over its B images, the window's sum is divided by float32(K) once
        self.accumulator = GradientAccumulator([p for _, p in self.named], self.images_per_step // self.images_per_call,
                                               divisor=self.images_per_step)
        self.images_seen = 0
        self.l2_loss = None           # of the last optimizer step's pre-update values (a device tensor), with weight_decay

    def step(self, inputs):
        """inputs: (image, gt_bboxes, gt_labels) of ONE image, or the batched call's (images, gt_bboxes, gt_labels, gt_offsets)
        of exactly `images_per_call` images (the only form when that is above 1).  The call's gradient is ONE backward() of the
        sum of its losses; the step's gradient is the calls' gradients added in ascending call order, divided by
        float32(images_per_step) once.  The images get the ids images_seen .. images_seen + B - 1.  Returns (the call's four
        losses as detached device tensors -- scalars for the three-tuple, [B] for the four-tuple --, whether the optimizer
        stepped)."""
        m = self.model
        batched = isinstance(inputs, (tuple, list)) and len(inputs) == 4
        if not batched and self.images_per_call != 1:
            raise ValueError('images_per_call=%d: step takes (images, gt_bboxes, gt_labels, gt_offsets)' % self.images_per_call)
        if batched and (not isinstance(inputs[0], torch.Tensor) or inputs[0].dim() != 4
                        or int(inputs[0].shape[0]) != self.images_per_call):
            raise ValueError('step takes exactly images_per_call=%d images per call' % self.images_per_call)
        image_id = self.images_seen
        m._anchor_target._next_image_id = image_id
        m._proposal_target._next_image_id = image_id
        if hasattr(m, '_next_dropout_image_id'):
            m._next_dropout_image_id = image_id
        losses = m(inputs, True)
        (sum(x.sum() for x in losses) if batched else sum(losses)).backward()
        gradients = self.accumulator.add([p.grad for _, p in self.named])
        for _, p in self.named:
            p.grad = None
        self.images_seen += self.images_per_call
        if gradients is not None:
            out = train_step(self.named, gradients, self.optimizer, learning_rate_bias_double=self.learning_rate_bias_double,
                             weight_decays=self.weight_decays, l2=self.weight_decays is not None)
            if out is not None:
                self.l2_loss = out.l2_loss
        return tuple(x.detach() for x in losses), gradients is not None

    # ---- state ------------------------------------------------------------------------------------------------------------------
    def global_step(self):
        """the optimizer's step count as a Python int (a host read)"""
        return int(self.optimizer.global_step)

    def state_dict(self):
        return {'model': self.model.dense.state_dict(), 'optimizer': self.optimizer.state_dict(),
                'images_seen': self.images_seen, 'accumulator': self.accumulator.state_dict()}

    def load_state_dict(self, state):
        self.model.dense.load_state_dict(state['model'])
        self.optimizer.load_state_dict(state['optimizer'])
        self.images_seen = int(state['images_seen'])
        self.accumulator.load_state_dict(state['accumulator'])

    def save(self, directory):
        """writes <directory>/model.ckpt-<global_step> and returns its path"""
        import os
        os.makedirs(directory, exist_ok=True)
        path = checkpoint_path(directory, self.global_step())
        torch.save(self.state_dict(), path)
        return path

    def restore(self, path):
        self.load_state_dict(torch.load(path, map_location='cpu'))

    # ---- the loop ---------------------------------------------------------------------------------------------------------------
    def train_one_epoch(self, dataset, logging_every_n_steps=20, save_every_n_steps=5000, save_path=None):
        """train.py:77-159 over an iterable of step()'s inputs; idx counts calls (images, as the reference's does, with one image
        per call); a batched call logs the mean of its images' losses"""
        idx = 0
        for inputs in dataset:
            losses, _ = self.step(inputs)
            if idx % logging_every_n_steps == 0:
                four = [float(x.mean()) for x in losses]
                l2 = 0.0 if self.l2_loss is None else float(self.l2_loss)
                lr = learning_rate_at(self.optimizer._schedule, self.global_step())
                print(self.LOG_FORMAT % ((idx + 1, lr) + tuple(four) + (l2, sum(four) + l2)), flush=True)
            if save_path is not None and idx % save_every_n_steps == 0 and idx != 0:
                self.save(save_path)
            idx += 1

    def train(self, dataset, epochs, ckpt_dir, restore_ckpt_file_path=None, logging_every_n_steps=20, save_every_n_steps=5000):
        """train.py:162-202: the explicit checkpoint file first, then the directory's latest checkpoint (which therefore wins),
        then `epochs` passes over the dataset"""
        import time
        if restore_ckpt_file_path is not None:
            self.restore(restore_ckpt_file_path)
        latest = latest_checkpoint(ckpt_dir)
        if latest is not None:
            self.restore(latest)
        for i in range(int(epochs)):
            print('epoch %d starting...' % (i + 1), flush=True)
            start = time.time()
            self.train_one_epoch(dataset, logging_every_n_steps, save_every_n_steps, ckpt_dir)
            print('epoch %d training finished, costing %d seconds...' % (i + 1, time.time() - start), flush=True)
