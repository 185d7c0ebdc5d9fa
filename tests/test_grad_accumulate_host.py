"""The K-image training step without a GPU: the export and the host-side error returns of odet_bucket_accumulate_f32,
training.GradientAccumulator on CPU tensors against tests/grad_accumulate_np.py by bytes on data whose image order and division
show (both shares measured here, on the CPU), the signed zeros, the fixed gradient set of a window, the state round trip in the
middle of a window, and the checkpoint files of training.Trainer: their names, the latest one, the restore order, and an epoch's
log lines and save schedule."""
import os

import numpy as np
import pytest
import torch

import grad_accumulate_np as anp

NUMELS = [0, 1, 3, 4095, 4096, 4097, 2 * 4096 + 5]
SHAPES = [(0,), (1,), (3,), (4095,), (64, 64), (4097,), (7, 1171)]
ABSENT = 2                                     # the gradient of this variable is None


def _bits(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().numpy()
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _variables():
    return [torch.zeros(s) for s in SHAPES]


def _grads(arrays):
    return [None if a is None else torch.from_numpy(a.copy()).reshape(s) for a, s in zip(arrays, SHAPES)]


def _same(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert (g is None) == (w is None), i
        if g is not None:
            assert np.array_equal(_bits(g).reshape(-1), _bits(w)), i


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_abi_export_and_host_side_error_returns():
    from tf_eager_object_detection_amd import _lib
    Lb = _lib.lib()
    assert hasattr(Lb, 'odet_bucket_accumulate_f32') and 'odet_bucket_accumulate_f32' in _lib.SIGNATURES
    P = 0x10000                                                      # pointer-valued integers nothing dereferences
    INVALID, LIMIT = -1, -4

    def acc(tensors=P, numels=P, T=2, chunks=P, K=2, bucket=P, BK=4, first=1, divisor=1.0):
        return Lb.odet_bucket_accumulate_f32(tensors, numels, T, chunks, K, bucket, BK, first, divisor, None), Lb.odet_last_error()

    rows = [('first 2', acc(first=2), INVALID), ('first -1', acc(first=-1), INVALID),
            ('divisor 0', acc(divisor=0.0), INVALID), ('divisor -0', acc(divisor=-0.0), INVALID),
            ('divisor negative', acc(divisor=-2.0), INVALID), ('divisor inf', acc(divisor=float('inf')), INVALID),
            ('divisor -inf', acc(divisor=float('-inf')), INVALID), ('divisor nan', acc(divisor=float('nan')), INVALID),
            ('divisor 0, later call', acc(first=0, divisor=0.0), INVALID),
            ('null bucket', acc(bucket=None), INVALID), ('misaligned bucket', acc(bucket=P + 4), INVALID),
            ('table larger than the bucket', acc(K=5), INVALID),
            # pack's other conditions and limits
            ('null tensors', acc(tensors=None), INVALID), ('null numels', acc(numels=None), INVALID),
            ('null chunks', acc(chunks=None), INVALID), ('negative T', acc(T=-1), INVALID), ('negative K', acc(K=-1), INVALID),
            ('negative bucket', acc(BK=-1), INVALID), ('chunks without tensors', acc(T=0), INVALID),
            ('T over the limit', acc(T=_lib.OPT_MAX_TENSORS + 1), LIMIT),
            ('bucket over the limit', acc(BK=_lib.OPT_MAX_CHUNKS + 1), LIMIT)]
    for label, (rc, msg), want in rows:
        print('%s -> %d %r' % (label, rc, msg))
        assert rc == want, (label, rc, msg)
        assert msg.startswith(b'odet_bucket_accumulate_f32') and b' failed: ' not in msg, msg   # (refused before any HIP call)
    # no-ops that launch nothing: an empty bucket, and a later call over an empty table
    assert acc(tensors=None, numels=None, T=0, chunks=None, K=0, bucket=None, BK=0)[0] == 0
    assert acc(K=0, first=0, divisor=3.0)[0] == 0


def test_python_front_refuses_a_bad_divisor_before_the_library():
    from tf_eager_object_detection_amd import ops
    tb = ops.BucketTables([4], 1)
    for d in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='divisor'):
            ops.bucket_accumulate(tb, [torch.zeros(4)], torch.zeros(4096), True, d)


# ---- the data is sharp ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [3, 5])
def test_data_shows_the_image_order_and_the_division(K):
    lists = anp.image_lists(K, NUMELS, 40 + K, absent=(ABSENT,))
    order, division = anp.order_share(lists), anp.division_share(lists)
    print('K = %d: the reversed order changes %.3f of the elements, a reciprocal multiply %.3f' % (K, order, division))
    assert order >= 0.25 and division >= 0.25
    # the restatement takes the ascending order and the division
    x = anp._flat(lists)
    s = x[0].copy()
    for k in range(1, K):
        s = (s + x[k]).astype(np.float32)
    want = (s / np.float32(K)).astype(np.float32)
    got = np.concatenate([a for a in anp.window(lists, True) if a is not None])
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(np.concatenate([a for a in anp.window(lists, False) if a is not None])), _bits(s))


def test_restatement_first_call_overwrites_a_nan_bucket_with_positive_zero():
    lists = anp.image_lists(2, NUMELS, 3, absent=(ABSENT,))
    b = anp.accumulate(None, lists[0], True, 1.0, bucket_chunks=9)
    assert b.size == 9 * 4096 and not np.isnan(b).any()
    used = np.zeros(b.size, bool)
    first, chunks, _ = anp.gnp.layout([None if a is None else a.size for a in lists[0]], 1)
    assert chunks == 1 + 1 + 1 + 2 + 3
    for a, f in zip(lists[0], first):
        if a is not None:
            used[f * 4096:f * 4096 + a.size] = True
    assert not _bits(b[~used]).any()                                             # +0.0, not -0.0
    marked = b.copy()
    marked[~used] = 77.0
    later = anp.accumulate(marked, lists[1], False, 2.0, bucket_chunks=9)
    assert (later[~used] == 77.0).all()                                          # a later call writes the tensors' elements only


# ---- GradientAccumulator on CPU tensors ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('average', [True, False], ids=['mean', 'sum'])
@pytest.mark.parametrize('K', [1, 2, 3, 5])
def test_accumulator_on_cpu_tensors_equals_the_restatement(K, average):
    from tf_eager_object_detection_amd import training
    acc = training.GradientAccumulator(_variables(), K, average=average)
    views = None
    for window in range(2):                                                      # the second window overwrites the first
        lists = anp.image_lists(K, NUMELS, 40 + K + 100 * window, absent=(ABSENT,))
        for k in range(K):
            assert acc.pending == k
            grads = _grads(lists[k])
            out = acc.add(grads)
            assert (out is None) == (k < K - 1)
        assert acc.pending == 0
        _same(out, anp.window(lists, average))
        assert [None if o is None else tuple(o.shape) for o in out] == [None if i == ABSENT else s for i, s in enumerate(SHAPES)]
        if K == 1:
            assert all(o is g for o, g in zip(out, grads))                       # as given, nothing copied
        elif views is None:
            views = out
        else:
            assert all(a is b for a, b in zip(views, out))                       # the same tensors in every window


def test_negative_zero():
    from tf_eager_object_detection_amd import training
    v = [torch.zeros(3)]
    minus = torch.tensor([-0.0, -0.0, 1.0])
    out = training.GradientAccumulator(v, 1).add([minus])
    assert out[0] is minus and _bits(out[0])[0] == 0x80000000                     # K = 1: the input's bits
    acc = training.GradientAccumulator(v, 2, average=False)
    assert acc.add([minus.clone()]) is None
    assert _bits(acc._layouts[(3,)].bucket)[0] == 0x80000000                      # the first image's bits, -0.0 included
    out = acc.add([torch.tensor([0.0, -0.0, 1.0])])
    assert list(_bits(out[0])) == [0x00000000, 0x80000000, int(_bits(np.float32([2.0]))[0])]      # (-0) + (+0) = +0
    assert _bits(anp.window([[np.float32([-0.0])], [np.float32([0.0])]], False)[0])[0] == 0
    assert _bits(anp.window([[np.float32([-0.0])]], True)[0])[0] == 0x80000000


def test_a_changed_gradient_set_raises_and_leaves_the_window():
    from tf_eager_object_detection_amd import training
    K = 3
    lists = anp.image_lists(K, NUMELS, 9, absent=(ABSENT,))
    acc = training.GradientAccumulator(_variables(), K)
    acc.add(_grads(lists[0]))
    before = acc.state_dict()
    bad = _grads(lists[1])
    bad[1] = None
    with pytest.raises(ValueError, match='set of present gradients'):
        acc.add(bad)
    more = _grads(lists[1])
    more[ABSENT] = torch.ones(SHAPES[ABSENT])
    with pytest.raises(ValueError, match='set of present gradients'):
        acc.add(more)
    with pytest.raises(TypeError):
        acc.add([None if g is None else g.half() for g in _grads(lists[1])])
    with pytest.raises(ValueError):
        acc.add(_grads(lists[1])[:-1])
    after = acc.state_dict()
    assert acc.pending == 1 and after['count'] == 1 and after['numels'] == before['numels']
    assert np.array_equal(_bits(after['bucket']), _bits(before['bucket']))
    assert acc.add(_grads(lists[1])) is None
    _same(acc.add(_grads(lists[2])), anp.window(lists, True))
    # reset drops an open window: the next image is a first image again, with any set
    acc.add(_grads(lists[0]))
    acc.reset()
    assert acc.pending == 0
    assert acc.add(bad) is None and acc.pending == 1
    with pytest.raises(ValueError):
        training.GradientAccumulator(_variables(), 0)
    with pytest.raises(TypeError):
        training.GradientAccumulator([torch.zeros(3).half()], 2)


@pytest.mark.parametrize('at', [1, 2])
def test_state_round_trip_in_the_middle_of_a_window(at):
    from tf_eager_object_detection_amd import training
    K = 3
    lists = anp.image_lists(K, NUMELS, 17, absent=(ABSENT,))
    acc = training.GradientAccumulator(_variables(), K)
    for k in range(at):
        acc.add(_grads(lists[k]))
    state = acc.state_dict()
    assert state['count'] == at and state['numels'] == [None if i == ABSENT else n for i, n in enumerate(NUMELS)]
    acc.add(_grads(lists[at]))                                                   # (the saved bucket is a copy: this does not reach it)
    fresh = training.GradientAccumulator(_variables(), K)
    fresh.load_state_dict(state)
    assert fresh.pending == at
    out = None
    for k in range(at, K):
        out = fresh.add(_grads(lists[k]))
    _same(out, anp.window(lists, True))
    closed = fresh.state_dict()
    assert closed['count'] == 0 and closed['bucket'] is None and closed['numels'] is None
    fresh.load_state_dict(closed)
    assert fresh.pending == 0
    with pytest.raises(ValueError):
        training.GradientAccumulator(_variables(), K + 1).load_state_dict(state)
    with pytest.raises(ValueError):
        training.GradientAccumulator(_variables(), K, average=False).load_state_dict(state)


# ---- checkpoints ---------------------------------------------------------------------------------------------------------------
class _Model:
    def __init__(self, seed):
        torch.manual_seed(seed)
        self.dense = torch.nn.Linear(5, 3)


class _Optimizer:
    """what Trainer needs of an optimizer to save and restore: a step count and a state"""

    def __init__(self, step=0):
        self.global_step = torch.tensor(step)

    def state_dict(self):
        return {'global_step': int(self.global_step)}

    def load_state_dict(self, state):
        self.global_step = torch.tensor(state['global_step'])


def test_checkpoint_names_and_the_latest_checkpoint(tmp_path):
    from tf_eager_object_detection_amd import training
    d = str(tmp_path)
    assert training.latest_checkpoint(d) is None and training.latest_checkpoint(os.path.join(d, 'missing')) is None
    assert training.checkpoint_path(d, 10) == os.path.join(d, 'model.ckpt-10')
    written = []
    for step in (9, 100, 10):
        written.append(training.Trainer(_Model(1), _Optimizer(step)).save(d))
    assert [os.path.basename(p) for p in written] == ['model.ckpt-9', 'model.ckpt-100', 'model.ckpt-10']
    for other in ('model.ckpt-', 'model.ckpt-1000.tmp', 'model.ckpt-x', 'checkpoint', 'xmodel.ckpt-5000'):
        open(os.path.join(d, other), 'w').close()
    assert training.latest_checkpoint(d) == os.path.join(d, 'model.ckpt-100')          # by number: 100 after 10 after 9
    os.remove(os.path.join(d, 'model.ckpt-100'))
    assert training.latest_checkpoint(d) == os.path.join(d, 'model.ckpt-10')


def test_save_and_restore_carry_the_whole_state(tmp_path):
    from tf_eager_object_detection_amd import training
    a = training.Trainer(_Model(1), _Optimizer(7), images_per_step=2)
    grads = [torch.full_like(p, 0.1 * (i + 1)) for i, (_, p) in enumerate(a.named)]
    assert a.accumulator.add(grads) is None
    a.images_seen = 15
    path = a.save(str(tmp_path))
    assert os.path.basename(path) == 'model.ckpt-7'
    b = training.Trainer(_Model(2), _Optimizer(0), images_per_step=2)
    assert not torch.equal(b.model.dense.weight, a.model.dense.weight)
    b.restore(path)
    assert b.images_seen == 15 and b.global_step() == 7 and b.accumulator.pending == 1
    for (n, p), (_, q) in zip(a.named, b.named):
        assert np.array_equal(_bits(p), _bits(q)), n
    more = [torch.full_like(p, 0.3) for _, p in a.named]
    for x, y in zip(a.accumulator.add(more), b.accumulator.add(more)):
        assert np.array_equal(_bits(x), _bits(y))


def test_train_one_epoch_logs_the_reference_line_and_saves_on_its_schedule(tmp_path, capsys):
    from tf_eager_object_detection_amd import training

    class Stepping(training.Trainer):
        def step(self, inputs):                                                  # (the model's part is the GPU tests')
            self.images_seen += 1
            self.optimizer.global_step = self.optimizer.global_step + 1
            return tuple(torch.tensor(x) for x in (0.5, 0.25, 1.0, 0.125)), True

    opt = _Optimizer(0)
    opt._schedule = training.piecewise_constant([2], [0.001, 0.0001])
    t = Stepping(_Model(1), opt)
    d = str(tmp_path)
    t.train_one_epoch(range(7), logging_every_n_steps=3, save_every_n_steps=2, save_path=d)
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith('steps')]
    # train.py:150: idx + 1, the learning rate, the four losses, the L2 loss, the total; lr from the step AFTER the update
    assert lines == ['steps 1, lr is 0.00100, loss: 0.5000, 0.2500, 1.0000, 0.1250, 0.0000, 1.8750',
                     'steps 4, lr is 0.00010, loss: 0.5000, 0.2500, 1.0000, 0.1250, 0.0000, 1.8750',
                     'steps 7, lr is 0.00010, loss: 0.5000, 0.2500, 1.0000, 0.1250, 0.0000, 1.8750']
    # saved at idx 2, 4, 6 (idx % 2 == 0 and idx != 0), after that image's step: global steps 3, 5, 7
    assert sorted(os.listdir(d)) == ['model.ckpt-3', 'model.ckpt-5', 'model.ckpt-7']
    t.train_one_epoch(range(3), logging_every_n_steps=100, save_every_n_steps=1, save_path=None)     # no path: nothing saved
    assert sorted(os.listdir(d)) == ['model.ckpt-3', 'model.ckpt-5', 'model.ckpt-7']


def test_train_restores_the_explicit_file_first_and_then_the_directory(tmp_path):
    from tf_eager_object_detection_amd import training
    ckpt_dir, other = str(tmp_path / 'ckpt'), str(tmp_path / 'other')
    explicit = training.Trainer(_Model(3), _Optimizer(500)).save(other)
    for step in (9, 10):
        training.Trainer(_Model(4), _Optimizer(step)).save(ckpt_dir)

    class Recording(training.Trainer):
        def restore(self, path):
            calls.append(path)
            super().restore(path)

    calls = []
    t = Recording(_Model(5), _Optimizer(0))
    t.train([], 0, ckpt_dir, restore_ckpt_file_path=explicit)
    assert calls == [explicit, os.path.join(ckpt_dir, 'model.ckpt-10')]
    assert t.global_step() == 10                                                 # the directory's latest checkpoint wins
    calls = []
    t = Recording(_Model(5), _Optimizer(0))
    t.train([], 0, str(tmp_path / 'empty'), restore_ckpt_file_path=explicit)
    assert calls == [explicit] and t.global_step() == 500
    calls = []
    Recording(_Model(5), _Optimizer(0)).train([], 0, str(tmp_path / 'empty'))
    assert calls == []
