"""The batched training call without a GPU: that the case table of odet_assign_levels_images (tests/assign_levels_images_np.py)
can fail at all, the new entry point's export and refusal rules through the built library (each returns before any HIP call),
caller_base.check_training_batch on CPU tensors, training.GradientAccumulator with a divisor of its own against
tests/grad_accumulate_np.py by bytes, its state with and without the new key, and Trainer's rule on images_per_call."""
import os

import numpy as np
import pytest
import torch

import assign_levels_images_np as al
import box_edge_cases as ec
import grad_accumulate_np as anp

INVALID, LIMIT = -1, -4


def _bits(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().numpy()
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the kernel's restatement and its cases -----------------------------------------------------------------------------------------
def test_the_table_holds_the_cases_it_names():
    three = al.BY_NAME['b3_n13_counts_13_0_5']
    assert (three.B, three.n, three.cnt()) == (3, 13, [13, 0, 5])
    full = al.BY_NAME['b2_n8192_all_items']
    assert (full.B, full.n, full.cnt()) == (2, 8192, [8192, 8192]) and al.MAX_ROIS == ec.ASSIGN_MAX_ROIS == 8 * 1024
    above = al.BY_NAME['b2_n13_count_above_n']
    assert above.counts[0] > above.n and above.cnt() == [13, 7]
    sweep, which = ec.level_sweep()
    for lo, hi in ec.LEVEL_RANGES:
        edges = al.BY_NAME['b2_level_boundaries_%d_%d' % (lo, hi)]
        assert edges.B == 2 and np.array_equal(_bits(edges.rois[0]), _bits(sweep)) and set(which) == set(range(-1, len(ec.LEVEL_BOUNDARIES)))


@pytest.mark.parametrize('case', al.CASES, ids=lambda c: c.name)
def test_the_images_of_a_case_differ(case):
    """image b's restated level and perm rows differ from every other image's: a wrong image offset changes bytes"""
    _, level, perm, _ = case.restated()
    for b in range(case.B):
        for o in range(b + 1, case.B):
            assert not np.array_equal(case.rois[b], case.rois[o])
            assert not np.array_equal(level[b], level[o]), (b, o)
            assert not np.array_equal(perm[b], perm[o]), (b, o)


@pytest.mark.parametrize('case', al.CASES, ids=lambda c: c.name)
def test_every_non_empty_image_lies_on_two_levels_and_the_restatement_is_a_partition(case):
    out, level, perm, counts = case.restated()
    for b, c in enumerate(case.cnt()):
        assert counts[b].sum() == c
        assert (c == 0) or np.count_nonzero(counts[b]) >= 2, b
        assert np.array_equal(np.sort(perm[b, :c]), np.arange(c))                       # perm counts rows INSIDE the image
        assert np.array_equal(_bits(out[b, :c]), _bits(case.rois[b][perm[b, :c]]))
        assert (np.diff(level[b, :c]) >= 0).all()
        # rows from the count on: nothing written
        assert (out[b, c:] == al.ROI_FILL).all() and (level[b, c:] == al.LEVEL_FILL).all() and (perm[b, c:] == al.PERM_FILL).all()


# ---- the built library ---------------------------------------------------------------------------------------------------------------
_NAMES = ('rois', 'B', 'n', 'count_dev', 'min_level', 'max_level', 'out_rois', 'out_level', 'out_perm', 'out_counts', 'stream')


def test_entry_point_refuses_bad_arguments_before_any_device_call():
    """pointer-VALUED integers nothing dereferences; every row returns before any HIP call, so this runs without a GPU"""
    from tf_eager_object_detection_amd import _lib
    L = _lib.lib()
    assert hasattr(L, 'odet_assign_levels_images') and len(_lib.SIGNATURES['odet_assign_levels_images'][1]) == len(_NAMES)
    good = dict(rois=0x20000, B=3, n=13, count_dev=0x29000, min_level=2, max_level=5, out_rois=0x30000, out_level=0x40000,
                out_perm=0x50000, out_counts=0x60000, stream=None)
    rows = [('B 0', dict(B=0), INVALID), ('B -1', dict(B=-1), INVALID), ('B 65', dict(B=65), LIMIT),
            ('n -1', dict(n=-1), INVALID), ('n 8193', dict(n=8193), LIMIT),
            ('max_level below min_level', dict(min_level=5, max_level=2), INVALID),
            ('nine levels', dict(min_level=0, max_level=8), INVALID),
            ('null rois', dict(rois=None), INVALID), ('null out_rois', dict(out_rois=None), INVALID),
            ('null out_level', dict(out_level=None), INVALID), ('null out_perm', dict(out_perm=None), INVALID),
            ('null out_counts', dict(out_counts=None), INVALID), ('null out_counts, n 0', dict(out_counts=None, n=0), INVALID)]
    for label, bad, want in rows:
        args = dict(good)
        args.update(bad)
        code = L.odet_assign_levels_images(*[args[k] for k in _NAMES])
        msg = L.odet_last_error()
        print('%s -> %d %r' % (label, code, msg))
        assert code == want, '%s returned %d: %r' % (label, code, msg)
        assert msg.startswith(b'odet_assign_levels_images:') and b' failed: ' not in msg, msg           # (no HIP call was made)


def test_header_names_the_new_entry_point():
    from tf_eager_object_detection_amd import _lib, ops
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'odet.h')).read()
    assert 'odet_assign_levels_images' in header.split('#define ODET_VERSION')[0]                      # the list of additions
    assert 'int odet_assign_levels_images(' in header and '#define ODET_ASSIGN_MAX_BATCH 64' in header
    assert '#define ODET_VERSION 103' in header and _lib.ODET_VERSION == 103
    assert ops.ASSIGN_IMAGES_MAX_BATCH == 64 == ops.TARGETS_MAX_BATCH


def test_python_front_refuses_on_cpu_tensors():
    from tf_eager_object_detection_amd import ops
    with pytest.raises(ops.L.OdetError, match='GPU'):                                  # as ops.assign_levels: no CPU path
        ops.assign_levels_images(torch.zeros(2, 5, 4), 2, 5)
    with pytest.raises(TypeError):
        ops.assign_levels_images(np.zeros((2, 5, 4), np.float32), 2, 5)


# ---- check_training_batch ------------------------------------------------------------------------------------------------------------
def _batch(B=2, G=(3, 2), H=32, W=48):
    total = sum(G)
    off = [0]
    for g in G:
        off.append(off[-1] + g)
    return (torch.zeros(B, H, W, 3), torch.zeros(total, 4), torch.zeros(total, dtype=torch.int64), torch.tensor(off, dtype=torch.int32))


def test_check_training_batch_accepts_a_batch_and_returns_host_offsets():
    from tf_eager_object_detection_amd.model.caller_base import check_training_batch
    inputs = _batch()
    images, boxes, labels, off = check_training_batch(inputs, 'hip', 'hip')
    assert images is inputs[0] and boxes is inputs[1] and labels is inputs[2] and off == [0, 3, 5]
    assert check_training_batch(inputs[:3] + ([0, 3, 5],), 'hip', 'hip')[3] == [0, 3, 5]
    assert check_training_batch(_batch(1, (4,)), 'hip', 'hip')[3] == [0, 4]                         # B = 1 takes the same path
    assert check_training_batch(_batch(2, (0, 5)), 'hip', 'hip')[3] == [0, 0, 5]                    # an image without boxes
    assert check_training_batch(_batch(64, (1,) * 64), 'hip', 'hip')[3][-1] == 64


def test_check_training_batch_refusals():
    from tf_eager_object_detection_amd.model.caller_base import check_training_batch
    images, boxes, labels, off = _batch()
    for targets, losses in (('torch', 'torch'), ('hip', 'torch'), ('torch', 'hip')):
        with pytest.raises(ValueError, match='only fused'):
            check_training_batch((images, boxes, labels, off), targets, losses)
    with pytest.raises(ValueError, match='1 .. 64 images'):
        check_training_batch(_batch(65, (1,) * 65), 'hip', 'hip')
    with pytest.raises(ValueError, match='1 .. 64 images'):
        check_training_batch((torch.zeros(0, 32, 48, 3), boxes[:0], labels[:0], off[:1]), 'hip', 'hip')
    for bad in (torch.zeros(32, 48, 3), torch.zeros(2, 3, 32, 48), torch.zeros(2, 32, 48, 1), None):
        with pytest.raises(ValueError, match=r'\[B,H,W,3\]'):
            check_training_batch((bad, boxes, labels, off), 'hip', 'hip')
    for bad in ([0, 3], [0, 3, 5, 5], [0, 3, 4], [0, 3, 6], [1, 3, 5], [0, 4, 3], [0, 6, 5], torch.tensor([0.0, 3.0, 5.0]),
                [0, 3.0, 5], torch.tensor([[0, 3, 5]])):
        with pytest.raises(ValueError, match='gt_offsets'):
            check_training_batch((images, boxes, labels, bad), 'hip', 'hip')
    with pytest.raises(ValueError, match='gt_bboxes'):
        check_training_batch((images, boxes.reshape(-1), labels, off), 'hip', 'hip')
    with pytest.raises(ValueError, match='gt_labels'):
        check_training_batch((images, boxes, labels[:-1], off), 'hip', 'hip')
    with pytest.raises(ValueError, match='gt_offsets'):
        check_training_batch((images, boxes, labels), 'hip', 'hip')


# ---- GradientAccumulator with a divisor of its own -----------------------------------------------------------------------------------
NUMELS = [0, 1, 3, 4095, 4096, 4097, 2 * 4096 + 5]
SHAPES = [(0,), (1,), (3,), (4095,), (64, 64), (4097,), (7, 1171)]
ABSENT = 2


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


def _statement(lists, divisor):
    """grad_accumulate_np's statement with a divisor of its own: the sum in ascending order, one float32 add per list, ONE
    division by float32(divisor) at the end"""
    bucket = None
    for k, arrays in enumerate(lists):
        bucket = anp.accumulate(bucket, arrays, k == 0, float(divisor) if k == len(lists) - 1 else 1.0)
    return anp.gnp.bucket_unpack(bucket, [None if a is None else a.size for a in lists[0]], 1)


@pytest.mark.parametrize('images,divisor', [(2, 4), (1, 2)])
def test_accumulator_with_a_divisor_equals_the_statement(images, divisor):
    from tf_eager_object_detection_amd import training
    acc = training.GradientAccumulator(_variables(), images, divisor=divisor)
    for window in range(2):
        lists = anp.image_lists(images, NUMELS, 70 + images + 100 * window, absent=(ABSENT,))
        out = None
        for k in range(images):
            assert acc.pending == k
            out = acc.add(_grads(lists[k]))
            assert (out is None) == (k < images - 1)
        assert acc.pending == 0
        _same(out, _statement(lists, divisor))
        assert [None if o is None else tuple(o.shape) for o in out] == [None if i == ABSENT else s for i, s in enumerate(SHAPES)]
        # the division is there, and it is by the divisor and not by the number of calls
        plain = _statement(lists, images)
        assert not np.array_equal(_bits(out[4]).reshape(-1), _bits(plain[4]))


def test_the_default_divisor_gives_the_bytes_of_before():
    from tf_eager_object_detection_amd import training
    for K in (1, 3):
        lists = anp.image_lists(K, NUMELS, 33 + K, absent=(ABSENT,))
        acc = training.GradientAccumulator(_variables(), K)
        assert acc.divisor == K
        grads = [_grads(a) for a in lists]
        out = [acc.add(g) for g in grads][-1]
        _same(out, anp.window(lists, True))
        if K == 1:
            assert all(o is g for o, g in zip(out, grads[0]))                        # as given, no launch, nothing copied
    one = training.GradientAccumulator(_variables(), 1, average=False, divisor=4)    # a sum: the pass-through stays
    g = _grads(anp.image_lists(1, NUMELS, 5)[0])
    assert all(o is x for o, x in zip(one.add(g), g))
    with pytest.raises(ValueError):
        training.GradientAccumulator(_variables(), 2, divisor=0)


def test_state_round_trip_with_and_without_the_new_key():
    from tf_eager_object_detection_amd import training
    lists = anp.image_lists(2, NUMELS, 19, absent=(ABSENT,))
    acc = training.GradientAccumulator(_variables(), 2, divisor=4)
    acc.add(_grads(lists[0]))
    state = acc.state_dict()
    assert state['divisor'] == 4 and state['count'] == 1
    fresh = training.GradientAccumulator(_variables(), 2, divisor=4)
    fresh.load_state_dict(state)
    _same(fresh.add(_grads(lists[1])), _statement(lists, 4))
    with pytest.raises(ValueError, match='divides by'):
        training.GradientAccumulator(_variables(), 2).load_state_dict(state)
    # a state written before the key existed: divisor = images
    old = training.GradientAccumulator(_variables(), 2)
    old.add(_grads(lists[0]))
    legacy = old.state_dict()
    del legacy['divisor']
    again = training.GradientAccumulator(_variables(), 2)
    again.load_state_dict(legacy)
    _same(again.add(_grads(lists[1])), anp.window(lists, True))
    with pytest.raises(ValueError, match='divides by'):
        training.GradientAccumulator(_variables(), 2, divisor=4).load_state_dict(legacy)


# ---- Trainer ---------------------------------------------------------------------------------------------------------------------------
class _Model:
    def __init__(self):
        torch.manual_seed(1)
        self.dense = torch.nn.Linear(5, 3)


class _Optimizer:
    global_step = torch.tensor(0)


def test_trainer_refuses_a_step_that_is_no_multiple_of_the_call():
    from tf_eager_object_detection_amd import training
    with pytest.raises(ValueError, match='multiple of images_per_call'):
        training.Trainer(_Model(), _Optimizer(), images_per_step=3, images_per_call=2)
    with pytest.raises(ValueError):
        training.Trainer(_Model(), _Optimizer(), images_per_step=2, images_per_call=0)
    t = training.Trainer(_Model(), _Optimizer(), images_per_step=4, images_per_call=2)
    assert (t.accumulator.images, t.accumulator.divisor) == (2, 4)
    t = training.Trainer(_Model(), _Optimizer(), images_per_step=2, images_per_call=2)
    assert (t.accumulator.images, t.accumulator.divisor) == (1, 2)
    with pytest.raises(ValueError, match='images_per_call'):                          # the three-tuple is one image
        t.step((torch.zeros(1, 8, 8, 3), torch.zeros(1, 4), torch.zeros(1)))
    with pytest.raises(ValueError, match='exactly images_per_call'):
        t.step((torch.zeros(3, 8, 8, 3), torch.zeros(1, 4), torch.zeros(1), [0, 1, 1, 1]))
    t = training.Trainer(_Model(), _Optimizer(), images_per_step=3)
    assert (t.accumulator.images, t.accumulator.divisor, t.images_per_call) == (3, 3, 1)
