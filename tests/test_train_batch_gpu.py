"""The batched training call on the GPU, by bytes unless said otherwise: odet_assign_levels_images against
tests/assign_levels_images_np.py and against ops.assign_levels image by image; the four-tuple call with ONE image against the
three-tuple call (four losses, every parameter gradient); every per-image stage of a two-image call against the single-image
functions; the independence of the images of a call; two images against the two one-image calls (the call's gradient is the SUM over
its images); training.Trainer with images_per_call against the three-tuple Trainer and against hand loops, with a resume inside an
open window; and the refusals.  Model and images are those of tests/test_grad_accumulate_gpu.py."""
import numpy as np
import pytest
import torch

import assign_levels_images_np as al
import grad_accumulate_np as anp

pytestmark = pytest.mark.gpu


def _bits(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _raw(t):
    """the bytes of a tensor of any dtype"""
    return np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()


def _mem(t):
    """the tensor's elements in memory order (dense tensors)"""
    return torch.as_strided(t, (t.numel(),), (1,), t.storage_offset())


# ---- 1. the kernel ------------------------------------------------------------------------------------------------------------------
def _prefilled(B, n, L):
    dev = 'cuda'
    return (torch.full((B, n, 4), float(al.ROI_FILL), dtype=torch.float32, device=dev),
            torch.full((B, n), int(al.LEVEL_FILL), dtype=torch.int32, device=dev),
            torch.full((B, n), int(al.PERM_FILL), dtype=torch.int64, device=dev),
            torch.full((B, L), int(al.COUNT_FILL), dtype=torch.int32, device=dev))


def _same_as_restated(got, want, what):
    for name, g, w in zip(('rois', 'level', 'perm', 'counts'), got, want):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        assert g.tobytes() == w.tobytes(), (what, name)


@pytest.mark.parametrize('case', al.CASES, ids=lambda c: c.name)
def test_assign_levels_images_equals_the_restatement_and_the_single_image_entry(case):
    from tf_eager_object_detection_amd import ops
    L = case.max_level - case.min_level + 1
    rois = torch.from_numpy(case.rois).cuda()
    counts = None if case.counts is None else torch.tensor(case.counts, dtype=torch.int32, device='cuda')
    out = _prefilled(case.B, case.n, L)
    got = ops.assign_levels_images(rois, case.min_level, case.max_level, count_dev=counts, out=out)
    assert all(a is b for a, b in zip(got, out))
    _same_as_restated(got, case.restated(), case.name)           # (the fill values included: rows >= cnt_b are not written)
    # image by image against the single-image entry, on the image's own rows and count
    for b, c in enumerate(case.cnt()):
        one = ops.assign_levels(rois[b], case.min_level, case.max_level, count_dev=None if counts is None else counts[b:b + 1])
        for name, g, w in zip(('rois', 'level', 'perm'), got, one):
            assert _raw(g[b, :c]) == _raw(w[:c]), (case.name, b, name)
        assert _raw(got[3][b]) == _raw(one[3]), (case.name, b)
    # no count_dev against counts of n everywhere
    full = torch.full((case.B,), case.n, dtype=torch.int32, device='cuda')
    a = ops.assign_levels_images(rois, case.min_level, case.max_level, out=_prefilled(case.B, case.n, L))
    f = ops.assign_levels_images(rois, case.min_level, case.max_level, count_dev=full, out=_prefilled(case.B, case.n, L))
    assert all(_raw(x) == _raw(y) for x, y in zip(a, f))
    _same_as_restated(a, al.restate(case.rois, None, case.min_level, case.max_level), case.name + ' without counts')


def test_assign_levels_images_without_out_and_with_no_rois():
    from tf_eager_object_detection_amd import ops
    case = al.BY_NAME['b3_n13_counts_13_0_5']
    rois = torch.from_numpy(case.rois).cuda()
    got = ops.assign_levels_images(rois, 2, 5)
    want = al.restate(case.rois, None, 2, 5)
    assert [tuple(g.shape) for g in got] == [(3, 13, 4), (3, 13), (3, 13), (3, 4)]
    assert [g.dtype for g in got] == [torch.float32, torch.int32, torch.int64, torch.int32]
    _same_as_restated(got, want, 'allocated outputs')
    # n == 0: the counts are zeroed, nothing else exists
    out = _prefilled(3, 0, 4)
    got = ops.assign_levels_images(rois[:, :0], 2, 5, out=out)
    assert not got[3].cpu().numpy().any()
    with pytest.raises(ValueError):
        ops.assign_levels_images(rois[0], 2, 5)
    with pytest.raises(ValueError):
        ops.assign_levels_images(rois, 2, 5, count_dev=torch.zeros(2, dtype=torch.int32, device='cuda'))


def test_one_captured_launch_replays_on_new_contents_and_counts():
    from tf_eager_object_detection_amd import ops
    first, second = al.BY_NAME['b3_n13_counts_13_0_5'], al.BY_NAME['b2_n13_count_above_n']
    B, n = 3, 13
    second_rois = np.concatenate([second.rois, first.rois[1:2]])             # three images of new contents
    second_counts = [4, 13, 9]
    rois = torch.from_numpy(first.rois).cuda()
    counts = torch.tensor(first.counts, dtype=torch.int32, device='cuda')
    out = _prefilled(B, n, 4)
    ops.assign_levels_images(rois, 2, 5, count_dev=counts, out=out)          # eager first
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.assign_levels_images(rois, 2, 5, count_dev=counts, out=out)
    rois.copy_(torch.from_numpy(second_rois))
    counts.copy_(torch.tensor(second_counts, dtype=torch.int32))
    for o, fill in zip(out, _prefilled(B, n, 4)):
        o.copy_(fill)
    graph.replay()
    torch.cuda.synchronize()
    _same_as_restated(out, al.restate(second_rois, second_counts, 2, 5), 'replay')
    assert _raw(out[1]) != al.restate(first.rois, first.counts, 2, 5)[1].tobytes()


# ---- the model and its images (tests/test_grad_accumulate_gpu.py) --------------------------------------------------------------------
IMAGE = (256, 352)
MODEL_A = dict(depth=50, training_targets='hip', training_losses='hip', train_neck=True, train_rpn_head=True, train_roi_head=True,
               roi_training_total_num_samples=32, roi_training_max_pos_samples=8)
MODEL_B = dict(MODEL_A, train_extractor=True, train_stem=True)
TRAINED = {'a': 28, 'b': 134}
SAMPLES = 32
WD = 1e-4
LR, MU = 0.01, 0.9
IMAGES = 6
DATA_SEED = 20               # (the seed of tests/test_grad_accumulate_gpu.py; test 5 says which were tried)
LABELS = [3, 7, 12]


def _model(seed, kw=MODEL_A):
    from tf_eager_object_detection_amd.model.base_fpn_model import ResnetV1Fpn
    torch.manual_seed(seed)
    m = ResnetV1Fpn(**kw)
    with torch.no_grad():                                   # (spreads the fresh RpnHead's proposals over sizes and pyramid levels)
        b = m.dense.rpn_bbox.bias
        b.add_(torch.linspace(0.0, 1.6, b.numel(), device=b.device, dtype=b.dtype))
    return m


def _image(k):
    rng = np.random.default_rng(DATA_SEED + k)
    return (rng.uniform(0, 255, (1,) + IMAGE + (3,)) - 110).astype(np.float32)


def _inputs(k, boxes):
    """the three-tuple of image k"""
    return (torch.from_numpy(_image(k)).cuda(), torch.from_numpy(boxes[k]).cuda(), torch.tensor(LABELS, device='cuda'))


def _batch(ks, boxes, device_offsets=True):
    """the four-tuple of the images ks"""
    off = [0]
    for k in ks:
        off.append(off[-1] + len(boxes[k]))
    return (torch.from_numpy(np.concatenate([_image(k) for k in ks])).cuda(),
            torch.from_numpy(np.concatenate([boxes[k] for k in ks])).cuda(), torch.tensor(LABELS * len(ks), device='cuda'),
            torch.tensor(off, dtype=torch.int32, device='cuda') if device_offsets else off)


def _set_image_id(m, k):
    m._anchor_target._next_image_id = k
    m._proposal_target._next_image_id = k


@pytest.fixture(scope='module')
def boxes():
    """ground truth from the model's own proposals, per image, on the weights of seed 1"""
    m = _model(1)
    out = []
    for k in range(IMAGES):
        img = torch.from_numpy(_image(k)).cuda()
        with torch.no_grad():
            p_list = m._neck(m._extractor(img, training=True), training=True)
            scores, deltas = m._get_fpn_head_results(p_list)
            rois = m._rpn_proposal((deltas, m._get_anchors(list(IMAGE)), m._fg_scores(scores), list(IMAGE)), training=True)
        big = rois[((rois[:, 2] - rois[:, 0]) >= 24) & ((rois[:, 3] - rois[:, 1]) >= 24)]
        assert big.shape[0] >= 3, 'the random model proposes fewer than 3 boxes of 24 pixels'
        out.append(big[[0, big.shape[0] // 3, 2 * big.shape[0] // 3]].cpu().numpy().copy())
    return out


@pytest.fixture(scope='module')
def model_a():
    m = _model(1)
    m.keep_training_pass = True
    return m


class _Call:
    """one training call with its backward pass: the losses [4, B], the gradients (flat, memory order; None where there is none) by
    parameter name, and the debug record"""

    def __init__(self, m, inputs, image_id):
        named = list(m.dense.named_parameters())
        _set_image_id(m, image_id)
        m.last_training_pass = None
        losses = m(inputs, True)
        assert len(losses) == 4
        sum(x.sum() for x in losses).backward()
        self.shapes = [tuple(x.shape) for x in losses]
        self.losses = np.stack([x.detach().cpu().numpy().reshape(-1) for x in losses])
        self.grads = {n: None if p.grad is None else _mem(p.grad).cpu().numpy().copy() for n, p in named}
        for _, p in named:
            p.grad = None
        self.rec = m.last_training_pass
        self.ids = (m._anchor_target._next_image_id, m._proposal_target._next_image_id)


def _slices(rec, b):
    """the bytes of image b's slice of every tensor of a debug record"""
    at, pt = rec['anchor_targets'], rec['proposal_targets']
    out = {'rpn_score': rec['rpn_score'][b], 'rpn_deltas': rec['rpn_deltas'][b], 'rois': rec['rois'][b], 'roi_counts': rec['roi_counts'][b],
           'sample_idx': at.sample_idx[b], 'sample_targets': at.sample_targets[b], 'anchor_counts': at.counts[b],
           'final_rois': pt.final_rois[b], 'final_labels': pt.final_labels[b], 'targets': pt.targets[b], 'inside': pt.inside[b],
           'outside': pt.outside[b], 'proposal_counts': pt.counts[b], 'sorted_rois': rec['sorted_rois'][b],
           'roi_level': rec['roi_level'][b], 'row_map': rec['row_map'][b], 'level_counts': rec['level_counts'][b],
           'roi_features': rec['roi_features'][b]}
    out.update({'map%d' % l: p[b] for l, p in enumerate(rec['maps'])})
    return {k: _raw(v) for k, v in out.items()}


RECORD_KEYS = {'rpn_score', 'rpn_deltas', 'maps', 'anchors', 'rois', 'roi_counts', 'anchor_targets', 'proposal_targets', 'sorted_rois',
               'roi_level', 'row_map', 'level_counts', 'roi_features'}


# ---- 2. B = 1 is the old call ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['a', 'b'])
def test_one_image_in_a_four_tuple_is_the_three_tuple_call(which, boxes):
    m = _model(1, MODEL_A if which == 'a' else MODEL_B)
    assert m.keep_training_pass is False and m.last_training_pass is None
    old = _Call(m, _inputs(0, boxes), 5)
    new = _Call(m, _batch([0], boxes), 5)
    assert new.rec is None                                                    # (no record unless asked for)
    assert old.shapes == [()] * 4 and new.shapes == [(1,)] * 4 and old.ids == new.ids == (6, 6)
    assert np.array_equal(_bits(new.losses), _bits(old.losses)) and np.isfinite(old.losses).all() and (old.losses > 0).all()
    assert sum(g is not None for g in old.grads.values()) == TRAINED[which]
    for n in old.grads:
        assert (old.grads[n] is None) == (new.grads[n] is None), n
        if old.grads[n] is not None:
            assert np.array_equal(_bits(new.grads[n]), _bits(old.grads[n])), n
            assert np.abs(old.grads[n]).max() > 0, n
    host = _Call(m, _batch([0], boxes, device_offsets=False), 5)              # (offsets as a host list: the same call)
    assert np.array_equal(_bits(host.losses), _bits(old.losses))


# ---- 3. the stages of a two-image call, image by image -----------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def two_images(model_a, boxes):
    return _Call(model_a, _batch([0, 1], boxes), 5)


def test_every_stage_of_a_two_image_call_is_the_single_image_function(model_a, two_images, boxes):
    from tf_eager_object_detection_amd import ops
    from tf_eager_object_detection_amd.model.base_fpn_model import BaseFPN
    m, rec = model_a, two_images.rec
    assert set(rec) == RECORD_KEYS and two_images.shapes == [(2,)] * 4 and two_images.ids == (7, 7)
    anchors, shape = rec['anchors'], list(IMAGE)
    at, pt = m._anchor_target, m._proposal_target
    assert tuple(rec['rpn_score'].shape) == (2, anchors.shape[0], 2) and tuple(rec['rpn_deltas'].shape) == (2, anchors.shape[0], 4)
    assert rec['rpn_score'].requires_grad and all(p.requires_grad for p in rec['maps']) and len(rec['maps']) == 4
    for b in range(2):
        gt = torch.from_numpy(boxes[b]).cuda()
        labels = torch.tensor(LABELS, device='cuda')
        off = torch.tensor([0, 3], dtype=torch.int32, device='cuda')
        with torch.no_grad():
            fg = m._fg_scores(rec['rpn_score'][b].detach())
            rois = m._rpn_proposal((rec['rpn_deltas'][b].detach(), anchors, fg, shape), training=True)
            cnt = int(rois.shape[0])
            assert int(rec['roi_counts'][b]) == cnt and 32 < cnt <= rec['rois'].shape[1]
            assert _raw(rec['rois'][b, :cnt]) == _raw(rois)
            a1 = at.batch(gt, off, shape, anchors, first_image_id=5 + b, dense=False)
            for name in ('sample_idx', 'sample_targets', 'counts'):
                assert _raw(getattr(rec['anchor_targets'], name)[b]) == _raw(getattr(a1, name)[0]), (b, name)
            p1 = pt.batch(rois[None], gt, labels, off, first_image_id=5 + b, strict=False)
            assert int(p1.counts[0, 3]) == SAMPLES                                # (every row written: the bytes below are data)
            for name in ('final_rois', 'final_labels', 'targets', 'inside', 'outside', 'counts'):
                assert _raw(getattr(rec['proposal_targets'], name)[b]) == _raw(getattr(p1, name)[0]), (b, name)
            srois, level, perm, counts = ops.assign_levels(p1.final_rois[0], m._min_level, m._max_level)
            assert _raw(rec['sorted_rois'][b]) == _raw(srois) and _raw(rec['roi_level'][b]) == _raw(level)
            assert _raw(rec['row_map'][b]) == _raw(perm) and _raw(rec['level_counts'][b]) == _raw(counts)
            assert int((counts > 0).sum()) >= 2, 'the RoIs of image %d lie on one level' % b
            rois_list, _ = m._assign_levels(p1.final_rois[0])
            feats = BaseFPN._get_roi_features(m, rois_list, [p[b:b + 1].detach() for p in rec['maps']], shape)
            assert tuple(rec['roi_features'].shape) == (2, SAMPLES, 7, 7, 256)
            assert _raw(rec['roi_features'][b]) == _raw(feats), b
    assert _raw(rec['rois'][0]) != _raw(rec['rois'][1]) and _raw(rec['row_map'][0]) != _raw(rec['row_map'][1])


# ---- 4. the images of a call are independent -------------------------------------------------------------------------------------------
def test_another_second_image_leaves_the_first_one_as_it_was(model_a, two_images, boxes):
    other = _Call(model_a, _batch([0, 2], boxes), 5)
    assert np.array_equal(_bits(other.losses[:, 0]), _bits(two_images.losses[:, 0]))
    assert all(other.losses[i, 1] != two_images.losses[i, 1] for i in range(4))
    was, now = _slices(two_images.rec, 0), _slices(other.rec, 0)
    for name in was:
        assert was[name] == now[name], name
    was, now = _slices(two_images.rec, 1), _slices(other.rec, 1)
    assert all(was[name] != now[name] for name in ('rpn_score', 'rois', 'sample_idx', 'final_rois', 'roi_features', 'map0'))


# ---- 5. two images against the two one-image calls ----------------------------------------------------------------------------------------
# What was found on the MI355X.  The float32 'exact' dense front gives image b the same bytes at B = 2 as at B = 1:
# rpn_score, rpn_deltas and P2..P5 are asserted byte-equal.  With that every discrete choice is the same at the first data seed
# tried (20, the seed of tests/test_grad_accumulate_gpu.py; no other was tried), and the eight losses came out with a relative
# difference of 0: asserted 0.  The parameter gradients differ in summation order only (the weight gradients add the rows of two
# images in one pass): largest observed max|g2 - (g1_0 + g1_1)| / max|g1_0 + g1_1| = 5.974e-07, at rpn_conv.bias
# (profiles/train_call_bench.json: parity); the bound is 8 x that.
GRAD_OBSERVED = 5.974e-07
GRAD_BOUND = 8 * GRAD_OBSERVED


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def test_two_images_equal_the_two_one_image_calls(model_a, two_images, boxes):
    m, two = model_a, two_images
    ones = [_Call(m, _batch([k], boxes), 5 + k) for k in range(2)]
    # the dense front
    front = {}
    for b in range(2):
        pairs = [('rpn_score', two.rec['rpn_score'][b], ones[b].rec['rpn_score'][0]),
                 ('rpn_deltas', two.rec['rpn_deltas'][b], ones[b].rec['rpn_deltas'][0])]
        pairs += [('P%d' % (l + 2), p2[b], p1[0]) for l, (p2, p1) in enumerate(zip(two.rec['maps'], ones[b].rec['maps']))]
        for name, x, y in pairs:
            front[(b, name)] = (_raw(x) == _raw(y), _rel(x.detach().cpu().numpy(), y.detach().cpu().numpy()))
    print('front (image, tensor): (bytes equal, relative difference)', front)
    assert all(eq for eq, _ in front.values()), front
    # every discrete output
    for b in range(2):
        r2, r1 = two.rec, ones[b].rec
        cnt = int(r1['roi_counts'][0])
        assert int(r2['roi_counts'][b]) == cnt and _raw(r2['rois'][b, :cnt]) == _raw(r1['rois'][0, :cnt]), b
        assert _raw(r2['anchor_targets'].sample_idx[b]) == _raw(r1['anchor_targets'].sample_idx[0]), b
        assert _raw(r2['proposal_targets'].final_rois[b]) == _raw(r1['proposal_targets'].final_rois[0]), b
        assert _raw(r2['proposal_targets'].final_labels[b]) == _raw(r1['proposal_targets'].final_labels[0]), b
    # losses and gradients
    loss_rel = [abs(float(two.losses[i, b]) - float(ones[b].losses[i, 0])) / abs(float(ones[b].losses[i, 0]))
                for i in range(4) for b in range(2)]
    grad_rel, first_alone = {}, {}
    for n, g2 in two.grads.items():
        g0, g1 = ones[0].grads[n], ones[1].grads[n]
        assert (g2 is None) == (g0 is None) == (g1 is None), n
        if g2 is not None:
            both = g0.astype(np.float64) + g1.astype(np.float64)
            grad_rel[n] = _rel(g2, both)
            first_alone[n] = float(np.abs(g0.astype(np.float64) - both).max() / np.abs(both).max())
    print('largest relative loss difference %.3e, largest relative gradient difference %.3e (%s)'
          % (max(loss_rel), max(grad_rel.values()), max(grad_rel, key=grad_rel.get)))
    assert len(grad_rel) == TRAINED['a']
    assert GRAD_BOUND <= 1e-3
    assert max(loss_rel) == 0.0 and np.array_equal(_bits(two.losses), _bits(np.concatenate([o.losses for o in ones], axis=1))), loss_rel
    assert all(v <= GRAD_BOUND for v in grad_rel.values()), {n: v for n, v in grad_rel.items() if v > GRAD_BOUND}
    # an omitted (or double-counted) image is seen: the first image alone fails the same bound almost everywhere
    failing = sum(v > GRAD_BOUND for v in first_alone.values())
    print('the first image alone fails the bound on %d of %d parameters' % (failing, len(first_alone)))
    assert failing >= 0.9 * len(first_alone)


# ---- 6. Trainer ---------------------------------------------------------------------------------------------------------------------------
def _state(m, opt):
    """every parameter and the momentum slot of every trained one, in memory order"""
    torch.cuda.synchronize()
    out = {n: _mem(p.detach()).cpu().numpy().copy() for n, p in m.dense.named_parameters()}
    out.update({n + '/momentum': opt.get_slot(p, 'momentum').cpu().numpy().copy() for n, p in _trained_a(m)})
    return out


def _trained_a(m):
    return [(n, p) for n, p in m.dense.named_parameters() if not n.startswith(('conv', 'bn'))]


def _equal_states(a, b):
    assert sorted(a) == sorted(b)
    for n in a:
        assert np.array_equal(_bits(a[n]), _bits(b[n])), n


def _trainer(m, opt, K, B=1):
    from tf_eager_object_detection_amd import training
    return training.Trainer(m, opt, images_per_step=K, images_per_call=B, learning_rate_bias_double=True, weight_decay=WD)


def _statement(lists, divisor):
    """tests/grad_accumulate_np.py's statement over the calls of a window: the sum in ascending call order, one float32 add per call,
    ONE division by float32(divisor) at the end"""
    bucket = None
    for k, arrays in enumerate(lists):
        bucket = anp.accumulate(bucket, arrays, k == 0, float(divisor) if k == len(lists) - 1 else 1.0)
    return anp.gnp.bucket_unpack(bucket, [None if a is None else a.size for a in lists[0]], 1)


def _hand_step(m, named, opt, flat):
    from tf_eager_object_detection_amd import training
    gradients = []
    for (n, p), g in zip(named, flat):
        if g is None:
            gradients.append(None)
            continue
        t = torch.empty_like(p)                              # (the variable's strides: the bucket holds memory order)
        assert t.stride() == p.stride()
        _mem(t).copy_(torch.from_numpy(g))
        gradients.append(t)
    training.train_step(named, gradients, opt, learning_rate_bias_double=True, weight_decays=training.l2_variables(m.dense, WD))


def test_trainer_fed_four_tuples_of_one_image_is_the_three_tuple_trainer(boxes):
    from tf_eager_object_detection_amd import training
    states = []
    for four in (False, True):
        m = _model(1)
        opt = training.MomentumOptimizer(LR, MU)
        t = _trainer(m, opt, 2)
        stepped = [t.step(_batch([k], boxes) if four else _inputs(k, boxes))[1] for k in range(4)]
        assert stepped == [False, True, False, True] and t.images_seen == 4 and t.global_step() == 2
        states.append(_state(m, opt))
    _equal_states(states[0], states[1])


@pytest.mark.parametrize('K', [2, 4])
def test_trainer_two_images_per_call_equals_the_hand_loop(K, boxes):
    from tf_eager_object_detection_amd import training
    calls = [[0, 1], [2, 3]]
    m = _model(1)
    initial = {n: _mem(p.detach()).cpu().numpy().copy() for n, p in m.dense.named_parameters()}
    opt = training.MomentumOptimizer(LR, MU)
    t = _trainer(m, opt, K, 2)
    stepped = []
    for ks in calls:
        losses, s = t.step(_batch(ks, boxes))
        assert [tuple(x.shape) for x in losses] == [(2,)] * 4
        stepped.append(s)
    W = K // 2
    assert stepped == [(i + 1) % W == 0 for i in range(2)] and t.images_seen == 4 and t.global_step() == 2 // W
    assert t.accumulator.pending == 0 and all(p.grad is None for _, p in t.named)
    assert (m._anchor_target._next_image_id, m._proposal_target._next_image_id) == (4, 4)
    got = _state(m, opt)

    h = _model(1)
    named = training.model_variables(h.dense)
    hopt = training.MomentumOptimizer(LR, MU)
    window, seen = [], 0
    for ks in calls:
        call = _Call(h, _batch(ks, boxes), seen)
        seen += 2
        window.append([call.grads[n] for n, _ in named])
        if len(window) == W:
            assert sum(g is not None for g in window[0]) == TRAINED['a']
            _hand_step(h, named, hopt, _statement(window, K))
            window = []
    _equal_states(got, _state(h, hopt))
    assert seen == t.images_seen
    for n, _ in _trained_a(m):
        assert not np.array_equal(_bits(got[n]), _bits(initial[n])), n                     # the steps moved it


def test_a_run_resumed_inside_an_open_window_of_calls_continues_with_the_same_bits(boxes, tmp_path):
    from tf_eager_object_detection_amd import training
    calls = [[0, 1], [2, 3], [4, 5], [0, 1]]
    m = _model(1)
    opt = training.MomentumOptimizer(LR, MU)
    whole = _trainer(m, opt, 4, 2)
    for ks in calls:
        last, _ = whole.step(_batch(ks, boxes))
    want = _state(m, opt)

    a = _model(1)
    head = _trainer(a, training.MomentumOptimizer(LR, MU), 4, 2)
    for ks in calls[:3]:
        head.step(_batch(ks, boxes))
    assert head.accumulator.pending == 1 and head.images_seen == 6          # a window left open
    path = head.save(str(tmp_path))

    b = _model(2)                                           # another seed: everything has to come from the checkpoint
    bopt = training.MomentumOptimizer(LR, MU)
    tail = _trainer(b, bopt, 4, 2)
    tail.restore(path)
    assert tail.images_seen == 6 and tail.accumulator.pending == 1 and tail.global_step() == 1
    got_last, stepped = tail.step(_batch(calls[3], boxes))
    assert stepped
    _equal_states(_state(b, bopt), want)
    assert tail.global_step() == whole.global_step() == 2 and tail.images_seen == whole.images_seen == 8
    assert np.array_equal(_bits(torch.stack(list(got_last))), _bits(torch.stack(list(last))))


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------------
def _ids(m):
    return (getattr(m._anchor_target, '_next_image_id', None), getattr(m._proposal_target, '_next_image_id', None),
            getattr(m, '_next_dropout_image_id', None))


def test_refusals_leave_the_image_ids_where_they_were(model_a, boxes):
    from tf_eager_object_detection_amd.model.base_faster_rcnn_model import TrainableResNetFasterRcnn, Vgg16FasterRcnn
    from tf_eager_object_detection_amd.model.base_fpn_model import ResnetV1Fpn
    four = _batch([0, 1], boxes)
    _set_image_id(model_a, 11)
    with pytest.raises(ValueError, match=r'\[1,H,W,3\]'):                   # inference with two images: refused as before
        model_a(four[0], False)
    with pytest.raises(ValueError, match='gt_offsets'):
        model_a(four[:3] + (four[3][:2],), True)
    assert _ids(model_a)[:2] == (11, 11)
    plain = ResnetV1Fpn(depth=50)                                           # training_targets='torch'
    before = _ids(plain)
    with pytest.raises(ValueError, match='only fused'):
        plain(four, True)
    assert _ids(plain) == before
    for make in (lambda: Vgg16FasterRcnn(training_targets='hip', training_losses='hip'),
                 lambda: TrainableResNetFasterRcnn(depth=50, roi_pooling_max_pooling_flag=False, training_targets='hip',
                                                   training_losses='hip')):
        single = make()
        before = _ids(single)
        with pytest.raises(ValueError, match='FPN family only'):
            single(four, True)
        assert _ids(single) == before
