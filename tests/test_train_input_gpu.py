"""odet_preprocess_train / preprocess_training_batch / losses_from_raw_images on the GPU: every image element, every box and
the offsets bit-identical (0 ulp; float16 compared as bits) to the numpy restatement of the reference's training input stage
(tests/train_input_np.py), the Philox flip flags, graph capture, and the chain into the fused targets and the caller models."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import targets_np as tn
import train_input_np as ti
from tf_eager_object_detection_amd import preprocess as P

pytestmark = pytest.mark.gpu

F = np.float32


def _raw(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _boxes(g, seed):
    """g rows (ymin, xmin, ymax, xmax): mostly inside [0, 1], some outside it, some with their corners the wrong way round,
    and products that sit exactly on an integer"""
    rng = np.random.default_rng(seed)
    b = rng.uniform(-0.2, 1.3, (g, 4)).astype(F)
    b[::3] = np.sort(rng.uniform(0, 1, (len(b[::3]), 4)).astype(F).reshape(-1, 2, 2), axis=1).reshape(-1, 4)
    b[1::7] = rng.integers(0, 11, (len(b[1::7]), 4)).astype(F) / F(10)
    return b


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


def _same_bits(got, want, msg=''):
    assert got.dtype == want.dtype and got.shape == want.shape, (msg, got.dtype, want.dtype, got.shape, want.shape)
    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=msg)


# ---- single images -----------------------------------------------------------------------------------------------------
# raw size -> edges.  (1, 1), (1, 2): the smallest; (5, 7) -> 8 x 11: the quoted non-commuting case; (97, 61): odd, portrait;
# (333, 517): 3 * w is no multiple of 16, so the partial chunks at both row ends are reversed; (375, 500): the flagship
SIZES = {(1, 1): {}, (1, 2): {}, (5, 7): dict(min_edge=8, max_edge=12), (97, 61): {}, (333, 517): {}, (375, 500): {}}


@functools.lru_cache(maxsize=None)
def _single_want(hw, norm, flip):
    raw, bx = _raw(*hw, seed=hw[0] * 7 + hw[1]), _boxes(9, hw[0] + hw[1])
    img, gb, off = ti.batch([raw], [bx], norm, [flip], True, **SIZES[hw])
    for a in (img, gb, off):
        a.setflags(write=False)
    return raw, bx, img, gb, off


@pytest.mark.parametrize('flip', [False, True], ids=['unflipped', 'flipped'])
@pytest.mark.parametrize('norm', ['caffe', 'tf'])
@pytest.mark.parametrize('hw', sorted(SIZES), ids=['%dx%d' % s for s in sorted(SIZES)])
def test_single_image_bit_exact(hw, norm, flip):
    raw, bx, img, gb, off = _single_want(hw, norm, flip)
    if hw == (5, 7):
        assert img.shape == (1, 8, 11, 3)
    lb = np.arange(9, dtype=np.int64) + 1
    for dtype, cast, source in ((torch.float32, np.float32, raw), (torch.float16, np.float16, torch.from_numpy(raw).cuda())):
        got = P.preprocess_training_batch([source], [bx], [lb], norm, flip=[flip], dtype=dtype, **SIZES[hw])
        batch, gt_boxes, gt_labels, gt_offsets, flipped = got
        assert batch.dtype == dtype and flipped == [flip]
        _same_bits(batch.cpu().numpy(), img.astype(cast), 'image')          # float16: the float32 result rounded once
        _same_bits(gt_boxes.cpu().numpy(), gb, 'boxes')
        assert gt_labels.dtype == torch.int32 and gt_labels.cpu().numpy().tolist() == lb.tolist()
        assert gt_offsets.dtype == torch.int32 and gt_offsets.cpu().numpy().tolist() == off.tolist() == [0, 9]
    if flip and hw[1] > 1:                                # (the flip is real work: the unflipped restatement differs)
        assert np.any(img != _single_want(hw, norm, False)[2])
        assert np.any(gb != _single_want(hw, norm, False)[3])


@pytest.mark.parametrize('norm', ['caffe', 'tf'])
@pytest.mark.parametrize('hw', [(97, 61), (333, 517)], ids=['97x61', '333x517'])
def test_augment_off_is_the_eval_entry_point_and_the_plain_scaling(hw, norm):
    raw, bx = _raw(*hw, seed=3), _boxes(12, 5)
    lb = np.zeros(12, np.int32)
    for dtype in (torch.float32, torch.float16):
        batch, gt_boxes, _, gt_offsets, flipped = P.preprocess_training_batch([raw], [bx], [lb], norm, augment=False, seed=9,
                                                                             dtype=dtype)
        ev = P.preprocess_images([raw], 'coco', norm, dtype=dtype)[0]
        assert flipped == [False]
        _same_bits(batch.cpu().numpy(), ev.cpu().numpy())
        H, W = batch.shape[1:3]
        _same_bits(gt_boxes.cpu().numpy(), ti.boxes(bx, hw[0], hw[1], H, W, augment=False))
        want = np.stack([bx[:, 1] * F(W - 1), bx[:, 0] * F(H - 1), bx[:, 3] * F(W - 1), bx[:, 2] * F(H - 1)], axis=1)
        _same_bits(gt_boxes.cpu().numpy(), want)
        assert gt_offsets.cpu().numpy().tolist() == [0, 12]


# ---- a batch ---------------------------------------------------------------------------------------------------------------
EDGES = dict(min_edge=150, max_edge=250)
TARGET = (150, 200)
G8 = [3, 0, 1, 1024, 0, 7, 2, 5]
FLIP8 = [True, False, True, True, False, False, True, False]


def _batch_sizes(n):
    """n distinct raw sizes (odd widths among them) that resize to TARGET under the coco rule"""
    out = []
    for h in list(range(75, 700, 29)) + list(range(76, 700)):
        for w in (int(round(h * TARGET[1] / TARGET[0])) + d for d in (1, 0, -1)):
            if (h, w) not in out and P.resized_shape(h, w, pipeline='coco', **EDGES)[:2] == TARGET:
                out.append((h, w))
                break
        if len(out) == n:
            return out
    raise AssertionError('not enough sizes')


@functools.lru_cache(maxsize=None)
def _batch_want(norm):
    sizes = _batch_sizes(8)
    assert len(set(sizes)) == 8 and any(w % 2 for _, w in sizes)
    raws = [_raw(h, w, seed=40 + i) for i, (h, w) in enumerate(sizes)]
    bxs = [_boxes(g, 60 + i) for i, g in enumerate(G8)]
    img, gb, off = ti.batch(raws, bxs, norm, FLIP8, True, **EDGES)
    for a in (img, gb, off):
        a.setflags(write=False)
    return sizes, raws, bxs, img, gb, off


@pytest.mark.parametrize('norm', ['caffe', 'tf'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.float16], ids=['f32', 'f16'])
def test_batch_of_eight_mixed_sources_flags_and_box_counts(norm, dtype):
    sizes, raws, bxs, img, gb, off = _batch_want(norm)
    ims = [raws[0], torch.from_numpy(raws[1])] + [torch.from_numpy(r).cuda() for r in raws[2:7]]
    # the last source: a GPU view inside a wider buffer, starting at an odd column (byte offset 15, row pitch 3 * (w + 13))
    h, w = sizes[7]
    wide = torch.zeros((h, w + 13, 3), dtype=torch.uint8, device='cuda')
    wide[:, 5:5 + w] = torch.from_numpy(raws[7]).cuda()
    view = wide[:, 5:5 + w]
    assert view.stride() == (3 * (w + 13), 3, 1) and not view.is_contiguous()
    ims.append(view)
    lbs = [np.arange(g, dtype=np.int64) % 20 + 1 for g in G8]
    lbs[5] = torch.from_numpy(lbs[5])                            # (a CPU tensor is a host array too)
    batch, gt_boxes, gt_labels, gt_offsets, flipped = P.preprocess_training_batch(ims, bxs, lbs, norm, flip=FLIP8,
                                                                                 dtype=dtype, **EDGES)
    assert tuple(batch.shape) == (8,) + TARGET + (3,) and batch.dtype == dtype and flipped == FLIP8
    g = batch.cpu().numpy()
    cast = np.float32 if dtype == torch.float32 else np.float16
    for i in range(8):
        _same_bits(g[i], img[i].astype(cast), 'image %d %s' % (i, sizes[i]))
    _same_bits(gt_boxes.cpu().numpy(), gb)
    assert gt_offsets.cpu().numpy().tolist() == off.tolist() == np.cumsum([0] + G8).tolist()
    assert gt_labels.cpu().numpy().tolist() == np.concatenate([np.asarray(l) for l in lbs]).tolist()


# ---- the flip rule ---------------------------------------------------------------------------------------------------------
SEEDS = (1, 2 ** 32 + 5)                                         # (one above 2^32: the high seed word takes part)


@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('first', [0, 64, 2 ** 32 - 64])
def test_philox_flags(seed, first):
    """64 images of 1 x 2 pixels, resized to 1 x 2: the flag is visible in the output"""
    raws = [_raw(1, 2, 200 + i) for i in range(64)]
    none = [np.zeros((0, 4), F)] * 64, [np.zeros(0, np.int32)] * 64
    edges = dict(min_edge=1, max_edge=2)
    want = ti.flip_flags(seed, first, 64)
    assert 0 < sum(want) < 64                                    # both values occur
    batch, gt_boxes, _, gt_offsets, flipped = P.preprocess_training_batch(raws, *none, 'tf', seed=seed, first_image_id=first,
                                                                         **edges)
    assert flipped == want == [P.flip_decision(seed, first + b) for b in range(64)]
    assert tuple(batch.shape) == (64, 1, 2, 3) and gt_boxes.shape == (0, 4) and gt_offsets.cpu().numpy().tolist() == [0] * 65
    _same_bits(batch.cpu().numpy(), ti.batch(raws, none[0], 'tf', want, True, **edges)[0])
    # a function of (seed, image id) alone: the same ids at other positions of another batch
    moved = P.preprocess_training_batch(raws[:32], none[0][:32], none[1][:32], 'tf', seed=seed, first_image_id=first + 32,
                                        **edges)[4]
    assert moved == want[32:]
    one = P.preprocess_training_batch(raws[:1], none[0][:1], none[1][:1], 'tf', seed=seed, first_image_id=first + 63,
                                      **edges)[4]
    assert one == want[63:]


def test_the_seed_matters():
    a, b = (ti.flip_flags(s, 0, 64) for s in SEEDS)
    assert a != b


# ---- graph capture -----------------------------------------------------------------------------------------------------
def test_the_call_captures_into_a_graph_with_its_flags_baked_in():
    """odet_preprocess_train itself (every buffer already on the device): no host read, no allocation; a replay repeats the
    flags of the capturing call"""
    from tf_eager_object_detection_amd import _lib as L
    sizes, raws, bxs, img, gb, off = _batch_want('caffe')
    B = 8
    dev = [torch.from_numpy(r).cuda() for r in raws]
    boxes_in = torch.from_numpy(np.concatenate(bxs)).cuda()
    n = int(off[-1])

    def launch(out, gt_boxes, gt_offsets):
        L.call('odet_preprocess_train', (C.c_void_p * B)(*[t.data_ptr() for t in dev]), (C.c_int * B)(*[h for h, _ in sizes]),
               (C.c_int * B)(*[w for _, w in sizes]), (C.c_longlong * B)(*[3 * w for _, w in sizes]), B, TARGET[0], TARGET[1], 0,
               (C.c_double * 3)(*ti.MEANS), L.dptr(boxes_in), (C.c_int * (B + 1))(*off.tolist()), 1,
               (C.c_int * B)(*[int(f) for f in FLIP8]), 0, 0, L.dptr(out), 0, L.dptr(gt_boxes), L.dptr(gt_offsets), None,
               L.stream())

    def buffers():
        return (torch.zeros((B,) + TARGET + (3,), device='cuda'), torch.zeros((n, 4), device='cuda'),
                torch.zeros(B + 1, dtype=torch.int32, device='cuda'))
    eager = buffers()
    launch(*eager)                                       # (also the warm-up: the kernel attributes are set once per device)
    torch.cuda.synchronize()
    held = buffers()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s), torch.cuda.graph(g, stream=s):
        launch(*held)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        for t in held:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(held, eager):
            assert torch.equal(a, b)
    _same_bits(held[0].cpu().numpy(), np.ascontiguousarray(img))
    _same_bits(held[1].cpu().numpy(), np.ascontiguousarray(gb))
    assert held[2].cpu().numpy().tolist() == off.tolist()


# ---- the chain into the fused targets ------------------------------------------------------------------------------------------
def test_chain_into_the_fused_anchor_target():
    """two small scenes -> preprocess_training_batch -> FusedAnchorTarget.batch == targets_np.anchor_target on the restated
    boxes, bit for bit"""
    from tf_eager_object_detection_amd.model.anchor_target import FusedAnchorTarget
    edges = dict(min_edge=64, max_edge=96)
    raws = [_raw(40, 60, 1), _raw(80, 120, 2)]
    assert [P.resized_shape(r.shape[0], r.shape[1], pipeline='coco', **edges)[:2] for r in raws] == [(64, 96)] * 2
    bxs = [np.array([[0.1, 0.1, 0.62, 0.5], [0.3, 0.45, 0.9, 0.95], [0.0, 0.0, 0.4, 0.3]], F),
           np.array([[0.2, 0.5, 0.75, 0.85], [0.05, 0.05, 0.55, 0.6]], F)]
    lbs = [np.array([1, 2, 3]), np.array([4, 5])]
    flips = [True, False]
    # one level, stride 8 on 64 x 96, three shapes of area 32^2 per cell: 8 * 12 * 3 = 288 anchors
    ys, xs = np.meshgrid(np.arange(8) * 8.0, np.arange(12) * 8.0, indexing='ij')
    wh = np.array([[45.0, 23.0], [32.0, 32.0], [23.0, 45.0]])
    cx, cy = xs.reshape(-1, 1), ys.reshape(-1, 1)
    anchors = np.stack([cx - wh[:, 0] / 2, cy - wh[:, 1] / 2, cx + wh[:, 0] / 2, cy + wh[:, 1] / 2], axis=-1).reshape(-1, 4)
    anchors = anchors.astype(F)
    hyper = dict(pos=0.5, neg=0.3, total=32, max_pos=8, means=(0.0, 0.0, 0.0, 0.0), stds=(0.1, 0.1, 0.2, 0.2))
    batch, gt_boxes, _, gt_offsets, flipped = P.preprocess_training_batch(raws, bxs, lbs, flip=flips, **edges)
    layer = FusedAnchorTarget(hyper['pos'], hyper['neg'], hyper['total'], hyper['max_pos'], hyper['means'], hyper['stds'], seed=7)
    got = layer.batch(gt_boxes, gt_offsets, (64, 96), torch.from_numpy(anchors).cuda(), first_image_id=3, parity=True)
    sampled = 0
    for b in range(2):
        gt = ti.boxes(bxs[b], raws[b].shape[0], raws[b].shape[1], 64, 96, True, flips[b])
        want = tn.anchor_target(gt, (64, 96), anchors, hyper['pos'], hyper['neg'], hyper['total'], hyper['max_pos'],
                                hyper['means'], hyper['stds'], seed=7, image_id=3 + b)
        for k, v in want.items():
            g = np.ascontiguousarray(getattr(got, k)[b].cpu().numpy())
            if v.dtype == np.float32:
                _same_bits(g, v, 'image %d %s' % (b, k))
            else:
                np.testing.assert_array_equal(g, v, err_msg='image %d %s' % (b, k))
        c = want['counts']
        assert c[3] > 0 and c[3] + c[4] == hyper['total']
        sampled += int(c[1] > c[3]) + int(c[2] > c[4])
    assert sampled >= 2                                  # the sampler had to choose: the Philox streams 0 / 1 took part


# ---- losses_from_raw_images against the manual chain -------------------------------------------------------------------
def _reset(m, seed):
    """a caller model back at its first training call: the target layers' image ids and torch's random stream (the 'torch'
    target layers' shuffles, the head's dropout)"""
    for layer in (m._anchor_target, m._proposal_target):
        if hasattr(layer, '_next_image_id'):
            layer._next_image_id = 0
    torch.manual_seed(seed)


@pytest.mark.parametrize('kind', ['hip', 'torch'])
def test_losses_from_raw_images_matches_the_manual_chain(kind):
    from tf_eager_object_detection_amd.model.base_fpn_model import ResnetV1Fpn
    from tf_eager_object_detection_amd.model.raw_images import losses_from_raw_images
    torch.manual_seed(1)
    m = ResnetV1Fpn(depth=50, training_targets=kind, training_losses=kind)
    edges = dict(min_edge=256, max_edge=352)
    raws = [_raw(128, 176, 31), _raw(150, 131, 32), _raw(256, 352, 33)]          # two resized shapes, in mixed order
    shapes = [P.resized_shape(r.shape[0], r.shape[1], pipeline='coco', **edges)[:2] for r in raws]
    assert shapes[0] == shapes[2] == (256, 352) and shapes[1] != shapes[0]
    bxs = [np.array([[0.12, 0.11, 0.78, 0.52], [0.4, 0.17, 0.98, 0.71]], F)] * 3
    lbs = [np.array([3, 7]), np.array([5, 9]), np.array([1, 20])]
    seed, first = 11, 40
    flags = ti.flip_flags(seed, first, 3)
    want = []
    _reset(m, 5)
    for i in range(3):
        batch, gb, gl, _, fl = P.preprocess_training_batch([raws[i]], [bxs[i]], [lbs[i]], seed=seed, first_image_id=first + i,
                                                           **edges)
        assert fl == [flags[i]]
        want.append([float(x) for x in m((batch, gb, gl), True)])
    _reset(m, 5)
    got, flipped = losses_from_raw_images(m, raws, bxs, lbs, seed=seed, first_image_id=first, **edges)
    assert flipped == flags and len(got) == 3 and all(len(t) == 4 for t in got)
    got = [[float(x) for x in t] for t in got]
    print('\n%s\n%s' % (want, got))
    # real losses: finite, both cross-entropies positive (a regression loss is 0 when an image has no foreground row:
    # a randomly initialised model proposes none for some images)
    assert np.all(np.isfinite(np.array(want))) and np.array(want)[:, [0, 2]].min() > 0
    _same_bits(np.array(got, F), np.array(want, F))
    # explicit flags override the rule, and change the result
    _reset(m, 5)
    other, flipped = losses_from_raw_images(m, raws, bxs, lbs, seed=seed, first_image_id=first, flip=[not f for f in flags],
                                            **edges)
    assert flipped == [not f for f in flags]
    assert [[float(x) for x in t] for t in other] != got
