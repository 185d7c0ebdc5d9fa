"""The RoI pooling over a batch of images without a GPU: that the shared case table (tests/roi_batch_cases.py) can fail at all, the
launch plan of the batched backward from the shapes alone (odet_roi_pool_backward_images_plan, the function the launcher itself
sizes its launch with), the refusal rules of the four new entry points through the built library (each returns before any HIP
call) and the Python fronts' argument errors on CPU tensors."""

import numpy as np
import pytest
import torch

import roi_batch_cases as bc
import roi_grad_np as rg

INVALID, LIMIT = -1, -4


@pytest.mark.parametrize('case', bc.CASES, ids=lambda c: c.name)
def test_the_images_of_a_case_differ(case):
    """image b's restated out, sel and every tapped dx differ from image b''s: a wrong image offset changes bytes"""
    out, sel, dx = case.restated()
    for b in range(case.B):
        for o in range(b + 1, case.B):
            assert not np.array_equal(case.rois()[b], case.rois()[o]) and not np.array_equal(case.dy()[b], case.dy()[o])
            assert all(not np.array_equal(m[b], m[o]) for m in case.maps())
            assert not np.array_equal(out[b], out[o]), (b, o)
            if sel is not None:
                assert not np.array_equal(sel[b], sel[o]), (b, o)
            for l in set(case.tapped(b)) | set(case.tapped(o)):
                assert not np.array_equal(dx[l][b], dx[l][o]), (b, o, l)


@pytest.mark.parametrize('case', bc.CASES, ids=lambda c: c.name)
def test_at_least_half_of_a_tapped_gradient_is_live(case):
    """of the dx elements of every non-empty image on the levels its RoIs lie on, at least one half is non-zero in the
    restatement (the table's lowest: 0.70, the image with 5 counted RoIs), so a tile written to the wrong place, or not at
    all, shows; an image without RoIs is all zeros and a level nothing taps is too"""
    _, _, dx = case.restated()
    for b, im in enumerate(case.images):
        levels = case.tapped(b)
        assert bool(levels) == (im.cnt > 0)
        for l in range(len(case.maps_hw)):
            if l not in levels:
                assert not dx[l][b].any()
        if levels:
            live = sum(int(np.count_nonzero(dx[l][b])) for l in levels)
            size = sum(dx[l][b].size for l in levels)
            print('%s image %d: %d of %d elements live (%.3f)' % (case.name, b, live, size, live / size))
            assert live * 2 >= size


def test_the_table_covers_what_it_names():
    names = set(bc.BY_NAME)
    assert len([n for n in names if n.startswith('batch_mode_')]) == len(rg.MODES)
    two = bc.BY_NAME['batch3_two_levels_counts_13_0_5']
    assert (two.B, two.maps_hw, two.C, two.P, two.n) == (3, ((9, 11), (5, 6)), 8, 7, 13) and list(two.counts()) == [13, 0, 5]
    assert two.tapped(1) == [] and two.tapped(2) == [0, 1]
    assert bc.BY_NAME['batch9_one_small_level'].B == 9
    assert all(w > 32 for _, w in bc.BY_NAME['batch2_wide_3x33_max2'].maps_hw)
    assert bc.BY_NAME['batch2_c264'].C == 264
    edges = bc.BY_NAME['batch2_roi_level_edges']
    assert edges.level()[0].min() < 0 and edges.level()[0].max() > 2 and edges.tapped(0) == [0, 1, 2] and edges.tapped(1) == [0, 2]
    assert bc.BY_NAME['batch2_dyadic_stride_max2_p7'].images[0].data == 'ints'


# ---- the plan ---------------------------------------------------------------------------------------------------------------------

def _ceil(a, b):
    return -(-a // b)


@pytest.mark.parametrize('case', bc.CASES, ids=lambda c: c.name)
def test_plan_of_every_case(case):
    code, p = bc.plan(case.maps_hw, case.C, case.B, case.n, case.P)
    assert code == 0
    per_level = [h * _ceil(w, 32) * _ceil(case.C, 256) for h, w in case.maps_hw]
    assert p['tiles'] == sum(per_level) and p['grid'] == case.B * sum(per_level)
    assert p['starts'] == [sum(per_level[:l]) for l in range(len(per_level))]
    assert p['slices'] == _ceil(case.C, 256)
    assert p['lds'] == min(max(w for _, w in case.maps_hw), 32) * min(case.C, 256) * 4 and p['lds'] <= 32 * 1024


def test_plan_of_the_bench_shapes_and_its_limits():
    from tf_eager_object_detection_amd import _lib
    L = _lib.lib()
    fpn = ((200, 334), (100, 167), (50, 84), (25, 42))                   # 800 x 1333: P2 .. P5
    code, p = bc.plan(fpn, 256, 8, 512, 7)
    tiles = 200 * 11 + 100 * 6 + 50 * 3 + 25 * 2
    assert code == 0 and p == dict(grid=8 * tiles, tiles=tiles, starts=[0, 2200, 2800, 2950], slices=1, lds=32 * 1024)
    assert bc.plan(fpn, 256, 64, 8192, 16)[0] == 0                       # the limits themselves pass
    for label, args, want in (('B 65', (fpn, 256, 65, 512, 7), LIMIT), ('n 8193', (fpn, 256, 8, 8193, 7), LIMIT),
                              ('P 17', (fpn, 256, 8, 512, 17), LIMIT), ('B 0', (fpn, 256, 0, 512, 7), INVALID),
                              ('C 6', (fpn, 6, 8, 512, 7), INVALID), ('a zero-row level', (((0, 5),), 8, 2, 5, 7), INVALID),
                              ('a level of 2 GiB', (((16384, 16384),), 4, 2, 5, 7), LIMIT),
                              # 2^26 one-cell rows of 4 channels = 1 GiB a level, 2^26 tiles an image: 32 images are 2^31 workgroups
                              ('a grid of 2^31', (((1 << 26, 1),), 4, 32, 5, 7), LIMIT)):
        code, _ = bc.plan(*args)
        msg = L.odet_last_error()
        assert code == want and msg.startswith(b'odet_roi_pool_backward_images_plan') and b' failed: ' not in msg, (label, code, msg)
    code, p = bc.plan(((1 << 26, 1),), 4, 31, 5, 7)                      # ... and 31 are not
    assert code == 0 and p['grid'] == 31 << 26 and p['tiles'] == 1 << 26


# ---- the refusal rules, through the built library: pointer-VALUED integers nothing dereferences; every row returns before any
# HIP call, so this runs without a GPU
_NAMES = {
    'images': ('levels', 'num_levels', 'C', 'B', 'rois', 'roi_level', 'n', 'count_dev', 'norm_mode', 'image_h', 'image_w', 'pool_size',
               'pool_mode', 'out', 'stream'),
    'argmax_images': ('levels', 'num_levels', 'C', 'B', 'rois', 'roi_level', 'n', 'count_dev', 'norm_mode', 'image_h', 'image_w',
                      'pool_size', 'sel', 'stream'),
    'backward_images': ('levels', 'num_levels', 'C', 'B', 'rois', 'roi_level', 'n', 'count_dev', 'norm_mode', 'image_h', 'image_w',
                        'pool_size', 'pool_mode', 'dy', 'sel', 'stream'),
}


def _levels(data=0x100000, H=17, W=17, stride=16.0):
    from tf_eager_object_detection_amd import _lib
    lv = (_lib.OdetLevel * 8)()
    for l in range(8):
        lv[l].data, lv[l].H, lv[l].W, lv[l].stride = (data + 0x1000000 * l if data else 0), H, W, stride
    return lv


def _rows(kind):
    rows = [('B 0', dict(B=0), INVALID), ('B -1', dict(B=-1), INVALID), ('B 65', dict(B=65), LIMIT),
            ('null levels', dict(levels=None), INVALID), ('null rois', dict(rois=None), INVALID),
            ('null level data', dict(levels=_levels(data=0)), INVALID), ('misaligned level data', dict(levels=_levels(data=0x100004)), INVALID),
            ('no roi_level with two levels', dict(roi_level=None), INVALID), ('zero levels', dict(num_levels=0), INVALID),
            ('nine levels', dict(num_levels=9), INVALID), ('C 6', dict(C=6), INVALID), ('C 0', dict(C=0), INVALID),
            ('negative n', dict(n=-1), INVALID), ('zero-row level', dict(levels=_levels(H=0)), INVALID),
            ('pool_size 0', dict(pool_size=0), INVALID), ('misaligned rois', dict(rois=0x20004), INVALID),
            ('misaligned roi_level', dict(roi_level=0x28002), INVALID), ('misaligned count_dev', dict(count_dev=0x29001), INVALID)]
    if kind != 'images':                  # (the forward leaves the modes, strides and sizes to its own launcher's rules, after these)
        rows += [('norm_mode 4', dict(norm_mode=4), INVALID), ('image shape 0 under NORM_IMAGE', dict(norm_mode=1, image_h=0), INVALID),
                 ('stride 0 under NORM_STRIDE', dict(levels=_levels(stride=0.0)), INVALID),
                 ('n 8193', dict(n=8193), LIMIT), ('pool_size 17', dict(pool_size=17), LIMIT),
                 ('a level of 2 GiB', dict(levels=_levels(H=16384, W=16384), C=4), LIMIT)]
    if kind == 'images':
        rows += [('null out', dict(out=None), INVALID), ('misaligned out', dict(out=0x50004), INVALID)]
    elif kind == 'argmax_images':
        rows += [('null sel', dict(sel=None), INVALID), ('misaligned sel', dict(sel=0x40002), INVALID)]
    else:
        rows += [('null dy', dict(dy=None), INVALID), ('misaligned dy', dict(dy=0x30004), INVALID),
                 ('MAX2 without sel', dict(pool_mode=1, sel=None), INVALID), ('NONE with sel', dict(pool_mode=0), INVALID),
                 ('pool_mode 3', dict(pool_mode=3, sel=None), INVALID), ('misaligned sel', dict(sel=0x40002), INVALID),
                 # 2^26 one-cell rows: two levels are 2^27 tiles an image, 16 images 2^31 workgroups
                 ('a grid of 2^31', dict(levels=_levels(H=1 << 26, W=1), C=4, B=16), LIMIT)]
    return rows


@pytest.mark.parametrize('kind', sorted(_NAMES))
def test_entry_points_refuse_bad_arguments_before_any_device_call(kind):
    from tf_eager_object_detection_amd import _lib
    L = _lib.lib()
    fn = getattr(L, 'odet_roi_pool_' + kind)
    good = dict(levels=_levels(), num_levels=2, C=8, B=3, rois=0x20000, roi_level=0x28000, n=13, count_dev=0x29000, norm_mode=0,
                image_h=0, image_w=0, pool_size=7, pool_mode=1, dy=0x30000, sel=0x40000, out=0x50000, stream=None)
    for label, bad, want in _rows(kind):
        args = dict(good)
        args.update(bad)
        code = fn(*[args[k] for k in _NAMES[kind]])
        msg = L.odet_last_error()
        print('%s: %s -> %d %r' % (kind, label, code, msg))
        assert code == want, '%s: %s returned %d: %r' % (kind, label, code, msg)
        assert msg.startswith(b'odet_roi_pool_' + kind.encode() + b':') and b' failed: ' not in msg, msg     # (no HIP call was made)
    # n == 0 is no launch for the forward and the select
    if kind != 'backward_images':
        args = dict(good, n=0, rois=None, sel=None, out=None)
        assert fn(*[args[k] for k in _NAMES[kind]]) == 0


def test_abi_table_and_header_name_the_new_entry_points():
    import os
    from tf_eager_object_detection_amd import _lib, ops
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'odet.h')).read()
    for kind, names in _NAMES.items():
        sym = 'odet_roi_pool_' + kind
        assert sym in header.split('#define ODET_VERSION')[0], sym                                    # the list of additions
        res, args = _lib.SIGNATURES[sym]
        assert len(args) == len(names)
    assert len(_lib.SIGNATURES['odet_roi_pool_backward_images_plan'][1]) == 11
    assert '#define ODET_VERSION 103' in header and _lib.ODET_VERSION == 103
    assert ops.ROI_IMAGES_MAX_BATCH == 64 == ops.TARGETS_MAX_BATCH


# ---- the Python fronts --------------------------------------------------------------------------------------------------------------

def test_python_fronts_refuse_on_cpu_tensors():
    from tf_eager_object_detection_amd import ops
    OdetError = ops.L.OdetError
    maps = [torch.zeros(2, 17, 17, 8)]
    rois = torch.zeros(2, 5, 4)
    dy = torch.zeros(2, 5, 7, 7, 8)
    sel = torch.zeros(2, 5, 7, 7, 8, dtype=torch.uint8)
    kw = dict(strides=[16.0])
    with pytest.raises(ValueError, match='float32'):
        ops.roi_pool_images([maps[0].half()], rois, None, ops.ROI_NORM_STRIDE, 7, ops.ROI_POOL_MAX2, **kw)
    with pytest.raises(ValueError, match='float32'):
        ops.roi_pool_argmax_images([maps[0].half()], rois, None, ops.ROI_NORM_STRIDE, 7, **kw)
    with pytest.raises(ValueError, match='float32'):
        ops.roi_pool_backward_images(dy, [maps[0].half()], rois, None, ops.ROI_NORM_STRIDE, 7, ops.ROI_POOL_AVG2, **kw)
    with pytest.raises(ValueError, match='float32'):
        ops.roi_pool_backward_images(dy.half(), maps, rois, None, ops.ROI_NORM_STRIDE, 7, ops.ROI_POOL_AVG2, **kw)
    with pytest.raises(ValueError, match='float32'):
        ops.roi_pool_trainable_images([maps[0].half()], rois, None, ops.ROI_NORM_STRIDE, 7, ops.ROI_POOL_MAX2, **kw)
    # (the rule on sel against pool_mode comes before anything asks for a device)
    with pytest.raises(ValueError, match='sel'):
        ops.roi_pool_backward_images(dy, maps, rois, None, ops.ROI_NORM_STRIDE, 7, ops.ROI_POOL_MAX2, **kw)
    with pytest.raises(ValueError, match='sel'):
        ops.roi_pool_backward_images(dy, maps, rois, None, ops.ROI_NORM_STRIDE, 7, ops.ROI_POOL_NONE, sel=sel, **kw)
    with pytest.raises(ValueError, match='pool_size'):
        ops.roi_pool_trainable_images(maps, rois, None, ops.ROI_NORM_STRIDE, 17, ops.ROI_POOL_MAX2, **kw)
    with pytest.raises(ValueError, match='images'):
        ops.roi_pool_trainable_images([torch.zeros(65, 3, 3, 8)], torch.zeros(65, 5, 4), None, ops.ROI_NORM_STRIDE, 7, ops.ROI_POOL_MAX2, **kw)
    with pytest.raises(ValueError, match=r'\[B,n,4\]'):
        ops.roi_pool_trainable_images(maps, rois[0], None, ops.ROI_NORM_STRIDE, 7, ops.ROI_POOL_MAX2, **kw)
    for call in (lambda: ops.roi_pool_images(maps, rois, None, ops.ROI_NORM_STRIDE, 7, ops.ROI_POOL_MAX2, **kw),
                 lambda: ops.roi_pool_argmax_images(maps, rois, None, ops.ROI_NORM_STRIDE, 7, **kw),
                 lambda: ops.roi_pool_backward_images(dy, maps, rois, None, ops.ROI_NORM_STRIDE, 7, ops.ROI_POOL_MAX2, sel=sel, **kw)):
        with pytest.raises(OdetError, match='GPU'):                       # (and no CPU path behind the checks)
            call()


def test_roi_pooling_images_is_exported_and_defaults_to_the_plain_path():
    import inspect
    from tf_eager_object_detection_amd.model import roi_pooling as rp
    assert 'roi_pooling_images' in rp.__all__
    sig = inspect.signature(rp.roi_pooling_images)
    assert list(sig.parameters) == ['maps', 'rois', 'roi_level', 'norm_mode', 'pool_size', 'pool_mode', 'strides', 'image_shape',
                                    'count_dev', 'trainable']
    assert sig.parameters['trainable'].default is False
