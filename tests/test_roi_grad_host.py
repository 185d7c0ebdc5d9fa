"""The RoI pooling backward without a GPU: the NumPy restatement (tests/roi_grad_np.py) against torch float64 autograd through a
plain-torch crop_and_resize + max_pool2d / avg_pool2d, the proof that the order of the sums shows in float32 bits, the refusal
rules of odet_roi_pool_argmax / odet_roi_pool_backward through the built library (each returns before any HIP call), and the
Python fronts' argument errors on CPU tensors."""

import numpy as np
import pytest
import torch

import roi_grad_np as rg

EPS = 2.0 ** -24


def _exact_cases():
    # dyadic lerp weights (roi_cases.roi_for coordinates on eighths of a cell), maps in 0..3, dy in -3..3: every product and
    # every partial sum is a small multiple of 2^-12, exact in float32 -- so ANY order gives the same bits and float64 agrees
    out = [rg.dyadic_case(norm, pool) for norm, pool in rg.MODES]
    out.append(rg.fpn_case(4, data='ints'))
    out.append(rg.dyadic_case(rg.NORM_STRIDE, rg.POOL_MAX2, P=1))
    out.append(rg.dyadic_case(rg.NORM_STRIDE, rg.POOL_NONE, P=1))
    return out


@pytest.mark.parametrize('case', _exact_cases(), ids=lambda c: c.name)
def test_exact_data_equals_torch_float64_autograd(case):
    """select + backward == torch float64 autograd through max_pool2d / avg_pool2d, exactly.  Maps of four values make tied
    samples in most bins: the first-maximum rule is exercised against torch's own."""
    maps, dy = case.maps(), case.dy()
    sel = None
    if case.pool == rg.POOL_MAX2:
        sel = rg.select(case, maps)
        tied = 0
        for r in range(case.cnt):
            v = rg.samples(case, maps, r).reshape(case.P, 2, case.P, 2, case.C)
            four = np.stack([v[:, 0, :, 0], v[:, 0, :, 1], v[:, 1, :, 0], v[:, 1, :, 1]])
            tied += int(((four == four.max(axis=0)).sum(axis=0) > 1).sum())
        print('%s: %d bins x channels with tied maxima, sel histogram %s' % (case.name, tied, np.bincount(sel.reshape(-1), minlength=5)))
        assert tied >= 20
    got = rg.backward(case, dy, sel)
    want = rg.torch_backward(case, maps, dy)
    assert any(np.abs(w).max() > 0 for w in want)
    for l, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.float32
        np.testing.assert_array_equal(g.astype(np.float64), w, err_msg='%s level %d' % (case.name, l))
    # exact data: the other orders give the same bits
    for order in ('rois_desc', 'j_first'):
        for g, o in zip(got, rg.backward(case, dy, sel, order=order)):
            np.testing.assert_array_equal(g, o)


def _random_cases():
    return [rg.mode_case(norm, pool, C=8) for norm, pool in rg.MODES] + [rg.fpn_case(8), rg.coords_case('pileup'), rg.order_case(),
                                                                         rg.coords_case('edge_rev'), rg.wide_case()]


@pytest.mark.parametrize('case', _random_cases(), ids=lambda c: c.name)
def test_random_data_within_the_rounding_bound_of_float64(case):
    """Normal data, the restatement's own sel imposed on the torch graph (a gather by index instead of max_pool2d: a near-tie
    between the float32 and the float64 forward cannot enter, and no case is excluded).  Each element lies within
    (count + 4) * 2^-24 * sum|contributions| of the float64 gradient: a contribution wx * (wy * g) carries at most four
    roundings (1 - lerp twice, two products; * 0.25f is exact) and each of the `count` adds one, relative to a partial sum that
    the sum of the absolute contributions bounds."""
    maps, dy = case.maps(), case.dy()
    sel = rg.select(case, maps) if case.pool == rg.POOL_MAX2 else None
    got, num, mag = rg.backward(case, dy, sel, stats=True)
    want = rg.torch_backward(case, maps, dy, sel)
    worst = 0.0
    for l, (g, w, k, m) in enumerate(zip(got, want, num, mag)):
        bound = (k + 4) * EPS * m
        err = np.abs(g.astype(np.float64) - w)
        with np.errstate(invalid='ignore', divide='ignore'):
            worst = max(worst, float(np.nanmax(np.where(bound > 0, err / bound, 0.0))))
        assert (err <= bound).all(), '%s level %d: %g over the bound at %s' % (case.name, l, (err - bound).max(),
                                                                                np.unravel_index(np.argmax(err - bound), err.shape))
        np.testing.assert_array_equal(g[k == 0], 0.0)
    print('%s: worst error / bound = %.3f, deepest sum %d contributions' % (case.name, worst, max(int(k.max()) for k in num)))
    assert max(int(k.max()) for k in num) >= 4


def test_the_order_of_the_sums_shows_in_float32_bits():
    """on the order data set, RoIs descending and j before top / bottom both change bits of dx: the byte comparisons of the GPU
    tests therefore pin the order"""
    case = rg.order_case()
    maps, dy = case.maps(), case.dy()
    sel = rg.select(case, maps)
    base = rg.backward(case, dy, sel)[0]
    for order in ('rois_desc', 'j_first'):
        other = rg.backward(case, dy, sel, order=order)[0]
        differ = int((base.view(np.uint32) != other.view(np.uint32)).sum())
        print('%s: %d of %d elements differ in bits' % (order, differ, base.size))
        assert differ >= base.size // 20
        np.testing.assert_allclose(other, base, rtol=0, atol=1e-4)


def test_select_codes_and_padding_rows():
    """an all-NaN bin gets code 4 (nothing compares equal), a bin with some NaN samples takes the first non-NaN maximum, an
    extrapolated sample (0) can be selected, rows at or beyond the count are 4"""
    case = rg.mode_case(rg.NORM_STRIDE, rg.POOL_MAX2, C=4, count=9)
    maps = [m.copy() for m in case.maps()]
    maps[0][5:9, 4:8, 1] = np.nan
    maps[0][:, :, 2] = -np.abs(maps[0][:, :, 2]) - 1           # negative everywhere: an extrapolated 0 wins where there is one
    sel = rg.select(case, maps)
    assert (sel[9:] == 4).all() and (sel[:9, ..., 0] < 4).all()
    assert (sel[:9, ..., 1] == 4).any() and (sel[:9, ..., 1] < 4).any()
    hit_outside = 0
    for r in range(9):
        _, ty, tx = rg.taps(case, r)
        ok = (ty[1][:, None] & tx[1][None, :]).reshape(case.P, 2, case.P, 2)
        s = sel[r, ..., 2]
        for py in range(case.P):
            for px in range(case.P):
                out4 = [not ok[py, a, px, b] for a in (0, 1) for b in (0, 1)]
                if any(out4):
                    assert s[py, px] == out4.index(True)                  # the first extrapolated sample: 0 > every negative
                    hit_outside += 1
    assert hit_outside >= 10
    # ... and it scatters nothing
    dy = case.dy()
    dx = rg.backward(case, dy, sel)[0]
    assert np.isfinite(dx[..., 0]).all() and np.isfinite(dx[..., 1]).all()


# ---- the refusal rules, through the built library: pointer-VALUED integers nothing dereferences; every row returns before any
# HIP call, so this runs without a GPU
_NAMES = {
    'argmax': ('levels', 'num_levels', 'C', 'rois', 'roi_level', 'n', 'count_dev', 'norm_mode', 'image_h', 'image_w', 'pool_size',
               'sel', 'stream'),
    'backward': ('levels', 'num_levels', 'C', 'rois', 'roi_level', 'n', 'count_dev', 'norm_mode', 'image_h', 'image_w', 'pool_size',
                 'pool_mode', 'dy', 'sel', 'stream'),
}
INVALID, LIMIT = -1, -4


def _levels(nl=2, data=0x100000, H=17, W=17, stride=16.0):
    from tf_eager_object_detection_amd import _lib
    lv = (_lib.OdetLevel * 8)()
    for l in range(8):
        lv[l].data, lv[l].H, lv[l].W, lv[l].stride = (data + 0x100000 * l if data else 0), H, W, stride
    return lv


def _rows(kind):
    rows = [('null levels', dict(levels=None), INVALID), ('null rois', dict(rois=None), INVALID),
            ('null level data', dict(levels=_levels(data=0)), INVALID), ('misaligned level data', dict(levels=_levels(data=0x100004)), INVALID),
            ('no roi_level with two levels', dict(roi_level=None), INVALID), ('zero levels', dict(num_levels=0), INVALID),
            ('nine levels', dict(num_levels=9), INVALID), ('negative levels', dict(num_levels=-1), INVALID),
            ('C 6', dict(C=6), INVALID), ('C 0', dict(C=0), INVALID), ('negative n', dict(n=-1), INVALID),
            ('norm_mode 4', dict(norm_mode=4), INVALID), ('norm_mode -1', dict(norm_mode=-1), INVALID),
            ('image shape 0 under NORM_IMAGE', dict(norm_mode=1, image_h=0), INVALID),
            ('stride 0 under NORM_STRIDE', dict(levels=_levels(stride=0.0)), INVALID), ('zero-row level', dict(levels=_levels(H=0)), INVALID),
            ('pool_size 0', dict(pool_size=0), INVALID), ('misaligned rois', dict(rois=0x20004), INVALID),
            ('n 8193', dict(n=8193), LIMIT), ('pool_size 17', dict(pool_size=17), LIMIT),
            ('a level of 2 GiB', dict(levels=_levels(H=16384, W=16384), C=4), LIMIT)]
    if kind == 'argmax':
        rows += [('null sel', dict(sel=None), INVALID), ('misaligned sel', dict(sel=0x40002), INVALID)]
    else:
        rows += [('null dy', dict(dy=None), INVALID), ('misaligned dy', dict(dy=0x30004), INVALID),
                 ('MAX2 without sel', dict(pool_mode=1, sel=None), INVALID), ('NONE with sel', dict(pool_mode=0), INVALID),
                 ('AVG2 with sel', dict(pool_mode=2), INVALID), ('pool_mode 3', dict(pool_mode=3, sel=None), INVALID),
                 ('pool_mode -1', dict(pool_mode=-1, sel=None), INVALID), ('misaligned sel', dict(sel=0x40002), INVALID)]
    return rows


@pytest.mark.parametrize('kind', ['argmax', 'backward'])
def test_entry_points_refuse_bad_arguments_before_any_device_call(kind):
    from tf_eager_object_detection_amd import _lib
    L = _lib.lib()
    fn = getattr(L, 'odet_roi_pool_' + kind)
    good = dict(levels=_levels(), num_levels=2, C=8, rois=0x20000, roi_level=0x28000, n=13, count_dev=None, norm_mode=0, image_h=0,
                image_w=0, pool_size=7, pool_mode=1, dy=0x30000, sel=0x40000, stream=None)
    for label, bad, want in _rows(kind):
        args = dict(good)
        args.update(bad)
        rc = fn(*[args[k] for k in _NAMES[kind]])
        msg = L.odet_last_error()
        print('%s: %s -> %d %r' % (kind, label, rc, msg))
        assert rc == want, '%s: %s returned %d: %r' % (kind, label, rc, msg)
        assert msg.startswith(b'odet_roi_pool_' + kind.encode()) and b' failed: ' not in msg, msg     # (no HIP call was made)
    # n == 0 is no launch for the select
    if kind == 'argmax':
        args = dict(good, n=0, rois=None, sel=None)
        assert fn(*[args[k] for k in _NAMES[kind]]) == 0


def test_python_fronts_refuse_on_cpu_tensors():
    from tf_eager_object_detection_amd import ops
    maps = [torch.zeros(1, 17, 17, 8)]
    rois = torch.zeros(5, 4)
    dy = torch.zeros(5, 7, 7, 8)
    sel = torch.zeros(5, 7, 7, 8, dtype=torch.uint8)
    with pytest.raises(ValueError, match='float32'):
        ops.roi_pool_argmax([maps[0].half()], rois, None, ops.ROI_NORM_STRIDE, 7, strides=[16.0])
    with pytest.raises(ValueError, match='float32'):
        ops.roi_pool_backward(dy, [maps[0].half()], rois, None, ops.ROI_NORM_STRIDE, 7, ops.ROI_POOL_AVG2, strides=[16.0])
    with pytest.raises(ValueError, match='float32'):
        ops.roi_pool_backward(dy.half(), maps, rois, None, ops.ROI_NORM_STRIDE, 7, ops.ROI_POOL_AVG2, strides=[16.0])
    with pytest.raises(ValueError, match='float32'):
        ops.roi_pool_trainable([maps[0].half()], rois, None, ops.ROI_NORM_STRIDE, 7, ops.ROI_POOL_MAX2, strides=[16.0])
    # (the rule on sel against pool_mode comes before anything asks for a device)
    with pytest.raises(ValueError, match='sel'):
        ops.roi_pool_backward(dy, maps, rois, None, ops.ROI_NORM_STRIDE, 7, ops.ROI_POOL_MAX2, strides=[16.0])
    with pytest.raises(ValueError, match='sel'):
        ops.roi_pool_backward(dy, maps, rois, None, ops.ROI_NORM_STRIDE, 7, ops.ROI_POOL_NONE, strides=[16.0], sel=sel)
    with pytest.raises(ValueError, match='pool_size'):
        ops.roi_pool_trainable(maps, rois, None, ops.ROI_NORM_STRIDE, 17, ops.ROI_POOL_MAX2, strides=[16.0])
    with pytest.raises(Exception, match='GPU'):                          # (and no CPU path behind the checks)
        ops.roi_pool_argmax(maps, rois, None, ops.ROI_NORM_STRIDE, 7, strides=[16.0])


def test_layers_take_trainable_and_default_to_the_plain_path():
    import inspect
    from tf_eager_object_detection_amd.model import roi_pooling as rp
    for cls in (rp.RoiPoolingCropAndResize2, rp.RoiPoolingCropAndResize, rp.RoiPoolingRoiAlign):
        assert inspect.signature(cls.__init__).parameters['trainable'].default is False
    for fn in (rp.roi_pooling_fpn_levels, rp.crop_and_resize, rp.roi_align):
        assert inspect.signature(fn).parameters['trainable'].default is False
