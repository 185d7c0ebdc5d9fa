"""The Python fronts of the RoI pooling (ops.roi_pool* and model/roi_pooling.py) without a GPU: the public signatures as they were
before the single-image and the batched fronts were joined, that ops.py holds each rule once, and every refusal of the fronts
through the single-image and through the batched function, on CPU tensors."""
import inspect
import re

import pytest
import torch

from tf_eager_object_detection_amd import _lib, ops
from tf_eager_object_detection_amd.model import roi_pooling

_POOL = ('(feature_maps, rois, roi_level, norm_mode, pool_size, pool_mode, strides=None, image_shape=None, count_dev=None%s)')
_ARGMAX = '(feature_maps, rois, roi_level, norm_mode, pool_size, strides=None, image_shape=None, count_dev=None, out=None)'
_BACKWARD = ('(dy, feature_shapes_or_maps, rois, roi_level, norm_mode, pool_size, pool_mode, strides=None, image_shape=None, '
             'count_dev=None, outs=None, sel=None)')
OPS_SIGNATURES = {
    'roi_order': '(rois, roi_level, image_shape, count_dev=None, out=None)',
    'roi_pool': _POOL % ', out=None, events=None, order=None',
    'roi_pool_argmax': _ARGMAX,
    'roi_pool_backward': _BACKWARD,
    'roi_pool_trainable': _POOL % '',
    'roi_pool_images': _POOL % ', out=None',
    'roi_pool_argmax_images': _ARGMAX,
    'roi_pool_backward_images': _BACKWARD,
    'roi_pool_trainable_images': _POOL % '',
}
_FORWARD = '(self, inputs, training=None, mask=None)'
LAYER_SIGNATURES = {
    'RoiPoolingCropAndResize': ('(self, pool_size, max_pooling_flag=True, trainable=False)', _FORWARD),
    'RoiPoolingRoiAlign': ('(self, pool_size, trainable=False)', _FORWARD),
    'RoiPoolingCropAndResize2': ('(self, pool_size, trainable=False)', _FORWARD),
    'crop_and_resize': '(image, boxes, box_ind, crop_size, pad_border=True, trainable=False)',
    'roi_align': '(featuremap, boxes, resolution, trainable=False)',
    'roi_pooling_fpn_levels': '(p_list, rois_sorted, roi_level, image_shape, pool_size, count_dev=None, out=None, trainable=False)',
    'roi_pooling_images': '(maps, rois, roi_level, norm_mode, pool_size, pool_mode, strides=None, image_shape=None, count_dev=None, '
                          'trainable=False)',
}


def test_the_public_signatures_are_the_ones_of_before():
    for name, want in OPS_SIGNATURES.items():
        assert str(inspect.signature(getattr(ops, name))) == want, name
    assert (ops.ROI_GRAD_MAX_ROIS, ops.ROI_GRAD_MAX_POOL, ops.ROI_IMAGES_MAX_BATCH) == (8192, 16, 64)
    assert inspect.isclass(ops.ProfEvent)
    assert sorted(roi_pooling.__all__) == sorted(LAYER_SIGNATURES)
    for name, want in LAYER_SIGNATURES.items():
        obj = getattr(roi_pooling, name)
        if inspect.isclass(obj):
            assert (str(inspect.signature(obj.__init__)), str(inspect.signature(obj.forward))) == want, name
            assert obj.call is obj.forward
        else:
            assert str(inspect.signature(obj)) == want, name


def test_ops_holds_each_rule_once():
    src = inspect.getsource(ops)
    classes = re.findall(r'^class (\w*RoiPool\w*)\(torch\.autograd\.Function\)', src, re.M)
    assert len(classes) == 1, classes
    functions = [n for n, v in vars(ops).items() if inspect.isclass(v) and issubclass(v, torch.autograd.Function) and 'RoiPool' in n]
    assert functions == classes
    for text in ('the RoI backward has no float16 form', 'all levels must share the channel count', 'is required for ROI_POOL_MAX2'):
        assert src.count(text) == 1, text


# ---- every refusal, through the single-image (form '') and the batched (form '_images') function ------------------------------------

def _operands(form):
    lead = (2,) if form else ()
    maps = [torch.zeros(2 if form else 1, 17, 17, 8)]
    rois = torch.zeros(lead + (5, 4))
    dy = torch.zeros(lead + (5, 7, 7, 8))
    return maps, rois, dy, torch.zeros(dy.shape, dtype=torch.uint8)


@pytest.mark.parametrize('form', ['', '_images'])
def test_the_fronts_refuse_on_cpu_tensors(form):
    """dy's dtype, the maps' dtype and the sel / pool_mode rule come before anything asks for a device, the trainable fronts'
    limits too; behind them there is no CPU path"""
    argmax, backward, trainable = (getattr(ops, n + form) for n in ('roi_pool_argmax', 'roi_pool_backward', 'roi_pool_trainable'))
    maps, rois, dy, sel = _operands(form)
    half = [maps[0].half()]
    norm, kw = ops.ROI_NORM_STRIDE, dict(strides=[16.0])
    with pytest.raises(ValueError, match='float32'):
        argmax(half, rois, None, norm, 7, **kw)
    with pytest.raises(ValueError, match='float32'):
        backward(dy, half, rois, None, norm, 7, ops.ROI_POOL_AVG2, **kw)
    with pytest.raises(ValueError, match='float32'):
        backward(dy.half(), maps, rois, None, norm, 7, ops.ROI_POOL_AVG2, **kw)
    with pytest.raises(ValueError, match='float32'):                      # (dy's dtype is asked first: the maps are wrong as well)
        backward(dy.half(), half, rois, None, norm, 7, ops.ROI_POOL_MAX2, **kw)
    with pytest.raises(ValueError, match='float32'):
        backward(dy, None, rois, None, norm, 7, ops.ROI_POOL_AVG2, outs=half, **kw)
    with pytest.raises(ValueError, match='float32'):
        trainable(half, rois, None, norm, 7, ops.ROI_POOL_MAX2, **kw)
    with pytest.raises(ValueError, match='sel'):
        backward(dy, maps, rois, None, norm, 7, ops.ROI_POOL_MAX2, **kw)
    with pytest.raises(ValueError, match='sel'):
        backward(dy, maps, rois, None, norm, 7, ops.ROI_POOL_NONE, sel=sel, **kw)
    with pytest.raises(ValueError, match='pool_size'):
        trainable(maps, rois, None, norm, 17, ops.ROI_POOL_MAX2, **kw)
    with pytest.raises(ValueError, match='pool_size'):                    # (the limit on the RoIs of an image, in the same text)
        trainable(maps, torch.zeros(rois.shape[:-2] + (8193, 4)), None, norm, 7, ops.ROI_POOL_MAX2, **kw)
    for call in (lambda: argmax(maps, rois, None, norm, 7, **kw),
                 lambda: backward(dy, maps, rois, None, norm, 7, ops.ROI_POOL_MAX2, sel=sel, **kw),
                 lambda: trainable(maps, rois, None, norm, 7, ops.ROI_POOL_MAX2, **kw),
                 lambda: (ops.roi_pool_images if form else ops.roi_pool)(maps, rois, None, norm, 7, ops.ROI_POOL_MAX2, **kw)):
        with pytest.raises(_lib.OdetError, match='GPU'):
            call()


def test_the_batched_fronts_own_refusals_on_cpu_tensors():
    maps, rois, _, _ = _operands('_images')
    args = (None, ops.ROI_NORM_STRIDE, 7, ops.ROI_POOL_MAX2)
    with pytest.raises(ValueError, match='float32'):
        ops.roi_pool_images([maps[0].half()], rois, *args)
    with pytest.raises(ValueError, match='images'):
        ops.roi_pool_trainable_images([torch.zeros(65, 3, 3, 8)], torch.zeros(65, 5, 4), *args)
    with pytest.raises(ValueError, match=r'\[B,n,4\]'):
        ops.roi_pool_trainable_images(maps, rois[0], *args)


@pytest.fixture
def rois_pass_the_device_check(monkeypatch):
    """The level table's rules on the batch size are asked on the host, ahead of the table's own device check, but behind the RoI
    front, which refuses CPU RoIs.  Here the front's cast lets them pass, so that these rules are reached without a GPU
    (tests/test_roi_fronts_gpu.py reaches them with nothing replaced)."""
    monkeypatch.setattr(_lib, 'f32c', lambda t, name='tensor': t.float().contiguous())


def test_the_level_table_refuses_buffers_of_another_batch_size(rois_pass_the_device_check):
    norm, kw = ops.ROI_NORM_STRIDE, dict(strides=[16.0])
    maps, rois, dy, _ = _operands('')
    with pytest.raises(ValueError, match='NHWC with batch 1'):
        ops.roi_pool_backward(dy, None, rois, None, norm, 7, ops.ROI_POOL_AVG2, outs=[torch.zeros(2, 17, 17, 8)], **kw)
    with pytest.raises(ValueError, match='NHWC with batch 1'):
        ops.roi_pool_argmax([torch.zeros(2, 17, 17, 8)], rois, None, norm, 7, **kw)
    with pytest.raises(ValueError, match='NHWC with batch 1'):
        ops.roi_pool([torch.zeros(17, 17, 8)], rois, None, norm, 7, ops.ROI_POOL_AVG2, **kw)
    maps, rois, dy, _ = _operands('_images')
    with pytest.raises(_lib.OdetError, match='share the batch size'):
        ops.roi_pool_backward_images(dy, None, rois, None, norm, 7, ops.ROI_POOL_AVG2, outs=[torch.zeros(3, 17, 17, 8)], **kw)
    with pytest.raises(_lib.OdetError, match='share the batch size'):
        ops.roi_pool_argmax_images([torch.zeros(3, 17, 17, 8)], rois, None, norm, 7, **kw)
    with pytest.raises(ValueError, match='NHWC with batch 1'):              # B = 1 of the batched form keeps the single-image text
        ops.roi_pool_backward_images(dy[:1], None, rois[:1], None, norm, 7, ops.ROI_POOL_AVG2, outs=[torch.zeros(2, 17, 17, 8)], **kw)
    with pytest.raises(_lib.OdetError, match=r'\[B,n\]'):
        ops.roi_pool_argmax_images(maps, rois, torch.zeros(2, 4, dtype=torch.int32), norm, 7, **kw)
