"""RoI feature extraction -- counterpart of the reference's object_detection/model/roi_pooling.py.

All three reference layers map onto ONE fused HIP kernel (odet_roi_pool): TF crop_and_resize
sampling + the 2x2 max / avg pool, without materialising the [R,14,14,C] crops.

`trainable=True` (a constructor argument of the layers, a keyword of the functions; default False = the plain path): when the
feature map requires a gradient the call goes through ops.roi_pool_trainable -- the same forward bits, and a graph whose
backward is odet_roi_pool_backward into the map (float32 only; the RoIs get none, as the reference stops it: roi_pooling.py:78).

`roi_pooling_images` is the same for a batch of images in dense [B,...] tensors (ops.roi_pool_images and its trainable form): one
select and one backward launch for the whole batch.

Every entry states its modes and hands over to `_pool`, which alone decides between the trainable and the plain call."""
import torch

from .. import ops

__all__ = ['RoiPoolingCropAndResize', 'RoiPoolingRoiAlign', 'RoiPoolingCropAndResize2', 'crop_and_resize',
           'roi_align', 'roi_pooling_fpn_levels', 'roi_pooling_images']


def _spatial_order(feature_map, rois, stride):
    """processing order of a single-level layer's RoIs (odet_roi_order: sorted by y, x centre) -- consecutive workgroups, which
    share an XCD, then tap one neighbourhood of the map, so every XCD's L2 fetches its part of the map once instead of most of
    it (round 4: the tensorpack RoIAlign layer moved 1.84 x its distinct bytes without it).  Results are the same bits in any
    order.  None for launches too small to pay for the extra launch."""
    n = int(rois.shape[0])
    if n < 128 or n > 8192:
        return None
    h, w = int(feature_map.shape[1]), int(feature_map.shape[2])
    return ops.roi_order(rois, None, (max(1, int(round(h * float(stride)))), max(1, int(round(w * float(stride))))))


def _pool(trainable, maps, rois, roi_level, norm_mode, pool_size, pool_mode, order_stride=None, images=False, out=None, **kw):
    """The one place that decides between the trainable and the plain call, for the single-image entries and (`images`) the
    batch.  Trainable, when asked for and a map requires a gradient: no order and no `out`, and a graph is recorded whatever the
    caller's grad mode (the layers' forward is decorated no_grad).  Plain: `order_stride` = the map's stride where the entry
    sorts its RoIs (_spatial_order)."""
    maps = list(maps)
    if trainable and any(isinstance(m, torch.Tensor) and m.requires_grad for m in maps):
        if out is not None:
            raise ValueError('the trainable form of the RoI pooling allocates its output (out must be None)')
        with torch.enable_grad():
            return (ops.roi_pool_trainable_images if images else ops.roi_pool_trainable)(maps, rois, roi_level, norm_mode,
                                                                                         pool_size, pool_mode, **kw)
    if images:
        return ops.roi_pool_images(maps, rois, roi_level, norm_mode, pool_size, pool_mode, **kw)
    order = None if order_stride is None else _spatial_order(maps[0], rois, order_stride)
    return ops.roi_pool(maps, rois, roi_level, norm_mode, pool_size, pool_mode, out=out, order=order, **kw)


class RoiPoolingCropAndResize2(torch.nn.Module):
    """reference model/roi_pooling.py:8-42 (FPN variant: boxes normalised by the IMAGE size,
    always crop 2P + 2x2 max-pool)."""

    def __init__(self, pool_size, trainable=False):
        super().__init__()
        self._pool_size = pool_size
        self._trainable = bool(trainable)

    @torch.no_grad()
    def forward(self, inputs, training=None, mask=None):
        shared_layers, rois, image_shape = inputs
        return _pool(self._trainable, [shared_layers], rois, None, ops.ROI_NORM_IMAGE, self._pool_size, ops.ROI_POOL_MAX2,
                     image_shape=image_shape)

    call = forward


class RoiPoolingCropAndResize(torch.nn.Module):
    """reference model/roi_pooling.py:45-90 (boxes / stride / (dim-1); crop 2P + max-pool when
    ``max_pooling_flag`` else crop P)."""

    def __init__(self, pool_size, max_pooling_flag=True, trainable=False):
        super().__init__()
        self._pool_size = pool_size
        self._max_pooling_flag = max_pooling_flag
        self._trainable = bool(trainable)

    @torch.no_grad()
    def forward(self, inputs, training=None, mask=None):
        shared_layers, rois, extractor_stride = inputs
        mode = ops.ROI_POOL_MAX2 if self._max_pooling_flag else ops.ROI_POOL_NONE
        return _pool(self._trainable, [shared_layers], rois, None, ops.ROI_NORM_STRIDE, self._pool_size, mode,
                     order_stride=extractor_stride, strides=[float(extractor_stride)])

    call = forward


def crop_and_resize(image, boxes, box_ind, crop_size, pad_border=True, trainable=False):
    """reference model/roi_pooling.py:93-137 (tensorpack-style aligned crop).  ``boxes`` are in
    feature-map coordinates; ``box_ind`` must be all zeros (batch = 1, as everywhere in the
    reference: roi_pooling.py:28,66,152)."""
    assert isinstance(crop_size, int), crop_size
    return _pool(trainable, [image], boxes, None, ops.ROI_NORM_TP_ALIGN if pad_border else 3, crop_size, ops.ROI_POOL_NONE,
                 order_stride=1.0, strides=[1.0])


def roi_align(featuremap, boxes, resolution, trainable=False):
    """reference model/roi_pooling.py:140-155: 4 samples per bin (crop 2*resolution) + 2x2 avg."""
    return _pool(trainable, [featuremap], boxes, None, ops.ROI_NORM_TP_ALIGN, resolution, ops.ROI_POOL_AVG2, order_stride=1.0,
                 strides=[1.0])


class RoiPoolingRoiAlign(torch.nn.Module):
    """reference model/roi_pooling.py:158-177."""

    def __init__(self, pool_size, trainable=False):
        super().__init__()
        self._pool_size = pool_size
        self._trainable = bool(trainable)

    @torch.no_grad()
    def forward(self, inputs, training=None, mask=None):
        shared_layers, rois, extractor_stride = inputs
        return _pool(self._trainable, [shared_layers], rois, None, ops.ROI_NORM_TP_ALIGN, self._pool_size, ops.ROI_POOL_AVG2,
                     order_stride=extractor_stride, strides=[float(extractor_stride)])

    call = forward


def roi_pooling_fpn_levels(p_list, rois_sorted, roi_level, image_shape, pool_size, count_dev=None, out=None, trainable=False):
    """Native addition: what reference model/fpn/base_fpn_model.py:152-161 (_get_roi_features)
    does with one RoiPoolingCropAndResize2 call per non-empty level + concat, as ONE launch over
    the level-sorted RoIs (``roi_level`` = 0-based level of each row)."""
    return _pool(trainable, p_list, rois_sorted, roi_level, ops.ROI_NORM_IMAGE, pool_size, ops.ROI_POOL_MAX2,
                 image_shape=image_shape, count_dev=count_dev, out=out)


def roi_pooling_images(maps, rois, roi_level, norm_mode, pool_size, pool_mode, strides=None, image_shape=None, count_dev=None,
                       trainable=False):
    """Native addition: the pooling of B images at once.  maps = one float32 [B,H,W,C] tensor per level, rois [B,n,4], roi_level
    int32 [B,n] (None with one level), count_dev int32 [B] (None: n RoIs in every image) -> [B,n,P,P,C]; image b is what the
    single-image layers give on image b, bit for bit.  With norm_mode=ROI_NORM_IMAGE, pool_mode=ROI_POOL_MAX2 and per-image
    level-sorted RoIs this is roi_pooling_fpn_levels for a batch.  ``trainable`` as everywhere in this module."""
    return _pool(trainable, maps, rois, roi_level, norm_mode, pool_size, pool_mode, images=True, strides=strides,
                 image_shape=image_shape, count_dev=count_dev)
