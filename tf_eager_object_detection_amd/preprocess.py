"""Eval input front end: decoded uint8 HWC images -> the preprocessed NHWC batch every entry point of this package takes.

Counterpart of the reference's eval loaders (the step its eval scripts start from):

* ``pipeline='voc'``: dataset/eval_pascal_tf_dataset.py:32-52 (``_map_from_cv2``, the default ``--dataset_type cv2`` of
  scripts/eval_pascal.py).  Input BGR (cv2.imread).  numpy normalisation, then ``cv2.resize`` (INTER_LINEAR), then an
  optional flip to RGB (``image_format='rgb'``, :50-51).
* ``pipeline='coco'``: dataset/utils/tf_dataset_utils.py:128-155 (``preprocessing_eval_func``, reached from
  scripts/eval_coco.py through dataset/coco_tf_dataset_generator.py:213-220).  Input RGB (decode_jpeg).
  ``_caffe_preprocessing`` (reversed to BGR, means subtracted) or ``_tf_preprocessing`` (RGB in [-1, 1]), then
  ``tf.image.resize_bilinear`` of TF 1.x.

The pixel work is one HIP launch for the whole batch (odet_preprocess_images); the exact per-pipeline arithmetic is in
include/odet.h.  The OpenCV resize is a restatement of resize.cpp (scalar paths); OpenCV builds whose SIMD vertical pass
fuses the multiply-add can differ from it by an ulp.

scripts/eval_coco.py:110-111 passes ``config['image_max_size']`` as ``min_size`` and ``config['image_min_size']`` as
``max_size`` -- swapped -- so what that script actually runs is ``min_edge=1000, max_edge=600``.  Nothing here guesses:
both edges are explicit arguments.
"""
import collections
import ctypes as C

import numpy as np
import torch

from . import _lib as L

__all__ = ['resized_shape', 'group_by_resized_shape', 'preprocess_images', 'PIPELINES', 'MAX_BATCH']

PIPELINES = {'voc': 0, 'coco': 1}
_PREPROCESSING = {'caffe': 0, 'tf': 1}
MAX_BATCH = 64                       # ODET_PREP_MAX_BATCH
CAFFE_PIXEL_MEANS = (103.939, 116.779, 123.68)


def _pipeline(pipeline):
    if pipeline not in PIPELINES:
        raise ValueError("pipeline must be 'voc' or 'coco', got %r" % (pipeline,))
    return PIPELINES[pipeline]


def resized_shape(h, w, min_edge=600, max_edge=1000, pipeline='voc'):
    """(new_h, new_w, img_scale) of a raw h x w image, each loader's rule taken literally.

    voc (eval_pascal_tf_dataset.py:41-46): Python floats (float64) -- scale = min(min_edge / min(h, w),
    max_edge / max(h, w)); new = int(scale * size); img_scale = float(scale) (float64).
    coco (tf_dataset_utils.py:144-150): tf.to_float(height / width), the edges as float32 constants, every operation in
    float32; new = tf.to_int32(scale * size) (truncation); img_scale is that float32 scale.

    The two differ: 1080 x 1920 -> 562 x 1000 (voc) vs 562 x 999 (coco)."""
    _pipeline(pipeline)
    h, w = int(h), int(w)
    if h <= 0 or w <= 0:
        raise ValueError('image size must be positive, got %d x %d' % (h, w))
    if pipeline == 'voc':
        scale = min(min_edge / min(h, w), max_edge / max(h, w))
        return int(scale * h), int(scale * w), float(scale)
    f = np.float32
    hf, wf = f(h), f(w)
    scale = min(f(f(min_edge) / min(hf, wf)), f(f(max_edge) / max(hf, wf)))
    return int(f(scale * hf)), int(f(scale * wf)), f(scale)


def _hw3(img, i):
    """(h, w) of one uint8 HWC image, or ValueError"""
    if isinstance(img, np.ndarray):
        dtype_ok, shape = img.dtype == np.uint8, img.shape
    elif isinstance(img, torch.Tensor):
        dtype_ok, shape = img.dtype == torch.uint8, tuple(img.shape)
    else:
        raise TypeError('image %d must be a numpy array or a torch tensor, got %s' % (i, type(img).__name__))
    if not dtype_ok:
        raise ValueError('image %d must be uint8 (a decoded image), got %s' % (i, img.dtype))
    if len(shape) != 3 or shape[2] != 3:
        raise ValueError('image %d must be [H, W, 3] (HWC, 3 channels), got shape %s' % (i, tuple(shape)))
    return int(shape[0]), int(shape[1])


def group_by_resized_shape(images, min_edge=600, max_edge=1000, pipeline='voc'):
    """{(new_h, new_w): [indices into images]} in first-seen order -- the batches preprocess_images accepts.
    images: uint8 HWC arrays / tensors, or (h, w) pairs."""
    groups = collections.OrderedDict()
    for i, img in enumerate(images):
        h, w = (int(img[0]), int(img[1])) if isinstance(img, tuple) else _hw3(img, i)
        nh, nw, _ = resized_shape(h, w, min_edge, max_edge, pipeline)
        groups.setdefault((nh, nw), []).append(i)
    return groups


def _on_device(img, device):
    """-> (uint8 GPU tensor whose rows are 3 * w contiguous bytes, row pitch in bytes).  CPU images go up in one pinned,
    asynchronous copy each; a GPU view with a row stride of its own keeps it (no copy)."""
    if isinstance(img, np.ndarray):
        img = torch.from_numpy(np.ascontiguousarray(img))
    if img.is_cuda:
        if img.device != device:
            raise ValueError('image on %s, expected %s' % (img.device, device))
        s = img.stride()
        if s[2] != 1 or s[1] != 3 or s[0] < 3 * img.shape[1]:
            img = img.contiguous()
            s = img.stride()
        return img, int(s[0])
    pinned = torch.empty(tuple(img.shape), dtype=torch.uint8, pin_memory=True)
    pinned.copy_(img)
    dev = pinned.to(device, non_blocking=True)
    return dev, 3 * int(img.shape[1])


def preprocess_images(images, pipeline, preprocessing_type='caffe', caffe_pixel_means=CAFFE_PIXEL_MEANS,
                      image_format='bgr', min_edge=600, max_edge=1000, dtype=torch.float32, device=None):
    """Decoded uint8 HWC images (numpy arrays, CPU or GPU tensors; channel order as the loader decodes: BGR for voc, RGB
    for coco) -> (batch [B, H, W, 3] float32 / float16 on the GPU, img_scale per image, (raw_h, raw_w) per image).

    Every image must resize to the same H x W (group_by_resized_shape splits a list); otherwise ValueError.
    image_format: 'bgr' or 'rgb' (voc only, :50-51); the coco loader's channel order follows preprocessing_type (BGR for
    caffe, RGB for tf), so it takes the default only.  img_scale: float64 for voc, float32 for coco (the loader's
    values).  dtype float16: the float32 result rounded once (to nearest even)."""
    p = _pipeline(pipeline)
    if preprocessing_type not in _PREPROCESSING:
        raise ValueError("preprocessing_type must be 'caffe' or 'tf', got %r" % (preprocessing_type,))
    if image_format not in ('bgr', 'rgb'):
        raise ValueError("image_format must be 'bgr' or 'rgb', got %r" % (image_format,))
    if pipeline == 'coco' and image_format != 'bgr':
        raise ValueError("image_format applies to the voc pipeline only (coco's order follows preprocessing_type)")
    if dtype not in (torch.float32, torch.float16):
        raise ValueError('dtype must be torch.float32 or torch.float16, got %s' % (dtype,))
    images = list(images)
    B = len(images)
    if B == 0:
        raise ValueError('no images')
    if B > MAX_BATCH:
        raise ValueError('%d images exceed the batch limit %d' % (B, MAX_BATCH))
    raw = [_hw3(img, i) for i, img in enumerate(images)]
    groups = group_by_resized_shape(raw, min_edge, max_edge, pipeline)
    if len(groups) != 1:
        raise ValueError('the images resize to %d different shapes, one batch takes one: %s (group them with '
                         'group_by_resized_shape)' % (len(groups), ', '.join('%dx%d: images %s' % (k[0], k[1], v)
                                                                              for k, v in groups.items())))
    (H, W), = groups.keys()
    scales = [resized_shape(h, w, min_edge, max_edge, pipeline)[2] for h, w in raw]
    means = None
    if preprocessing_type == 'caffe':
        means = [float(m) for m in caffe_pixel_means]
        if len(means) != 3:
            raise ValueError('caffe_pixel_means must have 3 values (BGR)')
    if H <= 0 or W <= 0:
        raise ValueError('the images resize to an empty %d x %d' % (H, W))
    if device is None:
        device = torch.device('cuda', torch.cuda.current_device())
    device = torch.device(device)
    dev, pitch = zip(*(_on_device(img, device) for img in images))
    out = torch.empty((B, H, W, 3), dtype=dtype, device=device)
    with torch.cuda.device(device):
        L.call('odet_preprocess_images', (C.c_void_p * B)(*[t.data_ptr() for t in dev]),
               (C.c_int * B)(*[h for h, _ in raw]), (C.c_int * B)(*[w for _, w in raw]),
               (C.c_longlong * B)(*pitch), B, H, W, p, _PREPROCESSING[preprocessing_type],
               int(image_format == 'rgb'), None if means is None else (C.c_double * 3)(*means), L.dptr(out),
               int(dtype == torch.float16), L.stream())
    return out, scales, raw
