"""Input front ends: decoded uint8 HWC images -> the preprocessed NHWC batch every entry point of this package takes
(preprocess_images, eval), and with their annotations -> what the fused training targets take (preprocess_training_batch).

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

The training stage (preprocess_training_batch, odet_preprocess_train) is image_argument_with_imgaug with the default
iaa.Fliplr(0.5) (tf_dataset_utils.py:10-52), preprocessing_training_func (:83-126) and the column swap of
scripts/train.py:84-96, in one launch; the flip comes BEFORE the resize, as in the reference.

scripts/eval_coco.py:110-111 passes ``config['image_max_size']`` as ``min_size`` and ``config['image_min_size']`` as
``max_size`` -- swapped -- so what that script actually runs is ``min_edge=1000, max_edge=600``.  Nothing here guesses:
both edges are explicit arguments.
"""
import collections
import ctypes as C

import numpy as np
import torch

from . import _lib as L

__all__ = ['resized_shape', 'group_by_resized_shape', 'preprocess_images', 'preprocess_training_batch', 'flip_decision',
           'PIPELINES', 'MAX_BATCH', 'MAX_BOXES']

PIPELINES = {'voc': 0, 'coco': 1}
_PREPROCESSING = {'caffe': 0, 'tf': 1}
MAX_BATCH = 64                       # ODET_PREP_MAX_BATCH
MAX_BOXES = 1024                     # ODET_PREP_MAX_BOXES
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


def flip_decision(seed, image_id):
    """odet_preprocess_train's flip rule for one image (include/odet.h): w0 >> 31 of philox((0, image_id, 5, 0), seed words).
    The library applies it itself to the consecutive ids first_image_id + b of one call; this host statement of it serves
    callers whose image ids are not consecutive (losses_from_raw_images groups by shape), who pass the flags as `flip`."""
    m = 0xFFFFFFFF
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = seed & m, seed >> 32
    c = [0, int(image_id) & m, 5, 0]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & m, (p0 >> 32) ^ c[3] ^ k1, p0 & m]
        k0, k1 = (k0 + 0x9E3779B9) & m, (k1 + 0xBB67AE85) & m
    return bool(c[0] >> 31)


def _host_array(a, i, what):
    if isinstance(a, torch.Tensor):
        if a.is_cuda:
            raise ValueError('%s %d must be a host array (numpy or CPU tensor): they go up in one copy' % (what, i))
        a = a.numpy()
    return np.asarray(a)


def preprocess_training_batch(images, boxes, labels, preprocessing_type='caffe', caffe_pixel_means=CAFFE_PIXEL_MEANS,
                              min_edge=600, max_edge=1000, augment=True, seed=0, first_image_id=0, flip=None,
                              dtype=torch.float32, device=None):
    """The reference's training input stage for a batch (one launch, odet_preprocess_train; semantics in include/odet.h).

    images: decoded uint8 RGB HWC images (numpy arrays, CPU or GPU tensors) that resize to one H x W under
    resized_shape(..., pipeline='coco').  boxes: per image a float32 [G, 4] host array of (ymin, xmin, ymax, xmax) in [0, 1]
    units of the raw image; labels: per image an integer [G] host array.  G = 0 is legal, G > 1024 is not.
    augment: image_argument_with_imgaug with iaa.Fliplr(0.5); image b flips by the Philox rule on (seed, first_image_id + b),
    or as flip[b] says when `flip` (B bools) is given.  augment=False: no flip, the boxes are not truncated.
    -> (batch [B, H, W, 3] float32 / float16, gt_boxes float32 [sum G, 4] (xmin, ymin, xmax, ymax) in pixels of the resized
    image, gt_labels int32 [sum G], gt_offsets int32 [B + 1], all on the GPU; flipped: list of B bools).
    The packed boxes and labels go up in ONE pinned, asynchronous copy."""
    if preprocessing_type not in _PREPROCESSING:
        raise ValueError("preprocessing_type must be 'caffe' or 'tf', got %r" % (preprocessing_type,))
    if dtype not in (torch.float32, torch.float16):
        raise ValueError('dtype must be torch.float32 or torch.float16, got %s' % (dtype,))
    images, boxes, labels = list(images), list(boxes), list(labels)
    B = len(images)
    if B == 0:
        raise ValueError('no images')
    if B > MAX_BATCH:
        raise ValueError('%d images exceed the batch limit %d' % (B, MAX_BATCH))
    if len(boxes) != B or len(labels) != B:
        raise ValueError('%d images, %d box arrays, %d label arrays: the lengths must match' % (B, len(boxes), len(labels)))
    augment = bool(augment)
    if flip is not None:
        if not augment:
            raise ValueError('flip flags given with augment=False (no flip without augmentation)')
        flip = [bool(f) for f in flip]
        if len(flip) != B:
            raise ValueError('%d images, %d flip flags: the lengths must match' % (B, len(flip)))
    raw = [_hw3(img, i) for i, img in enumerate(images)]
    offsets = [0]
    for i in range(B):
        bx, lb = _host_array(boxes[i], i, 'boxes'), _host_array(labels[i], i, 'labels')
        if bx.dtype != np.float32:
            raise ValueError('boxes %d must be float32, got %s' % (i, bx.dtype))
        if bx.ndim != 2 or bx.shape[1] != 4:
            raise ValueError('boxes %d must be [G, 4] (ymin, xmin, ymax, xmax), got shape %s' % (i, bx.shape))
        if not np.issubdtype(lb.dtype, np.integer):
            raise ValueError('labels %d must be integers, got %s' % (i, lb.dtype))
        if lb.ndim != 1 or lb.shape[0] != bx.shape[0]:
            raise ValueError('labels %d must be [G] with G = %d boxes, got shape %s' % (i, bx.shape[0], lb.shape))
        if bx.shape[0] > MAX_BOXES:
            raise ValueError('image %d has %d boxes, the limit is %d' % (i, bx.shape[0], MAX_BOXES))
        if not np.isfinite(bx).all():
            raise ValueError('boxes %d hold a value that is not finite' % i)
        boxes[i], labels[i] = bx, lb
        offsets.append(offsets[-1] + bx.shape[0])
    groups = group_by_resized_shape(raw, min_edge, max_edge, 'coco')
    if len(groups) != 1:
        raise ValueError('the images resize to %d different shapes, one batch takes one: %s (group them with '
                         'group_by_resized_shape)' % (len(groups), ', '.join('%dx%d: images %s' % (k[0], k[1], v)
                                                                              for k, v in groups.items())))
    (H, W), = groups.keys()
    if H <= 0 or W <= 0:
        raise ValueError('the images resize to an empty %d x %d' % (H, W))
    means = None
    if preprocessing_type == 'caffe':
        means = [float(m) for m in caffe_pixel_means]
        if len(means) != 3:
            raise ValueError('caffe_pixel_means must have 3 values (BGR)')
    if device is None:
        device = torch.device('cuda', torch.cuda.current_device())
    device = torch.device(device)
    dev, pitch = zip(*(_on_device(img, device) for img in images))
    n = offsets[-1]
    if n:                                # [4n float32 | n int32] in one pinned buffer, one copy
        pinned = torch.empty(5 * n, dtype=torch.int32, pin_memory=True)
        pinned[:4 * n].view(torch.float32).copy_(torch.from_numpy(np.concatenate(boxes, axis=0).reshape(-1)))
        pinned[4 * n:].copy_(torch.from_numpy(np.concatenate(labels, axis=0).astype(np.int32)))   # tf.to_int32 (train.py:96)
        up = pinned.to(device, non_blocking=True)
        boxes_in, gt_labels = up[:4 * n].view(torch.float32).view(n, 4), up[4 * n:]
    else:
        boxes_in = torch.empty((0, 4), dtype=torch.float32, device=device)
        gt_labels = torch.empty((0,), dtype=torch.int32, device=device)
    out = torch.empty((B, H, W, 3), dtype=dtype, device=device)
    gt_boxes = torch.empty((n, 4), dtype=torch.float32, device=device)
    gt_offsets = torch.empty((B + 1,), dtype=torch.int32, device=device)
    flipped = (C.c_int * B)()
    with torch.cuda.device(device):
        L.call('odet_preprocess_train', (C.c_void_p * B)(*[t.data_ptr() for t in dev]),
               (C.c_int * B)(*[h for h, _ in raw]), (C.c_int * B)(*[w for _, w in raw]), (C.c_longlong * B)(*pitch),
               B, H, W, _PREPROCESSING[preprocessing_type], None if means is None else (C.c_double * 3)(*means),
               L.dptr(boxes_in) if n else None, (C.c_int * (B + 1))(*offsets), int(augment),
               None if flip is None else (C.c_int * B)(*[int(f) for f in flip]), int(seed) & 0xFFFFFFFFFFFFFFFF,
               int(first_image_id) & 0xFFFFFFFF, L.dptr(out), int(dtype == torch.float16),
               L.dptr(gt_boxes) if n else None, L.dptr(gt_offsets), flipped, L.stream())
    return out, gt_boxes, gt_labels, gt_offsets, [bool(f) for f in flipped]
