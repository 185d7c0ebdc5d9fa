"""numpy restatement of the training input stage (include/odet.h "training input front end", odet_preprocess_train): the
reference's image_argument_with_imgaug with iaa.Fliplr(0.5) (dataset/utils/tf_dataset_utils.py:10-52),
preprocessing_training_func (:55-80, 83-126) and the column swap of scripts/train.py:84-96, with the flip decided by
stream 5 of the Philox rule.  Every cast is explicit (np.float64 / np.float32), so nothing depends on the installed numpy's
promotion rules.  The checker of tests/test_train_input_host.py and tests/test_train_input_gpu.py; the product never
imports it."""
import numpy as np

from oracle import oracle_np as on
from tf_eager_object_detection_amd import preprocess as P

import targets_np as tn

MEANS = (103.939, 116.779, 123.68)
STREAM_IMAGE_FLIP = 5
F32, F64 = np.float32, np.float64


def flip_flag(seed, image_id):
    """w0 >> 31 of philox((0, image_id, 5, 0), (seed low word, seed high word))"""
    w0 = tn.philox((0, int(image_id) & tn.MASK, STREAM_IMAGE_FLIP, 0), tn._seed_words(seed))[0]
    return bool(int(w0) >> 31)


def flip_flags(seed, first_image_id, count):
    return [flip_flag(seed, first_image_id + b) for b in range(count)]


def _unit(i, size):
    """iaa_bbox.y1 / height in float64, clipped to [0, 1], .astype(np.float32) (:48-52)"""
    q = F64(i) / F64(size)
    q = F64(0) if q < 0 else q
    q = F64(1) if q > 1 else q
    return F32(q)


def boxes(boxes_yxyx, h, w, H, W, augment=True, flip=False):
    """float32 [G, 4] (ymin, xmin, ymax, xmax) in [0, 1] of the raw h x w image -> float32 [G, 4] (xmin, ymin, xmax, ymax) in
    pixels of the resized H x W image"""
    src = np.asarray(boxes_yxyx, F32).reshape(-1, 4)
    out = np.zeros((len(src), 4), F32)
    sy, sx = F32(H - 1), F32(W - 1)                                   # tf.to_float(n_height - 1), (n_width - 1) (:120-123)
    for g, (y1, x1, y2, x2) in enumerate(src):
        if augment:
            # int(bbox[k] * size) (:31-32): the reference's numpy makes float32 scalar * int a float64 product
            iy1, ix1 = int(F64(y1) * F64(h)), int(F64(x1) * F64(w))
            iy2, ix2 = int(F64(y2) * F64(h)), int(F64(x2) * F64(w))
            if ix1 > ix2:                                             # ia.BoundingBox.__init__
                ix1, ix2 = ix2, ix1
            if iy1 > iy2:
                iy1, iy2 = iy2, iy1
            if flip:                                                  # Fliplr on the corners: x' = width - x, min / max re-taken
                ix1, ix2 = w - ix2, w - ix1
            y1, x1, y2, x2 = _unit(iy1, h), _unit(ix1, w), _unit(iy2, h), _unit(ix2, w)
        out[g] = (F32(x1) * sx, F32(y1) * sy, F32(x2) * sx, F32(y2) * sy)     # x first: train.py:89-93
    return out


def normalise(raw, norm):
    """_caffe_preprocessing / _tf_preprocessing (:55-80) of a uint8 RGB image"""
    img = raw.astype(F32)
    if norm == 'caffe':                                 # reverse to BGR, subtract float32 means
        img = img[..., ::-1]
        return np.stack([img[..., c] - F32(MEANS[c]) for c in range(3)], axis=-1)
    return (img * F32(1.0 / 255)) * F32(2.0) - F32(1.0)  # convert_image_dtype multiplies by float32(1/255)


def image(raw, norm, flip=False, min_edge=600, max_edge=1000):
    """uint8 RGB [h, w, 3] -> float32 [H, W, 3]: flip (image[:, ::-1]) BEFORE normalisation and the TF 1.x resize"""
    if flip:
        raw = raw[:, ::-1]
    H, W, _ = P.resized_shape(raw.shape[0], raw.shape[1], min_edge, max_edge, 'coco')
    return on.tf_resize_bilinear_legacy(normalise(np.ascontiguousarray(raw), norm)[None], (H, W))[0]


def batch(raws, boxes_list, norm, flips, augment=True, min_edge=600, max_edge=1000):
    """-> (images float32 [B, H, W, 3], gt_boxes float32 [sum G, 4], gt_offsets int32 [B + 1])"""
    ims, bxs, off = [], [], [0]
    for raw, bx, f in zip(raws, boxes_list, flips):
        h, w = raw.shape[:2]
        H, W, _ = P.resized_shape(h, w, min_edge, max_edge, 'coco')
        ims.append(image(raw, norm, bool(f) and augment, min_edge, max_edge))
        bxs.append(boxes(bx, h, w, H, W, augment, bool(f)))
        off.append(off[-1] + len(bxs[-1]))
    return np.stack(ims), np.concatenate(bxs).reshape(-1, 4).astype(F32), np.asarray(off, np.int32)
