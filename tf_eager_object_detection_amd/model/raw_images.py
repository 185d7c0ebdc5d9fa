"""Training losses from decoded images: the reference's train_one_epoch step (scripts/train.py:84-100) starting from the decoded
uint8 image and its annotations instead of the dataset's output -- the training twin of evaluation/raw_images.py.

preprocess_training_batch (image_argument_with_imgaug + preprocessing_training_func + the column swap, one HIP launch per
group of images that share a resized shape) -> model((image, gt_bboxes, gt_labels), True) per image -> the four losses.
"""
from .. import preprocess as P
from .base_faster_rcnn_model import BaseFasterRcnn
from .base_fpn_model import BaseFPN

__all__ = ['losses_from_raw_images']


def losses_from_raw_images(model, images, boxes, labels, preprocessing_type='caffe', caffe_pixel_means=P.CAFFE_PIXEL_MEANS,
                           min_edge=600, max_edge=1000, augment=True, seed=0, first_image_id=0, flip=None):
    """images: decoded uint8 RGB HWC images; boxes / labels: per image float32 [G, 4] (ymin, xmin, ymax, xmax) in [0, 1] and
    integer [G] host arrays (preprocess.preprocess_training_batch's arguments).  model: a caller object (ResnetV1Fpn,
    ResNetFasterRcnn, Vgg16FasterRcnn) with either training_targets setting; any image size, one float32 image per call.
    -> ([(rpn_cls_loss, rpn_reg_loss, roi_cls_loss, roi_reg_loss) per image, in input order], [flipped per image]).

    The image id of images[i] is first_image_id + i: its flip is a function of (seed, id) alone, whatever group it lands
    in; flip (one bool per image) overrides the rule.  The model calls run in input order, so the target layers' own
    image ids advance as in a loop over single images."""
    if not isinstance(model, (BaseFPN, BaseFasterRcnn)):
        raise TypeError('losses_from_raw_images: %s is not a caller object (BaseFPN / BaseFasterRcnn)'
                        % type(model).__name__)
    images, boxes, labels = list(images), list(boxes), list(labels)
    n = len(images)
    if len(boxes) != n or len(labels) != n:
        raise ValueError('%d images, %d box arrays, %d label arrays: the lengths must match' % (n, len(boxes), len(labels)))
    augment = bool(augment)
    if flip is not None:
        if not augment:
            raise ValueError('flip flags given with augment=False (no flip without augmentation)')
        flip = [bool(f) for f in flip]
        if len(flip) != n:
            raise ValueError('%d images, %d flip flags: the lengths must match' % (n, len(flip)))
    elif augment:                         # a group's ids are not consecutive: the flags travel explicitly
        flip = [P.flip_decision(seed, first_image_id + i) for i in range(n)]
    per_image = [None] * n
    for idx in P.group_by_resized_shape(images, min_edge, max_edge, 'coco').values():
        for k in range(0, len(idx), P.MAX_BATCH):
            part = idx[k:k + P.MAX_BATCH]
            batch, gt_boxes, gt_labels, _, flipped = P.preprocess_training_batch(
                [images[i] for i in part], [boxes[i] for i in part], [labels[i] for i in part], preprocessing_type,
                caffe_pixel_means, min_edge, max_edge, augment=augment, flip=[flip[i] for i in part] if augment else None)
            lo = 0
            for b, i in enumerate(part):
                hi = lo + len(boxes[i])
                per_image[i] = (batch[b:b + 1], gt_boxes[lo:hi], gt_labels[lo:hi], flipped[b])
                lo = hi
    losses = [tuple(model((img, gt, gl), True)) for img, gt, gl, _ in per_image]
    return losses, [f for _, _, _, f in per_image]
