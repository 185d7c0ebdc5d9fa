"""Detection from decoded images: the reference's per-image eval loop (evaluation/pascal_eval_files_utils.py:76-106)
starting from the decoded uint8 image instead of the loader's output.

preprocess_images (the loader's normalisation + resize, one HIP launch) -> model.im_detect(image, img_scale) ->
pascal_eval.detect_image(..., raw_h, raw_w) -> per image, per class, the [n, 5] float32 arrays (x1, y1, x2, y2, score)
in raw-image pixels: the reference's all_boxes[j][i].
"""
from .. import preprocess as P
from ..model.base_faster_rcnn_model import BaseFasterRcnn
from ..model.base_fpn_model import BaseFPN
from ..model.detector_base import Detector
from .pascal_eval import detect_image

__all__ = ['detect_raw_images']


def detect_raw_images(model, images, pipeline, preprocessing_type='caffe', caffe_pixel_means=P.CAFFE_PIXEL_MEANS,
                      image_format='bgr', min_edge=600, max_edge=1000, score_threshold=0.0, iou_threshold=0.5,
                      max_objects_per_class=50, max_objects_per_image=50, target_means=None, target_stds=None,
                      min_size=10, detect=detect_image):
    """images: decoded uint8 HWC images (numpy arrays or tensors; BGR for pipeline 'voc', RGB for 'coco').
    -> one list per image, indexed by class id (entry 0 unused), of float32 [n, 5] arrays in raw-image pixels.

    model is either
    * a caller object (ResnetV1Fpn, ResNetFasterRcnn, Vgg16FasterRcnn): any image size, one float32 image per call; or
    * a fast detector (ResNetFpnDetector, ResNetC4Detector, Vgg16Detector): up to max_batch images go through one
      preprocessing launch and one im_detect, in the detector's dtype (float16 models get the float16 batch).  Every
      image must resize to model.image_shape (ValueError otherwise, before any work is queued).
    The preprocessing arguments are those of preprocess.preprocess_images; the rest those of pascal_eval.detect_image
    (pascal_eval_files_utils.py:19-29 defaults).  detect: the per-image loop, called with detect_image's arguments;
    coco_eval.detect_image_coco gives the COCO script's cap (each list entry is then its (boxes, labels, scores))."""
    images = list(images)
    prep = dict(pipeline=pipeline, preprocessing_type=preprocessing_type, caffe_pixel_means=caffe_pixel_means,
                image_format=image_format, min_edge=min_edge, max_edge=max_edge)
    det = dict(num_classes=model.num_classes, score_threshold=score_threshold, iou_threshold=iou_threshold,
               max_objects_per_class=max_objects_per_class, max_objects_per_image=max_objects_per_image,
               target_means=target_means, target_stds=target_stds, min_size=min_size)
    out = []
    if isinstance(model, (BaseFPN, BaseFasterRcnn)):
        for img in images:
            batch, scales, raw = P.preprocess_images([img], **prep)
            scores, deltas, rois = model.im_detect(batch, scales[0])
            out.append(detect(scores, deltas, rois, 1.0, raw[0][0], raw[0][1], **det))   # (rois already / img_scale)
        return out
    if isinstance(model, Detector):
        want = tuple(model.image_shape)
        for shape, idx in P.group_by_resized_shape(images, min_edge, max_edge, pipeline).items():
            if shape != want:
                raise ValueError('images %s resize to %dx%d, the detector runs %dx%d (image_shape); build a detector for '
                                 'that shape or group the images' % (idx, shape[0], shape[1], want[0], want[1]))
        step = len(model._hot)                                         # max_batch
        for i in range(0, len(images), step):
            batch, scales, raw = P.preprocess_images(images[i:i + step], dtype=model.dtype, **prep)
            for (scores, deltas, rois), (h, w) in zip(model.im_detect(batch, scales), raw):
                out.append(detect(scores, deltas, rois, 1.0, h, w, **det))
        return out
    raise TypeError('detect_raw_images: %s is neither a caller object (BaseFPN / BaseFasterRcnn) nor a fast detector '
                    '(ResNetFpnDetector / ResNetC4Detector / Vgg16Detector)' % type(model).__name__)
