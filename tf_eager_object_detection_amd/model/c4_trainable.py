"""The float32 ResNet-C4 detector of model/frcnn_detector.py with a backward pass: ResNetC4Detector.extractor_trainable and
roi_head_trainable (reference resnet_faster_rcnn.py:102-158 get_resnet_v1_extractor with conv1 and the conv2 stack built
trainable=False, :109, :139-141; :161-185 get_resnet_v1_roi_head: the conv5 stack on the crops, GlobalAveragePooling2D, score /
boxes).  The bottlenecks are extractor_trainable.py's block_trainable -- forward bit-equal to the blocks' own launches, backward on
this package's kernels --, the pooling is ops.global_avg_pool_trainable (csrc/c4_grad.hip), the final pair the detectors' shared
_final_outputs_trainable.  The RpnHead's is model/rpn_trainable.py on the one level (SingleLevelDetector.rpn_trainable)."""
import torch

from .. import ops
from .extractor_trainable import block_trainable
from .layers import _nhwc, _stem
from .trainable_common import require_exact_f32

FROZEN_STAGES = ('conv1', 'conv2')                        # trainable=False in the reference
EXTRACTOR_STAGES = ('conv3', 'conv4')
HEAD_STAGE = 'conv5'


def trained_names(det, roi_head=True, rpn_head=True, extractor=True):
    """the parameters (names in det.named_parameters()) that a backward pass through the named trainable parts fills, read off the
    module tree: conv3 + conv4 / the RpnHead's three layers / conv5 + score + bbox"""
    tops = (EXTRACTOR_STAGES if extractor else ()) + (('rpn_conv', 'rpn_score', 'rpn_bbox') if rpn_head else ()) \
        + ((HEAD_STAGE, 'score', 'bbox') if roi_head else ())
    return [n for n, _ in det.named_parameters() if n.split('.')[0] in tops]


def frozen_names(det):
    """the parameters no backward pass reaches: conv1 and the conv2 stack"""
    return [n for n, _ in det.named_parameters() if n.split('.')[0] in FROZEN_STAGES]


def extractor_trainable(det, images_nhwc):
    """det.features(images_nhwc) with a backward pass into conv3 and conv4, bit-equal to it.  The stem and the conv2 stack run
    under no_grad on features()' launches: the backward stops at conv3's first block, whose input requires no gradient (its
    parameters' gradients are computed, no input gradient)."""
    require_exact_f32(det, 'extractor_trainable')
    with torch.no_grad():
        x = det.conv2(_stem(det.conv1, images_nhwc, det.dtype))
    for name in EXTRACTOR_STAGES:
        for blk in getattr(det, name):
            x = block_trainable(blk, x)
    return x


def head_map_trainable(det, roi_features):
    """det.conv5 on the NHWC crops [R,7,7,1024] with a backward pass, the whole batch of crops in one pass: the channels_last
    [R,2048,7,7] map, bit-equal to det.conv5's.  Crops that require a gradient (ops.roi_pool_trainable's) get one: the first
    block's block_input_grad."""
    require_exact_f32(det, 'roi_head_trainable')
    x = roi_features.permute(0, 3, 1, 2).to(det.dtype)                          # NCHW view of NHWC memory
    for blk in getattr(det, HEAD_STAGE):
        x = block_trainable(blk, x)
    return x


def head_activation_trainable(det, roi_features):
    """conv5 -> global average pooling [R,2048], the input of the score / bbox layers: ops.global_avg_pool's stated order, not
    head_activation's Tensor.mean (the two agree to the pooling's rounding)"""
    return ops.global_avg_pool_trainable(_nhwc(head_map_trainable(det, roi_features)))


def roi_head_trainable(det, roi_features):
    """det.roi_head(roi_features) with a backward pass into the conv5 stack, score and bbox, and into the crops when they require
    a gradient: (score logits [R,C], box deltas [R,4C])"""
    return det._final_outputs_trainable(head_activation_trainable(det, roi_features))
