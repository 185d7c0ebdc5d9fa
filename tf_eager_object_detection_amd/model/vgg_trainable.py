"""The float32 VGG16 detector of model/frcnn_detector.py with a backward pass: Vgg16Detector.extractor_trainable and
roi_head_trainable (reference vgg16_faster_rcnn.py:260-342 Vgg16Extractor with block1_* / block2_* built trainable=False, :178-257
Vgg16RoiHead with both dropouts active in training).  The forward passes are features()' and roi_head()'s own launches (outputs
bit-equal); the backward runs on this package's kernels -- the nine 3x3 convolutions of blocks 3-5 on ops.conv3x3_trainable_levels
(one level), the two that carry a pooling on ops.conv3x3_relu_pool_trainable (odet_relu_maxpool2_backward_f32 in front of the weight
gradient), the Dense layers with ops.dropout_trainable between them on trainable_common.fc_head_trainable (the FPN head's too; here
under the name roi_head_trainable).  The RpnHead's is model/rpn_trainable.py on the one level (SingleLevelDetector.rpn_trainable)."""
import torch

from .. import ops
from .layers import _nhwc, _no_kernel, _own_conv3x3
from .trainable_common import fc_head_trainable as roi_head_trainable, flipped_weight, require_exact_f32  # noqa: F401

FIRST_TRAINED = 4                        # convs[4] = block3_conv1: blocks 1-2 (convs[0..3]) are frozen, :265-288


def trained_convs(det):
    """the nine convolutions that train, block3_conv1 .. block5_conv3, in order"""
    return list(det.convs)[FIRST_TRAINED:]


def extractor_trainable(det, images_nhwc):
    """det.features(images_nhwc) with a backward pass into block3_conv1 .. block5_conv3, bit-equal to it.  Blocks 1-2 run under
    no_grad on features()' launches: the backward stops at block3_conv1's weight gradient (its input requires no gradient, so no
    input gradient is computed there and none through block1_pool / block2_pool)."""
    require_exact_f32(det, 'extractor_trainable')
    plan = det._layer_plan()
    with torch.no_grad():
        x = det._first_conv(images_nhwc)
        for i, pooled in plan:
            if i < FIRST_TRAINED:
                x = det._layer(i, pooled, x)
    x = _nhwc(x)
    for i, pooled in plan:
        if i < FIRST_TRAINED:
            continue
        conv = det.convs[i]
        if not _own_conv3x3(conv, x.permute(0, 3, 1, 2)) or conv.bias is None:
            raise _no_kernel('3x3 convolution', conv, x)
        # (the flipped weight only where the backward pass will compute an input gradient)
        wf = flipped_weight(conv) if torch.is_grad_enabled() and x.requires_grad else None
        if pooled:
            x = ops.conv3x3_relu_pool_trainable(x, conv.weight, conv.bias, flipped=wf)
        else:
            x = ops.conv3x3_trainable_levels([x], conv.weight, conv.bias, relu=True, flipped=wf)[0]
    return x.permute(0, 3, 1, 2)
