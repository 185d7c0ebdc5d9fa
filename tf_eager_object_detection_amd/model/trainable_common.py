"""What the trainable parts (neck_trainable.py, extractor_trainable.py, rpn_trainable.py, vgg_trainable.py, c4_trainable.py) and the
caller models' train_* keywords share, and the one trainable FC head of the FPN and VGG16 detectors (fc_head_trainable).  Imports
ops and derived only: every model file may import it."""
import torch

from .. import ops
from ..derived import derived


def check_train_flags(model, dtype, f32_form, *flags):
    """the caller models' train_* keywords, each (value, name, what has no other form): the first one set without float32 and
    f32_form 'exact' is the error"""
    for on, name, what in flags:
        if on and (dtype != torch.float32 or f32_form != 'exact'):
            raise ValueError("%s: %s=True needs dtype=torch.float32 and f32_form='exact' (%s no float16 or split-precision form), "
                             "got %s, %r" % (model, name, what, dtype, f32_form))


def require_exact_f32(det, who):
    """a detector's trainable part `who` runs only in float32 and f32_form 'exact': the backward kernels have no other form"""
    if det.dtype != torch.float32 or det.f32_form != 'exact':
        raise ValueError("%s needs dtype=torch.float32 and f32_form='exact' (got %s, %r)" % (who, det.dtype, det.f32_form))


def fc_head_trainable(det, roi_features, keep_prob=1.0, seed=0, image_id=0):
    """det.roi_head(roi_features) of an FC head with a backward pass into fc1, fc2, score and bbox, and tf.nn.dropout(keep_prob) behind
    fc1 (Philox stream 6) and fc2 (stream 7) as the reference trains the VGG16 head (vgg16_faster_rcnn.py:250-253); keep_prob 1 (the
    FPN head): bit-equal to roi_head.  Features that require a gradient (ops.roi_pool_trainable's) get one: fc1's dense_dgrad.
    `det` has fc1, fc2, `dtype`, `f32_form` and _FinalLayer's _final_outputs_trainable (score, bbox): ResNetFpnDetector, Vgg16Detector."""
    require_exact_f32(det, 'roi_head_trainable')
    x = roi_features.reshape(roi_features.shape[0], -1).to(det.dtype)            # Flatten() of NHWC crops
    x = ops.dense_trainable(x, det.fc1.weight, det.fc1.bias, relu=True)
    x = ops.dropout_trainable(x, keep_prob, seed, image_id, ops.DROPOUT_STREAM_FC1)
    x = ops.dense_trainable(x, det.fc2.weight, det.fc2.bias, relu=True)
    x = ops.dropout_trainable(x, keep_prob, seed, image_id, ops.DROPOUT_STREAM_FC2)
    return det._final_outputs_trainable(x)


def flipped_weight(conv, half=False):
    """a 3x3 convolution's weight flipped and transposed (ops.conv3x3_flipped_weight, read off the ops module at every call): the
    weight whose forward convolution is the layer's input gradient; derived on the layer, rebuilt after an optimiser step.
    `half`: times 0.5 -- the neck's s2, so that the convolution's result IS the gradient of l2's output (the merge's 0.5 applied:
    every product and every partial sum is halved exactly, a power of two) and the finest level takes no elementwise pass."""
    if half:
        return derived(conv, 'flip_half', (conv.weight,), lambda w: ops.conv3x3_flipped_weight(w).mul_(0.5))
    return derived(conv, 'flip', (conv.weight,), ops.conv3x3_flipped_weight)


def rows(x):
    """an NHWC map [B,H,W,C] as the Dense backward's [rows, C]"""
    return x.view(-1, int(x.shape[3]))


def weight2d(w):
    """a [cout, cin, 1, 1] weight as the Dense backward's [cout, cin] (the same floats in either memory format)"""
    return w.reshape(int(w.shape[0]), -1).contiguous()


def param_layouts(params):
    return [(tuple(p.shape), tuple(p.stride())) for p in params]


def in_param_layout(g, layout):
    """a [cout, cin] weight gradient as a view in its [cout, cin, 1, 1] parameter's own shape and memory format (param_layouts)"""
    shape, stride = layout
    return torch.as_strided(g, shape, stride, g.storage_offset())


def pointwise_backward(g, x, weight, y_relu=None, x_relu=None, need_dx=True):
    """a 1x1 convolution's backward as the Dense backward over pixels: ops.dense_wgrad, then (need_dx) ops.dense_dgrad, with their
    gates.  ``g`` [B,H,W,cout], ``x`` [B,H,W,cin] contiguous NHWC, ``weight`` [cout,cin,1,1] -> (dw [cout,cin], db, dx like x or None)"""
    gate = None if y_relu is None else rows(y_relu)
    dw, db = ops.dense_wgrad(rows(g), rows(x), y_relu=gate)
    dx = None
    if need_dx:
        dx = ops.dense_dgrad(rows(g), weight2d(weight), y_relu=gate, x_relu=None if x_relu is None else rows(x_relu)).view(x.shape)
    return dw, db, dx
