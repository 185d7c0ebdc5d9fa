"""The float32 ResNet extractor of model/fpn_detector.py with a backward pass: ResNetFpnDetector.extractor_trainable (reference
resnet_fpn.py:208-289: conv1_conv and conv2..conv5 trainable, batch-norm frozen -- _fold_frozen_bn has folded it into the weights,
so the folded weights ARE the parameters).  One torch.autograd.Function per bottleneck (model/layers.py's _Block): the forward is
_Block.forward's own launches (outputs bit-equal, same shapes and strides); the backward runs the block in reverse on this package's
kernels -- the 1x1 convolutions as the Dense backward over pixels with the ReLU gates applied while staging, the 3x3 convolution's
weight gradient as ops.conv3x3_wgrad_f32_levels and its input gradient as the forward kernel on the flipped weight, the block's join
(shortcut + first convolution, with the stride-2 scatter of a stage's first block) as ops.block_input_grad.  The stem (conv1 and
its pooling), which the reference trains as well (resnet_fpn.py:233: trainable=True), runs under no_grad by default and conv1 stays
frozen; with `train_stem` it runs ops.stem_trainable -- the overlapping max-pooling's backward, then conv1's weight and bias
gradient as ONE ops.dense_wgrad on the stem's patch matrix -- and every parameter of the extractor receives a gradient."""
import torch

from .. import ops
from ..derived import derived
from .layers import _conv_epi, _nhwc, _stem
from .trainable_common import flipped_weight, in_param_layout, param_layouts, pointwise_backward, require_exact_f32

STAGES = ('conv2', 'conv3', 'conv4', 'conv5')


def block_layers(blk):
    """a bottleneck's convolutions in the order of its parameters: c1, c2, c3 (, short)"""
    return (blk.c1, blk.c2, blk.c3) + ((blk.short,) if blk.short is not None else ())


@ops.carries_grad_form
class _BlockTrainable(torch.autograd.Function):
    """One bottleneck with a backward pass.  Forward: _Block.forward's float32 launches (pointwise, conv3x3_f32, then pointwise with
    the residual or pointwise_dual); saves the block's input x (a strided block: xs = stride_gather(x, s) in its place, the only form
    the backward reads), c1's output a, c2's output b and the block's output y.  Backward, with dy arriving:
        c3     dw, db = dense_wgrad(dy, b, y_relu=y);   db_gated = dense_dgrad(dy, w3, y_relu=y, x_relu=b)   (c2's ReLU gate applied)
        c2     dw, db = conv3x3_wgrad_f32_levels([a], [db_gated]);   da = conv3x3_dgrad_f32_levels([db_gated], w2, flipped)
        c1     dw, db = dense_wgrad(da, x or xs, y_relu=a);   d1 = dense_dgrad(da, w1, y_relu=a)              (d1, d2, dx only when x
        short  dw, db = dense_wgrad(dy, x or xs, y_relu=y);   d2 = dense_dgrad(dy, ws, y_relu=y)               requires a gradient)
        dx = block_input_grad(d1, dy, y)  (identity shortcut)  or  block_input_grad(d1, d2=d2, stride, in_hw)  (convolutional one)
    Each 1x1 line is one trainable_common.pointwise_backward.  The forward's concatenated [w3 | ws] weight is a forward detail:
    the backward reads the two parameters themselves."""

    @staticmethod
    def forward(ctx, blk, wf2, x, *params):
        ctx.set_materialize_grads(False)                                         # (an output nothing reads arrives as None)
        a = _conv_epi(blk.c1, x, relu=True)
        b = _conv_epi(blk.c2, a, relu=True)
        stride = int(blk.c1.stride[0])
        if blk.short is not None:
            w, bias = blk._dual_weights()
            y = ops.pointwise_dual(_nhwc(b), _nhwc(x), w, bias, stride, relu=True).permute(0, 3, 1, 2)
        else:
            y = _conv_epi(blk.c3, b, relu=True, residual=x)
        if wf2 is not None:                                                       # (None: no graph is being recorded)
            xn = _nhwc(x)
            ctx.stride, ctx.in_hw = stride, (int(xn.shape[1]), int(xn.shape[2]))
            ctx.layouts = param_layouts(params)
            ctx.save_for_backward(wf2, xn if stride == 1 else ops.stride_gather(xn, stride), _nhwc(a), _nhwc(b), _nhwc(y), *params)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        n_params = len(ctx.layouts)
        if dy is None:
            return (None,) * (3 + n_params)
        wf2, xs, a, b, y = ctx.saved_tensors[:5]
        weights = ctx.saved_tensors[5::2]
        need_dx = ctx.needs_input_grad[2]
        dy = _nhwc(dy)
        # c3, then c2 on the gradient that leaves c3 already gated by c2's ReLU
        dw3, db3, db_gated = pointwise_backward(dy, b, weights[2], y_relu=y, x_relu=b)
        dw2, db2 = ops.conv3x3_wgrad_f32_levels([a], [db_gated])
        da = ops.conv3x3_dgrad_f32_levels([db_gated], weights[1], flipped=wf2)[0]
        # c1 and the shortcut convolution read the block's (subsampled) input
        dw1, db1, d1 = pointwise_backward(da, xs, weights[0], y_relu=a, need_dx=need_dx)
        grads = [(dw1, db1), (ops._conv3x3_weight_grad(dw2, weights[1]), db2), (dw3, db3)]
        dx = None
        if n_params == 8:
            dws, dbs, d2 = pointwise_backward(dy, xs, weights[3], y_relu=y, need_dx=need_dx)
            grads.append((dws, dbs))
            if need_dx:
                dx = ops.block_input_grad(d1, d2=d2, stride=ctx.stride, in_hw=ctx.in_hw)
        elif need_dx:
            dx = ops.block_input_grad(d1, dy=dy, y=y)
        # in the order of the parameters, each gradient in its parameter's own shape and memory format (a [cout, cin, 1, 1] weight:
        # the same cout x cin floats in either format)
        d_params = []
        for i, (dw, db) in enumerate(grads):
            if dw.dim() == 2:
                dw = in_param_layout(dw, ctx.layouts[2 * i])
            d_params += [dw, db]
        return (None, None, None if dx is None else dx.permute(0, 3, 1, 2)) + tuple(d_params)


def block_trainable(blk, x):
    """blk(x) (a layers._Block on a channels_last float32 map) with a backward pass into the block's 6 or 8 parameters, and into
    x when it requires a gradient; float32, f32_form 'exact' only"""
    if x.dtype != torch.float32 or ops.current_f32_form() != 'exact':
        raise ValueError("block_trainable needs a float32 map and f32_form='exact' (the bottleneck backward has no float16 or "
                         "split-precision form), got %s, %r" % (x.dtype, ops.current_f32_form()))
    wf2 = flipped_weight(blk.c2) if torch.is_grad_enabled() else None
    params = [p for conv in block_layers(blk) for p in (conv.weight, conv.bias)]
    return _BlockTrainable.apply(blk, wf2, x, *params)


def stem_trainable(conv1, images_nhwc):
    """_stem(conv1, images_nhwc, torch.float32) with a backward pass into conv1 (ops.stem_trainable on the layer's cached patch
    weight): the same launches, bit-equal, with its shape and strides"""
    w = derived(conv1, 'stem_f32', (conv1.weight,), lambda weight: ops.patch_weight(weight, ops.STEM_PATCH_K))
    return ops.stem_trainable(images_nhwc, conv1.weight, conv1.bias, stem_weight=w).permute(0, 3, 1, 2)


def extractor_trainable(det, images_nhwc, train_stem=False):
    """det.extractor(images_nhwc) with a backward pass into conv2..conv5: (C2, C3, C4, C5), bit-equal to extractor()'s.  The stem
    (conv1 + pooling) runs under no_grad as in extractor() and conv1 stays frozen, unless `train_stem`: then it runs stem_trainable,
    conv2's first block sees an input that requires a gradient (block_input_grad's convolutional-shortcut form at stride 1) and
    conv1's weight and bias receive theirs."""
    require_exact_f32(det, 'extractor_trainable')
    if train_stem:
        x = stem_trainable(det.conv1, images_nhwc)
    else:
        with torch.no_grad():
            x = _stem(det.conv1, images_nhwc, det.dtype)
    outs = []
    for name in STAGES:
        for blk in getattr(det, name):
            x = block_trainable(blk, x)
        outs.append(x)
    return tuple(outs)
