"""The float32 ResnetFpnNeck of model/fpn_detector.py with a backward pass: ResNetFpnDetector.neck_trainable.  The forward is neck()'s
own launches (outputs bit-equal, same shapes and strides); the backward runs the neck in reverse on this package's kernels -- the
three 3x3 output convolutions' weight gradients as ops.conv3x3_wgrad_f32_levels and their input gradients as the forward kernel on
the flipped weights, the top-down merges' backward as ops.fpn_topdown_backward (one launch per coarse level: the resize's transpose
with the level's other gradient terms folded in), the four 1x1 convolutions as the Dense backward over pixels (layers: model/layers.py)."""
import torch

from .. import ops
from .layers import _conv_epi, _nhwc
from .trainable_common import flipped_weight, in_param_layout, param_layouts, pointwise_backward, require_exact_f32

_LAYERS = ('p5', 'l4', 'l3', 'l2', 's4', 's3', 's2')


@ops.carries_grad_form
class _NeckTrainable(torch.autograd.Function):
    """The float32 neck with a backward pass.  Forward: neck()'s launches; saves C2..C5 and the merged maps m2..m4 (the inputs of
    s2..s4, which the forward has in memory anyway).  Backward, with dP2..dP6 arriving (any of them may be absent and drops its
    terms): s_k's dw / db and input gradient per level -> the cascade from fine to coarse, h_k = the gradient of level k's
    lateral output = the gradient of the resized map one level up:
        h2 = s2's input gradient on the HALVED flipped weight (trainable_common.flipped_weight(half=True): no elementwise pass)
        h3 = fpn_topdown_backward(h2, base = s3's input gradient, out_scale = 0.5)
        h4 = fpn_topdown_backward(h3, base = s4's input gradient, out_scale = 0.5)
        g5 = fpn_topdown_backward(h4, base = dP5, sub = dP6, out_scale = 1)
    -> the 1x1 layers as Dense layers over pixels (trainable_common.pointwise_backward): dw / db from (h_k, C_k) (p5: g5, C5), and
    the input gradient into a C_k only where that map requires one."""

    @staticmethod
    def forward(ctx, det, wf4, wf3, wf2h, c2, c3, c4, c5, *params):
        ctx.set_materialize_grads(False)                                         # (an output nothing reads arrives as None)
        p5 = _conv_epi(det.p5, c5)
        p6 = p5[:, :, ::2, ::2]                                                  # MaxPooling2D(1x1, stride 2)
        m4 = det._lateral_merge(p5, det.l4, c4)
        m3 = det._lateral_merge(m4, det.l3, c3)
        m2 = det._lateral_merge(m3, det.l2, c2)
        outs = (_conv_epi(det.s2, m2), _conv_epi(det.s3, m3), _conv_epi(det.s4, m4), p5, p6)
        ctx.layouts = param_layouts(params)
        ctx.save_for_backward(wf4, wf3, wf2h, *[_nhwc(t) for t in (c2, c3, c4, c5, m2, m3, m4)], *params)
        return outs

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *d_outs):
        wf4, wf3, wf2h, c2, c3, c4, c5, m2, m3, m4 = ctx.saved_tensors[:10]
        weights = dict(zip(_LAYERS, ctx.saved_tensors[10::2]))
        dp2, dp3, dp4, dp5, dp6 = [None if g is None else _nhwc(g) for g in d_outs]
        grads = {}
        # the 3x3 output convolutions: parameter gradients, and the input gradient (s2's already halved: h2)
        dm = {}
        for name, m, dp, wf in (('s4', m4, dp4, wf4), ('s3', m3, dp3, wf3), ('s2', m2, dp2, wf2h)):
            if dp is None:
                continue
            dw, db = ops.conv3x3_wgrad_f32_levels([m], [dp])
            grads[name] = (ops._conv3x3_weight_grad(dw, weights[name]), db)
            dm[name] = ops.conv3x3_dgrad_f32_levels([dp], weights[name], flipped=wf)[0]
        # the cascade, fine to coarse
        h = dm.get('s2')
        hs = {'l2': h}
        for lat, name, m in (('l3', 's3', m3), ('l4', 's4', m4)):
            base = dm.get(name)
            if h is not None or base is not None:
                h = ops.fpn_topdown_backward(h, m.shape[1:3], base=base, out_scale=0.5)
            hs[lat] = h
        if h is not None or dp5 is not None or dp6 is not None:
            h = ops.fpn_topdown_backward(h, c5.shape[1:3], base=dp5, sub=dp6, out_scale=1.0)
        hs['p5'] = h
        # the 1x1 layers as Dense layers over pixels
        d_c = []
        for i, (name, c) in enumerate((('l2', c2), ('l3', c3), ('l4', c4), ('p5', c5))):
            g, dx = hs[name], None
            if g is not None:
                dw, db, dx = pointwise_backward(g, c, weights[name], need_dx=ctx.needs_input_grad[4 + i])
                grads[name] = (dw, db)
            d_c.append(None if dx is None else dx.permute(0, 3, 1, 2))
        # in the order of the parameters, each gradient in its parameter's own shape and memory format (a [256, cin, 1, 1] weight:
        # the same 256 x cin floats in either format)
        d_params = []
        for i, name in enumerate(_LAYERS):
            dw, db = grads.get(name, (None, None))
            if dw is not None and dw.dim() == 2:
                dw = in_param_layout(dw, ctx.layouts[2 * i])
            d_params += [dw, db]
        return (None, None, None, None) + tuple(d_c) + tuple(d_params)


def neck_trainable(det, c_list):
    """det.neck(c_list) with a backward pass into p5, l4, l3, l2, s4, s3 and s2: `.backward()` leaves the fourteen parameters'
    gradients in their own shapes and memory formats and carries a gradient into those maps of c_list that require one (the
    models' own maps do with train_extractor: model/extractor_trainable.py)."""
    require_exact_f32(det, 'neck_trainable')
    flips = (None, None, None)
    if torch.is_grad_enabled():
        flips = (flipped_weight(det.s4), flipped_weight(det.s3), flipped_weight(det.s2, half=True))
    params = [p for name in _LAYERS for p in (getattr(det, name).weight, getattr(det, name).bias)]
    return _NeckTrainable.apply(det, *flips, *c_list, *params)
