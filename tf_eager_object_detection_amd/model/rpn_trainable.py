"""The float32 RpnHead with a backward pass: ResNetFpnDetector.rpn_trainable over the levels, SingleLevelDetector.rpn_trainable on its
one.  The forward is the FPN rpn()'s own launches (outputs bit-equal); the backward runs the head's layers in reverse on this package's
kernels -- the pair of 1x1 convolutions (its derived weights: model/layers.py) as the Dense backward over pixels (ops.dense_wgrad /
dense_dgrad), the 3x3 convolution's weight gradient as ops.conv3x3_wgrad_f32_levels over all levels in one call, its input gradient
as the forward kernel on the flipped weight."""
import torch

from .. import ops
from .layers import _nhwc, _no_kernel, _own_conv3x3, rpn_pair_padded, rpn_pair_weights
from .trainable_common import flipped_weight, in_param_layout, param_layouts, require_exact_f32


@ops.carries_grad_form
class _RpnHeadTrainable(torch.autograd.Function):
    """The float32 RpnHead over all levels with a backward pass.  Forward: rpn()'s launches, with the levels' 512-channel
    activations h in ONE [sum rows, 512] buffer (the 3x3 convolution writes the levels' views), so that the pair of 1x1
    convolutions is one GEMM over all levels.  Backward: unpack per level -> the pair's dw / db (ops.dense_wgrad) and dh
    (ops.dense_dgrad with x_relu = h: the 3x3 layer's ReLU gate in its epilogue) over all rows at once -> the 3x3 layer's dw / db
    in one ops.conv3x3_wgrad_f32_levels call -> dx (the forward kernel on the flipped weight) only when a map requires one."""

    @staticmethod
    def forward(ctx, conv_w, conv_b, score_w, score_b, bbox_w, bbox_b, wpad, bpair, wflip, A, *xs):
        B = int(xs[0].shape[0])
        rows = [B * int(x.shape[1]) * int(x.shape[2]) for x in xs]
        cmid = int(conv_w.shape[0])
        hbuf = torch.empty((sum(rows), cmid), dtype=torch.float32, device=xs[0].device)
        hs, off = [], 0
        for x, r in zip(xs, rows):
            hs.append(hbuf[off:off + r].view(B, int(x.shape[1]), int(x.shape[2]), cmid))
            off += r
        ops.conv3x3_f32_levels(list(xs), conv_w, conv_b, relu=True, outs=hs)
        pair = ops.dense(hbuf, wpad, None)
        n = sum(rows) // B * A
        scores = torch.empty((B, n, 2), dtype=torch.float32, device=hbuf.device)
        deltas = torch.empty((B, n, 4), dtype=torch.float32, device=hbuf.device)
        off = aoff = 0
        for r in rows:
            ops.rpn_pack_pair(pair[off:off + r, :6 * A].contiguous().view(B, 1, r // B, 6 * A), bpair, A, scores, deltas, aoff)
            off += r
            aoff += r // B * A
        ctx.A, ctx.rows, ctx.B, ctx.n = A, rows, B, len(xs)
        ctx.pair_layouts = param_layouts((score_w, bbox_w))
        ctx.save_for_backward(hbuf, wpad, wflip, conv_w, *xs)
        return scores, deltas

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_scores, d_deltas):
        hbuf, wpad, wflip, conv_w = ctx.saved_tensors[:4]
        xs = list(ctx.saved_tensors[4:])
        A, B, rows = ctx.A, ctx.B, ctx.rows
        n = sum(rows) // B * A
        d_scores = torch.zeros((B, n, 2), dtype=torch.float32, device=hbuf.device) if d_scores is None else d_scores.contiguous()
        d_deltas = torch.zeros((B, n, 4), dtype=torch.float32, device=hbuf.device) if d_deltas is None else d_deltas.contiguous()
        dpair = torch.empty((sum(rows), int(wpad.shape[0])), dtype=torch.float32, device=hbuf.device)
        off = aoff = 0
        for r in rows:
            ops.rpn_unpack_pair(d_scores, d_deltas, A, r // B, aoff, dpair[off:off + r])
            off += r
            aoff += r // B * A
        dwp, dbp = ops.dense_wgrad(dpair, hbuf)
        dh = ops.dense_dgrad(dpair, wpad, x_relu=hbuf)
        dhs, off = [], 0
        for x, r in zip(xs, rows):
            dhs.append(dh[off:off + r].view(B, int(x.shape[1]), int(x.shape[2]), -1))
            off += r
        dw3, db3 = ops.conv3x3_wgrad_f32_levels(xs, dhs)
        dxs = [None] * ctx.n
        if any(ctx.needs_input_grad[10:]):
            got = ops.conv3x3_dgrad_f32_levels(dhs, conv_w, flipped=wflip)
            dxs = [g if need else None for g, need in zip(got, ctx.needs_input_grad[10:])]
        n2, n6 = 2 * A, 6 * A
        # the pair's rows in the two parameters' own shapes and strides ([n, 512, 1, 1]: the same n x 512 floats in either format)
        dws = [in_param_layout(g, layout) for g, layout in zip((dwp[:n2], dwp[n2:n6]), ctx.pair_layouts)]
        return (ops._conv3x3_weight_grad(dw3, conv_w), db3, dws[0], dbp[:n2], dws[1], dbp[n2:n6], None, None, None, None) + tuple(dxs)


def rpn_trainable(det, p_list):
    """det.rpn(p_list) with a backward pass into rpn_conv, rpn_score and rpn_bbox: `.backward()` leaves the six parameters'
    gradients in their own shapes and memory formats -- the pair's from the padded [64, 512] contraction, handed out as row
    slices the way _FinalTrainable does -- and carries a gradient into those maps of p_list that require one (the models' own
    maps do with train_neck=True: neck_trainable consumes it)."""
    require_exact_f32(det, 'rpn_trainable')
    p0 = p_list[0]
    if not _own_conv3x3(det.rpn_conv, p0) or det.rpn_conv.out_channels % 256:
        raise _no_kernel('RpnHead', det.rpn_conv, p0)
    w, b = rpn_pair_weights(det)
    # (the flipped weight, 4.7 MB, only where the backward pass will compute an input gradient)
    wflip = flipped_weight(det.rpn_conv) if torch.is_grad_enabled() and any(p.requires_grad for p in p_list) else None
    return _RpnHeadTrainable.apply(det.rpn_conv.weight, det.rpn_conv.bias, det.rpn_score.weight, det.rpn_score.bias,
                                   det.rpn_bbox.weight, det.rpn_bbox.bias, rpn_pair_padded(det, w), b, wflip, det.A,
                                   *[_nhwc(p) for p in p_list])
