"""Losses -- counterpart of the reference's model/losses.py (:4-28), on torch tensors (autograd-capable), and the fused
HIP losses on the compact targets (csrc/losses.hip) as torch.autograd Functions."""
import torch
import torch.nn.functional as F

__all__ = ['cls_loss', 'smooth_l1_loss', 'fused_rpn_losses', 'fused_roi_losses']


def cls_loss(logits, labels, weight=1):
    """tf.losses.sparse_softmax_cross_entropy(logits, labels, weights=weight) with its default reduction
    (SUM_BY_NONZERO_WEIGHTS): weighted sum / number of non-zero weights."""
    ce = F.cross_entropy(logits, labels.to(torch.int64), reduction='none')
    w = torch.as_tensor(weight, dtype=ce.dtype, device=ce.device)
    w = w.expand_as(ce) if w.dim() > 0 else w.expand(ce.shape)
    nz = (w != 0).sum().clamp_min(1).to(ce.dtype)
    return (ce * w).sum() / nz


def smooth_l1_loss(bbox_pred, bbox_targets, bbox_inside_weights, bbox_outside_weights, sigma=1.0, dim=(1,)):
    """losses.py:16-28: smooth L1 with the py-faster-rcnn sigma, summed over `dim`, mean over the rest."""
    sigma_2 = sigma ** 2
    in_box_diff = bbox_inside_weights * (bbox_pred - bbox_targets)
    abs_in = in_box_diff.abs()
    sign = (abs_in < 1.0 / sigma_2).to(in_box_diff.dtype).detach()
    in_loss = in_box_diff.pow(2) * (sigma_2 / 2.0) * sign + (abs_in - 0.5 / sigma_2) * (1.0 - sign)
    return (bbox_outside_weights * in_loss).sum(dim=tuple(dim)).mean()


class _FusedRpnLoss(torch.autograd.Function):
    """ops.rpn_losses forward (losses + the compact unit gradients), ops.rpn_losses_backward backward"""

    @staticmethod
    def forward(ctx, scores, deltas, sample_idx, sample_targets, counts, sigma, layout, num_anchors):
        from .. import ops
        out = ops.rpn_losses(scores, deltas, sample_idx, sample_targets, counts, sigma, layout, num_anchors)
        ctx.save_for_backward(sample_idx, out.row_grad_scores, out.row_grad_deltas)
        ctx.head = (scores.shape, deltas.shape, scores.dtype, deltas.dtype, deltas.numel() // (4 * sample_idx.shape[0]),
                    layout, num_anchors)
        return out.losses[:, 0], out.losses[:, 1]

    @staticmethod
    def backward(ctx, grad_cls, grad_reg):
        from .. import ops
        sample_idx, row_gs, row_gd = ctx.saved_tensors
        s_shape, d_shape, s_dtype, d_dtype, n, layout, num_anchors = ctx.head
        upstream = torch.stack([grad_cls.float(), grad_reg.float()], dim=1).contiguous()
        g = ops.rpn_losses_backward(sample_idx, row_gs, row_gd, upstream, n, layout, num_anchors,
                                    scores=ctx.needs_input_grad[0], deltas=ctx.needs_input_grad[1])
        gs = None if g.grad_scores is None else g.grad_scores.reshape(s_shape).to(s_dtype)
        gd = None if g.grad_deltas is None else g.grad_deltas.reshape(d_shape).to(d_dtype)
        return gs, gd, None, None, None, None, None, None


class _FusedRoiLoss(torch.autograd.Function):
    """ops.roi_losses: the losses in forward, the dense gradients at the arriving upstream in backward (one launch each)"""

    @staticmethod
    def forward(ctx, scores, deltas, final_labels, targets, inside, outside, counts, row_map, sigma):
        from .. import ops
        out = ops.roi_losses(scores, deltas, final_labels, targets, inside, outside, counts, sigma, row_map=row_map, grads=False)
        ctx.save_for_backward(scores, deltas, final_labels, targets, inside, outside, counts, row_map)
        ctx.sigma = sigma
        return out.losses[:, 0], out.losses[:, 1]

    @staticmethod
    def backward(ctx, grad_cls, grad_reg):
        from .. import ops
        scores, deltas, final_labels, targets, inside, outside, counts, row_map = ctx.saved_tensors
        upstream = torch.stack([grad_cls.float(), grad_reg.float()], dim=1).contiguous()
        g = ops.roi_losses(scores, deltas, final_labels, targets, inside, outside, counts, ctx.sigma, row_map=row_map,
                           upstream=upstream, losses=False, grad_scores=ctx.needs_input_grad[0],
                           grad_deltas=ctx.needs_input_grad[1])
        gs = None if g.grad_scores is None else g.grad_scores.to(scores.dtype)
        gd = None if g.grad_deltas is None else g.grad_deltas.to(deltas.dtype)
        return gs, gd, None, None, None, None, None, None, None


def fused_rpn_losses(scores, deltas, anchor_targets, sigma, layout, num_anchors):
    """The RPN pair of base_fpn_model.py:278-289 / base_faster_rcnn_model.py:200-215 for a batch, from the COMPACT anchor
    targets (ops.AnchorTargets of `FusedAnchorTarget.batch(..., dense=False)`): scores in `layout` (ops.RPN_LAYOUT_*, `num_anchors` =
    anchors per location; any shape of 2N floats per image), deltas of 4N floats per image -> (cls [B], reg [B]).  `.backward()` through either leaves
    the dense gradients in scores.grad / deltas.grad (zero outside the sampled rows).  float32 only: cast with .float()."""
    return _FusedRpnLoss.apply(scores, deltas, anchor_targets.sample_idx, anchor_targets.sample_targets, anchor_targets.counts,
                               float(sigma), int(layout), int(num_anchors))


def fused_roi_losses(scores, deltas, proposal_targets, sigma, row_map=None):
    """The RoI pair of base_fpn_model.py:291-301 for a batch: scores [B,R,C], deltas [B,R,4C] of the head on the sampled RoIs,
    `proposal_targets` = ops.ProposalTargets; row_map int32 [B,R] = the target row of every head row (the FPN caller's
    level-order permutation; None: identity) -> (cls [B], reg [B]), differentiable with respect to scores and deltas."""
    if row_map is not None:
        row_map = row_map.to(torch.int32).contiguous()
    t = proposal_targets
    return _FusedRoiLoss.apply(scores, deltas, t.final_labels, t.targets, t.inside, t.outside, t.counts, row_map, float(sigma))
