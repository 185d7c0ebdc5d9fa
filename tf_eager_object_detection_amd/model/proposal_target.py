"""RoI-head training targets -- counterpart of the reference's model/proposal_target.py (ProposalTarget, :8-124).

SURVEY.md section 8(f) rank 4: pairwise_iou (a9) and encode_bbox_with_mean_and_std (a6) are the path's HIP
kernels; sampling uses a torch generator where the reference uses tf.random_shuffle / np.random.choice, so parity
is exact on the assignment (`assign`) and distribution-level on the sampled batch."""
import torch

from .. import ops
from ..utils.bbox_tf import pairwise_iou
from ..utils.bbox_transform import encode_bbox_with_mean_and_std

__all__ = ['ProposalTarget', 'FusedProposalTarget', 'training_target_layers']


class ProposalTarget:
    """Same constructor and call signature as the reference's keras model.

    reference_row_labels=True keeps a quirk of the reference: the class column a positive row's targets and
    inside weights are written to is taken from `labels[row]` (:96, :113 -- the label of RoI number `row` of the
    INPUT, not of the sampled foreground RoI in that row); False uses the sampled RoI's own label."""

    def __init__(self, num_classes=21, pos_iou_threshold=0.5, neg_iou_threshold=0.5, total_num_samples=128,
                 max_pos_samples=32, target_means=None, target_stds=None, generator=None, reference_row_labels=True):
        self._num_classes = num_classes
        self._pos_iou_threshold = pos_iou_threshold
        self._neg_iou_threshold = neg_iou_threshold
        self._total_num_samples = total_num_samples
        self._max_pos_samples = max_pos_samples
        self._target_means = [0, 0, 0, 0] if target_means is None else target_means
        self._target_stds = [1, 1, 1, 1] if target_stds is None else target_stds
        self._generator = generator
        self._reference_row_labels = reference_row_labels

    def assign(self, rois, gt_bboxes, gt_labels):
        """The deterministic part (:55-63): -> (labels of the best-overlapping gt per RoI, gt_assignment int64,
        fg_inds, bg_inds)."""
        iou = pairwise_iou(rois, gt_bboxes)                                                # :55
        max_overlaps, gt_assignment = iou.max(dim=1)                                       # :56-57
        labels = gt_labels[gt_assignment]                                                  # :58
        fg = (max_overlaps >= self._pos_iou_threshold).nonzero()[:, 0]                     # :61
        bg = ((max_overlaps < self._pos_iou_threshold) &
              (max_overlaps >= self._neg_iou_threshold)).nonzero()[:, 0]                   # :62-63
        return labels, gt_assignment, fg, bg

    def _shuffle(self, t):
        return t[torch.randperm(t.numel(), device=t.device, generator=self._generator)]

    def __call__(self, inputs, training=None, mask=None):
        rois, gt_bboxes, gt_labels = inputs
        labels, gt_assignment, fg, bg = self.assign(rois, gt_bboxes, gt_labels)
        if fg.numel() > self._max_pos_samples:                                             # :66-67
            fg = self._shuffle(fg)[:self._max_pos_samples]
        want_bg = self._total_num_samples - fg.numel()
        if bg.numel() > want_bg:                                                           # :68-70
            bg = self._shuffle(bg)[:want_bg]
        elif bg.numel() < want_bg:                                                         # :73-76 np.random.choice
            if bg.numel() == 0:
                raise ValueError('no background RoI to sample from (the reference fails here as well)')
            pick = torch.randint(0, bg.numel(), (want_bg,), device=bg.device, generator=self._generator)
            bg = bg[pick]
        keep = torch.cat([fg, bg])                                                         # :80
        final_rois = rois[keep]
        final_labels = labels[keep].clone()
        final_labels[fg.numel():] = 0                                                      # :84-85
        nfg, nk = fg.numel(), keep.numel()
        inside = torch.zeros((nk, self._num_classes, 4), dtype=torch.float32, device=rois.device)
        targets = torch.zeros_like(inside)
        if nfg > 0:
            rows = torch.arange(nfg, device=rois.device)
            cols = (labels[:nfg] if self._reference_row_labels else labels[fg]).to(torch.int64)   # :96 / :113
            inside[rows, cols] = 1.0
            enc = encode_bbox_with_mean_and_std(final_rois[:nfg], gt_bboxes[gt_assignment[fg]],
                                                target_means=self._target_means, target_stds=self._target_stds)
            targets[rows, cols] = enc                                                      # :103-113
        inside = inside.reshape(nk, self._num_classes * 4)
        targets = targets.reshape(nk, self._num_classes * 4)
        return final_rois, final_labels, targets, inside, torch.ones_like(inside)          # :118-124

    call = __call__


class FusedProposalTarget:
    """The same batch from ONE call of the fused HIP stage (ops.proposal_targets, csrc/targets.hip), sampled by the
    counter-based rule of include/odet.h.  Outputs have the fixed shape [total_num_samples, ...].

    strict=True reads the call's `counts` once and raises the ValueError of `ProposalTarget` for an image that wants
    background rows and has no candidate; strict=False never touches the host (such an image has rows written < S)."""

    def __init__(self, num_classes=21, pos_iou_threshold=0.5, neg_iou_threshold=0.5, total_num_samples=128,
                 max_pos_samples=32, target_means=None, target_stds=None, seed=0, reference_row_labels=True, strict=True):
        self._num_classes = num_classes
        self._pos_iou_threshold = pos_iou_threshold
        self._neg_iou_threshold = neg_iou_threshold
        self._total_num_samples = total_num_samples
        self._max_pos_samples = max_pos_samples
        self._target_means = [0, 0, 0, 0] if target_means is None else target_means
        self._target_stds = [1, 1, 1, 1] if target_stds is None else target_stds
        self._seed = seed
        self._reference_row_labels = reference_row_labels
        self._strict = strict
        self._next_image_id = 0

    def batch(self, rois, gt_boxes, gt_labels, gt_offsets, first_image_id=0, roi_counts=None, strict=None):
        """rois [B,Rmax,4], packed ground truth -> ops.ProposalTargets, every tensor batch-first.  `strict` overrides the
        layer's setting for this call (False: no host read)."""
        out = ops.proposal_targets(rois, gt_boxes, gt_labels, gt_offsets, self._num_classes, self._pos_iou_threshold,
                                   self._neg_iou_threshold, self._total_num_samples, self._max_pos_samples,
                                   self._target_means, self._target_stds, reference_row_labels=self._reference_row_labels,
                                   seed=self._seed, first_image_id=first_image_id, roi_counts=roi_counts)
        if (self._strict if strict is None else strict) and \
                bool((out.counts[:, 3] < self._total_num_samples).any()):                       # the one host read
            raise ValueError('no background RoI to sample from (the reference fails here as well)')
        return out

    def __call__(self, inputs, training=None, mask=None):
        rois, gt_bboxes, gt_labels = inputs
        off = torch.tensor([0, gt_bboxes.shape[0]], dtype=torch.int32, device=rois.device)
        out = self.batch(rois.reshape(1, -1, 4), gt_bboxes, gt_labels, off, first_image_id=self._next_image_id)
        self._next_image_id += 1
        return out.final_rois[0], out.final_labels[0].to(gt_labels.dtype), out.targets[0], out.inside[0], out.outside[0]

    call = __call__


def training_target_layers(kind, anchor_kw, proposal_kw):
    """The (anchor target, proposal target) pair of a caller model: `kind` = 'torch' (AnchorTarget / ProposalTarget, tensor
    ops around the kernels, generator-driven sampling) or 'hip' (the fused stage, counter-based sampling)."""
    from .anchor_target import AnchorTarget, FusedAnchorTarget
    if kind == 'torch':
        return AnchorTarget(**anchor_kw), ProposalTarget(**proposal_kw)
    if kind == 'hip':
        return FusedAnchorTarget(**anchor_kw), FusedProposalTarget(**proposal_kw)
    raise ValueError("training_targets must be 'torch' or 'hip', got %r" % (kind,))
