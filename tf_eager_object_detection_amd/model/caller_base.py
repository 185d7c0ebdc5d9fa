"""What the two families of caller objects (model/base_fpn_model.py: BaseFPN / ResnetV1Fpn; model/base_faster_rcnn_model.py:
BaseFasterRcnn and its concrete models) share: ONE pass -- the front (dense parts -> anchors -> fg softmax -> RegionProposal), both
training branches, pooling + RoI head of a training call, the inference tail, im_detect -- written once in `CallerModel`; the
grad-mode rule (`run_part`), the train flags' dependency check, the construction of the layers both families build, the RpnHead's
implementation and the plumbing of a model whose dense parts are a detector (`DenseParts`).  A family supplies its constructor, its
sequence of dense parts with its anchor generation (`_dense_front`), its RPN layout constant, how its pooling layer is called and
what the RoI head's rows are (see `CallerModel`).  This module depends on neither detector file and neither caller file; both
caller files import from it.

The training branches run every dense part under no_grad unless a keyword switched its backward pass on (`_train_extractor`,
`_train_neck`, `_train_rpn_head`, `_train_roi_head`; float32, f32_form 'exact'): that part then runs its trainable form in the
caller's grad mode, and the losses carry a graph into its layers."""
import torch

from .. import ops
from .detector_base import caller_range_checked  # noqa: F401
from .layers import _nhwc  # noqa: F401  (the callers' NHWC view, the detectors' own helper)
from .losses import cls_loss, fused_roi_losses, fused_rpn_losses, smooth_l1_loss
from .prediction import post_ops_prediction
from .proposal_target import training_target_layers
from .region_proposal import RegionProposal


def check_training_losses(training_losses, training_targets):
    """training_losses: 'torch' = model/losses.py on the dense targets, 'hip' = the fused losses on the compact targets (which
    only the fused target stage produces)"""
    if training_losses not in ('torch', 'hip'):
        raise ValueError("training_losses must be 'torch' or 'hip', got %r" % (training_losses,))
    if training_losses == 'hip' and training_targets != 'hip':
        raise ValueError("training_losses='hip' needs training_targets='hip', got training_targets=%r" % (training_targets,))
    return training_losses


def check_train_dependencies(train_extractor, train_neck, train_rpn_head, train_roi_head, has_neck, train_stem=False):
    """a part trains only when a gradient reaches it.  With a neck (FPN): C2..C5 receive one only through neck_trainable, and the
    neck's outputs only through the RpnHead's input gradient or the trainable RoI pooling.  Without one (single level): the
    shared map receives one only through those two.  The stem (FPN only) receives one only through conv2's first block."""
    head = train_rpn_head or train_roi_head
    if train_stem and not train_extractor:
        raise ValueError('train_stem=True needs train_extractor=True: no gradient reaches the stem otherwise')
    if train_extractor and has_neck and not train_neck:
        raise ValueError('train_extractor=True needs train_neck=True: no gradient reaches the extractor otherwise')
    if train_neck and not head:
        raise ValueError('train_neck=True needs train_rpn_head=True or train_roi_head=True: no gradient reaches the neck otherwise')
    if train_extractor and not has_neck and not head:
        raise ValueError('train_extractor=True needs train_rpn_head=True or train_roi_head=True: no gradient reaches the extractor '
                         'otherwise')


def run_part(on, trainable, plain):
    """the grad-mode rule of the training branches: `on` (a training call AND the part's train flag) runs `trainable()` in the
    caller's grad mode; everything else runs `plain()` under no_grad"""
    if on:
        return trainable()
    with torch.no_grad():
        return plain()


def _image_nhwc(image):
    """the reference's input: one preprocessed image [1,H,W,3] float (model/roi_pooling.py:28: batch 1)"""
    if not isinstance(image, torch.Tensor) or image.dim() != 4 or image.shape[0] != 1 or image.shape[3] != 3:
        raise ValueError('image must be a [1,H,W,3] tensor (the reference runs one image per call)')
    if not image.is_cuda:
        raise ops.L.OdetError('image must live on the GPU: tf_eager_object_detection_amd has no CPU path')
    return image.float().contiguous()


TRAINING_BATCH_MAX = ops.TARGETS_MAX_BATCH     # what one fused targets call produces


def check_training_batch(inputs, training_targets, training_losses):
    """the input rules of the batched training call -- (images [B,H,W,3], gt_bboxes [sum G,4], gt_labels [sum G], gt_offsets
    int [B+1]) -- as a pure function (CPU tensors pass it): ValueError naming the reason, else (images, gt_bboxes, gt_labels,
    the offsets as a list of B+1 Python ints: the call's one read of them)"""
    if training_targets != 'hip' or training_losses != 'hip':
        raise ValueError("the batched training call needs training_targets='hip' and training_losses='hip' (the batched stages "
                         "exist only fused), got training_targets=%r, training_losses=%r" % (training_targets, training_losses))
    if not isinstance(inputs, (tuple, list)) or len(inputs) != 4:
        raise ValueError('the batched training call takes (images, gt_bboxes, gt_labels, gt_offsets)')
    images, gt_bboxes, gt_labels, gt_offsets = inputs
    if not isinstance(images, torch.Tensor) or images.dim() != 4 or images.shape[3] != 3:
        raise ValueError('images must be a [B,H,W,3] tensor, got %s'
                         % (tuple(images.shape) if isinstance(images, torch.Tensor) else type(images).__name__,))
    B = int(images.shape[0])
    if not 1 <= B <= TRAINING_BATCH_MAX:
        raise ValueError('a training call takes 1 .. %d images, got %d' % (TRAINING_BATCH_MAX, B))
    if not isinstance(gt_bboxes, torch.Tensor) or gt_bboxes.dim() != 2 or gt_bboxes.shape[1] != 4:
        raise ValueError('gt_bboxes must be a [sum G,4] tensor (the images\' boxes packed in image order)')
    G = int(gt_bboxes.shape[0])
    if not isinstance(gt_labels, torch.Tensor) or gt_labels.numel() != G:
        raise ValueError('gt_labels must hold one label per box of gt_bboxes (%d)' % G)
    if isinstance(gt_offsets, torch.Tensor):
        if gt_offsets.dim() != 1 or gt_offsets.is_floating_point() or gt_offsets.is_complex() or gt_offsets.dtype == torch.bool:
            raise ValueError('gt_offsets must be a vector of B + 1 ints')
        off = gt_offsets.tolist()
    else:
        off = list(gt_offsets)
        if any(isinstance(v, bool) or not isinstance(v, int) for v in off):
            raise ValueError('gt_offsets must hold B + 1 ints')
    if len(off) != B + 1:
        raise ValueError('gt_offsets has %d entries for %d images (B + 1 wanted)' % (len(off), B))
    if off[0] != 0 or any(b < a for a, b in zip(off, off[1:])) or off[-1] != G:
        raise ValueError('gt_offsets must be non-decreasing from 0 to the number of boxes (%d), got %s' % (G, off))
    return images, gt_bboxes, gt_labels, off


class _Part(torch.nn.Module):
    """a dense part of a concrete model as a callable layer: `fn(x)` with keras' call signature"""

    def __init__(self, fn):
        super().__init__()
        self._fn = [fn]

    @torch.no_grad()
    def forward(self, inputs, training=None, mask=None):
        return self._fn[0](inputs)

    call = forward


class DenseRpnHead(torch.nn.Module):
    """the two families' RpnHead: the convolutions live in `dense` (a detector: rpn_conv, rpn_score, rpn_bbox), the outputs are
    reshaped to [-1, score width] / [-1, 4].  A family's class says how wide a score row is and how the detector takes the input."""

    def __init__(self, num_anchors, weight_decay=0.0001, dense=None):
        super().__init__()
        self._num_anchors = num_anchors
        self._dense = [dense]                    # (not a sub-module: the parameters belong to the model that owns `dense`)
        if dense is not None and dense.A != num_anchors:
            raise ValueError('RpnHead: %d anchors per cell but the dense part was built for %d' % (num_anchors, dense.A))

    def _score_width(self):
        raise NotImplementedError

    @staticmethod
    def _dense_input(inputs):
        return inputs

    def _rows(self, scores, deltas):
        return scores.reshape(-1, self._score_width()), deltas.reshape(-1, 4)

    @torch.no_grad()
    def forward(self, inputs, training=None, mask=None):
        return self._rows(*self._dense[0].rpn(self._dense_input(inputs)))

    call = forward


class CallerModel(torch.nn.Module):
    """The pass of a caller object, in the reference's order (model/fpn/base_fpn_model.py:202-276,
    model/faster_rcnn/base_faster_rcnn_model.py:126-198).  A family supplies:
      _rpn_layout, _rpn_head_type ops.RPN_LAYOUT_FPN / ops.RPN_LAYOUT_FRCNN; its RpnHead class
      _extractor_stride           what post_ops_prediction is told (FPN: 16)
      _dense_front                its dense parts and its anchor generation, each part through `run_part`
      _rpn_score_rows             the RPN scores as [N, 2] (bg, fg) rows for the 'torch' RPN loss
      _rois_for_head              RoIs -> (what `_pool_rois` takes, the head rows' target rows or None)
      _pool_rois                  how its pooling layer is called
      _start_training_call        per-call state of a training call (the single level's dropout image id)
      _batched_training, _training_batch   whether it has the batched training call (a four-tuple of inputs), and its pass (FPN)"""

    # What the training branches run with a backward pass.  BaseFPN sets these from its keywords; BaseFasterRcnn keeps the
    # reference's arguments, so its concrete models set them on the instance before they call its constructor.
    _train_extractor = False   # the extractor: its outputs require a gradient (FPN: needs the trainable neck; else a trainable head)
    _train_stem = False        # the FPN stem: conv1 receives a gradient too (needs the trainable extractor)
    _train_neck = False        # the neck: P2..P6 require a gradient (needs a trainable head)
    _train_rpn_head = False    # the RpnHead: the two RPN losses carry a graph into its layers
    _train_roi_head = False    # the RoI head: the two RoI losses carry a graph into its layers
    grad_form = 'exact'        # the arithmetic of the trainable parts' gradient GEMMs: 'exact' | 'x3' (ops.grad_form)
    _rpn_layout = None
    _rpn_head_type = None
    # The batched training call (a FOUR-tuple of inputs: check_training_batch).  A family that has it sets the flag and supplies
    # `_training_batch`; keep_training_pass=True leaves the call's tensors in `last_training_pass` (references, no copies).
    _batched_training = False
    _training_targets = None
    keep_training_pass = False
    last_training_pass = None

    def _init_shared_layers(self, a):
        """the layers and attributes both families build from the reference's constructor arguments (`a`: name -> value), at the
        point where the reference builds its RegionProposal; `_num_anchors` is set"""
        self._rpn_sigma, self._roi_sigma = a['rpn_sigma'], a['roi_sigma']
        self._roi_proposal_means, self._roi_proposal_stds = a['roi_proposal_means'], a['roi_proposal_stds']
        for name in ('max_objects_per_image', 'max_objects_per_class', 'nms_iou_threshold', 'score_threshold'):
            setattr(self, '_prediction_' + name, a['prediction_' + name])
        rpn_code = dict(target_means=a['rpn_proposal_means'], target_stds=a['rpn_proposal_stds'])
        pick = lambda prefix, *names: {n: a[prefix + n] for n in names}
        self._rpn_proposal = RegionProposal(
            num_anchors=self._num_anchors, **rpn_code,
            **pick('rpn_proposal_', 'num_pre_nms_train', 'num_post_nms_train', 'num_pre_nms_test', 'num_post_nms_test',
                   'nms_iou_threshold'))
        sampling = ('pos_iou_threshold', 'neg_iou_threshold', 'total_num_samples', 'max_pos_samples')
        # training_targets: 'torch' = AnchorTarget / ProposalTarget (generator-driven sampling), 'hip' = the fused stage
        self._training_targets = a['training_targets']
        self._anchor_target, self._proposal_target = training_target_layers(
            a['training_targets'], dict(pick('rpn_training_', *sampling), **rpn_code),
            dict(pick('roi_training_', *sampling), num_classes=a['num_classes'], target_means=a['roi_proposal_means'],
                 target_stds=a['roi_proposal_stds']))

    def _get_roi_head(self):
        raise NotImplementedError

    def _get_extractor(self):
        raise NotImplementedError

    def _get_rpn_head(self, weight_decay):
        return self._rpn_head_type(num_anchors=self._num_anchors, weight_decay=weight_decay, dense=self.__dict__.get('_dense_ref'))

    def _get_trainable_extractor_results(self, image):
        """_extractor with a graph into its trainable layers, bit-equal to it"""
        raise NotImplementedError('train_extractor=True needs a dense part with a trainable extractor')

    def _get_trainable_rpn_head_results(self, maps):
        """the RpnHead on all of `maps` with a graph into its layers: (scores, boxes) in the family's rows, bit-equal to it"""
        raise NotImplementedError('train_rpn_head=True needs a dense part with a trainable RPN head')

    def _get_trainable_roi_head(self):
        """_roi_head with a graph into the RoI head's layers, as a callable on the RoI features"""
        raise NotImplementedError('train_roi_head=True needs a dense part with a trainable RoI head')

    def _start_training_call(self):
        pass

    def _fg_scores(self, rpn_score):
        """tf.nn.softmax(all_fpn_scores)[:, 1] (base_fpn_model.py:223) / the reshape, transpose, softmax, transpose, slice of the
        [A bg | A fg] layout (base_faster_rcnn_model.py:147-151) -- the HIP kernel, bit-identical to the fused proposal stage"""
        return ops.rpn_fg_softmax(rpn_score, self._num_anchors, self._rpn_layout)

    def _anchors_and_proposals(self, image, training, trainable=True):
        """the front of every entry (base_fpn_model.py:208-224, base_faster_rcnn_model.py:130-153 / :279-300): the family's dense
        parts and anchors -> fg scores -> RegionProposal.  In a training call a part whose train flag is set takes its trainable
        form in the caller's grad mode (`trainable=False`: no part does -- BaseFPN.predict_rois); every other part runs under
        no_grad, and anchors, softmax and proposals see detached values."""
        image_shape = [int(image.shape[1]), int(image.shape[2])]
        features, anchors, rpn_score, rpn_bbox_txtytwth = self._dense_front(image, image_shape, training,
                                                                            bool(training) and trainable)
        with torch.no_grad():
            scores = self._fg_scores(rpn_score.detach())
            rois = self._rpn_proposal((rpn_bbox_txtytwth.detach(), anchors, scores, image_shape), training=training)
        return image_shape, features, anchors, rpn_score, rpn_bbox_txtytwth, rois

    # ---- base_fpn_model.py:202-276, base_faster_rcnn_model.py:126-198 ----------------------------------------------------------
    @caller_range_checked
    def forward(self, inputs, training=None, mask=None):
        # (the trainable parts record the form on their graph nodes: `.backward()` may run anywhere, ops.keep_grad_form)
        with ops.grad_form(self.grad_form):
            return self._forward(inputs, training)

    def _forward(self, inputs, training):
        if training and isinstance(inputs, (tuple, list)) and len(inputs) == 4:
            return self._forward_images(inputs)
        if training:
            image, gt_bboxes, gt_labels = inputs
        else:
            image = inputs
        image = _image_nhwc(image)
        if training:
            self._start_training_call()
        image_shape, features, anchors, rpn_score, rpn_bbox_txtytwth, rois = self._anchors_and_proposals(image, training)
        if training:
            losses = self._fused_losses if self._training_losses == 'hip' else self._torch_losses
            return losses(rpn_score, rpn_bbox_txtytwth, anchors, rois, gt_bboxes, gt_labels, features, image_shape, training)
        with torch.no_grad():
            head_rois, row_map = self._rois_for_head(rois)
            roi_features = self._pool_rois(head_rois, features, image_shape, training)
            roi_score, roi_bboxes_txtytwth = self._roi_head(roi_features, training=training)
            roi_score_softmax = torch.softmax(roi_score.float(), dim=-1)
            roi_bboxes_txtytwth = roi_bboxes_txtytwth.float().reshape(-1, self.num_classes, 4)
            final_rois = rois if row_map is None else torch.cat(head_rois, dim=0)
            return post_ops_prediction(roi_score_softmax, roi_bboxes_txtytwth, final_rois, image_shape,
                                       self._roi_proposal_means, self._roi_proposal_stds,
                                       max_num_per_class=self._prediction_max_objects_per_class,
                                       max_num_per_image=self._prediction_max_objects_per_image,
                                       nms_iou_threshold=self._prediction_nms_iou_threshold,
                                       score_threshold=self._prediction_score_threshold,
                                       extractor_stride=self._extractor_stride, num_classes=self.num_classes)

    call = forward

    def _forward_images(self, inputs):
        """the batched training call: (images [B,H,W,3], gt_bboxes [sum G,4], gt_labels [sum G], gt_offsets int [B+1]) -> four
        float32 [B] tensors (rpn_cls, rpn_reg, roi_cls, roi_reg per image).  Every refusal comes before any state changes."""
        if not self._batched_training:
            raise ValueError('%s: the batched training call (a four-tuple of inputs) is built for the FPN family only -- a '
                             'single-level model needs one dropout image id per image of the batch, which is a change of its '
                             'own; call it with (image, gt_bboxes, gt_labels) per image' % type(self).__name__)
        images, gt_bboxes, gt_labels, off = check_training_batch(inputs, self._training_targets, self._training_losses)
        if not images.is_cuda:
            raise ops.L.OdetError('images must live on the GPU: tf_eager_object_detection_amd has no CPU path')
        gt_offsets = inputs[3]
        if not (isinstance(gt_offsets, torch.Tensor) and gt_offsets.is_cuda and gt_offsets.dtype == torch.int32):
            gt_offsets = torch.tensor(off, dtype=torch.int32, device=images.device)
        return self._training_batch(images.float().contiguous(), gt_bboxes, gt_labels, gt_offsets.contiguous())

    def _training_batch(self, images, gt_bboxes, gt_labels, gt_offsets):
        raise NotImplementedError

    def _torch_losses(self, rpn_score, rpn_bbox_txtytwth, anchors, rois, gt_bboxes, gt_labels, maps, image_shape, training):
        """training_losses='torch' (base_fpn_model.py:232-264, base_faster_rcnn_model.py:155-185): the target layers' dense outputs
        through model/losses.py"""
        rpn_labels, rpn_bbox_targets, rpn_in_weights, rpn_out_weights = self._anchor_target(
            (gt_bboxes, image_shape, anchors), training)
        rpn_cls_loss, rpn_reg_loss = self._get_rpn_loss(rpn_score, rpn_bbox_txtytwth, rpn_labels, rpn_bbox_targets,
                                                        rpn_in_weights, rpn_out_weights)
        final_rois, *roi_targets = self._proposal_target((rois, gt_bboxes, gt_labels), training)
        head_rois, row_map = self._rois_for_head(final_rois)
        roi_score, roi_bboxes_txtytwth = self._training_roi_head(head_rois, maps, image_shape, training)
        if row_map is not None:
            roi_targets = [t[row_map] for t in roi_targets]       # labels, box targets, inside and outside weights in head order
        roi_cls_loss, roi_reg_loss = self._get_roi_loss(roi_score, roi_bboxes_txtytwth, *roi_targets)
        return rpn_cls_loss, rpn_reg_loss, roi_cls_loss, roi_reg_loss

    def _fused_losses(self, rpn_score, rpn_bbox_txtytwth, anchors, rois, gt_bboxes, gt_labels, maps, image_shape, training):
        """training_losses='hip': the same four scalars from the compact targets, the scores read in the family's own layout (no
        re-layout, no dense [N,4] target, no nonzero); the image ids advance as the target layers' own single-image calls advance
        them, so both settings draw the same samples"""
        off = torch.tensor([0, gt_bboxes.shape[0]], dtype=torch.int32, device=anchors.device)
        at, pt = self._anchor_target, self._proposal_target
        anchor_targets = at.batch(gt_bboxes, off, image_shape, anchors, first_image_id=at._next_image_id, dense=False)
        at._next_image_id += 1
        rpn_cls_loss, rpn_reg_loss = fused_rpn_losses(rpn_score.float()[None], rpn_bbox_txtytwth.float()[None],
                                                      anchor_targets, self._rpn_sigma, self._rpn_layout, self._num_anchors)
        # strict=False: no host read.  An image that wants background rows and has no candidate does not raise here as it does on
        # the 'torch' path: it has rows written < S, and the loss kernel gives the unwritten rows no weight and zero gradient.
        proposal_targets = pt.batch(rois.reshape(1, -1, 4), gt_bboxes, gt_labels, off, first_image_id=pt._next_image_id,
                                    strict=False)
        pt._next_image_id += 1
        head_rois, row_map = self._rois_for_head(proposal_targets.final_rois[0])
        roi_score, roi_bboxes_txtytwth = self._training_roi_head(head_rois, maps, image_shape, training)
        roi_cls_loss, roi_reg_loss = fused_roi_losses(roi_score.float()[None], roi_bboxes_txtytwth.float()[None],
                                                      proposal_targets, self._roi_sigma,
                                                      row_map=None if row_map is None else row_map[None])
        return rpn_cls_loss[0], rpn_reg_loss[0], roi_cls_loss[0], roi_reg_loss[0]

    def _training_roi_head(self, rois, maps, image_shape, training):
        """pooling + RoI head of both training branches: under no_grad, unless train_roi_head -- then the head runs its trainable
        form outside it, so the two RoI losses carry a graph.  The pooling stays under no_grad as long as no map requires a
        gradient (the models' own maps do with train_neck / the single level's train_extractor); when one does, the pooling layer
        takes its trainable form, the head's first layer receives an input that requires a gradient and computes its input
        gradient, and odet_roi_pool_backward carries it into the maps."""
        map_list = maps if isinstance(maps, (list, tuple)) else (maps,)
        if self._train_roi_head and any(isinstance(p, torch.Tensor) and p.requires_grad for p in map_list):
            return self._get_trainable_roi_head()(self._pool_rois(rois, maps, image_shape, training))
        with torch.no_grad():
            roi_features = self._pool_rois(rois, maps, image_shape, training)
            if not self._train_roi_head:
                return self._roi_head(roi_features, training=training)
        return self._get_trainable_roi_head()(roi_features)

    def _rpn_score_rows(self, rpn_score):
        return rpn_score

    def _rois_for_head(self, rois):
        return rois, None

    def _get_rpn_loss(self, rpn_score, rpn_bbox_txtytwth, anchor_target_labels, anchor_target_bboxes_txtytwth,
                      anchor_target_in_weights, anchor_target_out_weights):
        """base_fpn_model.py:278-289, base_faster_rcnn_model.py:200-215"""
        rpn_score = self._rpn_score_rows(rpn_score)
        rpn_selected = torch.nonzero(anchor_target_labels >= 0)[:, 0]                               # :282
        rpn_cls_loss = cls_loss(logits=rpn_score[rpn_selected], labels=anchor_target_labels[rpn_selected])
        rpn_reg_loss = smooth_l1_loss(rpn_bbox_txtytwth, anchor_target_bboxes_txtytwth, anchor_target_in_weights,
                                      anchor_target_out_weights, self._rpn_sigma, dim=[0, 1])
        return rpn_cls_loss, rpn_reg_loss

    def _get_roi_loss(self, roi_score, roi_bbox_txtytwth, proposal_target_labels, proposal_target_bboxes_txtytwth,
                      proposal_target_in_weights, proposal_target_out_weights):
        roi_cls_loss = cls_loss(logits=roi_score, labels=proposal_target_labels)
        roi_reg_loss = smooth_l1_loss(roi_bbox_txtytwth, proposal_target_bboxes_txtytwth, proposal_target_in_weights,
                                      proposal_target_out_weights, sigma=self._roi_sigma)
        return roi_cls_loss, roi_reg_loss

    @caller_range_checked
    @torch.no_grad()
    def im_detect(self, preprocessed_img, img_scale):
        """base_fpn_model.py:364-390, base_faster_rcnn_model.py:279-306: (softmax scores, raw box regressions, the RoIs in the
        head's row order -- FPN: level-sorted -- divided by the scale)"""
        image = _image_nhwc(preprocessed_img)
        image_shape, features, _, _, _, rois = self._anchors_and_proposals(image, False)
        head_rois, row_map = self._rois_for_head(rois)
        roi_features = self._pool_rois(head_rois, features, image_shape, False)
        roi_score, roi_bboxes_txtytwth = self._roi_head(roi_features, training=False)
        new_rois = rois if row_map is None else torch.cat(head_rois, dim=0)
        div = torch.full((1,), float(img_scale), dtype=torch.float32, device=new_rois.device)     # (a true float32 division)
        return torch.softmax(roi_score.float(), dim=-1), roi_bboxes_txtytwth.float(), new_rois / div


class DenseParts:
    """mixin of the concrete models: the dense parts are a detector (model/fpn_detector.py's ResNetFpnDetector or a
    SingleLevelDetector of model/frcnn_detector.py; their layers: model/layers.py), owned as `dense` and reachable as `_dense_ref`
    before the base constructor asks for the layers"""

    def _init_with_dense(self, dense, dtype, device, base_init, kw):
        torch.nn.Module.__init__(self)             # (the dense part must exist before the base constructor asks for the layers)
        dense.to(device=device, dtype=dtype, memory_format=torch.channels_last).eval()
        self.__dict__['_dense_ref'] = dense
        base_init(self, **kw)
        self.dense = dense

    def _get_roi_head(self):
        return _Part(self._dense_ref.roi_head)

    def _get_trainable_extractor_results(self, image):
        return self._dense_ref.extractor_trainable(image)

    def _get_trainable_rpn_head_results(self, maps):
        return self._rpn_head._rows(*self._dense_ref.rpn_trainable(maps))

    def _get_trainable_roi_head(self):
        return self._dense_ref.roi_head_trainable
