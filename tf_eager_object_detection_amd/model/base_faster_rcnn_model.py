"""BaseFasterRcnn / RpnHead / ResNetFasterRcnn (TrainableResNetFasterRcnn) / Vgg16FasterRcnn -- counterparts of the
reference's model/faster_rcnn/base_faster_rcnn_model.py (BaseFasterRcnn :16-306, RpnHead :309-350), resnet_faster_rcnn.py
(ResNetFasterRcnn :188-293) and vgg16_faster_rcnn.py (Vgg16FasterRcnn :11-115): the CALLER objects of the single-level hot
path, with the reference's constructor arguments, `call(inputs, training=None, mask=None)` and `im_detect`.

`call` composes the reference-named layers in the reference's order (:126-198): `_extractor` -> `_anchor_generator`
(generate_by_anchor_base_tf) -> `_rpn_head` -> the [A bg | A fg] score re-layout + softmax -> `_rpn_proposal` ->
`_roi_pooling` (RoiPoolingCropAndResize) -> `_roi_head` -> softmax -> post_ops_prediction, with dynamic shapes and one image
per call as in the reference.  The static-shape, sync-free arrangement for throughput is model/frcnn_detector.py.

The training branches run every dense part under no_grad unless a keyword switches its backward pass on (Vgg16FasterRcnn,
TrainableResNetFasterRcnn; float32, f32_form 'exact'): `train_roi_head` runs the RoI head's trainable form -- VGG16's with the
reference's two dropouts -- (the two RoI losses carry a graph into fc1, fc2, score and bbox / into the conv5 stack, score and
bbox), `train_rpn_head` the RpnHead's (the two RPN losses carry a graph into rpn_conv, rpn_score and rpn_bbox), `train_extractor`
(with at least one of the two) the extractor's: the shared map requires a gradient, which the RpnHead's input gradient and the
trainable RoI pooling deliver, and the losses carry a graph into block3_conv1 .. block5_conv3 / into conv3 and conv4."""
import contextlib
import math

import torch

from .. import ops
from ..utils.anchor_generator import generate_anchor_base, generate_by_anchor_base_tf
from .fpn_detector import caller_range_checked
from .base_fpn_model import _Part, _image_nhwc, check_training_losses
from .detector_base import check_caller_f32_form
from .losses import cls_loss, fused_roi_losses, fused_rpn_losses, smooth_l1_loss
from .prediction import post_ops_prediction
from .proposal_target import training_target_layers
from .region_proposal import RegionProposal
from .roi_pooling import RoiPoolingCropAndResize
from .trainable_common import check_train_flags

__all__ = ['BaseFasterRcnn', 'RpnHead', 'ResNetFasterRcnn', 'TrainableResNetFasterRcnn', 'Vgg16FasterRcnn']


class RpnHead(torch.nn.Module):
    """reference base_faster_rcnn_model.py:309-350: scores reshaped to [-1, 2A] ([A bg | A fg] per cell), boxes to [-1, 4];
    the convolutions live in `dense` (a detector of model/frcnn_detector.py)."""

    def __init__(self, num_anchors, weight_decay=0.0001, dense=None):
        super().__init__()
        self._num_anchors = num_anchors
        self._dense = [dense]
        if dense is not None and dense.A != num_anchors:
            raise ValueError('RpnHead: %d anchors per cell but the dense part was built for %d' % (num_anchors, dense.A))

    @torch.no_grad()
    def forward(self, inputs, training=None, mask=None):
        scores, deltas = self._dense[0].rpn(inputs)
        return scores.reshape(-1, 2 * self._num_anchors), deltas.reshape(-1, 4)

    call = forward


class BaseFasterRcnn(torch.nn.Module):
    """reference base_faster_rcnn_model.py:16-118 (same constructor arguments, same private attribute names)."""

    # What the training branches run with a backward pass.  The constructor keeps the reference's arguments, so a concrete model
    # with trainable dense parts (Vgg16FasterRcnn) sets these on the instance before it calls it.
    _train_extractor = False   # the extractor: the shared map requires a gradient (needs a trainable head)
    _train_roi_head = False    # the RoI head: the two RoI losses carry a graph into its layers
    _train_rpn_head = False    # the RpnHead: the two RPN losses carry a graph into its layers

    def __init__(self, num_classes, weight_decay, ratios, scales, extractor_stride, rpn_proposal_means, rpn_proposal_stds,
                 rpn_proposal_num_pre_nms_train, rpn_proposal_num_post_nms_train, rpn_proposal_num_pre_nms_test,
                 rpn_proposal_num_post_nms_test, rpn_proposal_nms_iou_threshold, rpn_sigma,
                 rpn_training_pos_iou_threshold, rpn_training_neg_iou_threshold, rpn_training_total_num_samples,
                 rpn_training_max_pos_samples, roi_proposal_means, roi_proposal_stds, roi_pool_size,
                 roi_pooling_max_pooling_flag, roi_sigma, roi_training_pos_iou_threshold, roi_training_neg_iou_threshold,
                 roi_training_total_num_samples, roi_training_max_pos_samples, prediction_max_objects_per_image,
                 prediction_max_objects_per_class, prediction_nms_iou_threshold, prediction_score_threshold,
                 training_targets='torch', training_losses='torch'):
        super().__init__()
        self._training_losses = check_training_losses(training_losses, training_targets)
        check_train_extractor(self._train_extractor, self._train_rpn_head, self._train_roi_head)
        # the image id of the RoI head's dropout masks: advances once per training call, whatever the target stage does
        self._next_dropout_image_id = 0
        self._dropout_image_id = 0
        self.num_classes = num_classes
        self.weight_decay = weight_decay
        self._ratios = ratios
        self._scales = scales
        self._num_anchors = len(ratios) * len(scales)
        self._extractor_stride = extractor_stride
        self._rpn_sigma = rpn_sigma
        self._roi_sigma = roi_sigma
        self._roi_proposal_means = roi_proposal_means
        self._roi_proposal_stds = roi_proposal_stds
        self._prediction_max_objects_per_image = prediction_max_objects_per_image
        self._prediction_max_objects_per_class = prediction_max_objects_per_class
        self._prediction_nms_iou_threshold = prediction_nms_iou_threshold
        self._prediction_score_threshold = prediction_score_threshold
        self._anchor_generator = generate_by_anchor_base_tf
        self._anchor_base = generate_anchor_base(extractor_stride, ratios, scales).astype('float32')      # :84 tf.to_float
        self._rpn_head = self._get_rpn_head(weight_decay)
        self._rpn_proposal = RegionProposal(
            num_anchors=self._num_anchors, num_pre_nms_train=rpn_proposal_num_pre_nms_train,
            num_post_nms_train=rpn_proposal_num_post_nms_train, num_pre_nms_test=rpn_proposal_num_pre_nms_test,
            num_post_nms_test=rpn_proposal_num_post_nms_test, nms_iou_threshold=rpn_proposal_nms_iou_threshold,
            target_means=rpn_proposal_means, target_stds=rpn_proposal_stds)
        self._roi_pooling = RoiPoolingCropAndResize(pool_size=roi_pool_size, max_pooling_flag=roi_pooling_max_pooling_flag,
                                                    trainable=self._train_roi_head)
        # training_targets: 'torch' = AnchorTarget / ProposalTarget (generator-driven sampling), 'hip' = the fused stage
        self._anchor_target, self._proposal_target = training_target_layers(
            training_targets,
            dict(pos_iou_threshold=rpn_training_pos_iou_threshold, neg_iou_threshold=rpn_training_neg_iou_threshold,
                 total_num_samples=rpn_training_total_num_samples, max_pos_samples=rpn_training_max_pos_samples,
                 target_means=rpn_proposal_means, target_stds=rpn_proposal_stds),
            dict(num_classes=num_classes, pos_iou_threshold=roi_training_pos_iou_threshold,
                 neg_iou_threshold=roi_training_neg_iou_threshold, total_num_samples=roi_training_total_num_samples,
                 max_pos_samples=roi_training_max_pos_samples, target_means=roi_proposal_means,
                 target_stds=roi_proposal_stds))
        self._extractor = self._get_extractor()
        self._roi_head = self._get_roi_head()

    def _get_roi_head(self):
        raise NotImplementedError

    def _get_extractor(self):
        raise NotImplementedError

    def _get_rpn_head(self, weight_decay):
        return RpnHead(num_anchors=self._num_anchors, weight_decay=weight_decay)

    def _trains_front(self, training):
        """the call records a graph through the extractor or the RpnHead"""
        return bool(training) and (self._train_extractor or self._train_rpn_head)

    def _anchors_and_proposals(self, image, training):
        """:130-153 / :279-300: extractor -> anchors -> RpnHead -> fg scores -> RegionProposal.  The layers themselves run under
        no_grad; in a training call the extractor and the RpnHead take their trainable forms where the keywords ask for them, and
        anchors, softmax and proposals see detached values"""
        image_shape = [int(image.shape[1]), int(image.shape[2])]
        if training and self._train_extractor:
            shared_features = self._get_trainable_extractor_results(image)
        else:
            shared_features = self._extractor(image, training=training)
        anchors = self._anchor_generator(self._anchor_base, self._extractor_stride,
                                         int(math.ceil(image_shape[0] / self._extractor_stride)),
                                         int(math.ceil(image_shape[1] / self._extractor_stride)))
        if training and self._train_rpn_head:
            rpn_score, rpn_bbox_txtytwth = self._get_trainable_rpn_head_results(shared_features)
        else:
            rpn_score, rpn_bbox_txtytwth = self._rpn_head(shared_features, training=training)
        with torch.no_grad():
            # :147-151 (reshape / transpose / softmax / transpose / slice): the fg probabilities of the [A bg | A fg] layout
            scores = ops.rpn_fg_softmax(rpn_score.detach(), self._num_anchors, ops.RPN_LAYOUT_FRCNN)
            rois = self._rpn_proposal((rpn_bbox_txtytwth.detach(), anchors, scores, image_shape), training=training)
        return image_shape, shared_features, anchors, rpn_score, rpn_bbox_txtytwth, rois

    def _get_trainable_extractor_results(self, image):
        """_extractor with a graph into its trainable layers, bit-equal to it"""
        raise NotImplementedError('train_extractor=True needs a dense part with a trainable extractor')

    def _get_trainable_rpn_head_results(self, shared_features):
        """_rpn_head with a graph into the RpnHead's layers: ([-1, 2A], [-1, 4]), bit-equal to it"""
        raise NotImplementedError('train_rpn_head=True needs a dense part with a trainable RPN head')

    def _get_trainable_roi_head(self):
        """_roi_head with a graph into the RoI head's layers, as a callable on the RoI features"""
        raise NotImplementedError('train_roi_head=True needs a dense part with a trainable RoI head')

    def _training_roi_head(self, shared_features, rois, training):
        """pooling + RoI head of both training branches: under no_grad, unless train_roi_head -- then the head runs its trainable
        form outside it, so the two RoI losses carry a graph.  The pooling stays under no_grad as long as the shared map requires
        no gradient (it does with train_extractor); when it does, the pooling layer takes its trainable form, the head's first
        layer computes its input gradient and odet_roi_pool_backward carries it into the map."""
        inputs = (shared_features, rois, self._extractor_stride)
        if self._train_roi_head and shared_features.requires_grad:
            return self._get_trainable_roi_head()(self._roi_pooling(inputs, training=training))
        with torch.no_grad():
            roi_features = self._roi_pooling(inputs, training=training)
            if not self._train_roi_head:
                return self._roi_head(roi_features, training=training)
        return self._get_trainable_roi_head()(roi_features)

    @caller_range_checked
    def forward(self, inputs, training=None, mask=None):
        if training:
            image, gt_bboxes, gt_labels = inputs
        else:
            image = inputs
        image = _image_nhwc(image)
        if training:
            self._dropout_image_id = self._next_dropout_image_id
            self._next_dropout_image_id += 1
        # (no_grad around the whole front unless this call records a graph through the extractor or the RpnHead)
        with contextlib.nullcontext() if self._trains_front(training) else torch.no_grad():
            image_shape, shared_features, anchors, rpn_score, rpn_bbox_txtytwth, rois = \
                self._anchors_and_proposals(image, training)
        if training and self._training_losses == 'hip':
            return self._fused_losses(rpn_score, rpn_bbox_txtytwth, anchors, rois, gt_bboxes, gt_labels, shared_features,
                                      image_shape, training)
        if training:
            rpn_labels, rpn_bbox_targets, rpn_in_weights, rpn_out_weights = self._anchor_target(
                (gt_bboxes, image_shape, anchors), training)
            rpn_cls_loss, rpn_reg_loss = self._get_rpn_loss(rpn_score, rpn_bbox_txtytwth, rpn_labels, rpn_bbox_targets,
                                                            rpn_in_weights, rpn_out_weights)
            final_rois, roi_labels, roi_bbox_target, roi_in_weights, roi_out_weights = self._proposal_target(
                (rois, gt_bboxes, gt_labels), training)
            roi_score, roi_bboxes_txtytwth = self._training_roi_head(shared_features, final_rois, training)
            roi_cls_loss, roi_reg_loss = self._get_roi_loss(roi_score, roi_bboxes_txtytwth, roi_labels, roi_bbox_target,
                                                            roi_in_weights, roi_out_weights)
            return rpn_cls_loss, rpn_reg_loss, roi_cls_loss, roi_reg_loss
        with torch.no_grad():
            roi_features = self._roi_pooling((shared_features, rois, self._extractor_stride), training=training)
            roi_score, roi_bboxes_txtytwth = self._roi_head(roi_features, training=training)
            roi_score_softmax = torch.softmax(roi_score.float(), dim=-1)
            roi_bboxes_txtytwth = roi_bboxes_txtytwth.float().reshape(-1, self.num_classes, 4)
            return post_ops_prediction(roi_score_softmax, roi_bboxes_txtytwth, rois, image_shape,
                                       self._roi_proposal_means, self._roi_proposal_stds,
                                       max_num_per_class=self._prediction_max_objects_per_class,
                                       max_num_per_image=self._prediction_max_objects_per_image,
                                       nms_iou_threshold=self._prediction_nms_iou_threshold,
                                       score_threshold=self._prediction_score_threshold,
                                       extractor_stride=self._extractor_stride, num_classes=self.num_classes)

    call = forward

    def _fused_losses(self, rpn_score, rpn_bbox_txtytwth, anchors, rois, gt_bboxes, gt_labels, shared_features, image_shape,
                      training):
        """training_losses='hip': the same four scalars from the compact targets, the scores read in their own
        [A bg | A fg] layout (no re-layout, no dense [N,4] target, no nonzero); image ids advance as in the layers' calls"""
        off = torch.tensor([0, gt_bboxes.shape[0]], dtype=torch.int32, device=anchors.device)
        at, pt = self._anchor_target, self._proposal_target
        anchor_targets = at.batch(gt_bboxes, off, image_shape, anchors, first_image_id=at._next_image_id, dense=False)
        at._next_image_id += 1
        rpn_cls_loss, rpn_reg_loss = fused_rpn_losses(rpn_score.float()[None], rpn_bbox_txtytwth.float()[None],
                                                      anchor_targets, self._rpn_sigma, ops.RPN_LAYOUT_FRCNN, self._num_anchors)
        # strict=False: no host read.  An image that wants background rows and has no candidate does not raise here as it does on
        # the 'torch' path: it has rows written < S, and the loss kernel gives the unwritten rows no weight and zero gradient.
        proposal_targets = pt.batch(rois.reshape(1, -1, 4), gt_bboxes, gt_labels, off, first_image_id=pt._next_image_id,
                                    strict=False)
        pt._next_image_id += 1
        roi_score, roi_bboxes_txtytwth = self._training_roi_head(shared_features, proposal_targets.final_rois[0], training)
        roi_cls_loss, roi_reg_loss = fused_roi_losses(roi_score.float()[None], roi_bboxes_txtytwth.float()[None],
                                                      proposal_targets, self._roi_sigma)
        return rpn_cls_loss[0], rpn_reg_loss[0], roi_cls_loss[0], roi_reg_loss[0]

    def _get_rpn_loss(self, rpn_score, rpn_bbox_txtytwth, anchor_target_labels, anchor_target_bboxes_txtytwth,
                      anchor_target_in_weights, anchor_target_out_weights):
        """:200-215: the [A bg | A fg] scores re-laid as [N, 2] rows before the selection"""
        rpn_score = rpn_score.reshape(-1, 2, self._num_anchors).permute(0, 2, 1).reshape(-1, 2)
        rpn_selected = torch.nonzero(anchor_target_labels >= 0)[:, 0]
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

    def predict_rpn(self, image, gt_bboxes):
        """:226-241 (a debugging helper): the anchors AnchorTarget labels positive for `gt_bboxes`.  The reference's body is
        stale against its own AnchorTarget (it passes (anchors, gt_bboxes, image_shape) and unpacks an index list and a count,
        model/anchor_target.py:37-107 takes (gt_bboxes, image_shape, anchors) and returns labels); this is its intent, written
        like BaseFPN.predict_rpns (model/fpn/base_fpn_model.py:326-340)."""
        image = _image_nhwc(image)
        image_shape = [int(image.shape[1]), int(image.shape[2])]
        anchors = self._anchor_generator(self._anchor_base, self._extractor_stride,
                                         int(math.ceil(image_shape[0] / self._extractor_stride)),
                                         int(math.ceil(image_shape[1] / self._extractor_stride)))
        rpn_labels, _, _, _ = self._anchor_target((gt_bboxes, image_shape, anchors), True)
        return anchors[torch.nonzero(rpn_labels > 0)[:, 0]]

    @torch.no_grad()
    def predict_roi(self, image, gt_bboxes, gt_labels):
        """:243-266: (final_rois, final_labels, final_bbox_targets, bbox_inside_weights, bbox_outside_weights) of the
        training-mode proposals"""
        image = _image_nhwc(image)
        rois = self._anchors_and_proposals(image, True)[5]
        return self._proposal_target((rois, gt_bboxes, gt_labels), True)

    @caller_range_checked
    @torch.no_grad()
    def im_detect(self, preprocessed_image, img_scale):
        """:279-306"""
        image = _image_nhwc(preprocessed_image)
        _, shared_features, _, _, _, rois = self._anchors_and_proposals(image, False)
        roi_features = self._roi_pooling((shared_features, rois, self._extractor_stride), training=False)
        roi_score, roi_bboxes_txtytwth = self._roi_head(roi_features, training=False)
        div = torch.full((1,), float(img_scale), dtype=torch.float32, device=rois.device)
        return torch.softmax(roi_score.float(), dim=-1), roi_bboxes_txtytwth.float(), rois / div


def check_train_extractor(train_extractor, train_rpn_head, train_roi_head):
    """train_extractor needs a trainable head: the shared map receives a gradient only through the RpnHead's input gradient or the
    trainable RoI pooling"""
    if train_extractor and not (train_rpn_head or train_roi_head):
        raise ValueError('train_extractor=True needs train_rpn_head=True or train_roi_head=True: no gradient reaches the extractor '
                         'otherwise')
    return bool(train_extractor)


def _features_nhwc(dense):
    """the detector's extractor output as the NHWC map RoiPoolingCropAndResize / RpnHead take"""
    def fn(image):
        return dense.features(image)
    return fn


class _FrcnnFromDense(BaseFasterRcnn):
    """shared plumbing of the two concrete models: the dense parts are a detector of model/frcnn_detector.py (`dense`)"""

    def _init_with_dense(self, dense, dtype, device, kw):
        torch.nn.Module.__init__(self)
        dense.to(device=device, dtype=dtype, memory_format=torch.channels_last).eval()
        self.__dict__['_dense_ref'] = dense
        BaseFasterRcnn.__init__(self, **kw)
        self.dense = dense

    def _get_extractor(self):
        return _Part(self._dense_ref.features)

    def _get_roi_head(self):
        return _Part(self._dense_ref.roi_head)

    def _get_rpn_head(self, weight_decay):
        return RpnHead(num_anchors=self._num_anchors, weight_decay=weight_decay, dense=self._dense_ref)

    def _anchors_and_proposals(self, image, training):
        out = list(super()._anchors_and_proposals(image, training))
        # the detectors keep maps channels_last [B,C,H,W]; the pooling layer takes the NHWC view of the same memory
        feat = out[1].permute(0, 2, 3, 1)
        out[1] = feat if feat.is_contiguous() else feat.contiguous()
        return tuple(out)

    def _get_trainable_extractor_results(self, image):
        return self._dense_ref.extractor_trainable(image)

    def _get_trainable_rpn_head_results(self, shared_features):
        scores, deltas = self._dense_ref.rpn_trainable(shared_features)
        return scores.reshape(-1, 2 * self._num_anchors), deltas.reshape(-1, 4)


_COMMON = dict(num_classes=21, weight_decay=0.0001, ratios=(0.5, 1.0, 2.0), scales=(8, 16, 32), extractor_stride=16,
               rpn_proposal_means=(0, 0, 0, 0), rpn_proposal_stds=(1.0, 1.0, 1.0, 1.0),
               rpn_proposal_num_pre_nms_train=12000, rpn_proposal_num_post_nms_train=2000,
               rpn_proposal_num_pre_nms_test=6000, rpn_proposal_num_post_nms_test=300, rpn_proposal_nms_iou_threshold=0.7,
               rpn_sigma=3.0, rpn_training_pos_iou_threshold=0.7, rpn_training_neg_iou_threshold=0.3,
               rpn_training_total_num_samples=256, rpn_training_max_pos_samples=128, roi_proposal_means=(0, 0, 0, 0),
               roi_proposal_stds=(0.1, 0.1, 0.2, 0.2), roi_pool_size=7, roi_pooling_max_pooling_flag=True, roi_sigma=1,
               roi_training_pos_iou_threshold=0.5, roi_training_neg_iou_threshold=0.1, roi_training_total_num_samples=128,
               roi_training_max_pos_samples=32, prediction_max_objects_per_image=50, prediction_max_objects_per_class=50,
               prediction_nms_iou_threshold=0.3, prediction_score_threshold=0.3, training_targets='torch',
               training_losses='torch')
_TRAIN_KEYWORDS = ('train_roi_head', 'train_rpn_head', 'train_extractor', 'dropout_seed')


class ResNetFasterRcnn(_FrcnnFromDense):
    """reference resnet_faster_rcnn.py:188-293: ResNet-{50,101,152} C4 extractor, RoI head = conv5 stack + global average
    pooling + score / box layers.  Keyword arguments and defaults as there (`_COMMON`; model_factory.py:117 passes
    roi_pooling_max_pooling_flag=False from the config).  This class refuses the train_* keywords; TrainableResNetFasterRcnn,
    the same constructor body, takes them."""

    _accepts_train_keywords = False

    def __init__(self, depth=50, roi_feature_size=(7, 7, 1024), dtype=torch.float32, device='cuda', f32_form='exact', **kwargs):
        from .frcnn_detector import ResNetC4Detector
        check_caller_f32_form(f32_form)
        if depth not in [50, 101, 152]:
            raise ValueError('unknown resnet layers number {}'.format(depth))
        if self._accepts_train_keywords:
            self._take_train_keywords(kwargs, dtype, f32_form)
        else:
            asked = sorted(k for k in _TRAIN_KEYWORDS if k in kwargs)
            if asked:
                raise NotImplementedError('ResNetFasterRcnn: %s: this class takes no training keywords (existing callers rely on '
                                          'the refusal); TrainableResNetFasterRcnn, the same model, takes train_roi_head, '
                                          'train_rpn_head and train_extractor' % ', '.join(asked))
        kw = dict(_COMMON)
        unknown = set(kwargs) - set(kw)
        if unknown:
            raise TypeError('unexpected keyword argument(s) %s' % sorted(unknown))
        kw.update(kwargs)
        self._depth = depth
        self._roi_feature_size = roi_feature_size
        if len(kw['ratios']) * len(kw['scales']) != 9 or kw['extractor_stride'] != 16:
            raise ValueError('ResNetFasterRcnn: the dense kernels are built for 9 anchors per cell at stride 16')
        self._init_with_dense(ResNetC4Detector(depth, kw['num_classes'], (64, 64), 1, dtype=dtype, f32_form=f32_form), dtype, device, kw)


class TrainableResNetFasterRcnn(ResNetFasterRcnn):
    """ResNetFasterRcnn with the three training keywords (float32, f32_form 'exact'; the module docstring), under Vgg16FasterRcnn's
    rules: `train_roi_head` (the conv5 stack on the crops, the global average pooling in ops.global_avg_pool's order, score and
    bbox), `train_rpn_head`, `train_extractor` (conv3 and conv4, with at least one of the two heads).  With all three
    `sum(losses).backward()` fills every parameter the reference trains -- conv3, conv4, conv5, the RpnHead, score, bbox: 94 of
    116 at depth 50, 196 of 218 at depth 101 -- and leaves the 22 of conv1 and the conv2 stack (trainable=False,
    resnet_faster_rcnn.py:109, 139-141) alone.  There is no dropout in this head, so no `dropout_seed`.  With the keywords off,
    and in every inference call, the model is ResNetFasterRcnn bit for bit; a training call's RoI scores go through the trainable
    head's pooling and differ from it by that pooling's rounding."""

    _accepts_train_keywords = True

    def __init__(self, depth=50, roi_feature_size=(7, 7, 1024), dtype=torch.float32, device='cuda', f32_form='exact',
                 train_roi_head=False, train_rpn_head=False, train_extractor=False, **kwargs):
        super().__init__(depth, roi_feature_size, dtype, device, f32_form, train_roi_head=train_roi_head,
                         train_rpn_head=train_rpn_head, train_extractor=train_extractor, **kwargs)

    def _take_train_keywords(self, kwargs, dtype, f32_form):
        """checks the three keywords, sets the _train_* attributes (before the base constructor reads them) and removes them from
        ``kwargs``"""
        roi, rpn, ext = (kwargs.pop(k) for k in ('train_roi_head', 'train_rpn_head', 'train_extractor'))
        check_train_flags('TrainableResNetFasterRcnn', dtype, f32_form,
                          (ext, 'train_extractor', 'the bottleneck backward has'),
                          (roi, 'train_roi_head', 'the bottleneck backward has'),
                          (rpn, 'train_rpn_head', 'the convolution backward has'))
        check_train_extractor(ext, rpn, roi)
        self._train_roi_head, self._train_rpn_head, self._train_extractor = bool(roi), bool(rpn), bool(ext)

    def _get_trainable_roi_head(self):
        return self._dense_ref.roi_head_trainable


class Vgg16FasterRcnn(_FrcnnFromDense):
    """reference vgg16_faster_rcnn.py:11-115: Vgg16Extractor (:260-342) + Vgg16RoiHead (:178-257).  `slim_ckpt_file_path` must be
    None: no checkpoint exists offline (random initialisation).  `train_roi_head`, `train_rpn_head`, `train_extractor` (float32,
    f32_form 'exact'; the module docstring): with all three `sum(losses).backward()` fills the 32 parameters the reference trains
    -- block3_conv1 .. block5_conv3, the RpnHead, fc1, fc2, score, bbox -- and leaves the eight of blocks 1-2 (trainable=False,
    :265-288) alone.  `roi_head_keep_dropout_rate` is the keep probability of the head's two dropouts (:250-253): active in a
    training call with `train_roi_head`, identity everywhere else; their masks come from `dropout_seed` and a per-call image id
    (ops.dropout)."""

    def __init__(self, slim_ckpt_file_path=None, roi_head_keep_dropout_rate=0.5, roi_feature_size=(7, 7, 512),
                 dtype=torch.float32, device='cuda', f32_form='exact', train_roi_head=False, train_rpn_head=False,
                 train_extractor=False, dropout_seed=0, **kwargs):
        from .frcnn_detector import Vgg16Detector
        check_caller_f32_form(f32_form)
        check_train_flags('Vgg16FasterRcnn', dtype, f32_form,
                          (train_extractor, 'train_extractor', 'the convolution and pooling backward have'),
                          (train_roi_head, 'train_roi_head', 'the Dense backward has'),
                          (train_rpn_head, 'train_rpn_head', 'the convolution backward has'))
        check_train_extractor(train_extractor, train_rpn_head, train_roi_head)
        if train_roi_head and not 0.0 < float(roi_head_keep_dropout_rate) <= 1.0:
            raise ValueError('Vgg16FasterRcnn: roi_head_keep_dropout_rate must be in (0, 1], got %r' % (roi_head_keep_dropout_rate,))
        if slim_ckpt_file_path is not None:
            raise ValueError('Vgg16FasterRcnn: checkpoint import is out of scope (SURVEY section 2); weights are random')
        kw = dict(_COMMON)
        unknown = set(kwargs) - set(kw)
        if unknown:
            raise TypeError('unexpected keyword argument(s) %s' % sorted(unknown))
        kw.update(kwargs)
        self._train_roi_head, self._train_rpn_head = bool(train_roi_head), bool(train_rpn_head)
        self._train_extractor = bool(train_extractor)
        self._roi_head_keep_dropout_rate = roi_head_keep_dropout_rate
        self._dropout_seed = int(dropout_seed)
        self._roi_feature_size = roi_feature_size
        if len(kw['ratios']) * len(kw['scales']) != 9 or kw['extractor_stride'] != 16:
            raise ValueError('Vgg16FasterRcnn: the dense kernels are built for 9 anchors per cell at stride 16')
        self._init_with_dense(Vgg16Detector(kw['num_classes'], (64, 64), 1, dtype=dtype, f32_form=f32_form), dtype, device, kw)

    def _get_trainable_roi_head(self):
        keep, seed, image_id = self._roi_head_keep_dropout_rate, self._dropout_seed, self._dropout_image_id
        return lambda roi_features: self._dense_ref.roi_head_trainable(roi_features, keep, seed, image_id)
