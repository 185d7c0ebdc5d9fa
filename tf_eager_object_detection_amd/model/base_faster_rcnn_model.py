"""BaseFasterRcnn / RpnHead / ResNetFasterRcnn (TrainableResNetFasterRcnn) / Vgg16FasterRcnn -- counterparts of the
reference's model/faster_rcnn/base_faster_rcnn_model.py (BaseFasterRcnn :16-306, RpnHead :309-350), resnet_faster_rcnn.py
(ResNetFasterRcnn :188-293) and vgg16_faster_rcnn.py (Vgg16FasterRcnn :11-115): the CALLER objects of the single-level hot
path, with the reference's constructor arguments, `call(inputs, training=None, mask=None)` and `im_detect`.

`call` (written once for both families: model/caller_base.py) composes the reference-named layers in the reference's order
(:126-198): `_extractor` -> `_anchor_generator` (generate_by_anchor_base_tf) -> `_rpn_head` -> the [A bg | A fg] score
re-layout + softmax -> `_rpn_proposal` ->
`_roi_pooling` (RoiPoolingCropAndResize) -> `_roi_head` -> softmax -> post_ops_prediction, with dynamic shapes and one image
per call as in the reference.  The static-shape, sync-free arrangement for throughput is model/frcnn_detector.py.

The training branches run every dense part under no_grad unless a keyword switches its backward pass on (Vgg16FasterRcnn,
TrainableResNetFasterRcnn; float32, f32_form 'exact'): `train_roi_head` runs the RoI head's trainable form -- VGG16's with the
reference's two dropouts -- (the two RoI losses carry a graph into fc1, fc2, score and bbox / into the conv5 stack, score and
bbox), `train_rpn_head` the RpnHead's (the two RPN losses carry a graph into rpn_conv, rpn_score and rpn_bbox), `train_extractor`
(with at least one of the two) the extractor's: the shared map requires a gradient, which the RpnHead's input gradient and the
trainable RoI pooling deliver, and the losses carry a graph into block3_conv1 .. block5_conv3 / into conv3 and conv4."""
import math

import torch

from .. import ops
from ..utils.anchor_generator import generate_anchor_base, generate_by_anchor_base_tf
from .caller_base import CallerModel, DenseParts, DenseRpnHead, _Part, _image_nhwc, _nhwc, check_train_dependencies, \
    check_training_losses, run_part
from .detector_base import check_caller_f32_form
from .roi_pooling import RoiPoolingCropAndResize
from .trainable_common import check_train_flags

__all__ = ['BaseFasterRcnn', 'RpnHead', 'ResNetFasterRcnn', 'TrainableResNetFasterRcnn', 'Vgg16FasterRcnn']


class RpnHead(DenseRpnHead):
    """reference base_faster_rcnn_model.py:309-350: scores reshaped to [-1, 2A] ([A bg | A fg] per cell), boxes to [-1, 4];
    the convolutions live in `dense` (a detector of model/frcnn_detector.py)."""

    def _score_width(self):
        return 2 * self._num_anchors


class BaseFasterRcnn(CallerModel):
    """reference base_faster_rcnn_model.py:16-118 (same constructor arguments, same private attribute names).  The constructor
    keeps the reference's arguments, so a concrete model with trainable dense parts (Vgg16FasterRcnn) sets the `_train_*`
    attributes (caller_base.CallerModel) on the instance before it calls it."""

    _rpn_layout = ops.RPN_LAYOUT_FRCNN
    _rpn_head_type = RpnHead

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
        check_train_dependencies(self._train_extractor, False, self._train_rpn_head, self._train_roi_head, has_neck=False)
        # the image id of the RoI head's dropout masks: advances once per training call, whatever the target stage does
        self._next_dropout_image_id = 0
        self._dropout_image_id = 0
        self.num_classes = num_classes
        self.weight_decay = weight_decay
        self._ratios = ratios
        self._scales = scales
        self._num_anchors = len(ratios) * len(scales)
        self._extractor_stride = extractor_stride
        self._anchor_generator = generate_by_anchor_base_tf
        self._anchor_base = generate_anchor_base(extractor_stride, ratios, scales).astype('float32')      # :84 tf.to_float
        self._rpn_head = self._get_rpn_head(weight_decay)
        self._init_shared_layers(locals())
        self._roi_pooling = RoiPoolingCropAndResize(pool_size=roi_pool_size, max_pooling_flag=roi_pooling_max_pooling_flag,
                                                    trainable=self._train_roi_head)
        self._extractor = self._get_extractor()
        self._roi_head = self._get_roi_head()

    def _start_training_call(self):
        self._dropout_image_id = self._next_dropout_image_id
        self._next_dropout_image_id += 1

    def _anchors(self, image_shape):
        return self._anchor_generator(self._anchor_base, self._extractor_stride,
                                      int(math.ceil(image_shape[0] / self._extractor_stride)),
                                      int(math.ceil(image_shape[1] / self._extractor_stride)))

    # ---- :130-146 / :279-296: the dense parts of the front (CallerModel._anchors_and_proposals) --
    def _dense_front(self, image, image_shape, training, train):
        shared_features = run_part(train and self._train_extractor, lambda: self._get_trainable_extractor_results(image),
                                   lambda: self._extractor(image, training=training))
        with torch.no_grad():
            anchors = self._anchors(image_shape)
        rpn_score, rpn_bbox_txtytwth = run_part(train and self._train_rpn_head,
                                                lambda: self._get_trainable_rpn_head_results(shared_features),
                                                lambda: self._rpn_head(shared_features, training=training))
        return shared_features, anchors, rpn_score, rpn_bbox_txtytwth

    def _pool_rois(self, rois, shared_features, image_shape, training):
        return self._roi_pooling((shared_features, rois, self._extractor_stride), training=training)

    def _rpn_score_rows(self, rpn_score):
        """:200-215: the [A bg | A fg] scores re-laid as [N, 2] rows before the selection"""
        return rpn_score.reshape(-1, 2, self._num_anchors).permute(0, 2, 1).reshape(-1, 2)

    def predict_rpn(self, image, gt_bboxes):
        """:226-241 (a debugging helper): the anchors AnchorTarget labels positive for `gt_bboxes`.  The reference's body is
        stale against its own AnchorTarget (it passes (anchors, gt_bboxes, image_shape) and unpacks an index list and a count,
        model/anchor_target.py:37-107 takes (gt_bboxes, image_shape, anchors) and returns labels); this is its intent, written
        like BaseFPN.predict_rpns (model/fpn/base_fpn_model.py:326-340)."""
        image = _image_nhwc(image)
        image_shape = [int(image.shape[1]), int(image.shape[2])]
        anchors = self._anchors(image_shape)
        rpn_labels, _, _, _ = self._anchor_target((gt_bboxes, image_shape, anchors), True)
        return anchors[torch.nonzero(rpn_labels > 0)[:, 0]]

    @torch.no_grad()
    def predict_roi(self, image, gt_bboxes, gt_labels):
        """:243-266: (final_rois, final_labels, final_bbox_targets, bbox_inside_weights, bbox_outside_weights) of the
        training-mode proposals"""
        image = _image_nhwc(image)
        rois = self._anchors_and_proposals(image, True)[5]
        return self._proposal_target((rois, gt_bboxes, gt_labels), True)


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


class _FrcnnFromDense(DenseParts, BaseFasterRcnn):
    """shared plumbing of the concrete models: the dense parts are a detector of model/frcnn_detector.py (`dense`)"""

    def _common_keywords(self, name, kwargs):
        """`_COMMON` with the caller's keywords, for the model `name` the messages speak of"""
        kw = dict(_COMMON)
        unknown = set(kwargs) - set(kw)
        if unknown:
            raise TypeError('unexpected keyword argument(s) %s' % sorted(unknown))
        kw.update(kwargs)
        if len(kw['ratios']) * len(kw['scales']) != 9 or kw['extractor_stride'] != 16:
            raise ValueError('%s: the dense kernels are built for 9 anchors per cell at stride 16' % name)
        return kw

    def _get_extractor(self):
        return _Part(self._dense_ref.features)

    def _anchors_and_proposals(self, image, training, trainable=True):
        out = list(super()._anchors_and_proposals(image, training, trainable))
        # the detectors keep maps channels_last [B,C,H,W]; the pooling layer takes the NHWC view of the same memory
        out[1] = _nhwc(out[1])
        return tuple(out)


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
        kw = self._common_keywords('ResNetFasterRcnn', kwargs)
        self._depth = depth
        self._roi_feature_size = roi_feature_size
        self._init_with_dense(ResNetC4Detector(depth, kw['num_classes'], (64, 64), 1, dtype=dtype, f32_form=f32_form,
                                               grad_form=self.grad_form), dtype, device,
                              BaseFasterRcnn.__init__, kw)


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
                 train_roi_head=False, train_rpn_head=False, train_extractor=False, grad_form='exact', **kwargs):
        self.grad_form = ops.check_grad_form(grad_form)
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
        check_train_dependencies(ext, False, rpn, roi, has_neck=False)
        self._train_roi_head, self._train_rpn_head, self._train_extractor = bool(roi), bool(rpn), bool(ext)


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
                 train_extractor=False, dropout_seed=0, grad_form='exact', **kwargs):
        from .frcnn_detector import Vgg16Detector
        self.grad_form = ops.check_grad_form(grad_form)
        check_caller_f32_form(f32_form)
        check_train_flags('Vgg16FasterRcnn', dtype, f32_form,
                          (train_extractor, 'train_extractor', 'the convolution and pooling backward have'),
                          (train_roi_head, 'train_roi_head', 'the Dense backward has'),
                          (train_rpn_head, 'train_rpn_head', 'the convolution backward has'))
        check_train_dependencies(train_extractor, False, train_rpn_head, train_roi_head, has_neck=False)
        if train_roi_head and not 0.0 < float(roi_head_keep_dropout_rate) <= 1.0:
            raise ValueError('Vgg16FasterRcnn: roi_head_keep_dropout_rate must be in (0, 1], got %r' % (roi_head_keep_dropout_rate,))
        if slim_ckpt_file_path is not None:
            raise ValueError('Vgg16FasterRcnn: checkpoint import is out of scope (SURVEY section 2); weights are random')
        kw = self._common_keywords('Vgg16FasterRcnn', kwargs)
        self._train_roi_head, self._train_rpn_head = bool(train_roi_head), bool(train_rpn_head)
        self._train_extractor = bool(train_extractor)
        self._roi_head_keep_dropout_rate = roi_head_keep_dropout_rate
        self._dropout_seed = int(dropout_seed)
        self._roi_feature_size = roi_feature_size
        self._init_with_dense(Vgg16Detector(kw['num_classes'], (64, 64), 1, dtype=dtype, f32_form=f32_form,
                                            grad_form=grad_form), dtype, device,
                              BaseFasterRcnn.__init__, kw)

    def _get_trainable_roi_head(self):
        keep, seed, image_id = self._roi_head_keep_dropout_rate, self._dropout_seed, self._dropout_image_id
        return lambda roi_features: self._dense_ref.roi_head_trainable(roi_features, keep, seed, image_id)
