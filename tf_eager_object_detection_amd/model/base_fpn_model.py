"""BaseFPN / RpnHead / ResnetV1Fpn -- counterparts of the reference's model/fpn/base_fpn_model.py (BaseFPN :14-390, RpnHead
:393-434) and model/fpn/resnet_fpn.py (ResnetV1Fpn :410-543): the CALLER objects of the hot path, with the reference's
constructor arguments, `call(inputs, training=None, mask=None)` and `im_detect(preprocessed_img, img_scale)`.

`call` (written once for both families: model/caller_base.py) composes the reference-NAMED layers of this package in the
reference's order -- `_extractor` -> `_neck` -> `_rpn_head` per level -> `_get_anchors` (make_anchors per level) -> fg
softmax -> `_rpn_proposal` (RegionProposal) ->
`_assign_levels` -> `_get_roi_features` (one RoiPoolingCropAndResize2 call per non-empty level + concat) -> `_roi_head` ->
softmax -> post_ops_prediction -- with the reference's dynamic shapes (one host sync per stage, as TF-eager has) and its
batch of one image (model/roi_pooling.py:28).  It is the drop-in reading of "base_fpn_model.py can call it"; the
static-shape, sync-free arrangement of the same stages for throughput is model/fpn_detector.py + pipeline.FpnHotPath.
Every tensor op between the layers that the reference delegates to TF (softmax, gather, concat, reshape) is a torch op on
the GPU; every detection op is a HIP kernel behind the C ABI.  Training (`training=True`) returns the four losses of the
forward pass (:232-264) on the target layers of this package; the dense kernels are inference kernels (no backward), except
the FPN RoI head with `train_roi_head=True` (float32, exact form): its four Dense layers then run ops.dense_trainable and the two
RoI losses carry a graph into fc1, fc2, score and bbox -- and, when the maps handed to the pooling require a gradient, through
ops.roi_pool_trainable into those maps (without `train_neck` the models' own maps never do).
Likewise the RpnHead with `train_rpn_head=True`: its three convolutions run fpn_detector's rpn_trainable over all levels at once and
the two RPN losses carry a graph into rpn_conv, rpn_score and rpn_bbox.  With `train_neck=True` (and at least one of the two heads
trainable) the neck runs fpn_detector's neck_trainable: P2..P6 require a gradient, the RoI pooling takes its trainable form, the
RpnHead returns its input gradient, the two heads' gradients meet in P2..P5 and the four losses carry a graph into the neck's seven
convolutions -- every parameter downstream of the extractor.  With `train_extractor=True` as well (which needs `train_neck`) the
extractor runs fpn_detector's extractor_trainable outside no_grad: C2..C5 require a gradient, neck_trainable delivers dC2..dC5 and the
losses carry a graph into every convolution of conv2..conv5 (reference resnet_fpn.py:208-225: trainable, batch-norm frozen); the stem
(conv1 and its pooling) stays under no_grad unless `train_stem=True` as well (which needs `train_extractor`): then it runs
ops.stem_trainable and conv1's weight and bias receive a gradient too, as in the reference (resnet_fpn.py:233: trainable=True) --
with all five keywords every parameter of the detector does (134 at depth 50, 236 at depth 101).
A training call whose inputs are a FOUR-tuple (images [B,H,W,3], gt_bboxes [sum G,4], gt_labels [sum G], gt_offsets int32 [B+1]) runs
B images in one forward and one backward pass (`_training_batch`; training_targets = training_losses = 'hip') and returns four
[B] tensors; with one image it is the three-tuple call, bit for bit."""
import torch

from .. import ops
from ..utils.anchor_generator import make_anchors
from .caller_base import CallerModel, DenseParts, DenseRpnHead, _Part, _image_nhwc, _nhwc, check_train_dependencies, \
    check_training_losses, run_part
from .detector_base import caller_range_checked, check_caller_f32_form
from .losses import fused_roi_losses, fused_rpn_losses
from .roi_pooling import RoiPoolingCropAndResize2, roi_pooling_images
from .trainable_common import check_train_flags

__all__ = ['BaseFPN', 'RpnHead', 'ResnetV1Fpn']


class RpnHead(DenseRpnHead):
    """reference base_fpn_model.py:393-434: 3x3 conv 512 + ReLU -> 1x1 score conv (2A) / 1x1 bbox conv (4A), outputs reshaped
    to [-1, 2] / [-1, 4].  The layers live in `dense` (a detector of model/fpn_detector.py: rpn_conv, rpn_score, rpn_bbox); the
    whole head of a level is one launch in float16 (ops.rpn_head_fused) and three in float32."""

    def _score_width(self):
        return 2

    @staticmethod
    def _dense_input(inputs):
        return [inputs]                          # (one level of the detector's list of levels)


class BaseFPN(CallerModel):
    """reference base_fpn_model.py:14-141 (same constructor arguments, same private attribute names)."""

    _rpn_layout = ops.RPN_LAYOUT_FPN
    _rpn_head_type = RpnHead
    _extractor_stride = 16

    def __init__(self, roi_feature_size=(7, 7, 256), num_classes=21, weight_decay=0.0001,
                 level_name_list=('p2', 'p3', 'p4', 'p5', 'p6'), min_level=2, max_level=5,
                 anchor_stride_list=(4, 8, 16, 32, 64), base_anchor_size_list=(32, 64, 128, 256, 512),
                 ratios=(0.5, 1.0, 2.0), scales=(1.,),
                 rpn_proposal_means=(0, 0, 0, 0), rpn_proposal_stds=(1.0, 1.0, 1.0, 1.0),
                 rpn_proposal_num_pre_nms_train=12000, rpn_proposal_num_post_nms_train=2000,
                 rpn_proposal_num_pre_nms_test=6000, rpn_proposal_num_post_nms_test=300,
                 rpn_proposal_nms_iou_threshold=0.7,
                 rpn_sigma=3.0, rpn_training_pos_iou_threshold=0.7, rpn_training_neg_iou_threshold=0.3,
                 rpn_training_total_num_samples=256, rpn_training_max_pos_samples=128,
                 roi_proposal_means=(0, 0, 0, 0), roi_proposal_stds=(0.1, 0.1, 0.2, 0.2),
                 roi_pool_size=7, roi_pooling_max_pooling_flag=True,
                 roi_sigma=1, roi_training_pos_iou_threshold=0.5, roi_training_neg_iou_threshold=0.1,
                 roi_training_total_num_samples=128, roi_training_max_pos_samples=32,
                 prediction_max_objects_per_image=50, prediction_max_objects_per_class=50,
                 prediction_nms_iou_threshold=0.3, prediction_score_threshold=0., training_targets='torch',
                 training_losses='torch', train_roi_head=False, train_rpn_head=False, train_neck=False, train_extractor=False,
                 grad_form='exact', train_stem=False):
        super().__init__()
        self.grad_form = ops.check_grad_form(grad_form)
        self._training_losses = check_training_losses(training_losses, training_targets)
        check_train_dependencies(train_extractor, train_neck, train_rpn_head, train_roi_head, has_neck=True, train_stem=train_stem)
        # True: the training branches run that part with a backward pass (caller_base.CallerModel)
        self._train_extractor, self._train_neck, self._train_stem = bool(train_extractor), bool(train_neck), bool(train_stem)
        self._train_roi_head, self._train_rpn_head = bool(train_roi_head), bool(train_rpn_head)
        self.roi_feature_size = roi_feature_size
        self.num_classes = num_classes
        self.weight_decay = weight_decay
        self._level_name_list = level_name_list
        self._min_level = min_level
        self._max_level = max_level
        self._anchor_stride_list = anchor_stride_list
        self._base_anchor_size_list = base_anchor_size_list
        self._ratios = ratios
        self._scales = scales
        self._num_anchors = len(ratios) * len(scales)

        self._extractor = self._get_extractor()
        self._neck = self._get_neck()
        self._rpn_head = self._get_rpn_head(weight_decay)
        self._init_shared_layers(locals())
        self._roi_pooling = RoiPoolingCropAndResize2(pool_size=roi_pool_size, trainable=self._train_roi_head)
        self._roi_head = self._get_roi_head()

    def _get_neck(self):
        raise NotImplementedError

    # ---- :143-200 ------------------------------------------------------------------------------
    def _get_roi_features(self, rois_list, p_list, image_shape):
        all_roi_features = []
        for level_name, cur_rois, cur_p, cur_stride in zip(self._level_name_list[:-1], rois_list, p_list,
                                                           self._anchor_stride_list):
            if cur_rois.shape[0] == 0:
                continue
            all_roi_features.append(self._roi_pooling((cur_p, cur_rois, image_shape)))
        return torch.cat(all_roi_features, dim=0)

    def _get_anchors(self, image_shape):
        all_anchors = []
        for idx in range(len(self._level_name_list)):
            extractor_stride = self._anchor_stride_list[idx]
            # (python's true division + ceil, as tf.ceil(image_shape[0] / extractor_stride) on python ints)
            all_anchors.append(make_anchors(base_anchor_size=self._base_anchor_size_list[idx], anchor_scales=self._scales,
                                            anchor_ratios=self._ratios,
                                            featuremap_height=float(-(-image_shape[0] // extractor_stride)),
                                            featuremap_width=float(-(-image_shape[1] // extractor_stride)),
                                            stride=extractor_stride))
        return torch.cat(all_anchors, dim=0)

    def _get_fpn_head_results(self, p_list, per_image=False):
        """per_image (the batched training call): a level's rows are [B * n_level, ...], image-major, so they are cut per image
        BEFORE the levels are joined -- [B, n, 2] / [B, n, 4]; joining the flat rows would mix the images"""
        all_fpn_scores, all_fpn_bbox_pred = [], []
        for level_name, p in zip(self._level_name_list, p_list):
            cur_score, cur_bboxes_pred = self._rpn_head(p)
            if per_image:
                cur_score, cur_bboxes_pred = cur_score.reshape(p.shape[0], -1, 2), cur_bboxes_pred.reshape(p.shape[0], -1, 4)
            all_fpn_scores.append(cur_score)
            all_fpn_bbox_pred.append(cur_bboxes_pred)
        dim = 1 if per_image else 0
        return torch.cat(all_fpn_scores, dim=dim), torch.cat(all_fpn_bbox_pred, dim=dim)

    # ---- :208-220: the dense parts of the front (CallerModel._anchors_and_proposals) ------------
    def _dense_front(self, image, image_shape, training, train, per_image=False):
        # extractor: conv2..conv5 OUTSIDE no_grad with train_extractor (the stem stays inside without train_stem): C2..C5 require
        # a gradient, which the trainable neck delivers.  neck: P2..P6 require a gradient with train_neck, which the RpnHead's
        # input gradient and the trainable RoI pooling deliver.  RpnHead: the head of all levels at once with train_rpn_head, so
        # that the RPN losses see these tensors and carry their graph
        c_list = run_part(train and self._train_extractor, lambda: self._get_trainable_extractor_results(image),
                          lambda: self._extractor(image, training=training))
        p_list = run_part(train and self._train_neck, lambda: self._get_trainable_neck_results(c_list),
                          lambda: self._neck(c_list, training=training))
        all_fpn_scores, all_fpn_bbox_pred = run_part(train and self._train_rpn_head,
                                                     lambda: self._get_trainable_rpn_head_results(list(p_list)),
                                                     lambda: self._get_fpn_head_results(p_list, per_image))
        if per_image:
            # (the trainable head's rows are the [B, n, ...] outputs of all levels at once, flattened image-major: a view back)
            B = int(image.shape[0])
            all_fpn_scores, all_fpn_bbox_pred = all_fpn_scores.reshape(B, -1, 2), all_fpn_bbox_pred.reshape(B, -1, 4)
        with torch.no_grad():
            all_anchors = self._get_anchors(image_shape)
        return p_list, all_anchors, all_fpn_scores, all_fpn_bbox_pred

    def _get_trainable_neck_results(self, c_list):
        """_neck with a graph into the neck's layers: (P2..P6), bit-equal to it"""
        raise NotImplementedError('train_neck=True needs a dense part with a trainable neck')

    def _rois_for_head(self, rois):
        return self._assign_levels(rois)

    def _pool_rois(self, rois_list, p_list, image_shape, training):
        return self._get_roi_features(rois_list, p_list, image_shape)

    def _assign_levels(self, all_rois):
        """:303-324 -> (rois per level min_level..max_level, the concatenated row indices): odet_assign_levels (levels,
        stable partition) + one host read of the level counts to cut the lists"""
        k = int(all_rois.shape[0])
        srois, level, perm, counts = ops.assign_levels(all_rois, self._min_level, self._max_level)
        cnt = counts.tolist()
        rois_list, off = [], 0
        for c in cnt:
            rois_list.append(srois[off:off + c])
            off += c
        return rois_list, perm[:k]

    # ---- the batched training call (CallerModel._forward_images) ----------------------------------
    _batched_training = True

    def _pooling_maps(self, p_list):
        """the maps of min_level..max_level as the batched pooling takes them: one NHWC [B,H,W,C] tensor per level"""
        return list(p_list[:len(self._level_name_list) - 1])

    def _training_batch(self, images, gt_bboxes, gt_labels, gt_offsets):
        """B images in one forward pass: the stages of `_fused_losses` in its order, each ONE call over the batch -- except the
        proposals, which stay `_rpn_proposal`'s exact mode image by image (the fused batched stage decodes from anchors in
        registers and is pinned to the anchor-tensor path to 1e-4 only; its batch form runs the sync-free mode).  Image b gets
        the sampler ids a loop over single images would give it.  Head rows stay level-sorted per image, so B = 1 does the
        three-tuple call's arithmetic.  After the proposal calls nothing is read on the host."""
        B = int(images.shape[0])
        image_shape = [int(images.shape[1]), int(images.shape[2])]
        p_list, anchors, rpn_score, rpn_deltas = self._dense_front(images, image_shape, True, True, per_image=True)
        n = int(anchors.shape[0])
        dev = anchors.device
        at, pt = self._anchor_target, self._proposal_target
        with torch.no_grad():
            fg = self._fg_scores(rpn_score.detach()).reshape(B, n)          # (elementwise: one launch over all B n rows)
            deltas = rpn_deltas.detach()
            r_max = max(min(int(self._rpn_proposal._num_post_nms_train), n), 1)
            rois = torch.zeros((B, r_max, 4), dtype=torch.float32, device=dev)
            kept = torch.zeros((B, r_max), dtype=torch.int32, device=dev)
            roi_counts = torch.zeros(B, dtype=torch.int32, device=dev)
            for b in range(B):
                self._rpn_proposal.padded((deltas[b], anchors, fg[b], image_shape), training=True,
                                          out=(rois[b], kept[b], roi_counts[b:b + 1]))
            anchor_targets = at.batch(gt_bboxes, gt_offsets, image_shape, anchors, first_image_id=at._next_image_id, dense=False)
            at._next_image_id += B
        rpn_cls_loss, rpn_reg_loss = fused_rpn_losses(rpn_score.float(), rpn_deltas.float(), anchor_targets, self._rpn_sigma,
                                                      self._rpn_layout, self._num_anchors)
        with torch.no_grad():
            # (strict=False: no host read, as in _fused_losses)
            proposal_targets = pt.batch(rois, gt_bboxes, gt_labels, gt_offsets, first_image_id=pt._next_image_id,
                                        roi_counts=roi_counts, strict=False)
            pt._next_image_id += B
            # all S rows of every image, as the single-image path: levels, stable partition, the rows' target rows -- no host
            # read of the level counts, no Python list per level
            sorted_rois, roi_level, row_map, level_counts = ops.assign_levels_images(proposal_targets.final_rois, self._min_level,
                                                                                    self._max_level)
        S = int(sorted_rois.shape[1])
        maps = self._pooling_maps(p_list)

        def pool():
            return roi_pooling_images(maps, sorted_rois, roi_level, ops.ROI_NORM_IMAGE, self._roi_pooling._pool_size,
                                      ops.ROI_POOL_MAX2, image_shape=image_shape, trainable=self._roi_pooling._trainable)

        def rows(features):
            return features.reshape((B * S,) + tuple(features.shape[2:]))

        # (_training_roi_head's decision between the trainable and the plain forms)
        if self._train_roi_head and any(m.requires_grad for m in maps):
            roi_features = pool()
            roi_score, roi_bboxes_txtytwth = self._get_trainable_roi_head()(rows(roi_features))
        else:
            with torch.no_grad():
                roi_features = pool()
                if not self._train_roi_head:
                    roi_score, roi_bboxes_txtytwth = self._roi_head(rows(roi_features), training=True)
            if self._train_roi_head:
                roi_score, roi_bboxes_txtytwth = self._get_trainable_roi_head()(rows(roi_features))
        roi_cls_loss, roi_reg_loss = fused_roi_losses(roi_score.float().reshape(B, S, -1), roi_bboxes_txtytwth.float().reshape(B, S, -1),
                                                      proposal_targets, self._roi_sigma, row_map=row_map)
        if self.keep_training_pass:
            self.last_training_pass = dict(
                rpn_score=rpn_score, rpn_deltas=rpn_deltas, maps=maps, anchors=anchors, rois=rois, roi_counts=roi_counts,
                anchor_targets=anchor_targets, proposal_targets=proposal_targets, sorted_rois=sorted_rois, roi_level=roi_level,
                row_map=row_map, level_counts=level_counts, roi_features=roi_features)
        return rpn_cls_loss, rpn_reg_loss, roi_cls_loss, roi_reg_loss

    # ---- :326-362 (im_detect :364-390: CallerModel) ---------------------------------------------
    def predict_rpns(self, image_shape, gt_bboxes):
        all_anchors = self._get_anchors(image_shape)
        rpn_labels, _, _, _ = self._anchor_target((gt_bboxes, image_shape, all_anchors), True)
        return all_anchors[torch.nonzero(rpn_labels > 0)[:, 0]]

    @caller_range_checked
    @torch.no_grad()
    def predict_rois(self, preprocessed_img, gt_bboxes, gt_labels, training=True):
        rois = self._anchors_and_proposals(_image_nhwc(preprocessed_img), training, trainable=False)[5]
        return self._proposal_target((rois, gt_bboxes, gt_labels), True)[0]


class ResnetV1Fpn(DenseParts, BaseFPN):
    """reference resnet_fpn.py:410-543 (same constructor arguments and defaults).  The dense parts -- extractor
    (get_resnet_v1_extractor :262-289), ResnetFpnNeck (:339-407), the RpnHead's convolutions and ResnetRoiHead (:292-336;
    dropout is inference-only identity) -- are the hand-written kernels of model/fpn_detector.ResNetFpnDetector, which this
    class owns as `dense`; weights are randomly initialised with the reference's initialisers (no checkpoints offline).
    `dtype`: torch.float32 (the reference's precision) or torch.float16 (throughput mode); `f32_form`: the float32 layers'
    arithmetic, 'exact' (float32 matrix instructions), 'x3' (split precision, three bfloat16 limbs) or 'x2' (two float16 limbs; a
    pass that leaves float16's range is repeated on three limbs: detector_base.caller_range_checked) -- ops.f32_form."""

    def __init__(self, depth=50, roi_head_keep_dropout_rate=0.5, roi_feature_size=(7, 7, 256), num_classes=21,
                 weight_decay=0.0001, level_name_list=('p2', 'p3', 'p4', 'p5', 'p6'), min_level=2, max_level=5,
                 top_down_dims=256, anchor_stride_list=(4, 8, 16, 32, 64), base_anchor_size_list=(32, 64, 128, 256, 512),
                 ratios=(0.5, 1.0, 2.0), scales=(1.,), rpn_proposal_means=(0, 0, 0, 0),
                 rpn_proposal_stds=(1.0, 1.0, 1.0, 1.0), rpn_proposal_num_pre_nms_train=12000,
                 rpn_proposal_num_post_nms_train=2000, rpn_proposal_num_pre_nms_test=6000,
                 rpn_proposal_num_post_nms_test=1000, rpn_proposal_nms_iou_threshold=0.7, rpn_sigma=3.0,
                 rpn_training_pos_iou_threshold=0.7, rpn_training_neg_iou_threshold=0.3,
                 rpn_training_total_num_samples=256, rpn_training_max_pos_samples=128, roi_proposal_means=(0, 0, 0, 0),
                 roi_proposal_stds=(0.1, 0.1, 0.2, 0.2), roi_pool_size=7, roi_pooling_max_pooling_flag=True, roi_sigma=1,
                 roi_training_pos_iou_threshold=0.5, roi_training_neg_iou_threshold=0.1,
                 roi_training_total_num_samples=256, roi_training_max_pos_samples=64,
                 prediction_max_objects_per_image=50, prediction_max_objects_per_class=50,
                 prediction_nms_iou_threshold=0.3, prediction_score_threshold=0.3, dtype=torch.float32, device='cuda',
                 f32_form='exact', training_targets='torch', training_losses='torch', train_roi_head=False, train_rpn_head=False,
                 train_neck=False, train_extractor=False, grad_form='exact', train_stem=False):
        from .fpn_detector import ResNetFpnDetector
        ops.check_grad_form(grad_form)
        check_caller_f32_form(f32_form)
        exact = lambda *flags: check_train_flags('ResnetV1Fpn', dtype, f32_form, *flags)
        exact((train_stem, 'train_stem', "the stem's backward has"),
              (train_extractor, 'train_extractor', 'the bottleneck backward has'),
              (train_neck, 'train_neck', "the neck's backward has"))
        check_train_dependencies(train_extractor, train_neck, train_rpn_head, train_roi_head, has_neck=True, train_stem=train_stem)
        exact((train_roi_head, 'train_roi_head', 'the Dense backward has'),
              (train_rpn_head, 'train_rpn_head', 'the convolution backward has'))
        if top_down_dims != 256 or tuple(roi_feature_size) != (roi_pool_size, roi_pool_size, top_down_dims):
            raise ValueError('ResnetV1Fpn: the dense kernels are built for 256 top-down channels and %dx%dx256 RoI features'
                             % (roi_pool_size, roi_pool_size))
        if len(ratios) * len(scales) != 3:
            raise ValueError('ResnetV1Fpn: the RpnHead is built for 3 anchors per cell (ratios x scales)')
        self._depth = depth
        self._roi_head_keep_dropout_rate = roi_head_keep_dropout_rate
        self._top_down_dims = top_down_dims
        self._init_with_dense(ResNetFpnDetector(depth, num_classes, (64, 64), 1, dtype=dtype, f32_form=f32_form,
                                                grad_form=grad_form), dtype, device,
                              BaseFPN.__init__, dict(
            roi_feature_size=roi_feature_size, num_classes=num_classes, weight_decay=weight_decay,
            level_name_list=level_name_list, min_level=min_level, max_level=max_level, anchor_stride_list=anchor_stride_list,
            base_anchor_size_list=base_anchor_size_list, ratios=ratios, scales=scales, rpn_proposal_means=rpn_proposal_means,
            rpn_proposal_stds=rpn_proposal_stds, rpn_proposal_num_pre_nms_train=rpn_proposal_num_pre_nms_train,
            rpn_proposal_num_post_nms_train=rpn_proposal_num_post_nms_train,
            rpn_proposal_num_pre_nms_test=rpn_proposal_num_pre_nms_test,
            rpn_proposal_num_post_nms_test=rpn_proposal_num_post_nms_test,
            rpn_proposal_nms_iou_threshold=rpn_proposal_nms_iou_threshold, rpn_sigma=rpn_sigma,
            rpn_training_pos_iou_threshold=rpn_training_pos_iou_threshold,
            rpn_training_neg_iou_threshold=rpn_training_neg_iou_threshold,
            rpn_training_total_num_samples=rpn_training_total_num_samples,
            rpn_training_max_pos_samples=rpn_training_max_pos_samples, roi_proposal_means=roi_proposal_means,
            roi_proposal_stds=roi_proposal_stds, roi_pool_size=roi_pool_size,
            roi_pooling_max_pooling_flag=roi_pooling_max_pooling_flag, roi_sigma=roi_sigma,
            roi_training_pos_iou_threshold=roi_training_pos_iou_threshold,
            roi_training_neg_iou_threshold=roi_training_neg_iou_threshold,
            roi_training_total_num_samples=roi_training_total_num_samples,
            roi_training_max_pos_samples=roi_training_max_pos_samples,
            prediction_max_objects_per_image=prediction_max_objects_per_image,
            prediction_max_objects_per_class=prediction_max_objects_per_class,
            prediction_nms_iou_threshold=prediction_nms_iou_threshold, prediction_score_threshold=prediction_score_threshold,
            training_targets=training_targets, training_losses=training_losses, train_roi_head=train_roi_head,
            train_rpn_head=train_rpn_head, train_neck=train_neck, train_extractor=train_extractor, grad_form=grad_form,
            train_stem=train_stem))

    def _get_extractor(self):
        return _Part(self._dense_ref.extractor)

    def _get_neck(self):
        return _Part(self._dense_ref.neck)

    def _get_trainable_extractor_results(self, image):
        return self._dense_ref.extractor_trainable(image, train_stem=self._train_stem)

    def _get_trainable_neck_results(self, c_list):
        return self._dense_ref.neck_trainable(list(c_list))

    def _get_roi_features(self, rois_list, p_list, image_shape):
        # the dense kernels keep maps channels_last [B,C,H,W]; the pooling layer takes the NHWC view of the same memory
        return super()._get_roi_features(rois_list, [_nhwc(p) for p in p_list], image_shape)

    def _pooling_maps(self, p_list):
        return [_nhwc(p) for p in super()._pooling_maps(p_list)]
