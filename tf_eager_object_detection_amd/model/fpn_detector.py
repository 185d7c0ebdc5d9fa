"""ResNet-FPN detector assembled around the HIP hot path -- counterpart of the reference's
model/fpn/resnet_fpn.py (ResnetV1Fpn: extractor, ResnetFpnNeck, ResnetRoiHead) + the inference
branch of model/fpn/base_fpn_model.py (BaseFPN.call, RpnHead).

SURVEY.md section 8(f) ranks 2-3 ("next"): the dense conv / FC stacks are genuine dense contractions and run on the
matrix cores through THIS REPOSITORY'S kernels: the layer builders and the routing to the kernels (no library convolution or
GEMM route, no CPU path: a layer no kernel takes raises) are model/layers.py's, shared with the single-level detectors and the
trainable parts (model/*_trainable.py, which import layers and never this file: they are imported here at the top).

float32 is the parity mode (exact-float32 matrix instructions), float16 the throughput mode.  Weights are randomly
initialised with the reference's initialisers (no checkpoints exist offline); frozen batch-norm (epsilon 1.001e-5,
inference statistics) is folded into the convolutions.  The pass that strings the parts together (prepare, forward,
im_detect, the after-pass checks, the HIP-graph capture) and the RoI heads' last layer are model/detector_base.py's, shared with
the single-level detectors; this file holds the network and the FPN's per-image arrangement.  The plain-torch formulation
of the same network (library convolutions; CPU shape bookkeeping and numerical reference) lives with the tests: tests/torch_reference.py.

Shapes follow the reference exactly so that feature maps and anchor grids agree:
conv1 = pad 3 + 7x7/2 valid, pool1 = pad 1 + 3x3/2 valid, the stride of a stage sits on the first
1x1 convolution of its first block, P6 = P5[::2, ::2], top-down merge = 0.5 * resize_bilinear(P_{k+1})
+ 0.5 * lateral with TF1's legacy resize (src = dst * in/out, no half-pixel offset).
"""
import torch
import torch.nn as nn

from .. import ops
from ..pipeline import FpnHotPath, FpnStepBatch
# (the detectors' shared pass lives in detector_base.py; its names stay importable from here)
from .detector_base import DEFAULT_BLIND_CHUNKS, Detector, _FinalLayer, _FinalTrainable, _NmsCompleteness, _in_f32_form, \
    _x3_workspace_of, caller_range_checked, check_caller_f32_form  # noqa: F401
from .extractor_trainable import extractor_trainable
from .layers import _BLOCKS, _conv, _conv_epi, _fold_frozen_bn, _nhwc, _no_kernel, _own_conv3x3, _pw_ok, _stack, _stem, \
    fc_head_activation, init_linears, rpn_head_layers, rpn_pair_padded, rpn_pair_weights, \
    tf_legacy_resize_bilinear  # noqa: F401  (tf_legacy_resize_bilinear: public surface, see __all__)
# (not used here: the test files of the commit before model/layers.py import these two from this file; new code imports layers)
from .layers import _Block, _conv_relu_pool  # noqa: F401
from .neck_trainable import neck_trainable
from .rpn_trainable import rpn_trainable
from .trainable_common import fc_head_trainable

__all__ = ['ResNetFpnDetector', 'tf_legacy_resize_bilinear']


class ResNetFpnDetector(Detector):
    """Inference-only ResNet-{50,101,152}-FPN detector (the pass itself: detector_base.Detector).  Batched arrangement:
    FpnStepBatch (of the sync-free NMS chunks the first is shared by the batch, the others are per image); per image
    (`batched=False`): one FpnHotPath and one RoI-head call per image, one after the other on the current stream."""

    _step_batch_class, _hot_path_class, _kept_rois = FpnStepBatch, FpnHotPath, 'sorted_rois'

    def __init__(self, depth=101, num_classes=21, image_shape=(800, 1333), num_proposals=1000, dtype=torch.float32,
                 max_batch=1, f32_form='exact', grad_form='exact', **hot_kwargs):
        super().__init__()
        b = _BLOCKS[depth]
        self._declare_modes(dtype, grad_form, f32_form, image_shape, num_classes)
        # extractor (resnet_fpn.py:228-259, 262-289)
        self.conv1 = _fold_frozen_bn(_conv(3, 64, 7, 2, 0))
        self.conv2 = _stack(64, 64, b[0], 1)
        self.conv3 = _stack(256, 128, b[1], 2)
        self.conv4 = _stack(512, 256, b[2], 2)
        self.conv5 = _stack(1024, 512, b[3], 2)
        # neck (resnet_fpn.py:339-407)
        self.p5 = _conv(2048, 256, 1)
        self.l4, self.l3, self.l2 = _conv(1024, 256, 1), _conv(512, 256, 1), _conv(256, 256, 1)
        self.s4, self.s3, self.s2 = _conv(256, 256, 3, 1, 1), _conv(256, 256, 3, 1, 1), _conv(256, 256, 3, 1, 1)
        # RPN head, shared by the five levels (base_fpn_model.py:393-434); 3 anchors per cell
        self.A = 3
        self.rpn_conv, self.rpn_score, self.rpn_bbox = rpn_head_layers(256, self.A)
        # RoI head (resnet_fpn.py:292-336): flatten(7,7,256) -> fc 1024 -> fc 1024 -> score / boxes
        self.fc1 = nn.Linear(7 * 7 * 256, 1024)
        self.fc2 = nn.Linear(1024, 1024)
        self.score = nn.Linear(1024, num_classes)
        self.bbox = nn.Linear(1024, 4 * num_classes)
        init_linears((self.fc1, 0.01), (self.fc2, 0.01), (self.score, 0.01), (self.bbox, 0.001))
        self._declare_hot_path(256, num_proposals, max_batch, hot_kwargs)

    # ---- dense parts ---------------------------------------------------------------------------
    @_in_f32_form
    def extractor(self, images_nhwc):
        """[B,H,W,3] -> (C2, C3, C4, C5) channels_last (get_resnet_v1_extractor, resnet_fpn.py:262-289)."""
        # conv1_pad + valid 7x7/2, bias + ReLU, pool1_pad (zeros) + 3x3/2 -- float16: one launch from the image; otherwise
        # the last three in one pass (x >= 0 after the ReLU, so skipping the window taps outside the map gives the same
        # maxima as the zero padding)
        x = _stem(self.conv1, images_nhwc, self.dtype)
        c2 = self.conv2(x)
        c3 = self.conv3(c2)
        c4 = self.conv4(c3)
        return c2, c3, c4, self.conv5(c4)

    @_in_f32_form
    def extractor_trainable(self, images_nhwc, train_stem=False):
        """extractor with a backward pass into conv2..conv5 (float32, f32_form 'exact'; model/extractor_trainable.py): outputs
        bit-equal to extractor()'s with its shapes and strides; the stem runs under no_grad and conv1 stays frozen, unless
        `train_stem` (one image group): then conv1's weight and bias receive a gradient too, as in the reference
        (resnet_fpn.py:233), and no parameter of the extractor is left without one"""
        return extractor_trainable(self, images_nhwc, train_stem=train_stem)

    def features(self, images_nhwc):
        """[B,H,W,3] -> (P2..P6), each [B,256,h,w] channels_last (= NHWC in memory)."""
        return self.neck(self.extractor(images_nhwc))

    @_in_f32_form
    def neck(self, c_list):
        """(C2..C5) -> (P2..P6) (ResnetFpnNeck.call, resnet_fpn.py:378-407)."""
        c2, c3, c4, c5 = c_list
        p5 = _conv_epi(self.p5, c5)
        p6 = p5[:, :, ::2, ::2]                                                  # MaxPooling2D(1x1, stride 2)
        p4 = self._lateral_merge(p5, self.l4, c4)
        p3 = self._lateral_merge(p4, self.l3, c3)
        p2 = self._lateral_merge(p3, self.l2, c2)
        return _conv_epi(self.s2, p2), _conv_epi(self.s3, p3), _conv_epi(self.s4, p4), p5, p6

    @_in_f32_form
    def neck_trainable(self, c_list):
        """neck with a backward pass into p5, l4, l3, l2, s4, s3 and s2 (float32, f32_form 'exact'; model/neck_trainable.py): outputs
        bit-equal to neck()'s with its shapes and strides, and a gradient into those maps of c_list that require one"""
        return neck_trainable(self, c_list)

    def _lateral_merge(self, top, conv, c):
        """P_k = 0.5 * resize_bilinear(P_{k+1}) + 0.5 * lateral(C_k) (resnet_fpn.py:385-398) in ONE launch: the merge rides in
        the epilogue of the lateral 1x1 convolution (ops.lateral_merge: the lateral map is never written; 226 vs 301 us for
        P2 at batch 8)."""
        if not _pw_ok(conv, c) or tuple(conv.stride) != (1, 1) or top.dtype != c.dtype:
            raise _no_kernel('lateral convolution + top-down merge', conv, c)
        return ops.lateral_merge(_nhwc(c), conv.weight, conv.bias, _nhwc(top)).permute(0, 3, 1, 2)

    @staticmethod
    def _merge(top, lateral):
        """0.5 * resize_bilinear(top) + 0.5 * lateral (resnet_fpn.py:385-398) as a launch of its own (ops.fpn_topdown_merge,
        float32 bit-identical to the TF1 restatement): for callers that already hold the lateral map."""
        return ops.fpn_topdown_merge(_nhwc(top), _nhwc(lateral)).permute(0, 3, 1, 2)

    @_in_f32_form
    def rpn(self, p_list):
        """shared RpnHead on every level; outputs concatenated P2->P6 in (y, x, anchor) order
        (base_fpn_model.py:188-200, 427-432): scores [B, N, 2], deltas [B, N, 4] (float32)."""
        p0 = p_list[0]
        if not _own_conv3x3(self.rpn_conv, p0) or self.rpn_conv.out_channels % 256:
            raise _no_kernel('RpnHead', self.rpn_conv, p0)
        # the two 1x1 convolutions run as ONE contraction (weights concatenated: the 512-channel activation is read once)
        w, b = rpn_pair_weights(self)
        B = p0.shape[0]
        n = sum(int(p.shape[2]) * int(p.shape[3]) for p in p_list) * self.A
        scores = torch.empty((B, n, 2), dtype=torch.float32, device=p0.device)
        deltas = torch.empty((B, n, 4), dtype=torch.float32, device=p0.device)
        xs = [_nhwc(p) for p in p_list]
        if p0.dtype == torch.float16:
            if 6 * self.A > 32 or self.rpn_conv.out_channels > 512:
                raise _no_kernel('RpnHead (more than 5 anchors per cell or more than 512 channels)', self.rpn_conv, p0)
            # the WHOLE head in one launch: the 3x3 convolution of all levels with bias + ReLU + both 1x1 convolutions in its
            # epilogue (ops.rpn_head_fused): the 512-channel activation is never written
            return ops.rpn_head_fused(xs, self.rpn_conv.weight, self.rpn_conv.bias, w, b, self.A, scores, deltas)
        # float32 (the parity mode): the 3x3 convolution of all levels in one launch on exact-float32 matrix instructions,
        # bias + ReLU in its epilogue (ops.conv3x3_f32_levels: the small levels' workgroups fill the tail of the big ones'),
        # the two 1x1 convolutions as the exact-float32 GEMM (weight rows zero-padded to 64), then ONE pass per level adds
        # the bias and writes the level's slices of the concatenated arrays (ops.rpn_pack_pair)
        heads = ops.conv3x3_f32_levels(xs, self.rpn_conv.weight, self.rpn_conv.bias, relu=True)
        off = 0
        for h in heads:
            sd = ops.pointwise(h, rpn_pair_padded(self, w), None)[..., :6 * self.A]
            ops.rpn_pack_pair(sd if sd.is_contiguous() else sd.contiguous(), b, self.A, scores, deltas, off)
            off += int(h.shape[1]) * int(h.shape[2]) * self.A
        return scores, deltas

    @_in_f32_form
    def rpn_trainable(self, p_list):
        """rpn with a backward pass into rpn_conv, rpn_score and rpn_bbox (float32, f32_form 'exact'; model/rpn_trainable.py):
        outputs bit-equal to rpn()'s, and a gradient into those maps of p_list that require one"""
        return rpn_trainable(self, p_list)

    def head_activation(self, roi_features):
        """flatten(7,7,256) -> fc 1024 -> fc 1024 (resnet_fpn.py:292-326): the input of the score / bbox layers; the Dense
        layers on the pointwise GEMM kernel with bias + ReLU in its epilogue"""
        return fc_head_activation(self, roi_features)

    @_in_f32_form
    def roi_head(self, roi_features):
        """RoI features [R,7,7,256] -> (class logits [R,Ccls], box regressions [R,4 Ccls]), float32 (resnet_fpn.py:292-336)"""
        return self._final_outputs(self.head_activation(roi_features))

    @_in_f32_form
    def roi_head_trainable(self, roi_features):
        """roi_head with a backward pass into fc1, fc2, score and bbox (float32, f32_form 'exact'; trainable_common.fc_head_trainable
        with no dropout): the same four layers through ops.dense_trainable, outputs bit-equal to roi_head's.  Features that require
        no gradient (the pooling of the models' own maps without train_neck) cost nothing more: fc1's input gradient -- a read of its
        51 MB of weights -- is then never computed.  Features from ops.roi_pool_trainable require one: fc1's dense_dgrad produces the
        [n,P,P,C] gradient that odet_roi_pool_backward carries into the feature maps, where neck_trainable consumes it."""
        return fc_head_trainable(self, roi_features)

    # ---- the model (the pass: detector_base.Detector) -----------------------------------------------
    def _dense(self, images_nhwc):
        """extractor -> neck -> RPN head: (rpn scores [B,N,2], rpn deltas [B,N,4], contiguous NHWC views of P2..P5)"""
        p_list = self.features(images_nhwc)
        rpn_scores, rpn_deltas = self.rpn(p_list)
        rpn_scores, rpn_deltas = rpn_scores.float().contiguous(), rpn_deltas.float().contiguous()
        # float16 maps go to the RoI kernel as they are, anything else as float32
        if self.dtype == torch.float16:
            maps = [p.permute(0, 2, 3, 1) for p in p_list[:4]]
        else:
            maps = [p.permute(0, 2, 3, 1).float() for p in p_list[:4]]
        return rpn_scores, rpn_deltas, [m if m.is_contiguous() else m.contiguous() for m in maps]

    @staticmethod
    def _maps_of(maps, b):
        return [m[b:b + 1].contiguous() for m in maps]

    def _per_image_to_head(self, B, rpn_scores, rpn_deltas, maps):
        """proposals -> level assignment -> RoI features -> RoI head, image after image"""
        heads = []
        for b in range(B):
            hot = self._hot[b]
            hot.stage_proposals(rpn_scores[b], rpn_deltas[b])
            feats = hot.stage_roi(self._maps_of(maps, b))
            logits, bbox = self.roi_head(feats)
            heads.append((torch.softmax(logits.float(), dim=-1).contiguous(), bbox.float().contiguous()))
        return heads

    def _forward_batched(self, B, rpn_scores, rpn_deltas, maps):
        """the hot path + RoI head + post-ops of B images given the dense parts' outputs"""
        return self._detect(self._hot_to_head(B, rpn_scores, rpn_deltas, maps))
