"""ResNet-C4 Faster R-CNN detector assembled around the HIP hot path -- counterpart of the reference's
model/faster_rcnn/resnet_faster_rcnn.py (ResNetFasterRcnn: extractor conv1..conv4, RoI head = conv5 stack +
global average pool + two dense layers) + the inference branch of model/faster_rcnn/base_faster_rcnn_model.py
(BaseFasterRcnn.call :126-198, RpnHead :309-350).  BASELINE config "ResNet-50 Faster R-CNN, 1x3x800x1333".

Same arrangement as model/fpn_detector.py: the convolutions are genuine dense contractions and run on the matrix cores
through this repository's kernels (NHWC, float32 = parity mode / float16 = throughput mode; no library convolution or GEMM
route, no CPU path); everything between them is FrcnnHotPath (anchors in registers -> [A bg | A fg] softmax -> decode /
clip -> exact NMS over all anchors -> 7x7 crop (ResNet) / 14x14 crop + 2x2 max (VGG16) on the stride-16 map ->
post_ops_prediction).  The pass that strings them together -- prepare, forward, im_detect, the after-pass checks, the
HIP-graph capture -- is detector_base.Detector's, shared with the FPN detector; this file holds what the single-level families
share (`SingleLevelDetector`: the RpnHead, the dense pass, the per-image (`batched=False`) arrangement) and, as siblings under it,
the two networks.  The layer builders and the kernel routing are model/layers.py's; the trainable parts (model/c4_trainable.py,
vgg_trainable.py, rpn_trainable.py) import layers, never this file, and are imported here at the top.  Weights are randomly
initialised with the reference's initialisers (no checkpoints offline), frozen batch-norm folded.  The plain-torch formulation of the
same networks lives with the tests (tests/torch_reference.py)."""
import torch
import torch.nn as nn

from .. import ops
from ..derived import derived
from ..pipeline import FrcnnHotPath, FrcnnStepBatch
from . import c4_trainable, vgg_trainable
from .detector_base import Detector, _in_f32_form
from .layers import _BLOCKS, _conv, _conv_epi, _conv_relu_pool, _fold_frozen_bn, _nhwc, _no_kernel, _patch_gemm, _patch_weight, \
    _stack, _stem, fc_head_activation, init_linears, rpn_head_layers, rpn_pair_padded, rpn_pair_weights
from .rpn_trainable import rpn_trainable
from .trainable_common import fc_head_trainable

__all__ = ['SingleLevelDetector', 'ResNetC4Detector', 'Vgg16Detector']


class SingleLevelDetector(Detector):
    """What the Faster R-CNN families on ONE stride-16 map share (the pass: detector_base.Detector): the RpnHead, the dense pass and the
    arrangements.  Batched: FrcnnStepBatch (odet_fpn_step_t.single_level); per image (`batched=False`): one FrcnnHotPath per image on a
    stream of its own, then ONE RoI-head call for the whole batch.  A family supplies its layers, `features` and `head_activation`."""

    _step_batch_class, _hot_path_class = FrcnnStepBatch, FrcnnHotPath

    def _prepare_per_image(self):
        # the images' RoI features are consecutive blocks of one buffer: the RoI head takes the whole batch at once
        h0 = self._hot[0]
        self._roi_feat_all = torch.zeros((self._max_batch,) + tuple(h0.roi_features.shape), dtype=self._feature_dtype,
                                         device=h0.device)
        for b, h in enumerate(self._hot):
            h.roi_features = self._roi_feat_all[b]
        # one stream per image: the hot path of an image is a chain of small launches (~130 us), the images'
        # chains run beside each other
        self._streams = [torch.cuda.Stream(device=h0.device) for _ in range(self._max_batch)]

    def _per_image(self, B, fn):
        """fn(b) for every image on its own stream; the current stream forks before and joins after (events, no host
        sync -- capturable into a HIP graph).  The tensors fn touches stay referenced by the caller past the join."""
        if B == 1:
            return [fn(0)]
        cur = torch.cuda.current_stream()
        fork = torch.cuda.Event()
        fork.record(cur)
        out = []
        for b in range(B):
            st = self._streams[b]
            st.wait_event(fork)
            with torch.cuda.stream(st):
                out.append(fn(b))
            done = torch.cuda.Event()
            done.record(st)
            cur.wait_event(done)
        return out

    @_in_f32_form
    def rpn(self, c4):
        """RpnHead: scores [B, fh*fw, 2A] ([A bg | A fg] per location), deltas [B, fh*fw*A, 4] (float32)."""
        x = _conv_epi(self.rpn_conv, c4, relu=True)
        B = x.shape[0]
        gran = 64 if x.dtype == torch.float16 else 32
        if x.shape[1] % gran or x.shape[1] < 2 * gran:
            raise _no_kernel('RpnHead 1x1 pair', self.rpn_score, x)
        # the two 1x1 convolutions as ONE contraction on the pointwise GEMM kernel (weight rows zero-padded to 64), then ONE
        # pass: + bias, float32, split (ops.rpn_pack_pair; [fh*fw, 2A] and [fh*fw*A, 2] are the same memory)
        w, b = rpn_pair_weights(self)
        sd = ops.pointwise(_nhwc(x), rpn_pair_padded(self, w), None)[..., :6 * self.A]
        n = int(sd.shape[1]) * int(sd.shape[2]) * self.A
        scores = torch.empty((B, n, 2), dtype=torch.float32, device=x.device)
        deltas = torch.empty((B, n, 4), dtype=torch.float32, device=x.device)
        ops.rpn_pack_pair(sd if sd.is_contiguous() else sd.contiguous(), b, self.A, scores, deltas, 0)
        return scores.view(B, -1, 2 * self.A), deltas

    @_in_f32_form
    def rpn_trainable(self, c):
        """rpn with a backward pass into rpn_conv, rpn_score and rpn_bbox (float32, f32_form 'exact'; model/rpn_trainable.py on
        the one level): outputs bit-equal to rpn()'s with its shapes, and a gradient into ``c`` when it requires one"""
        scores, deltas = rpn_trainable(self, [c])
        return scores.view(scores.shape[0], -1, 2 * self.A), deltas        # ([B,n,2] and [B,fh*fw,2A] are the same memory)

    @_in_f32_form
    def roi_head(self, roi_features):
        """-> (score logits [R,C], box deltas [R,4C]), float32"""
        return self._final_outputs(self.head_activation(roi_features))

    # ---- the model (the pass: detector_base.Detector) -----------------------------------------------
    def _dense(self, images_nhwc):
        """extractor -> RPN head (base_faster_rcnn_model.py:132-153): (rpn scores [B,fh*fw,2A], rpn deltas [B,N,4], the
        contiguous NHWC stride-16 map in the hot path's feature dtype)"""
        c4 = self.features(images_nhwc)
        rpn_scores, rpn_deltas = self.rpn(c4)
        rpn_scores, rpn_deltas = rpn_scores.float().contiguous(), rpn_deltas.float().contiguous()
        maps = c4.permute(0, 2, 3, 1).to(self._feature_dtype)                    # NHWC view (.to: the same tensor when the dtype is)
        return rpn_scores, rpn_deltas, maps.contiguous()

    @staticmethod
    def _maps_of(maps, b):
        return maps[b:b + 1]

    def _per_image_to_head(self, B, rpn_scores, rpn_deltas, maps):
        def proposals_and_crops(b):
            hot = self._hot[b]
            hot.stage_proposals(rpn_scores[b], rpn_deltas[b])
            hot.stage_roi(maps[b:b + 1])
        self._per_image(B, proposals_and_crops)
        K = self._roi_feat_all.shape[1]
        feats = self._roi_feat_all[:B].reshape((B * K,) + tuple(self._roi_feat_all.shape[2:]))
        logits, bbox = self.roi_head(feats)                                      # one head pass for the whole batch
        cls = torch.softmax(logits.float(), dim=-1).reshape(B, K, -1).contiguous()
        bbox = bbox.float().reshape(B, K, -1).contiguous()
        return [(cls[b], bbox[b]) for b in range(B)]


class ResNetC4Detector(SingleLevelDetector):
    """ResNet-{50,101,152} C4 Faster R-CNN (the pass and the RpnHead: SingleLevelDetector; trainable parts:
    model/c4_trainable.py): extractor conv1..conv4, RoI head = conv5 stack on the 7x7 crops + global average pool."""

    def __init__(self, depth=50, num_classes=21, image_shape=(800, 1333), num_proposals=300, dtype=torch.float32,
                 max_batch=1, roi_chunk=0, f32_form='exact', grad_form='exact', **hot_kwargs):
        super().__init__()
        b = _BLOCKS[depth]
        self._declare_modes(dtype, grad_form, f32_form, image_shape, num_classes)
        # extractor (resnet_faster_rcnn.py:104-153): conv1 .. conv4, stride 16
        self.conv1 = _fold_frozen_bn(_conv(3, 64, 7, 2, 0))
        self.conv2 = _stack(64, 64, b[0], 1)
        self.conv3 = _stack(256, 128, b[1], 2)
        self.conv4 = _stack(512, 256, b[2], 2)
        # RPN head (base_faster_rcnn_model.py:309-350); 9 anchors per cell, scores laid out [A bg | A fg]
        self.A = 9
        self.rpn_conv, self.rpn_score, self.rpn_bbox = rpn_head_layers(1024, self.A)
        # RoI head (resnet_faster_rcnn.py:156-183): conv5 stack (stride1 = 1) on the 7x7 crops, GAP, 2 dense
        self.conv5 = _stack(1024, 512, b[3], 1)
        self.score = nn.Linear(2048, num_classes)
        self.bbox = nn.Linear(2048, 4 * num_classes)
        init_linears((self.score, 0.01), (self.bbox, 0.001))
        # config/faster_rcnn_config.py: 'resnet_roi_pooling_max_pooling_flag': False (7x7 crop, no pool) -- what
        # model_factory.py:117 passes, overriding the class default
        self._declare_hot_path(1024, num_proposals, max_batch, hot_kwargs, pool_size=7, max_pooling_flag=False)
        self._roi_chunk = int(roi_chunk)

    # ---- dense parts ---------------------------------------------------------------------------
    @_in_f32_form
    def features(self, images_nhwc):
        """[B,H,W,3] -> C4 [B,1024,ceil(H/16),ceil(W/16)] channels_last (= NHWC in memory)."""
        # conv1_pad + valid 7x7/2, bias + ReLU, pool1_pad (zeros) + 3x3/2 (float16: one launch from the image)
        x = _stem(self.conv1, images_nhwc, self.dtype)
        return self.conv4(self.conv3(self.conv2(x)))

    @_in_f32_form
    def extractor_trainable(self, images_nhwc):
        """features with a backward pass into conv3 and conv4: the output bit-equal to features()'s with its shape and strides;
        conv1 and the conv2 stack run under no_grad and stay frozen (resnet_faster_rcnn.py:109, 139-141)"""
        return c4_trainable.extractor_trainable(self, images_nhwc)

    def head_activation(self, roi_features):
        """[R,7,7,1024] NHWC -> conv5 -> global average pool [R,2048] (resnet_faster_rcnn.py:156-183): the input of the score /
        bbox layers"""
        x = roi_features.permute(0, 3, 1, 2).to(self.dtype)                      # NCHW view of NHWC memory
        R = x.shape[0]
        step = self._roi_chunk if self._roi_chunk > 0 else R
        outs = [self.conv5(x[i:i + step]).mean(dim=(2, 3)) for i in range(0, R, step)]
        return (outs[0] if len(outs) == 1 else torch.cat(outs, 0)).contiguous()

    @_in_f32_form
    def roi_head_trainable(self, roi_features):
        """roi_head with a backward pass into the conv5 stack, score and bbox: all crops in one pass (no `roi_chunk`), the pooling
        in ops.global_avg_pool's stated order -- the logits differ from roi_head's by the pooling's rounding only"""
        return c4_trainable.roi_head_trainable(self, roi_features)


class Vgg16Detector(SingleLevelDetector):
    """VGG16 Faster R-CNN (the pass and the RpnHead: SingleLevelDetector; trainable parts: model/vgg_trainable.py) -- counterpart of model/faster_rcnn/vgg16_faster_rcnn.py
    (Vgg16Extractor :260-342: 13 3x3 'same' convolutions + ReLU, four 2x2/2 'same' max-pools, stride 16;
    Vgg16RoiHead :178-257: flatten(7,7,512) -> fc 4096 -> fc 4096 -> score / boxes) around FrcnnHotPath
    (14x14 crop + 2x2 max on 512 channels).  BASELINE config "VGG16 Faster R-CNN, 1x3x600x800"."""

    _CFG = ((64, 2), (128, 2), (256, 3), (512, 3), (512, 3))

    def __init__(self, num_classes=21, image_shape=(600, 800), num_proposals=300, dtype=torch.float32, max_batch=1,
                 f32_form='exact', grad_form='exact', **hot_kwargs):
        super().__init__()
        self._declare_modes(dtype, grad_form, f32_form, image_shape, num_classes)
        convs, cin = [], 3
        for cout, n in self._CFG:
            for _ in range(n):
                convs.append(_conv(cin, cout, 3, 1, 1))
                cin = cout
        self.convs = nn.ModuleList(convs)
        self.A = 9
        self.rpn_conv, self.rpn_score, self.rpn_bbox = rpn_head_layers(512, self.A)
        self.fc1 = nn.Linear(7 * 7 * 512, 4096)
        self.fc2 = nn.Linear(4096, 4096)
        self.score = nn.Linear(4096, num_classes)
        self.bbox = nn.Linear(4096, 4 * num_classes)
        init_linears((self.fc1, 0.01), (self.fc2, 0.01), (self.score, 0.01), (self.bbox, 0.001))
        self._declare_hot_path(512, num_proposals, max_batch, hot_kwargs, pool_size=7, max_pooling_flag=True)

    def _first_conv(self, images_nhwc):
        """conv1_1 + ReLU from the image, channels_last"""
        first = self.convs[0]
        if not images_nhwc.is_cuda or not images_nhwc.is_contiguous() or first.out_channels != 64:
            raise _no_kernel('first convolution', first, images_nhwc)
        if self.dtype == torch.float16 and images_nhwc.dtype in (torch.float32, torch.float16):
            # conv1_1 straight from the image (ops.conv3x3_rgb: bias + ReLU in the launch, its output written once)
            packed = derived(first, 'rgb_f16', (first.weight,), ops.conv3x3_rgb_pack_weights)
            return ops.conv3x3_rgb(images_nhwc, packed, first.bias, relu=True).permute(0, 3, 1, 2)
        if self.dtype == torch.float32 and images_nhwc.dtype == torch.float32:
            # float32 (parity mode): conv1_1 as the exact-float32 GEMM on its patch matrix (ops.rgb_patches3x3_f32)
            w = derived(first, 'rgb_f32', (first.weight,), lambda weight: _patch_weight(weight, 64))
            Hn, Wn = int(images_nhwc.shape[1]), int(images_nhwc.shape[2])
            return _patch_gemm(images_nhwc, Hn * Wn * 64 * 4, ops.rgb_patches3x3_f32, w, first.bias, True)
        raise _no_kernel('first convolution', first, images_nhwc)

    def _layer_plan(self):
        """(index into convs, pooled) of the convolutions after conv1_1; pooled: a stage's last convolution, with
        MaxPooling2D((2,2), 2, padding='same') behind it (blocks 1-4)"""
        plan, i = [], 0
        for bi, (_, n) in enumerate(self._CFG):
            for k in range(n):
                if i:
                    plan.append((i, k == n - 1 and bi < 4))
                i += 1
        return plan

    def _layer(self, i, pooled, x):
        if pooled:
            # the stage's last convolution: bias + ReLU + MaxPooling2D((2,2), 2, padding='same') in one pass
            return _conv_relu_pool(self.convs[i], x, 2, 2, ceil_mode=True)
        return _conv_epi(self.convs[i], x, relu=True)

    @_in_f32_form
    def features(self, images_nhwc):
        """[B,H,W,3] -> conv5_3 [B,512,ceil(H/16),ceil(W/16)] channels_last."""
        x = self._first_conv(images_nhwc)
        for i, pooled in self._layer_plan():
            x = self._layer(i, pooled, x)
        return x

    @_in_f32_form
    def extractor_trainable(self, images_nhwc):
        """features with a backward pass into block3_conv1 .. block5_conv3 (float32, f32_form 'exact'; model/vgg_trainable.py):
        the output bit-equal to features()'s with its shape and strides; blocks 1-2 run under no_grad and stay frozen"""
        return vgg_trainable.extractor_trainable(self, images_nhwc)

    def head_activation(self, roi_features):
        """flatten(7,7,512) -> fc6 -> fc7 (vgg16_faster_rcnn.py:178-257; dropout: inference): the FC head of model/layers.py"""
        return fc_head_activation(self, roi_features)

    @_in_f32_form
    def roi_head_trainable(self, roi_features, keep_prob=1.0, seed=0, image_id=0):
        """roi_head with a backward pass into fc1, fc2, score and bbox and the reference's two dropouts (float32, f32_form 'exact';
        trainable_common.fc_head_trainable): fc1 -> dropout (stream 6) -> fc2 -> dropout (stream 7) -> score / bbox; with
        keep_prob 1 the outputs are bit-equal to roi_head's"""
        return fc_head_trainable(self, roi_features, keep_prob, seed, image_id)
