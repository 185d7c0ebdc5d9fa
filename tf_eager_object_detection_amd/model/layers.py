"""The layer builders and the kernel routing of the assembled detectors (model/fpn_detector.py, model/frcnn_detector.py) and of
their trainable parts.  The dense conv / FC stacks are genuine dense contractions and run on the matrix cores through THIS
REPOSITORY'S kernels -- there is no library convolution or GEMM route here, at any batch size, and no CPU path (a layer no
kernel takes raises):

  3x3 convolutions   ops.conv3x3_f16 / conv3x3_f32 (implicit GEMM; the ring form at batch 1-2 on the small maps), with the
                     block's last 1x1 convolution + shortcut + ReLU in the same launch where the map is large enough
                     (ops.conv3x3_conv1x1_f16), with the RpnHead's two 1x1 convolutions in the launch (ops.rpn_head_fused)
  1x1 / dense        ops.pointwise / dense (the same kernel with one tap; strided; two sources along K for a stage's first
                     block; the FPN top-down merge in the lateral's epilogue), ops.conv1x1_f16 (register-resident, short K)
  stem               ops.stem_conv7_pool3 (float16: one launch from the image) / the patch-matrix GEMM (float32)

Imports ops and derived only: every model file may import it."""
import math

import torch
import torch.nn as nn

from .. import ops
from ..derived import derived

_BLOCKS = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3), 152: (3, 8, 36, 3)}
_BN_EPS = 1.001e-5


def _pad_rows64(t):
    """t [rows, ...] with zero rows up to the next multiple of 64 (the GEMM kernel's output-channel granule)"""
    out = torch.zeros(((int(t.shape[0]) + 63) // 64 * 64,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    out[:t.shape[0]] = t
    return out


def _nhwc(x):
    """the NHWC memory of a channels_last [B,C,H,W] tensor as a contiguous [B,H,W,C] view"""
    y = x.permute(0, 2, 3, 1)
    return y if y.is_contiguous() else y.contiguous()


def _conv(cin, cout, k, stride=1, padding=0, std=None):
    c = nn.Conv2d(cin, cout, k, stride=stride, padding=padding, bias=True)
    if std is None:
        nn.init.kaiming_normal_(c.weight, mode='fan_in', nonlinearity='relu')     # keras 'he_normal'
    else:
        nn.init.normal_(c.weight, 0.0, std)                                       # tf.random_normal_initializer
    nn.init.zeros_(c.bias)
    return c


def rpn_head_layers(cin, A):
    """the RpnHead's (rpn_conv, rpn_score, rpn_bbox) for A anchors per cell, created and initialised in this order"""
    return _conv(cin, 512, 3, 1, 1, std=0.01), _conv(512, 2 * A, 1, std=0.01), _conv(512, 4 * A, 1, std=0.001)


def init_linears(*pairs):
    """tf.random_normal_initializer(stddev=std) weights and zero biases for every (Linear, std), in the given order"""
    for m, std in pairs:
        nn.init.normal_(m.weight, 0.0, std)
        nn.init.zeros_(m.bias)


def _fold_frozen_bn(conv):
    """keras BatchNormalization(trainable=False)(x, training=False) with fresh statistics
    (gamma 1, beta 0, mean 0, var 1) is a multiplication by 1/sqrt(1 + eps): folded into the conv."""
    s = 1.0 / math.sqrt(1.0 + _BN_EPS)
    with torch.no_grad():
        conv.weight.mul_(s)
        conv.bias.mul_(s)
    return conv


def _no_kernel(what, conv, x):
    return RuntimeError('%s: no kernel of this package takes the layer (kernel %s, stride %s, %d -> %d channels, input %s %s on '
                        '%s); the detectors run float16 / float32 NHWC maps on the GPU and have no library or CPU route'
                        % (what, tuple(conv.kernel_size), tuple(conv.stride), conv.in_channels, conv.out_channels,
                           tuple(x.shape), x.dtype, x.device))


def _mfma_ok(conv, x):
    """ops.conv1x1_f16 (register-resident operand, weights staged per 64-channel group) takes this 1x1 stride-1 convolution"""
    return (x.is_cuda and x.dtype == torch.float16 and tuple(conv.kernel_size) == (1, 1) and tuple(conv.stride) == (1, 1)
            and tuple(conv.padding) == (0, 0) and conv.in_channels in (64, 128, 256, 512) and conv.out_channels % 64 == 0)


def _pw_ok(conv, x):
    """the pointwise GEMM kernel takes this 1x1 convolution (stride 1 or 2, no padding)"""
    if not x.is_cuda or x.dtype not in (torch.float16, torch.float32):
        return False
    gran = 64 if x.dtype == torch.float16 else 32          # channels per K-step
    return (tuple(conv.kernel_size) == (1, 1) and tuple(conv.padding) == (0, 0)
            and tuple(conv.stride) in ((1, 1), (2, 2)) and conv.in_channels % gran == 0 and conv.in_channels >= 2 * gran
            and conv.out_channels % 64 == 0)


def _route_1x1(conv, x):
    """'mfma' (ops.conv1x1_f16) or 'pw' (ops.pointwise) for this 1x1 convolution.  A fixed rule (the two kernels differ in
    rounding order, so the route must not depend on timing): the LDS-staged GEMM wherever it applies (K >= 128; every first
    1x1 of a bottleneck, the last one with its shortcut, the neck's P5, strided layers, float32) except for 64-channel
    outputs, which -- like the K = 64 layers the GEMM does not take -- go to the register-resident kernel
    (tools/exp/pointwise_layers.py; round 4, cold L2, inside a HIP graph: conv4's last 1x1 with its shortcut at batch 1 / 4
    12.1 / 20.5 us on the GEMM, 13.3 / 30.9 on the register-resident kernel, tools/r04/small_tiles.py)."""
    mfma, pw = _mfma_ok(conv, x), _pw_ok(conv, x)
    if mfma and (conv.out_channels <= 64 or not pw):
        return 'mfma'
    if pw:
        return 'pw'
    raise _no_kernel('1x1 convolution', conv, x)


def _own_conv3x3(conv, x):
    """the implicit-GEMM kernel (ops.conv3x3_f16 / conv3x3_f32) takes this 3x3 stride-1 'same' convolution: float16 with
    cin % 64 == 0 and cout % 64 == 0, float32 with cin % 32 == 0 and cout % 64 == 0 -- at every map size (the launcher picks
    the workgroup tile: 128 .. 256-pixel slabs, or the 64 x 64 ring form when the map has few pixels)"""
    if not x.is_cuda or x.dtype not in (torch.float16, torch.float32):
        return False
    if tuple(conv.kernel_size) != (3, 3) or tuple(conv.stride) != (1, 1) or tuple(conv.padding) != (1, 1):
        return False
    gran = 64 if x.dtype == torch.float16 else 32
    return conv.in_channels % gran == 0 and conv.out_channels % 64 == 0


# A fused bottleneck tail (3x3 + last 1x1 + shortcut + ReLU in one launch) pays from this many 128-pixel slabs on: its
# workgroup must hold ALL middle channels of its pixels, so a small map makes few workgroups (conv4 at batch 1 / 4: 33 /
# 132 on 256 CUs) and the two launches -- 3x3 with its epilogue (ring tiles at batch 1), then the 1x1 GEMM with the shortcut
# in its epilogue -- win: conv4 30.4 vs 53.0 us at batch 1, 48.5 vs 53.0 at batch 2, 55.5 vs 59.0 at batch 4; at batch 8 (263
# slabs) the fused launch: 84.1 vs 90.7; conv3 (cmid 128) at batch 2 / 263 slabs: 33.9 vs 39.6; conv2 from batch 1 on
# (tools/r04/small_tiles.py --only tail, cold L2, inside a HIP graph; profiles/r04_small_tiles_tail.json)
_FUSED_TAIL_MIN_SLABS = 200

# the float32 mode's patch matrices (stem, VGG16's first convolution) are addressed with 32-bit byte offsets
_PATCH_BYTES_MAX = ops.PATCH_BYTES_MAX


_patch_weight = ops.patch_weight


def _patch_gemm(images_nhwc, per_image, patches, w, bias=None, relu=False, tail=None):
    """tail?(ops.pointwise(patches(images), w, bias, relu)) as a channels_last [B,C,h,w] map.  The patch matrix (`per_image` bytes
    an image) is addressed with 32-bit byte offsets: the images go through in groups that keep it below 4 GiB"""
    B = int(images_nhwc.shape[0])
    step = max(1, min(B, _PATCH_BYTES_MAX // per_image))
    parts = []
    for i in range(0, B, step):
        y = ops.pointwise(patches(images_nhwc[i:i + step]), w, bias, None, relu)
        parts.append(y if tail is None else tail(y))
    y = parts[0] if len(parts) == 1 else torch.cat(parts, 0)
    return y.permute(0, 3, 1, 2)


def _stem(conv1, images_nhwc, dtype):
    """conv1_pad + 7x7/2 'valid' + folded BN + ReLU + pool1_pad + 3x3/2 max-pooling (resnet_fpn.py:262-289).  float16: ONE
    launch from the image (ops.stem_conv7_pool3: the 64-channel convolution output, 273 MB at batch 8, never goes to
    memory); float32 (parity mode): the 7x7 / 2 convolution as the exact-float32 GEMM on its patch matrix
    (ops.stem_patches_f32: 160 floats per output pixel), then bias + ReLU + the 3x3 / 2 pooling in one pass."""
    ok = (images_nhwc.is_cuda and images_nhwc.is_contiguous() and conv1.out_channels == 64
          and tuple(conv1.kernel_size) == (7, 7) and tuple(conv1.stride) == (2, 2))
    if ok and dtype == torch.float16 and images_nhwc.dtype in (torch.float32, torch.float16):
        packed = derived(conv1, 'stem_f16', (conv1.weight,), ops.stem_pack_weights)
        return ops.stem_conv7_pool3(images_nhwc, packed, conv1.bias).permute(0, 3, 1, 2)
    if ok and dtype == torch.float32 and images_nhwc.dtype == torch.float32:
        w = derived(conv1, 'stem_f32', (conv1.weight,), lambda weight: _patch_weight(weight, 160))
        H, W = int(images_nhwc.shape[1]), int(images_nhwc.shape[2])
        per_image = ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1) * 160 * 4
        return _patch_gemm(images_nhwc, per_image, ops.stem_patches_f32, w,
                           tail=lambda y: ops.bias_relu_maxpool(y, conv1.bias, 3, 2, 1, False))
    raise _no_kernel('stem', conv1, images_nhwc)


def _conv_relu_pool(conv, x, kernel, stride, pool_pad=0, ceil_mode=False):
    """max_pool(relu(conv3x3(x) + bias)) (vgg16_faster_rcnn.py:260-342).  float16 with the 2x2 / 2 'same' pooling: in the
    convolution's own launch (its pixel order makes a pooling window four neighbouring lanes: the un-pooled map is never
    written); otherwise the convolution without its epilogue, then ONE pass (ops.bias_relu_maxpool) that reads its output
    once and writes the pooled map."""
    if not _own_conv3x3(conv, x) or conv.bias is None:
        raise _no_kernel('3x3 convolution + pooling', conv, x)
    if x.dtype == torch.float16 and kernel == 2 and stride == 2 and pool_pad == 0 and ceil_mode:
        return ops.conv3x3_relu_pool2_f16(_nhwc(x), conv.weight, conv.bias).permute(0, 3, 1, 2)
    yn = (ops.conv3x3_f32 if x.dtype == torch.float32 else ops.conv3x3_f16)(_nhwc(x), conv.weight)
    return ops.bias_relu_maxpool(yn, conv.bias, kernel, stride, pool_pad, ceil_mode).permute(0, 3, 1, 2)


def _conv_epi(conv, x, relu=False, residual=None, extra_bias=None):
    """conv -> + bias (+ extra_bias) (+ residual) -> ReLU in ONE launch of this package's kernels; x / residual / result are
    channels_last [B,C,H,W] tensors (= NHWC in memory)."""
    bias = conv.bias if extra_bias is None else conv.bias + extra_bias
    if tuple(conv.kernel_size) == (1, 1):
        res = None if residual is None else _nhwc(residual)
        xn = _nhwc(x)
        if _route_1x1(conv, x) == 'mfma':
            return ops.conv1x1_f16(xn, conv.weight, bias, res, relu).permute(0, 3, 1, 2)
        return ops.pointwise(xn, conv.weight, bias, res, relu, conv.stride[0]).permute(0, 3, 1, 2)
    if residual is None and _own_conv3x3(conv, x):
        # the implicit GEMM with bias (+ ReLU) in its epilogue
        fn = ops.conv3x3_f32 if x.dtype == torch.float32 else ops.conv3x3_f16
        return fn(_nhwc(x), conv.weight, bias, relu=relu).permute(0, 3, 1, 2)
    raise _no_kernel('convolution', conv, x)


class _Block(nn.Module):
    """reference resnet_fpn.py:154-205 block1 (bottleneck, stride on the first 1x1)."""

    def __init__(self, cin, filters, stride, conv_shortcut):
        super().__init__()
        self.short = _fold_frozen_bn(_conv(cin, 4 * filters, 1, stride)) if conv_shortcut else None
        self.c1 = _fold_frozen_bn(_conv(cin, filters, 1, stride))
        self.c2 = _fold_frozen_bn(_conv(filters, filters, 3, 1, 1))
        self.c3 = _fold_frozen_bn(_conv(filters, 4 * filters, 1))
        # Random initialisation only (there are no checkpoints offline): with fresh batch-norm statistics
        # a he_normal residual branch doubles the activation variance per block and 33 blocks overflow
        # fp16; damping the last conv of the branch keeps the random network's activations O(1).
        with torch.no_grad():
            self.c3.weight.mul_(0.2)

    def _dual_weights(self):
        """[w3 | w_shortcut] along K and b3 + b_shortcut (ops.pointwise_dual), derived from the four parameters"""
        def build(*ps):
            with torch.no_grad():
                n = self.c3.out_channels
                w = torch.cat([ps[0].reshape(n, -1), ps[2].reshape(n, -1)], 1).contiguous()
                b = (ps[1].float() + ps[3].float()).to(ps[1].dtype).contiguous()
            return w, b
        return derived(self, 'dual', (self.c3.weight, self.c3.bias, self.short.weight, self.short.bias), build)

    def forward(self, x):
        y = _conv_epi(self.c1, x, relu=True)
        if self.short is not None:
            # a stage's first block: the last 1x1 convolution AND the convolutional shortcut + Add + ReLU as ONE contraction
            # over [c2's output | the block's (strided) input] with the weights concatenated along K (ops.pointwise_dual) --
            # the shortcut map is never written or re-read, one launch instead of two
            gran = 64 if x.dtype == torch.float16 else 32
            if (self.c3.in_channels % gran or self.short.in_channels % gran or self.c3.out_channels % 64
                    or tuple(self.short.stride) not in ((1, 1), (2, 2))):
                raise _no_kernel('bottleneck with a convolutional shortcut', self.short, x)
            y = _conv_epi(self.c2, y, relu=True)
            w, b = self._dual_weights()
            return ops.pointwise_dual(_nhwc(y), _nhwc(x), w, b, self.short.stride[0], relu=True).permute(0, 3, 1, 2)
        # Add([shortcut, x]) + ReLU ride on c3's epilogue
        if y.dtype == torch.float16 and _own_conv3x3(self.c2, y) and self.c2.out_channels in (64, 128, 256):
            m = int(y.shape[0]) * int(y.shape[2]) * int(y.shape[3])
            if (m + 127) // 128 >= _FUSED_TAIL_MIN_SLABS:
                # the 3x3 convolution AND the block's last 1x1 convolution + bias + shortcut + ReLU in one launch
                # (ops.conv3x3_conv1x1_f16: the 64 / 128 / 256-channel activation between them stays in LDS): conv4 83 vs
                # 108 us at batch 8 (253 vs 320 at 30), conv3 122 vs 134 (400 vs 477), conv2 198 vs 226 (640-700 vs 787)
                out = ops.conv3x3_conv1x1_f16(_nhwc(y), self.c2.weight, self.c2.bias, self.c3.weight, self.c3.bias,
                                              residual=_nhwc(x), relu=True)
                return out.permute(0, 3, 1, 2)
        y = _conv_epi(self.c2, y, relu=True)
        return _conv_epi(self.c3, y, relu=True, residual=x)


def _stack(cin, filters, blocks, stride1):
    layers = [_Block(cin, filters, stride1, True)]
    for _ in range(blocks - 1):
        layers.append(_Block(4 * filters, filters, 1, False))
    return nn.Sequential(*layers)


def tf_legacy_resize_bilinear(x, out_hw):
    """tf.image.resize_bilinear(x, size) of TF 1.x with align_corners=False (resnet_fpn.py:385-398):
    source coordinate = destination index * (in / out), top/left = floor, bottom/right = min(+1, in-1).
    x: [B,C,H,W] (any memory format)."""
    B, C, H, W = x.shape
    oh, ow = int(out_hw[0]), int(out_hw[1])
    dev = x.device
    ys = torch.arange(oh, device=dev, dtype=torch.float32) * (float(H) / float(oh))
    xs = torch.arange(ow, device=dev, dtype=torch.float32) * (float(W) / float(ow))
    y0 = ys.floor().long().clamp_(max=H - 1)
    x0 = xs.floor().long().clamp_(max=W - 1)
    y1 = (y0 + 1).clamp_(max=H - 1)
    x1 = (x0 + 1).clamp_(max=W - 1)
    wy = (ys - y0.float()).to(x.dtype).view(1, 1, oh, 1)
    wx = (xs - x0.float()).to(x.dtype).view(1, 1, 1, ow)
    top = x[:, :, y0, :]
    bot = x[:, :, y1, :]
    tl, tr = top[:, :, :, x0], top[:, :, :, x1]
    bl, br = bot[:, :, :, x0], bot[:, :, :, x1]
    t = tl + (tr - tl) * wx
    b = bl + (br - bl) * wx
    return t + (b - t) * wy


def rpn_pair_weights(m):
    """[6A, 512, 1, 1] weight and [6A] bias of m.rpn_score and m.rpn_bbox concatenated along the output channel
    (the RpnHead's two 1x1 convolutions as one contraction); derived on the module: rebuilt when a parameter
    was modified (weight loading, an optimiser step) or moved."""
    def build(*ps):
        with torch.no_grad():
            w = torch.cat([ps[0], ps[2]], 0).contiguous(memory_format=torch.channels_last)
            b = torch.cat([ps[1], ps[3]], 0).contiguous()
        return w, b
    return derived(m, 'rpn_pair', (m.rpn_score.weight, m.rpn_score.bias, m.rpn_bbox.weight, m.rpn_bbox.bias), build)


def rpn_pair_padded(m, w):
    """the concatenated [6A, cin, 1, 1] RpnHead weight (rpn_pair_weights' own tensor) as [64 k, cin] with zero rows"""
    def build(w):
        with torch.no_grad():
            return _pad_rows64(w.reshape(w.shape[0], -1))
    return derived(m, 'rpn_pad', (w,), build)


def fc_head_activation(det, roi_features):
    """flatten(7,7,C) -> fc1 -> fc2 (resnet_fpn.py:292-326, vgg16_faster_rcnn.py:178-257 with its dropouts at inference): the input
    of the score / bbox layers; the Dense layers on the pointwise GEMM kernel with bias + ReLU in its epilogue"""
    x = roi_features.reshape(roi_features.shape[0], -1).to(det.dtype)            # Flatten() of NHWC crops
    x = ops.dense(x if x.is_contiguous() else x.contiguous(), det.fc1.weight, det.fc1.bias, relu=True)
    return ops.dense(x, det.fc2.weight, det.fc2.bias, relu=True)
