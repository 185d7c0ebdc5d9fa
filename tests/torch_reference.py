"""Plain-torch formulations of the detectors' dense parts (library convolutions / GEMMs on whatever device the module lives
on): the CPU shape-bookkeeping tests and the numerical reference of the GPU tests.  The product package has no such route
(tf_eager_object_detection_amd/model/*_detector.py run this repository's kernels only); these functions take the SAME
modules -- hence the same folded weights -- and restate what the reference's Keras layers compute
(model/fpn/resnet_fpn.py:154-289, 339-407; base_fpn_model.py:393-434; faster_rcnn/resnet_faster_rcnn.py:31-185;
faster_rcnn/vgg16_faster_rcnn.py:260-342; base_faster_rcnn_model.py:309-350)."""
import torch
import torch.nn.functional as F

from tf_eager_object_detection_amd.model.layers import tf_legacy_resize_bilinear


def block(blk, x):
    """resnet_fpn.py:154-205 block1: 1x1 (stride) -> 3x3 -> 1x1, (convolutional) shortcut, Add, ReLU; frozen BN folded"""
    sc = x if blk.short is None else blk.short(x)
    y = F.relu(blk.c1(x))
    y = F.relu(blk.c2(y))
    return F.relu(blk.c3(y) + sc)


def stack(seq, x):
    for blk in seq:
        x = block(blk, x)
    return x


def resnet_stem(conv1, images_nhwc, dtype):
    """conv1_pad (3) + 7x7/2 'valid' + BN + ReLU + pool1_pad (1, zeros) + 3x3/2 max-pooling (resnet_fpn.py:262-289)"""
    x = images_nhwc.to(dtype).permute(0, 3, 1, 2)
    x = F.relu(F.conv2d(F.pad(x, (3, 3, 3, 3)), conv1.weight, conv1.bias, 2))
    return F.max_pool2d(F.pad(x, (1, 1, 1, 1)), 3, 2)


def fpn_features(m, images_nhwc):
    """ResNetFpnDetector.features in plain torch: (P2..P6), NCHW"""
    x = resnet_stem(m.conv1, images_nhwc, m.dtype)
    c2 = stack(m.conv2, x)
    c3 = stack(m.conv3, c2)
    c4 = stack(m.conv4, c3)
    c5 = stack(m.conv5, c4)
    p5 = m.p5(c5)
    p6 = p5[:, :, ::2, ::2]

    def merge(top, lateral):
        return tf_legacy_resize_bilinear(top, lateral.shape[2:]) * 0.5 + lateral * 0.5
    p4 = merge(p5, m.l4(c4))
    p3 = merge(p4, m.l3(c3))
    p2 = merge(p3, m.l2(c2))
    return m.s2(p2), m.s3(p3), m.s4(p4), p5, p6


def fpn_rpn(m, p_list):
    """shared RpnHead on every level, concatenated P2->P6 in (y, x, anchor) order (base_fpn_model.py:188-200, 427-432)"""
    scores, deltas = [], []
    for p in p_list:
        x = F.relu(m.rpn_conv(p))
        B = x.shape[0]
        scores.append(m.rpn_score(x).permute(0, 2, 3, 1).reshape(B, -1, 2))
        deltas.append(m.rpn_bbox(x).permute(0, 2, 3, 1).reshape(B, -1, 4))
    return torch.cat(scores, 1), torch.cat(deltas, 1)


def fpn_roi_head(m, roi_features):
    x = roi_features.reshape(roi_features.shape[0], -1).to(m.dtype)
    x = F.relu(m.fc2(F.relu(m.fc1(x))))
    return m.score(x), m.bbox(x)


def c4_features(m, images_nhwc):
    """ResNetC4Detector.features: conv1 .. conv4 (resnet_faster_rcnn.py:104-153)"""
    x = resnet_stem(m.conv1, images_nhwc, m.dtype)
    return stack(m.conv4, stack(m.conv3, stack(m.conv2, x)))


def frcnn_rpn(m, feat):
    """RpnHead of the single-level models: scores [B, fh*fw, 2A] ([A bg | A fg]), deltas [B, fh*fw*A, 4]"""
    x = F.relu(m.rpn_conv(feat))
    B = x.shape[0]
    scores = m.rpn_score(x).permute(0, 2, 3, 1).reshape(B, -1, 2 * m.A)
    deltas = m.rpn_bbox(x).permute(0, 2, 3, 1).reshape(B, -1, 4)
    return scores, deltas


def vgg16_features(m, images_nhwc):
    """Vgg16Detector.features: 13 3x3 'same' convolutions + ReLU, four 2x2/2 'same' max-pools (vgg16_faster_rcnn.py:260-342)"""
    x = images_nhwc.to(m.dtype).permute(0, 3, 1, 2)
    i = 0
    for bi, (_, n) in enumerate(m._CFG):
        for k in range(n):
            x = F.relu(m.convs[i](x))
            if k == n - 1 and bi < 4:
                x = F.max_pool2d(x, 2, 2, ceil_mode=True)
            i += 1
    return x
