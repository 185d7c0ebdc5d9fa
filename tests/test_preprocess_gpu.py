"""odet_preprocess_images / preprocess_images / detect_raw_images on the GPU: every output element bit-identical (0 ulp) to a
numpy restatement of the reference's eval loaders, written out here:
  voc  = dataset/eval_pascal_tf_dataset.py:32-52: numpy normalisation, then OpenCV's INTER_LINEAR (resize.cpp: the xofs /
         alpha tables of cv::resize, HResizeLinear, VResizeLinear, and the INTER_AREA switch at exactly 2x), then the flip;
  coco = dataset/utils/tf_dataset_utils.py:55-80, 128-155: TF normalisation, then oracle_np.tf_resize_bilinear_legacy."""
import numpy as np
import pytest
import torch

from oracle import oracle_np as on
from tf_eager_object_detection_amd import preprocess as P

pytestmark = pytest.mark.gpu

MEANS = (103.939, 116.779, 123.68)
F = np.float32


def ulp_distance(a, b):
    """element-wise distance of two float32 arrays in units in the last place (0 = identical bits; +0 == -0)"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    ia = a.view(np.int32).astype(np.int64)
    ib = b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, np.int64(-2 ** 31) - ia, ia)
    ib = np.where(ib < 0, np.int64(-2 ** 31) - ib, ib)
    return np.abs(ia - ib)


# ---- the restatement ----------------------------------------------------------------------------------------------------
def cv_resize_linear(img, H, W):
    """cv2.resize(img, (W, H)) of a float32 HWC image, INTER_LINEAR, restated from resize.cpp's scalar paths"""
    h, w = img.shape[:2]
    if w == 2 * W and h == 2 * H:              # INTER_LINEAR -> INTER_AREA (resizeAreaFast_): sum of the 2x2 block * 0.25f
        s = ((img[0::2, 0::2] + img[0::2, 1::2]) + img[1::2, 0::2]) + img[1::2, 1::2]
        return (s * F(0.25)).astype(np.float32)
    scale_x = 1.0 / (W / w)                    # 1 / inv_scale_x, float64
    scale_y = 1.0 / (H / h)
    fx = ((np.arange(W) + 0.5) * scale_x - 0.5).astype(np.float32)
    sx = np.floor(fx).astype(np.int64)
    fx = (fx - sx.astype(np.float32)).astype(np.float32)
    lo = sx < 0
    fx[lo], sx[lo] = 0, 0
    hi = sx >= w - 1
    fx[hi], sx[hi] = 0, w - 1
    sx1 = np.minimum(sx + 1, w - 1)
    a0, a1 = (F(1) - fx)[None, :, None], fx[None, :, None]
    rows = img[:, sx] * a0 + img[:, sx1] * a1                        # HResizeLinear on every source row
    fy = ((np.arange(H) + 0.5) * scale_y - 0.5).astype(np.float32)
    sy = np.floor(fy).astype(np.int64)
    fy = (fy - sy.astype(np.float32)).astype(np.float32)
    r0, r1 = np.clip(sy, 0, h - 1), np.clip(sy + 1, 0, h - 1)       # the row index is clipped, the weights stay
    b0, b1 = (F(1) - fy)[:, None, None], fy[:, None, None]
    return (rows[r0] * b0 + rows[r1] * b1).astype(np.float32)        # VResizeLinear


def restate(raw, pipeline, norm, image_format='bgr', min_edge=600, max_edge=1000):
    """one uint8 HWC image -> (float32 [H, W, 3], img_scale) as the reference loader computes it"""
    h, w = raw.shape[:2]
    if pipeline == 'voc':
        img = raw.astype(np.float32)
        if norm == 'caffe':
            img -= np.array([[MEANS]])                  # float32 -= float64: computed in float64 (:37)
        else:
            img = img / 255.0 * 2.0 - 1.0               # (:39)
        scale = min(min_edge / min(h, w), max_edge / max(h, w))
        img = cv_resize_linear(img, int(scale * h), int(scale * w))
        if image_format == 'rgb':
            img = img[..., ::-1]
        return np.ascontiguousarray(img), float(scale)
    img = raw.astype(np.float32)
    if norm == 'caffe':                                 # _caffe_preprocessing: reverse to BGR, subtract float32 means
        img = img[..., ::-1]
        img = np.stack([img[..., c] - F(MEANS[c]) for c in range(3)], axis=-1)
    else:                                               # convert_image_dtype multiplies by float32(1/255)
        img = (img * F(1.0 / 255)) * F(2.0) - F(1.0)
    hf, wf = F(h), F(w)
    scale = min(F(F(min_edge) / min(hf, wf)), F(F(max_edge) / max(hf, wf)))
    nh, nw = int(F(scale * hf)), int(F(scale * wf))
    return on.tf_resize_bilinear_legacy(img[None], (nh, nw))[0], scale


def _raw(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


COMBOS = [('voc', 'caffe', 'bgr'), ('voc', 'caffe', 'rgb'), ('voc', 'tf', 'bgr'), ('voc', 'tf', 'rgb'),
          ('coco', 'caffe', 'bgr'), ('coco', 'tf', 'bgr')]
SIZES = [(375, 500), (1080, 1920), (1200, 2000), (40, 1000), (1, 1), (333, 517), (97, 61)]


@pytest.mark.parametrize('combo', COMBOS, ids=['-'.join(c) for c in COMBOS])
@pytest.mark.parametrize('hw', SIZES, ids=['%dx%d' % s for s in SIZES])
def test_single_image_bit_exact(combo, hw):
    pipeline, norm, fmt = combo
    raw = _raw(*hw, seed=hw[0] * 7 + hw[1])
    want, scale = restate(raw, pipeline, norm, fmt)
    got, scales, raws = P.preprocess_images([raw], pipeline, norm, image_format=fmt)
    assert tuple(got.shape) == (1,) + want.shape and got.dtype == torch.float32
    assert scales[0] == scale and type(scales[0]) is type(scale) and raws == [hw]
    d = ulp_distance(got[0].cpu().numpy(), want)
    assert d.max() == 0, (np.argwhere(d > 0)[:5], d.max())
    # float16: the float32 result rounded once, to nearest even
    g16 = P.preprocess_images([torch.from_numpy(raw).cuda()], pipeline, norm, image_format=fmt, dtype=torch.float16)[0]
    np.testing.assert_array_equal(g16[0].cpu().numpy().view(np.uint16), want.astype(np.float16).view(np.uint16))


def _batch_sizes(pipeline, target, n):
    """n raw sizes (distinct, odd widths among them) that resize to `target` under the pipeline's rule"""
    out = []
    for h in list(range(150, 1700, 53)) + list(range(151, 1700)):
        for w in (int(round(h * target[1] / target[0])) + d for d in (0, 1, -1)):
            if (h, w) not in out and 0 < w <= 4096 and P.resized_shape(h, w, pipeline=pipeline)[:2] == target:
                out.append((h, w))
                break
        if len(out) == n:
            return out
    raise AssertionError('not enough sizes')


@pytest.mark.parametrize('pipeline, norm, fmt', [('voc', 'caffe', 'bgr'), ('voc', 'tf', 'rgb'), ('coco', 'caffe', 'bgr'),
                                                 ('coco', 'tf', 'bgr')])
@pytest.mark.parametrize('dtype', [torch.float32, torch.float16], ids=['f32', 'f16'])
def test_batch_of_eight_mixed_raw_sizes_and_a_pitched_row(pipeline, norm, fmt, dtype):
    sizes = _batch_sizes(pipeline, (600, 800), 6) + [(1200, 1600), (375, 500)]   # (1200 x 1600: the exact-2x switch in voc)
    assert len(set(sizes)) == 8
    raws = [_raw(h, w, seed=i) for i, (h, w) in enumerate(sizes)]
    ims = [raws[0], torch.from_numpy(raws[1])] + [torch.from_numpy(r).cuda() for r in raws[2:7]]
    # the last source: a GPU view whose rows are 3 * w bytes apart inside a wider buffer (row pitch 3 * (w + 13))
    h, w = sizes[7]
    wide = torch.zeros((h, w + 13, 3), dtype=torch.uint8, device='cuda')
    wide[:, 5:5 + w] = torch.from_numpy(raws[7]).cuda()
    view = wide[:, 5:5 + w]
    assert view.stride() == (3 * (w + 13), 3, 1) and not view.is_contiguous()
    ims.append(view)
    got, scales, rs = P.preprocess_images(ims, pipeline, norm, image_format=fmt, dtype=dtype)
    assert tuple(got.shape) == (8, 600, 800, 3) and got.dtype == dtype and rs == sizes
    g = got.cpu().numpy()
    for i, r in enumerate(raws):
        want, scale = restate(r, pipeline, norm, fmt)
        assert scales[i] == scale
        if dtype == torch.float32:
            assert ulp_distance(g[i], want).max() == 0, (i, sizes[i])
        else:
            np.testing.assert_array_equal(g[i].view(np.uint16), want.astype(np.float16).view(np.uint16))


def test_the_call_captures_into_a_graph():
    """no host sync, no host->device copy: the launch replays from a HIP graph"""
    raws = [torch.from_numpy(_raw(375, 500, s)).cuda() for s in range(4)]
    P.preprocess_images(raws, 'voc')                      # (warm-up: the kernel attributes are set once per device)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s), torch.cuda.graph(g, stream=s):
        out = P.preprocess_images(raws, 'voc')[0]
    torch.cuda.current_stream().wait_stream(s)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    for i in range(4):
        want, _ = restate(raws[i].cpu().numpy(), 'voc', 'caffe')
        assert ulp_distance(out[i].cpu().numpy(), want).max() == 0


def test_float16_stem_from_the_float16_batch_equals_the_float32_batch():
    """the ResNet stem (odet_stem_conv7_pool3_f16) converts a float32 image to float16 itself (v_cvt_pk_f16_f32, round to
    nearest even): feeding it the float16 batch gives the same bits as feeding it the float32 batch"""
    from tf_eager_object_detection_amd.model.layers import _stem
    torch.manual_seed(3)
    conv1 = torch.nn.Conv2d(3, 64, 7, stride=2).cuda().half()
    raws = [_raw(375, 500, s) for s in range(2)]
    b32 = P.preprocess_images(raws, 'voc', dtype=torch.float32)[0]
    b16 = P.preprocess_images(raws, 'voc', dtype=torch.float16)[0]
    assert torch.equal(b32.half(), b16)
    y32 = _stem(conv1, b32, torch.float16)
    y16 = _stem(conv1, b16, torch.float16)
    assert y32.dtype == y16.dtype == torch.float16 and float(y32.float().abs().max()) > 0
    assert torch.equal(y32.contiguous().view(torch.int16), y16.contiguous().view(torch.int16))


# ---- detect_raw_images against the manual chain ---------------------------------------------------------------------------
DET = dict(score_threshold=0.0, iou_threshold=0.5, max_objects_per_class=50, max_objects_per_image=50, min_size=10)


def _same(a, b):
    assert len(a) == len(b)
    n = 0
    for x, y in zip(a, b):
        assert len(x) == len(y)
        for j in range(1, len(x)):
            assert x[j].dtype == y[j].dtype == np.float32 and x[j].shape == y[j].shape
            np.testing.assert_array_equal(x[j], y[j])
            n += x[j].shape[0]
    return n


def test_detect_raw_images_caller_object_matches_the_manual_chain():
    from tf_eager_object_detection_amd.evaluation.pascal_eval import detect_image
    from tf_eager_object_detection_amd.evaluation.raw_images import detect_raw_images
    from tf_eager_object_detection_amd.model.base_fpn_model import ResnetV1Fpn
    torch.manual_seed(1)
    m = ResnetV1Fpn(depth=50, rpn_proposal_num_post_nms_test=300, prediction_score_threshold=0.0)
    raws = [_raw(150, 200, 11), _raw(171, 133, 12)]             # (any size: one image per call)
    edges = dict(min_edge=256, max_edge=352)
    want = []
    for r in raws:
        img, scale = restate(r, 'voc', 'caffe', **edges)
        s, d, rois = m.im_detect(torch.from_numpy(img[None]).cuda(), scale)
        want.append(detect_image(s, d, rois, 1.0, r.shape[0], r.shape[1], **DET))
    got = detect_raw_images(m, raws, 'voc', **edges, **DET)
    assert _same(got, want) > 0


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16], ids=['f32', 'f16'])
def test_detect_raw_images_fast_detector_matches_the_manual_chain(dtype):
    from tf_eager_object_detection_amd.evaluation.pascal_eval import detect_image
    from tf_eager_object_detection_amd.evaluation.raw_images import detect_raw_images
    from tf_eager_object_detection_amd.model.fpn_detector import ResNetFpnDetector
    torch.manual_seed(1)
    det = ResNetFpnDetector(image_shape=(600, 800), max_batch=4, dtype=dtype).prepare()
    raws = [_raw(375, 500, 20 + i) for i in range(4)]
    imgs, scales = zip(*(restate(r, 'voc', 'caffe') for r in raws))
    batch = torch.from_numpy(np.stack(imgs)).cuda().to(dtype)   # (float16: the float32 result rounded once)
    want = [detect_image(s, d, rois, 1.0, 375, 500, **DET) for s, d, rois in det.im_detect(batch, list(scales))]
    got = detect_raw_images(det, raws, 'voc', **DET)
    assert _same(got, want) > 0
    with pytest.raises(ValueError, match='333x500|600x900'):
        detect_raw_images(det, raws[:2] + [_raw(333, 500, 1)], 'voc', **DET)
