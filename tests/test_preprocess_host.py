"""The eval input front end's host side (tf_eager_object_detection_amd/preprocess.py, odet_preprocess_images's argument
checks): the resize rules of the two reference loaders taken literally, the batch checks, the C ABI's argument errors.
No GPU needed."""
import ctypes as C

import numpy as np
import pytest
import torch

from tf_eager_object_detection_amd import preprocess as P


# (h, w) -> (voc rule, coco rule) at min_edge 600 / max_edge 1000
# voc: eval_pascal_tf_dataset.py:41-46 (float64, int()); coco: tf_dataset_utils.py:144-150 (float32, tf.to_int32)
@pytest.mark.parametrize('hw, voc, coco', [
    ((375, 500), (600, 800), (600, 800)),
    ((333, 500), (600, 900), (600, 900)),
    ((500, 375), (800, 600), (800, 600)),
    ((1080, 1920), (562, 1000), (562, 999)),
    ((100, 177), (564, 1000), (564, 999)),
    ((1200, 2000), (600, 1000), (600, 1000)),
    ((1, 1), (600, 600), (600, 600)),
])
def test_resized_shape_table(hw, voc, coco):
    assert P.resized_shape(*hw, pipeline='voc')[:2] == voc
    assert P.resized_shape(*hw, pipeline='coco')[:2] == coco


def test_resized_shape_rules_disagree():
    """at least four sizes where float64 and float32 arithmetic give different shapes (the two loaders differ)"""
    diff = []
    for h in range(100, 1100, 7):
        for w in (177, 1920, 999, 1333, 1501):
            a = P.resized_shape(h, w, pipeline='voc')[:2]
            b = P.resized_shape(h, w, pipeline='coco')[:2]
            if a != b:
                diff.append(((h, w), a, b))
    assert len(diff) >= 4
    assert P.resized_shape(1080, 1920, pipeline='voc')[:2] != P.resized_shape(1080, 1920, pipeline='coco')[:2]
    assert P.resized_shape(100, 177, pipeline='voc')[:2] != P.resized_shape(100, 177, pipeline='coco')[:2]
    # each rule on its own terms: float64 product vs float32 product, both truncated
    for (h, w), a, b in diff[:20]:
        s64 = min(600 / min(h, w), 1000 / max(h, w))
        assert a == (int(s64 * h), int(s64 * w))
        f = np.float32
        s32 = min(f(f(600) / f(min(h, w))), f(f(1000) / f(max(h, w))))
        assert b == (int(f(s32 * f(h))), int(f(s32 * f(w))))


def test_img_scale_types():
    h, w, s = P.resized_shape(375, 500, pipeline='voc')
    assert type(s) is float and s == 1.6
    h, w, s = P.resized_shape(375, 500, pipeline='coco')
    assert isinstance(s, np.float32) and s == np.float32(1.6)


def test_swapped_coco_edges():
    """scripts/eval_coco.py:110-111 passes image_max_size as min_size and image_min_size as max_size: with the COCO
    config's 1000 / 600 the script actually asks for min_edge 1000, max_edge 600 -- the max edge wins, so a landscape
    image's long side is 600."""
    assert P.resized_shape(480, 640, 600, 1000, pipeline='coco')[:2] == (600, 800)
    assert P.resized_shape(480, 640, 1000, 600, pipeline='coco')[:2] == (450, 600)
    assert P.resized_shape(427, 640, 1000, 600, pipeline='coco')[:2] == (400, 600)


def test_group_by_resized_shape():
    ims = [np.zeros((375, 500, 3), np.uint8), np.zeros((333, 500, 3), np.uint8), np.zeros((750, 1000, 3), np.uint8)]
    g = P.group_by_resized_shape(ims)
    assert list(g.items()) == [((600, 800), [0, 2]), ((600, 900), [1])]
    assert P.group_by_resized_shape([(375, 500), (1080, 1920)], pipeline='coco') == {(600, 800): [0], (562, 999): [1]}


def test_preprocess_images_value_errors():
    ok = np.zeros((375, 500, 3), np.uint8)
    with pytest.raises(ValueError, match='different shapes.*600x800: images \\[0\\].*600x900: images \\[1\\]'):
        P.preprocess_images([ok, np.zeros((333, 500, 3), np.uint8)], 'voc')
    with pytest.raises(ValueError, match='uint8'):
        P.preprocess_images([ok.astype(np.float32)], 'voc')
    with pytest.raises(ValueError, match='uint8'):
        P.preprocess_images([torch.zeros((375, 500, 3), dtype=torch.float32)], 'voc')
    with pytest.raises(ValueError, match='3 channels'):
        P.preprocess_images([np.zeros((375, 500, 4), np.uint8)], 'voc')
    with pytest.raises(ValueError, match='3 channels'):
        P.preprocess_images([np.zeros((375, 500), np.uint8)], 'voc')
    with pytest.raises(ValueError):
        P.preprocess_images([ok], 'imagenet')
    with pytest.raises(ValueError):
        P.preprocess_images([ok], 'voc', preprocessing_type='torch')
    with pytest.raises(ValueError, match='voc pipeline only'):
        P.preprocess_images([ok], 'coco', image_format='rgb')
    with pytest.raises(ValueError, match='batch limit'):
        P.preprocess_images([ok] * 65, 'voc')


def _prep(L, B=1, H=600, W=800, images=True, out=True, pipeline=0, preprocessing=0, rgb=0, means=True, w=500, pitch=None):
    keep = np.zeros(16, np.float32)
    ptr = C.c_void_p(keep.ctypes.data)                  # (never dereferenced: every call below fails its checks first)
    n = max(B, 1)
    ims = (C.c_void_p * n)(*([ptr] * n)) if images else None
    hs = (C.c_int * n)(*([375] * n))
    ws = (C.c_int * n)(*([w] * n))
    ps = (C.c_longlong * n)(*([3 * w if pitch is None else pitch] * n))
    m = (C.c_double * 3)(103.939, 116.779, 123.68) if means else None
    return L.odet_preprocess_images(ims, hs, ws, ps, B, H, W, pipeline, preprocessing, rgb, m,
                                    ptr if out else None, 0, None)


def test_abi_argument_errors():
    from tf_eager_object_detection_amd import _lib
    L = _lib.lib()
    INVALID, LIMIT = -1, -4
    assert _prep(L, images=False) == INVALID and b'null pointer' in L.odet_last_error()
    assert _prep(L, out=False) == INVALID and b'null pointer' in L.odet_last_error()
    assert _prep(L, means=False) == INVALID and b'null pointer' in L.odet_last_error()
    assert _prep(L, B=65) == LIMIT and b'exceeds 64' in L.odet_last_error()
    assert _prep(L, B=-1) == INVALID
    assert _prep(L, H=0) == INVALID and b'non-positive output size' in L.odet_last_error()
    assert _prep(L, W=-3) == INVALID and b'non-positive output size' in L.odet_last_error()
    assert _prep(L, H=9000) == LIMIT
    assert _prep(L, pipeline=2) == INVALID
    assert _prep(L, preprocessing=2) == INVALID
    assert _prep(L, pipeline=1, rgb=1) == INVALID                     # (the coco loader has no image_format)
    assert _prep(L, w=5000) == LIMIT
    assert _prep(L, pitch=1499) == INVALID and b'row pitch' in L.odet_last_error()
    # B == 0 is a no-op, whatever the pointers
    assert L.odet_preprocess_images(None, None, None, None, 0, 600, 800, 0, 0, 0, None, None, 0, None) == 0
