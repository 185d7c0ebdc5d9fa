"""The training input stage's host side: the known answers of its numpy restatement (tests/train_input_np.py), the ValueErrors
of preprocess.preprocess_training_batch / model.raw_images.losses_from_raw_images, and odet_preprocess_train's argument
errors through ctypes.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import oracle_np as on
from tf_eager_object_detection_amd import preprocess as P

import train_input_np as ti

F = np.float32


# ---- the restatement's own known answers ----------------------------------------------------------------------------------
def test_box_known_answer_unflipped_and_flipped():
    box = np.array([[0.1, 0.7, 0.9, 1.0]], F)
    np.testing.assert_array_equal(ti.boxes(box, 10, 10, 16, 16, True, False), np.array([[9, 1.5, 15, 12]], F))
    np.testing.assert_array_equal(ti.boxes(box, 10, 10, 16, 16, True, True), np.array([[0, 1.5, 6, 12]], F))


def test_truncation_is_a_float64_product():
    """float32(0.7) * 10: 6.99999988... in float64 (truncates to 6), exactly 7 in float32"""
    assert int(np.float64(F(0.7)) * np.float64(10)) == 6
    assert int(F(F(0.7) * F(10))) == 7
    got = ti.boxes(np.array([[0.0, 0.7, 1.0, 1.0]], F), 10, 10, 11, 11, True, False)
    np.testing.assert_array_equal(got, np.array([[6, 0, 10, 10]], F))            # 6 / 10 * 10, not 7 / 10 * 10


def test_augment_off_takes_the_values_as_they_are():
    box = np.array([[0.1, 0.7, 0.9, 1.0], [1.5, -0.25, 0.5, 0.3]], F)            # (no truncation, no clip, no swap)
    want = np.stack([box[:, 1] * F(15), box[:, 0] * F(15), box[:, 3] * F(15), box[:, 2] * F(15)], axis=1)
    np.testing.assert_array_equal(ti.boxes(box, 10, 10, 16, 16, False, False), want)
    assert want[1, 1] == F(22.5) and want[1, 0] == F(-3.75)


def test_negative_inputs_truncate_toward_zero_and_clip_to_0():
    # -0.05 * 10 = -0.5 -> 0 (toward zero, not floor's -1); -0.35 * 10 = -3.5 -> -3 -> -0.3 -> clipped to 0
    got = ti.boxes(np.array([[-0.05, -0.35, 0.5, 0.5]], F), 10, 10, 11, 11, True, False)
    np.testing.assert_array_equal(got, np.array([[0, 0, 5, 5]], F))
    assert int(np.float64(F(-0.35)) * 10.0) == -3
    # flipped: x' = 10 - (-3) = 13 -> 1.3 -> clipped to 1
    got = ti.boxes(np.array([[-0.05, -0.35, 0.5, 0.5]], F), 10, 10, 11, 11, True, True)
    np.testing.assert_array_equal(got, np.array([[5, 0, 10, 5]], F))


def test_inputs_above_1_clip_to_1():
    got = ti.boxes(np.array([[0.2, 0.2, 1.7, 2.5]], F), 10, 20, 11, 21, True, False)
    np.testing.assert_array_equal(got, np.array([[4, 2, 20, 10]], F))
    got = ti.boxes(np.array([[0.2, 0.2, 1.7, 2.5]], F), 10, 20, 11, 21, True, True)   # (20 - 50, 20 - 4) -> (0, 16)
    np.testing.assert_array_equal(got, np.array([[0, 2, 16, 10]], F))


def test_min_max_swap():
    """imgaug's BoundingBox constructor orders each axis' corners"""
    a = ti.boxes(np.array([[0.9, 0.8, 0.1, 0.3]], F), 10, 10, 11, 11, True, False)
    b = ti.boxes(np.array([[0.1, 0.3, 0.9, 0.8]], F), 10, 10, 11, 11, True, False)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(a, np.array([[3, 1, 8, 8]], F))        # (float32(0.9) * 10 = 8.99999976 -> 8)


@pytest.mark.parametrize('hw, HW, differ, total', [((5, 7), (8, 11), 216, 264), ((4, 6), (3, 5), 45, 45)])
def test_flip_and_resize_do_not_commute(hw, HW, differ, total):
    """TF 1.x resize_bilinear is not mirror-symmetric: flipping after the resize gives other pixels"""
    raw = np.random.default_rng(hw[0] * 100 + hw[1]).integers(0, 256, hw + (3,), dtype=np.uint8)
    first = on.tf_resize_bilinear_legacy(ti.normalise(np.ascontiguousarray(raw[:, ::-1]), 'tf')[None], HW)[0]
    after = on.tf_resize_bilinear_legacy(ti.normalise(raw, 'tf')[None], HW)[0][:, ::-1]
    assert first.size == total
    assert int(np.count_nonzero(first != after)) == differ


def test_flip_flag_is_stream_5_word_0_top_bit():
    import targets_np as tn
    seen = set()
    for seed, image_id in [(0, 0), (1, 7), (2 ** 40 + 3, 2 ** 32 - 1), (12345, 99)]:
        w0 = int(tn.philox((0, image_id, 5, 0), (seed & 0xFFFFFFFF, seed >> 32))[0])
        assert ti.flip_flag(seed, image_id) == bool(w0 >> 31)
        assert P.flip_decision(seed, image_id) == ti.flip_flag(seed, image_id)
        seen.add(ti.flip_flag(seed, image_id))
    flags = [ti.flip_flag(3, i) for i in range(64)]
    assert flags == [P.flip_decision(3, i) for i in range(64)] and 16 < sum(flags) < 48


# ---- the Python functions' ValueErrors ------------------------------------------------------------------------------------
def _ok():
    return np.zeros((375, 500, 3), np.uint8), np.array([[0.1, 0.2, 0.5, 0.6]], F), np.array([3], np.int64)


def test_preprocess_training_batch_value_errors():
    img, bx, lb = _ok()
    T = P.preprocess_training_batch
    with pytest.raises(ValueError, match='different shapes.*600x800: images \\[0\\].*600x900: images \\[1\\]'):
        T([img, np.zeros((333, 500, 3), np.uint8)], [bx, bx], [lb, lb])
    with pytest.raises(ValueError, match='uint8'):
        T([img.astype(np.float32)], [bx], [lb])
    with pytest.raises(ValueError, match='3 channels'):
        T([np.zeros((375, 500), np.uint8)], [bx], [lb])
    with pytest.raises(ValueError, match="'caffe' or 'tf'"):
        T([img], [bx], [lb], preprocessing_type='torch')
    with pytest.raises(ValueError, match='dtype'):
        T([img], [bx], [lb], dtype=torch.float64)
    with pytest.raises(ValueError, match='no images'):
        T([], [], [])
    with pytest.raises(ValueError, match='batch limit'):
        T([img] * 65, [bx] * 65, [lb] * 65)
    with pytest.raises(ValueError, match='lengths must match'):
        T([img, img], [bx], [lb, lb])
    with pytest.raises(ValueError, match='lengths must match'):
        T([img], [bx], [lb, lb])
    with pytest.raises(ValueError, match='lengths must match'):
        T([img], [bx], [lb], flip=[True, False])
    with pytest.raises(ValueError, match='augment=False'):
        T([img], [bx], [lb], augment=False, flip=[False])
    with pytest.raises(ValueError, match='float32'):
        T([img], [bx.astype(np.float64)], [lb])
    with pytest.raises(ValueError, match='\\[G, 4\\]'):
        T([img], [np.zeros((1, 5), F)], [lb])
    with pytest.raises(ValueError, match='\\[G, 4\\]'):
        T([img], [np.zeros(4, F)], [lb])
    with pytest.raises(ValueError, match='integers'):
        T([img], [bx], [lb.astype(np.float32)])
    with pytest.raises(ValueError, match='G = 1 boxes'):
        T([img], [bx], [np.array([1, 2])])
    with pytest.raises(ValueError, match='limit is 1024'):
        T([img], [np.zeros((1025, 4), F)], [np.zeros(1025, np.int32)])
    with pytest.raises(ValueError, match='not finite'):
        T([img], [np.array([[0.1, np.nan, 0.5, 0.6]], F)], [lb])
    with pytest.raises(ValueError, match='3 values'):
        T([img], [bx], [lb], caffe_pixel_means=(1.0, 2.0))
    # torch CPU tensors are host arrays too: the same checks
    with pytest.raises(ValueError, match='float32'):
        T([img], [torch.zeros((1, 4), dtype=torch.float64)], [torch.tensor([1])])


def test_losses_from_raw_images_argument_errors():
    from tf_eager_object_detection_amd.model.raw_images import losses_from_raw_images
    from tf_eager_object_detection_amd.model.base_fpn_model import BaseFPN
    img, bx, lb = _ok()
    with pytest.raises(TypeError, match='caller object'):
        losses_from_raw_images(object(), [img], [bx], [lb])
    m = BaseFPN.__new__(BaseFPN)                          # (never called: every case fails its checks first)
    with pytest.raises(ValueError, match='lengths must match'):
        losses_from_raw_images(m, [img, img], [bx], [lb, lb])
    with pytest.raises(ValueError, match='lengths must match'):
        losses_from_raw_images(m, [img], [bx], [lb], flip=[True, True])
    with pytest.raises(ValueError, match='augment=False'):
        losses_from_raw_images(m, [img], [bx], [lb], augment=False, flip=[True])
    with pytest.raises(ValueError, match='float32'):
        losses_from_raw_images(m, [img], [bx.astype(np.float64)], [lb])


# ---- the C ABI's argument errors (null device pointers: every call fails its checks before any device work) -------------------
def _train(L, B=1, H=600, W=800, images=True, out=True, preprocessing=0, means=True, w=500, pitch=None, offsets=None,
           offsets_ptr=True, offsets_dev=True, boxes=True, boxes_out=True, augment=1, flip=None, f16=0):
    keep = np.zeros(16, np.float32)
    ptr = C.c_void_p(keep.ctypes.data)                  # (never dereferenced)
    n = max(B, 1)
    ims = (C.c_void_p * n)(*([ptr] * n)) if images else None
    hs = (C.c_int * n)(*([375] * n))
    ws = (C.c_int * n)(*([w] * n))
    ps = (C.c_longlong * n)(*([3 * w if pitch is None else pitch] * n))
    m = (C.c_double * 3)(103.939, 116.779, 123.68) if means else None
    off = list(range(n + 1)) if offsets is None else offsets
    offs = (C.c_int * len(off))(*off) if offsets_ptr else None
    fl = None if flip is None else (C.c_int * len(flip))(*flip)
    return L.odet_preprocess_train(ims, hs, ws, ps, B, H, W, preprocessing, m, ptr if boxes else None, offs, augment, fl, 0, 0,
                                   ptr if out else None, f16, ptr if boxes_out else None, ptr if offsets_dev else None,
                                   None, None)


def test_abi_argument_errors():
    from tf_eager_object_detection_amd import _lib
    L = _lib.lib()
    INVALID, LIMIT = -1, -4
    # the limits and argument errors of odet_preprocess_images
    assert _train(L, images=False) == INVALID and b'null pointer' in L.odet_last_error()
    assert _train(L, out=False) == INVALID and b'null pointer' in L.odet_last_error()
    assert _train(L, means=False) == INVALID and b'null pointer' in L.odet_last_error()
    assert _train(L, means=False, preprocessing=1, boxes=False) == INVALID and b'(boxes)' in L.odet_last_error()
    assert _train(L, B=65) == LIMIT and b'exceeds 64' in L.odet_last_error()
    assert _train(L, B=-1) == INVALID
    assert _train(L, H=0) == INVALID and b'non-positive output size' in L.odet_last_error()
    assert _train(L, W=-3) == INVALID and b'non-positive output size' in L.odet_last_error()
    assert _train(L, H=9000) == LIMIT
    assert _train(L, preprocessing=2) == INVALID
    assert _train(L, f16=2) == INVALID
    assert _train(L, w=5000) == LIMIT
    assert _train(L, pitch=1499) == INVALID and b'row pitch' in L.odet_last_error()
    assert L.odet_last_error().startswith(b'odet_preprocess_train:')
    # its own
    assert _train(L, offsets_ptr=False) == INVALID and b'gt_offsets' in L.odet_last_error()
    assert _train(L, offsets_dev=False) == INVALID and b'gt_offsets' in L.odet_last_error()
    assert _train(L, offsets=[1, 2]) == INVALID and b'must be 0' in L.odet_last_error()
    assert _train(L, B=3, offsets=[0, 5, 4, 6]) == INVALID and b'decrease at image 1' in L.odet_last_error()
    assert _train(L, B=2, offsets=[0, 2, 1027]) == LIMIT and b'image 1 has 1025 boxes' in L.odet_last_error()
    assert _train(L, boxes=False) == INVALID and b'(boxes)' in L.odet_last_error()
    assert _train(L, boxes_out=False) == INVALID and b'(boxes)' in L.odet_last_error()
    assert _train(L, augment=0, flip=[0]) == INVALID and b'augment = 0' in L.odet_last_error()
    assert _train(L, augment=2) == INVALID and b'augment must be 0 or 1' in L.odet_last_error()
    assert _train(L, flip=[2]) == INVALID and b'flip[0] = 2' in L.odet_last_error()
    # B == 0 is a no-op, whatever the pointers
    assert L.odet_preprocess_train(None, None, None, None, 0, 600, 800, 0, None, None, None, 1, None, 0, 0, None, 0, None,
                                   None, None, None) == 0
    assert L.odet_version() == 103
