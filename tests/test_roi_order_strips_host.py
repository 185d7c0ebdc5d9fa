"""The strip order of the RoIs (d_roi_order_bucket) on the host model of an XCD's L2 (tools/roi_order_model.py): on the
bench's seeded proposals it must save what it was chosen for.  No GPU."""
import numpy as np
import pytest

from tools import roi_order_model as m

IMAGE = (800, 1333)


@pytest.fixture(scope='module')
def model():
    rois, levels, shapes = m.bench_proposals(1234, IMAGE)
    steps, _ = m.cell_steps(m.footprints(rois, levels, shapes, IMAGE), levels, shapes)
    old = m.order_of(m.bucket_bands(rois, levels, IMAGE))
    new = m.order_of(m.bucket_strips(rois, levels, IMAGE))
    return dict(rois=rois, levels=levels, shapes=shapes, steps=steps, old=old, new=new)


def test_new_order_is_a_permutation(model):
    n = len(model['rois'])
    assert n > 0
    np.testing.assert_array_equal(np.sort(model['new']), np.arange(n))
    b = m.bucket_strips(model['rois'], model['levels'], IMAGE)[model['new']]
    assert np.all(np.diff(b) >= 0)
    assert b.min() >= 0 and b.max() < len(model['shapes']) * 256


@pytest.mark.parametrize('K,cells,bound', [(32, 2048, 0.75), (64, 4096, 0.90)])
def test_strips_miss_less_than_bands(model, K, cells, bound):
    old = m.misses(model['steps'], model['old'], K, cells)
    new = m.misses(model['steps'], model['new'], K, cells)
    union = sum(m.union_cells(model['steps'], model['levels'], len(model['shapes'])))
    print('K %d, %d cells: bands %d, strips %d (ratio %.3f), union %d' % (K, cells, old, new, new / old, union))
    assert union <= new                                   # (the floor: every tapped cell is fetched at least once)
    assert new <= bound * old


def test_serpentine_flips_odd_strips():
    # two boxes with the same y, one in strip 0 and one in strip 1 of a 4096 x 4096 image: bins 3 and 31 - 3
    rois = np.float32([[100, 400, 140, 480], [612, 400, 652, 480]])
    b = m.bucket_strips(rois, np.zeros(2, np.int64), (4096, 4096))
    assert b.tolist() == [0 * 32 + 3, 1 * 32 + 28]
    # the clamp: a centre on the right / bottom edge is strip 7 (odd: bin 31 -> 0)
    edge = np.float32([[4096, 4096, 4096, 4096]])
    assert m.bucket_strips(edge, np.zeros(1, np.int64), (4096, 4096)).tolist() == [7 * 32 + 0]
