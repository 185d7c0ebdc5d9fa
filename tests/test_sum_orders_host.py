"""tests/order_data.py proved on the CPU, from the restatements alone: on every data set the header's order and each wrong
order the set lists give DIFFERENT float32 bits in the watched output, everything is finite, and every wrong order of
order_data.TABLE is separated by at least one data set (so tests/test_sum_orders_gpu.py, which asks the GPU for the header's
bytes on the same data, fails for a kernel that sums in any of those orders)."""
import numpy as np
import pytest

import order_data as od

SETS = od.all_sets()


def _id(ds):
    return '%s: %s' % (ds['sum'], ds['name'])


@pytest.mark.parametrize('ds', SETS, ids=_id)
def test_inputs_and_expected_outputs_are_finite(ds):
    for a in od.inputs_of(ds):
        assert np.isfinite(a).all()
    for wrong in [None] + ds['wrong']:
        for k, v in od.expected(ds, wrong).items():
            assert np.isfinite(v).all(), (wrong, k)


@pytest.mark.parametrize('ds', SETS, ids=_id)
def test_every_listed_wrong_order_changes_the_float32_bits(ds):
    want = od.expected(ds)
    assert ds['wrong'] and set(ds['wrong']) <= set(od.TABLE[ds['sum']])
    print()
    for wrong in ds['wrong']:
        got = od.expected(ds, wrong)
        for k in ds['watch']:
            assert got[k].dtype == want[k].dtype == np.float32 and got[k].shape == want[k].shape
            assert got[k].tobytes() != want[k].tobytes(), (wrong, k)
        k = ds['watch'][0]
        print('%-28s %-36s header %s  wrong %s' % (_id(ds)[:28], wrong, want[k].reshape(-1)[:2], got[k].reshape(-1)[:2]))


def test_every_wrong_order_of_the_table_has_a_data_set():
    for row, wrongs in od.TABLE.items():
        for wrong in wrongs:
            sets = [ds for ds in SETS if ds['sum'] == row and wrong in ds['wrong']]
            assert sets, 'no data set separates "%s" of "%s"' % (wrong, row)
    assert {ds['sum'] for ds in SETS} == set(od.TABLE)
    # C > 64: the tie partner and the small terms on either side of column 64
    names = [ds['name'] for ds in SETS if ds['sum'] == 'roi classes C=81']
    assert any('column 70' in n for n in names) and any('column 1' in n for n in names)


def test_the_two_class_sum_needs_no_case():
    """e_0 + e_1 is one float64 addition: commutative, so no RPN data set claims an order of the class sum"""
    assert not any(ds['sum'].startswith('rpn') and 'class' in w for ds in SETS for w in ds['wrong'])
    assert not any('class' in w for row, ws in od.TABLE.items() if row.startswith('rpn') for w in ws)


def test_the_softmax_tie_is_what_construction_b_says():
    z1, zs, zn = od.softmax_tie()
    e1 = od.ln.exp32(z1)
    assert 0.5 <= e1 < 1 and int(round(float(e1) * 2 ** 24)) % 2 == 1
    s = 1.0 + float(e1)
    assert float(np.float32(s)) < s                                     # the tie 1 + e_1 rounds down
    assert float(od.ln.exp32(zs)) < 2.0 ** -53 < 4 * float(od.ln.exp32(zs))
    print('z1 = %r  e1 = %r  1 + e1 -> %r | %r' % (z1, e1, np.float32(s), np.nextafter(np.float32(s), np.float32(2))))
