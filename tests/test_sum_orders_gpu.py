"""The ordered sums of the training kernels on data where the order SHOWS (tests/order_data.py; the separation is proved on the
CPU by tests/test_sum_orders_host.py): odet_rpn_loss, odet_roi_loss and the L2 sum of odet_l2_loss / odet_opt_step against the
restatements by BYTES.  No unit in the last place is allowed behind exp / log here -- the orders differ by exactly one -- which
is why the builders keep every exponential and logarithm away from a float32 rounding boundary."""
import numpy as np
import pytest
import torch

import optimizer_np as onp
import order_data as od

pytestmark = pytest.mark.gpu
CH = onp.CH
f32 = np.float32


def _id(ds):
    return '%s: %s' % (ds['sum'], ds['name'])


def _same(what, got, want):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), '%s: got %s, the header\'s order gives %s' % (
        what, got.reshape(-1)[:4], want.reshape(-1)[:4])


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))).cuda()


@pytest.mark.parametrize('ds', od.rpn_sets(), ids=_id)
def test_rpn_loss_sums_in_the_headers_order(ds):
    from tf_eager_object_detection_amd import ops
    want = od.expected(ds)
    got = ops.rpn_losses(_dev(ds['scores'][None]), _dev(ds['deltas'][None]), _dev(ds['sample_idx'][None]),
                         _dev(ds['sample_targets'][None]), _dev(ds['counts'][None]), ds['sigma'], ds['layout'], ds['A'])
    torch.cuda.synchronize()
    print('\n%s: losses %s' % (_id(ds), got.losses[0].tolist()))
    for k in ('losses', 'row_grad_scores', 'row_grad_deltas'):
        _same('%s %s' % (_id(ds), k), getattr(got, k)[0], want[k])


@pytest.mark.parametrize('ds', od.roi_sets(), ids=_id)
def test_roi_loss_sums_in_the_headers_order(ds):
    from tf_eager_object_detection_amd import ops
    want = od.expected(ds)
    rm = None if ds['row_map'] is None else _dev(ds['row_map'][None])
    got = ops.roi_losses(_dev(ds['scores'][None]), _dev(ds['deltas'][None]), _dev(ds['labels'][None]), _dev(ds['targets'][None]),
                         _dev(ds['inside'][None]), _dev(ds['outside'][None]), _dev(ds['counts'][None]), ds['sigma'], row_map=rm)
    torch.cuda.synchronize()
    print('\n%s: losses %s' % (_id(ds), got.losses[0].tolist()))
    for k in ('losses', 'grad_scores', 'grad_deltas'):
        _same('%s %s' % (_id(ds), k), getattr(got, k)[0], want[k])


def _offset_view(a):
    """the same values as a view one element into a larger buffer: 4-byte aligned, the kernel's scalar path"""
    buf = torch.zeros(a.size + 4, dtype=torch.float32, device='cuda')
    v = buf[1:1 + a.size]
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 != 0
    return v


def _l2_four_ways(ds):
    from tf_eager_object_detection_amd import training
    want = od.expected(ds)['tensor_loss']
    rng = np.random.default_rng(5)
    others = [rng.normal(0, 1, n).astype(f32) for n in (3, CH + 1)]
    ways = (('aligned, alone', lambda: [_dev(ds['w'])], 0),
            ('aligned, third of a list', lambda: [_dev(others[0]), _dev(others[1]), _dev(ds['w'])], 2),
            ('offset view, alone', lambda: [_offset_view(ds['w'])], 0),
            ('offset view, second of a list', lambda: [_dev(others[1]), _offset_view(ds['w'])], 1))
    print()
    for how, make, pos in ways:
        variables = make()
        assert (variables[pos].data_ptr() % 16 == 0) == how.startswith('aligned')
        wds = [1e-4] * len(variables)
        wds[pos] = ds['wd']
        out = training.MomentumOptimizer(0.01, 0.9).l2_loss(variables, wds)
        torch.cuda.synchronize()
        print('%s, %s: %r' % (ds['name'], how, float(out.tensor_l2_losses[pos])))
        _same('%s, %s' % (ds['name'], how), out.tensor_l2_losses[pos].reshape(1), want)
        per = [onp.l2_loss(v.cpu().numpy(), wd) for v, wd in zip(variables, wds)]
        _same('%s, %s: total' % (ds['name'], how), out.l2_loss.reshape(1), np.array([onp.add_n(per)], f32))
        # the same sum from the fused step (the update kernel's L2 output is of the PRE-update values)
        for opt in (training.MomentumOptimizer(0.01, 0.9), training.AdamOptimizer(1e-3)):
            variables = make()
            grads = [torch.zeros_like(v) for v in variables]
            fused = opt.apply_gradients(zip(grads, variables), weight_decays=wds, l2=True)
            torch.cuda.synchronize()
            _same('%s, %s: fused %s' % (ds['name'], how, type(opt).__name__), fused.tensor_l2_losses[pos].reshape(1), want)


@pytest.mark.parametrize('ds', od.l2_sets(), ids=_id)
def test_l2_sum_in_the_headers_order_on_both_paths_and_anywhere_in_a_list(ds):
    _l2_four_ways(ds)


def test_l2_sum_of_more_than_512_chunks():
    """the finish kernel's lanes take their chunks eight at a time: chunk 513 is lane 1's first of the second trip"""
    ds = od.l2_many_chunks()
    assert ds['w'].size > 512 * CH
    _l2_four_ways(ds)


def _run_list(ds, fused):
    from tf_eager_object_detection_amd import training
    variables = [_dev(w) for w in ds['tensors']]
    opt = training.AdamOptimizer(1e-3) if fused == 'adam' else training.MomentumOptimizer(0.01, 0.9)
    if fused:
        out = opt.apply_gradients(zip([torch.zeros_like(v) for v in variables], variables), weight_decays=ds['wds'], l2=True)
    else:
        out = opt.l2_loss(variables, ds['wds'])
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('fused', [False, 'momentum', 'adam'], ids=['l2_loss', 'momentum step', 'adam step'])
@pytest.mark.parametrize('ds', od.add_n_sets() + [od.add_n_many_tensors()], ids=_id)
def test_add_n_is_float32_left_to_right(ds, fused):
    """... and, with 1100 tensors, the finish kernel stages the records past 1024 on a second trip"""
    want = od.expected(ds)
    out = _run_list(ds, fused)
    print('\n%s: total %r over %d tensors' % (ds['name'], float(out.l2_loss), len(ds['tensors'])))
    _same(ds['name'] + ' per tensor', out.tensor_l2_losses, want['tensor_losses'])
    _same(ds['name'] + ' total', out.l2_loss.reshape(1), want['total'])
