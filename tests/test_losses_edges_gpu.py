"""tests/losses_edge_cases.py on the GPU: every case of the table through ops.roi_losses / ops.rpn_losses /
ops.rpn_losses_backward against tests/losses_np.py by BYTES (a zero of the wrong sign, a flushed subnormal or a clamp that
differs from the header's rule fails), the documented limits with a good call after each refusal, and the zero fill of the
dense gradients at the sizes where its scalar tails and a further grid-stride trip run."""
import numpy as np
import pytest
import torch

import losses_edge_cases as ec

pytestmark = pytest.mark.gpu

ROI, RPN, BWD = ec.roi_cases(), ec.rpn_cases(), ec.backward_cases()


def _id(c):
    return c['name']


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(what, got, want):
    got = got.detach().cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.nonzero(got.reshape(-1).view(np.uint32) != want.reshape(-1).view(np.uint32))[0]
        raise AssertionError('%s: %d of %d elements differ, first at %d: got %r, restated %r'
                             % (what, len(bad), got.size, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]]))


def _run_roi(c, upstream):
    from tf_eager_object_detection_amd import ops
    up = None if upstream is None else _dev(np.tile(upstream, (c['B'], 1)))
    out = ops.roi_losses(_dev(c['scores']), _dev(c['deltas']), _dev(c['labels']), _dev(c['targets']), _dev(c['inside']),
                         _dev(c['outside']), _dev(c['counts']), c['sigma'], row_map=_dev(c['row_map']), upstream=up)
    torch.cuda.synchronize()
    return out


def _check_roi(c):
    for upstream in (None,) + ec.UPSTREAMS:
        got = _run_roi(c, upstream)
        assert got.losses.shape == (c['B'], 2) and got.grad_scores.shape == (c['B'], c['R'], c['C'])
        for b, want in enumerate(ec.roi_expected(c, upstream)):
            what = '%s, image %d, upstream %s' % (c['name'], b, None if upstream is None else upstream.tolist())
            for k in ('losses', 'grad_scores', 'grad_deltas'):
                _same('%s: %s' % (what, k), getattr(got, k)[b], want[k])


@pytest.mark.parametrize('c', ROI, ids=_id)
def test_roi_loss_edge_case(c):
    _check_roi(c)


@pytest.mark.parametrize('what,C,R,S,B', ec.ROI_OVER_LIMIT, ids=[o[0] for o in ec.ROI_OVER_LIMIT])
def test_roi_loss_over_a_limit_is_refused_and_the_next_call_succeeds(what, C, R, S, B):
    from tf_eager_object_detection_amd import _lib, ops
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device='cuda')
    with pytest.raises(_lib.OdetError, match='odet error -4'):
        ops.roi_losses(z(B, R, C), z(B, R, 4 * C), z(B, S, dtype=torch.int32), z(B, S, 4 * C), z(B, S, 4 * C), z(B, S, 4 * C),
                       z(B, 4, dtype=torch.int32), 1.0)
    _check_roi(ROI[1])


def _run_rpn(c, upstream):
    from tf_eager_object_detection_amd import ops
    idx = _dev(c['sample_idx'])
    fwd = ops.rpn_losses(_dev(c['scores']), _dev(c['deltas']), idx, _dev(c['sample_targets']), _dev(c['counts']), c['sigma'],
                         c['layout'], c['A'])
    bwd = ops.rpn_losses_backward(idx, fwd.row_grad_scores, fwd.row_grad_deltas, _dev(upstream), c['N'], c['layout'], c['A'])
    torch.cuda.synchronize()
    return dict(losses=fwd.losses, row_grad_scores=fwd.row_grad_scores, row_grad_deltas=fwd.row_grad_deltas,
                grad_scores=bwd.grad_scores, grad_deltas=bwd.grad_deltas)


def _check_rpn(c):
    for up in ec.UPSTREAMS:
        upstream = np.tile(up, (c['B'], 1))
        got = _run_rpn(c, upstream)
        for b, want in enumerate(ec.rpn_expected(c, upstream)):
            for k in ('losses', 'row_grad_scores', 'row_grad_deltas', 'grad_scores', 'grad_deltas'):
                _same('%s, image %d, upstream %s: %s' % (c['name'], b, up.tolist(), k), got[k][b], want[k])


@pytest.mark.parametrize('c', RPN, ids=_id)
def test_rpn_loss_edge_case(c):
    _check_rpn(c)


@pytest.mark.parametrize('what,S,B', ec.RPN_OVER_LIMIT, ids=[o[0] for o in ec.RPN_OVER_LIMIT])
def test_rpn_loss_over_a_limit_is_refused_and_the_next_call_succeeds(what, S, B):
    from tf_eager_object_detection_amd import _lib, ops
    N = 90
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device='cuda')
    idx = z(B, S, dtype=torch.int32)
    with pytest.raises(_lib.OdetError, match='odet error -4'):
        ops.rpn_losses(z(B, 2 * N), z(B, N, 4), idx, z(B, S, 4), z(B, 5, dtype=torch.int32), 3.0)
    with pytest.raises(_lib.OdetError, match='odet error -4'):
        ops.rpn_losses_backward(idx, z(B, S, 2), z(B, S, 4), z(B, 2), N)
    _check_rpn(RPN[0])


def _poison(*shapes):
    """NaNs in blocks of the sizes the outputs will have: the caching allocator hands the same blocks to the next
    torch.empty of that size, so an element the fill leaves out is not a lucky zero"""
    for shape in shapes:
        torch.full(shape, float('nan'), device='cuda')
    torch.cuda.synchronize()


def _run_backward(c):
    from tf_eager_object_detection_amd import ops
    B, N = c['B'], c['N']
    _poison((B, 2 * N), (B, N, 4))
    out = ops.rpn_losses_backward(_dev(c['sample_idx']), _dev(c['row_gs']), _dev(c['row_gd']), _dev(c['upstream']), N,
                                  scores=c['want_scores'], deltas=c['want_deltas'])
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('c', BWD, ids=_id)
def test_dense_gradients_fill_and_scatter_edge_case(c):
    got = _run_backward(c)
    assert (got.grad_scores is None) == (not c['want_scores']) and (got.grad_deltas is None) == (not c['want_deltas'])
    for b, (gs, gd) in enumerate(ec.backward_expected(c)):
        if c['want_scores']:
            _same('%s, image %d: grad_scores' % (c['name'], b), got.grad_scores[b], gs)
        if c['want_deltas']:
            _same('%s, image %d: grad_deltas' % (c['name'], b), got.grad_deltas[b], gd)


def test_dense_gradients_of_154_mb_are_zero_outside_the_sampled_rows():
    """B = 64, N = 100 003: more 16-byte vectors than 8192 blocks store in four trips.  Checked on the device: the sampled
    rows against the restatement by bits, and the number of non-zero BIT PATTERNS in everything else (none)."""
    c = ec.backward_case('154 MB', ec.BIG_FILL['N'], ec.BIG_FILL['B'], S=16, seed=9)
    assert ec.fill_path(c['N'], c['B'])['trips'] == 5
    got = _run_backward(c)
    B, N, S = c['B'], c['N'], c['S']
    ok = (c['sample_idx'] >= 0) & (c['sample_idx'] < N)
    bi, ki = np.nonzero(ok)
    rows = torch.from_numpy(c['sample_idx'][bi, ki].astype(np.int64)).cuda()
    bi_t = torch.from_numpy(bi).cuda()
    for name, dense, row_g, u in (('grad_scores', got.grad_scores.view(B, N, 2), c['row_gs'], 0),
                                  ('grad_deltas', got.grad_deltas, c['row_gd'], 1)):
        want = (c['upstream'][:, u][bi, None] * row_g[bi, ki]).astype(np.float32)
        _same('154 MB: %s at the sampled rows' % name, dense[bi_t, rows], want)
        nonzero = int(torch.count_nonzero(dense.reshape(-1).view(torch.int32)))
        assert nonzero == int(np.count_nonzero(want.view(np.uint32))), (name, nonzero)
    assert len(bi) == B * (S - 2)
