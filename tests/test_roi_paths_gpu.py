"""GPU half of the RoI pooling path tests: every case of tests/roi_cases.py runs inside the diagnostic library.

 * the plan the launcher recorded for THAT launch equals the case's, and the launch counter advanced by exactly one;
 * the result is compared without a tolerance: float32 bits against the reference-order result (oracle_np's functions, the C
   oracle where the host test proved it equal), float16 bits against the float64 result rounded once on the dyadic data and
   against the reference-order float32 result rounded once on random data, the declared-behaviour cases against zeros;
 * the output was pre-filled with NaN: every row is written, the rows at or beyond the device count are zero;
 * the batched cases (FrcnnStepBatch / FpnStepBatch, STAGE_ROI alone) also equal their images run one at a time through
   ops.roi_pool.

Each passing case prints one `ROI-PLAN` line with its launch form and its path histogram from classify() (pytest -rP)."""
import numpy as np
import pytest

import roi_cases as rc


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16 if a.dtype == np.float16 else np.uint32)


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert not np.isnan(got.astype(np.float32)).any(), '%s: rows left unwritten' % what
    # +0.0 and -0.0: the reference order and the kernel form the same signed zeros (the padded rows are +0.0)
    diff = _bits(got) != _bits(want)
    assert not diff.any(), '%s: %d of %d differ, first at %s: got %r want %r' % (
        what, int(diff.sum()), diff.size, np.argwhere(diff)[0].tolist(), got[tuple(np.argwhere(diff)[0])], want[tuple(np.argwhere(diff)[0])])


def _run(name):
    from tools import _diag
    c = rc.BY_NAME[name]
    want = rc.expected(c, fast=True)
    with _diag.diag_library() as lib:
        before = _diag.last_roi_plan(lib)['count']
        got = [rc.run_single(c)] if c.via == 'ops' else rc.run_batch(c)
        plan = _diag.last_roi_plan(lib)
        assert plan['count'] == before + 1, (name, 'RoI launches: %d' % (plan['count'] - before))
        assert {k: plan[k] for k in c.want_plan()} == c.want_plan(), (name, plan)
        for b in range(c.B):
            _same(got[b], want[b], '%s [image %d]' % (name, b))
            cnt = max(rc.count_of(c, b), 0)
            assert not got[b][cnt:].any()                              # rows at or beyond the count are zero
        if c.via != 'ops':
            for b in range(c.B):
                _same(rc.run_single(c, b, order=False), got[b], '%s [image %d alone]' % (name, b))
    print('ROI-PLAN %s :: %s :: %s :: %s' % (c.form(), ' '.join('%s %d' % kv for kv in sorted(rc.histogram(c).items())),
                                           'inst %s/%s/%s %s' % (rc.POOLS[c.pool], rc.NORMS[c.norm], 'f16' if c.f16 else 'f32', c.via), name))


@pytest.mark.gpu
@pytest.mark.parametrize('name', [c.name for c in rc.CASES if not c.zero])
def test_roi_case(name):
    _run(name)


@pytest.mark.gpu
@pytest.mark.parametrize('name', [c.name for c in rc.CASES if c.zero])
def test_roi_declared_zero_case(name):
    """no reference has these inputs (NaN / inf coordinates, NORM_STRIDE's division by dim - 1 == 0): the kernel's header says no
    tap is ever formed from them, so every output is zero -- and no address is formed either"""
    _run(name)
