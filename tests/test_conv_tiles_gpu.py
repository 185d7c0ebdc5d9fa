"""GPU half of the per-instantiation convolution tests: every case of tests/conv_tile_cases.py runs inside the diagnostic
library with its tile forced (or nothing forced, for a natural case), the plan the launcher recorded for THAT launch must be
the case's form, tile, limb count and K split, and the result is compared without a tolerance:

 * float16: the stored bits == the float64 result rounded once (data exact in float32, sharp in float16);
 * exact float32 and the split forms on exact data (integers, and the limb-sensitive data that makes every kept limb product
   count): torch.equal against the float64 result;
 * forced K splits: that, bit-identical results from run to run on random data, ticket words zero afterwards;
 * the split forms on random data keep the criterion of tests/test_detector.py -- as close to float64 as the exact-float32
   form, e_split <= max(2 e_exact, 2e-6) -- per tile.

Each passing case prints one `TILE-PLAN` line naming the instantiation it ran on (pytest -rP shows them)."""
import pytest
import torch

import conv_tile_cases as ct
from test_f16_rounding_gpu import _assert_same_bits

F32_FORM = {('f32', 1): 'exact', ('split', 3): 'x3', ('split', 2): 'x2'}


def _check_plan(tc, lib, before, what):
    from tools import _diag
    plan = _diag.last_plan(tc.family, lib)
    want = tc.want_plan()
    assert {k: plan[k] for k in want} == want, (tc.name, what, plan)
    assert plan['count'] == before + 1, (tc.name, what, 'launches of the family: %d' % (plan['count'] - before))
    return plan


def _report(tc, plan):
    print('TILE-PLAN %s limbs %d %s tile %dx%dx%dx%d ksplit %d %s blocks %d :: %s' % (
        (tc.family, tc.limbs, 'plain' if tc.form == 'pooled' else tc.form) + plan['tile'] + (plan['ksplit'], tc.form, plan['blocks'], tc.name)))


def _tickets_are_zero():
    from tf_eager_object_detection_amd import ops
    torch.cuda.synchronize()
    assert ops._X3_WS, 'no split-K workspace was allocated'
    for ws in ops._X3_WS.values():
        assert int(ws.buf[:16384].max().item()) == 0                  # every ticket drawn back to zero
        assert ws.range_ok()                                          # and nothing reported out of range


@pytest.mark.gpu
@pytest.mark.parametrize('name', [c.name for c in ct.CASES if c.family == 'f16'])
def test_float16_tile_case(name):
    from tf_eager_object_detection_amd import ops
    from tools._diag import diag_library
    tc = ct.BY_NAME[name]
    case = tc.build()
    d = {k: t.cuda() for k, t in case.tensors.items()}
    with diag_library() as lib:
        tc.force(lib)
        for what, call, want, pre in tc.f16_launches(case):
            before = ct.plan_count(lib, 'f16')
            got = call(ops, d)
            plan = _check_plan(tc, lib, before, what)
            got = list(got) if isinstance(got, (list, tuple)) else [got]
            assert len(got) == len(want)
            for j, (g, w) in enumerate(zip(got, want)):
                _assert_same_bits(g, w, '%s / %s [output %d]' % (name, what, j), pre[j] if pre is not None and j < len(pre) else None)
    torch.cuda.synchronize()
    _report(tc, plan)


@pytest.mark.gpu
@pytest.mark.parametrize('name', [c.name for c in ct.CASES if c.family != 'f16'])
def test_float32_tile_case(name):
    from tf_eager_object_detection_amd import ops
    from tools._diag import diag_library
    tc = ct.BY_NAME[name]
    case = tc.build()
    with ops.f32_form(F32_FORM[(tc.family, tc.limbs)]), diag_library() as lib:
        tc.force(lib)
        for v in case.variants:
            d = {k: t.cuda() for k, t in v.tensors.items()}
            before = ct.plan_count(lib, tc.family)
            got = v.run(ops, d)
            plan = _check_plan(tc, lib, before, v.name)
            assert len(got) == len(v.want)
            for j, (g, w) in enumerate(zip(got, v.want)):
                g = g.cpu()
                assert g.dtype == torch.float32 and tuple(g.shape) == tuple(w.shape)
                bad = g.double() != w
                assert not bool(bad.any()), '%s / %s [map %d]: %d of %d values differ from the float64 result; first: got %r, expected %r' % (
                    name, v.name, j, int(bad.sum()), bad.numel(), float(g[bad][0]), float(w[bad][0]))
        if tc.ksplit > 1:
            # a K split adds its parts in a fixed order: the same bits from run to run on data that rounds
            gen = torch.Generator(device='cuda')
            gen.manual_seed(tc.ksplit * 131 + tc.args['cin'])
            iv = case.variants[0]
            d = {}
            for k, t in iv.tensors.items():
                r = torch.randn(tuple(t.shape), device='cuda', generator=gen) * (0.05 if k == 'w' else 1.0)
                d[k] = r.contiguous(memory_format=torch.channels_last) if t.dim() == 4 and k == 'w' else r
            a1, a2 = iv.run(ops, d), iv.run(ops, d)
            _check_plan(tc, lib, before + 2, 'random data')
            assert all(torch.equal(p, q) for p, q in zip(a1, a2))
    if tc.family == 'split':
        _tickets_are_zero()
    _report(tc, plan)


@pytest.mark.gpu
@pytest.mark.parametrize('name', [c.name for c in ct.CASES if c.data == 'limbs'])
def test_split_form_on_random_data_is_as_close_to_float64_as_the_exact_form(name):
    """one launch per (limb count, tile, form): random activations and weights, the tile forced for the split form, the exact
    form on its own pick; the project's criterion of tests/test_detector.py"""
    import torch.nn.functional as F
    from tf_eager_object_detection_amd import ops
    from tools._diag import diag_library
    tc = ct.BY_NAME[name]
    a = tc.args
    gen = torch.Generator(device='cuda')
    gen.manual_seed(a['cin'] * 7 + sum(tc.tile) + tc.limbs)
    B, cin, cout = a['B'], a['cin'], a['cout']
    H, W = tc.maps()[0]
    k = 1 if tc.form == 'pointwise' else 3
    x = torch.randn((B, H, W, cin), device='cuda', generator=gen) * 3
    w = (torch.randn((cout, cin, k, k), device='cuda', generator=gen) * (cin * k * k) ** -0.5).contiguous(memory_format=torch.channels_last)
    b = torch.randn(cout, device='cuda', generator=gen)
    want = F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), b.double(), 1, k // 2).permute(0, 2, 3, 1)
    run = (lambda: ops.conv3x3_f32(x, w, b)) if k == 3 else (lambda: ops.pointwise(x, w.reshape(cout, cin).contiguous(), b))
    with ops.f32_form('exact'):
        ex = run()
    with ops.f32_form(F32_FORM[(tc.family, tc.limbs)]), diag_library() as lib:
        tc.force(lib)
        before = ct.plan_count(lib, 'split')
        sp = run()
        plan = _check_plan(tc, lib, before, 'random data')
    rms = float(want.pow(2).mean().sqrt())
    e_ex, e_sp = float((ex.double() - want).abs().max()) / rms, float((sp.double() - want).abs().max()) / rms
    print('e_exact %.3g e_split %.3g' % (e_ex, e_sp))
    assert e_sp <= max(2.0 * e_ex, 2e-6), (name, e_ex, e_sp)
    _report(tc, plan)
