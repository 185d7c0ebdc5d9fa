"""How the float16 kernels ROUND, to the bit.

Every float16 layer of the detectors ends in a hand-written float32 -> float16 store.  The integer-valued halves of the
convolution tests in tests/test_detector.py never round (every value stays a float16), their random-data halves allow several
float16 ulps.  Here each float16-storing form runs on the dyadic data of tests/exact_data.py -- exact in float32 in any summation
order (proved per case), NOT exact in float16 -- and must store the float64 result rounded ONCE to nearest even: torch.equal on
the bits, no tolerance anywhere.  The contract per form is in the case builders' docstrings and DESIGN section 4.

The CPU half (`-m "not gpu"`) asserts, from the float64 reference alone and for every case the GPU half runs, that the proof
holds and that the case is sharp: >= 1/4 of the non-zero outputs are not float16 values, >= 1/10 are exact ties (>= 1/20 in
each direction), truncation would change >= 1/10, ties-away >= 1/20, a late float16 bias / residual add >= 1/20 -- the wrong
contracts are restated in numpy / torch there; a wrong kernel is never built or run."""
import numpy as np
import pytest
import torch

import exact_data as ed

CASE_NAMES = sorted(ed.CASES)


# ---- CPU: the helper and the sharpness of every case ---------------------------------------------------------------------------

def test_single_rounding_and_wrong_contracts_known_answers_cpu():
    v = np.float64([2049.0, 2051.0, -2049.0, -2051.0, 2049.25, 4098.0, 1000.25, 2048.125])
    h, lo, hi = ed._neighbours(v)
    np.testing.assert_array_equal(h, [2048, 2052, -2048, -2052, 2050, 4096, 1000, 2048])        # ties to even
    np.testing.assert_array_equal(ed.trunc16(v), [2048, 2050, -2048, -2050, 2048, 4096, 1000, 2048])
    np.testing.assert_array_equal(ed.away16(v), [2050, 2052, -2050, -2052, 2050, 4100, 1000.5, 2048])
    assert torch.equal(ed.rn16(torch.tensor(v)), torch.tensor(h).half())
    # the late float16 add: 2049 + 1 -> float16(2049) = 2048, + 1 = 2049 -> 2048; the contract: 2050
    acc, b = torch.tensor([2049.0, 4098.0]), torch.tensor([1.0, 1.0])
    assert ed.late_epilogue(acc.double(), b.double()).tolist() == [2048.0, 4096.0]
    assert ed.rn16(ed.epilogue(acc.double(), b.double())).tolist() == [2050.0, 4100.0]
    s = ed.sharpness(torch.tensor([2049.0, 2051.0, 2050.0, 0.0, 2049.5]))
    assert s['n'] == 4 and s['inexact'] == 0.75 and s['ties'] == 0.5 and s['ties_to_zero'] == 0.25 and s['ties_away'] == 0.25
    assert s['trunc'] == 0.5 and s['away'] == 0.25


def test_proof_and_single_rounding_refuse_what_they_must_cpu():
    one = torch.ones(4, dtype=torch.float64)
    assert ed.prove_f32_exact(one * (2.0 ** 24 - 1), 1.0, integers=(one,)) == 2.0 ** 24 - 1
    with pytest.raises(AssertionError):
        ed.prove_f32_exact(one * 2.0 ** 24, 1.0)                         # 2^24 quanta: odd sums no longer exact
    with pytest.raises(AssertionError):
        ed.prove_f32_exact(one * 2.0 ** 22, 0.25)                        # the same in quarters
    with pytest.raises(AssertionError):
        ed.prove_f32_exact(one, 0.25, quanta=(one * 0.125,))             # not a multiple of the quantum
    with pytest.raises(AssertionError):
        ed.prove_f32_exact(one, 1.0, integers=(one * 0.5,))
    with pytest.raises(AssertionError):
        ed.rn16(torch.tensor([1.0 + 2.0 ** -30], dtype=torch.float64))  # not a float32: would be rounded twice
    with pytest.raises(AssertionError):
        ed.as_f16(torch.tensor([2049.0], dtype=torch.float64))
    with pytest.raises(AssertionError):                                  # small integers: nothing rounds -> not sharp
        ed.assert_sharp(torch.randint(-600, 600, (10000,)).double())


@pytest.mark.parametrize('name', CASE_NAMES)
def test_case_is_exact_in_float32_and_sharp_cpu(name):
    """the proof (inside the builder) and the floors, for every recipe the GPU half runs"""
    case = ed.CASES[name]()
    assert case.worst_quanta < ed.F32_EXACT
    case.assert_not_vacuous()
    for v in case.variants:
        for w in v.want:
            assert w.dtype in (torch.float16, torch.float32) and bool(torch.isfinite(w.float()).all())


@pytest.mark.parametrize('kind', ['subnormal', 'top'])
def test_range_cases_fill_their_bands_cpu(kind):
    case = ed.range_case(kind)
    ed.assert_bands(case, kind)
    for v in case.variants:
        want = v.want[0].double()
        if kind == 'subnormal':            # gradual: the expected values are subnormal float16 numbers, not zeros
            nz = want[want != 0].abs()
            assert nz.numel() >= 10 * ed.BAND_FLOOR and float(nz.max()) < 2.0 ** -14 and float(nz.min()) == 2.0 ** -24
        else:
            assert int(torch.isinf(want).sum()) >= ed.BAND_FLOOR and int((want.abs() == 65504).sum()) >= ed.BAND_FLOOR


def test_decision_boundary_set_is_complete_and_two_conversions_agree_on_it_cpu():
    v = ed.f16_decision_boundaries()
    assert v.dtype == np.float32 and 300_000 < v.size < 1_000_000
    have = set(v[np.isfinite(v)].view(np.uint32).tolist())
    h = np.arange(0, 0x7C00, dtype=np.uint16).view(np.float16).astype(np.float32)
    for sign in (1.0, -1.0):
        mids = ((h[:-1].astype(np.float64) + h[1:].astype(np.float64)) / 2).astype(np.float32) * np.float32(sign)
        for arr in (mids, np.nextafter(mids, np.float32(np.inf)), np.nextafter(mids, np.float32(-np.inf)), h * np.float32(sign)):
            assert set(arr.view(np.uint32).tolist()) <= have
    for x in (2.0 ** -25, 65504.0, 65520.0, 65519.99609375, 65520.00390625, 1e-45):
        assert np.float32(x).view(np.uint32) in have and np.float32(-x).view(np.uint32) in have
    assert np.isnan(v).sum() >= 4 and np.isinf(v).sum() >= 2 and np.isneginf(v).any()
    # torch's conversion (the GPU test's reference) against numpy's: two independent round-to-nearest-even implementations
    a = ed.f16_bits_nan_as_one(torch.from_numpy(v).half().view(torch.int16).numpy().view(np.uint16))
    with np.errstate(over='ignore'):
        b = ed.f16_bits_nan_as_one(v.astype(np.float16).view(np.uint16))
    np.testing.assert_array_equal(a, b)
    # and the wrong modes differ on it: truncation on every midpoint and upper neighbour, ties-away on every other midpoint
    fin = v[np.isfinite(v) & (np.abs(v) < 65504)].astype(np.float64)
    rn = fin.astype(np.float32).astype(np.float16).astype(np.float64)
    assert (ed.trunc16(fin) != rn).mean() > 0.2 and (ed.away16(fin) != rn).mean() > 0.05


@pytest.mark.parametrize('kind', ['rgb', 'stem'])
def test_input_conversion_cases_see_the_conversion_mode_cpu(kind):
    right = ed.input_conversion_case(kind)
    wrong_t = ed.input_conversion_case(kind, convert=lambda img: torch.from_numpy(ed.trunc16(img.double().numpy())))
    wrong_a = ed.input_conversion_case(kind, convert=lambda img: torch.from_numpy(ed.away16(img.double().numpy())))
    cat = lambda c: torch.cat([w.reshape(-1) for w in c.variants[0].want]).double()
    r, t, a = cat(right), cat(wrong_t), cat(wrong_a)
    nz = r != 0
    assert int(nz.sum()) > 10000
    assert float((t != r)[nz].double().mean()) >= ed.FLOOR_TRUNC and float((a != r)[nz].double().mean()) >= ed.FLOOR_AWAY
    assert bool((r < 0).any()) == (kind == 'rgb')                     # (the stem shows the negative pixels in its second pass)
    if kind == 'stem':
        pos, neg = right.variants[0].want
        assert int((pos != 0).sum()) > 1000 and int((neg != 0).sum()) > 1000


FUZZ_KINDS = ['conv3x3', 'rpn_head_fused', 'conv3x3_conv1x1', 'stem', 'pointwise', 'lateral_merge', 'pointwise_dual', 'conv3x3_rgb',
              'conv3x3_relu_pool2']


def test_fuzz_slice_is_exact_and_sharp_per_kind_cpu():
    """the random shapes are small and odd (a share over one such case is noise): the floors hold per KIND over the slice"""
    pre, late = {}, {}
    for i in range(ed.FUZZ_CASES):
        case = ed.fuzz_case(i)
        assert case.worst_quanta < ed.F32_EXACT
        for what, value, floor in case.checks:
            assert value > 0, (case.name, what)
        for v in case.variants:
            if v.pre is None:
                continue
            k = (i % 9, v.late is not None)
            pre.setdefault(k, []).extend(p.reshape(-1) for p in v.pre)
            if v.late is not None:
                late.setdefault(k, []).extend(t.reshape(-1) for t in v.late)
    assert {k[0] for k in pre} == set(range(9)) - {1}                 # (the RpnHead's outputs are float32: held by its checks)
    for k in pre:
        ed.assert_sharp(torch.cat(pre[k]), torch.cat(late[k]) if k in late else None, 'fuzz kind %s' % FUZZ_KINDS[k[0]])


# ---- GPU -----------------------------------------------------------------------------------------------------------------------

def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16) if t.dtype == torch.float16 else t.view(torch.int32)


def _assert_same_bits(got, want, what, pre=None):
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (what, got.dtype, tuple(got.shape), tuple(want.shape))
    g, w = _bits(got), _bits(want)
    if torch.equal(g, w):
        return
    bad = (g != w).reshape(-1)
    i = int(torch.nonzero(bad)[0])
    mask = 0xFFFF if want.dtype == torch.float16 else 0xFFFFFFFF
    exact = '' if pre is None else ', float64 value %r' % float(pre.reshape(-1)[i])
    raise AssertionError('%s: %d of %d elements differ; first at flat index %d: expected bits 0x%X (%r), got 0x%X (%r)%s' % (
        what, int(bad.sum()), bad.numel(), i, int(w.reshape(-1)[i]) & mask, float(want.reshape(-1)[i]),
        int(g.reshape(-1)[i]) & mask, float(got.detach().cpu().reshape(-1)[i]), exact))


def _run_case(case):
    from tf_eager_object_detection_amd import ops
    d = {k: t.cuda() for k, t in case.tensors.items()}
    for v in case.variants:
        got = v.call(ops, d)
        got = list(got) if isinstance(got, (list, tuple)) else [got]
        assert len(got) == len(v.want), (case.name, v.name)
        for j, (g, w) in enumerate(zip(got, v.want)):
            pre = v.pre[j] if v.pre is not None and j < len(v.pre) else None
            _assert_same_bits(g, w, '%s / %s [output %d]' % (case.name, v.name, j), pre)
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize('name', CASE_NAMES)
def test_float16_store_is_one_rounding_of_the_float32_value(name):
    """every float16-storing form and epilogue switch (tests/exact_data.py CASES): the stored bits are the float64 result rounded
    once to nearest even; the float32 outputs of the RpnHead forms and of dense_f16_out_f32 are the float64 values themselves"""
    _run_case(ed.CASES[name]())


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['subnormal', 'top'])
def test_float16_range_ends_through_a_layer(kind):
    """ops.pointwise / ops.conv3x3_f16 with results in float16's subnormal range (subnormal INPUTS too: gradual underflow both
    ways, nothing flushed) and around its top ([65504, 65520) -> 65504, beyond -> inf, -inf -> 0 under the ReLU)"""
    _run_case(ed.range_case(kind))


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['rgb', 'stem'])
def test_float32_image_is_converted_to_nearest_even(kind):
    """the INPUT conversion of ops.conv3x3_rgb / ops.stem_conv7_pool3 on float32 images: one-hot weights, the output is the
    converted pixel; pixels are float16 ties and their float32 neighbours"""
    _run_case(ed.input_conversion_case(kind))


@pytest.mark.gpu
def test_packed_conversion_on_every_float16_decision_boundary():
    """d_cvt_pk_f16 / d_cvt8_f16 / d_pack8_f16 (csrc/odet_internal.h: inline v_cvt_pk_f16_f32) as the product compiles them
    (odet_debug_cvt_f16 of the diagnostic build) == torch's float32 -> float16 conversion on the CPU, bit for bit, on the complete
    set of decision boundaries; every value goes through both halves of the packed instruction, next to different neighbours"""
    from tf_eager_object_detection_amd import _lib
    from tools import _diag
    h = _diag.diag_handle()
    v = ed.f16_decision_boundaries()
    v = np.concatenate([v, np.zeros(-v.size % 8 + 8, np.float32)])
    for shift in (0, 1, 3):
        arr = np.ascontiguousarray(np.roll(v, shift))
        src = torch.from_numpy(arr).cuda()
        out_pk = torch.full((arr.size,), 7.0, dtype=torch.float16, device='cuda')
        out_p8 = torch.full((arr.size,), 7.0, dtype=torch.float16, device='cuda')
        _lib.check(h.odet_debug_cvt_f16(src.data_ptr(), out_pk.data_ptr(), out_p8.data_ptr(), arr.size, _lib.stream()))
        torch.cuda.synchronize()
        want = ed.f16_bits_nan_as_one(torch.from_numpy(arr).half().view(torch.int16).numpy().view(np.uint16))
        for name, out in (('d_cvt8_f16', out_pk), ('d_cvt_pk_f16 + d_pack8_f16', out_p8)):
            got = ed.f16_bits_nan_as_one(out.cpu().view(torch.int16).numpy().view(np.uint16))
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, '%s, shift %d: %d differ; first: float32 bits 0x%08X (%r) -> expected 0x%04X, got 0x%04X' % (
                name, shift, bad.size, int(arr[bad[0]:bad[0] + 1].view(np.uint32)[0]), float(arr[bad[0]]), int(want[bad[0]]), int(got[bad[0]]))


@pytest.mark.gpu
@pytest.mark.parametrize('i', range(ed.FUZZ_CASES))
def test_fuzz_slice_on_data_that_rounds(i):
    """a bounded, seeded slice of tools/fuzz_conv.py's float16 kinds on the dyadic generator: odd random shapes, bit for bit"""
    _run_case(ed.fuzz_case(i))
