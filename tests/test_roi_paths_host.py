"""CPU half of the RoI pooling path tests: the case table of tests/roi_cases.py against its own claims.

 * coverage: every row path, bin class, carry flavour, instantiation, coordinate edge and launch form the table is meant to reach
   IS reached by a named case, according to classify() (the numpy float32 restatement of the kernel's path choice); a path id
   classify can return without a case fails;
 * plans: every single-image case through its C entry point in the diagnostic library's plan-only mode, the batched cases and a
   sweep through the same planning function (odet_debug_roi_plan) -- and the walk of every swept plan assigns each
   (image, RoI, slice, row) exactly once;
 * references: float32 reference order == float64 on the dyadic cases, C oracle == numpy oracle wherever both apply;
 * sharpness: the float16 dyadic cases round (floors computed from the reference alone), and each wrong contract, restated in
   numpy, changes at least 1/20 of the outputs of the cases aimed at it."""
import numpy as np
import pytest

import roi_cases as rc

CASES = rc.CASES


@pytest.fixture(scope='module')
def lib():
    from tools import _diag
    h = _diag.diag_handle()
    yield h
    h.odet_debug_plan_only(0)


def _where(pred):
    return [c.name for c in CASES if pred(c)]


# ---- coverage -----------------------------------------------------------------------------------------------------------------------

def test_case_names_are_unique_and_sizes_stay_tiny():
    assert len(set(rc.NAMES)) == len(CASES) >= 100
    for c in CASES:
        assert c.purpose and c.n <= 32 and all(max(hw) <= 33 for hw in c.maps_hw)


def test_every_row_path_classify_can_return_has_a_case():
    seen = {}
    for c in CASES:
        for path in rc.histogram(c):
            seen.setdefault(path, []).append(c.name)
    assert set(seen) == set(rc.ROW_PATHS), sorted(set(rc.ROW_PATHS) ^ set(seen))


CARRY = [(dx, m, why) for dx, m, why in ((0, 0, 'first'), (0, 0, 'after2'), (0, 1, ''), (0, 2, 'two'), (1, 0, 'first'), (1, 0, 'after2'),
                                         (1, 0, 'gap'), (1, 1, ''), (1, 2, 'three'), (2, 0, ''))]


@pytest.mark.parametrize('pool', ['max2', 'avg2'])
def test_carry_form_reaches_every_dy_dx_m(pool):
    """float32, C = 256: every (DY, DX, M) with DX < 2 -- M = 0 at the first bin, right after a DX = 2 bin and from a column gap,
    M = 1, M = 2 after a two-column and after a three-column bin -- and every (DY, DX = 2)"""
    c = rc.BY_NAME['paths_f32_c256_%s' % pool]
    assert c.row_form == 'carry'
    ev = rc.carry_events(c)
    missing = [(dy,) + e for dy in (0, 1, 2) for e in CARRY if (dy,) + e not in ev]
    assert not missing, missing
    assert {(dy, dx, m) for dy, dx, m, _ in ev} >= {(dy, dx, m) for dy in (0, 1, 2) for dx in (0, 1) for m in (0, 1, 2)}


@pytest.mark.parametrize('name,form', [('paths_f16_c256', 'full'), ('paths_f32_c8', 'partial'), ('paths_f16_c8', 'partial'),
                                       ('paths_f32_c260', 'partial'), ('paths_f16_c260', 'partial')])
def test_plain_row_functions_reach_every_dy_dx(name, form):
    for pool in ('max2', 'avg2'):
        c = rc.BY_NAME['%s_%s' % (name, pool)]
        assert c.row_form == form
        have = {(dy, dx) for dy, dx, _, _ in rc.carry_events(c)}
        assert have == {(dy, dx) for dy in (0, 1, 2) for dx in (0, 1, 2)}, (c.name, have)
    assert rc.BY_NAME[name + '_max2'].C % 256 in ((0,) if form == 'full' else (8, 4))      # C = 260: one active lane in the second pass


def test_single_sample_path_has_cases_with_every_sample_inside_and_with_guards():
    full = [c.name for c in CASES if c.pool == rc.POOL_NONE and not c.zero
            and any(r['path'] == 'single' and r['yok'] & 1 and all(r['bins']) for r in rc.classify(c))]
    cut = [c.name for c in CASES if c.pool == rc.POOL_NONE and not c.zero
           and any(r['path'] == 'single' and (not r['yok'] & 1 or not all(r['bins'])) for r in rc.classify(c))]
    assert 'paths_f32_c256_none' in full and 'paths_f16_c256_none' in full and len(cut) >= 8


@pytest.mark.parametrize('f16', [False, True])
@pytest.mark.parametrize('C', [64, 1024])
@pytest.mark.parametrize('pool', ['max2', 'avg2'])
def test_guarded_cases_reach_every_guard(f16, C, pool):
    c = rc.BY_NAME['guarded_%s_c%d_%s' % ('f16' if f16 else 'f32', C, pool)]
    rows = [r for r in rc.classify(c) if r['path'] == 'guarded']
    # yok: bit 0 = the upper sample row of the bin is inside, bit 1 = the lower one
    assert {r['yok'] for r in rows} == {0, 1, 2, 3}                    # both out, bottom out, top out, (x alone out)
    live = [r for r in rows if r['yok']]
    xs = [r['bins'] for r in live]
    assert any(b[0] != 3 and b[-1] == 3 for b in xs) and any(b[0] == 3 and b[-1] != 3 for b in xs)      # left / right
    assert any(b[0] != 3 and b[-1] != 3 and 3 in b for b in xs)                                          # both sides of a row
    assert any({1, 2} & set(b) for b in xs)                            # a bin with one sample column out: mixed zero / live
    out = {r['r'] for r in rows} - {r['r'] for r in rows if r['yok'] and any(r['bins'])}
    assert out, 'no RoI entirely outside'
    assert (c.want_plan()['slices'] > 1) == (C == 1024)
    ref = np.concatenate([x.reshape(-1) for x in rc.reference(c)])
    assert 0.2 < float((ref != 0).mean()) < 0.95


def test_all_24_instantiations_have_inside_and_guarded_rows_and_the_pad_ring():
    for pool in rc.POOLS:
        for norm in rc.NORMS:
            for f16 in (False, True):
                cs = [c for c in CASES if c.instantiation == (pool, norm, f16) and not c.zero]
                recs = [r for c in cs for r in rc.classify(c)]
                if pool == rc.POOL_NONE:
                    inside = [r for r in recs if r['path'] == 'single' and r['yok'] & 1 and all(r['bins'])]
                    guarded = [r for r in recs if r['path'] == 'single' and (not r['yok'] & 1 or not all(r['bins']))]
                else:
                    inside = [r for r in recs if r['path'].startswith('dy')]
                    guarded = [r for r in recs if r['path'] == 'guarded']
                assert inside and guarded, (pool, norm, f16)
    for c in CASES:
        if c.norm == rc.NORM_TP and c.group == 'b':
            # samples in the pad ring: inside (ok) with the padded coordinate below 1 / above dim: the index clamps to 0 / dim - 1
            H, W = c.maps_hw[0]
            ring = set()
            for r in range(c.n):
                _, ty, tx = rc.roi_taps(c, 0, r)
                for side, (inn, ok, lo, hi, _), dim in (('y', ty, H), ('x', tx, W)):
                    if np.any(ok & (inn < 1) & (lo == 0) & (hi == 0)):
                        ring.add(side + '-low')
                    if np.any(ok & (inn > dim) & (lo == dim - 1) & (hi == dim - 1)):
                        ring.add(side + '-high')
            assert ring == {'y-low', 'y-high', 'x-low', 'x-high'}, (c.name, ring)


def _samples(c, img=0):
    for r in range(c.n):
        _, ty, tx = rc.roi_taps(c, img, r)
        yield r, ty, tx


@pytest.mark.parametrize('f16', ['f32', 'f16'])
@pytest.mark.parametrize('pool', ['none', 'max2', 'avg2'])
def test_coordinate_edge_cases_hold_their_edges(f16, pool):
    at, beyond = rc.BY_NAME['edge_at_%s_%s' % (f16, pool)], rc.BY_NAME['edge_beyond_%s_%s' % (f16, pool)]
    lim = np.float32(16)
    facts = set()
    for r, ty, tx in _samples(at):
        for inn, ok, lo, hi, lerp in (ty, tx):
            facts |= {'zero'} if np.any((inn == 0) & ok) else set()
            facts |= {'limit'} if np.any((inn == lim) & ok & (lo == 16) & (hi == 16)) else set()
            facts |= {'integer'} if np.any(ok & (inn > 0) & (inn < lim) & (lo == hi)) else set()
            facts |= {'degenerate'} if inn.size > 1 and np.all(inn == inn[0]) else set()
    assert facts == {'zero', 'limit', 'integer', 'degenerate'}, facts
    facts = set()
    for r, ty, tx in _samples(beyond):
        for inn, ok, lo, hi, lerp in (ty, tx):
            facts |= {'above'} if np.all(inn == np.nextafter(lim, np.float32(np.inf))) and not ok.any() else set()
            facts |= {'below'} if np.all((inn < 0) & (inn > -1e-20)) and not ok.any() else set()
    assert facts == {'above', 'below'}, facts


def test_reversed_boxes_p1_and_thin_maps_are_in_the_table():
    for t in ('f32', 'f16'):
        c = rc.BY_NAME['edge_reversed_%s_max2' % t]
        rev = set()
        for r, ty, tx in _samples(c):
            rev.add((bool(ty[0][-1] < ty[0][0]), bool(tx[0][-1] < tx[0][0])))
        assert rev == {(False, False), (True, False), (False, True), (True, True)}
        assert 'dy2' in rc.histogram(c)                                # (a negative y step is never a sharing class)
        # every sample inside, but a bin's second sample column left of its first: such rows take the guarded form
        assert any(r.get('reversed_x') for r in rc.classify(c))
        for hw in ((1, 17), (17, 1), (1, 1)):
            c = rc.BY_NAME['edge_map%dx%d_%s' % (hw + (t,))]
            assert c.norm == rc.NORM_IMAGE and c.maps_hw == (hw,)
            assert float(np.mean(np.concatenate([x.reshape(-1) for x in rc.reference(c)]) != 0)) > 0.3
        one = rc.BY_NAME['form_p1_none_%s' % t]
        assert one.crop == 1 and rc.BY_NAME['form_p1_max2_%s' % t].crop == 2
        _, ty, tx = rc.roi_taps(one, 0, 0)
        roi = one.images[0].rois[0]
        assert ty[0].size == 1 and ty[0][0] == np.float32(0.5) * (roi[1] + roi[3]) / np.float32(16)      # the centre sample
        # -0.0 only survives as a sample coordinate when crop == 1 (start + 0 * scale is +0.0 otherwise): it is inside
        c = rc.BY_NAME['edge_p1_centre_%s' % t]
        ins = [(tx[0][0], bool(tx[1][0])) for _, ty, tx in _samples(c)]
        assert any(v == 0 and np.signbit(v) and ok for v, ok in ins) and any(v == 0 and not np.signbit(v) and ok for v, ok in ins)
        assert any(v == 16 and ok for v, ok in ins) and any(v > 16 and v < 16.00001 and not ok for v, ok in ins)
        assert any(v == 0 and ok for v, ok in ins[-2:]) and any(v < 0 and not ok for v, ok in ins[-2:])


@pytest.mark.parametrize('name', _where(lambda c: c.zero))
def test_declared_zero_cases_form_no_tap(name):
    """NaN / inf coordinates and NORM_STRIDE on a one-row / one-column map: TF's test would let a NaN through to an index; the
    kernel's positive test never forms one.  Per RoI one axis has no inside sample at all, so every output is zero."""
    c = rc.BY_NAME[name]
    for r, ty, tx in _samples(c):
        assert not ty[1].any() or not tx[1].any(), (name, r)
        assert not np.isfinite(np.concatenate([ty[0], tx[0]])).all()
    assert all(r['path'] in ('guarded', 'single') for r in rc.classify(c))


FORM_CASES = {
    'single image, one slice': ['form_p7_f32', 'form_p17_f32', 'form_p17_f16', 'form_p17_c512_f32', 'form_p64_c8_f32', 'form_p1_none_f32',
                                'form_p1_max2_f16'],
    'B = 1 sliced': ['form_b1_c%d_%s' % (C, t) for C in (512, 768, 1024, 2048) for t in ('f32', 'f16')],
}


def test_launch_forms_of_the_issue_are_all_in_the_table():
    for names in FORM_CASES.values():
        for n in names:
            assert n in rc.BY_NAME, n
    p = rc.BY_NAME['form_p17_f32'].want_plan()
    assert p['waves'] == 8 and (13 * 17) % 8 != 0 and 17 % 8 != 0      # a workgroup's 8 rows straddle two RoIs
    have = {(c.via, c.B, c.C, c.pool, c.f16) for c in CASES if c.via != 'ops'}
    for B, C in ((2, 512), (2, 768), (2, 1024), (4, 512), (4, 1024), (8, 512), (8, 1024), (3, 512), (5, 512)):
        assert {(pool) for via, b, cc, pool, _ in have if (via, b, cc) == ('frcnn', B, C)} == {rc.POOL_MAX2, rc.POOL_NONE}, (B, C)
    assert {(pool, f16) for via, _, _, pool, f16 in have if via == 'frcnn'} == {(p_, t) for p_ in (rc.POOL_MAX2, rc.POOL_NONE) for t in (False, True)}
    assert {(C, f16) for via, _, C, _, f16 in have if via == 'fpn'} == {(C, t) for C in (256, 512) for t in (False, True)}
    groups = {(c.B, c.want_plan()['slices'] > 1, c.want_plan()['roi_groups']) for c in CASES if c.via != 'ops'}
    assert {(2, True, 2), (2, True, 0), (2, True, 1), (4, True, 1), (4, True, 0), (8, True, 0), (3, True, 4), (5, True, 4)} <= groups
    for c in CASES:
        if c.via == 'ops':
            continue
        p = c.want_plan()
        assert c.n == 13 and len({id(m) for lv in c.maps() for m in lv}) == c.B * len(c.maps_hw)
        assert not any(np.array_equal(c.images[0].rois, im.rois) for im in c.images[1:])           # every image its own RoIs
        assert not any(np.array_equal(c.maps()[0][0], lv[0]) for lv in c.maps()[1:])
        seen, escaped = rc.walk_plan(p, c.B, c.n, c.P)
        slots = p['grid_x'] // 8 * p['xcds_per_img'] * (p['slices'] if p['roi_groups'] == 0 else 1)
        assert escaped == 0 and slots > 0
        counts = [im.count for im in c.images]
        if c.B >= 3:
            assert 0 in counts and any(0 < k < c.n for k in counts) and any(k > c.n for k in counts), c.name
        if c.via == 'fpn':
            assert any(((im.level < 0) | (im.level > 3)).any() for im in c.images)
    assert {c.order for c in CASES} == {None, 'identity', 'reversed', 'spatial'}
    assert {c.order for c in CASES if c.via != 'ops'} == {'identity', 'reversed', 'spatial'}
    # slots past the last RoI (ri >= n) and the slot >= rois_per_xcd exit both occur among the batched forms
    past = [c.name for c in CASES if c.via != 'ops' and c.want_plan()['rois_per_xcd'] * max(c.want_plan()['roi_groups'], 1) > c.n
            and c.want_plan()['roi_groups'] > 0]
    assert past


# ---- plans --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', _where(lambda c: c.via == 'ops'))
def test_single_image_case_plans_as_the_table_says_in_plan_only_mode(lib, name):
    c = rc.BY_NAME[name]
    assert rc.plan_only_call(c, lib) | {'count': 0} == c.want_plan() | {'count': 0}


@pytest.mark.parametrize('name', _where(lambda c: c.via != 'ops'))
def test_batched_case_plans_as_the_table_says(lib, name):
    from tools import _diag
    c = rc.BY_NAME[name]
    assert _diag.roi_plan(c.B, c.C, c.n, c.P, c.f16, c.pool, c.norm, handle=lib) == c.want_plan()


def test_plan_sweep_assigns_every_roi_slice_and_row_exactly_once(lib):
    from tools import _diag
    checked = 0
    for B in range(1, 9):
        for C in (8, 64, 256, 260, 512, 768, 1024, 2048):
            for n in (1, 2, 7, 8, 13, 31, 64):
                for P in (1, 2, 7, 14, 16, 17, 33, 64):
                    p = _diag.roi_plan(B, C, n, P, handle=lib)
                    assert {k: p[k] for k in rc.plan_of(B, C, n, P)} == rc.plan_of(B, C, n, P)
                    assert p['grid_x'] % 8 == 0 and p['grid_x'] > 0 and p['threads'] == p['waves'] * 64 <= 1024
                    seen, escaped = rc.walk_plan(p, B, n, P)
                    assert escaped == 0, (B, C, n, P)                  # no slot maps past n (or past the image) without leaving
                    assert len(seen) == B * n * p['slices'] * P and set(seen.values()) == {1}, (B, C, n, P)
                    checked += 1
    assert checked == 8 * 8 * 7 * 8


# ---- references -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', _where(lambda c: c.dyadic))
def test_float32_reference_order_equals_float64_on_the_dyadic_cases(name):
    c = rc.BY_NAME[name]
    for ref, ex in zip(rc.reference(c), rc.exact(c)):
        assert np.array_equal(ref.astype(np.float64), ex), name
        assert float((ex != 0).mean()) > 0.5


@pytest.mark.parametrize('name', _where(lambda c: not c.zero and not c.dyadic and c.group in 'abc' and not c.f16))
def test_float64_restatement_agrees_with_the_reference_order_on_random_data(name):
    """(not exact there: the float32 lerps round; a mistake in the taps of the mirror would be far larger)"""
    c = rc.BY_NAME[name]
    for ref, ex in zip(rc.reference(c), rc.exact(c)):
        assert np.allclose(ref, ex, rtol=0, atol=2e-5), (name, float(np.abs(ref - ex).max()))


@pytest.mark.parametrize('name', _where(lambda c: rc.c_reference.__call__ and (c.norm, c.pool) in (
    (rc.NORM_STRIDE, rc.POOL_MAX2), (rc.NORM_STRIDE, rc.POOL_NONE), (rc.NORM_IMAGE, rc.POOL_MAX2), (rc.NORM_TP, rc.POOL_AVG2)) and not c.zero))
def test_c_oracle_equals_numpy_oracle(name):
    c = rc.BY_NAME[name]
    got = rc.c_reference(c)
    assert got is not None
    for a, b in zip(got, rc.reference(c)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name


# ---- sharpness --------------------------------------------------------------------------------------------------------------------

FLOORS = {rc.POOL_NONE: 0.1, rc.POOL_MAX2: 0.1, rc.POOL_AVG2: 0.05}


@pytest.mark.parametrize('name', _where(lambda c: c.f16 and c.data in ('ints', 'subnormal')))
def test_dyadic_float16_cases_round(name):
    c = rc.BY_NAME[name]
    s = rc.sharpness(c)
    print('SHARP %s not_f16 %.3f ties %.3f away %.3f toward %.3f' % (name, s['not_f16'], s['ties'], s['ties_away'], s['ties_toward']))
    floor = FLOORS[c.pool]
    assert s['not_f16'] >= 0.5 and s['ties'] >= floor, s
    assert s['ties_away'] >= floor / 3 and s['ties_toward'] >= floor / 3, s


@pytest.mark.parametrize('name', _where(lambda c: c.f16 and c.data == 'max'))
def test_maps_at_the_largest_float16_stay_finite(name):
    c = rc.BY_NAME[name]
    for ex in rc.exact(c):
        assert float(np.abs(ex).max()) == 65504.0 and np.isfinite(rc.round_f16(ex).astype(np.float32)).all()
        assert float((np.abs(ex) == 65504.0).mean()) > 0.02
    # the float32 sum of four such samples is far from float32's range: (a + b + c + d) / 4 is exact
    assert np.float32(65504) * 4 / 4 == 65504


@pytest.mark.parametrize('name,contract', [(c.name, a) for c in CASES for a in c.aim])
def test_wrong_contracts_change_the_cases_aimed_at_them(name, contract):
    c = rc.BY_NAME[name]
    right = np.concatenate([e.reshape(-1) for e in rc.exact(c)])
    if contract in ('trunc', 'away'):
        a, b = rc.round_f16(right), rc.round_f16(right, contract)
    elif contract == 'sample16':
        a, b = rc.round_f16(right), rc.round_f16(np.concatenate([e.reshape(-1) for e in rc.exact(c, sample16=True)]))
    else:
        wrong = np.concatenate([e.reshape(-1) for e in rc.exact(c, inside=contract)])
        a, b = (rc.round_f16(right), rc.round_f16(wrong)) if c.f16 else (right.astype(np.float32), wrong.astype(np.float32))
    changed = float((a != b).mean())
    print('CONTRACT %s %s changes %.3f of the outputs' % (name, contract, changed))
    assert changed >= 0.05, (name, contract, changed)


def test_every_wrong_contract_has_cases_in_both_types_where_it_applies():
    aims = {}
    for c in CASES:
        for a in c.aim:
            aims.setdefault(a, set()).add(c.f16)
    assert aims == {'trunc': {True}, 'away': {True}, 'sample16': {True}, 'lt': {False, True}, 'ulp': {False, True}}
