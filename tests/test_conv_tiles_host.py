"""CPU half of the per-instantiation convolution tests: the case table of tests/conv_tile_cases.py against the tile tables of
the kernel files, in the diagnostic build's plan-only mode (include/odet_diag.h: the launchers check, plan, record and return
before any HIP call, so the C ABI runs here with pointer-valued integers nothing dereferences).

 * the table covers every (family, form, tile) the library reports, and a tile added later without a case fails;
 * every case lands on its intended form, tile and K split -- an override that silently did not apply shows here;
 * the coverage rules (partial last slab, slabs cut inside a row and across the image border, padded workgroups, channel tiles,
   multi-level launches, K depths around the stage counts, the forced K splits) hold, computed from the table;
 * every float16 case is exact in float32 and sharp in float16, every float32 case proved exact;
 * the split forms' limb-sensitive data: every product the kernel keeps changes its case's expected result, every product it
   drops is zero;
 * a sweep of shapes through the launchers' own picks: every tile a picker reaches has a natural case, and the three tiles
   no picker reaches are exactly the ones the table marks so."""
import pytest
import torch

import conv_tile_cases as ct
import exact_data as ed

NAMES = [c.name for c in ct.CASES]
FORCED = [c for c in ct.CASES if c.mode == 'forced']


@pytest.fixture(scope='module')
def lib():
    from tools import _diag
    h = _diag.diag_handle()
    yield h
    ct.clear_overrides(h)
    h.odet_debug_plan_only(0)


def _tables(lib):
    from tools import _diag
    return {fam: _diag.tile_table(fam, lib) for fam in _diag.FAMILIES}


def test_tile_lists_of_the_case_module_are_the_librarys(lib):
    t = _tables(lib)
    want16 = {tile: {'plain', 'pointwise', 'tail', 'pooled'} | ({'rpn'} if tile in ct.F16_RPN else set()) for tile in ct.F16_TWO_STAGE}
    want16.update({tile: {'plain', 'pointwise'} for tile in ct.F16_RINGS})
    assert {e['tile']: set(e['forms']) for e in t['f16']} == want16 and len(t['f16']) == len(want16) == 15
    assert all(e['limbs'] == 1 for e in t['f16'] + t['f32'])
    assert [e['tile'] for e in t['f32']] == [ct.tile_of('f32', 1, mt, wn) for mt, wn in ct.F32_TILES]
    assert [(e['limbs'], e['tile']) for e in t['split']] == [(nl, ct.tile_of('split', nl, mt, wn)) for nl in (3, 2)
                                                             for mt, wn in ct.SPLIT_TILES[nl]]
    assert all(set(e['forms']) == {'plain', 'pointwise'} for e in t['f32'] + t['split'])
    # the instantiations: the pooled form is the plain kernel's epilogue, not a kernel of its own
    n = {fam: sum(len(set(e['forms']) - {'pooled'}) for e in t[fam]) for fam in t}
    assert n == {'f16': 48, 'f32': 20, 'split': 18}


def test_every_form_of_every_tile_has_a_forced_case(lib):
    have = {(c.family, c.limbs, c.form, c.tile) for c in FORCED}
    missing = [(fam, e['limbs'], form, e['tile']) for fam, entries in _tables(lib).items() for e in entries for form in e['forms']
               if (fam, e['limbs'], form, e['tile']) not in have]
    assert not missing, missing
    assert set(ct.F16_NEVER_PICKED) <= {c.tile for c in FORCED if c.family == 'f16'}


@pytest.mark.parametrize('name', NAMES)
def test_case_lands_on_its_form_tile_and_split_in_plan_only_mode(lib, name):
    tc = ct.BY_NAME[name]
    plan = tc.plan(lib)
    want = tc.want_plan()
    assert {k: plan[k] for k in want} == want, (name, plan)
    f = tc.facts()
    tiles_n = 1 if tc.form == 'rpn' else tc.channel_tiles()           # (the RpnHead workgroup walks its channel tiles itself)
    assert plan['blocks'] == (f['slabs'] + 7) // 8 * 8 * tiles_n * tc.ksplit, (name, plan, f)


def test_plan_only_mode_and_overrides_are_cleared_by_the_context_manager():
    from tools import _diag
    from tf_eager_object_detection_amd import _lib
    tc = next(c for c in FORCED if c.family == 'f32')
    with _diag.diag_library() as lib:
        tc.force(lib)
        lib.odet_debug_plan_only(1)
    h = _diag.diag_handle()
    before = ct.plan_count(h, 'f32')
    # plan-only is off again: the same call now goes on to the kernels' set-up, which needs a device -- or launches on one
    rc = tc._abi_call(h, _lib) if not torch.cuda.is_available() else None
    if rc is not None:
        assert rc != 0 and b' failed: ' in h.odet_last_error()
        assert ct.plan_count(h, 'f32') == before
    # and the override is gone: in plan-only mode the launcher's own pick comes back, unforced
    h.odet_debug_plan_only(1)
    try:
        assert tc._abi_call(h, _lib) == 0
        assert not _diag.last_plan('f32', h)['forced']
    finally:
        h.odet_debug_plan_only(0)


# ---- the coverage rules, computed from the table ---------------------------------------------------------------------------------

def _by_tile():
    out = {}
    for c in FORCED:
        out.setdefault((c.family, c.limbs, c.tile), []).append(c)
    return out


DEEP_K = 16        # K-steps: eight times the stages of a two-stage loop -- the steady-state body runs many times between
#                    prologue and drain (the split forms' loop is unrolled NA = 2 or 3 steps and peels 2 NS - 1 at the end)


def test_slab_rules_hold_for_every_tile():
    for key, cases in sorted(_by_tile().items()):
        facts = [c.facts() for c in cases]
        TM = ct.tile_pixels(key[2])
        assert any(f['partial'] for f in facts), key                   # M is not a multiple of TM
        assert any(f['cut_row'] for f in facts), key                   # a slab ends inside an image row
        assert any(f['spans_border'] and c.args['B'] >= 2 for f, c in zip(facts, cases)), key
        assert any(f['slabs'] % 8 for f in facts), key                 # padded workgroups of the (slabs + 7) / 8 * 8 grid
        assert any(c.channel_tiles() >= 2 for c in cases), key
        multi = [c for c in cases if c.form == 'plain' and len(c.maps()) >= 2]
        assert any(c.facts()['smallest'] < TM for c in multi), key    # a level smaller than one tile in a multi-level launch


def test_k_depth_rules_hold_for_every_tile():
    for (family, limbs, tile), cases in sorted(_by_tile().items()):
        ks = [c.ksteps() for c in cases if c.ksplit == 1]
        ns = tile[3]
        if family == 'f16' and ns > 2:                                 # rings
            assert min(ks) < ns and max(ks) > 2 * ns, (tile, ks)
        elif family == 'split':
            pw = {c.ksteps() for c in cases if c.form == 'pointwise' and c.ksplit == 1}
            assert {1, 2, 3} <= pw and max(pw) >= DEEP_K, (limbs, tile, pw)
        else:
            # the shortest K any entry point of the family takes: two K-steps (pointwise: cin >= 2 K-steps)
            assert min(ks) == 2 and max(ks) >= DEEP_K, (family, tile, ks)


def test_every_split_tile_has_the_forced_k_splits_in_both_forms():
    for (family, limbs, tile), cases in sorted(_by_tile().items()):
        if family != 'split':
            assert all(c.ksplit == 1 for c in cases)
            continue
        have = {(c.form, c.ksplit) for c in cases if c.ksplit > 1}
        assert have == {(form, S) for form in ('plain', 'pointwise') for S in ct.FORCED_KSPLITS}, (limbs, tile, have)
        assert all(c.ksplit <= c.ksteps() for c in cases)             # (a split wider than K is dropped by the override)
        assert any(c.ksteps() % c.ksplit for c in cases if c.ksplit > 1), (limbs, tile)      # parts of unequal length


def test_every_tile_height_shapes_pick_five_distinct_tiles(lib):
    tiles = [t for _, t in ct.EVERY_TILE_HEIGHT]
    assert sorted(tiles) == [(8, 4, mt, 2) for mt in (4, 5, 6, 7, 8)]
    got = [ct.BY_NAME[c.name].plan(lib)['tile'] for c in ct.CASES
           if c.mode == 'natural' and c.family == 'f16' and c.op == 'conv3x3' and (c.args['H'], c.args['W']) in dict(ct.EVERY_TILE_HEIGHT)
           and c.args['cout'] == 256 and c.args['cin'] == 64 and c.args['B'] == 1]
    assert sorted(set(got)) == sorted(tiles)
    # the shapes the test ran before are still in the table (nothing that was asserted is lost)
    kept = {(c.args['H'], c.args['W']) for c in ct.CASES if c.mode == 'natural' and c.family == 'f16' and c.op == 'conv3x3'}
    assert {(20, 84), (328, 100), (209, 200), (300, 167), (349, 167)} <= kept


# ---- the launchers' own picks over a sweep of shapes ---------------------------------------------------------------------------

SWEEP_MAPS = [(7, 9), (13, 21), (20, 33), (25, 42), (37, 45), (50, 84), (64, 96), (75, 100), (100, 167), (113, 100), (128, 250),
              (100, 334), (150, 201), (191, 250), (170, 334), (191, 334), (200, 334)]


def _sweep(lib):
    reached = set()

    def go(family, form, op, args, limbs=1):
        try:
            p = ct.TileCase(family, form, (0, 0, 0, 0), op, args, mode='natural', limbs=limbs).plan(lib)
        except AssertionError:
            return                                                     # (a shape the entry point refuses)
        assert not p['forced']
        reached.add((family, limbs, form, p['tile']))
    for B in (1, 2):
        for H, W in SWEEP_MAPS:
            for cout in (64, 128, 192, 256, 512):
                for cin in (64, 128):
                    go('f16', 'plain', 'conv3x3', dict(B=B, H=H, W=W, cin=cin, cout=cout))
                    go('f16', 'pooled', 'pool', dict(B=B, H=H, W=W, cin=cin, cout=cout))
                for cin in (128, 256, 1024):
                    go('f16', 'pointwise', 'pointwise', dict(B=B, H=H, W=W, cin=cin, cout=cout))
                if cout in (64, 128, 256):
                    go('f16', 'tail', 'tail', dict(B=B, H=H, W=W, cin=64, cout=cout, n3=128))
                if cout in (256, 512):
                    go('f16', 'rpn', 'rpn', dict(B=B, A=3, shapes=((H, W),), cin=64, cout=cout))
                go('f32', 'plain', 'conv3x3', dict(B=B, H=H, W=W, cin=32, cout=cout))
                go('f32', 'pointwise', 'pointwise', dict(B=B, H=H, W=W, cin=64, cout=cout))
                for limbs in (3, 2):
                    for cin in (32, 256):
                        go('split', 'plain', 'conv3x3', dict(B=B, H=H, W=W, cin=cin, cout=cout), limbs)
                    for cin in (64, 512):
                        go('split', 'pointwise', 'pointwise', dict(B=B, H=H, W=W, cin=cin, cout=cout), limbs)
    return reached


def test_every_tile_a_picker_reaches_has_a_natural_case(lib):
    reached = _sweep(lib)
    natural = {(c.family, c.limbs, c.form, c.tile) for c in ct.CASES if c.mode == 'natural'}
    assert not sorted(reached - natural, key=str), sorted(reached - natural, key=str)
    # the pickers never choose these three for any shape of the sweep, in any form: they run forced only
    assert {t for fam, _, _, t in reached if fam == 'f16'} == set(ct.F16_TWO_STAGE + ct.F16_RINGS) - set(ct.F16_NEVER_PICKED)
    assert len(reached) >= 70


# ---- the data ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', [c.name for c in ct.CASES if c.family == 'f16'])
def test_float16_case_is_exact_in_float32_and_sharp(name):
    tc = ct.BY_NAME[name]
    case = tc.build()
    assert case.worst_quanta < ed.F32_EXACT
    case.assert_not_vacuous()
    launches = tc.f16_launches(case)
    assert launches
    for what, call, want, pre in launches:
        assert all(w.dtype in (torch.float16, torch.float32) and bool(torch.isfinite(w.float()).all()) for w in want)


@pytest.mark.parametrize('name', [c.name for c in ct.CASES if c.family != 'f16'])
def test_float32_case_is_proved_exact_and_its_expected_values_are_float32(name):
    tc = ct.BY_NAME[name]
    case = tc.build()                                                  # (prove_f32_exact runs inside, per variant)
    assert case.worst_quanta < ed.F32_EXACT
    kinds = [v.limb_kind for v in case.variants if v.limb_kind]
    assert kinds == (list(ct.LIMB_KINDS[tc.limbs]) if tc.data == 'limbs' else [])
    for v in case.variants:
        for w in v.want:
            assert torch.equal(w.float().double(), w) and float(w.abs().max()) > 0
            assert float((w != 0).double().mean()) > 0.2               # (a ReLU zeroes about half)


def test_integer_data_lives_in_the_top_limb_alone_and_the_limb_data_does_not():
    """why the limb-sensitive variants exist: on the integer data every limb below the top one is zero, so all kept products
    but one multiply by zero"""
    g = ed.Gen(1)
    x, w = g.ints((64, 96), ed.X_MAX), g.ints((64, 96), 15)
    for limbs in (3, 2):
        for t in (x, w):
            assert all(float(l.abs().max()) == 0 for l in ct.split_limbs(t, limbs, ct.f16x2_exponent(t))[1:])
        xl, wl, _ = ct.limb_operands(g, 'x_limbs', limbs, (64, 96), 64, 96)
        assert all(float((l != 0).double().mean()) > 0.5 for l in ct.split_limbs(xl, limbs))
        assert all(float(l.abs().max()) == 0 for l in ct.split_limbs(wl, limbs, ct.f16x2_exponent(wl))[1:])


@pytest.mark.parametrize('name', [c.name for c in ct.CASES if c.data == 'limbs'])
def test_every_kept_limb_product_changes_its_case_and_every_dropped_one_is_zero(name):
    """the float64 restatement of the kernel's sum of limb products (kept / dropped read from the kernel header): the kept
    products add up to the exact result, so the dropped ones are zero; zeroing any one product a variant is built to exercise
    changes more than a tenth of its expected outputs; over the variants of a case every kept product is exercised"""
    tc = ct.BY_NAME[name]
    kept, dropped = ct.kept_products(tc.limbs)
    case = tc.build()
    exercised = set()
    for v in case.variants:
        if not v.limb_kind:
            continue
        prods, full = v.products
        for m in range(len(full)):
            assert torch.equal(sum(prods[k][m] for k in kept), full[m]), (name, v.name)
            for k in dropped:
                assert float(prods[k][m].abs().max()) == 0.0, (name, v.name, k)
        for k in ct.LIMB_KIND_PRODUCTS[(tc.limbs, v.limb_kind)]:
            assert k in kept
            changed = torch.cat([(torch.relu(full[m] - prods[k][m]) != v.want[m]).reshape(-1) for m in range(len(full))]).double().mean()
            assert float(changed) > 0.1, (name, v.name, k, float(changed))        # (of all outputs; the ReLU zeroes about half)
            exercised.add(k)
    assert exercised == set(kept), (name, exercised)


# ---- what the product launches ---------------------------------------------------------------------------------------------------

def test_every_tile_the_three_model_families_launch_has_a_case(lib):
    """the dense layers of ResNet-101-FPN, ResNet-50-C4 and VGG16 at batch 1, 2, 4 and 8, at the BASELINE image sizes, in float16
    and the three float32 forms, through the launchers' own picks: every instantiation a product launch reaches has a forced
    case and a natural one.  (DESIGN.md lists the reached instantiations and the ones no product launch reaches.)"""
    reached = ct.model_sweep(lib)
    forced = {c.instantiation() for c in ct.CASES if c.mode == 'forced'}
    natural = {c.instantiation() for c in ct.CASES if c.mode == 'natural'}
    assert set(reached) <= forced, sorted(set(reached) - forced, key=str)
    assert set(reached) <= natural, sorted(set(reached) - natural, key=str)
    models = {m for uses in reached.values() for m, _, _ in uses}
    assert models == set(ct.MODEL_IMAGES) and len(reached) >= 30
    assert not {t for fam, _, _, t in reached if fam == 'f16'} & set(ct.F16_NEVER_PICKED)
