"""CPU tests of the NMS driver's launch plan (csrc/nms.hip: nms_plan / nms_run), on the diagnostic library in plan-only mode:

 * known plans: the planning function alone (odet_debug_nms_plan) on the sizes the detectors run;
 * the rule: every field of a swept plan equals plan_of() below, the driver's decisions restated in plain Python;
 * the entry points hand the driver what they were given: odet_nms, odet_region_proposal, odet_fpn_proposals,
   odet_frcnn_proposals and a step batch, with pointer-valued integers for the device arrays -- the driver checks, plans,
   records (odet_debug_last_nms_plan) and returns before any HIP call."""
import ctypes as C

import numpy as np
import pytest

NMS_CHUNK, SEL_MAX, LDS_CAND, PREP_TILE, SEL_TILE = 4096, 8192, 1536, 512, 2048


@pytest.fixture(scope='module')
def lib():
    from tools import _diag
    h = _diag.diag_handle()
    yield h
    h.odet_debug_plan_only(0)


# ---- the rule, restated --------------------------------------------------------------------------------------------------------------

def tri(cap):
    nb = (cap + 63) // 64
    return nb * (nb + 1) // 2


def plan_of(n, K, first_chunk, blind_chunks, sync_free, B=1):
    blind = max(blind_chunks, 1)
    c = (K * 3 // 2 + 63) // 64 * 64                   # ~1.5 K candidates in whole 64-blocks ...
    if c > 64:
        c -= 32                                        # ... less half a block of slack for boundary ties
    if first_chunk > 0:
        c = max(c, (first_chunk + 63) // 64 * 64 - 32)
    target = min(max(c, 256), NMS_CHUNK, n)
    lds0 = target <= LDS_CAND
    limit = LDS_CAND if lds0 else NMS_CHUNK
    wide = bool(sync_free) and blind >= 2
    sel_limit = SEL_MAX if wide else limit
    cap = min(NMS_CHUNK, (n + 63) // 64 * 64)
    return {'n': n, 'K': K, 'first_chunk': first_chunk, 'B': B, 'sync_free': int(bool(sync_free)), 'blind': blind,
            'target': target, 'lds0': int(lds0), 'limit': limit, 'wide': int(wide),
            'sel_target': min(n, target + NMS_CHUNK) if wide else target, 'sel_limit': sel_limit,
            'prep_grid': -(-n // PREP_TILE), 'sel_grid': -(-n // SEL_TILE), 'rank_wgs': (min(n, sel_limit) + 63) // 64,
            'cap0': min(limit, cap), 'tiles0': tri(min(limit, cap)), 'cap': cap, 'tiles': tri(cap),
            'further': blind - 1 if sync_free else 0,
            'sel_chunks': 1 if sync_free and blind >= 2 else 0,
            'full_sort': 1 if sync_free and blind >= 3 else 0,
            'fail_empty_chunk': blind - 1 if sync_free else -1,
            'max_chunks': 0 if sync_free else -(-n // NMS_CHUNK) + 1}


def chunks_of(p):
    """the chunks a plan enqueues without asking the host: (chunk, source, carries fail_empty)"""
    out = [(0, 'selection', p['fail_empty_chunk'] == 0)]
    for c in range(1, p['further'] + 1):
        out.append((c, 'selection' if c <= p['sel_chunks'] else 'full order', p['fail_empty_chunk'] == c))
    return out


# ---- (a) known plans -----------------------------------------------------------------------------------------------------------------

KNOWN = {
    # name: (n, K, first_chunk, blind, sync_free), expected fields
    'A': ((267069, 1000, 0, 1, True), dict(target=1504, lds0=1, limit=1536, wide=0, sel_target=1504, sel_limit=1536, prep_grid=522,
                                           sel_grid=131, rank_wgs=24, cap0=1536, tiles0=300, further=0)),
    'B': ((267069, 1000, 0, 2, True), dict(target=1504, lds0=1, limit=1536, wide=1, sel_target=5600, sel_limit=8192, prep_grid=522,
                                           sel_grid=131, rank_wgs=128, cap0=1536, tiles0=300, further=1, cap=4096, tiles=2080,
                                           sel_chunks=1, full_sort=0, fail_empty_chunk=1)),
    'B_blind3': ((267069, 1000, 0, 3, True), dict(target=1504, lds0=1, limit=1536, wide=1, sel_target=5600, sel_limit=8192,
                                                  prep_grid=522, sel_grid=131, rank_wgs=128, cap0=1536, tiles0=300, further=2,
                                                  cap=4096, tiles=2080, sel_chunks=1, full_sort=1, fail_empty_chunk=2)),
    'C': ((267069, 1000, 4096, 1, True), dict(target=4064, lds0=0, limit=4096, wide=0, sel_target=4064, sel_limit=4096,
                                              prep_grid=522, sel_grid=131, rank_wgs=64, cap0=4096, tiles0=2080, further=0)),
    'D': ((3000, 2000, 0, 1, False), dict(target=2976, lds0=0, limit=4096, wide=0, sel_target=2976, sel_limit=4096, rank_wgs=47,
                                          cap0=3008, tiles0=1128, further=0, max_chunks=2, fail_empty_chunk=-1)),
    'E': ((4, 10, 0, 1, False), dict(target=4, lds0=1, limit=1536, wide=0, sel_target=4, sel_limit=1536, prep_grid=1, sel_grid=1,
                                     rank_wgs=1, cap0=64, tiles0=1)),
}


@pytest.mark.parametrize('name', sorted(KNOWN))
def test_known_plans(lib, name):
    from tools import _diag
    args, want = KNOWN[name]
    p = _diag.nms_plan(*args, handle=lib)
    assert {k: p[k] for k in want} == want
    assert p == plan_of(*args)


def test_known_plans_further_chunks(lib):
    from tools import _diag
    b2 = _diag.nms_plan(*KNOWN['B'][0], handle=lib)
    assert chunks_of(b2) == [(0, 'selection', False), (1, 'selection', True)] and not b2['full_sort']
    b3 = _diag.nms_plan(*KNOWN['B_blind3'][0], handle=lib)
    assert chunks_of(b3) == [(0, 'selection', False), (1, 'selection', False), (2, 'full order', True)] and b3['full_sort']


# ---- (b) the rule --------------------------------------------------------------------------------------------------------------------

def test_plan_sweep_equals_the_restated_rule(lib):
    from tools import _diag
    checked = 0
    for n in (1, 63, 64, 65, 255, 256, 257, 1535, 1536, 1537, 4095, 4096, 4097, 8191, 8193, 120015, 446118):
        for K in (1, 42, 43, 100, 300, 1000, 1024, 1045, 1046, 2000, 2752, 20000):
            for first_chunk in (0, 1, 1536, 1537, 4096):
                for blind in (0, 1, 2, 3, 17):
                    for sync_free in (True, False):
                        p = _diag.nms_plan(n, K, first_chunk, blind, sync_free, handle=lib)
                        assert p == plan_of(n, K, first_chunk, blind, sync_free), (n, K, first_chunk, blind, sync_free)
                        assert p['lds0'] == int(p['target'] <= 1536)
                        ch = chunks_of(p)
                        assert len(ch) == (p['blind'] if sync_free else 1)
                        assert sum(fe for _, _, fe in ch) == (1 if sync_free else 0)
                        assert not sync_free or ch[-1][2]                   # (the LAST sync-free chunk carries it)
                        checked += 1
    assert checked == 17 * 12 * 5 * 5 * 2
    # batches: the grids' second dimension, nothing else
    for B in (2, 8):
        assert _diag.nms_plan(267069, 1000, 0, 3, True, B, handle=lib) == plan_of(267069, 1000, 0, 3, True, B)


# ---- (c) the entry points ------------------------------------------------------------------------------------------------------------

FAKE = C.c_void_p(0x10000000)            # stands for every device array: nothing dereferences it in plan-only mode
WS = C.c_void_p(0x40000000)
M0 = (C.c_float * 4)(0, 0, 0, 0)
S1 = (C.c_float * 4)(1, 1, 1, 1)


def _fpn_tables():
    from tf_eager_object_detection_amd import synthetic as syn
    from tf_eager_object_detection_amd.utils.anchor_generator import fpn_level_tables
    fh, fw, wh = fpn_level_tables((800, 1333), syn.FPN_STRIDES, syn.FPN_BASE_SIZES, syn.FPN_SCALES, syn.FPN_RATIOS)
    wh = np.ascontiguousarray(wh, dtype=np.float32)
    return [int(v) for v in fh], [int(v) for v in fw], [int(v) for v in syn.FPN_STRIDES], wh


def _call(lib, name, n, K, blind, done, ws_bytes=None):
    """one plan-only call of entry point `name` -> (return code, n the driver should see)"""
    nb = getattr(lib, name + '_workspace_bytes')(n, K) if ws_bytes is None else ws_bytes
    if name == 'odet_nms':
        return lib.odet_nms(FAKE, FAKE, n, K, 0.7, FAKE, None, FAKE, blind, done, WS, nb, None)
    if name == 'odet_region_proposal':
        return lib.odet_region_proposal(FAKE, FAKE, FAKE, n, 800, 1333, M0, S1, K, 0.7, FAKE, FAKE, FAKE, blind, done, WS, nb, None)
    if name == 'odet_fpn_proposals':
        fh, fw, st, wh = _fpn_tables()
        nl = len(fh)
        return lib.odet_fpn_proposals(FAKE, FAKE, nl, wh.shape[1], (C.c_int * nl)(*fh), (C.c_int * nl)(*fw), (C.c_int * nl)(*st),
                                      wh.ctypes.data_as(C.c_void_p), 800, 1333, M0, S1, K, 0.7, 2, 5, FAKE, FAKE, FAKE, FAKE, FAKE,
                                      FAKE, FAKE, None, blind, done, WS, nb, None)
    base = np.arange(36, dtype=np.float32)
    return lib.odet_frcnn_proposals(FAKE, FAKE, base.ctypes.data_as(C.c_void_p), 9, 16, 38, 50, 600, 800, M0, S1, K, 0.7, FAKE, FAKE,
                                    FAKE, blind, done, WS, nb, None)


def _sizes(name):
    if name == 'odet_fpn_proposals':
        fh, fw, _, wh = _fpn_tables()
        return sum(a * b for a, b in zip(fh, fw)) * wh.shape[1], 1000
    return {'odet_nms': (9000, 100), 'odet_region_proposal': (267069, 2000), 'odet_frcnn_proposals': (38 * 50 * 9, 300)}[name]


ENTRY_POINTS = ('odet_nms', 'odet_region_proposal', 'odet_fpn_proposals', 'odet_frcnn_proposals')


@pytest.mark.parametrize('sync_free', [True, False])
@pytest.mark.parametrize('name', ENTRY_POINTS)
def test_entry_points_feed_the_plan_what_they_were_given(lib, name, sync_free):
    from tools import _diag
    n, K = _sizes(name)
    if name == 'odet_fpn_proposals':
        assert n == 267069
    for blind in (1, 3):
        before = _diag.last_nms_plan(lib)['count']
        lib.odet_debug_plan_only(1)
        try:
            rc = _call(lib, name, n, K, blind, FAKE if sync_free else None)
        finally:
            lib.odet_debug_plan_only(0)
        assert rc == 0, lib.odet_last_error()
        p = _diag.last_nms_plan(lib)
        assert p.pop('count') == before + 1
        assert p == plan_of(n, K, 0, blind, sync_free, 1)          # (none of the four entry points has a first_chunk argument)


@pytest.mark.parametrize('name', ENTRY_POINTS)
def test_trivial_results_record_nothing_and_touch_nothing_in_plan_only_mode(lib, name):
    from tools import _diag
    before = _diag.last_nms_plan(lib)['count']
    lib.odet_debug_plan_only(1)
    try:
        if name in ('odet_nms', 'odet_region_proposal'):
            assert _call(lib, name, 0, 10, 1, FAKE) == 0 and _call(lib, name, 10, 0, 1, None) == 0
        elif name == 'odet_frcnn_proposals':                      # (no anchors: an empty feature map)
            assert lib.odet_frcnn_proposals(FAKE, FAKE, np.arange(36, dtype=np.float32).ctypes.data_as(C.c_void_p), 9, 16, 0, 50, 600,
                                            800, M0, S1, 300, 0.7, FAKE, FAKE, FAKE, 1, FAKE, WS, 0, None) == 0
        else:
            z = (C.c_int * 1)(0)
            w = (C.c_int * 1)(8)
            wh = np.ones((1, 3, 2), np.float32)
            assert lib.odet_fpn_proposals(FAKE, FAKE, 1, 3, z, w, w, wh.ctypes.data_as(C.c_void_p), 800, 1333, M0, S1, 100, 0.7, 2, 5,
                                          FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None, 1, FAKE, WS, 0, None) == 0
    finally:
        lib.odet_debug_plan_only(0)
    assert _diag.last_nms_plan(lib)['count'] == before


@pytest.mark.parametrize('name', ENTRY_POINTS)
def test_too_small_workspace_is_still_refused(lib, name):
    from tools import _diag
    n, K = _sizes(name)
    need = getattr(lib, name + '_workspace_bytes')(n, K)
    before = _diag.last_nms_plan(lib)['count']
    lib.odet_debug_plan_only(1)
    try:
        rc = _call(lib, name, n, K, 1, FAKE, ws_bytes=need - 1)
    finally:
        lib.odet_debug_plan_only(0)
    assert rc == -2                                                 # ODET_E_WORKSPACE
    assert lib.odet_last_error().decode() == '%s: workspace too small (%d < %d)' % (name, need - 1, need)
    assert _diag.last_nms_plan(lib)['count'] == before


def _step(done, blind, first_chunk):
    from tf_eager_object_detection_amd import _lib
    fh, fw, st, wh = _fpn_tables()
    s = _lib.OdetFpnStep()
    s.image_h, s.image_w, s.num_levels, s.A = 800, 1333, len(fh), wh.shape[1]
    for l in range(len(fh)):
        s.fh[l], s.fw[l], s.stride[l] = fh[l], fw[l], st[l]
    for i, v in enumerate(wh.reshape(-1)):
        s.wh[i] = float(v)
    for k in range(4):
        s.rpn_means[k], s.rpn_stds[k] = 0.0, 1.0
    s.num_proposals, s.rpn_nms_iou, s.min_level, s.max_level = 1000, 0.7, 2, 5
    s.blind_chunks, s.nms_first_chunk = blind, first_chunk
    for f in ('rpn_logits', 'rpn_deltas', 'rois', 'roi_idx', 'roi_count', 'sorted_rois', 'roi_level', 'roi_perm', 'level_counts'):
        setattr(s, f, FAKE.value)
    s.nms_done = FAKE.value if done else None
    s.ws_rpn = WS.value
    return s


def test_step_batches_plan_one_job_for_all_images_and_need_the_sync_free_mode(lib):
    """odet_fpn_step_enqueue_batch, proposal stage only: the one caller that sets B > 1 and the step's nms_first_chunk"""
    from tools import _diag
    for done, blind, first_chunk in ((True, 3, 0), (True, 1, 4096), (False, 1, 0)):
        steps = [_step(done, blind, first_chunk) for _ in range(2)]
        for s in steps:
            s.ws_rpn_bytes = lib.odet_fpn_proposals_workspace_bytes(267069, 1000)
        ptrs = (C.c_void_p * 2)(*[C.addressof(s) for s in steps])
        before = _diag.last_nms_plan(lib)['count']
        lib.odet_debug_plan_only(1)
        try:
            rc = lib.odet_fpn_step_enqueue_batch(ptrs, 2, 1)         # ODET_STAGE_PROPOSALS
        finally:
            lib.odet_debug_plan_only(0)
        p = _diag.last_nms_plan(lib)
        if done:
            assert rc == 0, lib.odet_last_error()
            assert p.pop('count') == before + 1
            assert p == plan_of(267069, 1000, first_chunk, blind, True, 2)
        else:
            assert rc == -1 and lib.odet_last_error().decode() == 'odet_nms: batches need the sync-free mode (out_done)'
            assert p['count'] == before
