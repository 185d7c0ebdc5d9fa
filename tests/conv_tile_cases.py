"""One table of cases for the implicit-GEMM convolution kernels: which instantiation each case runs, on which shape and data.

The dense layers are built many times over (csrc/conv3x3.hip, conv_f32.hip, conv_x3.hip: MT, WN, NS, TAIL, BLK and NL are
template parameters, so fragment indexing, the stage ring, the counted waits, the lane-to-channel map of the epilogue and the
float16 store are separate machine code per instantiation) and host-side cost models choose between them.  A case names its
kernel -- family, form, tile {nw, wn, mt, ns}, limb count, K split -- and says whether the tile is FORCED through the
diagnostic build's override (include/odet_diag.h) or must be the launcher's own NATURAL pick; both halves of the suite check
that against `odet_debug_last_plan`: tests/test_conv_tiles_host.py in plan-only mode on the CPU, tests/test_conv_tiles_gpu.py
on the launch whose result it compares.

The tile lists below are written out, not read from the library: tests/test_conv_tiles_host.py holds them against
`odet_debug_tile_table`, so a tile added to a kernel file without a case here fails there.

Data.  float16 cases: the dyadic builders of tests/exact_data.py (exact in float32 in any order, sharp in float16; expected = the
float64 result rounded once).  Exact-float32 and split-precision cases: integer / dyadic data proved exact with the same
`prove_f32_exact`; expected = the float64 result itself.  The split forms also run LIMB-SENSITIVE data: one operand spans all
its limbs, the other fits one (both ways round, and two limbs x two limbs for the three-limb form), sparse weights so that the
proof holds; every limb product the kernel drops is zero by construction and every product it keeps changes the result
(`limb_products`, checked on the CPU).

Plain module (CPU only: torch on the CPU + numpy + ctypes); only `run_*` touch the GPU."""
import ctypes as C
import math
import os
import re

import torch

import exact_data as ed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16_BK, F32_BK = 64, 32                   # input channels per K-step (128 bytes of a pixel's row)

# ---- the tile lists ------------------------------------------------------------------------------------------------------------
# float16 (kTiles of csrc/conv3x3.hip): (nw, wn, mt, ns); the two-stage tiles have plain / pointwise / bottleneck-tail kernels
# and the plain kernel's pooling epilogue, the wn = 4 tiles of 4 .. 8 pixel tiles also the fused RpnHead kernel; the rings
# (ns > 2) plain and pointwise only
F16_TWO_STAGE = [(8, 4, mt, 2) for mt in (4, 5, 6, 7, 8)] + [(8, 2, mt, 2) for mt in (2, 3, 4)] + [(8, 1, 1, 2), (8, 1, 2, 2)] + \
                [(8, 4, 2, 2), (8, 4, 3, 2), (8, 2, 1, 2)]
F16_RINGS = [(4, 1, 1, 8), (4, 1, 1, 4)]
F16_RPN = [(8, 4, mt, 2) for mt in (4, 5, 6, 7, 8)]
# the three tiles no picker chooses for any shape swept (they ship, and tools force them)
F16_NEVER_PICKED = [(8, 4, 2, 2), (8, 4, 3, 2), (8, 2, 1, 2)]
# exact float32 (F32_FOR_TILES of csrc/conv_f32.hip): (mt, wn); three stages where TM % 64 == 0 and they fit 160 KB
F32_TILES = [(4, 4), (5, 4), (6, 4), (7, 4), (8, 4), (2, 2), (3, 2), (4, 2), (1, 1), (2, 1)]
# split precision (X3_FOR_TILES / X2_FOR_TILES of csrc/conv_x3.hip): (mt, wn) per limb count
SPLIT_TILES = {3: [(4, 2), (2, 2), (4, 4), (2, 1), (1, 1)], 2: [(2, 2), (4, 4), (2, 1), (1, 1)]}
FORCED_KSPLITS = (2, 8)


def f32_stages(mt, wn):
    tm, tn = (8 // wn) * 16 * mt, 64 * wn
    return 3 if tm % 64 == 0 and 3 * (tm + tn) * 128 <= 160 * 1024 else 2


def tile_of(family, limbs, mt, wn):
    """(nw, wn, mt, ns) as the last plan reports it for the float32 families"""
    return (8, wn, mt, f32_stages(mt, wn)) if family == 'f32' else (8, wn, mt, 3 if limbs == 2 else 2)


def tile_pixels(tile):
    nw, wn, mt, ns = tile
    return (nw // wn) * 16 * mt


# ---- shapes ----------------------------------------------------------------------------------------------------------------------

def slab_facts(B, maps, TM):
    """what the slabs of `TM` pixels do on maps [(H, W)] of batch B (one launch): partial last slab, a slab boundary inside an
    image row, a slab that holds pixels of two images, the slab count"""
    f = {'partial': False, 'cut_row': False, 'spans_border': False, 'slabs': 0, 'smallest': min(B * h * w for h, w in maps)}
    for H, W in maps:
        P, M = H * W, B * H * W
        n = (M + TM - 1) // TM
        f['slabs'] += n
        f['partial'] |= M % TM != 0
        f['cut_row'] |= any(((s * TM) % P) % W != 0 for s in range(1, n))
        f['spans_border'] |= any((i * P) % TM != 0 for i in range(1, B))
    return f


def pick_map(TM, B=2, even=False, both_even=False):
    """the smallest H x W (odd W: rows never line up with 16-pixel tiles) on which slabs of TM pixels are partial, cut a row,
    span the image border and do not fill a group of 8 -- three or more slabs, so that first, inner and last slab differ;
    both_even: H and W even (the map a top-down merge doubles)"""
    best = None
    for W in range(6, 40, 2) if both_even else range(5, 40, 2):
        for H in range(4, 60, 2) if both_even else range(3, 60):
            Hi, Wi = ((H + 1) & ~1, (W + 1) & ~1) if even else (H, W)       # (the pooled form's index space)
            f = slab_facts(B, [(Hi, Wi)], TM)
            if f['partial'] and f['cut_row'] and f['spans_border'] and 3 <= f['slabs'] <= 7 and (best is None or H * W < best[0]):
                best = (H * W, H, W)
    assert best is not None, TM
    return best[1], best[2]


SMALL_LEVEL = (3, 5)                      # 30 pixels at batch 2: smaller than the smallest tile (64 pixels)


# ---- the case ------------------------------------------------------------------------------------------------------------------

class TileCase:
    """family 'f16' / 'f32' / 'split'; form 'plain' / 'pointwise' / 'tail' / 'rpn' / 'pooled'; tile (nw, wn, mt, ns); mode
    'forced' / 'natural'; op + args: the entry point and its shape; data: which builder"""

    def __init__(self, family, form, tile, op, args, mode='forced', limbs=1, ksplit=1, data='dyadic'):
        self.family, self.form, self.tile, self.op, self.args = family, form, tuple(tile), op, dict(args)
        self.mode, self.limbs, self.ksplit, self.data = mode, limbs, ksplit, data
        a = self.args
        shape = '-'.join('%s%s' % (k, str(v).replace(' ', '')) for k, v in sorted(a.items()))
        self.name = '%s%s-%s-%dx%dx%dx%d%s-%s-%s-%s-%s' % (family, '' if limbs == 1 else limbs, form, *self.tile,
                                                          '' if ksplit == 1 else '-S%d' % ksplit, mode, op, data, shape)

    # -- geometry, for the coverage rules
    def maps(self):
        a = self.args
        if 'shapes' in a:
            return [tuple(s) for s in a['shapes']]
        H, W = a['H'], a['W']
        if self.form == 'pooled':
            return [((H + 1) & ~1, (W + 1) & ~1)]
        s = a.get('stride', 1)
        return [((H + s - 1) // s, (W + s - 1) // s)]

    def facts(self):
        return slab_facts(self.args['B'], self.maps(), tile_pixels(self.tile))

    def ksteps(self):
        bk = F16_BK if self.family == 'f16' else F32_BK
        return ((1 if self.form == 'pointwise' else 9) * self.args['cin'] + self.args.get('cin2', 0)) // bk

    def channel_tiles(self):
        return self.args['cout'] // (64 * self.tile[1])

    def instantiation(self):
        """the kernel this case runs: the pooled form is the plain form's kernel"""
        return (self.family, self.limbs, 'plain' if self.form == 'pooled' else self.form, self.tile)

    def want_plan(self):
        return {'family': self.family, 'form': self.form, 'tile': self.tile, 'limbs': self.limbs, 'ksplit': self.ksplit,
                'forced': self.mode == 'forced'}

    # -- the override (a diagnostic-library handle)
    def force(self, lib):
        clear_overrides(lib)
        if self.mode != 'forced':
            return
        nw, wn, mt, ns = self.tile
        if self.family == 'f16':
            rc = lib.odet_debug_conv_tile(1 if self.form == 'pointwise' else 0, nw, wn, mt, ns)
        elif self.family == 'f32':
            rc = lib.odet_debug_f32_tile(mt, wn)
        else:
            rc = lib.odet_debug_x3_tile(mt, wn, self.ksplit)
        assert rc == 0, self.name

    # -- plan only: the C ABI with pointer-valued integers nothing dereferences
    def plan(self, lib):
        """sets the override, calls the entry point in plan-only mode, returns the recorded plan (tools._diag.last_plan's dict)"""
        from tools import _diag
        from tf_eager_object_detection_amd import _lib
        self.force(lib)
        assert lib.odet_debug_plan_only(1) == 0
        try:
            before = plan_count(lib, self.family)
            rc = self._abi_call(lib, _lib)
            assert rc == 0, (self.name, rc, lib.odet_last_error())
            plan = _diag.last_plan(self.family, lib)
            assert plan['count'] == before + 1, self.name
            return plan
        finally:
            lib.odet_debug_plan_only(0)
            clear_overrides(lib)

    def _abi_call(self, lib, _lib):
        a, P = self.args, (lambda i: 0x100000 * (i + 1))          # 16-byte aligned, distinct
        B, cin, cout = a['B'], a['cin'], a['cout']
        lv = (_lib.OdetConvLevel * _lib.MAX_LEVELS)()
        maps = [tuple(s) for s in a['shapes']] if 'shapes' in a else [(a['H'], a['W'])]
        for i, (h, w) in enumerate(maps):
            lv[i].x, lv[i].y, lv[i].H, lv[i].W = P(20 + i), P(40 + i), h, w
        ws = (P(60), int(lib.odet_x3_workspace_bytes()))
        sfx = {'f16': 'f16', 'f32': 'f32', 'split': 'x%d' % self.limbs}[self.family]
        tail = {'f16': (None,), 'f32': (None,), 'split': ((0,) if self.limbs == 2 else ()) + ws + (None,)}[self.family]
        if self.op == 'conv3x3':
            return getattr(lib, 'odet_conv3x3_' + sfx)(P(0), P(1), P(2), P(3), B, a['H'], a['W'], cin, cout, 1, *tail)
        if self.op == 'conv3x3_levels':
            return getattr(lib, 'odet_conv3x3_%s_levels' % sfx)(lv, len(maps), P(1), P(2), B, cin, cout, 1, *tail)
        if self.op == 'pointwise':
            return getattr(lib, 'odet_pointwise_' + sfx)(P(0), P(1), P(2), P(4), P(3), B, a['H'], a['W'], a.get('stride', 1), cin, cout,
                                                          1, *tail)
        if self.op == 'lateral':
            return lib.odet_lateral_merge_f16(P(0), P(1), P(2), P(4), a['H'] // 2, a['W'] // 2, P(3), B, a['H'], a['W'], cin, cout, None)
        if self.op == 'dual':
            return lib.odet_pointwise_dual_f16(P(0), cin, P(4), a['cin2'], a['H'], a['W'], a['stride'], P(1), P(2), P(3), B, cout, 1, None)
        if self.op == 'pool':
            return lib.odet_conv3x3_relu_pool2_f16(P(0), P(1), P(2), P(3), B, a['H'], a['W'], cin, cout, None)
        if self.op == 'tail':
            return lib.odet_bottleneck_tail_f16(P(0), P(1), P(2), P(5), P(6), P(4), P(3), B, a['H'], a['W'], cin, cout, a['n3'], 1, None)
        if self.op == 'rpn':
            n = sum(h * w for h, w in maps) * a['A']
            for i in range(len(maps)):
                lv[i].y = None
            return lib.odet_rpn_head_fused_f16(lv, len(maps), P(1), P(2), P(5), P(6), a['A'], B, cin, cout, P(7), n * 2, P(8), n * 4, None)
        raise AssertionError(self.op)

    # -- data
    def build(self):
        """float16: an exact_data Case; float32 families: an F32Case"""
        a = self.args
        if self.family == 'f16':
            if self.op == 'conv3x3':
                return ed.conv3x3_case(a['B'], a['H'], a['W'], a['cin'], a['cout'], full=False)
            if self.op == 'conv3x3_levels':
                return ed.conv3x3_levels_case(a['B'], tuple(tuple(s) for s in a['shapes']), a['cin'], a['cout'])
            if self.op == 'pointwise':
                return ed.pointwise_case(a['B'], a['H'], a['W'], a['cin'], a['cout'], a.get('stride', 1))
            if self.op == 'lateral':
                return ed.lateral_case(a['B'], a['H'], a['W'], a['H'] // 2, a['W'] // 2, a['cin'])
            if self.op == 'dual':
                return ed.pointwise_dual_case(a['B'], a['H'], a['W'], a['cin'], a['cin2'], a['cout'], a['stride'])
            if self.op == 'pool':
                return ed.conv3x3_pool_case(a['B'], a['H'], a['W'], a['cin'], a['cout'])
            if self.op == 'tail':
                return ed.tail_case(a['B'], a['H'], a['W'], a['cin'], a['n3'], a['cout'])
            if self.op == 'rpn':
                return ed.rpn_fused_case(a['B'], a['A'], a['cin'], a['cout'], tuple(tuple(s) for s in a['shapes']))
            raise AssertionError(self.op)
        return f32_case(self)

    def f16_launches(self, case):
        """[(what, call(ops, d), want tensors, pre)]: ONE launch of the kernel under test each (the builders' two-launch
        comparison forms are tests/test_f16_rounding_gpu.py's business)"""
        out = []
        for v in case.variants:
            if self.op == 'tail':
                use_r = v.name.endswith('1')
                call = lambda ops, d, use_r=use_r: ops.conv3x3_conv1x1_f16(d['x'], d['w2'], d['b2'], d['w3'], d['b3'],
                                                                          residual=d['r'] if use_r else None, relu=True)
                out.append((v.name, call, v.want[:1], v.pre))
            elif self.op == 'rpn' and v.name != 'fused':
                continue
            elif self.op == 'lateral':
                key, b = ('exact', 'bi') if v.name.startswith('exact') else ('rounding', 'b')
                call = lambda ops, d, key=key, b=b: ops.lateral_merge(d['x_' + key], d['w_' + key], d[b], d['top'])
                out.append((v.name, call, v.want[:1], v.pre))
            else:
                out.append((v.name, v.call, v.want, v.pre))
        return out


def clear_overrides(lib):
    lib.odet_debug_conv_tile(0, 0, 0, 0, 0)
    lib.odet_debug_conv_tile(1, 0, 0, 0, 0)
    lib.odet_debug_f32_tile(0, 0)
    lib.odet_debug_x3_tile(0, 0, 0)


def plan_count(lib, family):
    """launches of the family recorded so far (0 before the first)"""
    from tools import _diag
    p = _diag.DebugPlan()
    lib.odet_debug_last_plan(_diag.FAMILIES.index(family), C.byref(p))        # (an error before the first launch: count stays 0)
    return p.count


# ---- exact-float32 and split-precision data --------------------------------------------------------------------------------------

def kept_products(limbs):
    """(kept, dropped) limb products (i, j) = x limb i times w limb j, 1 = the top limb, READ FROM THE KERNEL HEADER of
    csrc/conv_x3.hip: the three-limb sum "a1 b1 + (a1 b2 + a2 b1) + ... (dropped: ...)" of the file's head, the two-limb
    "h h ..., h l + l h ... (dropped: l l" of the tile's"""
    src = open(os.path.join(ROOT, 'tf_eager_object_detection_amd', 'csrc', 'conv_x3.hip')).read()
    if limbs == 3:
        m = re.search(r'a \. b\s+~\s+(.*?)\(dropped:(.*?)<=', src, flags=re.S)
        pairs = lambda s: [(int(i), int(j)) for i, j in re.findall(r'a(\d) b(\d)', s)]
    else:
        m = re.search(r'three products -- (.*?)\(dropped:(.*?)<=', src, flags=re.S)
        pairs = lambda s: [('hl'.index(i) + 1, 'hl'.index(j) + 1) for i, j in re.findall(r'\b([hl]) ([hl])\b', s)]
    assert m, 'the kernel header no longer states its limb products'
    kept, dropped = pairs(m.group(1)), pairs(m.group(2))
    assert len(set(kept)) == len(kept) == (6 if limbs == 3 else 3) and len(dropped) == (3 if limbs == 3 else 1)
    assert sorted(kept + dropped) == [(i, j) for i in range(1, limbs + 1) for j in range(1, limbs + 1)]
    return kept, dropped


def split_limbs(v64, limbs, w_exp=0):
    """the limbs of float32 values as csrc/conv_x3.hip splits them (x3_split2 / x2_split2), as float64 tensors whose sum is the
    value the kernel works with: three bfloat16 limbs, or float16 h and l * 2^-11 of v * 2^w_exp (scaled back)"""
    v = v64.float()
    assert torch.equal(v.double(), v64)
    if limbs == 3:
        a1 = v.bfloat16().float()
        r1 = v - a1
        a2 = r1.bfloat16().float()
        r2 = r1 - a2
        a3 = r2.bfloat16().float()
        out = [a1.double(), a2.double(), a3.double()]
    else:
        s = torch.ldexp(v, torch.tensor(w_exp))
        h = s.half().float()
        l = ((s - h) * 2048.0).half().float()
        out = [h.double() * 2.0 ** -w_exp, l.double() * 2.0 ** (-11 - w_exp)]
    assert all(bool(torch.isfinite(t).all()) for t in out)
    return out


def f16x2_exponent(w64):
    """ops.f16x2_exponent on the CPU: the largest |w| * 2^e lies in [512, 1024)"""
    top = float(w64.abs().max())
    return 0 if top == 0.0 else max(-100, min(100, 9 - math.frexp(top)[1] + 1))


LIMB_KINDS = {3: ('x_limbs', 'w_limbs', 'xw_two_limbs'), 2: ('x_limbs', 'w_limbs')}
# the products a kind makes non-zero (x limb, w limb); over the kinds of a limb count: every kept product
LIMB_KIND_PRODUCTS = {(3, 'x_limbs'): [(1, 1), (2, 1), (3, 1)], (3, 'w_limbs'): [(1, 1), (1, 2), (1, 3)],
                      (3, 'xw_two_limbs'): [(1, 1), (1, 2), (2, 1), (2, 2)],
                      (2, 'x_limbs'): [(1, 1), (2, 1)], (2, 'w_limbs'): [(1, 1), (1, 2)]}
SPARSE_NNZ = 4                            # non-zero weights per output channel of the limb-sensitive data


def _wide(g, shape, lo_bits, hi_bits, s):
    """+-n * 2^-s, n uniform in [2^lo_bits, 2^hi_bits): more than lo_bits significant bits"""
    n = torch.randint(2 ** lo_bits, 2 ** hi_bits, tuple(shape), generator=g.g).double()
    sign = 2 * torch.randint(0, 2, tuple(shape), generator=g.g).double() - 1
    return n * sign * 2.0 ** -s


def _small(g, shape, amax=3):
    """non-zero integers in [-amax, amax]"""
    n = torch.randint(1, amax + 1, tuple(shape), generator=g.g).double()
    return n * (2 * torch.randint(0, 2, tuple(shape), generator=g.g).double() - 1)


def _sparse_mask(g, cout, K):
    m = torch.zeros(cout, K, dtype=torch.float64)
    idx = torch.rand(cout, K, generator=g.g).argsort(dim=1)[:, :SPARSE_NNZ]
    m.scatter_(1, idx, 1.0)
    return m


def limb_operands(g, kind, limbs, x_shape, cout, K):
    """(x [x_shape], w [cout, K], quantum): one operand spans all its limbs, the other fits one; w has SPARSE_NNZ non-zeros per row.
    20 significant bits: the remainder after the top bfloat16 limb (8 bits, round to nearest) then has up to 11, so the third
    limb is non-zero for most values -- with 18 bits it is for one value in six --; two float16 limbs take 11 + 9.  The bound of
    the proof: 4 weights x 3 x 2^20 quanta = 0.75 x 2^24.  Two limbs x two limbs: 10 bits each."""
    mask = _sparse_mask(g, cout, K)
    if kind == 'x_limbs':
        return _wide(g, x_shape, 19, 20, 16), _small(g, (cout, K)) * mask, 2.0 ** -16
    if kind == 'w_limbs':
        return _small(g, x_shape), _wide(g, (cout, K), 19, 20, 16) * mask, 2.0 ** -16
    assert kind == 'xw_two_limbs' and limbs == 3
    return _wide(g, x_shape, 9, 10, 9), _wide(g, (cout, K), 9, 10, 9) * mask, 2.0 ** -18


class F32Variant:
    def __init__(self, name, tensors, want, run, limb_kind=None, products=None):
        self.name, self.tensors, self.want, self.run, self.limb_kind, self.products = name, tensors, want, run, limb_kind, products


class F32Case:
    """variants: [F32Variant]; want = the float64 results (lists, one tensor per map); run(ops, d) -> list of float32 tensors"""

    def __init__(self, name, variants, worst_quanta):
        self.name, self.variants, self.worst_quanta = name, variants, worst_quanta


def _contract(tc, xs, w):
    """(float64 result per map, absolute-value contraction per map) of the case's operation without its epilogue; w [cout, K]"""
    a = tc.args
    if tc.form == 'pointwise':
        s = a.get('stride', 1)
        return [ed.gemm_acc(x[:, ::s, ::s], w) for x in xs]
    w4 = w.view(a['cout'], 3, 3, a['cin']).permute(0, 3, 1, 2)
    return [ed.conv3x3_acc(x, w4) for x in xs]


def _weight_tensor(tc, w):
    a = tc.args
    if tc.form == 'pointwise':
        return w.float().contiguous()
    return w.view(a['cout'], 3, 3, a['cin']).permute(0, 3, 1, 2).float().contiguous(memory_format=torch.channels_last)


def _f32_run(tc, nmaps, use_bias, use_res):
    a = tc.args

    def run(ops, d):
        b = d['b'] if use_bias else None
        if tc.op == 'pointwise':
            return [pointwise_f32(ops, d['x0'], d['w'], b, d['r'] if use_res else None, True, a.get('stride', 1))]
        if tc.op == 'conv3x3':
            return [ops.conv3x3_f32(d['x0'], d['w'], b, relu=True)]
        return ops.conv3x3_f32_levels([d['x%d' % i] for i in range(nmaps)], d['w'], b, relu=True)
    return run


def pointwise_f32(ops, x, w, bias, residual, relu, stride):
    """ops.pointwise; the split forms' one-K-step layer (cin = 32) goes to the C ABI directly: the Python wrapper asks every
    form for the exact form's two K-steps, the split forms' entry points take one (csrc/conv_x3.hip)"""
    cin = int(x.shape[3])
    if cin >= 2 * F32_BK or ops.current_f32_form() == 'exact':
        return ops.pointwise(x, w, bias, residual, relu, stride)
    from tf_eager_object_detection_amd import _lib as L
    B, H, W = (int(v) for v in x.shape[:3])
    cout = int(w.shape[0])
    out = torch.empty((B, (H + stride - 1) // stride, (W + stride - 1) // stride, cout), dtype=torch.float32, device=x.device)
    ws, sym, wp, extra = ops._f32_sym('odet_pointwise_%s', w, w)
    ops._f32_call(ws, sym, L.dptr(x), wp, L.dptr(bias) if bias is not None else None,
                  L.dptr(residual) if residual is not None else None, L.dptr(out), B, H, W, stride, cin, cout, 1 if relu else 0,
                  *extra, L.stream())
    return out


def f32_case(tc):
    """integer data (activations |x| <= 63, weights |w| <= 15, bias and shortcut in quarters, ReLU) for both float32 families;
    the split family adds its limb-sensitive variants (no bias: the contraction alone)"""
    a = tc.args
    g = ed.Gen(4243 + a['cin'] * 7 + a['cout'] + tc.limbs * 100003 + sum(tc.tile) * 17 + tc.ksplit)
    maps = [tuple(s) for s in a['shapes']] if 'shapes' in a else [(a['H'], a['W'])]
    K = a['cin'] * (1 if tc.form == 'pointwise' else 9)
    cout, B = a['cout'], a['B']
    variants, worst = [], 0.0
    xs = [g.ints((B, h, w, a['cin']), ed.X_MAX) for h, w in maps]
    w = g.ints((cout, K), 15)
    b = g.quanta((cout,), 12, 2)
    accs = _contract(tc, xs, w)
    use_res = tc.form == 'pointwise'
    r = g.quanta(tuple(accs[0][0].shape), 64, 2) if use_res else None
    extra = b.abs() + (r.abs().max() if use_res else 0.0)
    worst = max(ed.prove_f32_exact(ab + extra, 0.25, integers=tuple(xs) + (w,), quanta=(b,) + ((r,) if use_res else ()))
                for _, ab in accs)
    want = [torch.relu(acc + b + (r if use_res else 0.0)) for acc, _ in accs]
    tensors = {'w': _weight_tensor(tc, w), 'b': b.float()}
    tensors.update({'x%d' % i: x.float() for i, x in enumerate(xs)})
    if use_res:
        tensors['r'] = r.float()
    variants.append(F32Variant('integers', tensors, want, _f32_run(tc, len(maps), True, use_res)))
    if tc.family == 'split' and tc.data == 'limbs':
        for kind in LIMB_KINDS[tc.limbs]:
            xl, wl, q = [], None, None
            for i, (h, w_) in enumerate(maps):
                x_, wl_, q = limb_operands(g, kind, tc.limbs, (B, h, w_, a['cin']), cout, K)
                xl.append(x_)
                wl = wl_ if wl is None else wl
            prods, abs_tot = limb_products(tc, xl, wl)
            worst = max(worst, max(ed.prove_f32_exact(t, q, quanta=tuple(xl) + (wl,)) for t in abs_tot))
            full = [acc for acc, _ in _contract(tc, xl, wl)]
            t = {'w': _weight_tensor(tc, wl)}
            t.update({'x%d' % i: x.float() for i, x in enumerate(xl)})
            variants.append(F32Variant(kind, t, [torch.relu(f) for f in full], _f32_run(tc, len(maps), False, False), kind,
                                       (prods, full)))
    return F32Case(tc.name, variants, worst)


def limb_products(tc, xs, w):
    """{(i, j): [float64 contraction of x limb i with w limb j, per map]} and the absolute-value contraction over ALL limb
    pairs per map (the bound on every partial sum of every order in which the kernel may add its limb products)"""
    w_exp = f16x2_exponent(w) if tc.limbs == 2 else 0
    wl = split_limbs(w, tc.limbs, w_exp)
    xl = [split_limbs(x, tc.limbs) for x in xs]
    prods = {}
    for i in range(tc.limbs):
        for j in range(tc.limbs):
            prods[(i + 1, j + 1)] = [acc for acc, _ in _contract(tc, [l[i] for l in xl], wl[j])]
    xa = [sum(t.abs() for t in l) for l in xl]
    wa = sum(t.abs() for t in wl)
    abs_tot = [ab for _, ab in _contract(tc, xa, wa)]
    return prods, abs_tot


# ---- the table -------------------------------------------------------------------------------------------------------------------

def _forced_f16():
    out = []
    for tile in F16_TWO_STAGE + F16_RINGS:
        nw, wn, mt, ns = tile
        TM, TN = tile_pixels(tile), 64 * wn
        H, W = pick_map(TM)
        # plain: two maps in one launch (the second smaller than one tile), two channel tiles; rings: K deeper than two rings
        out.append(TileCase('f16', 'plain', tile, 'conv3x3_levels',
                            dict(B=2, shapes=((H, W), SMALL_LEVEL), cin=128 if ns > 2 else 64, cout=2 * TN)))
        # pointwise: the shortest K the entry point takes (two K-steps: fewer than any ring has stages)
        out.append(TileCase('f16', 'pointwise', tile, 'pointwise', dict(B=2, H=H, W=W, cin=128, cout=2 * TN)))
        # the pointwise kernel's other epilogue and operand paths: the top-down merge, two sources along K (the second strided)
        He, We = pick_map(TM, both_even=True)
        out.append(TileCase('f16', 'pointwise', tile, 'lateral', dict(B=2, H=He, W=We, cin=128, cout=256)))
        out.append(TileCase('f16', 'pointwise', tile, 'dual', dict(B=2, H=2 * H - 1, W=2 * W - 1, cin=64, cin2=128, cout=2 * TN, stride=2)))
        if ns == 2:
            out.append(TileCase('f16', 'tail', tile, 'tail', dict(B=2, H=H, W=W, cin=128, cout=TN, n3=128)))
            Hp, Wp = pick_map(TM, even=True)
            out.append(TileCase('f16', 'pooled', tile, 'pool', dict(B=2, H=Hp, W=Wp, cin=128, cout=2 * TN)))
        if tile in F16_RPN:
            out.append(TileCase('f16', 'rpn', tile, 'rpn', dict(B=2, A=3, shapes=((H, W), SMALL_LEVEL), cin=64, cout=512)))
    return out


def _forced_f32():
    out = []
    for mt, wn in F32_TILES:
        tile = tile_of('f32', 1, mt, wn)
        H, W = pick_map(tile_pixels(tile))
        out.append(TileCase('f32', 'plain', tile, 'conv3x3_levels', dict(B=2, shapes=((H, W), SMALL_LEVEL), cin=64, cout=128 * wn),
                            data='integers'))
        out.append(TileCase('f32', 'pointwise', tile, 'pointwise', dict(B=2, H=H, W=W, cin=64, cout=128 * wn), data='integers'))
    return out


def _forced_split():
    out = []
    for limbs, tiles in SPLIT_TILES.items():
        for mt, wn in tiles:
            tile = tile_of('split', limbs, mt, wn)
            H, W = pick_map(tile_pixels(tile))
            mk = lambda form, op, args, **kw: out.append(TileCase('split', form, tile, op, args, limbs=limbs, **kw))
            mk('plain', 'conv3x3_levels', dict(B=2, shapes=((H, W), SMALL_LEVEL), cin=64, cout=128 * wn), data='limbs')
            for cin in (32, 64, 96):                      # 1, 2, 3 K-steps: the branches of the kernel's counted waits
                mk('pointwise', 'pointwise', dict(B=2, H=H, W=W, cin=cin, cout=128 * wn), data='limbs' if cin == 96 else 'integers')
            mk('pointwise', 'pointwise', dict(B=2, H=H, W=W, cin=512, cout=64 * wn), data='integers')        # deep: 16 K-steps
            for S in FORCED_KSPLITS:
                mk('plain', 'conv3x3', dict(B=2, H=H, W=W, cin=32, cout=128 * wn), ksplit=S, data='integers')        # 9 K-steps
                mk('pointwise', 'pointwise', dict(B=2, H=H, W=W, cin=256, cout=128 * wn), ksplit=S, data='integers')  # 8 K-steps
    return out


# Natural cases: shapes on which the launcher's own pick IS the tile (no override); confirmed in plan-only mode by
# tests/test_conv_tiles_host.py.  float16 3x3, cin 64 -> cout 256: the five 256-channel tile heights -- what
# tests/test_detector.py's test_conv3x3_f16_every_tile_height runs --, then that test's earlier shapes (picks written next to them)
EVERY_TILE_HEIGHT = [((128, 250), (8, 4, 4, 2)), ((100, 334), (8, 4, 5, 2)), ((191, 250), (8, 4, 6, 2)), ((170, 334), (8, 4, 7, 2)),
                     ((191, 334), (8, 4, 8, 2))]
EARLIER_TILE_HEIGHT_SHAPES = [((20, 84), (4, 1, 1, 8)), ((328, 100), (8, 4, 5, 2)), ((209, 200), (8, 2, 2, 2)), ((300, 167), (8, 2, 2, 2)),
                              ((349, 167), (8, 2, 2, 2))]


def _natural():
    out = []
    for (H, W), tile in EVERY_TILE_HEIGHT + EARLIER_TILE_HEIGHT_SHAPES:
        out.append(TileCase('f16', 'plain', tile, 'conv3x3', dict(B=1, H=H, W=W, cin=64, cout=256), mode='natural'))
    for family, form, tile, op, args, limbs, ksplit in NATURAL_PICKS:
        out.append(TileCase(family, form, tile, op, args, mode='natural', limbs=limbs, ksplit=ksplit,
                            data='dyadic' if family == 'f16' else 'integers'))
    return out


# (family, form, tile, op, args, limbs, ksplit): found by sweeping small shapes through the launchers in plan-only mode
NATURAL_PICKS = [
    ('f16', 'plain', (4, 1, 1, 4), 'conv3x3', dict(B=1, H=100, W=167, cin=64, cout=64), 1, 1),
    ('f16', 'plain', (4, 1, 1, 8), 'conv3x3', dict(B=1, H=7, W=9, cin=64, cout=64), 1, 1),
    ('f16', 'plain', (8, 1, 1, 2), 'conv3x3', dict(B=1, H=100, W=334, cin=64, cout=64), 1, 1),
    ('f16', 'plain', (8, 1, 2, 2), 'conv3x3', dict(B=1, H=200, W=334, cin=64, cout=64), 1, 1),
    ('f16', 'plain', (8, 2, 2, 2), 'conv3x3', dict(B=1, H=100, W=167, cin=64, cout=128), 1, 1),
    ('f16', 'plain', (8, 2, 3, 2), 'conv3x3', dict(B=1, H=200, W=334, cin=64, cout=128), 1, 1),
    ('f16', 'plain', (8, 2, 4, 2), 'conv3x3', dict(B=1, H=191, W=334, cin=64, cout=128), 1, 1),
    ('f16', 'pointwise', (4, 1, 1, 4), 'pointwise', dict(B=1, H=100, W=167, cin=128, cout=64), 1, 1),
    ('f16', 'pointwise', (4, 1, 1, 8), 'pointwise', dict(B=1, H=7, W=9, cin=128, cout=64), 1, 1),
    ('f16', 'pointwise', (8, 1, 1, 2), 'pointwise', dict(B=1, H=100, W=334, cin=128, cout=64), 1, 1),
    ('f16', 'pointwise', (8, 1, 2, 2), 'pointwise', dict(B=1, H=191, W=334, cin=128, cout=64), 1, 1),
    ('f16', 'pointwise', (8, 2, 2, 2), 'pointwise', dict(B=1, H=100, W=167, cin=128, cout=128), 1, 1),
    ('f16', 'pointwise', (8, 2, 3, 2), 'pointwise', dict(B=1, H=113, W=100, cin=128, cout=512), 1, 1),
    ('f16', 'pointwise', (8, 2, 4, 2), 'pointwise', dict(B=1, H=191, W=334, cin=128, cout=128), 1, 1),
    ('f16', 'pointwise', (8, 4, 4, 2), 'pointwise', dict(B=1, H=128, W=250, cin=128, cout=256), 1, 1),
    ('f16', 'pointwise', (8, 4, 5, 2), 'pointwise', dict(B=1, H=100, W=167, cin=128, cout=512), 1, 1),
    ('f16', 'pointwise', (8, 4, 6, 2), 'pointwise', dict(B=1, H=191, W=250, cin=128, cout=256), 1, 1),
    ('f16', 'pointwise', (8, 4, 7, 2), 'pointwise', dict(B=1, H=170, W=334, cin=128, cout=256), 1, 1),
    ('f16', 'pointwise', (8, 4, 8, 2), 'pointwise', dict(B=1, H=191, W=334, cin=128, cout=256), 1, 1),
    ('f16', 'pooled', (8, 1, 1, 2), 'pool', dict(B=1, H=7, W=9, cin=64, cout=64), 1, 1),
    ('f16', 'pooled', (8, 1, 2, 2), 'pool', dict(B=1, H=200, W=334, cin=64, cout=64), 1, 1),
    ('f16', 'pooled', (8, 2, 3, 2), 'pool', dict(B=1, H=200, W=334, cin=64, cout=128), 1, 1),
    ('f16', 'pooled', (8, 2, 4, 2), 'pool', dict(B=1, H=7, W=9, cin=64, cout=128), 1, 1),
    ('f16', 'pooled', (8, 4, 4, 2), 'pool', dict(B=1, H=7, W=9, cin=64, cout=256), 1, 1),
    ('f16', 'pooled', (8, 4, 5, 2), 'pool', dict(B=1, H=100, W=167, cin=64, cout=512), 1, 1),
    ('f16', 'pooled', (8, 4, 6, 2), 'pool', dict(B=2, H=113, W=100, cin=64, cout=512), 1, 1),
    ('f16', 'pooled', (8, 4, 7, 2), 'pool', dict(B=1, H=170, W=334, cin=64, cout=256), 1, 1),
    ('f16', 'pooled', (8, 4, 8, 2), 'pool', dict(B=1, H=150, W=201, cin=64, cout=512), 1, 1),
    ('f16', 'rpn', (8, 4, 4, 2), 'rpn', dict(B=1, A=3, shapes=((7, 9),), cin=64, cout=256), 1, 1),
    ('f16', 'rpn', (8, 4, 5, 2), 'rpn', dict(B=1, A=3, shapes=((100, 334),), cin=64, cout=256), 1, 1),
    ('f16', 'rpn', (8, 4, 6, 2), 'rpn', dict(B=1, A=3, shapes=((191, 250),), cin=64, cout=256), 1, 1),
    ('f16', 'rpn', (8, 4, 7, 2), 'rpn', dict(B=1, A=3, shapes=((170, 334),), cin=64, cout=256), 1, 1),
    ('f16', 'rpn', (8, 4, 8, 2), 'rpn', dict(B=1, A=3, shapes=((191, 334),), cin=64, cout=256), 1, 1),
    ('f16', 'tail', (8, 1, 1, 2), 'tail', dict(B=1, H=7, W=9, cin=64, cout=64, n3=128), 1, 1),
    ('f16', 'tail', (8, 1, 2, 2), 'tail', dict(B=1, H=100, W=334, cin=64, cout=64, n3=128), 1, 1),
    ('f16', 'tail', (8, 2, 2, 2), 'tail', dict(B=1, H=7, W=9, cin=64, cout=128, n3=128), 1, 1),
    ('f16', 'tail', (8, 2, 3, 2), 'tail', dict(B=1, H=100, W=334, cin=64, cout=128, n3=128), 1, 1),
    ('f16', 'tail', (8, 2, 4, 2), 'tail', dict(B=1, H=170, W=334, cin=64, cout=128, n3=128), 1, 1),
    ('f16', 'tail', (8, 4, 4, 2), 'tail', dict(B=1, H=7, W=9, cin=64, cout=256, n3=128), 1, 1),
    ('f16', 'tail', (8, 4, 5, 2), 'tail', dict(B=1, H=100, W=334, cin=64, cout=256, n3=128), 1, 1),
    ('f16', 'tail', (8, 4, 6, 2), 'tail', dict(B=1, H=191, W=250, cin=64, cout=256, n3=128), 1, 1),
    ('f16', 'tail', (8, 4, 7, 2), 'tail', dict(B=1, H=170, W=334, cin=64, cout=256, n3=128), 1, 1),
    ('f16', 'tail', (8, 4, 8, 2), 'tail', dict(B=2, H=150, W=201, cin=64, cout=256, n3=128), 1, 1),
    ('f32', 'plain', (8, 1, 2, 3), 'conv3x3', dict(B=1, H=7, W=9, cin=32, cout=64), 1, 1),
    ('f32', 'plain', (8, 2, 2, 3), 'conv3x3', dict(B=1, H=7, W=9, cin=32, cout=128), 1, 1),
    ('f32', 'plain', (8, 2, 3, 3), 'conv3x3', dict(B=1, H=100, W=167, cin=32, cout=256), 1, 1),
    ('f32', 'plain', (8, 2, 4, 3), 'conv3x3', dict(B=1, H=170, W=334, cin=32, cout=128), 1, 1),
    ('f32', 'plain', (8, 4, 4, 3), 'conv3x3', dict(B=2, H=75, W=100, cin=32, cout=512), 1, 1),
    ('f32', 'plain', (8, 4, 5, 2), 'conv3x3', dict(B=1, H=100, W=167, cin=32, cout=512), 1, 1),
    ('f32', 'plain', (8, 4, 6, 2), 'conv3x3', dict(B=2, H=113, W=100, cin=32, cout=512), 1, 1),
    ('f32', 'plain', (8, 4, 7, 2), 'conv3x3', dict(B=1, H=170, W=334, cin=32, cout=256), 1, 1),
    ('f32', 'plain', (8, 4, 8, 2), 'conv3x3', dict(B=1, H=150, W=201, cin=32, cout=512), 1, 1),
    ('f32', 'pointwise', (8, 1, 2, 3), 'pointwise', dict(B=1, H=7, W=9, cin=64, cout=64), 1, 1),
    ('f32', 'pointwise', (8, 2, 2, 3), 'pointwise', dict(B=1, H=7, W=9, cin=64, cout=128), 1, 1),
    ('f32', 'pointwise', (8, 2, 3, 3), 'pointwise', dict(B=1, H=100, W=167, cin=64, cout=256), 1, 1),
    ('f32', 'pointwise', (8, 2, 4, 3), 'pointwise', dict(B=1, H=170, W=334, cin=64, cout=128), 1, 1),
    ('f32', 'pointwise', (8, 4, 4, 3), 'pointwise', dict(B=2, H=75, W=100, cin=64, cout=512), 1, 1),
    ('f32', 'pointwise', (8, 4, 5, 2), 'pointwise', dict(B=1, H=100, W=167, cin=64, cout=512), 1, 1),
    ('f32', 'pointwise', (8, 4, 6, 2), 'pointwise', dict(B=2, H=113, W=100, cin=64, cout=512), 1, 1),
    ('f32', 'pointwise', (8, 4, 7, 2), 'pointwise', dict(B=1, H=170, W=334, cin=64, cout=256), 1, 1),
    ('f32', 'pointwise', (8, 4, 8, 2), 'pointwise', dict(B=1, H=150, W=201, cin=64, cout=512), 1, 1),
    ('split', 'plain', (8, 1, 1, 3), 'conv3x3', dict(B=1, H=7, W=9, cin=32, cout=64), 2, 1),
    ('split', 'plain', (8, 2, 2, 3), 'conv3x3', dict(B=1, H=100, W=167, cin=32, cout=128), 2, 1),
    ('split', 'plain', (8, 4, 4, 3), 'conv3x3', dict(B=1, H=100, W=167, cin=32, cout=256), 2, 1),
    ('split', 'pointwise', (8, 1, 1, 3), 'pointwise', dict(B=1, H=7, W=9, cin=64, cout=64), 2, 1),
    ('split', 'pointwise', (8, 2, 2, 3), 'pointwise', dict(B=1, H=100, W=167, cin=64, cout=128), 2, 1),
    ('split', 'pointwise', (8, 4, 4, 3), 'pointwise', dict(B=1, H=100, W=167, cin=64, cout=256), 2, 1),
    ('split', 'plain', (8, 1, 1, 2), 'conv3x3', dict(B=1, H=7, W=9, cin=32, cout=64), 3, 1),
    ('split', 'plain', (8, 1, 2, 2), 'conv3x3', dict(B=1, H=200, W=334, cin=256, cout=64), 3, 2),
    ('split', 'plain', (8, 2, 2, 2), 'conv3x3', dict(B=1, H=100, W=167, cin=32, cout=128), 3, 1),
    ('split', 'plain', (8, 2, 4, 2), 'conv3x3', dict(B=1, H=100, W=334, cin=32, cout=128), 3, 1),
    ('split', 'plain', (8, 4, 4, 2), 'conv3x3', dict(B=1, H=100, W=167, cin=32, cout=256), 3, 1),
    ('split', 'pointwise', (8, 1, 1, 2), 'pointwise', dict(B=1, H=7, W=9, cin=64, cout=64), 3, 1),
    ('split', 'pointwise', (8, 2, 2, 2), 'pointwise', dict(B=1, H=100, W=167, cin=64, cout=128), 3, 1),
    ('split', 'pointwise', (8, 2, 4, 2), 'pointwise', dict(B=1, H=100, W=334, cin=64, cout=128), 3, 1),
    ('split', 'pointwise', (8, 4, 4, 2), 'pointwise', dict(B=1, H=100, W=167, cin=64, cout=256), 3, 1),
]


def all_cases():
    return _forced_f16() + _forced_f32() + _forced_split() + _natural()


CASES = all_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ---- the product's own launches: the three model families' dense layers ------------------------------------------------------------
# A restatement of the routing rules of model/layers.py and of the detectors' own layers (which 1x1 convolutions go to the
# pointwise GEMM, from how many slabs on a bottleneck runs as the fused tail, what the float32 mode replaces) as a list of
# (form, entry point, shape) per model, batch and precision -- only the launches of the three convolution files; the stem, the
# RGB convolution and the register-resident 1x1 kernel are other kernels.  tests/test_conv_tiles_host.py runs the list through
# the launchers in plan-only mode; DESIGN.md lists what it reaches.
MODEL_IMAGES = {'resnet101fpn': (800, 1333), 'resnet50c4': (800, 1333), 'vgg16': (600, 800)}       # the BASELINE configs' sizes
MODEL_PROPOSALS = {'resnet101fpn': 1000, 'resnet50c4': 300, 'vgg16': 300}
FUSED_TAIL_MIN_SLABS = 200                # model/layers.py _FUSED_TAIL_MIN_SLABS


def _half(hw):
    return ((hw[0] + 1) // 2, (hw[1] + 1) // 2)


def _resnet_stage(out, B, hw, cin, f, blocks, stride, f16):
    """one stage of bottlenecks on the input map `hw`; returns its output map"""
    o = _half(hw) if stride == 2 else hw
    pw16 = lambda k: k % 64 == 0 and k >= 128                          # (_pw_ok, float16)
    mfma = lambda k, n, s: f16 and s == 1 and k in (64, 128, 256, 512) and (n <= 64 or not pw16(k))       # (_route_1x1 -> 'mfma')

    def one_by_one(k, n, on, s=1):
        if not mfma(k, n, s):
            out.append(('pointwise', 'pointwise', dict(B=B, H=on[0], W=on[1], cin=k, cout=n, stride=s)))
    one_by_one(cin, f, hw, stride)                                                              # block 1: c1 (strided)
    out.append(('plain', 'conv3x3', dict(B=B, H=o[0], W=o[1], cin=f, cout=f)))                  # c2
    out.append(('pointwise', 'pointwise', dict(B=B, H=o[0], W=o[1], cin=f + cin, cout=4 * f)))  # c3 + shortcut: one contraction
    for _ in range(blocks - 1):
        one_by_one(4 * f, f, o)
        if f16 and f in (64, 128, 256) and (B * o[0] * o[1] + 127) // 128 >= FUSED_TAIL_MIN_SLABS:
            out.append(('tail', 'tail', dict(B=B, H=o[0], W=o[1], cin=f, cout=f, n3=4 * f)))
        else:
            out.append(('plain', 'conv3x3', dict(B=B, H=o[0], W=o[1], cin=f, cout=f)))
            one_by_one(f, 4 * f, o)
    return o


def model_launches(model, B, f16):
    """[(form, op, args)] of one forward pass of `model` at batch B, float16 (True) or one of the float32 forms (False)"""
    out = []
    H, W = MODEL_IMAGES[model]
    R = MODEL_PROPOSALS[model]
    dense = lambda rows, k, n: out.append(('pointwise', 'pointwise', dict(B=1, H=1, W=rows, cin=k, cout=n)))
    if model == 'vgg16':
        hw, cin = (H, W), 64
        if not f16:                                                    # conv1_1 as the GEMM on its patch matrix
            out.append(('pointwise', 'pointwise', dict(B=B, H=H, W=W, cin=64, cout=64)))
        for stage, (cout, n) in enumerate(((64, 1), (128, 2), (256, 3), (512, 3), (512, 3))):   # (conv1_1 is the RGB kernel's)
            for i in range(n):
                pooled = stage < 4 and i == n - 1
                out.append(('pooled', 'pool', dict(B=B, H=hw[0], W=hw[1], cin=cin, cout=cout)) if pooled and f16 else
                           ('plain', 'conv3x3', dict(B=B, H=hw[0], W=hw[1], cin=cin, cout=cout)))
                cin = cout
                if pooled:
                    hw = _half(hw)
        out.append(('plain', 'conv3x3', dict(B=B, H=hw[0], W=hw[1], cin=512, cout=512)))        # RpnHead's 3x3
        out.append(('pointwise', 'pointwise', dict(B=B, H=hw[0], W=hw[1], cin=512, cout=64)))   # both 1x1, rows padded to 64
        for rows in sorted({R, B * R}):
            dense(rows, 7 * 7 * 512, 4096), dense(rows, 4096, 4096), dense(rows, 4096, 128)
        return out
    hw = _half(_half((H, W)))                                          # the stem: 7x7 / 2, 3x3 / 2 pooling
    if not f16:
        s = _half((H, W))
        out.append(('pointwise', 'pointwise', dict(B=B, H=s[0], W=s[1], cin=160, cout=64)))     # the stem's patch-matrix GEMM
    depth4 = 23 if model == 'resnet101fpn' else 6
    c2 = _resnet_stage(out, B, hw, 64, 64, 3, 1, f16)
    c3 = _resnet_stage(out, B, c2, 256, 128, 4, 2, f16)
    c4 = _resnet_stage(out, B, c3, 512, 256, depth4, 2, f16)
    if model == 'resnet50c4':
        out.append(('plain', 'conv3x3', dict(B=B, H=c4[0], W=c4[1], cin=1024, cout=512)))
        out.append(('pointwise', 'pointwise', dict(B=B, H=c4[0], W=c4[1], cin=512, cout=64)))
        for rows in sorted({R, B * R}):                                # conv5 on the 7 x 7 crops, then the score / box layer
            _resnet_stage(out, rows, (7, 7), 1024, 512, 3, 1, f16)
            dense(rows, 2048, 128)
        return out
    c5 = _resnet_stage(out, B, c4, 1024, 512, 3, 2, f16)
    out.append(('pointwise', 'pointwise', dict(B=B, H=c5[0], W=c5[1], cin=2048, cout=256)))     # P5
    for cm, k in ((c4, 1024), (c3, 512), (c2, 256)):
        out.append(('pointwise', 'pointwise', dict(B=B, H=cm[0], W=cm[1], cin=k, cout=256)))    # lateral + top-down merge
        out.append(('plain', 'conv3x3', dict(B=B, H=cm[0], W=cm[1], cin=256, cout=256)))        # smoothing
    levels = (c2, c3, c4, c5, _half(c5))
    if f16:
        out.append(('rpn', 'rpn', dict(B=B, A=3, shapes=levels, cin=256, cout=512)))
    else:
        out.append(('plain', 'conv3x3_levels', dict(B=B, shapes=levels, cin=256, cout=512)))
        for lv in levels:
            out.append(('pointwise', 'pointwise', dict(B=B, H=lv[0], W=lv[1], cin=512, cout=64)))
    for rows in sorted({R, B * R}):
        dense(rows, 7 * 7 * 256, 1024), dense(rows, 1024, 1024), dense(rows, 1024, 128)
    return out


PRECISIONS = {'float16': ('f16', 1), 'float32 exact': ('f32', 1), 'float32 x3': ('split', 3), 'float32 x2': ('split', 2)}


def model_sweep(lib, batches=(1, 2, 4, 8)):
    """{(family, limbs, form, tile): [(model, batch, precision)]} over the three models, `batches` and the four precisions, from
    the launchers' recorded plans in plan-only mode (no override)"""
    reached, seen = {}, {}
    for model in MODEL_IMAGES:
        for B in batches:
            for prec, (family, limbs) in PRECISIONS.items():
                for form, op, args in model_launches(model, B, family == 'f16'):
                    key = (family, limbs, form, op, repr(sorted(args.items())))
                    if key not in seen:
                        tc = TileCase(family, form, (0, 0, 0, 0), op, args, mode='natural', limbs=limbs)
                        p = tc.plan(lib)
                        assert p['form'] == form and not p['forced'], (key, p)
                        seen[key] = (family, limbs, 'plain' if form == 'pooled' else form, p['tile'])
                    reached.setdefault(seen[key], []).append((model, B, prec))
    return reached
