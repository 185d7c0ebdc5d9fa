"""The RoI pooling case table (csrc/roi.hip: k_roi_pool) and a host restatement of the kernel's data-dependent path choice.

Every case names what it is for.  tests/test_roi_paths_host.py proves on the CPU that the table reaches every row path, bin
class, instantiation, coordinate edge and launch form it claims; tests/test_roi_paths_gpu.py runs every case inside the
diagnostic library, asserts the recorded launch plan and compares bits.

 * classify(case): numpy float32 mirror of make_axis / make_tap<PAD> / share_class and the carry rule of roi_row_carry_pass
   (`last`, reset after a DX == 2 bin), written from the kernel header's description: per (RoI, output row) the row path, per bin
   DX and M.  Test infrastructure only.
 * reference(case): the reference's own order -- oracle_np.tf_crop_and_resize then tf_max_pool_2x2 / tf_avg_pool_2x2 / nothing,
   the four normalisations as oracle_np has them.  The combinations oracle_np has no function for are compositions of its
   functions (NORM_IMAGE without the max-pooling needs the box division of roi_pooling.py:30-35, one IEEE division per
   coordinate, restated in _image_boxes).
 * exact(case): float64, (1 - wy)((1 - wx) a + wx b) + wy (...) on the taps of classify's mirror, pooled in float64, rounded
   once.  On the dyadic cases (data 'ints' / 'subnormal' / 'max') it is the true value and the host test proves the float32
   reference-order result equal to it.

Geometry is given in CELLS: a sample axis is (a, extent) -- first sample at cell coordinate a, the crop's samples spread over
`extent` cells -- and roi_for() turns it into the image-pixel box each normalisation maps back onto those samples."""
import functools
import zlib

import numpy as np

from oracle import oracle_np as onp

F32 = np.float32
POOL_NONE, POOL_MAX2, POOL_AVG2 = 0, 1, 2
NORM_STRIDE, NORM_IMAGE, NORM_TP, NORM_NOPAD = 0, 1, 2, 3
POOLS = {POOL_NONE: 'none', POOL_MAX2: 'max2', POOL_AVG2: 'avg2'}
NORMS = {NORM_STRIDE: 'stride', NORM_IMAGE: 'image', NORM_TP: 'tp', NORM_NOPAD: 'nopad'}
ROW_PATHS = ('single', 'guarded', 'dy0', 'dy1', 'dy2', 'padded')      # everything classify() can return for a row
ROW_FORMS = ('carry', 'full', 'partial')                              # roi_row_carry / roi_row<FULL> / roi_row<!FULL>


# ---- the launch plan, restated (csrc/roi.hip: roi_plan) -------------------------------------------------------------------------

def plan_of(B, C, n, P):
    waves = P if P <= 16 else 8
    slices = C // 256 if (waves == P and C % 256 == 0 and C > 256) else 1
    nblocks = n * slices if slices > 1 else (n * P + waves - 1) // waves
    xcd_images = 1 if B in (2, 4, 8) else 0
    xcds = 8 // B if xcd_images else 8
    bpx, rpx, groups = (nblocks + xcds - 1) // xcds, 0, 0
    if slices > 1:
        if xcds % slices == 0:
            groups = xcds // slices
            rpx = (n + groups - 1) // groups
            bpx = rpx
        else:
            rpx = (n + xcds - 1) // xcds
            bpx = rpx * slices
        nblocks = bpx * xcds
    return dict(waves=waves, slices=slices, roi_groups=groups, rois_per_xcd=rpx, blocks_per_xcd=bpx, nblocks=nblocks,
                xcd_images=xcd_images, xcds_per_img=xcds, grid_x=bpx * 8, grid_y=1 if xcd_images else B, threads=waves * 64)


def walk_plan(p, B, n, P):
    """the kernel's workgroup -> (image, RoI, slice, row) map of a plan, walked on the host: {(img, ri, slice, py): times}, and
    the number of waves that address a RoI >= n without leaving (must be 0)"""
    seen, escaped = {}, 0
    for by in range(p['grid_y']):
        for bx in range(p['grid_x']):
            xcd, slot = bx & 7, bx >> 3
            img = xcd // p['xcds_per_img'] if p['xcd_images'] else by
            sub = xcd - img * p['xcds_per_img'] if p['xcd_images'] else xcd
            lb = sub * p['blocks_per_xcd'] + slot
            if slot >= p['blocks_per_xcd'] or lb >= p['nblocks']:
                continue
            for w in range(p['waves']):
                sl = 0
                if p['slices'] > 1:
                    if p['roi_groups'] > 0:
                        sl = sub % p['slices']
                        ri = (sub // p['slices']) * p['rois_per_xcd'] + slot
                        if slot >= p['rois_per_xcd']:
                            continue
                    else:
                        sl = slot // p['rois_per_xcd']
                        ri = sub * p['rois_per_xcd'] + (slot - sl * p['rois_per_xcd'])
                    py = w
                elif p['waves'] == P:
                    ri, py = lb, w
                else:
                    u = lb * p['waves'] + w
                    ri, py = u // P, u % P
                if ri >= n:
                    continue
                if not (0 <= img < B and 0 <= sl < p['slices'] and 0 <= py < P):
                    escaped += 1
                    continue
                seen[(img, ri, sl, py)] = seen.get((img, ri, sl, py), 0) + 1
    return seen, escaped


# ---- cases ------------------------------------------------------------------------------------------------------------------------

class Image:
    """one image of a case: its RoIs (image pixels, x1 y1 x2 y2), their levels, the device count and the processing order"""

    def __init__(self, rois, level=None, count=None):
        self.rois = np.ascontiguousarray(rois, np.float32).reshape(-1, 4)
        self.level = None if level is None else np.asarray(level, np.int32)
        self.count = count


class RoiCase:
    def __init__(self, name, purpose, f16, pool, norm, C, P, images, maps_hw=((17, 17),), stride=16.0, image_shape=(0, 0),
                 data='normal', order=None, via='ops', group='a', want_plan=None, zero=False, aim=()):
        self.name, self.purpose, self.f16, self.pool, self.norm, self.C, self.P = name, purpose, bool(f16), pool, norm, C, P
        self.images, self.maps_hw, self.stride, self.image_shape = images, tuple(maps_hw), float(stride), tuple(image_shape)
        self.data, self.order, self.via, self.group, self.zero, self.aim = data, order, via, group, zero, tuple(aim)
        self.B, self.n = len(images), images[0].rois.shape[0]
        assert all(im.rois.shape[0] == self.n for im in images) and self.n <= 32
        assert all(h <= 33 and w <= 33 for h, w in self.maps_hw) and C in (8, 64, 256, 260, 512, 768, 1024, 2048)
        self.plan_literal = dict(want_plan or {})
        self.dyadic = data in ('ints', 'subnormal', 'max')

    S = property(lambda self: 1 if self.pool == POOL_NONE else 2)
    crop = property(lambda self: self.P * self.S)
    instantiation = property(lambda self: (self.pool, self.norm, self.f16))
    row_form = property(lambda self: ('carry' if not self.f16 else 'full') if self.C % 256 == 0 else 'partial')

    def want_plan(self):
        p = plan_of(self.B, self.C, self.n, self.P)
        p.update(B=self.B, C=self.C, n=self.n, P=self.P, f16=int(self.f16), pool_mode=self.pool, norm_mode=self.norm)
        for k, v in self.plan_literal.items():
            assert p[k] == v, (self.name, k, p[k], v)                  # the table's literal and the restated rule agree
        return p

    def form(self):
        p = self.want_plan()
        return 'B%d C%d P%d n%d: waves %d slices %d groups %d xcds/img %d%s grid %dx%d' % (
            self.B, self.C, self.P, self.n, p['waves'], p['slices'], p['roi_groups'], p['xcds_per_img'],
            '' if p['xcd_images'] else ' (image from blockIdx.y)', p['grid_x'], p['grid_y'])

    @functools.lru_cache(maxsize=None)
    def maps(self):
        """[image][level] -> [H, W, C] arrays in the maps' element type; every image has its own"""
        rng = np.random.default_rng(zlib.crc32(self.name.encode()))
        out = []
        for _ in range(self.B):
            lv = []
            for h, w in self.maps_hw:
                shape = (h, w, self.C)
                if self.data == 'normal':
                    m = rng.standard_normal(shape).astype(np.float32)
                elif self.data == 'ints':            # float16: even integers in [2048, 4096) (one ulp = 2); float32: integers < 2^12
                    m = (2048 + 2 * rng.integers(0, 1024, shape)) if self.f16 else rng.integers(0, 4096, shape)
                    m = m.astype(np.float32)
                elif self.data == 'subnormal':       # the same, scaled into float16's subnormal range: k * 2^-24, k < 1024
                    m = (rng.integers(1, 1024, shape).astype(np.float64) * 2.0 ** -24).astype(np.float32)
                else:                                # 'max': +-65504, the sign per cell and channel
                    m = (rng.integers(0, 2, shape) * 2 - 1).astype(np.float32) * F32(65504)
                m = m.astype(np.float16) if self.f16 else m
                m.setflags(write=False)
                lv.append(m)
            out.append(lv)
        return out

    def orders(self):
        """[image] -> int32 processing order for 'identity' / 'reversed' (ops.roi_order's is computed on the GPU), else None"""
        if self.order == 'identity':
            return [np.arange(self.n, dtype=np.int32)] * self.B
        if self.order == 'reversed':
            return [np.arange(self.n, dtype=np.int32)[::-1].copy()] * self.B
        return [None] * self.B


def roi_for(norm, ax, ex, ay, ey, crop, px=16.0):
    """the box whose crop samples start at cell (ay, ax) and spread over (ey, ex) cells; px = image pixels per cell"""
    def axis(a, e):
        if norm in (NORM_TP, NORM_NOPAD):        # tensorpack: samples at x0 + sw / 2 - 0.5 + i * sw, sw = (x1 - x0) / crop
            d = e / max(crop - 1, 1)
            lo = a - d / 2 + 0.5
            return lo, lo + crop * d
        return a, a + e
    x0, x1 = axis(ax, ex)
    y0, y1 = axis(ay, ey)
    return [x0 * px, y0 * px, x1 * px, y1 * px]


# ---- classify: the kernel's path choice, restated in numpy float32 --------------------------------------------------------------

def _axis_taps(lo_n, hi_n, dim_s, crop, pad, dim, inside='le'):
    """make_axis + make_tap<PAD> for every sample of one axis: (in, ok, lo, hi, lerp) arrays.  `inside`: 'le' is the kernel's and
    TF's test; 'lt' (in == dim - 1 outside) and 'ulp' (one ulp beyond either end inside) are the WRONG contracts the host test
    measures the cases against."""
    with np.errstate(all='ignore'):
        limit = F32(dim_s - 1)
        if crop > 1:
            scale = F32(F32(F32(hi_n - lo_n) * limit) / F32(crop - 1))
            start = F32(lo_n * limit)
            inn = (start + (np.arange(crop, dtype=np.float32) * scale).astype(np.float32)).astype(np.float32)
        else:
            inn = np.array([F32(F32(F32(0.5) * F32(lo_n + hi_n)) * limit)], np.float32)
        if inside == 'le':
            ok = (inn >= 0) & (inn <= limit)
        elif inside == 'lt':
            ok = (inn >= 0) & (inn < limit)
        else:
            ok = (inn >= np.nextafter(F32(0), F32(-1))) & (inn <= np.nextafter(limit, F32(np.inf)))
        safe = np.where(ok, inn, F32(0))
        f = np.floor(safe)
        lerp = (safe - f).astype(np.float32)
        lo, hi = f.astype(np.int64), np.ceil(safe).astype(np.int64)
        if pad:
            lo, hi = np.clip(lo - 1, 0, dim - 1), np.clip(hi - 1, 0, dim - 1)
        lo, hi = np.clip(lo, 0, dim - 1), np.clip(hi, 0, dim - 1)      # (only the wrong contracts ever need this clamp)
        lo, hi = np.where(ok, lo, 0), np.where(ok, hi, 0)
        if inside == 'ulp':
            lerp = np.where(inn < 0, F32(0), lerp)
    return inn, ok, lo, hi, lerp


def _norm_box(case, roi, H, W):
    """the normalised box (y1n, x1n, y2n, x2n) and the sampled map's dims, operation by operation as the kernel forms them"""
    x, y, z, w = (F32(v) for v in roi)
    with np.errstate(all='ignore'):
        if case.norm == NORM_IMAGE:
            ih, iw = F32(case.image_shape[0]), F32(case.image_shape[1])
            return F32(y / ih), F32(x / iw), F32(w / ih), F32(z / iw), H, W
        st = F32(case.stride)
        if case.norm == NORM_STRIDE:
            hm, wm = F32(H - 1), F32(W - 1)
            return F32(F32(y / st) / hm), F32(F32(x / st) / wm), F32(F32(w / st) / hm), F32(F32(z / st) / wm), H, W
        pad = case.norm == NORM_TP
        Hs, Ws = (H + 2, W + 2) if pad else (H, W)
        x0, y0, x1, y1 = F32(x / st), F32(y / st), F32(z / st), F32(w / st)
        if pad:
            x0, y0, x1, y1 = F32(x0 + F32(1)), F32(y0 + F32(1)), F32(x1 + F32(1)), F32(y1 + F32(1))
        cs = F32(case.crop)
        sw, sh = F32(F32(x1 - x0) / cs), F32(F32(y1 - y0) / cs)
        imh, imw = F32(Hs - 1), F32(Ws - 1)
        x1n = F32(F32(F32(x0 + F32(sw / F32(2))) - F32(0.5)) / imw)
        y1n = F32(F32(F32(y0 + F32(sh / F32(2))) - F32(0.5)) / imh)
        nw = F32(F32(sw * F32(case.crop - 1)) / imw)
        nh = F32(F32(sh * F32(case.crop - 1)) / imh)
        return y1n, x1n, F32(y1n + nh), F32(x1n + nw), Hs, Ws


def roi_taps(case, img, r, inside='le'):
    """(level, y taps, x taps) of RoI r of image img"""
    im = case.images[img]
    lvl = 0 if im.level is None else int(min(max(int(im.level[r]), 0), len(case.maps_hw) - 1))
    H, W = case.maps_hw[lvl]
    y1n, x1n, y2n, x2n, Hs, Ws = _norm_box(case, im.rois[r], H, W)
    pad = case.norm == NORM_TP
    return lvl, _axis_taps(y1n, y2n, Hs, case.crop, pad, H, inside), _axis_taps(x1n, x2n, Ws, case.crop, pad, W, inside)


def _share(lo0, hi0, lo1, hi1):
    d = lo1 - lo0
    return int(d) if (hi0 == lo0 + 1 and hi1 == lo1 + 1 and d in (0, 1)) else 2


def count_of(case, img):
    c = case.images[img].count
    return case.n if c is None else min(int(c), case.n)


@functools.lru_cache(maxsize=None)
def classify(case):
    """[{img, r, py, path, form, yok, bins}]: path in ROW_PATHS; bins = [(DX, M)] for the all-inside paths (M as the carry rule
    gives it, whatever the row function), [xok] for 'guarded' and 'single'"""
    out = []
    S, P, pad = case.S, case.P, case.norm == NORM_TP
    for img in range(case.B):
        cnt = count_of(case, img)
        for r in range(case.n):
            if r >= cnt:
                out.extend(dict(img=img, r=r, py=py, path='padded', form=None, yok=0, bins=[]) for py in range(P))
                continue
            _, ty, tx = roi_taps(case, img, r)
            xok = [int(tx[1][px * S]) | (int(tx[1][px * S + S - 1]) << 1) for px in range(P)]
            for py in range(P):
                s0, s1 = py * S, py * S + S - 1
                yok = int(ty[1][s0]) | (int(ty[1][s1]) << 1)
                rec = dict(img=img, r=r, py=py, form=None, yok=yok)
                if S == 1:
                    rec.update(path='single', bins=[x & 1 for x in xok])
                elif yok != 3 or any(x != 3 for x in xok) or any(tx[2][px * S + 1] < tx[2][px * S] for px in range(P)):
                    # (the last clause: a bin of a reversed box whose second sample column lies left of its first)
                    rec.update(path='guarded', bins=list(xok), reversed_x=all(x == 3 for x in xok) and yok == 3)
                else:
                    dy = 2 if pad else _share(ty[2][s0], ty[3][s0], ty[2][s1], ty[3][s1])
                    bins, last = [], None
                    for px in range(P):
                        a, b = px * S, px * S + 1
                        dx = 2 if pad else _share(tx[2][a], tx[3][a], tx[2][b], tx[3][b])
                        c0 = int(tx[2][a])
                        if dx == 2:
                            m, last = 0, None
                        else:
                            m = 0 if last is None else (1 if c0 == last else (2 if c0 + 1 == last else 0))
                            last = c0 + 1 + dx
                        bins.append((dx, m))
                    rec.update(path='dy%d' % dy, form=case.row_form, bins=bins)
                out.append(rec)
    return out


def histogram(case):
    h = {}
    for rec in classify(case):
        h[rec['path']] = h.get(rec['path'], 0) + 1
    return h


def carry_events(case):
    """{(DY, DX, M, why)} over the all-inside rows of a case: why tells the M = 0 / M = 2 flavours apart -- 'first' bin, 'after2'
    (right after a DX == 2 bin), 'gap' (a column gap), and for M = 2 'two' / 'three' (columns of the previous bin)"""
    ev = set()
    for rec in classify(case):
        if not rec['path'].startswith('dy'):
            continue
        dy = int(rec['path'][2])
        for px, (dx, m) in enumerate(rec['bins']):
            prev = rec['bins'][px - 1][0] if px else None
            if dx == 2:
                why = ''
            elif m == 0:
                why = 'first' if px == 0 else ('after2' if prev == 2 else 'gap')
            elif m == 2:
                why = 'two' if prev == 0 else 'three'
            else:
                why = ''
            ev.add((dy, dx, m, why))
    return ev


# ---- references -------------------------------------------------------------------------------------------------------------------

def _image_boxes(rois, image_shape):
    """roi_pooling.py:30-35 (as oracle_np.roi_pooling_crop_and_resize2 has it): the boxes divided by the image size"""
    rois = onp.f32(rois).reshape(-1, 4)
    h, w = F32(image_shape[0]), F32(image_shape[1])
    return np.stack([rois[:, 1] / h, rois[:, 0] / w, rois[:, 3] / h, rois[:, 2] / w], axis=1)


def _pooled(case, crops):
    if case.pool == POOL_MAX2:
        return onp.tf_max_pool_2x2(crops)
    if case.pool == POOL_AVG2:
        return onp.tf_avg_pool_2x2(crops)
    return crops


def _ref_level(case, feat, rois):
    feat = feat.astype(np.float32)[None]
    P, crop = case.P, case.crop
    ind = np.zeros(rois.shape[0], np.int32)
    if case.norm == NORM_STRIDE:
        if case.pool == POOL_AVG2:
            return onp.tf_avg_pool_2x2(onp.roi_pooling_crop_and_resize(feat, rois, case.stride, crop, False))
        return onp.roi_pooling_crop_and_resize(feat, rois, case.stride, P, case.pool == POOL_MAX2)
    if case.norm == NORM_IMAGE:
        if case.pool == POOL_MAX2:
            return onp.roi_pooling_crop_and_resize2(feat, rois, case.image_shape, P)
        return _pooled(case, onp.tf_crop_and_resize(feat, _image_boxes(rois, case.image_shape), ind, [crop, crop]))
    boxes = onp.f32(rois).reshape(-1, 4) / F32(case.stride)            # roi_pooling.py:175 (oracle_np.roi_pooling_roi_align)
    if case.norm == NORM_TP and case.pool == POOL_AVG2:
        return onp.roi_align(feat, boxes, P)
    return _pooled(case, onp.crop_and_resize_tp(feat, boxes, ind, crop, pad_border=case.norm == NORM_TP))


def _by_level(case, img):
    im = case.images[img]
    cnt = max(count_of(case, img), 0)
    nl = len(case.maps_hw)
    lvl = np.zeros(case.n, np.int64) if im.level is None else np.clip(im.level.astype(np.int64), 0, nl - 1)
    for l in range(nl):
        idx = np.nonzero((lvl == l) & (np.arange(case.n) < cnt))[0]
        if idx.size:
            yield l, idx


@functools.lru_cache(maxsize=None)
def reference(case):
    """[image] -> float32 [n, P, P, C] in the reference's own order; rows at or beyond the count are zero.  RoI levels outside
    the range are clamped first (declared behaviour of the kernel: the reference has no such input)."""
    assert not case.zero
    out = []
    with np.errstate(all='ignore'):
        for img in range(case.B):
            o = np.zeros((case.n, case.P, case.P, case.C), np.float32)
            for l, idx in _by_level(case, img):
                o[idx] = _ref_level(case, case.maps()[img][l], case.images[img].rois[idx])
            o.setflags(write=False)
            out.append(o)
    return out


def c_reference(case):
    """the same from the C oracle where it has the function, else None"""
    from oracle import c_oracle as co
    key = (case.norm, case.pool)
    if key not in ((NORM_STRIDE, POOL_MAX2), (NORM_STRIDE, POOL_NONE), (NORM_IMAGE, POOL_MAX2), (NORM_TP, POOL_AVG2)) or case.zero:
        return None
    out = []
    for img in range(case.B):
        o = np.zeros((case.n, case.P, case.P, case.C), np.float32)
        for l, idx in _by_level(case, img):
            feat = np.ascontiguousarray(case.maps()[img][l].astype(np.float32))
            rois = np.ascontiguousarray(case.images[img].rois[idx])
            if case.norm == NORM_TP:
                o[idx] = co.roi_align(feat, rois, case.stride, pool=case.P)
            elif case.norm == NORM_IMAGE:
                o[idx] = co.roi_pool(feat, rois, image_shape=case.image_shape, pool=case.P)
            else:
                o[idx] = co.roi_pool(feat, rois, stride=case.stride, pool=case.P, max_pool=case.pool == POOL_MAX2)
        out.append(o)
    return out


def exact(case, inside='le', sample16=False):
    """[image] -> float64 [n, P, P, C]: bilinear weights (1 - wy)((1 - wx) a + wx b) + wy (...) on the taps of the float32
    mirror, pooled in float64; NOT yet rounded.  inside / sample16: the wrong contracts (see _axis_taps; sample16 rounds every
    sample to float16 before the pooling)."""
    P, S = case.P, case.S
    out = []
    for img in range(case.B):
        o = np.zeros((case.n, P, P, case.C), np.float64)
        for r in range(max(count_of(case, img), 0)):
            lvl, ty, tx = roi_taps(case, img, r, inside)
            m = case.maps()[img][lvl].astype(np.float64)
            wy, wx = ty[4].astype(np.float64)[:, None, None], tx[4].astype(np.float64)[None, :, None]
            tl, tr = m[ty[2]][:, tx[2]], m[ty[2]][:, tx[3]]
            bl, br = m[ty[3]][:, tx[2]], m[ty[3]][:, tx[3]]
            v = (1 - wy) * ((1 - wx) * tl + wx * tr) + wy * ((1 - wx) * bl + wx * br)
            v = v * (ty[1][:, None, None] & tx[1][None, :, None])
            if sample16:
                v = v.astype(np.float16).astype(np.float64)
            if S == 2:
                v = v.reshape(P, 2, P, 2, case.C)
                v = v.max(axis=(1, 3)) if case.pool == POOL_MAX2 else v.sum(axis=(1, 3)) / 4.0
            o[r] = v
        out.append(o)
    return out


def round_f16(x, mode='rne'):
    """float64 -> float16: 'rne' (the contract), 'trunc' and 'away' (ties away from zero) the wrong ones"""
    x = np.asarray(x, np.float64)
    rn = x.astype(np.float16)
    if mode == 'rne':
        return rn
    r = rn.astype(np.float64)
    toward = np.where(np.abs(r) > np.abs(x), np.nextafter(rn, np.float16(0)), rn)
    if mode == 'trunc':
        return toward
    t = toward.astype(np.float64)
    far = np.nextafter(toward, np.where(x < 0, np.float16(-np.inf), np.float16(np.inf)).astype(np.float16))
    tie = (x != t) & (np.abs(x - t) == np.abs(far.astype(np.float64) - x))
    return np.where(tie, far, rn)


def expected(case, fast=False):
    """[image] -> what the kernel must store, in the output's element type"""
    if case.zero:
        return [np.zeros((case.n, case.P, case.P, case.C), np.float16 if case.f16 else np.float32) for _ in range(case.B)]
    if case.f16 and case.dyadic:
        return [round_f16(e) for e in exact(case)]
    ref = (c_reference(case) if fast else None) or reference(case)
    return [r.astype(np.float16) for r in ref] if case.f16 else list(ref)


def sharpness(case):
    """of the non-zero exact outputs of a float16 case: the share that is no float16 value, the share of exact ties, and the
    ties' split (rounded away from zero / toward zero)"""
    x = np.concatenate([e.reshape(-1) for e in exact(case)])
    x = x[x != 0]
    rn = round_f16(x).astype(np.float64)
    lo = round_f16(x, 'trunc').astype(np.float64)
    hi = np.nextafter(round_f16(x, 'trunc'), np.where(x < 0, -np.inf, np.inf).astype(np.float16)).astype(np.float64)
    tie = (x != rn) & (np.abs(x - lo) == np.abs(hi - x))
    n = float(x.size)
    return dict(not_f16=float((x != rn).sum()) / n, ties=float(tie.sum()) / n,
                ties_away=float((tie & (np.abs(rn) > np.abs(x))).sum()) / n, ties_toward=float((tie & (np.abs(rn) < np.abs(x))).sum()) / n)


# ---- the table ------------------------------------------------------------------------------------------------------------------

CASES = []


def _add(*a, **k):
    c = RoiCase(*a, **k)
    assert c.name not in {x.name for x in CASES}, c.name
    CASES.append(c)
    return c


def _tag(f16):
    return 'f16' if f16 else 'f32'


# (a) row and bin paths on a 33 x 33 map, crop 14.  Sample axes (first sample, spacing) in cells; no sample on an integer unless
# the DX == 2 (hi == lo) bin is the point.
PATH_X = [(0.125, 0.25),    # DX 0 throughout: M = 0 first, then M = 2 after a two-column bin and M = 1, alternating
          (0.75, 0.5),      # DX 1 throughout: M = 0 first, then M = 2 after a three-column bin
          (0.625, 0.75),    # DX 1, 0, 1, 0 ...: every bin starts on its neighbour's last column, M = 1
          (0.25, 1.5),      # DX 1 with a column gap between neighbours: M = 0 from a gap
          (0.25, 0.25),     # every second bin has a sample on an integer (DX 2): DX 0 with M = 0 right after a DX 2 bin
          (0.75, 0.75),     # DX 1, 2, 1, 2: DX 1 with M = 0 right after a DX 2 bin
          (0.25, 2.0)]      # DX 2 throughout (samples two cells apart)
PATH_Y = [(0.125, 0.25), (0.75, 0.5), (0.25, 2.0)]                     # DY 0, DY 1, DY 2 on every row


def _path_rois(norm, crop, px=16.0):
    return [roi_for(norm, ax, dx * (crop - 1), ay, dy * (crop - 1), crop, px) for ay, dy in PATH_Y for ax, dx in PATH_X]


for _f16 in (False, True):
    for _C in (256, 8, 260):
        for _pool in (POOL_MAX2, POOL_AVG2):
            _add('paths_%s_c%d_%s' % (_tag(_f16), _C, POOLS[_pool]),
                 'every (DY, DX, M) of the all-inside rows on %s' % ('roi_row_carry' if (_C == 256 and not _f16) else
                                                                    'roi_row<FULL>' if _C == 256 else 'roi_row<!FULL>'),
                 _f16, _pool, NORM_STRIDE, _C, 7, [Image(_path_rois(NORM_STRIDE, 14))], maps_hw=((33, 33),), group='a')
    _add('paths_%s_c256_none' % _tag(_f16), 'the single-sample path, all samples inside', _f16, POOL_NONE, NORM_STRIDE, 256, 7,
         [Image(_path_rois(NORM_STRIDE, 7))], maps_hw=((33, 33),), group='a')

# guarded rows on a 17 x 17 map: (first sample, extent) per axis
A_IN, A_LO, A_HI, A_BOTH, A_OUT = (1.25, 6.5), (-1.25, 6.5), (10.75, 6.5), (-1.75, 19.5), (20.0, 6.5)
GUARD_YX = [(A_LO, A_IN), (A_HI, A_IN), (A_BOTH, A_IN), (A_IN, A_LO), (A_IN, A_HI), (A_IN, A_BOTH), (A_LO, A_LO), (A_HI, A_HI),
            (A_BOTH, A_BOTH), (A_OUT, A_IN), (A_IN, A_OUT), (A_IN, A_IN), ((0.125, 3.25), (0.75, 6.5))]


def _rois_yx(norm, crop, yx, px=16.0):
    return [roi_for(norm, x[0], x[1], y[0], y[1], crop, px) for y, x in yx]


for _f16 in (False, True):
    for _C in (64, 1024):
        for _pool in (POOL_MAX2, POOL_AVG2):
            _add('guarded_%s_c%d_%s' % (_tag(_f16), _C, POOLS[_pool]),
                 'guarded rows: top / bottom / both sample rows out, x out on the left / right / both, a RoI all outside; %s'
                 % ('a sliced launch' if _C == 1024 else 'one slice'),
                 _f16, _pool, NORM_STRIDE, _C, 7, [Image(_rois_yx(NORM_STRIDE, 14, GUARD_YX))], group='a',
                 want_plan=dict(slices=4, roi_groups=2, rois_per_xcd=7, grid_x=56) if _C == 1024 else dict(slices=1))

# (b) all 24 instantiations: all-inside rows, guarded rows, and for the padded tensorpack form samples in the pad ring on each of
# the four sides (index clamps to 0 and to dim - 1) plus samples beyond the ring
R_LO, R_HI, O_LO, O_HI = (-0.75, 6.5), (10.25, 6.5), (-1.75, 6.5), (11.25, 6.5)
INST_YX = [(A_IN, A_IN), (R_LO, A_IN), (R_HI, A_IN), (A_IN, R_LO), (A_IN, R_HI), (R_LO, R_HI), (R_HI, R_LO), (O_LO, A_IN),
           (O_HI, A_IN), (A_IN, O_LO), (A_IN, O_HI), (O_LO, O_HI), (A_OUT, A_IN), ((0.125, 3.25), (0.75, 6.5))]
for _f16 in (False, True):
    for _norm in (NORM_STRIDE, NORM_IMAGE, NORM_TP, NORM_NOPAD):
        for _pool in (POOL_NONE, POOL_MAX2, POOL_AVG2):
            _add('inst_%s_%s_%s' % (_tag(_f16), NORMS[_norm], POOLS[_pool]),
                 'the (%s, %s, %s) instantiation: all-inside and guarded rows' % (POOLS[_pool], NORMS[_norm], _tag(_f16)),
                 _f16, _pool, _norm, 64, 7, [Image(_rois_yx(_norm, 7 if _pool == POOL_NONE else 14, INST_YX))],
                 image_shape=(256, 256), group='b')

# (c) coordinate edges, 17 x 17 map, stride 16 (cell c = pixel 16 c; dim - 1 = 16 cells = pixel 256)
_UP = float(np.nextafter(F32(256), F32(np.inf)))
_DN0 = float(np.nextafter(F32(0), F32(-1)))
EDGE_AT = [[0.0, 0.0, 104.0, 104.0],            # first sample exactly 0 on both axes
           [152.0, 152.0, 256.0, 256.0],        # last sample exactly dim - 1 on both axes
           [0.0, 152.0, 256.0, 256.0], [152.0, 0.0, 256.0, 104.0],
           [256.0, 40.0, 256.0, 200.0],         # degenerate x1 == x2 == dim - 1
           [40.0, 256.0, 200.0, 256.0],         # degenerate y1 == y2 == dim - 1
           [-0.0, -0.0, -0.0, -0.0],            # -0.0 is inside
           [_DN0, 40.0, _DN0, 200.0],           # nextafter(0, -1) / stride underflows to -0.0: inside
           [16.0, 16.0, 224.0, 224.0],          # integer interior samples (spacing one cell): hi == lo, class 2
           [84.0, 20.0, 84.0, 228.0], [20.0, 84.0, 228.0, 84.0], [84.0, 84.0, 84.0, 84.0]]      # degenerate interior
EDGE_BEYOND = [[_UP, 40.0, _UP, 200.0], [40.0, _UP, 200.0, _UP], [_UP, _UP, _UP, _UP],           # one ulp beyond dim - 1
               [_DN0 * 2 ** 60, 40.0, _DN0 * 2 ** 60, 200.0], [40.0, -2.0 ** -100, 200.0, -2.0 ** -100],   # just below 0
               [-2.0 ** -100, -2.0 ** -100, -2.0 ** -100, -2.0 ** -100],
               [_UP, -2.0 ** -100, _UP, -2.0 ** -100],
               [40.0, 40.0, 200.0, 200.0]]      # (one live RoI)
EDGE_REV = [[200.0, 40.0, 40.0, 200.0], [40.0, 200.0, 200.0, 40.0], [200.0, 200.0, 40.0, 40.0],   # reversed: x, y, both
            [256.0, 256.0, 0.0, 0.0], [300.0, 100.0, -40.0, 20.0], [40.0, 40.0, 200.0, 200.0]]
for _f16 in (False, True):
    for _pool in (POOL_NONE, POOL_MAX2, POOL_AVG2):
        _t = '%s_%s' % (_tag(_f16), POOLS[_pool])
        _add('edge_at_%s' % _t, 'samples exactly at 0 and at dim - 1, -0.0, integer interior samples, degenerate boxes',
             _f16, _pool, NORM_STRIDE, 64, 7, [Image(EDGE_AT)], group='c', aim=('lt',))
        _add('edge_beyond_%s' % _t, 'samples one ulp beyond dim - 1 and just below 0 (degenerate boxes put every sample there)',
             _f16, _pool, NORM_STRIDE, 64, 7, [Image(EDGE_BEYOND)], group='c', aim=('ulp',))
    _add('edge_reversed_%s_max2' % _tag(_f16), 'reversed boxes (negative scale) on x, on y and on both', _f16, POOL_MAX2,
         NORM_STRIDE, 64, 7, [Image(EDGE_REV)], group='c')
    _add('edge_reversed_%s_none' % _tag(_f16), 'reversed boxes, single-sample path', _f16, POOL_NONE, NORM_IMAGE, 64, 7,
         [Image(EDGE_REV)], image_shape=(256, 256), group='c')
    _add('edge_p1_centre_%s' % _tag(_f16), 'P = 1 under NONE: the centre sample at -0.0 (inside), at 0, at dim - 1 and beyond', _f16,
         POOL_NONE, NORM_STRIDE, 64, 1, [Image([[-0.0, -0.0, -0.0, -0.0], [-0.0, 40.0, -0.0, 200.0], [0.0, 0.0, 0.0, 0.0],
                                                [256.0, 256.0, 256.0, 256.0], [200.0, 256.0, 312.0, 256.0], [_UP, 40.0, _UP, 40.0],
                                                [40.0, 40.0, 200.0, 200.0], [-8.0, 40.0, 8.0, 200.0], [-8.0, 40.0, 4.0, 200.0]])],
         group='c')
    for _hw in ((1, 17), (17, 1), (1, 1)):
        _add('edge_map%dx%d_%s' % (_hw + (_tag(_f16),)), 'a %d x %d map under NORM_IMAGE (dim - 1 == 0: every sample at 0)' % _hw,
             _f16, POOL_MAX2, NORM_IMAGE, 64, 7, [Image(EDGE_REV + EDGE_AT[:4])], maps_hw=(_hw,), image_shape=(256, 256), group='c')

# declared behaviour with no reference: the output is all zeros
_NAN, _INF = float('nan'), float('inf')
ZERO_COORDS = [[_NAN, 40.0, 200.0, 200.0], [40.0, _NAN, 200.0, 200.0], [40.0, 40.0, _NAN, 200.0], [40.0, 40.0, 200.0, _NAN],
               [_INF, 40.0, 200.0, 200.0], [40.0, -_INF, 200.0, 200.0], [40.0, 40.0, _INF, 200.0], [40.0, 40.0, 200.0, -_INF],
               [_NAN, _NAN, _NAN, _NAN], [-_INF, -_INF, _INF, _INF], [_INF, _INF, _INF, _INF]]
for _f16 in (False, True):
    for _pool, _norm in ((POOL_MAX2, NORM_STRIDE), (POOL_NONE, NORM_IMAGE), (POOL_AVG2, NORM_TP), (POOL_AVG2, NORM_NOPAD)):
        _add('zero_nonfinite_%s_%s_%s' % (_tag(_f16), NORMS[_norm], POOLS[_pool]), 'NaN / +-inf box coordinates: no tap is formed',
             _f16, _pool, _norm, 64, 7, [Image(ZERO_COORDS)], image_shape=(256, 256), group='z', zero=True)
    _add('zero_stride_1xW_%s' % _tag(_f16), 'NORM_STRIDE on a one-row map: division by dim - 1 == 0', _f16, POOL_MAX2, NORM_STRIDE,
         64, 7, [Image(EDGE_AT[:4] + EDGE_REV)], maps_hw=((1, 17),), group='z', zero=True)
    _add('zero_stride_Hx1_%s' % _tag(_f16), 'NORM_STRIDE on a one-column map', _f16, POOL_NONE, NORM_STRIDE,
         64, 7, [Image(EDGE_AT[:4] + EDGE_REV)], maps_hw=((17, 1),), group='z', zero=True)

# (d) launch forms.  13 RoIs per image, drawn per image from one pool (inside, guarded, fine and coarse spacing)
POOL17 = GUARD_YX + [(R_LO, R_HI), ((2.75, 13.0), (0.125, 3.25)), ((0.625, 9.75), (3.375, 9.75)), ((5.125, 3.25), (8.75, 6.5))]


def _form_images(name, B, norm, crop, counts=(None,), px=16.0, n=13):
    rng = np.random.default_rng(zlib.crc32(('rois ' + name).encode()))
    return [Image([_rois_yx(norm, crop, POOL17, px)[i] for i in rng.permutation(len(POOL17))[:n]], count=counts[b % len(counts)])
            for b in range(B)]


def _add_form(name, purpose, f16, pool, C, P, want_plan, n=13, order=None, maps_hw=((17, 17),), counts=(None,)):
    crop = P * (1 if pool == POOL_NONE else 2)
    return _add(name, purpose, f16, pool, NORM_STRIDE, C, P, _form_images(name, 1, NORM_STRIDE, crop, counts, n=n),
                maps_hw=maps_hw, group='d', want_plan=want_plan, order=order)


_add_form('form_p7_f32', 'P = 7, one slice, a workgroup per RoI; the device count below n', False, POOL_MAX2, 256, 7,
          dict(waves=7, slices=1, nblocks=13, blocks_per_xcd=2, grid_x=16, grid_y=1, threads=448), counts=(9,))
_add_form('form_p7_f16_spatial', 'P = 7 with ops.roi_order\'s processing order', True, POOL_MAX2, 256, 7,
          dict(waves=7, slices=1, grid_x=16), order='spatial')
for _f16 in (False, True):
    _add_form('form_p17_%s' % _tag(_f16), 'P = 17: 8 waves per workgroup, n P = 221 rows (no multiple of 8), workgroups straddling '
              'two RoIs', _f16, POOL_MAX2, 256, 17, dict(waves=8, slices=1, nblocks=28, blocks_per_xcd=4, grid_x=32, threads=512),
              order='reversed' if _f16 else None)
    _add_form('form_p17_c512_%s' % _tag(_f16), 'P = 17 with C = 512: two 256-channel slices walked inside one wave', _f16, POOL_AVG2,
              512, 17, dict(waves=8, slices=1, nblocks=28, grid_x=32), counts=(20,))
    _add_form('form_p64_c8_%s' % _tag(_f16), 'P = 64 (every lane holds a bin column) with C = 8', _f16, POOL_MAX2, 8, 64,
              dict(waves=8, slices=1, nblocks=24, blocks_per_xcd=3, grid_x=24, threads=512), n=3, maps_hw=((33, 33),))
    _add_form('form_p1_none_%s' % _tag(_f16), 'P = 1 under NONE: the crop == 1 centre sample', _f16, POOL_NONE, 64, 1,
              dict(waves=1, slices=1, nblocks=13, blocks_per_xcd=2, grid_x=16, threads=64), order='identity')
    _add_form('form_p1_max2_%s' % _tag(_f16), 'P = 1 under MAX2: crop 2, the samples on the box corners', _f16, POOL_MAX2, 64, 1,
              dict(waves=1, slices=1, grid_x=16, threads=64))
    for _C, _lit in ((512, dict(slices=2, roi_groups=4, rois_per_xcd=4, blocks_per_xcd=4, grid_x=32)),
                     (768, dict(slices=3, roi_groups=0, rois_per_xcd=2, blocks_per_xcd=6, grid_x=48)),
                     (1024, dict(slices=4, roi_groups=2, rois_per_xcd=7, blocks_per_xcd=7, grid_x=56)),
                     (2048, dict(slices=8, roi_groups=1, rois_per_xcd=13, blocks_per_xcd=13, grid_x=104))):
        _pool = POOL_MAX2 if (_C // 256 + _f16) % 2 == 0 else POOL_NONE
        _add_form('form_b1_c%d_%s' % (_C, _tag(_f16)), 'B = 1, sliced: %d slices, %s' % (
            _lit['slices'], 'roi_groups %d' % _lit['roi_groups'] if _lit['roi_groups'] else 'slice-major on 8 XCDs'), _f16, _pool, _C, 7,
            dict(_lit, waves=7, xcd_images=0, xcds_per_img=8, grid_y=1), counts=(None if _C != 768 else 11,),
            order=('reversed' if _C == 1024 else None))

# batched launches through the public step ABI (FrcnnStepBatch: STRIDE x {MAX2, NONE}; FpnStepBatch: IMAGE x MAX2, four levels)
BATCH_COUNTS = (9, 20, 0, 5, 31, 0, 12, 20)          # below K, above K (clamped by the kernel), 0, ...
BATCH_FORMS = [(2, 512, dict(xcds_per_img=4, slices=2, roi_groups=2, rois_per_xcd=7, grid_x=56)),
               (2, 768, dict(xcds_per_img=4, slices=3, roi_groups=0, rois_per_xcd=4, blocks_per_xcd=12, grid_x=96)),
               (2, 1024, dict(xcds_per_img=4, slices=4, roi_groups=1, rois_per_xcd=13, grid_x=104)),
               (4, 512, dict(xcds_per_img=2, slices=2, roi_groups=1, rois_per_xcd=13, grid_x=104)),
               (4, 1024, dict(xcds_per_img=2, slices=4, roi_groups=0, rois_per_xcd=7, blocks_per_xcd=28, grid_x=224)),
               (8, 512, dict(xcds_per_img=1, slices=2, roi_groups=0, rois_per_xcd=13, blocks_per_xcd=26, grid_x=208)),
               (8, 1024, dict(xcds_per_img=1, slices=4, roi_groups=0, rois_per_xcd=13, blocks_per_xcd=52, grid_x=416)),
               (3, 512, dict(xcd_images=0, xcds_per_img=8, slices=2, roi_groups=4, rois_per_xcd=4, grid_x=32, grid_y=3)),
               (5, 512, dict(xcd_images=0, xcds_per_img=8, slices=2, roi_groups=4, rois_per_xcd=4, grid_x=32, grid_y=5))]
_ORDERS = ('identity', 'reversed', 'spatial')
for _i, (_B, _C, _lit) in enumerate(BATCH_FORMS):
    for _j, (_pool, _f16) in enumerate(((POOL_MAX2, bool(_i % 2)), (POOL_NONE, not _i % 2))):
        _name = 'batch_frcnn_b%d_c%d_%s_%s' % (_B, _C, POOLS[_pool], _tag(_f16))
        _add(_name, 'FrcnnStepBatch, B = %d, C = %d: %s' % (_B, _C, ', '.join('%s %s' % kv for kv in sorted(_lit.items()))),
             _f16, _pool, NORM_STRIDE, _C, 7, _form_images(_name, _B, NORM_STRIDE, 7 if _pool == POOL_NONE else 14, BATCH_COUNTS),
             image_shape=(272, 272), via='frcnn', group='d', order=_ORDERS[(_i + _j) % 3],
             want_plan=dict(_lit, waves=7, xcd_images=_lit.get('xcd_images', 1), grid_y=_lit.get('grid_y', 1)))

FPN_HW = ((33, 33), (17, 17), (9, 9), (5, 5))          # image 128 x 128: 4, 8, 16, 32 pixels per cell


def _fpn_images(name, B):
    rng = np.random.default_rng(zlib.crc32(('rois ' + name).encode()))
    out = []
    for b in range(B):
        rois, lv = [], []
        for r in range(13):
            level = int(rng.integers(0, 4))
            m = FPN_HW[level][0] - 1
            ext = m * 13.0 / 32
            ys, xs = ((0.375, -0.75, m * 0.5 + 0.125, 0.25 * m)[int(rng.integers(0, 4))] for _ in range(2))
            rois.append(roi_for(NORM_IMAGE, xs, ext * (1 + int(rng.integers(0, 2))), ys, ext, 14, 128.0 / m))
            lv.append(level if r % 5 else (-1 if level == 0 else 6 if level == 3 else level))      # (out of range: clamped)
        order = np.argsort(np.clip(lv, 0, 3), kind='stable')         # level-sorted, as the proposal stage leaves them
        out.append(Image(np.asarray(rois)[order], level=np.asarray(lv)[order], count=BATCH_COUNTS[(b + 1) % len(BATCH_COUNTS)]))
    return out


for _B, _C, _f16, _order, _lit in ((2, 256, False, 'spatial', dict(xcd_images=1, xcds_per_img=4, slices=1, nblocks=13, blocks_per_xcd=4, grid_x=32)),
                                   (8, 256, True, 'identity', dict(xcd_images=1, xcds_per_img=1, slices=1, blocks_per_xcd=13, grid_x=104)),
                                   (3, 256, True, 'reversed', dict(xcd_images=0, slices=1, blocks_per_xcd=2, grid_x=16, grid_y=3)),
                                   (2, 512, False, 'reversed', dict(xcds_per_img=4, slices=2, roi_groups=2, rois_per_xcd=7, grid_x=56)),
                                   (4, 512, True, 'spatial', dict(xcds_per_img=2, slices=2, roi_groups=1, rois_per_xcd=13, grid_x=104)),
                                   (8, 512, False, 'identity', dict(xcds_per_img=1, slices=2, roi_groups=0, rois_per_xcd=13, grid_x=208)),
                                   (5, 512, True, 'spatial', dict(xcd_images=0, slices=2, roi_groups=4, grid_x=32, grid_y=5))):
    _name = 'batch_fpn_b%d_c%d_%s' % (_B, _C, _tag(_f16))
    _add(_name, 'FpnStepBatch over four levels (levels outside the range are clamped), B = %d, C = %d' % (_B, _C), _f16, POOL_MAX2,
         NORM_IMAGE, _C, 7, _fpn_images(_name, _B), maps_hw=FPN_HW, image_shape=(128, 128), via='fpn', group='d', order=_order,
         want_plan=dict(_lit, waves=7))
_add('fpn_levels_f32_ops', 'four levels through the single-image entry point, levels outside the range clamped', False, POOL_MAX2,
     NORM_IMAGE, 256, 7, _fpn_images('fpn_levels_f32_ops', 1), maps_hw=FPN_HW, image_shape=(128, 128), group='d',
     want_plan=dict(waves=7, slices=1, grid_x=16))

# (e) float16 rounding, sharp: 17 x 17 x 8 maps, 24 RoIs whose samples fall every half cell from corners on quarter cells
def _sharp_rois(crop):
    rng = np.random.default_rng(24)
    ext = (crop - 1) / 2.0
    hi = int((16 - ext) * 4)
    return [roi_for(NORM_STRIDE, int(rng.integers(0, hi + 1)) / 4.0, ext, int(rng.integers(0, hi + 1)) / 4.0, ext, crop)
            for _ in range(24)]


for _pool in (POOL_NONE, POOL_MAX2, POOL_AVG2):
    _rois = _sharp_rois(7 if _pool == POOL_NONE else 14)
    # (ties away from zero differs from nearest-even on the ties that round toward zero, half of them: AVG2's ties, a twentieth
    # of its outputs, cannot show it on a twentieth -- that contract is aimed at NONE and MAX2, AVG2 has the per-sample rounding)
    for _data, _what in (('ints', 'even integers in [2048, 4096): results between float16 values, exact ties in both directions'),
                         ('subnormal', 'the same scaled into float16\'s subnormal range: nothing may be flushed'),
                         ('max', 'maps at +-65504: AVG2 must not overflow')):
        _add('sharp_f16_%s_%s' % (_data, POOLS[_pool]), _what, True, _pool, NORM_STRIDE, 8, 7, [Image(_rois)], data=_data, group='e',
             aim=(('trunc', 'sample16') if _pool == POOL_AVG2 else ('trunc', 'away')) if _data == 'ints' else ())
    _add('sharp_f32_ints_%s' % POOLS[_pool], 'the float32 twin: integers below 2^12, exact in float32', False, _pool, NORM_STRIDE, 8, 7,
         [Image(_rois)], data='ints', group='e')

BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]


def plan_only_call(case, lib):
    """the single-image case through its C entry point in the diagnostic library's plan-only mode (the launcher checks, plans,
    records and returns before any HIP call; pointer-valued integers stand for the arrays) -> the recorded plan"""
    import ctypes as C
    from tf_eager_object_detection_amd import _lib
    from tools import _diag
    assert case.B == 1
    nl = len(case.maps_hw)
    levels = (_lib.OdetLevel * nl)()
    for l, (h, w) in enumerate(case.maps_hw):
        levels[l].data, levels[l].H, levels[l].W, levels[l].stride = 0x10000 * (l + 1), h, w, case.stride
    fake = C.c_void_p(0x1000)
    level = fake if case.images[0].level is not None else None
    count = fake if case.images[0].count is not None else None
    ih, iw = case.image_shape
    tail = (case.norm, ih, iw, case.P, case.pool, fake, None)
    before = _diag.last_roi_plan(lib)['count']
    lib.odet_debug_plan_only(1)
    try:
        if case.f16:
            rc = lib.odet_roi_pool_f16(levels, nl, case.C, fake, level, case.n, count, fake if case.order else None, *tail)
        elif case.order:
            rc = lib.odet_roi_pool_ordered(levels, nl, case.C, fake, level, case.n, count, fake, *(tail + (None, None)))
        else:
            rc = lib.odet_roi_pool(levels, nl, case.C, fake, level, case.n, count, *tail)
    finally:
        lib.odet_debug_plan_only(0)
    assert rc == 0, lib.odet_last_error()
    plan = _diag.last_roi_plan(lib)
    assert plan['count'] == before + 1
    return plan


# ---- running a case on the GPU (inside tools._diag.diag_library()) ---------------------------------------------------------------

def nan_filled(shape, dtype, device):
    import torch
    return torch.full(shape, float('nan'), dtype=dtype, device=device)


def _order_tensor(case, img, rois_t, level_t, count_t, dev):
    import torch
    from tf_eager_object_detection_amd import ops
    if case.order == 'spatial':
        shape = case.image_shape if case.image_shape[0] else (case.maps_hw[0][0] * int(case.stride), case.maps_hw[0][1] * int(case.stride))
        return ops.roi_order(rois_t, level_t, shape, count_dev=count_t)
    o = case.orders()[img]
    return None if o is None else torch.from_numpy(o).to(dev)


def run_single(case, img=0, order=True):
    """image `img` of the case through ops.roi_pool -> numpy, the output pre-filled with NaN"""
    import torch
    from tf_eager_object_detection_amd import ops
    dev = torch.device('cuda')
    im = case.images[img]
    maps = [torch.from_numpy(np.ascontiguousarray(m)).to(dev)[None] for m in case.maps()[img]]
    rois = torch.from_numpy(im.rois).to(dev)
    level = None if im.level is None else torch.from_numpy(im.level).to(dev)
    count = None if im.count is None else torch.tensor([im.count], dtype=torch.int32, device=dev)
    out = nan_filled((case.n, case.P, case.P, case.C), torch.float16 if case.f16 else torch.float32, dev)
    ops.roi_pool(maps, rois, level, case.norm, case.P, case.pool, strides=[case.stride] * len(maps),
                 image_shape=case.image_shape if case.image_shape[0] else None, count_dev=count, out=out,
                 order=_order_tensor(case, img, rois, level, count, dev) if order else None)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def run_batch(case):
    """the case's images in ONE launch through FrcnnStepBatch / FpnStepBatch: the test writes every slot's RoIs, levels, count and
    order, pre-fills the features with NaN and enqueues STAGE_ROI alone -> [image] numpy"""
    import torch
    from tf_eager_object_detection_amd.pipeline import FpnStepBatch, FrcnnStepBatch
    dev = torch.device('cuda')
    fdt = torch.float16 if case.f16 else torch.float32
    if case.via == 'frcnn':
        sb = FrcnnStepBatch(case.B, case.image_shape, 3, case.n, case.C, pool_size=case.P, max_pooling_flag=case.pool == POOL_MAX2,
                            extractor_stride=int(case.stride), feature_dtype=fdt)
    else:
        sb = FpnStepBatch(case.B, case.image_shape, 3, case.n, case.C, pool_size=case.P, feature_dtype=fdt)
    keep = []
    for b, h in enumerate(sb.slots):
        im = case.images[b]
        maps = [torch.from_numpy(np.ascontiguousarray(m)).to(dev)[None].contiguous() for m in case.maps()[b]]
        zeros = [torch.zeros(h.N * 2, device=dev), torch.zeros(h.N * 4, device=dev), torch.zeros((case.n, 3), device=dev),
                 torch.zeros((case.n, 3, 4), device=dev)]
        sb.bind(b, zeros[0], zeros[1], maps if case.via == 'fpn' else maps[0], zeros[2], zeros[3])
        rois = torch.from_numpy(im.rois).to(dev)
        h.rois.copy_(rois)
        level = None
        if case.via == 'fpn':
            h.sorted_rois.copy_(rois)
            level = torch.from_numpy(im.level).to(dev)
            h.roi_level.copy_(level)
        h.roi_count.fill_(int(im.count))
        h.roi_order.copy_(_order_tensor(case, b, rois, level, h.roi_count, dev)[:case.n])
        keep.append((maps, zeros))
    sb.roi_features.copy_(nan_filled(tuple(sb.roi_features.shape), fdt, dev))
    sb.enqueue(sb.STAGE_ROI, case.B)
    torch.cuda.synchronize()
    return [sb.roi_features[b].cpu().numpy() for b in range(case.B)]
