"""The RoI pooling backward (csrc/roi_grad.hip) restated on the CPU in NumPy float32, operation by operation and in the kernels'
order of sums, plus the cases the host and GPU tests share.

 * taps(case, r): the forward's sample rows / columns -- roi_cases' float32 mirror of roi_norm_box / make_axis / make_tap<PAD>.
 * samples(case, maps, r): the crop's samples with lerp_tap's operations (t = tl + (tr - tl) xw; b likewise; t + (b - t) yw),
   extrapolated samples 0.
 * select(case, maps): sel [n,P,P,C] uint8 -- pool4's fmaxf tree, then the first of (0,0),(0,1),(1,0),(1,1) equal to it; 4 = none.
 * backward(case, dy, sel, order): dx per level.  order 'kernel' is the contract: a cell receives its contributions in ascending
   (RoI r; sample row i; top before bottom; sample column j; left before right), each wx * (wy * g) with a separate add.
   'rois_desc' and 'j_first' are two OTHER orders, for the tests that show the order matters.  stats=True also returns, per
   element, the number of contributions and the float64 sum of their absolute values (the tests' bound).

Test infrastructure only."""
import zlib

import numpy as np

import roi_cases as rc

F32 = np.float32
POOL_NONE, POOL_MAX2, POOL_AVG2 = rc.POOL_NONE, rc.POOL_MAX2, rc.POOL_AVG2
NORM_STRIDE, NORM_IMAGE, NORM_TP, NORM_NOPAD = rc.NORM_STRIDE, rc.NORM_IMAGE, rc.NORM_TP, rc.NORM_NOPAD
# the five (norm, pool) pairs the Python layers reach
MODES = [(NORM_STRIDE, POOL_MAX2), (NORM_STRIDE, POOL_NONE), (NORM_IMAGE, POOL_MAX2), (NORM_TP, POOL_AVG2), (NORM_NOPAD, POOL_NONE)]


class GradCase:
    """one image: RoIs (image pixels, x1 y1 x2 y2), their levels, the device count, the level shapes"""

    def __init__(self, name, norm, pool, C, P, rois, level=None, count=None, maps_hw=((17, 17),), stride=16.0, image_shape=(0, 0),
                 data='normal'):
        self.name, self.norm, self.pool, self.C, self.P = name, norm, pool, int(C), int(P)
        self.rois = np.ascontiguousarray(rois, np.float32).reshape(-1, 4)
        self.level = None if level is None else np.asarray(level, np.int32)
        self.count, self.maps_hw, self.stride, self.image_shape, self.data = count, tuple(maps_hw), float(stride), tuple(image_shape), data
        self.n = self.rois.shape[0]
        assert self.level is not None or len(self.maps_hw) == 1

    S = property(lambda self: 1 if self.pool == POOL_NONE else 2)
    crop = property(lambda self: self.P * self.S)
    cnt = property(lambda self: self.n if self.count is None else max(min(int(self.count), self.n), 0))

    def rng(self, what):
        return np.random.default_rng(zlib.crc32(('%s %s' % (self.name, what)).encode()))

    def maps(self):
        """[level] -> float32 [H,W,C]: 'normal' or small integers ('ints': every product and sum of the dyadic cases is exact)"""
        g = self.rng('maps')
        if self.data == 'ints':
            return [g.integers(0, 4, (h, w, self.C)).astype(np.float32) for h, w in self.maps_hw]
        return [g.standard_normal((h, w, self.C)).astype(np.float32) for h, w in self.maps_hw]

    def dy(self):
        g = self.rng('dy')
        shape = (self.n, self.P, self.P, self.C)
        if self.data == 'ints':
            return g.integers(-3, 4, shape).astype(np.float32)
        return g.standard_normal(shape).astype(np.float32)


def taps(case, r, roi=None):
    """(level, (in, ok, lo, hi, lerp) of the sample rows, the same of the sample columns) of RoI r"""
    lvl = 0 if case.level is None else int(min(max(int(case.level[r]), 0), len(case.maps_hw) - 1))
    H, W = case.maps_hw[lvl]
    y1n, x1n, y2n, x2n, Hs, Ws = rc._norm_box(case, case.rois[r] if roi is None else roi, H, W)
    pad = case.norm == NORM_TP
    return lvl, rc._axis_taps(y1n, y2n, Hs, case.crop, pad, H), rc._axis_taps(x1n, x2n, Ws, case.crop, pad, W)


def samples(case, maps, r):
    """float32 [crop, crop, C]: lerp_tap in its operation order; extrapolated samples are 0"""
    lvl, ty, tx = taps(case, r)
    m = maps[lvl]
    with np.errstate(all='ignore'):
        yw, xw = ty[4][:, None, None], tx[4][None, :, None]
        tl, tr = m[ty[2]][:, tx[2]], m[ty[2]][:, tx[3]]
        bl, br = m[ty[3]][:, tx[2]], m[ty[3]][:, tx[3]]
        t = (tl + ((tr - tl) * xw).astype(np.float32)).astype(np.float32)
        b = (bl + ((br - bl) * xw).astype(np.float32)).astype(np.float32)
        v = (t + ((b - t) * yw).astype(np.float32)).astype(np.float32)
    ok = ty[1][:, None, None] & tx[1][None, :, None]
    return np.where(ok, v, F32(0)).astype(np.float32)


def select(case, maps):
    """uint8 [n,P,P,C]; rows at or beyond the count are 4"""
    assert case.pool == POOL_MAX2
    P = case.P
    sel = np.full((case.n, P, P, case.C), 4, np.uint8)
    for r in range(case.cnt):
        v = samples(case, maps, r).reshape(P, 2, P, 2, case.C)
        a, b, c, d = v[:, 0, :, 0], v[:, 0, :, 1], v[:, 1, :, 0], v[:, 1, :, 1]
        o = np.fmax(np.fmax(a, b), np.fmax(c, d))
        with np.errstate(invalid='ignore'):
            sel[r] = np.where(a == o, 0, np.where(b == o, 1, np.where(c == o, 2, np.where(d == o, 3, 4))))
    return sel


def backward(case, dy, sel=None, order='kernel', stats=False):
    """[level] -> float32 [H,W,C] (and with stats: [level] -> int count [H,W,C], [level] -> float64 sum of |contributions|)"""
    assert (case.pool == POOL_MAX2) == (sel is not None)
    S, crop, C = case.S, case.crop, case.C
    dx = [np.zeros((h, w, C), np.float32) for h, w in case.maps_hw]
    num = [np.zeros((h, w, C), np.int64) for h, w in case.maps_hw] if stats else None
    mag = [np.zeros((h, w, C), np.float64) for h, w in case.maps_hw] if stats else None
    dy = np.asarray(dy, np.float32)
    one = F32(1)
    everything = np.ones(C, bool)
    rs = range(case.cnt - 1, -1, -1) if order == 'rois_desc' else range(case.cnt)
    with np.errstate(all='ignore'):
        for r in rs:
            lvl, ty, tx = taps(case, r)
            acc = dx[lvl]

            def add(i, tb, j, lr):
                yy = int(ty[3][i] if tb else ty[2][i])
                xx = int(tx[3][j] if lr else tx[2][j])
                wy = ty[4][i] if tb else F32(one - ty[4][i])
                wx = tx[4][j] if lr else F32(one - tx[4][j])
                g = dy[r, i // S, j // S]
                keep = everything
                if case.pool == POOL_AVG2:
                    g = (g * F32(0.25)).astype(np.float32)
                elif case.pool == POOL_MAX2:
                    keep = sel[r, i // S, j // S] == 2 * (i & 1) + (j & 1)
                con = (wx * (wy * g).astype(np.float32)).astype(np.float32)
                acc[yy, xx] = np.where(keep, (acc[yy, xx] + con).astype(np.float32), acc[yy, xx])
                if stats:
                    num[lvl][yy, xx] += keep
                    mag[lvl][yy, xx] += np.where(keep, np.abs(con.astype(np.float64)), 0.0)

            if order == 'j_first':
                for j in range(crop):
                    for lr in (0, 1):
                        for i in range(crop):
                            for tb in (0, 1):
                                if ty[1][i] and tx[1][j]:
                                    add(i, tb, j, lr)
            else:
                for i in range(crop):
                    if not ty[1][i]:
                        continue
                    for tb in (0, 1):
                        for j in range(crop):
                            if tx[1][j]:
                                add(i, tb, j, 0)
                                add(i, tb, j, 1)
    return (dx, num, mag) if stats else dx


# ---- the float64 statement in torch: autograd through a plain crop_and_resize + pooling -------------------------------------------

def torch_crops(case, tmaps, r):
    """[crop, crop, C] samples of RoI r from torch maps (any dtype), bilinear weights (1 - w) a + w b on the mirror's taps"""
    import torch
    lvl, ty, tx = taps(case, r)
    m = tmaps[lvl]
    dt = m.dtype
    ylo, yhi, xlo, xhi = (torch.as_tensor(np.asarray(a, np.int64), device=m.device) for a in (ty[2], ty[3], tx[2], tx[3]))
    wy = torch.as_tensor(ty[4].astype(np.float64), device=m.device).to(dt)[:, None, None]
    wx = torch.as_tensor(tx[4].astype(np.float64), device=m.device).to(dt)[None, :, None]
    top = (1 - wx) * m[ylo][:, xlo] + wx * m[ylo][:, xhi]
    bot = (1 - wx) * m[yhi][:, xlo] + wx * m[yhi][:, xhi]
    ok = torch.as_tensor(ty[1][:, None, None] & tx[1][None, :, None], device=m.device)
    return torch.where(ok, (1 - wy) * top + wy * bot, torch.zeros((), dtype=dt, device=m.device))


def torch_forward(case, tmaps, sel=None):
    """[n,P,P,C] pooled features as a differentiable torch graph over `tmaps` ([level] -> [H,W,C]).  MAX2: max_pool2d, or with
    `sel` (numpy uint8) the imposed choice -- a gather by index, code 4 contributing nothing.  Rows beyond the count are zero."""
    import torch
    P, C = case.P, case.C
    rows = []
    for r in range(case.n):
        if r >= case.cnt:
            rows.append(torch.zeros((P, P, C), dtype=tmaps[0].dtype, device=tmaps[0].device))
            continue
        v = torch_crops(case, tmaps, r)
        if case.pool == POOL_NONE:
            rows.append(v)
        elif case.pool == POOL_AVG2:
            rows.append(torch.nn.functional.avg_pool2d(v.permute(2, 0, 1)[None], 2)[0].permute(1, 2, 0))
        elif sel is None:
            rows.append(torch.nn.functional.max_pool2d(v.permute(2, 0, 1)[None], 2)[0].permute(1, 2, 0))
        else:
            four = v.reshape(P, 2, P, 2, C).permute(0, 2, 1, 3, 4).reshape(P, P, 4, C)
            s = torch.as_tensor(sel[r].astype(np.int64), device=v.device)
            picked = torch.gather(four, 2, s.clamp(max=3)[:, :, None, :])[:, :, 0, :]
            rows.append(torch.where(s < 4, picked, torch.zeros((), dtype=v.dtype, device=v.device)))
    return torch.stack(rows)


def torch_backward(case, maps, dy, sel=None):
    """[level] -> float64 [H,W,C]: torch autograd of torch_forward in float64"""
    import torch
    tm = [torch.tensor(m.astype(np.float64), requires_grad=True) for m in maps]
    out = torch_forward(case, tm, sel)
    out.backward(torch.tensor(np.asarray(dy, np.float64)))
    return [np.zeros(m.shape) if t.grad is None else t.grad.numpy() for t, m in zip(tm, maps)]


# ---- cases ---------------------------------------------------------------------------------------------------------------------------

def mix_rois(norm, crop, n=13, px=16.0):
    """13 RoIs of roi_cases' pool on a 17 x 17 map: inside, partly outside on each side, all outside, fine and coarse spacing"""
    return rc._rois_yx(norm, crop, rc.POOL17, px)[:n]


def _crop(pool, P):
    return P * (1 if pool == POOL_NONE else 2)


def mode_case(norm, pool, C=8, P=7, data='normal', name=None, count=None):
    return GradCase(name or 'mode_%s_%s_c%d_p%d_%s' % (rc.NORMS[norm], rc.POOLS[pool], C, P, data), norm, pool, C, P,
                    mix_rois(norm, _crop(pool, P)), image_shape=(256, 256), data=data, count=count)


def dyadic_case(norm, pool, P=7, C=4):
    """integer data and RoIs whose samples sit on eighths of a cell whatever the crop (first sample, SPACING per axis), on a map
    whose sampled size minus one is 16 (15 x 15 under the padded tensorpack mode), so that every coordinate, weight, product and
    partial sum is exact in float32: inside, partly outside on each side, on integers (lo == hi), reversed"""
    crop = _crop(pool, P)
    hw = 15 if norm == NORM_TP else 17
    k = max(crop - 1, 1)
    axes = [(0.125, 0.25), (0.75, 0.5), (-1.25, 0.5), (hw - 6.25, 0.75), (2.0, 1.0), (9.5, -0.5), (0.375, 1.125), (3.0, 0.0)]
    yx = [((ay, sy * k), (ax, sx * k)) for (ay, sy), (ax, sx) in zip(axes, axes[3:] + axes[:3])] + \
         [((ay, sy * k), (ax, sx * k)) for (ay, sy), (ax, sx) in zip(axes[:5], axes[1:6])]
    return GradCase('dyadic_%s_%s_p%d' % (rc.NORMS[norm], rc.POOLS[pool], P), norm, pool, C, P, rc._rois_yx(norm, crop, yx),
                    maps_hw=((hw, hw),), image_shape=(256, 256) if norm != NORM_IMAGE else (16 * (hw - 1), 16 * (hw - 1)), data='ints')


def fpn_case(C, data='normal', pool=POOL_MAX2):
    """roi_cases' four-level pyramid (33, 17, 9, 5 at image 128 x 128): 13 level-sorted RoIs, some levels outside the range
    (clamped), the device count below n"""
    im = rc._fpn_images('fpn_levels_f32_ops', 1)[0]
    return GradCase('fpn_c%d_%s_%s' % (C, rc.POOLS[pool], data), NORM_IMAGE, pool, C, 7, im.rois, level=im.level, count=im.count,
                    maps_hw=rc.FPN_HW, image_shape=(128, 128), data=data)


def wide_case(pool=POOL_MAX2):
    """a 3 x 33 map: one cell past the kernel's 32-cell tile; RoIs across the tile edge, inside one tile, in the last cell"""
    crop = _crop(pool, 7)
    yx = [((0.25, 1.5), (29.5, 3.25)), ((0.0, 2.0), (0.5, 31.5)), ((0.5, 1.0), (31.25, 0.5)), ((0.125, 1.75), (24.0, 8.0)),
          ((1.0, 0.5), (31.0, 1.0)), ((0.75, 1.0), (32.0, 0.0)), ((0.5, 1.25), (3.5, 26.0))]
    return GradCase('wide_3x33_%s' % rc.POOLS[pool], NORM_STRIDE, pool, 8, 7, rc._rois_yx(NORM_STRIDE, crop, yx), maps_hw=((3, 33),))


def coords_case(which, norm=NORM_STRIDE, pool=POOL_MAX2, C=8):
    P = 7
    crop = _crop(pool, P)
    if which == 'small':            # RoIs smaller than a cell: all samples in one cell
        yx = [((3.25 + 0.5 * k, 0.5), (5.125 + k, 0.25)) for k in range(7)] + [((16.0, 0.0), (16.0, 0.0)), ((0.0, 0.0), (0.0, 0.0))]
        rois = rc._rois_yx(norm, crop, yx)
    elif which == 'pileup':         # every RoI on cell rows 8 / 9, spread and stacked along x
        yx = [((8.25, 0.5), (0.5 + (k % 5), 6.5 + k)) for k in range(13)]
        rois = rc._rois_yx(norm, crop, yx)
    else:
        rois = {'edge_at': rc.EDGE_AT, 'edge_beyond': rc.EDGE_BEYOND, 'edge_rev': rc.EDGE_REV, 'nonfinite': rc.ZERO_COORDS}[which]
    return GradCase('coords_%s_%s_%s' % (which, rc.NORMS[norm], rc.POOLS[pool]), norm, pool, C, P, rois, image_shape=(256, 256))


def order_case():
    """the data set on which the order of the sums shows: 13 overlapping RoIs on a 9 x 9 map, normal data"""
    yx = [((0.3 + 0.37 * k, 3.1 + 0.21 * k), (0.2 + 0.29 * k, 4.3 - 0.17 * k)) for k in range(13)]
    return GradCase('order', NORM_STRIDE, POOL_MAX2, 8, 7, rc._rois_yx(NORM_STRIDE, 14, yx), maps_hw=((9, 9),))
