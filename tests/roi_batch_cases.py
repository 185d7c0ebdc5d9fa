"""The cases of the RoI pooling over a batch of images (ops.roi_pool_images / roi_pool_argmax_images / roi_pool_backward_images)
that the host and GPU tests share, and their restatement: tests/roi_grad_np.py applied image by image -- the definition of the
batched calls (image b's out, sel and dx are the single-image results on image b alone, bit for bit).

A BatchCase is a list of roi_grad_np.GradCase, one per image, that share the modes, C, P, n, the level shapes, the stride and the
image shape, with other data (the GradCase's name seeds it) and other RoIs per image, so that a wrong image offset changes bytes.
Each is the smallest shape at which its subject can still go wrong.

Test infrastructure only."""
import ctypes as C

import numpy as np

import roi_cases as rc
import roi_grad_np as rg

F32 = np.float32


def _image(base, b, rois=None, level=None, count=None):
    """image b of a batch: `base` with its own name (= its own maps and dy) and, where given, its own RoIs / levels / count"""
    return rg.GradCase('%s_img%d' % (base.name, b), base.norm, base.pool, base.C, base.P, base.rois if rois is None else rois,
                       level=base.level if level is None else level, count=count, maps_hw=base.maps_hw, stride=base.stride,
                       image_shape=base.image_shape, data=base.data)


def _rows_rolled(base, b):
    """the base's RoIs (and levels) in another row order for every image: rolled by 3 b rows, reversed on odd images"""
    idx = np.roll(np.arange(base.n), 3 * b)
    idx = idx[::-1] if b & 1 else idx
    return base.rois[idx], (None if base.level is None else base.level[idx])


def _pixel_boxes(name, n, h, w):
    """n boxes (x1 y1 x2 y2, pixels) over an h x w image: centres anywhere inside, edges of 0.3 .. 0.9 of the image, so that most
    cross a border and together they cover the maps"""
    g = np.random.default_rng(rg.zlib.crc32(name.encode()))
    cy, cx = g.uniform(0.1, 0.9, n) * h, g.uniform(0.1, 0.9, n) * w
    bh, bw = g.uniform(0.3, 0.9, n) * h, g.uniform(0.3, 0.9, n) * w
    return np.stack([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], axis=1).astype(np.float32)


def forward(case, maps):
    """float32 [n,P,P,C]: roi_grad_np.samples (lerp_tap in its operation order) and roi.hip's pool4 -- the fmaxf tree, or
    (((a + b) + c) + d) / 4; rows at or beyond the count are zero"""
    P = case.P
    out = np.zeros((case.n, P, P, case.C), np.float32)
    with np.errstate(all='ignore'):
        for r in range(case.cnt):
            v = rg.samples(case, maps, r)
            if case.pool != rg.POOL_NONE:
                v = v.reshape(P, 2, P, 2, case.C)
                a, b, c, d = v[:, 0, :, 0], v[:, 0, :, 1], v[:, 1, :, 0], v[:, 1, :, 1]
                v = np.fmax(np.fmax(a, b), np.fmax(c, d)) if case.pool == rg.POOL_MAX2 else (((a + b) + c) + d) / F32(4.0)
            out[r] = v
    return out


class BatchCase:
    def __init__(self, name, images, catches):
        self.name, self.images, self.catches = name, list(images), catches
        a = self.images[0]
        for im in self.images:
            assert (im.norm, im.pool, im.C, im.P, im.n, im.maps_hw, im.stride, im.image_shape) == \
                   (a.norm, a.pool, a.C, a.P, a.n, a.maps_hw, a.stride, a.image_shape), name
            assert (im.level is None) == (a.level is None)
        self.B, self.n, self.P, self.C, self.norm, self.pool = len(self.images), a.n, a.P, a.C, a.norm, a.pool
        self.maps_hw, self.stride, self.image_shape = a.maps_hw, a.stride, a.image_shape
        self._memo = {}

    def _once(self, key, make):
        if key not in self._memo:
            v = make()
            for t in (v if isinstance(v, list) else [v]):
                if t is not None:
                    t.setflags(write=False)
            self._memo[key] = v
        return self._memo[key]

    def rois(self):
        return self._once('rois', lambda: np.stack([im.rois for im in self.images]))                        # [B,n,4]

    def level(self):
        return None if self.images[0].level is None else self._once('level', lambda: np.stack([im.level for im in self.images]))

    def counts(self):
        """int32 [B], or None when no image has a count"""
        if all(im.count is None for im in self.images):
            return None
        return self._once('counts', lambda: np.array([im.n if im.count is None else im.count for im in self.images], np.int32))

    def maps(self):
        """[level] -> float32 [B,H,W,C]"""
        def make():
            per = [im.maps() for im in self.images]
            return [np.stack([per[b][l] for b in range(self.B)]) for l in range(len(self.maps_hw))]
        return self._once('maps', make)

    def dy(self):
        return self._once('dy', lambda: np.stack([im.dy() for im in self.images]))                          # [B,n,P,P,C]

    def restated(self):
        """(out [B,n,P,P,C], sel [B,n,P,P,C] or None, [level] -> dx [B,H,W,C]): roi_grad_np on every image alone.  Computed once."""
        def make():
            maps, dy = self.maps(), self.dy()
            outs, sels, dxs = [], [], []
            for b, im in enumerate(self.images):
                mb = [m[b] for m in maps]
                outs.append(forward(im, mb))
                sel = rg.select(im, mb) if im.pool == rg.POOL_MAX2 else None
                sels.append(sel)
                dxs.append(rg.backward(im, dy[b], sel))
            return [np.stack(outs), np.stack(sels) if sels[0] is not None else None] + \
                   [np.stack([dxs[b][l] for b in range(self.B)]) for l in range(len(self.maps_hw))]
        v = self._once('restated', make)
        return v[0], v[1], v[2:]

    def tapped(self, b):
        """the levels image b's counted RoIs lie on"""
        im = self.images[b]
        return sorted({rg.taps(im, r)[0] for r in range(im.cnt)})


def plan(maps_hw, C_, B, n, P):
    """odet_roi_pool_backward_images_plan -> (rc, dict(grid, tiles, starts, slices, lds)); host only"""
    from tf_eager_object_detection_amd import _lib
    lv = (_lib.OdetLevel * len(maps_hw))()
    for l, (h, w) in enumerate(maps_hw):
        lv[l].data, lv[l].H, lv[l].W, lv[l].stride = 0, h, w, 0.0
    grid, tiles, slices, lds = C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_int(-1)
    starts = (C.c_int * len(maps_hw))()
    code = _lib.lib().odet_roi_pool_backward_images_plan(lv, len(maps_hw), C_, B, n, P, C.byref(grid), C.byref(tiles), starts,
                                                         C.byref(slices), C.byref(lds))
    return code, dict(grid=grid.value, tiles=tiles.value, starts=list(starts), slices=slices.value, lds=lds.value)


# ---- the table ----------------------------------------------------------------------------------------------------------------------

def _modes():
    out = []
    for norm, pool in rg.MODES:
        base = rg.mode_case(norm, pool)
        out.append(BatchCase('batch_' + base.name, [_image(base, b, *_rows_rolled(base, b)) for b in range(2)],
                             'a mode that breaks under batching'))
    return out


def _two_level():
    hw, shape, n = ((9, 11), (5, 6)), (72, 88), 13
    ims = []
    for b, count in enumerate((13, 0, 5)):
        rois = _pixel_boxes('two_level_%d' % b, n, *shape)
        area = (rois[:, 2] - rois[:, 0]) * (rois[:, 3] - rois[:, 1])
        level = (area > np.median(area)).astype(np.int32)
        if b == 0:                                        # level-sorted, as _assign_levels hands them over
            order = np.argsort(level, kind='stable')
            rois, level = rois[order], level[order]
        else:                                             # (any row order is allowed) alternating: a count of 5 reaches both levels
            level = (np.arange(n) & 1).astype(np.int32)
        ims.append(rg.GradCase('two_level_img%d' % b, rg.NORM_IMAGE, rg.POOL_MAX2, 8, 7, rois, level=level, count=count, maps_hw=hw,
                               image_shape=shape))
    return BatchCase('batch3_two_levels_counts_13_0_5', ims,
                     "the forward path that takes the image from blockIdx.y; an empty image; a partial count")


def _group_boundary():
    base = rg.GradCase('nine', rg.NORM_STRIDE, rg.POOL_MAX2, 4, 7, _pixel_boxes('nine', 5, 80, 96), maps_hw=((5, 6),))
    return BatchCase('batch9_one_small_level', [_image(base, b, rois=_pixel_boxes('nine_%d' % b, 5, 80, 96)) for b in range(9)],
                     "the forward's second group; the ninth image's offsets")


def _two_x_tiles(pool):
    base = rg.wide_case(pool)
    return BatchCase('batch2_' + base.name, [_image(base, b, *_rows_rolled(base, b)) for b in range(2)], 'x-tile indexing across images')


def _two_slices():
    base = rg.mode_case(rg.NORM_STRIDE, rg.POOL_MAX2, C=264)
    return BatchCase('batch2_c264', [_image(base, b, *_rows_rolled(base, b)) for b in range(2)],
                     'channel slices 256 + 8; the second slice has two active lanes')


def _level_edges():
    # three small levels (roi_grad_np.fpn_case's 33 x 33 level stays mostly untouched by 13 RoIs: 0.43 of its tapped elements live)
    level = (np.arange(13) % 3).astype(np.int32)
    base = rg.GradCase('level_edges', rg.NORM_IMAGE, rg.POOL_MAX2, 8, 7, _pixel_boxes('level_edges', 13, 72, 88), level=level,
                       maps_hw=((9, 11), (5, 6), (3, 3)), image_shape=(72, 88))
    outside = level.copy()
    outside[0], outside[-1], outside[5] = -2, 9, 3        # clamped to 0, 2 and 2, as the forward does
    no_level1 = np.where(level == 1, 2, level).astype(np.int32)
    return BatchCase('batch2_roi_level_edges', [_image(base, 0, level=outside),
                                                _image(base, 1, rois=_pixel_boxes('level_edges_1', 13, 72, 88), level=no_level1)],
                     'out-of-range levels clamped; one level without RoIs in one image only')


def _exact():
    base = rg.dyadic_case(rg.NORM_STRIDE, rg.POOL_MAX2)
    return BatchCase('batch2_' + base.name, [_image(base, b, *_rows_rolled(base, b)) for b in range(2)],
                     'bytes that hold for any correct order, alongside the ordered cases')


CASES = _modes() + [_two_level(), _group_boundary(), _two_x_tiles(rg.POOL_MAX2), _two_x_tiles(rg.POOL_NONE), _two_slices(),
                    _level_edges(), _exact()]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
