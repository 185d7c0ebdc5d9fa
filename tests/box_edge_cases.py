"""Edge-value tables and the float32 statement of the box primitives (csrc/boxes.hip with d_decode_box, d_clip_box, d_pair_iou,
d_encode_box and d_roi_level of csrc/odet_internal.h): decode, encode, clip, the two box filters, where_greater, pairwise_iou,
assign_levels and gather_rows.

THE STATEMENT is oracle/oracle_np.py's operation sequence, one IEEE float32 operation per reference operation, with the one
rule the oracles leave open made explicit: every min / max of clip, of the IoU and of the level is IEEE minNum / maxNum
(`minnum` / `maxnum` below: the operand that is a number wins over a NaN), and every comparison with a NaN is false.  exp and
log are the oracles' correctly rounded form (float64, rounded once).  Decode and encode need no rule: plain arithmetic.

COMPARISON (`same`): NaN at the same positions (payload and sign ignored), +0 == -0, every other value -- infinities included
-- at most `max_ulp` steps of the float32 number line away: 0 everywhere, 1 behind exp / log (decode, encode), the bar
tests/test_gpu_parity.py `close` derives (two float64 libraries may differ in their last bit before the one rounding).

tests/test_box_edges_host.py anchors the statement on the two oracles and checks that the tables reach what they are for;
tests/test_box_edges_gpu.py compares the kernels with it.  Everything here is deterministic and small."""
import numpy as np

F = np.float32
INF, NAN = F(np.inf), F(np.nan)
M0 = (0.0, 0.0, 0.0, 0.0)
S1 = (1.0, 1.0, 1.0, 1.0)
S2 = (0.1, 0.1, 0.2, 0.2)
M1 = (0.5, -0.25, 0.125, 1.0)
IMAGE = (600, 800)                 # (height, width) of every clip / filter case
CP_TILE = 1024                     # CP_BLOCK * CP_ITEMS of csrc/boxes.hip
CP_SCAN_THREADS = 1024             # k_cp_scan: one workgroup, `per` tiles per thread
ASSIGN_MAX_ROIS = 8192             # ODET_ASSIGN_MAX_ROIS
LEVEL_BAND = 1e-4                  # d_roi_level: the exact expression decides inside this distance of an integer
IOU_MAX_COLUMNS = 65535 * 64       # 4 194 240: odet_pairwise_iou's one-launch limit
GATHER_GRID, GATHER_BLOCK = 4096, 256


def f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


def up(x, steps=1):
    """x moved `steps` float32 neighbours up (down when negative)"""
    x = F(x)
    for _ in range(abs(steps)):
        x = np.nextafter(x, INF if steps > 0 else -INF)
    return x


# ---- comparison ---------------------------------------------------------------------------------------------------------
def _line(a):
    """float32 -> int64 position on the number line (+0 and -0 on the same point); NaN must be masked by the caller"""
    i = f32(a).view(np.int32).astype(np.int64)
    return np.where(i < 0, np.int64(-2 ** 31) - i, i)


def ulp_distance(a, b):
    return np.abs(_line(a) - _line(b))


def same(got, want, max_ulp=0, what=''):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, '%s: shape %s, want %s' % (what, got.shape, want.shape)
    if got.dtype != np.float32 or want.dtype != np.float32:
        assert got.dtype.kind in 'iu' and want.dtype.kind in 'iu', '%s: dtypes %s / %s' % (what, got.dtype, want.dtype)
        bad = np.argwhere(got != want)
        assert not len(bad), '%s: %d of %d differ, first at %s: got %s want %s' % (
            what, len(bad), got.size, bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
        return
    if not got.size:
        return
    nan = np.isnan(want)
    bad = np.argwhere(np.isnan(got) != nan)
    assert not len(bad), '%s: NaN at %d other positions, first at %s: got %r want %r' % (
        what, len(bad), bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
    d = ulp_distance(np.where(nan, F(0), got), np.where(nan, F(0), want))
    bad = np.argwhere(d > max_ulp)
    assert not len(bad), '%s: %d of %d beyond %d ulp (worst %d), first at %s: got %r want %r' % (
        what, len(bad), got.size, max_ulp, int(d.max()), bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def count_differences(a, b):
    """how many values of two float32 arrays differ under `same` at 0 ulp"""
    a, b = f32(a), f32(b)
    na, nb = np.isnan(a), np.isnan(b)
    return int(np.sum((na != nb) | (~na & ~nb & (ulp_distance(np.where(na, F(0), a), np.where(nb, F(0), b)) != 0))))


def has_nan(*arrays):
    """per row: does any of the row's inputs hold a NaN"""
    out = None
    for a in arrays:
        r = np.isnan(f32(a).reshape(len(a), -1)).any(axis=1)
        out = r if out is None else out | r
    return out


# ---- the statement ------------------------------------------------------------------------------------------------------
def minnum(a, b):
    """IEEE 754-2008 minNum: the smaller operand; where exactly one is a NaN, the other one"""
    return np.fmin(a, b)


def maxnum(a, b):
    """IEEE 754-2008 maxNum"""
    return np.fmax(a, b)


def exp32(x):
    with np.errstate(all='ignore'):
        return np.exp(f32(x).astype(np.float64)).astype(np.float32)


def log32(x):
    with np.errstate(all='ignore'):
        return np.log(f32(x).astype(np.float64)).astype(np.float32)


def clip(boxes, min_value, max_height, max_width):
    b = f32(boxes).reshape(-1, 4)
    mv, wmax, hmax = F(min_value), F(max_width - 1), F(max_height - 1)
    return np.stack([maxnum(minnum(b[:, 0], wmax), mv), maxnum(minnum(b[:, 1], hmax), mv),
                     maxnum(minnum(b[:, 2], wmax), mv), maxnum(minnum(b[:, 3], hmax), mv)], axis=1)


def decode(anchors, deltas, means, stds, clip_shape=None):
    a = f32(anchors).reshape(-1, 4)
    with np.errstate(all='ignore'):
        d = f32(deltas).reshape(-1, 4) * f32(stds) + f32(means)
        width = a[:, 2] - a[:, 0] + F(1)
        height = a[:, 3] - a[:, 1] + F(1)
        cx = a[:, 0] + F(0.5) * width
        cy = a[:, 1] + F(0.5) * height
        cx = cx + d[:, 0] * width
        cy = cy + d[:, 1] * height
        width = width * exp32(d[:, 2])
        height = height * exp32(d[:, 3])
        x1 = cx - F(0.5) * width
        y1 = cy - F(0.5) * height
        out = np.stack([x1, y1, x1 + width, y1 + height], axis=1)
    return out if clip_shape is None else clip(out, 0, clip_shape[0], clip_shape[1])


def encode(src, dst, means, stds):
    b, g = f32(src).reshape(-1, 4), f32(dst).reshape(-1, 4)
    with np.errstate(all='ignore'):
        width, height = b[:, 2] - b[:, 0] + F(1), b[:, 3] - b[:, 1] + F(1)
        cx, cy = b[:, 0] + F(0.5) * width, b[:, 1] + F(0.5) * height
        gw, gh = g[:, 2] - g[:, 0] + F(1), g[:, 3] - g[:, 1] + F(1)
        gcx, gcy = g[:, 0] + F(0.5) * gw, g[:, 1] + F(0.5) * gh
        d = np.stack([(gcx - cx) / width, (gcy - cy) / height, log32(gw / width), log32(gh / height)], axis=1)
        return (d - f32(means)) / f32(stds)


def clip_filter(boxes, min_value, max_height, max_width, min_edge):
    """-> (kept clipped boxes, their ascending indices)"""
    c = clip(boxes, min_value, max_height, max_width)
    with np.errstate(all='ignore'):
        e0 = c[:, 2] - c[:, 0] + F(1)
        e1 = c[:, 3] - c[:, 1] + F(1)
        keep = (e1 >= F(min_edge)) & (e0 >= F(min_edge))            # a comparison with a NaN is false
    idx = np.nonzero(keep)[0].astype(np.int64)
    return c[idx], idx


def range_filter(boxes, max_height, max_width):
    b = f32(boxes).reshape(-1, 4)
    with np.errstate(all='ignore'):
        keep = (b[:, 0] >= F(0)) & (b[:, 1] >= F(0)) & (b[:, 2] <= F(max_width - 1)) & (b[:, 3] <= F(max_height - 1))
    return np.nonzero(keep)[0].astype(np.int64)


def where_greater(values, threshold):
    with np.errstate(all='ignore'):
        return np.nonzero(f32(values) > F(threshold))[0].astype(np.int64)


def pairwise_iou(b1, b2):
    p, q = f32(b1).reshape(-1, 1, 4), f32(b2).reshape(1, -1, 4)
    with np.errstate(all='ignore'):
        a1 = (p[..., 3] - p[..., 1] + F(1)) * (p[..., 2] - p[..., 0] + F(1))
        a2 = (q[..., 3] - q[..., 1] + F(1)) * (q[..., 2] - q[..., 0] + F(1))
        ih = maxnum(F(0), minnum(p[..., 3], q[..., 3]) - maxnum(p[..., 1], q[..., 1]) + F(1))
        iw = maxnum(F(0), minnum(p[..., 2], q[..., 2]) - maxnum(p[..., 0], q[..., 0]) + F(1))
        inter = ih * iw
        uni = a1 + a2 - inter
        return np.where(inter == F(0), F(0), inter / uni).astype(np.float32)       # NaN == 0 is false: NaN / uni


def roi_levels(rois, min_level, max_level):
    """0-based level (level - min_level) of every RoI"""
    r = f32(rois).reshape(-1, 4)
    with np.errstate(all='ignore'):
        h = maxnum(F(0), r[:, 3] - r[:, 1])
        w = maxnum(F(0), r[:, 2] - r[:, 0])
        lv = np.floor(F(4) + log32(np.sqrt(w * h + F(1e-8)) / F(224)) / log32(F(2)))
        lv = minnum(maxnum(lv, F(min_level)), F(max_level))         # a NaN level (inf x 0) becomes min_level
    return lv.astype(np.int32) - np.int32(min_level)


def assign_levels(rois, min_level, max_level):
    """-> (sorted rois, their 0-based levels, perm int64, counts int32): a stable partition by level"""
    r = f32(rois).reshape(-1, 4)
    lv = roi_levels(r, min_level, max_level)
    perm = np.argsort(lv, kind='stable').astype(np.int64)
    counts = np.bincount(lv, minlength=max_level - min_level + 1).astype(np.int32)
    return r[perm], lv[perm], perm, counts


def gather_rows(src, idx, count=None):
    """the rows the kernel writes: min(count, n) of them"""
    idx = np.asarray(idx)
    cnt = len(idx) if count is None else max(min(int(count), len(idx)), 0)
    return f32(src)[idx[:cnt].astype(np.int64)]


# ---- decode -------------------------------------------------------------------------------------------------------------
DELTA_VALUES = [0.0, 1e-40, -1e-40, 50.0, -50.0, 87.3, 88.0, 88.8, 89.0, 100.0, -87.0, -104.0, -200.0, 1e30, -1e30, 3e38,
                -3e38, np.inf, -np.inf, np.nan]
ANCHOR = (96.0, 64.0, 159.0, 191.0)                      # 64 x 128
ODD_ANCHORS = [(159.0, 191.0, 96.0, 64.0),               # reversed
               (100.0, 100.0, 99.0, 150.0),              # zero width: x2 = x1 - 1
               (100.0, 100.0, 150.0, 99.0),              # zero height
               (1e30, 1e30, 1e30, 1e30), (-1e30, -1e30, 1e30, 1e30), (-1e30, -1e30, -1e30, -1e30)]
ODD_ANCHORS += [tuple(v if k == s else ANCHOR[k] for k in range(4)) for s in range(4) for v in (np.nan, np.inf, -np.inf)]
ODD_DELTAS = [(0.0, 0.0, 0.0, 0.0), (0.1, -0.2, 0.3, -0.1), (0.0, 0.0, 88.8, 0.0), (0.0, 0.0, 0.0, -104.0), (3e38, 0.0, 0.0, 0.0)]
DECODE_SETTINGS = [(M0, S1, None), (M0, S2, None), (M0, S1, IMAGE), (M0, S2, IMAGE)]


def decode_table():
    """-> (anchors [n,4], deltas [n,4])"""
    anchors, deltas = [], []
    for v in DELTA_VALUES:
        for d in ((0, 0, v, 0), (0, 0, 0, v), (0, 0, v, v), (v, 0, 0, 0), (0, v, 0, 0), (v, v, 0, 0), (0.25, -0.5, v, -v),
                  (v, -v, 0.5, -0.5)):
            anchors.append(ANCHOR)
            deltas.append(d)
    for a in ODD_ANCHORS:
        for d in ODD_DELTAS:
            anchors.append(a)
            deltas.append(d)
    rng = np.random.default_rng(31)                       # and a few ordinary rows
    xy = rng.uniform(0, 500, (16, 2))
    anchors += np.concatenate([xy, xy + rng.uniform(1, 300, (16, 2))], axis=1).tolist()
    deltas += rng.normal(0, 1, (16, 4)).tolist()
    with np.errstate(all='ignore'):
        return f32(anchors), f32(deltas)


# ---- encode -------------------------------------------------------------------------------------------------------------
ENCODE_SETTINGS = [(M0, S1), (M0, S2), (M1, S2)]
BOX = (10.0, 20.0, 73.0, 147.0)


def encode_table():
    """-> (src [n,4], gt [n,4])"""
    x1, y1, x2, y2 = BOX
    thin = [(x1, y1, x1 - 1 - k, y2) for k in range(3)] + [(x1, y1, x2, y1 - 1 - k) for k in range(3)]     # width / height 0, -1, -2
    thin += [(x1, y1, x1 - 1, y1 - 1), (x1, y1, x1 - 3, y1 - 2)]
    src, gt = [], []
    for t in thin:                                         # division by zero, log(0), log of a negative
        src += [t, BOX, t]
        gt += [BOX, t, t]
    for a in thin[:3]:
        for b in thin[:3]:
            src.append(a)
            gt.append(b)
    for s in range(4):
        for v in (np.inf, -np.inf, np.nan):
            odd = tuple(v if k == s else BOX[k] for k in range(4))
            src += [odd, BOX, odd]
            gt += [BOX, odd, odd]
    for b in (BOX, (0.0, 0.0, 0.0, 0.0), (-5.5, 3.25, 100.75, 3.25), (1e30, 1e30, 1e30, 1e30), (0.0, 0.0, 3e38, 3e38)):
        src.append(b)                                      # ground truth equal to the source
        gt.append(b)
    huge, one, half = (0.0, 0.0, 3e38, 3e38), (5.0, 5.0, 5.0, 5.0), (5.0, 5.0, 4.5, 4.5)
    wide, small = (0.0, 0.0, 1e38, 2e38), (7.0, 7.0, 6.0 + 2.0 ** -20, 6.0 + 2.0 ** -22)
    src += [huge, half, wide, small, huge, one, small, half]     # ratios: subnormal (1 / 3e38), overflowing (3e38 / 0.5), ...
    gt += [one, huge, small, wide, half, huge, half, small]
    rng = np.random.default_rng(32)
    xy = rng.uniform(0, 500, (16, 2))
    a = np.concatenate([xy, xy + rng.uniform(1, 300, (16, 2))], axis=1)
    src += a.tolist()
    gt += (a + rng.uniform(-3, 3, a.shape)).tolist()
    return f32(src), f32(gt)


# ---- clip and the box filters -------------------------------------------------------------------------------------------
MIN_EDGE = 16.0
CLIP_SETTINGS = [0.0, 10.0, -3.5]                          # min_value
FILTER_SETTINGS = [(0.0, 16.0), (10.0, 16.0), (0.0, 1.0), (-3.5, 0.0)]     # (min_value, min_edge)


def clip_table():
    h, w = IMAGE
    base = (100.0, 100.0, 300.0, 300.0)
    values = [-0.0, np.inf, -np.inf, 1e30, -1e30, 3e38, -3e38, np.nan, -5.0, 1000.0, 10.0, -3.5, 1e-40, -1e-40]
    for edge in (0.0, w - 1.0, h - 1.0, 10.0, -3.5):       # exactly on a border and on its float32 neighbours either side
        values += [F(edge), up(edge, 1), up(edge, -1)]
    rows = [tuple(v if k == s else base[k] for k in range(4)) for v in values for s in range(4)]
    rows += [(np.nan,) * 4, (np.inf,) * 4, (-np.inf,) * 4, (-np.inf, -np.inf, np.inf, np.inf), (np.inf, np.inf, -np.inf, -np.inf),
             (np.nan, np.nan, 300.0, 300.0), (100.0, 100.0, np.nan, np.nan), (np.nan, 100.0, np.nan, 300.0),
             (300.0, 300.0, 100.0, 100.0), (900.0, 700.0, -50.0, -60.0), (0.0, 0.0, w - 1.0, h - 1.0), (0.0, 0.0, float(w), float(h)),
             (-1.0, 0.0, 10.0, 10.0), (0.0, -1.0, 10.0, 10.0), (790.0, 590.0, 900.0, 900.0), (-40.0, -40.0, 14.0, 15.0)]
    for lo in (100.0, 0.0, 10.0):                          # an edge exactly min_edge, and one ulp below it, on either axis
        hi = lo + MIN_EDGE - 1
        rows += [(lo, lo, hi, hi), (lo, lo, up(hi, -1), hi), (lo, lo, hi, up(hi, -1)), (up(lo, 1), lo, hi, hi),
                 (lo, up(lo, 1), hi, hi), (lo, lo, up(hi, 1), up(hi, 1))]
    rows += [(w - MIN_EDGE, h - MIN_EDGE, 2000.0, 2000.0), (up(w - MIN_EDGE, 1), h - MIN_EDGE, 2000.0, 2000.0),
             (w - MIN_EDGE, up(h - MIN_EDGE, 1), 2000.0, 2000.0), (300.0, 300.0, 300.0, 300.0), (300.0, 300.0, up(300, -1), 300.0)]
    with np.errstate(all='ignore'):
        return f32(rows)


# ---- pairwise IoU -------------------------------------------------------------------------------------------------------
IOU_SIZES = [(n, m) for n in (1, 3, 4, 5) for m in (1, 63, 64, 65)]


def iou_boxes():
    """The IoU table is every pair of these boxes, in both operand orders.  (`uni == 0` is reached only together with
    `inter == 0`, the pairs of two zero-area boxes, where the result is 0 and not 0 / 0: a box with a width or a height <= 0
    has an intersection of 0 with everything, and two boxes of positive area have a union >= the larger area.)"""
    a = (10.0, 10.0, 50.0, 50.0)
    rows = [a, a,                                            # identical
            (51.0, 10.0, 90.0, 50.0), (10.0, 51.0, 50.0, 90.0),    # touching: iw / ih exactly 0
            (50.0, 10.0, 90.0, 50.0), (50.0, 50.0, 90.0, 90.0),    # one shared column / pixel
            (20.0, 20.0, 30.0, 30.0), (0.0, 0.0, 799.0, 599.0), (10.5, 10.25, 49.75, 50.125),
            (50.0, 50.0, 10.0, 10.0), (50.0, 10.0, 10.0, 50.0),    # reversed in both axes (area > 0) and in one (area < 0)
            (10.0, 10.0, 9.0, 50.0), (10.0, 10.0, 50.0, 9.0), (10.0, 10.0, 9.0, 9.0),      # zero width / height / both
            (30.0, 30.0, 29.0, 29.0),                                # a second zero-area box: uni == 0 with inter == 0
            (10.0, 10.0, 5.0, 50.0), (10.0, 10.0, 8.0, 8.0),         # negative width; both negative (area 1)
            (0.0, 0.0, 1e20, 1e20), (-1e20, -1e20, 1e20, 1e20), (-3e38, -3e38, 3e38, 3e38), (3e38, 3e38, 3e38, 3e38),
            (0.0, 0.0, np.inf, np.inf), (-np.inf, -np.inf, np.inf, np.inf), (np.inf, np.inf, np.inf, np.inf),
            (-np.inf, 10.0, 50.0, 50.0), (10.0, 10.0, 50.0, np.inf), (-np.inf, -np.inf, -np.inf, -np.inf)]
    rows += [tuple(np.nan if k == s else a[k] for k in range(4)) for s in range(4)]
    rows.append((np.nan,) * 4)
    return f32(rows)


def iou_operands(n, m):
    """n x m operands that keep every kind of box of the table at every size"""
    t = iou_boxes()
    k = len(t)
    return t[(np.arange(n) * 7 + 3) % k], t[(np.arange(m) * 5 + n) % k]


def iou_wide(m):
    """one box against m columns (the column limit): the table, cycled, between ordinary boxes"""
    t = iou_boxes()
    rng = np.random.default_rng(33)
    xy = rng.uniform(0, 700, (m, 2)).astype(np.float32)
    b2 = np.concatenate([xy, xy + rng.uniform(0, 200, (m, 2)).astype(np.float32)], axis=1)
    b2[::97] = t[np.arange(len(b2[::97])) % len(t)]
    return f32([[300.0, 200.0, 500.0, 450.0]]), b2


# ---- assign_levels ------------------------------------------------------------------------------------------------------
LEVEL_RANGES = [(2, 5), (0, 7)]                            # the model's, and one where every boundary below moves the result
LEVEL_BOUNDARIES = [224.0 * 2.0 ** k for k in range(-2, 3)]
LEVEL_NEIGHBOURS = 512


def level_sweep():
    """-> (rois [n,4], boundary index per row or -1): squares (0, 0, e, e) with e walking the float32 neighbours of each
    boundary edge length, geometric steps out to 1e-3 relative, and non-square pairs with the same product"""
    rois, which = [], []
    for bi, b in enumerate(LEVEL_BOUNDARIES):
        lo = up(b, -LEVEL_NEIGHBOURS)
        e = lo
        for _ in range(2 * LEVEL_NEIGHBOURS + 1):
            rois.append((0.0, 0.0, e, e))
            e = np.nextafter(e, INF)
        for t in np.linspace(3.0, 7.0, 17):
            for s in (1.0, -1.0):
                e = F(b * (1.0 + s * 10.0 ** -t))
                rois += [(0.0, 0.0, e, e), (37.0, 11.0, F(37.0) + e, F(11.0) + e)]
        for j in range(-8, 9):
            e = up(b, j)
            rois += [(0.0, 0.0, F(2) * e, e / F(2)), (0.0, 0.0, e / F(4), F(4) * e), (0.0, 0.0, F(3) * e, e / F(3)),
                     (5.0, 9.0, F(5) + e / F(7), F(9) + F(7) * e)]
        which += [bi] * (len(rois) - len(which))
    odd = [(5.0, 5.0, 5.0, 5.0), (5.0, 5.0, 100.0, 5.0), (10.0, 10.0, 5.0, 5.0), (10.0, 10.0, 5.0, 500.0), (0.0, 0.0, 1e-30, 1e-30),
           (0.0, 0.0, 1e-4, 1e-4), (0.0, 0.0, 1e20, 1e20), (0.0, 0.0, 3e38, 3e38), (-3e38, -3e38, 3e38, 3e38), (0.0, 0.0, np.inf, np.inf),
           (0.0, 0.0, np.inf, 0.0), (0.0, 0.0, 0.0, np.inf), (np.inf, np.inf, np.inf, np.inf), (-np.inf, 0.0, np.inf, 100.0),
           (np.nan,) * 4, (0.0, 0.0, 1.0, 1.0), (0.0, 0.0, 799.0, 599.0)]
    odd += [tuple(np.nan if k == s else (0.0, 0.0, 224.0, 224.0)[k] for k in range(4)) for s in range(4)]
    rois += odd
    which += [-1] * len(odd)
    rng = np.random.default_rng(34)                        # interleave: levels alternate inside every thread's run of RoIs
    order = rng.permutation(len(rois))
    rois, which = f32(rois)[order], np.array(which)[order]
    assert len(rois) <= ASSIGN_MAX_ROIS
    return rois, which


def level_position(rois):
    """float64: the unrounded 4 + log2(sqrt(w h + 1e-8) / 224) of finite upright RoIs"""
    r = f32(rois).astype(np.float64)
    return 4.0 + np.log2(np.sqrt((r[:, 2] - r[:, 0]) * (r[:, 3] - r[:, 1]) + 1e-8) / 224.0)


# ---- compaction ---------------------------------------------------------------------------------------------------------
COMPACT_SIZES = [1, 1023, 1024, 1025, 4 * 1024 + 3]
COMPACT_KINDS = ['all', 'none', 'alternating', 'first', 'last', 'one_per_tile']
COMPACT_LARGE = 1024 * 1025 + 1                            # 1026 tiles: k_cp_scan's threads take 2 tiles each


def keep_mask(n, kind):
    m = np.zeros(n, bool)
    if kind == 'all':
        m[:] = True
    elif kind == 'alternating':
        m[::2] = True
    elif kind == 'first':
        m[0] = True
    elif kind == 'last':
        m[-1] = True
    elif kind == 'one_per_tile':
        t = np.arange(-(-n // CP_TILE))
        i = t * CP_TILE + (t * 389 + 1023) % CP_TILE       # tile 0: its last element
        m[np.minimum(i, n - 1)] = True
    elif kind == 'large':                                  # the first and the last tile, sparsely in between
        m[0:CP_TILE:2] = True
        m[CP_TILE + 5::4099] = True
        m[-1] = True
    else:
        assert kind == 'none'
    return m


def compact_cases():
    return [(n, k) for n in COMPACT_SIZES for k in COMPACT_KINDS] + [(COMPACT_LARGE, 'large')]


def mask_values(mask):
    """where_greater(values, 0.5) keeps exactly the mask"""
    return np.where(mask, F(1), F(0.5)).astype(np.float32)          # a dropped value EQUALS the threshold: strict >


def mask_boxes(mask, which):
    """boxes that clip_filter(0, IMAGE, 16) / range_filter(IMAGE) keep exactly where the mask is set"""
    keep = f32([100.0, 100.0, 200.0, 115.0])                         # an edge of exactly 16
    drop = f32([100.0, 100.0, 200.0, up(115.0, -1)]) if which == 'clip_filter' else f32([-1.0, 0.0, 10.0, 10.0])
    return np.where(mask[:, None], keep, drop).astype(np.float32)


WHERE_THRESHOLDS = [0.05, np.inf, -np.inf, np.nan, 0.0, -0.0]


def where_values():
    thr = F(0.05)
    v = [thr, up(thr, 1), up(thr, -1), np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 1.0, -1.0, 3.4e38, -3.4e38]
    return f32(v * 5)[:67]


# ---- gather_rows --------------------------------------------------------------------------------------------------------
GATHER_ROW_FLOATS = [1, 4, 324]
GATHER_STRIDE_CASE = (4100, 257)                           # more than GATHER_GRID * GATHER_BLOCK elements: a second pass
GATHER_SPARE = 8                                           # valid index entries and output rows kept beyond n


def gather_indices(n, rows, kind, seed=0):
    """n + GATHER_SPARE valid indices into `rows` rows (the spare ones are there for a count above n)"""
    t = n + GATHER_SPARE
    if kind == 'descending':
        return (rows - 1 - np.arange(t) % rows).astype(np.int64)
    if kind == 'repeated':
        return ((np.arange(t) // 3) * 5 % rows).astype(np.int64)
    return np.random.default_rng(35 + seed).integers(0, rows, t).astype(np.int64)


def gather_cases():
    """(rows of src, row_floats, n, index kind, index dtype, count or None)"""
    out = []
    for rf in GATHER_ROW_FLOATS:
        for dt in (np.int32, np.int64):
            out += [(50, rf, 37, 'random', dt, None), (50, rf, 37, 'repeated', dt, 0), (50, rf, 37, 'descending', dt, 20),
                    (50, rf, 37, 'random', dt, 37 + 3)]
    n, rf = GATHER_STRIDE_CASE
    out += [(300, rf, n, 'random', np.int32, None), (300, rf, n, 'descending', np.int64, n - 1), (300, rf, n, 'random', np.int64, n + 5)]
    return out


# ---- the fused stage ----------------------------------------------------------------------------------------------------
def fused_case():
    """-> (deltas, anchors, scores, the 16 rows): ~2000 anchors of a 600 x 800 image, 16 of them with a dw or dh >= 88.8 (the
    decoded box is x1 = -inf, x2 = NaN before the clip), six of those with the highest scores"""
    rng = np.random.default_rng(36)
    ys, xs = np.meshgrid(np.arange(8, 600, 24), np.arange(8, 800, 24), indexing='ij')
    c = np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.float32)
    c = np.repeat(c, 3, axis=0)[:2000]
    half = np.tile(f32([[16, 16], [32, 16], [16, 32]]), (len(c) // 3 + 1, 1))[:len(c)]
    anchors = np.concatenate([c - half, c + half - F(1)], axis=1)
    n = len(anchors)
    deltas = rng.normal(0, 0.2, (n, 4)).astype(np.float32)
    scores = rng.permutation(n).astype(np.float32) / F(n)           # distinct
    hot = rng.choice(n, 16, replace=False)
    big = f32([88.8, 89.0, 100.0, 1e30, 3e38, np.inf, 88.8, 95.0] * 2)
    deltas[hot[:8], 2] = big[:8]
    deltas[hot[8:], 3] = big[8:]
    deltas[hot[12:], 2] = big[12:]
    scores[hot[:6]] = F(2) + np.arange(6, dtype=np.float32)         # above every other score
    return deltas, anchors, scores, hot
