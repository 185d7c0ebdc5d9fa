"""NumPy restatement of odet_bucket_accumulate_f32, of training.GradientAccumulator and of the data-parallel mean of means, bit for
bit (include/odet.h "gradient exchange"), and the data on which the image order and the division show.  Written from the header's
text alone: it shares no code with ops.py, training.py or parallel.py; the bucket layout is grad_exchange_np's.

Tensors are flat float32 arrays in MEMORY order; None marks an absent tensor."""
import numpy as np

import grad_exchange_np as gnp

CHUNK = gnp.CHUNK


def accumulate(bucket, arrays, first, divisor=1.0, bucket_chunks=None):
    """one call of odet_bucket_accumulate_f32 on a copy of `bucket` (None with first: a bucket of NaN, which a first call must
    overwrite everywhere).  s = g when first else bucket + g, ONE float32 add; then s / float32(divisor) unless divisor == 1."""
    numels = [None if a is None else a.size for a in arrays]
    first_chunk, chunks, _ = gnp.layout(numels, 1)
    total = chunks if bucket_chunks is None else int(bucket_chunks)
    assert total >= chunks
    d = np.float32(divisor)
    assert np.isfinite(d) and d > 0
    out = np.full(total * CHUNK, np.nan, np.float32) if bucket is None else np.asarray(bucket, np.float32).copy()
    assert out.size == total * CHUNK
    if first:
        out[:] = np.float32(0.0)                                   # tails, absent records, padding chunks: +0.0f
    for a, f in zip(arrays, first_chunk):
        if a is None or a.size == 0:
            continue
        g = np.asarray(a, np.float32).reshape(-1)
        lo = f * CHUNK
        s = g.copy() if first else (out[lo:lo + g.size] + g).astype(np.float32)
        if d != np.float32(1.0):
            s = (s / d).astype(np.float32)
        out[lo:lo + g.size] = s
    return out


def window_bucket(image_lists, average=True, bucket_chunks=None):
    """the bucket after the K calls of one window: image 0 first, one add per image in ascending order, float32(K) on the last"""
    K = len(image_lists)
    bucket = None
    for k, arrays in enumerate(image_lists):
        divisor = float(K) if (average and k == K - 1) else 1.0
        bucket = accumulate(bucket, arrays, k == 0, divisor, bucket_chunks)
    return bucket


def window(image_lists, average=True):
    """what GradientAccumulator.add returns on the K-th image: a flat array (or None) per variable.  K == 1: the gradients as
    given."""
    if len(image_lists) == 1:
        return [None if a is None else np.asarray(a, np.float32).reshape(-1).copy() for a in image_lists[0]]
    numels = [None if a is None else a.size for a in image_lists[0]]
    for arrays in image_lists[1:]:
        assert [None if a is None else a.size for a in arrays] == numels, 'the set of present gradients is fixed by the first image'
    return gnp.bucket_unpack(window_bucket(image_lists, average), numels, 1)


def mean_of_means(rank_image_lists, rank_image_scalars=None):
    """parallel.DataParallelTrainer with images_per_rank = K: rank_image_lists[r][k] is the gradient list of rank r's k-th image.
    Every rank forms its own image mean (window), then the exchange averages the ranks in ascending rank order: two roundings.
    The scalars (the four losses) travel as one more tensor of the list.  Returns (list, scalars or None)."""
    lists = []
    for r, images in enumerate(rank_image_lists):
        if rank_image_scalars is not None:
            images = [list(a) + [np.asarray(s, np.float32).reshape(-1)] for a, s in zip(images, rank_image_scalars[r])]
        lists.append(window(images, True))
    if rank_image_scalars is None:
        return gnp.exchange(lists, True)
    return gnp.exchange([l[:-1] for l in lists], True, [l[-1] for l in lists])


# ---- data on which the image order and the division show ------------------------------------------------------------------------
CANDIDATES = 4


def mixed(rng, shape):
    """float32 values of mixed magnitude (2^-4 .. 2^4 times a normal draw)"""
    return (rng.standard_normal(shape) * np.exp2(rng.integers(-4, 5, shape))).astype(np.float32)


def _order_shows(x):
    """x float32 [K, n] -> bool [n]: the sum in REVERSED image order has other bits than the ascending one"""
    return gnp.rank_mean(x, False).view(np.uint32) != gnp.rank_mean(x[::-1], False).view(np.uint32)


def _division_shows(x):
    """x float32 [K, n] -> bool [n]: s * float32(1 / K) differs from s / float32(K), s the ascending sum"""
    K = np.float32(x.shape[0])
    s = gnp.rank_mean(x, False)
    rec = np.float32(np.float32(1.0) / K)
    return (s / K).astype(np.float32).view(np.uint32) != (s * rec).astype(np.float32).view(np.uint32)


def image_columns(K, n, rng):
    """float32 [K, n]: per element the first of CANDIDATES random draws on which the image order shows (even elements) or the
    division shows (odd elements), the first draw where none does.  Random float32 sums show the order in about 3 of 10
    elements at K = 3 and the division in 2 of 10 at K = 5; the choice lifts both shares well above a quarter."""
    cand = mixed(rng, (CANDIDATES, K, n))
    pick = np.zeros(n, np.int64)
    if K >= 3 and n:
        even = (np.arange(n) % 2) == 0
        shows = np.stack([np.where(even, _order_shows(c), _division_shows(c)) for c in cand])     # [CANDIDATES, n]
        pick = np.argmax(shows, axis=0)                              # (the first True; 0 where there is none)
    return cand[pick, :, np.arange(n)].T.copy()


def image_lists(K, numels, seed, absent=()):
    """K gradient lists over `numels` (None at the absent places) of image_columns data"""
    rng = np.random.default_rng(seed)
    lists = [[] for _ in range(K)]
    for i, n in enumerate(numels):
        cols = None if (i in absent or n is None) else image_columns(K, n, rng)
        for k in range(K):
            lists[k].append(None if cols is None else cols[k].copy())
    return lists


def _flat(image_lists_):
    """[K, total] over the present tensors"""
    return np.stack([np.concatenate([a.reshape(-1) for a in arrays if a is not None]) for arrays in image_lists_])


def order_share(image_lists_):
    return float(np.mean(_order_shows(_flat(image_lists_))))


def division_share(image_lists_):
    return float(np.mean(_division_shows(_flat(image_lists_))))
