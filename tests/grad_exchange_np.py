"""NumPy restatement of csrc/grad_exchange.hip and of parallel.GradientExchange, bit for bit (include/odet.h "gradient exchange"),
and the data on which the order of the rank sum shows.  Written from the header's text alone: it shares no code with ops.py.

Tensors are flat float32 arrays in MEMORY order; None marks an absent tensor."""
import numpy as np

CHUNK = 4096


def layout(numels, world):
    """numels (None = absent) -> (first chunk per tensor or None, table chunks, shard chunks): a present tensor takes
    ceil(numel / CHUNK) whole chunks in list order; the bucket is world * shard_chunks chunks"""
    first, c = [], 0
    for n in numels:
        if n is None:
            first.append(None)
            continue
        first.append(c)
        c += -(-int(n) // CHUNK)
    return first, c, -(-c // int(world))


def bucket_pack(arrays, world=1):
    """the bucket of a tensor list: +0.0 in every chunk tail and in the padding chunks"""
    first, _, shard = layout([None if a is None else a.size for a in arrays], world)
    bucket = np.zeros(world * shard * CHUNK, np.float32)
    for a, f in zip(arrays, first):
        if a is not None:
            bucket[f * CHUNK:f * CHUNK + a.size] = np.asarray(a, np.float32).reshape(-1)
    return bucket


def bucket_unpack(bucket, numels, world=1):
    first, _, shard = layout(numels, world)
    assert bucket.size == world * shard * CHUNK
    return [None if n is None else bucket[f * CHUNK:f * CHUNK + n].copy() for n, f in zip(numels, first)]


def rank_mean(parts, average=True):
    """parts float32 [world, n]: one float32 add per rank in ascending rank, then ONE float32 division by float32(world)"""
    parts = np.asarray(parts, np.float32)
    s = parts[0].copy()
    for r in range(1, parts.shape[0]):
        s = (s + parts[r]).astype(np.float32)
    if average:
        s = (s / np.float32(parts.shape[0])).astype(np.float32)
    return s


def exchange(rank_lists, average=True, rank_scalars=None):
    """What every rank holds after GradientExchange.exchange: rank_lists[r] is rank r's gradient list (the same None set on every
    rank), rank_scalars[r] its optional scalars.  Returns (list of flat arrays or None, scalars or None)."""
    world = len(rank_lists)
    buckets = []
    for r in range(world):
        arrays = list(rank_lists[r]) + ([np.asarray(rank_scalars[r], np.float32).reshape(-1)] if rank_scalars is not None else [])
        buckets.append(bucket_pack(arrays, world))
    numels = [None if a is None else a.size for a in arrays]
    shard = buckets[0].size // world
    # rank r reduces shard r of every rank; the all-gather concatenates the shards in rank order
    out = np.concatenate([rank_mean(np.stack([b[r * shard:(r + 1) * shard] for b in buckets]), average) for r in range(world)])
    got = bucket_unpack(out, numels, world)
    return (got[:len(rank_lists[0])], got[-1]) if rank_scalars is not None else (got, None)


# ---- data on which the order shows ------------------------------------------------------------------------------------------
T24 = float(2 ** 24)
ORDER_SETS = {3: [[T24, 1, 1]],
              4: [[T24, 1, 1, 1]],                                   # ascending 16777216, reversed 16777220, tree 16777218, f64 16777220
              5: [[T24, 1, 1, 1, 1]],
              8: [[1, T24, 1, -T24, 1, 1, 1, 1]]}                    # ascending 4, reversed 6, tree 5, f64 6
# sums whose division by world differs from the multiplication by float32(1 / world)
DIVISION_SETS = {3: [[1, 2, 2], [3, 2, 2], [4, 3, 3]],               # s = 5, 7, 10
                 5: [[1, 2, 2, 2, 2], [3, 2, 3, 2, 3]]}              # s = 9, 13


def order_columns(world):
    """float32 [world, k]: the rank terms of k elements on which a wrong order or a reciprocal multiply changes bits (k = 0 for
    world 1 and 2, where one correctly rounded add has no order)"""
    cols = ORDER_SETS.get(world, []) + DIVISION_SETS.get(world, [])
    return np.asarray(cols, np.float32).reshape(len(cols), world).T.copy()


def sum_ascending(terms):
    s = np.float32(terms[0])
    for t in terms[1:]:
        s = np.float32(s + np.float32(t))
    return s


def sum_reversed(terms):
    return sum_ascending(list(terms)[::-1])


def sum_tree(terms):
    v = [np.float32(t) for t in terms]
    while len(v) > 1:
        v = [np.float32(v[i] + v[i + 1]) if i + 1 < len(v) else v[i] for i in range(0, len(v), 2)]
    return v[0]


def sum_f64(terms):
    return np.float32(np.sum(np.asarray(terms, np.float64)))


def rank_parts(world, n, seed):
    """float32 [world, n]: the order columns first (as many as fit), random data of mixed magnitude after them"""
    rng = np.random.default_rng(seed)
    parts = (rng.standard_normal((world, n)) * np.exp2(rng.integers(-12, 12, (world, n)))).astype(np.float32)
    cols = order_columns(world)
    k = min(n, cols.shape[1])
    parts[:, :k] = cols[:, :k]
    return parts


# ---- the tensor list of the tests: every chunk-boundary case, an empty tensor, an absent one in the middle ------------------
CASE_NUMELS = [0, 1, 3, 4, 6, 5, 4095, 4096, 4097, 2 * 4096 + 7]
CASE_ABSENT = 4                                      # the gradient of this variable is None


def case_arrays(seed, absent=(CASE_ABSENT,)):
    """the list's flat float32 arrays for `seed` (a rank): random data of mixed magnitude, None at the absent places"""
    rng = np.random.default_rng(1000 + seed)
    out = []
    for i, n in enumerate(CASE_NUMELS):
        a = (rng.standard_normal(n) * np.exp2(rng.integers(-12, 12, n))).astype(np.float32)
        out.append(None if i in absent else a)
    return out


def case_rank_arrays(world, absent=(CASE_ABSENT,)):
    """every rank's list, with the order columns of `world` written over the first elements of the largest tensor"""
    lists = [case_arrays(r, absent) for r in range(world)]
    cols = order_columns(world)
    for r in range(world):
        lists[r][-1][:cols.shape[1]] = cols[r]
        lists[r][6][4090:4090 + min(5, cols.shape[1])] = cols[r][:5]     # (across a 16-byte group and the chunk's tail)
    return lists
