"""The data-parallel gradient exchange without a GPU: the bucket layout's properties, the sharpness of the order data the GPU
tests use (proved here on the CPU, as tests/order_data.py does for the other sums), parallel.GradientExchange and
parallel.broadcast_variables on three gloo ranks with CPU tensors against tests/grad_exchange_np.py by bytes, and the argument
and limit returns of the three new C-ABI entry points."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import grad_exchange_np as gnp

WORLD = 3


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- layout --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('world', [1, 2, 3, 8])
def test_layout_offsets_are_chunk_multiples_and_no_shard_splits_a_chunk(world):
    from tf_eager_object_detection_amd import ops
    numels = [None if i == gnp.CASE_ABSENT else n for i, n in enumerate(gnp.CASE_NUMELS)]
    tb = ops.BucketTables(numels, world)
    assert ops.OPT_CHUNK == gnp.CHUNK == 4096
    first, chunks, shard = gnp.layout(numels, world)
    assert (tb.first_chunk, tb.num_chunks, tb.shard_chunks) == (first, chunks, shard)
    want_chunks = sum(-(-n // 4096) for n in numels if n is not None)
    assert tb.num_chunks == want_chunks == 1 + 1 + 1 + 1 + 1 + 1 + 2 + 3
    assert tb.bucket_chunks == world * tb.shard_chunks >= tb.num_chunks and tb.bucket_chunks - tb.num_chunks < world
    assert tb.shard_numel == tb.shard_chunks * 4096 and tb.bucket_numel == tb.bucket_chunks * 4096     # no shard splits a chunk
    end = 0
    for i, n in enumerate(numels):
        if n is None:
            assert tb.offset(i) is None
            continue
        assert tb.offset(i) % ops.OPT_CHUNK == 0 and tb.offset(i) == end        # whole chunks, in list order, no gap
        end += -(-n // 4096) * 4096
    # the chunk table is the optimizer's, over the present tensors: table chunk c is bucket chunk c
    for c, (t, o) in enumerate(tb.chunk_list):
        assert numels[t] is not None and o % 4096 == 0 and o < numels[t] and c == tb.first_chunk[t] + o // 4096


def test_restatement_pack_unpack_and_padding():
    arrays = gnp.case_arrays(0)
    for world in (1, 3, 8):
        b = gnp.bucket_pack(arrays, world)
        first, chunks, shard = gnp.layout([None if a is None else a.size for a in arrays], world)
        assert b.size == world * shard * 4096
        used = np.zeros(b.size, bool)
        for a, f in zip(arrays, first):
            if a is not None:
                used[f * 4096:f * 4096 + a.size] = True
        assert not _bits(b[~used]).any()                                       # +0.0, not -0.0
        back = gnp.bucket_unpack(b, [None if a is None else a.size for a in arrays], world)
        for a, g in zip(arrays, back):
            assert (a is None and g is None) or np.array_equal(_bits(a), _bits(g))


# ---- the order data is sharp ---------------------------------------------------------------------------------------------------
def test_order_data_separates_the_ascending_sum_from_every_other_order():
    four = gnp.ORDER_SETS[4][0]
    assert [float(f(four)) for f in (gnp.sum_ascending, gnp.sum_reversed, gnp.sum_tree, gnp.sum_f64)] == \
        [16777216.0, 16777220.0, 16777218.0, 16777220.0]
    eight = gnp.ORDER_SETS[8][0]
    assert [float(f(eight)) for f in (gnp.sum_ascending, gnp.sum_reversed, gnp.sum_tree, gnp.sum_f64)] == [4.0, 6.0, 5.0, 6.0]
    for world in (4, 8):
        for terms in gnp.ORDER_SETS[world]:
            asc = gnp.sum_ascending(terms)
            assert asc != gnp.sum_reversed(terms) and asc != gnp.sum_tree(terms) and asc != gnp.sum_f64(terms)
    for world in (3, 5):                                   # (a three-term tree IS the ascending sum)
        for terms in gnp.ORDER_SETS[world]:
            assert gnp.sum_ascending(terms) != gnp.sum_reversed(terms) and gnp.sum_ascending(terms) != gnp.sum_f64(terms)
    for world in (3, 4, 5, 8):                             # the restatement takes the ascending order
        cols = gnp.order_columns(world)
        got = gnp.rank_mean(cols, average=False)
        for k in range(cols.shape[1]):
            assert got[k] == gnp.sum_ascending(list(cols[:, k]))


def test_division_data_separates_the_division_from_a_reciprocal_multiply():
    want = {3: [5.0, 7.0, 10.0], 5: [9.0, 13.0]}
    for world in (3, 5):
        w = np.float32(world)
        rec = np.float32(np.float32(1.0) / w)
        sums = [gnp.sum_ascending(t) for t in gnp.DIVISION_SETS[world]]
        assert [float(s) for s in sums] == want[world]
        for s in sums:
            assert np.float32(s / w) != np.float32(s * rec), (world, s)
        cols = gnp.order_columns(world)
        k0 = len(gnp.ORDER_SETS[world])
        got = gnp.rank_mean(cols)
        for k, s in enumerate(sums):
            assert got[k0 + k] == np.float32(s / w) and got[k0 + k] != np.float32(s * rec)
    # the tiled data of the GPU test carries the columns at every size that holds them
    for world in (3, 4, 5, 8):
        cols = gnp.order_columns(world)
        for n in (1, 4095, 4096, 4097):
            parts = gnp.rank_parts(world, n, 7)
            k = min(n, cols.shape[1])
            assert parts.shape == (world, n) and np.array_equal(parts[:, :k], cols[:, :k])
    assert gnp.order_columns(1).shape == (1, 0) and gnp.order_columns(2).shape == (2, 0)


# ---- three gloo ranks, CPU tensors -----------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _shapes():
    """a shape per tensor of the list (the largest one 2-D: the views take their variable's shape)"""
    return [(n,) for n in gnp.CASE_NUMELS[:-1]] + [(3, 2733)]


def _worker(rank, port, q):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=WORLD)
    try:
        from tf_eager_object_detection_amd import parallel
        lists = gnp.case_rank_arrays(WORLD)
        variables = [torch.zeros(s) for s in _shapes()]
        grads = [None if a is None else torch.from_numpy(a.copy()).reshape(s) for a, s in zip(lists[rank], _shapes())]
        scalars = torch.tensor([1.0 + rank, 2.0 ** 24 if rank == 0 else 1.0, 3.0, 4.0 + 3 * rank])
        ex = parallel.GradientExchange(variables)
        out, mean = ex.exchange(grads, scalars=scalars)
        res = dict(rank=rank, out=[None if o is None else o.numpy().reshape(-1).copy() for o in out], mean=mean.numpy().copy(),
                   shapes=[None if o is None else tuple(o.shape) for o in out])
        out2 = ex.exchange(grads)                                   # another present set (no scalars): a second layout
        res['out2'] = [None if o is None else o.numpy().reshape(-1).copy() for o in out2]
        again, _ = ex.exchange(grads, scalars=scalars)
        res['same_views'] = all(a is b for a, b in zip(out, again))
        res['sum'] = parallel.GradientExchange(variables, average=False).exchange(grads)[-1].numpy().reshape(-1).copy()
        # a rank whose None set differs: every rank raises
        bad = list(grads)
        if rank == 1:
            bad[2] = None
        try:
            parallel.GradientExchange(variables).exchange(bad)
            res['mismatch'] = 'no error'
        except ValueError as e:
            res['mismatch'] = 'ValueError: %s' % e
        with pytest.raises(TypeError):
            ex.exchange([None if g is None else g.half() for g in grads])
        # broadcast: rank 0's bytes everywhere
        rng = np.random.default_rng(50 + rank)
        params = [torch.from_numpy(rng.standard_normal(int(np.prod(s))).astype(np.float32)).reshape(s) for s in _shapes()]
        versions = [p._version for p in params]
        parallel.broadcast_variables(params)
        res['params'] = [p.numpy().reshape(-1).copy() for p in params]
        res['bumped'] = all(p._version > v for p, v in zip(params, versions))
        q.put(res)
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope='module')
def gloo_results():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, port, q)) for r in range(WORLD)]
    for p in procs:
        p.start()
    results = sorted((q.get(timeout=120) for _ in range(WORLD)), key=lambda r: r['rank'])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return results


def test_gloo_exchange_equals_the_restatement_on_every_rank(gloo_results):
    lists = gnp.case_rank_arrays(WORLD)
    rank_scalars = [np.float32([1.0 + r, 2.0 ** 24 if r == 0 else 1.0, 3.0, 4.0 + 3 * r]) for r in range(WORLD)]
    want, want_mean = gnp.exchange(lists, True, rank_scalars)
    want2, _ = gnp.exchange(lists, True)
    want_sum, _ = gnp.exchange(lists, False)
    assert float(want_mean[1]) == float(np.float32(np.float32(2.0 ** 24) / np.float32(3)))     # (2^24 + 1 + 1 in rank order)
    for res in gloo_results:
        assert res['shapes'] == [None if i == gnp.CASE_ABSENT else s for i, s in enumerate(_shapes())]
        for i, (g, w) in enumerate(zip(res['out'], want)):
            assert (g is None and w is None) or np.array_equal(_bits(g), _bits(w)), i
        for i, (g, w) in enumerate(zip(res['out2'], want2)):
            assert (g is None and w is None) or np.array_equal(_bits(g), _bits(w)), i
        assert np.array_equal(_bits(res['mean']), _bits(want_mean))
        assert np.array_equal(_bits(res['sum']), _bits(want_sum[-1]))
        assert res['same_views']
    for res in gloo_results[1:]:                                                 # identical across the ranks
        for a, b in zip(gloo_results[0]['out'], res['out']):
            assert (a is None and b is None) or np.array_equal(_bits(a), _bits(b))


def test_gloo_a_differing_none_set_raises_on_every_rank(gloo_results):
    for res in gloo_results:
        assert res['mismatch'].startswith('ValueError') and 'disagree' in res['mismatch'], res['mismatch']


def test_gloo_broadcast_leaves_rank_0_bytes_everywhere(gloo_results):
    rng = np.random.default_rng(50)
    want = [rng.standard_normal(int(np.prod(s))).astype(np.float32) for s in _shapes()]
    for res in gloo_results:
        assert res['bumped']
        for g, w in zip(res['params'], want):
            assert np.array_equal(_bits(g), _bits(w))


def test_single_process_returns_the_gradients_as_given():
    from tf_eager_object_detection_amd import parallel
    variables = [torch.zeros(5), torch.zeros(3)]
    grads = [torch.ones(5), None]
    ex = parallel.GradientExchange(variables)
    out = ex.exchange(grads)
    assert out[0] is grads[0] and out[1] is None
    sc = torch.tensor([1.0, 2.0])
    out, mean = ex.exchange(grads, scalars=sc)
    assert out[0] is grads[0] and mean is sc
    with pytest.raises(TypeError):
        ex.exchange([torch.ones(5).half(), None])
    with pytest.raises(ValueError):
        ex.exchange([torch.ones(4), None])
    with pytest.raises(TypeError):
        parallel.GradientExchange([torch.zeros(5).half()])
    with pytest.raises(TypeError):
        parallel.broadcast_variables([torch.zeros(5).half()])


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_abi_exports_argument_and_limit_returns():
    from tf_eager_object_detection_amd import _lib
    Lb = _lib.lib()
    assert Lb.odet_version() == 103
    for name in ('odet_bucket_pack_f32', 'odet_bucket_unpack_f32', 'odet_rank_mean_f32'):
        assert hasattr(Lb, name) and name in _lib.SIGNATURES
    assert _lib.RANK_MEAN_MAX_WORLD == 64
    P = 0x10000                                                      # pointer-valued integers nothing dereferences
    INVALID, LIMIT = -1, -4

    def pack(tensors=P, numels=P, T=2, chunks=P, K=2, bucket=P, BK=4):
        return Lb.odet_bucket_pack_f32(tensors, numels, T, chunks, K, bucket, BK, None), Lb.odet_last_error()

    def unpack(bucket=P, BK=4, tensors=P, numels=P, T=2, chunks=P, K=2):
        return Lb.odet_bucket_unpack_f32(bucket, BK, tensors, numels, T, chunks, K, None), Lb.odet_last_error()

    def mean(parts=P, world=2, n=8, average=1, out=P):
        return Lb.odet_rank_mean_f32(parts, world, n, average, out, None), Lb.odet_last_error()

    rows = []
    for label, f in (('pack', pack), ('unpack', unpack)):
        rows += [('%s: null tensors' % label, f(tensors=None), INVALID), ('%s: null numels' % label, f(numels=None), INVALID),
                 ('%s: null chunks' % label, f(chunks=None), INVALID), ('%s: null bucket' % label, f(bucket=None), INVALID),
                 ('%s: misaligned bucket' % label, f(bucket=P + 4), INVALID), ('%s: negative T' % label, f(T=-1), INVALID),
                 ('%s: negative K' % label, f(K=-1), INVALID), ('%s: negative bucket' % label, f(BK=-1), INVALID),
                 ('%s: table larger than the bucket' % label, f(K=5), INVALID),
                 ('%s: chunks without tensors' % label, f(T=0), INVALID),
                 ('%s: T over the limit' % label, f(T=_lib.OPT_MAX_TENSORS + 1), LIMIT),
                 ('%s: bucket over the limit' % label, f(BK=_lib.OPT_MAX_CHUNKS + 1), LIMIT)]
    rows += [('mean: null parts', mean(parts=None), INVALID), ('mean: null out', mean(out=None), INVALID),
             ('mean: world 0', mean(world=0), INVALID), ('mean: world -1', mean(world=-1), INVALID),
             ('mean: world 65', mean(world=65), LIMIT), ('mean: negative n', mean(n=-1), INVALID),
             ('mean: average 2', mean(average=2), INVALID), ('mean: misaligned parts', mean(parts=P + 2), INVALID),
             ('mean: n over the limit', mean(n=(_lib.OPT_MAX_CHUNKS * _lib.OPT_CHUNK) + 1), LIMIT)]
    for label, (rc, msg), want in rows:
        print('%s -> %d %r' % (label, rc, msg))
        assert rc == want, (label, rc, msg)
        assert msg.startswith(b'odet_') and b' failed: ' not in msg, msg   # (refused before any HIP call)
    # no-ops that launch nothing
    assert mean(parts=None, out=None, n=0)[0] == 0
    assert pack(tensors=None, numels=None, T=0, chunks=None, K=0, bucket=None, BK=0)[0] == 0
    assert unpack(tensors=None, numels=None, T=0, chunks=None, K=0, bucket=None, BK=0)[0] == 0
    assert unpack(K=0)[0] == 0


def test_python_front_refuses_cpu_tensors_and_bad_layouts():
    from tf_eager_object_detection_amd import _lib, ops
    with pytest.raises(_lib.OdetError, match='no CPU path'):
        ops.rank_mean(torch.zeros(2, 8))
    with pytest.raises(ValueError):
        ops.rank_mean(torch.zeros(8))
    with pytest.raises(ValueError):
        ops.rank_mean(torch.zeros(65, 8))
    tb = ops.BucketTables([4, None, 5], 2)
    with pytest.raises(ValueError):
        tb.check([torch.zeros(4), torch.zeros(1), torch.zeros(5)])           # present where the layout has none
    with pytest.raises(TypeError):
        tb.check([torch.zeros(4).half(), None, torch.zeros(5)])
    with pytest.raises(ValueError):
        tb.check([torch.zeros(4), None, torch.zeros(10)[::2]])               # not dense
    with pytest.raises(ValueError):
        ops.BucketTables([4], 0)
