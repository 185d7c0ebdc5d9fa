"""The data-parallel gradient exchange on the GPU, by bytes against tests/grad_exchange_np.py: the bucket pack / unpack launches on
aligned and shifted views, odet_rank_mean_f32 on the data whose order shows (tests/test_grad_exchange_host.py proves it sharp),
parallel.GradientExchange on three ranks sharing cuda:0 (backend gloo: RCCL wants one device per rank) followed by two training
steps, the RCCL call path with one rank, and parallel.DataParallelTrainer end to end on two ranks.  The ranks are fresh
processes (spawn), never a re-exec of a process that touched the GPU; a card admits at most six processes, so no case has more
than three ranks."""
import os
import queue
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import grad_exchange_np as gnp

pytestmark = pytest.mark.gpu

GUARD = 123.0


def _bits(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _mem(t):
    """the tensor's elements in memory order (dense tensors)"""
    return torch.as_strided(t, (t.numel(),), (1,), t.storage_offset())


def _views(arrays, shift, fill=None):
    """one device view per array, `shift` elements past a 16-byte boundary, with 4 guard elements on each side"""
    bufs, views = [], []
    for a in arrays:
        if a is None:
            bufs.append(None)
            views.append(None)
            continue
        buf = torch.full((a.size + 16,), GUARD, dtype=torch.float32, device='cuda')
        v = buf[4 + shift:4 + shift + a.size]
        assert a.size == 0 or v.data_ptr() % 16 == 4 * shift
        if fill is None:
            v.copy_(torch.from_numpy(a))
        bufs.append(buf)
        views.append(v)
    return bufs, views


# ---- pack / unpack ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shift', [0, 1], ids=['aligned', 'shifted'])
@pytest.mark.parametrize('world', [1, 3, 8])
def test_pack_into_a_nan_bucket_equals_the_restatement(world, shift):
    from tf_eager_object_detection_amd import ops
    arrays = gnp.case_arrays(3)
    _, views = _views(arrays, shift)
    tb = ops.BucketTables([None if a is None else a.size for a in arrays], world, 'cuda:0')
    bucket = torch.full((tb.bucket_numel,), float('nan'), dtype=torch.float32, device='cuda:0')
    assert ops.bucket_pack(tb, views, bucket) is bucket
    want = gnp.bucket_pack(arrays, world)
    assert want.size == bucket.numel() and np.array_equal(_bits(bucket), _bits(want))      # the +0.0 padding included
    # the same tensors again: the pointer column is not uploaded a second time
    assert tb.set_pointers(views) is False


@pytest.mark.parametrize('shift', [0, 1], ids=['aligned', 'shifted'])
def test_unpack_is_the_exact_inverse_and_leaves_the_guards(shift):
    from tf_eager_object_detection_amd import ops
    arrays = gnp.case_arrays(4)
    world = 3
    tb = ops.BucketTables([None if a is None else a.size for a in arrays], world, 'cuda:0')
    rng = np.random.default_rng(9)
    host = rng.standard_normal(tb.bucket_numel).astype(np.float32)          # (padding and tails hold data too: never unpacked)
    want = gnp.bucket_unpack(host, [None if a is None else a.size for a in arrays], world)
    bucket = torch.from_numpy(host).cuda()
    bufs, views = _views(arrays, shift, fill=GUARD)
    ops.bucket_unpack(tb, bucket, views)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(bucket), _bits(host))
    for a, buf, v, w in zip(arrays, bufs, views, want):
        if a is None:
            continue
        assert np.array_equal(_bits(v), _bits(w))
        b = buf.cpu().numpy()
        lo = 4 + shift
        assert (b[:lo] == GUARD).all() and (b[lo + a.size:] == GUARD).all()
    # pack then unpack: the round trip
    _, src = _views(arrays, shift)
    round_trip = ops.bucket_pack(tb, src)
    bufs, dst = _views(arrays, 1 - shift, fill=GUARD)
    ops.bucket_unpack(tb, round_trip, dst)
    for a, v in zip(arrays, dst):
        assert a is None or np.array_equal(_bits(v), _bits(a))


def test_pack_refuses_what_the_layout_does_not_hold():
    from tf_eager_object_detection_amd import ops
    tb = ops.BucketTables([5, None], 2, 'cuda:0')
    with pytest.raises(TypeError):
        ops.bucket_pack(tb, [torch.zeros(5, device='cuda').half(), None])
    with pytest.raises(ValueError):
        ops.bucket_pack(tb, [torch.zeros(5, device='cuda'), torch.zeros(1, device='cuda')])
    with pytest.raises(ValueError):
        ops.bucket_pack(tb, [torch.zeros(5, device='cuda'), None], torch.zeros(17, device='cuda'))


# ---- rank_mean -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 4095, 4096, 4097])
@pytest.mark.parametrize('world', [1, 2, 3, 4, 5, 8])
def test_rank_mean_adds_in_ascending_rank_and_divides_once(world, n):
    from tf_eager_object_detection_amd import ops
    parts = gnp.rank_parts(world, n, 100 * world + n)
    if world == 1:
        parts[0, 0] = -0.0
        if n > 1:
            parts[0, 1], parts[0, n - 1] = np.inf, -np.inf
    dev = torch.from_numpy(parts).cuda()
    for average in (True, False):
        got = ops.rank_mean(dev, average=average)
        want = gnp.rank_mean(parts, average)
        assert got.shape == (n,) and np.array_equal(_bits(got), _bits(want)), (world, n, average)
        if world == 1:
            assert np.array_equal(_bits(got), _bits(parts[0]))             # the input's bits: -0.0 and inf unchanged
    out = torch.full((n + 8,), GUARD, dtype=torch.float32, device='cuda')        # an output one element past a 16-byte boundary
    ops.rank_mean(dev, out=out[1:1 + n])
    o = out.cpu().numpy()
    assert (o[:1] == GUARD).all() and (o[1 + n:] == GUARD).all() and np.array_equal(_bits(o[1:1 + n]), _bits(gnp.rank_mean(parts)))


def test_rank_mean_world_64_and_the_limit():
    from tf_eager_object_detection_amd import ops
    parts = gnp.rank_parts(64, 2 * 4096 + 3, 5)
    got = ops.rank_mean(torch.from_numpy(parts).cuda())
    assert np.array_equal(_bits(got), _bits(gnp.rank_mean(parts)))
    with pytest.raises(ValueError):
        ops.rank_mean(torch.zeros(65, 4, device='cuda'))


# ---- ranks on one card -----------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _spawn(target, world, *args, timeout=600):
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port, q) + args) for r in range(world)]
    for p in procs:
        p.start()
    results, waited = [], 0
    try:
        while len(results) < world:
            try:
                results.append(q.get(timeout=2))
            except queue.Empty:                              # (a rank that died ends the test at once, not at the time limit)
                waited += 2
                dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
                assert not dead and waited < timeout, 'rank exit codes %s after %d s' % ([p.exitcode for p in procs], waited)
        for p in procs:
            p.join(timeout=120)
            assert p.exitcode == 0
    finally:
        for p in procs:                                      # (a rank left waiting for one that died)
            if p.is_alive():
                p.terminate()
                p.join(timeout=30)
    return sorted(results, key=lambda r: r['rank'])


def _init(rank, world, port, backend='gloo'):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    import torch.distributed as dist
    torch.cuda.set_device(0)
    if backend == 'nccl':
        os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0')
        dist.init_process_group('nccl', rank=rank, world_size=world, device_id=torch.device('cuda', 0))
    else:
        dist.init_process_group('gloo', rank=rank, world_size=world)
    return dist


STEPS = 2
LR, MU = 0.01, 0.9


def _step_lists(world, step):
    """every rank's gradient list of training step `step` (the order columns in the largest tensor)"""
    lists = gnp.case_rank_arrays(world)
    if step:
        rng = np.random.default_rng(500 + step)
        for r in range(world):
            for a in lists[r]:
                if a is not None:
                    a *= np.float32(rng.uniform(0.5, 2.0))
    return lists


def _initial_variables():
    rng = np.random.default_rng(77)
    return [rng.normal(0, 0.05, n).astype(np.float32) for n in gnp.CASE_NUMELS]


def _train(named, opt, gradients):
    from tf_eager_object_detection_amd import training
    training.train_step(named, gradients, opt, learning_rate_bias_double=True, weight_decays={'v%d.weight' % i: 1e-4 for i in (7, 8)})


def _names():
    return ['v%d.%s' % (i, 'bias' if i % 3 == 0 else 'weight') for i in range(len(gnp.CASE_NUMELS))]


def _three_ranks(rank, world, port, q):
    dist = _init(rank, world, port)
    try:
        from tf_eager_object_detection_amd import ops, parallel, training
        variables = [torch.from_numpy(a).cuda() for a in _initial_variables()]
        named = list(zip(_names(), variables))
        ex = parallel.GradientExchange(variables)
        opt = training.MomentumOptimizer(LR, MU)
        uploads = []
        real = ops.OptimizerTables.set_gradients
        ops.OptimizerTables.set_gradients = lambda self, p: uploads.append(real(self, p)) or uploads[-1]
        res = dict(rank=rank, exchanged=[], pointers=[])
        for step in range(STEPS):
            grads = [None if a is None else torch.from_numpy(a).cuda() for a in _step_lists(world, step)[rank]]
            out = ex.exchange(grads)
            res['exchanged'].append([None if o is None else o.cpu().numpy().copy() for o in out])
            res['pointers'].append([None if o is None else o.data_ptr() for o in out])
            _train(named, opt, out)
        torch.cuda.synchronize()
        ops.OptimizerTables.set_gradients = real
        res['uploads'] = uploads
        res['variables'] = [v.cpu().numpy().copy() for v in variables]
        q.put(res)
    finally:
        dist.destroy_process_group()


def test_three_ranks_exchange_then_train_identically():
    from tf_eager_object_detection_amd import training
    world = 3
    results = _spawn(_three_ranks, world)
    # the single process fed the restatement's mean gradients
    variables = [torch.from_numpy(a).cuda() for a in _initial_variables()]
    named = list(zip(_names(), variables))
    opt = training.MomentumOptimizer(LR, MU)
    wants = []
    for step in range(STEPS):
        want, _ = gnp.exchange(_step_lists(world, step))
        wants.append(want)
        _train(named, opt, [None if w is None else torch.from_numpy(w).cuda() for w in want])
    assert wants[0][-1][0] == np.float32(np.float32(2.0 ** 24) / np.float32(3))         # (2^24 + 1 + 1 in rank order, / 3)
    for res in results:
        for step in range(STEPS):
            for i, (g, w) in enumerate(zip(res['exchanged'][step], wants[step])):
                assert (g is None and w is None) or np.array_equal(_bits(g), _bits(w)), (res['rank'], step, i)
        assert res['pointers'][0] == res['pointers'][1]                                   # the same views every step
        assert res['uploads'] == [True, False]                                            # the pointers did not move
        for i, (g, v) in enumerate(zip(res['variables'], variables)):
            assert np.array_equal(_bits(g), _bits(v)), (res['rank'], i)
    for res in results[1:]:
        for a, b in zip(results[0]['variables'], res['variables']):
            assert np.array_equal(_bits(a), _bits(b))
    # the step moved what had a gradient and left the rest alone
    for i, (v, a) in enumerate(zip(variables, _initial_variables())):
        assert np.array_equal(_bits(v), _bits(a)) == (i == gnp.CASE_ABSENT or a.size == 0), i


def _rccl_rank(rank, world, port, q):
    """one rank, backend "nccl" (= RCCL): the two collectives of the exchange, forced for a world of one"""
    dist = _init(rank, world, port, 'nccl')
    try:
        from tf_eager_object_detection_amd import parallel
        arrays = gnp.case_arrays(6)
        arrays[1][0] = -0.0
        variables = [torch.zeros(n, device='cuda') for n in gnp.CASE_NUMELS]
        grads = [None if a is None else torch.from_numpy(a).cuda() for a in arrays]
        calls = []
        real_a2a, real_ag = dist.all_to_all_single, dist.all_gather_into_tensor
        dist.all_to_all_single = lambda out, inp, **kw: calls.append(('all_to_all_single', tuple(out.shape), tuple(inp.shape))) or real_a2a(out, inp, **kw)
        dist.all_gather_into_tensor = lambda out, inp, **kw: calls.append(('all_gather_into_tensor', tuple(out.shape), tuple(inp.shape))) or real_ag(out, inp, **kw)
        ex = parallel.GradientExchange(variables, force_collective=True)
        exchanges = 2
        for _ in range(exchanges):
            out = ex.exchange(grads)
        torch.cuda.synchronize()
        dist.all_to_all_single, dist.all_gather_into_tensor = real_a2a, real_ag
        same = all((o is None and a is None) or np.array_equal(_bits(o), _bits(a)) for o, a in zip(out, arrays))
        plain = parallel.GradientExchange(variables).exchange(grads)
        q.put(dict(rank=rank, backend=dist.get_backend(), world=dist.get_world_size(), calls=calls, same=same, exchanges=exchanges,
                   as_given=all(a is b for a, b in zip(plain, grads))))
    finally:
        dist.destroy_process_group()


def test_rccl_call_path_with_one_rank():
    """backend "nccl", world 1, force_collective: exactly one all_to_all_single and one all_gather_into_tensor per exchange, over
    the whole bucket; the result has the input's bits.  Without force_collective the gradients come back as given."""
    got = _spawn(_rccl_rank, 1, timeout=300)[0]
    _, chunks, shard = gnp.layout([None if i == gnp.CASE_ABSENT else n for i, n in enumerate(gnp.CASE_NUMELS)], 1)
    n = chunks * gnp.CHUNK
    assert shard == chunks == 11
    assert got['backend'] == 'nccl' and got['world'] == 1
    assert got['calls'] == [('all_to_all_single', (n,), (n,)), ('all_gather_into_tensor', (n,), (n,))] * got['exchanges']
    assert got['same'] and got['as_given']


# ---- end to end: two ranks, one image each -----------------------------------------------------------------------------------------
IMAGE = (256, 352)
MODEL = dict(depth=50, training_targets='hip', training_losses='hip', train_neck=True, train_rpn_head=True, train_roi_head=True,
             roi_training_total_num_samples=32, roi_training_max_pos_samples=8)
WD = 1e-4


def _model(seed):
    from tf_eager_object_detection_amd.model.base_fpn_model import ResnetV1Fpn
    torch.manual_seed(seed)
    m = ResnetV1Fpn(**MODEL)
    with torch.no_grad():                                   # (spreads the fresh RpnHead's proposals over sizes and pyramid levels)
        b = m.dense.rpn_bbox.bias
        b.add_(torch.linspace(0.0, 1.6, b.numel(), device=b.device, dtype=b.dtype))
    return m


def _image(k):
    rng = np.random.default_rng(20 + k)
    return (rng.uniform(0, 255, (1,) + IMAGE + (3,)) - 110).astype(np.float32)


def _set_image_id(m, k):
    m._anchor_target._next_image_id = k
    m._proposal_target._next_image_id = k
    if hasattr(m, '_next_dropout_image_id'):
        m._next_dropout_image_id = k


def _trained(m):
    return [(n, p) for n, p in m.dense.named_parameters() if not n.startswith(('conv', 'bn'))]


def _e2e_rank(rank, world, port, q, boxes):
    dist = _init(rank, world, port)
    try:
        from tf_eager_object_detection_amd import parallel, training
        m = _model(1 if rank == 0 else 2)                    # rank 1 starts from other weights: the broadcast has to fix that
        first = _mem(_trained(m)[0][1].detach()).cpu().numpy().copy()
        trainer = parallel.DataParallelTrainer(m, training.MomentumOptimizer(LR, MU), learning_rate_bias_double=True, weight_decay=WD)
        inputs = (torch.from_numpy(_image(rank)).cuda(), torch.from_numpy(boxes[rank]).cuda(), torch.tensor([3, 7, 12], device='cuda'))
        losses = trainer.step(inputs)
        torch.cuda.synchronize()
        named = training.model_variables(m.dense)
        q.put(dict(rank=rank, first=first, losses=[float(x) for x in losses],
                   loss_bits=[int(_bits(x.reshape(1))[0]) for x in losses],
                   variables={n: _mem(p.detach()).cpu().numpy().copy() for n, p in _trained(m)},
                   no_grad_left=all(p.grad is None for _, p in named), step_index=trainer.step_index))
    finally:
        dist.destroy_process_group()


def test_data_parallel_trainer_two_ranks_equal_the_single_process_restatement():
    from tf_eager_object_detection_amd import training
    m = _model(1)
    trained = _trained(m)
    assert len(trained) == 28
    # ground truth from the model's own proposals (test_block_grad_gpu.test_caller_model_trains_its_extractor), per image
    boxes, inputs = [], []
    for k in range(2):
        img = torch.from_numpy(_image(k)).cuda()
        with torch.no_grad():
            p_list = m._neck(m._extractor(img, training=True), training=True)
            scores, deltas = m._get_fpn_head_results(p_list)
            rois = m._rpn_proposal((deltas, m._get_anchors(list(IMAGE)), m._fg_scores(scores), list(IMAGE)), training=True)
        big = rois[((rois[:, 2] - rois[:, 0]) >= 24) & ((rois[:, 3] - rois[:, 1]) >= 24)]
        assert big.shape[0] >= 3, 'the random model proposes fewer than 3 boxes of 24 pixels'
        gt = big[[0, big.shape[0] // 3, 2 * big.shape[0] // 3]].clone()
        boxes.append(gt.cpu().numpy().copy())
        inputs.append((img, gt, torch.tensor([3, 7, 12], device='cuda')))
    initial = {n: _mem(p.detach()).cpu().numpy().copy() for n, p in trained}
    results = _spawn(_e2e_rank, 2, boxes)

    # the single-process restatement: the two images one after the other with image ids 0 and 1, on the same weights
    named = training.model_variables(m.dense)
    rank_grads, rank_losses = [], []
    for k in range(2):
        _set_image_id(m, k)
        losses = m(inputs[k], True)
        sum(losses).backward()
        rank_grads.append([None if p.grad is None else _mem(p.grad).cpu().numpy().copy() for _, p in named])
        rank_losses.append(np.float32([float(x.detach()) for x in losses]))
        for _, p in named:
            p.grad = None
    assert [g is not None for g in rank_grads[0]] == [g is not None for g in rank_grads[1]]
    assert sum(g is not None for g in rank_grads[0]) == 28
    mean, mean_losses = gnp.exchange(rank_grads, True, rank_losses)
    gradients = []
    for (n, p), g in zip(named, mean):
        if g is None:
            gradients.append(None)
            continue
        t = torch.empty_like(p)                              # (the variable's strides: the bucket holds memory order)
        assert t.stride() == p.stride()
        _mem(t).copy_(torch.from_numpy(g))
        gradients.append(t)
    training.train_step(named, gradients, training.MomentumOptimizer(LR, MU), learning_rate_bias_double=True,
                        weight_decays=training.l2_variables(m.dense, WD))
    torch.cuda.synchronize()

    assert not np.array_equal(_bits(results[1]['first']), _bits(results[0]['first']))     # rank 1 did start elsewhere
    assert np.array_equal(_bits(results[0]['first']), _bits(initial[trained[0][0]]))
    for res in results:
        assert res['no_grad_left'] and res['step_index'] == 1
        assert sorted(res['variables']) == sorted(n for n, _ in trained)
        for n, p in trained:
            got = res['variables'][n]
            assert np.array_equal(_bits(got), _bits(_mem(p.detach()))), (res['rank'], n)
            assert not np.array_equal(_bits(got), _bits(initial[n])), n                     # the step moved it
        assert res['loss_bits'] == [int(b) for b in _bits(mean_losses)], (res['losses'], mean_losses)
    for n, _ in trained:
        assert np.array_equal(_bits(results[0]['variables'][n]), _bits(results[1]['variables'][n])), n
