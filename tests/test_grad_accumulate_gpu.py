"""The K-image training step on the GPU, by bytes against tests/grad_accumulate_np.py: odet_bucket_accumulate_f32 on aligned and
shifted tensors (what a first call and a later call write, and what they leave), one captured window replayed on new gradients,
training.Trainer end to end against a hand loop, the exact resume from a checkpoint taken inside an open window, and
parallel.DataParallelTrainer with two images per rank on two ranks sharing cuda:0 (backend gloo).  The ranks are fresh processes
(spawn), never a re-exec of a process that touched the GPU.  The data's sharpness (image order, division) is proved on the CPU by
tests/test_grad_accumulate_host.py."""
import os
import queue
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import grad_accumulate_np as anp

pytestmark = pytest.mark.gpu

NUMELS = [0, 1, 3, 4095, 4096, 4097, 2 * 4096 + 5, None]
CHUNK = 4096
MARK = 77.0


def _bits(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _mem(t):
    """the tensor's elements in memory order (dense tensors)"""
    return torch.as_strided(t, (t.numel(),), (1,), t.storage_offset())


def _views(arrays, shift):
    """one device view per array, `shift` elements past a 16-byte boundary"""
    views = []
    for a in arrays:
        if a is None:
            views.append(None)
            continue
        buf = torch.zeros(a.size + 16, dtype=torch.float32, device='cuda')
        v = buf[4 + shift:4 + shift + a.size]
        assert a.size == 0 or v.data_ptr() % 16 == 4 * shift
        v.copy_(torch.from_numpy(a))
        views.append(v)
    return views


# ---- the kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shift', [0, 1], ids=['aligned', 'shifted'])
@pytest.mark.parametrize('K', [1, 2, 3, 5])
def test_accumulate_equals_the_restatement_and_writes_nothing_else(K, shift):
    from tf_eager_object_detection_amd import ops
    lists = anp.image_lists(K, NUMELS, 40 + K)
    tb = ops.BucketTables(NUMELS, 2, 'cuda:0')                 # (9 table chunks in a bucket of 10: one padding chunk)
    assert (tb.num_chunks, tb.bucket_chunks) == (9, 10)
    n = tb.bucket_numel
    whole = torch.full((n + 2 * CHUNK,), float('nan'), dtype=torch.float32, device='cuda:0')      # NaN bucket between NaN guards
    bucket = whole[CHUNK:CHUNK + n]
    used = np.zeros(n, bool)
    for i, m in enumerate(NUMELS):
        if m:
            used[tb.offset(i):tb.offset(i) + m] = True
    want = None
    for k in range(K):
        divisor = float(K) if k == K - 1 else 1.0
        assert ops.bucket_accumulate(tb, _views(lists[k], shift), bucket, k == 0, divisor) is bucket
        want = anp.accumulate(want, lists[k], k == 0, divisor, bucket_chunks=10)
        got = bucket.cpu().numpy()
        if k == 0:
            # a first call writes every element: +0.0f in the tails, the absent record's place and the padding chunk
            assert np.array_equal(_bits(got), _bits(want)) and not _bits(got[~used]).any()
            bucket[torch.from_numpy(~used).cuda()] = MARK
        else:
            # a later call writes the present tensors' elements and nothing else
            assert np.array_equal(_bits(got[used]), _bits(want[used])), k
            assert (got[~used] == MARK).all(), k
    assert np.array_equal(_bits(bucket.cpu().numpy()[used]), _bits(anp.window_bucket(lists, True, 10)[used]))
    guards = whole.cpu().numpy()
    assert np.isnan(guards[:CHUNK]).all() and np.isnan(guards[CHUNK + n:]).all()


def test_a_first_call_may_divide_and_a_sum_keeps_its_bits():
    from tf_eager_object_detection_amd import ops
    lists = anp.image_lists(3, NUMELS, 5)
    tb = ops.BucketTables(NUMELS, 1, 'cuda:0')
    bucket = torch.full((tb.bucket_numel,), float('nan'), dtype=torch.float32, device='cuda:0')
    ops.bucket_accumulate(tb, _views(lists[0], 0), bucket, True, 3.0)
    assert np.array_equal(_bits(bucket), _bits(anp.accumulate(None, lists[0], True, 3.0)))
    want = None
    for k in range(3):
        ops.bucket_accumulate(tb, _views(lists[k], k % 2), bucket, k == 0)
        want = anp.accumulate(want, lists[k], k == 0)
    assert np.array_equal(_bits(bucket), _bits(want)) and np.array_equal(_bits(want), _bits(anp.window_bucket(lists, False)))
    # signed zeros: the first image's bits, then (-0) + (+0) = +0
    z = ops.BucketTables([2], 1, 'cuda:0')
    b = z.new_bucket()
    ops.bucket_accumulate(z, [torch.tensor([-0.0, -0.0], device='cuda')], b, True)
    assert list(_bits(b[:2])) == [0x80000000, 0x80000000]
    ops.bucket_accumulate(z, [torch.tensor([0.0, -0.0], device='cuda')], b, False)
    assert list(_bits(b[:2])) == [0x00000000, 0x80000000]


# ---- graph capture ---------------------------------------------------------------------------------------------------------------
def test_a_captured_window_replays_on_new_gradients():
    from tf_eager_object_detection_amd import training
    K = 3
    shapes = [(0,), (1,), (3,), (4095,), (64, 64), (4097,), (7, 1171), (5,)]
    variables = [torch.zeros(s, device='cuda') for s in shapes]
    grads = [None if n is None else torch.zeros(s, device='cuda') for n, s in zip(NUMELS, shapes)]       # the tensors the graph reads
    stage = [[None if g is None else torch.zeros_like(g) for g in grads] for _ in range(K)]

    def write(lists):
        for k in range(K):
            for s, a in zip(stage[k], lists[k]):
                if s is not None:
                    _mem(s).copy_(torch.from_numpy(a))

    def window(acc):
        out = None
        for k in range(K):
            for g, s in zip(grads, stage[k]):
                if g is not None:
                    g.copy_(s)
            out = acc.add(grads)
        return out

    acc = training.GradientAccumulator(variables, K)
    first = anp.image_lists(K, NUMELS, 61)
    write(first)
    views = window(acc)                                        # eager: binds the pointer column the capture will meet
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = window(acc)
    assert all(a is b for a, b in zip(views, captured))
    second = anp.image_lists(K, NUMELS, 62)
    write(second)
    graph.replay()
    torch.cuda.synchronize()
    got = [None if v is None else _mem(v).cpu().numpy().copy() for v in views]
    eager = window(training.GradientAccumulator(variables, K))
    for i, (g, e, w) in enumerate(zip(got, eager, anp.window(second, True))):
        assert (g is None) == (w is None), i
        if g is not None:
            assert np.array_equal(_bits(g), _bits(w)) and np.array_equal(_bits(g), _bits(_mem(e))), i
    assert not np.array_equal(_bits(got[-2]), _bits(anp.window(first, True)[-2]))


# ---- the trainer, end to end -------------------------------------------------------------------------------------------------------
IMAGE = (256, 352)
MODEL = dict(depth=50, training_targets='hip', training_losses='hip', train_neck=True, train_rpn_head=True, train_roi_head=True,
             roi_training_total_num_samples=32, roi_training_max_pos_samples=8)
WD = 1e-4
LR, MU = 0.01, 0.9
IMAGES = 6


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


def _inputs(k, boxes):
    return (torch.from_numpy(_image(k)).cuda(), torch.from_numpy(boxes[k]).cuda(), torch.tensor([3, 7, 12], device='cuda'))


def _set_image_id(m, k):
    m._anchor_target._next_image_id = k
    m._proposal_target._next_image_id = k
    if hasattr(m, '_next_dropout_image_id'):
        m._next_dropout_image_id = k


def _trained(m):
    return [(n, p) for n, p in m.dense.named_parameters() if not n.startswith(('conv', 'bn'))]


@pytest.fixture(scope='module')
def boxes():
    """ground truth from the model's own proposals (tests/test_grad_exchange_gpu.py), per image, on the weights of seed 1"""
    m = _model(1)
    assert len(_trained(m)) == 28
    out = []
    for k in range(IMAGES):
        img = torch.from_numpy(_image(k)).cuda()
        with torch.no_grad():
            p_list = m._neck(m._extractor(img, training=True), training=True)
            scores, deltas = m._get_fpn_head_results(p_list)
            rois = m._rpn_proposal((deltas, m._get_anchors(list(IMAGE)), m._fg_scores(scores), list(IMAGE)), training=True)
        big = rois[((rois[:, 2] - rois[:, 0]) >= 24) & ((rois[:, 3] - rois[:, 1]) >= 24)]
        assert big.shape[0] >= 3, 'the random model proposes fewer than 3 boxes of 24 pixels'
        out.append(big[[0, big.shape[0] // 3, 2 * big.shape[0] // 3]].cpu().numpy().copy())
    return out


def _hand_image(m, named, inputs, image_id):
    """one image by hand: its gradients copied out (flat, memory order; None where there is none) and its four losses"""
    _set_image_id(m, image_id)
    losses = m(inputs, True)
    sum(losses).backward()
    grads = [None if p.grad is None else _mem(p.grad).cpu().numpy().copy() for _, p in named]
    for _, p in named:
        p.grad = None
    return grads, np.float32([float(x.detach()) for x in losses])


def _hand_step(m, named, opt, flat):
    from tf_eager_object_detection_amd import training
    gradients = []
    for (n, p), g in zip(named, flat):
        if g is None:
            gradients.append(None)
            continue
        t = torch.empty_like(p)                              # (the variable's strides: the bucket holds memory order)
        assert t.stride() == p.stride()
        _mem(t).copy_(torch.from_numpy(g))
        gradients.append(t)
    training.train_step(named, gradients, opt, learning_rate_bias_double=True, weight_decays=training.l2_variables(m.dense, WD))


def _state(m, opt):
    """every parameter and the momentum slot of every trained one, in memory order"""
    torch.cuda.synchronize()
    out = {n: _mem(p.detach()).cpu().numpy().copy() for n, p in m.dense.named_parameters()}
    out.update({n + '/momentum': opt.get_slot(p, 'momentum').cpu().numpy().copy() for n, p in _trained(m)})
    return out


def _equal_states(a, b):
    assert sorted(a) == sorted(b)
    for n in a:
        assert np.array_equal(_bits(a[n]), _bits(b[n])), n


def _trainer(m, opt, K):
    from tf_eager_object_detection_amd import training
    return training.Trainer(m, opt, images_per_step=K, learning_rate_bias_double=True, weight_decay=WD)


def test_trainer_two_images_per_step_equals_the_hand_loop(boxes):
    from tf_eager_object_detection_amd import training
    m = _model(1)
    initial = _state_without_slots(m)
    opt = training.MomentumOptimizer(LR, MU)
    t = _trainer(m, opt, 2)
    stepped = []
    for k in range(4):
        losses, s = t.step(_inputs(k, boxes))
        assert len(losses) == 4
        stepped.append(s)
    assert stepped == [False, True, False, True] and t.images_seen == 4 and t.global_step() == 2 and t.accumulator.pending == 0
    assert all(p.grad is None for _, p in t.named)
    got = _state(m, opt)

    h = _model(1)
    named = training.model_variables(h.dense)
    hopt = training.MomentumOptimizer(LR, MU)
    for w in range(2):
        lists = [_hand_image(h, named, _inputs(2 * w + k, boxes), 2 * w + k)[0] for k in range(2)]
        assert sum(g is not None for g in lists[0]) == 28
        _hand_step(h, named, hopt, anp.window(lists, True))
    _equal_states(got, _state(h, hopt))
    for n, _ in _trained(m):
        assert not np.array_equal(_bits(got[n]), _bits(initial[n])), n                     # the steps moved it


def _state_without_slots(m):
    return {n: _mem(p.detach()).cpu().numpy().copy() for n, p in m.dense.named_parameters()}


def test_trainer_one_image_per_step_is_the_hand_loop_with_no_accumulate_launch(boxes, monkeypatch):
    from tf_eager_object_detection_amd import ops, training
    launches = []
    real = ops.bucket_accumulate
    monkeypatch.setattr(ops, 'bucket_accumulate', lambda *a, **kw: launches.append(1) or real(*a, **kw))
    m = _model(1)
    opt = training.MomentumOptimizer(LR, MU)
    t = _trainer(m, opt, 1)
    trainer_losses = []
    for k in range(2):
        losses, s = t.step(_inputs(k, boxes))
        assert s
        trainer_losses.append(_bits(torch.stack([x.reshape(()) for x in losses])))
    assert launches == [] and t.global_step() == 2 and t.images_seen == 2
    got = _state(m, opt)

    h = _model(1)
    named = training.model_variables(h.dense)
    hopt = training.MomentumOptimizer(LR, MU)
    for k in range(2):
        _set_image_id(h, k)
        losses = h(_inputs(k, boxes), True)
        sum(losses).backward()
        training.train_step(named, [p.grad for _, p in named], hopt, learning_rate_bias_double=True,
                            weight_decays=training.l2_variables(h.dense, WD))
        for _, p in named:
            p.grad = None
        assert np.array_equal(trainer_losses[k], _bits(torch.stack([x.detach().reshape(()) for x in losses])))
    _equal_states(got, _state(h, hopt))


def test_a_run_resumed_inside_an_open_window_continues_with_the_same_bits(boxes, tmp_path):
    from tf_eager_object_detection_amd import training
    K = 2
    m = _model(1)
    opt = training.MomentumOptimizer(LR, MU)
    whole = _trainer(m, opt, K)
    for k in range(IMAGES):
        last, _ = whole.step(_inputs(k, boxes))
    want = _state(m, opt)

    a = _model(1)
    aopt = training.MomentumOptimizer(LR, MU)
    head = _trainer(a, aopt, K)
    for k in range(3):
        head.step(_inputs(k, boxes))
    assert head.accumulator.pending == 1                    # a window left open
    path = head.save(str(tmp_path))
    assert os.path.basename(path) == 'model.ckpt-1' and training.latest_checkpoint(str(tmp_path)) == path

    b = _model(2)                                           # another seed: everything has to come from the checkpoint
    bopt = training.MomentumOptimizer(LR, MU)
    tail = _trainer(b, bopt, K)
    tail.restore(path)
    assert tail.images_seen == 3 and tail.accumulator.pending == 1 and tail.global_step() == 1
    for k in range(3, IMAGES):
        got_last, _ = tail.step(_inputs(k, boxes))
    _equal_states(_state(b, bopt), want)
    assert tail.global_step() == whole.global_step() == 3 and tail.images_seen == whole.images_seen == IMAGES
    assert np.array_equal(_bits(torch.stack([x.reshape(()) for x in got_last])), _bits(torch.stack([x.reshape(()) for x in last])))


# ---- data parallel: two ranks on one card, two images each -------------------------------------------------------------------------
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


def _dp_rank(rank, world, port, q, boxes):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from tf_eager_object_detection_amd import parallel, training
        m = _model(1 if rank == 0 else 2)                    # rank 1 starts from other weights: the broadcast fixes that
        trainer = parallel.DataParallelTrainer(m, training.MomentumOptimizer(LR, MU), learning_rate_bias_double=True, weight_decay=WD,
                                               images_per_rank=2)
        # image k of rank r has the id k * world + r: the rank takes the images with its ids
        losses = trainer.step([_inputs(k * world + rank, boxes) for k in range(2)])
        torch.cuda.synchronize()
        with pytest.raises(ValueError):
            trainer.step([_inputs(rank, boxes)])
        q.put(dict(rank=rank, loss_bits=[int(_bits(x.reshape(1))[0]) for x in losses],
                   variables={n: _mem(p.detach()).cpu().numpy().copy() for n, p in _trained(m)},
                   no_grad_left=all(p.grad is None for _, p in trainer.named), step_index=trainer.step_index))
    finally:
        dist.destroy_process_group()


def test_data_parallel_two_images_per_rank_equals_the_mean_of_means(boxes):
    from tf_eager_object_detection_amd import training
    results = _spawn(_dp_rank, 2, boxes)
    m = _model(1)
    named = training.model_variables(m.dense)
    initial = _state_without_slots(m)
    images = [_hand_image(m, named, _inputs(i, boxes), i) for i in range(4)]                # ids 0 .. 3 on the same weights
    rank_lists = [[images[k * 2 + r][0] for k in range(2)] for r in range(2)]
    rank_scalars = [[images[k * 2 + r][1] for k in range(2)] for r in range(2)]
    mean, mean_losses = anp.mean_of_means(rank_lists, rank_scalars)
    _hand_step(m, named, training.MomentumOptimizer(LR, MU), mean)
    torch.cuda.synchronize()
    for res in results:
        assert res['no_grad_left'] and res['step_index'] == 1
        for n, p in _trained(m):
            got = res['variables'][n]
            assert np.array_equal(_bits(got), _bits(_mem(p.detach()))), (res['rank'], n)
            assert not np.array_equal(_bits(got), _bits(initial[n])), n
        assert res['loss_bits'] == [int(b) for b in _bits(mean_losses)]
