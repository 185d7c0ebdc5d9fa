"""Image-parallel multi-GPU harness: one process per GPU (torch.distributed, backend "nccl" =
RCCL over xGMI on ROCm; "gloo" for the CPU tests), images sharded round-robin over ranks,
ONE all-gather of fixed-size detection records per batch.

The reference has no multi-GPU code at all (README "multi gpu support" is an unchecked TODO;
batch is hard-wired to 1: model/roi_pooling.py:28,66,152).  The path shards naturally by image
-- no stage has cross-image state -- so there is no data-path collective inside an image; the
only exchange is the final record all-gather, which is latency-bound (<= 7.2 KB per image).

Record layout per image: float32 [max_det, 6] = (x1, y1, x2, y2, score, label), padded rows have
score = -1; plus the valid count.  Packed as one float32 [max_det*6 + 1] vector so a batch costs
exactly one collective.

Training is data-parallel with one image per rank (second half of this file): GradientExchange averages the gradients over
the ranks in ascending rank order on csrc/grad_exchange.hip, between two collectives that only move bytes;
broadcast_variables starts the replicas equal; DataParallelTrainer is the loop body around them (images_per_rank = K > 1: every
rank first forms the mean of its own K images, training.GradientAccumulator).
"""
import torch
import torch.distributed as dist


def shard_images(num_images, rank, world_size):
    """Image indices owned by `rank`: r, r+G, r+2G, ... (weak scaling: per-GPU work is fixed when the
    global batch grows with the number of GPUs)."""
    return list(range(rank, num_images, world_size))


def pack_detections(boxes, labels, scores, count, max_det, out=None):
    """Padded post-ops outputs (+ device count) -> float32 [max_det*6+1] record vector.  GPU tensors:
    one HIP launch (odet_pack_detections), no host sync.  CPU tensors (gloo tests): torch ops."""
    if boxes.is_cuda:
        from . import _lib as L
        rec = out if out is not None else torch.empty(max_det * 6 + 1, dtype=torch.float32, device=boxes.device)
        L.check(L.lib().odet_pack_detections(L.dptr(boxes), L.dptr(labels), L.dptr(scores), L.dptr(count),
                                             boxes.shape[0], int(max_det), L.dptr(rec), L.stream()))
        return rec
    m = min(int(count.reshape(-1)[0]), boxes.shape[0], max_det)
    rec = torch.zeros(max_det * 6 + 1, dtype=torch.float32)
    body = rec[:max_det * 6].view(max_det, 6)
    body[:, 4] = -1.0
    body[:m, 0:4] = boxes[:m]
    body[:m, 4] = scores[:m]
    body[:m, 5] = labels[:m].to(torch.float32)
    rec[max_det * 6] = float(m)
    return rec


def unpack_detections(rec, max_det):
    """record vector -> (boxes [M,4], labels int32 [M], scores [M]) with M = stored count (host sync)."""
    m = int(rec[max_det * 6].item())
    body = rec[:max_det * 6].view(max_det, 6)[:m]
    return body[:, 0:4], body[:, 5].to(torch.int32), body[:, 4]


def all_gather_detections(rec, group=None):
    """One collective per batch: every rank receives every rank's record vector -> [world, len]."""
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    if world == 1:
        return rec[None]
    out = torch.empty((world, rec.numel()), dtype=rec.dtype, device=rec.device)
    if rec.is_cuda:
        dist.all_gather_into_tensor(out, rec.contiguous(), group=group)
    else:
        parts = [torch.empty_like(rec) for _ in range(world)]     # gloo: list form
        dist.all_gather(parts, rec.contiguous(), group=group)
        out = torch.stack(parts, 0)
    return out


class GroupExchange:
    """The exchange of the throughput arrangement (bench.py, FpnStreamPool): every rank keeps S stream groups of B
    images in flight; when a group's launches are enqueued, the B fixed-size records of that group of EVERY rank go
    through ONE all-gather (concatenation form) into ``gathered[g]`` = [world, B, rec_len].

    GPU tensors: the collective runs on a communication stream that waits (on the device) for the group's stream;
    the group's stream only waits for the small staging copy, so its next images may overwrite the records while
    the collective is still in flight.  CPU tensors (gloo tests): the same calls without streams.

    A group with fewer than B valid images (ragged tail of a finite image list) passes ``valid``: the records of the
    missing images are sent as empty records (count 0, scores -1), so every rank still contributes B records."""

    def __init__(self, n_groups, batch, rec_len, device, group=None, force_collective=False):
        self.S, self.B, self.rec_len = int(n_groups), int(batch), int(rec_len)
        self.group = group
        # (a one-rank process group still issues the collective: rehearsal of the RCCL call path on a 1-GPU box)
        self.force_collective = bool(force_collective) and dist.is_initialized()
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        dev = torch.device(device)
        self.cuda = dev.type == 'cuda'
        self.gathered = torch.zeros((self.S, self.world, self.B, self.rec_len), dtype=torch.float32, device=dev)
        self.staging = torch.zeros((self.S, self.B, self.rec_len), dtype=torch.float32, device=dev)
        self.comm = torch.cuda.Stream(device=dev) if self.cuda else None
        empty = torch.zeros(self.rec_len, dtype=torch.float32)
        empty[:self.rec_len - 1].view(-1, 6)[:, 4] = -1.0
        self.empty = empty.to(dev)

    def _stage(self, g, records, valid):
        self.staging[g].copy_(records)
        if valid is not None and valid < self.B:
            self.staging[g, valid:] = self.empty

    def gather(self, g, records, producer_stream=None, valid=None):
        """records: [B, rec_len] block of group g (written on ``producer_stream``).  Returns gathered[g]
        ([world, B, rec_len]; on the GPU it is complete once the communication stream has run)."""
        if not self.cuda:
            self._stage(g, records, valid)
            if self.world == 1:
                self.gathered[g, 0].copy_(self.staging[g])
            else:
                parts = [torch.empty_like(self.staging[g]) for _ in range(self.world)]
                dist.all_gather(parts, self.staging[g].contiguous(), group=self.group)
                self.gathered[g].copy_(torch.stack(parts, 0))
            return self.gathered[g]
        st = producer_stream if producer_stream is not None else torch.cuda.current_stream()
        self.comm.wait_stream(st)
        with torch.cuda.stream(self.comm):
            self._stage(g, records, valid)
            copied = torch.cuda.Event()
            copied.record(self.comm)
            if self.world == 1 and not self.force_collective:
                self.gathered[g, 0].copy_(self.staging[g])
            elif dist.get_backend(self.group) == 'gloo':
                # rehearsal of the multi-rank path on a box with fewer GPUs than ranks: gloo moves host memory
                host = self.staging[g].cpu()                      # (synchronises the communication stream)
                parts = [torch.empty_like(host) for _ in range(self.world)]
                dist.all_gather(parts, host, group=self.group)
                self.gathered[g].copy_(torch.stack(parts, 0))
            else:
                dist.all_gather_into_tensor(self.gathered[g].view(self.world * self.B, self.rec_len), self.staging[g],
                                            group=self.group)
        st.wait_event(copied)            # the group's next images may overwrite its records from here on
        return self.gathered[g]

    def synchronize(self):
        if self.cuda:
            self.comm.synchronize()


# ---- data-parallel training: one image per rank, gradients averaged over the ranks in ascending rank order ----------------------
def _world(group):
    return dist.get_world_size(group) if dist.is_initialized() else 1


def _pack_torch(tables, tensors, bucket):
    """ops.bucket_pack in torch ops (CPU tensors, the gloo host tests): +0.0 wherever no tensor lives"""
    bucket.zero_()
    for i, t in enumerate(tables.check(tensors)):
        if t is not None and t.numel():
            o = tables.offset(i)
            bucket[o:o + t.numel()] = torch.as_strided(t, (t.numel(),), (1,), t.storage_offset())
    return bucket


def _unpack_torch(tables, bucket, tensors):
    for i, t in enumerate(tables.check(tensors)):
        if t is not None and t.numel():
            o = tables.offset(i)
            torch.as_strided(t, (t.numel(),), (1,), t.storage_offset()).copy_(bucket[o:o + t.numel()])


def _rank_mean_torch(parts, average):
    """ops.rank_mean in torch ops: one float32 add per rank in ascending rank, one float32 division by a TENSOR divisor"""
    s = parts[0].clone()
    for r in range(1, parts.shape[0]):
        s = s + parts[r]
    return s / torch.full_like(s, float(parts.shape[0])) if average else s


def check_gradients(variables, gradients):
    """the rule of GradientExchange (and of training.GradientAccumulator): one gradient or None per variable, float32, on the
    variable's device, with its shape and strides"""
    if len(gradients) != len(variables):
        raise ValueError('%d gradients for %d variables' % (len(gradients), len(variables)))
    for i, (g, v) in enumerate(zip(gradients, variables)):
        if g is None:
            continue
        if g.dtype == torch.float16:
            raise TypeError('gradient %d is float16: the gradient exchange is float32 only' % i)
        if g.dtype != torch.float32:
            raise TypeError('gradient %d must be float32, got %s' % (i, g.dtype))
        if g.device != v.device:
            raise ValueError('gradient %d lives on %s, its variable on %s' % (i, g.device, v.device))
        if g.shape != v.shape or (g.numel() > 1 and g.stride() != v.stride() and not (g.is_contiguous() and v.is_contiguous())):
            raise ValueError('gradient %d (shape %s, strides %s) does not have the layout of its variable (shape %s, strides %s)'
                             % (i, tuple(g.shape), g.stride(), tuple(v.shape), v.stride()))


class _ExchangeLayout:
    """the buffers of one set of present gradients: the bucket, what the all-to-all receives, the reduced shard, the views"""

    def __init__(self, numels, shapes, world, device):
        from . import ops
        self.tables = ops.BucketTables(numels, world, device)
        self.bucket = torch.zeros(self.tables.bucket_numel, dtype=torch.float32, device=device)
        self.recv = torch.empty(self.tables.bucket_numel, dtype=torch.float32, device=device)
        self.shard = torch.empty(self.tables.shard_numel, dtype=torch.float32, device=device)
        self.views = [None if n is None else torch.as_strided(self.bucket, shape, stride, self.tables.offset(i))
                      for i, (n, (shape, stride)) in enumerate(zip(numels, shapes))]


class GradientExchange:
    """The gradient exchange of data-parallel training (one image per rank): every rank ends with the same bits, the float32 sum
    of the ranks' gradients in ASCENDING RANK order (divided by float32(world) with `average`), whatever the collective library
    does inside -- the two collectives only move bytes and csrc/grad_exchange.hip does the arithmetic:
        pack (one launch) -> all_to_all_single (rank r receives shard r of every rank, [world, shard]) -> odet_rank_mean_f32
        -> all_gather_into_tensor back into the bucket,
    all on the current stream; per-rank traffic is that of a ring all-reduce.  tests/grad_exchange_np.py restates it.

    exchange(gradients) takes one gradient or None per variable and returns a list of the same shape whose tensors are VIEWS into
    the exchange's own bucket with the variable's shape and strides: the same tensors every step, so the optimizer's pointer
    column is uploaded once (and the next exchange overwrites them).  The layout follows the set of present gradients; when that
    set is first seen, or differs from the previous step's, the ranks compare a digest of it through one host-side gather and
    every rank raises ValueError on a mismatch.  (A set that changes on one rank only, later on, leaves the others waiting in
    their collective: the sets have to change together.)  Gradients are float32 with their variable's layout
    (Optimizer.prepare's rule); float16 raises TypeError.

    world == 1 without force_collective returns the gradients as given, with no launch.  Backend "gloo" with GPU tensors moves host
    copies through the two collectives (the rehearsal form of GroupExchange); CPU tensors run the same steps in torch ops."""

    def __init__(self, variables, group=None, average=True, force_collective=False):
        from . import ops
        self.variables = list(variables)
        for i, v in enumerate(self.variables):
            if v.dtype != torch.float32:
                raise TypeError('variable %d must be float32, got %s' % (i, v.dtype))
            if not ops.memory_dense(v):
                raise ValueError('variable %d is not dense in memory (shape %s, strides %s)' % (i, tuple(v.shape), v.stride()))
        self.group, self.average = group, bool(average)
        self.world = _world(group)
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.force_collective = bool(force_collective) and dist.is_initialized()
        self._layouts = {}
        self._key = None

    def _check(self, gradients, scalars):
        check_gradients(self.variables, gradients)
        if scalars is not None and (scalars.dtype != torch.float32 or not scalars.is_contiguous()):
            raise TypeError('scalars must be a contiguous float32 tensor')

    def _agree(self, numels):
        import hashlib
        digest = hashlib.sha256(repr(numels).encode()).hexdigest()
        if self.world > 1:
            digests = [None] * self.world
            dist.all_gather_object(digests, digest, group=self.group)       # the one host-side gather
            if any(d != digest for d in digests):
                raise ValueError('the ranks disagree on the set of present gradients: rank %d has digest %s, the ranks %s'
                                 % (self.rank, digest[:12], [d[:12] for d in digests]))

    def _layout(self, gradients, scalars, device):
        numels = tuple(None if g is None else g.numel() for g in gradients) + (None if scalars is None else scalars.numel(),)
        if numels != self._key:
            self._agree(numels)
            self._key = numels
        lay = self._layouts.get(numels)
        if lay is None:
            shapes = [(tuple(v.shape), v.stride()) for v in self.variables]
            shapes.append(((0,), (1,)) if scalars is None else (tuple(scalars.shape), scalars.stride()))
            lay = self._layouts[numels] = _ExchangeLayout(list(numels), shapes, self.world, device)
        return lay

    def exchange(self, gradients, scalars=None):
        """gradients: one float32 tensor or None per variable.  Returns the list of rank means (views, see the class); with
        `scalars` (a small float32 tensor, e.g. the four losses) returns (list, rank mean of scalars) at no second collective."""
        from . import ops
        gradients = list(gradients)
        self._check(gradients, scalars)
        if self.world == 1 and not self.force_collective:
            return gradients if scalars is None else (gradients, scalars)
        device = self.variables[0].device if self.variables else (scalars.device if scalars is not None else torch.device('cpu'))
        lay = self._layout(gradients, scalars, device)
        tensors = gradients + [scalars]
        tb, W = lay.tables, self.world
        if tb.bucket_numel:
            cuda = device.type == 'cuda'
            if cuda:
                ops.bucket_pack(tb, tensors, lay.bucket)
            else:
                _pack_torch(tb, tensors, lay.bucket)
            parts = lay.recv.view(W, tb.shard_numel)
            if not cuda:
                dist.all_to_all_single(lay.recv, lay.bucket, group=self.group)
                lay.shard.copy_(_rank_mean_torch(parts, self.average))
                dist.all_gather_into_tensor(lay.bucket, lay.shard, group=self.group)
            elif dist.get_backend(self.group) == 'gloo':
                # rehearsal of the multi-rank path on a box with fewer GPUs than ranks: gloo moves host memory
                host = lay.bucket.cpu()
                got = torch.empty_like(host)
                dist.all_to_all_single(got, host, group=self.group)
                lay.recv.copy_(got)
                ops.rank_mean(parts, self.average, out=lay.shard)
                host_shard = lay.shard.cpu()
                dist.all_gather_into_tensor(host, host_shard, group=self.group)
                lay.bucket.copy_(host)
            else:
                dist.all_to_all_single(lay.recv, lay.bucket, group=self.group)
                ops.rank_mean(parts, self.average, out=lay.shard)
                dist.all_gather_into_tensor(lay.bucket, lay.shard, group=self.group)
        out = lay.views[:-1]
        return list(out) if scalars is None else (list(out), lay.views[-1])


def broadcast_variables(variables, src=0, group=None):
    """Every rank ends with rank `src`'s bytes in its float32 variables: pack (one launch), ONE dist.broadcast of the bucket,
    unpack (one launch).  The variables' version counters are bumped, as Optimizer.mark_updated does, so that the tensors the
    detectors derive from their weights rebuild.  Without a process group (or with one rank) nothing happens."""
    from . import ops
    variables = [v.detach() for v in variables]
    for i, v in enumerate(variables):
        if v.dtype != torch.float32:
            raise TypeError('variable %d must be float32, got %s' % (i, v.dtype))
    if _world(group) == 1 or not variables:
        return
    device = variables[0].device
    tables = ops.BucketTables([v.numel() for v in variables], 1, device)
    if device.type != 'cuda':
        bucket = _pack_torch(tables, variables, tables.new_bucket())
        dist.broadcast(bucket, src=src, group=group)
        _unpack_torch(tables, bucket, variables)
    else:
        bucket = ops.bucket_pack(tables, variables)
        if dist.get_backend(group) == 'gloo':
            host = bucket.cpu()
            dist.broadcast(host, src=src, group=group)
            bucket.copy_(host)
        else:
            dist.broadcast(bucket, src=src, group=group)
        ops.bucket_unpack(tables, bucket, variables)
    torch.autograd.graph.increment_version(variables)


class DataParallelTrainer:
    """The loop body of the reference's scripts/train.py:99-103 with one image per rank: forward, backward, gradient exchange,
    training.train_step on the exchanged gradients -- every rank takes the same step on the rank mean of the gradients, so the
    replicas keep identical weights (the optimizer slots start at zero everywhere and stay equal; they are not exchanged).

    The constructor broadcasts rank 0's variables.  model: a trainable caller model (model.dense holds the parameters);
    weight_decay: None, or the L2 coefficient of training.l2_variables."""

    def __init__(self, model, optimizer, group=None, learning_rate_bias_double=False, weight_decay=None, images_per_rank=1):
        from . import training
        self.model, self.optimizer, self.group = model, optimizer, group
        self.images_per_rank = int(images_per_rank)
        if self.images_per_rank < 1:
            raise ValueError('images_per_rank must be at least 1, got %d' % self.images_per_rank)
        self.learning_rate_bias_double = bool(learning_rate_bias_double)
        self.named = training.model_variables(model.dense)
        self.weight_decays = None if weight_decay is None else training.l2_variables(model.dense, weight_decay)
        self.world = _world(group)
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.step_index = 0
        broadcast_variables([p for _, p in self.named], 0, group)
        self.exchange = GradientExchange([p for _, p in self.named], group)
        self.accumulator = None
        if self.images_per_rank > 1:
            # the four losses travel as one more tensor of the accumulated list
            variables = [p for _, p in self.named]
            device = variables[0].device if variables else torch.device('cpu')
            self.accumulator = training.GradientAccumulator(variables + [torch.zeros(4, dtype=torch.float32, device=device)],
                                                            self.images_per_rank)

    def _image(self, inputs, image_id):
        """forward and backward of one image under its Philox image id; returns the four losses as a float32 [4] tensor"""
        m = self.model
        m._anchor_target._next_image_id = image_id
        m._proposal_target._next_image_id = image_id
        if hasattr(m, '_next_dropout_image_id'):
            m._next_dropout_image_id = image_id
        losses = m(inputs, True)
        sum(losses).backward()
        return torch.stack([x.detach().reshape(()) for x in losses])

    def step(self, inputs):
        """inputs: (image, gt_bboxes, gt_labels) of THIS rank's image; with images_per_rank = K > 1 the list of this rank's K
        images.  Returns the four losses' rank means (device tensors).

        K > 1: image k of the step has the id (step_index * K + k) * world + rank; the rank forms its own mean over its images
        (training.GradientAccumulator: the float32 sum in ascending k, / float32(K)), then the exchange averages the ranks'
        means as before -- the rank mean of the ranks' image means, two roundings; the losses go the same way.  K == 1 is the
        path, the ids and the bits of one image per rank."""
        from . import training
        if self.accumulator is not None:
            inputs = list(inputs)
            K = self.images_per_rank
            if len(inputs) != K:
                raise ValueError('%d images for a step of %d images per rank' % (len(inputs), K))
            self.accumulator.reset()
            for k, one in enumerate(inputs):
                scalars = self._image(one, (self.step_index * K + k) * self.world + self.rank)
                out = self.accumulator.add([p.grad for _, p in self.named] + [scalars])
                for _, p in self.named:
                    p.grad = None
            gradients, means = self.exchange.exchange(out[:-1], scalars=out[-1])
        else:
            scalars = self._image(inputs, self.step_index * self.world + self.rank)   # ranks draw different samples and dropout masks
            gradients, means = self.exchange.exchange([p.grad for _, p in self.named], scalars=scalars)
        training.train_step(self.named, gradients, self.optimizer, learning_rate_bias_double=self.learning_rate_bias_double,
                            weight_decays=self.weight_decays)
        for _, p in self.named:
            p.grad = None
        self.step_index += 1
        return tuple(means.clone().unbind(0))
