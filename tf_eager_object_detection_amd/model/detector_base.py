"""What the three assembled detectors (model/fpn_detector.py, model/frcnn_detector.py) share: ONE pass -- prepare, the dense
parts, the batched hot path with the RoI head between its stages, the after-pass checks (sync-free NMS completeness, the two-limb
float32 form's range), im_detect and the HIP-graph capture -- written once in `Detector`; the RoI heads' last layer
(`_FinalLayer`) and the float32 form's plumbing.  A family supplies its network and what genuinely differs (see `Detector`).
This module depends on neither detector file; both import from it (its only sibling import: model/layers.py, the layer builders)."""
import contextlib
import functools

import torch
import torch.nn as nn

from .. import ops
from ..derived import derived
from .layers import _nhwc, _pad_rows64  # noqa: F401  (_nhwc: importable from here, as the caller models take it)

# sync-free NMS chunks of the assembled detectors unless the caller says otherwise: the first two from the ranked
# selection (shared launches), the third on the full order -- enough for clustered (trained-like) and massively tied
# (random-init float16) score distributions; an image that still does not complete is reported empty and flagged
DEFAULT_BLIND_CHUNKS = 4


def check_caller_f32_form(form):
    """the reference-surface caller objects (base_fpn_model.py, base_faster_rcnn_model.py) take every float32 form; with 'x2'
    their call / im_detect / predict_rois read the dense part's range status word after the pass and repeat an out-of-range
    pass on three limbs (run_range_checked below), as the detectors do"""
    if form not in ('exact', 'x3', 'x2'):
        raise ValueError("f32_form must be 'exact', 'x3' or 'x2'")


def caller_range_checked(method):
    """decorator for the caller objects' composed passes (call / im_detect / predict_rois): with the dense part on the two-limb
    form, a pass that reported an out-of-range activation is repeated on three limbs (run_range_checked)"""
    @functools.wraps(method)
    def run(self, *args, **kw):
        dense = self.__dict__.get('_dense_ref')
        if dense is None or getattr(dense, 'f32_form', 'exact') != 'x2':
            return method(self, *args, **kw)
        return dense.run_range_checked(lambda: method(self, *args, **kw))
    return run


def _in_f32_form(method):
    """runs a detector's dense method in the detector's `f32_form` (ops.f32_form) and, for the backward of a trainable part, `grad_form`"""
    @functools.wraps(method)
    def run(self, *args, **kw):
        form, grad = getattr(self, 'f32_form', 'exact'), getattr(self, 'grad_form', 'exact')
        with ops.f32_form(form, workspace=_x3_workspace_of(self) if form != 'exact' else None), ops.grad_form(grad):
            return method(self, *args, **kw)
    return run


def _x3_workspace_of(model):
    """the ops.X3Workspace (split-K tickets / parts, the two-limb form's range status word) a detector instance OWNS, on its
    parameters' device (moved to another GPU: a new one there).  Every launch of the instance, eager on any stream or replayed from
    a graph, uses it (range_ok() reads its own launches' word), so one instance's passes must not run concurrently with each other."""
    dev = next(model.parameters()).device
    ws = model.__dict__.get('_x3_ws')
    if dev.type == 'cuda' and (ws is None or ws.buf.device != dev):      # (off the GPU nothing launches: none is made)
        ws = model.__dict__['_x3_ws'] = ops.X3Workspace(dev)
    return ws


class _FinalLayer:
    """The RoI heads' last layer of the three detectors: class logits and box regressions as ONE contraction with the
    concatenated [Ccls + 4 Ccls, K] weights (rows zero-padded to a multiple of 64) on the pointwise GEMM kernel, float32
    results in both modes (float32 accumulation AND no rounding of the result: a float16 logit near 10 is 0.008 coarse,
    1 % of a softmax score)."""

    def _final_layer(self):
        def build(*ps):
            with torch.no_grad():
                wc = torch.cat([ps[0], ps[2]], 0)
                wpad = _pad_rows64(wc)
                b = _pad_rows64(torch.cat([ps[1], ps[3]], 0).float())
            gran = 64 if wc.dtype == torch.float16 else 32
            return wpad if wc.shape[1] % gran == 0 and wc.shape[1] >= 2 * gran else None, b.contiguous()
        return derived(self, 'final', (self.score.weight, self.score.bias, self.bbox.weight, self.bbox.bias), build)

    def _final_outputs(self, x):
        """x [rows, K] (the head's last activation) -> (class logits [rows, Ccls], box regressions [rows, 4 Ccls])"""
        n1 = self.score.out_features
        n5 = n1 + self.bbox.out_features
        wpad, b32 = self._final_layer()
        if not x.is_cuda or x.dtype not in (torch.float16, torch.float32) or wpad is None:
            raise RuntimeError('RoI head: the last layer needs a float16 / float32 GPU activation with a multiple of %d >= %d '
                               'channels (got %s %s on %s)' % (64 if x.dtype == torch.float16 else 32,
                                                                128 if x.dtype == torch.float16 else 64, tuple(x.shape), x.dtype, x.device))
        x = x if x.is_contiguous() else x.contiguous()
        y = ops.dense(x, wpad, b32) if x.dtype == torch.float32 else ops.dense_f16_out_f32(x, wpad, b32)
        return y[:, :n1], y[:, n1:n5]

    def _final_outputs_trainable(self, x):
        """_final_outputs with a backward pass (float32): still ONE contraction on the padded concatenated weights; the padded
        weight gets a gradient [pad64(5 C), K] and the padded bias one [pad64(5 C)], whose row slices are the gradients of
        score / bbox (the dy of the padding columns is zero, so the padding rows' gradients are zero and go nowhere)"""
        n1 = self.score.out_features
        n5 = n1 + self.bbox.out_features
        wpad, b32 = self._final_layer()
        if not x.is_cuda or x.dtype != torch.float32 or wpad is None or wpad.dtype != torch.float32:
            raise RuntimeError('RoI head (trainable): the last layer needs a float32 GPU activation with a multiple of 32 >= 64 '
                               'channels (got %s %s on %s)' % (tuple(x.shape), x.dtype, x.device))
        y = _FinalTrainable.apply(x if x.is_contiguous() else x.contiguous(), self.score.weight, self.score.bias, self.bbox.weight,
                                  self.bbox.bias, wpad, b32)
        return y[:, :n1], y[:, n1:n5]


@ops.carries_grad_form
class _FinalTrainable(torch.autograd.Function):
    """the padded final layer: ops.dense on the derived (padded, concatenated) weights forward; one ops.dense_wgrad on them
    backward, handed out as row slices in the order (score.weight, score.bias, bbox.weight, bbox.bias)"""

    @staticmethod
    def forward(ctx, x, score_w, score_b, bbox_w, bbox_b, wpad, bpad):
        ctx.save_for_backward(x, wpad)
        ctx.rows = (int(score_w.shape[0]), int(score_w.shape[0]) + int(bbox_w.shape[0]))
        return ops.dense(x, wpad, bpad)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, wpad = ctx.saved_tensors
        n1, n5 = ctx.rows
        dy = dy if dy.is_contiguous() else dy.contiguous()
        dw, db = ops.dense_wgrad(dy, x)
        dx = ops.dense_dgrad(dy, wpad) if ctx.needs_input_grad[0] else None
        return dx, dw[:n1], db[:n1], dw[n1:n5], db[n1:n5], None, None


class _NmsCompleteness:
    """The detectors run the proposal stage sync-free (no host check between kernels; graph-capturable) with a fixed
    number of NMS chunks.  If an image needs more than those, the hot path reports it EMPTY and flags it
    (nms_done = 0, include/odet.h): `forward()` reads the flags after the last launch of the pass whenever it is not
    being captured into a HIP graph and `check_nms` is on (default), and sends ONLY the flagged images through the pass
    again from the RPN head's outputs with the exact proposal stage (host-checked chunks, as many as the image needs:
    the reference's NMS is always exact, model/region_proposal.py:73-81) -- their outputs are overwritten in place, the
    other images are not touched; `nms_reruns` counts them.  Throughput loops that do not want a host sync per pass set
    `model.check_nms = False` and call `recover()` (on 'x2' also `range_ok()`) themselves, after a replay too; `check_complete()` raises."""

    check_nms = True
    nms_reruns = 0
    _last_batch = 0
    _last_pass = None            # (rpn scores, rpn deltas, maps, heads) of the last pass: what a re-run starts from

    def nms_done(self, batch=None):
        """device int32 flags (1 = complete) of the images of the last pass"""
        n = self._last_batch if batch is None else batch
        return [h.nms_done for h in self._hot[:n]]

    def incomplete(self, batch=None):
        """indices of the images of the last pass whose sync-free NMS did not complete (one device -> host copy)"""
        steps = getattr(self, '_steps', None)
        if steps is not None and hasattr(steps, 'nms_done_all'):
            n = self._last_batch if batch is None else batch
            flags = steps.nms_done_all[:n].tolist()
        else:
            flags = [int(t.item()) for t in self.nms_done(batch)]
        return [b for b, f in enumerate(flags) if f != 1]

    def check_complete(self, batch=None):
        bad = self.incomplete(batch)
        if bad:
            raise RuntimeError('the RPN NMS of image(s) %s did not complete inside blind_chunks = %d sync-free chunks: their '
                               'results are reported EMPTY (recover() re-runs them in the exact mode)'
                               % (bad, self._hot[0].blind_chunks))

    def recover(self, batch=None, last_pass=None):
        """re-runs the flagged images of the last pass (or of `last_pass`, a captured graph's) in the exact mode; -> their indices"""
        bad = self.incomplete(batch)
        last_pass = last_pass or self._last_pass
        if bad and last_pass is None:
            raise RuntimeError('image(s) %s incomplete and no pass to re-run them from' % bad)
        for b in bad:
            self._rerun_exact(b, last_pass)
        self.nms_reruns += len(bad)
        return bad

    def _rerun_exact(self, b, last_pass):
        """image b of `last_pass` again from the RPN head's outputs: exact proposals -> RoI features -> RoI head ->
        post-ops, into the buffers the pass handed out"""
        rpn_scores, rpn_deltas, maps, heads = last_pass
        if maps is None:
            raise RuntimeError('image %d flagged incomplete after its pass was checked and its maps released' % b)
        hot = self._hot[b]
        hot.stage_proposals(rpn_scores[b], rpn_deltas[b], exact=True)
        feats = hot.stage_roi(self._maps_of(maps, b))
        logits, bbox = self.roi_head(feats)
        cls, dlt = heads[b]
        if cls.shape[0] == logits.shape[0] and cls.is_contiguous() and dlt.is_contiguous():
            torch.softmax(logits.float(), dim=-1, out=cls)
            dlt.view(dlt.shape[0], -1).copy_(bbox)
        else:
            cls, dlt = torch.softmax(logits.float(), dim=-1).contiguous(), bbox.float().contiguous()
            heads[b] = (cls, dlt)
        hot.stage_detect(cls, dlt)

    def _after_pass(self, batch, check):
        """-> False if the pass has to be repeated on the three-limb form (its workspace's passed()), else True"""
        self._last_batch = batch
        if check is None:
            check = self.check_nms and not torch.cuda.is_current_stream_capturing()
        x2 = getattr(self, 'f32_form', 'exact') == 'x2'
        if check:
            if x2 and not _x3_workspace_of(self).passed():
                return False
            self.recover(batch)
            # every image of the pass is complete: nothing is left to re-run, so the pass's pyramid (P2..P5: ~90 MB per image)
            # is released here instead of staying pinned until the next pass ends; the RPN outputs and the heads' outputs stay
            lp = self._last_pass
            if lp is not None:
                self._last_pass = (lp[0], lp[1], None, lp[3])
        elif x2 and not torch.cuda.is_current_stream_capturing():      # (a pass being captured launches nothing: replays mark)
            _x3_workspace_of(self).mark_unchecked()       # (host only: whoever checks next cannot call a set word its own)
        return True

    # ---- the two-limb float32 form's RANGE (f32_form = 'x2': float16 limbs).  An activation beyond float16's range becomes an
    # infinite limb and every sum it enters is non-finite before bias / shortcut / ReLU, whatever the weights' signs: the
    # launch's epilogue ORs 1 into the RANGE STATUS word of the instance's workspace (include/odet.h; csrc/conv_f32_common.h) --
    # a flag, not a propagated value: a -inf that a ReLU maps to 0 is still reported.  The word is read where the NMS flags
    # are read; a pass that set it is run again on the three-limb form (bfloat16 limbs: float32's range), counted in
    # `range_reruns`.  The word's rules are ops.X3Workspace's; this class keeps no range state of its own: a checked pass asks
    # passed(), an unchecked one (check_nms = False, a graph replay) says mark_unchecked(), the caller asks range_ok().  What a
    # checked pass reports about itself is not the caller's (that pass was repeated); what unchecked launches reported is, also
    # when a checked pass or im_detect has read the word in between.
    range_reruns = 0

    def range_ok(self):
        """the caller's read: ops.X3Workspace.range_ok() of the instance's workspace (one host sync, on the current stream only)"""
        ws = self.__dict__.get('_x3_ws')
        return ws is None or ws.range_ok()                 # (no workspace: no split-precision launch yet)

    @contextlib.contextmanager
    def _on_three_limbs(self):
        """what repeats a two-limb pass that went out of range runs inside this: counted in `range_reruns`, on the three-limb
        form, and back on two limbs afterwards whatever happened"""
        self.range_reruns += 1
        self.f32_form = 'x3'
        try:
            yield
        finally:
            self.f32_form = 'x2'

    def run_range_checked(self, fn):
        """fn() -> result on this instance's float32 form; a two-limb pass that reported an out-of-range activation is repeated
        on three limbs (`range_reruns`).  For composed passes (im_detect, the caller objects' call).  A composed pass may also
        FAIL on the non-finite maps of such a pass (no proposal survives, the reference's own torch.cat / tf.concat of an empty
        list raises): the error is the range's if the status word is set -- then the pass is repeated, else it is the caller's."""
        if getattr(self, 'f32_form', 'exact') != 'x2':
            return fn()
        ws = _x3_workspace_of(self)
        try:
            out = fn()
        except Exception:
            if ws is None or ws.passed():                  # (no workspace: not on the GPU, where every layer raises)
                raise
        else:
            if ws.passed():
                return out
        # out of range -- or the word was left by earlier unchecked launches: one needless repeat, and passed() keeps it reported
        with self._on_three_limbs():
            return fn()

    def _forward_checked(self, images_nhwc, check, run):
        """run(images) -> outputs, then the after-pass checks; a two-limb pass out of range is repeated on three limbs"""
        outs = run(images_nhwc)
        if not self._after_pass(len(outs), check):
            with self._on_three_limbs():
                outs = run(images_nhwc)
                self._after_pass(len(outs), check)
        return outs


class Detector(_NmsCompleteness, _FinalLayer, nn.Module):
    """An assembled detector's pass, written once.  `forward(images)` takes NHWC float images [B,H,W,3] (already
    mean-subtracted, as the reference's input pipeline delivers them) and returns, per image, the padded detections of
    post_ops_prediction plus their count on the device.  A family supplies, besides its network (`roi_head`, ...):

      _step_batch_class, _hot_path_class   the hot path of the batched / the per-image arrangement (pipeline.py)
      _dense(images)                       -> (rpn scores [B,..], rpn deltas [B,N,4], maps): float32 contiguous RPN outputs and
                                           the contiguous NHWC map(s) of the batch in the hot path's feature dtype
      _maps_of(maps, b)                    image b's share of `maps`, as the hot path's stage_roi / bind take it
      _kept_rois                           the hot-path tensor whose rows are the proposals in the order of the head's rows
      _prepare_per_image, _per_image_to_head, _per_image     the `batched=False` arrangement, which differs by family"""

    _step_batch_class = _hot_path_class = None
    _kept_rois = 'rois'
    _hot = ()                    # the hot-path slots, one per image of the largest batch (prepare)
    _steps = None                # the step batch of the batched arrangement; None: per image
    _cls = _dlt = None           # batched arrangement: the heads' outputs [max_batch, K, Ccls] / [max_batch, K, 4 Ccls] ...
    _bound = False               # ... and whether every step descriptor has been filled once (then only pointers are rebound)
    _max_batch = 1
    _hot_args = ()               # (image_shape, num_classes, num_proposals, channels) and the keywords of the hot-path classes;
    _hot_kwargs = {}             # `batched=False` among them selects the per-image arrangement

    def _declare_modes(self, dtype, grad_form, f32_form, image_shape, num_classes):
        """the modes every constructor sets before it builds its layers.  f32_form (float32 only): 'exact' = exact-float32 matrix
        instructions (the parity mode), 'x3' = three bfloat16 limbs per operand (float32-class accuracy at 2.6 x the peak rate),
        'x2' = two float16 limbs (their range: _NmsCompleteness.range_ok); grad_form: 'exact' | 'x3' (ops.grad_form)"""
        # (one tuple assignment on purpose: test_detectors_share_one_pass counts this file's plain assignments to f32_form,
        # which are the two of the x2 -> x3 switch in _on_three_limbs; setting the mode at construction is not that switch)
        self.dtype, self.f32_form, self.grad_form = dtype, f32_form, ops.check_grad_form(grad_form)
        self.image_shape = (int(image_shape[0]), int(image_shape[1]))
        self.num_classes = num_classes

    def _declare_hot_path(self, channels, num_proposals, max_batch, hot_kwargs, **defaults):
        self._hot_args = (self.image_shape, self.num_classes, num_proposals, channels)
        self._hot_kwargs = dict(defaults, blind_chunks=DEFAULT_BLIND_CHUNKS)
        self._hot_kwargs.update(hot_kwargs)
        self._hot = []
        self._max_batch = max_batch

    def prepare(self, device='cuda'):
        """Moves the model to the GPU and allocates the hot path.  The images of a batch go through the hot path in the SAME
        kernel launches and through the RoI head as one batch (the family's step batch; sync-free NMS with `blind_chunks`
        chunks); `batched=False` in the hot-path keywords selects the family's per-image arrangement -- however often the
        detector is prepared (the keywords are read from a copy)."""
        self.to(device=device, dtype=self.dtype, memory_format=torch.channels_last).eval()
        ops.invalidate_planes(self)                   # (every derived tensor: the weights may have been rewritten through .data)
        # float16 maps go to the RoI kernel as they are, anything else as float32
        fd = self._feature_dtype = torch.float16 if self.dtype == torch.float16 else torch.float32
        kw = dict(self._hot_kwargs)
        batched = kw.pop('batched', True)
        self._steps = None
        if self._max_batch <= 64 and batched:
            self._steps = self._step_batch_class(self._max_batch, *self._hot_args, feature_dtype=fd, **kw)
            self._hot = self._steps.slots
            K, dev = self._hot_args[2], self._hot[0].device
            self._cls = torch.zeros((self._max_batch, K, self.num_classes), dtype=torch.float32, device=dev)
            self._dlt = torch.zeros((self._max_batch, K, 4 * self.num_classes), dtype=torch.float32, device=dev)
            self._bound = False
        else:
            self._hot = [self._hot_path_class(*self._hot_args, feature_dtype=fd, **kw) for _ in range(self._max_batch)]
            self._prepare_per_image()
        return self

    # ---- the per-image arrangement's defaults: one image after the other on the current stream --------
    def _prepare_per_image(self):
        pass

    def _per_image(self, B, fn):
        return [fn(b) for b in range(B)]

    # ---- the pass -----------------------------------------------------------------------------------
    def _hot_to_head(self, B, rpn_scores, rpn_deltas, maps):
        """proposals -> RoI features -> RoI head.  Per image (class softmax [K,Ccls], raw deltas [K,4*Ccls]) for the RoIs of its
        hot-path slot; rows >= the image's proposal count are padding."""
        if self._steps is None:
            return self._per_image_to_head(B, rpn_scores, rpn_deltas, maps)
        # B images in the same hot-path launches, the RoI head on all B x K crops at once
        sb = self._steps
        bind = sb.rebind if self._bound else sb.bind
        for b in range(B):
            bind(b, rpn_scores[b], rpn_deltas[b], self._maps_of(maps, b), self._cls[b], self._dlt[b])
        if B == self._max_batch:
            self._bound = True                      # every descriptor has been filled once
        sb.enqueue(sb.STAGE_PROPOSALS | sb.STAGE_ROI, B)
        K = self._cls.shape[1]
        feats = sb.roi_features[:B].reshape((B * K,) + tuple(sb.roi_features.shape[2:]))
        logits, bbox = self.roi_head(feats)
        torch.softmax(logits.float(), dim=-1, out=self._cls[:B].view(B * K, -1))
        self._dlt[:B].view(B * K, -1).copy_(bbox)
        return [(self._cls[b], self._dlt[b]) for b in range(B)]

    def _run_to_head(self, images_nhwc):
        """everything of the inference pass before post_ops_prediction (base_fpn_model.py:208-265 / :372-382,
        base_faster_rcnn_model.py:132-187 / :279-304)"""
        B = images_nhwc.shape[0]
        if B > len(self._hot):
            raise ValueError('batch %d exceeds max_batch %d' % (B, len(self._hot)))
        rpn_scores, rpn_deltas, maps = self._dense(images_nhwc)
        heads = self._hot_to_head(B, rpn_scores, rpn_deltas, maps)
        self._last_pass = (rpn_scores, rpn_deltas, maps, heads)
        return heads

    def _detect(self, heads):
        B = len(heads)
        if self._steps is None:
            return self._per_image(B, lambda b: self._hot[b].stage_detect(heads[b][0], heads[b][1]))
        sb = self._steps
        sb.enqueue(sb.STAGE_DETECT, B)
        return [(h.det_boxes, h.det_labels, h.det_scores, h.det_count) for h in sb.slots[:B]]

    @torch.no_grad()
    def forward(self, images_nhwc, check=None):
        """-> per image (boxes [M,4], labels [M], scores [M], count) padded to max_per_image, count on the device
        (post_ops_prediction, base_fpn_model.py:267-275 / base_faster_rcnn_model.py:189-197).  check: see _NmsCompleteness."""
        return self._forward_checked(images_nhwc, check, lambda im: self._detect(self._run_to_head(im)))

    @torch.no_grad()
    def im_detect(self, images_nhwc, img_scale):
        """The evaluation entry of the reference models (base_fpn_model.py:364-390, base_faster_rcnn_model.py:279-306): per
        image (softmax scores [R,Ccls], raw deltas [R,4*Ccls], rois / img_scale [R,4]) for the R proposals the image kept, in
        the order of `_kept_rois` (FPN: level-sorted with empty levels dropped, :384-388; single level: NMS order) -- what
        evaluation.pascal_eval.detect_image (pascal_eval_files_utils.py:76-106) consumes with img_scale = 1.  img_scale: one
        number or one per image.  Host-syncs once (R is data dependent, as in the reference)."""
        heads = self.run_range_checked(lambda: self._run_to_head(images_nhwc))     # ('x2': out of range -> again on three limbs)
        B = len(heads)
        self._last_batch = B
        self.recover(B)
        out = []
        for b, (cls, dlt) in enumerate(heads):
            hot = self._hot[b]
            rois = getattr(hot, self._kept_rois)
            k = int(hot.roi_count.item())
            sc = img_scale[b] if isinstance(img_scale, (list, tuple)) or (hasattr(img_scale, 'ndim') and img_scale.ndim > 0) else img_scale
            # tensor / tensor: a true float32 division per element (tensor / python-number multiplies by the reciprocal
            # on the GPU, which is not what tf.to_float(img_scale) division gives)
            div = torch.full((1,), float(sc), dtype=torch.float32, device=rois.device)
            out.append((cls[:k].clone(), dlt[:k].clone(), rois[:k] / div))
        return out

    # ---- HIP-graph replay ---------------------------------------------------------------------------
    def capture(self, batch, warmup=3):
        """Captures forward() for `batch` images of self.image_shape into ONE HIP graph (the whole detector:
        convolutions, neck merges, the sync-free hot path, the RoI head) and
        returns `run(images_nhwc) -> outputs`: the images are copied into the graph's static input and the
        graph is replayed -- a few hundred launches cost one host call, which is what a batch-1 latency
        step is bound by.  Needs the sync-free proposal stage (blind_chunks >= 1: no host check inside).
        A replay makes NO after-pass check (no host sync): `run.recover()` re-runs images whose sync-free NMS did not complete
        (from the CAPTURED pass's tensors), and with f32_form = 'x2' the caller reads `run.range_ok()` (ops.X3Workspace.range_ok
        of the workspace captured with: False = some replay since the last call left float16's range -- forward() those again)."""
        if not self._hot:
            raise RuntimeError('prepare() first')
        dev = next(self.parameters()).device
        static_in = torch.zeros((batch,) + self.image_shape + (3,), dtype=torch.float32, device=dev)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(max(1, warmup)):                  # every lazy allocation (weight packs, workspaces)
                self.forward(static_in)
            side.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                static_out = self.forward(static_in)
        torch.cuda.current_stream(dev).wait_stream(side)
        # what the graph's launches use, whatever the instance does afterwards: the workspace of the passes above (None: they
        # made no split-precision launch, and none is allocated for them) and the captured pass's own tensors
        ws, lp = self.__dict__.get('_x3_ws'), self._last_pass

        def run(images_nhwc):
            static_in.copy_(images_nhwc)
            if ws is not None:
                ws.mark_unchecked()                          # (host only)
            graph.replay()
            return static_out

        run.graph = graph
        run.range_ok = self.range_ok if ws is None else ws.range_ok
        run.recover = lambda: self.recover(batch, lp)
        return run
