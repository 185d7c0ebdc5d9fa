"""The float32 layers' arithmetic forms and what they need on the host: the two ambient forms (`f32_form` for the forward layers,
`grad_form` for the gradient GEMMs), the weights' limb planes, and the split-precision workspace with the two-limb form's RANGE
STATUS word -- the ONE owner of that word's rules (X3Workspace).  `ops` imports every name back (ops.f32_form, ops.X3Workspace,
...); this module imports `_lib` and `derived` only."""
import contextvars
import ctypes as C
import functools
import math

import torch

from . import _lib as L
from .derived import derived

# ---- the float32 layers' arithmetic form ------------------------------------------------------------------------------------
# 'exact': v_mfma_f32_16x16x4_f32 (csrc/conv_f32.hip) -- every product and sum rounded to float32 once, a chain of fmaf.
# 'x3':    split precision (csrc/conv_x3.hip) -- float32 operands as three bfloat16 limbs, six limb products per k on the
#          bfloat16 matrix instructions, float32 accumulation: within float32 rounding of the float64 truth like 'exact',
#          2.6 x its peak rate.  Same tensors in memory; only the weights get a cached companion (their limb planes).
# 'x2':    the two-limb float16 form of the same kernel -- h + l * 2^-11 (operands to one float32 ulp), three products, half the
#          matrix work of 'x3'; for data inside float16's RANGE (|activation| <= 65504, else infinities / NaN; include/odet.h).
# A fixed choice of the caller (the detectors' `f32_form` argument), never a timing decision: the two forms round differently.
# The form (and, optionally, the split-K / status workspace the launches of the block use) is AMBIENT state of the calling
# context, held in a contextvars.ContextVar: two Python threads (or asyncio tasks) that enter and leave `f32_form` blocks in any
# interleaving each see their own value -- a form switch is never implicit and can never leak into another thread's layers.
_F32_CTX = contextvars.ContextVar('odet_f32_form', default=('exact', None))


def current_f32_form():
    return _F32_CTX.get()[0]


class _FormBlock:
    """a `with` block that sets one ContextVar to one value; re-entrant: ONE object may be entered again inside itself (a stack
    of tokens, pushed on the way in, popped on the way out -- by an exception too)"""

    def __init__(self, ctx, value):
        self._ctx, self._value, self._tokens = ctx, value, []

    def __enter__(self):
        self._tokens.append(self._ctx.set(self._value))
        return self

    def __exit__(self, *exc):
        self._ctx.reset(self._tokens.pop())
        return False


class f32_form(_FormBlock):
    """with ops.f32_form('x3'): ...  -- the form the float32 conv3x3 / pointwise / dense / lateral_merge / pointwise_dual calls
    inside the block run on.  `workspace`: an ops.X3Workspace the block's split-precision launches use (the detectors own one
    per instance); None = the calling stream's default workspace.
    The form is a ContextVar, and a Python thread starts with an EMPTY context: a worker thread started inside a block sees
    'exact' (and no workspace), not the block's form, unless it runs under contextvars.copy_context() (ctx.run(fn)) or enters
    a block of its own."""

    def __init__(self, form, workspace=None):
        if form not in ('exact', 'x3', 'x2'):
            raise ValueError("f32 form must be 'exact', 'x3' or 'x2'")
        if workspace is not None and not isinstance(workspace, X3Workspace):
            raise TypeError('workspace must be an ops.X3Workspace')
        self.form, self.workspace = form, workspace
        super().__init__(_F32_CTX, (form, workspace))


# ---- the gradient GEMMs' arithmetic form -------------------------------------------------------------------------------------
# A second ambient form, beside f32_form (which the forward layers read and under which every backward front keeps refusing
# anything but 'exact'): 'exact' runs the Dense / 3x3 gradients on v_mfma_f32_16x16x4_f32, 'x3' on three bfloat16 limbs and six
# limb products per k (csrc/grad_gemm.h: dg_tile_x3; the 3x3 input gradient: the forward's x3 kernel on the flipped weight).
# The bias gradients are the same ordered float32 sums in either.  A two-limb form is not offered.
# autograd runs `backward` on a thread of its own, where a ContextVar shows its default: a torch.autograd.Function whose backward
# reaches these ops records the form in `forward` and re-enters it in `backward` (carries_grad_form).
_GRAD_CTX = contextvars.ContextVar('odet_grad_form', default='exact')
GRAD_FORMS = ('exact', 'x3')


def current_grad_form():
    return _GRAD_CTX.get()


def check_grad_form(form):
    if form not in GRAD_FORMS:
        raise ValueError("grad form must be 'exact' or 'x3', got %r" % (form,))
    return form


class grad_form(_FormBlock):
    """with ops.grad_form('x3'): ...  -- the form dense_dgrad / dense_wgrad / conv3x3_wgrad_f32_levels /
    conv3x3_dgrad_f32_levels calls inside the block, and the backward passes of the *_trainable functions called inside it, run on."""

    def __init__(self, form):
        self.form = check_grad_form(form)
        super().__init__(_GRAD_CTX, form)


def carries_grad_form(cls):
    """class decorator of a torch.autograd.Function whose backward reaches the gradient ops -- the ONE place that carries the
    form across threads: forward records the caller's grad form on the node, the whole of backward runs inside it (a node that
    no forward made has recorded none: the default, 'exact')"""
    forward, backward = cls.forward, cls.backward

    @functools.wraps(forward)
    def record(ctx, *args):
        ctx.grad_form = current_grad_form()
        return forward(ctx, *args)

    @functools.wraps(backward)
    def reenter(ctx, *grads):
        with grad_form(getattr(ctx, 'grad_form', 'exact')):
            return backward(ctx, *grads)
    cls.forward, cls.backward = staticmethod(record), staticmethod(reenter)
    return cls


def split_bf16x3(w):
    """float32 contiguous GPU tensor (even element count) -> its three bfloat16 limb planes, int16 [3, *w.shape]
    (odet_split_bf16x3): w == plane0 + plane1 + plane2 exactly (round to nearest even at every limb)."""
    if w.dtype != torch.float32 or not w.is_cuda or not w.is_contiguous() or w.numel() % 2:
        raise ValueError('split_bf16x3: needs a contiguous float32 GPU tensor with an even element count')
    planes = torch.empty((3,) + tuple(w.shape), dtype=torch.int16, device=w.device)
    L.call('odet_split_bf16x3', L.dptr(w), C.c_void_p(planes.data_ptr()), w.numel(), L.stream())
    return planes


def f16x2_exponent(w):
    """the power of two the two-limb planes of `w` are scaled by: the largest |w| * 2^e lies in [512, 1024)"""
    top = float(w.abs().max())
    if not math.isfinite(top):
        raise ValueError('split_f16x2: the weights must be finite')
    return 0 if top == 0.0 else max(-100, min(100, 9 - math.frexp(top)[1] + 1))


def split_f16x2(w, w_exp=None):
    """float32 contiguous GPU tensor (even element count) -> (its two float16 limb planes of w * 2^w_exp, int16 [2, *w.shape];
    w_exp) (odet_split_f16x2): w * 2^w_exp = plane0 + plane1 * 2^-11 to within one float32 ulp."""
    if w.dtype != torch.float32 or not w.is_cuda or not w.is_contiguous() or w.numel() % 2:
        raise ValueError('split_f16x2: needs a contiguous float32 GPU tensor with an even element count')
    if w_exp is None:
        w_exp = f16x2_exponent(w)
    planes = torch.empty((2,) + tuple(w.shape), dtype=torch.int16, device=w.device)
    L.call('odet_split_f16x2', L.dptr(w), C.c_void_p(planes.data_ptr()), w.numel(), int(w_exp), L.stream())
    return planes, int(w_exp)


class X3Workspace:
    """The caller-owned workspace of the split-precision launches (include/odet.h): split-K ticket words in bytes
    [0, odet_x2_status_offset()) (zero-filled once; every launch leaves them zero), the two-limb form's RANGE STATUS word at that
    offset, the split-K parts.  One workspace serves launches that are ordered on the device (one stream, or one captured graph
    replayed by one stream at a time): two launches that run CONCURRENTLY must not share one -- the detectors own one per
    instance for that reason (a captured graph keeps using the instance's, whatever stream replays it), bare `ops` calls get one
    per (device, stream).

    The status word's rules, all of them here.  Launches only OR into the word; only passed() and range_ok() clear it, and
    neither ever drops a report that someone still has to be told about.  Two pieces of host state stand beside the word:
      the MARK   launches have been enqueued on this workspace that nobody has checked yet (mark_unchecked(): an unchecked pass,
                 a graph replay);
      the LATCH  a report the caller has not seen: passed() found the word set while the mark was set, so the report may be
                 the unchecked launches' and not (only) the checked pass's -- that pass is repeated anyway, and the report
                 stays for range_ok()."""

    def __init__(self, device):
        self.buf = torch.zeros(int(L.lib().odet_x3_workspace_bytes()), dtype=torch.uint8, device=device)
        off = int(L.lib().odet_x2_status_offset())
        self._tickets = self.buf[:off]
        self._status = self.buf[off:off + 4].view(torch.int32)
        self._latch = self._mark = False

    def args(self):
        return C.c_void_p(self.buf.data_ptr()), self.buf.numel()

    def range_flag(self):
        """the status word as a device tensor (int32 [1]; non-zero: a two-limb launch since the last clear saw a non-finite sum)"""
        return self._status

    def _take_word(self):
        """-> whether the word was set (one host sync: waits for the CURRENT stream's launches); clears it when it was"""
        bad = int(self._status.item()) != 0
        if bad:
            self._status.zero_()
        return bad

    def mark_unchecked(self):
        """host only: launches go onto this workspace whose report no after-pass check will read"""
        self._mark = True

    def passed(self):
        """the after-pass read of a checked pass: True iff the word is clear.  A set word is cleared (the pass is repeated on
        three limbs); if unchecked launches went before it, it is latched for range_ok() as well"""
        bad = self._take_word()
        self._latch |= bad and self._mark
        self._mark = False
        return not bad

    def range_ok(self):
        """the CALLER's read: True iff no two-limb launch on this workspace since the last call reported an activation outside
        float16's range that the caller has not been told about -- the word, or a report latched by passed().  Clears all of it.
        One host sync, which waits for the current stream ONLY: after launches or graph replays on another stream, wait for
        that stream first."""
        bad = self._take_word() or self._latch
        self._latch = self._mark = False
        return not bad

    def reset(self):
        """the ticket words back to zero (after a failed or aborted launch they may be left non-zero).  Never the status word:
        a report outlives the failure"""
        self._tickets.zero_()


_X3_WS = {}


def _x3_workspace(device):
    """the workspace of the current context: the one the enclosing f32_form block names, else the CURRENT stream's on `device`
    (allocated at the stream's first split-precision launch -- a warm-up pass before a HIP-graph capture)"""
    ws = _F32_CTX.get()[1]
    if ws is not None:
        return ws
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _X3_WS.get(key)
    if ws is None:
        ws = X3Workspace(device)
        _X3_WS[key] = ws
    return ws


# form -> entry-point suffix, the name a weight's limb planes are derived under, their splitter, and how the derived value reads
# as (planes, extra arguments ahead of the workspace's)
_F32_FORMS = {
    'exact': ('f32', None, None, None),
    'x3': ('x3', 'x3', split_bf16x3, lambda planes: (planes, ())),
    'x2': ('x2', 'x2', split_f16x2, lambda planes_exp: (planes_exp[0], (planes_exp[1],))),
}


def _f32_sym(pattern, w, holder=None):
    """(workspace, entry point, weight pointer, extra arguments before the stream) of a float32 layer in the current form:
    `pattern` % the form's suffix; the workspace is the one the launch is handed (in `extra`), None for 'exact'.
    The limb planes are derived FROM and kept ON the tensor object the caller passed (`holder`: the layer's
    parameter, or a module's derived concatenation; `w` itself when None) until that tensor is modified (derived.py: they live
    exactly as long as the weight they belong to -- no global cache that could outlive or be cleared under a captured HIP
    graph); `w`, the holder's contiguous float32 view, is read only when they are built.  (split_f16x2 reads its exponent from
    the weights -- one host synchronisation per weight tensor, at its first use: a warm-up pass before a HIP-graph capture, as
    for the workspace)"""
    sfx, name, split, read = _F32_FORMS[_F32_CTX.get()[0]]
    if name is None:
        return None, pattern % sfx, L.dptr(w), ()
    holder = w if holder is None else holder
    planes, extra = read(derived(holder, name, (holder,), lambda _: split(w)))
    ws = _x3_workspace(w.device)
    return ws, pattern % sfx, C.c_void_p(planes.data_ptr()), extra + ws.args()


def _f32_call(ws, sym, *args):
    """L.call for a dense layer (`ws`: the X3Workspace the launch was handed, None for 'exact' and float16); a split-precision
    launch that FAILS may leave that workspace's tickets non-zero: reset them"""
    try:
        L.call(sym, *args)
    except L.OdetError:
        if ws is not None:
            ws.reset()
        raise
