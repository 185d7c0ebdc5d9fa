"""What tests/test_grad_x3_host.py and tests/test_grad_x3_gpu.py share: the grids of the exact-form gradient tests (imported, not
copied), the extra shapes that reach the split-precision launcher's remaining instantiations, the plan queries, and the data of the
split-precision backward (csrc/grad_gemm.h: dg_tile_x3) -- integer data, the three limb-sensitive kinds and the dropped-product
witness -- for the ONE contraction all three entry points are, C[n][m] = sum_k A[k][m] * B[k][n]:

            A [K][M]               B [K][N]                   C [N][M]
    wgrad   x  [rows][cin]         dz [rows][cout]            dw [cout][cin]
    dgrad   w  [cout][cin]         dz^T (dz [rows][cout])     dx [rows][cin]
    conv    x shifted by the tap   dz [pixels][cout]          dw [cout][(tap, cin)]

All data is float64 on the CPU, exactly representable in float32."""
import ctypes as C
import os
import re

import numpy as np
import torch

import conv_tile_cases as ct
import exact_data as ed
from test_conv_grad_gpu import CHANNELS, HEAD_PYRAMID, PYRAMID, SINGLE
from test_conv_grad_gpu import RANDOM as CONV_RANDOM
from test_dense_grad_gpu import GRID, HEAD
from test_dense_grad_gpu import RANDOM as DENSE_RANDOM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -23

# ---- shapes ---------------------------------------------------------------------------------------------------------------------
# dense (rows, cin, cout).  The 128-edge tile needs 256 tiles of 128 x 128: one row of 32768 input channels reaches it for dgrad
# (N-major B) and wgrad (K-major B) alike; it never splits (a split needs at most 128 tiles)
DENSE_WIDE = (1, 32768, 64)
DENSE_SHAPES = GRID + HEAD + [DENSE_WIDE]
# what the launcher has: (kind, tile edge, split?) -> a shape of DENSE_SHAPES that must reach it
DENSE_REACH = {('dgrad', 64, False): (5, 96, 64), ('dgrad', 64, True): (256, 1024, 1024), ('dgrad', 128, False): DENSE_WIDE,
               ('wgrad', 64, False): (130, 160, 192), ('wgrad', 64, True): (256, 1024, 128), ('wgrad', 128, False): DENSE_WIDE}
# conv (maps, batch, cin, cout); the 128-edge tile needs both channel counts multiples of 128: the head's 256 -> 512 cuts its
# contraction, one pixel at 128 -> 128 does not
CONV_CASES = [([s], b, ci, co) for s in SINGLE for b in (1, 2) for ci, co in CHANNELS] \
    + [(PYRAMID, 2, ci, co) for ci, co in CHANNELS] + [(HEAD_PYRAMID, 1, 256, 512), ([(1, 1)], 1, 128, 128)]
CONV_REACH = {(64, False): ([(3, 7)], 2, 96, 64), (64, True): ([(17, 40)], 1, 64, 64), (128, False): ([(1, 1)], 1, 128, 128),
              (128, True): (HEAD_PYRAMID, 1, 256, 512)}


def lib():
    from tf_eager_object_detection_amd import _lib
    return _lib.lib()


def levels(maps, ptrs=(None, None, None)):
    from tf_eager_object_detection_amd import _lib
    lv = (_lib.OdetConvGradLevel * max(1, len(maps)))()
    for i, (h, w) in enumerate(maps):
        lv[i].x, lv[i].dy, lv[i].y_relu, lv[i].H, lv[i].W = ptrs[0], ptrs[1], ptrs[2], h, w
    return lv


def dense_plan(kind, shape):
    """(tile edge, parts) of the split-precision launch of a dense shape, from the library's plan query"""
    t, p = C.c_int(-1), C.c_int(-1)
    rc = lib().odet_dense_grad_x3_plan(1 if kind == 'wgrad' else 0, *shape, C.byref(t), C.byref(p))
    assert rc == 0, lib().odet_last_error()
    return t.value, p.value


def conv_plan(case):
    maps, batch, cin, cout = case
    t, p = C.c_int(-1), C.c_int(-1)
    rc = lib().odet_conv3x3_wgrad_x3_plan(levels(maps), len(maps), batch, cin, cout, C.byref(t), C.byref(p))
    assert rc == 0, lib().odet_last_error()
    return t.value, p.value


def kept_products():
    """(kept, dropped) limb products (i, j) = A limb i times B limb j, READ FROM THE HEADER of dg_tile_x3 (csrc/grad_gemm.h), in
    the notation conv_tile_cases.kept_products reads from csrc/conv_x3.hip"""
    src = open(os.path.join(ROOT, 'tf_eager_object_detection_amd', 'csrc', 'grad_gemm.h')).read()
    m = re.search(r'a \. b\s+~\s+(.*?)\(dropped:(.*?)<=', src, flags=re.S)
    assert m, 'the header of dg_tile_x3 no longer states its limb products'
    pairs = lambda s: [(int(i), int(j)) for i, j in re.findall(r'a(\d) b(\d)', s)]
    kept, dropped = pairs(m.group(1)), pairs(m.group(2))
    assert len(set(kept)) == len(kept) == 6 and len(dropped) == 3
    assert sorted(kept + dropped) == [(i, j) for i in (1, 2, 3) for j in (1, 2, 3)]
    return kept, dropped


def limb_products(a, b):
    """{(i, j): sum_k A_i[k][m] B_j[k][n] as [N][M]} over the three bfloat16 limbs of A [K][M] and B [K][N], and the contraction of
    the limbs' absolute values (what bounds every partial sum of every order)"""
    al, bl = ct.split_limbs(a, 3), ct.split_limbs(b, 3)
    assert torch.equal(sum(al), a) and torch.equal(sum(bl), b)
    prods = {(i + 1, j + 1): bl[j].t() @ al[i] for i in range(3) for j in range(3)}
    return prods, sum(t.abs() for t in bl).t() @ sum(t.abs() for t in al)


def limb_abs_total(a, b):
    """the contraction of the limbs' absolute values alone (limb_products' second result, one product instead of ten)"""
    return sum(t.abs() for t in ct.split_limbs(b, 3)).t() @ sum(t.abs() for t in ct.split_limbs(a, 3))


def kept_value(a, b):
    """what the six kept products give, and the proof that it is exact in float32 at every partial sum in any order (every limb
    product is a multiple of the quantum found here)"""
    prods, abs_total = limb_products(a, b)
    kept, _ = kept_products()
    return sum(prods[p] for p in kept), abs_total


# ---- data -----------------------------------------------------------------------------------------------------------------------
GATES = (0.0, -0.0, -1.0, 2.0 ** -120, 3.0, -2.0 ** -120)          # y_relu / x_relu values: only the 4th and 5th open the gate


def gates(g, shape):
    idx = torch.randint(0, len(GATES), tuple(shape), generator=g.g)
    return torch.tensor(GATES, dtype=torch.float64)[idx]


def integer_operands(g, K, M, N):
    """integers that live in the top limb alone (|v| <= 8: bfloat16 holds them); partial sums below 2^24"""
    a, b = g.ints((K, M), 8), g.ints((K, N), 4)
    ed.prove_f32_exact(b.abs().t() @ a.abs(), 1.0, integers=(a, b))
    return a, b, 1.0


LIMB_KINDS = ct.LIMB_KINDS[3]                                # 'x_limbs': A spans three limbs and B one; 'w_limbs': the reverse; two x two


def limb_operands(g, kind, K, M, N):
    """A [K][M], B [K][N] (four non-zeros per column n, so an output is a sum of four products) and their quantum, proven exact at
    every partial sum of the LIMB products in any order"""
    x, w, q = ct.limb_operands(g, kind, 3, (M, K), N, K)
    a, b = x.t().contiguous(), w.t().contiguous()
    ed.prove_f32_exact(limb_abs_total(a, b), q, quanta=(a, b))           # (limbs and limb products are multiples of q like the operands)
    return a, b, q


def witness_operands(K, M, N, k0=0, k1=4):
    """The dropped-product witness in every output element: k0 holds a = -1, b = 1 + 2^-8 + 2^-17; k1 holds a = 1 + 2^-9,
    b = 1 + 2^-9 + 2^-18; all other k are zero.  The six kept products sum to 0 (every partial sum a multiple of 2^-18 below 4);
    the dropped a2 b3 = 2^-27 is what a chain of fused float32 multiply-adds in ascending k returns.
    -> (A [K][M], B [K][N], kept value, exact-form value)"""
    a, b = torch.zeros(K, M, dtype=torch.float64), torch.zeros(K, N, dtype=torch.float64)
    a[k0], b[k0] = -1.0, 1 + 2.0 ** -8 + 2.0 ** -17
    a[k1], b[k1] = 1 + 2.0 ** -9, 1 + 2.0 ** -9 + 2.0 ** -18
    return a, b, 0.0, 2.0 ** -27


def fused_chain(a, b):
    """sum_k a[k] b[k] for one output element as the exact form adds it: ascending k, one float32 rounding per fused step"""
    acc = np.float32(0.0)
    for x, y in zip(a.tolist(), b.tolist()):
        acc = np.float32(float(acc) + x * y)                  # (float64 holds acc + x y exactly for this data: one rounding)
    return float(acc)


# ---- the three entry points on (A, B) ------------------------------------------------------------------------------------------
def f32(t):
    v = t.float()
    assert torch.equal(v.double(), t), 'the data must be float32 values'
    return v.contiguous()


def conv_pixels(maps, batch):
    return batch * sum(h * w for h, w in maps)


def conv_maps(a_pix, maps, batch):
    """[pixels, C] rows numbered as the kernel numbers them (level, image, row, column) -> one [B,H,W,C] map per level"""
    out, off = [], 0
    for h, w in maps:
        n = batch * h * w
        out.append(a_pix[off:off + n].reshape(batch, h, w, -1).contiguous())
        off += n
    return out


def conv_wgrad_f64(xs, dzs):
    """dw [cout,3,3,cin] = sum over levels and pixels of dz[b,y,x,co] * x[b,y+ky-1,x+kx-1,ci], float64"""
    cout, cin = dzs[0].shape[3], xs[0].shape[3]
    dw = torch.zeros(cout, 3, 3, cin, dtype=torch.float64)
    for x, dz in zip(xs, dzs):
        H, W = x.shape[1:3]
        xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
        for ky in range(3):
            for kx in range(3):
                dw[:, ky, kx, :] += torch.einsum('bhwo,bhwi->oi', dz, xp[:, ky:ky + H, kx:kx + W, :])
    return dw
