// Shared by the float32 forms of the implicit-GEMM convolution kernel: the exact-float32 matrix-instruction form
// (conv_f32.hip) and the split-precision form (conv_x3.hip: float32 operands as three bfloat16 limbs, six products per
// K-step on v_mfma_f32_16x16x32_bf16, float32 accumulation; or two float16 limbs, three products).  All take ConvF32Params,
// leave a lane with pixel l15 of every 16-pixel tile and channels c0 + 16 t .. + 3 of tile t, and finish with the same epilogue.
// The host side is shared too: the launch plan below the epilogue checks the arguments, fills ConvF32Params and computes the
// launch geometry once for all forms; the two files keep their kernels, tile lists, tile picks, LDS sizes and dispatch.
#ifndef ODET_CONV_F32_COMMON_H_
#define ODET_CONV_F32_COMMON_H_
#include <hip/hip_runtime.h>

#include "odet_internal.h"

typedef float c3f4 __attribute__((ext_vector_type(4)));

struct ConvF32Params {
  const float* x[ODET_MAX_LEVELS]; float* y[ODET_MAX_LEVELS];
  const float* w; const float* bias;
  long long M[ODET_MAX_LEVELS];
  int H[ODET_MAX_LEVELS], W[ODET_MAX_LEVELS];
  long long tile_start[ODET_MAX_LEVELS + 1];
  int num_levels, cin, cout, relu;
  int tiles_n;
  // pointwise form (TAPS == 1, one map): output row m = (image, yo, xo) of a Ho x Wo map reads input pixel (yo, xo) * stride
  int stride, Ho, Wo;
  long long Min;
  const float* res;               // + shortcut [M][cout]
  const float* top; int th, tw; float tys, txs;   // or the FPN top-down merge: 0.5 * resize(top) + 0.5 * (conv + bias)
  const float* x2; int cin2, k1steps; long long Min2;   // or two sources along K ([x | x2(::stride)], weights concatenated)
  // split-K (conv_x3.hip only; 0 / 1 = off): ksplit consecutive workgroups share an output tile, each takes a contiguous part
  // of the K-steps and leaves its float32 partial tile in `part`; the one that draws the last of the tile's tickets adds the
  // parts in their fixed order 0 .. ksplit - 1 and runs the epilogue (deterministic; exact on integers)
  int ksplit; float* part; unsigned* ticket;
  float acc_scale;                // conv_x3.hip's two-limb float16 form: 2^-w_exp (the weight planes hold w * 2^w_exp); else unused
  // conv_x3.hip's two-limb form: the RANGE status word (nullable).  An activation beyond float16's range becomes an infinite
  // limb, and every product with it is infinite or NaN: every sum it enters is non-finite BEFORE bias / shortcut / ReLU, whatever
  // the weights' signs -- the epilogue ORs 1 into the word when it sees one (a wave ballot, then at most one atomic per wave)
  unsigned* status;
};

// bias (+ shortcut | FPN top-down merge) (+ ReLU) and the stores of a wave's MT x 4 accumulator tiles
template <int MT, int TAPS>
__device__ __forceinline__ void conv_f32_epilogue(const ConvF32Params& p, c3f4 (&acc)[MT][4], long long tile_m, int TM, int TN,
                                                  int wm, int wn, int tn, int l15, int lq, int lv, long long M, int cout) {
  // lane = pixel l15 of every pixel tile; tile t of the wave's 64-channel group: channels c0 + 16 t .. + 3
  const int c0 = tn * TN + wn * 64 + lq * 4;
  if (p.status) {
    // the raw sums, before anything can hide a non-finite one (ReLU maps -inf to 0): rows past M were computed from zeros
    bool bad = false;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) bad |= !(__builtin_fabsf(acc[mt][t][j]) <= 3.4028234663852886e38f);
    const unsigned long long any = __builtin_amdgcn_ballot_w64(bad);
    if (any != 0ull && (int)(threadIdx.x & 63) == (int)__builtin_ctzll(any)) atomicOr(p.status, 1u);
  }
  c3f4 bv[4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
    bv[t] = p.bias ? *reinterpret_cast<const c3f4*>(p.bias + c0 + 16 * t) : (c3f4){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const long long m = tile_m * TM + wm * 16 * MT + mt * 16 + l15;
    if (m < M) {
      float* dst = p.y[lv] + m * cout + c0;
      if constexpr (TAPS == 1) {
        if (p.top) {
          // the FPN top-down merge (neck.hip's arithmetic and operation order, float32 throughout: bit-identical to
          // odet_fpn_topdown_merge applied to the convolution's float32 result)
          const long long opx = (long long)p.Ho * p.Wo;
          const long long img = m / opx;
          const int rem = (int)(m - img * opx);
          const int yy = rem / p.Wo, xx = rem - yy * p.Wo;
          const float fy = (float)yy * p.tys, fx = (float)xx * p.txs;
          const float y0f = floorf(fy), x0f = floorf(fx);
          const int y0 = (int)y0f, x0 = (int)x0f;
          const int y1 = min(y0 + 1, p.th - 1), x1 = min(x0 + 1, p.tw - 1);
          const float yl = fy - y0f, xl = fx - x0f;
          const float* tb = p.top + (img * p.th * p.tw) * cout + c0;
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const c3f4 a = *reinterpret_cast<const c3f4*>(tb + ((long long)y0 * p.tw + x0) * cout + 16 * t);
            const c3f4 b = *reinterpret_cast<const c3f4*>(tb + ((long long)y0 * p.tw + x1) * cout + 16 * t);
            const c3f4 c = *reinterpret_cast<const c3f4*>(tb + ((long long)y1 * p.tw + x0) * cout + 16 * t);
            const c3f4 d = *reinterpret_cast<const c3f4*>(tb + ((long long)y1 * p.tw + x1) * cout + 16 * t);
            c3f4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const float lat = acc[mt][t][j] + bv[t][j];
              const float tp = a[j] + (b[j] - a[j]) * xl;
              const float bt = c[j] + (d[j] - c[j]) * xl;
              const float up = tp + (bt - tp) * yl;
              o[j] = up * 0.5f + lat * 0.5f;
            }
            *reinterpret_cast<c3f4*>(dst + 16 * t) = o;
          }
          continue;
        }
      }
      const bool has_res = TAPS == 1 && p.res != nullptr;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        c3f4 o, r = (c3f4){0.0f, 0.0f, 0.0f, 0.0f};
        if (has_res) r = *reinterpret_cast<const c3f4*>(p.res + m * cout + c0 + 16 * t);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float v = acc[mt][t][j] + bv[t][j];
          if (has_res) v += r[j];
          if (p.relu) v = v < 0.0f ? 0.0f : v;
          o[j] = v;
        }
        *reinterpret_cast<c3f4*>(dst + 16 * t) = o;
      }
    }
  }
}

// ---- host side: the launch plan ---------------------------------------------------------------------------------------------
// A launch function of either file reads: shared plan (arguments checked, ConvF32Params filled) -> the kernels' LDS limit ->
// the form's tile pick -> conv_f32_plan_tiles -> the form's extras (split-K, status word) -> launch.
#define CONV_F32_BK 32            // float32 input channels per K-step (128 bytes of a pixel's row), all forms

// The checks on which the forms differ for no reason of design: INHERITED, not designed.  Each form keeps its own value until
// a change of behaviour unifies them on their merits.
struct ConvF32Rules {
  unsigned long long weight_bytes;  // inherited: bytes per weight in the "weights too large" bound, 4 (exact) / 6 (split, x2 too)
  long long max_blocks;             // inherited: workgroups of a launch, below 1 << 31 (exact) / 1 << 28 (split)
  bool align3x3;                    // inherited: only the split forms' 3x3 path asks for 16-byte aligned weights, bias and maps
};

static void conv_f32_defaults(ConvF32Params* p) {
  p->stride = 1; p->Ho = p->Wo = 0; p->Min = 0; p->res = nullptr; p->top = nullptr; p->th = p->tw = 0; p->tys = p->txs = 0.0f;
  p->x2 = nullptr; p->cin2 = 0; p->k1steps = 0; p->Min2 = 0;
  p->ksplit = 0; p->part = nullptr; p->ticket = nullptr; p->acc_scale = 1.0f; p->status = nullptr;
}

// 3x3 convolution with shared weights over `num_levels` maps: everything of the plan that does not depend on the tile
static int conv_f32_plan_levels(const char* who, const ConvF32Rules& r, const odet_conv_level_t* levels, int num_levels,
                                const void* w, const void* bias, int batch, int cin, int cout, int relu, ConvF32Params* p) {
  ODET_REQUIRE(levels && w, "%s: null pointer", who);
  ODET_REQUIRE(num_levels >= 1 && num_levels <= ODET_MAX_LEVELS, "%s: num_levels %d out of range", who, num_levels);
  ODET_REQUIRE(batch > 0, "%s: bad batch", who);
  ODET_REQUIRE(cin > 0 && cin % CONV_F32_BK == 0, "%s: cin %d must be a multiple of %d", who, cin, CONV_F32_BK);
  ODET_REQUIRE(cout > 0 && cout % 64 == 0, "%s: cout %d must be a multiple of 64", who, cout);
  ODET_REQUIRE((unsigned long long)cout * 9ull * cin * r.weight_bytes < 0x7FFFFFFFull, "%s: weights too large", who);
  ODET_REQUIRE(!r.align3x3 || ((uintptr_t)w % 16 == 0 && (uintptr_t)bias % 16 == 0), "%s: pointers must be 16-byte aligned", who);
  conv_f32_defaults(p);
  for (int l = 0; l < ODET_MAX_LEVELS; ++l) {
    const odet_conv_level_t& L = levels[l < num_levels ? l : 0];
    ODET_REQUIRE(L.x && L.y && L.H > 0 && L.W > 0, "%s: bad level %d", who, l);
    ODET_REQUIRE(!r.align3x3 || ((uintptr_t)L.x | (uintptr_t)L.y) % 16 == 0, "%s: maps must be 16-byte aligned", who);
    const long long M = (long long)batch * L.H * L.W;
    ODET_REQUIRE((unsigned long long)M * cin * 4ull + 2ull * (L.W + 1) * cin * 4ull < 0xFFFFFFF0ull,
                 "%s: level %d input larger than 4 GiB", who, l);
    p->x[l] = (const float*)L.x; p->y[l] = (float*)L.y; p->M[l] = M; p->H[l] = L.H; p->W[l] = L.W;
  }
  p->w = (const float*)w; p->bias = (const float*)bias;
  p->num_levels = num_levels; p->cin = cin; p->cout = cout; p->relu = relu ? 1 : 0;
  return ODET_OK;
}

// what a pointwise launch adds to the contraction: a shortcut, or the FPN top-down merge, or a second source along K
struct ConvF32PwEpilogue { const void* res; const void* top; int th, tw; const void* x2; int cin2; };

// 1x1 convolution (stride 1 or 2) / dense layer on one map; the caller checks `cin` first (the forms' rules differ)
static int conv_f32_plan_pointwise(const char* who, const ConvF32Rules& r, const void* x, const void* w, const void* bias, void* y,
                                   int batch, int H, int W, int stride, int cin, int cout, int relu, const ConvF32PwEpilogue& epi,
                                   ConvF32Params* p) {
  ODET_REQUIRE(x && w && y, "%s: null pointer", who);
  ODET_REQUIRE(batch > 0 && H > 0 && W > 0 && (stride == 1 || stride == 2), "%s: bad shape", who);
  ODET_REQUIRE(cout > 0 && cout % 64 == 0, "%s: cout %d must be a multiple of 64", who, cout);
  ODET_REQUIRE(((uintptr_t)x | (uintptr_t)w | (uintptr_t)y | (uintptr_t)bias | (uintptr_t)epi.res | (uintptr_t)epi.top |
                (uintptr_t)epi.x2) % 16 == 0, "%s: pointers must be 16-byte aligned", who);
  ODET_REQUIRE(!(epi.res && epi.top), "%s: shortcut and top-down merge exclude each other", who);
  ODET_REQUIRE(!epi.top || (stride == 1 && epi.th > 0 && epi.tw > 0 && !relu), "%s: bad merge arguments", who);
  const int Ho = (H + stride - 1) / stride, Wo = (W + stride - 1) / stride;
  const int cin2 = epi.x2 ? epi.cin2 : 0;
  const long long M = (long long)batch * Ho * Wo, Min2 = (long long)batch * H * W;
  const long long Min = epi.x2 ? M : Min2;
  ODET_REQUIRE((unsigned long long)Min * cin * 4ull < 0xFFFFFFF0ull, "%s: input larger than 4 GiB", who);
  ODET_REQUIRE(!epi.x2 || (cin2 > 0 && cin2 % CONV_F32_BK == 0 && (unsigned long long)Min2 * cin2 * 4ull < 0xFFFFFFF0ull),
               "%s: bad second source", who);
  ODET_REQUIRE((unsigned long long)cout * (cin + cin2) * r.weight_bytes < 0x7FFFFFFFull, "%s: weights too large", who);
  conv_f32_defaults(p);
  for (int l = 0; l < ODET_MAX_LEVELS; ++l) {
    p->x[l] = (const float*)x; p->y[l] = (float*)y; p->M[l] = M; p->H[l] = H; p->W[l] = W;
  }
  p->res = (const float*)epi.res;
  p->top = (const float*)epi.top; p->th = epi.th; p->tw = epi.tw;
  p->tys = epi.top ? (float)epi.th / (float)Ho : 0.0f;
  p->txs = epi.top ? (float)epi.tw / (float)Wo : 0.0f;
  p->stride = stride; p->Ho = Ho; p->Wo = Wo; p->Min = Min;
  p->x2 = (const float*)epi.x2; p->cin2 = cin2; p->k1steps = cin / CONV_F32_BK; p->Min2 = Min2;
  p->w = (const float*)w; p->bias = (const float*)bias;
  p->num_levels = 1; p->cin = cin; p->cout = cout; p->relu = relu ? 1 : 0;
  return ODET_OK;
}

// the tile-dependent rest of either plan, for tiles of `tile_pixels` pixels x 64 * wn channels: every level's first slab, the
// channel tiles, and the workgroup count -- slabs padded to whole groups of 8 (the kernels' XCD-aware order)
static int conv_f32_plan_tiles(const char* who, const ConvF32Rules& r, int tile_pixels, int wn, ConvF32Params* p, long long* blocks) {
  long long total = 0;
  for (int l = 0; l < ODET_MAX_LEVELS; ++l) {
    p->tile_start[l] = total;
    if (l < p->num_levels) total += (p->M[l] + tile_pixels - 1) / tile_pixels;
  }
  p->tile_start[ODET_MAX_LEVELS] = total;
  p->tiles_n = p->cout / (64 * wn);
  *blocks = (total + 7) / 8 * 8 * p->tiles_n;
  ODET_REQUIRE(*blocks < r.max_blocks, "%s: too many workgroups", who);
  return ODET_OK;
}

// more than 64 KB of dynamic LDS has to be allowed per kernel, once per device
static hipError_t conv_f32_raise_lds_limit(OdetPerDeviceOnce* once, const void* const* kernels, size_t count, int bytes) {
  return once->run([=] {
    hipError_t rc = hipSuccess;
    for (size_t i = 0; i < count; ++i) {
      const hipError_t e = hipFuncSetAttribute(kernels[i], hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
      if (e != hipSuccess) rc = e;
    }
    return rc;
  });
}

#endif  // ODET_CONV_F32_COMMON_H_
