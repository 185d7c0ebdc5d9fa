// FPN neck, top-down merge: P_k = 0.5 * resize_bilinear(P_{k+1}, size(C_k)) + 0.5 * lateral(C_k)
// (reference model/fpn/resnet_fpn.py:385-398: tf.image.resize_bilinear of TF 1.x, align_corners=False,
// then keras Add of the two halves).  SURVEY 8(f) rank 3 -- the one part of the neck that is not a dense
// contraction: HBM-bound (lateral in, P_k out; the coarse map is 1/4 of the size and stays in L2), NHWC so a
// pixel's C channels are one coalesced segment.  Same float32 operation order as the TF kernel
// (resize_bilinear_op.cc): scale = in / out; src = dst * scale; lo = floor; hi = min(lo + 1, in - 1);
// top = tl + (tr - tl) * xl; bot = bl + (br - bl) * xl; up = top + (bot - top) * yl; out = up*0.5 + lat*0.5.
#include <hip/hip_fp16.h>

#include "grad_elementwise.h"

typedef uint32_t neck_u4 __attribute__((ext_vector_type(4)));   // 16 B, the type the non-temporal builtins take

template <typename FT>
struct NeckVec;
template <>
struct NeckVec<float> {                 // 4 channels = 16 B per lane
  static constexpr int N = 4;
  typedef float4 raw;
  static __device__ __forceinline__ void unpack(const raw& r, float (&f)[8]) { f[0] = r.x; f[1] = r.y; f[2] = r.z; f[3] = r.w; }
  static __device__ __forceinline__ raw pack(const float (&f)[8]) { return make_float4(f[0], f[1], f[2], f[3]); }
};
template <>
struct NeckVec<__half> {                // 8 channels = 16 B per lane
  static constexpr int N = 8;
  typedef uint4 raw;
  static __device__ __forceinline__ void unpack(const raw& r, float (&f)[8]) {
    const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float2 t = __half22float2(*reinterpret_cast<const __half2*>(&w[i]));
      f[2 * i] = t.x; f[2 * i + 1] = t.y;
    }
  }
  static __device__ __forceinline__ raw pack(const float (&f)[8]) {
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const __half2 t = __floats2half2_rn(f[2 * i], f[2 * i + 1]);
      w[i] = *reinterpret_cast<const uint32_t*>(&t);
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
  }
};

struct NeckParams {
  const void* top; const void* lat; void* out;
  int h, w, H, W, C;            // coarse map h x w, fine map H x W
  int vec_per_px;               // C / N
  long long total;              // B * H * W * vec_per_px
  float ys, xs;                 // h / H, w / W (float32, as TF computes them)
};

template <typename FT>
__global__ void __launch_bounds__(256) k_fpn_topdown_merge(NeckParams p) {
  typedef NeckVec<FT> V;
  typedef typename V::raw raw;
  const raw* __restrict__ top = reinterpret_cast<const raw*>(p.top);
  const raw* __restrict__ lat = reinterpret_cast<const raw*>(p.lat);
  raw* __restrict__ out = reinterpret_cast<raw*>(p.out);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < p.total; i += (long long)gridDim.x * 256) {
    const int v = (int)(i % p.vec_per_px);
    long long px = i / p.vec_per_px;
    const int x = (int)(px % p.W);
    px /= p.W;
    const int y = (int)(px % p.H);
    const int b = (int)(px / p.H);
    const float fy = (float)y * p.ys, fx = (float)x * p.xs;
    const float y0f = floorf(fy), x0f = floorf(fx);
    const int y0 = (int)y0f, x0 = (int)x0f;
    const int y1 = min(y0 + 1, p.h - 1), x1 = min(x0 + 1, p.w - 1);
    const float yl = fy - y0f, xl = fx - x0f;
    const long long tb = (long long)b * p.h * p.w;
    float tl[8], tr[8], bl[8], br[8], la[8], o[8];
    V::unpack(top[(tb + (long long)y0 * p.w + x0) * p.vec_per_px + v], tl);
    V::unpack(top[(tb + (long long)y0 * p.w + x1) * p.vec_per_px + v], tr);
    V::unpack(top[(tb + (long long)y1 * p.w + x0) * p.vec_per_px + v], bl);
    V::unpack(top[(tb + (long long)y1 * p.w + x1) * p.vec_per_px + v], br);
    {                                                        // the lateral map is streamed once
      const neck_u4 t = __builtin_nontemporal_load(reinterpret_cast<const neck_u4*>(&lat[i]));
      raw r;
      __builtin_memcpy(&r, &t, 16);
      V::unpack(r, la);
    }
#pragma unroll
    for (int k = 0; k < V::N; ++k) {
      const float t = tl[k] + (tr[k] - tl[k]) * xl;
      const float bt = bl[k] + (br[k] - bl[k]) * xl;
      const float up = t + (bt - t) * yl;
      o[k] = up * 0.5f + la[k] * 0.5f;
    }
    out[i] = V::pack(o);
  }
}

extern "C" int odet_fpn_topdown_merge(const void* top, int h, int w, const void* lateral, int H, int W, int B,
                                      int C, void* out, int f16, odet_stream_t stream) {
  ODET_REQUIRE(top && lateral && out, "odet_fpn_topdown_merge: null pointer");
  ODET_REQUIRE(h > 0 && w > 0 && H > 0 && W > 0 && B >= 0 && C > 0, "odet_fpn_topdown_merge: bad sizes");
  const int n = f16 ? 8 : 4;
  ODET_REQUIRE(C % n == 0, "odet_fpn_topdown_merge: C must be a multiple of %d (got %d)", n, C);
  if (B == 0) return ODET_OK;
  NeckParams p;
  p.top = top; p.lat = lateral; p.out = out;
  p.h = h; p.w = w; p.H = H; p.W = W; p.C = C;
  p.vec_per_px = C / n;
  p.total = (long long)B * H * W * p.vec_per_px;
  p.ys = (float)h / (float)H;
  p.xs = (float)w / (float)W;
  const int grid = ge_grid(p.total);
  if (f16)
    hipLaunchKernelGGL(k_fpn_topdown_merge<__half>, dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
  else
    hipLaunchKernelGGL(k_fpn_topdown_merge<float>, dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
  ODET_LAUNCH_CHECK();
  return ODET_OK;
}

// ---- the top-down merge's backward, float32 ----------------------------------------------------------------------------------
// The transpose of the resize above as a GATHER per coarse pixel (include/odet.h states the order of sums): a lane owns four
// channels of one coarse pixel (Y, X), walks the fine rows y with floor(y * ys) in {Y - 1, Y} and the fine columns likewise --
// contiguous ranges, since floor((float)y * ys) is monotone in y -- in ascending (y, x), and adds the taps of each fine pixel
// that land on (Y, X) in the order TL, TR, BL, BR onto an accumulator that starts at +0.  No atomics, every element of d_top
// written once.  A fine row (column) whose only tap on Y (X) is its bottom (right) one with weight exactly 0 is skipped: it
// would add (g * 0) * wx = +-0, which leaves every finite accumulator as it is (an accumulator that starts at +0 is never -0).
struct NeckBwdParams {
  const float4* fine; const float4* base; const float4* sub; float4* d_top;
  int h, w, H, W;               // coarse map h x w (d_top, base), fine map H x W
  int sw;                       // width of sub: ceil(w / 2)
  int vec_per_px;               // C / 4
  long long total;              // B * h * w * vec_per_px
  float ys, xs;                 // h / H, w / W: the forward's own float32 scales
  float out_scale;
};

// the first i in [0, n] with floorf((float)i * s) >= t (n when there is none): an estimate, then steps against the forward's
// own expression -- exact whatever the estimate's rounding, because the expression is monotone in i
static __device__ __forceinline__ int neck_first_at_least(int t, int n, float s) {
  if (t <= 0) return 0;
  int e = (int)fminf(ceilf((float)t / s), (float)n);
  while (e > 0 && floorf((float)(e - 1) * s) >= (float)t) --e;
  while (e < n && floorf((float)e * s) < (float)t) ++e;
  return e;
}

__global__ void __launch_bounds__(256) k_fpn_topdown_backward_f32(NeckBwdParams p) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < p.total; i += (long long)gridDim.x * 256) {
    const int v = (int)(i % p.vec_per_px);
    long long px = i / p.vec_per_px;
    const int X = (int)(px % p.w);
    px /= p.w;
    const int Y = (int)(px % p.h);
    const int b = (int)(px / p.h);
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (p.fine) {
      const int ylo = neck_first_at_least(Y - 1, p.H, p.ys), yhi = neck_first_at_least(Y + 1, p.H, p.ys);
      const int xlo = neck_first_at_least(X - 1, p.W, p.xs), xhi = neck_first_at_least(X + 1, p.W, p.xs);
      const float4* __restrict__ fb = p.fine + (long long)b * p.H * p.W * p.vec_per_px + v;
      for (int y = ylo; y < yhi; ++y) {
        const float fy = (float)y * p.ys;
        const float y0f = floorf(fy);
        const int y0 = (int)y0f, y1 = min(y0 + 1, p.h - 1);
        const float yl = fy - y0f;
        const bool top = y0 == Y, bot = y1 == Y;
        if (!top && yl == 0.0f) continue;
        const float wt = 1.0f - yl, wb = yl;
        for (int x = xlo; x < xhi; ++x) {
          const float fx = (float)x * p.xs;
          const float x0f = floorf(fx);
          const int x0 = (int)x0f, x1 = min(x0 + 1, p.w - 1);
          const float xl = fx - x0f;
          const bool left = x0 == X, right = x1 == X;
          if (!left && xl == 0.0f) continue;
          const float wl = 1.0f - xl, wr = xl;
          const float4 g4 = fb[((long long)y * p.W + x) * p.vec_per_px];
          const float g[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            if (top) {
              const float gy = g[k] * wt;
              if (left) acc[k] = acc[k] + gy * wl;
              if (right) acc[k] = acc[k] + gy * wr;
            }
            if (bot) {
              const float gy = g[k] * wb;
              if (left) acc[k] = acc[k] + gy * wl;
              if (right) acc[k] = acc[k] + gy * wr;
            }
          }
        }
      }
    }
    // base + sub + S, left to right; an absent term is skipped, not added as a zero
    float t[4];
    bool have = false;
    if (p.base) {                                            // streamed once
      const neck_u4 r = __builtin_nontemporal_load(reinterpret_cast<const neck_u4*>(&p.base[i]));
      __builtin_memcpy(t, &r, 16);
      have = true;
    }
    if (p.sub && !((Y | X) & 1)) {
      const float4 s4 = p.sub[(((long long)b * ((p.h + 1) / 2) + (Y >> 1)) * p.sw + (X >> 1)) * p.vec_per_px + v];
      const float s[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) t[k] = have ? t[k] + s[k] : s[k];
      have = true;
    }
    if (p.fine) {
#pragma unroll
      for (int k = 0; k < 4; ++k) t[k] = have ? t[k] + acc[k] : acc[k];
      have = true;
    }
    if (!have) t[0] = t[1] = t[2] = t[3] = 0.0f;
    p.d_top[i] = make_float4(p.out_scale * t[0], p.out_scale * t[1], p.out_scale * t[2], p.out_scale * t[3]);
  }
}

extern "C" int odet_fpn_topdown_backward_f32(const float* fine, int H, int W, const float* base, const float* sub,
                                             float out_scale, float* d_top, int h, int w, int B, int C, odet_stream_t stream) {
  const char* who = "odet_fpn_topdown_backward_f32";
  ODET_REQUIRE(d_top, "%s: null d_top", who);
  ODET_REQUIRE(fine || base || sub, "%s: at least one of fine, base and sub is needed", who);
  ODET_REQUIRE(h > 0 && w > 0, "%s: bad sizes (h %d, w %d)", who, h, w);
  GE_REQUIRE_NHWC(who, B, H, W, C, (uintptr_t)fine | (uintptr_t)base | (uintptr_t)sub | (uintptr_t)d_top);
  if (B == 0) return ODET_OK;
  NeckBwdParams p;
  p.fine = reinterpret_cast<const float4*>(fine);
  p.base = reinterpret_cast<const float4*>(base);
  p.sub = reinterpret_cast<const float4*>(sub);
  p.d_top = reinterpret_cast<float4*>(d_top);
  p.h = h; p.w = w; p.H = H; p.W = W;
  p.sw = (w + 1) / 2;
  p.vec_per_px = C / 4;
  p.total = (long long)B * h * w * p.vec_per_px;
  p.ys = (float)h / (float)H;
  p.xs = (float)w / (float)W;
  p.out_scale = out_scale;
  const int grid = ge_grid(p.total);
  hipLaunchKernelGGL(k_fpn_topdown_backward_f32, dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
  ODET_LAUNCH_CHECK();
  return ODET_OK;
}
