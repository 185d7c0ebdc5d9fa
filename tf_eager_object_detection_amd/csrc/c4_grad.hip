// The one operator of the ResNet-C4 training graph (reference model/faster_rcnn/resnet_faster_rcnn.py) that the other backward
// passes do not have: GlobalAveragePooling2D between the conv5 stack and the two Dense layers (:168), forward and backward.
//   odet_global_avg_pool_f32            out[r,c] = (x[r,0,c] + x[r,1,c] + ... + x[r,hw-1,c]) / (float)hw: the float32 sum over the
//                                       pixels in the order p = 0 .. hw-1, every add rounded, started from x[r,0,c] itself; then one
//                                       IEEE division
//   odet_global_avg_pool_backward_f32   dx[r,p,c] = g[r,c] / (float)hw for every p: TF's _MeanGrad, a broadcast and a true division
// HBM-bound streams in block_grad.hip's layout: a lane owns four channels (16 bytes), a wave 1 KiB of consecutive channels of one
// pixel.  The forward's lane walks its row's pixels serially -- the order IS the result -- through two register sets of GAP_DEPTH
// pixels, one being added while the other loads, so that one workgroup per CU (the head's own shape: 128 x 49 x 2048 is 256
// workgroups) keeps 32 to 64 KiB in flight; x is read once (non-temporal loads).  The backward's lane divides its four channels
// of g once and stores them to GAP_BWD_PIXELS consecutive pixels; g is re-read from L2.  No LDS, no atomics, no cross-lane
// traffic; every output element is written exactly once.
#include "grad_elementwise.h"

#define GAP_DEPTH 8          // pixels per register set of the forward
#define GAP_BWD_PIXELS 8     // pixels per lane of the backward

struct GapParams {
  const float4* x; float4* out;
  int hw;
  int vec_per_px;               // C / 4
  long long total;              // lanes: rows * vec_per_px forward; rows * ceil(hw / GAP_BWD_PIXELS) * vec_per_px backward
};

// N pixels' vectors of one lane, the loads issued together
template <int N>
static __device__ __forceinline__ void gap_load(float4 (&v)[N], const float4* x, long long stride) {
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = ge_stream(x + k * stride);
}

// s + v[0] + v[1] + ... in that order
template <int N>
static __device__ __forceinline__ void gap_add(const float4 (&v)[N], float s[4]) {
#pragma unroll
  for (int k = 0; k < N; ++k) {
    s[0] += v[k].x; s[1] += v[k].y; s[2] += v[k].z; s[3] += v[k].w;
  }
}

__global__ void __launch_bounds__(256) k_global_avg_pool_f32(GapParams p) {
  const float n = (float)p.hw;
  const long long stride = p.vec_per_px;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < p.total; i += (long long)gridDim.x * 256) {
    const long long r = i / p.vec_per_px;
    const float4* x = p.x + (r * p.hw * p.vec_per_px + i % p.vec_per_px);
    // -0 + a == a for every a, -0 and +0 included: the sum starts from the first pixel itself
    float s[4] = {-0.0f, -0.0f, -0.0f, -0.0f};
    int px = 0;
    if (p.hw >= 2 * GAP_DEPTH) {
      // two register sets: the next GAP_DEPTH pixels are on their way while this set is added, GAP_DEPTH .. 2 GAP_DEPTH loads in flight
      float4 a[GAP_DEPTH], b[GAP_DEPTH];
      gap_load(a, x, stride);
      for (; px + 2 * GAP_DEPTH <= p.hw; px += GAP_DEPTH) {
        gap_load(b, x + (px + GAP_DEPTH) * stride, stride);
        gap_add(a, s);
#pragma unroll
        for (int k = 0; k < GAP_DEPTH; ++k) a[k] = b[k];
      }
      gap_add(a, s);
      px += GAP_DEPTH;
    }
    for (; px + 4 <= p.hw; px += 4) {
      float4 v[4];
      gap_load(v, x + px * stride, stride);
      gap_add(v, s);
    }
    for (; px < p.hw; ++px) {
      float4 v[1];
      gap_load(v, x + px * stride, stride);
      gap_add(v, s);
    }
    p.out[i] = make_float4(s[0] / n, s[1] / n, s[2] / n, s[3] / n);
  }
}

// a lane owns four channels of GAP_BWD_PIXELS consecutive pixels of one row: its index is taken apart and g divided once per
// GAP_BWD_PIXELS stores (the 64-bit index divisions, one per store, cost as much as the store stream itself)
__global__ void __launch_bounds__(256) k_global_avg_pool_backward_f32(GapParams p) {
  const float n = (float)p.hw;
  const int groups = (p.hw + GAP_BWD_PIXELS - 1) / GAP_BWD_PIXELS;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < p.total; i += (long long)gridDim.x * 256) {
    const int v = (int)(i % p.vec_per_px);
    const long long t = i / p.vec_per_px;
    const int p0 = (int)(t % groups) * GAP_BWD_PIXELS;
    const long long r = t / groups;
    const float4 g = p.x[r * p.vec_per_px + v];
    const float4 d = make_float4(g.x / n, g.y / n, g.z / n, g.w / n);
    const int p1 = p0 + GAP_BWD_PIXELS < p.hw ? p0 + GAP_BWD_PIXELS : p.hw;
    float4* out = p.out + ((r * p.hw + p0) * p.vec_per_px + v);
    for (int px = p0; px < p1; ++px, out += p.vec_per_px) *out = d;
  }
}

static int gap_launch(const char* who, bool backward, const float* in, float* out, int rows, int hw, int channels,
                      odet_stream_t stream) {
  ODET_REQUIRE(in && out, "%s: null pointer", who);
  ODET_REQUIRE(rows >= 1 && hw >= 1, "%s: rows and hw must be at least 1 (got %d, %d)", who, rows, hw);
  ODET_REQUIRE(channels > 0 && channels % 4 == 0, "%s: channels must be a positive multiple of 4 (got %d)", who, channels);
  ODET_REQUIRE(((uintptr_t)in | (uintptr_t)out) % 16 == 0, "%s: pointers must be 16-byte aligned", who);
  GapParams p;
  p.x = reinterpret_cast<const float4*>(in);
  p.out = reinterpret_cast<float4*>(out);
  p.hw = hw;
  p.vec_per_px = channels / 4;
  p.total = (long long)rows * p.vec_per_px * (backward ? (hw + GAP_BWD_PIXELS - 1) / GAP_BWD_PIXELS : 1);
  if (backward)
    hipLaunchKernelGGL(k_global_avg_pool_backward_f32, dim3(ge_grid(p.total)), dim3(256), 0, (hipStream_t)stream, p);
  else
    hipLaunchKernelGGL(k_global_avg_pool_f32, dim3(ge_grid(p.total)), dim3(256), 0, (hipStream_t)stream, p);
  ODET_LAUNCH_CHECK();
  return ODET_OK;
}

extern "C" int odet_global_avg_pool_f32(const float* x, int rows, int hw, int channels, float* out, odet_stream_t stream) {
  return gap_launch("odet_global_avg_pool_f32", false, x, out, rows, hw, channels, stream);
}

extern "C" int odet_global_avg_pool_backward_f32(const float* g, int rows, int hw, int channels, float* dx, odet_stream_t stream) {
  return gap_launch("odet_global_avg_pool_backward_f32", true, g, dx, rows, hw, channels, stream);
}
