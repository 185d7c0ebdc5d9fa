// The two operators of the VGG16 training graph (reference model/faster_rcnn/vgg16_faster_rcnn.py) that the other backward passes
// do not have; the contractions are dense_grad.hip's and conv_grad.hip's:
//   odet_relu_maxpool2_backward_f32   MaxPooling2D((2,2), 2, 'same') after a ReLU convolution (:307, :325 block3_pool, block4_pool),
//                                     the backward of odet_bias_relu_maxpool's 2x2 / 2 ceil-mode form: TF's MaxPoolGrad, then ReluGrad.
//                                     a = max(z + bias, 0);  dz = dpool[window] at the FIRST position of the window (row-major) that
//                                     holds its maximum, when that maximum is > 0;  +0 everywhere else
//   odet_dropout_f32 /                tf.nn.dropout of TF r1.13 (:250-253, keep_rate 0.5) with the counter-based rule in place of TF's
//   odet_dropout_backward_f32         generator: element e takes word e & 3 of philox((e >> 2, image_id, stream_id, 0), seed),
//                                     u = bitcast((word & 0x7fffff) | 0x3f800000) - 1, keep = floor(keep_prob + u),
//                                     y = (x / keep_prob) * keep,  dx = (dy * keep) / keep_prob; the mask is recomputed, never stored
// HBM-bound streams in block_grad.hip's layout: a lane owns four channels (16 bytes) of one pooling window, or four consecutive
// elements (one Philox call); the operands are read once (non-temporal loads), the result is stored normally (the next launch reads
// it).  The windows do not overlap, so the pooling backward is a gather: no atomics, no LDS, no stored arg-max; every output element
// is written exactly once.
#include "grad_elementwise.h"

struct PoolGradParams {
  const float4* z; const float4* bias; const float4* dpool; float4* dz;
  int H, W, OH, OW;
  int vec_per_px;               // C / 4
  long long total;              // B * OH * OW * vec_per_px: one lane per window and four channels
};

__global__ void __launch_bounds__(256) k_relu_maxpool2_backward_f32(PoolGradParams p) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < p.total; i += (long long)gridDim.x * 256) {
    const int v = (int)(i % p.vec_per_px);
    long long t = i / p.vec_per_px;
    const int ox = (int)(t % p.OW);
    t /= p.OW;
    const int oy = (int)(t % p.OH);
    const long long b = t / p.OH;
    const int y0 = 2 * oy, x0 = 2 * ox;                        // (always inside the map: OH = ceil(H / 2))
    const bool in_x = x0 + 1 < p.W, in_y = y0 + 1 < p.H;
    const bool in[4] = {true, in_x, in_y, in_x && in_y};
    const long long base = ((b * p.H + y0) * p.W + x0) * p.vec_per_px + v;
    const long long off[4] = {0, p.vec_per_px, (long long)p.W * p.vec_per_px, (long long)(p.W + 1) * p.vec_per_px};
    const float4 bv = p.bias[v];
    const float bs[4] = {bv.x, bv.y, bv.z, bv.w};
    float a[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (!in[k]) continue;
      const float4 zv = ge_stream(&p.z[base + off[k]]);
      const float zs[4] = {zv.x, zv.y, zv.z, zv.w};
#pragma unroll
      for (int c = 0; c < 4; ++c) a[k][c] = zs[c] + bs[c];     // the sum the forward forms
    }
    const float4 gv = ge_stream(&p.dpool[i]);
    const float g[4] = {gv.x, gv.y, gv.z, gv.w};
    int win[4];                                                // the first tap that holds the window's maximum
    float best[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) { win[c] = 0; best[c] = a[0][c]; }
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      if (!in[k]) continue;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (a[k][c] > best[c]) { best[c] = a[k][c]; win[c] = k; }   // strictly greater: the first maximum stays
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (!in[k]) continue;
      float r[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) r[c] = (win[c] == k && best[c] > 0.0f) ? g[c] : 0.0f;
      p.dz[base + off[k]] = make_float4(r[0], r[1], r[2], r[3]);
    }
  }
}

struct DropoutParams {
  const float* x; float* y;
  long long n;
  float keep_prob;
  uint32_t k0, k1, image_id, stream_id;
};

// 1.0f where element e of the group with words w[] is kept, else 0.0f
static __device__ __forceinline__ float vg_keep(uint32_t word, float keep_prob) {
  const float u = __uint_as_float((word & 0x7fffffu) | 0x3f800000u) - 1.0f;     // TF's Uint32ToFloat: [0, 1)
  return floorf(keep_prob + u);
}

// BACKWARD: dx = (dy * keep) / keep_prob;  forward: y = (x / keep_prob) * keep
template <bool BACKWARD>
__global__ void __launch_bounds__(256) k_dropout_f32(DropoutParams p) {
  const long long groups = (p.n + 3) >> 2;
  for (long long gi = (long long)blockIdx.x * 256 + threadIdx.x; gi < groups; gi += (long long)gridDim.x * 256) {
    uint32_t w[4];
    odet_philox4((uint32_t)gi, p.image_id, p.stream_id, 0u, p.k0, p.k1, w);
    const long long e0 = gi << 2;
    float xs[4], r[4];
    const bool whole = e0 + 4 <= p.n;
    if (whole) {
      const float4 xv = ge_stream(reinterpret_cast<const float4*>(p.x + e0));
      xs[0] = xv.x; xs[1] = xv.y; xs[2] = xv.z; xs[3] = xv.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) xs[k] = e0 + k < p.n ? p.x[e0 + k] : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float keep = vg_keep(w[k], p.keep_prob);
      r[k] = BACKWARD ? (xs[k] * keep) / p.keep_prob : (xs[k] / p.keep_prob) * keep;
    }
    if (whole) {
      *reinterpret_cast<float4*>(p.y + e0) = make_float4(r[0], r[1], r[2], r[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (e0 + k < p.n) p.y[e0 + k] = r[k];
    }
  }
}

extern "C" int odet_relu_maxpool2_backward_f32(const float* z, const float* bias, const float* dpool, float* dz, int B, int H, int W,
                                               int C, odet_stream_t stream) {
  const char* who = "odet_relu_maxpool2_backward_f32";
  ODET_REQUIRE(z && bias && dpool && dz, "%s: null pointer", who);
  GE_REQUIRE_NHWC(who, B, H, W, C, (uintptr_t)z | (uintptr_t)bias | (uintptr_t)dpool | (uintptr_t)dz);
  if (B == 0) return ODET_OK;
  PoolGradParams p;
  p.z = reinterpret_cast<const float4*>(z);
  p.bias = reinterpret_cast<const float4*>(bias);
  p.dpool = reinterpret_cast<const float4*>(dpool);
  p.dz = reinterpret_cast<float4*>(dz);
  p.H = H; p.W = W;
  p.OH = (H + 1) / 2;
  p.OW = (W + 1) / 2;
  p.vec_per_px = C / 4;
  p.total = (long long)B * p.OH * p.OW * p.vec_per_px;
  hipLaunchKernelGGL(k_relu_maxpool2_backward_f32, dim3(ge_grid(p.total)), dim3(256), 0, (hipStream_t)stream, p);
  ODET_LAUNCH_CHECK();
  return ODET_OK;
}

static int vg_dropout(const char* who, bool backward, const float* x, float* y, long long n, float keep_prob, uint64_t seed,
                      uint32_t image_id, uint32_t stream_id, odet_stream_t stream) {
  ODET_REQUIRE(n >= 0 && n <= (1ll << 34), "%s: n must be in [0, 2^34] (got %lld)", who, n);
  ODET_REQUIRE(keep_prob > 0.0f && keep_prob <= 1.0f, "%s: keep_prob must be in (0, 1] (got %g)", who, (double)keep_prob);
  if (n == 0) return ODET_OK;
  ODET_REQUIRE(x && y, "%s: null pointer", who);
  ODET_REQUIRE(((uintptr_t)x | (uintptr_t)y) % 16 == 0, "%s: pointers must be 16-byte aligned", who);
  if (keep_prob == 1.0f) {                                     // tf.nn.dropout returns its input unchanged
    if (x != y) ODET_HIP(hipMemcpyAsync(y, x, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return ODET_OK;
  }
  DropoutParams p;
  p.x = x; p.y = y; p.n = n; p.keep_prob = keep_prob;
  p.k0 = (uint32_t)seed; p.k1 = (uint32_t)(seed >> 32);
  p.image_id = image_id; p.stream_id = stream_id;
  const int grid = ge_grid((n + 3) >> 2);
  if (backward)
    hipLaunchKernelGGL(k_dropout_f32<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
  else
    hipLaunchKernelGGL(k_dropout_f32<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
  ODET_LAUNCH_CHECK();
  return ODET_OK;
}

extern "C" int odet_dropout_f32(const float* x, float* y, long long n, float keep_prob, uint64_t seed, uint32_t image_id,
                                uint32_t stream_id, odet_stream_t stream) {
  return vg_dropout("odet_dropout_f32", false, x, y, n, keep_prob, seed, image_id, stream_id, stream);
}

extern "C" int odet_dropout_backward_f32(const float* dy, float* dx, long long n, float keep_prob, uint64_t seed, uint32_t image_id,
                                         uint32_t stream_id, odet_stream_t stream) {
  return vg_dropout("odet_dropout_backward_f32", true, dy, dx, n, keep_prob, seed, image_id, stream_id, stream);
}
