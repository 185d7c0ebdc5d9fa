// The two elementwise launches of a ResNet bottleneck's backward (reference model/fpn/resnet_fpn.py:154-205 read in reverse; the
// contractions are dense_grad.hip's and conv_grad.hip's):
//   odet_stride_gather_f32      out[b,i,j,:] = x[b, i*s, j*s, :] -- the contiguous [rows, cin] input that the Dense weight gradient of
//                               a strided 1x1 convolution needs (the forward reads the map strided and never writes this)
//   odet_block_input_grad_f32   the block's join: the gradient with respect to the block's input, either
//                               dx = (y > 0 ? dy : +0) + d1                    (identity shortcut: the final ReLU's gate on the shortcut's
//                                                                               gradient, plus c1's input gradient), or
//                               dx[b,Y,X,:] = d1[b,Y/s,X/s,:] + d2[b,Y/s,X/s,:] where Y % s == 0 and X % s == 0, +0 elsewhere
//                                                                              (convolutional shortcut: the gather's transpose with the
//                                                                               two branches' input gradients summed)
// HBM-bound streams.  The layout of k_fpn_topdown_backward_f32 (neck.hip): a lane owns four channels (16 bytes), a pixel's lanes
// are consecutive; the operands are read once (non-temporal loads), the result is stored normally (the next launch reads it).  One
// float32 add per element, no LDS, no atomics, no workspace; every output element is written exactly once.
#include "grad_elementwise.h"

struct GatherParams {
  const float4* x; float4* out;
  int H, W, Ho, Wo, stride;
  int vec_per_px;               // C / 4
  long long total;              // B * Ho * Wo * vec_per_px
};

__global__ void __launch_bounds__(256) k_stride_gather_f32(GatherParams p) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < p.total; i += (long long)gridDim.x * 256) {
    const int v = (int)(i % p.vec_per_px);
    long long px = i / p.vec_per_px;
    const int X = (int)(px % p.Wo);
    px /= p.Wo;
    const int Y = (int)(px % p.Ho);
    const long long b = px / p.Ho;
    p.out[i] = ge_stream(&p.x[((b * p.H + (long long)Y * p.stride) * p.W + (long long)X * p.stride) * p.vec_per_px + v]);
  }
}

struct JoinParams {
  const float4* dy; const float4* y; const float4* d1; const float4* d2; float4* dx;
  int H, W, Ho, Wo, stride;
  int vec_per_px;               // C / 4
  long long total;              // B * H * W * vec_per_px
};

// IDENTITY: dy, y, d1 at the lane's own index
template <bool IDENTITY>
__global__ void __launch_bounds__(256) k_block_input_grad_f32(JoinParams p) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < p.total; i += (long long)gridDim.x * 256) {
    float4 r;
    if (IDENTITY) {
      const float4 g = ge_stream(&p.dy[i]), y = ge_stream(&p.y[i]), a = ge_stream(&p.d1[i]);
      r = make_float4((y.x > 0.0f ? g.x : 0.0f) + a.x, (y.y > 0.0f ? g.y : 0.0f) + a.y, (y.z > 0.0f ? g.z : 0.0f) + a.z,
                      (y.w > 0.0f ? g.w : 0.0f) + a.w);
    } else {
      const int v = (int)(i % p.vec_per_px);
      long long px = i / p.vec_per_px;
      const int X = (int)(px % p.W);
      px /= p.W;
      const int Y = (int)(px % p.H);
      const long long b = px / p.H;
      r = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (p.stride == 1 || !((Y | X) & 1)) {
        const int sh = p.stride - 1;                         // stride 1 or 2
        const long long src = ((b * p.Ho + (Y >> sh)) * p.Wo + (X >> sh)) * p.vec_per_px + v;
        r = ge_stream(&p.d1[src]);
        if (p.d2) {
          const float4 t = ge_stream(&p.d2[src]);
          r = make_float4(r.x + t.x, r.y + t.y, r.z + t.z, r.w + t.w);
        }
      }
    }
    p.dx[i] = r;
  }
}

extern "C" int odet_stride_gather_f32(const float* x, int B, int H, int W, int C, int stride, float* out, odet_stream_t stream) {
  const char* who = "odet_stride_gather_f32";
  ODET_REQUIRE(x && out, "%s: null pointer", who);
  GE_REQUIRE_NHWC(who, B, H, W, C, (uintptr_t)x | (uintptr_t)out);
  ODET_REQUIRE(stride == 1 || stride == 2, "%s: stride must be 1 or 2 (got %d)", who, stride);
  if (B == 0) return ODET_OK;
  GatherParams p;
  p.x = reinterpret_cast<const float4*>(x);
  p.out = reinterpret_cast<float4*>(out);
  p.H = H; p.W = W; p.stride = stride;
  p.Ho = (H - 1) / stride + 1;
  p.Wo = (W - 1) / stride + 1;
  p.vec_per_px = C / 4;
  p.total = (long long)B * p.Ho * p.Wo * p.vec_per_px;
  hipLaunchKernelGGL(k_stride_gather_f32, dim3(ge_grid(p.total)), dim3(256), 0, (hipStream_t)stream, p);
  ODET_LAUNCH_CHECK();
  return ODET_OK;
}

extern "C" int odet_block_input_grad_f32(const float* dy, const float* y, const float* d1, const float* d2, float* dx, int B, int H,
                                         int W, int C, int stride, odet_stream_t stream) {
  const char* who = "odet_block_input_grad_f32";
  ODET_REQUIRE(dx, "%s: null dx", who);
  ODET_REQUIRE(d1, "%s: null d1", who);
  const bool identity = dy && y && !d2, conv = !dy && !y;
  ODET_REQUIRE(identity || conv, "%s: either dy, y and d1 without d2 (identity shortcut) or d1 (and d2) without dy and y "
               "(convolutional shortcut)", who);
  GE_REQUIRE_NHWC(who, B, H, W, C, (uintptr_t)dy | (uintptr_t)y | (uintptr_t)d1 | (uintptr_t)d2 | (uintptr_t)dx);
  ODET_REQUIRE(stride == 1 || stride == 2, "%s: stride must be 1 or 2 (got %d)", who, stride);
  ODET_REQUIRE(!identity || stride == 1, "%s: the identity form takes stride 1 only (got %d)", who, stride);
  if (B == 0) return ODET_OK;
  JoinParams p;
  p.dy = reinterpret_cast<const float4*>(dy);
  p.y = reinterpret_cast<const float4*>(y);
  p.d1 = reinterpret_cast<const float4*>(d1);
  p.d2 = reinterpret_cast<const float4*>(d2);
  p.dx = reinterpret_cast<float4*>(dx);
  p.H = H; p.W = W; p.stride = stride;
  p.Ho = (H - 1) / stride + 1;
  p.Wo = (W - 1) / stride + 1;
  p.vec_per_px = C / 4;
  p.total = (long long)B * H * W * p.vec_per_px;
  if (identity)
    hipLaunchKernelGGL(k_block_input_grad_f32<true>, dim3(ge_grid(p.total)), dim3(256), 0, (hipStream_t)stream, p);
  else
    hipLaunchKernelGGL(k_block_input_grad_f32<false>, dim3(ge_grid(p.total)), dim3(256), 0, (hipStream_t)stream, p);
  ODET_LAUNCH_CHECK();
  return ODET_OK;
}
