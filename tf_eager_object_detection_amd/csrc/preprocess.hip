// Eval input front end: decoded uint8 HWC images -> one NHWC float32 / float16 batch [B, H, W, 3], mean-subtracted and
// resized, as the reference's eval loaders produce it (one launch for the whole batch):
//   voc  = dataset/eval_pascal_tf_dataset.py:32-52 (cv2.imread BGR -> numpy normalisation -> cv2.resize INTER_LINEAR ->
//          optional flip to RGB);
//   coco = dataset/utils/tf_dataset_utils.py:55-80, 128-155 (decode_jpeg RGB -> _caffe_preprocessing / _tf_preprocessing ->
//          tf.image.resize_bilinear of TF 1.x, align_corners=False).
// One IEEE float32 operation per reference operation (the build passes -ffp-contract=off); float16 output is the float32
// result rounded once to nearest even.
//
// Shape: one workgroup per output row of one image (grid H x B).  The workgroup stages the two source rows it interpolates
// between in LDS, already normalised and in output channel order (2 x 3w floats, w <= ODET_PREP_MAX_RAW_W), then writes the
// row with 16-byte stores; the (at most V - 1) elements before the first and after the last 16-byte boundary of the row are
// single stores.  The launch is bound by its output writes (12 or 6 bytes per output pixel against <= 4 staged source bytes
// per output pixel at the flagship sizes).
#include <hip/hip_fp16.h>

#include "odet_internal.h"

#define PREP_THREADS 256

struct PrepParams {
  const uint8_t* src[ODET_PREP_MAX_BATCH];
  long long pitch[ODET_PREP_MAX_BATCH];   // bytes between consecutive source rows
  int h[ODET_PREP_MAX_BATCH];
  int w[ODET_PREP_MAX_BATCH];
  int H, W, pipeline, norm;
  int src_ch[3];                          // output channel c reads source channel src_ch[c]
  double mean_d[3];                       // voc caffe: numpy's float32 -= float64[3] runs in float64
  float mean_f[3];                        // coco caffe: tensor - python float subtracts a float32 constant
  void* out;
};

// the per-pixel normalisation of the output channel c whose source byte is u
__device__ __forceinline__ float prep_norm(const PrepParams& p, uint32_t u, int c) {
  if (p.pipeline == ODET_PREP_VOC) {
    if (p.norm == ODET_PREP_CAFFE) return (float)((double)u - p.mean_d[c]);   // img -= np.array([[means]]) (:37)
    return (((float)u / 255.0f) * 2.0f) - 1.0f;                               // img / 255.0 * 2.0 - 1.0 (:39)
  }
  if (p.norm == ODET_PREP_CAFFE) return (float)u - p.mean_f[c];                // tf_dataset_utils.py:67-71
  return (((float)u * (float)(1.0 / 255.0)) * 2.0f) - 1.0f;                   // convert_image_dtype multiplies (:80)
}

template <typename T>
struct PrepOut;
template <>
struct PrepOut<float> {
  static constexpr int V = 4;             // elements per 16-byte store
  static __device__ __forceinline__ void put1(float* o, float v) { *o = v; }
  static __device__ __forceinline__ void putv(float* o, const float (&v)[8]) {
    *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
  }
};
template <>
struct PrepOut<__half> {
  static constexpr int V = 8;
  static __device__ __forceinline__ void put1(__half* o, float v) { *o = __float2half_rn(v); }
  static __device__ __forceinline__ void putv(__half* o, const float (&v)[8]) {
    uint32_t q[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const __half2 t = __floats2half2_rn(v[2 * i], v[2 * i + 1]);
      q[i] = *reinterpret_cast<const uint32_t*>(&t);
    }
    *reinterpret_cast<uint4*>(o) = make_uint4(q[0], q[1], q[2], q[3]);
  }
};

enum { PREP_CV_LINEAR = 0, PREP_CV_AREA2 = 1, PREP_TF_LEGACY = 2 };

// Everything an output element of this row needs besides its own column.
struct PrepRow {
  const float* L0;
  const float* L1;
  int mode, w;
  double scale_x;                         // cv: 1 / ((double)W / w)
  float xs;                               // tf: (float)w / (float)W
  float b0, b1;                           // cv linear: (1 - fy, fy); tf: b0 = y lerp
};

__device__ __forceinline__ float prep_value(const PrepRow& r, int e) {
  const int dx = e / 3;
  const int c = e - 3 * dx;
  if (r.mode == PREP_CV_AREA2) {          // resizeAreaFast_: sum += S[ofs[0]] + ... + S[ofs[3]]; D = sum * (1.f / 4)
    const int i = 6 * dx + c;
    return (((r.L0[i] + r.L0[i + 3]) + r.L1[i]) + r.L1[i + 3]) * 0.25f;
  }
  if (r.mode == PREP_TF_LEGACY) {         // resize_bilinear_op.cc, legacy scaler
    const float fx = (float)dx * r.xs;
    const int x0 = min((int)floorf(fx), r.w - 1);
    const int x1 = min(x0 + 1, r.w - 1);
    const float xl = fx - (float)x0;
    const float tl = r.L0[3 * x0 + c], tr = r.L0[3 * x1 + c];
    const float bl = r.L1[3 * x0 + c], br = r.L1[3 * x1 + c];
    const float top = tl + (tr - tl) * xl;
    const float bot = bl + (br - bl) * xl;
    return top + (bot - top) * r.b0;
  }
  // OpenCV resize.cpp, INTER_LINEAR: the xofs / alpha tables of cv::resize, HResizeLinear, VResizeLinear
  float fx = (float)(((double)dx + 0.5) * r.scale_x - 0.5);
  int sx = (int)floorf(fx);
  fx -= (float)sx;
  if (sx < 0) { fx = 0.0f; sx = 0; }
  if (sx >= r.w - 1) { fx = 0.0f; sx = r.w - 1; }
  const int sx1 = min(sx + 1, r.w - 1);   // (weight 0 where clamped: S * 1 + S' * 0 == S, OpenCV's copy branch)
  const float a0 = 1.0f - fx, a1 = fx;
  const float h0 = r.L0[3 * sx + c] * a0 + r.L0[3 * sx1 + c] * a1;
  const float h1 = r.L1[3 * sx + c] * a0 + r.L1[3 * sx1 + c] * a1;
  return h0 * r.b0 + h1 * r.b1;
}

template <typename T>
__global__ void __launch_bounds__(PREP_THREADS) k_preprocess(PrepParams p) {
  extern __shared__ float prep_lds[];
  const int dy = blockIdx.x, b = blockIdx.y;
  const int h = p.h[b], w = p.w[b];
  const int H = p.H, W = p.W;
  PrepRow r;
  r.w = w;
  r.scale_x = 0.0;
  r.xs = 0.0f;
  r.b0 = 0.0f;
  r.b1 = 0.0f;
  int y0, y1;
  if (p.pipeline == ODET_PREP_VOC && w == 2 * W && h == 2 * H) {
    // cv::resize switches INTER_LINEAR to INTER_AREA when both axes shrink by exactly 2
    r.mode = PREP_CV_AREA2;
    y0 = 2 * dy;
    y1 = 2 * dy + 1;
  } else if (p.pipeline == ODET_PREP_VOC) {
    r.mode = PREP_CV_LINEAR;
    r.scale_x = 1.0 / ((double)W / (double)w);
    const double scale_y = 1.0 / ((double)H / (double)h);
    float fy = (float)(((double)dy + 0.5) * scale_y - 0.5);
    const int sy = (int)floorf(fy);
    fy -= (float)sy;
    // resizeGeneric_Invoker: the ROW index is clipped to [0, h - 1], the weights (1 - fy, fy) are kept (unlike x)
    y0 = min(max(sy, 0), h - 1);
    y1 = min(max(sy + 1, 0), h - 1);
    r.b0 = 1.0f - fy;
    r.b1 = fy;
  } else {
    r.mode = PREP_TF_LEGACY;
    r.xs = (float)w / (float)W;
    const float ys = (float)h / (float)H;
    const float fy = (float)dy * ys;
    y0 = min((int)floorf(fy), h - 1);
    y1 = min(y0 + 1, h - 1);
    r.b0 = fy - (float)y0;
  }
  // stage the two source rows, normalised, in output channel order.  A row is cut at the 16-byte boundaries of its
  // address: the chunks wholly inside the row are read with one 16-byte load each, the (at most two) partial chunks at its
  // ends byte by byte, only their bytes inside the row; up to PREP_INFLIGHT chunks per thread are in flight before any
  // is unpacked.
  const int n_src = 3 * w;
  float* L0 = prep_lds;
  float* L1 = prep_lds + n_src;
  const uint8_t* s0 = p.src[b] + (long long)y0 * p.pitch[b];
  const uint8_t* s1 = p.src[b] + (long long)y1 * p.pitch[b];
  const int off0 = (int)((uintptr_t)s0 & 15), off1 = (int)((uintptr_t)s1 & 15);
  const int nch0 = (off0 + n_src + 15) >> 4;
  const int nch = nch0 + ((off1 + n_src + 15) >> 4);
  constexpr int PREP_INFLIGHT = 4;
  for (int k0 = threadIdx.x; k0 < nch; k0 += PREP_INFLIGHT * PREP_THREADS) {
    uint32_t q[PREP_INFLIGHT][4];
#pragma unroll
    for (int r = 0; r < PREP_INFLIGHT; ++r) {
      const int k = k0 + r * PREP_THREADS;
      if (k >= nch) break;
      const bool second = k >= nch0;
      const uint8_t* s = second ? s1 : s0;
      const int first = (second ? k - nch0 : k) * 16 - (second ? off1 : off0);   // row byte index of the chunk's byte 0
      if (first >= 0 && first + 16 <= n_src) {
        const uint4 v = *reinterpret_cast<const uint4*>(s + first);
        q[r][0] = v.x; q[r][1] = v.y; q[r][2] = v.z; q[r][3] = v.w;
      } else {
        q[r][0] = q[r][1] = q[r][2] = q[r][3] = 0u;
        for (int i = 0; i < 16; ++i)
          if (first + i >= 0 && first + i < n_src) q[r][i >> 2] |= (uint32_t)s[first + i] << (8 * (i & 3));
      }
    }
#pragma unroll
    for (int r = 0; r < PREP_INFLIGHT; ++r) {
      const int k = k0 + r * PREP_THREADS;
      if (k >= nch) break;
      const bool second = k >= nch0;
      float* L = second ? L1 : L0;
      const int first = (second ? k - nch0 : k) * 16 - (second ? off1 : off0);
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int j = first + i;
        if (j < 0 || j >= n_src) continue;
        const int x = j / 3;
        const int sc = j - 3 * x;
        const int c = p.src_ch[sc];      // (src_ch is the identity or the reversal: its own inverse)
        L[3 * x + c] = prep_norm(p, (q[r][i >> 2] >> (8 * (i & 3))) & 255u, c);
      }
    }
  }
  __syncthreads();
  r.L0 = L0;
  r.L1 = L1;

  constexpr int V = PrepOut<T>::V;
  const int n = 3 * W;
  const long long ob = ((long long)b * H + dy) * (long long)n;
  T* row = reinterpret_cast<T*>(p.out) + ob;
  const int head = min((int)((V - ob % V) % V), n);     // elements before the row's first 16-byte boundary
  const int nvec = (n - head) / V;
  const int tail = head + nvec * V;
  for (int i = threadIdx.x; i < nvec; i += PREP_THREADS) {
    const int e = head + i * V;
    float v[8];
#pragma unroll
    for (int k = 0; k < V; ++k) v[k] = prep_value(r, e + k);
    PrepOut<T>::putv(row + e, v);
  }
  const int t = threadIdx.x;
  if (t < head) PrepOut<T>::put1(row + t, prep_value(r, t));
  if (t >= 64 && t - 64 < n - tail) PrepOut<T>::put1(row + tail + (t - 64), prep_value(r, tail + (t - 64)));
}

static const unsigned PREP_LDS_MAX = 2u * 3u * ODET_PREP_MAX_RAW_W * 4u;

static hipError_t prep_prepare_kernels() {
  static OdetPerDeviceOnce once;
  return once.run([] {
    hipError_t e = hipFuncSetAttribute((const void*)k_preprocess<float>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       PREP_LDS_MAX);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute((const void*)k_preprocess<__half>, hipFuncAttributeMaxDynamicSharedMemorySize, PREP_LDS_MAX);
  });
}

extern "C" int odet_preprocess_images(const void* const* images, const int* raw_h, const int* raw_w,
                                      const long long* row_pitch, int B, int H, int W, int pipeline, int preprocessing,
                                      int rgb, const double* means, void* out, int f16, odet_stream_t stream) {
  ODET_REQUIRE(B >= 0, "odet_preprocess_images: negative batch %d", B);
  if (B > ODET_PREP_MAX_BATCH)
    return odet_set_error(ODET_E_LIMIT, "odet_preprocess_images: batch %d exceeds %d", B, ODET_PREP_MAX_BATCH);
  ODET_REQUIRE(H > 0 && W > 0, "odet_preprocess_images: non-positive output size %d x %d", H, W);
  if (H > ODET_PREP_MAX_OUT || W > ODET_PREP_MAX_OUT)
    return odet_set_error(ODET_E_LIMIT, "odet_preprocess_images: output size %d x %d exceeds %d", H, W, ODET_PREP_MAX_OUT);
  ODET_REQUIRE(pipeline == ODET_PREP_VOC || pipeline == ODET_PREP_COCO, "odet_preprocess_images: unknown pipeline %d",
               pipeline);
  ODET_REQUIRE(preprocessing == ODET_PREP_CAFFE || preprocessing == ODET_PREP_TF,
               "odet_preprocess_images: unknown preprocessing %d", preprocessing);
  ODET_REQUIRE(rgb == 0 || (rgb == 1 && pipeline == ODET_PREP_VOC),
               "odet_preprocess_images: rgb must be 0 or 1, and 1 only for the voc pipeline");
  ODET_REQUIRE(f16 == 0 || f16 == 1, "odet_preprocess_images: f16 must be 0 or 1");
  if (B == 0) return ODET_OK;
  ODET_REQUIRE(images && raw_h && raw_w && row_pitch && out, "odet_preprocess_images: null pointer");
  ODET_REQUIRE(means || preprocessing == ODET_PREP_TF, "odet_preprocess_images: null pointer (means)");
  ODET_REQUIRE(((uintptr_t)out & 15) == 0, "odet_preprocess_images: out must be 16-byte aligned");
  PrepParams p;
  int max_w = 0;
  for (int i = 0; i < B; ++i) {
    ODET_REQUIRE(images[i], "odet_preprocess_images: null pointer (image %d)", i);
    ODET_REQUIRE(raw_h[i] > 0 && raw_w[i] > 0, "odet_preprocess_images: image %d has size %d x %d", i, raw_h[i], raw_w[i]);
    if (raw_w[i] > ODET_PREP_MAX_RAW_W || raw_h[i] > ODET_PREP_MAX_RAW_H)
      return odet_set_error(ODET_E_LIMIT, "odet_preprocess_images: image %d (%d x %d) exceeds %d x %d", i, raw_h[i],
                            raw_w[i], ODET_PREP_MAX_RAW_H, ODET_PREP_MAX_RAW_W);
    ODET_REQUIRE(row_pitch[i] >= 3ll * raw_w[i], "odet_preprocess_images: image %d row pitch %lld < 3 * %d", i,
                 row_pitch[i], raw_w[i]);
    p.src[i] = (const uint8_t*)images[i];
    p.pitch[i] = row_pitch[i];
    p.h[i] = raw_h[i];
    p.w[i] = raw_w[i];
    max_w = max_w > raw_w[i] ? max_w : raw_w[i];
  }
  p.H = H;
  p.W = W;
  p.pipeline = pipeline;
  p.norm = preprocessing;
  for (int c = 0; c < 3; ++c) {
    // voc: BGR in, flipped after the resize when rgb (:50-51); coco caffe: RGB in, tf.reverse to BGR before the means (:66)
    const int sc = (pipeline == ODET_PREP_VOC) ? (rgb ? 2 - c : c) : (preprocessing == ODET_PREP_CAFFE ? 2 - c : c);
    p.src_ch[c] = sc;
    const double m = means ? (pipeline == ODET_PREP_VOC ? means[sc] : means[c]) : 0.0;
    p.mean_d[c] = m;
    p.mean_f[c] = (float)m;
  }
  p.out = out;
  ODET_HIP(prep_prepare_kernels());
  const size_t lds = (size_t)2 * 3 * max_w * sizeof(float);
  if (f16)
    hipLaunchKernelGGL(k_preprocess<__half>, dim3(H, B), dim3(PREP_THREADS), lds, (hipStream_t)stream, p);
  else
    hipLaunchKernelGGL(k_preprocess<float>, dim3(H, B), dim3(PREP_THREADS), lds, (hipStream_t)stream, p);
  ODET_LAUNCH_CHECK();
  return ODET_OK;
}
