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
//
// Training input front end (odet_preprocess_train): the same row workgroups, with the horizontal flip of
// image_argument_with_imgaug (dataset/utils/tf_dataset_utils.py:16-52, iaa.Fliplr) folded into the LDS staging -- source
// column x lands at w - 1 - x, BEFORE normalisation and resize, as the reference orders them -- plus one more workgroup per
// image (blockIdx.x == H) for its ground-truth boxes and its row of the offsets.
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

// One output row of one image.  flip (the training launch only) mirrors the source columns while they are staged.
template <typename T, bool TRAIN>
__device__ __forceinline__ void prep_row(const PrepParams& p, float* prep_lds, int dy, int b, bool flip) {
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
        L[3 * ((TRAIN && flip) ? w - 1 - x : x) + c] = prep_norm(p, (q[r][i >> 2] >> (8 * (i & 3))) & 255u, c);
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

template <typename T>
__global__ void __launch_bounds__(PREP_THREADS) k_preprocess(PrepParams p) {
  extern __shared__ float prep_lds[];
  prep_row<T, false>(p, prep_lds, blockIdx.x, blockIdx.y, false);
}

// ---- training: the boxes of image_argument_with_imgaug + preprocessing_training_func + train_one_epoch ------------------
struct PrepTrain {
  unsigned long long flip_mask;           // bit b: image b is mirrored (decided on the host: baked into a captured graph)
  int augment;
  int32_t gt_off[ODET_PREP_MAX_BATCH + 1];
  const float* boxes_in;                  // [sum G, 4] (ymin, xmin, ymax, xmax), normalised to the raw image
  float* boxes_out;                       // [sum G, 4] (xmin, ymin, xmax, ymax), pixels of the resized image
  int32_t* off_out;                       // [B + 1]
};

// int(bbox[k] * size) (tf_dataset_utils.py:31-32): the float32 scalar times a Python int is a float64 product, truncated
// toward zero.  (Python's int is unbounded; the clamp keeps the conversion defined, and everything that far out clips.)
__device__ __forceinline__ long long prep_trunc(float v, int size) {
  const double lim = 4611686018427387904.0;   // 2^62
  const double d = (double)v * (double)size;
  return (long long)fmin(fmax(d, -lim), lim);
}
// iaa_bbox.y1 / height in float64, clipped to [0, 1], .astype(np.float32) (:48-52)
__device__ __forceinline__ float prep_unit(long long i, int size) {
  double q = (double)i / (double)size;
  q = q < 0.0 ? 0.0 : q;
  q = q > 1.0 ? 1.0 : q;
  return (float)q;
}

__device__ __forceinline__ void prep_boxes(const PrepParams& p, const PrepTrain& t, int b, bool flip) {
  const int lo = t.gt_off[b], hi = t.gt_off[b + 1];
  if (threadIdx.x == 0) {
    t.off_out[b] = lo;
    if (b == (int)gridDim.y - 1) t.off_out[b + 1] = hi;
  }
  const int h = p.h[b], w = p.w[b];
  const float sy = (float)(p.H - 1), sx = (float)(p.W - 1);      // tf.to_float(n_height - 1), (n_width - 1) (:120-123)
  for (int g = lo + (int)threadIdx.x; g < hi; g += PREP_THREADS) {
    const float* in = t.boxes_in + 4ll * g;
    float y1 = in[0], x1 = in[1], y2 = in[2], x2 = in[3];
    if (t.augment) {
      long long iy1 = prep_trunc(y1, h), ix1 = prep_trunc(x1, w), iy2 = prep_trunc(y2, h), ix2 = prep_trunc(x2, w);
      if (ix1 > ix2) { const long long s = ix1; ix1 = ix2; ix2 = s; }      // ia.BoundingBox.__init__
      if (iy1 > iy2) { const long long s = iy1; iy1 = iy2; iy2 = s; }
      if (flip) {                                                           // Fliplr: x' = width - x on both corners
        const long long a = (long long)w - ix2, c = (long long)w - ix1;
        ix1 = a;
        ix2 = c;
      }
      y1 = prep_unit(iy1, h);
      x1 = prep_unit(ix1, w);
      y2 = prep_unit(iy2, h);
      x2 = prep_unit(ix2, w);
    }
    float* o = t.boxes_out + 4ll * g;
    o[0] = x1 * sx;                                                         // x first: scripts/train.py:89-93
    o[1] = y1 * sy;
    o[2] = x2 * sx;
    o[3] = y2 * sy;
  }
}

template <typename T>
__global__ void __launch_bounds__(PREP_THREADS) k_preprocess_train(PrepParams p, PrepTrain t) {
  extern __shared__ float prep_lds[];
  const int b = blockIdx.y;
  const bool flip = (t.flip_mask >> b) & 1ull;
  if ((int)blockIdx.x == p.H)
    prep_boxes(p, t, b, flip);
  else
    prep_row<T, true>(p, prep_lds, blockIdx.x, b, flip);
}

static const unsigned PREP_LDS_MAX = 2u * 3u * ODET_PREP_MAX_RAW_W * 4u;

static hipError_t prep_prepare_kernels() {
  static OdetPerDeviceOnce once;
  return once.run([] {
    hipError_t e = hipFuncSetAttribute((const void*)k_preprocess<float>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       PREP_LDS_MAX);
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute((const void*)k_preprocess<__half>, hipFuncAttributeMaxDynamicSharedMemorySize, PREP_LDS_MAX);
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute((const void*)k_preprocess_train<float>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            PREP_LDS_MAX);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute((const void*)k_preprocess_train<__half>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               PREP_LDS_MAX);
  });
}

// The argument checks and the parameter block both entry points share.  *empty = 1: B == 0, nothing to launch.
static int prep_setup(const char* who, const void* const* images, const int* raw_h, const int* raw_w,
                      const long long* row_pitch, int B, int H, int W, int pipeline, int preprocessing, int rgb,
                      const double* means, void* out, int f16, PrepParams* pp, int* max_w_out, int* empty) {
  PrepParams& p = *pp;
  *empty = 0;
  ODET_REQUIRE(B >= 0, "%s: negative batch %d", who, B);
  if (B > ODET_PREP_MAX_BATCH) return odet_set_error(ODET_E_LIMIT, "%s: batch %d exceeds %d", who, B, ODET_PREP_MAX_BATCH);
  ODET_REQUIRE(H > 0 && W > 0, "%s: non-positive output size %d x %d", who, H, W);
  if (H > ODET_PREP_MAX_OUT || W > ODET_PREP_MAX_OUT)
    return odet_set_error(ODET_E_LIMIT, "%s: output size %d x %d exceeds %d", who, H, W, ODET_PREP_MAX_OUT);
  ODET_REQUIRE(pipeline == ODET_PREP_VOC || pipeline == ODET_PREP_COCO, "%s: unknown pipeline %d", who, pipeline);
  ODET_REQUIRE(preprocessing == ODET_PREP_CAFFE || preprocessing == ODET_PREP_TF, "%s: unknown preprocessing %d", who,
               preprocessing);
  ODET_REQUIRE(rgb == 0 || (rgb == 1 && pipeline == ODET_PREP_VOC),
               "%s: rgb must be 0 or 1, and 1 only for the voc pipeline", who);
  ODET_REQUIRE(f16 == 0 || f16 == 1, "%s: f16 must be 0 or 1", who);
  if (B == 0) {
    *empty = 1;
    return ODET_OK;
  }
  ODET_REQUIRE(images && raw_h && raw_w && row_pitch && out, "%s: null pointer", who);
  ODET_REQUIRE(means || preprocessing == ODET_PREP_TF, "%s: null pointer (means)", who);
  ODET_REQUIRE(((uintptr_t)out & 15) == 0, "%s: out must be 16-byte aligned", who);
  int max_w = 0;
  for (int i = 0; i < B; ++i) {
    ODET_REQUIRE(images[i], "%s: null pointer (image %d)", who, i);
    ODET_REQUIRE(raw_h[i] > 0 && raw_w[i] > 0, "%s: image %d has size %d x %d", who, i, raw_h[i], raw_w[i]);
    if (raw_w[i] > ODET_PREP_MAX_RAW_W || raw_h[i] > ODET_PREP_MAX_RAW_H)
      return odet_set_error(ODET_E_LIMIT, "%s: image %d (%d x %d) exceeds %d x %d", who, i, raw_h[i], raw_w[i],
                            ODET_PREP_MAX_RAW_H, ODET_PREP_MAX_RAW_W);
    ODET_REQUIRE(row_pitch[i] >= 3ll * raw_w[i], "%s: image %d row pitch %lld < 3 * %d", who, i, row_pitch[i], raw_w[i]);
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
  *max_w_out = max_w;
  return ODET_OK;
}

extern "C" int odet_preprocess_images(const void* const* images, const int* raw_h, const int* raw_w,
                                      const long long* row_pitch, int B, int H, int W, int pipeline, int preprocessing,
                                      int rgb, const double* means, void* out, int f16, odet_stream_t stream) {
  PrepParams p;
  int max_w = 0, empty = 0;
  const int rc = prep_setup("odet_preprocess_images", images, raw_h, raw_w, row_pitch, B, H, W, pipeline, preprocessing, rgb,
                            means, out, f16, &p, &max_w, &empty);
  if (rc != ODET_OK || empty) return rc;
  ODET_HIP(prep_prepare_kernels());
  const size_t lds = (size_t)2 * 3 * max_w * sizeof(float);
  if (f16)
    hipLaunchKernelGGL(k_preprocess<__half>, dim3(H, B), dim3(PREP_THREADS), lds, (hipStream_t)stream, p);
  else
    hipLaunchKernelGGL(k_preprocess<float>, dim3(H, B), dim3(PREP_THREADS), lds, (hipStream_t)stream, p);
  ODET_LAUNCH_CHECK();
  return ODET_OK;
}

extern "C" int odet_preprocess_train(const void* const* images, const int* raw_h, const int* raw_w,
                                     const long long* row_pitch, int B, int H, int W, int preprocessing,
                                     const double* means, const float* boxes_yxyx, const int* gt_offsets, int augment,
                                     const int* flip, uint64_t seed, uint32_t first_image_id, void* out, int f16,
                                     float* gt_boxes_xyxy, int32_t* gt_offsets_dev, int* flipped, odet_stream_t stream) {
  static const char* who = "odet_preprocess_train";
  ODET_REQUIRE(augment == 0 || augment == 1, "%s: augment must be 0 or 1", who);
  ODET_REQUIRE(!flip || augment == 1, "%s: flip flags given with augment = 0", who);
  PrepParams p;
  int max_w = 0, empty = 0;
  const int rc = prep_setup(who, images, raw_h, raw_w, row_pitch, B, H, W, ODET_PREP_COCO, preprocessing, 0, means, out, f16,
                            &p, &max_w, &empty);
  if (rc != ODET_OK || empty) return rc;
  ODET_REQUIRE(gt_offsets && gt_offsets_dev, "%s: null pointer (gt_offsets)", who);
  ODET_REQUIRE(gt_offsets[0] == 0, "%s: gt_offsets[0] = %d, must be 0", who, gt_offsets[0]);
  PrepTrain t;
  t.flip_mask = 0ull;
  t.augment = augment;
  t.gt_off[0] = 0;
  for (int i = 0; i < B; ++i) {
    const int g = gt_offsets[i + 1] - gt_offsets[i];
    ODET_REQUIRE(gt_offsets[i + 1] >= gt_offsets[i], "%s: gt_offsets decrease at image %d (%d -> %d)", who, i, gt_offsets[i],
                 gt_offsets[i + 1]);
    if (g > ODET_PREP_MAX_BOXES)
      return odet_set_error(ODET_E_LIMIT, "%s: image %d has %d boxes, exceeds %d", who, i, g, ODET_PREP_MAX_BOXES);
    t.gt_off[i + 1] = gt_offsets[i + 1];
    int f = 0;
    if (flip) {
      ODET_REQUIRE(flip[i] == 0 || flip[i] == 1, "%s: flip[%d] = %d, must be 0 or 1", who, i, flip[i]);
      f = flip[i];
    } else if (augment) {                  // stream 5 of the sampling rule (include/odet.h "training targets")
      uint32_t w0, w1;
      odet_philox2(0u, first_image_id + (uint32_t)i, TG_STREAM_IMAGE_FLIP, 0u, (uint32_t)seed, (uint32_t)(seed >> 32),
                   &w0, &w1);
      f = (int)(w0 >> 31);
    }
    if (f) t.flip_mask |= 1ull << i;
  }
  ODET_REQUIRE(gt_offsets[B] == 0 || (boxes_yxyx && gt_boxes_xyxy), "%s: null pointer (boxes)", who);
  if (flipped)
    for (int i = 0; i < B; ++i) flipped[i] = (int)((t.flip_mask >> i) & 1ull);
  t.boxes_in = boxes_yxyx;
  t.boxes_out = gt_boxes_xyxy;
  t.off_out = gt_offsets_dev;
  ODET_HIP(prep_prepare_kernels());
  const size_t lds = (size_t)2 * 3 * max_w * sizeof(float);
  if (f16)
    hipLaunchKernelGGL(k_preprocess_train<__half>, dim3(H + 1, B), dim3(PREP_THREADS), lds, (hipStream_t)stream, p, t);
  else
    hipLaunchKernelGGL(k_preprocess_train<float>, dim3(H + 1, B), dim3(PREP_THREADS), lds, (hipStream_t)stream, p, t);
  ODET_LAUNCH_CHECK();
  return ODET_OK;
}
