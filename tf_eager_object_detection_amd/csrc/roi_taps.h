// The sample coordinates of RoI pooling (tf.image.crop_and_resize): ONE definition for the forward (roi.hip, roi_half.hip) and
// the backward (roi_grad.hip), so that both tap the same cells with the same weights, bit for bit.
//
//   roi_norm_box<NORM>   the normalised box (y1, x1, y2, x2) of a RoI, exactly as the reference builds it per layer
//   make_axis            TF's start / per-sample step of one axis of the crop
//   make_tap<PAD>        one sample along one axis: inside?, floor / ceil cell, lerp weight
#ifndef ODET_ROI_TAPS_H_
#define ODET_ROI_TAPS_H_

#include "odet_internal.h"

struct Axis {
  float start;   // in_(0)
  float scale;   // per-sample step
  float limit;   // dim - 1 (in sampled-map coordinates)
  float single;  // crop == 1: the one sample coordinate
};

// TF crop_and_resize_op.cc: in = lo_n * (dim-1) + i * scale, scale = (hi_n - lo_n)*(dim-1)/(crop-1)
__device__ __forceinline__ Axis make_axis(float lo_n, float hi_n, int dim, int crop) {
  Axis a;
  a.limit = (float)(dim - 1);
  a.scale = (crop > 1) ? (hi_n - lo_n) * a.limit / (float)(crop - 1) : 0.0f;
  a.start = lo_n * a.limit;
  a.single = 0.5f * (lo_n + hi_n) * a.limit;   // crop == 1 path
  return a;
}

struct Tap {      // one sample along one axis
  bool ok;        // TF: not extrapolated (0 <= in <= dim-1; NaN fails)
  int lo, hi;     // floor / ceil cell (after the SYMMETRIC-pad remap for the padded tensorpack mode)
  float lerp;
};

template <bool PAD>
__device__ __forceinline__ Tap make_tap(const Axis& a, int i, int crop, int dim) {
  Tap t;
  const float in = (crop > 1) ? a.start + (float)i * a.scale : a.single;
  // TF: extrapolate when (in < 0 || in > dim-1).  Written as the positive test so that a NaN
  // coordinate can never turn into a tap index.
  t.ok = (in >= 0.0f && in <= a.limit);
  const float f = floorf(in);
  t.lerp = in - f;
  int lo = (int)f, hi = (int)ceilf(in);
  if (PAD) {   // SYMMETRIC 1-px pad == edge replicate: padded[i] = src[clamp(i-1)]
    lo = min(max(lo - 1, 0), dim - 1);
    hi = min(max(hi - 1, 0), dim - 1);
  }
  if (!t.ok) { lo = 0; hi = 0; }     // never an address
  t.lo = lo; t.hi = hi;
  return t;
}

struct RoiBox {
  float y1n, x1n, y2n, x2n;   // normalised box (y1,x1,y2,x2) exactly as the reference builds it
  int Hs, Ws;                 // dims of the map crop_and_resize samples (padded for TP_ALIGN)
};

// roi = (x1, y1, x2, y2) in image pixels; H, W, st: the RoI's level; crop: samples per axis
template <int NORM>
__device__ __forceinline__ RoiBox roi_norm_box(float4 roi, int H, int W, float st, float image_h, float image_w, int crop) {
  constexpr bool PAD = (NORM == ODET_ROI_NORM_TP_ALIGN);
  float y1n, x1n, y2n, x2n;
  int Hs = H, Ws = W;     // dims of the map crop_and_resize samples (padded for TP_ALIGN)
  if (NORM == ODET_ROI_NORM_IMAGE) {
    y1n = roi.y / image_h; x1n = roi.x / image_w;                // roi_pooling.py:30-35
    y2n = roi.w / image_h; x2n = roi.z / image_w;
  } else if (NORM == ODET_ROI_NORM_STRIDE) {
    const float hm = (float)(H - 1), wm = (float)(W - 1);
    y1n = (roi.y / st) / hm; x1n = (roi.x / st) / wm;            // roi_pooling.py:64,69-74
    y2n = (roi.w / st) / hm; x2n = (roi.z / st) / wm;
  } else {
    const float off = PAD ? 1.0f : 0.0f;
    if (PAD) { Hs = H + 2; Ws = W + 2; }                         // roi_pooling.py:100
    float x0 = roi.x / st, y0 = roi.y / st;                      // :175
    float x1 = roi.z / st, y1 = roi.w / st;
    if (PAD) { x0 = x0 + off; y0 = y0 + off; x1 = x1 + off; y1 = y1 + off; }   // :101
    const float cs = (float)crop;
    const float sw = (x1 - x0) / cs, sh = (y1 - y0) / cs;        // :120-121
    const float imh = (float)(Hs - 1), imw = (float)(Ws - 1);
    x1n = (x0 + sw / 2.0f - 0.5f) / imw;                         // :124
    y1n = (y0 + sh / 2.0f - 0.5f) / imh;                         // :125
    const float nw = sw * (float)(crop - 1) / imw;               // :127
    const float nh = sh * (float)(crop - 1) / imh;               // :128
    y2n = y1n + nh; x2n = x1n + nw;                              // :130
  }
  return RoiBox{y1n, x1n, y2n, x2n, Hs, Ws};
}

// TF's bilinear sample of four taps in its own operation order (no FMA: the library is built with -ffp-contract=off)
__device__ __forceinline__ float4 lerp_tap(float4 tl, float4 tr, float4 bl, float4 br, float xw, float yw) {
  float4 r;
  float t, b;
  t = tl.x + (tr.x - tl.x) * xw; b = bl.x + (br.x - bl.x) * xw; r.x = t + (b - t) * yw;
  t = tl.y + (tr.y - tl.y) * xw; b = bl.y + (br.y - bl.y) * xw; r.y = t + (b - t) * yw;
  t = tl.z + (tr.z - tl.z) * xw; b = bl.z + (br.z - bl.z) * xw; r.z = t + (b - t) * yw;
  t = tl.w + (tr.w - tl.w) * xw; b = bl.w + (br.w - bl.w) * xw; r.w = t + (b - t) * yw;
  return r;
}

#endif  // ODET_ROI_TAPS_H_
