// Fused training losses: the four losses of model/losses.py:4-28 as base_fpn_model.py:278-301 / base_faster_rcnn_model.py:200-231
// call them, straight from the compact targets of csrc/targets.hip and the raw head outputs of a batch, with their gradients
// with respect to the head outputs.  No allocation, no host read, no float atomics.
//
// Arithmetic.  Every element operation is one float32 operation in the reference's order (the tree is built without FMA
// contraction); exp / log are d_exp32 / d_log32.  Every SUM is accumulated in float64 in a fixed order and rounded to float32
// once: the classes of a softmax row in ascending order; the 4 coordinates of an RPN row in ascending order; the 4C columns
// of a RoI row as 64 partial sums (partial l takes columns l, l + 64, ... in ascending order) added in ascending l; the rows
// of an image in ascending order.  tests/losses_np.py restates all of it with numpy's cumsum, bit for bit.
// These kernels are latency bound (a few hundred gathered rows per image); the only bandwidth-bound part is the zero fill of
// the dense RPN gradients.
#include "odet_internal.h"

#define LS_MAX_SAMPLES 1024   // RPN rows per image: one lane per row
#define LS_MAX_CLASSES 1024   // RoI classes: a wave keeps a row's exponentials in 4 KB of LDS
#define LS_MAX_ROWS 2048      // RoI-head rows per image: the row terms wait in LDS for the ordered sum
#define LS_RPN_THREADS 1024
#define LS_ROI_THREADS 512
#define LS_ROI_WAVES (LS_ROI_THREADS / ODET_WAVE)

// losses.py:17-22 constants, formed in float32 on the host
struct SlConst { float s2, thr, half_s2, half_inv; };

static SlConst sl_const(float sigma) {
  SlConst k;
  k.s2 = sigma * sigma;          // :17
  k.thr = 1.0f / k.s2;           // :21
  k.half_s2 = k.s2 / 2.0f;       // :22
  k.half_inv = 0.5f / k.s2;      // :22
  return k;
}

// losses.py:18-23 for one element, and d loss / d pred = outside * inside * (sigma_2 * d | sign(d))
__device__ __forceinline__ void d_smooth_l1(float pred, float tgt, float in, float out, SlConst k, float* loss, float* grad) {
  const float d = in * (pred - tgt);                                                          // :18-19
  const float ad = fabsf(d);                                                                  // :20
  const float sign = ad < k.thr ? 1.0f : 0.0f;                                                // :21
  const float in_loss = d * d * k.half_s2 * sign + (ad - k.half_inv) * (1.0f - sign);         // :22
  *loss = out * in_loss;                                                                      // :23
  const float slope = sign != 0.0f ? k.s2 * d : (d > 0.0f ? 1.0f : -1.0f);
  *grad = out * in * slope;
}

// ---------------------------------------------------------------------------------------------------------- RPN --
// offsets of an anchor's (bg, fg) logits inside one image's scores
__device__ __forceinline__ void d_rpn_score_offsets(int layout, int A, int idx, size_t* o0, size_t* o1) {
  if (layout == ODET_RPN_LAYOUT_FPN) {
    *o0 = (size_t)idx * 2;
    *o1 = *o0 + 1;
  } else {                                   // [A bg | A fg] per location
    const int loc = idx / A, an = idx - loc * A;
    *o0 = (size_t)loc * 2 * A + an;
    *o1 = *o0 + A;
  }
}

struct RpnLossArgs {
  const float* scores; const float4* deltas; int N, layout, A;
  const int32_t* sample_idx; const float4* sample_targets; const int32_t* counts; int S;
  SlConst k;
  float* losses; float2* row_gs; float4* row_gd;
};

// one workgroup per image, one lane per sampled row; lanes 0 and 64 add the row terms in order
__global__ void __launch_bounds__(LS_RPN_THREADS) k_rpn_loss(RpnLossArgs a) {
  __shared__ float s_ce[LS_MAX_SAMPLES];
  __shared__ double s_reg[LS_MAX_SAMPLES];
  const int b = blockIdx.x, t = threadIdx.x;
  int kfg = a.counts[b * 5 + 3], kbg = a.counts[b * 5 + 4];
  if (kfg < 0 || kbg < 0) { kfg = 0; kbg = 0; }            // (a counts row of -1: an image over the box limit)
  kfg = min(kfg, a.S);
  const int n = min(kfg + kbg, a.S);
  const float nf = (float)max(n, 1);
  const float outside = 1.0f / nf;                          // anchor_target.py:99-101, as odet_anchor_target forms it
  float ce = 0.0f;
  double reg = 0.0;
  float2 gs = make_float2(0.0f, 0.0f);
  float4 gd = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (t < n) {
    const int idx = a.sample_idx[(size_t)b * a.S + t];
    if ((unsigned)idx < (unsigned)a.N) {
      const bool fg = t < kfg;
      size_t o0, o1;
      d_rpn_score_offsets(a.layout, a.A, idx, &o0, &o1);
      const float* x = a.scores + (size_t)b * a.N * 2;
      const float x0 = x[o0], x1 = x[o1];
      const float mx = fmaxf(x0, x1);
      const float z0 = x0 - mx, z1 = x1 - mx;
      const float e0 = d_exp32(z0), e1 = d_exp32(z1);
      double s = 0.0;
      s += (double)e0;
      s += (double)e1;
      const float sf = (float)s;
      ce = d_log32(sf) - (fg ? z1 : z0);
      gs.x = (e0 / sf - (fg ? 0.0f : 1.0f)) / nf;
      gs.y = (e1 / sf - (fg ? 1.0f : 0.0f)) / nf;
      if (fg) {
        const float4 p = a.deltas[(size_t)b * a.N + idx];
        const float4 g = a.sample_targets[(size_t)b * a.S + t];
        float l;
        d_smooth_l1(p.x, g.x, 1.0f, outside, a.k, &l, &gd.x); reg += (double)l;
        d_smooth_l1(p.y, g.y, 1.0f, outside, a.k, &l, &gd.y); reg += (double)l;
        d_smooth_l1(p.z, g.z, 1.0f, outside, a.k, &l, &gd.z); reg += (double)l;
        d_smooth_l1(p.w, g.w, 1.0f, outside, a.k, &l, &gd.w); reg += (double)l;
      }
    }
  }
  if (t < a.S) {
    a.row_gs[(size_t)b * a.S + t] = gs;
    a.row_gd[(size_t)b * a.S + t] = gd;
  }
  s_ce[t] = ce;
  s_reg[t] = reg;
  __syncthreads();
  if (t == 0) {
    double acc = 0.0;
    for (int r = 0; r < n; ++r) acc += (double)s_ce[r];
    a.losses[b * 2 + 0] = (float)acc / nf;
  }
  if (t == ODET_WAVE) {
    double acc = 0.0;
    for (int r = 0; r < n; ++r) acc += s_reg[r];
    a.losses[b * 2 + 1] = (float)acc;                       // dim=[0,1]: a sum, the mean is over nothing
  }
}

// zero fill of two float buffers (16-byte aligned) with 16-byte stores; the tails (< 4 floats each) with scalar stores
__global__ void __launch_bounds__(256) k_zero_fill2(float* p0, size_t n0, float* p1, size_t n1) {
  const size_t v0 = n0 / 4, v1 = n1 / 4;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t first = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  for (size_t i = first; i < v0 + v1; i += stride) {
    if (i < v0) ((float4*)p0)[i] = z;
    else ((float4*)p1)[i - v0] = z;
  }
  if (first < n0 - v0 * 4) p0[v0 * 4 + first] = 0.0f;
  if (first < n1 - v1 * 4) p1[v1 * 4 + first] = 0.0f;
}

struct RpnBwdArgs {
  const int32_t* sample_idx; const float2* row_gs; const float4* row_gd; const float* upstream;
  int N, layout, A, S;
  float* grad_scores; float4* grad_deltas;
};

// sample_idx holds no duplicates: every address is written by one lane
__global__ void __launch_bounds__(LS_RPN_THREADS) k_rpn_loss_scatter(RpnBwdArgs a) {
  const int b = blockIdx.x, t = threadIdx.x;
  if (t >= a.S) return;
  const int idx = a.sample_idx[(size_t)b * a.S + t];
  if ((unsigned)idx >= (unsigned)a.N) return;
  if (a.grad_scores) {
    const float up = a.upstream[b * 2 + 0];
    const float2 g = a.row_gs[(size_t)b * a.S + t];
    size_t o0, o1;
    d_rpn_score_offsets(a.layout, a.A, idx, &o0, &o1);
    float* out = a.grad_scores + (size_t)b * a.N * 2;
    out[o0] = up * g.x;
    out[o1] = up * g.y;
  }
  if (a.grad_deltas) {
    const float up = a.upstream[b * 2 + 1];
    const float4 g = a.row_gd[(size_t)b * a.S + t];
    a.grad_deltas[(size_t)b * a.N + idx] = make_float4(up * g.x, up * g.y, up * g.z, up * g.w);
  }
}

static int rpn_layout_check(const char* who, int num_anchors, int batch, int layout, int A, int S) {
  ODET_REQUIRE(batch >= 0 && num_anchors >= 0, "%s: negative size", who);
  ODET_REQUIRE(layout == ODET_RPN_LAYOUT_FPN || layout == ODET_RPN_LAYOUT_FRCNN, "%s: unknown score layout %d", who, layout);
  ODET_REQUIRE(layout == ODET_RPN_LAYOUT_FPN || (A > 0 && num_anchors % A == 0),
               "%s: %d anchors are not a multiple of %d anchors per location", who, num_anchors, A);
  if (batch > 64) return odet_set_error(ODET_E_LIMIT, "%s: batch %d exceeds 64", who, batch);
  if (S < 1 || S > LS_MAX_SAMPLES)
    return odet_set_error(ODET_E_LIMIT, "%s: total_num_samples %d outside 1..%d", who, S, LS_MAX_SAMPLES);
  return ODET_OK;
}

extern "C" int odet_rpn_loss(const float* scores, const float* deltas, int num_anchors, int batch, int layout,
                             int anchors_per_location, const int32_t* sample_idx, const float* sample_targets,
                             const int32_t* counts, int total_num_samples, float sigma, float* losses,
                             float* row_grad_scores, float* row_grad_deltas, odet_stream_t stream) {
  const int rc = rpn_layout_check("odet_rpn_loss", num_anchors, batch, layout, anchors_per_location, total_num_samples);
  if (rc != ODET_OK) return rc;
  if (batch == 0) return ODET_OK;
  ODET_REQUIRE(scores && deltas && sample_idx && sample_targets && counts && losses && row_grad_scores && row_grad_deltas,
               "odet_rpn_loss: null pointer");
  ODET_REQUIRE(sigma > 0.0f, "odet_rpn_loss: sigma must be positive");
  RpnLossArgs a;
  a.scores = scores; a.deltas = (const float4*)deltas; a.N = num_anchors; a.layout = layout; a.A = anchors_per_location;
  a.sample_idx = sample_idx; a.sample_targets = (const float4*)sample_targets; a.counts = counts; a.S = total_num_samples;
  a.k = sl_const(sigma);
  a.losses = losses; a.row_gs = (float2*)row_grad_scores; a.row_gd = (float4*)row_grad_deltas;
  hipLaunchKernelGGL(k_rpn_loss, dim3(batch), dim3(LS_RPN_THREADS), 0, (hipStream_t)stream, a);
  ODET_LAUNCH_CHECK();
  return ODET_OK;
}

extern "C" int odet_rpn_loss_backward(const int32_t* sample_idx, const float* row_grad_scores, const float* row_grad_deltas,
                                      const float* upstream, int num_anchors, int batch, int layout, int anchors_per_location,
                                      int total_num_samples, float* grad_scores, float* grad_deltas, odet_stream_t stream) {
  const int rc = rpn_layout_check("odet_rpn_loss_backward", num_anchors, batch, layout, anchors_per_location, total_num_samples);
  if (rc != ODET_OK) return rc;
  if (batch == 0) return ODET_OK;
  ODET_REQUIRE(sample_idx && row_grad_scores && row_grad_deltas && upstream, "odet_rpn_loss_backward: null pointer");
  if (!grad_scores && !grad_deltas) return ODET_OK;
  ODET_REQUIRE(((uintptr_t)grad_scores | (uintptr_t)grad_deltas) % 16 == 0,
               "odet_rpn_loss_backward: the gradients must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const size_t n0 = grad_scores ? (size_t)batch * num_anchors * 2 : 0, n1 = grad_deltas ? (size_t)batch * num_anchors * 4 : 0;
  if (n0 + n1 > 0) {
    const size_t vec = n0 / 4 + n1 / 4;
    const size_t blocks = (vec + 256 * 4 - 1) / (256 * 4);             // four stores per lane
    hipLaunchKernelGGL(k_zero_fill2, dim3((unsigned)(blocks < 1 ? 1 : (blocks > 8192 ? 8192 : blocks))), dim3(256), 0, st,
                       grad_scores, n0, grad_deltas, n1);
    ODET_LAUNCH_CHECK();
  }
  RpnBwdArgs a;
  a.sample_idx = sample_idx; a.row_gs = (const float2*)row_grad_scores; a.row_gd = (const float4*)row_grad_deltas;
  a.upstream = upstream; a.N = num_anchors; a.layout = layout; a.A = anchors_per_location; a.S = total_num_samples;
  a.grad_scores = grad_scores; a.grad_deltas = (float4*)grad_deltas;
  hipLaunchKernelGGL(k_rpn_loss_scatter, dim3(batch), dim3(LS_RPN_THREADS), 0, st, a);   // (after the fill: stream order)
  ODET_LAUNCH_CHECK();
  return ODET_OK;
}

// ---------------------------------------------------------------------------------------------------------- RoI --
struct RoiLossArgs {
  const float* scores; const float* deltas; int R, C;
  const int32_t* labels; const float* targets; const float* inside; const float* outside; const int32_t* counts; int S;
  const int32_t* row_map;
  SlConst k;
  const float* upstream;
  float* losses; float* gs; float* gd;
};

// one workgroup per image, one wave per head row (coalesced reads and gradient writes); every lane of a wave adds the same
// values in the same order, so the wave's sums need no LDS and no barrier
__global__ void __launch_bounds__(LS_ROI_THREADS) k_roi_loss(RoiLossArgs a) {
  __shared__ float s_e[LS_ROI_WAVES][LS_MAX_CLASSES];      // a lane re-reads only what it wrote itself
  __shared__ float s_ce[LS_MAX_ROWS];
  __shared__ double s_reg[LS_MAX_ROWS];
  const int b = blockIdx.x, wave = threadIdx.x / ODET_WAVE, lane = threadIdx.x % ODET_WAVE;
  int rows = a.counts[b * 4 + 3];
  rows = min(max(rows, 0), a.S);                            // (a counts row of -1: nothing written)
  const float nf = (float)max(rows, 1);
  const float up_cls = a.upstream ? a.upstream[b * 2 + 0] : 1.0f;
  const float up_reg = a.upstream ? a.upstream[b * 2 + 1] : 1.0f;
  const int C = a.C, W = 4 * a.C;
  for (int r = wave; r < a.R; r += LS_ROI_WAVES) {
    const int m = a.row_map ? a.row_map[(size_t)b * a.R + r] : r;
    const int label = (m >= 0 && m < rows) ? a.labels[(size_t)b * a.S + m] : -1;
    const bool valid = (unsigned)label < (unsigned)C;       // (uniform over the wave)
    const float* x = a.scores + ((size_t)b * a.R + r) * C;
    float* gs = a.gs ? a.gs + ((size_t)b * a.R + r) * C : nullptr;
    float* gd = a.gd ? a.gd + ((size_t)b * a.R + r) * W : nullptr;
    float ce = 0.0f;
    double reg = 0.0;
    if (valid) {
      float mx = -INFINITY;
      for (int j = lane; j < C; j += ODET_WAVE) mx = fmaxf(mx, x[j]);
#pragma unroll
      for (int o = ODET_WAVE / 2; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
      double s = 0.0;
      for (int j0 = 0; j0 < C; j0 += ODET_WAVE) {           // classes in ascending order
        const int j = j0 + lane;
        float e = 0.0f;
        if (j < C) { e = d_exp32(x[j] - mx); s_e[wave][j] = e; }
        const int cnt = min(ODET_WAVE, C - j0);
        for (int l = 0; l < cnt; ++l) s += (double)__shfl(e, l);
      }
      const float sf = (float)s;
      ce = d_log32(sf) - (x[label] - mx);
      if (gs)
        for (int j = lane; j < C; j += ODET_WAVE) gs[j] = up_cls * ((s_e[wave][j] / sf - (j == label ? 1.0f : 0.0f)) / nf);
      const float* pr = a.deltas + ((size_t)b * a.R + r) * W;
      const float* tg = a.targets + ((size_t)b * a.S + m) * W;
      const float* in = a.inside + ((size_t)b * a.S + m) * W;
      const float* ou = a.outside + ((size_t)b * a.S + m) * W;
      double part = 0.0;
      for (int c = lane; c < W; c += ODET_WAVE) {
        float l, g;
        d_smooth_l1(pr[c], tg[c], in[c], ou[c], a.k, &l, &g);
        part += (double)l;
        if (gd) gd[c] = up_reg * (g / nf);
      }
      for (int l = 0; l < ODET_WAVE; ++l) reg += __shfl(part, l);
    } else {
      if (gs) for (int j = lane; j < C; j += ODET_WAVE) gs[j] = 0.0f;
      if (gd) for (int c = lane; c < W; c += ODET_WAVE) gd[c] = 0.0f;
    }
    if (lane == 0) { s_ce[r] = ce; s_reg[r] = reg; }
  }
  __syncthreads();
  if (!a.losses) return;
  if (threadIdx.x == 0) {
    double acc = 0.0;
    for (int r = 0; r < a.R; ++r) acc += (double)s_ce[r];
    a.losses[b * 2 + 0] = (float)acc / nf;
  }
  if (threadIdx.x == ODET_WAVE) {
    double acc = 0.0;
    for (int r = 0; r < a.R; ++r) acc += s_reg[r];
    a.losses[b * 2 + 1] = (float)acc / nf;
  }
}

extern "C" int odet_roi_loss(const float* scores, const float* deltas, int num_rows, int num_classes, int batch,
                             const int32_t* final_labels, const float* targets, const float* inside, const float* outside,
                             const int32_t* counts, int total_num_samples, const int32_t* row_map, float sigma,
                             const float* upstream, float* losses, float* grad_scores, float* grad_deltas,
                             odet_stream_t stream) {
  ODET_REQUIRE(batch >= 0 && num_rows >= 0, "odet_roi_loss: negative size");
  ODET_REQUIRE(num_classes > 0, "odet_roi_loss: num_classes must be positive");
  if (num_classes > LS_MAX_CLASSES)
    return odet_set_error(ODET_E_LIMIT, "odet_roi_loss: %d classes exceed %d", num_classes, LS_MAX_CLASSES);
  if (num_rows > LS_MAX_ROWS) return odet_set_error(ODET_E_LIMIT, "odet_roi_loss: %d rows exceed %d", num_rows, LS_MAX_ROWS);
  if (batch > 64) return odet_set_error(ODET_E_LIMIT, "odet_roi_loss: batch %d exceeds 64", batch);
  if (total_num_samples < 1 || total_num_samples > LS_MAX_SAMPLES)
    return odet_set_error(ODET_E_LIMIT, "odet_roi_loss: total_num_samples %d outside 1..%d", total_num_samples, LS_MAX_SAMPLES);
  if (batch == 0) return ODET_OK;
  ODET_REQUIRE((num_rows == 0 || (scores && deltas)) && final_labels && targets && inside && outside && counts,
               "odet_roi_loss: null pointer");             // (no head row: the losses are 0, nothing of the head is read)
  ODET_REQUIRE(sigma > 0.0f, "odet_roi_loss: sigma must be positive");
  if (!losses && !grad_scores && !grad_deltas) return ODET_OK;
  RoiLossArgs a;
  a.scores = scores; a.deltas = deltas; a.R = num_rows; a.C = num_classes;
  a.labels = final_labels; a.targets = targets; a.inside = inside; a.outside = outside; a.counts = counts;
  a.S = total_num_samples; a.row_map = row_map; a.k = sl_const(sigma); a.upstream = upstream;
  a.losses = losses; a.gs = grad_scores; a.gd = grad_deltas;
  hipLaunchKernelGGL(k_roi_loss, dim3(batch), dim3(LS_ROI_THREADS), 0, (hipStream_t)stream, a);
  ODET_LAUNCH_CHECK();
  return ODET_OK;
}
