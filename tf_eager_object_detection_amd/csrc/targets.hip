// Fused training targets: model/anchor_target.py:49-107 and model/proposal_target.py:54-124 for a batch of images, without the
// dense IoU matrix and without a host read.  The pair loop runs twice (column maxima, then everything that depends on them);
// d_pair_iou gives both passes the same bits.  The random sub-sampling is a counter-based rule the CPU can restate exactly:
// every candidate i owns the 64-bit key  philox((i, image_id, stream, 0), seed)[0:2]  and "keep k" means the k smallest
// (key, i) pairs -- a uniformly random k-subset, as the reference's shuffle-and-slice.  The k-th pair is found by a radix
// select over the 84-bit number key * 2^20 + i in 12-bit digits (no two candidates share it, so the select always ends
// with an exact threshold); whoever needs the decision later compares its own pair with that threshold.
// Every cross-workgroup combination is an integer maximum or an integer sum: results do not depend on arrival order.
#include "odet_internal.h"

#define TG_MAX_GT 1024         // ground-truth boxes per image (16 KB of LDS)
#define TG_MAX_SAMPLES 1024    // total_num_samples: one sampled row per thread of the ordering workgroup
#define TG_MAX_INDEX (1 << 20) // candidates per image: the index is the low 20 bits of the selection number
#define TG_BLOCK 256
#define TG_SEL_THREADS 1024
#define TG_BINS 4096

// (the Philox streams TG_STREAM_* and the generator itself, odet_philox2: odet_internal.h, shared with preprocess.hip)
// per-candidate class byte in the workspace
enum { TG_FG = 1, TG_BG = 0, TG_IGNORE = -1, TG_OUTSIDE = -2 };

#ifdef ODET_DIAG
// Diagnostic build only (-DODET_DIAG: tools/libodet_hip_diag.so, include/odet_diag.h; the shipped library has neither the entry
// point nor the field): every SELECTION key (d_key64 and the stored high word of d_key_hi, all four streams) is ANDed with a
// mask that travels next to the seed, so that tests can make keys collide and walk the deep levels of d_tg_radix_select.
// The with-replacement draw (stream 4) is no selection key and stays as it is.  ~0 clears.
#include <atomic>
struct TgSeed { uint32_t lo, hi; unsigned long long mask; };
#define TG_KEY_MASK(s, v) ((v) & (s).mask)
#define TG_KEY_MASK_HI(s, v) ((v) & (uint32_t)((s).mask >> 32))
static std::atomic<unsigned long long> g_tg_key_mask{~0ull};
extern "C" int odet_debug_tg_key_mask(unsigned long long and_mask) {
  g_tg_key_mask.store(and_mask);
  return ODET_OK;
}
#define TG_SEED_DIAG(a) (a).seed.mask = g_tg_key_mask.load()
#else
struct TgSeed { uint32_t lo, hi; };
#define TG_KEY_MASK(s, v) (v)
#define TG_KEY_MASK_HI(s, v) (v)
#define TG_SEED_DIAG(a) ((void)0)
#endif
struct TgThr { unsigned long long key; uint32_t idx; int32_t none; };   // selected  <=>  !none && (key64, i) <= (key, idx)

__device__ __forceinline__ unsigned long long d_key64(uint32_t stream, uint32_t image, uint32_t i, TgSeed s) {
  uint32_t w0, w1;
  odet_philox2(i, image, stream, 0u, s.lo, s.hi, &w0, &w1);
  return TG_KEY_MASK(s, ((unsigned long long)w0 << 32) | w1);
}
__device__ __forceinline__ uint32_t d_key_hi(uint32_t stream, uint32_t image, uint32_t i, TgSeed s) {
  uint32_t w0, w1;
  odet_philox2(i, image, stream, 0u, s.lo, s.hi, &w0, &w1);
  return TG_KEY_MASK_HI(s, w0);
}

// is candidate i (stored high key word w0) among the kept ones?  The low word is only computed on the threshold's high word.
__device__ __forceinline__ bool d_tg_selected(TgThr t, uint32_t w0, uint32_t i, uint32_t stream, uint32_t image, TgSeed s) {
  if (t.none) return false;
  const uint32_t thi = (uint32_t)(t.key >> 32);
  if (w0 != thi) return w0 < thi;
  const unsigned long long key = d_key64(stream, image, i, s);
  return key < t.key || (key == t.key && i <= t.idx);
}

// The k-th smallest (key64, i) among the n_cand candidates { i < n : cls[i] == want } as a threshold, by ONE workgroup of
// TG_SEL_THREADS threads: digit l of V = key64 * 2^20 + i (12 bits, most significant first) is histogrammed over the candidates
// that agree with the digits chosen so far; the digit where the running count reaches the rows still needed is chosen.  A level
// whose chosen digit holds exactly the rows still needed ends the walk (all of them are kept).  Levels 0 and 1 read the stored
// high word only.  hist: LDS [TG_BINS], sh: LDS [24].  Every thread returns the same threshold.
__device__ TgThr d_tg_radix_select(const int8_t* __restrict__ cls, const uint32_t* __restrict__ khi, int n, int want, int k,
                                   int n_cand, uint32_t stream, uint32_t image, TgSeed seed, int* hist, int* sh) {
  TgThr t;
  t.key = ~0ull; t.idx = 0xFFFFFFFFu; t.none = (k <= 0) ? 1 : 0;
  if (k <= 0 || n_cand <= k) return t;            // nothing / everything kept (uniform over the workgroup)
  unsigned long long pk = 0;
  uint32_t pi = 0;
  int need = k;
  for (int l = 0; l < 7; ++l) {
    for (int b = threadIdx.x; b < TG_BINS; b += TG_SEL_THREADS) hist[b] = 0;
    __syncthreads();
    const int shift = 72 - 12 * l;                // position of digit l in V
    for (int i = threadIdx.x; i < n; i += TG_SEL_THREADS) {
      if (cls[i] != want) continue;
      const uint32_t w0 = khi[i];
      unsigned long long key = (unsigned long long)w0 << 32;
      if (l == 1 && ((w0 ^ (uint32_t)(pk >> 32)) >> 20) != 0) continue;
      if (l >= 2) {
        if (((w0 ^ (uint32_t)(pk >> 32)) >> 8) != 0) continue;
        key = d_key64(stream, image, (uint32_t)i, seed);
        if (l <= 5 ? (((key ^ pk) >> (64 - 12 * l)) != 0) : (key != pk || (((uint32_t)i ^ pi) >> 12) != 0)) continue;
      }
      int d;
      if (shift >= 20) d = (int)((key >> (shift - 20)) & 0xFFFu);
      else if (l == 5) d = (int)(((key & 0xFu) << 8) | (((uint32_t)i >> 12) & 0xFFu));
      else d = i & 0xFFF;
      atomicAdd(&hist[d], 1);
    }
    __syncthreads();
    // the digit where the inclusive running count first reaches `need`: thread t owns bins 4t .. 4t+3
    int c[4], s = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) { c[q] = hist[threadIdx.x * 4 + q]; s += c[q]; }
    int total;
    int ex = block_excl_scan(s, sh, &total);
    if (ex < need && need <= ex + s) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (ex < need && need <= ex + c[q]) { sh[17] = threadIdx.x * 4 + q; sh[18] = ex; sh[19] = c[q]; }
        ex += c[q];
      }
    }
    __syncthreads();
    const int d = sh[17], below = sh[18], cnt = sh[19];
    __syncthreads();
    need -= below;
    if (shift >= 20) pk |= (unsigned long long)d << (shift - 20);
    else if (l == 5) { pk |= (unsigned long long)(d >> 8); pi |= (uint32_t)(d & 0xFF) << 12; }
    else pi |= (uint32_t)d;
    if (cnt == need) {                             // the whole digit is kept: the remaining low bits of the threshold are ones
      if (shift >= 20) { pk |= (1ull << (shift - 20)) - 1ull; pi = 0xFFFFFFFFu; }
      else pi |= (1u << shift) - 1u;
      break;
    }
  }
  t.key = pk; t.idx = pi;
  return t;
}

// rank of (key, idx) among m listed pairs in LDS (strict lexicographic order; all pairs differ)
__device__ __forceinline__ int d_tg_rank(const unsigned long long* keys, const int* idx, int m, unsigned long long key, int i) {
  int r = 0;
  for (int j = 0; j < m; ++j) {
    const unsigned long long kj = keys[j];
    r += (kj < key || (kj == key && idx[j] < i)) ? 1 : 0;
  }
  return r;
}

// Zero fill of a workspace head (column maxima, counters) as a kernel node, not a memset node: the words cleared are the same.
// Property relied on: a captured graph of these calls can be replayed any number of times with eager calls in between, and
// every replay starts from cleared counters (tests/test_losses_gpu.py replays twice; DESIGN 3.9 has what was seen otherwise).
__global__ void __launch_bounds__(TG_BLOCK) k_tg_zero(uint32_t* p, size_t words) {
  const size_t i = (size_t)blockIdx.x * TG_BLOCK + threadIdx.x;
  if (i < words) p[i] = 0u;
}

static int tg_zero_head(void* workspace, size_t head_bytes, hipStream_t st) {
  const size_t words = (head_bytes + 3) / 4;               // (the head ends on a 4-byte boundary inside the workspace)
  hipLaunchKernelGGL(k_tg_zero, dim3((unsigned)((words + TG_BLOCK - 1) / TG_BLOCK)), dim3(TG_BLOCK), 0, st, (uint32_t*)workspace, words);
  ODET_LAUNCH_CHECK();
  return ODET_OK;
}

__device__ __forceinline__ bool d_inside(float4 a, float wmax, float hmax) {
  return a.x >= 0.0f && a.y >= 0.0f && a.z <= wmax && a.w <= hmax;      // bbox_tf.py:94-99
}

// ------------------------------------------------------------------------------------------------- anchor targets --
struct AtArgs {
  const float4* anchors; int N;
  const float4* gt; const int32_t* gt_off; int B;
  float wmax, hmax, pos, neg;
  int S, max_pos;
  Vec4 means, stds;
  TgSeed seed; uint32_t first_image;
  // workspace
  uint32_t* colmax;     // [B, TG_MAX_GT] bit patterns of the column maxima (zero-filled per call)
  int32_t* cnt;         // [B, 8]: inside, fg, bg candidates; list slots of fg, bg (zero-filled per call)
  TgThr* thr;           // [B, 2]
  int8_t* cls;          // [B, N]
  uint32_t* khi;        // [B, N]
  int32_t* amax;        // [B, N] (the caller's `argmax` when given)
  int32_t* list;        // [B, 2, S] kept anchors in arrival order
  // outputs (nullable except counts, sample_idx, sample_targets)
  float* labels; float4* targets; float4* inside; float4* outside;
  int32_t* sample_idx; float4* sample_targets; int32_t* counts; int32_t* labels_before;
};

// pass 1: column maxima.  One lane per anchor, the image's boxes in LDS; a lane touches the LDS maximum of a column only when
// its IoU beats the value it reads there (the value only grows, so a stale read costs one redundant atomic, never a miss),
// and the workgroup touches the global maximum under the same test.  Integer maxima on the bit pattern (IoU >= 0).
__global__ void __launch_bounds__(TG_BLOCK) k_at_colmax(AtArgs a) {
  __shared__ float4 s_gt[TG_MAX_GT];
  __shared__ uint32_t s_max[TG_MAX_GT];
  const int b = blockIdx.y;
  const int g0 = a.gt_off[b], G = a.gt_off[b + 1] - g0;
  if (G <= 0 || G > TG_MAX_GT) return;
  for (int g = threadIdx.x; g < G; g += TG_BLOCK) { s_gt[g] = a.gt[g0 + g]; s_max[g] = 0u; }
  __syncthreads();
  const int i = blockIdx.x * TG_BLOCK + threadIdx.x;
  if (i < a.N) {
    const float4 p = a.anchors[i];
    if (d_inside(p, a.wmax, a.hmax)) {
      for (int g = 0; g < G; ++g) {
        const uint32_t v = __float_as_uint(d_pair_iou(p, s_gt[g]));
        if (v > s_max[g]) atomicMax(&s_max[g], v);
      }
    }
  }
  __syncthreads();
  uint32_t* cm = a.colmax + (size_t)b * TG_MAX_GT;
  for (int g = threadIdx.x; g < G; g += TG_BLOCK) {
    const uint32_t v = s_max[g];
    if (v > cm[g]) atomicMax(&cm[g], v);
  }
}

// pass 2: row maximum, first arg-maximum, the gt-argmax test against the finished column maxima, labels before sampling
// (anchor_target.py:61-69), the candidates' key words and the three counts.
__global__ void __launch_bounds__(TG_BLOCK) k_at_label(AtArgs a) {
  __shared__ float4 s_gt[TG_MAX_GT];
  __shared__ float s_max[TG_MAX_GT];
  __shared__ int s_cnt[3];
  const int b = blockIdx.y;
  const int g0 = a.gt_off[b];
  int G = a.gt_off[b + 1] - g0;
  const bool bad = G > TG_MAX_GT || G < 0;
  if (bad) G = 0;
  for (int g = threadIdx.x; g < G; g += TG_BLOCK) {
    s_gt[g] = a.gt[g0 + g];
    s_max[g] = __uint_as_float(a.colmax[(size_t)b * TG_MAX_GT + g]);
  }
  if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const int i = blockIdx.x * TG_BLOCK + threadIdx.x;
  int lab = TG_OUTSIDE, am = -1;
  if (i < a.N && !bad) {
    const float4 p = a.anchors[i];
    if (d_inside(p, a.wmax, a.hmax)) {
      float mx = 0.0f;
      bool isarg = false;
      if (G > 0) {
        mx = -1.0f;
        for (int g = 0; g < G; ++g) {
          const float v = d_pair_iou(p, s_gt[g]);
          if (v > mx) { mx = v; am = g; }          // strict: the FIRST maximum (:61)
          isarg = isarg || (v == s_max[g]);        // :64 (a box that meets no inside anchor has maximum 0: sic)
        }
      }
      lab = TG_IGNORE;
      if (mx < a.neg) lab = TG_BG;                 // :67
      if (isarg) lab = TG_FG;                      // :68
      if (mx >= a.pos) lab = TG_FG;                // :69
    }
  }
  if (i < a.N) {
    const size_t o = (size_t)b * a.N + i;
    a.cls[o] = (int8_t)lab;
    a.amax[o] = am;
    if (a.labels_before) a.labels_before[o] = lab == TG_OUTSIDE ? -1 : lab;
    if (lab >= 0)
      a.khi[o] = d_key_hi(lab == TG_FG ? TG_STREAM_ANCHOR_FG : TG_STREAM_ANCHOR_BG, a.first_image + b, (uint32_t)i, a.seed);
  }
  const int lane = threadIdx.x & 63;
  const unsigned long long m_in = __ballot(lab != TG_OUTSIDE), m_fg = __ballot(lab == TG_FG), m_bg = __ballot(lab == TG_BG);
  if (lane == 0) {
    if (m_in) atomicAdd(&s_cnt[0], __popcll(m_in));
    if (m_fg) atomicAdd(&s_cnt[1], __popcll(m_fg));
    if (m_bg) atomicAdd(&s_cnt[2], __popcll(m_bg));
  }
  __syncthreads();
  if (threadIdx.x < 3 && s_cnt[threadIdx.x]) atomicAdd(&a.cnt[b * 8 + threadIdx.x], s_cnt[threadIdx.x]);
}

// the two thresholds of an image (blockIdx.x: 0 foreground, 1 background) and its row of `counts`
__global__ void __launch_bounds__(TG_SEL_THREADS) k_at_select(AtArgs a) {
  __shared__ int hist[TG_BINS];
  __shared__ int sh[24];
  const int b = blockIdx.y, kind = blockIdx.x;
  const int G = a.gt_off[b + 1] - a.gt_off[b];
  const int n_in = a.cnt[b * 8 + 0], n_fg = a.cnt[b * 8 + 1], n_bg = a.cnt[b * 8 + 2];
  const int k_fg = min(n_fg, a.max_pos);                     // :73-77
  const int k_bg = min(n_bg, max(a.S - k_fg, 0));            // :78-84
  const TgThr t = d_tg_radix_select(a.cls + (size_t)b * a.N, a.khi + (size_t)b * a.N, a.N, kind == 0 ? TG_FG : TG_BG,
                                    kind == 0 ? k_fg : k_bg, kind == 0 ? n_fg : n_bg,
                                    kind == 0 ? TG_STREAM_ANCHOR_FG : TG_STREAM_ANCHOR_BG, a.first_image + b, a.seed, hist, sh);
  if (threadIdx.x == 0) {
    a.thr[b * 2 + kind] = t;
    if (kind == 0) {
      const bool bad = G > TG_MAX_GT || G < 0;
      int32_t* c = a.counts + b * 5;
      c[0] = bad ? -1 : n_in; c[1] = bad ? -1 : n_fg; c[2] = bad ? -1 : n_bg; c[3] = bad ? -1 : k_fg; c[4] = bad ? -1 : k_bg;
    }
  }
}

// final labels and the dense surface (:86-107); kept anchors are also appended to the image's two lists
__global__ void __launch_bounds__(TG_BLOCK) k_at_write(AtArgs a) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * TG_BLOCK + threadIdx.x;
  if (i >= a.N) return;
  const size_t o = (size_t)b * a.N + i;
  const int lab = a.cls[o];
  int fin = -1;
  if (lab >= 0) {
    const int kind = lab == TG_FG ? 0 : 1;
    if (d_tg_selected(a.thr[b * 2 + kind], a.khi[o], (uint32_t)i, kind == 0 ? TG_STREAM_ANCHOR_FG : TG_STREAM_ANCHOR_BG,
                      a.first_image + b, a.seed)) {
      fin = lab;
      const int slot = atomicAdd(&a.cnt[b * 8 + 3 + kind], 1);
      if (slot < a.S) a.list[((size_t)b * 2 + kind) * a.S + slot] = i;
    }
  }
  if (a.labels) a.labels[o] = (float)fin;
  if (a.targets) {
    float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const int am = a.amax[o];
    if (lab != TG_OUTSIDE && am >= 0) t = d_encode_box(a.anchors[i], a.gt[a.gt_off[b] + am], a.means.v, a.stds.v);   // :88-90
    a.targets[o] = t;
  }
  if (a.inside) { const float v = fin == 1 ? 1.0f : 0.0f; a.inside[o] = make_float4(v, v, v, v); }                       // :93-95
  if (a.outside) {
    const int n_fg = a.cnt[b * 8 + 1], n_bg = a.cnt[b * 8 + 2];
    const int k_fg = min(n_fg, a.max_pos), k_bg = min(n_bg, max(a.S - k_fg, 0));
    const float v = fin >= 0 ? 1.0f / (float)(k_fg + k_bg) : 0.0f;                                                        // :99-101
    a.outside[o] = make_float4(v, v, v, v);
  }
}

// the compact form: kept foreground anchors in ascending index order, then the background ones, -1 / 0 padding
__global__ void __launch_bounds__(TG_SEL_THREADS) k_at_compact(AtArgs a) {
  __shared__ int s_idx[TG_MAX_SAMPLES];
  const int b = blockIdx.x, t = threadIdx.x;
  const int n_fg = a.cnt[b * 8 + 1], n_bg = a.cnt[b * 8 + 2];
  const int k_fg = min(n_fg, a.max_pos), k_bg = min(n_bg, max(a.S - k_fg, 0));
  const int32_t* lf = a.list + (size_t)b * 2 * a.S;
  const int32_t* lb = lf + a.S;
  if (t < k_fg) s_idx[t] = lf[t];
  else if (t < k_fg + k_bg) s_idx[t] = lb[t - k_fg];
  __syncthreads();
  int pos = -1, mine = -1;
  if (t < k_fg + k_bg) {
    mine = s_idx[t];
    const int lo = t < k_fg ? 0 : k_fg, hi = t < k_fg ? k_fg : k_fg + k_bg;
    pos = lo;
    for (int j = lo; j < hi; ++j) pos += s_idx[j] < mine ? 1 : 0;
  }
  if (pos >= 0 && (unsigned)mine < (unsigned)a.N) {
    const int am = a.amax[(size_t)b * a.N + mine];         // (-1: an image without ground truth, targets 0)
    a.sample_idx[(size_t)b * a.S + pos] = mine;
    a.sample_targets[(size_t)b * a.S + pos] =
        am >= 0 ? d_encode_box(a.anchors[mine], a.gt[a.gt_off[b] + am], a.means.v, a.stds.v) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  } else if (t < a.S) {
    a.sample_idx[(size_t)b * a.S + t] = -1;
    a.sample_targets[(size_t)b * a.S + t] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
}

static size_t at_head_bytes(int B) { return odet_align_up((size_t)B * TG_MAX_GT * 4, 256) + odet_align_up((size_t)B * 8 * 4, 256); }

extern "C" size_t odet_anchor_target_workspace_bytes(int num_anchors, int batch, int total_num_samples) {
  const size_t n = num_anchors < 0 ? 0 : (size_t)num_anchors, B = batch < 1 ? 1 : (size_t)batch;
  const size_t S = total_num_samples < 1 ? 1 : (size_t)total_num_samples;
  return at_head_bytes((int)B) + odet_align_up(B * 2 * sizeof(TgThr), 256) + odet_align_up(B * n, 256) +
         2 * odet_align_up(B * n * 4, 256) + odet_align_up(B * 2 * S * 4, 256) + 512;
}

extern "C" int odet_anchor_target(const float* anchors, int num_anchors, const float* gt_boxes, const int32_t* gt_offsets,
                                  int batch, int image_h, int image_w, float pos_iou_threshold, float neg_iou_threshold,
                                  int total_num_samples, int max_pos_samples, const float* means, const float* stds,
                                  uint64_t seed, uint32_t first_image_id, float* labels, float* targets, float* inside,
                                  float* outside, int32_t* sample_idx, float* sample_targets, int32_t* counts,
                                  int32_t* labels_before_sampling, int32_t* argmax, void* workspace, size_t workspace_bytes,
                                  odet_stream_t stream) {
  ODET_REQUIRE(batch >= 0 && num_anchors >= 0, "odet_anchor_target: negative size");
  if (batch == 0) return ODET_OK;
  ODET_REQUIRE(anchors && gt_boxes && gt_offsets && means && stds && sample_idx && sample_targets && counts,
               "odet_anchor_target: null pointer");
  ODET_REQUIRE(image_h > 0 && image_w > 0, "odet_anchor_target: bad image shape");
  if (batch > 64) return odet_set_error(ODET_E_LIMIT, "odet_anchor_target: batch %d exceeds 64", batch);
  if (num_anchors > TG_MAX_INDEX)
    return odet_set_error(ODET_E_LIMIT, "odet_anchor_target: %d anchors exceed %d", num_anchors, TG_MAX_INDEX);
  if (total_num_samples < 1 || total_num_samples > TG_MAX_SAMPLES)
    return odet_set_error(ODET_E_LIMIT, "odet_anchor_target: total_num_samples %d outside 1..%d", total_num_samples, TG_MAX_SAMPLES);
  ODET_REQUIRE(max_pos_samples >= 0 && max_pos_samples <= total_num_samples,
               "odet_anchor_target: max_pos_samples must lie in 0..total_num_samples");
  const size_t need = odet_anchor_target_workspace_bytes(num_anchors, batch, total_num_samples);
  if (!workspace || workspace_bytes < need)
    return odet_set_error(ODET_E_WORKSPACE, "odet_anchor_target: workspace too small (%zu < %zu)", workspace_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  const size_t B = (size_t)batch, n = (size_t)num_anchors;
  OdetArena ar{(char*)workspace, workspace_bytes, 0};
  AtArgs a;
  a.anchors = (const float4*)anchors; a.N = num_anchors; a.gt = (const float4*)gt_boxes; a.gt_off = gt_offsets; a.B = batch;
  a.wmax = (float)(image_w - 1); a.hmax = (float)(image_h - 1); a.pos = pos_iou_threshold; a.neg = neg_iou_threshold;
  a.S = total_num_samples; a.max_pos = max_pos_samples;
  for (int k = 0; k < 4; ++k) { a.means.v[k] = means[k]; a.stds.v[k] = stds[k]; }
  a.seed.lo = (uint32_t)seed; a.seed.hi = (uint32_t)(seed >> 32); a.first_image = first_image_id;
  TG_SEED_DIAG(a);
  a.colmax = ar.take<uint32_t>(B * TG_MAX_GT);
  a.cnt = ar.take<int32_t>(B * 8);
  const size_t head = ar.off;
  a.thr = ar.take<TgThr>(B * 2);
  a.cls = ar.take<int8_t>(B * n);
  a.khi = ar.take<uint32_t>(B * n);
  int32_t* ws_amax = ar.take<int32_t>(B * n);
  a.amax = argmax ? argmax : ws_amax;
  a.list = ar.take<int32_t>(B * 2 * total_num_samples);
  a.labels = labels; a.targets = (float4*)targets; a.inside = (float4*)inside; a.outside = (float4*)outside;
  a.sample_idx = sample_idx; a.sample_targets = (float4*)sample_targets; a.counts = counts;
  a.labels_before = labels_before_sampling;
  { const int zrc = tg_zero_head(workspace, head, st); if (zrc != ODET_OK) return zrc; }
  const dim3 grid((num_anchors + TG_BLOCK - 1) / TG_BLOCK, batch);
  if (num_anchors > 0) {
    hipLaunchKernelGGL(k_at_colmax, grid, dim3(TG_BLOCK), 0, st, a);
    ODET_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_at_label, grid, dim3(TG_BLOCK), 0, st, a);
    ODET_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_at_select, dim3(2, batch), dim3(TG_SEL_THREADS), 0, st, a);
  ODET_LAUNCH_CHECK();
  if (num_anchors > 0) {
    hipLaunchKernelGGL(k_at_write, grid, dim3(TG_BLOCK), 0, st, a);
    ODET_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_at_compact, dim3(batch), dim3(TG_SEL_THREADS), 0, st, a);
  ODET_LAUNCH_CHECK();
  return ODET_OK;
}

// ----------------------------------------------------------------------------------------------- proposal targets --
struct PtArgs {
  const float4* rois; const int32_t* roi_counts; int R;
  const float4* gt; const int32_t* gt_labels; const int32_t* gt_off; int B;
  int num_classes; float pos, neg;
  int S, max_pos;
  Vec4 means, stds;
  int row_labels;
  TgSeed seed; uint32_t first_image;
  int32_t* cnt;         // [B, 8]: fg, bg candidates (zero-filled per call)
  int8_t* cls;          // [B, R]
  uint32_t* khi;        // [B, R]
  float4* final_rois; int32_t* final_labels; float* targets; float* inside; float* outside;
  int32_t* keep; int32_t* gt_assignment; int32_t* counts;
};

// proposal_target.py:55-63: row maximum, first arg-maximum, foreground / background candidates, their key words
__global__ void __launch_bounds__(TG_BLOCK) k_pt_assign(PtArgs a) {
  __shared__ float4 s_gt[TG_MAX_GT];
  __shared__ int s_cnt[2];
  const int b = blockIdx.y;
  const int g0 = a.gt_off[b];
  int G = a.gt_off[b + 1] - g0;
  const bool bad = G > TG_MAX_GT || G < 0;
  if (bad) G = 0;
  for (int g = threadIdx.x; g < G; g += TG_BLOCK) s_gt[g] = a.gt[g0 + g];
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const int r = blockIdx.x * TG_BLOCK + threadIdx.x;
  const int cntr = a.roi_counts ? min(max(a.roi_counts[b], 0), a.R) : a.R;
  int c = TG_OUTSIDE, am = -1;
  if (r < cntr && !bad) {
    const float4 p = a.rois[(size_t)b * a.R + r];
    float mx = 0.0f;
    if (G > 0) {
      mx = -1.0f;
      for (int g = 0; g < G; ++g) {
        const float v = d_pair_iou(p, s_gt[g]);
        if (v > mx) { mx = v; am = g; }
      }
    }
    c = TG_IGNORE;
    if (mx >= a.pos) c = TG_FG;                               // :61
    else if (mx >= a.neg) c = TG_BG;                          // :62-63 (below the POSITIVE threshold)
  }
  if (r < a.R) {
    const size_t o = (size_t)b * a.R + r;
    a.cls[o] = (int8_t)c;
    a.gt_assignment[o] = am;
    if (c >= 0) a.khi[o] = d_key_hi(c == TG_FG ? TG_STREAM_ROI_FG : TG_STREAM_ROI_BG, a.first_image + b, (uint32_t)r, a.seed);
  }
  const int lane = threadIdx.x & 63;
  const unsigned long long m_fg = __ballot(c == TG_FG), m_bg = __ballot(c == TG_BG);
  if (lane == 0) {
    if (m_fg) atomicAdd(&s_cnt[0], __popcll(m_fg));
    if (m_bg) atomicAdd(&s_cnt[1], __popcll(m_bg));
  }
  __syncthreads();
  if (threadIdx.x < 2 && s_cnt[threadIdx.x]) atomicAdd(&a.cnt[b * 8 + threadIdx.x], s_cnt[threadIdx.x]);
}

__device__ __forceinline__ int d_pt_label(const PtArgs& a, int b, int row) {
  const int am = a.gt_assignment[(size_t)b * a.R + row];
  return am >= 0 ? a.gt_labels[a.gt_off[b] + am] : 0;        // :58
}

// one workgroup per image: both selections, the row order of the contract, every output of fixed shape (:66-124)
__global__ void __launch_bounds__(TG_SEL_THREADS) k_pt_sample(PtArgs a) {
  __shared__ int hist[TG_BINS];
  __shared__ int sh[24];
  __shared__ unsigned long long s_key[TG_MAX_SAMPLES];
  __shared__ int s_idx[TG_MAX_SAMPLES];
  __shared__ int s_keep[TG_MAX_SAMPLES];
  __shared__ int s_slot[2];
  const int b = blockIdx.x, t = threadIdx.x;
  const uint32_t image = a.first_image + b;
  const int8_t* cls = a.cls + (size_t)b * a.R;
  const uint32_t* khi = a.khi + (size_t)b * a.R;
  const int n_fg = a.cnt[b * 8 + 0], n_bg = a.cnt[b * 8 + 1];
  const int k_fg = min(n_fg, a.max_pos);                     // :66-67
  const int want = a.S - k_fg;
  const bool replace = n_bg < want;                          // :73-76
  const int k_bg = replace ? n_bg : want;                    // background candidates listed (all of them when drawing with replacement)
  const int rows = k_fg + ((replace && n_bg == 0) ? 0 : want);
  const TgThr tf = d_tg_radix_select(cls, khi, a.R, TG_FG, k_fg, n_fg, TG_STREAM_ROI_FG, image, a.seed, hist, sh);
  const TgThr tb = d_tg_radix_select(cls, khi, a.R, TG_BG, k_bg, n_bg, TG_STREAM_ROI_BG, image, a.seed, hist, sh);
  if (t < 2) s_slot[t] = 0;
  __syncthreads();
  // kept rows in arrival order: foreground in [0, k_fg), background in [k_fg, k_fg + k_bg); the sort key is the candidate's
  // key64 where its kind was sampled and 0 where it was not (then the row index alone orders)
  const bool fg_sampled = n_fg > a.max_pos, bg_sampled = n_bg > want;
  for (int r = t; r < a.R; r += TG_SEL_THREADS) {
    const int c = cls[r];
    if (c < 0) continue;
    const int kind = c == TG_FG ? 0 : 1;
    const uint32_t stream = kind == 0 ? TG_STREAM_ROI_FG : TG_STREAM_ROI_BG;
    if (!d_tg_selected(kind == 0 ? tf : tb, khi[r], (uint32_t)r, stream, image, a.seed)) continue;
    const int slot = (kind == 0 ? 0 : k_fg) + atomicAdd(&s_slot[kind], 1);
    if (slot < TG_MAX_SAMPLES) {
      s_idx[slot] = r;
      s_key[slot] = (kind == 0 ? fg_sampled : bg_sampled) ? d_key64(stream, image, (uint32_t)r, a.seed) : 0ull;
    }
  }
  __syncthreads();
  int row = -1, pos = -1;
  if (t < k_fg) { row = s_idx[t]; pos = d_tg_rank(s_key, s_idx, k_fg, s_key[t], row); }
  else if (t < k_fg + k_bg) { row = s_idx[t]; pos = k_fg + d_tg_rank(s_key + k_fg, s_idx + k_fg, k_bg, s_key[t], row); }
  __syncthreads();
  if (pos >= 0) s_keep[pos] = row;
  __syncthreads();
  if (replace && n_bg > 0) {                                 // s_keep[k_fg ..) is bg_ascending; the draws go behind a copy of it
    if (t < k_bg) s_idx[t] = s_keep[k_fg + t];
    __syncthreads();
    if (t < want) {
      uint32_t w0, w1;
      odet_philox2((uint32_t)t, image, TG_STREAM_ROI_REPLACE, 0u, a.seed.lo, a.seed.hi, &w0, &w1);
      s_keep[k_fg + t] = s_idx[(int)(((unsigned long long)w0 * (unsigned long long)n_bg) >> 32)];
    }
    __syncthreads();
  }
  // outputs
  const int W = 4 * a.num_classes;
  float* tg = a.targets + (size_t)b * a.S * W;
  float* in = a.inside + (size_t)b * a.S * W;
  float* ou = a.outside + (size_t)b * a.S * W;
  for (int e = t; e < a.S * W; e += TG_SEL_THREADS) { tg[e] = 0.0f; in[e] = 0.0f; ou[e] = (e / W) < rows ? 1.0f : 0.0f; }
  __syncthreads();
  if (t < a.S) {
    const size_t o = (size_t)b * a.S + t;
    const int src = t < rows ? s_keep[t] : -1;
    if ((unsigned)src < (unsigned)a.R) {
      const float4 box = a.rois[(size_t)b * a.R + src];
      a.keep[o] = src;
      a.final_rois[o] = box;
      a.final_labels[o] = t < k_fg ? d_pt_label(a, b, src) : 0;                                  // :84-85
      if (t < k_fg) {
        const int col = a.row_labels ? d_pt_label(a, b, t) : d_pt_label(a, b, src);              // :96 / :113 labels[row]: sic
        const int am = a.gt_assignment[(size_t)b * a.R + src];
        if (am >= 0 && col >= 0 && col < a.num_classes) {
          const float4 e = d_encode_box(box, a.gt[a.gt_off[b] + am], a.means.v, a.stds.v);      // :103-113
          float* q = tg + (size_t)t * W + 4 * col;
          q[0] = e.x; q[1] = e.y; q[2] = e.z; q[3] = e.w;
          float* w = in + (size_t)t * W + 4 * col;
          w[0] = 1.0f; w[1] = 1.0f; w[2] = 1.0f; w[3] = 1.0f;
        }
      }
    } else {
      a.keep[o] = -1;
      a.final_rois[o] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      a.final_labels[o] = 0;
    }
  }
  if (t == 0) {
    const int G = a.gt_off[b + 1] - a.gt_off[b];
    const bool bad = G > TG_MAX_GT || G < 0;
    int32_t* c = a.counts + b * 4;
    c[0] = bad ? -1 : n_fg; c[1] = bad ? -1 : n_bg; c[2] = bad ? -1 : k_fg; c[3] = bad ? -1 : rows;
  }
}

extern "C" size_t odet_proposal_target_workspace_bytes(int max_rois, int batch) {
  const size_t R = max_rois < 0 ? 0 : (size_t)max_rois, B = batch < 1 ? 1 : (size_t)batch;
  return odet_align_up(B * 8 * 4, 256) + odet_align_up(B * R, 256) + odet_align_up(B * R * 4, 256) + 512;
}

extern "C" int odet_proposal_target(const float* rois, const int32_t* roi_counts, int max_rois, const float* gt_boxes,
                                    const int32_t* gt_labels, const int32_t* gt_offsets, int batch, int num_classes,
                                    float pos_iou_threshold, float neg_iou_threshold, int total_num_samples,
                                    int max_pos_samples, const float* means, const float* stds, int reference_row_labels,
                                    uint64_t seed, uint32_t first_image_id, float* final_rois, int32_t* final_labels,
                                    float* targets, float* inside, float* outside, int32_t* keep, int32_t* gt_assignment,
                                    int32_t* counts, void* workspace, size_t workspace_bytes, odet_stream_t stream) {
  ODET_REQUIRE(batch >= 0 && max_rois >= 0, "odet_proposal_target: negative size");
  if (batch == 0) return ODET_OK;
  ODET_REQUIRE(rois && gt_boxes && gt_labels && gt_offsets && means && stds && final_rois && final_labels && targets &&
               inside && outside && keep && gt_assignment && counts, "odet_proposal_target: null pointer");
  ODET_REQUIRE(num_classes > 0, "odet_proposal_target: num_classes must be positive");
  if (batch > 64) return odet_set_error(ODET_E_LIMIT, "odet_proposal_target: batch %d exceeds 64", batch);
  if (max_rois > 65536) return odet_set_error(ODET_E_LIMIT, "odet_proposal_target: %d RoIs exceed 65536", max_rois);
  if (total_num_samples < 1 || total_num_samples > TG_MAX_SAMPLES)
    return odet_set_error(ODET_E_LIMIT, "odet_proposal_target: total_num_samples %d outside 1..%d", total_num_samples, TG_MAX_SAMPLES);
  ODET_REQUIRE(max_pos_samples >= 0 && max_pos_samples <= total_num_samples,
               "odet_proposal_target: max_pos_samples must lie in 0..total_num_samples");
  const size_t need = odet_proposal_target_workspace_bytes(max_rois, batch);
  if (!workspace || workspace_bytes < need)
    return odet_set_error(ODET_E_WORKSPACE, "odet_proposal_target: workspace too small (%zu < %zu)", workspace_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  const size_t B = (size_t)batch, R = (size_t)max_rois;
  OdetArena ar{(char*)workspace, workspace_bytes, 0};
  PtArgs a;
  a.rois = (const float4*)rois; a.roi_counts = roi_counts; a.R = max_rois; a.gt = (const float4*)gt_boxes;
  a.gt_labels = gt_labels; a.gt_off = gt_offsets; a.B = batch; a.num_classes = num_classes;
  a.pos = pos_iou_threshold; a.neg = neg_iou_threshold; a.S = total_num_samples; a.max_pos = max_pos_samples;
  for (int k = 0; k < 4; ++k) { a.means.v[k] = means[k]; a.stds.v[k] = stds[k]; }
  a.row_labels = reference_row_labels ? 1 : 0;
  a.seed.lo = (uint32_t)seed; a.seed.hi = (uint32_t)(seed >> 32); a.first_image = first_image_id;
  TG_SEED_DIAG(a);
  a.cnt = ar.take<int32_t>(B * 8);
  const size_t head = ar.off;
  a.cls = ar.take<int8_t>(B * R);
  a.khi = ar.take<uint32_t>(B * R);
  a.final_rois = (float4*)final_rois; a.final_labels = final_labels; a.targets = targets; a.inside = inside;
  a.outside = outside; a.keep = keep; a.gt_assignment = gt_assignment; a.counts = counts;
  { const int zrc = tg_zero_head(workspace, head, st); if (zrc != ODET_OK) return zrc; }
  if (max_rois > 0) {
    hipLaunchKernelGGL(k_pt_assign, dim3((max_rois + TG_BLOCK - 1) / TG_BLOCK, batch), dim3(TG_BLOCK), 0, st, a);
    ODET_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_pt_sample, dim3(batch), dim3(TG_SEL_THREADS), 0, st, a);
  ODET_LAUNCH_CHECK();
  return ODET_OK;
}
