// PASCAL VOC evaluation: evaluation/detectron_pascal_evaluation_utils.py voc_eval (:86-222) and voc_ap (:54-83) as
// scripts/eval_pascal.py:74-96 runs them per class, and the paired bootstrap of evaluation/precision_gate.py
// (_map_weighted) that re-weights the same matches per resample.  Everything is float64 with the reference's operation
// order (-ffp-contract=off); the host (evaluation/voc_eval_gpu.py) packs ground truth and detections into segments =
// (class, image) pairs.
//
//   k_voc_match (grid = segments, one wave): the walk of :173-211 for one image's detections of one class.  The
//     detections are ranked (stable, score desc: the order in which the global walk meets them), the ground truth sits in
//     LDS; per detection the lanes share the ground-truth boxes, each keeps its first maximum, a wave reduction picks the
//     first maximum of all (np.max / np.argmax), lane 0 keeps the `det` marks.
//   order: odet_coco_order (class asc, score desc, entry index asc) is np.argsort(-confidence, kind='stable') of every
//     class, because entries are class-major, image-ascending and sorted inside their segment.
//   k_voc_accumulate (grid = classes): :213-220 and voc_ap.  Chunks of VA_THREADS x VA_ITEMS sorted entries, a block
//     prefix sum with a carry between chunks gives tp / fp; the 11-point maxima are kept per thread and merged in LDS;
//     the area metric walks the chunks backwards with a block suffix maximum (the envelope) and a carry, writes its
//     terms to a workspace and adds them up in the order numpy's np.sum adds them (voc_np_sum), so that it too equals
//     the host value.
//   k_voc_bootstrap (grid = resamples x classes): the same curve with every entry weighted by how often its image was
//     drawn; nothing is stored but the AP.
#include <cfloat>
#include <climits>

#include "odet_internal.h"

#define VM_THREADS 64
#define VA_THREADS 256
#define VA_WAVES (VA_THREADS / 64)
#define VA_ITEMS 8
#define VA_CHUNK (VA_THREADS * VA_ITEMS)
#define VOC_LDS_MAX (150 * 1024)

typedef unsigned long long u64;
typedef long long i64;

struct VocMatchParams {
  const int32_t* gt_off; const int32_t* dt_off;
  const double* gt_box; const uint8_t* gt_hard; const double* dt_box; const double* dt_score;
  double thr;
  int maxd, maxg, num_entries, num_gt;
  double* o_score; uint8_t* o_flag; int32_t* o_npos;
};

static size_t voc_match_lds(int maxd, int maxg) {
  return (size_t)maxd * 8 + (size_t)maxg * 4 * 8 + (size_t)maxd * 4 + 2 * (size_t)maxg + 16;
}

__global__ void __launch_bounds__(VM_THREADS) k_voc_match(VocMatchParams p) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int s = blockIdx.x, lane = threadIdx.x;
  const int g0 = p.gt_off[s], G = p.gt_off[s + 1] - g0;
  const int d0 = p.dt_off[s], D = p.dt_off[s + 1] - d0;
  // the LDS was sized for maxd / maxg and the arrays for num_gt / num_entries: a segment outside them (a caller that
  // passed wrong maxima or offsets) is skipped, never overrun
  if (G < 0 || D < 0 || G > p.maxg || D > p.maxd || g0 < 0 || d0 < 0 || (i64)g0 + G > p.num_gt ||
      (i64)d0 + D > p.num_entries)
    return;
  // layout: dkey [maxd] (u64) | gbox [maxg][4] (double) | sidx [maxd] (int) | ghard [maxg] | gdet [maxg]
  u64* dkey = reinterpret_cast<u64*>(smem);
  double* gbox = reinterpret_cast<double*>(dkey + p.maxd);
  int* sidx = reinterpret_cast<int*>(gbox + (size_t)p.maxg * 4);
  uint8_t* ghard = reinterpret_cast<uint8_t*>(sidx + p.maxd);
  uint8_t* gdet = ghard + p.maxg;

  int np = 0;
  for (int j = lane; j < G; j += VM_THREADS) {
    const double* b = p.gt_box + (size_t)(g0 + j) * 4;
    gbox[j * 4 + 0] = b[0]; gbox[j * 4 + 1] = b[1]; gbox[j * 4 + 2] = b[2]; gbox[j * 4 + 3] = b[3];
    const uint8_t h = p.gt_hard[g0 + j] ? 1 : 0;
    ghard[j] = h;
    gdet[j] = 0;                                                   // :141 det = [False] * len(R)
    np += h ? 0 : 1;                                               // :145 npos = npos + sum(~difficult)
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) np += __shfl_xor(np, d);
  if (lane == 0) p.o_npos[s] = np;
  for (int i = lane; i < D; i += VM_THREADS) dkey[i] = coco_desc_key(p.dt_score[d0 + i]);
  __syncthreads();
  // :169 np.argsort(-confidence) restricted to this image (stable): the rank of every detection by (key, index)
  for (int i = lane; i < D; i += VM_THREADS) {
    const u64 ki = dkey[i];
    int r = 0;
    for (int j = 0; j < D; ++j) {
      const u64 kj = dkey[j];
      r += (kj < ki || (kj == ki && j < i)) ? 1 : 0;
    }
    sidx[r] = i;
  }
  __syncthreads();
  for (int r = lane; r < D; r += VM_THREADS) p.o_score[d0 + r] = p.dt_score[d0 + sidx[r]];

  for (int r = 0; r < D; ++r) {                                    // :177 for d in range(nd)
    const double* bb = p.dt_box + (size_t)(d0 + sidx[r]) * 4;
    const double bx1 = bb[0], by1 = bb[1], bx2 = bb[2], by2 = bb[3];
    const double barea = ((bx2 - bx1) + 1.) * ((by2 - by1) + 1.);
    double best = -INFINITY;                                       // :180 ovmax = -np.inf
    int bj = INT_MAX;
    bool nan = false;
    for (int j = lane; j < G; j += VM_THREADS) {
      const double gx1 = gbox[j * 4 + 0], gy1 = gbox[j * 4 + 1], gx2 = gbox[j * 4 + 2], gy2 = gbox[j * 4 + 3];
      const double iw = fmax((fmin(gx2, bx2) - fmax(gx1, bx1)) + 1., 0.);            // :186-190
      const double ih = fmax((fmin(gy2, by2) - fmax(gy1, by1)) + 1., 0.);            // :187-191
      const double inters = iw * ih;                                                 // :192
      const double uni = (barea + ((gx2 - gx1) + 1.) * ((gy2 - gy1) + 1.)) - inters; // :195-197
      const double ov = inters / uni;                                                // :199
      if (ov != ov) nan = true;                                    // np.max propagates a NaN: ovmax > ovthresh is False
      else if (ov > best) { best = ov; bj = j; }                   // first maximum of this lane (j ascending)
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {                             // :200-201 np.max / np.argmax: first maximum of all
      const double ob = __shfl_xor(best, d);
      const int oj = __shfl_xor(bj, d);
      if (ob > best || (ob == best && oj < bj)) { best = ob; bj = oj; }
    }
    nan = __any(nan) != 0;
    uint8_t flag = ODET_VOC_FP;                                    // :210-211
    if (G > 0 && !nan && best > p.thr && bj < G) {                 // :203 (strict)
      if (ghard[bj]) flag = ODET_VOC_IGNORED;                      // :204 neither tp nor fp
      else if (!gdet[bj]) flag = ODET_VOC_TP;                      // :205-207
    }                                                              // :208-209 fp
    if (lane == 0) {
      if (flag == ODET_VOC_TP) gdet[bj] = 1;
      p.o_flag[d0 + r] = flag;
    }
    __syncthreads();
  }
}

extern "C" int odet_voc_match(int num_segments, const int32_t* seg_gt_off, const int32_t* seg_dt_off,
                              const double* gt_box, const uint8_t* gt_difficult, const double* dt_box,
                              const double* dt_score, double ovthresh, int max_seg_dets, int max_seg_gt, int num_gt,
                              int num_entries, double* out_score, uint8_t* out_flag, int32_t* out_npos,
                              odet_stream_t stream) {
  ODET_REQUIRE(num_segments >= 0 && max_seg_dets >= 0 && max_seg_gt >= 0 && num_entries >= 0 && num_gt >= 0,
               "odet_voc_match: negative size");
  if (max_seg_dets > ODET_VOC_MAX_SEG_DETS)
    return odet_set_error(ODET_E_LIMIT, "odet_voc_match: %d detections in one segment exceed %d", max_seg_dets,
                          ODET_VOC_MAX_SEG_DETS);
  if (max_seg_gt > ODET_VOC_MAX_SEG_GT)
    return odet_set_error(ODET_E_LIMIT, "odet_voc_match: %d ground-truth boxes in one segment exceed %d", max_seg_gt,
                          ODET_VOC_MAX_SEG_GT);
  if (num_entries > ODET_VOC_MAX_ENTRIES)
    return odet_set_error(ODET_E_LIMIT, "odet_voc_match: %d detections exceed %d", num_entries, ODET_VOC_MAX_ENTRIES);
  if (num_segments == 0) return ODET_OK;
  ODET_REQUIRE(seg_gt_off && seg_dt_off && out_npos, "odet_voc_match: null pointer");
  ODET_REQUIRE((max_seg_gt == 0 || (gt_box && gt_difficult)) &&
               (max_seg_dets == 0 || (dt_box && dt_score && out_score && out_flag)), "odet_voc_match: null pointer");
  VocMatchParams p;
  p.gt_off = seg_gt_off; p.dt_off = seg_dt_off; p.gt_box = gt_box; p.gt_hard = gt_difficult; p.dt_box = dt_box;
  p.dt_score = dt_score; p.thr = ovthresh; p.maxg = max_seg_gt; p.num_entries = num_entries;
  p.maxd = (max_seg_dets + 1) & ~1;                               // (even: gbox starts on 16 bytes behind dkey)
  p.num_gt = num_gt; p.o_score = out_score; p.o_flag = out_flag; p.o_npos = out_npos;
  const size_t lds = voc_match_lds(p.maxd, p.maxg);               // (at the limits: 83 KB)
  if (lds > VOC_LDS_MAX) return odet_set_error(ODET_E_LIMIT, "odet_voc_match: %zu B of LDS", lds);
  static OdetPerDeviceOnce once;
  ODET_HIP(once.run([] { return hipFuncSetAttribute((const void*)k_voc_match, hipFuncAttributeMaxDynamicSharedMemorySize, VOC_LDS_MAX); }));
  hipLaunchKernelGGL(k_voc_match, dim3(num_segments), dim3(VM_THREADS), lds, (hipStream_t)stream, p);
  ODET_LAUNCH_CHECK();
  return ODET_OK;
}

// ---------------------------------------------------------------------------------- the curve --
// the area metric's terms: (entries + 1) doubles per class and resample; the 11-point metric needs none
extern "C" size_t odet_voc_eval_workspace_bytes(int num_entries, int num_classes, int num_resamples, int metric) {
  if (metric != ODET_VOC_AP_AREA || num_resamples <= 0) return 0;
  const size_t per = (size_t)(num_entries > 0 ? num_entries : 0) + (size_t)(num_classes > 0 ? num_classes : 0);
  return odet_align_up(per * (size_t)num_resamples * sizeof(double), 256);
}

__device__ __forceinline__ i64 wave_incl_scan_i64(i64 v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const i64 t = __shfl_up(v, d);
    if (lane >= d) v += t;
  }
  return v;
}

// exclusive prefix sums of two values over the VA_THREADS threads; lds [2][VA_WAVES]
__device__ __forceinline__ void block_excl_scan2(i64 a, i64 b, i64* lds, i64* xa, i64* xb, i64* ta, i64* tb) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const i64 ia = wave_incl_scan_i64(a), ib = wave_incl_scan_i64(b);
  __syncthreads();
  if (lane == 63) { lds[w] = ia; lds[VA_WAVES + w] = ib; }
  __syncthreads();
  i64 pa = 0, pb = 0, sa = 0, sb = 0;
#pragma unroll
  for (int k = 0; k < VA_WAVES; ++k) {
    if (k < w) { pa += lds[k]; pb += lds[VA_WAVES + k]; }
    sa += lds[k]; sb += lds[VA_WAVES + k];
  }
  *xa = pa + ia - a; *xb = pb + ib - b; *ta = sa; *tb = sb;
}

// exclusive SUFFIX maximum (over the threads after this one; 0 for the last: the values are >= 0) and the maximum of all
__device__ __forceinline__ double block_excl_suffix_max(double v, double* lds /*[VA_WAVES]*/, double* all) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double t = __shfl_down(inc, d);
    if (lane + d < 64) inc = fmax(inc, t);
  }
  double exc = __shfl_down(inc, 1);
  if (lane == 63) exc = 0.0;
  __syncthreads();
  if (lane == 0) lds[w] = inc;
  __syncthreads();
  double tot = 0.0;
#pragma unroll
  for (int k = 0; k < VA_WAVES; ++k) {
    if (k > w) exc = fmax(exc, lds[k]);
    tot = fmax(tot, lds[k]);
  }
  *all = tot;
  return exc;
}

struct VocCurveLds {
  i64 scan[2 * VA_WAVES];
  double smax[VA_WAVES];
  double red[VA_THREADS];
  u64 pmax[ODET_VOC_R];
  double thr[ODET_VOC_R];
};

// weighted tp / fp contribution of the sorted entry `pos`
__device__ __forceinline__ void voc_entry_weights(const uint8_t* __restrict__ sflag, const int32_t* __restrict__ simg,
                                                  const int32_t* __restrict__ counts, int num_images, bool ign_is_fp,
                                                  int pos, i64* wt, i64* wf) {
  const uint8_t f = sflag[pos];
  i64 w = 1;
  if (counts) {
    const int im = simg[pos];
    w = (im >= 0 && im < num_images) ? (i64)counts[im] : 0;
  }
  if (f == ODET_VOC_TP) *wt = w;
  else if (f == ODET_VOC_FP || ign_is_fp) *wf = w;
}

// numpy's pairwise_sum (numpy/_core/src/umath/loops_utils.h.src) of a[0..n) with a[i] = last[-i] (the terms are stored
// in reverse): below 8 elements a plain loop from 0., up to 128 eight running sums combined as ((r0+r1)+(r2+r3)) +
// ((r4+r5)+(r6+r7)) and the remainder added one by one, above that the two halves (the left one n/2 rounded down to a
// multiple of 8).  n <= VOC_NP_BUF, so the explicit stack of the recursion stays below 8 frames.
#define VOC_NP_BUF 8192
__device__ double voc_np_pairwise(const double* last, int n0) {
  int f_off[10], f_n[10], f_stage[10];
  double f_left[10];
  int sp = 1;
  f_off[0] = 0; f_n[0] = n0; f_stage[0] = 0; f_left[0] = 0.0;
  double ret = 0.0;
  while (sp > 0) {
    const int t = sp - 1;
    const int off = f_off[t], n = f_n[t];
    if (n <= 128) {
      const double* a = last - off;                                // a[i] = a[-i] below
      double res;
      if (n < 8) {
        res = 0.;
        for (int i = 0; i < n; ++i) res += a[-i];
      } else {
        double r0 = a[0], r1 = a[-1], r2 = a[-2], r3 = a[-3], r4 = a[-4], r5 = a[-5], r6 = a[-6], r7 = a[-7];
        int i;
        for (i = 8; i < n - (n % 8); i += 8) {
          r0 += a[-(i + 0)]; r1 += a[-(i + 1)]; r2 += a[-(i + 2)]; r3 += a[-(i + 3)];
          r4 += a[-(i + 4)]; r5 += a[-(i + 5)]; r6 += a[-(i + 6)]; r7 += a[-(i + 7)];
        }
        res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
        for (; i < n; ++i) res += a[-i];
      }
      ret = res;
      --sp;
      continue;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    if (f_stage[t] == 0) {
      f_stage[t] = 1;
      f_off[sp] = off; f_n[sp] = n2; f_stage[sp] = 0; ++sp;
    } else if (f_stage[t] == 1) {
      f_left[t] = ret;
      f_stage[t] = 2;
      f_off[sp] = off + n2; f_n[sp] = n - n2; f_stage[sp] = 0; ++sp;
    } else {
      ret = f_left[t] + ret;
      --sp;
    }
  }
  return ret;
}

// np.sum of the T terms stored in reverse (term i at terms[T-1-i]): add.reduce walks the array in pieces of the ufunc
// buffer (8192 elements), each summed pairwise, the pieces added up in order.  One thread per piece, thread 0 folds.
// The result is valid in thread 0.
__device__ double voc_np_sum(const double* terms, i64 T, double* red /*[VA_THREADS]*/) {
  const int tid = threadIdx.x;
  const i64 npieces = (T + VOC_NP_BUF - 1) / VOC_NP_BUF;
  double acc = 0.0;
  for (i64 c0 = 0; c0 < npieces; c0 += VA_THREADS) {
    const i64 c = c0 + tid;
    double v = 0.0;
    if (c < npieces) {
      const i64 off = c * VOC_NP_BUF;
      const i64 len = T - off < VOC_NP_BUF ? T - off : VOC_NP_BUF;
      v = voc_np_pairwise(terms + (T - 1 - off), (int)len);
    }
    red[tid] = v;
    __syncthreads();
    if (tid == 0) {
      const i64 m = npieces - c0 < VA_THREADS ? npieces - c0 : VA_THREADS;
      for (int j = 0; j < (int)m; ++j) acc = acc + red[j];
    }
    __syncthreads();
  }
  return acc;
}

// The curve of one class over its sorted entries [e0, e1): tp / fp flags from sflag, every entry weighted by
// counts[simg[pos]] (counts == nullptr: weight 1).  ign_is_fp: precision_gate._map_weighted's rule (~tp is a false
// positive); otherwise an ignored entry adds to neither sum (:204-209).  o_rec / o_prec (nullable): the curves.
// want07 / want_area: which AP to compute; terms: scratch of (e1 - e0) + 1 doubles for the area metric.  All threads of the block call it; the results are valid in thread 0.
__device__ void voc_curve(int e0, int e1, const uint8_t* __restrict__ sflag, const int32_t* __restrict__ simg,
                          const int32_t* __restrict__ counts, int num_images, bool ign_is_fp, i64 npos_i,
                          VocCurveLds* L, double* __restrict__ o_rec, double* __restrict__ o_prec, bool want07,
                          bool want_area, double* __restrict__ terms, double* ap07, double* ap_area) {
  const int tid = threadIdx.x;
  const double npos = (double)npos_i;
  const double eps = DBL_EPSILON;                                  // np.finfo(np.float64).eps
  for (int j = tid; j < ODET_VOC_R; j += VA_THREADS) L->pmax[j] = 0ull;
  __syncthreads();
  double pm[ODET_VOC_R];
#pragma unroll
  for (int j = 0; j < ODET_VOC_R; ++j) pm[j] = 0.0;
  i64 carry_tp = 0, carry_fp = 0;
  for (int base = e0; base < e1; base += VA_CHUNK) {
    const int lo = base + tid * VA_ITEMS;
    i64 wt[VA_ITEMS], wf[VA_ITEMS];
    i64 stp = 0, sfp = 0;
#pragma unroll
    for (int q = 0; q < VA_ITEMS; ++q) {
      wt[q] = 0; wf[q] = 0;
      const int pos = lo + q;
      if (pos < e1) voc_entry_weights(sflag, simg, counts, num_images, ign_is_fp, pos, &wt[q], &wf[q]);
      stp += wt[q]; sfp += wf[q];
    }
    i64 xtp, xfp, ttp, tfp;
    block_excl_scan2(stp, sfp, L->scan, &xtp, &xfp, &ttp, &tfp);
    i64 tp = carry_tp + xtp, fp = carry_fp + xfp;
#pragma unroll
    for (int q = 0; q < VA_ITEMS; ++q) {
      const int pos = lo + q;
      if (pos >= e1) break;
      tp += wt[q]; fp += wf[q];                                                       // :214-215 np.cumsum
      const double dtp = (double)tp;
      const double rc = npos_i > 0 ? dtp / npos : dtp * 0.0;                          // :216
      const double pr = dtp / fmax(dtp + (double)fp, eps);                            // :219
      if (o_rec) { o_rec[pos] = rc; o_prec[pos] = pr; }
      if (want07) {
#pragma unroll
        for (int j = 0; j < ODET_VOC_R; ++j)
          if (rc >= L->thr[j]) pm[j] = fmax(pm[j], pr);                               // :62-65 np.max(prec[rec >= t])
      }
    }
    carry_tp += ttp; carry_fp += tfp;
  }
  if (want07) {
#pragma unroll
    for (int j = 0; j < ODET_VOC_R; ++j)
      if (pm[j] > 0.0) atomicMax(&L->pmax[j], (u64)__double_as_longlong(pm[j]));     // (non-negative doubles: bit order)
    __syncthreads();
    if (tid == 0) {
      double ap = 0.;                                                                 // :60
      for (int j = 0; j < ODET_VOC_R; ++j) ap = ap + __longlong_as_double((i64)L->pmax[j]) / 11.;   // :66
      *ap07 = ap;
    }
  }
  if (!want_area) return;
  // :68-82: mrec = [0, rec, 1], mpre = [0, prec, 0], mpre = its suffix maximum, np.sum((mrec[i+1] - mrec[i]) * mpre[i+1])
  // over the i where mrec changes.  Walked backwards, chunk by chunk (the cumulative sums of a chunk's start are the
  // totals minus what lies behind it); the terms go to `terms` from its start in REVERSE order, so that no count is
  // needed before the walk, and voc_np_sum adds them up in numpy's order.
  const int n = e1 - e0;
  const double rec_last = npos_i > 0 ? (double)carry_tp / npos : (double)carry_tp * 0.0;
  i64 carry_cnt = 0;
  if (n == 0 || rec_last != 1.0) {                                 // the step to mrec[-1] = 1 is a term: times mpre[-1] = 0
    if (tid == 0) terms[0] = (1.0 - rec_last) * 0.0;
    carry_cnt = 1;
  }
  double carry_max = 0.0;
  i64 end_tp = carry_tp, end_fp = carry_fp;
  const int nchunks = (n + VA_CHUNK - 1) / VA_CHUNK;
  for (int c = nchunks - 1; c >= 0; --c) {
    const int lo = e0 + c * VA_CHUNK + tid * VA_ITEMS;
    i64 wt[VA_ITEMS], wf[VA_ITEMS];
    i64 stp = 0, sfp = 0;
#pragma unroll
    for (int q = 0; q < VA_ITEMS; ++q) {
      wt[q] = 0; wf[q] = 0;
      const int pos = lo + q;
      if (pos < e1) voc_entry_weights(sflag, simg, counts, num_images, ign_is_fp, pos, &wt[q], &wf[q]);
      stp += wt[q]; sfp += wf[q];
    }
    i64 xtp, xfp, ttp, tfp;
    block_excl_scan2(stp, sfp, L->scan, &xtp, &xfp, &ttp, &tfp);
    i64 tp = (end_tp - ttp) + xtp, fp = (end_fp - tfp) + xfp;
    double rc[VA_ITEMS + 1], pr[VA_ITEMS];
    rc[0] = npos_i > 0 ? (double)tp / npos : (double)tp * 0.0;     // rec of the entry before (0 = mrec[0] at the start)
    double lmax = 0.0;
    unsigned change = 0;
    i64 nchange = 0;
#pragma unroll
    for (int q = 0; q < VA_ITEMS; ++q) {
      tp += wt[q]; fp += wf[q];
      const double dtp = (double)tp;
      rc[q + 1] = npos_i > 0 ? dtp / npos : dtp * 0.0;
      pr[q] = (lo + q < e1) ? dtp / fmax(dtp + (double)fp, eps) : 0.0;
      lmax = fmax(lmax, pr[q]);
      if (lo + q < e1 && rc[q + 1] != rc[q]) { change |= 1u << q; ++nchange; }       // :77 mrec[1:] != mrec[:-1]
    }
    i64 xc, xz, tc, tz;
    block_excl_scan2(nchange, 0, L->scan, &xc, &xz, &tc, &tz);
    double cmax;
    double m = fmax(carry_max, block_excl_suffix_max(lmax, L->smax, &cmax));
    i64 after = carry_cnt + (tc - xc - nchange);                   // terms behind this thread's entries
#pragma unroll
    for (int q = VA_ITEMS - 1; q >= 0; --q) {
      if (lo + q >= e1) continue;
      m = fmax(m, pr[q]);                                          // :72-73 the envelope
      if ((change >> q) & 1u) terms[after++] = (rc[q + 1] - rc[q]) * m;              // :82
    }
    carry_max = fmax(carry_max, cmax);
    end_tp -= ttp; end_fp -= tfp; carry_cnt += tc;
  }
  __syncthreads();                                                 // (this block's own global writes, read below)
  const double sum = voc_np_sum(terms, carry_cnt, L->red);
  if (tid == 0) *ap_area = sum;
}

// npos of a class: sum over its segments of weight(image) * npos(segment)
__device__ i64 voc_class_npos(int s0, int s1, const int32_t* __restrict__ seg_npos, const int32_t* __restrict__ seg_image,
                              const int32_t* __restrict__ counts, int num_images, VocCurveLds* L) {
  i64 part = 0;
  for (int s = s0 + (int)threadIdx.x; s < s1; s += VA_THREADS) {
    i64 w = 1;
    if (counts) {
      const int im = seg_image[s];
      w = (im >= 0 && im < num_images) ? (i64)counts[im] : 0;
    }
    part += w * (i64)seg_npos[s];
  }
  i64 xa, xb, ta, tb;
  block_excl_scan2(part, 0, L->scan, &xa, &xb, &ta, &tb);
  __syncthreads();
  return ta;
}

struct VocAccParams {
  const int32_t* cls_seg_off; const int32_t* cls_e_off; const int32_t* seg_npos; const int32_t* order;
  const uint8_t* flag; const int32_t* image;
  double thr[ODET_VOC_R];
  int num_entries, num_segments;
  double* rec; double* prec; double* ap07; double* ap_area; int64_t* npos; uint8_t* sflag; int32_t* simg;
  double* terms;
};

__global__ void __launch_bounds__(VA_THREADS) k_voc_accumulate(VocAccParams p) {
  __shared__ VocCurveLds L;
  const int k = blockIdx.x, tid = threadIdx.x;
  for (int j = tid; j < ODET_VOC_R; j += VA_THREADS) L.thr[j] = p.thr[j];
  int s0 = p.cls_seg_off[k], s1 = p.cls_seg_off[k + 1];
  int e0 = p.cls_e_off[k], e1 = p.cls_e_off[k + 1];
  s0 = max(s0, 0); s1 = min(s1, p.num_segments); e0 = max(e0, 0); e1 = min(e1, p.num_entries);
  // the entries in the class's score order (:169-171), once, so that the curve and the bootstrap read them in a row
  for (int pos = e0 + tid; pos < e1; pos += VA_THREADS) {
    const int e = p.order[pos];
    const bool ok = e >= 0 && e < p.num_entries;
    p.sflag[pos] = ok ? p.flag[e] : (uint8_t)ODET_VOC_IGNORED;
    p.simg[pos] = ok ? p.image[e] : -1;
  }
  __syncthreads();                                                 // (this block's own global writes, read below)
  const i64 npos = voc_class_npos(s0, s1, p.seg_npos, nullptr, nullptr, 0, &L);
  double a07 = 0.0, aar = 0.0;
  voc_curve(e0, e1, p.sflag, p.simg, nullptr, 0, false, npos, &L, p.rec, p.prec, true, true, p.terms + (e0 + k), &a07, &aar);
  if (tid == 0) { p.ap07[k] = a07; p.ap_area[k] = aar; p.npos[k] = npos; }
}

extern "C" int odet_voc_accumulate(int num_classes, int num_segments, int num_entries, const int32_t* cls_seg_off,
                                   const int32_t* cls_entry_off, const int32_t* seg_npos, const int32_t* order,
                                   const uint8_t* entry_flag, const int32_t* entry_image, const double* rec_thrs,
                                   double* out_rec, double* out_prec, double* out_ap07, double* out_ap_area,
                                   int64_t* out_npos, uint8_t* out_sorted_flag, int32_t* out_sorted_image,
                                   void* workspace, size_t workspace_bytes, odet_stream_t stream) {
  ODET_REQUIRE(num_classes >= 1 && num_segments >= 0 && num_entries >= 0, "odet_voc_accumulate: bad sizes");
  if (num_entries > ODET_VOC_MAX_ENTRIES)
    return odet_set_error(ODET_E_LIMIT, "odet_voc_accumulate: %d detections exceed %d", num_entries,
                          ODET_VOC_MAX_ENTRIES);
  ODET_REQUIRE(cls_seg_off && cls_entry_off && rec_thrs && out_ap07 && out_ap_area && out_npos,
               "odet_voc_accumulate: null pointer");
  ODET_REQUIRE(num_segments == 0 || seg_npos, "odet_voc_accumulate: null pointer");
  ODET_REQUIRE(num_entries == 0 || (order && entry_flag && entry_image && out_rec && out_prec && out_sorted_flag &&
                                    out_sorted_image), "odet_voc_accumulate: null pointer");
  const size_t need = odet_voc_eval_workspace_bytes(num_entries, num_classes, 1, ODET_VOC_AP_AREA);
  if (!workspace || workspace_bytes < need)
    return odet_set_error(ODET_E_WORKSPACE, "odet_voc_accumulate: workspace too small (%zu < %zu)", workspace_bytes, need);
  VocAccParams p;
  p.terms = (double*)workspace;
  p.cls_seg_off = cls_seg_off; p.cls_e_off = cls_entry_off; p.seg_npos = seg_npos; p.order = order;
  p.flag = entry_flag; p.image = entry_image;
  for (int j = 0; j < ODET_VOC_R; ++j) p.thr[j] = rec_thrs[j];
  p.num_entries = num_entries; p.num_segments = num_segments;
  p.rec = out_rec; p.prec = out_prec; p.ap07 = out_ap07; p.ap_area = out_ap_area; p.npos = out_npos;
  p.sflag = out_sorted_flag; p.simg = out_sorted_image;
  hipLaunchKernelGGL(k_voc_accumulate, dim3(num_classes), dim3(VA_THREADS), 0, (hipStream_t)stream, p);
  ODET_LAUNCH_CHECK();
  return ODET_OK;
}

// ------------------------------------------------------------------------------- the bootstrap --
struct VocBootParams {
  const int32_t* cls_seg_off; const int32_t* cls_e_off; const int32_t* seg_image; const int32_t* seg_npos;
  const uint8_t* sflag; const int32_t* simg; const int32_t* counts;
  double thr[ODET_VOC_R];
  int num_entries, num_segments, num_images, num_classes, metric;
  double* ap; int64_t* npos; double* terms;
};

__global__ void __launch_bounds__(VA_THREADS) k_voc_bootstrap(VocBootParams p) {
  __shared__ VocCurveLds L;
  const int b = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
  for (int j = tid; j < ODET_VOC_R; j += VA_THREADS) L.thr[j] = p.thr[j];
  int s0 = p.cls_seg_off[k], s1 = p.cls_seg_off[k + 1];
  int e0 = p.cls_e_off[k], e1 = p.cls_e_off[k + 1];
  s0 = max(s0, 0); s1 = min(s1, p.num_segments); e0 = max(e0, 0); e1 = min(e1, p.num_entries);
  const int32_t* counts = p.counts + (size_t)b * p.num_images;
  // precision_gate._map_weighted: npos = np.dot(counts, npos_img), w = counts[im], cumsum(tp * w), cumsum((~tp) * w)
  const i64 npos = voc_class_npos(s0, s1, p.seg_npos, p.seg_image, counts, p.num_images, &L);
  double a07 = 0.0, aar = 0.0;
  const bool area = p.metric == ODET_VOC_AP_AREA;
  voc_curve(e0, e1, p.sflag, p.simg, counts, p.num_images, true, npos, &L, nullptr, nullptr, !area, area,
            area ? p.terms + (size_t)b * ((size_t)p.num_entries + p.num_classes) + (e0 + k) : nullptr, &a07, &aar);
  if (tid == 0) {
    p.ap[(size_t)b * p.num_classes + k] = area ? aar : a07;
    p.npos[(size_t)b * p.num_classes + k] = npos;
  }
}

extern "C" int odet_voc_bootstrap(int num_resamples, int num_classes, int num_images, int num_segments,
                                  int num_entries, const int32_t* cls_seg_off, const int32_t* cls_entry_off,
                                  const int32_t* seg_image, const int32_t* seg_npos, const uint8_t* sorted_flag,
                                  const int32_t* sorted_image, const int32_t* counts, const double* rec_thrs,
                                  int metric, double* out_ap, int64_t* out_npos, void* workspace,
                                  size_t workspace_bytes, odet_stream_t stream) {
  ODET_REQUIRE(num_resamples >= 0 && num_classes >= 1 && num_classes <= 65535 && num_images >= 1 &&
               num_segments >= 0 && num_entries >= 0, "odet_voc_bootstrap: bad sizes");
  ODET_REQUIRE(metric == ODET_VOC_AP_07 || metric == ODET_VOC_AP_AREA, "odet_voc_bootstrap: unknown metric %d", metric);
  if (num_entries > ODET_VOC_MAX_ENTRIES)
    return odet_set_error(ODET_E_LIMIT, "odet_voc_bootstrap: %d detections exceed %d", num_entries,
                          ODET_VOC_MAX_ENTRIES);
  if (num_resamples == 0) return ODET_OK;
  ODET_REQUIRE(cls_seg_off && cls_entry_off && counts && rec_thrs && out_ap && out_npos,
               "odet_voc_bootstrap: null pointer");
  ODET_REQUIRE(num_segments == 0 || (seg_image && seg_npos), "odet_voc_bootstrap: null pointer");
  ODET_REQUIRE(num_entries == 0 || (sorted_flag && sorted_image), "odet_voc_bootstrap: null pointer");
  const size_t need = odet_voc_eval_workspace_bytes(num_entries, num_classes, num_resamples, metric);
  if (need && (!workspace || workspace_bytes < need))
    return odet_set_error(ODET_E_WORKSPACE, "odet_voc_bootstrap: workspace too small (%zu < %zu)", workspace_bytes, need);
  VocBootParams p;
  p.terms = (double*)workspace;
  p.cls_seg_off = cls_seg_off; p.cls_e_off = cls_entry_off; p.seg_image = seg_image; p.seg_npos = seg_npos;
  p.sflag = sorted_flag; p.simg = sorted_image; p.counts = counts;
  for (int j = 0; j < ODET_VOC_R; ++j) p.thr[j] = rec_thrs[j];
  p.num_entries = num_entries; p.num_segments = num_segments; p.num_images = num_images; p.num_classes = num_classes;
  p.metric = metric;
  p.ap = out_ap; p.npos = out_npos;
  hipLaunchKernelGGL(k_voc_bootstrap, dim3(num_resamples, num_classes), dim3(VA_THREADS), 0, (hipStream_t)stream, p);
  ODET_LAUNCH_CHECK();
  return ODET_OK;
}
