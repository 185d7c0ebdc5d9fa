// COCO bbox evaluation: pycocotools' COCOeval (iouType 'bbox', the default Params of setDetParams) as scripts/eval_coco.py:65-73
// eval_by_cocotools runs it.  evaluate() is a sequential greedy match for every (image, category, area range, IoU threshold),
// accumulate() a stable sort and cumulative sums per (category, area range, maxDets).  Everything is float64, as in
// pycocotools; the host (evaluation/coco_eval.py) packs GT and results into segments = (category, image) pairs.
//
//   k_coco_match (grid = segments, one wave): computeIoU + evaluateImg(maxDet = 100) for the 4 area ranges x 10 thresholds.
//     The segment's detections are ranked (stable, score desc) and the best 100 kept; the GT order of each area range
//     (stable, _ignore last) is built by one lane per range; the kept x GT IoU tile is staged in LDS when it fits
//     (recomputed per visit otherwise); then lane a*10 + t walks the greedy match of (area a, threshold t) -- the 40 walks
//     run side by side, every detection's 40 matched / ignored bits leave as two ballots.
//   odet_coco_order: accumulate's np.argsort(-dtScores, kind='mergesort') over each category's concatenation = a stable
//     sort of all kept detections by (category, score desc), ties in concatenation order: three stable LSD radix sorts
//     of sort.hip (low and high word of an order-keeping 64-bit score key, then the category), each pass gathering
//     through the permutation of the previous one.
//   k_coco_accumulate (grid = 10 thresholds x 12 (area, maxDets) x categories): one block scan over the category's
//     sorted entries with rank < maxDets gives the cumulative TP / FP counts; every entry's recall falls in a bucket
//     b = max{j : recThrs[j] <= rc}, the bucket keeps its largest precision and first position, and suffix max / min over
//     the buckets give the envelope at searchsorted(rc, recThrs, 'left') without storing the curves.
#include <climits>

#include "odet_internal.h"

#define CM_THREADS 64
#define CA_THREADS 256
#define CA_ITEMS 8
#define COCO_TA (ODET_COCO_T * ODET_COCO_A)    // 40 (area, threshold) walks; bit a*10 + t
#define COCO_LDS_MAX (150 * 1024)

typedef unsigned long long u64;

struct CocoMatchParams {
  const int32_t* gt_off; const int32_t* dt_off; const int32_t* e_off;
  const double* gt_box; const double* gt_area; const uint8_t* gt_crowd;
  const double* dt_box; const double* dt_score;
  double thr[ODET_COCO_T];
  double arng[2 * ODET_COCO_A];
  int maxd, maxg, tile_cap, gwords, num_entries;
  double* o_score; u64* o_matched; u64* o_ignored; int32_t* o_rank; int32_t* o_npig;
};

// maskApi.c bbIou for one (detection, GT) pair, xywh boxes, float64, no contraction (-ffp-contract=off)
__device__ __forceinline__ double coco_bb_iou(const double* d, double da, const double* g, bool crowd) {
  const double w = fmin(d[2] + d[0], g[2] + g[0]) - fmax(d[0], g[0]);
  if (w <= 0.0) return 0.0;
  const double h = fmin(d[3] + d[1], g[3] + g[1]) - fmax(d[1], g[1]);
  if (h <= 0.0) return 0.0;
  const double i = w * h;
  const double u = crowd ? da : (da + g[2] * g[3]) - i;
  return i / u;
}

static size_t coco_match_lds(int maxd, int maxg, int tile_cap, int gwords) {
  return (size_t)maxd * 8 + (size_t)ODET_COCO_KEEP * 5 * 8 + (size_t)maxg * 5 * 8 + (size_t)tile_cap * 8 +
         (size_t)ODET_COCO_KEEP * 4 + (size_t)ODET_COCO_A * maxg * 4 + (size_t)COCO_TA * gwords * 4 + (size_t)maxg + 16;
}

// (coco_desc_key, the score key of the ranks below and of odet_coco_order: odet_internal.h, shared with voc_eval.hip)

__global__ void __launch_bounds__(CM_THREADS) k_coco_match(CocoMatchParams p) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int s = blockIdx.x, tid = threadIdx.x;
  const int g0 = p.gt_off[s], G = p.gt_off[s + 1] - g0;
  const int d0 = p.dt_off[s], D = p.dt_off[s + 1] - d0;
  const int e0 = p.e_off[s], Dk = p.e_off[s + 1] - e0;
  // the LDS was sized for maxd / maxg: a segment above them (a caller that passed wrong maxima) is skipped, never overrun
  if (G < 0 || D < 0 || G > p.maxg || D > p.maxd || Dk != min(D, ODET_COCO_KEEP) || e0 < 0 ||
      e0 + Dk > p.num_entries)
    return;
  // layout: dkey [maxd] (u64) | kbox [100][4] | karea [100] | gbox [maxg][4] | garea [maxg] | tile [tile_cap] (doubles) |
  //         kidx [100] | gord [4][maxg] | gtm [40][gwords] | gcrowd [maxg]
  u64* dkey = reinterpret_cast<u64*>(smem);
  double* kbox = reinterpret_cast<double*>(dkey + p.maxd);
  double* karea = kbox + ODET_COCO_KEEP * 4;
  double* gbox = karea + ODET_COCO_KEEP;
  double* garea = gbox + (size_t)p.maxg * 4;
  double* tile = garea + p.maxg;
  int* kidx = reinterpret_cast<int*>(tile + p.tile_cap);
  int* gord = kidx + ODET_COCO_KEEP;
  uint32_t* gtm = reinterpret_cast<uint32_t*>(gord + ODET_COCO_A * p.maxg);
  uint8_t* gcrowd = reinterpret_cast<uint8_t*>(gtm + COCO_TA * p.gwords);
  __shared__ int s_nnon[ODET_COCO_A];

  for (int i = tid; i < D; i += CM_THREADS) dkey[i] = coco_desc_key(p.dt_score[d0 + i]);
  for (int j = tid; j < G; j += CM_THREADS) {
    const double* b = p.gt_box + (size_t)(g0 + j) * 4;
    gbox[j * 4 + 0] = b[0]; gbox[j * 4 + 1] = b[1]; gbox[j * 4 + 2] = b[2]; gbox[j * 4 + 3] = b[3];
    garea[j] = p.gt_area[g0 + j];
    gcrowd[j] = p.gt_crowd[g0 + j] ? 1 : 0;
  }
  for (int w = tid; w < COCO_TA * p.gwords; w += CM_THREADS) gtm[w] = 0u;
  __syncthreads();

  // evaluateImg: np.argsort([-d['score']], kind='mergesort')[0:maxDet] -- the stable rank of every detection, by
  // (key, index): a strict total order, so r runs over 0..D-1 once each and every kidx slot below Dk is written
  for (int i = tid; i < D; i += CM_THREADS) {
    const u64 ki = dkey[i];
    int r = 0;
    for (int j = 0; j < D; ++j) {
      const u64 kj = dkey[j];
      r += (kj < ki || (kj == ki && j < i)) ? 1 : 0;
    }
    if (r < Dk) kidx[r] = i;
  }
  // the GT order of each area range: _ignore = iscrowd or area outside [lo, hi]; stable, _ignore last
  if (tid < ODET_COCO_A) {
    const double lo = p.arng[2 * tid], hi = p.arng[2 * tid + 1];
    int nnon = 0;
    for (int j = 0; j < G; ++j) nnon += (gcrowd[j] || garea[j] < lo || garea[j] > hi) ? 0 : 1;
    int pn = 0, pi = nnon;
    for (int j = 0; j < G; ++j) {
      const bool ig = gcrowd[j] || garea[j] < lo || garea[j] > hi;
      gord[tid * p.maxg + (ig ? pi++ : pn++)] = j;
    }
    s_nnon[tid] = nnon;
    p.o_npig[(size_t)s * ODET_COCO_A + tid] = nnon;
  }
  __syncthreads();
  for (int r = tid; r < Dk; r += CM_THREADS) {
    const int i = kidx[r];
    const double* b = p.dt_box + (size_t)(d0 + i) * 4;
    kbox[r * 4 + 0] = b[0]; kbox[r * 4 + 1] = b[1]; kbox[r * 4 + 2] = b[2]; kbox[r * 4 + 3] = b[3];
    karea[r] = b[2] * b[3];                                   // loadRes: ann['area'] = bb[2] * bb[3]
    p.o_score[e0 + r] = p.dt_score[d0 + i];
    p.o_rank[e0 + r] = r;
  }
  __syncthreads();
  const bool use_tile = (long long)Dk * G <= (long long)p.tile_cap;
  if (use_tile) {
    for (int q = tid; q < Dk * G; q += CM_THREADS) {
      const int r = q / G, j = q - r * G;
      tile[q] = coco_bb_iou(kbox + r * 4, karea[r], gbox + j * 4, gcrowd[j] != 0);
    }
    __syncthreads();
  }

  // the greedy match, lane = a*10 + t
  const bool walker = tid < COCO_TA;
  const int a = walker ? tid / ODET_COCO_T : 0, t = walker ? tid - a * ODET_COCO_T : 0;
  const double lo = p.arng[2 * a], hi = p.arng[2 * a + 1];
  const double thr0 = fmin(p.thr[t], 1.0 - 1e-10);             // iou = min([t, 1-1e-10])
  const int nnon = s_nnon[a];
  const int* order = gord + a * p.maxg;
  uint32_t* mym = gtm + (size_t)(walker ? tid : 0) * p.gwords;
  for (int r = 0; r < Dk; ++r) {
    bool matched = false, ignored = false;
    if (walker) {
      double best = thr0;
      int m = -1;
      bool mig = false;
      for (int k = 0; k < G; ++k) {
        const int j = order[k];
        const bool crowd = gcrowd[j] != 0;
        if (((mym[j >> 5] >> (j & 31)) & 1u) && !crowd) continue;   // already matched, not a crowd
        const bool igj = k >= nnon;
        if (m > -1 && !mig && igj) break;                             // matched a regular GT, the rest are ignored
        const double iou = use_tile ? tile[r * G + j] : coco_bb_iou(kbox + r * 4, karea[r], gbox + j * 4, crowd);
        if (iou < best) continue;
        best = iou;
        m = j;
        mig = igj;
      }
      if (m >= 0) {
        mym[m >> 5] |= 1u << (m & 31);
        matched = true;
        ignored = mig;                                                // dtIg = gtIg[m]
      } else {
        ignored = karea[r] < lo || karea[r] > hi;                     // unmatched and outside the area range
      }
    }
    const u64 mb = __ballot(matched), ib = __ballot(ignored);
    if (tid == 0) {
      p.o_matched[e0 + r] = mb;
      p.o_ignored[e0 + r] = ib;
    }
  }
}

extern "C" int odet_coco_match(int num_segments, const int32_t* seg_gt_off, const int32_t* seg_dt_off,
                               const int32_t* seg_entry_off, const double* gt_box, const double* gt_area,
                               const uint8_t* gt_crowd, const double* dt_box, const double* dt_score,
                               const double* iou_thrs, const double* area_rng, int max_seg_dets, int max_seg_gt,
                               int num_entries, double* out_score, uint64_t* out_matched, uint64_t* out_ignored,
                               int32_t* out_rank, int32_t* out_npig, odet_stream_t stream) {
  ODET_REQUIRE(num_segments >= 0 && max_seg_dets >= 0 && max_seg_gt >= 0 && num_entries >= 0,
               "odet_coco_match: negative size");
  if (max_seg_dets > ODET_COCO_MAX_SEG_DETS)
    return odet_set_error(ODET_E_LIMIT, "odet_coco_match: %d detections in one segment exceed %d", max_seg_dets,
                          ODET_COCO_MAX_SEG_DETS);
  if (max_seg_gt > ODET_COCO_MAX_SEG_GT)
    return odet_set_error(ODET_E_LIMIT, "odet_coco_match: %d GT in one segment exceed %d", max_seg_gt,
                          ODET_COCO_MAX_SEG_GT);
  if (num_entries > ODET_COCO_MAX_ENTRIES)
    return odet_set_error(ODET_E_LIMIT, "odet_coco_match: %d kept detections exceed %d", num_entries,
                          ODET_COCO_MAX_ENTRIES);
  if (num_segments == 0) return ODET_OK;
  ODET_REQUIRE(seg_gt_off && seg_dt_off && seg_entry_off && iou_thrs && area_rng && out_npig,
               "odet_coco_match: null pointer");
  ODET_REQUIRE((max_seg_gt == 0 || (gt_box && gt_area && gt_crowd)) &&
               (max_seg_dets == 0 || (dt_box && dt_score && out_score && out_matched && out_ignored && out_rank)),
               "odet_coco_match: null pointer");
  CocoMatchParams p;
  p.gt_off = seg_gt_off; p.dt_off = seg_dt_off; p.e_off = seg_entry_off;
  p.gt_box = gt_box; p.gt_area = gt_area; p.gt_crowd = gt_crowd; p.dt_box = dt_box; p.dt_score = dt_score;
  for (int t = 0; t < ODET_COCO_T; ++t) p.thr[t] = iou_thrs[t];
  for (int k = 0; k < 2 * ODET_COCO_A; ++k) p.arng[k] = area_rng[k];
  p.maxd = max_seg_dets; p.maxg = max_seg_gt; p.gwords = (max_seg_gt + 31) / 32; p.num_entries = num_entries;
  const int maxk = max_seg_dets < ODET_COCO_KEEP ? max_seg_dets : ODET_COCO_KEEP;
  const size_t base = coco_match_lds(p.maxd, p.maxg, 0, p.gwords);
  const long long want = (long long)maxk * max_seg_gt;
  const long long room = base < COCO_LDS_MAX ? (long long)((COCO_LDS_MAX - base) / 8) : 0;
  p.tile_cap = (int)(want < room ? want : room);
  p.o_score = out_score; p.o_matched = (u64*)out_matched; p.o_ignored = (u64*)out_ignored; p.o_rank = out_rank;
  p.o_npig = out_npig;
  const size_t lds = coco_match_lds(p.maxd, p.maxg, p.tile_cap, p.gwords);
  if (lds > COCO_LDS_MAX) return odet_set_error(ODET_E_LIMIT, "odet_coco_match: %zu B of LDS", lds);
  static OdetPerDeviceOnce once;
  ODET_HIP(once.run([] { return hipFuncSetAttribute((const void*)k_coco_match, hipFuncAttributeMaxDynamicSharedMemorySize, COCO_LDS_MAX); }));
  hipLaunchKernelGGL(k_coco_match, dim3(num_segments), dim3(CM_THREADS), lds, (hipStream_t)stream, p);
  ODET_LAUNCH_CHECK();
  return ODET_OK;
}

// ------------------------------------------------------------------------------------ order --
__global__ void __launch_bounds__(256) k_coco_key_lo(int n, const double* __restrict__ score, uint32_t* __restrict__ keys) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) keys[i] = (uint32_t)coco_desc_key(score[i]);
}

// after the sort by the low word: perm = that order, keys = the high word of the entries in that order
__global__ void __launch_bounds__(256) k_coco_key_hi(int n, const double* __restrict__ score, const uint32_t* __restrict__ p1,
                                                     uint32_t* __restrict__ perm, uint32_t* __restrict__ keys) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const uint32_t e = p1[i];
    perm[i] = e;
    keys[i] = (uint32_t)(coco_desc_key(score[e]) >> 32);
  }
}

// after the sort by the high word: perm2 = perm1 composed with it, keys = category of those entries
__global__ void __launch_bounds__(256) k_coco_key_cat(int n, int K, const int32_t* __restrict__ cat_off,
                                                      const uint32_t* __restrict__ perm1, const uint32_t* __restrict__ p2,
                                                      uint32_t* __restrict__ perm2, uint32_t* __restrict__ keys) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const uint32_t e = perm1[p2[i]];
    perm2[i] = e;
    int lo = 0, hi = K;                                  // category = last k with cat_off[k] <= e
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (cat_off[mid] <= (int)e) lo = mid; else hi = mid;
    }
    keys[i] = (uint32_t)lo;
  }
}

__global__ void __launch_bounds__(256) k_coco_compose(int n, const uint32_t* __restrict__ perm2, const uint32_t* __restrict__ p3,
                                                      int32_t* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = (int32_t)perm2[p3[i]];
}

extern "C" size_t odet_coco_eval_workspace_bytes(int num_entries) {
  const size_t n = (size_t)(num_entries > 0 ? num_entries : 1);
  return 6 * odet_align_up(n * 4, 256) + odet_align_up(odet_sort_hist_entries((int)n) * 4, 256) + 256;
}

extern "C" int odet_coco_order(int num_entries, int num_cats, const int32_t* cat_entry_off, const double* entry_score,
                               int32_t* out_order, void* workspace, size_t workspace_bytes, odet_stream_t stream) {
  ODET_REQUIRE(num_entries >= 0 && num_cats >= 1, "odet_coco_order: bad sizes");
  if (num_entries > ODET_COCO_MAX_ENTRIES)
    return odet_set_error(ODET_E_LIMIT, "odet_coco_order: %d entries exceed %d", num_entries, ODET_COCO_MAX_ENTRIES);
  if (num_entries == 0) return ODET_OK;
  ODET_REQUIRE(cat_entry_off && entry_score && out_order, "odet_coco_order: null pointer");
  const size_t need = odet_coco_eval_workspace_bytes(num_entries);
  if (!workspace || workspace_bytes < need)
    return odet_set_error(ODET_E_WORKSPACE, "odet_coco_order: workspace too small (%zu < %zu)", workspace_bytes, need);
  const int n = num_entries;
  OdetArena ar{(char*)workspace, workspace_bytes, 0};
  uint32_t* ka = ar.take<uint32_t>(n);
  uint32_t* va = ar.take<uint32_t>(n);
  uint32_t* kb = ar.take<uint32_t>(n);
  uint32_t* vb = ar.take<uint32_t>(n);
  uint32_t* perm1 = ar.take<uint32_t>(n);
  uint32_t* perm2 = ar.take<uint32_t>(n);
  uint32_t* hist = ar.take<uint32_t>(odet_sort_hist_entries(n));
  ODET_REQUIRE(ka && va && kb && vb && perm1 && perm2 && hist, "odet_coco_order: workspace arena exhausted");
  hipStream_t st = (hipStream_t)stream;
  const OdetSortImage img{ka, va, kb, vb, hist, nullptr};
  const dim3 grid((n + 255) / 256);
  hipLaunchKernelGGL(k_coco_key_lo, grid, dim3(256), 0, st, n, entry_score, ka);
  ODET_LAUNCH_CHECK();
  int rc = odet_sort_keys_desc_batch(n, 1, &img, st);             // (stable: key asc, index asc; result in va)
  if (rc != ODET_OK) return rc;
  hipLaunchKernelGGL(k_coco_key_hi, grid, dim3(256), 0, st, n, entry_score, (const uint32_t*)va, perm1, ka);
  ODET_LAUNCH_CHECK();
  rc = odet_sort_keys_desc_batch(n, 1, &img, st);
  if (rc != ODET_OK) return rc;
  hipLaunchKernelGGL(k_coco_key_cat, grid, dim3(256), 0, st, n, num_cats, cat_entry_off, (const uint32_t*)perm1,
                     (const uint32_t*)va, perm2, ka);
  ODET_LAUNCH_CHECK();
  rc = odet_sort_keys_desc_batch(n, 1, &img, st);
  if (rc != ODET_OK) return rc;
  hipLaunchKernelGGL(k_coco_compose, grid, dim3(256), 0, st, n, (const uint32_t*)perm2, (const uint32_t*)va, out_order);
  ODET_LAUNCH_CHECK();
  return ODET_OK;
}

// ------------------------------------------------------------------------------- accumulate --
struct CocoAccParams {
  const int32_t* cat_seg_off; const int32_t* cat_e_off; const int32_t* npig; const int32_t* order;
  const double* score; const u64* matched; const u64* ignored; const int32_t* rank;
  double rec[ODET_COCO_R];
  int maxdets[ODET_COCO_M];
  int K;
  double* prec; double* recall; double* scores;
};

__global__ void __launch_bounds__(CA_THREADS) k_coco_accumulate(CocoAccParams p) {
  const int t = blockIdx.x, am = blockIdx.y, k = blockIdx.z, tid = threadIdx.x;
  const int a = am / ODET_COCO_M, m = am - a * ODET_COCO_M;
  const int bit = a * ODET_COCO_T + t;
  const int maxdet = p.maxdets[m];
  __shared__ double s_rec[ODET_COCO_R];
  __shared__ u64 s_bmax[ODET_COCO_R];     // largest precision (bits of a non-negative double) of the bucket
  __shared__ int s_bfirst[ODET_COCO_R];   // first sorted position of the bucket
  __shared__ int lds17[17];
  const size_t cell = (size_t)k * (ODET_COCO_A * ODET_COCO_M) + a * ODET_COCO_M + m;
  const size_t kam = (size_t)p.K * ODET_COCO_A * ODET_COCO_M;

  const int s0 = p.cat_seg_off[k], s1 = p.cat_seg_off[k + 1];
  int np_part = 0;
  for (int s = s0 + tid; s < s1; s += CA_THREADS) np_part += p.npig[(size_t)s * ODET_COCO_A + a];
  int npig;
  (void)block_excl_scan(np_part, lds17, &npig);
  if (s1 <= s0 || npig == 0) {                                    // no evalImg of this category, or npig == 0: stays -1
    for (int j = tid; j < ODET_COCO_R; j += CA_THREADS) {
      p.prec[((size_t)t * ODET_COCO_R + j) * kam + cell] = -1.0;
      p.scores[((size_t)t * ODET_COCO_R + j) * kam + cell] = -1.0;
    }
    if (tid == 0) p.recall[(size_t)t * kam + cell] = -1.0;
    return;
  }
  for (int j = tid; j < ODET_COCO_R; j += CA_THREADS) { s_rec[j] = p.rec[j]; s_bmax[j] = 0ull; s_bfirst[j] = INT_MAX; }
  __syncthreads();
  const double dn = (double)npig;
  const int e0 = p.cat_e_off[k], e1 = p.cat_e_off[k + 1];
  int carry_tp = 0, carry_fp = 0, carry_nd = 0;
  for (int base = e0; base < e1; base += CA_THREADS * CA_ITEMS) {
    const int lo = base + tid * CA_ITEMS;
    uint32_t ftp = 0, ffp = 0, finc = 0;                           // per-item flags
    int ctp = 0, cfp = 0, cnd = 0;
#pragma unroll
    for (int q = 0; q < CA_ITEMS; ++q) {
      const int pos = lo + q;
      if (pos < e1) {
        const int e = p.order[pos];
        const bool inc = p.rank[e] < maxdet;
        const bool mt = (p.matched[e] >> bit) & 1ull, ig = (p.ignored[e] >> bit) & 1ull;
        const bool tp = inc && mt && !ig, fp = inc && !mt && !ig;
        finc |= (inc ? 1u : 0u) << q; ftp |= (tp ? 1u : 0u) << q; ffp |= (fp ? 1u : 0u) << q;
        cnd += inc; ctp += tp; cfp += fp;
      }
    }
    int tot_tp, tot_fp, tot_nd;
    const int xtp = block_excl_scan(ctp, lds17, &tot_tp);
    const int xfp = block_excl_scan(cfp, lds17, &tot_fp);
    (void)block_excl_scan(cnd, lds17, &tot_nd);
    int tp = carry_tp + xtp, fp = carry_fp + xfp;
    int cur_b = -1, cur_first = 0;
    double cur_max = 0.0;
#pragma unroll
    for (int q = 0; q < CA_ITEMS; ++q) {
      if (!((finc >> q) & 1u)) continue;
      tp += (ftp >> q) & 1u;
      fp += (ffp >> q) & 1u;
      const double rc = (double)tp / dn;
      const double pr = (double)tp / (((double)fp + (double)tp) + 2.220446049250313e-16);   // np.spacing(1)
      int blo = 0, bhi = ODET_COCO_R;                               // b = max{j : recThrs[j] <= rc} (recThrs[0] = 0)
      while (bhi - blo > 1) {
        const int mid = (blo + bhi) >> 1;
        if (s_rec[mid] <= rc) blo = mid; else bhi = mid;
      }
      if (blo != cur_b) {
        if (cur_b >= 0) {
          atomicMax(&s_bmax[cur_b], (u64)__double_as_longlong(cur_max));
          atomicMin(&s_bfirst[cur_b], cur_first);
        }
        cur_b = blo; cur_first = lo + q; cur_max = pr;
      } else {
        cur_max = fmax(cur_max, pr);
      }
    }
    if (cur_b >= 0) {
      atomicMax(&s_bmax[cur_b], (u64)__double_as_longlong(cur_max));
      atomicMin(&s_bfirst[cur_b], cur_first);
    }
    carry_tp += tot_tp; carry_fp += tot_fp; carry_nd += tot_nd;
  }
  __syncthreads();
  for (int j = tid; j < ODET_COCO_R; j += CA_THREADS) {
    // q[j] = pr_envelope[idx_j] = max over buckets >= j; ss[j] = score at idx_j = the first position of those buckets;
    // both 0 once idx_j == nd (no bucket >= j)
    u64 mx = 0ull;
    int first = INT_MAX;
    for (int b = j; b < ODET_COCO_R; ++b) {
      mx = s_bmax[b] > mx ? s_bmax[b] : mx;
      first = s_bfirst[b] < first ? s_bfirst[b] : first;
    }
    const size_t o = ((size_t)t * ODET_COCO_R + j) * kam + cell;
    p.prec[o] = first == INT_MAX ? 0.0 : __longlong_as_double((long long)mx);
    p.scores[o] = first == INT_MAX ? 0.0 : p.score[p.order[first]];
  }
  if (tid == 0) p.recall[(size_t)t * kam + cell] = carry_nd ? (double)carry_tp / dn : 0.0;
}

extern "C" int odet_coco_accumulate(int num_cats, const int32_t* cat_seg_off, const int32_t* cat_entry_off,
                                    const int32_t* npig, const int32_t* order, const double* entry_score,
                                    const uint64_t* entry_matched, const uint64_t* entry_ignored,
                                    const int32_t* entry_rank, const double* rec_thrs, const int* max_dets,
                                    double* out_precision, double* out_recall, double* out_scores,
                                    odet_stream_t stream) {
  ODET_REQUIRE(num_cats >= 1 && num_cats <= 65535, "odet_coco_accumulate: bad category count");
  ODET_REQUIRE(cat_seg_off && cat_entry_off && rec_thrs && max_dets && out_precision && out_recall && out_scores,
               "odet_coco_accumulate: null pointer");
  CocoAccParams p;
  p.cat_seg_off = cat_seg_off; p.cat_e_off = cat_entry_off; p.npig = npig; p.order = order;
  p.score = entry_score; p.matched = (const u64*)entry_matched; p.ignored = (const u64*)entry_ignored;
  p.rank = entry_rank;
  for (int j = 0; j < ODET_COCO_R; ++j) p.rec[j] = rec_thrs[j];
  for (int m = 0; m < ODET_COCO_M; ++m) p.maxdets[m] = max_dets[m];
  p.K = num_cats;
  p.prec = out_precision; p.recall = out_recall; p.scores = out_scores;
  hipLaunchKernelGGL(k_coco_accumulate, dim3(ODET_COCO_T, ODET_COCO_A * ODET_COCO_M, num_cats), dim3(CA_THREADS), 0,
                     (hipStream_t)stream, p);
  ODET_LAUNCH_CHECK();
  return ODET_OK;
}
