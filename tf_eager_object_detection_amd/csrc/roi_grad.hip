// The backward of the fused RoI pooling (roi.hip: crop_and_resize + 2x2 max / avg / no pool) with respect to the float32
// feature maps -- TF r1.13's CropAndResizeGradImage and max-pool gradient, with the sums in an order fixed by the data's indices
// (TF and torch scatter with float atomics in whatever order the hardware picks).  B images per launch (the *_images entry
// points; the single-image ones are their B = 1 call): the images share the level shapes, n, P and the modes and lie dense --
// maps / dx [B,H,W,C] per level, rois [B,n,4], roi_level [B,n], count_dev [B], dy / sel [B,n,P,P,C] -- and image b's sel and dx
// are the definition below applied to image b alone, bit for bit.
//
// Definition.  crop = P (POOL_NONE) or 2P.  ty(r,i), tx(r,j): the Taps of roi_taps.h, the forward's own.  Upstream per sample:
//   NONE  g = dy[r,i,j,c]         AVG2  g = dy[r,i>>1,j>>1,c] * 0.25f
//   MAX2  g = dy[r,i>>1,j>>1,c] for the ONE selected sample of the bin and channel (sel, below), nothing for the other three
// A sample with ty.ok && tx.ok adds wx * (wy * g) -- two float32 multiplies and a separate add, no FMA -- to up to four cells:
// wy = 1 - ty.lerp on row ty.lo, ty.lerp on row ty.hi; wx = 1 - tx.lerp on column tx.lo, tx.lerp on tx.hi; when lo == hi both
// contributions are added, the zero-weighted one included.  dx[l][y][x][c] starts at +0.0f and receives its contributions in
// ascending (RoI r; sample row i; top before bottom; sample column j; left before right), RoIs with r < count on level l only.
//
//   k_roi_pool_select   POOL_MAX2: one wave per (image, RoI, output row), lanes along channels (4 each), the four samples of a bin
//                       with lerp_tap in the plain 16-tap form (bit-identical to the forward's deduplicated forms), the
//                       forward's fmaxf tree, and sel[n,P,P,C] (uint8) = the FIRST sample in the order (0,0),(0,1),(1,0),(1,1)
//                       that compares equal to the pooled value: 0..3 = 2*di+dj, 4 = none (an all-NaN bin; rows >= count).
//   k_roi_pool_grad     a GATHER by cell row: no sort, no workspace, no atomics, no memset, nothing read from dx.  A one-wave
//                       workgroup owns (image, level, cell row y, RG_XT cells, 256 channels) and keeps that tile in LDS
//                       (at most 32 x 1 KiB; a lane = 4 channels of a cell: 64 lanes x 16 B, conflict-free).  It walks the RoIs
//                       of its image in ascending order, 64 at a time, lane = RoI: a lane builds its RoI's row axis and a bit mask over
//                       (i, top | bottom) of the sample rows that tap y (2 crop <= 64 bits: P <= 16).  The wave visits the set
//                       bits in order (ballot, readlane); for each hit it runs j ascending, left before right, lanes along
//                       channels, adding into LDS -- an address is only ever updated by one lane, in program order, which
//                       fixes the order of every sum.  The tile is stored once, 16 bytes per lane.  P2 of an 800 x 1333 image
//                       (200 x 334 cells x 256 channels) is 200 x 11 tiles; no kernel needs more than 32 KiB of LDS.
//                       Serial depth of a tile: the hits of the RoIs that tap it, in the worst case 2 crop hits per RoI.
//                       A batch: the image is the slowest index of the grid (B x the tiles of an image, one image's tiles
//                       neighbours) and a tile walks the RoIs of ITS image only, r < count[b] -- the serial depth of a tile does
//                       not grow with B, which a concatenated RoI list with an image index per RoI would make it do.
#include <hip/hip_runtime.h>

#include "roi_taps.h"

#define RG_XT 32          // cells of a row per tile
#define RG_CS 256         // channels per tile
#define RG_MAX_N 8192
#define RG_MAX_P 16
#define RG_MAX_B 64       // images per launch (what the batched training targets hand over)

struct RoiGradParams {
  void* data[ODET_MAX_LEVELS];     // select: the maps (read); grad: dx of each level (written); [B,H,W,C], image 0's base
  int H[ODET_MAX_LEVELS];
  int W[ODET_MAX_LEVELS];
  float stride[ODET_MAX_LEVELS];
  int start[ODET_MAX_LEVELS];      // grad: first workgroup of each level among an image's `tiles`
  const float4* rois;              // [B,n]; roi_level [B,n], count_dev [B], dy / sel [B,n,P,P,C]: image b's rows start at b * n
  const int32_t* roi_level;
  const int32_t* count_dev;
  const float* dy;
  uint8_t* sel;                    // select: written; grad: read (POOL_MAX2)
  int C, n, P, num_levels, slices;
  int tiles;                       // grad: workgroups per image
  float image_h, image_w;
};

__device__ __forceinline__ int rg_rl_i(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ float rg_rl_f(float v, int l) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}
__device__ __forceinline__ int rg_uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

// first of (a, b, c, d) that compares equal to the forward's pooled value (pool4: the same fmaxf tree), 4 = none
__device__ __forceinline__ uint32_t rg_pick(float a, float b, float c, float d) {
  const float o = fmaxf(fmaxf(a, b), fmaxf(c, d));
  return a == o ? 0u : (b == o ? 1u : (c == o ? 2u : (d == o ? 3u : 4u)));
}

template <int NORM>
__global__ void __launch_bounds__(64) k_roi_pool_select(RoiGradParams p) {
  constexpr bool PAD = (NORM == ODET_ROI_NORM_TP_ALIGN);
  const int lane = threadIdx.x;
  const int P = p.P, C = p.C;
  const int row = (int)blockIdx.x / P, py = (int)blockIdx.x - row * P;     // row = b * n + r of [B,n]
  const int b = row / p.n, r = row - b * p.n;
  const int cnt = min(p.count_dev ? p.count_dev[b] : p.n, p.n);
  uint32_t* __restrict__ srow = reinterpret_cast<uint32_t*>(p.sel + ((size_t)row * P + py) * P * C);   // [P][C / 4]
  const int C4 = C >> 2;
  if (r >= cnt) {
    for (int px = 0; px < P; ++px)
      for (int q = lane; q < C4; q += 64) srow[px * C4 + q] = 0x04040404u;
    return;
  }
  const int lvl = min(max(p.roi_level ? p.roi_level[row] : 0, 0), p.num_levels - 1);
  const int H = p.H[lvl], W = p.W[lvl];
  const int crop = 2 * P;
  const RoiBox nb = roi_norm_box<NORM>(p.rois[row], H, W, p.stride[lvl], p.image_h, p.image_w, crop);
  const Axis ay = make_axis(nb.y1n, nb.y2n, nb.Hs, crop);
  const Axis ax = make_axis(nb.x1n, nb.x2n, nb.Ws, crop);
  const float4* __restrict__ feat = reinterpret_cast<const float4*>(p.data[lvl]) + (size_t)b * H * W * C4;   // image b's map
  const Tap ty[2] = {make_tap<PAD>(ay, 2 * py, crop, H), make_tap<PAD>(ay, 2 * py + 1, crop, H)};
  for (int px = 0; px < P; ++px) {
    const Tap tx[2] = {make_tap<PAD>(ax, 2 * px, crop, W), make_tap<PAD>(ax, 2 * px + 1, crop, W)};
    for (int q = lane; q < C4; q += 64) {
      float4 v[2][2];
#pragma unroll
      for (int sy = 0; sy < 2; ++sy) {
#pragma unroll
        for (int sx = 0; sx < 2; ++sx) {
          float4 res = make_float4(0, 0, 0, 0);      // TF: an extrapolated sample is 0
          if (ty[sy].ok && tx[sx].ok) {
            const size_t top = (size_t)ty[sy].lo * W, bot = (size_t)ty[sy].hi * W;
            const float4 tl = feat[(top + tx[sx].lo) * C4 + q], tr = feat[(top + tx[sx].hi) * C4 + q];
            const float4 bl = feat[(bot + tx[sx].lo) * C4 + q], br = feat[(bot + tx[sx].hi) * C4 + q];
            res = lerp_tap(tl, tr, bl, br, tx[sx].lerp, ty[sy].lerp);
          }
          v[sy][sx] = res;
        }
      }
      const uint32_t code = rg_pick(v[0][0].x, v[0][1].x, v[1][0].x, v[1][1].x) |
                            (rg_pick(v[0][0].y, v[0][1].y, v[1][0].y, v[1][1].y) << 8) |
                            (rg_pick(v[0][0].z, v[0][1].z, v[1][0].z, v[1][1].z) << 16) |
                            (rg_pick(v[0][0].w, v[0][1].w, v[1][0].w, v[1][1].w) << 24);
      srow[px * C4 + q] = code;
    }
  }
}

template <int POOL, int NORM>
__global__ void __launch_bounds__(64) k_roi_pool_grad(RoiGradParams p) {
  constexpr bool PAD = (NORM == ODET_ROI_NORM_TP_ALIGN);
  constexpr int S = (POOL == ODET_ROI_POOL_NONE) ? 1 : 2;
  extern __shared__ __align__(16) float4 rg_acc[];     // [cells of the tile][lanes4]
  const int lane = threadIdx.x;
  const int P = p.P, C = p.C, crop = P * S;
  // workgroup -> (image, level, cell row, x tile, channel slice)
  const int img = (int)blockIdx.x / p.tiles, tile = (int)blockIdx.x - img * p.tiles;
  int l = 0;
#pragma unroll
  for (int k = 1; k < ODET_MAX_LEVELS; ++k)
    if (k < p.num_levels && tile >= p.start[k]) l = k;
  const int H = p.H[l], W = p.W[l];
  const int xtiles = (W + RG_XT - 1) / RG_XT;
  int u = tile - p.start[l];
  const int per_row = xtiles * p.slices;
  const int y = u / per_row;
  u -= y * per_row;
  const int xt = u / p.slices, sl = u - xt * p.slices;
  const int x0 = xt * RG_XT, xn = min(RG_XT, W - x0);
  const int ch0 = sl * RG_CS;
  const int lanes4 = min(RG_CS, C - ch0) >> 2;          // lanes that hold channels: lane q = channels ch0 + 4 q ..
  const bool active = lane < lanes4;
  const int C4 = C >> 2;

  for (int i = lane; i < xn * lanes4; i += 64) rg_acc[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  __syncthreads();

  // this image's RoIs, levels, count and upstream rows: the walk below never leaves them
  const size_t row0 = (size_t)img * p.n;
  const float4* __restrict__ rois = p.rois + row0;
  const int32_t* __restrict__ roi_level = p.roi_level ? p.roi_level + row0 : nullptr;
  const int cnt = min(p.count_dev ? p.count_dev[img] : p.n, p.n);
  const float st = p.stride[l];
  const float4* __restrict__ dy4 = reinterpret_cast<const float4*>(p.dy) + row0 * P * P * C4 + (ch0 >> 2) + lane;
  const uint32_t* __restrict__ sel4 = reinterpret_cast<const uint32_t*>(p.sel) + row0 * P * P * C4 + (ch0 >> 2) + lane;
  for (int base = 0; base < cnt; base += 64) {
    // lane = RoI: which (sample row, top | bottom) of it tap cell row y
    const int r = base + lane;
    unsigned long long mask = 0;
    float4 roi = make_float4(0, 0, 0, 0);
    if (r < cnt) {
      const int lv = min(max(roi_level ? roi_level[r] : 0, 0), p.num_levels - 1);
      if (lv == l) {
        roi = rois[r];
        const RoiBox nb = roi_norm_box<NORM>(roi, H, W, st, p.image_h, p.image_w, crop);
        const Axis ay = make_axis(nb.y1n, nb.y2n, nb.Hs, crop);
        for (int i = 0; i < crop; ++i) {
          const Tap t = make_tap<PAD>(ay, i, crop, H);
          if (t.ok) {                                   // (an extrapolated row sets no bit)
            if (t.lo == y) mask |= 1ull << (2 * i);
            if (t.hi == y) mask |= 1ull << (2 * i + 1);
          }
        }
      }
    }
    unsigned long long live = __builtin_amdgcn_ballot_w64(mask != 0);
    while (live) {
      const int L = rg_uni(__builtin_ctzll(live));
      live &= live - 1;
      const int rr = base + L;
      unsigned long long hits = ((unsigned long long)(uint32_t)rg_rl_i((int)(mask >> 32), L) << 32) |
                                (uint32_t)rg_rl_i((int)(uint32_t)mask, L);
      const float4 ur = make_float4(rg_rl_f(roi.x, L), rg_rl_f(roi.y, L), rg_rl_f(roi.z, L), rg_rl_f(roi.w, L));
      // the RoI's axes again, the same operations on the same values: wave-uniform
      const RoiBox nb = roi_norm_box<NORM>(ur, H, W, st, p.image_h, p.image_w, crop);
      const Axis ay = make_axis(nb.y1n, nb.y2n, nb.Hs, crop);
      const Axis ax = make_axis(nb.x1n, nb.x2n, nb.Ws, crop);
      // lane j: sample column j; which of its two cells lie in this tile
      const Tap tx = make_tap<PAD>(ax, min(lane, crop - 1), crop, W);
      const int lo_in = (tx.ok && tx.lo >= x0 && tx.lo < x0 + xn) ? 1 : 0;
      const int hi_in = (tx.ok && tx.hi >= x0 && tx.hi < x0 + xn) ? 1 : 0;
      const unsigned long long jmask = __builtin_amdgcn_ballot_w64(lane < crop && (lo_in | hi_in));
      if (jmask == 0) continue;
      while (hits) {
        const int b = rg_uni(__builtin_ctzll(hits));
        hits &= hits - 1;
        const int i = b >> 1;
        const Tap ty = make_tap<PAD>(ay, i, crop, H);
        const float wy = (b & 1) ? ty.lerp : 1.0f - ty.lerp;
        const size_t rowoff = ((size_t)rr * P + (i / S)) * P;          // dy / sel row of this sample row, in cells
        const uint32_t want_hi = (uint32_t)(2 * (i & 1));
        unsigned long long jm = jmask;
        int j = rg_uni(__builtin_ctzll(jm));
        float4 g = make_float4(0, 0, 0, 0), gn = g;
        uint32_t s = 0, sn = 0;
        if (active) {
          g = dy4[(rowoff + j / S) * C4];
          if (POOL == ODET_ROI_POOL_MAX2) s = sel4[(rowoff + j / S) * C4];
        }
        while (jm) {
          jm &= jm - 1;
          const int jn = jm ? rg_uni(__builtin_ctzll(jm)) : j;
          if (active && jm) {                           // the next column's upstream while this one is added
            gn = dy4[(rowoff + jn / S) * C4];
            if (POOL == ODET_ROI_POOL_MAX2) sn = sel4[(rowoff + jn / S) * C4];
          }
          const int lo = rg_rl_i(tx.lo, j) - x0, hi = rg_rl_i(tx.hi, j) - x0;
          const int lo_ok = rg_rl_i(lo_in, j), hi_ok = rg_rl_i(hi_in, j);
          const float lerp = rg_rl_f(tx.lerp, j);
          if (active) {
            bool kx = true, ky = true, kz = true, kw = true;
            if (POOL == ODET_ROI_POOL_AVG2) { g.x = g.x * 0.25f; g.y = g.y * 0.25f; g.z = g.z * 0.25f; g.w = g.w * 0.25f; }
            if (POOL == ODET_ROI_POOL_MAX2) {
              const uint32_t want = want_hi + (uint32_t)(j & 1);
              kx = (s & 0xFFu) == want; ky = ((s >> 8) & 0xFFu) == want;
              kz = ((s >> 16) & 0xFFu) == want; kw = (s >> 24) == want;
            }
            const float tx_ = wy * g.x, ty_ = wy * g.y, tz_ = wy * g.z, tw_ = wy * g.w;
            if (lo_ok) {                                // left
              const float wl = 1.0f - lerp;
              float4 a = rg_acc[lo * lanes4 + lane];
              if (kx) a.x = a.x + wl * tx_;
              if (ky) a.y = a.y + wl * ty_;
              if (kz) a.z = a.z + wl * tz_;
              if (kw) a.w = a.w + wl * tw_;
              rg_acc[lo * lanes4 + lane] = a;
            }
            if (hi_ok) {                                // right
              float4 a = rg_acc[hi * lanes4 + lane];
              if (kx) a.x = a.x + lerp * tx_;
              if (ky) a.y = a.y + lerp * ty_;
              if (kz) a.z = a.z + lerp * tz_;
              if (kw) a.w = a.w + lerp * tw_;
              rg_acc[hi * lanes4 + lane] = a;
            }
          }
          j = jn; g = gn; s = sn;
        }
      }
    }
  }
  __syncthreads();
  // every element of the tile is written once
  float4* __restrict__ out = reinterpret_cast<float4*>(p.data[l]) + (((size_t)img * H + y) * W + x0) * C4 + (ch0 >> 2);
  for (int i = lane; i < xn * lanes4; i += 64) {
    const int cell = i / lanes4, q = i - cell * lanes4;
    out[(size_t)cell * C4 + q] = rg_acc[i];
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
// the checks every entry point shares, in the forward's order; nothing here touches the device.  `launch` = false (the plan
// query): the shapes alone -- no pointer, mode or stride is looked at.
static int rg_fill(const char* who, bool launch, const odet_level_t* levels, int num_levels, int C, int B, const float* rois,
                   const int32_t* roi_level, int n, const int32_t* count_dev, int norm_mode, int image_h, int image_w, int pool_size,
                   RoiGradParams* p) {
  ODET_REQUIRE(B >= 1, "%s: batch %d must be positive", who, B);
  if (B > RG_MAX_B) return odet_set_error(ODET_E_LIMIT, "%s: batch %d above the limit of %d images", who, B, RG_MAX_B);
  ODET_REQUIRE(n >= 0, "%s: negative n", who);
  ODET_REQUIRE(num_levels > 0 && num_levels <= ODET_MAX_LEVELS, "%s: num_levels %d out of range", who, num_levels);
  ODET_REQUIRE(levels && (rois || n == 0 || !launch), "%s: null pointer", who);
  ODET_REQUIRE(num_levels == 1 || roi_level || n == 0 || !launch, "%s: roi_level required with several levels", who);
  ODET_REQUIRE(C > 0 && (C & 3) == 0, "%s: C must be a positive multiple of 4 (got %d)", who, C);
  if (launch) ODET_REQUIRE(norm_mode >= 0 && norm_mode <= 3, "%s: unknown norm_mode %d", who, norm_mode);
  ODET_REQUIRE(pool_size > 0, "%s: pool_size %d must be positive", who, pool_size);
  if (launch && norm_mode == ODET_ROI_NORM_IMAGE) ODET_REQUIRE(image_h > 0 && image_w > 0, "%s: bad image shape", who);
  if (n > RG_MAX_N) return odet_set_error(ODET_E_LIMIT, "%s: n %d above the limit of %d RoIs", who, n, RG_MAX_N);
  if (pool_size > RG_MAX_P)
    return odet_set_error(ODET_E_LIMIT, "%s: pool_size %d above the limit of %d (a RoI's row mask has 64 bits)", who, pool_size, RG_MAX_P);
  for (int l = 0; l < ODET_MAX_LEVELS; ++l) {
    const odet_level_t* L = &levels[l < num_levels ? l : 0];
    ODET_REQUIRE((L->data || !launch) && L->H > 0 && L->W > 0, "%s: bad level %d", who, l);
    if (launch) {
      ODET_REQUIRE((uintptr_t)L->data % 16 == 0, "%s: level %d must be 16-byte aligned", who, l);
      if (norm_mode != ODET_ROI_NORM_IMAGE) ODET_REQUIRE(L->stride > 0.0f, "%s: bad stride on level %d", who, l);
    }
    if ((size_t)L->H * (size_t)L->W * (size_t)C * 4 >= (1ull << 31))      // (per image; image offsets are size_t)
      return odet_set_error(ODET_E_LIMIT, "%s: level %d is larger than 2 GiB", who, l);
    p->data[l] = const_cast<float*>(L->data); p->H[l] = L->H; p->W[l] = L->W; p->stride[l] = L->stride;
    p->start[l] = 0;
  }
  if (launch)
    ODET_REQUIRE((uintptr_t)rois % 16 == 0 && (uintptr_t)roi_level % 4 == 0 && (uintptr_t)count_dev % 4 == 0,
                 "%s: rois must be 16-byte aligned, roi_level and count_dev 4", who);
  p->rois = (const float4*)rois; p->roi_level = roi_level; p->count_dev = count_dev;
  p->dy = nullptr; p->sel = nullptr;
  p->C = C; p->n = n; p->P = pool_size; p->num_levels = num_levels; p->slices = (C + RG_CS - 1) / RG_CS;
  p->tiles = 0;
  p->image_h = (float)image_h; p->image_w = (float)image_w;
  return ODET_OK;
}

// The launch of k_roi_pool_grad, from the shapes alone (rg_fill's H, W, slices): one workgroup per (image, level, cell row,
// RG_XT cells, RG_CS channels), the image slowest.  Fills p->start and p->tiles.  The launcher and the plan query both size
// the launch here.
static int rg_plan(const char* who, int B, RoiGradParams* p, int* grid, int* lds_bytes) {
  long long tiles = 0;
  int wmax = 0;
  for (int l = 0; l < p->num_levels; ++l) {
    p->start[l] = (int)tiles;
    tiles += (long long)p->H[l] * ((p->W[l] + RG_XT - 1) / RG_XT) * p->slices;
    if (tiles * B >= (1ll << 31)) return odet_set_error(ODET_E_LIMIT, "%s: too many tiles", who);
    wmax = p->W[l] > wmax ? p->W[l] : wmax;
  }
  p->tiles = (int)tiles;
  *grid = (int)(tiles * B);
  *lds_bytes = (int)((wmax < RG_XT ? wmax : RG_XT) * (p->C < RG_CS ? p->C : RG_CS) * sizeof(float));
  return ODET_OK;
}

extern "C" int odet_roi_pool_backward_images_plan(const odet_level_t* levels, int num_levels, int C, int B, int n, int pool_size,
                                                  int* grid, int* tiles_per_image, int* level_start, int* slices, int* lds_bytes) {
  const char* who = "odet_roi_pool_backward_images_plan";
  RoiGradParams p;
  const int rc = rg_fill(who, false, levels, num_levels, C, B, nullptr, nullptr, n, nullptr, 0, 0, 0, pool_size, &p);
  if (rc != ODET_OK) return rc;
  ODET_REQUIRE(grid && tiles_per_image && level_start && slices && lds_bytes, "%s: null pointer", who);
  const int prc = rg_plan(who, B, &p, grid, lds_bytes);
  if (prc != ODET_OK) return prc;
  *tiles_per_image = p.tiles;
  *slices = p.slices;
  for (int l = 0; l < num_levels; ++l) level_start[l] = p.start[l];
  return ODET_OK;
}

static int rg_argmax(const char* who, const odet_level_t* levels, int num_levels, int C, int B, const float* rois,
                     const int32_t* roi_level, int n, const int32_t* count_dev, int norm_mode, int image_h, int image_w,
                     int pool_size, uint8_t* sel, odet_stream_t stream) {
  RoiGradParams p;
  const int rc = rg_fill(who, true, levels, num_levels, C, B, rois, roi_level, n, count_dev, norm_mode, image_h, image_w, pool_size, &p);
  if (rc != ODET_OK) return rc;
  ODET_REQUIRE(sel || n == 0, "%s: null pointer", who);
  ODET_REQUIRE((uintptr_t)sel % 4 == 0, "%s: sel must be 4-byte aligned", who);
  if (n == 0) return ODET_OK;
  p.sel = sel;
  const dim3 grid((unsigned)(B * n * pool_size)), block(64);      // (at most 64 x 8192 x 16 = 2^23)
  hipStream_t st = (hipStream_t)stream;
  switch (norm_mode) {
    case ODET_ROI_NORM_STRIDE: hipLaunchKernelGGL(k_roi_pool_select<ODET_ROI_NORM_STRIDE>, grid, block, 0, st, p); break;
    case ODET_ROI_NORM_IMAGE: hipLaunchKernelGGL(k_roi_pool_select<ODET_ROI_NORM_IMAGE>, grid, block, 0, st, p); break;
    case ODET_ROI_NORM_TP_ALIGN: hipLaunchKernelGGL(k_roi_pool_select<ODET_ROI_NORM_TP_ALIGN>, grid, block, 0, st, p); break;
    default: hipLaunchKernelGGL(k_roi_pool_select<ODET_ROI_NORM_TP_ALIGN_NOPAD>, grid, block, 0, st, p); break;
  }
  ODET_LAUNCH_CHECK();
  return ODET_OK;
}

extern "C" int odet_roi_pool_argmax(const odet_level_t* levels, int num_levels, int C, const float* rois, const int32_t* roi_level,
                                    int n, const int32_t* count_dev, int norm_mode, int image_h, int image_w, int pool_size,
                                    uint8_t* sel, odet_stream_t stream) {
  return rg_argmax("odet_roi_pool_argmax", levels, num_levels, C, 1, rois, roi_level, n, count_dev, norm_mode, image_h, image_w,
                   pool_size, sel, stream);
}

extern "C" int odet_roi_pool_argmax_images(const odet_level_t* levels, int num_levels, int C, int B, const float* rois,
                                           const int32_t* roi_level, int n, const int32_t* count_dev, int norm_mode, int image_h,
                                           int image_w, int pool_size, uint8_t* sel, odet_stream_t stream) {
  return rg_argmax("odet_roi_pool_argmax_images", levels, num_levels, C, B, rois, roi_level, n, count_dev, norm_mode, image_h,
                   image_w, pool_size, sel, stream);
}

template <int POOL>
static void rg_launch_norm(int norm_mode, dim3 grid, unsigned lds, hipStream_t st, const RoiGradParams& p) {
  const dim3 block(64);
  switch (norm_mode) {
    case ODET_ROI_NORM_STRIDE: hipLaunchKernelGGL((k_roi_pool_grad<POOL, ODET_ROI_NORM_STRIDE>), grid, block, lds, st, p); break;
    case ODET_ROI_NORM_IMAGE: hipLaunchKernelGGL((k_roi_pool_grad<POOL, ODET_ROI_NORM_IMAGE>), grid, block, lds, st, p); break;
    case ODET_ROI_NORM_TP_ALIGN: hipLaunchKernelGGL((k_roi_pool_grad<POOL, ODET_ROI_NORM_TP_ALIGN>), grid, block, lds, st, p); break;
    default: hipLaunchKernelGGL((k_roi_pool_grad<POOL, ODET_ROI_NORM_TP_ALIGN_NOPAD>), grid, block, lds, st, p); break;
  }
}

static int rg_backward(const char* who, const odet_level_t* levels, int num_levels, int C, int B, const float* rois,
                       const int32_t* roi_level, int n, const int32_t* count_dev, int norm_mode, int image_h, int image_w,
                       int pool_size, int pool_mode, const float* dy, const uint8_t* sel, odet_stream_t stream) {
  RoiGradParams p;
  const int rc = rg_fill(who, true, levels, num_levels, C, B, rois, roi_level, n, count_dev, norm_mode, image_h, image_w, pool_size, &p);
  if (rc != ODET_OK) return rc;
  ODET_REQUIRE(pool_mode >= 0 && pool_mode <= 2, "%s: unknown pool_mode %d", who, pool_mode);
  ODET_REQUIRE(dy || n == 0, "%s: null pointer", who);
  if (pool_mode == ODET_ROI_POOL_MAX2) ODET_REQUIRE(sel || n == 0, "%s: POOL_MAX2 needs sel (odet_roi_pool_argmax)", who);
  else ODET_REQUIRE(!sel, "%s: sel goes with POOL_MAX2 only", who);
  ODET_REQUIRE((uintptr_t)dy % 16 == 0 && (uintptr_t)sel % 4 == 0, "%s: dy must be 16-byte aligned, sel 4", who);
  // n == 0 (and an image whose count is 0) still writes every dx (zeros)
  int blocks = 0, lds = 0;
  const int prc = rg_plan(who, B, &p, &blocks, &lds);
  if (prc != ODET_OK) return prc;
  p.dy = dy; p.sel = const_cast<uint8_t*>(sel);
  const dim3 grid((unsigned)blocks);
  hipStream_t st = (hipStream_t)stream;
  if (pool_mode == ODET_ROI_POOL_NONE) rg_launch_norm<ODET_ROI_POOL_NONE>(norm_mode, grid, (unsigned)lds, st, p);
  else if (pool_mode == ODET_ROI_POOL_MAX2) rg_launch_norm<ODET_ROI_POOL_MAX2>(norm_mode, grid, (unsigned)lds, st, p);
  else rg_launch_norm<ODET_ROI_POOL_AVG2>(norm_mode, grid, (unsigned)lds, st, p);
  ODET_LAUNCH_CHECK();
  return ODET_OK;
}

extern "C" int odet_roi_pool_backward(const odet_level_t* levels, int num_levels, int C, const float* rois, const int32_t* roi_level,
                                      int n, const int32_t* count_dev, int norm_mode, int image_h, int image_w, int pool_size,
                                      int pool_mode, const float* dy, const uint8_t* sel, odet_stream_t stream) {
  return rg_backward("odet_roi_pool_backward", levels, num_levels, C, 1, rois, roi_level, n, count_dev, norm_mode, image_h, image_w,
                     pool_size, pool_mode, dy, sel, stream);
}

extern "C" int odet_roi_pool_backward_images(const odet_level_t* levels, int num_levels, int C, int B, const float* rois,
                                             const int32_t* roi_level, int n, const int32_t* count_dev, int norm_mode, int image_h,
                                             int image_w, int pool_size, int pool_mode, const float* dy, const uint8_t* sel,
                                             odet_stream_t stream) {
  return rg_backward("odet_roi_pool_backward_images", levels, num_levels, C, B, rois, roi_level, n, count_dev, norm_mode, image_h,
                     image_w, pool_size, pool_mode, dy, sel, stream);
}

// The forward over the same dense layout: the images go through odet_roi_pool_batch (roi.hip; its kernel and plans untouched) in
// groups of at most ODET_MAX_BATCH, each image's pointers made from the base and the image stride, no processing order.  Every
// image's out is what odet_roi_pool gives on that image alone: the batch only changes which workgroup takes which RoI.
extern "C" int odet_roi_pool_images(const odet_level_t* levels, int num_levels, int C, int B, const float* rois,
                                    const int32_t* roi_level, int n, const int32_t* count_dev, int norm_mode, int image_h,
                                    int image_w, int pool_size, int pool_mode, float* out, odet_stream_t stream) {
  const char* who = "odet_roi_pool_images";
  ODET_REQUIRE(B >= 1, "%s: batch %d must be positive", who, B);
  if (B > RG_MAX_B) return odet_set_error(ODET_E_LIMIT, "%s: batch %d above the limit of %d images", who, B, RG_MAX_B);
  ODET_REQUIRE(n >= 0, "%s: negative n", who);
  ODET_REQUIRE(num_levels > 0 && num_levels <= ODET_MAX_LEVELS, "%s: num_levels %d out of range", who, num_levels);
  ODET_REQUIRE(levels && ((rois && out) || n == 0), "%s: null pointer", who);
  ODET_REQUIRE(num_levels == 1 || roi_level || n == 0, "%s: roi_level required with several levels", who);
  ODET_REQUIRE(C > 0 && (C & 3) == 0, "%s: C must be a positive multiple of 4 (got %d)", who, C);
  ODET_REQUIRE(pool_size > 0, "%s: pool_size %d must be positive", who, pool_size);
  for (int l = 0; l < num_levels; ++l) {
    ODET_REQUIRE(levels[l].data && levels[l].H > 0 && levels[l].W > 0, "%s: bad level %d", who, l);
    ODET_REQUIRE((uintptr_t)levels[l].data % 16 == 0, "%s: level %d must be 16-byte aligned", who, l);
  }
  ODET_REQUIRE((uintptr_t)rois % 16 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)roi_level % 4 == 0 && (uintptr_t)count_dev % 4 == 0,
               "%s: rois and out must be 16-byte aligned, roi_level and count_dev 4", who);
  if (n == 0) return ODET_OK;
  const size_t out_stride = (size_t)n * pool_size * pool_size * C;
  for (int b0 = 0; b0 < B; b0 += ODET_MAX_BATCH) {
    const int group = B - b0 < ODET_MAX_BATCH ? B - b0 : ODET_MAX_BATCH;
    odet_level_t lv[ODET_MAX_BATCH][ODET_MAX_LEVELS];
    RoiImageIO io[ODET_MAX_BATCH];
    for (int i = 0; i < group; ++i) {
      const size_t b = (size_t)(b0 + i);
      for (int l = 0; l < num_levels; ++l) {
        lv[i][l] = levels[l];
        lv[i][l].data = levels[l].data + b * (size_t)levels[l].H * (size_t)levels[l].W * (size_t)C;
      }
      io[i] = RoiImageIO{lv[i], rois + b * n * 4, roi_level ? roi_level + b * n : nullptr, count_dev ? count_dev + b : nullptr,
                         nullptr, out + b * out_stride};
    }
    // (the remaining argument rules are the single-image forward's; they refuse the first group before anything is launched)
    const int rc = odet_roi_pool_batch(io, group, num_levels, C, n, norm_mode, image_h, image_w, pool_size, pool_mode,
                                       (hipStream_t)stream, RoiEvents{nullptr, nullptr}, 0);
    if (rc != ODET_OK) return rc;
  }
  return ODET_OK;
}

