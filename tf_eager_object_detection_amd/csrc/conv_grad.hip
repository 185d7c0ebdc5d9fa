// The float32 weight gradient of a 3x3 stride-1 'same' convolution with shared weights over a list of maps (the RpnHead over
// the pyramid levels, base_fpn_model.py:393-434) on the exact-float32 matrix instruction (v_mfma_f32_16x16x4_f32):
//
//   dw[co][ky][kx][ci] = sum_level sum_b sum_y sum_x  dz[b,y,x,co] * x[b, y+ky-1, x+kx-1, ci]     (taps outside the map: zero)
//   db[co]             = sum_level sum_b sum_y sum_x  dz[b,y,x,co]
//
// with dz = y_relu > 0 ? dy : 0 formed while the operand is staged (a select, strict '>'), or dy itself for a level without
// y_relu.  x [B,H,W,cin] and dy / y_relu [B,H,W,cout] are the forward's own NHWC tensors, dw [cout][3][3][cin] its weight
// layout; nothing is transposed or copied.  (The INPUT gradient needs no kernel: it is the forward convolution of dz with the
// flipped, transposed weight -- ops.conv3x3_dgrad_f32_levels.)
//
// It is the wgrad arrangement of dense_grad.hip, C[n = co][m = (ky, kx, ci)] = sum_k A[k][m] * B[k][n] with k = the PIXELS of
// all levels numbered through (levels in the order given; in a level image, row, column) and both operands K-major, on the
// SAME tile routine (grad_gemm.h: tile, LDS padding, two stages, one barrier per K-step, stores).  What is new is the A
// operand: column m = (tap, ci) of pixel k is x at the pixel shifted by the tap.  A thread's 16-byte piece lies in ONE tap
// (cin % 32 == 0), which it decodes once; per K-step it decodes its rows' pixels to (level, image, y, x) and reads the shifted
// pixel only when (y + ky - 1, x + kx - 1) lies inside the map -- decided on the COORDINATES, so a shift never reads across a
// row end, an image of the batch or a level; everything else is staged as zeros.  The dz tile is the same for the 9 taps and
// the cin / T channel tiles of a column of workgroups: their re-reads come from L2.
//
// Order of sums (a function of the shapes alone; no atomics; every element of dw and db written exactly once): an element adds
// its products in ascending k, four per matrix instruction.  The contraction is long and the output small (the head: 2304 x
// 512 = 72 tiles of 128^2), so it is CUT along k into cg_plan's `parts` equal runs of whole K-steps; each part leaves its
// float32 partial in the caller's workspace and dense_grad.hip's reduce launch adds the parts in the order 0 .. parts - 1.
// db: dense_grad.hip's bias kernels over the levels' rows numbered through (rows r = p, p + P, ... ascending for p = 0 .. P - 1,
// then the P sums left to right; P = 4 below 4096 pixels, 256 from there on).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "grad_gemm.h"

struct ConvGradLevel {
  const float* x; const float* dy; const float* y;   // y: nullable
  int H, W, HW, start;                                // start: the level's first k (levels past num_levels: K)
};

struct ConvGradParams {
  ConvGradLevel lv[ODET_MAX_LEVELS];
  float* out;                       // dw, or the parts [parts][cout][9 cin]
  int num_levels, cin, cout, K, kper;
};

// ONE kernel for both forms (X3: grad_gemm.h's split-precision tile routine).  s_lv lies in front of the dynamic region, whose
// start the split-precision routine's transposed LDS reads need 16-byte aligned: the table's size is a multiple of 16 and the
// region is declared 16-byte aligned
static_assert(sizeof(ConvGradLevel) * ODET_MAX_LEVELS % 16 == 0, "the level table must keep the dynamic LDS 16-byte aligned");
template <int WT, bool X3>
__global__ void __launch_bounds__(256) k_conv3x3_wgrad(ConvGradParams p) {
  constexpr int T = 32 * WT;
  constexpr int PER = T / 32;
  __shared__ ConvGradLevel s_lv[ODET_MAX_LEVELS];
  const int tid = threadIdx.x;
  const int M = 9 * p.cin, N = p.cout;
  const int tiles_m = (M + T - 1) / T;
  const int m0 = (int)(blockIdx.x % (unsigned)tiles_m) * T, n0 = (int)(blockIdx.x / (unsigned)tiles_m) * T;
  const int kbeg = (int)blockIdx.z * p.kper;
  const int kend = min(p.K, kbeg + p.kper);
#pragma unroll
  for (int l = 0; l < ODET_MAX_LEVELS; ++l)
    if (tid == l) s_lv[l] = p.lv[l];
  __syncthreads();

  // this thread's columns: the same for every piece and K-step (256 i is a multiple of T / 4)
  const int c = (tid % (T / 4)) * 4;
  const int gm = m0 + c, gn = n0 + c;
  const int tap = gm / p.cin;                             // (>= 9 for columns past M: never loaded)
  const int ci = gm - tap * p.cin;
  const int ty = tap / 3 - 1, tx = tap - (tap / 3) * 3 - 1;
  const bool a_on = gm < M, b_on = gn < N;

  auto fetch = [&](int k0, c3f4 (&ra)[PER], c3f4 (&rb)[PER]) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int gk = k0 + (tid + 256 * i) / (T / 4);
      ra[i] = (c3f4){0.0f, 0.0f, 0.0f, 0.0f};
      rb[i] = (c3f4){0.0f, 0.0f, 0.0f, 0.0f};
      if (gk >= kend) continue;
      int l = 0;
#pragma unroll
      for (int j = 1; j < ODET_MAX_LEVELS; ++j) l += (gk >= s_lv[j].start) ? 1 : 0;   // (start = K from num_levels on)
      const ConvGradLevel L = s_lv[l];
      const int r = gk - L.start;                         // pixel (image, y, x) of the level
      if (a_on) {
        const int rem = r - (r / L.HW) * L.HW;
        const int y = rem / L.W, x = rem - y * L.W;
        const int ys = y + ty, xs = x + tx;
        if (ys >= 0 && ys < L.H && xs >= 0 && xs < L.W)   // inside the SAME image's map: r + ty W + tx is that pixel
          ra[i] = *reinterpret_cast<const c3f4*>(L.x + (long long)(r + ty * L.W + tx) * p.cin + ci);
      }
      if (b_on) {
        const long long off = (long long)r * N + gn;
        c3f4 v = *reinterpret_cast<const c3f4*>(L.dy + off);
        if (L.y) {
          const c3f4 yv = *reinterpret_cast<const c3f4*>(L.y + off);
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = yv[j] > 0.0f ? v[j] : 0.0f;
        }
        rb[i] = v;
      }
    }
  };
  if constexpr (X3) dg_tile_x3<WT, true>(fetch, kbeg, kend, m0, n0, M, N, M, nullptr, p.out + (long long)blockIdx.z * N * M);
  else dg_tile<WT, true>(fetch, kbeg, kend, m0, n0, M, N, M, nullptr, p.out + (long long)blockIdx.z * N * M);
}

// ---- host side --------------------------------------------------------------------------------------------------------------
// pixels of all levels: below this, (part + 1) * kper (at most K + 16 parts * 32 of rounding) stays inside int
#define CG_MAX_PIXELS 0x7FFF0000ll

struct ConvGradPlan { int wt, parts, kper; long long tiles, K; };

// Tile and cut of dw [cout][9 cin] with contraction K = batch * sum H W -- a function of the shapes alone.  128 x 128 tiles
// when both edges divide (cin, cout multiples of 128), else 64 x 64.  The output never fills the machine at a detector's
// channel counts, so the contraction is cut: as many parts as bring the launch to 512 workgroups (two of the 128^2 form per
// CU of 256), at most 16, each of at least 64 k, and none below K = 256; parts are equal runs of whole K-steps (dg_split)
static ConvGradPlan cg_plan(long long K, int cin, int cout) {
  ConvGradPlan pl;
  pl.K = K;
  pl.wt = (cin % 128 == 0 && cout % 128 == 0) ? 4 : 2;
  const int T = 32 * pl.wt;
  pl.tiles = (long long)((9 * cin + T - 1) / T) * ((cout + T - 1) / T);
  long long parts = 1;
  if (K >= 256) parts = std::max<long long>(1, std::min<long long>(std::min<long long>(512 / pl.tiles, K / 64), 16));
  pl.parts = dg_split(K, parts, &pl.kper);
  return pl;
}

// The split-precision form's (X3 = true): the same tile rule and target of 512 workgroups, cut so that K / parts >= 128, not
// 64 (dense_grad.hip's dgx_plan: an assumption about a K-step's cost that the measured launches do not bear out; a shape rule)
static ConvGradPlan cgx_plan(long long K, int cin, int cout) {
  ConvGradPlan pl;
  pl.K = K;
  pl.wt = (cin % 128 == 0 && cout % 128 == 0) ? 4 : 2;
  const int T = 32 * pl.wt;
  pl.tiles = (long long)((9 * cin + T - 1) / T) * ((cout + T - 1) / T);
  long long parts = 1;
  if (K >= 256) parts = std::max<long long>(1, std::min<long long>(std::min<long long>(512 / pl.tiles, K / 128), 16));
  pl.parts = dg_split(K, parts, &pl.kper);
  return pl;
}

// ONE walk of the level list, for the query and the entry point: K = batch * sum H W -> num_levels when every level has a
// positive size and K stays below CG_MAX_PIXELS; else the first level that fails, *K >= CG_MAX_PIXELS when it is the sum
static int cg_walk_levels(const odet_conv_grad_level_t* levels, int num_levels, int batch, long long* K) {
  *K = 0;
  for (int l = 0; l < num_levels; ++l) {
    if (levels[l].H < 1 || levels[l].W < 1) return l;
    *K += (long long)batch * levels[l].H * levels[l].W;
    if (*K >= CG_MAX_PIXELS) return l;
  }
  return num_levels;
}

// the argument rules of the entry point (the forward's, conv_f32_plan_levels, on shapes alone); K out for the plan
static int cg_check_shapes(const char* who, const odet_conv_grad_level_t* levels, int num_levels, int batch, int cin, int cout,
                           long long* K) {
  ODET_REQUIRE(levels, "%s: null pointer", who);
  ODET_REQUIRE(num_levels >= 1 && num_levels <= ODET_MAX_LEVELS, "%s: num_levels %d out of range", who, num_levels);
  ODET_REQUIRE(batch > 0, "%s: bad batch", who);
  ODET_REQUIRE(cin > 0 && cin % CONV_F32_BK == 0, "%s: cin %d must be a multiple of %d", who, cin, CONV_F32_BK);
  ODET_REQUIRE(cout > 0 && cout % 64 == 0, "%s: cout %d must be a multiple of 64", who, cout);
  ODET_REQUIRE((unsigned long long)cout * 9ull * cin * 4ull < 0x7FFFFFFFull, "%s: weights too large", who);
  const int l = cg_walk_levels(levels, num_levels, batch, K);
  ODET_REQUIRE(l == num_levels || *K >= CG_MAX_PIXELS, "%s: bad level %d", who, l);
  ODET_REQUIRE(l == num_levels, "%s: more than 2^31 - 2^16 pixels", who);
  return ODET_OK;
}

static size_t cg_workspace_bytes(bool x3, const odet_conv_grad_level_t* levels, int num_levels, int batch, int cin, int cout) {
  long long K;
  if (!levels || num_levels < 1 || num_levels > ODET_MAX_LEVELS || batch < 1 || cin < 1 || cout < 1) return 0;
  if (cg_walk_levels(levels, num_levels, batch, &K) != num_levels) return 0;
  return dg_workspace_bytes((x3 ? cgx_plan(K, cin, cout) : cg_plan(K, cin, cout)).parts, cout, 9ll * cin);
}

extern "C" size_t odet_conv3x3_wgrad_workspace_bytes(const odet_conv_grad_level_t* levels, int num_levels, int batch, int cin,
                                                     int cout) {
  return cg_workspace_bytes(false, levels, num_levels, batch, cin, cout);
}

extern "C" size_t odet_conv3x3_wgrad_x3_workspace_bytes(const odet_conv_grad_level_t* levels, int num_levels, int batch, int cin,
                                                        int cout) {
  return cg_workspace_bytes(true, levels, num_levels, batch, cin, cout);
}

extern "C" int odet_conv3x3_wgrad_x3_plan(const odet_conv_grad_level_t* levels, int num_levels, int batch, int cin, int cout,
                                          int* tile_edge, int* parts) {
  const char* who = "odet_conv3x3_wgrad_x3_plan";
  long long K;
  ODET_REQUIRE(tile_edge && parts, "%s: null pointer", who);
  const int rs = cg_check_shapes(who, levels, num_levels, batch, cin, cout, &K);
  if (rs != ODET_OK) return rs;
  const ConvGradPlan pl = cgx_plan(K, cin, cout);
  *tile_edge = 32 * pl.wt; *parts = pl.parts;
  return ODET_OK;
}

static hipError_t cg_prepare_kernels() {
  static const void* const kernels[] = {(const void*)k_conv3x3_wgrad<4, false>, (const void*)k_conv3x3_wgrad<2, false>};
  static OdetPerDeviceOnce once;
  return conv_f32_raise_lds_limit(&once, kernels, sizeof(kernels) / sizeof(kernels[0]), DG_LDS_MAX);
}

static hipError_t cgx_prepare_kernels() {
  static const void* const kernels[] = {(const void*)k_conv3x3_wgrad<4, true>, (const void*)k_conv3x3_wgrad<2, true>};
  static OdetPerDeviceOnce once;
  return conv_f32_raise_lds_limit(&once, kernels, sizeof(kernels) / sizeof(kernels[0]), DG_X3_LDS_MAX);
}

// (db is not part of the split-precision form: the same ordered float32 sums, the same bits, in either)
static int cg_wgrad(const char* who, bool x3, const odet_conv_grad_level_t* levels, int num_levels, float* dw, float* db, int batch,
                    int cin, int cout, void* workspace, size_t workspace_bytes, odet_stream_t stream) {
  long long K;
  ODET_REQUIRE(dw, "%s: null pointer", who);
  const int rs = cg_check_shapes(who, levels, num_levels, batch, cin, cout, &K);
  if (rs != ODET_OK) return rs;
  ODET_REQUIRE((uintptr_t)dw % 16 == 0 && (uintptr_t)db % 4 == 0, "%s: pointers must be 16-byte aligned (db: 4)", who);
  for (int l = 0; l < num_levels; ++l) {
    ODET_REQUIRE(levels[l].x && levels[l].dy, "%s: null pointer in level %d", who, l);
    ODET_REQUIRE(((uintptr_t)levels[l].x | (uintptr_t)levels[l].dy | (uintptr_t)levels[l].y_relu) % 16 == 0,
                 "%s: maps must be 16-byte aligned", who);
  }
  const ConvGradPlan pl = x3 ? cgx_plan(K, cin, cout) : cg_plan(K, cin, cout);
  const size_t need = dg_workspace_bytes(pl.parts, cout, 9ll * cin);
  const int rw = dg_check_workspace(who, x3 ? "odet_conv3x3_wgrad_x3_workspace_bytes" : "odet_conv3x3_wgrad_workspace_bytes", need,
                                    workspace, workspace_bytes);
  if (rw != ODET_OK) return rw;
  const hipStream_t st = (hipStream_t)stream;
  ODET_HIP(x3 ? cgx_prepare_kernels() : cg_prepare_kernels());
  ConvGradParams p = {};
  DgBiasRows rows = {};
  int k = 0;
  for (int l = 0; l < ODET_MAX_LEVELS; ++l) {
    ConvGradLevel& L = p.lv[l];
    L.start = (int)pl.K;
    if (l >= num_levels) continue;
    L.x = (const float*)levels[l].x; L.dy = (const float*)levels[l].dy; L.y = (const float*)levels[l].y_relu;
    L.H = levels[l].H; L.W = levels[l].W; L.HW = L.H * L.W; L.start = k;
    rows.dy[l] = L.dy; rows.y[l] = L.y; rows.rows[l] = (long long)batch * L.HW;
    k += batch * L.HW;
  }
  rows.count = num_levels;
  p.out = need ? (float*)workspace : dw;
  p.num_levels = num_levels; p.cin = cin; p.cout = cout; p.K = (int)pl.K; p.kper = pl.kper;
  const dim3 grid((unsigned)pl.tiles, 1, (unsigned)pl.parts);
  if (x3) {
    const unsigned lds = dg_x3_lds_bytes(pl.wt, true);
    if (pl.wt == 4) hipLaunchKernelGGL((k_conv3x3_wgrad<4, true>), grid, dim3(256), lds, st, p);
    else hipLaunchKernelGGL((k_conv3x3_wgrad<2, true>), grid, dim3(256), lds, st, p);
  } else {
    if (pl.wt == 4) hipLaunchKernelGGL((k_conv3x3_wgrad<4, false>), grid, dim3(256), dg_lds_bytes(4), st, p);
    else hipLaunchKernelGGL((k_conv3x3_wgrad<2, false>), grid, dim3(256), dg_lds_bytes(2), st, p);
  }
  ODET_LAUNCH_CHECK();
  if (need) {
    const int rr = dg_reduce_parts((const float*)workspace, pl.parts, (long long)cout * 9 * cin / 4, nullptr, dw, st);
    if (rr != ODET_OK) return rr;
  }
  return db ? dg_bias_grad(rows, db, cout, st) : ODET_OK;
}

extern "C" int odet_conv3x3_wgrad_f32_levels(const odet_conv_grad_level_t* levels, int num_levels, float* dw, float* db, int batch,
                                             int cin, int cout, void* workspace, size_t workspace_bytes, odet_stream_t stream) {
  return cg_wgrad("odet_conv3x3_wgrad_f32_levels", false, levels, num_levels, dw, db, batch, cin, cout, workspace, workspace_bytes,
                  stream);
}

extern "C" int odet_conv3x3_wgrad_x3_levels(const odet_conv_grad_level_t* levels, int num_levels, float* dw, float* db, int batch,
                                            int cin, int cout, void* workspace, size_t workspace_bytes, odet_stream_t stream) {
  return cg_wgrad("odet_conv3x3_wgrad_x3_levels", true, levels, num_levels, dw, db, batch, cin, cout, workspace, workspace_bytes,
                  stream);
}
