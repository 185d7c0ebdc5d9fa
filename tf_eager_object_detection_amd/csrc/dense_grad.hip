// The float32 backward of a Dense layer y = relu?(x . w^T + b) (resnet_fpn.py:292-336, the FPN RoI head) on the exact-float32
// matrix instruction of conv_f32.hip (v_mfma_f32_16x16x4_f32: every product and every sum rounded to float32 once):
//
//   odet_dense_dgrad_f32   dx[rows, cin]  = dz . w          contraction along cout   (* (x_relu > 0) in the epilogue)
//   odet_dense_wgrad_f32   dw[cout, cin]  = dz^T . x        contraction along rows;  db[cout] = column sums of dz
//
// with dz = y_relu > 0 ? dy : 0 formed while the operand is staged (TF's ReluGrad: strict '>', a select -- no dz tensor).
// All tensors row-major in the forward's own layouts: x [rows, cin], w [cout, cin], y / dy [rows, cout]; nothing is transposed
// in memory.  Both are ONE kernel, C[n][m] = sum_k A[k][m] * B(k, n) with m = cin in both (the output's contiguous axis):
//
//            A [K][M]                 B                              C [N][M]
//   wgrad    x  [rows][cin]           dz [rows][cout]  (K-major)     dw [cout][cin]
//   dgrad    w  [cout][cin]           dz [rows][cout]  (N-major)     dx [rows][cin]
//
// Tiling (the routine itself is grad_gemm.h's dg_tile, which conv_grad.hip runs too; this file supplies the operand fetch).  A
// workgroup of 4 waves (2 along m x 2 along n) owns a (32 WT)^2 tile, WT = 4 (128 x 128) or 2 (64 x 64); a wave
// holds WT x WT MFMA tiles.  A is the MFMA's first operand, so a lane ends with four CONSECUTIVE m of one output row n: the
// four lanes of a row store 64 contiguous bytes per instruction and every element of C is written once.  A K-step is 32: the
// tile's rows go global -> registers (16-byte loads, the mask applied there) -> LDS while the previous step's MFMAs run (two
// LDS stages, one barrier per step).  LDS rows are padded (K-major: row stride T + 16 floats, N-major: 32 + 4) so that the 64
// lanes of an operand read hit 64 different banks.  Everything outside the matrices (the K tail of wgrad, whose `rows` is
// whatever the sampler delivered; the row edge of dgrad; cin = 96 or 160 against a 64-wide tile) is staged as zeros and
// never stored.
//
// Order of sums (a function of the shape alone; no atomics): an element adds its products in ascending k, four per matrix
// instruction.  A launch with few tiles and a long contraction is SPLIT along k into `ksplit` equal parts of whole K-steps
// (dg_plan: a rule on (M, N, K) only); each part leaves its float32 partial tile in the caller's workspace and a second
// launch adds the parts in the order 0 .. ksplit - 1 and applies the epilogue mask.  db: a column's rows r = p, p + P, ... are
// added in ascending r for p = 0 .. P - 1, then the P sums left to right; P = 4, or 256 from 4096 rows on (a rule on the row
// count alone: a Dense layer run over a pyramid's pixels).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "grad_gemm.h"

struct DenseGradParams {
  const float* a;                 // [K][M]
  const float* b;                 // dy: [K][N] (wgrad) or [N][K] (dgrad)
  const float* bmask;             // y_relu in dy's layout (nullable)
  const float* omask;             // x_relu [N][M] (nullable; a split launch leaves it to the reduction)
  float* out;                     // [N][M], or the parts [ksplit][N][M]
  int M, N, K, kper;              // part z of a launch takes k in [z * kper, min(K, (z + 1) * kper)); kper % DG_BK == 0
};

// the tile routines of grad_gemm.h (X3: the split-precision one) on operands that are plain row-major matrices: ONE operand
// fetch for both forms
template <int WT, bool BKMAJOR, bool X3>
__global__ void __launch_bounds__(256) k_dense_grad(DenseGradParams p) {
  constexpr int T = 32 * WT;
  constexpr int PER = T / 32;
  const int tid = threadIdx.x;
  const int tiles_m = (p.M + T - 1) / T;
  const int m0 = (int)(blockIdx.x % (unsigned)tiles_m) * T, n0 = (int)(blockIdx.x / (unsigned)tiles_m) * T;
  const int kbeg = (int)blockIdx.z * p.kper;
  const int kend = min(p.K, kbeg + p.kper);
  const int M = p.M, N = p.N;
  const long long ldb = BKMAJOR ? N : p.K;

  auto fetch = [&](int k0, c3f4 (&ra)[PER], c3f4 (&rb)[PER]) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int idx = tid + 256 * i;
      {
        const int k = idx / (T / 4), c = (idx % (T / 4)) * 4;
        const int gk = k0 + k, gm = m0 + c;
        ra[i] = (c3f4){0.0f, 0.0f, 0.0f, 0.0f};
        if (gk < kend && gm < M) ra[i] = *reinterpret_cast<const c3f4*>(p.a + (long long)gk * M + gm);
      }
      int gk, gn;
      if constexpr (BKMAJOR) {
        gk = k0 + idx / (T / 4); gn = n0 + (idx % (T / 4)) * 4;
      } else {
        gn = n0 + idx / (DG_BK / 4); gk = k0 + (idx % (DG_BK / 4)) * 4;
      }
      rb[i] = (c3f4){0.0f, 0.0f, 0.0f, 0.0f};
      if (gk < kend && gn < N) {
        const long long off = BKMAJOR ? (long long)gk * ldb + gn : (long long)gn * ldb + gk;
        c3f4 v = *reinterpret_cast<const c3f4*>(p.b + off);
        if (p.bmask) {
          const c3f4 y = *reinterpret_cast<const c3f4*>(p.bmask + off);
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = y[j] > 0.0f ? v[j] : 0.0f;
        }
        rb[i] = v;
      }
    }
  };
  if constexpr (X3) dg_tile_x3<WT, BKMAJOR>(fetch, kbeg, kend, m0, n0, M, N, M, p.omask, p.out + (long long)blockIdx.z * N * M);
  else dg_tile<WT, BKMAJOR>(fetch, kbeg, kend, m0, n0, M, N, M, p.omask, p.out + (long long)blockIdx.z * N * M);
}

// the parts of a split launch, added in the order 0 .. ksplit - 1, and the epilogue mask
__global__ void __launch_bounds__(256) k_dense_grad_reduce(const float* __restrict__ parts, int ksplit, long long total4,
                                                           const float* __restrict__ omask, float* __restrict__ out) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total4; i += (long long)gridDim.x * 256) {
    c3f4 v = reinterpret_cast<const c3f4*>(parts)[i];
    for (int z = 1; z < ksplit; ++z) {
      const c3f4 q = reinterpret_cast<const c3f4*>(parts)[(long long)z * total4 + i];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = v[j] + q[j];
    }
    if (omask) {
      const c3f4 y = reinterpret_cast<const c3f4*>(omask)[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = y[j] > 0.0f ? v[j] : 0.0f;
    }
    reinterpret_cast<c3f4*>(out)[i] = v;
  }
}

// db[c] = sum over the rows of dz[:, c], the rows of the listed matrices numbered through: thread (c, p) adds rows p, p + 4, ...
// in ascending order, then p = 0 .. 3 left to right
__global__ void __launch_bounds__(256) k_dense_bias_grad(DgBiasRows q, float* __restrict__ db, int cout) {
  __shared__ float part[4][64];
  const int c = (int)blockIdx.x * 64 + (threadIdx.x & 63), ph = threadIdx.x >> 6;
  float s = 0.0f;
  if (c < cout) {
    int first = ph;                                       // this thread's first row of the matrix at hand
#pragma unroll
    for (int l = 0; l < ODET_MAX_LEVELS; ++l) {
      if (l >= q.count) break;
      const float* __restrict__ dy = q.dy[l];
      const float* __restrict__ y = q.y[l];
      const long long rows = q.rows[l];
      for (long long r = first; r < rows; r += 4) {
        const long long off = r * cout + c;
        float v = dy[off];
        if (y) v = y[off] > 0.0f ? v : 0.0f;
        s = s + v;
      }
      first = (int)((first + 4 - rows % 4) % 4);
    }
  }
  part[ph][threadIdx.x & 63] = s;
  __syncthreads();
  if (ph == 0 && c < cout) db[c] = ((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) + part[3][threadIdx.x];
}

int dg_reduce_parts(const float* parts, int nparts, long long total4, const float* omask, float* out, hipStream_t st) {
  const unsigned blocks = (unsigned)std::min<long long>((total4 + 255) / 256, 256 * 16);
  hipLaunchKernelGGL(k_dense_grad_reduce, dim3(blocks), dim3(256), 0, st, parts, nparts, total4, omask, out);
  ODET_LAUNCH_CHECK();
  return ODET_OK;
}

// The same sums for a LONG list of rows (a layer run over pixels: the RpnHead's 89 023 at 800 x 1333, where four running sums
// per channel take milliseconds): 256 running sums per channel.  A workgroup owns 16 channels; thread (phase p, quad) adds
// rows r = p, p + 256, ... of the list in ascending r for its four channels (eight loads in flight, the adds in order), then
// one thread per quad adds the phases p = 0 .. 255 left to right.  cout % 16 == 0
__global__ void __launch_bounds__(1024) k_dense_bias_grad_long(DgBiasRows q, float* __restrict__ db, int cout) {
  __shared__ c3f4 part[DG_BIAS_LONG_PHASES][4];
  const int cq = threadIdx.x & 3, ph = threadIdx.x >> 2;
  const int c = (int)blockIdx.x * 16 + cq * 4;
  c3f4 s = (c3f4){0.0f, 0.0f, 0.0f, 0.0f};
  long long first = ph;                                   // this thread's first row of the matrix at hand
#pragma unroll
  for (int l = 0; l < ODET_MAX_LEVELS; ++l) {
    if (l >= q.count) break;
    const float* __restrict__ dy = q.dy[l] + c;
    const float* __restrict__ y = q.y[l] ? q.y[l] + c : nullptr;
    const long long rows = q.rows[l];
    auto load = [&](long long r) {
      c3f4 v = *reinterpret_cast<const c3f4*>(dy + r * cout);
      if (y) {
        const c3f4 yv = *reinterpret_cast<const c3f4*>(y + r * cout);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = yv[j] > 0.0f ? v[j] : 0.0f;
      }
      return v;
    };
    long long r = first;
    for (; r + 7 * DG_BIAS_LONG_PHASES < rows; r += 8 * DG_BIAS_LONG_PHASES) {
      c3f4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = load(r + u * DG_BIAS_LONG_PHASES);
#pragma unroll
      for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] = s[j] + v[u][j];
    }
    for (; r < rows; r += DG_BIAS_LONG_PHASES) {
      const c3f4 v = load(r);
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] = s[j] + v[j];
    }
    first = (first + DG_BIAS_LONG_PHASES - rows % DG_BIAS_LONG_PHASES) % DG_BIAS_LONG_PHASES;
  }
  part[ph][cq] = s;
  __syncthreads();
  if (ph == 0) {
    c3f4 t = part[0][cq];
    for (int p = 1; p < DG_BIAS_LONG_PHASES; ++p) {
      const c3f4 v = part[p][cq];
#pragma unroll
      for (int j = 0; j < 4; ++j) t[j] = t[j] + v[j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) db[c + j] = t[j];        // (db is only 4-byte aligned)
  }
}

int dg_bias_grad(const DgBiasRows& rows, float* db, int cout, hipStream_t st) {
  long long total = 0;
  for (int l = 0; l < rows.count; ++l) total += rows.rows[l];
  if (total >= DG_BIAS_LONG_ROWS && cout % 16 == 0)
    hipLaunchKernelGGL(k_dense_bias_grad_long, dim3((unsigned)(cout / 16)), dim3(1024), 0, st, rows, db, cout);
  else
    hipLaunchKernelGGL(k_dense_bias_grad, dim3((unsigned)((cout + 63) / 64)), dim3(256), 0, st, rows, db, cout);
  ODET_LAUNCH_CHECK();
  return ODET_OK;
}

// ---- host side --------------------------------------------------------------------------------------------------------------
struct DenseGradPlan { int wt, ksplit, kper; long long tiles; };

// tile and split of C [N][M] with contraction K -- a function of the shape alone.  128 x 128 tiles where they still give every
// CU one; else 64 x 64, and when even those leave half the machine idle and the contraction is long, up to 8 parts of at
// least 64 k each (whole K-steps)
static DenseGradPlan dg_plan(int M, int N, int K) {
  DenseGradPlan pl;
  const long long t128 = (long long)((M + 127) / 128) * ((N + 127) / 128);
  pl.wt = t128 >= 256 ? 4 : 2;
  const int T = 32 * pl.wt;
  pl.tiles = (long long)((M + T - 1) / T) * ((N + T - 1) / T);
  int ks = 1;
  if (pl.tiles <= 128 && K >= 256) ks = (int)std::max<long long>(1, std::min<long long>(std::min<long long>(256 / pl.tiles, K / 64), 8));
  pl.ksplit = dg_split(K, ks, &pl.kper);
  return pl;
}

int dg_split(long long K, long long parts, int* kper) {
  *kper = (int)(((K + parts - 1) / parts + DG_BK - 1) / DG_BK * DG_BK);
  return (int)std::max<long long>(1, (K + *kper - 1) / *kper);
}

size_t dg_workspace_bytes(int parts, long long N, long long M) {
  return parts > 1 ? (size_t)parts * (size_t)N * (size_t)M * sizeof(float) : 0;
}

int dg_check_workspace(const char* who, const char* query_name, size_t need, const void* workspace, size_t workspace_bytes) {
  if (!need) return ODET_OK;
  if (!workspace || workspace_bytes < need)
    return odet_set_error(ODET_E_WORKSPACE, "%s: workspace of %zu bytes, %zu needed (%s)", who,
                          workspace ? workspace_bytes : (size_t)0, need, query_name);
  ODET_REQUIRE((uintptr_t)workspace % 16 == 0, "%s: the workspace must be 16-byte aligned", who);
  return ODET_OK;
}

static int dg_check_shape(const char* who, int rows, int cin, int cout) {
  ODET_REQUIRE(rows >= 1, "%s: rows %d must be positive", who, rows);
  ODET_REQUIRE(cin % 32 == 0 && cin >= 64, "%s: cin %d must be a multiple of 32, at least 64", who, cin);
  ODET_REQUIRE(cout > 0 && cout % 64 == 0, "%s: cout %d must be a multiple of 64", who, cout);
  return ODET_OK;
}

// the split-precision form's tile and split (grad_gemm.h: dg_tile_x3) -- again a function of the shape alone.  The same tile
// rule (128 x 128, one workgroup per CU at that form's LDS size, where every CU still gets one); the contraction is cut so
// that K / parts >= 128, not 64 -- chosen on the ASSUMPTION that a K-step would cost about a third of the exact form's, which the
// measured launches do not bear out (tools/grad_x3_bench.py: the step is bound by the in-kernel split); kept as a shape rule
static DenseGradPlan dgx_plan(int M, int N, int K) {
  DenseGradPlan pl;
  const long long t128 = (long long)((M + 127) / 128) * ((N + 127) / 128);
  pl.wt = t128 >= 256 ? 4 : 2;
  const int T = 32 * pl.wt;
  pl.tiles = (long long)((M + T - 1) / T) * ((N + T - 1) / T);
  int ks = 1;
  if (pl.tiles <= 128 && K >= 256) ks = (int)std::max<long long>(1, std::min<long long>(std::min<long long>(256 / pl.tiles, K / 128), 8));
  pl.ksplit = dg_split(K, ks, &pl.kper);
  return pl;
}

static DenseGradPlan dg_plan_of(bool x3, int wgrad, int rows, int cin, int cout) {
  const int N = wgrad ? cout : rows, K = wgrad ? rows : cout;
  return x3 ? dgx_plan(cin, N, K) : dg_plan(cin, N, K);
}

extern "C" size_t odet_dense_grad_workspace_bytes(int wgrad, int rows, int cin, int cout) {
  if (rows < 1 || cin < 1 || cout < 1) return 0;
  return dg_workspace_bytes(dg_plan_of(false, wgrad, rows, cin, cout).ksplit, wgrad ? cout : rows, cin);
}

extern "C" size_t odet_dense_grad_x3_workspace_bytes(int wgrad, int rows, int cin, int cout) {
  if (rows < 1 || cin < 1 || cout < 1) return 0;
  return dg_workspace_bytes(dg_plan_of(true, wgrad, rows, cin, cout).ksplit, wgrad ? cout : rows, cin);
}

extern "C" int odet_dense_grad_x3_plan(int wgrad, int rows, int cin, int cout, int* tile_edge, int* parts) {
  const char* who = "odet_dense_grad_x3_plan";
  ODET_REQUIRE(tile_edge && parts, "%s: null pointer", who);
  const int rs = dg_check_shape(who, rows, cin, cout);
  if (rs != ODET_OK) return rs;
  const DenseGradPlan pl = dg_plan_of(true, wgrad, rows, cin, cout);
  *tile_edge = 32 * pl.wt; *parts = pl.ksplit;
  return ODET_OK;
}

static hipError_t dg_prepare_kernels() {
  static const void* const kernels[] = {(const void*)k_dense_grad<4, true, false>, (const void*)k_dense_grad<4, false, false>,
                                        (const void*)k_dense_grad<2, true, false>, (const void*)k_dense_grad<2, false, false>};
  static OdetPerDeviceOnce once;
  return conv_f32_raise_lds_limit(&once, kernels, sizeof(kernels) / sizeof(kernels[0]), DG_LDS_MAX);
}

static hipError_t dgx_prepare_kernels() {
  static const void* const kernels[] = {(const void*)k_dense_grad<4, true, true>, (const void*)k_dense_grad<4, false, true>,
                                        (const void*)k_dense_grad<2, true, true>, (const void*)k_dense_grad<2, false, true>};
  static OdetPerDeviceOnce once;
  return conv_f32_raise_lds_limit(&once, kernels, sizeof(kernels) / sizeof(kernels[0]), DG_X3_LDS_MAX);
}

// C [N][M] = A^T-free contraction of the file comment; every argument already checked
template <bool BKMAJOR>
static int dg_launch(const char* who, bool x3, const float* a, const float* b, const float* bmask, const float* omask, float* out,
                     int M, int N, int K, void* workspace, size_t workspace_bytes, hipStream_t st) {
  const DenseGradPlan pl = x3 ? dgx_plan(M, N, K) : dg_plan(M, N, K);
  ODET_REQUIRE(pl.tiles < (1ll << 31), "%s: too many workgroups", who);
  const size_t need = dg_workspace_bytes(pl.ksplit, N, M);
  const int rw = dg_check_workspace(who, x3 ? "odet_dense_grad_x3_workspace_bytes" : "odet_dense_grad_workspace_bytes", need,
                                    workspace, workspace_bytes);
  if (rw != ODET_OK) return rw;
  ODET_HIP(x3 ? dgx_prepare_kernels() : dg_prepare_kernels());
  DenseGradParams p;
  p.a = a; p.b = b; p.bmask = bmask; p.omask = need ? nullptr : omask; p.out = need ? (float*)workspace : out;
  p.M = M; p.N = N; p.K = K; p.kper = pl.kper;
  const dim3 grid((unsigned)pl.tiles, 1, (unsigned)pl.ksplit);
  if (x3) {
    const unsigned lds = dg_x3_lds_bytes(pl.wt, BKMAJOR);
    if (pl.wt == 4) hipLaunchKernelGGL((k_dense_grad<4, BKMAJOR, true>), grid, dim3(256), lds, st, p);
    else hipLaunchKernelGGL((k_dense_grad<2, BKMAJOR, true>), grid, dim3(256), lds, st, p);
  } else {
    const unsigned lds = dg_lds_bytes(pl.wt);
    if (pl.wt == 4) hipLaunchKernelGGL((k_dense_grad<4, BKMAJOR, false>), grid, dim3(256), lds, st, p);
    else hipLaunchKernelGGL((k_dense_grad<2, BKMAJOR, false>), grid, dim3(256), lds, st, p);
  }
  ODET_LAUNCH_CHECK();
  if (need) {
    return dg_reduce_parts((const float*)workspace, pl.ksplit, (long long)N * M / 4, omask, out, st);
  }
  return ODET_OK;
}

static int dg_dgrad(const char* who, bool x3, const float* dy, const float* w, const float* y_relu, const float* x_relu, float* dx,
                    int rows, int cin, int cout, void* workspace, size_t workspace_bytes, odet_stream_t stream) {
  ODET_REQUIRE(dy && w && dx, "%s: null pointer", who);
  const int rs = dg_check_shape(who, rows, cin, cout);
  if (rs != ODET_OK) return rs;
  ODET_REQUIRE(((uintptr_t)dy | (uintptr_t)w | (uintptr_t)y_relu | (uintptr_t)x_relu | (uintptr_t)dx) % 16 == 0,
               "%s: pointers must be 16-byte aligned", who);
  return dg_launch<false>(who, x3, w, dy, y_relu, x_relu, dx, cin, rows, cout, workspace, workspace_bytes, (hipStream_t)stream);
}

// (db is not part of the split-precision form: the same ordered float32 sums, the same bits, in either)
static int dg_wgrad(const char* who, bool x3, const float* dy, const float* x, const float* y_relu, float* dw, float* db, int rows,
                    int cin, int cout, void* workspace, size_t workspace_bytes, odet_stream_t stream) {
  ODET_REQUIRE(dy && x && dw, "%s: null pointer", who);
  const int rs = dg_check_shape(who, rows, cin, cout);
  if (rs != ODET_OK) return rs;
  ODET_REQUIRE(((uintptr_t)dy | (uintptr_t)x | (uintptr_t)y_relu | (uintptr_t)dw) % 16 == 0 && (uintptr_t)db % 4 == 0,
               "%s: pointers must be 16-byte aligned (db: 4)", who);
  const int rl = dg_launch<true>(who, x3, x, dy, y_relu, nullptr, dw, cin, cout, rows, workspace, workspace_bytes, (hipStream_t)stream);
  if (rl != ODET_OK) return rl;
  if (db) {
    DgBiasRows q = {};
    q.dy[0] = dy; q.y[0] = y_relu; q.rows[0] = rows; q.count = 1;
    return dg_bias_grad(q, db, cout, (hipStream_t)stream);
  }
  return ODET_OK;
}

extern "C" int odet_dense_dgrad_f32(const float* dy, const float* w, const float* y_relu, const float* x_relu, float* dx, int rows,
                                    int cin, int cout, void* workspace, size_t workspace_bytes, odet_stream_t stream) {
  return dg_dgrad("odet_dense_dgrad_f32", false, dy, w, y_relu, x_relu, dx, rows, cin, cout, workspace, workspace_bytes, stream);
}

extern "C" int odet_dense_dgrad_x3(const float* dy, const float* w, const float* y_relu, const float* x_relu, float* dx, int rows,
                                   int cin, int cout, void* workspace, size_t workspace_bytes, odet_stream_t stream) {
  return dg_dgrad("odet_dense_dgrad_x3", true, dy, w, y_relu, x_relu, dx, rows, cin, cout, workspace, workspace_bytes, stream);
}

extern "C" int odet_dense_wgrad_f32(const float* dy, const float* x, const float* y_relu, float* dw, float* db, int rows, int cin,
                                    int cout, void* workspace, size_t workspace_bytes, odet_stream_t stream) {
  return dg_wgrad("odet_dense_wgrad_f32", false, dy, x, y_relu, dw, db, rows, cin, cout, workspace, workspace_bytes, stream);
}

extern "C" int odet_dense_wgrad_x3(const float* dy, const float* x, const float* y_relu, float* dw, float* db, int rows, int cin,
                                   int cout, void* workspace, size_t workspace_bytes, odet_stream_t stream) {
  return dg_wgrad("odet_dense_wgrad_x3", true, dy, x, y_relu, dw, db, rows, cin, cout, workspace, workspace_bytes, stream);
}
