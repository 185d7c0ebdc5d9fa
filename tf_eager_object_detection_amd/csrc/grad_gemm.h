// What the float32 backward kernels share (dense_grad.hip: the Dense layer's dgrad / wgrad; conv_grad.hip: the 3x3
// convolution's wgrad): ONE workgroup tile routine C[n][m] = sum_k A[k][m] * B(k, n) on v_mfma_f32_16x16x4_f32, and the host
// side of the two small launches that follow a gradient GEMM (the ordered sum of a split launch's parts, the bias gradient).
// A kernel supplies only how a K-step's operand rows reach registers (`fetch`); tile shape, LDS layout and padding, the two
// stages with one barrier per K-step, the accumulation order and the stores are written once, here.
#ifndef ODET_GRAD_GEMM_H_
#define ODET_GRAD_GEMM_H_
#include <hip/hip_runtime.h>

#include "conv_f32_common.h"
#include "x3_split.h"

#define DG_BK 32                  // k per K-step
#define DG_PADK 16                // K-major LDS rows: T + 16 floats
#define DG_STRN (DG_BK + 4)       // N-major LDS rows: 36 floats
#define DG_LDS_MAX (80 * 1024)
#define DG_BIAS_LONG_ROWS 4096    // db: from this many rows on, 256 running sums per column instead of 4
#define DG_BIAS_LONG_PHASES 256

// dynamic LDS of a launch with tile edge 32 * wt
static inline unsigned dg_lds_bytes(int wt) { return (unsigned)(2 * 2 * DG_BK * (32 * wt + DG_PADK) * sizeof(float)); }

#ifdef __HIPCC__
// One (32 WT)^2 tile of C by a workgroup of 4 waves (2 along m x 2 along n; a wave holds WT x WT MFMA tiles), k in
// [kbeg, kend) in steps of DG_BK.  fetch(k0, ra, rb): thread `tid` loads its PER = WT 16-byte pieces of the step's A rows
// (piece i = element idx = tid + 256 i: k0 + idx / (T / 4), columns (idx % (T / 4)) * 4 .. + 3 of the tile) and of B (K-major:
// the same indexing along n; N-major: row idx / 8 of the tile, k0 + (idx % 8) * 4 .. + 3), zeros outside the matrices.  A is the
// MFMA's first operand, so a lane ends with four CONSECUTIVE m of one output row n: columns m < mlim of rows n < N are stored
// (16 bytes each, every element once) to out[n * ldc + m], kept only where omask > 0 when omask is given.
template <int WT, bool BKMAJOR, typename Fetch>
__device__ __forceinline__ void dg_tile(Fetch&& fetch, int kbeg, int kend, int m0, int n0, int mlim, int N, long long ldc,
                                        const float* omask, float* out) {
  constexpr int T = 32 * WT;                              // tile edge (m and n)
  constexpr int STRK = T + DG_PADK;
  constexpr int A_ST = DG_BK * STRK;                      // floats per stage and operand (N-major: T * 36 <= A_ST for T <= 128)
  constexpr int PER = T / 32;                             // 16-byte loads per thread, operand and K-step
  extern __shared__ __align__(16) float dg_lds[];
  const int tid = threadIdx.x;
  const int lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
  const int wv = tid >> 6, wm = wv & 1, wn = wv >> 1;

  c3f4 ra[PER], rb[PER];
  auto stash = [&](int stage) {
    float* sa = dg_lds + stage * 2 * A_ST;
    float* sb = sa + A_ST;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int idx = tid + 256 * i;
      *reinterpret_cast<c3f4*>(sa + (idx / (T / 4)) * STRK + (idx % (T / 4)) * 4) = ra[i];
      if constexpr (BKMAJOR) *reinterpret_cast<c3f4*>(sb + (idx / (T / 4)) * STRK + (idx % (T / 4)) * 4) = rb[i];
      else *reinterpret_cast<c3f4*>(sb + (idx / (DG_BK / 4)) * DG_STRN + (idx % (DG_BK / 4)) * 4) = rb[i];
    }
  };

  c3f4 acc[WT][WT];
#pragma unroll
  for (int mt = 0; mt < WT; ++mt)
#pragma unroll
    for (int nt = 0; nt < WT; ++nt) acc[mt][nt] = (c3f4){0.0f, 0.0f, 0.0f, 0.0f};

  const int aoff = wm * (T / 2) + l15;
  const int boff = BKMAJOR ? wn * (T / 2) + l15 : (wn * (T / 2) + l15) * DG_STRN;
  const int steps = (kend - kbeg + DG_BK - 1) / DG_BK;    // (>= 1: the host gives every part at least one k)
  fetch(kbeg, ra, rb);
  stash(0);
  __syncthreads();
  for (int s = 0; s < steps; ++s) {
    const int stage = s & 1;
    if (s + 1 < steps) fetch(kbeg + (s + 1) * DG_BK, ra, rb);
    const float* sa = dg_lds + stage * 2 * A_ST;
    const float* sb = sa + A_ST;
#pragma unroll
    for (int kk = 0; kk < DG_BK / 4; ++kk) {
      const int k = kk * 4 + lq;                          // lane (l15, lq) feeds k = lq of the instruction's four
      float af[WT], bf[WT];
#pragma unroll
      for (int mt = 0; mt < WT; ++mt) af[mt] = sa[k * STRK + aoff + mt * 16];
#pragma unroll
      for (int nt = 0; nt < WT; ++nt) bf[nt] = BKMAJOR ? sb[k * STRK + boff + nt * 16] : sb[boff + nt * 16 * DG_STRN + k];
#pragma unroll
      for (int mt = 0; mt < WT; ++mt)
#pragma unroll
        for (int nt = 0; nt < WT; ++nt)
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[mt], bf[nt], acc[mt][nt], 0, 0, 0);
    }
    if (s + 1 < steps) stash(stage ^ 1);                  // (the stage read in step s - 1: everyone passed the barrier since)
    __syncthreads();
  }

  // lane: output row n = .. + l15, columns m = .. + 4 lq .. + 3 of every MFMA tile
#pragma unroll
  for (int nt = 0; nt < WT; ++nt) {
    const int n = n0 + wn * (T / 2) + nt * 16 + l15;
    if (n >= N) continue;
#pragma unroll
    for (int mt = 0; mt < WT; ++mt) {
      const int m = m0 + wm * (T / 2) + mt * 16 + lq * 4;
      if (m >= mlim) continue;
      c3f4 v = acc[mt][nt];
      if (omask) {
        const c3f4 y = *reinterpret_cast<const c3f4*>(omask + (long long)n * ldc + m);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = y[j] > 0.0f ? v[j] : 0.0f;
      }
      *reinterpret_cast<c3f4*>(out + (long long)n * ldc + m) = v;
    }
  }
}
#endif  // __HIPCC__

// ---- the split-precision form ------------------------------------------------------------------------------------------------
// dg_tile's contract (fetch, k range, tile origin and limits, omask, out; <WT, BKMAJOR>) on the bfloat16 matrix instruction
// v_mfma_f32_16x16x32_bf16: both operands are float32 in memory and in `fetch`'s registers (the ReLU gate is applied there,
// before any split); each is then split in registers into three bfloat16 limbs (x3_split.h: a == a1 + a2 + a3 exactly) and a
// product is the six limb products of conv_x3.hip, each exact in float32, summed in the float32 accumulator:
//
//        a . b  ~  a1 b1 + (a1 b2 + a2 b1) + (a1 b3 + a2 b2 + a3 b1)         (dropped: a2 b3 + a3 b2 + a3 b3 <= 2^-23 |a b|, random sign)
//
// LDS image of a stage: [3 limb planes of A][3 limb planes of B], 2-byte elements, written (8 bytes per piece and limb)
// while the previous K-step's MFMAs run; two stages, one barrier per K-step (32 k = ONE matrix instruction per limb product).
//   K-major plane  [32 k][T + 16 elements]  rows of 2 T + 32 bytes = 8 * odd dwords (40 / 72).  The instruction wants 8 consecutive k
//                  per lane while the contraction index is the slow one here, so the plane is read TRANSPOSED
//                  (ds_read_b64_tr_b16: a group of 16 lanes takes 4 k-rows x 16 columns, a lane ends with 4 k of its column):
//                  lane group q reads rows 4 q .. 4 q + 3, then 16 + 4 q .. 16 + 4 q + 3.  A 32-lane half covers 8 consecutive rows
//                  x 32 bytes, and 8 rows of 8 * odd dwords start in the 8 different multiples of 8 banks: conflict-free.
//   N-major plane  [T n][32 k + 8 elements]  rows of 80 bytes = 4 * odd dwords (dgrad's dz), read plainly (ds_read_b64 at
//                  k = 4 q and 16 + 4 q -- the SAME k per lane as the transposed read gives the other operand): 16 rows of a
//                  half start in the 16 different multiples of 4 banks, a row's two lane groups take dwords 0-1 and 2-3:
//                  conflict-free.
// Every address is a multiple of 8 from a 16-byte aligned dynamic base; a kernel on this routine keeps its static __shared__
// a multiple of 16 bytes (an unaligned base makes the transposed read return wrong data silently) and every lane issues every read (uniform flow).
// Size: dg_x3_lds_bytes -- T = 64: 60 KB (either B): two workgroups (8 waves) per CU; T = 128: 108 KB (K-major B) / 114 KB (N-major),
// above DG_LDS_MAX and inside the CU's 160 KB: ONE workgroup (4 waves, one per SIMD) per CU.
// Order of sums: an element adds the 32 k of a K-step inside one instruction per limb product (the instruction's inner order
// is undocumented, as for the exact form), the products in the order written above from the smallest terms' side LAST
// (a1 b1 first), K-steps ascending.  A function of the shapes alone -- bit-equal from call to call -- no atomics; zeros
// outside the matrices are staged, never stored; every output element written once, in 16-byte stores.
#define DG_X3_LDS_MAX (128 * 1024)
#define DG_X3_STRN 80             // bytes per N-major row: 32 k of 2 bytes + 16

constexpr unsigned dg_x3_plane_bytes(int wt, bool kmajor) {
  return kmajor ? (unsigned)(DG_BK * (2 * 32 * wt + 32)) : (unsigned)(32 * wt * DG_X3_STRN);
}
// dynamic LDS of a launch with tile edge 32 * wt (a multiple of 16: a kernel's own LDS data may follow it)
constexpr unsigned dg_x3_lds_bytes(int wt, bool bkmajor) {
  return 2 * 3 * (dg_x3_plane_bytes(wt, true) + dg_x3_plane_bytes(wt, bkmajor));
}

#ifdef __HIPCC__
typedef short dgx_s4 __attribute__((ext_vector_type(4)));
typedef short dgx_s8 __attribute__((ext_vector_type(8)));
typedef unsigned int dgx_u2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) dgx_s4* dgx_lds_s4;

template <int WT, bool BKMAJOR, typename Fetch>
__device__ __forceinline__ void dg_tile_x3(Fetch&& fetch, int kbeg, int kend, int m0, int n0, int mlim, int N, long long ldc,
                                           const float* omask, float* out) {
  constexpr int T = 32 * WT;
  constexpr int STRK = 2 * T + 32;                        // bytes per K-major row
  constexpr int PA = DG_BK * STRK;                        // bytes per limb plane
  constexpr int PB = BKMAJOR ? PA : T * DG_X3_STRN;
  constexpr int STAGE = 3 * PA + 3 * PB;
  constexpr int PER = T / 32;
  extern __shared__ __align__(16) unsigned char dg_lds_x3[];
  const int tid = threadIdx.x;
  const int lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
  const int wv = tid >> 6, wm = wv & 1, wn = wv >> 1;

  c3f4 ra[PER], rb[PER];
  // a piece's four float32 -> 8 bytes in each of the three limb planes
  auto put = [&](unsigned char* plane0, int plane_bytes, int off, const c3f4 v) {
    unsigned h0, m0_, l0, h1, m1, l1;
    x3_split2((x3f2){v[0], v[1]}, h0, m0_, l0);
    x3_split2((x3f2){v[2], v[3]}, h1, m1, l1);
    *reinterpret_cast<dgx_u2*>(plane0 + off) = (dgx_u2){h0, h1};
    *reinterpret_cast<dgx_u2*>(plane0 + plane_bytes + off) = (dgx_u2){m0_, m1};
    *reinterpret_cast<dgx_u2*>(plane0 + 2 * plane_bytes + off) = (dgx_u2){l0, l1};
  };
  auto stash = [&](int stage) {
    unsigned char* sa = dg_lds_x3 + stage * STAGE;
    unsigned char* sb = sa + 3 * PA;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int idx = tid + 256 * i;
      put(sa, PA, (idx / (T / 4)) * STRK + (idx % (T / 4)) * 8, ra[i]);
      if constexpr (BKMAJOR) put(sb, PB, (idx / (T / 4)) * STRK + (idx % (T / 4)) * 8, rb[i]);
      else put(sb, PB, (idx / (DG_BK / 4)) * DG_X3_STRN + (idx % (DG_BK / 4)) * 8, rb[i]);
    }
  };
  // the 8 k of lane group lq (4 lq .. + 3 and 16 + 4 lq .. + 3) of 16 columns from `col` of a K-major plane, transposed: lane
  // 4 q + p of a group addresses row q, columns 4 p .. 4 p + 3 of the block and receives column l15's four rows
  auto read_tr = [&](const unsigned char* plane, int col) {
    const unsigned char* a = plane + (4 * lq + (l15 >> 2)) * STRK + (col + (l15 & 3) * 4) * 2;
    const dgx_s4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((dgx_lds_s4)a);
    const dgx_s4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((dgx_lds_s4)(a + 16 * STRK));
    return __builtin_bit_cast(x3b8, (dgx_s8)__builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
  };
  // the same 8 k of row `row` of an N-major plane
  auto read_n = [&](const unsigned char* plane, int row) {
    const unsigned char* a = plane + row * DG_X3_STRN + lq * 8;
    const dgx_s4 lo = *reinterpret_cast<const dgx_s4*>(a);
    const dgx_s4 hi = *reinterpret_cast<const dgx_s4*>(a + 32);
    return __builtin_bit_cast(x3b8, (dgx_s8)__builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
  };

  c3f4 acc[WT][WT];
#pragma unroll
  for (int mt = 0; mt < WT; ++mt)
#pragma unroll
    for (int nt = 0; nt < WT; ++nt) acc[mt][nt] = (c3f4){0.0f, 0.0f, 0.0f, 0.0f};

  const int steps = (kend - kbeg + DG_BK - 1) / DG_BK;    // (>= 1: the host gives every part at least one k)
  fetch(kbeg, ra, rb);
  stash(0);
  __syncthreads();
  for (int s = 0; s < steps; ++s) {
    const int stage = s & 1;
    if (s + 1 < steps) fetch(kbeg + (s + 1) * DG_BK, ra, rb);
    const unsigned char* sa = dg_lds_x3 + stage * STAGE;
    const unsigned char* sb = sa + 3 * PA;
    x3b8 af[3][WT];
#pragma unroll
    for (int l = 0; l < 3; ++l)
#pragma unroll
      for (int mt = 0; mt < WT; ++mt) af[l][mt] = read_tr(sa + l * PA, wm * (T / 2) + mt * 16);
#pragma unroll
    for (int nt = 0; nt < WT; ++nt) {
      x3b8 bf[3];
#pragma unroll
      for (int l = 0; l < 3; ++l) {
        if constexpr (BKMAJOR) bf[l] = read_tr(sb + l * PB, wn * (T / 2) + nt * 16);
        else bf[l] = read_n(sb + l * PB, wn * (T / 2) + nt * 16 + l15);
      }
#pragma unroll
      for (int mt = 0; mt < WT; ++mt) {
        c3f4 v = acc[mt][nt];
        v = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[0][mt], bf[0], v, 0, 0, 0);
        v = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[0][mt], bf[1], v, 0, 0, 0);
        v = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[1][mt], bf[0], v, 0, 0, 0);
        v = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[0][mt], bf[2], v, 0, 0, 0);
        v = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[1][mt], bf[1], v, 0, 0, 0);
        v = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[2][mt], bf[0], v, 0, 0, 0);
        acc[mt][nt] = v;
      }
    }
    if (s + 1 < steps) stash(stage ^ 1);                  // (the stage read in step s - 1: everyone passed the barrier since)
    __syncthreads();
  }

  // lane: output row n = .. + l15, columns m = .. + 4 lq .. + 3 of every MFMA tile
#pragma unroll
  for (int nt = 0; nt < WT; ++nt) {
    const int n = n0 + wn * (T / 2) + nt * 16 + l15;
    if (n >= N) continue;
#pragma unroll
    for (int mt = 0; mt < WT; ++mt) {
      const int m = m0 + wm * (T / 2) + mt * 16 + lq * 4;
      if (m >= mlim) continue;
      c3f4 v = acc[mt][nt];
      if (omask) {
        const c3f4 y = *reinterpret_cast<const c3f4*>(omask + (long long)n * ldc + m);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = y[j] > 0.0f ? v[j] : 0.0f;
      }
      *reinterpret_cast<c3f4*>(out + (long long)n * ldc + m) = v;
    }
  }
}
#endif  // __HIPCC__

// ---- host side, defined in dense_grad.hip -----------------------------------------------------------------------------------
// K cut into at most `parts` equal runs of whole K-steps: the run length in *kper, the number of non-empty runs returned (>= 1);
// how many parts a launch asks for is each plan's own rule
int dg_split(long long K, long long parts, int* kper);
// the workspace a launch cut into `parts` needs for its partial [N][M] outputs (uncut: none), and the caller's checked against
// it: ODET_E_WORKSPACE naming the query that sizes it when missing or short; 16-byte aligned
size_t dg_workspace_bytes(int parts, long long N, long long M);
int dg_check_workspace(const char* who, const char* query_name, size_t need, const void* workspace, size_t workspace_bytes);

// out[i] = ((parts[0][i] + parts[1][i]) + ...) + parts[nparts - 1][i] for the total4 16-byte groups of one part, kept only where
// omask > 0 when omask is given
int dg_reduce_parts(const float* parts, int nparts, long long total4, const float* omask, float* out, hipStream_t st);

// db[c] = the column sums of dz over the rows of `count` row-major [rows, cout] matrices taken as ONE list of rows (matrix
// after matrix): the list's rows r = p, p + P, ... are added in ascending r for p = 0 .. P - 1, then the P sums left to right,
// with P = 4 running sums per column below DG_BIAS_LONG_ROWS rows in all and P = DG_BIAS_LONG_PHASES from there on (a rule on
// the row count alone).  dz = y > 0 ? dy : 0 where a matrix has a y.  cout % 64 == 0
struct DgBiasRows {
  const float* dy[ODET_MAX_LEVELS]; const float* y[ODET_MAX_LEVELS];
  long long rows[ODET_MAX_LEVELS];
  int count;
};
int dg_bias_grad(const DgBiasRows& rows, float* db, int cout, hipStream_t st);

#endif  // ODET_GRAD_GEMM_H_
