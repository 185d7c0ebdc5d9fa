// What the float32 backward kernels share (dense_grad.hip: the Dense layer's dgrad / wgrad; conv_grad.hip: the 3x3
// convolution's wgrad): ONE workgroup tile routine C[n][m] = sum_k A[k][m] * B(k, n) on v_mfma_f32_16x16x4_f32, and the host
// side of the two small launches that follow a gradient GEMM (the ordered sum of a split launch's parts, the bias gradient).
// A kernel supplies only how a K-step's operand rows reach registers (`fetch`); tile shape, LDS layout and padding, the two
// stages with one barrier per K-step, the accumulation order and the stores are written once, here.
#ifndef ODET_GRAD_GEMM_H_
#define ODET_GRAD_GEMM_H_
#include <hip/hip_runtime.h>

#include "conv_f32_common.h"

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
