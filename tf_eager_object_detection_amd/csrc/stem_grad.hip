// The one operator of the FPN stem's training graph (reference model/fpn/resnet_fpn.py:233-242: conv1_conv trainable, bn_conv1
// frozen, conv1_relu, pool1_pad, pool1_pool) that the other backward passes do not have; conv1's weight and bias gradient are
// dense_grad.hip's contraction on the stem's patch matrix:
//   odet_relu_maxpool3_backward_f32   the backward of odet_bias_relu_maxpool's 3x3 / stride 2 / pad 1 floor-mode form: TF's
//                                     MaxPoolGrad through pool1_pad, then ReluGrad.  v = z + bias (one float32 add);  window (p,q)
//                                     covers rows 2p-1..2p+1 and columns 2q-1..2q+1 inside the map;  its winner is the first tap in
//                                     row-major order whose v exceeds every tap before it and +0 (so a window whose maximum is
//                                     <= 0 has none, and a NaN never wins);  dz[i,j] = the float32 sum of dpool[p,q] over the
//                                     windows that (i,j) wins, in ascending (p,q) order, started from the first term;  +0 where
//                                     there is none
// The windows overlap: an odd row (column) belongs to two window rows (columns), so a pixel is in up to four windows.  The
// arrangement: a workgroup of 256 takes SG_BAND window rows of a strip of window columns; a lane owns ONE window
// column and four channels and walks down the band.  It finds each window's winner once, from the six new taps of the step and the
// scan of the row of three it kept in registers from the step above; the winner codes (4 bits a channel) and dpool go to the lane
// of the window column on the left through LDS (two slots in turn: one barrier a step); the window row above stays in registers.
// The lane then writes the two rows (2p-1, 2p) of its two pixel columns (2q, 2q+1) whose windows are all known now.  A strip's last
// window column and a band's row p1 are halos, computed for the neighbours' sums and written by the next strip / band.  No
// atomics, no arg-max tensor in memory, every dz element written exactly once.
#include "grad_elementwise.h"

#define SG_THREADS 256
#define SG_BAND 6               // window rows a workgroup emits (12 map rows); one more is computed as the halo.  2 .. 8 measured
                                // on 400 x 667 x 64: 38.0, 35.3, 36.6, 33.6, 32.0 (6), 35.6 (8) us
#define SG_WAVES 4              // waves per SIMD = workgroups per CU asked for: 102 VGPRs, no scratch (5 and 6 spill and are slower: 48 and 85 us)
#define SG_VEC_MAX 64           // channel vectors (of 4) a workgroup holds per window column: C > 256 goes in chunks
#define SG_NONE 9u              // the winner code of a window that passes nothing (taps are 0..8 = 3 * dy + dx)

struct StemPoolGradParams {
  const float4* z; const float4* bias; const float4* dpool; float4* dz;
  int H, W, OH, OW;
  int vec_per_px;               // C / 4
  int cv;                       // channel vectors per chunk = min(vec_per_px, SG_VEC_MAX)
  int tq;                       // window columns per workgroup = SG_THREADS / cv (>= 4), the last one the halo
  int chunks, strips, bands;    // the grid: chunks * strips * bands * B workgroups
};

struct SgRaw { float4 t[3]; };                                     // one map row's three taps of a window as loaded (z, four channels)
struct SgRowMax { float best[4]; uint32_t win; };                  // a row's first maximum above +0 per channel, its dx (2 bits; 3: none)

// row `r` of the window column whose taps start at column c0 (= 2q - 1): the loads alone, so that they can be in flight across a
// barrier; taps outside the map read as z = 0 and are masked in sg_row_max
static __device__ __forceinline__ SgRaw sg_load_row(const StemPoolGradParams& p, long long img, int r, int c0, int v, bool live) {
  SgRaw o;
#pragma unroll
  for (int dx = 0; dx < 3; ++dx) {
    const int c = c0 + dx;
    o.t[dx] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (live && r >= 0 && r < p.H && c >= 0 && c < p.W) o.t[dx] = p.z[((img * p.H + r) * p.W + c) * p.vec_per_px + v];
  }
  return o;
}

// the row-major scan of one row from +0: v = z + bias, the forward's sum; a tap outside the map never wins.  Scanning a window's
// three rows from +0 and keeping the first row whose maximum is strictly greater gives the window's first maximum: the same winner
// as one scan over the nine taps.
static __device__ __forceinline__ SgRowMax sg_row_max(const StemPoolGradParams& p, const SgRaw& raw, int r, int c0, const float b[4]) {
  SgRowMax o;
  o.win = 0;
  const bool row_in = r >= 0 && r < p.H;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    float best = 0.0f;
    uint32_t win = 3u;
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const float z = c == 0 ? raw.t[dx].x : c == 1 ? raw.t[dx].y : c == 2 ? raw.t[dx].z : raw.t[dx].w;
      const float v = z + b[c];
      if (row_in && c0 + dx >= 0 && c0 + dx < p.W && v > best) { best = v; win = dx; }
    }
    o.best[c] = best;
    o.win |= win << (2 * c);
  }
  return o;
}

struct SgWin { uint32_t k; float g[4]; };                         // four winner codes (4 bits each) and the window's dpool

// adds window w's term to the pixel at tap `tap` of that window: the sum starts from the first term
static __device__ __forceinline__ void sg_add(float acc[4], bool has[4], const SgWin& w, uint32_t tap) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    if (((w.k >> (4 * c)) & 15u) == tap) {
      acc[c] = has[c] ? acc[c] + w.g[c] : w.g[c];
      has[c] = true;
    }
  }
}

__global__ void __launch_bounds__(SG_THREADS, SG_WAVES) k_relu_maxpool3_backward_f32(StemPoolGradParams p) {
  __shared__ uint32_t s_k[2][SG_THREADS];
  __shared__ float4 s_g[2][SG_THREADS];
  int t = blockIdx.x;
  const int chunk = t % p.chunks; t /= p.chunks;
  const int strip = t % p.strips; t /= p.strips;
  const int band = t % p.bands;
  const long long img = t / p.bands;
  const int ql = threadIdx.x / p.cv;                              // the lane's window column inside the strip
  const int v = chunk * p.cv + threadIdx.x % p.cv;
  const int q = strip * (p.tq - 1) + ql;
  const bool live = ql < p.tq && v < p.vec_per_px && q < p.OW;   // the lane has a window column
  const bool writes = live && ql < p.tq - 1;                      // ... and it is not the strip's halo
  const bool has_right = writes && q + 1 < p.OW;                  // (ql + 1 < tq: the neighbour is in this workgroup)
  const int p0 = band * SG_BAND, p1 = min(p0 + SG_BAND, p.OH);
  float b[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (live) { const float4 bv = p.bias[v]; b[0] = bv.x; b[1] = bv.y; b[2] = bv.z; b[3] = bv.w; }
  const int c0 = 2 * q - 1;
  const SgWin none = {SG_NONE * 0x1111u, {0.0f, 0.0f, 0.0f, 0.0f}};
  SgWin up = none, up_right = none;                               // the window row above: this column's and the right one's
  // the window row's top row is the bottom row of the one above: kept as its scan; the two new rows arrive as raw loads that were
  // asked for a step earlier (before that step's barrier), and dpool with them
  SgRowMax top = sg_row_max(p, sg_load_row(p, img, 2 * p0 - 1, c0, v, live), 2 * p0 - 1, c0, b);
  SgRaw raw_mid = sg_load_row(p, img, 2 * p0, c0, v, live);
  SgRaw raw_bot = sg_load_row(p, img, 2 * p0 + 1, c0, v, live);
  float4 g_next = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (live) g_next = ge_stream(&p.dpool[((img * p.OH + p0) * p.OW + q) * p.vec_per_px + v]);
#pragma unroll 1
  for (int pw = p0; pw <= p1; ++pw) {                             // pw == p1: the halo row, or no window at all (p1 == OH)
    const bool window = live && pw < p.OH;
    const SgRowMax mid = sg_row_max(p, raw_mid, 2 * pw, c0, b), bot = sg_row_max(p, raw_bot, 2 * pw + 1, c0, b);
    const float4 gv = g_next;
    if (pw < p1) {                                                // the next step's loads
      const bool more = live && pw + 1 < p.OH;
      raw_mid = sg_load_row(p, img, 2 * pw + 2, c0, v, more);
      raw_bot = sg_load_row(p, img, 2 * pw + 3, c0, v, more);
      if (more) g_next = ge_stream(&p.dpool[((img * p.OH + pw + 1) * p.OW + q) * p.vec_per_px + v]);
    }
    SgWin cur = none;
    if (window) {
      cur.g[0] = gv.x; cur.g[1] = gv.y; cur.g[2] = gv.z; cur.g[3] = gv.w;
      cur.k = 0;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float best = 0.0f;
        uint32_t win = SG_NONE;
        if (top.best[c] > best) { best = top.best[c]; win = (top.win >> (2 * c)) & 3u; }
        if (mid.best[c] > best) { best = mid.best[c]; win = 3u + ((mid.win >> (2 * c)) & 3u); }
        if (bot.best[c] > best) { best = bot.best[c]; win = 6u + ((bot.win >> (2 * c)) & 3u); }
        cur.k |= win << (4 * c);
      }
    }
    const int slot = (pw - p0) & 1;
    s_k[slot][threadIdx.x] = cur.k;
    s_g[slot][threadIdx.x] = make_float4(cur.g[0], cur.g[1], cur.g[2], cur.g[3]);
    __syncthreads();                                              // (slot is written again two steps on, behind the next barrier)
    SgWin right = none;
    if (has_right) {
      right.k = s_k[slot][threadIdx.x + p.cv];
      const float4 gv = s_g[slot][threadIdx.x + p.cv];
      right.g[0] = gv.x; right.g[1] = gv.y; right.g[2] = gv.z; right.g[3] = gv.w;
    }
    if (writes) {
      const int xe = 2 * q, xo = 2 * q + 1;
      const int yo = 2 * pw - 1, ye = 2 * pw;
      if (pw > p0 && yo < p.H) {                                  // the odd row between window rows pw-1 and pw
        float a0[4] = {0.0f, 0.0f, 0.0f, 0.0f}, a1[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        bool h0[4] = {false, false, false, false}, h1[4] = {false, false, false, false};
        sg_add(a0, h0, up, 7); sg_add(a0, h0, cur, 1);
        sg_add(a1, h1, up, 8); sg_add(a1, h1, up_right, 6); sg_add(a1, h1, cur, 2); sg_add(a1, h1, right, 0);
        const long long o = ((img * p.H + yo) * p.W + xe) * p.vec_per_px + v;
        p.dz[o] = make_float4(a0[0], a0[1], a0[2], a0[3]);
        if (xo < p.W) p.dz[o + p.vec_per_px] = make_float4(a1[0], a1[1], a1[2], a1[3]);
      }
      if (pw < p1) {                                              // the even row: window row pw alone
        float a0[4] = {0.0f, 0.0f, 0.0f, 0.0f}, a1[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        bool h0[4] = {false, false, false, false}, h1[4] = {false, false, false, false};
        sg_add(a0, h0, cur, 4);
        sg_add(a1, h1, cur, 5); sg_add(a1, h1, right, 3);
        const long long o = ((img * p.H + ye) * p.W + xe) * p.vec_per_px + v;
        p.dz[o] = make_float4(a0[0], a0[1], a0[2], a0[3]);
        if (xo < p.W) p.dz[o + p.vec_per_px] = make_float4(a1[0], a1[1], a1[2], a1[3]);
      }
    }
    up = cur; up_right = right;
    top = bot;
  }
}

extern "C" int odet_relu_maxpool3_backward_f32(const float* z, const float* bias, const float* dpool, float* dz, int B, int H, int W,
                                               int C, odet_stream_t stream) {
  const char* who = "odet_relu_maxpool3_backward_f32";
  ODET_REQUIRE(z && bias && dpool && dz, "%s: null pointer", who);
  GE_REQUIRE_NHWC(who, B, H, W, C, (uintptr_t)z | (uintptr_t)bias | (uintptr_t)dpool | (uintptr_t)dz);
  if (B == 0) return ODET_OK;
  StemPoolGradParams p;
  p.z = reinterpret_cast<const float4*>(z);
  p.bias = reinterpret_cast<const float4*>(bias);
  p.dpool = reinterpret_cast<const float4*>(dpool);
  p.dz = reinterpret_cast<float4*>(dz);
  p.H = H; p.W = W;
  p.OH = (H - 1) / 2 + 1;
  p.OW = (W - 1) / 2 + 1;
  p.vec_per_px = C / 4;
  p.cv = std::min(p.vec_per_px, SG_VEC_MAX);
  p.tq = SG_THREADS / p.cv;
  p.chunks = (p.vec_per_px + p.cv - 1) / p.cv;
  p.strips = (p.OW + p.tq - 2) / (p.tq - 1);
  p.bands = (p.OH + SG_BAND - 1) / SG_BAND;
  const long long blocks = (long long)p.chunks * p.strips * p.bands * B;
  ODET_REQUIRE(blocks < (1ll << 31), "%s: too many workgroups (%lld)", who, blocks);
  hipLaunchKernelGGL(k_relu_maxpool3_backward_f32, dim3((unsigned)blocks), dim3(SG_THREADS), 0, (hipStream_t)stream, p);
  ODET_LAUNCH_CHECK();
  return ODET_OK;
}
