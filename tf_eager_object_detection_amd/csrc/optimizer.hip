// The training step of scripts/train.py:22-50, 101-103 as ONE multi-tensor apply: the L2 regulariser of every kernel
// (keras regularizers.l2), the bias-gradient doubling of train_step, tf.train.piecewise_constant on the global step, and
// MomentumOptimizer / AdamOptimizer.apply_gradients (TF r1.13 training_ops.cc ApplyMomentum / ApplyAdam), for the whole
// variable list in one update launch (grid = number of chunks) and one one-workgroup finish launch.  No allocation, no host
// read, no float atomics; no launch has two workgroups writing one address: the update launch only READS the step and the beta
// powers, the finish launch (after it in stream order) is their only writer.
//
// Arithmetic (include/odet.h "training step").  Every element operation is one float32 operation in the header's order (the
// tree is built without FMA contraction; divide and sqrt are correctly rounded).  The L2 sum of a tensor is a float64 sum in
// an order that is a function of the tensor alone: element j of a chunk belongs to lane (j / 4) % 256 whether the chunk goes
// through the 16-byte path or the scalar one, so the bits do not depend on the alignment either.  tests/optimizer_np.py
// restates all of it with numpy, bit for bit.
//
// Bandwidth bound (appendix "element-wise" of the kernel guide): a lane moves 16 bytes per load / store of a float32 array
// (8 bytes of a float16 one), four such groups per lane in flight (all loads of a chunk are issued before its first store).
#include "odet_internal.h"

#define OPT_THREADS 256
#define OPT_GROUPS (ODET_OPT_CHUNK / (OPT_THREADS * 4))     // groups of 4 elements per lane: 4
#define OPT_WAVES (OPT_THREADS / ODET_WAVE)
#define OPT_FINISH_THREADS 1024
#define OPT_FINISH_WAVES (OPT_FINISH_THREADS / ODET_WAVE)

static_assert(OPT_GROUPS * OPT_THREADS * 4 == ODET_OPT_CHUNK, "a chunk is a whole number of groups per lane");
static_assert(sizeof(odet_opt_tensor_t) == 64 && sizeof(odet_opt_chunk_t) == 16, "table records are part of the ABI");

enum { OPT_L2_ONLY = 0, OPT_MOMENTUM = ODET_OPT_MOMENTUM, OPT_ADAM = ODET_OPT_ADAM };

typedef _Float16 opt_h4 __attribute__((ext_vector_type(4)));

struct OptArgs {
  const odet_opt_tensor_t* tensors; const void* const* grads; const odet_opt_chunk_t* chunks; const odet_opt_state_t* state;
  int num_tensors, num_chunks, num_boundaries;
  float momentum, beta1, beta2, epsilon;
  double* partials;                                         // nullable: no L2 output wanted
};

// four elements j .. j + 3 of an array (the chunk's 16-byte / 8-byte path where `vec` and the group is whole, else element by
// element; elements at or past n read as 0)
__device__ __forceinline__ void d_ld4_f32(const float* p, int64_t j, int64_t n, bool vec, float* o) {
  if (vec && j + 4 <= n) {
    const float4 v = *reinterpret_cast<const float4*>(p + j);
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (j + e < n) ? p[j + e] : 0.0f;
  }
}
__device__ __forceinline__ void d_ld4_f16(const _Float16* p, int64_t j, int64_t n, bool vec, float* o) {
  if (vec && j + 4 <= n) {
    const opt_h4 v = *reinterpret_cast<const opt_h4*>(p + j);
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (float)v[e];         // (exact)
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (j + e < n) ? (float)p[j + e] : 0.0f;
  }
}
__device__ __forceinline__ void d_st4_f32(float* p, int64_t j, int64_t n, bool vec, const float* v) {
  if (vec && j + 4 <= n) {
    *reinterpret_cast<float4*>(p + j) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (j + e < n) p[j + e] = v[e];
  }
}
__device__ __forceinline__ void d_st4_f16(_Float16* p, int64_t j, int64_t n, bool vec, const float* v) {
  if (vec && j + 4 <= n) {
    opt_h4 h;
#pragma unroll
    for (int e = 0; e < 4; ++e) h[e] = (_Float16)v[e];      // round to nearest even, once
    *reinterpret_cast<opt_h4*>(p + j) = h;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (j + e < n) p[j + e] = (_Float16)v[e];
  }
}

// v[i] = v[i] + v[i ^ o] for o = 32, 16, ..., 1: every lane ends with the same bits (the two operands of each sum swap places
// between the partners, and a float64 sum does not depend on their order)
__device__ __forceinline__ double d_tree64(double v) {
#pragma unroll
  for (int o = ODET_WAVE / 2; o > 0; o >>= 1) v = v + __shfl_xor(v, o);
  return v;
}

// one workgroup per chunk
template <int KIND>
__global__ void __launch_bounds__(OPT_THREADS) k_opt_update(OptArgs a) {
  __shared__ double s_wave[OPT_WAVES];
  const odet_opt_chunk_t ck = a.chunks[blockIdx.x];
  if ((unsigned)ck.tensor >= (unsigned)a.num_tensors) return;
  const odet_opt_tensor_t tr = a.tensors[ck.tensor];
  const int64_t n = tr.numel, base = ck.offset;
  if (base < 0 || base >= n || base % ODET_OPT_CHUNK) return;
  const bool var_f16 = tr.flags & ODET_OPT_VAR_F16, grad_f16 = tr.flags & ODET_OPT_GRAD_F16;
  float* const w32 = var_f16 ? tr.master : (float*)tr.var;  // what the update and the L2 term use
  if (!w32) return;                                         // (a float16 variable without its master: not updated)
  const void* const grad = (KIND == OPT_L2_ONLY) ? nullptr : a.grads[ck.tensor];
  const float wd = tr.weight_decay;
  const bool update = KIND != OPT_L2_ONLY && grad && tr.slot0 && (KIND != OPT_ADAM || tr.slot1);
  const int64_t part = (int64_t)tr.first_chunk + base / ODET_OPT_CHUNK;
  const bool want_l2 = a.partials && wd != 0.0f && part >= 0 && part < a.num_chunks;
  if (!update && !want_l2) return;                          // (uniform over the workgroup: before the barrier)

  // alignment of everything this chunk touches (uniform): float32 arrays to 16 bytes, float16 arrays to 8
  uintptr_t bits = (uintptr_t)w32;
  if (var_f16 && update) bits |= (uintptr_t)tr.var * 2;
  if (update) {
    bits |= grad_f16 ? (uintptr_t)grad * 2 : (uintptr_t)grad;
    bits |= (uintptr_t)tr.slot0;
    if (KIND == OPT_ADAM) bits |= (uintptr_t)tr.slot1;
  }
  const bool vec = (bits & 15) == 0;

  // the schedule and the step's scalars, from the state block (read only here)
  float lr = 0.0f, alpha = 0.0f;
  if (update) {
    const int64_t step = a.state->global_step;
    int i = 0;
    for (int k = 0; k < a.num_boundaries; ++k) i += a.state->boundaries[k] < step ? 1 : 0;
    lr = a.state->values[i];
    if (KIND == OPT_ADAM) {
      const float b1p = a.state->beta1_power, b2p = a.state->beta2_power;
      alpha = lr * sqrtf(1.0f - b2p) / (1.0f - b1p);
    }
  }
  const float one_minus_b1 = 1.0f - a.beta1, one_minus_b2 = 1.0f - a.beta2;

  float w[OPT_GROUPS][4], g[OPT_GROUPS][4], s0[OPT_GROUPS][4], s1[OPT_GROUPS][4];
#pragma unroll
  for (int k = 0; k < OPT_GROUPS; ++k) {                    // every load of the chunk before its first store
    const int64_t j = base + (int64_t)(k * OPT_THREADS + threadIdx.x) * 4;
    d_ld4_f32(w32, j, n, vec, w[k]);
    if (update) {
      if (grad_f16) d_ld4_f16((const _Float16*)grad, j, n, vec, g[k]);
      else d_ld4_f32((const float*)grad, j, n, vec, g[k]);
      d_ld4_f32(tr.slot0, j, n, vec, s0[k]);
      if (KIND == OPT_ADAM) d_ld4_f32(tr.slot1, j, n, vec, s1[k]);
    }
  }

  double sum = 0.0;
#pragma unroll
  for (int k = 0; k < OPT_GROUPS; ++k) {
    const int64_t j = base + (int64_t)(k * OPT_THREADS + threadIdx.x) * 4;
    if (want_l2) {
#pragma unroll
      for (int e = 0; e < 4; ++e) sum += (double)(w[k][e] * w[k][e]);     // (elements past the end are 0: they add +0)
    }
    if (!update) continue;
    float nw[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float gr = g[k][e];
      if (wd != 0.0f) gr = gr + wd * (2.0f * w[k][e]);
      gr = gr * tr.grad_scale;
      if (KIND == OPT_MOMENTUM) {
        const float acc = s0[k][e] * a.momentum + gr;
        s0[k][e] = acc;
        nw[e] = w[k][e] - acc * lr;
      } else {
        const float m = s0[k][e] + (gr - s0[k][e]) * one_minus_b1;
        const float v = s1[k][e] + (gr * gr - s1[k][e]) * one_minus_b2;
        s0[k][e] = m;
        s1[k][e] = v;
        nw[e] = w[k][e] - (m * alpha) / (sqrtf(v) + a.epsilon);
      }
    }
    d_st4_f32(tr.slot0, j, n, vec, s0[k]);
    if (KIND == OPT_ADAM) d_st4_f32(tr.slot1, j, n, vec, s1[k]);
    d_st4_f32(w32, j, n, vec, nw);
    if (var_f16) d_st4_f16((_Float16*)tr.var, j, n, vec, nw);
  }

  if (want_l2) {                                            // (uniform)
    sum = d_tree64(sum);
    if ((threadIdx.x & (ODET_WAVE - 1)) == 0) s_wave[threadIdx.x / ODET_WAVE] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
      double acc = 0.0;
#pragma unroll
      for (int v = 0; v < OPT_WAVES; ++v) acc += s_wave[v];
      a.partials[part] = acc;
    }
  }
}

struct OptFinishArgs {
  const odet_opt_tensor_t* tensors; odet_opt_state_t* state; const double* partials;
  int num_tensors, num_chunks, advance, adam;
  float beta1, beta2;
  float* tensor_losses; float* total_loss;
};

// one workgroup: a wave per tensor for the L2 sums, thread 0 for add_n and the state.  Latency is all this launch costs, so the
// records are staged in LDS by all lanes at once and a lane fetches its partials eight at a time (added in order all the same).
#define OPT_FINISH_BATCH 8
__global__ void __launch_bounds__(OPT_FINISH_THREADS) k_opt_finish(OptFinishArgs a) {
  __shared__ float s_loss[ODET_OPT_MAX_TENSORS];
  __shared__ float s_wd[ODET_OPT_MAX_TENSORS];
  __shared__ int32_t s_first[ODET_OPT_MAX_TENSORS];
  __shared__ int32_t s_nc[ODET_OPT_MAX_TENSORS];
  const int wave = threadIdx.x / ODET_WAVE, lane = threadIdx.x % ODET_WAVE;
  if (a.partials) {
    for (int t = threadIdx.x; t < a.num_tensors; t += OPT_FINISH_THREADS) {
      const odet_opt_tensor_t* tr = a.tensors + t;
      const int64_t n = tr->numel;
      const int64_t nc = n > 0 ? (n + ODET_OPT_CHUNK - 1) / ODET_OPT_CHUNK : 0;
      s_wd[t] = tr->weight_decay;
      s_first[t] = tr->first_chunk;
      s_nc[t] = (int32_t)(nc < a.num_chunks ? nc : a.num_chunks);
    }
    __syncthreads();
    for (int t = wave; t < a.num_tensors; t += OPT_FINISH_WAVES) {
      const float wd = s_wd[t];
      float loss = 0.0f;
      if (wd != 0.0f) {                                     // (uniform over the wave)
        const int64_t first = s_first[t];
        const int nc = s_nc[t];
        double s = 0.0;
        for (int c0 = 0; c0 < nc; c0 += ODET_WAVE * OPT_FINISH_BATCH) {   // lane l: chunks l, l + 64, ... in ascending order
          double v[OPT_FINISH_BATCH];
#pragma unroll
          for (int u = 0; u < OPT_FINISH_BATCH; ++u) {
            const int c = c0 + u * ODET_WAVE + lane;
            const int64_t p = first + c;
            v[u] = (c < nc && p >= 0 && p < a.num_chunks) ? a.partials[p] : 0.0;   // (an absent chunk adds +0: the same bits)
          }
#pragma unroll
          for (int u = 0; u < OPT_FINISH_BATCH; ++u) s += v[u];
        }
        s = d_tree64(s);
        loss = wd * (float)s;
      }
      if (lane == 0) {
        s_loss[t] = loss;
        if (a.tensor_losses) a.tensor_losses[t] = loss;
      }
    }
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  if (a.partials && a.total_loss) {
    float total = 0.0f;
    for (int t = 0; t < a.num_tensors; ++t) total = total + s_loss[t];     // add_n: left to right in table order
    *a.total_loss = total;
  }
  if (a.advance) {
    a.state->global_step = a.state->global_step + 1;
    if (a.adam) {
      a.state->beta1_power = a.state->beta1_power * a.beta1;
      a.state->beta2_power = a.state->beta2_power * a.beta2;
    }
  }
}

static int opt_check(const char* who, const odet_opt_config_t* cfg, bool need_kind) {
  ODET_REQUIRE(cfg, "%s: null config", who);
  ODET_REQUIRE(cfg->num_tensors >= 0 && cfg->num_chunks >= 0 && cfg->num_boundaries >= 0, "%s: negative count", who);
  if (cfg->num_tensors > ODET_OPT_MAX_TENSORS)
    return odet_set_error(ODET_E_LIMIT, "%s: %d tensors exceed %d", who, cfg->num_tensors, ODET_OPT_MAX_TENSORS);
  if (cfg->num_chunks > ODET_OPT_MAX_CHUNKS)
    return odet_set_error(ODET_E_LIMIT, "%s: %d chunks exceed %d", who, cfg->num_chunks, ODET_OPT_MAX_CHUNKS);
  if (cfg->num_boundaries > ODET_OPT_MAX_BOUNDARIES)
    return odet_set_error(ODET_E_LIMIT, "%s: %d schedule boundaries exceed %d", who, cfg->num_boundaries, ODET_OPT_MAX_BOUNDARIES);
  if (need_kind) {
    ODET_REQUIRE(cfg->kind == ODET_OPT_MOMENTUM || cfg->kind == ODET_OPT_ADAM, "%s: unknown optimizer kind %d", who, cfg->kind);
    if (cfg->kind == ODET_OPT_ADAM)
      ODET_REQUIRE(cfg->beta1 >= 0.0f && cfg->beta1 < 1.0f && cfg->beta2 >= 0.0f && cfg->beta2 < 1.0f && cfg->epsilon >= 0.0f,
                   "%s: beta1, beta2 must lie in [0, 1) and epsilon must not be negative", who);
  }
  return ODET_OK;
}

extern "C" size_t odet_opt_partials_bytes(int num_chunks) {
  return sizeof(double) * (size_t)(num_chunks > 1 ? num_chunks : 1);
}

static int opt_run(const char* who, int kind, const odet_opt_config_t* cfg, const odet_opt_tensor_t* tensors,
                   const void* const* grads, const odet_opt_chunk_t* chunks, odet_opt_state_t* state, void* partials,
                   size_t partials_bytes, float* tensor_losses, float* total_loss, hipStream_t st) {
  const bool want_l2 = tensor_losses || total_loss;
  if (want_l2) {
    ODET_REQUIRE(partials, "%s: the L2 outputs need the partials buffer", who);
    ODET_REQUIRE((uintptr_t)partials % 8 == 0, "%s: the partials buffer must be 8-byte aligned", who);
    if (partials_bytes < odet_opt_partials_bytes(cfg->num_chunks))
      return odet_set_error(ODET_E_WORKSPACE, "%s: partials buffer of %zu bytes, %zu needed", who, partials_bytes,
                            odet_opt_partials_bytes(cfg->num_chunks));
  }
  OptArgs a;
  a.tensors = tensors; a.grads = grads; a.chunks = chunks; a.state = state;
  a.num_tensors = cfg->num_tensors; a.num_chunks = cfg->num_chunks; a.num_boundaries = cfg->num_boundaries;
  a.momentum = cfg->momentum; a.beta1 = cfg->beta1; a.beta2 = cfg->beta2; a.epsilon = cfg->epsilon;
  a.partials = want_l2 ? (double*)partials : nullptr;
  if (cfg->num_chunks > 0 && cfg->num_tensors > 0) {
    const dim3 grid((unsigned)cfg->num_chunks), block(OPT_THREADS);
    if (kind == OPT_MOMENTUM) hipLaunchKernelGGL(k_opt_update<OPT_MOMENTUM>, grid, block, 0, st, a);
    else if (kind == OPT_ADAM) hipLaunchKernelGGL(k_opt_update<OPT_ADAM>, grid, block, 0, st, a);
    else if (want_l2) hipLaunchKernelGGL(k_opt_update<OPT_L2_ONLY>, grid, block, 0, st, a);
    ODET_LAUNCH_CHECK();
  }
  OptFinishArgs f;
  f.tensors = tensors; f.state = state; f.partials = a.partials;
  f.num_tensors = cfg->num_tensors; f.num_chunks = cfg->num_chunks;
  f.advance = kind != OPT_L2_ONLY; f.adam = kind == OPT_ADAM;
  f.beta1 = cfg->beta1; f.beta2 = cfg->beta2;
  f.tensor_losses = tensor_losses; f.total_loss = total_loss;
  if (f.advance || want_l2) {
    hipLaunchKernelGGL(k_opt_finish, dim3(1), dim3(OPT_FINISH_THREADS), 0, st, f);   // (after the update: stream order)
    ODET_LAUNCH_CHECK();
  }
  return ODET_OK;
}

extern "C" int odet_opt_step(const odet_opt_config_t* cfg, const odet_opt_tensor_t* tensors, const void* const* grads,
                             const odet_opt_chunk_t* chunks, odet_opt_state_t* state, void* partials, size_t partials_bytes,
                             float* tensor_losses, float* total_loss, odet_stream_t stream) {
  const int rc = opt_check("odet_opt_step", cfg, true);
  if (rc != ODET_OK) return rc;
  ODET_REQUIRE(state, "odet_opt_step: null pointer (state)");
  ODET_REQUIRE(cfg->num_tensors == 0 || (tensors && grads), "odet_opt_step: null pointer (tensor table / gradient column)");
  ODET_REQUIRE(cfg->num_chunks == 0 || chunks, "odet_opt_step: null pointer (chunk table)");
  return opt_run("odet_opt_step", cfg->kind, cfg, tensors, grads, chunks, state, partials, partials_bytes, tensor_losses,
                 total_loss, (hipStream_t)stream);
}

extern "C" int odet_l2_loss(const odet_opt_config_t* cfg, const odet_opt_tensor_t* tensors, const odet_opt_chunk_t* chunks,
                            void* partials, size_t partials_bytes, float* tensor_losses, float* total_loss,
                            odet_stream_t stream) {
  const int rc = opt_check("odet_l2_loss", cfg, false);
  if (rc != ODET_OK) return rc;
  ODET_REQUIRE(cfg->num_tensors == 0 || tensors, "odet_l2_loss: null pointer (tensor table)");
  ODET_REQUIRE(cfg->num_chunks == 0 || chunks, "odet_l2_loss: null pointer (chunk table)");
  ODET_REQUIRE(tensor_losses || total_loss, "odet_l2_loss: null pointer (no output)");
  return opt_run("odet_l2_loss", OPT_L2_ONLY, cfg, tensors, nullptr, chunks, nullptr, partials, partials_bytes, tensor_losses,
                 total_loss, (hipStream_t)stream);
}
