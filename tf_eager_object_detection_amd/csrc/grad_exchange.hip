// The arithmetic and the byte moves of the data-parallel gradient exchange (parallel.GradientExchange): a whole gradient list
// packed into one contiguous float32 bucket in ONE launch, its inverse, and the sum over the ranks' parts in ASCENDING RANK
// order.  The collectives around them (all_to_all_single, all_gather_into_tensor) only move bytes, so the exchanged gradient is
// a function of the data alone: tests/grad_exchange_np.py restates all three bit for bit.  No allocation, no host read, no
// atomics; every output element is written exactly once by one lane.  odet_bucket_accumulate_f32 adds one image's gradient list
// into such a bucket (training.GradientAccumulator, tests/grad_accumulate_np.py): the K-image step in one launch per image.
//
// Layout (include/odet.h "gradient exchange"): the optimizer's chunk table (odet_opt_chunk_t, ODET_OPT_CHUNK elements) built over
// the PRESENT tensors, so chunk c of the table is chunk c of the bucket; the chunks past the table pad the bucket to a whole
// number of shards and hold +0.0f.
//
// Bandwidth bound (appendix "element-wise" of the kernel guide): a lane moves 16 bytes per load / store, every load of a
// workgroup's share is issued before its first store.
#include "odet_internal.h"

#define GX_THREADS 256
#define GX_GROUPS (ODET_OPT_CHUNK / (GX_THREADS * 4))       // groups of 4 elements per lane and chunk: 4
#define GX_RM_GROUPS 2                                      // rank_mean: groups of 4 elements per lane
#define GX_RM_BATCH 8                                       // rank_mean: ranks loaded before their adds
#define GX_RM_BLOCK ((int64_t)GX_THREADS * 4 * GX_RM_GROUPS)

static_assert(GX_GROUPS * GX_THREADS * 4 == ODET_OPT_CHUNK, "a chunk is a whole number of groups per lane");
static_assert(sizeof(odet_opt_chunk_t) == 16, "the chunk record is part of the ABI");

struct BucketArgs {
  const void* const* tensors; const int64_t* numels; const odet_opt_chunk_t* chunks; float* bucket;
  int num_tensors, num_chunks;
};

// one workgroup per bucket chunk.  PACK: tensor -> bucket (the chunk's tail and the padding chunks are written as +0.0f);
// else bucket -> tensor (only the tensor's own elements are written).
template <bool PACK>
__global__ void __launch_bounds__(GX_THREADS) k_bucket_move(BucketArgs a) {
  const int64_t c = blockIdx.x;
  float* const slot = a.bucket + c * ODET_OPT_CHUNK;        // (16-byte aligned: the host checked the bucket)
  float* t = nullptr;
  int64_t n = 0, base = 0;
  if (c < a.num_chunks) {
    const odet_opt_chunk_t ck = a.chunks[c];
    if ((unsigned)ck.tensor < (unsigned)a.num_tensors) {
      t = (float*)a.tensors[ck.tensor];
      n = a.numels[ck.tensor];
      base = ck.offset;
      if (base < 0 || base >= n || base % ODET_OPT_CHUNK) t = nullptr;     // (a record that does not fit: skipped)
    }
  }
  if (!PACK && !t) return;                                  // (uniform over the workgroup)
  const bool vec = t && ((uintptr_t)t & 15) == 0;           // (base is a multiple of the chunk: t + base is aligned with t)

  float v[GX_GROUPS][4];
#pragma unroll
  for (int k = 0; k < GX_GROUPS; ++k) {                     // every load before the first store
    const int e0 = (k * GX_THREADS + (int)threadIdx.x) * 4;
    if (PACK) {
      const int64_t j = base + e0;
      if (vec && j + 4 <= n) {
        const float4 q = *reinterpret_cast<const float4*>(t + j);
        v[k][0] = q.x; v[k][1] = q.y; v[k][2] = q.z; v[k][3] = q.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[k][e] = (t && j + e < n) ? t[j + e] : 0.0f;
      }
    } else {
      const float4 q = *reinterpret_cast<const float4*>(slot + e0);
      v[k][0] = q.x; v[k][1] = q.y; v[k][2] = q.z; v[k][3] = q.w;
    }
  }
#pragma unroll
  for (int k = 0; k < GX_GROUPS; ++k) {
    const int e0 = (k * GX_THREADS + (int)threadIdx.x) * 4;
    if (PACK) {
      *reinterpret_cast<float4*>(slot + e0) = make_float4(v[k][0], v[k][1], v[k][2], v[k][3]);
    } else {
      const int64_t j = base + e0;
      if (vec && j + 4 <= n) {
        *reinterpret_cast<float4*>(t + j) = make_float4(v[k][0], v[k][1], v[k][2], v[k][3]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (j + e < n) t[j + e] = v[k][e];
      }
    }
  }
}

// One image of a K-image window (training.GradientAccumulator): one workgroup per bucket chunk, shaped as k_bucket_move<true> is (a
// sibling: pack and unpack keep their machine code).  FIRST: bucket = g, and every element of the bucket is written as pack
// writes it (+0.0f in the tails, in absent records and in the padding chunks); else bucket = bucket + g, ONE float32 add, over
// the present tensors' own elements and nothing else.  DIVIDE: the sum then goes through one IEEE division by `divisor`.
// Per element 8 bytes are read and 4 written (FIRST: 4 and 4); both operands of a lane's share are loaded before its first store.
//
// WHOLE (uniform over the workgroup): the chunk lies inside its tensor and the tensor is 16-byte aligned -- 16-byte accesses on
// both sides and no bound in the code.  Every other chunk (a tensor's last one, a shifted tensor, an absent record) goes element
// by element under its bound, with the same bits.  Two bodies under a uniform branch, not one body with a per-group test: the
// compiler folds a per-group "whole group, else by element" into the by-element form and the 16-byte stores are gone.
template <bool FIRST, bool DIVIDE, bool WHOLE>
__device__ __forceinline__ void bucket_accumulate_chunk(float* __restrict__ slot, const float* __restrict__ t, int64_t base, int64_t n,
                                                        float divisor) {
  float g[GX_GROUPS][4], b[GX_GROUPS][4];
#pragma unroll
  for (int k = 0; k < GX_GROUPS; ++k) {                     // every load before the first store
    const int e0 = (k * GX_THREADS + (int)threadIdx.x) * 4;
    const int64_t j = base + e0;
    if (WHOLE) {
      const float4 q = *reinterpret_cast<const float4*>(t + j);
      g[k][0] = q.x; g[k][1] = q.y; g[k][2] = q.z; g[k][3] = q.w;
      if (!FIRST) {
        const float4 r = *reinterpret_cast<const float4*>(slot + e0);
        b[k][0] = r.x; b[k][1] = r.y; b[k][2] = r.z; b[k][3] = r.w;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool in = t && j + e < n;
        g[k][e] = in ? t[j + e] : 0.0f;
        if (!FIRST) b[k][e] = in ? slot[e0 + e] : 0.0f;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < GX_GROUPS; ++k) {
    const int e0 = (k * GX_THREADS + (int)threadIdx.x) * 4;
    const int64_t j = base + e0;
    float s[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      s[e] = FIRST ? g[k][e] : b[k][e] + g[k][e];           // one float32 add per image
      if (DIVIDE) s[e] = s[e] / divisor;                    // IEEE division, correctly rounded (+0.0f stays +0.0f: divisor > 0)
    }
    if (FIRST || WHOLE) {
      *reinterpret_cast<float4*>(slot + e0) = make_float4(s[0], s[1], s[2], s[3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (j + e < n) slot[e0 + e] = s[e];
    }
  }
}

template <bool FIRST, bool DIVIDE>
__global__ void __launch_bounds__(GX_THREADS) k_bucket_accumulate(BucketArgs a, float divisor) {
  const int64_t c = blockIdx.x;
  float* const slot = a.bucket + c * ODET_OPT_CHUNK;        // (16-byte aligned: the host checked the bucket)
  const float* t = nullptr;
  int64_t n = 0, base = 0;
  if (c < a.num_chunks) {
    const odet_opt_chunk_t ck = a.chunks[c];
    if ((unsigned)ck.tensor < (unsigned)a.num_tensors) {
      t = (const float*)a.tensors[ck.tensor];
      n = a.numels[ck.tensor];
      base = ck.offset;
      if (base < 0 || base >= n || base % ODET_OPT_CHUNK) t = nullptr;     // (a record that does not fit: absent)
    }
  }
  if (!FIRST && !t) return;                                 // (uniform over the workgroup)
  // (base is a multiple of the chunk: t + base is aligned with t)
  if (t && ((uintptr_t)t & 15) == 0 && base + ODET_OPT_CHUNK <= n) bucket_accumulate_chunk<FIRST, DIVIDE, true>(slot, t, base, n, divisor);
  else bucket_accumulate_chunk<FIRST, DIVIDE, false>(slot, t, base, n, divisor);
}

// out[i] = ((parts[0][i] + parts[1][i]) + ...) + parts[world - 1][i], then / float32(world) with `average`.  A lane owns
// GX_RM_GROUPS groups of four consecutive elements; the rows of GX_RM_BATCH ranks are loaded before they are added, in rank order.
__global__ void __launch_bounds__(GX_THREADS) k_rank_mean(const float* __restrict__ parts, int world, int64_t n, int average,
                                                          float* __restrict__ out) {
  const int64_t j0 = (int64_t)blockIdx.x * GX_RM_BLOCK + (int64_t)threadIdx.x * 4;
  const bool out_vec = ((uintptr_t)out & 15) == 0;
  float s[GX_RM_GROUPS][4];
  for (int r0 = 0; r0 < world; r0 += GX_RM_BATCH) {
    float p[GX_RM_BATCH][GX_RM_GROUPS][4];
#pragma unroll
    for (int u = 0; u < GX_RM_BATCH; ++u) {
      const int r = r0 + u;
      if (r >= world) break;                                // (uniform)
      const float* row = parts + (int64_t)r * n;
      const bool vec = ((uintptr_t)row & 15) == 0;          // (uniform: a row whose start is not 16-byte aligned goes by element)
#pragma unroll
      for (int k = 0; k < GX_RM_GROUPS; ++k) {
        const int64_t j = j0 + (int64_t)k * GX_THREADS * 4;
        if (vec && j + 4 <= n) {
          const float4 q = *reinterpret_cast<const float4*>(row + j);
          p[u][k][0] = q.x; p[u][k][1] = q.y; p[u][k][2] = q.z; p[u][k][3] = q.w;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) p[u][k][e] = (j + e < n) ? row[j + e] : 0.0f;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < GX_RM_BATCH; ++u) {
      const int r = r0 + u;
      if (r >= world) break;
#pragma unroll
      for (int k = 0; k < GX_RM_GROUPS; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) s[k][e] = (r == 0) ? p[u][k][e] : s[k][e] + p[u][k][e];   // one float32 add per rank
    }
  }
  const float w = (float)world;
#pragma unroll
  for (int k = 0; k < GX_RM_GROUPS; ++k) {
    const int64_t j = j0 + (int64_t)k * GX_THREADS * 4;
    if (average) {
#pragma unroll
      for (int e = 0; e < 4; ++e) s[k][e] = s[k][e] / w;    // IEEE division, correctly rounded: not a reciprocal multiply
    }
    if (out_vec && j + 4 <= n) {
      *reinterpret_cast<float4*>(out + j) = make_float4(s[k][0], s[k][1], s[k][2], s[k][3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (j + e < n) out[j + e] = s[k][e];
    }
  }
}

static int bucket_check(const char* who, const void* tensors, const void* numels, int num_tensors, const void* chunks, int num_chunks,
                        const void* bucket, int64_t bucket_chunks) {
  ODET_REQUIRE(num_tensors >= 0 && num_chunks >= 0 && bucket_chunks >= 0, "%s: negative count", who);
  if (num_tensors > ODET_OPT_MAX_TENSORS)
    return odet_set_error(ODET_E_LIMIT, "%s: %d tensors exceed %d", who, num_tensors, ODET_OPT_MAX_TENSORS);
  if (num_chunks > ODET_OPT_MAX_CHUNKS || bucket_chunks > ODET_OPT_MAX_CHUNKS)
    return odet_set_error(ODET_E_LIMIT, "%s: %lld chunks exceed %d", who,
                          (long long)(bucket_chunks > num_chunks ? bucket_chunks : num_chunks), ODET_OPT_MAX_CHUNKS);
  ODET_REQUIRE(num_chunks <= bucket_chunks, "%s: %d chunks do not fit a bucket of %lld", who, num_chunks, (long long)bucket_chunks);
  ODET_REQUIRE(num_tensors == 0 || (tensors && numels), "%s: null pointer (pointer column / numels)", who);
  ODET_REQUIRE(num_chunks == 0 || (chunks && num_tensors > 0), "%s: null pointer (chunk table)", who);
  ODET_REQUIRE(bucket_chunks == 0 || bucket, "%s: null pointer (bucket)", who);
  ODET_REQUIRE((uintptr_t)bucket % 16 == 0, "%s: the bucket must be 16-byte aligned", who);
  return ODET_OK;
}

extern "C" int odet_bucket_pack_f32(const void* const* tensors, const int64_t* numels, int num_tensors,
                                    const odet_opt_chunk_t* chunks, int num_chunks, float* bucket, int64_t bucket_chunks,
                                    odet_stream_t stream) {
  const int rc = bucket_check("odet_bucket_pack_f32", tensors, numels, num_tensors, chunks, num_chunks, bucket, bucket_chunks);
  if (rc != ODET_OK) return rc;
  if (bucket_chunks == 0) return ODET_OK;
  BucketArgs a;
  a.tensors = tensors; a.numels = numels; a.chunks = chunks; a.bucket = bucket;
  a.num_tensors = num_tensors; a.num_chunks = num_chunks;
  hipLaunchKernelGGL(k_bucket_move<true>, dim3((unsigned)bucket_chunks), dim3(GX_THREADS), 0, (hipStream_t)stream, a);
  ODET_LAUNCH_CHECK();
  return ODET_OK;
}

extern "C" int odet_bucket_unpack_f32(const float* bucket, int64_t bucket_chunks, void* const* tensors, const int64_t* numels,
                                      int num_tensors, const odet_opt_chunk_t* chunks, int num_chunks, odet_stream_t stream) {
  const int rc = bucket_check("odet_bucket_unpack_f32", tensors, numels, num_tensors, chunks, num_chunks, bucket, bucket_chunks);
  if (rc != ODET_OK) return rc;
  if (num_chunks == 0) return ODET_OK;
  BucketArgs a;
  a.tensors = (const void* const*)tensors; a.numels = numels; a.chunks = chunks; a.bucket = const_cast<float*>(bucket);
  a.num_tensors = num_tensors; a.num_chunks = num_chunks;
  hipLaunchKernelGGL(k_bucket_move<false>, dim3((unsigned)num_chunks), dim3(GX_THREADS), 0, (hipStream_t)stream, a);
  ODET_LAUNCH_CHECK();
  return ODET_OK;
}

extern "C" int odet_bucket_accumulate_f32(const void* const* tensors, const int64_t* numels, int num_tensors,
                                          const odet_opt_chunk_t* chunks, int num_chunks, float* bucket, int64_t bucket_chunks,
                                          int first, float divisor, odet_stream_t stream) {
  const int rc = bucket_check("odet_bucket_accumulate_f32", tensors, numels, num_tensors, chunks, num_chunks, bucket, bucket_chunks);
  if (rc != ODET_OK) return rc;
  ODET_REQUIRE(first == 0 || first == 1, "odet_bucket_accumulate_f32: first must be 0 or 1, got %d", first);
  ODET_REQUIRE(divisor > 0.0f && divisor <= 3.402823466e38f, "odet_bucket_accumulate_f32: the divisor must be finite and > 0");
  const int64_t blocks = first ? bucket_chunks : num_chunks;            // (a later image touches the table's chunks only)
  if (blocks == 0) return ODET_OK;
  BucketArgs a;
  a.tensors = tensors; a.numels = numels; a.chunks = chunks; a.bucket = bucket;
  a.num_tensors = num_tensors; a.num_chunks = num_chunks;
  const dim3 grid((unsigned)blocks), block(GX_THREADS);
  const hipStream_t st = (hipStream_t)stream;
  if (divisor == 1.0f) {
    if (first) hipLaunchKernelGGL((k_bucket_accumulate<true, false>), grid, block, 0, st, a, divisor);
    else hipLaunchKernelGGL((k_bucket_accumulate<false, false>), grid, block, 0, st, a, divisor);
  } else {
    if (first) hipLaunchKernelGGL((k_bucket_accumulate<true, true>), grid, block, 0, st, a, divisor);
    else hipLaunchKernelGGL((k_bucket_accumulate<false, true>), grid, block, 0, st, a, divisor);
  }
  ODET_LAUNCH_CHECK();
  return ODET_OK;
}

extern "C" int odet_rank_mean_f32(const float* parts, int world, int64_t n, int average, float* out, odet_stream_t stream) {
  ODET_REQUIRE(world >= 1, "odet_rank_mean_f32: world must be at least 1, got %d", world);
  if (world > ODET_RANK_MEAN_MAX_WORLD)
    return odet_set_error(ODET_E_LIMIT, "odet_rank_mean_f32: world %d exceeds %d", world, ODET_RANK_MEAN_MAX_WORLD);
  ODET_REQUIRE(n >= 0, "odet_rank_mean_f32: negative size");
  if (n > (int64_t)ODET_OPT_MAX_CHUNKS * ODET_OPT_CHUNK)
    return odet_set_error(ODET_E_LIMIT, "odet_rank_mean_f32: %lld elements exceed %lld", (long long)n,
                          (long long)ODET_OPT_MAX_CHUNKS * ODET_OPT_CHUNK);
  ODET_REQUIRE(average == 0 || average == 1, "odet_rank_mean_f32: average must be 0 or 1, got %d", average);
  if (n == 0) return ODET_OK;
  ODET_REQUIRE(parts && out, "odet_rank_mean_f32: null pointer");
  ODET_REQUIRE((uintptr_t)parts % 4 == 0 && (uintptr_t)out % 4 == 0, "odet_rank_mean_f32: pointers must be 4-byte aligned");
  const int64_t blocks = (n + GX_RM_BLOCK - 1) / GX_RM_BLOCK;     // (at most 2^25: the grid follows n alone)
  hipLaunchKernelGGL(k_rank_mean, dim3((unsigned)blocks), dim3(GX_THREADS), 0, (hipStream_t)stream, parts, world, n, average, out);
  ODET_LAUNCH_CHECK();
  return ODET_OK;
}
