// What the elementwise backward launches share (block_grad.hip, vgg_grad.hip, neck.hip's merge and its backward): HBM-bound
// streams in ONE layout -- a lane owns 16 bytes, a pixel's lanes are consecutive, workgroups of 256 walk the elements grid-stride.
// Written once, here: the load that reads an operand once, the grid rule, the argument rules every entry point opens with.
#ifndef ODET_GRAD_ELEMENTWISE_H_
#define ODET_GRAD_ELEMENTWISE_H_
#include <algorithm>

#include "odet_internal.h"

typedef uint32_t ge_u4 __attribute__((ext_vector_type(4)));   // 16 B, the type the non-temporal builtins take

#ifdef __HIPCC__
// 16 bytes of an operand that is read once (non-temporal)
static __device__ __forceinline__ float4 ge_stream(const float4* p) {
  const ge_u4 t = __builtin_nontemporal_load(reinterpret_cast<const ge_u4*>(p));
  float4 r;
  __builtin_memcpy(&r, &t, 16);
  return r;
}
#endif  // __HIPCC__

// workgroups of 256 for `total` lanes: grid-stride beyond 64 workgroups per CU
static inline int ge_grid(long long total) { return (int)std::min<long long>((total + 255) / 256, 256 * 64); }

// an NHWC float32 map [B,H,W,C], C in whole lanes; `pointers`: the operands' addresses or-ed together (a null one adds nothing)
#define GE_REQUIRE_NHWC(who, B, H, W, C, pointers)                                                              \
  do {                                                                                                          \
    ODET_REQUIRE((H) > 0 && (W) > 0 && (B) >= 0, "%s: bad sizes (B %d, H %d, W %d)", who, B, H, W);           \
    ODET_REQUIRE((C) > 0 && (C) % 4 == 0, "%s: C must be a positive multiple of 4 (got %d)", who, C);          \
    ODET_REQUIRE((pointers) % 16 == 0, "%s: pointers must be 16-byte aligned", who);                           \
  } while (0)

#endif  // ODET_GRAD_ELEMENTWISE_H_
