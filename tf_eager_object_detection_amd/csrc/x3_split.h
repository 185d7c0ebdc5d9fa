// The split of a float32 operand into three bfloat16 limbs, the ONE statement of it that the split-precision kernels share
// (conv_x3.hip: the forward convolutions; grad_gemm.h: dg_tile_x3, the gradient GEMMs):
//
//        a = a1 + a2 + a3,   a1 = bf16(a),  a2 = bf16(a - a1),  a3 = bf16(a - a1 - a2)        (round to nearest even; 3 x 8 = 24 bits)
#ifndef ODET_X3_SPLIT_H_
#define ODET_X3_SPLIT_H_
#include <hip/hip_runtime.h>

#ifdef __HIPCC__
typedef __bf16 x3b8 __attribute__((ext_vector_type(8)));
typedef __bf16 x3b2 __attribute__((ext_vector_type(2)));
typedef float x3f2 __attribute__((ext_vector_type(2)));

// two float32 -> their three bfloat16 limbs, packed (low half = first value)
__device__ __forceinline__ void x3_split2(const x3f2 a, unsigned& h, unsigned& m, unsigned& l) {
  const x3b2 hb = __builtin_convertvector(a, x3b2);
  h = __builtin_bit_cast(unsigned, hb);
  const x3f2 hf = {__builtin_bit_cast(float, h << 16), __builtin_bit_cast(float, h & 0xFFFF0000u)};
  const x3f2 r1 = a - hf;                                 // exact (the difference has at most 16 significant bits)
  const x3b2 mb = __builtin_convertvector(r1, x3b2);
  m = __builtin_bit_cast(unsigned, mb);
  const x3f2 mf = {__builtin_bit_cast(float, m << 16), __builtin_bit_cast(float, m & 0xFFFF0000u)};
  const x3f2 r2 = r1 - mf;                                // exact (at most 8 significant bits are left)
  const x3b2 lb = __builtin_convertvector(r2, x3b2);
  l = __builtin_bit_cast(unsigned, lb);
}
#endif  // __HIPCC__

#endif  // ODET_X3_SPLIT_H_
