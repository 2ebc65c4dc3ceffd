// Device helpers shared by the elementwise, quantize and fused-quantize
// kernels.  One definition each: the fused kernels in fp8_fused.hip must
// produce the bytes of bias_gelu.hip / layernorm.hip followed by
// fp8_quant.hip, so they evaluate the very same inline functions.
#pragma once

#include "common.h"

// tanh-GeLU via the sigmoid identity: 0.5x(1+tanh(z)) == x*sigmoid(2z),
// evaluated with ONE hardware __expf instead of libm tanhf (the tanh
// path ran the elementwise kernels 1.7-1.9x off the HBM roofline —
// VALU-bound on the polynomial tanh expansion).  Same function, only
// the evaluation differs; bf16 outputs agree to rounding.
__device__ __forceinline__ float gelu_sigmoid(float x) {
  const float k2 = 2.0f * 0.7978845608028654f;
  float z2 = k2 * (x + 0.044715f * x * x * x);
  return 1.0f / (1.0f + __expf(-z2));
}

__device__ __forceinline__ float gelu_f(float x) {
  return x * gelu_sigmoid(x);
}

// e4m3: clamp 448; e5m2 (ISA name bf8): clamp 57344. RNE conversion via
// the packed hardware converters.
template <bool E5M2>
__device__ __forceinline__ unsigned short cvt2_fp8(float a, float b) {
  a = __builtin_amdgcn_fmed3f(a, E5M2 ? 57344.f : 448.f,
                              E5M2 ? -57344.f : -448.f);
  b = __builtin_amdgcn_fmed3f(b, E5M2 ? 57344.f : 448.f,
                              E5M2 ? -57344.f : -448.f);
  unsigned int packed =
      E5M2 ? __builtin_amdgcn_cvt_pk_bf8_f32(a, b, 0, false)
           : __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
  return (unsigned short)(packed & 0xffff);
}

__device__ __forceinline__ void atomic_max_f32(float* addr, float v) {
  // positive floats compare correctly as uints.  Guard with a plain
  // read first: with ~80k blocks all reducing into ONE scalar, the
  // serialized same-address atomics would otherwise dominate; after
  // the first few blocks the running max is usually already >= v and
  // the atomic is skipped (monotonic, so the race is benign).
  volatile unsigned int* a = reinterpret_cast<volatile unsigned int*>(addr);
  if (__float_as_uint(v) > *a)
    atomicMax(reinterpret_cast<unsigned int*>(addr), __float_as_uint(v));
}

typedef unsigned char u8x8 __attribute__((ext_vector_type(8)));
typedef unsigned char u8x16 __attribute__((ext_vector_type(16)));
