// select_key.h -- the monotone key every exact select of this library orders f32 values by (frontend.hip, column_select.hip).
// key order == float order for every non-NaN float, with -0.0 before +0.0 and +-inf ordinary values; key2f(f2key(f)) gives f's bits back.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

__device__ __forceinline__ uint32_t f2key(float f) {
  uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k) {
  uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  return __uint_as_float(u);
}
