// The one opt-in to more than 64 KiB of dynamic LDS.  The attribute belongs to a kernel ON A DEVICE, so the high-water mark is per
// device; the first call per (kernel, device) must come outside a stream capture (warm-up steps do).  The template parameter is the
// kernel pointer itself: two instantiations of one kernel template have the same type and must not share a slot.  No lock: the
// library is process-wide, not thread-safe (include/orcai_hip.h).
#pragma once
#include <hip/hip_runtime.h>

namespace orcai_lds {
constexpr int MAXDEV = 64;
template <auto Kernel>
hipError_t ensure_dynamic_lds(size_t bytes) {
  static size_t granted[MAXDEV] = {};
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e == hipSuccess && (dev < 0 || dev >= MAXDEV)) e = hipErrorInvalidDevice;
  if (e != hipSuccess || bytes <= granted[dev]) return e;
  e = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess) granted[dev] = bytes;
  return e;
}
}  // namespace orcai_lds
