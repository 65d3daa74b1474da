// num_cu.h -- the compute-unit count the conv planners size their grids and reduction splits by.
#pragma once

#include <hip/hip_runtime.h>

namespace tb {

// Of the device current at the first call; 256 if the query fails.  One cache for the whole library.
inline int num_cu() {
  static const int n = [] {
    int dev = 0, c = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c < 1)
      c = 256;
    return c;
  }();
  return n;
}

}  // namespace tb
