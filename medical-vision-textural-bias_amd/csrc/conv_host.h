// conv_host.h -- host helpers the conv launchers share: the z-segment search and the LDS-attribute launch.
#pragma once

#include <hip/hip_runtime.h>

#include "num_cu.h"
#include "texbias.h"

namespace tb {

// z segment length of a z-marching launch: `base` blocks per z segment, `per_cu` blocks resident per CU; the
// launch takes ceil(blocks / (CUs x per_cu)) rounds of len + fill plane steps (`fill` ring-fill planes per
// segment).  Candidates are D and every length from D - 1 down to min_len; of equal costs the longest wins.
inline int zseg(int D, int base, int per_cu, int fill, int min_len = 1) {
  const int slots = per_cu * num_cu();
  int best = 1 << 30, zl = D;
  for (int l = D; l >= 1 && (l == D || l >= min_len); --l) {
    const int zs = (D + l - 1) / l, rounds = (base * zs + slots - 1) / slots, cost = rounds * (l + fill);
    if (cost < best) best = cost, zl = l;
  }
  return zl;
}

// Launch a kernel that carves up to 160 KiB of dynamic LDS.  The attribute belongs to the kernel on the
// current device, so it is set with every launch (no cache to go stale on another device).
template <class Args>
int launch_lds(void (*kern)(Args), dim3 grid, dim3 block, size_t lds, hipStream_t st, const Args& a) {
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 163840) !=
      hipSuccess)
    return TB_ERR_HIP;
  hipLaunchKernelGGL(kern, grid, block, lds, st, a);
  return hipGetLastError() == hipSuccess ? TB_OK : TB_ERR_HIP;
}

}  // namespace tb
