// gemm_core.h -- the tile pipeline shared by the matrix-core conv GEMMs (conv_gemm.hip: forward and
// input gradient; conv_wgrad_gemm.hip: weight gradient).
//
// A 256-thread block computes a BM x BP tile of C = A B^T over stages of KC = 32 reduction elements.  A
// stage lives in LDS as BM rows of A then BP rows of B, each [32 k + 4 pad] floats, k in natural order.
// The four waves (WGM x 4 / WGM) own TM x TN sub-tiles of 32 x 32 on mfma_f32_32x32x2f32 (exact f32: one
// rounding per product, as a k-ordered fmaf chain); each lane reads its 16 operands of a stage as four
// 16-B LDS reads.  Stages are double-buffered in LDS and in two register slots: while stage s runs from
// LDS buffer s & 1, the global loads of stage s + 2 are in flight in slot s & 1 and stage s + 1 (loaded a
// stage earlier) is written to the other buffer; one barrier per stage.  A kernel supplies the block
// decode, the stagers (load / store below) and the epilogue's store.
//
// What the kernels rely on:
//   * load is called for stages at and past nst (the loop issues s + 2 unconditionally, with no branch
//     round it): a stager masks itself and reads zeros through its buffer descriptor's range check
//     (offset 0x80000000).
//   * nst == 0 is a real case (conv_gemm.hip: the k slices of a sub-pixel class past its K): the block
//     loads nothing, still reaches the barrier, and its epilogue stores zeros.
//   * The MFMA order along the reduction is fixed -- within a stage step st pairs element st (lanes 0-31)
//     with element 16 + st (lanes 32-63), half 0 then half 1, stages in order -- so results are
//     bit-reproducible across changes of everything else.
//   * Slot and buffer indices are compile-time (Idx<0> / Idx<1>): the stagers' register slots stay in
//     registers; a runtime index would send them to scratch.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>
#include <type_traits>

namespace tb {
namespace gemm {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int KC = 32;    // reduction elements per stage
constexpr int NTH = 256;  // threads per block
constexpr int RS = 36;    // LDS floats per tile row: 32 k + 4 pad (16-B reads of 16 rows hit distinct banks)

template <int I>
using Idx = std::integral_constant<int, I>;

__device__ __forceinline__ int xcd_remap(int b, int nb) {
  // hardware dispatch sends block b to XCD b % 8: give XCD x the contiguous logical range of blocks
  const int q = nb >> 3, r = nb & 7, x = b & 7, i = b >> 3;
  return x < r ? x * (q + 1) + i : r * (q + 1) + (x - r) * q + i;
}

template <int BM, int BP, int WGM>
struct Tile {
  static constexpr int WGN = 4 / WGM;
  static constexpr int TM = BM / WGM / 32, TN = BP / WGN / 32;
  static constexpr int LBUF = (BM + BP) * RS;  // floats per stage buffer
  static_assert(TM >= 1 && TN >= 1, "tile");

  f32x16 acc[TM][TN];
  int wm, wn, kk, l32;

  __device__ __forceinline__ Tile(int w, int lane) : wm(w % WGM), wn(w / WGM), kk(lane >> 5), l32(lane & 31) {
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
      for (int tn = 0; tn < TN; ++tn)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.f;
  }

  // MFMA steps 8 h .. 8 h + 7 of the stage in LDS buffer sl
  template <int sl, int h>
  __device__ __forceinline__ void half(const float* lds) {
    const float* L = lds + sl * LBUF;
    f32x4 af[TM][2], bf[TN][2];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
      const float* src = L + ((wm * TM + tm) * 32 + l32) * RS + 16 * kk + 8 * h;
#pragma unroll
      for (int q = 0; q < 2; ++q) af[tm][q] = *reinterpret_cast<const f32x4*>(src + 4 * q);
    }
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
      const float* src = L + (BM + (wn * TN + tn) * 32 + l32) * RS + 16 * kk + 8 * h;
#pragma unroll
      for (int q = 0; q < 2; ++q) bf[tn][q] = *reinterpret_cast<const f32x4*>(src + 4 * q);
    }
#pragma unroll
    for (int st = 0; st < 8; ++st)
#pragma unroll
      for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
          acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[tm][st >> 2][st & 3], bf[tn][st >> 2][st & 3],
                                                             acc[tm][tn], 0, 0, 0);
  }

  // The nst stages of the block.  load(Idx<slot>, s) issues the global loads of stage s into register slot
  // `slot`; store(Idx<slot>) writes that slot to LDS buffer `slot` (stage s uses slot and buffer s & 1).
  template <class Load, class Store>
  __device__ __forceinline__ void run(const float* lds, int nst, Load&& load, Store&& store) {
    if (nst > 0) {
      load(Idx<0>{}, 0);
      store(Idx<0>{});
      load(Idx<1>{}, 1);
    }
    __syncthreads();
    for (int s = 0; s < nst; s += 2) {
      stage<0>(lds, s, load, store);
      if (s + 1 < nst) stage<1>(lds, s + 1, load, store);
    }
  }

  // stage s (slot and buffer sl): its first 8 MFMA steps, then the loads of stage s + 2, the last 8 steps,
  // stage s + 1 to the other LDS buffer
  template <int sl, class Load, class Store>
  __device__ __forceinline__ void stage(const float* lds, int s, Load& load, Store& store) {
    half<sl, 0>(lds);
    load(Idx<sl>{}, s + 2);
    half<sl, 1>(lds);
    store(Idx<1 - sl>{});
    __syncthreads();
  }

  // The lane's accumulators: column (lane & 31) of each 32 x 32 sub-tile, rows (r & 3) + 8 (r >> 2) +
  // 4 (lane >> 5).  column(col) is called once per column in the tile (TN of them) and returns the sink
  // that is then called as sink(row in tile, value) for that column's 16 TM rows.
  template <class Column>
  __device__ __forceinline__ void epilogue(Column&& column) {
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
      auto sink = column((wn * TN + tn) * 32 + l32);
#pragma unroll
      for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int r = 0; r < 16; ++r) sink((wm * TM + tm) * 32 + (r & 3) + 8 * (r >> 2) + 4 * kk, acc[tm][tn][r]);
    }
  }
};

inline size_t lds_bytes(int BM, int BP) { return (size_t)2 * (BM + BP) * RS * sizeof(float); }

// Launch nb blocks of the tile kernel Kern with `lds` bytes of dynamic LDS; the first launch of each
// kernel raises its dynamic-LDS limit.
template <auto Kern, class Args>
hipError_t launch_tile(size_t lds, int64_t nb, const Args& a, hipStream_t st) {
  static std::once_flag once;
  static hipError_t attr = hipSuccess;
  std::call_once(once, [&] {
    attr = hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  });
  if (attr != hipSuccess) return attr;
  hipLaunchKernelGGL(Kern, dim3((unsigned)nb), dim3(NTH), lds, st, a);
  return hipGetLastError();
}

}  // namespace gemm
}  // namespace tb
