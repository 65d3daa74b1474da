// gemm_core.h -- the tile pipeline shared by the matrix-core conv GEMMs (conv_gemm.hip: forward and
// input gradient; conv_wgrad_gemm.hip: weight gradient), as two tiles with one contract (run / stage /
// epilogue, what the kernels rely on below): Tile, exact f32 on mfma_f32_32x32x2f32 (the weight gradient
// and conv_gemm.hip's 32 x 128 and 64 x 64 tiles), and SplitTile, split precision on
// v_mfma_f32_32x32x16_bf16 (split_bf16.h; conv_gemm.hip's 128 x 128 tile), described at its definition.
//
// Tile: a 256-thread block computes a BM x BP tile of C = A B^T over stages of KC = 32 reduction elements.  A
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
//   * The MFMA order along the reduction is fixed -- Tile: within a stage step st pairs element st (lanes
//     0-31) with element 16 + st (lanes 32-63), half 0 then half 1, stages in order; SplitTile: see there
//     -- so results are bit-reproducible across changes of everything else.
//   * Slot and buffer indices are compile-time (Idx<0> / Idx<1>): the stagers' register slots stay in
//     registers; a runtime index would send them to scratch.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>
#include <type_traits>

#include "split_bf16.h"

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

// ---- the split-precision tile --------------------------------------------------------------------------
constexpr int SRS = 80;  // LDS bytes per row of one part image: 32 k bf16 + 16 B pad

// NT threads (NT / 64 waves as WGM x NT / 64 / WGM) compute the BM x BP tile in split precision
// (split_bf16.h): the same run / stage / epilogue, the same 32-k stages, the same register slots and
// barriers as Tile, the stage in LDS as three bf16 part images.
//
// LDS, per stage buffer: image p (part p = 0, 1, 2) at p * (BM + BP) * SRS bytes, in it row r (A rows 0 ..
// BM - 1, then the BP rows of B) at r * SRS, k innermost: element k of a row at byte 2 k.  The stagers write
// 16-B octets (8 k of one row and part); fragment (row l32, k = 16 ks + 8 kk .. + 7) is one ds_read_b128.
// Banks, with the row pitch of 20 dwords:
//   * ds_read_b128 is served in groups of 16 lanes, rows {0-3, 12-15, 20-27} or {4-11, 16-19, 28-31} of one
//     kk, 64 banks: 20 r mod 64 = 4 (5 r mod 16); either row set holds one row of every residue mod 16
//     ({0-3, 12-15, 20-27} = {0-3, 12-15, 4-11} mod 16) and 5 is odd, so 5 r mod 16 takes 16 different
//     values: the 16 reads of 4 dwords cover the 64 banks once;
//   * ds_write_b128 is served in groups of 8 consecutive lanes = 8 consecutive rows at one k octet, 32
//     banks: 20 r mod 32 = 4 (5 r mod 8), eight different values: the 32 banks once.
//
// Order along the reduction (fixed, so results are bit-reproducible): stages in order; in a stage the 16-k
// step ks = 0 (k 0 - 15: lanes 0-31 elements 0-7, lanes 32-63 elements 8-15) then ks = 1; in a step, per
// sub-tile, a1 b1, a0 b2, a2 b0, a0 b1, a1 b0 into `lo` and a0 b0 into `hi`.  hi + lo is taken once, in the
// epilogue, before the kernel's sink adds bias / `add` or stores the partial.
//
// The accumulator of v_mfma_f32_32x32x16_bf16 maps as that of v_mfma_f32_32x32x2_f32 (CDNA4 ISA, "32x32"
// output layout, four 8-row blocks: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)); A is
// row (lane & 31), k = 8 (lane >> 5) + j, B likewise with its column.
template <int BM, int BP, int WGM, int NT>
struct SplitTile {
  static constexpr int NW = NT / 64, WGN = NW / WGM;
  static constexpr int TM = BM / WGM / 32, TN = BP / WGN / 32;
  static constexpr int IMG = (BM + BP) * SRS;  // bytes per part image
  static constexpr int LBUF = 3 * IMG;         // bytes per stage buffer
  static_assert(TM >= 1 && TN >= 1 && WGM * WGN * 64 == NT, "tile");

  f32x16s hi[TM][TN], lo[TM][TN];
  int wm, wn, kk, l32;

  __device__ __forceinline__ SplitTile(int w, int lane) : wm(w % WGM), wn(w / WGM), kk(lane >> 5), l32(lane & 31) {
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
      for (int tn = 0; tn < TN; ++tn)
#pragma unroll
        for (int r = 0; r < 16; ++r) hi[tm][tn][r] = 0.f, lo[tm][tn][r] = 0.f;
  }

  // byte offset in a part image of A row `row` / B row `row`, k octet `oct` (the stagers' store address)
  static __device__ __forceinline__ int a_off(int row, int oct) { return row * SRS + 16 * oct; }
  static __device__ __forceinline__ int b_off(int row, int oct) { return (BM + row) * SRS + 16 * oct; }

  // the 16-k step ks of the stage in LDS buffer sl
  template <int sl, int ks>
  __device__ __forceinline__ void half(const char* lds) {
    const char* L = lds + sl * LBUF + 32 * ks + 16 * kk;
    bf16x8 af[TM][3], bf[TN][3];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
      for (int p = 0; p < 3; ++p)
        af[tm][p] = *reinterpret_cast<const bf16x8*>(L + p * IMG + ((wm * TM + tm) * 32 + l32) * SRS);
#pragma unroll
    for (int tn = 0; tn < TN; ++tn)
#pragma unroll
      for (int p = 0; p < 3; ++p)
        bf[tn][p] = *reinterpret_cast<const bf16x8*>(L + p * IMG + (BM + (wn * TN + tn) * 32 + l32) * SRS);
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
      for (int tn = 0; tn < TN; ++tn) mfma_split6_32(af[tm], bf[tn], hi[tm][tn], lo[tm][tn]);
  }

  template <class Load, class Store>
  __device__ __forceinline__ void run(const char* lds, int nst, Load&& load, Store&& store) {
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

  // stage s: its first 16 k, then the loads of stage s + 2, the last 16 k, stage s + 1 (split at this
  // store) to the other LDS buffer
  template <int sl, class Load, class Store>
  __device__ __forceinline__ void stage(const char* lds, int s, Load& load, Store& store) {
    half<sl, 0>(lds);
    load(Idx<sl>{}, s + 2);
    half<sl, 1>(lds);
    store(Idx<1 - sl>{});
    __syncthreads();
  }

  // as Tile::epilogue, on hi + lo
  template <class Column>
  __device__ __forceinline__ void epilogue(Column&& column) {
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
      auto sink = column((wn * TN + tn) * 32 + l32);
#pragma unroll
      for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          sink((wm * TM + tm) * 32 + (r & 3) + 8 * (r >> 2) + 4 * kk, hi[tm][tn][r] + lo[tm][tn][r]);
    }
  }
};

inline size_t split_lds_bytes(int BM, int BP) { return (size_t)2 * 3 * (BM + BP) * SRS; }

// Launch nb blocks of NT threads of the tile kernel Kern with `lds` bytes of dynamic LDS; the first launch
// of each kernel raises its dynamic-LDS limit.
template <auto Kern, int NT = NTH, class Args>
hipError_t launch_tile(size_t lds, int64_t nb, const Args& a, hipStream_t st) {
  static std::once_flag once;
  static hipError_t attr = hipSuccess;
  std::call_once(once, [&] {
    attr = hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  });
  if (attr != hipSuccess) return attr;
  hipLaunchKernelGGL(Kern, dim3((unsigned)nb), dim3(NT), lds, st, a);
  return hipGetLastError();
}

}  // namespace gemm
}  // namespace tb
