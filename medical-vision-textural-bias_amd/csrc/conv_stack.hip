// conv_stack.hip -- the deep ConvTranspose3d(3, stride 2, padding 1, output_padding 1) products (Cin a multiple
// of 32 -> Cout 32 or 64: the U-Net's up2 / up3 forwards and the input gradients of its stacked stride-2 units
// 32 -> 128 and 64 -> 256) in sub-pixel form on the split-bf16 matrix cores, with the eight parity classes
// stacked over ONE gather.
//
// conv_gemm.hip's kind == 2 runs every parity class as its own set of blocks: M is 32 or 64, the tiles are
// small, and an input voxel is gathered and split up to 8 times.  Here the k loop runs offset-major: a stage is
// (neighbour offset o of {0, 1}^3, 32 input channels, 64 positions of the input grid); its X~ image is gathered
// and split once and feeds every class that uses the offset (8, 4, 4, 2, 4, 2, 2, 1 classes: the 27 real
// (class, offset) pairs, no multiply-add on a zero weight).  The A operand of a stage is the classes' weight
// slabs stacked, 32 output channels each: up to 256 rows (convT_stack_plan.h: tables, pack layout, plan).
//
// Block: 512 threads, 32 output channels (Cout = 64: two m tiles) x 8 classes x 64 positions, on the stage loop
// of gemm_core.h's SplitTile (32-k stages, two LDS buffers, two register slots, one barrier per stage, the
// six-product step of split_bf16.h, per class one hi / lo pair summed once in the epilogue).
//   * Waves: wave w owns position half w & 1 (32 positions) and the two classes {7,1} {3,5} {2,4} {6,0}[w >> 1]:
//     two 32 x 32 accumulator pairs, 64 VGPRs.  A stage at offset o runs on the accumulators whose class contains
//     o; with waves w and w + 4 on one SIMD the four SIMDs hold, for every offset, the same number of active
//     accumulators (4; 2 2 2; 1 1 1; and one each on two SIMDs for o = 7): 14 accumulator-stages per channel
//     block on the busiest SIMD against 13.5 on average.  (The SIMD a wave lands on only changes the balance.)
//   * LDS: per stage buffer three bf16 part images of 256 A rows + 64 X~ rows of 80 B = 76 800 B, two buffers
//     153 600 B (one block per CU, two waves per SIMD); after the loop the first 65 536 B hold the block's
//     result [class][channel][position] f32, from which each thread stores the px = 0 / 1 values of a position as
//     one float2 (bias, then `add`, then the store; `add` is fetched before the k loop) or, with k split over
//     channel slices, the partials that k_cts_reduce sums in slice order (no float atomics).
//   * VGPRs: 64 accumulator + 36 fragment + 48 A slots + 16 X~ slots + 32 `add` values; the table of
//     scripts/resource_usage.py is in profiles/r25/README.md.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "convT_stack_plan.h"
#include "gemm_core.h"
#include "num_cu.h"
#include "texbias.h"

namespace {

using namespace tb::gemm;
namespace cts = tb::cts;

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int AROWS = 8 * cts::MB;                  // stacked A rows of a stage (offset 0: all 8 classes)
constexpr int IMG = (AROWS + cts::BP) * SRS;        // bytes per part image
constexpr int LBUF = 3 * IMG;                       // bytes per stage buffer
constexpr int LDS_BYTES = 2 * LBUF;                 // 153 600
static_assert(8 * cts::MB * cts::BP * 4 <= LDS_BYTES && LDS_BYTES <= 163840, "lds");

struct CSArgs {
  const float* x;
  const char* A;  // three bf16 part images, `apart` elements apart
  const float* bias;
  const float* add;
  float* y;
  float* part;
  int64_t xsn, ysn, addsn, apart;
  int64_t xbytes, abytes;
  int Cin, Cout, D, H, W;
  int P, ptiles, mtiles, CB, nsplit, cper;
};

// W [Cin][Cout][27] -> the three part images in stage order (cts::pack_index); one thread per weight
__global__ __launch_bounds__(256) void k_cts_pack(const float* __restrict__ W, uint16_t* __restrict__ out, int Cin,
                                                   int Cout, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int tap = (int)(i % 27);
  const int64_t cm = i / 27;
  const int m = (int)(cm % Cout), c = (int)(cm / Cout);
  unsigned p0, p1, p2;
  tb::split3_pk(W[i], 0.f, p0, p1, p2);
  uint16_t* o = out + cts::pack_index(Cin, c, m, tap);
  o[0] = (uint16_t)p0, o[total] = (uint16_t)p1, o[2 * total] = (uint16_t)p2;
}

__global__ __launch_bounds__(cts::NT) void k_convT_stack(const CSArgs a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = (int)threadIdx.x, lane = tid & 63, l32 = lane & 31, kk = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  int b = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int mt = b % a.mtiles;
  b /= a.mtiles;
  const int pt = b % a.ptiles, split = b / a.ptiles;
  const int cb_beg = split * a.cper;
  const int ncb = min(a.CB, cb_beg + a.cper) - cb_beg;
  const int nst = 8 * ncb;  // offset-major, then the slice's channel blocks
  const int p0 = pt * cts::BP;
  const int HW = a.H * a.W, S = a.D * HW;

  // the wave's position half and its two classes
  const int tile = w & 1;
  const int c0 = (0x6237 >> (4 * (w >> 1))) & 7, c1 = (0x0451 >> (4 * (w >> 1))) & 7;

  // the lane's position p0 + lane (the gather's, and the store's): voxel, validity of the 8 neighbours
  const int p = p0 + lane;
  const bool pok = p < a.P;
  int t = pok ? p : 0;
  const int px = t % a.W;
  t /= a.W;
  const int py = t % a.H;
  t /= a.H;
  const int pz = t % a.D, pn = t / a.D;
  const int xo = 4 * ((int)(pn * a.xsn) + pz * HW + py * a.W + px);
  uint32_t vm = 0;
#pragma unroll
  for (int o = 0; o < 8; ++o) {
    const bool v = pok && pz + ((o >> 2) & 1) < a.D && py + ((o >> 1) & 1) < a.H && px + (o & 1) < a.W;
    vm |= (v ? 1u : 0u) << o;
  }
  const int ysc = 8 * S, YW = 2 * a.W, YH = 2 * a.H;
  const int ysp = (2 * pz * YH + 2 * py) * YW + 2 * px;  // class 0's voxel of the position within a channel

  // `add`, fetched ahead of the k loop: thread item u = (parity pair zy = u >> 2, channel w + 8 (u & 3))
  const bool direct = a.nsplit == 1;
  const float* addp = direct ? a.add : nullptr;
  f32x2 av[16];
  if (addp) {
    const float* ab = addp + pn * a.addsn + ysp;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int m = mt * cts::MB + w + 8 * (u & 3), zy = u >> 2;
      av[u] = pok ? *reinterpret_cast<const f32x2*>(ab + m * ysc + ((zy >> 1) * YH + (zy & 1)) * YW) : f32x2{0.f, 0.f};
    }
  }

  // out-of-range offsets read 0 through the buffer descriptors (zero padding, stages past the slice)
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(a.x), 0, __builtin_amdgcn_readfirstlane((int)a.xbytes), 0x00020000);
  const __amdgpu_buffer_rsrc_t ar = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<char*>(a.A), 0, __builtin_amdgcn_readfirstlane((int)a.abytes), 0x00020000);
  const int apart2 = __builtin_amdgcn_readfirstlane((int)(2 * a.apart));
  const int xsc4 = 4 * S;

  float rb[2][8];
  u32x4 ra[2][2][3];
  int snc[2] = {0, 0};  // classes of the stage held in each register slot (0: none)
  auto load = [&](auto SL, int s) {
    constexpr int sl = decltype(SL)::value;
    const bool in = s < nst;
    const int o = in ? s / ncb : 0;
    const int cb = in ? cb_beg + s - o * ncb : 0;
    const int nc = cts::ncls_of(o);
    snc[sl] = in ? nc : 0;
    if (w < 4) {  // X~: waves 0-3, channels 8 w .. + 7 of the block, the lane's position
      const int off = 4 * (((o >> 2) & 1) * HW + ((o >> 1) & 1) * a.W + (o & 1));
      const int vo = (in && ((vm >> o) & 1u)) ? xo + off : (int)0x80000000;
      const int soff = (cb * cts::KCH + 8 * w) * xsc4;
#pragma unroll
      for (int r = 0; r < 8; ++r)
        rb[sl][r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xr, vo, soff + r * xsc4, 0));
    }
    // A: the stage's nc * 128 16-B items, contiguous in the pack
    const int base = 2 * (int)cts::stage_base(a.CB, mt, o, cb);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int it = tid + cts::NT * u;
      const int vo = (in && it < nc * 128) ? base + 16 * it : (int)0x80000000;
#pragma unroll
      for (int q = 0; q < 3; ++q)
        ra[sl][u][q] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(ar, vo, q * apart2, 0));
    }
  };
  auto store = [&](auto SL) {
    constexpr int sl = decltype(SL)::value;
    char* L = lds + sl * LBUF;
    const int nrows = snc[sl] * cts::MB;
    if (nrows == 0) return;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int it = tid + cts::NT * u;
      if (it < nrows * 4) {
        const int row = it & (nrows - 1), oct = it / nrows;
#pragma unroll
        for (int q = 0; q < 3; ++q) *reinterpret_cast<u32x4*>(L + q * IMG + row * SRS + 16 * oct) = ra[sl][u][q];
      }
    }
    if (w < 4) {
      unsigned q[3][4];
#pragma unroll
      for (int j = 0; j < 4; ++j) tb::split3_pk(rb[sl][2 * j], rb[sl][2 * j + 1], q[0][j], q[1][j], q[2][j]);
      char* d = L + (AROWS + lane) * SRS + 16 * w;
#pragma unroll
      for (int i = 0; i < 3; ++i) *reinterpret_cast<u32x4*>(d + i * IMG) = u32x4{q[i][0], q[i][1], q[i][2], q[i][3]};
    }
  };

  tb::f32x16s hi[2], lo[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) hi[i][r] = 0.f, lo[i][r] = 0.f;

  // the 16-k step ks of the stage (offset o) in LDS buffer sl, on the wave's accumulators whose class uses o
  auto half = [&](auto SL, auto KS, int o) {
    constexpr int sl = decltype(SL)::value, ks = decltype(KS)::value;
    const bool u0 = cts::uses(c0, o), u1 = cts::uses(c1, o);
    if (!u0 && !u1) return;
    const char* L = lds + sl * LBUF + 32 * ks + 16 * kk;
    tb::bf16x8 bf[3], af[3];
#pragma unroll
    for (int q = 0; q < 3; ++q)
      bf[q] = *reinterpret_cast<const tb::bf16x8*>(L + q * IMG + (AROWS + tile * 32 + l32) * SRS);
    if (u0) {
      const int row = cts::MB * cts::rank_of(c0, o) + l32;
#pragma unroll
      for (int q = 0; q < 3; ++q) af[q] = *reinterpret_cast<const tb::bf16x8*>(L + q * IMG + row * SRS);
      tb::mfma_split6_32(af, bf, hi[0], lo[0]);
    }
    if (u1) {
      const int row = cts::MB * cts::rank_of(c1, o) + l32;
#pragma unroll
      for (int q = 0; q < 3; ++q) af[q] = *reinterpret_cast<const tb::bf16x8*>(L + q * IMG + row * SRS);
      tb::mfma_split6_32(af, bf, hi[1], lo[1]);
    }
  };
  auto stage = [&](auto SL, int s) {
    constexpr int sl = decltype(SL)::value;
    const int o = s / ncb;
    half(SL, Idx<0>{}, o);
    load(SL, s + 2);
    half(SL, Idx<1>{}, o);
    store(Idx<1 - sl>{});
    __syncthreads();
  };
  load(Idx<0>{}, 0);
  store(Idx<0>{});
  load(Idx<1>{}, 1);
  __syncthreads();
  for (int s = 0; s < nst; s += 2) {
    stage(Idx<0>{}, s);
    stage(Idx<1>{}, s + 1);  // nst is even
  }

  // the block's result to LDS as [class][channel][position] (every wave is past the loop's last barrier)
  float* out = reinterpret_cast<float*>(lds);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int cls = i ? c1 : c0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = (r & 3) + 8 * (r >> 2) + 4 * kk;
      out[(cls * cts::MB + m) * cts::BP + tile * 32 + l32] = hi[i][r] + lo[i][r];
    }
  }
  __syncthreads();
  if (!pok) return;
  if (!direct) {
    // partials [slice][class][channel][position]
#pragma unroll
    for (int u = 0; u < 32; ++u) {
      const int m = w + 8 * (u & 3), cls = u >> 2;
      a.part[((int64_t)(split * 8 + cls) * a.Cout + mt * cts::MB + m) * a.P + p] = out[(cls * cts::MB + m) * cts::BP + lane];
    }
    return;
  }
  float* yb = a.y + pn * a.ysn + ysp;
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const int ml = w + 8 * (u & 3), zy = u >> 2, m = mt * cts::MB + ml;
    const float bv = a.bias ? a.bias[m] : 0.f;
    f32x2 v = {out[((2 * zy) * cts::MB + ml) * cts::BP + lane] + bv, out[((2 * zy + 1) * cts::MB + ml) * cts::BP + lane] + bv};
    if (addp) v += av[u];
    *reinterpret_cast<f32x2*>(yb + m * ysc + ((zy >> 1) * YH + (zy & 1)) * YW) = v;
  }
}

// y = bias + add + the slices' partials in slice order; one thread per (parity pair zy, channel, position),
// the px = 0 / 1 values as one float2
__global__ __launch_bounds__(256) void k_cts_reduce(const CSArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t per = (int64_t)a.Cout * a.P;
  if (i >= 4 * per) return;
  const int zy = (int)(i / per);
  const int64_t r = i - zy * per;
  const int m = (int)(r / a.P), p = (int)(r - (int64_t)m * a.P);
  const float* src = a.part + ((int64_t)(2 * zy) * a.Cout + m) * a.P + p;
  float s0 = 0.f, s1 = 0.f;
  for (int k = 0; k < a.nsplit; ++k) s0 += src[k * 8 * per], s1 += src[k * 8 * per + per];
  const float bv = a.bias ? a.bias[m] : 0.f;
  f32x2 v = {s0 + bv, s1 + bv};
  int t = p;
  const int px = t % a.W;
  t /= a.W;
  const int py = t % a.H;
  t /= a.H;
  const int pz = t % a.D, pn = t / a.D;
  const int YW = 2 * a.W, YH = 2 * a.H;
  const int64_t sp = (int64_t)m * 8 * a.D * a.H * a.W + ((int64_t)(2 * pz + (zy >> 1)) * YH + 2 * py + (zy & 1)) * YW + 2 * px;
  if (a.add) v += *reinterpret_cast<const f32x2*>(a.add + pn * a.addsn + sp);
  *reinterpret_cast<f32x2*>(a.y + pn * a.ysn + sp) = v;
}

int g_force_split = 0;

}  // namespace

int tb_convT3d_stack_set_split(int slices) {
  g_force_split = slices > 0 ? slices : 0;
  return TB_OK;
}

size_t tb_convT3d_stack_ws_bytes(int N, int Cin, int Cout, int Di, int Hi, int Wi) {
  cts::Plan pl;
  if (cts::make_plan(N, Cin, Cout, Di, Hi, Wi, tb::num_cu(), g_force_split, pl) != 0) return 0;
  return pl.ws_bytes();
}

int tb_convT3d_stack_config(int N, int Cin, int Cout, int Di, int Hi, int Wi, int64_t* cfg) {
  cts::Plan pl;
  const int rc = cts::make_plan(N, Cin, Cout, Di, Hi, Wi, tb::num_cu(), g_force_split, pl);
  if (rc != 0 || !cfg) return rc != 0 ? rc : TB_ERR_INVALID_ARG;
  cfg[0] = cts::BP, cfg[1] = pl.nsplit, cfg[2] = pl.cper, cfg[3] = pl.blocks(), cfg[4] = pl.P;
  cfg[5] = 4 * pl.part_floats, cfg[6] = (int64_t)pl.pack_bytes(), cfg[7] = (int64_t)pl.ws_bytes();
  return TB_OK;
}

int tb_convT3d_stack_pack_index(int Cin, int Cout, int c, int m, int tap, int64_t* index, int* cls, int* offset) {
  if (Cin < 1 || Cin % cts::KCH || (Cout != 32 && Cout != 64) || c < 0 || c >= Cin || m < 0 || m >= Cout || tap < 0 ||
      tap >= 27 || !index || !cls || !offset)
    return TB_ERR_INVALID_ARG;
  cts::pair_of_tap(tap, *cls, *offset);
  *index = cts::pack_index(Cin, c, m, tap);
  return TB_OK;
}

int tb_convT3d_stack_f32(const float* x, const float* W, const float* bias, const float* add, int64_t add_sn, float* y,
                         int64_t y_sn, int N, int Cin, int Cout, int Di, int Hi, int Wi, void* ws, size_t ws_bytes,
                         void* stream) {
  if (!x || !W || !y) return TB_ERR_INVALID_ARG;
  cts::Plan pl;
  const int rc = cts::make_plan(N, Cin, Cout, Di, Hi, Wi, tb::num_cu(), g_force_split, pl);
  if (rc != 0) return rc;
  if (!ws || ws_bytes < pl.ws_bytes()) return TB_ERR_WORKSPACE;
  const int64_t S = (int64_t)Di * Hi * Wi;
  CSArgs a{};
  a.x = x, a.bias = bias, a.add = add, a.y = y;
  a.xsn = (int64_t)Cin * S;
  a.ysn = y_sn > 0 ? y_sn : (int64_t)Cout * 8 * S;
  a.addsn = add_sn > 0 ? add_sn : (int64_t)Cout * 8 * S;
  // float2 stores / loads: 8-B aligned bases and even sample strides
  if (a.ysn < (int64_t)Cout * 8 * S || (a.ysn & 1) || (reinterpret_cast<uintptr_t>(y) & 7)) return TB_ERR_INVALID_ARG;
  if (add && (a.addsn < (int64_t)Cout * 8 * S || (a.addsn & 1) || (reinterpret_cast<uintptr_t>(add) & 7)))
    return TB_ERR_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(x) & 3) || (reinterpret_cast<uintptr_t>(W) & 3)) return TB_ERR_INVALID_ARG;
  a.xbytes = 4 * (int64_t)N * Cin * S;
  a.Cin = Cin, a.Cout = Cout, a.D = Di, a.H = Hi, a.W = Wi;
  a.P = pl.P, a.ptiles = pl.ptiles, a.mtiles = pl.mtiles, a.CB = pl.CB, a.nsplit = pl.nsplit, a.cper = pl.cper;
  a.apart = pl.pack_elems, a.abytes = 6 * pl.pack_elems;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* wsb = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(ws) + 255) & ~uintptr_t(255));
  hipLaunchKernelGGL(k_cts_pack, dim3((unsigned)((pl.pack_elems + 255) / 256)), dim3(256), 0, st, W,
                     reinterpret_cast<uint16_t*>(wsb), Cin, Cout, pl.pack_elems);
  if (hipGetLastError() != hipSuccess) return TB_ERR_HIP;
  a.A = wsb;
  a.part = reinterpret_cast<float*>(wsb + pl.pack_bytes());
  if (launch_tile<&k_convT_stack, cts::NT>(LDS_BYTES, pl.blocks(), a, st) != hipSuccess) return TB_ERR_HIP;
  if (a.nsplit > 1) {
    const int64_t tot = 4 * (int64_t)Cout * a.P;
    hipLaunchKernelGGL(k_cts_reduce, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, a);
    if (hipGetLastError() != hipSuccess) return TB_ERR_HIP;
  }
  return TB_OK;
}
