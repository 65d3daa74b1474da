// conv_gemm.hip -- the U-Net's channel-deep convolutions as implicit GEMMs on the matrix cores.
//
// The reference's MONAI UNet (10_scripts/20_Gibbs_filters/stylized_gibbs12p5.py:192-199; module tree
// source_code/test.ipynb:754-1010) has, besides the full-resolution layers of conv_up.hip, the
// stride-2 entries of levels 1-3 (16 -> 32, 32 -> 64, 64 -> 128, each twice: the unit and its
// residual), the bottom unit (128 -> 256, 256 -> 256, a 1x1x1 128 -> 256 residual) and the
// ConvTranspose3d ups (384 -> 64, 128 -> 32).  MIOpen/CK ran them at 23-51 TFLOP/s plus NCDHW <->
// NDHWC transposes (~4.5 ms of a 17.2 ms C3 step, forward and input gradient included).  Here every
// one of them, and every input gradient, is one kernel:
//
//   Y[m][q] = bias[m] + add[m][q] + sum_{k < K} A[m][k] X~[k][q]          (q: GEMM position, k = (c, tap))
//
// with X~ gathered from the NCDHW input on the fly (no im2col buffer): position q = (n, oz, oy, ox) of
// the position grid, tap j of the class's tap list with offsets (dz, dy, dx), input voxel
// (S oz + dz, S oy + dy, S ox + dx) (zero outside), output voxel (ymul oz + pz, ymul oy + py, ymul ox + px):
//   * Conv3d 3x3x3 / 1x1x1, stride S, padding 1 / 0: one class, taps (tz - 1, ty - 1, tx - 1), A = W;
//   * the input gradient of a stride-1 Conv3d: A[c][m t] = W[m][c][26 - t] (packed by k_cg_pack);
//   * ConvTranspose3d(stride 2, padding 1, output_padding 1) forward -- and, with a stride-2 Conv3d's
//     weight, that layer's input gradient -- in sub-pixel form: 8 parity classes (pz, py, px), per axis
//     parity 0 takes tap 1 at offset 0, parity 1 taps 2 (offset 0) and 0 (offset +1); position grid =
//     the input grid, ymul = 2, A_cls[m][c T_cls + j] = W[c][m][tap_j]: every multiply-add a real tap.
//
// k runs tap-major (k = tap Cin + c, A packed to match by k_cg_pack; Cin % 8 == 0), so the 8 k rows a
// wave gathers per stage are 8 channels of ONE tap: the tap's offset and every lane's validity bit are
// per stage, the 8 loads per lane one base address plus channel strides.  A block computes a BM x BP tile
// of Y on the tile pipeline of gemm_core.h: A rows staged by float4 loads, X~ gathered by scalar loads
// (each lane's positions fixed for the block).  Small GEMMs split k over nsplit slices into float
// partials summed by k_cg_reduce (which adds bias / add and scatters to the output grid).  Blocks are
// numbered so that the m tiles of one position tile land on one XCD (its L2 serves the X~ re-reads).
//
// The 128 x 128 tile (M > 64) runs in split precision on the bf16 matrix cores (SplitTile of gemm_core.h,
// 512 threads): k_cg_pack writes A as its three bf16 parts, which the A stager moves to LDS as they are, and
// the gathered X~ is split at its LDS store; bias, `add`, the partials and k_cg_reduce stay f32.  The
// 32 x 128 and 64 x 64 tiles measured no faster that way on any C3 layer (they are held by the gather, not by
// the f32 MFMA rate) and stay on the f32 Tile (profiles/r17/README.md).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>

#include "gemm_core.h"
#include "num_cu.h"
#include "texbias.h"

namespace {

using namespace tb::gemm;

struct CGArgs {
  const float* x;
  const void* A;  // packed by k_cg_pack: f32, or the three bf16 part images
  const float* bias;
  const float* add;
  float* y;
  float* part;
  int64_t xsn, ysn, addsn;  // batch strides (floats); channel strides below
  int64_t xbytes;           // bytes of x from its base (the gather's buffer range)
  int xsc, ysc;
  int Cin, M;
  int IDm, IH, IW;  // input extents
  int OD, OH, OW;   // position grid
  int YH, YW;       // output H, W extents
  int S, ymul;
  int P;            // N OD OH OW
  int nsplit, kper, mtiles, ptiles, ncls;
  int kind;  // taps: 0 = 3x3x3 (tz - 1, ty - 1, tx - 1), 1 = 1x1x1, 2 = sub-pixel class (parity bits = class)
  int64_t aoff[8];
  int64_t apart;  // elements between the bf16 part images of the packed A (split tiles)
  int Kc[8], Tc[8];
};

// tap j of class cls: input offsets and the weight's tap index (host and device)
__host__ __device__ inline void tap_of(int kind, int cls, int j, int& dz, int& dy, int& dx, int& widx) {
  if (kind == 0) {
    dz = j / 9 - 1, dy = (j / 3) % 3 - 1, dx = j % 3 - 1, widx = j;
  } else if (kind == 1) {
    dz = dy = dx = 0, widx = 0;
  } else {
    // parity 0: tap 1 at offset 0; parity 1: i = 0 -> tap 2 at offset 0, i = 1 -> tap 0 at offset +1
    const int pz = (cls >> 2) & 1, py = (cls >> 1) & 1, px = cls & 1;
    const int nx = 1 + px, ny = 1 + py;
    const int ix = j % nx, iy = (j / nx) % ny, iz = j / (nx * ny);
    dz = pz ? iz : 0, dy = py ? iy : 0, dx = px ? ix : 0;
    const int tz = pz ? (iz ? 0 : 2) : 1, ty = py ? (iy ? 0 : 2) : 1, tx = px ? (ix ? 0 : 2) : 1;
    widx = tz * 9 + ty * 3 + tx;
  }
}

// SP: the split-precision tile (SplitTile, NT threads; A read as the three bf16 part images k_cg_pack wrote,
// the gathered X~ split at its LDS store); otherwise the f32 Tile on NT = NTH threads and an f32 A.
template <int BM, int BP, int WGM, int NT, bool SP>
__global__ __launch_bounds__(NT) void k_conv_gemm(const CGArgs a) {
  using TileT = std::conditional_t<SP, SplitTile<BM, BP, WGM, NT>, Tile<BM, BP, WGM>>;
  using LdsT = std::conditional_t<SP, char, float>;
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  static_assert(SP || NT == NTH, "the f32 tile runs on NTH threads");
  constexpr int PG = NT / 256;                         // position groups: wave w gathers k octet w & 3 of group w >> 2
  constexpr int NPOS = BP / (64 * PG);                 // gather positions per lane
  constexpr int AQ = SP ? (BM * 4 + NT - 1) / NT       // A (row, k octet) items per thread per stage, three parts each
                        : BM * KC / 4 / NT;            // A float4 per thread per stage
  static_assert(NPOS >= 1 && AQ >= 1, "tile");
  extern __shared__ __attribute__((aligned(16))) char lds_raw[];
  LdsT* const lds_dyn = reinterpret_cast<LdsT*>(lds_raw);
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wk = w & 3, pg = w >> 2;
  int b = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int mt = b % a.mtiles;
  b /= a.mtiles;
  const int pt = b % a.ptiles;
  b /= a.ptiles;
  const int split = b % a.nsplit, cls = b / a.nsplit;
  const int T = a.Tc[cls], K = a.Kc[cls];
  const int Cin = a.Cin;
  const int k_beg = split * a.kper;
  const int k_end = min(K, k_beg + a.kper);
  const int m0 = mt * BM, p0 = pt * BP;
  const int IHW = a.IH * a.IW;

  // gather positions: lane + 64 (PG i + pg) of the tile; byte offset of the tap-(0,0,0) voxel of channel 0
  // and the per-tap validity bits
  int xo[NPOS];
  uint32_t vm[NPOS];
#pragma unroll
  for (int i = 0; i < NPOS; ++i) {
    const int p = p0 + lane + 64 * (PG * i + pg);
    const bool ok = p < a.P;
    int t = ok ? p : 0;
    const int ox = t % a.OW;
    t /= a.OW;
    const int oy = t % a.OH;
    t /= a.OH;
    const int oz = t % a.OD, n = t / a.OD;
    const int bz = a.S * oz, by = a.S * oy, bx = a.S * ox;
    xo[i] = 4 * ((int)(n * a.xsn) + bz * IHW + by * a.IW + bx);
    uint32_t m = 0;
    for (int j = 0; j < T; ++j) {
      int dz, dy, dx, wi;
      tap_of(a.kind, cls, j, dz, dy, dx, wi);
      const int iz = bz + dz, iy = by + dy, ix = bx + dx;
      const bool v = ok && iz >= 0 && iz < a.IDm && iy >= 0 && iy < a.IH && ix >= 0 && ix < a.IW;
      m |= (v ? 1u : 0u) << j;
    }
    vm[i] = m;
  }
  // the input through a buffer descriptor: an out-of-range offset reads 0 (the zero padding and the
  // k rows past k_end), so the gather needs no selects
  const uint32_t xbytes = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.xbytes);
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, (int)xbytes, 0x00020000);
  const int xsc4 = 4 * a.xsc;

  // the stagers' two register slots (gemm_core.h); stage s holds k rows k_beg + 32 s .. + 31
  float rb[2][NPOS][8];
  std::conditional_t<SP, u32x4[2][AQ][3], f32x4[2][AQ]> ra;
  auto gather = [&](auto SL, int k0) {
    constexpr int sl = decltype(SL)::value;
    // rows k0 + 8 wk .. + 7: channels c .. c + 7 of tap t (Cin % 8 == 0)
    const int k = k0 + 8 * wk;
    const int t = k / Cin, c = k - t * Cin;
    const bool kin = k < k_end;
    int dz, dy, dx, wi;
    tap_of(a.kind, cls, kin ? t : 0, dz, dy, dx, wi);
    const int off = 4 * ((dz * a.IH + dy) * a.IW + dx);
    const int soff = c * xsc4;
#pragma unroll
    for (int i = 0; i < NPOS; ++i) {
      const bool v = kin && ((vm[i] >> t) & 1u);
      const int vo = v ? xo[i] + off : (int)0x80000000;
#pragma unroll
      for (int r = 0; r < 8; ++r)
        rb[sl][i][r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xr, vo, soff + r * xsc4, 0));
    }
  };
  // A of the class: f32 [M][K], or three bf16 images [M][K] a.apart elements apart (range: to the end of
  // the third image's rows of this class)
  const int esz = SP ? 2 : 4;
  const char* Ab = reinterpret_cast<const char*>(a.A) + esz * a.aoff[cls];
  const int apart2 = __builtin_amdgcn_readfirstlane((int)(2 * a.apart));
  const uint32_t abytes =
      (uint32_t)__builtin_amdgcn_readfirstlane((int)(esz * (int64_t)a.M * K + (SP ? 2 * (int64_t)apart2 : 0)));
  const __amdgpu_buffer_rsrc_t ar = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(Ab), 0, (int)abytes, 0x00020000);
  auto aload = [&](auto SL, int k0) {
    constexpr int sl = decltype(SL)::value;
#pragma unroll
    for (int u = 0; u < AQ; ++u) {
      if constexpr (SP) {
        const int it = tid + NT * u, row = it % BM, kq = k0 + 8 * (it / BM);
        const int m = m0 + row;
        const bool v = (BM * 4 % NT == 0 || it < BM * 4) && m < a.M && kq < k_end;
        const int vo = v ? 2 * (m * K + kq) : (int)0x80000000;
#pragma unroll
        for (int p = 0; p < 3; ++p)
          ra[sl][u][p] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(ar, vo, p * apart2, 0));
      } else {
        const int q4 = tid + NT * u, row = q4 % BM, kq = k0 + 4 * (q4 / BM);
        const int m = m0 + row;
        const int vo = (m < a.M && kq < k_end) ? 4 * (m * K + kq) : (int)0x80000000;
        ra[sl][u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ar, vo, 0, 0));
      }
    }
  };
  auto load = [&](auto SL, int s) {  // masked by k < k_end: past the slice both read zeros
    gather(SL, k_beg + s * KC);
    aload(SL, k_beg + s * KC);
  };
  auto store = [&](auto SL) {
    constexpr int sl = decltype(SL)::value;
    if constexpr (SP) {
      char* L = lds_dyn + sl * TileT::LBUF;
#pragma unroll
      for (int u = 0; u < AQ; ++u) {
        const int it = tid + NT * u;
        if (BM * 4 % NT == 0 || it < BM * 4) {
#pragma unroll
          for (int p = 0; p < 3; ++p)
            *reinterpret_cast<u32x4*>(L + p * TileT::IMG + TileT::a_off(it % BM, it / BM)) = ra[sl][u][p];
        }
      }
#pragma unroll
      for (int i = 0; i < NPOS; ++i) {
        unsigned q[3][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) tb::split3_pk(rb[sl][i][2 * j], rb[sl][i][2 * j + 1], q[0][j], q[1][j], q[2][j]);
        char* d = L + TileT::b_off(lane + 64 * (PG * i + pg), wk);
#pragma unroll
        for (int p = 0; p < 3; ++p)
          *reinterpret_cast<u32x4*>(d + p * TileT::IMG) = u32x4{q[p][0], q[p][1], q[p][2], q[p][3]};
      }
    } else {
      float* L = lds_dyn + sl * TileT::LBUF;
#pragma unroll
      for (int u = 0; u < AQ; ++u) {
        const int q4 = tid + NT * u, row = q4 % BM, c4 = q4 / BM;
        *reinterpret_cast<f32x4*>(L + row * RS + 4 * c4) = ra[sl][u];
      }
#pragma unroll
      for (int i = 0; i < NPOS; ++i) {
        float* d = L + (BM + lane + 64 * i) * RS + 8 * w;
        *reinterpret_cast<f32x4*>(d) = f32x4{rb[sl][i][0], rb[sl][i][1], rb[sl][i][2], rb[sl][i][3]};
        *reinterpret_cast<f32x4*>(d + 4) = f32x4{rb[sl][i][4], rb[sl][i][5], rb[sl][i][6], rb[sl][i][7]};
      }
    }
  };

  TileT tile(w, lane);
  // an empty slice (a sub-pixel class whose K ends before k_beg) runs no stage and stores zeros
  tile.run(lds_dyn, k_beg < k_end ? (k_end - k_beg + KC - 1) / KC : 0, load, store);

  const int M = a.M, P = a.P;
  if (a.nsplit > 1) {
    tile.epilogue([&](int col) {
      const int p = p0 + col;
      float* dst = a.part + ((int64_t)(cls * a.nsplit + split) * M) * P + p;
      return [=](int row, float v) {
        const int m = m0 + row;
        if (p < P && m < M) dst[(int64_t)m * P] = v;
      };
    });
    return;
  }
  const float* bias = a.bias;
  const int ysc = a.ysc;
  tile.epilogue([&](int col) {
    const int p = p0 + col;
    int t = p;
    const int ox = t % a.OW;
    t /= a.OW;
    const int oy = t % a.OH;
    t /= a.OH;
    const int oz = t % a.OD, n = t / a.OD;
    const int pc = a.kind == 2 ? cls : 0;
    const int64_t sp = ((int64_t)(a.ymul * oz + (pc >> 2)) * a.YH + (a.ymul * oy + ((pc >> 1) & 1))) * a.YW +
                       a.ymul * ox + (pc & 1);
    float* yo = a.y + n * a.ysn + sp;
    const float* ad = a.add ? a.add + n * a.addsn + sp : nullptr;
    return [=](int row, float v) {
      const int m = m0 + row;
      if (p < P && m < M) {
        v += bias ? bias[m] : 0.f;
        if (ad) v += ad[(int64_t)m * ysc];
        yo[(int64_t)m * ysc] = v;
      }
    };
  });
}

// y = bias + add + sum of the split partials, scattered to the output grid; one thread per (cls, m, q)
__global__ __launch_bounds__(256) void k_cg_reduce(const CGArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t per = (int64_t)a.M * a.P;
  if (i >= per * a.ncls) return;
  const int cls = (int)(i / per);
  const int64_t r = i - cls * per;
  const int m = (int)(r / a.P), p = (int)(r - (int64_t)m * a.P);
  const float* src = a.part + (int64_t)cls * a.nsplit * per + (int64_t)m * a.P + p;
  float v = a.bias ? a.bias[m] : 0.f;
  float s = 0.f;
  for (int k = 0; k < a.nsplit; ++k) s += src[k * per];
  v += s;
  int t = p;
  const int ox = t % a.OW;
  t /= a.OW;
  const int oy = t % a.OH;
  t /= a.OH;
  const int oz = t % a.OD, n = t / a.OD;
  const int pc = a.kind == 2 ? cls : 0;
  const int64_t sp =
      ((int64_t)(a.ymul * oz + (pc >> 2)) * a.YH + (a.ymul * oy + ((pc >> 1) & 1))) * a.YW + a.ymul * ox + (pc & 1);
  if (a.add) v += a.add[n * a.addsn + (int64_t)m * a.ysc + sp];
  a.y[n * a.ysn + (int64_t)m * a.ysc + sp] = v;
}

// Packed A operands, k tap-major: A_cls[m][j Cin + c] = W(m, c, tap_j of cls).  mode 0 (Conv3d, W
// [M][Cin][T]): W[m][c][widx]; mode 1 (input gradient of a stride-1 conv whose weight is Wl [Cin][M][T]):
// Wl[c][m][T - 1 - widx]; mode 2 (sub-pixel classes, Wt [Cin][M][27]): Wt[c][m][widx].
// SP: written as its three bf16 parts (split_bf16.h), image p at out + p total elements -- the split tile's A
// stager then moves 16-B octets to LDS with no conversion.
template <bool SP>
__global__ __launch_bounds__(256) void k_cg_pack(const float* __restrict__ W, void* __restrict__ out, int mode,
                                                 int64_t total, const CGArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  int cls = 0;
  while (cls + 1 < a.ncls && i >= a.aoff[cls + 1]) ++cls;
  const int64_t r = i - a.aoff[cls];
  const int Kc = a.Kc[cls], Cin = a.Cin, M = a.M;
  const int m = (int)(r / Kc), k = (int)(r - (int64_t)m * Kc);
  const int j = k / Cin, c = k - j * Cin;
  int dz, dy, dx, wi;
  tap_of(a.kind, cls, j, dz, dy, dx, wi);
  const int TW = a.kind == 1 ? 1 : 27;  // taps in the weight tensor
  float v;
  if (mode == 0) v = W[((int64_t)m * Cin + c) * TW + wi];
  else if (mode == 1) v = W[((int64_t)c * M + m) * TW + (TW - 1 - wi)];
  else v = W[((int64_t)c * M + m) * 27 + wi];
  if constexpr (SP) {
    unsigned p0, p1, p2;
    tb::split3_pk(v, 0.f, p0, p1, p2);
    uint16_t* o = static_cast<uint16_t*>(out) + i;
    o[0] = (uint16_t)p0, o[total] = (uint16_t)p1, o[2 * total] = (uint16_t)p2;
  } else {
    static_cast<float*>(out)[i] = v;
  }
}

struct Plan {
  CGArgs a;
  int BM, BP, WGM;
  bool split;  // the split-precision tile (its packed A is three bf16 images, 6 B per element)
  size_t pack_floats, part_floats;
  size_t pack_bytes() const { return (pack_floats * (split ? 6 : 4) + 255) & ~size_t(255); }
  size_t ws_bytes() const { return pack_bytes() + 4 * ((part_floats + 63) & ~size_t(63)) + 256; }
};

// The tiles: M <= 32 -> 32 x 128; M <= 64 -> 64 x 64; else 128 x 128 on 512 threads (eight waves of 64 x 32:
// its two split stage buffers are 120 KB, one block per CU, so the block itself brings two waves per SIMD).
struct TileCfg {
  int BM, BP, WGM, NT;
  bool split;
};
constexpr TileCfg kTiles[3] = {{32, 128, 1, NTH, false}, {64, 64, 2, NTH, false}, {128, 128, 2, 512, true}};

// Fill the geometry and tiling of a call (no device pointers).  Returns TB_OK or an error code.
int make_plan(int mode, int N, int Cin, int M, int D, int H, int Wd, int stride, int ksize, Plan& pl) {
  if (N < 1 || Cin < 1 || M < 1 || D < 1 || H < 1 || Wd < 1) return TB_ERR_INVALID_ARG;
  if (mode < 0 || mode > 2 || (ksize != 3 && ksize != 1) || (stride != 1 && stride != 2)) return TB_ERR_INVALID_ARG;
  if (Cin % 8 != 0) return TB_ERR_UNSUPPORTED_SIZE;
  if (mode == 2 && (ksize != 3 || stride != 2)) return TB_ERR_INVALID_ARG;
  if (mode == 1 && stride != 1) return TB_ERR_INVALID_ARG;
  CGArgs& a = pl.a;
  a = CGArgs{};
  a.Cin = Cin, a.M = M, a.IDm = D, a.IH = H, a.IW = Wd;
  a.xsc = D * H * Wd;
  if ((int64_t)N * Cin * D * H * Wd >= (int64_t)1 << 31) return TB_ERR_UNSUPPORTED_SIZE;
  if (mode == 2) {
    a.S = 1, a.ymul = 2, a.OD = D, a.OH = H, a.OW = Wd, a.YH = 2 * H, a.YW = 2 * Wd, a.ncls = 8, a.kind = 2;
    int64_t off = 0;
    for (int cls = 0; cls < 8; ++cls) {
      const int T = (1 + ((cls >> 2) & 1)) * (1 + ((cls >> 1) & 1)) * (1 + (cls & 1));
      a.Tc[cls] = T, a.Kc[cls] = Cin * T, a.aoff[cls] = off;
      off += (int64_t)M * Cin * T;
    }
    pl.pack_floats = (size_t)off;
  } else {
    const int pad = ksize == 3 ? 1 : 0;
    a.S = stride, a.ymul = 1, a.ncls = 1, a.kind = ksize == 3 ? 0 : 1;
    a.OD = (D + 2 * pad - ksize) / stride + 1, a.OH = (H + 2 * pad - ksize) / stride + 1,
    a.OW = (Wd + 2 * pad - ksize) / stride + 1;
    a.YH = a.OH, a.YW = a.OW;
    const int T = ksize * ksize * ksize;
    a.Tc[0] = T, a.Kc[0] = Cin * T, a.aoff[0] = 0;
    pl.pack_floats = (size_t)M * Cin * T;
  }
  a.ysc = a.ymul == 2 ? 8 * a.OD * a.OH * a.OW : a.OD * a.OH * a.OW;
  if ((int64_t)N * M * a.ysc >= (int64_t)1 << 31) return TB_ERR_UNSUPPORTED_SIZE;
  a.P = N * a.OD * a.OH * a.OW;
  const TileCfg& tc = kTiles[M <= 32 ? 0 : (M <= 64 ? 1 : 2)];
  pl.BM = tc.BM, pl.BP = tc.BP, pl.WGM = tc.WGM, pl.split = tc.split;
  a.apart = (int64_t)pl.pack_floats;
  if (6 * (int64_t)pl.pack_floats >= (int64_t)1 << 31) return TB_ERR_UNSUPPORTED_SIZE;
  a.mtiles = (M + pl.BM - 1) / pl.BM;
  a.ptiles = (a.P + pl.BP - 1) / pl.BP;
  int Kmax = 0;
  for (int c = 0; c < a.ncls; ++c) Kmax = a.Kc[c] > Kmax ? a.Kc[c] : Kmax;
  // split k to minimise (rounds of the chip's block slots) x (stages per block + a fixed per-block cost
  // of ~3 stages: position decode, tap masks, partial stores); ties keep the smaller split
  const int64_t base = (int64_t)a.mtiles * a.ptiles * a.ncls;
  int occ = (int)(163840 / (pl.split ? split_lds_bytes(pl.BM, pl.BP) : lds_bytes(pl.BM, pl.BP)));
  occ = occ > 4 ? 4 : (occ < 1 ? 1 : occ);
  const int64_t slots = (int64_t)occ * tb::num_cu();
  const int stages = (Kmax + KC - 1) / KC;
  double best = 1e30;
  int ns = 1;
  for (int s = 1; s <= 16 && s <= stages; ++s) {
    const int64_t blocks = base * s;
    const int64_t rounds = (blocks + slots - 1) / slots;
    const double cost = (double)rounds * ((stages + s - 1) / s + 3);
    if (cost < best * 0.97) best = cost, ns = s;
  }
  a.kper = ((Kmax + ns - 1) / ns + KC - 1) / KC * KC;
  a.nsplit = (Kmax + a.kper - 1) / a.kper;
  pl.part_floats = a.nsplit > 1 ? (size_t)a.ncls * a.nsplit * M * a.P : 0;
  return TB_OK;
}

template <int I>
hipError_t launch(const CGArgs& a, hipStream_t st) {
  constexpr TileCfg c = kTiles[I];
  const int64_t nb = (int64_t)a.mtiles * a.ptiles * a.nsplit * a.ncls;
  return launch_tile<&k_conv_gemm<c.BM, c.BP, c.WGM, c.NT, c.split>, c.NT>(
      c.split ? split_lds_bytes(c.BM, c.BP) : lds_bytes(c.BM, c.BP), nb, a, st);
}

}  // namespace

size_t tb_conv3d_gemm_workspace_bytes(int mode, int N, int Cin, int M, int D, int H, int Wd, int stride, int ksize) {
  Plan pl;
  if (make_plan(mode, N, Cin, M, D, H, Wd, stride, ksize, pl) != TB_OK) return 0;
  return pl.ws_bytes();
}

int tb_conv3d_gemm_f32(int mode, const float* x, int64_t xsn, const float* W, const float* bias, const float* add,
                       int64_t addsn, float* y, int64_t ysn, int N, int Cin, int M, int D, int H, int Wd, int stride,
                       int ksize, void* ws, size_t ws_bytes, void* stream) {
  if (!x || !W || !y) return TB_ERR_INVALID_ARG;
  Plan pl;
  const int rc = make_plan(mode, N, Cin, M, D, H, Wd, stride, ksize, pl);
  if (rc != TB_OK) return rc;
  CGArgs& a = pl.a;
  if (!ws || ws_bytes < pl.ws_bytes()) return TB_ERR_WORKSPACE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  a.x = x, a.bias = bias, a.add = add, a.y = y;
  a.xsn = xsn > 0 ? xsn : (int64_t)Cin * a.xsc;
  a.ysn = ysn > 0 ? ysn : (int64_t)M * a.ysc;
  a.addsn = addsn > 0 ? addsn : a.ysn;
  a.xbytes = 4 * ((int64_t)(N - 1) * a.xsn + (int64_t)Cin * a.xsc);
  if (a.xbytes >= (int64_t)1 << 31) return TB_ERR_UNSUPPORTED_SIZE;
  char* wsb = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(ws) + 255) & ~uintptr_t(255));
  {
    const int64_t total = (int64_t)pl.pack_floats;
    const dim3 grid((unsigned)((total + 255) / 256));
    if (pl.split) hipLaunchKernelGGL(k_cg_pack<true>, grid, dim3(256), 0, st, W, (void*)wsb, mode, total, a);
    else hipLaunchKernelGGL(k_cg_pack<false>, grid, dim3(256), 0, st, W, (void*)wsb, mode, total, a);
    a.A = wsb;
  }
  a.part = reinterpret_cast<float*>(wsb + pl.pack_bytes());
  hipError_t e = hipSuccess;
  if (pl.BM == 32) e = launch<0>(a, st);
  else if (pl.BM == 64) e = launch<1>(a, st);
  else e = launch<2>(a, st);
  if (e != hipSuccess) return TB_ERR_HIP;
  if (a.nsplit > 1) {
    const int64_t tot = (int64_t)a.ncls * a.M * a.P;
    hipLaunchKernelGGL(k_cg_reduce, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, a);
    if (hipGetLastError() != hipSuccess) return TB_ERR_HIP;
  }
  return TB_OK;
}

int tb_conv3d_gemm_config(int mode, int N, int Cin, int M, int D, int H, int Wd, int stride, int ksize, int64_t* cfg) {
  Plan pl;
  const int rc = make_plan(mode, N, Cin, M, D, H, Wd, stride, ksize, pl);
  if (rc != TB_OK || !cfg) return rc != TB_OK ? rc : TB_ERR_INVALID_ARG;
  cfg[0] = pl.BM, cfg[1] = pl.BP, cfg[2] = pl.a.nsplit, cfg[3] = pl.a.kper;
  cfg[4] = (int64_t)pl.a.mtiles * pl.a.ptiles * pl.a.nsplit * pl.a.ncls;
  cfg[5] = pl.a.P;
  return TB_OK;
}
