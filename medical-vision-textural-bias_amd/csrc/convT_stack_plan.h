// convT_stack_plan.h -- the (class, offset) tables, the packed-weight index map and the host plan of
// k_convT_stack (conv_stack.hip).  Plain C++ (no HIP types), so the plan also builds into a stand-alone host
// program; under hipcc the small helpers are __host__ __device__.
//
// ConvTranspose3d(3, stride 2, padding 1, output_padding 1) in sub-pixel form: output voxel 2 i + p per axis
// (parity p) reads input i + d (neighbour offset d) through tap t: p = 0 -> (d 0, tap 1); p = 1 -> (d 0, tap 2)
// and (d 1, tap 0).  With class cls = 4 pz + 2 py + px and offset o = 4 dz + 2 dy + dx the pair (cls, o) is a real
// tap iff o is a sub-mask of cls: 27 pairs; offset o serves the 8 >> popcount(o) classes that contain it, and
// among those class cls has rank = the bits of cls outside o, compressed (ascending class order).
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define TB_CTS_HD __host__ __device__
#else
#define TB_CTS_HD
#endif

namespace tb {
namespace cts {

constexpr int BP = 64;    // positions per block
constexpr int MB = 32;    // output channels per block (each of the 8 classes: 256 stacked A rows)
constexpr int KCH = 32;   // channels per stage
constexpr int NT = 512;   // threads per block

TB_CTS_HD inline int ncls_of(int o) { return 8 >> (((o >> 2) & 1) + ((o >> 1) & 1) + (o & 1)); }

// (class, offset) pairs of the offsets before o: 0 8 12 16 18 22 24 26 (27 in all)
TB_CTS_HD inline int pair_base(int o) {
  int s = 0;
  for (int i = 0; i < o; ++i) s += ncls_of(i);
  return s;
}

TB_CTS_HD inline bool uses(int cls, int o) { return (cls & o) == o; }

TB_CTS_HD inline int rank_of(int cls, int o) {
  int r = 0, n = 0;
  for (int b = 0; b < 3; ++b)
    if (!((o >> b) & 1)) r |= ((cls >> b) & 1) << n++;
  return r;
}

// the weight's tap index (tz 9 + ty 3 + tx) of the pair
TB_CTS_HD inline int tap_index(int cls, int o) {
  int t[3];
  for (int b = 0; b < 3; ++b) t[b] = ((cls >> b) & 1) ? (((o >> b) & 1) ? 0 : 2) : 1;
  return t[2] * 9 + t[1] * 3 + t[0];
}

// the pair of a tap: the inverse of tap_index
TB_CTS_HD inline void pair_of_tap(int tap, int& cls, int& o) {
  const int t[3] = {tap % 3, (tap / 3) % 3, tap / 9};
  cls = o = 0;
  for (int b = 0; b < 3; ++b) {
    if (t[b] != 1) cls |= 1 << b;
    if (t[b] == 0) o |= 1 << b;
  }
}

// Element index, in one bf16 part image, of the stage (m tile mt, offset o, channel block cb): the stage's
// ncls_of(o) * 32 rows x 32 k follow, as [k octet 4][row][8 k] with row = 32 rank + output channel in tile.
TB_CTS_HD inline int64_t stage_base(int CB, int mt, int o, int cb) {
  return ((int64_t)(mt * 27 + pair_base(o)) * CB + (int64_t)cb * ncls_of(o)) * (MB * KCH);
}

// where W[c][m][tap] goes
TB_CTS_HD inline int64_t pack_index(int Cin, int c, int m, int tap) {
  int cls, o;
  pair_of_tap(tap, cls, o);
  const int k = c % KCH, row = MB * rank_of(cls, o) + m % MB;
  return stage_base(Cin / KCH, m / MB, o, c / KCH) + ((int64_t)(k >> 3) * (MB * ncls_of(o)) + row) * 8 + (k & 7);
}

struct Plan {
  int N, Cin, Cout, D, H, W;
  int P, ptiles, mtiles, CB;
  int nsplit, cper;  // k slices, channel blocks per slice
  int64_t pack_elems;   // elements per bf16 part image: 27 Cin Cout
  int64_t part_floats;  // split partials: nsplit x 8 classes x Cout x P
  size_t pack_bytes() const { return ((size_t)pack_elems * 6 + 255) & ~(size_t)255; }
  size_t ws_bytes() const { return pack_bytes() + 4 * (((size_t)part_floats + 63) & ~(size_t)63) + 256; }
  int64_t blocks() const { return (int64_t)ptiles * mtiles * nsplit; }
};

// 0 = ok, 1 = invalid argument, 2 = unsupported size (TB_OK / TB_ERR_INVALID_ARG / TB_ERR_UNSUPPORTED_SIZE).
// force_split > 0 asks for that many k slices (measurement scripts, tests); num_cu: block slots of the chip
// (one block per CU).
inline int make_plan(int N, int Cin, int Cout, int D, int H, int W, int num_cu, int force_split, Plan& pl) {
  if (N < 1 || Cin < 1 || Cout < 1 || D < 1 || H < 1 || W < 1) return 1;
  if ((Cout != 32 && Cout != 64) || Cin % KCH != 0) return 2;
  const int64_t S = (int64_t)D * H * W;
  // 32-bit byte offsets: over x as a whole (the gather's buffer), within a sample of y
  if (4 * (int64_t)N * Cin * S >= (int64_t)1 << 31 || 4 * (int64_t)Cout * 8 * S >= (int64_t)1 << 31) return 2;
  if ((int64_t)N * S > ((int64_t)1 << 30)) return 2;
  pl.N = N, pl.Cin = Cin, pl.Cout = Cout, pl.D = D, pl.H = H, pl.W = W;
  pl.P = (int)(N * S);
  pl.ptiles = (pl.P + BP - 1) / BP;
  pl.mtiles = Cout / MB;
  pl.CB = Cin / KCH;
  pl.pack_elems = (int64_t)27 * Cin * Cout;
  // k slices: rounds of the chip's block slots x (stages per block + a fixed per-block cost of ~6 stages:
  // decode, pipeline fill, the epilogue through LDS) at ~0.5 us per stage, plus, when split, the partials'
  // round trip (written once, read once, at ~3 TB/s) and the reduce launch.  Ties keep fewer slices.
  const int64_t base = (int64_t)pl.ptiles * pl.mtiles;
  const int slots = num_cu > 0 ? num_cu : 256;
  double best = 1e30;
  int ns = 1;
  for (int s = 1; s <= pl.CB && s <= 8; ++s) {
    const int cper = (pl.CB + s - 1) / s;
    if ((pl.CB + cper - 1) / cper != s) continue;  // the same slices as a smaller s
    const int64_t rounds = (base * s + slots - 1) / slots;
    double cost = 0.5 * (double)rounds * (8 * cper + 6);
    if (s > 1) cost += 3.0 + 2.0 * s * 8.0 * Cout * (double)pl.P * 4.0 / 3.0e6;
    if (cost < best * 0.97) best = cost, ns = s;
  }
  if (force_split > 0) ns = force_split < pl.CB ? force_split : pl.CB;
  pl.cper = (pl.CB + ns - 1) / ns;
  pl.nsplit = (pl.CB + pl.cper - 1) / pl.cper;
  pl.part_floats = pl.nsplit > 1 ? (int64_t)pl.nsplit * 8 * Cout * pl.P : 0;
  if (4 * pl.part_floats >= (int64_t)1 << 40) return 2;
  return 0;
}

}  // namespace cts
}  // namespace tb
