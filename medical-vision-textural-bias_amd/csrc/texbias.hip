// texbias.hip -- gfx950 kernels and the C ABI (include/texbias.h) of the texbias library.
//
// The pass kernels A/B/C (and the spectrum statistics) live in kern_*.hip, one translation unit
// per kernel and radix set; this file holds the small kernels and the host side of the C ABI.
// Pass plan of one k-space filter call (DESIGN.md "Kernels"):
//   A  k_slab_fwd   per (bc, h) slab: real rows -> pair-packed R2C along D -> C2C along W,
//                   in one 150 KB LDS slab; stores the half spectrum (digit-reversed W).
//   B  k_kspace     per (bc, tile of T spectrum columns): C2C along H (DIF), the sample's
//                   op program on every coefficient, inverse along H (DIT).
//   C  k_slab_inv   per (bc, h) slab: inverse W, C2R along D, scale 1/N, zero D-padding,
//                   per-sample min/max epilogue.
//   D  k_salt_pepper  Philox u, class, sparse in-place MIN/MAX scatter.
#include <hip/hip_runtime.h>

#include <cmath>
#include <math.h>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "band.h"
#include "fft_core.h"
#include "kernels.h"
#include "point.h"
#include "plan_host.h"
#include "sap_core.h"
#include "spike_grad.h"
#include "wrap.h"

using namespace tb;

namespace {

thread_local int g_last_hip = 0;
// compiled (compile-time) plans enabled: TEXBIAS_COMPILED_PLANS=0 or tb_set_compiled_plans(0) turns
// them off, e.g. to compare against the generic passes
bool g_compiled_plans = [] {
  const char* e = std::getenv("TEXBIAS_COMPILED_PLANS");
  return !(e && e[0] == '0');
}();

inline int hip_fail(hipError_t e) {
  g_last_hip = (int)e;
  return TB_ERR_HIP;
}
#define TB_HIP(call)                              \
  do {                                            \
    hipError_t e_ = (call);                       \
    if (e_ != hipSuccess) return hip_fail(e_);    \
  } while (0)

// ------------------------------------------------------------------ timing
struct TimingRec {
  hipEvent_t a, b;
  int slot;
  double bytes;
};
std::mutex g_tmu;
bool g_timing = false;
std::vector<TimingRec> g_recs;
std::vector<hipEvent_t> g_pool;
const char* g_slot_kernel[4] = {"", "", "", ""};

hipEvent_t ev_get() {
  if (!g_pool.empty()) {
    hipEvent_t e = g_pool.back();
    g_pool.pop_back();
    return e;
  }
  // Timing-only events: no system-scope release / acquire around the pass (hipEventDisableSystemFence),
  // so the end stamp is not delayed by an L2 write-back and the pass does not start on invalidated
  // caches -- the stamps bracket the kernel itself (round 6: every pass 1-2 us shorter than with
  // default events, which rocprofv3's kernel durations confirm).
  hipEvent_t e = nullptr;
  if (hipEventCreateWithFlags(&e, hipEventDisableSystemFence) != hipSuccess) return nullptr;
  return e;
}
struct Timer {  // records [begin, end) of one pass when timing is enabled
  hipEvent_t a = nullptr, b = nullptr;
  int slot;
  double bytes;
  hipStream_t st;
  // bytes: the launch's algorithmic HBM bytes (each global input/output element counted once)
  Timer(int s, hipStream_t stream, double nbytes = 0.0, const char* kernel = nullptr)
      : slot(s), bytes(nbytes), st(stream) {
    if (!g_timing) return;
    std::lock_guard<std::mutex> lk(g_tmu);
    if (kernel) g_slot_kernel[s] = kernel;
    a = ev_get();
    b = ev_get();
    if (a) (void)hipEventRecord(a, st);
  }
  ~Timer() {
    if (!a || !b) return;
    (void)hipEventRecord(b, st);
    std::lock_guard<std::mutex> lk(g_tmu);
    g_recs.push_back({a, b, slot, bytes});
  }
};

// ---------------------------------------------------------------- kernels

__global__ void k_minmax_init(uint32_t* mm, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    mm[2 * i] = 0xffffffffu;
    mm[2 * i + 1] = 0u;
  }
}

template <int NT>
__global__ __launch_bounds__(NT) void k_minmax(const float* __restrict__ x, uint32_t* __restrict__ mm, int64_t rows,
                                               int len, int64_t ld, int64_t sb) {
  __shared__ float red[2 * NT / 64];
  const int b = blockIdx.y;
  const float* xb = x + b * sb;
  const int64_t n = rows * len;
  float lo = 3.402823466e38f, hi = -3.402823466e38f;
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
    const int64_t r = i / len;
    const float v = xb[r * ld + (i - r * len)];
    lo = fminf(lo, v);
    hi = fmaxf(hi, v);
  }
  block_minmax_atomic<NT>(lo, hi, red, mm + 2 * b);
}

struct SapThr {
  float lo[TB_MAX_BATCH], hi[TB_MAX_BATCH];
};

template <int NT>
__global__ __launch_bounds__(NT) void k_salt_pepper(const float* __restrict__ x, float* __restrict__ y,
                                                    int8_t* __restrict__ cls, const float* __restrict__ uin,
                                                    uint64_t seed, uint64_t offset, SapThr thr,
                                                    const uint32_t* __restrict__ mm, int b0, int64_t rows, int len,
                                                    int64_t ld, int64_t sb, int sparse) {
  const int bl = blockIdx.y;
  const int b = b0 + bl;
  const int64_t n = rows * len;
  const float vmin = key2f(mm[2 * b]) * 0.5f, vmax = key2f(mm[2 * b + 1]) * 0.5f;
  const float lo = thr.lo[bl], hi = thr.hi[bl];
  const int64_t lin0 = (int64_t)b * n;  // logical (unpadded) voxel index of this sample
  const int64_t ngroups = (n + 3) / 4;
  for (int64_t g = (int64_t)blockIdx.x * NT + threadIdx.x; g < ngroups; g += (int64_t)gridDim.x * NT) {
    u32x4 r;
    if (!uin) r = philox((uint64_t)(lin0 / 4 + g), offset, seed);  // n % 4 handled below
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t i = 4 * g + q;
      if (i >= n) break;
      // element offset of voxel i; 32-bit division while the sample fits (the 64-bit one is ~4x the
      // VALU work), and in the sparse Philox path only for the ~p of voxels that are written
      auto offset_of = [&]() -> int64_t {
        const int64_t row = n < 0x7fffffff ? (int64_t)((uint32_t)i / (uint32_t)len) : i / len;
        return b * sb + row * ld + (i - row * len);
      };
      float u;
      int64_t off = -1;
      if (uin) {
        off = offset_of();
        u = uin[off];
      } else {
        // counter of logical voxel L = lin0 + i: the group index and lane of L itself, so the
        // stream is independent of how samples are batched when n % 4 == 0 (the usual case)
        if ((lin0 & 3) == 0) u = u01(r.v[q]);
        else {
          const int64_t L = lin0 + i;
          u = u01(philox((uint64_t)(L >> 2), offset, seed).v[L & 3]);
        }
      }
      const int c = sap_class(u, lo, hi);
      if (cls || !sparse || c) {
        if (off < 0) off = offset_of();
        if (cls) cls[off] = (int8_t)c;
        if (sparse) {
          if (c) y[off] = c == 1 ? vmin : vmax;
        } else {
          y[off] = c == 0 ? x[off] : (c == 1 ? vmin : vmax);
        }
      }
    }
  }
}

// Salt-and-pepper from the device stream: instead of one uniform per voxel, each lane walks a
// segment of SAP_SEG voxels jumping straight to the next changed voxel -- the gap to it is
// geometric, floor(log(u) / log(1 - p)) -- and draws its class (MIN with probability lo / hi).
// The changed voxels form the same Bernoulli(p) field with P(MIN) = p_lo, P(MAX) = p_hi - p_lo
// as u <= lo / lo < u <= hi of the reference (:478-479), at ~p of the RNG work.
#ifndef TB_SAP_SEG
#define TB_SAP_SEG 256  // voxels per thread: 4 waves per SIMD on a C3 launch (1024: 61 us, 256: 51.5 us;
                        // blocks walking the volume last to first, where the previous pass's last lines
                        // might still be cached: no change, 48.2 vs 48.5 us; round 6: the same walk into
                        // a per-wave LDS bitmap, then stored in address order with one masked store per
                        // 64 voxels -- half the L2 requests -- 78 vs 48 us, dropped)
#endif
constexpr int SAP_SEG = TB_SAP_SEG;
struct SapGeomArgs {
  float* y;
  int8_t* cls;
  uint64_t seed, offset;
  float lo[TB_MAX_BATCH], hi[TB_MAX_BATCH];
  const uint32_t* mm;
  int b0;
  int64_t rows;
  int len;
  int64_t ld, sb;
};
__global__ __launch_bounds__(256) void k_sap_geom(SapGeomArgs a) {
  const int bl = blockIdx.y, b = a.b0 + bl;
  const int64_t n = a.rows * a.len;
  const int64_t start = ((int64_t)blockIdx.x * 256 + threadIdx.x) * SAP_SEG;
  const float p = a.hi[bl];
  if (start >= n || !(p > 0.f)) return;
  const int64_t end = start + SAP_SEG < n ? start + SAP_SEG : n;
  const float vmin = key2f(a.mm[2 * b]) * 0.5f, vmax = key2f(a.mm[2 * b + 1]) * 0.5f;
  const float pmin = a.lo[bl] > 0.f ? a.lo[bl] / p : 0.f;  // P(MIN | changed)
  const float lq = p >= 1.f ? -INFINITY : log1pf(-p);
  const uint64_t ctr0 = ((uint64_t)b << 44) ^ ((uint64_t)(start / SAP_SEG) << 20);
  int64_t pos = start - 1;
  uint32_t j = 0;
  for (;;) {
    const u32x4 r = philox(ctr0 | j++, a.offset, a.seed);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float u1 = ((float)(r.v[2 * h] >> 8) + 1.0f) * (1.0f / 16777216.0f);  // (0, 1]
      const float g = lq == -INFINITY ? 0.f : floorf(logf(u1) / lq);
      pos += 1 + (g < (float)SAP_SEG ? (int64_t)g : (int64_t)SAP_SEG);
      if (pos >= end) return;
      const int c = u01(r.v[2 * h + 1]) < pmin ? 1 : 2;
      const int64_t row = n < 0x7fffffff ? (int64_t)((uint32_t)pos / (uint32_t)a.len) : pos / a.len;
      const int64_t off = b * a.sb + row * a.ld + (pos - row * a.len);
      a.y[off] = c == 1 ? vmin : vmax;
      if (a.cls) a.cls[off] = (int8_t)c;
    }
  }
}

__global__ void k_disk_mask(float* __restrict__ m, int64_t outer, int n0, int n1, int n2, int int_r, int64_t r2i,
                            float r2f, int inside_off) {
  const int64_t per = (int64_t)n0 * n1 * n2;
  const int64_t total = outer * per;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t r = i % per;
    const int i2 = (int)(r % n2);
    r /= n2;
    const int i1 = (int)(r % n1);
    const int i0 = (int)(r / n1);
    const int64_t d0 = i0 - n0 / 2, d1 = i1 - n1 / 2, d2 = i2 - n2 / 2;
    const int64_t s = d0 * d0 + d1 * d1 + d2 * d2;
    bool in = int_r ? (s < r2i) : ((float)s < r2f);
    if (inside_off) in = !in;
    m[i] = in ? 1.f : 0.f;
  }
}

}  // namespace

// ------------------------------------------------------------------- plan
struct tb_plan {
  tb_plan_dev dev;
  PlanTables host;
  void* dmem = nullptr;
  int rset_h = RS_ALL;   // radix set of the H axis (pass B)
  int rset_wd = RS_ALL;  // radix set of the W and D axes (passes A, C)
  int lds_max = 65536;
  int ncu = 256;         // compute units (grid of the persistent compiled-plan slab kernels)
  bool ct_slab = false;  // (W, D) has a compile-time slab plan (slab_ct.h)
  bool ct_tile = false;  // H has a compile-time pass-B plan (kspace_ct.h)
  bool ct_half = false;  // (H, W, D) has half-unit passes A / C and the split pass B (slab_ct.h HalfPlan)
  float* tds = nullptr;  // band pass C': [D/2 + 1][2][NCOLS] cos / sin(2 pi kd d / D), d < D/2 + 1, else 0
  float* tbt = nullptr;  // band pass A': [2][KSd][2][64] B fragments of the folded D product
  void* tbt16 = nullptr;  // band pass A', compiled D: split-f16 B fragments [KS16][cos/sin][hi/lo][64][8]
  bool generic = false;  // full-spectrum route on the direct-DFT fallback (kern_generic.hip)
  double* wrapq = nullptr;  // odd D <= WRAP_MAX_COLS: the wrap route's D circulant table q[D] (wrap.h)
};

namespace {

constexpr int NT_SAP = 256;

bool needs_all(const tb_axis& ax) {
  for (int s = 0; s < ax.nst; ++s) {
    const int r = ax.radix[s];
    if (r > 10 && r != 12 && r != 15 && r != 16) return true;
  }
  return false;
}

int pick_tile(int H, int lds_max) {
  // ~32 KB tiles (measured best of 16/32/64 KB at H = 240: 4 workgroups per CU, 128-B rows)
  constexpr int budget = 32768;
  int T = budget / (H * 8);
  if (T > 64) T = 64;
  if (T >= 16) T &= ~7;   // whole 64-B segments per tile row
  if (T < 4) T = 4;
  while (tile_geo(H, T).total_cf * 8 > lds_max && T > 1) --T;
  return T;
}

}  // namespace

// Exported functions: C linkage comes from their declarations in texbias.h.
int tb_version(void) { return TB_VERSION; }

const char* tb_error_string(int code) {
  switch (code) {
    case TB_OK: return "ok";
    case TB_ERR_INVALID_ARG: return "invalid argument";
    case TB_ERR_UNSUPPORTED_SIZE: return "unsupported transform size (an axis above the direct-DFT fallback's 10240)";
    case TB_ERR_HIP: return "HIP runtime error";
    case TB_ERR_WORKSPACE: return "workspace too small";
    default: return "unknown error";
  }
}

int tb_last_hip_error(void) { return g_last_hip; }

int tb_plan_create(int H, int W, int D, tb_plan** out) {
  if (!out) return TB_ERR_INVALID_ARG;
  *out = nullptr;
  tb_plan* p = new tb_plan();
  int rc = build_tables(H, W, D, p->host);
  if (rc == TB_ERR_UNSUPPORTED_SIZE) {
    // an axis with a prime factor > 31: the full-spectrum route runs on the direct-DFT fallback
    // (the band passes take any size); the mixed-radix tables are never read
    p->generic = true;
    const int n[3] = {H, W, D};
    for (int a = 0; a < 3; ++a) {
      if (!factorize(n[a], p->host.ax[a])) {
        p->host.ax[a].n = n[a];
        p->host.ax[a].nst = 0;
      }
      p->host.tw[a] = twiddles(n[a]);
    }
    p->host.rev_d.resize(D);
    p->host.irev_h.resize(H);
    p->host.irev_w.resize(W);
    for (int i = 0; i < D; ++i) p->host.rev_d[i] = i;
    for (int i = 0; i < H; ++i) p->host.irev_h[i] = i;
    for (int i = 0; i < W; ++i) p->host.irev_w[i] = i;
  } else if (rc != TB_OK) {
    delete p;
    return rc;
  }
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { delete p; return hip_fail(hipGetLastError()); }
  int lds = 0;
  if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) == hipSuccess && lds > 0)
    p->lds_max = lds;
  int ncu = 0;
  if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && ncu > 0)
    p->ncu = ncu;
  // compile-time slab plan: same shape and therefore the same radix order as the runtime plan
  p->ct_slab = !p->generic && tb::slab_ct_supported(W, D);
  p->ct_tile = !p->generic && tb::kspace_ct_supported(H);
  p->ct_half = !p->generic && tb::slab_half_supported(W, D) && tb::kspace_half_supported(H, W, D);
  const SlabGeo sg = slab_geo(W, D);
  if ((size_t)sg.total_cf * 8 > (size_t)p->lds_max) p->generic = true;  // slab above the LDS: fallback too
  if (p->generic) p->ct_slab = p->ct_half = false;
  // device tables: tw[H], tw[W], tw[D] (cf) + rev_d[D], irev_h[H], irev_w[W] (int)
  const size_t ncf = (size_t)H + W + D, nint = (size_t)D + H + W;
  const size_t bytes = ncf * sizeof(cf) + nint * sizeof(int);
  std::vector<char> buf(bytes);
  char* q = buf.data();
  size_t off_tw[3], off_i[3];
  size_t o = 0;
  const int n[3] = {H, W, D};
  for (int a = 0; a < 3; ++a) {
    off_tw[a] = o;
    std::memcpy(q + o, p->host.tw[a].data(), n[a] * sizeof(cf));
    o += n[a] * sizeof(cf);
  }
  const std::vector<int>* iv[3] = {&p->host.rev_d, &p->host.irev_h, &p->host.irev_w};
  for (int a = 0; a < 3; ++a) {
    off_i[a] = o;
    std::memcpy(q + o, iv[a]->data(), iv[a]->size() * sizeof(int));
    o += iv[a]->size() * sizeof(int);
  }
  if (hipMalloc(&p->dmem, bytes) != hipSuccess) { delete p; return hip_fail(hipGetLastError()); }
  if (hipMemcpy(p->dmem, buf.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(p->dmem);
    delete p;
    return hip_fail(hipGetLastError());
  }
  char* d = static_cast<char*>(p->dmem);
  p->dev.H = H; p->dev.W = W; p->dev.D = D; p->dev.pad = 0;
  for (int a = 0; a < 3; ++a) {
    p->dev.ax[a] = p->host.ax[a];
    p->dev.tw[a] = reinterpret_cast<const cf*>(d + off_tw[a]);
  }
  p->dev.rev_d = reinterpret_cast<const int*>(d + off_i[0]);
  p->dev.irev_h = reinterpret_cast<const int*>(d + off_i[1]);
  p->dev.irev_w = reinterpret_cast<const int*>(d + off_i[2]);
  if (D <= BAND_MAX_D) {  // folded synthesis table (pass C') and the D-product B fragments (pass A'),
                         // double precision; plans no band route can take (D > BAND_MAX_D) skip them
    const int Dh = D / 2 + 1, ncols = 32 * ((Dh + 31) / 32), KSd = (Dh + 3) / 4;
    std::vector<float> ts((size_t)Dh * 2 * ncols, 0.f), tb((size_t)2 * KSd * 2 * 64, 0.f);
    for (int k = 0; k < Dh; ++k)
      for (int d = 0; d < Dh; ++d) {
        const double ang = 2.0 * 3.14159265358979323846 * (double)(((int64_t)k * d) % D) / (double)D;
        ts[((size_t)k * 2) * ncols + d] = (float)std::cos(ang);
        ts[((size_t)k * 2 + 1) * ncols + d] = (float)std::sin(ang);
      }
    for (int nt = 0; nt < 2; ++nt)
      for (int ks = 0; ks < KSd; ++ks)
        for (int part = 0; part < 2; ++part)
          for (int ln = 0; ln < 64; ++ln) {
            const int d = 4 * ks + (ln >> 4), kd = 16 * nt + (ln & 15);
            if (d >= Dh || kd >= Dh) continue;
            const double ang = 2.0 * 3.14159265358979323846 * (double)(((int64_t)kd * d) % D) / (double)D;
            tb[(((size_t)nt * KSd + ks) * 2 + part) * 64 + ln] = (float)(part ? std::sin(ang) : std::cos(ang));
          }
    if (D == 155) {  // the compiled pass-A' kernel's split-f16 table (x 2^8, hi / lo halves)
      const int KS16 = tb::band_fwd16_ks(D);
      std::vector<_Float16> t16((size_t)KS16 * 2 * 2 * 64 * 8);
      for (int ks = 0; ks < KS16; ++ks)
        for (int part = 0; part < 2; ++part)
          for (int ln = 0; ln < 64; ++ln)
            for (int i = 0; i < 8; ++i) {  // B[k = 8 (ln / 16) + i][n = ln % 16]: folded d, kd
              const int d = 32 * ks + 8 * (ln >> 4) + i, kd = ln & 15;
              double v = 0.0;
              if (d < Dh && kd < Dh) {
                const double ang = 2.0 * 3.14159265358979323846 * (double)(((int64_t)kd * d) % D) / (double)D;
                v = (part ? std::sin(ang) : std::cos(ang)) * (double)tb::BAND_FWD16_TSCALE;
              }
              const float vf = (float)v;
              const _Float16 h = (_Float16)vf, l = (_Float16)(vf - (float)h);
              t16[((((size_t)ks * 2 + part) * 2 + 0) * 64 + ln) * 8 + i] = h;
              t16[((((size_t)ks * 2 + part) * 2 + 1) * 64 + ln) * 8 + i] = l;
            }
      if (hipMalloc(&p->tbt16, t16.size() * 2) != hipSuccess ||
          hipMemcpy(p->tbt16, t16.data(), t16.size() * 2, hipMemcpyHostToDevice) != hipSuccess) {
        tb_plan_destroy(p);
        return hip_fail(hipGetLastError());
      }
    }
    if (hipMalloc(reinterpret_cast<void**>(&p->tds), ts.size() * 4) != hipSuccess ||
        hipMemcpy(p->tds, ts.data(), ts.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&p->tbt), tb.size() * 4) != hipSuccess ||
        hipMemcpy(p->tbt, tb.data(), tb.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
      tb_plan_destroy(p);
      return hip_fail(hipGetLastError());
    }
  }
  if ((D & 1) && D <= WRAP_MAX_COLS) {  // separable wrap route's D-axis circulant (float64)
    std::vector<double> q(D);
    tb::wrap_q_table(D, q.data());
    if (hipMalloc(reinterpret_cast<void**>(&p->wrapq), q.size() * 8) != hipSuccess ||
        hipMemcpy(p->wrapq, q.data(), q.size() * 8, hipMemcpyHostToDevice) != hipSuccess) {
      tb_plan_destroy(p);
      return hip_fail(hipGetLastError());
    }
  }
  p->rset_h = needs_all(p->host.ax[0]) ? RS_ALL : RS_SMALL;
  p->rset_wd = (needs_all(p->host.ax[1]) || needs_all(p->host.ax[2])) ? RS_ALL : RS_SMALL;
  *out = p;
  return TB_OK;
}

int tb_plan_destroy(tb_plan* plan) {
  if (!plan) return TB_OK;
  if (plan->dmem) (void)hipFree(plan->dmem);
  if (plan->tds) (void)hipFree(plan->tds);
  if (plan->tbt) (void)hipFree(plan->tbt);
  if (plan->tbt16) (void)hipFree(plan->tbt16);
  if (plan->wrapq) (void)hipFree(plan->wrapq);
  delete plan;
  return TB_OK;
}

size_t tb_workspace_bytes(const tb_plan* plan, int bc) {
  if (!plan || bc < 0) return 0;
  const size_t spec = (size_t)bc * plan->dev.H * plan->dev.W * (plan->dev.D / 2 + 1) * sizeof(cf);
  // the band passes' largest layout (band_plan() refuses boxes past these limits)
  BandGeo g{};
  g.KH = BAND_MAX_KH;
  g.KW = 31;
  g.NDk = BAND_MAX_NDK;
  g.ncol = BAND_MAX_ZCOL;
  g.KS = 32;
  g.NCOL = 32 * ((plan->dev.D / 2 + 1 + 31) / 32);
  g.cat = 0;  // 2 KS = 64 rows: the most either layout uses
  g.PT = 0;
  g.NTD = (plan->dev.D + 31) / 32 + 64;  // the split-f16 table for any pad up to 2048 columns
  const size_t band = band_ws(g, plan->dev.H, bc).total;
  const size_t gen = plan->generic ? gen_workspace_bytes(plan->dev.H, plan->dev.W, plan->dev.D, bc) : 0;
  const size_t m = spec > band ? spec : band;
  return m > gen ? m : gen;
}

int tb_plan_radices(const tb_plan* plan, int axis, int* radices) {
  if (!plan || axis < 0 || axis > 2 || !radices) return -1;
  const tb_axis& a = plan->dev.ax[axis];
  for (int s = 0; s < a.nst; ++s) radices[s] = a.radix[s];
  return a.nst;
}

static bool use_ct_slab(const tb_plan* p) { return g_compiled_plans && p->ct_slab; }

// Half units + split spectrum for the full route's passes (slab_ct.h HalfPlan) where the plan has
// them; TEXBIAS_HALF=0 or tb_set_half_units(0): the whole-slab compiled passes.
static bool g_half = [] {
  const char* e = std::getenv("TEXBIAS_HALF");
  return !(e && e[0] == '0');
}();
static bool use_half(const tb_plan* p) { return g_half && g_compiled_plans && p->ct_half; }

// channel-volumes per A -> B -> C chain (tb_set_chain_chunk; 0 = all, the default).  Chunks of
// 2..4 channel-volumes keep the spectrum within the Infinity Cache between passes, but measured
// slower at C3 (0.99 / 0.94 / 0.89 vs 0.85 ms per step: the passes are latency-bound, not
// HBM-bound, and smaller launches leave more of the chip idle in their tails).
static int g_chunk = -1;  // tb_set_chain_chunk
static int chunk_bc(const tb_plan*) { return g_chunk > 0 ? g_chunk : 0; }

template <int RS>
static int launch_slab_fwd(const tb_plan* p, const float* x, const int64_t* xs, cf* S, int bc0, int nbc,
                           hipStream_t st) {
  SlabFwdArgs a{p->dev, x, xs[0], xs[1], xs[2], S, bc0, nbc};
  if (use_ct_slab(p)) {
    TB_HIP(tb::launch_slab_fwd_ct(a, p->ncu, st));
    return TB_OK;
  }
  const size_t lds = (size_t)slab_geo(p->dev.W, p->dev.D).total_cf * sizeof(cf);
  TB_HIP(tb::launch_slab_fwd<RS>(a, dim3(p->dev.H, nbc), lds, st));
  return TB_OK;
}

// ------------------------------------------------------------ band-limited plans (band.h)
// TEXBIAS_BAND=0 or tb_set_band_plans(0) forces the full-spectrum passes for every program.
static bool g_band = [] {
  const char* e = std::getenv("TEXBIAS_BAND");
  return !(e && e[0] == '0');
}();
// Spike-only programs (plane waves, k-space spikes) in closed form (point.h); TEXBIAS_POINT=0 or
// tb_set_point_plans(0): the full-spectrum passes.
static bool g_point = [] {
  const char* e = std::getenv("TEXBIAS_POINT");
  return !(e && e[0] == '0');
}();
// Wrap-only programs on the separable route (wrap.h); TEXBIAS_WRAP=0 or tb_set_wrap_plans(0): the
// full-spectrum passes.
static bool g_wrap = [] {
  const char* e = std::getenv("TEXBIAS_WRAP");
  return !(e && e[0] == '0');
}();
// Pass C' synthesis in split f16 on the matrix cores (k_band_inv16) when the launch's V rows fit
// (band columns + every sample's points <= 64); TEXBIAS_INV16=0 or tb_set_band_inv16(0): the f32 kernel.
static bool g_inv16 = [] {
  const char* e = std::getenv("TEXBIAS_INV16");
  return !(e && e[0] == '0');
}();
// measurement only: TEXBIAS_BAND_DIAG=0xIIFF skips stages of A' (FF) / C' (II); results invalid
static int g_band_diag = [] {
  const char* e = std::getenv("TEXBIAS_BAND_DIAG");
  return e ? (int)std::strtol(e, nullptr, 0) : 0;
}();

// A low-pass op that zeroes every coefficient outside a box around DC (all channels).
static bool band_is_lowpass(const tb_op& op) {
  if (op.chan != -1) return false;
  if (op.kind == TB_OP_DISK) return op.i[1] == 0;       // inside_off = False: keeps the disk
  if (op.kind == TB_OP_GIBBS) return true;
  if (op.kind == TB_OP_LAYER) return op.l == 0;          // alpha known on the host
  return false;
}
// The op's own keep-test on a total squared distance (apply_ops' arithmetic, fft_core.h).
static bool band_keeps(const tb_op& op, int64_t sq) {
  if (op.kind == TB_OP_DISK) return op.i[0] ? (sq < op.l) : ((float)sq < op.f[0]);
  if (op.kind == TB_OP_GIBBS) return sq <= op.l;
  return layer_in(op, (int)sq);
}
// Largest |signed frequency| on an axis of length n that the op can keep, the other axes at their
// smallest term `rest` (disk: 0; Gibbs / layer: 0 for odd n, 1 for even n -- the (n-1)/2 centre);
// `half`: the D axis, stored kd in [0, n/2] only.  -1 when no coefficient survives.
static int band_extent(const tb_op& op, int n, int64_t rest, bool half) {
  int K = -1;
  const int kmax = half ? n / 2 : n - 1;
  for (int k = 0; k <= kmax; ++k) {
    const AxisGeo g = axis_geo(k, n);
    const int64_t term = op.kind == TB_OP_DISK ? g.dsq : (g.ef < g.en ? g.ef : g.en);
    if (!band_keeps(op, term + rest)) continue;
    const int m = (half || k <= (n - 1) / 2) ? k : n - k;
    K = m > K ? m : K;
  }
  return K;
}
static int band_minterm(const tb_op& op, int n) { return (op.kind == TB_OP_DISK || (n & 1)) ? 0 : 1; }

// Box of one sample's program (false: no low-pass, the full passes run).
static bool band_box(const tb_sample_ops& so, int H, int W, int D, int& KH, int& KW, int& KD) {
  for (int o = 0; o < so.n; ++o) {
    const tb_op& op = so.op[o];
    if (!band_is_lowpass(op)) continue;
    const int mh = band_minterm(op, H), mw = band_minterm(op, W), md = band_minterm(op, D);
    KH = band_extent(op, H, mw + md, false);
    KW = band_extent(op, W, mh + md, false);
    KD = band_extent(op, D, mh + mw, true);
    if (KH < 0 || KW < 0 || KD < 0) KH = KW = KD = 0;  // nothing kept: the box degenerates to DC
    return true;
  }
  return false;
}
// Stored (kd <= D/2) coefficients of the program's spikes that fall outside the box.
static bool band_points(const tb_sample_ops& so, int H, int W, int D, int KH, int KW, int KD, BandSamplePts& sp) {
  sp.n = 0;
  for (int o = 0; o < so.n; ++o) {
    const tb_op& op = so.op[o];
    if (op.kind != TB_OP_SPIKE) continue;
    const int f[2][3] = {{op.i[0], op.i[1], op.i[2]},
                         {(H - op.i[0]) % H, (W - op.i[1]) % W, (D - op.i[2]) % D}};
    for (int q = 0; q < 2; ++q) {
      const int kh = f[q][0], kw = f[q][1], kd = f[q][2];
      if (kd > D / 2) continue;
      const int mh = kh <= (H - 1) / 2 ? kh : H - kh, mw = kw <= (W - 1) / 2 ? kw : W - kw;
      if (mh <= KH && mw <= KW && kd <= KD) continue;  // inside the box: handled by pass B'
      bool dup = false;
      for (int j = 0; j < sp.n; ++j) dup |= sp.p[j].kh == kh && sp.p[j].kw == kw && sp.p[j].kd == kd;
      if (dup) continue;
      if (sp.n == BAND_MAX_PTS) return false;
      sp.p[sp.n].kh = (int16_t)kh;
      sp.p[sp.n].kw = (int16_t)kw;
      sp.p[sp.n].kd = (int16_t)kd;
      sp.p[sp.n].pad = 0;
      ++sp.n;
    }
  }
  return true;
}

// Band geometry shared by samples [s0, s1) of `ops`, or false when the run must use the full passes.
static bool band_plan(const tb_plan* p, const tb_sample_ops* ops, int s0, int s1, int y_pad, size_t ws_bytes, int bcn,
                      BandGeo& g, BandSamplePts* sp) {
  const int H = p->dev.H, W = p->dev.W, D = p->dev.D;
  int KH = 0, KW = 0, KD = 0, npt = 0;
  for (int s = s0; s < s1; ++s) {
    int kh, kw, kd;
    if (!band_box(ops[s], H, W, D, kh, kw, kd)) return false;
    KH = kh > KH ? kh : KH;
    KW = kw > KW ? kw : KW;
    KD = kd > KD ? kd : KD;
  }
  for (int s = s0; s < s1; ++s) {
    if (!band_points(ops[s], H, W, D, KH, KW, KD, sp[s - s0])) return false;
    npt = sp[s - s0].n > npt ? sp[s - s0].n : npt;
  }
  g.KH = KH;
  g.KW = KW;
  g.NDk = KD + 1;
  g.NW = 2 * KW + 1;
  g.ncol = g.NW * g.NDk;
  g.KS = g.NDk + npt;
  g.NCOL = 32 * ((D / 2 + 1 + 31) / 32);
  int ptot = 0;
  for (int s = s0; s < s1; ++s) ptot += sp[s - s0].n;
  g.cat = (g_inv16 && g.NDk + ptot <= 32) ? 1 : 0;
  g.PT = g.cat ? ptot : 0;
  g.NTD = (D + y_pad + 31) / 32;
  if (D > BAND_MAX_D || 2 * KH + 1 > H || 2 * KW + 1 > W || g.NDk > BAND_MAX_NDK || KW >= 32 || KH > BAND_MAX_KH)
    return false;
  if (g.ncol > BAND_MAX_ZCOL || W > 1024 || band_hc_lds(H, KH) > 160000) return false;
  if (2 * g.KS > 64 || g.KS > 32) return false;  // pass C' holds V in at most two 32-row MFMA tiles
  // worth it only when the box is a small part of the half spectrum
  if ((double)(2 * KH + 1) * g.ncol * 4.0 > (double)H * W * (D / 2 + 1)) return false;
  if (g.cat && band_inv16_carve(g, W).total > 160000) {
    g.cat = 0;
    g.PT = 0;
  }
  if (band_lds_fwd(g, W, D, false) > 160000 || band_lds_fwd(g, W, D, true) > 160000 ||
      (!g.cat && band_inv_carve(g, W, D).total > 160000))
    return false;
  if (band_ws(g, H, bcn).total > ws_bytes) return false;
  return true;
}

enum { RUN_COPY = 0, RUN_FULL = 1, RUN_BAND = 2, RUN_POINT = 3, RUN_WRAP = 4 };

// The run [s0, s1) takes the separable wrap route: every program wrap-only (with the same alpha
// product when D is odd: one circulant table per launch), a shape the route takes, room for its partials.
static bool wrap_run(const tb_plan* p, const tb_sample_ops* ops, int s, int y_pad, size_t ws_bytes, float* alpha) {
  if (!g_wrap || ws_bytes < tb::wrap_ws_bytes()) return false;
  if (!tb::wrap_shape_ok(p->dev.H, p->dev.W, p->dev.D, y_pad)) return false;
  if ((p->dev.D & 1) && !p->wrapq) return false;
  return tb::wrap_program(ops[s], alpha);
}

static int run_wrap(const tb_plan* p, const float* x, const int64_t* xs, float* y, const int64_t* ys, int y_pad,
                    char* ws, int b0, int nb, int C, const tb_sample_ops* ops, uint32_t* minmax, hipStream_t st) {
  const int H = p->dev.H, W = p->dev.W, D = p->dev.D;
  tb::WrapArgs a;
  std::memset(&a, 0, sizeof(a));
  a.H = H, a.W = W, a.D = D;
  a.x = x, a.xsbc = xs[0], a.xsh = xs[1], a.xsw = xs[2];
  a.y = y, a.ysbc = ys[0], a.ysh = ys[1], a.ysw = ys[2];
  a.ypad = y_pad, a.bc0 = b0 * C, a.C = C, a.nbc = nb * C;
  a.q = p->wrapq;
  a.mm = minmax;
  a.mmp = reinterpret_cast<float2*>(ws);
  a.cnt = reinterpret_cast<uint32_t*>(ws + (size_t)tb::WRAP_MAX_WG * TB_MAX_BATCH * 8);
  // 16-B loads: contiguous rows and 16-B aligned role chunks (every row start of a 4-row chunk,
  // W/2 rows apart); 16-B stores: every output row start 16-B aligned
  const bool xal = (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (xs[0] & 3) == 0 && (xs[1] & 3) == 0;
  const bool vld = (D & 1) ? (xal && xs[2] == D && (((int64_t)(W / 2) * D) & 3) == 0)
                           : (xal && (xs[2] & 3) == 0);
  const bool vst = (reinterpret_cast<uintptr_t>(y) & 15) == 0 && (ys[0] & 3) == 0 && (ys[1] & 3) == 0 && (ys[2] & 3) == 0;
  a.vec = (vld ? 1 : 0) | (vst ? 2 : 0);
  float alpha[TB_MAX_BATCH];
  for (int i = 0; i < nb; ++i) tb::wrap_program(ops[b0 + i], &alpha[i]);
  const double vox = (double)nb * C * H * W;
  Timer t(2, st, vox * (D + D + y_pad) * 4.0, (D & 1) ? "k_wrap_dgemm" : "k_wrap_even");
  TB_HIP(tb::launch_wrap(a, alpha, nb, p->ncu, st));
  return TB_OK;
}

template <int RA, int RB>
static int run_full(const tb_plan* p, const float* x, const int64_t* xs, float* y, const int64_t* ys, int y_pad, cf* S,
                    int b0, int nb, int C, const tb_sample_ops* ops, uint32_t* minmax, hipStream_t st) {
  const int H = p->dev.H, W = p->dev.W, D = p->dev.D;
  const int Dh = D / 2 + 1;
  const float scale = (float)(1.0 / ((double)H * (double)W * (double)D));
  const int T = pick_tile(H, p->lds_max);
  const int ntiles = (W * Dh + T - 1) / T;
  const size_t lds_b = (size_t)tile_geo(H, T).total_cf * sizeof(cf);
  const size_t lds_s = (size_t)slab_geo(W, D).total_cf * sizeof(cf);
  BatchOps bo;
  std::memset(&bo, 0, sizeof(bo));
  for (int i = 0; i < nb; ++i) bo.s[i] = ops[b0 + i];
  // A -> B -> C per chunk of channel-volumes: a chunk's half spectrum is re-read by B and C while
  // it is still in the 256 MiB Infinity Cache (chunk_bc(); 0 = the whole group in one chain)
  const int nbc = nb * C;
  const int g = chunk_bc(p) > 0 ? chunk_bc(p) : nbc;
  for (int c0 = 0; c0 < nbc; c0 += g) {
    const int ng = (nbc - c0) < g ? (nbc - c0) : g;
    const int bc0 = b0 * C + c0;
    const double vox = (double)ng * H * W * D, spec = (double)ng * H * W * Dh * 8.0;
    const bool half = use_half(p);
    {
      Timer t(0, st, vox * 4.0 + spec, half ? "k_slab_fwd_half" : use_ct_slab(p) ? "k_slab_fwd_ct16" : "k_slab_fwd");
      if (half) {
        SlabFwdArgs a{p->dev, x, xs[0], xs[1], xs[2], S, bc0, ng};
        TB_HIP(tb::launch_slab_fwd_half(a, st));
      } else {
        const int rc = launch_slab_fwd<RA>(p, x, xs, S, bc0, ng, st);
        if (rc) return rc;
      }
    }
    {
      Timer t(1, st, 2.0 * spec,
              half ? "k_kspace_half"
              : (g_compiled_plans && p->ct_tile)
                  ? (tb::kspace_ct_persistent(W * Dh) ? "k_kspace_ct2p" : "k_kspace_ct2")
                  : "k_kspace");
      if (half) {
        KspaceArgs ka{p->dev, S, bc0, C, 32, c0, bo, ng};
        TB_HIP(tb::launch_kspace_half(ka, p->ncu, st));
      } else if (g_compiled_plans && p->ct_tile) {
        const int Tc = tb::kspace_ct_tile(W * Dh);
        KspaceArgs ka{p->dev, S, bc0, C, Tc, c0, bo, ng};
        TB_HIP(tb::launch_kspace_ct(ka, dim3((W * Dh + Tc - 1) / Tc, ng), p->ncu, st));
      } else {
        KspaceArgs ka{p->dev, S, bc0, C, T, c0, bo, ng};
        TB_HIP(launch_kspace<RB>(ka, dim3(ntiles, ng), lds_b, st));
      }
    }
    {
      Timer t(2, st, spec + (double)ng * H * W * (D + y_pad) * 4.0,
              half ? "k_slab_inv_half" : use_ct_slab(p) ? "k_slab_inv_ct" : "k_slab_inv");
      SlabInvArgs ia{p->dev, S, y, ys[0], ys[1], ys[2], y_pad, bc0, C, scale, minmax, ng};
      if (half)
        TB_HIP(tb::launch_slab_inv_half(ia, st));
      else if (use_ct_slab(p))
        TB_HIP(tb::launch_slab_inv_ct(ia, p->ncu, st));
      else
        TB_HIP(launch_slab_inv<RA>(ia, dim3(H, ng), lds_s, st));
    }
  }
  return TB_OK;
}

static int run_band(const tb_plan* p, const float* x, const int64_t* xs, float* y, const int64_t* ys, int y_pad,
                    char* ws, int bcn_total, int b0, int nb, int C, const tb_sample_ops* ops, const BandGeo& g,
                    const BandSamplePts* sp, uint32_t* minmax, hipStream_t st) {
  const int H = p->dev.H, W = p->dev.W, D = p->dev.D;
  const BandWs wl = band_ws(g, H, bcn_total);
  cf* P = reinterpret_cast<cf*>(ws + wl.off_P);
  float4* AB = reinterpret_cast<float4*>(ws + wl.off_AB);
  cf* pts = reinterpret_cast<cf*>(ws + wl.off_pts);
  const int nbc = nb * C, bc0 = b0 * C;
  const double pbytes = (double)nbc * H * g.ncol * 8.0, abytes = (double)nbc * (g.KH + 1) * g.ncol * 16.0;
  tb::FwdSplit split{};
  {
    Timer t(0, st, (double)nbc * H * W * D * 4.0 + pbytes, "k_band_fwd");
    BandFwdArgs fa{p->dev, x, xs[0], xs[1], xs[2], P, bc0, nbc, g, g_band_diag & 0xff, p->tbt};
    // 16-B vector strips: contiguous rows, and 16-B aligned strips where the compiled even-D staging needs them
    const bool al = (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (xs[0] & 3) == 0 && (xs[1] & 3) == 0;
    fa.vec = xs[2] == D && ((D & 1) || al || !tb::band_fwd_use_ct(D, g.NDk <= 16 ? 1 : 2));
    fa.tbt16 = p->tbt16;
    TB_HIP(tb::launch_band_fwd(fa, p->ncu, st));
    split = fa.split;
  }
  {
    Timer t(1, st, pbytes + abytes, "k_band_hcol");
    BandMidArgs ma;
    std::memset(&ma, 0, sizeof(ma));
    ma.pl = p->dev;
    ma.P = P;
    ma.AB = AB;
    ma.pts = pts;
    ma.M2F = reinterpret_cast<float*>(ws + wl.off_m2f);
    ma.scale = (float)(1.0 / ((double)H * (double)W * (double)D));
    ma.bc0 = bc0;
    ma.C = C;
    ma.cofs = 0;
    ma.nbc = nbc;
    ma.g = g;
    ma.split = split;
    int p0 = 0;
    for (int i = 0; i < nb; ++i) {
      ma.sp[i] = sp[i];
      ma.ops.s[i] = ops[b0 + i];
      ma.p0[i] = p0;
      for (int j = 0; j < sp[i].n; ++j) ma.pkd[p0 + j] = sp[i].p[j].kd;
      p0 += sp[i].n;
    }
    ma.T16 = ws + wl.off_t16;
    ma.tds = p->tds;
    ma.cnt = reinterpret_cast<uint32_t*>(ws + wl.off_cnt);
    ma.mm = g.cat ? minmax : nullptr;
    TB_HIP(tb::launch_band_mid(ma, st));
  }
  {
    // the events bracket k_band_inv16 (with the per-sample min/max keys from its last workgroup) or
    // k_band_inv alone (k_band_minmax after it runs untimed): the kernel's duration, as rocprofv3 reports it
    Timer t(2, st, abytes + (double)nbc * H * W * (D + y_pad) * 4.0, g.cat ? "k_band_inv16" : "k_band_inv");
    BandInvArgs ia;
    std::memset(&ia, 0, sizeof(ia));
    ia.pl = p->dev;
    ia.M2F = reinterpret_cast<float*>(ws + wl.off_m2f);
    ia.AB = AB;
    ia.pts = pts;
    ia.y = y;
    ia.sbc = ys[0];
    ia.sh = ys[1];
    ia.sw = ys[2];
    ia.ypad = y_pad;
    ia.bc0 = bc0;
    ia.C = C;
    ia.cofs = 0;
    ia.nbc = nbc;
    ia.scale = (float)(1.0 / ((double)H * (double)W * (double)D));
    ia.mm = minmax;
    ia.mmp = reinterpret_cast<float2*>(ws + wl.off_mmp);
    ia.tds = p->tds;
    ia.T16 = ws + wl.off_t16;
    ia.g = g;
    ia.diag = (g_band_diag >> 8) & 0xffff;
    ia.cnt = g.cat ? reinterpret_cast<uint32_t*>(ws + wl.off_cnt) : nullptr;
    for (int i = 0; i < nb; ++i) ia.sp[i] = sp[i];
    TB_HIP(tb::launch_band_inv(ia, p->ncu, st));
  }
  // the split-f16 C' writes the keys from its last workgroup; the f32 C' leaves them to k_band_minmax
  if (minmax && !g.cat) TB_HIP(tb::launch_band_minmax(reinterpret_cast<float2*>(ws + wl.off_mmp), minmax, b0 * C, C, nbc, H, W, st));
  return TB_OK;
}

// full-spectrum route of a plan the mixed-radix passes do not take (tb_plan::generic)
static int run_generic(const tb_plan* p, const float* x, const int64_t* xs, float* y, const int64_t* ys, int y_pad,
                       void* ws, int b0, int nb, int C, const tb_sample_ops* ops, uint32_t* minmax, hipStream_t st) {
  BatchOps bo;
  std::memset(&bo, 0, sizeof(bo));
  for (int i = 0; i < nb; ++i) bo.s[i] = ops[b0 + i];
  const double vox = (double)nb * C * p->dev.H * p->dev.W * p->dev.D;
  Timer t(1, st, vox * (4.0 + 2.0 * 16.0 * 6.0 + 16.0 + 4.0), "k_gen_dft");
  const GenLaunch g{p->dev, x, xs, y, ys, static_cast<cf*>(ws), y_pad, b0 * C, C, nb * C, minmax, &bo};
  TB_HIP(tb::launch_gen_filter(g, st));
  return TB_OK;
}

// Samples per chain of the closed-form route's three launches (0 = the whole launch group): per-sample chains would let k_point_apply re-read a 142 MB sample from the Infinity
// Cache, but cost more in launches and smaller grids than they saved.
static int point_chunk(const tb_plan* p, int C) {
  (void)p;
  (void)C;
  return 0;  // measured: one sample per chain 0.240 vs 0.213 ms per C3 step (planes)
}

static int run_point(const tb_plan* p, const float* x, const int64_t* xs, float* y, const int64_t* ys, int y_pad,
                     char* ws, int b0, int nb, int C, const tb_sample_ops* ops, uint32_t* minmax,
                     hipStream_t st) {
  const int H = p->dev.H, W = p->dev.W, D = p->dev.D;
  const int cs = point_chunk(p, C) > 0 ? point_chunk(p, C) : nb;
  for (int s0 = 0; s0 < nb; s0 += cs) {
    const int ns = nb - s0 < cs ? nb - s0 : cs, sb = b0 + s0;
    const int nbc = ns * C;
    tb::PointArgs a;
    std::memset(&a, 0, sizeof(a));
    a.H = H, a.W = W, a.D = D;
    a.x = x, a.xsbc = xs[0], a.xsh = xs[1], a.xsw = xs[2];
    a.y = y, a.ysbc = ys[0], a.ysh = ys[1], a.ysw = ys[2];
    a.ypad = y_pad, a.bc0 = sb * C, a.C = C, a.nbc = nbc, a.mm = minmax;
    const tb::PointWs wl = tb::point_ws(nbc);
    a.part = reinterpret_cast<double*>(ws + wl.part);
    a.delta = reinterpret_cast<float*>(ws + wl.delta);
    a.mmp = reinterpret_cast<float2*>(ws + wl.mmp);
    a.cnt = reinterpret_cast<uint32_t*>(ws + wl.cnt);
    a.namax = 1;
    for (int i = 0; i < ns; ++i) {
      a.ops.s[i] = ops[sb + i];
      for (int c = 0; c < C; ++c) {
        int n = 0;
        for (int o = 0; o < ops[sb + i].n; ++o) n += ops[sb + i].op[o].chan < 0 || ops[sb + i].op[o].chan == c;
        a.namax = n > a.namax ? n : a.namax;
      }
    }
    tb::point_grid(a, p->ncu);
    const double vox = (double)nbc * H * W * D;
    {
      Timer t(0, st, vox * 4.0, "k_point_dft");
      TB_HIP(tb::launch_point(a, st, 0));
    }
    {
      Timer t(1, st, (double)nbc * a.parts * TB_MAX_OPS * 16.0, "k_point_delta");
      TB_HIP(tb::launch_point(a, st, 1));
    }
    {
      Timer t(2, st, vox * 4.0 + (double)nbc * H * W * (D + y_pad) * 4.0, "k_point_apply");
      TB_HIP(tb::launch_point(a, st, 2));
    }
  }
  return TB_OK;
}

static int run_copy(const tb_plan* p, const float* x, const int64_t* xs, float* y, const int64_t* ys, int y_pad, int b0,
                    int nb, int C, uint32_t* minmax, hipStream_t st) {
  const int H = p->dev.H, W = p->dev.W, D = p->dev.D;
  const int nbc = nb * C;
  Timer t(2, st, (double)nbc * H * W * (2.0 * D + y_pad) * 4.0, "k_copy_pad");
  CopyArgs ca{x, xs[0], xs[1], xs[2], y, ys[0], ys[1], ys[2], H, W, D, y_pad, b0 * C, C, nbc, minmax};
  TB_HIP(tb::launch_copy_pad(ca, st));
  return TB_OK;
}

// TB_OP_MASK / TB_OP_CMASK ops carry a device address the kernels dereference: checked here, before any launch
static bool mask_ops_ok(const tb_plan* p, const tb_sample_ops* ops, int B, int C) {
  for (int b = 0; b < B; ++b)
    for (int o = 0; o < ops[b].n && o < TB_MAX_OPS; ++o) {
      const tb_op& op = ops[b].op[o];
      if (op.kind != TB_OP_MASK && op.kind != TB_OP_CMASK) continue;
      if (op.l == 0 || op.i[1] != p->dev.W || op.i[2] != p->dev.D || (op.i[0] != 1 && op.i[0] != C)) return false;
    }
  return true;
}

template <int RA, int RB>
static int kspace_filter(const tb_plan* p, const float* x, const int64_t* xs, float* y, const int64_t* ys, int y_pad,
                         void* ws, size_t ws_bytes, int B, int C, const tb_sample_ops* ops, uint32_t* minmax,
                         void* stream) {
  if (!p || !x || !y || !xs || !ys || !ops || B < 1 || C < 1 || y_pad < 0) return TB_ERR_INVALID_ARG;
  if (ws_bytes < tb_workspace_bytes(p, B * C) || !ws) return TB_ERR_WORKSPACE;
  for (int b = 0; b < B; ++b)
    if (ops[b].n < 0 || ops[b].n > TB_MAX_OPS) return TB_ERR_INVALID_ARG;
  if (!mask_ops_ok(p, ops, B, C)) return TB_ERR_INVALID_ARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  // Runs of consecutive samples with the same route, in launch groups of <= TB_MAX_BATCH samples
  // (the op programs travel in the kernel arguments): empty programs are copied through (the
  // reference returns the input untouched), low-pass programs take the band passes A'/B'/C',
  // the rest the full-spectrum passes A/B/C.  Routes are planned first: the band passes write
  // their samples' min/max keys outright, the others accumulate them atomically from a reset.
  struct Run {
    int s0, s1, route;
    BandGeo g;
    BandSamplePts sp[TB_MAX_BATCH];
  };
  std::vector<Run> runs;
  bool atomic_keys = false;
  for (int b0 = 0; b0 < B; b0 += TB_MAX_BATCH) {
    const int nb = (B - b0) < TB_MAX_BATCH ? (B - b0) : TB_MAX_BATCH;
    int i = 0;
    while (i < nb) {
      float al0 = 0.f, al = 0.f;
      auto route = [&](int s, float* alpha) {
        return ops[s].n == 0 ? RUN_COPY : (wrap_run(p, ops, s, y_pad, ws_bytes, alpha) ? RUN_WRAP : RUN_FULL);
      };
      Run run;
      run.route = route(b0 + i, &al0);
      int j = i + 1;
      // odd D: one circulant table per launch (k_wrap_dgemm builds it from one alpha); even D: k_wrap_even
      // carries every sample's 2-tap weights, so mixed alphas share the launch
      while (j < nb && route(b0 + j, &al) == run.route && (run.route != RUN_WRAP || al == al0 || !(p->dev.D & 1))) ++j;
      run.s0 = b0 + i;
      run.s1 = b0 + j;
      if (run.route == RUN_FULL && g_point && ws_bytes >= tb::point_ws(B * C).total &&
          tb::point_strides_ok(p->dev.H, p->dev.W, p->dev.D, y_pad, xs, ys)) {
        bool pt = true;
        for (int s = run.s0; s < run.s1 && pt; ++s) pt = tb::point_program(ops[s], p->dev.H, p->dev.W, p->dev.D);
        if (pt) run.route = RUN_POINT;
      }
      if (run.route == RUN_FULL && g_band && band_plan(p, ops, run.s0, run.s1, y_pad, ws_bytes, B * C, run.g, run.sp))
        run.route = RUN_BAND;
      atomic_keys |= run.route == RUN_COPY || run.route == RUN_FULL;  // the other routes write their keys outright
      runs.push_back(run);
      i = j;
    }
  }
  if (minmax && atomic_keys) {
    hipLaunchKernelGGL(k_minmax_init, dim3((B + 255) / 256), dim3(256), 0, st, minmax, B);
    TB_HIP(hipGetLastError());
  }
  for (const Run& run : runs) {
    const int nb = run.s1 - run.s0;
    int rc = TB_OK;
    if (run.route == RUN_COPY)
      rc = run_copy(p, x, xs, y, ys, y_pad, run.s0, nb, C, minmax, st);
    else if (run.route == RUN_WRAP)
      rc = run_wrap(p, x, xs, y, ys, y_pad, static_cast<char*>(ws), run.s0, nb, C, ops, minmax, st);
    else if (run.route == RUN_POINT)
      rc = run_point(p, x, xs, y, ys, y_pad, static_cast<char*>(ws), run.s0, nb, C, ops, minmax, st);
    else if (run.route == RUN_BAND)
      rc = run_band(p, x, xs, y, ys, y_pad, static_cast<char*>(ws), B * C, run.s0, nb, C, ops, run.g, run.sp, minmax,
                    st);
    else if (p->generic)
      rc = run_generic(p, x, xs, y, ys, y_pad, ws, run.s0, nb, C, ops, minmax, st);
    else
      rc = run_full<RA, RB>(p, x, xs, y, ys, y_pad, static_cast<cf*>(ws), run.s0, nb, C, ops, minmax, st);
    if (rc) return rc;
  }
  return TB_OK;
}

template <int RA, int RB>
static int kspace_stats(const tb_plan* p, const float* x, const int64_t* xs, void* ws, size_t ws_bytes, int B,
                             int C, const tb_sample_ops* ops, double* out, void* stream) {
  if (!p || !x || !xs || !ops || !out || B < 1 || C < 1) return TB_ERR_INVALID_ARG;
  if (ws_bytes < tb_workspace_bytes(p, B * C) || !ws) return TB_ERR_WORKSPACE;
  if (!mask_ops_ok(p, ops, B, C)) return TB_ERR_INVALID_ARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  cf* S = static_cast<cf*>(ws);
  const int H = p->dev.H, W = p->dev.W, D = p->dev.D;
  const int T = pick_tile(H, p->lds_max);
  const int ntiles = (W * (D / 2 + 1) + T - 1) / T;
  const size_t lds_b = (size_t)tile_geo(H, T).total_cf * sizeof(cf);
  int rc = TB_OK;
  TB_HIP(hipMemsetAsync(out, 0, sizeof(double) * B * C, st));
  if (p->generic) {
    for (int b0 = 0; b0 < B; b0 += TB_MAX_BATCH) {
      const int nb = (B - b0) < TB_MAX_BATCH ? (B - b0) : TB_MAX_BATCH;
      BatchOps bo;
      std::memset(&bo, 0, sizeof(bo));
      for (int i = 0; i < nb; ++i) bo.s[i] = ops[b0 + i];
      const GenLaunch g{p->dev, x, xs, nullptr, nullptr, S, 0, b0 * C, C, nb * C, nullptr, &bo};
      TB_HIP(tb::launch_gen_logabs(g, out, st));
    }
    return TB_OK;
  }
  for (int b0 = 0; b0 < B; b0 += TB_MAX_BATCH) {
    const int nb = (B - b0) < TB_MAX_BATCH ? (B - b0) : TB_MAX_BATCH;
    BatchOps bo;
    std::memset(&bo, 0, sizeof(bo));
    for (int i = 0; i < nb; ++i) bo.s[i] = ops[b0 + i];
    rc = launch_slab_fwd<RA>(p, x, xs, S, b0 * C, nb * C, st);
    if (rc) return rc;
    StatsArgs sa{p->dev, S, b0 * C, C, T, 0, out, bo};
    TB_HIP(launch_kspace_stats<RB>(sa, dim3(ntiles, nb * C), lds_b, st));
  }
  return TB_OK;
}

// ------------------------------------------------------------ mask gradient (maskgrad.h)
// Tile of the mask-gradient pass: half of pass B's width (the x and g tiles share one pass-B tile of
// LDS), narrowed until a workgroup's register slots hold its coefficients.
static int maskgrad_tile(const tb_plan* p) {
  int T = pick_tile(p->dev.H, p->lds_max) / 2;
  if (T < 1) T = 1;
  while (T > 1 && p->dev.H * T > MG_MAX_TILE) --T;
  return T;
}
// The element-wise fallback also takes a plan whose single column exceeds the register slots or the
// LDS, and one whose volume offsets pass 32 bits.
static bool maskgrad_generic(const tb_plan* p) {
  const int H = p->dev.H;
  return p->generic || H > MG_MAX_TILE || (size_t)tile_geo(H, 2).total_cf * sizeof(cf) > (size_t)p->lds_max ||
         (int64_t)H * p->dev.W * (p->dev.D / 2 + 1) >= (1LL << 31);
}

size_t tb_mask_grad_workspace_bytes(const tb_plan* plan, int bc) {
  if (!plan || bc < 0) return 0;
  const int H = plan->dev.H, W = plan->dev.W, D = plan->dev.D;
  if (maskgrad_generic(plan)) return gen_maskgrad_workspace_bytes(H, W, D, bc);
  return (size_t)2 * bc * H * W * (D / 2 + 1) * sizeof(cf);
}

template <int RA, int RB>
static int kspace_mask_grad(const tb_plan* p, const float* x, const int64_t* xs, const float* g, const int64_t* gs,
                            float* dM, int Cm, void* ws, int B, int C, hipStream_t st, int cplx) {
  const int H = p->dev.H, W = p->dev.W, D = p->dev.D, Dh = D / 2 + 1;
  const double scale = 1.0 / ((double)H * (double)W * (double)D);
  const double dm_bytes = (double)Cm * H * W * D * (cplx ? 8.0 : 4.0);
  if (maskgrad_generic(p)) {
    for (int b0 = 0; b0 < B; b0 += TB_MAX_BATCH) {
      const int nb = (B - b0) < TB_MAX_BATCH ? (B - b0) : TB_MAX_BATCH;
      const double vox = (double)nb * C * H * W * D;
      cf* b0p = static_cast<cf*>(ws);
      cf* b1p = b0p + (size_t)nb * C * H * W * D;
      cf* b2p = b1p + (size_t)nb * C * H * W * D;
      {
        // per voxel: 4 B read and 8 B written by the load, 16 B per axis; twice
        Timer t(0, st, 2.0 * vox * 60.0, "k_gen_dft");
        const GenLaunch gx{p->dev, x, xs, nullptr, nullptr, b1p, 0, b0 * C, C, nb * C, nullptr, nullptr};
        TB_HIP(tb::launch_gen_spectrum(gx, st));
        const GenLaunch gg{p->dev, g, gs, nullptr, nullptr, b0p, 0, b0 * C, C, nb * C, nullptr, nullptr};
        TB_HIP(tb::launch_gen_spectrum(gg, st));
      }
      {
        Timer t(1, st, 2.0 * (double)nb * C * H * W * Dh * 8.0 + dm_bytes, "k_gen_maskgrad");
        TB_HIP(tb::launch_gen_maskgrad(p->dev, b2p, b1p, dM, C, nb, Cm, b0 > 0 ? 1 : 0, st, cplx));
      }
    }
    return TB_OK;
  }
  const int T = maskgrad_tile(p);
  const int ntiles = (W * Dh + T - 1) / T;
  const size_t lds = (size_t)tile_geo(H, 2 * T).total_cf * sizeof(cf);
  cf* Sx = static_cast<cf*>(ws);
  cf* Sg = Sx + (size_t)B * C * H * W * Dh;
  for (int b0 = 0; b0 < B; b0 += TB_MAX_BATCH) {
    const int nb = (B - b0) < TB_MAX_BATCH ? (B - b0) : TB_MAX_BATCH;
    const double vox = (double)nb * C * H * W * D, spec = (double)nb * C * H * W * Dh * 8.0;
    {
      Timer t(0, st, 2.0 * (vox * 4.0 + spec), use_ct_slab(p) ? "k_slab_fwd_ct16" : "k_slab_fwd");
      int rc = launch_slab_fwd<RA>(p, x, xs, Sx, b0 * C, nb * C, st);
      if (rc) return rc;
      rc = launch_slab_fwd<RA>(p, g, gs, Sg, b0 * C, nb * C, st);
      if (rc) return rc;
    }
    {
      Timer t(1, st, 2.0 * spec + dm_bytes, cplx ? "k_kspace_cmaskgrad" : "k_kspace_maskgrad");
      const MaskGradArgs ma{p->dev, Sx, Sg, dM, b0 * C, C, nb, Cm, T, b0 > 0 ? 1 : 0, (float)scale, cplx};
      TB_HIP(launch_kspace_maskgrad<RB>(ma, dim3(ntiles, Cm), lds, st));
    }
  }
  return TB_OK;
}

static int mask_grad_entry(const tb_plan* p, const float* x, const int64_t* xs, const float* g, const int64_t* gs,
                           float* dM, int Cm, void* ws, size_t ws_bytes, int B, int C, void* stream, int cplx) {
  if (!p || !x || !xs || !g || !gs || !dM || B < 1 || C < 1 || (Cm != 1 && Cm != C)) return TB_ERR_INVALID_ARG;
  if (!ws || ws_bytes < tb_mask_grad_workspace_bytes(p, B * C)) return TB_ERR_WORKSPACE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define TB_ARGS p, x, xs, g, gs, dM, Cm, ws, B, C, st, cplx
  if (p->rset_wd == RS_SMALL)
    return p->rset_h == RS_SMALL ? kspace_mask_grad<RS_SMALL, RS_SMALL>(TB_ARGS) : kspace_mask_grad<RS_SMALL, RS_ALL>(TB_ARGS);
  return p->rset_h == RS_SMALL ? kspace_mask_grad<RS_ALL, RS_SMALL>(TB_ARGS) : kspace_mask_grad<RS_ALL, RS_ALL>(TB_ARGS);
#undef TB_ARGS
}

int tb_kspace_mask_grad_f32(const tb_plan* p, const float* x, const int64_t* xs, const float* g, const int64_t* gs,
                            float* dM, int Cm, void* ws, size_t ws_bytes, int B, int C, void* stream) {
  return mask_grad_entry(p, x, xs, g, gs, dM, Cm, ws, ws_bytes, B, C, stream, 0);
}

int tb_kspace_cmask_grad_f32(const tb_plan* p, const float* x, const int64_t* xs, const float* g, const int64_t* gs,
                             void* dM, int Cm, void* ws, size_t ws_bytes, int B, int C, void* stream) {
  return mask_grad_entry(p, x, xs, g, gs, static_cast<float*>(dM), Cm, ws, ws_bytes, B, C, stream, 1);
}

// ------------------------------------------------------------ radial profiles (radial.h)
// Fused route: [S_x][S_g (gradient)][partials of the shell reduction].  Composed route (plans of
// maskgrad_generic(), or tb_set_radial_fused(0)): [workspace of the mask gradient][dense dM][partials of
// the dense bin reduction].  tb_radial_workspace_bytes covers both, so the switch may change between the
// query and the call.
static bool g_radial_fused = true;

static size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// dense bin reduction over N elements per channel: chunks of RB_CHUNK elements, at most 1024 units
struct RadialBinGrid {
  int cpu, units;
};
static RadialBinGrid radial_bin_grid(int64_t N) {
  const int64_t chunks = (N + tb::RB_CHUNK - 1) / tb::RB_CHUNK;
  RadialBinGrid g;
  g.cpu = (int)((chunks + 1023) / 1024);
  g.units = (int)((chunks + g.cpu - 1) / g.cpu);
  return g;
}
// tiles per unit of the fused reduction: about eight workgroups per compute unit
static int radial_tpg(const tb_plan* p, int ntiles, int slots) {
  int64_t t = ((int64_t)ntiles * slots) / ((int64_t)p->ncu * 8);
  if (t < 1) t = 1;
  if (t > 16) t = 16;
  return (int)t;
}
static size_t radial_spec_bytes(const tb_plan* p, int bc) {
  return align256((size_t)bc * p->dev.H * p->dev.W * (p->dev.D / 2 + 1) * sizeof(cf));
}
static size_t radial_fused_bytes(const tb_plan* p, int bc, int K, int with_g) {
  const int T = maskgrad_tile(p);
  const int ntiles = (p->dev.W * (p->dev.D / 2 + 1) + T - 1) / T;
  return (with_g ? 2 : 1) * radial_spec_bytes(p, bc) + (size_t)ntiles * bc * K * sizeof(double);
}
static size_t radial_composed_bytes(const tb_plan* p, int bc, int K) {
  const int64_t N = (int64_t)p->dev.H * p->dev.W * p->dev.D;
  return align256(tb_mask_grad_workspace_bytes(p, bc)) + align256((size_t)bc * N * sizeof(float)) +
         (size_t)radial_bin_grid(N).units * bc * K * sizeof(double);
}

size_t tb_radial_workspace_bytes(const tb_plan* plan, int bc, int K, int with_g) {
  if (!plan || bc < 1 || K < 1 || K > TB_RADIAL_MAX_BINS) return 0;
  const size_t c = radial_composed_bytes(plan, bc, K);
  if (maskgrad_generic(plan)) return c;
  const size_t f = radial_fused_bytes(plan, bc, K, with_g);
  return f > c ? f : c;
}

static bool radial_args_ok(int K, double dr, int mode) {
  return K >= 1 && K <= TB_RADIAL_MAX_BINS && std::isfinite(dr) && dr > 0.0 &&
         (mode == TB_RADIAL_NEAREST || mode == TB_RADIAL_LINEAR);
}

// q[Cm][K] = scale * bin(A[Cm][H][W][D]); part: radial_bin_grid(N).units * Cm * K doubles
static int radial_bin(const tb_plan* p, const float* A, int Cm, int K, float inv_dr, int mode, float* q, double* part,
                      hipStream_t st) {
  const int H = p->dev.H, W = p->dev.W, D = p->dev.D;
  const RadialBinGrid bg = radial_bin_grid((int64_t)H * W * D);
  Timer t(2, st, (double)Cm * H * W * D * 4.0, "k_radial_bin");
  const tb::RadialDenseArgs da{H, W, D, Cm, K, mode, inv_dr, A, nullptr, part, tb::RB_CHUNK, bg.cpu};
  TB_HIP(tb::launch_radial_bin(da, bg.units, st));
  const tb::RadialSumArgs sa{part, q, bg.units, Cm * K, 1.0, 0};
  TB_HIP(tb::launch_radial_sum(sa, st));
  return TB_OK;
}

// g = nullptr: the power spectrum P[B*C][K]; else the profile gradient dp[Cp][K]
template <int RA, int RB>
static int kspace_radial(const tb_plan* p, const float* x, const int64_t* xs, const float* g, const int64_t* gs,
                         float* out, int Cp, int K, float inv_dr, int mode, void* ws, int B, int C, hipStream_t st) {
  const int H = p->dev.H, W = p->dev.W, D = p->dev.D, Dh = D / 2 + 1;
  const int64_t N = (int64_t)H * W * D;
  const bool self = g == nullptr;
  if (maskgrad_generic(p) || !g_radial_fused) {
    char* w = static_cast<char*>(ws);
    float* dM = reinterpret_cast<float*>(w + align256(tb_mask_grad_workspace_bytes(p, B * C)));
    double* part = reinterpret_cast<double*>(reinterpret_cast<char*>(dM) + align256((size_t)B * C * N * sizeof(float)));
    if (!self) {
      const int rc = kspace_mask_grad<RA, RB>(p, x, xs, g, gs, dM, Cp, ws, B, C, st, 0);
      if (rc) return rc;
      return radial_bin(p, dM, Cp, K, inv_dr, mode, out, part, st);
    }
    for (int b = 0; b < B; ++b) {  // one sample at a time: no sum over samples
      const float* xb = x + (int64_t)b * C * xs[0];
      int rc = kspace_mask_grad<RA, RB>(p, xb, xs, xb, xs, dM, C, ws, 1, C, st, 0);
      if (rc) return rc;
      rc = radial_bin(p, dM, C, K, inv_dr, mode, out + (size_t)b * C * K, part, st);
      if (rc) return rc;
    }
    return TB_OK;
  }
  const int T = maskgrad_tile(p);
  const int ntiles = (W * Dh + T - 1) / T;
  const size_t lds = (size_t)tb::radial_lds_cf(H, T, K) * sizeof(cf);
  cf* Sx = static_cast<cf*>(ws);
  cf* Sg = reinterpret_cast<cf*>(static_cast<char*>(ws) + radial_spec_bytes(p, B * C));
  double* part = reinterpret_cast<double*>(static_cast<char*>(ws) + (self ? 1 : 2) * radial_spec_bytes(p, B * C));
  const double scale = 1.0 / (double)N;
  for (int b0 = 0; b0 < B; b0 += TB_MAX_BATCH) {
    const int nb = (B - b0) < TB_MAX_BATCH ? (B - b0) : TB_MAX_BATCH;
    const double vox = (double)nb * C * N, spec = (double)nb * C * H * W * Dh * 8.0;
    const int slots = self ? nb * C : Cp;
    const int tpg = radial_tpg(p, ntiles, slots);
    const int units = (ntiles + tpg - 1) / tpg;
    {
      Timer t(0, st, (self ? 1.0 : 2.0) * (vox * 4.0 + spec), use_ct_slab(p) ? "k_slab_fwd_ct16" : "k_slab_fwd");
      int rc = launch_slab_fwd<RA>(p, x, xs, Sx, b0 * C, nb * C, st);
      if (rc) return rc;
      if (!self) {
        rc = launch_slab_fwd<RA>(p, g, gs, Sg, b0 * C, nb * C, st);
        if (rc) return rc;
      }
    }
    {
      Timer t(1, st, (self ? 1.0 : 2.0) * spec + (double)units * slots * K * 8.0, self ? "k_radial_power" : "k_radial_grad");
      const tb::RadialArgs ra{p->dev, Sx, Sg, part, b0 * C, C, nb, self ? 1 : Cp, T, tpg, K, mode, inv_dr};
      TB_HIP(launch_radial<RB>(ra, self, dim3(units, slots), lds, st));
    }
    {
      Timer t(2, st, (double)units * slots * K * 8.0, "k_radial_sum");
      const tb::RadialSumArgs sa{part, self ? out + (size_t)b0 * C * K : out, units, slots * K, scale,
                                 (!self && b0 > 0) ? 1 : 0};
      TB_HIP(tb::launch_radial_sum(sa, st));
    }
  }
  return TB_OK;
}

static int radial_entry(const tb_plan* p, const float* x, const int64_t* xs, const float* g, const int64_t* gs,
                        float* out, int Cp, int K, double dr, int mode, void* ws, size_t ws_bytes, int B, int C,
                        void* stream) {
  if (!ws || ws_bytes < tb_radial_workspace_bytes(p, B * C, K, g ? 1 : 0)) return TB_ERR_WORKSPACE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const float inv_dr = (float)(1.0 / dr);
#define TB_ARGS p, x, xs, g, gs, out, Cp, K, inv_dr, mode, ws, B, C, st
  if (p->rset_wd == RS_SMALL)
    return p->rset_h == RS_SMALL ? kspace_radial<RS_SMALL, RS_SMALL>(TB_ARGS) : kspace_radial<RS_SMALL, RS_ALL>(TB_ARGS);
  return p->rset_h == RS_SMALL ? kspace_radial<RS_ALL, RS_SMALL>(TB_ARGS) : kspace_radial<RS_ALL, RS_ALL>(TB_ARGS);
#undef TB_ARGS
}

int tb_kspace_radial_power_f32(const tb_plan* p, const float* x, const int64_t* xs, float* P, int K, double dr,
                               int mode, void* ws, size_t ws_bytes, int B, int C, void* stream) {
  if (!p || !x || !xs || !P || B < 1 || C < 1 || !radial_args_ok(K, dr, mode)) return TB_ERR_INVALID_ARG;
  return radial_entry(p, x, xs, nullptr, nullptr, P, 1, K, dr, mode, ws, ws_bytes, B, C, stream);
}

int tb_kspace_radial_grad_f32(const tb_plan* p, const float* x, const int64_t* xs, const float* g, const int64_t* gs,
                              float* dp, int Cp, int K, double dr, int mode, void* ws, size_t ws_bytes, int B, int C,
                              void* stream) {
  if (!p || !x || !xs || !g || !gs || !dp || B < 1 || C < 1 || (Cp != 1 && Cp != C) || !radial_args_ok(K, dr, mode))
    return TB_ERR_INVALID_ARG;
  return radial_entry(p, x, xs, g, gs, dp, Cp, K, dr, mode, ws, ws_bytes, B, C, stream);
}

int tb_radial_mask_f32(const tb_plan* p, const float* prof, int Cp, int K, double dr, int mode, float* M, void* stream) {
  if (!p || !prof || !M || Cp < 1 || !radial_args_ok(K, dr, mode)) return TB_ERR_INVALID_ARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const tb::RadialDenseArgs da{p->dev.H, p->dev.W, p->dev.D, Cp, K, mode, (float)(1.0 / dr), prof, M, nullptr, 0, 0};
  TB_HIP(tb::launch_radial_expand(da, st));
  return TB_OK;
}

int tb_radial_bin_f32(const tb_plan* p, const float* A, int Cm, int K, double dr, int mode, float* q, void* ws,
                      size_t ws_bytes, void* stream) {
  if (!p || !A || !q || Cm < 1 || !radial_args_ok(K, dr, mode)) return TB_ERR_INVALID_ARG;
  const int64_t N = (int64_t)p->dev.H * p->dev.W * p->dev.D;
  if (!ws || ws_bytes < (size_t)radial_bin_grid(N).units * Cm * K * sizeof(double)) return TB_ERR_WORKSPACE;
  return radial_bin(p, A, Cm, K, (float)(1.0 / dr), mode, q, static_cast<double*>(ws),
                    reinterpret_cast<hipStream_t>(stream));
}

int tb_set_radial_fused(int enable) {
  g_radial_fused = enable != 0;
  return TB_OK;
}

// ------------------------------------------------------------ centred spectrum export / import (spectrum.h)
// Tile of the export / import pass: pass B's width (one tile of LDS, whole 64-B segments per row, 16
// columns = one 128-B line of 8-byte coefficients per row at H = 240), narrowed until the tile holds
// at most SP_MAX_TILE coefficients.  Plans that maskgrad_generic() sends to the direct-DFT route go
// there here as well, so a single column always fits.
static int spectrum_tile(const tb_plan* p) {
  int T = pick_tile(p->dev.H, p->lds_max);
  while (T > 1 && p->dev.H * T > SP_MAX_TILE) --T;
  return T;
}

size_t tb_spectrum_workspace_bytes(const tb_plan* plan, int bc) {
  if (!plan || bc < 0) return 0;
  const int H = plan->dev.H, W = plan->dev.W, D = plan->dev.D;
  if (maskgrad_generic(plan)) return gen_workspace_bytes(H, W, D, bc);
  return (size_t)bc * H * W * (D / 2 + 1) * sizeof(cf);
}

template <int RA, int RB>
static int kspace_export(const tb_plan* p, const float* x, const int64_t* xs, cf* K, void* ws, int B, int C,
                         hipStream_t st) {
  const int H = p->dev.H, W = p->dev.W, D = p->dev.D, Dh = D / 2 + 1;
  const bool gen = maskgrad_generic(p);
  const int T = gen ? 1 : spectrum_tile(p);
  const int ntiles = (W * Dh + T - 1) / T;
  const size_t lds = (size_t)tile_geo(H, T).total_cf * sizeof(cf);
  cf* S = static_cast<cf*>(ws);
  for (int b0 = 0; b0 < B; b0 += TB_MAX_BATCH) {
    const int nb = (B - b0) < TB_MAX_BATCH ? (B - b0) : TB_MAX_BATCH;
    const double vox = (double)nb * C * H * W * D, spec = (double)nb * C * H * W * Dh * 8.0;
    if (gen) {
      const GenLaunch g{p->dev, x, xs, nullptr, nullptr, S, 0, b0 * C, C, nb * C, nullptr, nullptr};
      {
        Timer t(0, st, vox * 60.0, "k_gen_dft");  // 4 B read and 8 B written by the load, 16 B per axis
        TB_HIP(tb::launch_gen_spectrum(g, st));
      }
      {
        Timer t(1, st, spec + vox * 8.0, "k_gen_export");
        TB_HIP(tb::launch_gen_export(g, K, st));
      }
      continue;
    }
    {
      Timer t(0, st, vox * 4.0 + spec, use_ct_slab(p) ? "k_slab_fwd_ct16" : "k_slab_fwd");
      const int rc = launch_slab_fwd<RA>(p, x, xs, S, b0 * C, nb * C, st);
      if (rc) return rc;
    }
    {
      Timer t(1, st, spec + vox * 8.0, "k_kspace_export");
      const SpectrumArgs sa{p->dev, S, K, b0 * C, T};
      TB_HIP(launch_kspace_export<RB>(sa, dim3(ntiles, nb * C), lds, st));
    }
  }
  return TB_OK;
}

template <int RA, int RB>
static int kspace_import(const tb_plan* p, const cf* K, float* y, const int64_t* ys, int y_pad, void* ws, int B,
                         int C, hipStream_t st) {
  const int H = p->dev.H, W = p->dev.W, D = p->dev.D, Dh = D / 2 + 1;
  const float scale = (float)(1.0 / ((double)H * (double)W * (double)D));
  const bool gen = maskgrad_generic(p);
  const int T = gen ? 1 : spectrum_tile(p);
  const int ntiles = (W * Dh + T - 1) / T;
  const size_t lds_b = (size_t)tile_geo(H, T).total_cf * sizeof(cf);
  const size_t lds_s = (size_t)slab_geo(W, D).total_cf * sizeof(cf);
  cf* S = static_cast<cf*>(ws);
  for (int b0 = 0; b0 < B; b0 += TB_MAX_BATCH) {
    const int nb = (B - b0) < TB_MAX_BATCH ? (B - b0) : TB_MAX_BATCH;
    const double vox = (double)nb * C * H * W * D, spec = (double)nb * C * H * W * Dh * 8.0;
    if (gen) {
      // the gather, three axes and the store pass
      Timer t(1, st, vox * (8.0 + 16.0 + 3.0 * 16.0) + (double)nb * C * H * W * (D + y_pad) * 4.0, "k_gen_import");
      const GenLaunch g{p->dev, nullptr, nullptr, y, ys, S, y_pad, b0 * C, C, nb * C, nullptr, nullptr};
      TB_HIP(tb::launch_gen_import(g, K, st));
      continue;
    }
    {
      Timer t(1, st, vox * 8.0 + spec, "k_kspace_import");
      const SpectrumArgs sa{p->dev, S, const_cast<cf*>(K), b0 * C, T};
      TB_HIP(launch_kspace_import<RB>(sa, dim3(ntiles, nb * C), lds_b, st));
    }
    {
      Timer t(2, st, spec + (double)nb * C * H * W * (D + y_pad) * 4.0, use_ct_slab(p) ? "k_slab_inv_ct" : "k_slab_inv");
      const SlabInvArgs ia{p->dev, S, y, ys[0], ys[1], ys[2], y_pad, b0 * C, C, scale, nullptr, nb * C};
      if (use_ct_slab(p))
        TB_HIP(tb::launch_slab_inv_ct(ia, p->ncu, st));
      else
        TB_HIP(launch_slab_inv<RA>(ia, dim3(H, nb * C), lds_s, st));
    }
  }
  return TB_OK;
}

int tb_kspace_export_f32(const tb_plan* p, const float* x, const int64_t* xs, void* K, void* ws, size_t ws_bytes,
                         int B, int C, void* stream) {
  if (!p || !x || !xs || !K || B < 1 || C < 1) return TB_ERR_INVALID_ARG;
  if (!ws || ws_bytes < tb_spectrum_workspace_bytes(p, B * C)) return TB_ERR_WORKSPACE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define TB_ARGS p, x, xs, static_cast<cf*>(K), ws, B, C, st
  if (p->rset_wd == RS_SMALL)
    return p->rset_h == RS_SMALL ? kspace_export<RS_SMALL, RS_SMALL>(TB_ARGS) : kspace_export<RS_SMALL, RS_ALL>(TB_ARGS);
  return p->rset_h == RS_SMALL ? kspace_export<RS_ALL, RS_SMALL>(TB_ARGS) : kspace_export<RS_ALL, RS_ALL>(TB_ARGS);
#undef TB_ARGS
}

int tb_kspace_import_f32(const tb_plan* p, const void* K, float* y, const int64_t* ys, int y_pad, void* ws,
                         size_t ws_bytes, int B, int C, void* stream) {
  if (!p || !K || !y || !ys || B < 1 || C < 1 || y_pad < 0) return TB_ERR_INVALID_ARG;
  if (!ws || ws_bytes < tb_spectrum_workspace_bytes(p, B * C)) return TB_ERR_WORKSPACE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define TB_ARGS p, static_cast<const cf*>(K), y, ys, y_pad, ws, B, C, st
  if (p->rset_wd == RS_SMALL)
    return p->rset_h == RS_SMALL ? kspace_import<RS_SMALL, RS_SMALL>(TB_ARGS) : kspace_import<RS_SMALL, RS_ALL>(TB_ARGS);
  return p->rset_h == RS_SMALL ? kspace_import<RS_ALL, RS_SMALL>(TB_ARGS) : kspace_import<RS_ALL, RS_ALL>(TB_ARGS);
#undef TB_ARGS
}

// ------------------------------------------------------------ amplitude mixing (ampmix.h)
// Tiles: the forward's x and partner tiles share one pass-B tile of LDS (half of pass B's width, as the
// mask gradient); the backward puts the upstream gradient's tile next to them at the same width -- a
// three-wide tile of at most 48 KB (three workgroups per CU by LDS) -- narrowed where that passes
// AM_MAX_TILE_BWD coefficients.
static int ampmix_tile(const tb_plan* p, bool bwd) {
  int T = pick_tile(p->dev.H, p->lds_max) / 2;
  if (T < 1) T = 1;
  const int cap = bwd ? AM_MAX_TILE_BWD / 3 : AM_MAX_TILE / 2;
  while (T > 1 && p->dev.H * T > cap) --T;
  while (T > 1 && (size_t)tile_geo(p->dev.H, (bwd ? 3 : 2) * T).total_cf * sizeof(cf) > (size_t)p->lds_max) --T;
  return T;
}
// the element-wise fallback also takes a plan whose single three-wide column exceeds the LDS
static bool ampmix_generic(const tb_plan* p) {
  return maskgrad_generic(p) || (size_t)tile_geo(p->dev.H, 3).total_cf * sizeof(cf) > (size_t)p->lds_max;
}

// Fused route, half spectra of bc volumes each: [S_x][S_y or X'][S_g -> Gx][Gy][sum of Gy over equal partners].
// Fallback, full spectra: [X][Y][X' or G -> Gx][scratch][Gy][sum of Gy].
size_t tb_ampmix_workspace_bytes(const tb_plan* plan, int bc, int with_g, int with_gy) {
  if (!plan || bc < 0) return 0;
  const int H = plan->dev.H, W = plan->dev.W, D = plan->dev.D;
  const size_t g = with_g || with_gy ? 1 : 0, gy = with_gy ? 2 : 0;
  if (ampmix_generic(plan)) return (4 + gy) * (size_t)bc * H * W * D * sizeof(cf);
  return (2 + g + gy) * (size_t)bc * H * W * (D / 2 + 1) * sizeof(cf);
}

namespace {
struct AmpMixCall {
  const float *x, *y;
  const int64_t *xs, *ys;
  const int* perm;
  const float* M;
  int Cm;
  const float* lam;
  const float* g;     // backward: upstream gradient
  const int64_t* gs;
  float* o1;          // forward: out; backward: gx
  const int64_t* o1s;
  int o1_pad;
  float* gy;          // backward: may be null
  const int64_t* gys;
};
}  // namespace

template <int RA>
static int ampmix_inverse(const tb_plan* p, const cf* S, float* y, const int64_t* ys, int y_pad, int b0, int nb, int C,
                          hipStream_t st) {
  const int H = p->dev.H, W = p->dev.W, D = p->dev.D;
  const float scale = (float)(1.0 / ((double)H * (double)W * (double)D));
  const size_t lds_s = (size_t)slab_geo(W, D).total_cf * sizeof(cf);
  Timer t(2, st, (double)nb * C * H * W * ((D / 2 + 1) * 8.0 + (D + y_pad) * 4.0), use_ct_slab(p) ? "k_slab_inv_ct" : "k_slab_inv");
  const SlabInvArgs ia{p->dev, S, y, ys[0], ys[1], ys[2], y_pad, b0 * C, C, scale, nullptr, nb * C};
  if (use_ct_slab(p))
    TB_HIP(tb::launch_slab_inv_ct(ia, p->ncu, st));
  else
    TB_HIP(launch_slab_inv<RA>(ia, dim3(H, nb * C), lds_s, st));
  return TB_OK;
}

template <int RA>
static int ampmix_forward_all(const tb_plan* p, const float* x, const int64_t* xs, cf* S, int B, int C, hipStream_t st) {
  const int H = p->dev.H, W = p->dev.W, D = p->dev.D, Dh = D / 2 + 1;
  for (int b0 = 0; b0 < B; b0 += TB_MAX_BATCH) {
    const int nb = (B - b0) < TB_MAX_BATCH ? (B - b0) : TB_MAX_BATCH;
    Timer t(0, st, (double)nb * C * H * W * (D * 4.0 + Dh * 8.0), use_ct_slab(p) ? "k_slab_fwd_ct16" : "k_slab_fwd");
    const int rc = launch_slab_fwd<RA>(p, x, xs, S, b0 * C, nb * C, st);
    if (rc) return rc;
  }
  return TB_OK;
}

// the fallback: full spectra, element-wise closed form, direct-DFT axes
static int ampmix_gen(const tb_plan* p, const AmpMixCall& c, void* ws, int B, int C, bool bwd, hipStream_t st) {
  const int H = p->dev.H, W = p->dev.W, D = p->dev.D;
  const size_t nv = (size_t)B * C * H * W * D;
  cf* X = static_cast<cf*>(ws);
  cf* Y = c.y ? X + nv : X;
  cf* O = X + 2 * nv;
  cf* tmp = X + 3 * nv;
  cf* Gy = X + 4 * nv;
  cf* Gys = X + 5 * nv;
  const double vol = (double)H * W * D;
  const int nsrc = 1 + (c.y ? 1 : 0) + (bwd ? 1 : 0);
  for (int s = 0; s < nsrc; ++s) {
    const bool isg = bwd && s == nsrc - 1;
    const float* src = isg ? c.g : (s == 0 ? c.x : c.y);
    const int64_t* ss = isg ? c.gs : (s == 0 ? c.xs : c.ys);
    cf* dst = isg ? O : (s == 0 ? X : Y);
    for (int b0 = 0; b0 < B; b0 += TB_MAX_BATCH) {
      const int nb = (B - b0) < TB_MAX_BATCH ? (B - b0) : TB_MAX_BATCH;
      Timer t(0, st, nb * C * vol * 60.0, "k_gen_dft");
      const GenLaunch gl{p->dev, src, ss, nullptr, nullptr, tmp, 0, b0 * C, C, nb * C, nullptr, nullptr};
      TB_HIP(tb::launch_gen_spectrum_to(gl, dst, st));
    }
  }
  const bool need_gy = bwd && c.gy;
  for (int b0 = 0; b0 < B; b0 += TB_MAX_BATCH) {
    const int nb = (B - b0) < TB_MAX_BATCH ? (B - b0) : TB_MAX_BATCH;
    const AmpMixArgs a{p->dev, X, Y, O, Gy, c.M, c.lam, c.perm, C, B, c.Cm, 1, b0 * C, need_gy ? 1 : 0};
    {
      Timer t(1, st, nb * C * vol * (bwd ? (need_gy ? 40.0 : 32.0) : 24.0) + c.Cm * vol * 4.0,
              bwd ? "k_gen_ampmix_bwd" : "k_gen_ampmix");
      if (bwd)
        TB_HIP(tb::launch_gen_ampmix_bwd(a, nb * C, st));
      else
        TB_HIP(tb::launch_gen_ampmix(a, nb * C, st));
    }
    {
      Timer t(2, st, nb * C * vol * (3.0 * 16.0 + 8.0) + (double)nb * C * H * W * (D + c.o1_pad) * 4.0, "k_gen_dft");
      const GenLaunch gl{p->dev, nullptr, nullptr, c.o1, c.o1s, tmp, c.o1_pad, b0 * C, C, nb * C, nullptr, nullptr};
      TB_HIP(tb::launch_gen_inverse(gl, O, st));
    }
  }
  if (!need_gy) return TB_OK;
  for (int b0 = 0; b0 < B; b0 += TB_MAX_BATCH) {
    const int nb = (B - b0) < TB_MAX_BATCH ? (B - b0) : TB_MAX_BATCH;
    if (c.perm) {
      Timer t(3, st, 2.0 * nb * C * vol * 8.0, "k_ampmix_gysum");
      TB_HIP(tb::launch_ampmix_gysum(Gy, Gys, c.perm, B, C, b0, nb, (int64_t)H * W * D, st));
    }
    Timer t(2, st, nb * C * vol * (3.0 * 16.0 + 8.0 + 4.0), "k_gen_dft");
    const GenLaunch gl{p->dev, nullptr, nullptr, c.gy, c.gys, tmp, 0, b0 * C, C, nb * C, nullptr, nullptr};
    TB_HIP(tb::launch_gen_inverse(gl, c.perm ? Gys : Gy, st));
  }
  return TB_OK;
}

template <int RA, int RB>
static int kspace_ampmix(const tb_plan* p, const AmpMixCall& c, void* ws, int B, int C, bool bwd, hipStream_t st) {
  if (ampmix_generic(p)) return ampmix_gen(p, c, ws, B, C, bwd, st);
  const int H = p->dev.H, W = p->dev.W, D = p->dev.D, Dh = D / 2 + 1;
  const size_t nv = (size_t)B * C * H * W * Dh;
  const int T = ampmix_tile(p, bwd);
  const int ntiles = (W * Dh + T - 1) / T;
  const size_t lds = (size_t)tile_geo(H, (bwd ? 3 : 2) * T).total_cf * sizeof(cf);
  cf* Sx = static_cast<cf*>(ws);
  cf* S2 = Sx + nv;
  cf* Sg = Sx + 2 * nv;
  cf* Sgy = Sx + 3 * nv;
  cf* Sgys = Sx + 4 * nv;
  // partners cross launch groups: every forward pass runs before the first per-coefficient launch
  int rc = ampmix_forward_all<RA>(p, c.x, c.xs, Sx, B, C, st);
  if (rc) return rc;
  if (c.y) {
    rc = ampmix_forward_all<RA>(p, c.y, c.ys, S2, B, C, st);
    if (rc) return rc;
  }
  if (bwd) {
    rc = ampmix_forward_all<RA>(p, c.g, c.gs, Sg, B, C, st);
    if (rc) return rc;
  }
  const cf* Sy = c.y ? S2 : Sx;
  // forward: X' over S_x when the partners have their own buffer, else into the second one
  cf* So = bwd ? Sg : (c.y ? Sx : S2);
  const bool need_gy = bwd && c.gy;
  for (int b0 = 0; b0 < B; b0 += TB_MAX_BATCH) {
    const int nb = (B - b0) < TB_MAX_BATCH ? (B - b0) : TB_MAX_BATCH;
    const double spec = (double)nb * C * H * W * Dh * 8.0;
    {
      Timer t(1, st, (bwd ? (need_gy ? 5.0 : 4.0) : 3.0) * spec + (double)c.Cm * H * W * D * 4.0,
              bwd ? "k_kspace_ampmix_bwd" : "k_kspace_ampmix");
      const AmpMixArgs a{p->dev, Sx, Sy, So, Sgy, c.M, c.lam, c.perm, C, B, c.Cm, T, b0 * C, need_gy ? 1 : 0};
      if (bwd)
        TB_HIP(launch_kspace_ampmix_bwd<RB>(a, dim3(ntiles, nb * C), lds, st));
      else
        TB_HIP(launch_kspace_ampmix<RB>(a, dim3(ntiles, nb * C), lds, st));
    }
    rc = ampmix_inverse<RA>(p, So, c.o1, c.o1s, c.o1_pad, b0, nb, C, st);
    if (rc) return rc;
  }
  if (!need_gy) return TB_OK;
  // Gy of sample b belongs to row perm[b] of y: summed over equal partners in the order of b, on the
  // half spectra (the inverse is linear), then one pass C
  for (int b0 = 0; b0 < B; b0 += TB_MAX_BATCH) {
    const int nb = (B - b0) < TB_MAX_BATCH ? (B - b0) : TB_MAX_BATCH;
    if (c.perm) {
      Timer t(3, st, 2.0 * (double)nb * C * H * W * Dh * 8.0, "k_ampmix_gysum");
      TB_HIP(tb::launch_ampmix_gysum(Sgy, Sgys, c.perm, B, C, b0, nb, (int64_t)H * W * Dh, st));
    }
    rc = ampmix_inverse<RA>(p, c.perm ? Sgys : Sgy, c.gy, c.gys, 0, b0, nb, C, st);
    if (rc) return rc;
  }
  return TB_OK;
}

static int ampmix_entry(const tb_plan* p, const AmpMixCall& c, void* ws, int B, int C, bool bwd, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define TB_ARGS p, c, ws, B, C, bwd, st
  if (p->rset_wd == RS_SMALL)
    return p->rset_h == RS_SMALL ? kspace_ampmix<RS_SMALL, RS_SMALL>(TB_ARGS) : kspace_ampmix<RS_SMALL, RS_ALL>(TB_ARGS);
  return p->rset_h == RS_SMALL ? kspace_ampmix<RS_ALL, RS_SMALL>(TB_ARGS) : kspace_ampmix<RS_ALL, RS_ALL>(TB_ARGS);
#undef TB_ARGS
}

int tb_kspace_ampmix_f32(const tb_plan* p, const float* x, const int64_t* xs, const float* y, const int64_t* ys_in,
                         const int* perm, const float* M, int Cm, const float* lam, float* out, const int64_t* outs,
                         int out_pad, void* ws, size_t ws_bytes, int B, int C, void* stream) {
  if (!p || !x || !xs || (y && !ys_in) || !M || !lam || !out || !outs || out_pad < 0 || B < 1 || C < 1 ||
      (Cm != 1 && Cm != C))
    return TB_ERR_INVALID_ARG;
  if (!ws || ws_bytes < tb_ampmix_workspace_bytes(p, B * C, 0, 0)) return TB_ERR_WORKSPACE;
  const AmpMixCall c{x, y, xs, ys_in, perm, M, Cm, lam, nullptr, nullptr, out, outs, out_pad, nullptr, nullptr};
  return ampmix_entry(p, c, ws, B, C, false, stream);
}

int tb_kspace_ampmix_bwd_f32(const tb_plan* p, const float* x, const int64_t* xs, const float* y, const int64_t* ys_in,
                             const int* perm, const float* M, int Cm, const float* lam, const float* g,
                             const int64_t* gs, float* gx, const int64_t* gxs, float* gy, const int64_t* gys, void* ws,
                             size_t ws_bytes, int B, int C, void* stream) {
  if (!p || !x || !xs || (y && !ys_in) || !M || !lam || !g || !gs || !gx || !gxs || (gy && !gys) || B < 1 || C < 1 ||
      (Cm != 1 && Cm != C))
    return TB_ERR_INVALID_ARG;
  if (!ws || ws_bytes < tb_ampmix_workspace_bytes(p, B * C, 1, gy ? 1 : 0)) return TB_ERR_WORKSPACE;
  const AmpMixCall c{x, y, xs, ys_in, perm, M, Cm, lam, g, gs, gx, gxs, 0, gy, gys};
  return ampmix_entry(p, c, ws, B, C, true, stream);
}

int tb_kspace_filter_f32(const tb_plan* p, const float* x, const int64_t* xs, float* y, const int64_t* ys, int y_pad,
                         void* ws, size_t ws_bytes, int B, int C, const tb_sample_ops* ops, uint32_t* minmax,
                         void* stream) {
  if (!p) return TB_ERR_INVALID_ARG;
#define TB_ARGS p, x, xs, y, ys, y_pad, ws, ws_bytes, B, C, ops, minmax, stream
  if (p->rset_wd == RS_SMALL)
    return p->rset_h == RS_SMALL ? kspace_filter<RS_SMALL, RS_SMALL>(TB_ARGS) : kspace_filter<RS_SMALL, RS_ALL>(TB_ARGS);
  return p->rset_h == RS_SMALL ? kspace_filter<RS_ALL, RS_SMALL>(TB_ARGS) : kspace_filter<RS_ALL, RS_ALL>(TB_ARGS);
#undef TB_ARGS
}

int tb_planes_closed_form_f32(const tb_plan* p, const float* x, const int64_t* xs, float* y, const int64_t* ys,
                              int y_pad, void* ws, size_t ws_bytes, int B, int C, const tb_sample_ops* ops,
                              uint32_t* minmax, void* stream) {
  if (!p || !x || !y || !xs || !ys || !ops || B < 1 || C < 1 || y_pad < 0 || !ws) return TB_ERR_INVALID_ARG;
  if (ws_bytes < tb::point_ws(B * C).total) return TB_ERR_WORKSPACE;
  for (int b = 0; b < B; ++b)
    if (ops[b].n < 1 || ops[b].n > TB_MAX_OPS || !tb::point_program(ops[b], p->dev.H, p->dev.W, p->dev.D))
      return TB_ERR_INVALID_ARG;  // not spike-only, or two spikes touch: tb_kspace_filter_f32 takes those
  if (!tb::point_strides_ok(p->dev.H, p->dev.W, p->dev.D, y_pad, xs, ys)) return TB_ERR_UNSUPPORTED_SIZE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  for (int b0 = 0; b0 < B; b0 += TB_MAX_BATCH) {
    const int nb = (B - b0) < TB_MAX_BATCH ? (B - b0) : TB_MAX_BATCH;
    const int rc = run_point(p, x, xs, y, ys, y_pad, static_cast<char*>(ws), b0, nb, C, ops, minmax, st);
    if (rc) return rc;
  }
  return TB_OK;
}

// ------------------------------------------------------------ trainable spike layer (spike_grad.h)
// spike_layer.forward (stylization_layers.py:143-151) = KSpaceSpikeNoise._set_spike
// (filters_and_operators.py:906-983) at one location for every channel, with the log-intensity read from
// device memory and the analytic gradients in place of the reference's finite differences.
// Workspace: the closed-form route's carve for the launch group, then its float64 dI shares.
static size_t spikes_share_bytes(int nbc) { return ((size_t)nbc * TB_MAX_OPS * sizeof(double) + 255) & ~(size_t)255; }

size_t tb_spikes_workspace_bytes(const tb_plan* plan, int bc) {
  if (!plan || bc < 1) return 0;
  return tb::point_ws(bc).total + spikes_share_bytes(bc);
}

// the layer's host program (S spikes on every channel); argument errors before geometry limits
static int spikes_program(const tb_plan* p, int S, const int32_t* loc, tb_sample_ops& so) {
  if (S < 1 || S > TB_MAX_OPS || !loc) return TB_ERR_INVALID_ARG;
  const int n[3] = {p->dev.H, p->dev.W, p->dev.D};
  std::memset(&so, 0, sizeof(so));
  so.n = S;
  for (int j = 0; j < S; ++j) {
    tb_op& op = so.op[j];
    op.kind = TB_OP_SPIKE;
    op.chan = -1;
    op.f[1] = NAN;  // own phase
    for (int ax = 0; ax < 3; ++ax) {
      if (loc[3 * j + ax] < 0 || loc[3 * j + ax] >= n[ax]) return TB_ERR_INVALID_ARG;
      op.i[ax] = loc[3 * j + ax];
    }
    for (int q = 0; q < j; ++q) {
      bool same = true, conj = true;
      for (int ax = 0; ax < 3; ++ax) {
        same &= op.i[ax] == so.op[q].i[ax];
        conj &= op.i[ax] == (n[ax] - so.op[q].i[ax]) % n[ax];
      }
      if (same || conj) return TB_ERR_INVALID_ARG;
    }
  }
  return tb::point_program(so, n[0], n[1], n[2]) ? TB_OK : TB_ERR_UNSUPPORTED_SIZE;
}

// launch arguments of one launch group: x -> y through the spikes `so` (y null: no apply is launched)
static tb::PointArgs spikes_group(const tb_plan* p, const float* x, const int64_t* xs, float* y, const int64_t* ys,
                                  int y_pad, char* ws, int b0, int nb, int C, const tb_sample_ops& so,
                                  const float* logI, double* coef, uint32_t* minmax) {
  tb::PointArgs a;
  std::memset(&a, 0, sizeof(a));
  const int nbc = nb * C;
  a.H = p->dev.H, a.W = p->dev.W, a.D = p->dev.D;
  a.x = x, a.xsbc = xs[0], a.xsh = xs[1], a.xsw = xs[2];
  a.y = y, a.ysbc = ys[0], a.ysh = ys[1], a.ysw = ys[2];
  a.ypad = y_pad, a.bc0 = b0 * C, a.C = C, a.nbc = nbc, a.mm = minmax;
  const tb::PointWs wl = tb::point_ws(nbc);
  a.part = reinterpret_cast<double*>(ws + wl.part);
  a.delta = reinterpret_cast<float*>(ws + wl.delta);
  a.mmp = reinterpret_cast<float2*>(ws + wl.mmp);
  a.cnt = reinterpret_cast<uint32_t*>(ws + wl.cnt);
  a.share = reinterpret_cast<double*>(ws + wl.total);
  a.namax = so.n;
  for (int i = 0; i < nb; ++i) a.ops.s[i] = so;
  a.logI = logI, a.coef = coef, a.nspk = so.n;
  tb::point_grid(a, p->ncu);
  return a;
}

int tb_kspace_spikes_f32(const tb_plan* p, const float* x, const int64_t* xs, float* y, const int64_t* ys, int y_pad,
                         void* ws, size_t ws_bytes, int B, int C, int S, const int32_t* loc, const float* logI,
                         double* coef, uint32_t* minmax, void* stream) {
  if (!p || !x || !xs || !y || !ys || B < 1 || C < 1 || y_pad < 0 || !logI) return TB_ERR_INVALID_ARG;
  tb_sample_ops so;
  const int rc = spikes_program(p, S, loc, so);
  if (rc) return rc;
  const int H = p->dev.H, W = p->dev.W, D = p->dev.D;
  if (!tb::point_strides_ok(H, W, D, y_pad, xs, ys)) return TB_ERR_UNSUPPORTED_SIZE;
  if (!ws || ws_bytes < tb_spikes_workspace_bytes(p, B * C)) return TB_ERR_WORKSPACE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  for (int b0 = 0; b0 < B; b0 += TB_MAX_BATCH) {
    const int nb = (B - b0) < TB_MAX_BATCH ? (B - b0) : TB_MAX_BATCH;
    const tb::PointArgs a = spikes_group(p, x, xs, y, ys, y_pad, static_cast<char*>(ws), b0, nb, C, so, logI, coef, minmax);
    const double vox = (double)a.nbc * H * W * D;
    {
      Timer t(0, st, vox * 4.0, "k_point_dft");
      TB_HIP(tb::launch_point(a, st, 0));
    }
    {
      Timer t(1, st, (double)a.nbc * a.parts * TB_MAX_OPS * 16.0, "k_spike_delta");
      TB_HIP(tb::launch_point(a, st, 3));
    }
    {
      Timer t(2, st, vox * 4.0 + (double)a.nbc * H * W * (D + y_pad) * 4.0, "k_point_apply");
      TB_HIP(tb::launch_point(a, st, 2));
    }
  }
  return TB_OK;
}

int tb_kspace_spikes_bwd_f32(const tb_plan* p, const float* g, const int64_t* gs, int B, int C, int S,
                             const int32_t* loc, const float* logI, const double* coef, float* gx, const int64_t* gxs,
                             float* dI, void* ws, size_t ws_bytes, void* stream) {
  if (!p || !g || !gs || B < 1 || C < 1 || !logI || !coef || (gx && !gxs)) return TB_ERR_INVALID_ARG;
  tb_sample_ops so;
  const int rc = spikes_program(p, S, loc, so);
  if (rc) return rc;
  const int H = p->dev.H, W = p->dev.W, D = p->dev.D;
  const int64_t* os = gx ? gxs : gs;
  if (!tb::point_strides_ok(H, W, D, 0, gs, os)) return TB_ERR_UNSUPPORTED_SIZE;
  if (!ws || ws_bytes < tb_spikes_workspace_bytes(p, B * C)) return TB_ERR_WORKSPACE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  for (int b0 = 0; b0 < B; b0 += TB_MAX_BATCH) {
    const int nb = (B - b0) < TB_MAX_BATCH ? (B - b0) : TB_MAX_BATCH;
    const tb::PointArgs a = spikes_group(p, g, gs, gx, os, 0, static_cast<char*>(ws), b0, nb, C, so, logI,
                                         const_cast<double*>(coef), nullptr);
    const double vox = (double)a.nbc * H * W * D;
    {
      Timer t(0, st, vox * 4.0, "k_point_dft");
      TB_HIP(tb::launch_point(a, st, 0));
    }
    {
      Timer t(1, st, (double)a.nbc * a.parts * TB_MAX_OPS * 16.0, "k_spike_gamma");
      TB_HIP(tb::launch_point(a, st, 4));
    }
    if (dI) {
      Timer t(3, st, (double)a.nbc * S * 8.0, "k_spike_dI_sum");  // its own slot: slot 2 is the apply's
      const tb::SpikeSumArgs sa{a.share, dI, a.nbc, S, b0 > 0 ? 1 : 0};
      TB_HIP(tb::launch_spike_dI_sum(sa, st));
    }
    if (gx) {
      Timer t(2, st, vox * 8.0, "k_point_apply");
      TB_HIP(tb::launch_point(a, st, 2));
    }
  }
  return TB_OK;
}

int tb_kspace_logabs_sum_f32(const tb_plan* p, const float* x, const int64_t* xs, void* ws, size_t ws_bytes, int B,
                             int C, const tb_sample_ops* ops, double* out, void* stream) {
  if (!p) return TB_ERR_INVALID_ARG;
#define TB_ARGS p, x, xs, ws, ws_bytes, B, C, ops, out, stream
  if (p->rset_wd == RS_SMALL)
    return p->rset_h == RS_SMALL ? kspace_stats<RS_SMALL, RS_SMALL>(TB_ARGS) : kspace_stats<RS_SMALL, RS_ALL>(TB_ARGS);
  return p->rset_h == RS_SMALL ? kspace_stats<RS_ALL, RS_SMALL>(TB_ARGS) : kspace_stats<RS_ALL, RS_ALL>(TB_ARGS);
#undef TB_ARGS
}

int tb_minmax_f32(const float* x, uint32_t* mm, int B, int64_t rows, int len, int64_t ld, int64_t sb, void* stream) {
  if (!x || !mm || B < 1 || rows < 1 || len < 1 || ld < len) return TB_ERR_INVALID_ARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  Timer t(3, st, (double)B * rows * len * 4.0, "k_minmax");
  hipLaunchKernelGGL(k_minmax_init, dim3((B + 255) / 256), dim3(256), 0, st, mm, B);
  const int64_t n = rows * len;
  int64_t blocks = (n + 256 * 8 - 1) / (256 * 8);
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(k_minmax<256>, dim3((unsigned)blocks, B), dim3(256), 0, st, x, mm, rows, len, ld, sb);
  TB_HIP(hipGetLastError());
  return TB_OK;
}

int tb_salt_pepper_f32(const float* x, float* y, int8_t* cls, const float* u_in, uint64_t seed, uint64_t offset,
                       const float* thr, const uint32_t* mm, int B, int64_t rows, int len, int64_t ld, int64_t sb,
                       void* stream) {
  if (!x || !y || !thr || !mm || B < 1 || rows < 1 || len < 1 || ld < len) return TB_ERR_INVALID_ARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t n = rows * len;
  if (u_in) {  // parity mode: the caller's uniform field, one class per voxel
    int64_t blocks = ((n + 3) / 4 + NT_SAP - 1) / NT_SAP;
    if (blocks > 2048) blocks = 2048;
    Timer t(3, st, (double)B * n * (12.0 + (cls ? 1.0 : 0.0)), "k_salt_pepper");
    for (int b0 = 0; b0 < B; b0 += TB_MAX_BATCH) {
      const int nb = (B - b0) < TB_MAX_BATCH ? (B - b0) : TB_MAX_BATCH;
      SapThr th;
      for (int i = 0; i < TB_MAX_BATCH; ++i) {
        th.lo[i] = i < nb ? thr[2 * (b0 + i)] : 0.f;
        th.hi[i] = i < nb ? thr[2 * (b0 + i) + 1] : 0.f;
      }
      hipLaunchKernelGGL(k_salt_pepper<NT_SAP>, dim3((unsigned)blocks, nb), dim3(NT_SAP), 0, st, x, y, cls, u_in, seed,
                         offset, th, mm, b0, rows, len, ld, sb, 0);
      TB_HIP(hipGetLastError());
    }
    return TB_OK;
  }
  // device stream: out of place = copy, then the sparse scatter of the changed voxels (the class
  // map, when asked for, is zeroed first); in place only the changed voxels are written
  for (int b = 0; b < B; ++b) {
    if (x != y)
      TB_HIP(hipMemcpy2DAsync(y + b * sb, ld * 4, x + b * sb, ld * 4, (size_t)len * 4, rows, hipMemcpyDeviceToDevice, st));
    if (cls) TB_HIP(hipMemset2DAsync(cls + b * sb, ld, 0, (size_t)len, rows, st));
  }
  // algorithmic bytes: one 4-B store per changed voxel (~p n), no reads
  double changed = 0.0;
  for (int b = 0; b < B; ++b) changed += (double)n * (thr[2 * b + 1] > 0.f ? (thr[2 * b + 1] < 1.f ? thr[2 * b + 1] : 1.f) : 0.f);
  Timer t(3, st, changed * (4.0 + (cls ? 1.0 : 0.0)), "k_sap_geom");
  const int64_t segs = (n + SAP_SEG - 1) / SAP_SEG;
  for (int b0 = 0; b0 < B; b0 += TB_MAX_BATCH) {
    const int nb = (B - b0) < TB_MAX_BATCH ? (B - b0) : TB_MAX_BATCH;
    SapGeomArgs ga;
    ga.y = y;
    ga.cls = cls;
    ga.seed = seed;
    ga.offset = offset;
    for (int i = 0; i < TB_MAX_BATCH; ++i) {
      ga.lo[i] = i < nb ? thr[2 * (b0 + i)] : 0.f;
      ga.hi[i] = i < nb ? thr[2 * (b0 + i) + 1] : 0.f;
    }
    ga.mm = mm;
    ga.b0 = b0;
    ga.rows = rows;
    ga.len = len;
    ga.ld = ld;
    ga.sb = sb;
    hipLaunchKernelGGL(k_sap_geom, dim3((unsigned)((segs + 255) / 256), nb), dim3(256), 0, st, ga);
    TB_HIP(hipGetLastError());
  }
  return TB_OK;
}

float tb_key_to_float(uint32_t key) { return key2f(key); }

int tb_disk_mask_f32(float* mask, int64_t outer, int n0, int n1, int n2, int int_r, int64_t r2i, float r2f,
                     int inside_off, void* stream) {
  if (!mask || outer < 1 || n0 < 1 || n1 < 1 || n2 < 1) return TB_ERR_INVALID_ARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t total = outer * n0 * n1 * n2;
  int64_t blocks = (total + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(k_disk_mask, dim3((unsigned)blocks), dim3(256), 0, st, mask, outer, n0, n1, n2, int_r, r2i, r2f,
                     inside_off);
  TB_HIP(hipGetLastError());
  return TB_OK;
}

int tb_set_chain_chunk(int n) {
  g_chunk = n;
  return TB_OK;
}

int tb_set_compiled_plans(int enable) {
  g_compiled_plans = enable != 0;
  return TB_OK;
}

int tb_set_band_plans(int enable) {
  g_band = enable != 0;
  return TB_OK;
}

int tb_set_wrap_plans(int enable) {
  g_wrap = enable != 0;
  return TB_OK;
}

int tb_set_half_units(int enable) {
  g_half = enable != 0;
  return TB_OK;
}

int tb_set_point_plans(int enable) {
  g_point = enable != 0;
  return TB_OK;
}

int tb_set_band_inv16(int enable) {
  g_inv16 = enable != 0;
  return TB_OK;
}

int tb_set_pass_timing(int enable) {
  std::lock_guard<std::mutex> lk(g_tmu);
  g_timing = enable != 0;
  for (auto& r : g_recs) { g_pool.push_back(r.a); g_pool.push_back(r.b); }
  g_recs.clear();
  return TB_OK;
}

int tb_get_pass_stats(float* ms, int* cnt, double* bytes) {
  if (!ms || !cnt) return TB_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(g_tmu);
  for (int i = 0; i < 4; ++i) {
    ms[i] = 0.f;
    cnt[i] = 0;
    if (bytes) bytes[i] = 0.0;
  }
  for (auto& r : g_recs) {
    TB_HIP(hipEventSynchronize(r.b));
    float t = 0.f;
    TB_HIP(hipEventElapsedTime(&t, r.a, r.b));
    ms[r.slot] += t;
    cnt[r.slot] += 1;
    if (bytes) bytes[r.slot] += r.bytes;
    g_pool.push_back(r.a);
    g_pool.push_back(r.b);
  }
  g_recs.clear();
  return TB_OK;
}

int tb_get_pass_times_ms(float* ms, int* cnt) { return tb_get_pass_stats(ms, cnt, nullptr); }

const char* tb_pass_kernel(int slot) {
  if (slot < 0 || slot > 3) return "";
  std::lock_guard<std::mutex> lk(g_tmu);
  return g_slot_kernel[slot];
}
