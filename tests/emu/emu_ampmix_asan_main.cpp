// Host sanitizer run of the amplitude-mixing passes (test infrastructure): emu_ampmix.cpp -- the ampmix.h code
// the gfx950 kernels run -- built as ONE executable with -fsanitize=address,undefined, so no sanitizer runtime
// has to be preloaded into Python.  Runs the forward and the backward entry points over three launch groups
// (17 samples) at 17 x 2 x 6 x 5 x 7 with a ragged tile, a per-channel mask and a non-permutation partner
// index that crosses the groups and holds values outside [0, B), with the partners given and taken from x;
// checks that lam = 0 returns the input, that every output is written and the pad columns are 0; exits
// non-zero on a violation (the sanitizers abort on their own findings).
#include "emu_ampmix.cpp"

#include <cmath>
#include <cstdio>
#include <random>

int main() {
  const int B = 17, C = 2, H = 6, W = 5, D = 7, T = 3, pad = 2;
  const int64_t N = (int64_t)H * W * D;
  std::vector<float> x((size_t)B * C * N), y(x.size()), g(x.size()), M((size_t)C * N), lam(B), zero(B, 0.f);
  std::vector<int> perm(B);
  std::mt19937 gen(33);
  std::normal_distribution<float> nd;
  std::uniform_real_distribution<float> ud(0.f, 1.f);
  for (auto& v : x) v = nd(gen);
  for (auto& v : y) v = nd(gen);
  for (auto& v : g) v = nd(gen);
  for (auto& v : M) v = ud(gen);
  for (auto& v : lam) v = ud(gen);
  for (int b = 0; b < B; ++b) perm[b] = (b * 7 + 3) % B;
  perm[0] = perm[1] = 16;  // a repeated partner in the last group
  perm[9] = -5;            // clamped to 0
  perm[16] = 1000;         // clamped to B - 1
  const int64_t st[3] = {N, (int64_t)W * D, D};
  const int64_t ost[3] = {(int64_t)H * W * (D + pad), (int64_t)W * (D + pad), D + pad};
  int fails = 0;
  for (int from_x = 0; from_x < 2; ++from_x) {
    const float* yp = from_x ? nullptr : y.data();
    std::vector<float> out((size_t)B * C * H * W * (D + pad), std::nanf(""));
    if (tbemu_kspace_ampmix_f32(H, W, D, x.data(), st, yp, st, perm.data(), M.data(), C, lam.data(), out.data(), ost, pad,
                                B, C, T))
      ++fails;
    for (size_t i = 0; i < out.size(); ++i) {
      const bool in_pad = (int)(i % (D + pad)) >= D;
      if (!std::isfinite(out[i]) || (in_pad && out[i] != 0.f)) { std::fprintf(stderr, "out %zu\n", i); ++fails; break; }
    }
    std::vector<float> id(x.size(), std::nanf(""));
    if (tbemu_kspace_ampmix_f32(H, W, D, x.data(), st, yp, st, perm.data(), M.data(), 1, zero.data(), id.data(), st, 0, B,
                                C, T))
      ++fails;
    for (size_t i = 0; i < id.size(); ++i)
      if (!(std::fabs(id[i] - x[i]) <= 1e-5f)) { std::fprintf(stderr, "lam = 0: %zu %g %g\n", i, id[i], x[i]); ++fails; break; }
    for (int with_gy = 0; with_gy < 2; ++with_gy) {
      std::vector<float> gx(x.size(), std::nanf("")), gy(x.size(), std::nanf(""));
      if (tbemu_kspace_ampmix_bwd_f32(H, W, D, x.data(), st, yp, st, perm.data(), M.data(), C, lam.data(), g.data(), st,
                                      gx.data(), st, with_gy ? gy.data() : nullptr, st, B, C, T))
        ++fails;
      for (float v : gx) if (!std::isfinite(v)) { std::fprintf(stderr, "gx not written\n"); ++fails; break; }
      if (with_gy)
        for (float v : gy) if (!std::isfinite(v)) { std::fprintf(stderr, "gy not written\n"); ++fails; break; }
    }
  }
  if (fails) return 1;
  std::printf("emu ampmix sanitizer run ok\n");
  return 0;
}
